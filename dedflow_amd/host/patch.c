/* Patch schedule for the residual assembly (assembly schedule 4, default).
 *
 * The colored RHS scatter fetches 4 node records and read-modify-writes 4 residual records per
 * tet, and inside a color no two tets share a node, so none of it is reused on chip (~1 KB/tet of
 * HBM traffic for 404 B/tet of algorithmic bytes).  Here spatial patches of <= 64 tets / <= 64
 * nodes (recursive coordinate bisection) stage their node records in LDS once, sum the residual of
 * every patch node in a FIXED order (per-patch adjacency lists) and write one partial record per
 * patch node; a second kernel adds, again in fixed order, the partials of every node into F.  No
 * colors, no atomics, two launches, bitwise reproducible.  Host-side, OpenMP tasks; deterministic
 * (patches are identified by their position in the RCB order).
 */
#include <string.h>
#include <omp.h>
#include "dedflow.h"
#include "dedflow_kernels.h"
#include "host_private.h"
#include "rcb.h"

#define RP_TETS 64  /* tets per patch: one lane each of the residual kernel's wave */
#define RP_NODES 64 /* distinct nodes per patch: one lane each */

typedef struct { index_type lo, hi; } Range;
typedef struct {
    const f64* c;          /* centroids */
    index_type* idx;       /* element permutation (RCB order) */
    const index_type* ien; /* host connectivity */
    index_type leaf, cap;  /* tets per patch, and the cap on its distinct nodes */
    Range* out;            /* emitted patches */
    index_type nout, capout;
} Ctx;

static int cmp_i32(const void* a, const void* b) {
    index_type x = *(const index_type*)a, y = *(const index_type*)b;
    return (x > y) - (x < y);
}

/* distinct nodes of elements idx[lo..hi); sorted unique ids returned in `keys` (room for 4 per element) */
static index_type patch_nodes(const Ctx* x, index_type lo, index_type hi, index_type* keys) {
    index_type n = 0;
    for (index_type e = lo; e < hi; ++e) {
        const index_type* nd = x->ien + (size_t)x->idx[e] * 4;
        for (int a = 0; a < 4; ++a) keys[n++] = nd[a];
    }
    qsort(keys, (size_t)n, sizeof(index_type), cmp_i32);
    index_type m = 0;
    for (index_type i = 0; i < n; ++i)
        if (i == 0 || keys[i] != keys[i - 1]) keys[m++] = keys[i];
    return m;
}


static void emit(Ctx* x, index_type lo, index_type hi) {
#pragma omp critical(dfl_patch_emit)
    {
        if (x->nout == x->capout) {
            x->capout *= 2;
            x->out = (Range*)realloc(x->out, sizeof(Range) * (size_t)x->capout);
        }
        x->out[x->nout].lo = lo;
        x->out[x->nout].hi = hi;
        x->nout++;
    }
}

static void split(Ctx* x, index_type lo, index_type hi) {
    const index_type n = hi - lo;
    if (n <= x->leaf) {
        index_type* keys = (index_type*)malloc(sizeof(index_type) * (size_t)n * 16);
        index_type nb = patch_nodes(x, lo, hi, keys);
        free(keys);
        if (nb <= x->cap || n <= 1) { emit(x, lo, hi); return; }
    }
    f64 bl[3] = {1e300, 1e300, 1e300}, bh[3] = {-1e300, -1e300, -1e300};
    for (index_type i = lo; i < hi; ++i)
        for (int d = 0; d < 3; ++d) {
            f64 v = x->c[(size_t)x->idx[i] * 3 + d];
            if (v < bl[d]) bl[d] = v;
            if (v > bh[d]) bh[d] = v;
        }
    int ax = 0;
    if (bh[1] - bl[1] > bh[ax] - bl[ax]) ax = 1;
    if (bh[2] - bl[2] > bh[ax] - bl[ax]) ax = 2;
    /* cut at a multiple of the leaf size so that leaves come out full (plain halving leaves them 60 % full on average) */
    index_type half = n / 2;
    if (n > x->leaf) {
        const index_type nleaf = (n + x->leaf - 1) / x->leaf;
        half = (nleaf / 2) * x->leaf;
    }
    select_kth(x->c, ax, x->idx + lo, n, half);
    if (n > 4096) {
#pragma omp task
        split(x, lo, lo + half);
#pragma omp task
        split(x, lo + half, hi);
#pragma omp taskwait
    } else {
        split(x, lo, lo + half);
        split(x, lo + half, hi);
    }
}

static int cmp_range(const void* a, const void* b) {
    index_type x = ((const Range*)a)->lo, y = ((const Range*)b)->lo;
    return (x > y) - (x < y);
}

/* Fixed-stride layout: patch p owns tet slots [p*64, (p+1)*64) and node slots [p*64, (p+1)*64) (unused node slots hold -1),
 * so every index array of a patch is addressed from the patch id alone and the loads of a patch form a two-hop chain
 * (lists -> node records); d_cnt[p] = num_tets | num_nodes << 16.  The adjacency of every patch node is cut into sub-lists
 * of exactly 4 entries (padding = slot 256, which holds 0.0): a two-level ordered sum in which all lanes of the first level
 * do the same work whatever the valence of their node. */
RhsPatchSched* DflBuildRhsPatchSchedule(Mesh3D* mesh) {
    const index_type T = mesh->num_tet, N = mesh->num_node;
    const index_type* ien = mesh->host->ien;
    const f64* xg = mesh->host->xg;
    RhsPatchSched* ps = (RhsPatchSched*)CdamMallocHost(SIZE_OF(RhsPatchSched));
    memset(ps, 0, sizeof *ps);
    f64* c = (f64*)malloc(sizeof(f64) * (size_t)T * 3);
    index_type* idx = (index_type*)malloc(sizeof(index_type) * (size_t)T);
#pragma omp parallel for schedule(static) num_threads(8)
    for (index_type e = 0; e < T; ++e) {
        for (int d = 0; d < 3; ++d) {
            f64 s = 0.0;
            for (int a = 0; a < 4; ++a) s += xg[(size_t)ien[(size_t)e * 4 + a] * 3 + d];
            c[(size_t)e * 3 + d] = 0.25 * s;
        }
        idx[e] = e;
    }
    /* a GPU box exposes every hardware thread of the host but grants one rank a ~16-core share:
       an uncapped OpenMP team (256 spinning threads) made the task tree 30x slower */
    int nt = omp_get_max_threads();
    if (getenv("DFL_HOST_THREADS")) nt = atoi(getenv("DFL_HOST_THREADS"));
    if (nt > 16) nt = 16;
    if (nt < 1) nt = 1;
    const int verbose = getenv("DFL_PATCH_VERBOSE") != NULL;
    double t0 = omp_get_wtime();
    Ctx x = {c, idx, ien, RP_TETS, RP_NODES, NULL, 0, 1024};
    x.out = (Range*)malloc(sizeof(Range) * (size_t)x.capout);
#pragma omp parallel num_threads(nt)
#pragma omp single
    split(&x, 0, T);
    qsort(x.out, (size_t)x.nout, sizeof(Range), cmp_range);
    const index_type P = x.nout;

    /* per patch: node list, local connectivity, adjacency (node -> (tet,a) in ascending tet order) */
    index_type* nn_of = (index_type*)malloc(sizeof(index_type) * (size_t)P);
    index_type** nodes_of = (index_type**)malloc(sizeof(index_type*) * (size_t)P);
#pragma omp parallel for schedule(dynamic, 64) num_threads(nt)
    for (index_type p = 0; p < P; ++p) {
        const index_type lo = x.out[p].lo, hi = x.out[p].hi;
        index_type* keys = (index_type*)malloc(sizeof(index_type) * (size_t)(hi - lo) * 4);
        nn_of[p] = patch_nodes(&x, lo, hi, keys);
        nodes_of[p] = keys;
    }
    const int64_t totn = (int64_t)P * RP_NODES;
    ASSERT(totn < 2147483647LL && (int64_t)P * RP_TETS * 4 < 2147483647LL);
    const size_t tslots = (size_t)P * RP_TETS;
    index_type* pnode = (index_type*)malloc(sizeof(index_type) * (size_t)(totn > 0 ? totn : 1));
    memset(pnode, 0xff, sizeof(index_type) * (size_t)(totn > 0 ? totn : 1)); /* -1 = unused slot */
    u8* lien = (u8*)calloc(tslots * 4 + 4, 1);
    index_type* cnt_of = (index_type*)malloc(sizeof(index_type) * (size_t)(P > 0 ? P : 1));
    uint16_t* sub4 = (uint16_t*)malloc(sizeof(uint16_t) * 512 * (size_t)(P > 0 ? P : 1));
    for (size_t i = 0; i < 512 * (size_t)P; ++i) sub4[i] = 256;
    uint16_t* sub_start = (uint16_t*)calloc((size_t)(RP_NODES + 1) * (size_t)(P > 0 ? P : 1), sizeof(uint16_t));
#pragma omp parallel for schedule(dynamic, 64) num_threads(nt)
    for (index_type p = 0; p < P; ++p) {
        const index_type lo = x.out[p].lo, ne = x.out[p].hi - lo, nn = nn_of[p];
        const index_type* keys = nodes_of[p];
        const size_t e0 = (size_t)p * RP_TETS;
        cnt_of[p] = ne | (nn << 16);
        memcpy(pnode + (size_t)p * RP_NODES, keys, sizeof(index_type) * (size_t)nn);
        uint16_t cnt[256]; /* local node ids are bytes */
        memset(cnt, 0, sizeof cnt);
        for (index_type k = 0; k < ne; ++k) {
            const index_type* nd = ien + (size_t)idx[lo + k] * 4;
            for (int a = 0; a < 4; ++a) {
                index_type l = 0, h = nn - 1;
                while (l < h) {
                    index_type mid = (l + h) >> 1;
                    if (keys[mid] < nd[a]) l = mid + 1; else h = mid;
                }
                lien[(e0 + k) * 4 + a] = (u8)l;
                cnt[l]++;
            }
        }
        uint16_t st[RP_NODES + 1]; /* adjacency group starts */
        uint16_t adj[RP_TETS * 4]; /* (local tet)*4 + a grouped by patch node, ascending tet */
        st[0] = 0;
        for (index_type k = 0; k < nn; ++k) st[k + 1] = (uint16_t)(st[k] + cnt[k]);
        uint16_t cur[256];
        memcpy(cur, st, sizeof(uint16_t) * (size_t)nn);
        for (index_type k = 0; k < ne; ++k)
            for (int a = 0; a < 4; ++a) adj[cur[lien[(e0 + k) * 4 + a]]++] = (uint16_t)(k * 4 + a);
        uint16_t* s4 = sub4 + (size_t)p * 512;
        uint16_t* ss = sub_start + (size_t)p * (RP_NODES + 1);
        index_type sidx = 0;
        for (index_type k = 0; k < nn; ++k) {
            ss[k] = (uint16_t)sidx;
            for (index_type q = st[k]; q < st[k + 1]; q += 4, ++sidx) {
                ASSERT(sidx < 128);
                for (index_type i = 0; i < 4 && q + i < st[k + 1]; ++i) s4[sidx * 4 + i] = adj[q + i];
            }
        }
        for (index_type k = nn; k <= RP_NODES; ++k) ss[k] = (uint16_t)sidx;
    }
    /* node -> its partial records (ascending patch order) */
    index_type* goff = (index_type*)calloc((size_t)N + 1, sizeof(index_type));
    for (int64_t i = 0; i < totn; ++i) if (pnode[i] >= 0) goff[pnode[i] + 1]++;
    for (index_type n = 0; n < N; ++n) goff[n + 1] += goff[n];
    index_type* gidx = (index_type*)malloc(sizeof(index_type) * (size_t)(totn > 0 ? totn : 1));
    {
        index_type* cur = (index_type*)malloc(sizeof(index_type) * (size_t)N);
        memcpy(cur, goff, sizeof(index_type) * (size_t)N);
        for (int64_t i = 0; i < totn; ++i) if (pnode[i] >= 0) gidx[cur[pnode[i]]++] = (index_type)i;
        free(cur);
    }
    ps->num_patch = P;
    ps->total_nodes = (index_type)totn;
    ps->d_pnode = (index_type*)CdamMallocDevice((ptrdiff_t)(totn > 0 ? totn : 1) * SIZE_OF(index_type));
    ps->d_cnt = (index_type*)CdamMallocDevice((ptrdiff_t)(P > 0 ? P : 1) * SIZE_OF(index_type));
    HIPGUARD(hipMemcpy(ps->d_cnt, cnt_of, sizeof(index_type) * (size_t)P, H2D));
    ps->d_lien = (u8*)CdamMallocDevice((ptrdiff_t)tslots * 4 + 4);
    ps->d_goff = (index_type*)CdamMallocDevice(((ptrdiff_t)N + 1) * SIZE_OF(index_type));
    ps->d_gidx = (index_type*)CdamMallocDevice((ptrdiff_t)(totn > 0 ? totn : 1) * SIZE_OF(index_type));
    ps->d_partial = (f64*)CdamMallocDevice((ptrdiff_t)(totn > 0 ? totn : 1) * 6 * SIZE_OF(f64));
    ps->d_sub4 = (uint16_t*)CdamMallocDevice((ptrdiff_t)512 * (P > 0 ? P : 1) * (ptrdiff_t)sizeof(uint16_t));
    ps->d_sub_start = (uint16_t*)CdamMallocDevice((ptrdiff_t)(RP_NODES + 1) * (P > 0 ? P : 1) * (ptrdiff_t)sizeof(uint16_t));
    HIPGUARD(hipMemcpy(ps->d_sub4, sub4, sizeof(uint16_t) * 512 * (size_t)P, H2D));
    HIPGUARD(hipMemcpy(ps->d_sub_start, sub_start, sizeof(uint16_t) * (size_t)(RP_NODES + 1) * (size_t)P, H2D));
    HIPGUARD(hipMemcpy(ps->d_pnode, pnode, sizeof(index_type) * (size_t)totn, H2D));
    HIPGUARD(hipMemcpy(ps->d_lien, lien, tslots * 4, H2D));
    HIPGUARD(hipMemcpy(ps->d_goff, goff, sizeof(index_type) * ((size_t)N + 1), H2D));
    HIPGUARD(hipMemcpy(ps->d_gidx, gidx, sizeof(index_type) * (size_t)totn, H2D));
    if (verbose) fprintf(stderr, "[rhspatch] %d patches, %lld patch nodes (%.2f per node) in %.2f s\n", P, (long long)totn,
                         (double)totn / (double)(N > 0 ? N : 1), omp_get_wtime() - t0);
    for (index_type p = 0; p < P; ++p) free(nodes_of[p]);
    free(cnt_of); free(sub4); free(sub_start);
    free(gidx); free(goff); free(lien); free(pnode);
    free(nodes_of); free(nn_of); free(x.out); free(idx); free(c);
    return ps;
}

void DflFreeRhsPatchSchedule(RhsPatchSched* ps) {
    if (!ps) return;
    CdamFreeDevice(ps->d_pnode, 0); CdamFreeDevice(ps->d_lien, 0);
    CdamFreeDevice(ps->d_goff, 0); CdamFreeDevice(ps->d_gidx, 0); CdamFreeDevice(ps->d_cnt, 0);
    CdamFreeDevice(ps->d_partial, 0); CdamFreeDevice(ps->d_sub4, 0); CdamFreeDevice(ps->d_sub_start, 0);
    CdamFreeHost(ps, SIZE_OF(RhsPatchSched));
}
