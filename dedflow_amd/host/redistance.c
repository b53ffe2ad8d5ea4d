/* Level-set redistancing: the exact narrow-band distance to the surface phi = level (build-defined, opt-in; model in
 * include/dedflow.h, "level-set redistancing", kernels in dedflow_amd/csrc/k_redistance.hip).  The reference never restores
 * |grad phi| = 1.
 *
 * Per mesh, built by DflMeshSetRedistance: the configuration, the cell grid over the mesh's bounding box (made there and again
 * by the first call after DflMeshGeometryChanged; both copy the coordinates to the host once), the hold mask of the boundary
 * groups, the scan and reduction scratch, the compacted node list, and the facet and entry lists of the last call.  A call
 * reads the facet and entry totals back once (it returns the first) and grows the two lists when a total exceeds the
 * capacity; it allocates nothing otherwise.  Without a configuration nothing of this exists and no call path touches it. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "dedflow.h"
#include "dedflow_kernels.h"
#include "host_private.h"

#define RD_MAX_CELLS (1 << 24)

typedef struct RedistanceState {
    DflRedistance cfg;
    index_type N, T;
    f64 cell_factor;                 /* DFL_REDISTANCE_CELL as the Set call read it */
    dfl_redistance_grid grid;
    index_type ncell;
    b32 grid_stale;                  /* the nodes moved since the grid was made */
    u8* hold;                        /* device [N], NULL: no group is held */
    DflBlockScan scan;               /* the facet counts of the tet passes; its chunk_sum also serves the cells */
    index_type *cell_count, *cell_start; /* device [cap_cell], [cap_cell + 1] */
    index_type cap_cell;
    f64* facets;                     /* device [cap_facets][9] */
    index_type* entries;             /* device [cap_entries] */
    index_type cap_facets, cap_entries;
    index_type *ncand, *list;        /* device [1], [N] */
    f64 *chg, *part, *out;           /* device [N], [2 max(nblk, dfl_node_reduce_max_part())], [6] */
    index_type nf_last;              /* facets of the last call, -1: none yet */
    index_type steps;                /* DflTimeStep calls since the Set call */
} RedistanceState;

static RedistanceState* st_of(const Mesh3D* mesh) {
    const MeshExt* x = (const MeshExt*)mesh->ext;
    return x ? x->redistance : NULL;
}

static void free_cells(RedistanceState* st) {
    CdamFreeDevice(st->cell_count, 0);
    CdamFreeDevice(st->cell_start, 0);
    st->cell_count = st->cell_start = NULL;
}

void DflRedistanceFree(RedistanceState* st) {
    if (!st) return;
    HIPGUARD(hipStreamSynchronize(DflStream()));
    free_cells(st);
    CdamFreeDevice(st->hold, 0);
    DflBlockScanFree(&st->scan);
    CdamFreeDevice(st->facets, 0);
    CdamFreeDevice(st->entries, 0);
    CdamFreeDevice(st->ncand, 0);
    CdamFreeDevice(st->list, 0);
    CdamFreeDevice(st->chg, 0);
    CdamFreeDevice(st->part, 0);
    CdamFreeDevice(st->out, 0);
    CdamFreeHost(st, SIZE_OF(RedistanceState));
}

void DflRedistanceGeometryChanged(RedistanceState* st) {
    if (st) st->grid_stale = TRUE;
}

int DflRedistanceCheck(const DflRedistance* c, char* why, size_t why_len) {
    if (!isfinite(c->level)) {
        snprintf(why, why_len, "level is not finite (%g)", c->level);
        return 1;
    }
    if (!isfinite(c->band)) {
        snprintf(why, why_len, "band is not finite (%g)", c->band);
        return 2;
    }
    if (!(c->band > 0.0)) {
        snprintf(why, why_len, "band must be positive, got %g", c->band);
        return 3;
    }
    if (c->every < 0) {
        snprintf(why, why_len, "every must not be negative, got %d", (int)c->every);
        return 4;
    }
    return 0;
}

/* the bounding box of the nodes and the cell grid over it: edge band * cell_factor, enlarged until the grid has at most 2^24
 * cells; the cell arrays grow to match.  Synchronises */
static void build_grid(RedistanceState* st, Mesh3D* mesh) {
    hipStream_t s = DflStream();
    f64 lo[3] = {0.0, 0.0, 0.0}, hi[3] = {0.0, 0.0, 0.0};
    HIPGUARD(hipStreamSynchronize(s));
    if (st->N > 0) DflMeshNodeBounds(mesh, lo, hi);
    f64 h = st->cfg.band * st->cell_factor;
    int64_t n[3];
    for (;;) {
        int64_t total = 1;
        for (int d = 0; d < 3; ++d) {
            const f64 c = floor((hi[d] - lo[d]) / h) + 1.0;
            n[d] = c < 1.0 ? 1 : (c > (f64)RD_MAX_CELLS ? RD_MAX_CELLS + 1 : (int64_t)c);
            total = total > RD_MAX_CELLS ? total : total * n[d];
        }
        if (total <= RD_MAX_CELLS) break;
        h *= 1.25;
    }
    for (int d = 0; d < 3; ++d) {
        st->grid.lo[d] = lo[d];
        st->grid.n[d] = (index_type)n[d];
    }
    st->grid.inv_h = 1.0 / h;
    st->ncell = (index_type)(n[0] * n[1] * n[2]);
    if (st->ncell > st->cap_cell) {
        free_cells(st);
        st->cap_cell = st->ncell;
        st->cell_count = (index_type*)CdamMallocDevice((ptrdiff_t)st->cap_cell * SIZE_OF(index_type));
        st->cell_start = (index_type*)CdamMallocDevice(((ptrdiff_t)st->cap_cell + 1) * SIZE_OF(index_type));
    }
    DflBlockScanReserve(&st->scan, st->ncell);
    st->grid_stale = FALSE;
}

/* hold[a] = 1 for the nodes of the boundary groups in `groups`; NULL when there is none */
static u8* build_hold(Mesh3D* mesh, index_type groups, index_type N) {
    index_type nb = mesh->num_bound < 31 ? mesh->num_bound : 31, any = 0;
    for (index_type g = 0; g < nb; ++g)
        if ((groups >> g) & 1) any += mesh->bound_node_offset[g + 1] - mesh->bound_node_offset[g];
    if (!any || N <= 0) return NULL;
    const index_type nbn = mesh->bound_node_offset[mesh->num_bound];
    index_type* node = (index_type*)CdamMallocHost((ptrdiff_t)nbn * SIZE_OF(index_type));
    u8* h = (u8*)CdamMallocHost((ptrdiff_t)N);
    HIPGUARD(hipMemcpy(node, mesh->bound_node, (size_t)nbn * sizeof(index_type), D2H));
    memset(h, 0, (size_t)N);
    for (index_type g = 0; g < nb; ++g)
        if ((groups >> g) & 1)
            for (index_type k = mesh->bound_node_offset[g]; k < mesh->bound_node_offset[g + 1]; ++k)
                if (node[k] >= 0 && node[k] < N) h[node[k]] = 1;
    u8* d = (u8*)CdamMallocDevice((ptrdiff_t)N);
    HIPGUARD(hipMemcpy(d, h, (size_t)N, H2D));
    CdamFreeHost(h, (ptrdiff_t)N);
    CdamFreeHost(node, (ptrdiff_t)nbn * SIZE_OF(index_type));
    return d;
}

void DflMeshSetRedistance(Mesh3D* mesh, const DflRedistance* cfg) {
    MeshExt* x = (MeshExt*)mesh->ext;
    if (!cfg) {
        DflRedistanceFree(x->redistance);
        x->redistance = NULL;
        return;
    }
    char why[160];
    if (DflRedistanceCheck(cfg, why, sizeof why)) {
        fprintf(stderr, "DflMeshSetRedistance: %s; unchanged\n", why);
        return;
    }
    f64 factor = 1.0;
    const char* env = getenv("DFL_REDISTANCE_CELL");
    if (env && env[0]) {
        char* end = NULL;
        factor = strtod(env, &end);
        if (end == env || !isfinite(factor) || !(factor >= 1.0)) {
            fprintf(stderr, "DflMeshSetRedistance: DFL_REDISTANCE_CELL must be a number >= 1 (a smaller cell breaks the 27-cell "
                            "search), got \"%s\"; unchanged\n", env);
            return;
        }
    }
    RedistanceState* st = x->redistance;
    const index_type N = Mesh3DNumNode(mesh), T = Mesh3DNumTet(mesh);
    HIPGUARD(hipStreamSynchronize(DflStream()));
    if (!st) {
        st = (RedistanceState*)CdamMallocHost(SIZE_OF(RedistanceState));
        memset(st, 0, sizeof *st);
        st->N = N;
        st->T = T;
        DflBlockScanAlloc(&st->scan, T, 0);
        const ptrdiff_t nb = st->scan.nblk > 0 ? st->scan.nblk : 1, nn = N > 0 ? N : 1, most = dfl_node_reduce_max_part();
        st->ncand = (index_type*)CdamMallocDevice(SIZE_OF(index_type));
        st->list = (index_type*)CdamMallocDevice(nn * SIZE_OF(index_type));
        st->chg = (f64*)CdamMallocDevice(nn * SIZE_OF(f64));
        st->part = (f64*)CdamMallocDevice(2 * (nb > most ? nb : most) * SIZE_OF(f64));
        st->out = (f64*)CdamMallocDevice(6 * SIZE_OF(f64));
        st->cap_facets = st->cap_entries = 1024;
        st->facets = (f64*)CdamMallocDevice((ptrdiff_t)st->cap_facets * 9 * SIZE_OF(f64));
        st->entries = (index_type*)CdamMallocDevice((ptrdiff_t)st->cap_entries * SIZE_OF(index_type));
        x->redistance = st;
    }
    st->cfg = *cfg;
    st->cell_factor = factor;
    st->nf_last = -1;
    st->steps = 0;
    CdamFreeDevice(st->hold, 0);
    st->hold = build_hold(mesh, cfg->hold_groups, N);
    build_grid(st, mesh);
    HIPGUARD(hipMemset(st->out, 0, 6 * sizeof(f64)));
    HIPGUARD(hipStreamSynchronize(DflStream()));
}

b32 DflMeshRedistanceEnabled(const Mesh3D* mesh) { return st_of(mesh) != NULL; }

b32 DflRedistanceInTimeStep(const Mesh3D* mesh) {
    const RedistanceState* st = st_of(mesh);
    return st && st->cfg.every > 0;
}

index_type DflMeshRedistance(Mesh3D* mesh, f64* w) {
    RedistanceState* st = st_of(mesh);
    if (!st) {
        fprintf(stderr, "DflMeshRedistance: no redistancing is set on this mesh (DflMeshSetRedistance)\n");
        return -1;
    }
    st->nf_last = 0;
    if (st->N <= 0 || st->T <= 0) return 0;
    const Mesh3DData* dev = Mesh3DDevice(mesh);
    hipStream_t s = DflStream();
    const f64 level = st->cfg.level, band = st->cfg.band;
    DflRangePush("DflMeshRedistance");
    if (st->grid_stale) build_grid(st, mesh);
    HIPGUARD(hipMemsetAsync(st->cell_count, 0, (size_t)st->ncell * sizeof(index_type), s));
    HIPGUARD(hipMemsetAsync(st->ncand, 0, sizeof(index_type), s));
    /* count: facets per workgroup, entries per cell, and the statistics of the field as it came */
    dfl_redistance_cut(st->T, dev->ien, dev->xg, w, st->N, level, &st->grid, st->scan.count, st->cell_count, st->part, s);
    dfl_redistance_reduce(st->scan.nblk, st->part, st->out, s);
    /* both scans (they take turns with chunk_sum), then the one synchronisation: both totals */
    index_type nf = 0, ne = 0;
    dfl_scan_counts(st->ncell, st->cell_count, st->scan.chunk_sum, st->cell_start, s);
    DflBlockScanEnqueue(&st->scan, &nf, s);
    HIPGUARD(hipMemcpyAsync(&ne, st->cell_start + st->ncell, sizeof ne, D2H, s));
    HIPGUARD(hipStreamSynchronize(s));
    if (nf < 0 || ne < 0) {
        fprintf(stderr, "DflMeshRedistance: more than 2^31 facets or cell entries (band %g against a much larger surface); "
                        "phi unchanged\n", band);
        DflRangePop();
        return -1;
    }
    if (nf > st->cap_facets) {
        CdamFreeDevice(st->facets, 0);
        st->cap_facets = DflGrowCap(nf);
        st->facets = (f64*)CdamMallocDevice((ptrdiff_t)st->cap_facets * 9 * SIZE_OF(f64));
    }
    if (ne > st->cap_entries) {
        CdamFreeDevice(st->entries, 0);
        st->cap_entries = DflGrowCap(ne);
        st->entries = (index_type*)CdamMallocDevice((ptrdiff_t)st->cap_entries * SIZE_OF(index_type));
    }
    if (nf > 0)
        dfl_redistance_emit(st->T, dev->ien, dev->xg, w, st->N, level, &st->grid, st->scan.base, st->cell_start, st->cell_count,
                            st->facets, st->cap_facets, st->entries, st->cap_entries, s);
    dfl_redistance_nodes(st->N, dev->xg, w, level, band, &st->grid, st->cell_start, st->entries, st->facets, st->cap_facets, st->hold,
                         st->ncand, st->list, st->chg, s);
    /* the statistics of the new field */
    dfl_redistance_cut(st->T, dev->ien, dev->xg, w, st->N, level, NULL, NULL, NULL, st->part, s);
    dfl_redistance_reduce(st->scan.nblk, st->part, st->out + 2, s);
    dfl_redistance_node_stats(st->N, st->chg, st->part, st->out + 4, s);
    st->nf_last = nf;
    DflRangePop();
    return nf;
}

index_type DflMeshRedistanceFacets(const Mesh3D* mesh, const f64** facets) {
    const RedistanceState* st = st_of(mesh);
    if (facets) *facets = st && st->nf_last > 0 ? st->facets : NULL;
    return st ? st->nf_last : -1;
}

void DflMeshRedistanceStats(Mesh3D* mesh, DflRedistanceStats* out) {
    RedistanceState* st = st_of(mesh);
    f64 h[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    memset(out, 0, sizeof *out);
    if (!st) {
        fprintf(stderr, "DflMeshRedistanceStats: no redistancing is set on this mesh (DflMeshSetRedistance)\n");
        return;
    }
    if (st->nf_last < 0) return; /* no call yet */
    hipStream_t s = DflStream();
    HIPGUARD(hipMemcpyAsync(h, st->out, sizeof h, D2H, s));
    HIPGUARD(hipStreamSynchronize(s));
    out->facets = st->nf_last;
    out->volume_before = h[0];
    out->grad_dev_before = h[1];
    out->volume_after = h[2];
    out->grad_dev_after = h[3];
    out->band_nodes = (int64_t)h[4];
    out->max_change = h[5];
}

f64 DflMeshLevelSetVolume(Mesh3D* mesh, const f64* w, f64 level) {
    const index_type N = Mesh3DNumNode(mesh), T = Mesh3DNumTet(mesh);
    if (N <= 0 || T <= 0) return 0.0;
    const Mesh3DData* dev = Mesh3DDevice(mesh);
    hipStream_t s = DflStream();
    const index_type per = dfl_tets_per_block(), nblk = (T + per - 1) / per;
    /* scratch of its own: the call works on a mesh without a configuration and leaves the last call's statistics alone */
    f64* part = (f64*)CdamMallocDevice(((ptrdiff_t)2 * nblk + 2) * SIZE_OF(f64));
    f64 h[2] = {0.0, 0.0};
    dfl_redistance_cut(T, dev->ien, dev->xg, w, N, level, NULL, NULL, NULL, part, s);
    dfl_redistance_reduce(nblk, part, part + 2 * (size_t)nblk, s);
    HIPGUARD(hipMemcpyAsync(h, part + 2 * (size_t)nblk, sizeof h, D2H, s));
    HIPGUARD(hipStreamSynchronize(s));
    CdamFreeDevice(part, 0);
    return h[0];
}

/* DflTimeStep: TRUE when this is an every-th step since the Set call, after redistancing wgold */
b32 DflRedistanceTimeStep(Mesh3D* mesh, f64* wgold) {
    RedistanceState* st = st_of(mesh);
    if (!st || st->cfg.every <= 0) return FALSE;
    if (++st->steps % st->cfg.every != 0) return FALSE;
    DflMeshRedistance(mesh, wgold);
    return TRUE;
}
