/* Porosity record: the connected components of the gas region, which of them are closed, and per closed one its volume, box
 * and wall temperatures (build-defined, opt-in; model in include/dedflow.h, "porosity record", kernels in
 * dedflow_amd/csrc/k_porosity.hip).  The reference has nothing of the kind.
 *
 * Per mesh, built by DflMeshSetPorosity: the configuration, the five [N] integer arrays of the labelling, the node and tet
 * workgroup counts with their scans, the volume partials, the rows, the list of the open groups' faces, one device record of
 * the totals with its pinned host copy, and small key lists.  An evaluation enqueues the labelling, the ranking and the tet
 * pass, copies the totals and waits once; the key lists grow when the closed tets exceed their capacity and nothing is
 * allocated otherwise; then emit, sort, evaluate and sum.  The state w is never written.  Without a configuration nothing of
 * this exists and no call path touches it. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "dedflow.h"
#include "dedflow_kernels.h"
#include "host_private.h"

typedef struct PorosityState {
    DflPorosity cfg;
    dfl_porosity_params prm;          /* cfg as the kernels take it */
    index_type N, T, nblk_node, nblk_tet;
    index_type *parent, *label, *open, *rank, *pore; /* device [N] */
    index_type *ncount, *nbase;       /* device [nblk_node], [nblk_node + 1] */
    index_type *tcount, *tbase;       /* device [nblk_tet], [nblk_tet + 1] */
    index_type* chunk_sum;            /* device: the scans' scratch */
    f64* part;                        /* device [nblk_tet][3] */
    dfl_pore_row* rows;               /* device [max_alloc] */
    index_type max_alloc;             /* rows the buffer holds */
    index_type nof, nof_alloc;        /* faces of the open groups; faces oface holds */
    index_type* oface;                /* device [nof_alloc]: their indices into bound_f2e / bound_forn */
    dfl_porosity_totals* tot;         /* device [1] */
    dfl_porosity_totals* h_tot;       /* pinned host [1]: valid after a synchronisation */
    uint64_t *key, *key_out;          /* device [cap] */
    f64* vals;                        /* device [cap][2] */
    void* temp;                       /* radix sort scratch for cap keys */
    int64_t temp_bytes;
    index_type cap;
    index_type steps;                 /* DflTimeStep calls since the Set call */
    index_type launches;              /* of the last evaluation */
    int64_t evaluations;
} PorosityState;

static PorosityState* st_of(const Mesh3D* mesh) {
    const MeshExt* x = (const MeshExt*)mesh->ext;
    return x ? x->porosity : NULL;
}

static void free_lists(PorosityState* st) {
    CdamFreeDevice(st->key, 0);
    CdamFreeDevice(st->key_out, 0);
    CdamFreeDevice(st->vals, 0);
    CdamFreeDevice(st->temp, 0);
    st->key = st->key_out = NULL;
    st->vals = NULL;
    st->temp = NULL;
}

static void alloc_lists(PorosityState* st, index_type cap) {
    st->cap = cap > 0 ? cap : 1;
    st->key = (uint64_t*)CdamMallocDevice((ptrdiff_t)st->cap * SIZE_OF(uint64_t));
    st->key_out = (uint64_t*)CdamMallocDevice((ptrdiff_t)st->cap * SIZE_OF(uint64_t));
    st->vals = (f64*)CdamMallocDevice((ptrdiff_t)st->cap * 2 * SIZE_OF(f64));
    st->temp_bytes = dfl_porosity_temp_bytes(st->cap);
    st->temp = CdamMallocDevice((ptrdiff_t)st->temp_bytes);
}

void DflPorosityFree(PorosityState* st) {
    if (!st) return;
    HIPGUARD(hipStreamSynchronize(DflStream()));
    CdamFreeDevice(st->parent, 0);
    CdamFreeDevice(st->label, 0);
    CdamFreeDevice(st->open, 0);
    CdamFreeDevice(st->rank, 0);
    CdamFreeDevice(st->pore, 0);
    CdamFreeDevice(st->ncount, 0);
    CdamFreeDevice(st->nbase, 0);
    CdamFreeDevice(st->tcount, 0);
    CdamFreeDevice(st->tbase, 0);
    CdamFreeDevice(st->chunk_sum, 0);
    CdamFreeDevice(st->part, 0);
    CdamFreeDevice(st->rows, 0);
    CdamFreeDevice(st->oface, 0);
    CdamFreeDevice(st->tot, 0);
    if (st->h_tot) HIPGUARD(hipHostFree(st->h_tot));
    free_lists(st);
    CdamFreeHost(st, SIZE_OF(PorosityState));
}

int DflPorosityCheck(const DflPorosity* c, char* why, size_t why_len) {
    if (!isfinite(c->level)) {
        snprintf(why, why_len, "level is not finite (%g)", c->level);
        return 1;
    }
    if (c->side != 1 && c->side != -1) {
        snprintf(why, why_len, "side must be +1 or -1, got %d", (int)c->side);
        return 2;
    }
    if (c->open_groups < 0) {
        snprintf(why, why_len, "open_groups must not be negative, got %d", (int)c->open_groups);
        return 3;
    }
    if (c->max_pores < 1 || c->max_pores > DFL_POROSITY_MAX_PORES) {
        snprintf(why, why_len, "max_pores must be in [1, %d], got %d", DFL_POROSITY_MAX_PORES, (int)c->max_pores);
        return 4;
    }
    if (c->every < 0) {
        snprintf(why, why_len, "every must not be negative, got %d", (int)c->every);
        return 5;
    }
    return 0;
}

/* the faces of the groups in the mask as indices into bound_f2e / bound_forn, ascending; returns their number */
static index_type open_faces(const Mesh3D* mesh, index_type mask, index_type* out) {
    index_type n = 0;
    for (index_type g = 0; g < mesh->num_bound && g < 31; ++g) {
        if (!(mask >> g & 1)) continue;
        for (index_type f = mesh->bound_elem_offset[g]; f < mesh->bound_elem_offset[g + 1]; ++f) {
            if (out) out[n] = f;
            ++n;
        }
    }
    return n;
}

void DflMeshSetPorosity(Mesh3D* mesh, const DflPorosity* cfg) {
    MeshExt* x = (MeshExt*)mesh->ext;
    if (!cfg) {
        DflPorosityFree(x->porosity);
        x->porosity = NULL;
        return;
    }
    char why[160];
    if (DflPorosityCheck(cfg, why, sizeof why)) {
        fprintf(stderr, "DflMeshSetPorosity: %s; unchanged\n", why);
        return;
    }
    hipStream_t s = DflStream();
    HIPGUARD(hipStreamSynchronize(s));
    PorosityState* st = x->porosity;
    if (!st) {
        st = (PorosityState*)CdamMallocHost(SIZE_OF(PorosityState));
        memset(st, 0, sizeof *st);
        st->N = Mesh3DNumNode(mesh);
        st->T = Mesh3DNumTet(mesh);
        const index_type per = dfl_tets_per_block();
        st->nblk_node = (st->N + per - 1) / per;
        st->nblk_tet = (st->T + per - 1) / per;
        const ptrdiff_t n = st->N > 0 ? st->N : 1, bn = st->nblk_node > 0 ? st->nblk_node : 1, bt = st->nblk_tet > 0 ? st->nblk_tet : 1;
        st->parent = (index_type*)CdamMallocDevice(n * SIZE_OF(index_type));
        st->label = (index_type*)CdamMallocDevice(n * SIZE_OF(index_type));
        st->open = (index_type*)CdamMallocDevice(n * SIZE_OF(index_type));
        st->rank = (index_type*)CdamMallocDevice(n * SIZE_OF(index_type));
        st->pore = (index_type*)CdamMallocDevice(n * SIZE_OF(index_type));
        st->ncount = (index_type*)CdamMallocDevice(bn * SIZE_OF(index_type));
        st->nbase = (index_type*)CdamMallocDevice((bn + 1) * SIZE_OF(index_type));
        st->tcount = (index_type*)CdamMallocDevice(bt * SIZE_OF(index_type));
        st->tbase = (index_type*)CdamMallocDevice((bt + 1) * SIZE_OF(index_type));
        st->chunk_sum = (index_type*)CdamMallocDevice((ptrdiff_t)dfl_scan_num_chunks((index_type)(bn > bt ? bn : bt)) * SIZE_OF(index_type));
        st->part = (f64*)CdamMallocDevice(bt * 3 * SIZE_OF(f64));
        st->tot = (dfl_porosity_totals*)CdamMallocDevice(SIZE_OF(dfl_porosity_totals));
        HIPGUARD(hipHostMalloc((void**)&st->h_tot, sizeof(dfl_porosity_totals), hipHostMallocDefault));
        alloc_lists(st, 1024);
        x->porosity = st;
    }
    if (cfg->max_pores > st->max_alloc) {
        CdamFreeDevice(st->rows, 0);
        st->rows = (dfl_pore_row*)CdamMallocDevice((ptrdiff_t)cfg->max_pores * SIZE_OF(dfl_pore_row));
        st->max_alloc = cfg->max_pores;
    }
    st->nof = open_faces(mesh, cfg->open_groups, NULL);
    if (st->nof > st->nof_alloc) {
        CdamFreeDevice(st->oface, 0);
        st->oface = (index_type*)CdamMallocDevice((ptrdiff_t)st->nof * SIZE_OF(index_type));
        st->nof_alloc = st->nof;
    }
    if (st->nof > 0) {
        index_type* h = (index_type*)CdamMallocHost((ptrdiff_t)st->nof * SIZE_OF(index_type));
        open_faces(mesh, cfg->open_groups, h);
        HIPGUARD(hipMemcpy(st->oface, h, (size_t)st->nof * sizeof(index_type), H2D));
        CdamFreeHost(h, (ptrdiff_t)st->nof * SIZE_OF(index_type));
    }
    st->cfg = *cfg;
    st->prm.level = cfg->level;
    st->prm.side = (f64)cfg->side;
    st->prm.max_pores = cfg->max_pores;
    st->steps = 0;
    st->launches = 0;
    st->evaluations = 0;
    memset(st->h_tot, 0, sizeof *st->h_tot);
    /* no evaluation yet: every node reads as metal outside any pore */
    HIPGUARD(hipMemsetAsync(st->label, 0xff, (size_t)(st->N > 0 ? st->N : 1) * sizeof(index_type), s));
    HIPGUARD(hipMemsetAsync(st->pore, 0xff, (size_t)(st->N > 0 ? st->N : 1) * sizeof(index_type), s));
    HIPGUARD(hipStreamSynchronize(s));
}

b32 DflMeshPorosityEnabled(const Mesh3D* mesh) { return st_of(mesh) != NULL; }

index_type DflMeshPorosity(Mesh3D* mesh, const f64* w) {
    PorosityState* st = st_of(mesh);
    if (!st) {
        fprintf(stderr, "DflMeshPorosity: no porosity record is set on this mesh (DflMeshSetPorosity)\n");
        return -1;
    }
    if (st->T <= 0 || st->N <= 0) return 0;
    hipStream_t s = DflStream();
    const Mesh3DData* dev = Mesh3DDevice(mesh);
    const dfl_porosity_params* p = &st->prm;
    DflRangePush("DflMeshPorosity");
    int n = dfl_porosity_label(st->N, st->T, dev->ien, w, p, st->nof, st->oface, mesh->bound_f2e, mesh->bound_forn, st->parent,
                               st->label, st->open, st->rows, st->tot, s);
    n += dfl_porosity_rank(st->N, dev->xg, p, st->label, st->open, st->ncount, st->nbase, st->chunk_sum, st->rank, st->pore, st->rows,
                           st->tot, s);
    n += dfl_porosity_tets(st->T, dev->ien, dev->xg, w, st->N, p, st->label, st->open, st->nblk_node, st->nbase, st->tcount,
                           st->tbase, st->chunk_sum, st->part, st->tot, s);
    HIPGUARD(hipMemcpyAsync(st->h_tot, st->tot, sizeof *st->h_tot, D2H, s));
    HIPGUARD(hipStreamSynchronize(s)); /* the one wait: the pore and closed-tet counts (and everything else of the totals) */
    const index_type closed = st->h_tot->count[2];
    if (closed > st->cap) {
        free_lists(st);
        alloc_lists(st, DflGrowCap(closed));
    }
    n += dfl_porosity_pores(st->T, dev->ien, dev->xg, w, st->N, p, st->label, st->open, st->pore, st->tbase, closed, st->key,
                            st->key_out, st->cap, st->vals, st->temp, st->temp_bytes, st->rows, s);
    st->launches = n;
    st->evaluations++;
    DflRangePop();
    return st->h_tot->count[1];
}

void DflMeshPorosityStats(Mesh3D* mesh, DflPorosityStats* out) {
    const PorosityState* st = st_of(mesh);
    if (!st) {
        fprintf(stderr, "DflMeshPorosityStats: no porosity record is set on this mesh (DflMeshSetPorosity)\n");
        return;
    }
    HIPGUARD(hipStreamSynchronize(DflStream()));
    const dfl_porosity_totals* t = st->h_tot;
    out->components = t->count[0];
    out->pores = t->count[1];
    out->listed = t->count[1] < st->prm.max_pores ? t->count[1] : st->prm.max_pores;
    out->bad_nodes = t->count[3];
    out->bad_tets = t->count[4];
    out->volume_metal = t->volume[0];
    out->volume_open = t->volume[1];
    out->volume_pores = t->volume[2];
    const f64 both = out->volume_metal + out->volume_pores;
    out->porosity = both > 0.0 ? out->volume_pores / both : 0.0;
}

/* the double an ordered integer of the kernels stands for (dfl_pore_row); + 0.0: a zero is +0.0 */
static f64 ordered_value(uint64_t k) {
    const uint64_t u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    f64 v;
    memcpy(&v, &u, sizeof v);
    return v + 0.0;
}

index_type DflMeshPorosityResult(Mesh3D* mesh, DflPore* out, index_type cap) {
    const PorosityState* st = st_of(mesh);
    if (!st) {
        fprintf(stderr, "DflMeshPorosityResult: no porosity record is set on this mesh (DflMeshSetPorosity)\n");
        return -1;
    }
    HIPGUARD(hipStreamSynchronize(DflStream()));
    const index_type pores = st->h_tot->count[1];
    const index_type listed = pores < st->prm.max_pores ? pores : st->prm.max_pores;
    const index_type n = listed < cap ? listed : cap;
    if (n <= 0 || !out) return listed;
    dfl_pore_row* h = (dfl_pore_row*)CdamMallocHost((ptrdiff_t)n * SIZE_OF(dfl_pore_row));
    HIPGUARD(hipMemcpy(h, st->rows, (size_t)n * sizeof(dfl_pore_row), D2H));
    for (index_type k = 0; k < n; ++k) {
        DflPore* r = out + k;
        r->label = h[k].label;
        r->nodes = h[k].nodes;
        r->tets = h[k].tets;
        r->volume = h[k].volume;
        r->volume_scale = h[k].volume_scale;
        for (int d = 0; d < 3; ++d) {
            r->lo[d] = ordered_value(h[k].ext[d]);
            r->hi[d] = ordered_value(h[k].ext[3 + d]);
        }
        r->T_wall_min = ordered_value(h[k].ext[6]);
        r->T_wall_max = ordered_value(h[k].ext[7]);
    }
    CdamFreeHost(h, (ptrdiff_t)n * SIZE_OF(dfl_pore_row));
    return listed;
}

index_type DflMeshPorosityLabels(const Mesh3D* mesh, const index_type** label, const index_type** pore) {
    const PorosityState* st = st_of(mesh);
    if (label) *label = st ? st->label : NULL;
    if (pore) *pore = st ? st->pore : NULL;
    return st ? st->N : 0;
}

index_type DflPorosityTestLaunches(const Mesh3D* mesh) {
    const PorosityState* st = st_of(mesh);
    return st ? st->launches : 0;
}

index_type DflPorosityTestCapacity(Mesh3D* mesh, index_type cap) {
    PorosityState* st = st_of(mesh);
    if (!st) return 0;
    if (cap > 0 && cap < st->cap) {
        HIPGUARD(hipStreamSynchronize(DflStream()));
        free_lists(st);
        alloc_lists(st, cap);
    }
    return st->cap;
}

b32 DflPorosityInTimeStep(const Mesh3D* mesh) {
    const PorosityState* st = st_of(mesh);
    return st && st->cfg.every > 0;
}

/* DflTimeStep: counts the call; on every every-th since the Set call evaluates at wgold */
void DflPorosityTimeStep(Mesh3D* mesh, const f64* wgold) {
    PorosityState* st = st_of(mesh);
    if (!st || st->cfg.every <= 0) return;
    if (++st->steps % st->cfg.every != 0) return;
    DflMeshPorosity(mesh, wgold);
}
