/* PC_AMGX: a native scalar algebraic multigrid behind the reference's PCCreateAMGX (pc.c:160-235, 279-295), with the
 * configuration the reference sketches at krylov.c:413-437 (AGGREGATION, SIZE_2, MULTICOLOR_DILU, V(0,3), omega 0.75,
 * DENSE_LU_SOLVER on >= 32 rows).  Kernels: csrc/k_amgx.hip.  Options: amgx_config.c.  Algorithm, and why the coarsest solve
 * tolerates a singular matrix: DESIGN.md "PC_AMGX".
 *
 * Structure (aggregates, Galerkin patterns and lists, colourings) is built on the host ONCE, in PCCreateAMGX, from the
 * values the matrix holds then -- as AMGX_solver_setup does in the reference's create -- and again only by PCAMGXRebuild.
 * amgx_build goes one level at a time: amgx_host_level (no HIP) completes the level's host structure from its matrix,
 * amgx_upload_level puts it on the device, amgx_galerkin_host forms the next level's matrix, and the level's host arrays
 * are freed.  The bucket lists (aggregate members, colour rows, Galerkin lists) come from csr_lists.h.
 * PCSetup recomputes every value on the device from the current fine values: Galerkin sums in list order, the smoother's
 * diagonal, the dense LU of the coarsest level.  Levels with more than `tail_rows` rows run one launch per colour and
 * triangular pass; all smaller levels and the coarse solve run in one launch of one workgroup (setup and cycle alike). */
#include <math.h>
#include <stddef.h>
#include <string.h>
#include "dedflow.h"
#include "dedflow_kernels.h"
#include "host_private.h"
#include "csr_lists.h"

/* ============================== hierarchy (host) ======================================= */
/* one pairwise pass.  Strength w_ij = (|a_ij|/|a_ii| + |a_ji|/|a_jj|) / 2 (a_ji = 0 if not stored; a ratio with a zero
 * diagonal counts 0); only neighbours with w_ij > 0 count.  Four handshake rounds: every unaggregated row picks its
 * strongest unaggregated neighbour (ties: the smaller column), mutual picks become pairs.  A row left over joins the
 * aggregate of its strongest neighbour if the rounds paired that one, else it stays a singleton.  Aggregates are numbered
 * in the order of their smallest member.  Returns the number of aggregates. */
static index_type amgx_pairwise(index_type n, const index_type* rp, const index_type* ci, const f64* val, index_type* agg) {
    const index_type nnz = rp[n];
    f64* dg = (f64*)malloc(sizeof(f64) * (size_t)(n > 0 ? n : 1));
    f64* w = (f64*)malloc(sizeof(f64) * (size_t)(nnz > 0 ? nnz : 1));
    index_type* label = (index_type*)malloc(sizeof(index_type) * (size_t)(n > 0 ? n : 1));
    index_type* pick = (index_type*)malloc(sizeof(index_type) * (size_t)(n > 0 ? n : 1));
    for (index_type i = 0; i < n; ++i) {
        const index_type d = csr_find(rp, ci, i, i);
        dg[i] = d >= 0 ? fabs(val[d]) : 0.0;
    }
    for (index_type i = 0; i < n; ++i)
        for (index_type k = rp[i]; k < rp[i + 1]; ++k) {
            const index_type j = ci[k];
            if (j == i) { w[k] = 0.0; continue; }
            const index_type t = csr_find(rp, ci, j, i);
            const f64 aij = dg[i] > 0.0 ? fabs(val[k]) / dg[i] : 0.0;
            const f64 aji = (t >= 0 && dg[j] > 0.0) ? fabs(val[t]) / dg[j] : 0.0;
            w[k] = 0.5 * (aij + aji);
        }
    for (index_type i = 0; i < n; ++i) label[i] = -1;
    for (int round = 0; round < 4; ++round) {
        for (index_type i = 0; i < n; ++i) {
            pick[i] = -1;
            if (label[i] >= 0) continue;
            f64 best = 0.0;
            for (index_type k = rp[i]; k < rp[i + 1]; ++k) {
                const index_type j = ci[k];
                if (j == i || label[j] >= 0) continue;
                if (w[k] > best) { best = w[k]; pick[i] = j; } /* ascending columns: the smaller j wins a tie */
            }
        }
        for (index_type i = 0; i < n; ++i) {
            const index_type j = pick[i];
            if (j > i && pick[j] == i) label[i] = label[j] = i;
        }
    }
    /* leftovers: decided against the paired state of the rounds only, so the order does not matter */
    for (index_type i = 0; i < n; ++i) {
        pick[i] = -1;
        if (label[i] >= 0) continue;
        f64 best = 0.0;
        index_type s = -1;
        for (index_type k = rp[i]; k < rp[i + 1]; ++k)
            if (ci[k] != i && w[k] > best) { best = w[k]; s = ci[k]; }
        pick[i] = s;
    }
    for (index_type i = 0; i < n; ++i)
        if (label[i] < 0) {
            const index_type s = pick[i];
            label[i] = (s >= 0 && label[s] >= 0) ? label[s] : -2 - i; /* -2 - i: singleton, resolved below */
        }
    for (index_type i = 0; i < n; ++i)
        if (label[i] <= -2) label[i] = i;
    /* numbering by the smallest member (pick reused as the smallest member of each label) */
    for (index_type i = 0; i < n; ++i) pick[i] = n;
    for (index_type i = 0; i < n; ++i)
        if (i < pick[label[i]]) pick[label[i]] = i;
    index_type nc = 0;
    index_type* id = (index_type*)malloc(sizeof(index_type) * (size_t)(n > 0 ? n : 1));
    for (index_type i = 0; i < n; ++i)
        if (pick[label[i]] == i) id[label[i]] = nc++;
    for (index_type i = 0; i < n; ++i) agg[i] = id[label[i]];
    free(id);
    free(dg);
    free(w);
    free(label);
    free(pick);
    return nc;
}

/* One level on the host.  All arrays are owned here (amgx_host_free).  The matrix (and, below level 0, the Galerkin lists
 * that produced it) comes first; amgx_host_level completes the rest from it. */
typedef struct AmgxHost {
    index_type n, nnz;
    index_type *rp, *ci;
    f64* val;
    index_type *goff, *gidx;             /* NULL on level 0 */
    index_type *diag, *trans;            /* position of a_ii; of a_ji for every a_ij (-1: not stored) */
    index_type ncolor, *color, *coff, *rows;
    index_type nc, *agg, *aoff, *amem;   /* nc == 0: the coarsest level, no map */
} AmgxHost;

/* everything but the matrix and the map with its members (what the Galerkin product of the next level reads) */
static void amgx_host_free_structure(AmgxHost* H) {
    free(H->goff);
    free(H->gidx);
    free(H->diag);
    free(H->trans);
    free(H->color);
    free(H->coff);
    free(H->rows);
    H->goff = H->gidx = H->diag = H->trans = H->color = H->coff = H->rows = NULL;
}
static void amgx_host_free(AmgxHost* H) {
    amgx_host_free_structure(H);
    free(H->rp);
    free(H->ci);
    free(H->val);
    free(H->agg);
    free(H->aoff);
    free(H->amem);
    memset(H, 0, sizeof *H);
}

/* The next level C = P^T A P for the map agg (nc aggregates, members amem[aoff[c] .. aoff[c+1]) ascending): pattern (columns
 * ascending), per coarse nonzero the ascending list of fine nonzeros summed into it, and the values in that order */
static void amgx_galerkin_host(index_type n, const index_type* rp, const index_type* ci, const f64* val, const index_type* agg,
                               index_type nc, const index_type* aoff, const index_type* amem, AmgxHost* C) {
    memset(C, 0, sizeof *C);
    index_type* mark = (index_type*)malloc(sizeof(index_type) * (size_t)(nc > 0 ? nc : 1));
    for (index_type c = 0; c < nc; ++c) mark[c] = -1;
    C->n = nc;
    C->rp = (index_type*)calloc((size_t)nc + 1, sizeof(index_type));
    size_t cap = (size_t)rp[n] + 1, used = 0;
    C->ci = (index_type*)malloc(sizeof(index_type) * cap);
    for (index_type c = 0; c < nc; ++c) {
        const size_t start = used;
        for (index_type t = aoff[c]; t < aoff[c + 1]; ++t) {
            const index_type i = amem[t];
            for (index_type k = rp[i]; k < rp[i + 1]; ++k) {
                const index_type J = agg[ci[k]];
                if (mark[J] != c) { mark[J] = c; C->ci[used++] = J; }
            }
        }
        /* insertion sort of the row (short rows) */
        for (size_t a = start + 1; a < used; ++a) {
            const index_type v = C->ci[a];
            size_t b = a;
            while (b > start && C->ci[b - 1] > v) { C->ci[b] = C->ci[b - 1]; --b; }
            C->ci[b] = v;
        }
        C->rp[c + 1] = (index_type)used;
    }
    free(mark);
    C->nnz = (index_type)used;
    const index_type nnzf = rp[n];
    index_type* pos = (index_type*)malloc(sizeof(index_type) * (size_t)(nnzf > 0 ? nnzf : 1));
    for (index_type i = 0; i < n; ++i)
        for (index_type k = rp[i]; k < rp[i + 1]; ++k) pos[k] = csr_find(C->rp, C->ci, agg[i], agg[ci[k]]);
    csr_bucket_fill(nnzf, pos, C->nnz, &C->goff, &C->gidx);
    free(pos);
    C->val = (f64*)malloc(sizeof(f64) * (size_t)(C->nnz > 0 ? C->nnz : 1));
    for (index_type k = 0; k < C->nnz; ++k) {
        f64 s = 0.0;
        for (index_type t = C->goff[k]; t < C->goff[k + 1]; ++t) s += val[C->gidx[t]];
        C->val[k] = s;
    }
}

/* `passes` pairwise passes composed (SIZE_2 / 4 / 8).  Loop state: the current graph (the caller's matrix, then the
 * Galerkin graph G of the map so far) and agg, the map from the caller's rows to the current graph's aggregates; every
 * pass pairs the rows of the current graph (step) and is composed into agg. */
static index_type amgx_aggregate(index_type n, const index_type* rp, const index_type* ci, const f64* val, int passes,
                                 index_type* agg) {
    index_type* step = (index_type*)malloc(sizeof(index_type) * (size_t)(n > 0 ? n : 1));
    AmgxHost G = {0};
    index_type cn = n, nc = n;
    for (index_type i = 0; i < n; ++i) agg[i] = i;
    for (int p = 0; p < passes; ++p) {
        if (p > 0) {
            if (nc <= 1) break;
            index_type *aoff, *amem;
            AmgxHost H;
            csr_bucket_fill(cn, step, nc, &aoff, &amem);
            amgx_galerkin_host(cn, rp, ci, val, step, nc, aoff, amem, &H);
            free(aoff);
            free(amem);
            amgx_host_free(&G);
            G = H;
            cn = nc;
            rp = G.rp;
            ci = G.ci;
            val = G.val;
        }
        nc = amgx_pairwise(cn, rp, ci, val, step);
        for (index_type i = 0; i < n; ++i) agg[i] = step[agg[i]];
    }
    amgx_host_free(&G);
    free(step);
    return nc;
}

index_type DflAMGXAggregateHost(index_type n, const index_type* rp, const index_type* ci, const f64* val, int passes,
                                index_type* agg_out) {
    return amgx_aggregate(n, rp, ci, val, passes < 1 ? 1 : passes, agg_out);
}

/* greedy colouring in ascending row order: the smallest colour no already-coloured neighbour has */
static index_type amgx_color(index_type n, const index_type* rp, const index_type* ci, index_type* color) {
    index_type* mark = (index_type*)malloc(sizeof(index_type) * (size_t)(n + 1));
    for (index_type c = 0; c <= n; ++c) mark[c] = -1;
    index_type nc = 0;
    for (index_type i = 0; i < n; ++i) color[i] = -1;
    for (index_type i = 0; i < n; ++i) {
        for (index_type k = rp[i]; k < rp[i + 1]; ++k) {
            const index_type j = ci[k];
            if (j != i && color[j] >= 0) mark[color[j]] = i;
        }
        index_type c = 0;
        while (mark[c] == i) ++c;
        color[i] = c;
        if (c + 1 > nc) nc = c + 1;
    }
    free(mark);
    return nc;
}

/* the structure of level number `depth` (from 1) from its matrix; no HIP in here.  The map comes first: the passes of
 * amgx_aggregate hold the most memory, so nothing else of the level is alive then. */
static void amgx_host_level(AmgxHost* H, const DflAMGXConfig* cfg, index_type depth) {
    const index_type n = H->n;
    /* stop rules: small enough, level budget, a pass that keeps more than 90 % of the rows */
    H->nc = 0;
    if (n > cfg->min_coarse_rows && depth < cfg->max_levels) {
        H->agg = (index_type*)malloc(sizeof(index_type) * (size_t)(n > 0 ? n : 1));
        H->nc = amgx_aggregate(n, H->rp, H->ci, H->val, cfg->selector_passes, H->agg);
        if ((f64)H->nc > 0.9 * (f64)n) {
            free(H->agg);
            H->agg = NULL;
            H->nc = 0;
        } else {
            csr_bucket_fill(n, H->agg, H->nc, &H->aoff, &H->amem);
        }
    }
    H->diag = (index_type*)malloc(sizeof(index_type) * (size_t)(n > 0 ? n : 1));
    H->trans = (index_type*)malloc(sizeof(index_type) * (size_t)(H->nnz > 0 ? H->nnz : 1));
    for (index_type i = 0; i < n; ++i) {
        H->diag[i] = csr_find(H->rp, H->ci, i, i);
        for (index_type k = H->rp[i]; k < H->rp[i + 1]; ++k) H->trans[k] = csr_find(H->rp, H->ci, H->ci[k], i);
    }
    H->color = (index_type*)malloc(sizeof(index_type) * (size_t)(n > 0 ? n : 1));
    H->ncolor = amgx_color(n, H->rp, H->ci, H->color);
    csr_bucket_fill(n, H->color, H->ncolor, &H->coff, &H->rows);
}
/* ============================== the preconditioner ===================================== */
#define AMGX_MAX_COARSE 2048 /* rows of the coarsest level: the dense LU runs in one workgroup */

typedef struct AmgxLevel {
    dfl_amgx_level d;      /* device pointers as the kernels see them */
    index_type* coff;      /* host [ncolor+1] */
    CSRAttr attr;          /* the level's pattern (device row_ptr / col_ind) for PCAMGXLevelMatrix */
    Matrix* mat;           /* CSR view of the level's values */
    b32 own_val;           /* val allocated here (not the caller's CSR values) */
} AmgxLevel;

typedef struct PCAmgx {
    DflAMGXConfig cfg;
    Matrix* A;              /* MAT_TYPE_CSR with its own values, or a view of a block-mode MatrixFS */
    const value_type* block_val; /* view: the parent's 4x4 blocks (entry [3][3] is A11) */
    index_type nlev, l0;    /* levels; the first level of the tail */
    index_type tail_rows;
    AmgxLevel* lev;
    dfl_amgx_level* d_lev;  /* device copy of the level records (the tail kernels read it) */
    b32 d_lev_stale;        /* the records changed since they were copied */
    value_type *t0, *e0, *w1; /* level 0: residual of later cycles, their correction, a second scratch */
    int64_t launches_apply, launches_setup;
    f64 op_complexity;
} PCAmgx;

static void* amgx_dev(size_t bytes) { return CdamMallocDevice((ptrdiff_t)(bytes > 0 ? bytes : 8)); }
static void* amgx_up(const void* h, size_t bytes) {
    void* d = amgx_dev(bytes);
    if (bytes) HIPGUARD(hipMemcpy(d, h, bytes, H2D));
    return d;
}

/* the device arrays a level owns, as members of dfl_amgx_level.  val is not among them (level 0 may hold the caller's:
 * own_val), nor zpiv (the second half of piv) */
#define LV(m) offsetof(dfl_amgx_level, m)
static const size_t amgx_level_owned[] = {LV(rp),   LV(ci),   LV(diag), LV(trans), LV(color), LV(rows), LV(coff), LV(agg), LV(aoff),
                                          LV(amem), LV(goff), LV(gidx), LV(einv),  LV(b),     LV(x),    LV(w),    LV(lu),  LV(piv)};
#undef LV

static void amgx_free_levels(PCAmgx* p) {
    if (!p->lev) return;
    HIPGUARD(hipStreamSynchronize(DflStream()));
    for (index_type l = 0; l < p->nlev; ++l) {
        AmgxLevel* L = &p->lev[l];
        if (L->mat) {
            ((MatrixCSR*)L->mat->data)->val = NULL; /* the values belong to this object or to the caller */
            MatrixDestroy(L->mat);
        }
        for (size_t k = 0; k < sizeof amgx_level_owned / sizeof amgx_level_owned[0]; ++k) {
            void* q;
            memcpy(&q, (char*)&L->d + amgx_level_owned[k], sizeof q);
            if (q) CdamFreeDevice(q, 0);
        }
        if (L->own_val) CdamFreeDevice(L->d.val, 0);
        free(L->coff);
    }
    free(p->lev);
    p->lev = NULL;
    if (p->d_lev) CdamFreeDevice(p->d_lev, 0);
    if (p->t0) CdamFreeDevice(p->t0, 0);
    if (p->e0) CdamFreeDevice(p->e0, 0);
    if (p->w1) CdamFreeDevice(p->w1, 0);
    p->d_lev = NULL;
    p->t0 = p->e0 = p->w1 = NULL;
    p->nlev = 0;
}

/* the fine matrix: pattern and current values on the host; FALSE if it is not a supported kind */
static b32 amgx_fine(PCAmgx* p, index_type* n_out, const CSRAttr** attr_out, value_type** dval_out) {
    Matrix* A = p->A;
    if (!A || A->type != MAT_TYPE_CSR) return FALSE;
    MatrixCSR* c = (MatrixCSR*)A->data;
    const CSRAttr* at = c->attr;
    if (!at || at->num_row != at->num_col || at->parent) return FALSE; /* scalar, square, not row-expanded */
    p->block_val = NULL;
    if (c->owner && c->owner->block_mode) {
        MatrixFS* fs = c->owner;
        if (c->owner_slot != fs->n_offset + 1 || fs->spy1x1 != at || fs->owned_rows != at->num_row) return FALSE;
        p->block_val = fs->block_val;
        *dval_out = NULL;
    } else {
        if (!c->val) return FALSE;
        *dval_out = c->val;
    }
    *n_out = at->num_row;
    *attr_out = at;
    return TRUE;
}

static void amgx_level_matrix(AmgxLevel* L) {
    L->attr.num_row = L->attr.num_col = L->d.n;
    L->attr.nnz = L->d.nnz;
    L->attr.row_ptr = (index_type*)L->d.rp;
    L->attr.col_ind = (index_type*)L->d.ci;
    L->attr.parent = NULL;
    L->mat = MatrixCreateTypeCSR(&L->attr, NULL);
    ((MatrixCSR*)L->mat->data)->val = L->d.val;
}

/* level L on the device from its host structure H.  val0: the device values of level 0 (the caller's array, or the
 * gathered A11 this level then owns); every other level uploads its own.  The coarsest level that fits gets the dense LU. */
static void amgx_upload_level(AmgxLevel* L, const AmgxHost* H, value_type* val0, b32 own_val0) {
    dfl_amgx_level* d = &L->d;
    const size_t n = (size_t)H->n, nnz = (size_t)H->nnz, I = sizeof(index_type);
    d->n = H->n;
    d->nnz = H->nnz;
    d->ncolor = H->ncolor;
    d->nc = H->nc;
    d->rp = (index_type*)amgx_up(H->rp, I * (n + 1));
    d->ci = (index_type*)amgx_up(H->ci, I * nnz);
    if (H->goff) {
        d->val = (value_type*)amgx_up(H->val, sizeof(f64) * nnz);
        L->own_val = TRUE;
        d->goff = (index_type*)amgx_up(H->goff, I * (nnz + 1));
        d->gidx = (index_type*)amgx_up(H->gidx, I * (size_t)H->goff[nnz]);
    } else {
        d->val = val0;
        L->own_val = own_val0;
    }
    d->trans = (index_type*)amgx_up(H->trans, I * nnz);
    d->diag = (index_type*)amgx_up(H->diag, I * n);
    d->rows = (index_type*)amgx_up(H->rows, I * n);
    d->color = (index_type*)amgx_up(H->color, I * n);
    d->coff = (index_type*)amgx_up(H->coff, I * ((size_t)H->ncolor + 1));
    L->coff = (index_type*)malloc(I * ((size_t)H->ncolor + 1));
    memcpy(L->coff, H->coff, I * ((size_t)H->ncolor + 1));
    d->einv = (value_type*)amgx_dev(sizeof(f64) * n);
    d->b = (value_type*)amgx_dev(sizeof(f64) * n);
    d->x = (value_type*)amgx_dev(sizeof(f64) * n);
    d->w = (value_type*)amgx_dev(sizeof(f64) * n);
    if (H->nc) {
        d->agg = (index_type*)amgx_up(H->agg, I * n);
        d->aoff = (index_type*)amgx_up(H->aoff, I * ((size_t)H->nc + 1));
        d->amem = (index_type*)amgx_up(H->amem, I * n);
    } else if (H->n <= AMGX_MAX_COARSE) {
        d->lu = (value_type*)amgx_dev(sizeof(f64) * n * n);
        d->piv = (index_type*)amgx_dev(I * 2 * n);
        d->zpiv = d->piv + n;
    }
}

/* structure of every level; returns FALSE (with a message) if the hierarchy cannot be built */
static b32 amgx_build(PCAmgx* p) {
    index_type n;
    const CSRAttr* at;
    value_type* dval;
    if (!amgx_fine(p, &n, &at, &dval)) {
        fprintf(stderr, "PCCreateAMGX: needs a square MAT_TYPE_CSR matrix with its own values or the A11 view of a block-mode "
                        "MatrixFS on one GPU\n");
        return FALSE;
    }
    hipStream_t s = DflStream();
    HIPGUARD(hipStreamSynchronize(s));
    AmgxHost H = {0}; /* the current level, coarsened until a stop rule holds */
    H.n = n;
    H.rp = (index_type*)malloc(sizeof(index_type) * ((size_t)n + 1));
    HIPGUARD(hipMemcpy(H.rp, at->row_ptr, sizeof(index_type) * ((size_t)n + 1), D2H));
    const index_type nnz = H.nnz = H.rp[n];
    H.ci = (index_type*)malloc(sizeof(index_type) * (size_t)(nnz > 0 ? nnz : 1));
    H.val = (f64*)malloc(sizeof(f64) * (size_t)(nnz > 0 ? nnz : 1));
    HIPGUARD(hipMemcpy(H.ci, at->col_ind, sizeof(index_type) * (size_t)nnz, D2H));
    value_type* v0 = dval;
    if (p->block_val) {
        v0 = (value_type*)amgx_dev(sizeof(f64) * (size_t)nnz);
        dfl_amgx_gather_a11(nnz, p->block_val, v0, s);
    }
    HIPGUARD(hipMemcpy(H.val, v0, sizeof(f64) * (size_t)nnz, D2H));
    b32 ok = TRUE;
    for (index_type i = 0; i < n && ok; ++i) {
        for (index_type k = H.rp[i] + 1; k < H.rp[i + 1]; ++k)
            if (H.ci[k] <= H.ci[k - 1]) ok = FALSE;
        if (csr_find(H.rp, H.ci, i, i) < 0) ok = FALSE;
    }
    if (!ok) {
        fprintf(stderr, "PCCreateAMGX: every row needs its diagonal and ascending column indices\n");
        if (p->block_val) CdamFreeDevice(v0, 0);
        amgx_host_free(&H);
        return FALSE;
    }
    int cap = 8;
    p->lev = (AmgxLevel*)calloc((size_t)cap, sizeof(AmgxLevel));
    p->nlev = 0;
    f64 nnz_total = 0.0;
    for (;;) {
        if (p->nlev == cap) {
            cap *= 2;
            p->lev = (AmgxLevel*)realloc(p->lev, sizeof(AmgxLevel) * (size_t)cap);
            memset(p->lev + cap / 2, 0, sizeof(AmgxLevel) * (size_t)(cap / 2));
        }
        nnz_total += H.nnz;
        amgx_host_level(&H, &p->cfg, p->nlev + 1);
        amgx_upload_level(&p->lev[p->nlev++], &H, v0, p->block_val != NULL);
        amgx_host_free_structure(&H);
        if (!H.nc) break;
        AmgxHost C;
        amgx_galerkin_host(H.n, H.rp, H.ci, H.val, H.agg, H.nc, H.aoff, H.amem, &C);
        amgx_host_free(&H);
        H = C;
    }
    if (H.n > AMGX_MAX_COARSE) {
        fprintf(stderr, "PCCreateAMGX: the coarsest level keeps %d rows (more than %d): no hierarchy\n", H.n, AMGX_MAX_COARSE);
        ok = FALSE;
    }
    amgx_host_free(&H);
    if (!ok) {
        amgx_free_levels(p);
        return FALSE;
    }
    p->op_complexity = nnz > 0 ? nnz_total / (f64)nnz : 1.0;
    /* the tail: the first level with at most tail_rows rows, the coarsest at the latest */
    p->l0 = p->nlev - 1;
    for (index_type l = 0; l < p->nlev; ++l)
        if (p->lev[l].d.n <= p->tail_rows) { p->l0 = l; break; }
    for (index_type l = 0; l < p->nlev; ++l) amgx_level_matrix(&p->lev[l]);
    p->t0 = (value_type*)amgx_dev(sizeof(f64) * (size_t)n);
    p->e0 = (value_type*)amgx_dev(sizeof(f64) * (size_t)n);
    p->w1 = (value_type*)amgx_dev(sizeof(f64) * (size_t)n);
    p->d_lev = (dfl_amgx_level*)amgx_dev(sizeof(dfl_amgx_level) * (size_t)p->nlev);
    p->d_lev_stale = TRUE;
    return TRUE;
}

static void amgx_upload_levels(PCAmgx* p) {
    dfl_amgx_level* h = (dfl_amgx_level*)malloc(sizeof(dfl_amgx_level) * (size_t)p->nlev);
    for (index_type l = 0; l < p->nlev; ++l) h[l] = p->lev[l].d;
    HIPGUARD(hipMemcpy(p->d_lev, h, sizeof(dfl_amgx_level) * (size_t)p->nlev, H2D));
    free(h);
}

static void amgx_setup(PC* pc) {
    PCAmgx* p = (PCAmgx*)pc->data;
    hipStream_t s = DflStream();
    int64_t nl = 0;
    AmgxLevel* L0 = &p->lev[0];
    MatrixCSR* c = (MatrixCSR*)p->A->data;
    if (p->block_val) {
        p->block_val = c->owner->block_val; /* the parent may have moved its block array (placement calibration) */
        dfl_amgx_gather_a11(L0->d.nnz, p->block_val, L0->d.val, s);
        nl++;
    } else if (c->val != L0->d.val) {
        L0->d.val = c->val;
        ((MatrixCSR*)L0->mat->data)->val = c->val;
        p->d_lev_stale = TRUE;
    }
    if (p->d_lev_stale) {
        amgx_upload_levels(p);
        p->d_lev_stale = FALSE;
    }
    const b32 jac = p->cfg.smoother == DFL_AMGX_SMOOTHER_JACOBI;
    for (index_type l = 0; l < p->l0; ++l) {
        AmgxLevel* L = &p->lev[l];
        if (l >= 1) { dfl_amgx_galerkin(L->d, p->lev[l - 1].d.val, s); nl++; }
        if (jac) { dfl_amgx_jacobi_setup(L->d, s); nl++; }
        else
            for (index_type cc = 0; cc < L->d.ncolor; ++cc) {
                dfl_amgx_dilu_setup_color(L->d, cc, L->coff[cc], L->coff[cc + 1] - L->coff[cc], s);
                nl++;
            }
    }
    dfl_amgx_tail_setup(p->d_lev, p->l0, p->nlev, jac, s);
    nl++;
    p->launches_setup = nl;
}

/* one smoothing step on grid level L (x / w swapped by Jacobi) */
static int64_t amgx_smooth(PCAmgx* p, AmgxLevel* L, dfl_amgx_level* d, b32 x_zero) {
    hipStream_t s = DflStream();
    const f64 om = p->cfg.relaxation_factor;
    if (p->cfg.smoother == DFL_AMGX_SMOOTHER_JACOBI) {
        dfl_amgx_jacobi_sweep(*d, om, x_zero, s);
        value_type* t = d->x;
        d->x = d->w;
        d->w = t;
        return 1;
    }
    for (index_type c = 0; c < d->ncolor; ++c) dfl_amgx_dilu_forward(*d, c, L->coff[c], L->coff[c + 1] - L->coff[c], x_zero, s);
    for (index_type c = d->ncolor - 1; c >= 0; --c)
        dfl_amgx_dilu_backward(*d, c, L->coff[c], L->coff[c + 1] - L->coff[c], om, x_zero, s);
    return 2 * (int64_t)d->ncolor;
}

/* where a level's iterate ends after pre + post sweeps that started in x (Jacobi alternates x and w) */
static value_type* amgx_final_x(const PCAmgx* p, index_type l, value_type* x, value_type* w) {
    if (l == p->nlev - 1) return x;
    const int sweeps = p->cfg.presweeps + p->cfg.postsweeps;
    return (p->cfg.smoother == DFL_AMGX_SMOOTHER_JACOBI && (sweeps & 1)) ? w : x;
}

/* one V-cycle from a zero initial guess: b -> x (level 0 uses b / x / w given here) */
static int64_t amgx_vcycle(PCAmgx* p, const value_type* b, value_type* x, value_type* w) {
    hipStream_t s = DflStream();
    int64_t nl = 0;
    const int pre = p->cfg.presweeps, post = p->cfg.postsweeps;
    dfl_amgx_level cur[64]; /* grid levels: the records with level 0's vectors and Jacobi's x / w exchanges applied */
    ASSERT(p->l0 <= 64);
    for (index_type l = 0; l < p->l0; ++l) {
        cur[l] = p->lev[l].d;
        if (l == 0) {
            cur[0].b = (value_type*)b;
            cur[0].x = x;
            cur[0].w = w;
        }
        for (int k = 0; k < pre; ++k) nl += amgx_smooth(p, &p->lev[l], &cur[l], k == 0);
        dfl_amgx_restrict(cur[l], p->lev[l + 1].d, pre == 0, s);
        nl++;
    }
    const b32 jac = p->cfg.smoother == DFL_AMGX_SMOOTHER_JACOBI;
    if (p->l0 == 0) dfl_amgx_tail_cycle(p->d_lev, 0, p->nlev, jac, pre, post, p->cfg.relaxation_factor, b, x, w, s);
    else {
        dfl_amgx_level* t = &p->lev[p->l0].d;
        dfl_amgx_tail_cycle(p->d_lev, p->l0, p->nlev, jac, pre, post, p->cfg.relaxation_factor, t->b, t->x, t->w, s);
    }
    nl++;
    for (index_type l = p->l0 - 1; l >= 0; --l) {
        const dfl_amgx_level* C = &p->lev[l + 1].d;
        dfl_amgx_prolong(cur[l], amgx_final_x(p, l + 1, C->x, C->w), pre == 0, s);
        nl++;
        for (int k = 0; k < post; ++k) nl += amgx_smooth(p, &p->lev[l], &cur[l], FALSE);
    }
    return nl;
}

/* z = M^-1 r: max_iters V-cycles, the first from z = 0, every further one z += V(r - A z) */
static void amgx_apply(PC* pc, value_type* r, value_type* z) {
    PCAmgx* p = (PCAmgx*)pc->data;
    hipStream_t s = DflStream();
    const index_type n = p->lev[0].d.n;
    const b32 odd = p->cfg.smoother == DFL_AMGX_SMOOTHER_JACOBI && p->nlev > 1 &&
                    ((p->cfg.presweeps + p->cfg.postsweeps) & 1);
    int64_t nl = 0;
    for (int it = 0; it < p->cfg.max_iters; ++it) {
        const value_type* b = r;
        value_type* out = z;
        if (it > 0) {
            dfl_amgx_residual(p->lev[0].d, r, z, p->t0, s);
            nl++;
            b = p->t0;
            out = p->e0;
        }
        /* the cycle's iterate starts in x and ends in x or w: arrange for it to end in `out` */
        if (odd) nl += amgx_vcycle(p, b, p->w1, out);
        else nl += amgx_vcycle(p, b, out, p->w1);
        if (it > 0) {
            dfl_daxpy(n, 1.0, p->e0, z, s);
            nl++;
        }
    }
    p->launches_apply = nl;
}

static void amgx_destroy(PC* pc) {
    PCAmgx* p = (PCAmgx*)pc->data;
    amgx_free_levels(p);
    free(p);
}

PC* PCCreateAMGX(Matrix* mat, void* options) {
    DflAMGXConfig cfg;
    if (DflAMGXParseConfig((const char*)options, &cfg)) return NULL;
    PCAmgx* p = (PCAmgx*)calloc(1, sizeof(PCAmgx));
    p->cfg = cfg;
    p->A = mat;
    p->tail_rows = 8192;
    const char* e = getenv("DFL_AMGX_TAIL_ROWS");
    if (e && *e) p->tail_rows = (index_type)atoi(e);
    if (!amgx_build(p)) {
        free(p);
        return NULL;
    }
    PC* pc = (PC*)CdamMallocHost(SIZE_OF(PC));
    memset(pc, 0, sizeof *pc);
    pc->type = PC_AMGX;
    pc->mat = mat;
    pc->data = p;
    pc->op->setup = amgx_setup;
    pc->op->apply = amgx_apply;
    pc->op->destroy = amgx_destroy;
    return pc;
}

void PCAMGXRebuild(PC* pc) {
    ASSERT(pc && pc->type == PC_AMGX);
    PCAmgx* p = (PCAmgx*)pc->data;
    amgx_free_levels(p);
    if (!amgx_build(p)) ASSERT(0 && "PCAMGXRebuild: the hierarchy cannot be rebuilt from the current values");
}

static PCAmgx* amgx_of(PC* pc) {
    ASSERT(pc && pc->type == PC_AMGX);
    return (PCAmgx*)pc->data;
}
index_type PCAMGXNumLevels(PC* pc) { return amgx_of(pc)->nlev; }
void PCAMGXInfo(PC* pc, index_type* rows, index_type* nnz, index_type* colors, f64* op_complexity, index_type* tail_level,
                int64_t* launches_apply, int64_t* launches_setup) {
    PCAmgx* p = amgx_of(pc);
    for (index_type l = 0; l < p->nlev; ++l) {
        if (rows) rows[l] = p->lev[l].d.n;
        if (nnz) nnz[l] = p->lev[l].d.nnz;
        if (colors) colors[l] = p->lev[l].d.ncolor;
    }
    if (op_complexity) *op_complexity = p->op_complexity;
    if (tail_level) *tail_level = p->l0;
    if (launches_apply) *launches_apply = p->launches_apply;
    if (launches_setup) *launches_setup = p->launches_setup;
}
const index_type* PCAMGXLevelAggregates(PC* pc, index_type l) {
    PCAmgx* p = amgx_of(pc);
    return (l >= 0 && l < p->nlev) ? p->lev[l].d.agg : NULL;
}
const index_type* PCAMGXLevelColors(PC* pc, index_type l) {
    PCAmgx* p = amgx_of(pc);
    return (l >= 0 && l < p->nlev) ? p->lev[l].d.color : NULL;
}
Matrix* PCAMGXLevelMatrix(PC* pc, index_type l) {
    PCAmgx* p = amgx_of(pc);
    return (l >= 0 && l < p->nlev) ? p->lev[l].mat : NULL;
}
const index_type* PCAMGXCoarsePivots(PC* pc) {
    PCAmgx* p = amgx_of(pc);
    return p->lev[p->nlev - 1].d.piv;
}
