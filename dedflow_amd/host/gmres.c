/* GMRES behind KrylovCreateGMRES: cached work space, the path plan of a solve, the operator, the Arnoldi step, the
 * host-read protocol and the two drivers (gmres_run, gmres_pipelined).
 *
 * Restates GMRESSolvePrivate (src/krylov.c:56-334): right-preconditioned full GMRES, classical Gram-Schmidt, Givens
 * rotations, residual recurrence, convergence test every 20 iterations.  Differences in mechanism only:
 *   - the two cublasDgemv + Dnrm2 + Dscal of an Arnoldi step are two fused passes (dfl_cgs_dots / dfl_cgs_update) and the
 *     normalisation is folded into the next preconditioner application -- or, one GPU with the Jacobi tree, never done:
 *     the basis stays unnormalised, the update applies M^-1 to the column it forms and the matvec divides by the norm
 *     (GMRES_STEP_RAW_BASIS); that step takes up to four products before it orthogonalises, so that one dots pass and one
 *     update pass over the basis serve up to four iterations (gmres_pair, gmres_block);
 *   - every scalar recurrence stays on the device; the host reads 8 bytes only when the reference tests convergence (every
 *     20th iteration) -- the reference syncs 2-3 times per iteration;
 *   - work space is cached in the Krylov object instead of malloc+memset per solve;
 *   - Krylov vectors cover [0,4N) when the phi/T tail of b is zero (it always is on the driver path, src/main.c:63-66),
 *     which leaves the arithmetic unchanged (Q5).
 *
 * What is fixed for the length of a solve (sizes, partitioning, which matvec and which orthogonalisation run, lazy host reads) is
 * decided once, in DflGmresPlanFill (GmresPlan, solver_private.h); the loop bodies only follow the plan. */
#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "dedflow.h"
#include "dedflow_kernels.h"
#include "host_private.h"
#include "solver_private.h"

/* ============================== work space ============================================== */
/* The Krylov basis and the preconditioned vector live OUTSIDE the device pool, in allocations of their own.  Measured on
 * MI355X (tools/probe_spmv_r2c.py, profiles/r02_spmv_placement.txt): the block-CSR SpMV takes 0.673 ms when its output
 * vector lies in the same 32 GiB pool chunk as the 3.3 GB value array it streams, and 0.570 ms when the output lies in any
 * other allocation (0.554 ms with the store compiled out) -- reads of the value array and writes of y compete when both
 * come from one physical neighbourhood.  DFL_KRYLOV_POOL=1 puts them back into the pool (A/B). */
static int g_ws_pool = -1; /* process default; DflKrylovWorkspaceInPool switches it (developer A/B) */
int DflWsInPool(void) {
    if (g_ws_pool < 0) { const char* e = getenv("DFL_KRYLOV_POOL"); g_ws_pool = (e && atoi(e) == 1) ? 1 : 0; }
    return g_ws_pool;
}
static f64* ws_vec_malloc(ptrdiff_t count) {
    if (DflWsInPool()) return (f64*)CdamMallocDevice(count * SIZE_OF(f64));
    void* p = DflVectorArenaAlloc((size_t)count * sizeof(f64));
    if (!p) HIPGUARD(hipMalloc(&p, (size_t)count * sizeof(f64)));
    HIPGUARD(hipMemsetAsync(p, 0, (size_t)count * sizeof(f64), DflStream()));
    return (f64*)p;
}
void DflKrylovWorkspaceInPool(int on) { g_ws_pool = on ? 1 : 0; } /* takes effect at the next solve of every solver */
void DflWsVecFreeAs(f64* p, int pooled) {
    if (!p) return;
    if (pooled) CdamFreeDevice(p, 0);
    else if (!DflVectorArenaFree(p)) HIPGUARD(hipFree(p));
}

void DflWsFree(KrylovExt* x) {
    DflWsVecFreeAs(x->Q, x->q_pooled); DflWsVecFreeAs(x->Z, x->ws_pooled); CdamFreeDevice(x->H, 0); DflWsVecFreeAs(x->tmp, x->ws_pooled); CdamFreeDevice(x->gv, 0);
    CdamFreeDevice(x->beta, 0); CdamFreeDevice(x->res_hist, 0); CdamFreeDevice(x->nrm_base, 0); CdamFreeDevice(x->work, 0);
    CdamFreeDevice(x->d_flag, 0); CdamFreeDevice(x->hraw, 0); CdamFreeDevice(x->h_unrot, 0); CdamFreeDevice(x->pair_buf, 0);
    x->Q = x->Z = x->H = x->tmp = x->gv = x->beta = x->res_hist = x->nrm = x->nrm_base = x->work = x->hraw = NULL;
    x->h_unrot = x->pair_buf = NULL;
    x->d_flag = NULL;
    x->ws_n = x->ws_maxit = x->ws_hist = 0;
}

/* maxit = basis columns per cycle (the restart length, or max_iter for full GMRES); hist = entries of the residual history */
void DflWsEnsure(KrylovExt* x, index_type n, index_type maxit, index_type ldh, index_type hist) {
    if (x->ws_n == n && x->ws_maxit == maxit && x->ws_hist >= hist && x->ws_pooled == DflWsInPool()) return;
    DflWsFree(x);
    x->ws_pooled = DflWsInPool();
    x->Q = ws_vec_malloc((ptrdiff_t)n * (maxit + 1 + DFL_BASIS_SPARE_COLS)); /* + the interleaved copies z4, z4b */
    x->q_pooled = x->ws_pooled;
    x->H = (f64*)CdamMallocDevice((ptrdiff_t)ldh * maxit * SIZE_OF(f64));
    x->tmp = ws_vec_malloc((ptrdiff_t)n * 2);
    x->gv = (f64*)CdamMallocDevice(2 * (ptrdiff_t)maxit * SIZE_OF(f64));
    x->beta = (f64*)CdamMallocDevice(((ptrdiff_t)maxit + 1) * SIZE_OF(f64));
    x->res_hist = (f64*)CdamMallocDevice(((ptrdiff_t)hist + 1) * SIZE_OF(f64));
    x->ws_hist = hist;
    /* four slots in front of nrm[]: the operand probes of a solve (tail of b, x), so that probes and ||r0|| = nrm[0] reach the
       host in one copy */
    x->nrm_base = (f64*)CdamMallocDevice(((ptrdiff_t)maxit + 2 + 4) * SIZE_OF(f64));
    x->nrm = x->nrm_base + 4;
    if (!x->h_stat) {
        HIPGUARD(hipHostMalloc((void**)&x->h_stat, 16 * sizeof(f64), hipHostMallocDefault));
        HIPGUARD(hipEventCreateWithFlags(&x->ev_stat, hipEventDisableTiming));
    }
    x->assume_valid = FALSE;
    x->work_len = dfl_cgs_work_size(n, maxit + 1) + dfl_reduce_work_size();
    x->work = (f64*)CdamMallocDevice((ptrdiff_t)x->work_len * SIZE_OF(f64));
    x->d_flag = (int*)CdamMallocDevice(16);
    HIPGUARD(hipMemsetAsync(x->d_flag, 0, 16, DflStream()));
    x->hraw = (f64*)CdamMallocDevice((ptrdiff_t)(ldh + 32) * SIZE_OF(f64));
    x->h_unrot = (f64*)CdamMallocDevice((ptrdiff_t)ldh * maxit * SIZE_OF(f64));
    x->pair_buf = (f64*)CdamMallocDevice((8 * (ptrdiff_t)ldh + 96) * SIZE_OF(f64));
    x->ws_n = n; x->ws_maxit = maxit; x->ws_fresh = TRUE;
}

/* ============================== sizes, operands ========================================= */
/* GMRES(m): m basis columns per cycle, then x is updated, the true residual recomputed and the recurrence restarted.  Not in
   the reference (its AMGX sketch asks for gmres_n_restart, krylov.c:409-437); m >= max_iter (default) is the reference's full
   GMRES.  ldh: leading dimension of H */
void DflGmresSizes(const KrylovExt* ex, index_type max_iter, index_type* m_out, index_type* ldh_out) {
    const index_type m = (ex->restart > 0 && ex->restart < max_iter) ? ex->restart : max_iter;
    *m_out = m;
    *ldh_out = CEIL_DIV(m + 1, 32) * 32;
}

/* Where the phi / T tail of a right-hand side begins: 4N for the block-mode (u,p,phi,T) system of 6N rows, n (no tail) for any
   other matrix.  When that tail of b is zero the Krylov vectors live on [0, begin): begin is then the active length (Q5). */
index_type DflKrylovTailBegin(Matrix* A) {
    const index_type n = MatrixNumRow(A);
    const b32 up_system = MatrixFSBlockValues(A) && n == 6 * ((MatrixFS*)A->data)->spy1x1->num_row;
    return up_system ? 4 * (n / 6) : n;
}

/* Two questions about the operands of a solve, answered with one 16-byte read: is the [begin, n) tail of b identically
 * zero (then the Krylov vectors live on [0, begin), Q5), and is the initial guess x identically zero (then r = b exactly
 * and the matvec of krylov.c:114 is skipped -- b - A*0 is b bit for bit)? */
void DflProbeOperands(const f64* b, index_type begin, index_type n, const f64* x, f64* scratch, b32* tail_zero, b32* x_zero) {
    f64 h[2] = {1.0, 1.0};
    hipStream_t s = DflStream();
    if (n > begin) dfl_dnrm2(n - begin, b + begin, scratch, scratch + 8, s);
    else HIPGUARD(hipMemsetAsync(scratch, 0, sizeof(f64), s));
    if (x) dfl_dnrm2(n, x, scratch + 1, scratch + 8, s);
    HIPGUARD(hipMemcpyAsync(h, scratch, (x ? 2 : 1) * sizeof(f64), D2H, s));
    HIPGUARD(hipStreamSynchronize(s));
    *tail_zero = h[0] == 0.0;
    *x_zero = x ? h[1] == 0.0 : FALSE;
}

/* partitioned runs: the local dot products cover ghost rows too, so those must be zero in every Krylov vector (SpMV and
 * the PC write owned rows only); enforced here for the residual instead of relying on the caller */
void DflZeroGhostRows(const KrylovExt* ex, Matrix* A, f64* v, index_type na) {
    if (!ex->has_comm || !MatrixFSBlockValues(A)) return;
    const index_type N = ((MatrixFS*)A->data)->spy1x1->num_row, no = ex->comm.num_owned_node;
    hipStream_t s = DflStream();
    if (no >= N || no < 0) return;
    HIPGUARD(hipMemsetAsync(v + (size_t)no * 3, 0, (size_t)(N - no) * 3 * sizeof(f64), s));
    for (index_type sec = 3; sec < 6 && (size_t)(sec + 1) * (size_t)N <= (size_t)na; ++sec)
        HIPGUARD(hipMemsetAsync(v + (size_t)sec * N + no, 0, (size_t)(N - no) * sizeof(f64), s));
}

/* ============================== preconditioner application ================================ */
/* z = M^{-1} (w / *d_nrm), w <- w / *d_nrm   (d_nrm == NULL: no scaling)
 * z4 != NULL: the application may ALSO leave z interleaved ([node][4], owned rows) for the matvec that follows
 * (DflMatrixFSMatVecX4Range); returns TRUE when it did -- the Jacobi tree writes it from registers -- FALSE when the caller has
 * to make the copy itself (dfl_interleave4) */
b32 DflPcApplyFusedX4(PC* pc, index_type na, f64* w, const f64* d_nrm, f64* z, f64* z4) {
    const f64 *d33, *d1;
    index_type N, nrows;
    hipStream_t s = DflStream();
    if (DflPcJacobiTreeData(pc, &d33, &d1, &N, &nrows)) {
        if (z4) {
            /* z == NULL (the caller reads nothing but the interleaved copy; vectors of 4N only): no reference-layout store */
            ASSERT(z || na == 4 * N);
            dfl_pc_jacobi_apply_scaled_rows_x4(nrows, N, na, d33, d1, w, d_nrm, w, z, z4, s);
            return TRUE;
        }
        if (d_nrm) dfl_pc_jacobi_apply_scaled_rows(nrows, N, na, d33, d1, w, d_nrm, w, z, s);
        else dfl_pc_jacobi_apply_rows(nrows, N, na, d33, d1, w, z, s);
        return FALSE;
    }
    if (d_nrm) dfl_dscal_inv_dev(na, d_nrm, w, s);
    if (pc && pc->type == PC_DECOMPOSITION) {
        /* a tree with AMG on A11: the sections inside the active length only (phi / T lie beyond [0,4N) when b's tail is 0) */
        PCDecomposition* d = (PCDecomposition*)pc->data;
        if (d->n_sec == 4 && d->pc[1] && d->pc[1]->type == PC_AMGX) {
            for (index_type i = 0; i < d->n_sec; ++i)
                if (d->offset[i] < na) PCApply(d->pc[i], w + d->offset[i], z + d->offset[i]);
            return FALSE;
        }
    }
    if (pc && pc->type == PC_ILU0) PCDILUSetActiveLength(pc, na);
    if (pc && pc->type == PC_TWOLEVEL) PCTwoLevelSetActiveLength(pc, na);
    if (pc) PCApply(pc, w, z);
    else dfl_dcopy(na, w, z, s);
    return FALSE;
}
void DflPcApplyFused(PC* pc, index_type na, f64* w, const f64* d_nrm, f64* z) { (void)DflPcApplyFusedX4(pc, na, w, d_nrm, z, NULL); }

/* ============================== the plan of a solve ======================================= */
/* Environment switches of the GMRES paths, read here and nowhere else.  Cached for the process: DFL_SPMV_X4=0 (the
   reference-layout gathers, A/B), DFL_SPMV_X4_MIN (smallest matrix, in nodes, that takes the interleaved path; tests set 1).
   Read at every solve (A/B): eager host reads, boundary rows on the library stream, three launches per fused-norm step,
   DFL_GMRES_RAW_BASIS=0 (one GPU: the normalised basis and the separate Jacobi pass instead of GMRES_STEP_RAW_BASIS),
   DFL_GMRES_BLOCK=1..4 (the most iterations the raw-basis step takes per pass over the basis, default 4), DFL_GMRES_TWO_STEP=0
   (the same as block 1: one iteration at a time), DFL_GMRES_FOLD_PC=0 (pairs and blocks: a Jacobi launch between two products
   instead of the product that writes M^-1 of its own output), DFL_GMRES_FUSE_FIXUP=0 (blocks of three and four: the update and
   the fix-up as two passes with the Gram matrix measured between them, instead of the one pass of dfl_cgs_update_fixup_block) */
typedef struct GmresEnv { b32 x4; index_type x4_min; b32 eager_sync, no_side_rows, no_fused_update_pc, raw_basis; int block; b32 fold_pc, fuse_fixup; } GmresEnv;
static GmresEnv gmres_env(void) {
    static int x4 = -1, x4_min = 4096;
    if (x4 < 0) {
        const char *off = getenv("DFL_SPMV_X4"), *min = getenv("DFL_SPMV_X4_MIN");
        if (min) x4_min = atoi(min);
        x4 = !(off && atoi(off) == 0);
    }
    const char *raw = getenv("DFL_GMRES_RAW_BASIS"), *two = getenv("DFL_GMRES_TWO_STEP"), *blk = getenv("DFL_GMRES_BLOCK");
    int block = 4;
    if (blk) {
        /* a value that is no number from 1 to 4 is clamped into that range (no number at all: the default) and named once, so
           that an A/B run with a typo does not measure something else unnoticed */
        static b32 warned = FALSE;
        char* end = NULL;
        const long v = strtol(blk, &end, 10);
        const b32 number = end != blk && *end == '\0';
        block = !number ? 4 : v < 1 ? 1 : v > 4 ? 4 : (int)v;
        if ((!number || v != block) && !warned) {
            fprintf(stderr, "[krylov] DFL_GMRES_BLOCK=%s is not one of 1, 2, 3, 4: using %d\n", blk, block);
            warned = TRUE;
        }
    }
    if (two && atoi(two) == 0) block = 1;
    const char *fold = getenv("DFL_GMRES_FOLD_PC"), *fuse = getenv("DFL_GMRES_FUSE_FIXUP");
    const GmresEnv e = {x4, x4_min, getenv("DFL_KRYLOV_EAGER_SYNC") != NULL, getenv("DFL_NO_SIDE_BOUNDARY_ROWS") != NULL,
                        getenv("DFL_NO_FUSED_UPDATE_PC") != NULL, !(raw && atoi(raw) == 0), block, !(fold && atoi(fold) == 0),
                        !(fuse && atoi(fuse) == 0)};
    return e;
}

static b32 gmres_lazy(const KrylovExt* ex, index_type max_iter) {
    index_type m, ldh;
    DflGmresSizes(ex, max_iter, &m, &ldh);
    return !ex->verbose && m >= max_iter && !gmres_env().eager_sync; /* quiet solver, no restarts (host reads, below) */
}

/* na: active length; ex->Q: the basis the solve will use (z4 is its spare column).  pipelined: the plan of gmres_pipelined --
   reference-layout matvec, eager reads, no FGMRES basis; its orthogonalisation is its own */
void DflGmresPlanFill(GmresPlan* p, const KrylovExt* ex, index_type max_iter, Matrix* A, PC* pc, index_type na, b32 pipelined) {
    const GmresEnv env = gmres_env();
    const DflComm* c = &ex->comm;
    memset(p, 0, sizeof *p);
    p->n = MatrixNumRow(A); p->na = na; p->maxit = max_iter;
    DflGmresSizes(ex, max_iter, &p->m, &p->ldh);
    p->dist = ex->has_comm;
    p->n_interior = p->dist ? c->num_interior_node : 0;
    p->owned_rows = MatrixFSOwnedRows(A);
    p->split_rows = p->dist && p->n_interior > 0 && MatrixFSBlockValues(A) && p->n_interior <= p->owned_rows;
    p->side = (p->split_rows && c->halo_begin && c->halo_stream && !env.no_side_rows) ? c->halo_stream(c->ctx) : NULL;
    if (pipelined) return; /* x4 none, no fused step, eager reads */
    p->lazy = gmres_lazy(ex, max_iter);
    p->Zb = ex->flexible ? ex->Z : NULL;
    const b32 tree_4n = DflPcJacobiTreeData(pc, &p->d33, &p->d1, &p->N, &p->rows) && na == 4 * p->N;
    /* fused norm + Jacobi tree on the (u,p) rows (partitioned runs of <= 500k owned nodes; the small last-level solver of
       PC_TWOLEVEL, which is bound by launch latency): update, Givens step and the next step's preconditioner application in
       one launch (csrc/k_cgs.hip, cgs_update_pc_kernel) */
    const b32 fuse_pc = ex->fused_norm && !ex->flexible && p->m + 2 <= 1024 && !env.no_fused_update_pc && tree_4n && p->rows > 0 &&
                        p->rows <= 500000; /* measured: 38 us against 31 + 7 + 6 us for the three kernels at 227k owned nodes, but
                                              274 us against 192 + 46 + 10 us at 1.73M (the node-per-thread mapping streams the
                                              basis with 8-byte loads): large ranks keep the three launches */
    p->step = fuse_pc ? GMRES_STEP_FUSED_UPDATE_PC : ex->fused_norm ? GMRES_STEP_FUSED_NORM
              : p->dist ? GMRES_STEP_TWO_REDUCTIONS : GMRES_STEP_REFERENCE;
    /* the matvec gathers from an interleaved copy of z: one GPU, or partitioned with split rows (owned part of the copy from the
       producer of z, ghost part behind the unpack) */
    p->x4_N = MatrixFSBlockValues(A) ? ((MatrixFS*)A->data)->spy1x1->num_row : 0;
    p->x4_owned = p->dist ? p->owned_rows : p->x4_N;
    if (env.x4 && p->x4_N >= env.x4_min && na >= 4 * p->x4_N) {
        if (!p->dist && !fuse_pc && p->owned_rows == p->x4_N) p->x4 = GMRES_X4_SINGLE;
        if (p->dist && p->split_rows) p->x4 = GMRES_X4_PARTITIONED;
    }
    if (p->x4 != GMRES_X4_NONE) p->z4 = ex->Q + (size_t)na * (size_t)(p->m + 1); /* the spare column of the basis block */
    /* with the Jacobi tree on 4N-vectors nothing reads z in the reference layout (tmp is rewritten before its next use): the
       kernel then stores the interleaved copy only -- 32 B per node and iteration less to write.  FGMRES keeps every z */
    p->x4_skip_z = p->x4 == GMRES_X4_SINGLE && tree_4n && p->N == p->x4_N && !p->Zb;
    /* one GPU, Jacobi tree, interleaved matvec input: the basis stays unnormalised (column k = r_k, nrm[k] = ||r_k||), the update
       kernel applies M^-1 to the column it has just formed and the matvec divides by nrm[k] -- the separate Jacobi pass, which
       read the new column back only to scale it, is gone (csrc/k_cgs.hip, cgs_update_jacobi_kernel).  Restarts, lazy or eager
       reads and the check interval have no say here: the arithmetic of a solve does not depend on them */
    if (p->step == GMRES_STEP_REFERENCE && p->x4_skip_z && p->rows == p->N && env.raw_basis) {
        p->step = GMRES_STEP_RAW_BASIS;
        p->block = env.block;
        /* between two products of a pair or block the Jacobi launch only read the product just stored and the inverse blocks to
           write z4: the row group that forms a row of the product holds its four components and has streamed the row's diagonal
           block, and writes z4 itself -- into the other of two interleaved copies, as rows of the same launch still gather from
           the one it reads */
        p->fold_pc = env.fold_pc && p->block > 1 && ((MatrixFS*)A->data)->spy1x1->diag_pos != NULL;
        if (p->fold_pc) p->z4b = p->z4 + (size_t)na;
        p->fuse_fixup = env.fuse_fixup && p->block >= 3;
    }
}

/* ============================== operator, residual, Arnoldi step =========================== */
static void matvec_rows(const GmresPlan* p, Matrix* A, f64* z, f64* y, index_type row0, index_type row1) {
    if (p->x4 == GMRES_X4_PARTITIONED) DflMatrixFSMatVecX4Range(A, p->z4, y, row0, row1);
    else MatrixFSMatVecRange(A, z, y, row0, row1);
}

/* z = M^-1 (q / *d_nrm) (d_nrm == NULL: q as it is); halo of z; y = A z  (owned rows).  q is left normalised.  z_ready: `z`
   already holds M^-1 q, written by the fused step (GMRES_STEP_FUSED_UPDATE_PC; GMRES_STEP_RAW_BASIS: the interleaved copy
   holds M^-1 of the raw column) */
static void gmres_apply_operator(const GmresPlan* p, KrylovExt* ex, Matrix* A, PC* pc, f64* q, const f64* d_nrm, f64* z, b32 z_ready,
                                 f64* y) {
    const DflComm* c = &ex->comm;
    hipStream_t s = DflStream();
    b32 wrote = FALSE;
    /* the block-mode matrix stores the (u,p) rows only and its matvec writes nothing beyond them.  With a non-zero phi / T tail of
       b the vectors cover [0, 6N): rows [4N, na) of A z are the zero of the reference's empty blocks, not what an earlier solve
       or restart cycle left in this column (a second solve on the same Krylov object gave another history before this) */
    const index_type up_rows = MatrixFSBlockValues(A) ? 4 * ((MatrixFS*)A->data)->spy1x1->num_row : p->na;
    if (p->na > up_rows) HIPGUARD(hipMemsetAsync(y + up_rows, 0, (size_t)(p->na - up_rows) * sizeof(f64), s));
    if (p->step == GMRES_STEP_RAW_BASIS) {
        /* q = r_k is left as it is; z4 = M^-1 r_k (column 0: made here; later columns: the update kernel has left it),
           y = (A z4) / nrm[k] */
        if (!z_ready) DFL_TIMED(DFL_TAG_PC, (void)DflPcApplyFusedX4(pc, p->na, q, NULL, NULL, p->z4));
        DFL_TIMED(DFL_TAG_SPMV, DflMatrixFSMatVecX4RangeScaled(A, p->z4, d_nrm, y, 0, p->x4_N));
        return;
    }
    if (p->x4 == GMRES_X4_SINGLE) {
        /* one GPU: one 16-byte load per lane and nonzero instead of two 8-byte loads (0.50 against 0.57 ms at 10M tets); the
           Jacobi tree writes the interleaved copy from registers, any other preconditioner is followed by one interleave pass */
        DFL_TIMED(DFL_TAG_PC, wrote = DflPcApplyFusedX4(pc, p->na, q, d_nrm, p->x4_skip_z ? NULL : z, p->z4));
        if (!wrote) dfl_interleave4(0, p->x4_N, p->x4_N, z, p->z4, s);
        DFL_TIMED(DFL_TAG_SPMV, DflMatrixFSMatVecX4Range(A, p->z4, y, 0, p->x4_N));
        return;
    }
    const b32 x4 = p->x4 == GMRES_X4_PARTITIONED;
    if (!z_ready) {
        DFL_TIMED(DFL_TAG_PC, wrote = DflPcApplyFusedX4(pc, p->na, q, d_nrm, z, p->z4));
        if (x4 && !wrote) dfl_interleave4(0, p->x4_owned, p->x4_N, z, p->z4, s);
    }
    if (!p->split_rows) {
        if (p->dist) c->halo_exchange(c->ctx, z);
        DFL_TIMED(DFL_TAG_SPMV, MatrixMatVec(A, z, y));
        return;
    }
    /* interior rows read no ghost entry: they run while the halo is in flight.  x4: the rows gather from the interleaved copy
       -- its owned part was written by the producer of z (before halo_begin), its ghost part is made behind the unpack, on the
       stream the boundary rows run on */
    if (c->halo_begin) c->halo_begin(c->ctx, z);
    else c->halo_exchange(c->ctx, z);
    DFL_TIMED(DFL_TAG_SPMV, matvec_rows(p, A, z, y, 0, p->n_interior));
    if (p->side) {
        /* the boundary rows go behind the unpack on the exchange's own stream: they write rows the interior launch does not
           touch and read ghost entries it does not read, so the two overlap; halo_end joins both */
        DflSetStream(p->side);
        if (x4) dfl_interleave4(p->x4_owned, p->x4_N, p->x4_N, z, p->z4, p->side);
        matvec_rows(p, A, z, y, p->n_interior, p->owned_rows);
        DflSetStream(s);
        c->halo_end(c->ctx, z);
    } else {
        if (c->halo_begin) c->halo_end(c->ctx, z);
        if (x4) dfl_interleave4(p->x4_owned, p->x4_N, p->x4_N, z, p->z4, s);
        DFL_TIMED(DFL_TAG_SPMV, matvec_rows(p, A, z, y, p->n_interior, p->owned_rows));
    }
}

static void gmres_clear_recurrence(const GmresPlan* p, KrylovExt* ex) { /* H, beta, Givens coefficients of a cycle */
    hipStream_t s = DflStream();
    HIPGUARD(hipMemsetAsync(ex->H, 0, (size_t)p->ldh * p->m * sizeof(f64), s));
    HIPGUARD(hipMemsetAsync(ex->beta, 0, ((size_t)p->m + 1) * sizeof(f64), s));
    HIPGUARD(hipMemsetAsync(ex->gv, 0, 2 * (size_t)p->m * sizeof(f64), s));
}

/* r = b - A x (krylov.c:112-116; skip_matvec: x is zero, r = b bit for bit), ghost rows zeroed, nrm[0] = beta[0] = ||r|| */
static void gmres_initial_residual(const GmresPlan* p, KrylovExt* ex, Matrix* A, f64* x, const f64* b, f64* r, b32 skip_matvec) {
    hipStream_t s = DflStream();
    dfl_dcopy(p->na, b, r, s);
    if (p->dist) ex->comm.halo_exchange(ex->comm.ctx, x);
    if (!skip_matvec) MatrixAMVPBY(A, -1.0, x, 1.0, r);
    if (p->dist) {
        DflZeroGhostRows(ex, A, r, p->na);
        dfl_ddot(p->na, r, r, ex->nrm, ex->work, s);
        ex->comm.allreduce_sum(ex->comm.ctx, ex->nrm, 1);
        dfl_dsqrt_dev(ex->nrm, s);
    } else dfl_dnrm2(p->na, r, ex->nrm, ex->work, s);
    HIPGUARD(hipMemcpyAsync(ex->beta, ex->nrm, sizeof(f64), D2D, s));
}

/* Classical Gram-Schmidt of w = Q[:,iter+1] against Q[:,0..iter], then the Givens rotations and the residual recurrence, all on
   the device: column iter of H, beta[iter+1], res_hist[iter]; nrm[iter+1] = the norm Q[:,iter+1] still has to be divided by.
   last: no Arnoldi step follows in this cycle (the raw-basis step then leaves out M^-1 of the new column) */
static void gmres_orthogonalise(const GmresPlan* p, KrylovExt* ex, index_type iter, f64* res_hist, b32 last) {
    const index_type na = p->na, ldh = p->ldh;
    const DflComm* c = &ex->comm;
    hipStream_t s = DflStream();
    f64 *const Q = ex->Q, *const H = ex->H, *const w = Q + (size_t)(iter + 1) * (size_t)na, *const h = H + (size_t)iter * (size_t)ldh;
    f64* const nrm = ex->nrm + iter + 1;
    switch (p->step) {
    case GMRES_STEP_FUSED_UPDATE_PC: /* ... and tmp = M^-1 of the normalised column, for the next matvec (z_ready) */
        DFL_TIMED(DFL_TAG_CGS_DOTS, dfl_cgs_dots(na, iter + 2, Q, na, w, ex->hraw, ex->work, s));
        if (p->dist) c->allreduce_sum(c->ctx, ex->hraw, iter + 2);
        DFL_TIMED(DFL_TAG_CGS_UPDATE,
                  dfl_cgs_update_pc_givens_x4(p->rows, p->N, iter + 1, Q, na, ex->hraw, w, p->d33, p->d1, ex->tmp, p->z4, iter, H, ldh,
                                              ex->gv, ex->beta, res_hist, nrm, ex->d_flag, s));
        break;
    case GMRES_STEP_FUSED_NORM:
        /* w itself is column iter+1 of Q: one extra "column" of the dots gives w.w, one all-reduce carries h and w.w */
        DFL_TIMED(DFL_TAG_CGS_DOTS, dfl_cgs_dots(na, iter + 2, Q, na, w, h, ex->work, s));
        if (p->dist) c->allreduce_sum(c->ctx, h, iter + 2);
        DFL_TIMED(DFL_TAG_CGS_UPDATE, dfl_cgs_update(na, iter + 1, Q, na, h, w, NULL, 0, ex->work, s));
        dfl_gmres_givens_pythagoras(iter, nrm, H, ldh, ex->gv, ex->beta, res_hist, ex->d_flag, s);
        break;
    case GMRES_STEP_TWO_REDUCTIONS:
        DFL_TIMED(DFL_TAG_CGS_DOTS, dfl_cgs_dots(na, iter + 1, Q, na, w, h, ex->work, s));
        c->allreduce_sum(c->ctx, h, iter + 1);
        DFL_TIMED(DFL_TAG_CGS_UPDATE, dfl_cgs_update(na, iter + 1, Q, na, h, w, nrm, 0, ex->work, s));
        c->allreduce_sum(c->ctx, nrm, 1);
        dfl_gmres_givens_sq(iter, nrm, H, ldh, ex->gv, ex->beta, res_hist, s);
        break;
    case GMRES_STEP_RAW_BASIS:
        /* columns 0..iter are r_j = nrm[j] q_j: h_j = <r_j, w> / nrm[j] into H, hraw[j] = h_j / nrm[j] multiplies r_j */
        DFL_TIMED(DFL_TAG_CGS_DOTS, dfl_cgs_dots_raw(na, iter + 1, Q, na, w, ex->nrm, h, ex->hraw, ex->work, s));
        /* (solves with pairs or blocks: a later one reads this column un-rotated) */
        DFL_TIMED(DFL_TAG_CGS_UPDATE,
                  dfl_cgs_update_jacobi_givens_keep(p->N, iter + 1, Q, na, ex->hraw, w, p->d33, p->d1, last ? NULL : p->z4, nrm,
                                                    ex->work, iter, H, ldh, ex->gv, ex->beta, res_hist,
                                                    p->block > 1 ? ex->h_unrot + (size_t)iter * (size_t)ldh : NULL, s));
        break;
    case GMRES_STEP_REFERENCE:
        DFL_TIMED(DFL_TAG_CGS_DOTS, dfl_cgs_dots(na, iter + 1, Q, na, w, h, ex->work, s));
        DFL_TIMED(DFL_TAG_CGS_UPDATE, dfl_cgs_update_givens(na, iter + 1, Q, na, h, w, nrm, ex->work, iter, H, ldh, ex->gv, ex->beta,
                                                            res_hist, s));
        break;
    }
}

/* The sb products of a pair or block that starts at column k: p_0 = (A z4) / nrm[k] into p0 (column k+1), p_i = A M^-1 p_{i-1}
   into column k+1+i.  At entry z4 (buffer 0) holds M^-1 r_k (k == 0: made here).  fold_pc: product i gathers from buffer i % 2 and,
   unless it is the last, writes M^-1 p_i into buffer (i + 1) % 2 itself; the last one is the plain kernel -- its successor's z4
   comes from the fix-up, which writes buffer 0 as the k == 0 application does.  Otherwise a Jacobi launch between two products */
static void gmres_products(const GmresPlan* p, KrylovExt* ex, Matrix* A, PC* pc, index_type k, int sb, f64* p0) {
    const index_type na = p->na;
    f64* const zb[2] = {p->z4, p->z4b};
    if (k == 0) DFL_TIMED(DFL_TAG_PC, (void)DflPcApplyFusedX4(pc, na, ex->Q, NULL, NULL, p->z4));
    for (int i = 0; i < sb; ++i) {
        f64* const y = p0 + (size_t)i * (size_t)na;
        const f64* const d_nrm = i == 0 ? ex->nrm + k : NULL;
        if (p->fold_pc && i + 1 < sb) {
            DFL_TIMED(DFL_TAG_SPMV, DflMatrixFSMatVecX4Pc(A, zb[i % 2], d_nrm, y, zb[(i + 1) % 2]));
            ex->last_folded++;
            continue;
        }
        f64* const src = p->fold_pc ? zb[i % 2] : p->z4;
        if (i > 0 && !p->fold_pc) DFL_TIMED(DFL_TAG_PC, (void)DflPcApplyFusedX4(pc, na, y - (size_t)na, NULL, NULL, p->z4));
        if (d_nrm) DFL_TIMED(DFL_TAG_SPMV, DflMatrixFSMatVecX4RangeScaled(A, src, d_nrm, y, 0, p->x4_N));
        else DFL_TIMED(DFL_TAG_SPMV, DflMatrixFSMatVecX4Range(A, src, y, 0, p->x4_N));
    }
}

/* Iterations k and k+1 of a cycle in one pass over the basis (GmresPlan.block >= 2).  At entry column k holds r_k and, k > 0, z4 holds
   M^-1 r_k.  p1 = B v_k = (A z4) / nrm[k] into column k+1, z4 = M^-1 p1, p2 = B p1 = A z4 into column k+2 -- in exact arithmetic
   the component of p2 orthogonal to v_0..v_{k+1} is a multiple of v_{k+2}, because B v_j lies in span(v_0..v_{j+1}).  One dots
   pass and one update pass over columns 0..k serve both vectors; p1' = r_{k+1}; the fix-up q = p2' - c p1' (one column) leaves
   r_{k+2} = q in column k+2 with z4 = M^-1 q for the step that follows (last: none does).  Columns k and k+1 of H, their Givens
   steps, beta and two entries of the history come from two small kernels (csrc/k_cgs_block.hip, pair_first_kernel and
   pair_second_kernel); nothing waits for the whole grid and no sum is taken atomically */
static void gmres_pair(const GmresPlan* p, KrylovExt* ex, Matrix* A, PC* pc, index_type k, f64* res_hist, b32 last) {
    const index_type na = p->na, ldh = p->ldh;
    hipStream_t s = DflStream();
    f64 *const Q = ex->Q, *const p1 = Q + (size_t)(k + 1) * (size_t)na, *const p2 = Q + (size_t)(k + 2) * (size_t)na;
    f64 *const c1 = ex->pair_buf, *const c2 = c1 + ldh, *const e = c2 + ldh, *const sc = e + ldh;
    f64 *const h1 = ex->H + (size_t)k * (size_t)ldh, *const h1_raw = ex->h_unrot + (size_t)k * (size_t)ldh;
    const int g2 = dfl_cgs_update2_parts(na), g1 = (int)CEIL_DIV(p->N, 256);
    gmres_products(p, ex, A, pc, k, 2, p1);
    DFL_TIMED(DFL_TAG_CGS_DOTS, dfl_cgs_dots2_raw(na, k + 1, Q, na, p1, p2, ex->nrm, h1, h1_raw, c1, e, c2, ex->work, s));
    DFL_TIMED(DFL_TAG_CGS_UPDATE, dfl_cgs_update2(na, k + 1, Q, na, c1, c2, p1, p2, ex->work, s));
    dfl_gmres_pair_first(g2, ex->work, k, ex->nrm, ex->H, ex->h_unrot, ldh, ex->gv, ex->beta, res_hist, sc, s);
    DFL_TIMED(DFL_TAG_CGS_UPDATE, dfl_cgs_update_jacobi(p->N, 1, p1, na, sc, p2, p->d33, p->d1, last ? NULL : p->z4, ex->work, s));
    dfl_gmres_pair_second(g1, ex->work, k, ex->nrm, ex->H, ex->h_unrot, ldh, e, sc, ex->gv, ex->beta, res_hist, ex->d_flag, s);
}

/* Iterations k..k+s-1 of a cycle, s = 3 or 4, in one pass over the basis: gmres_pair generalised.  p_0 = B v_k = (A z4) / nrm[k]
   into column k+1, then z4 = M^-1 p_{i-1}, p_i = A z4 into column k+1+i.  One dots pass and one update pass over columns 0..k
   serve all s vectors (dfl_cgs_dots_block, dfl_cgs_update_block); the updated p_i' span v_{k+1}..v_{k+s} and are orthogonalised
   among themselves through their s x s Gram matrix, whose partials the update leaves: dfl_gmres_block_first forms the unit
   triangular C, one pass over the s columns writes q_i = sum_{l<=i} C[i,l] p_l' = r_{k+1+i} in place (dfl_cgs_fixup_block) with
   z4 = M^-1 q_{s-1} for the step that follows (last: none does), dfl_gmres_block_second measures the norms and computes columns
   k+1..k+s-1 of H.  Nothing waits for the whole grid and no sum is taken atomically */
static void gmres_block(const GmresPlan* p, KrylovExt* ex, Matrix* A, PC* pc, index_type k, int sb, f64* res_hist, b32 last) {
    const index_type na = p->na, ldh = p->ldh;
    hipStream_t s = DflStream();
    f64 *const Q = ex->Q, *const p0 = Q + (size_t)(k + 1) * (size_t)na;
    f64 *const c = ex->pair_buf, *const e = c + 4 * (size_t)ldh, *const sc = e + 4 * (size_t)ldh;
    f64 *const h = ex->H + (size_t)k * (size_t)ldh, *const h_raw = ex->h_unrot + (size_t)k * (size_t)ldh;
    const int gu = dfl_cgs_update_block_parts(na, sb), gf = (int)CEIL_DIV(p->N, 256);
    gmres_products(p, ex, A, pc, k, sb, p0);
    if (p->fuse_fixup) {
        /* r_j / nu_j are orthonormal, so the Gram matrix of the updated vectors follows from that of the products and the dots
           before the update runs: C is known beforehand, and one pass subtracts the old columns, applies C in its registers and
           stores q_0..q_{s-1} and z4 once -- the p_i' never travel through memory.  C only chooses the basis inside the block; the
           norms and the U[l,i] that go into H are measured on the vectors formed, as is their orthogonality (DFL_GMRES_ORTH_TAU) */
        DFL_TIMED(DFL_TAG_CGS_DOTS, dfl_cgs_dots_block_gram(na, k + 1, sb, Q, na, p0, na, ex->nrm, h, h_raw, e, c, ldh, sc, ex->work, s));
        DFL_TIMED(DFL_TAG_CGS_UPDATE, dfl_cgs_update_fixup_block(p->N, k + 1, sb, Q, na, c, ldh, p0, na, sc, p->d33, p->d1,
                                                                 last ? NULL : p->z4, ex->work, s));
        dfl_gmres_block_fused(gf, ex->work, sb, k, ex->nrm, ex->H, ex->h_unrot, ldh, e, ldh, sc, ex->gv, ex->beta, res_hist, ex->d_flag,
                              DFL_GMRES_ORTH_TAU, s);
        ex->last_fused++;
        return;
    }
    DFL_TIMED(DFL_TAG_CGS_DOTS, dfl_cgs_dots_block(na, k + 1, sb, Q, na, p0, na, ex->nrm, h, h_raw, e, c, ldh, ex->work, s));
    DFL_TIMED(DFL_TAG_CGS_UPDATE, dfl_cgs_update_block(na, k + 1, sb, Q, na, c, ldh, p0, na, ex->work, s));
    dfl_gmres_block_first(gu, ex->work, sb, k, ex->nrm, ex->H, ex->h_unrot, ldh, ex->gv, ex->beta, res_hist, sc, s);
    DFL_TIMED(DFL_TAG_CGS_UPDATE, dfl_cgs_fixup_block(p->N, sb, p0, na, sc, p->d33, p->d1, last ? NULL : p->z4, ex->work, s));
    dfl_gmres_block_second(gf, ex->work, sb, k, ex->nrm, ex->H, ex->h_unrot, ldh, e, ldh, sc, ex->gv, ex->beta, res_hist, ex->d_flag, s);
}

/* H y = beta, x += M^-1 (Q[:,0:iter] y)   (FGMRES: x += Z[:,0:iter] y).  Column `iter` of the basis may still be
   un-normalised, but it is not used; columns < iter are normalised (raw basis: none is, y_j is divided by nrm[j] instead) */
static void gmres_update_solution(const GmresPlan* p, KrylovExt* ex, PC* pc, index_type iter, f64* x) {
    hipStream_t s = DflStream();
    f64* const tmp = ex->tmp;
    dfl_gmres_trsv(iter, ex->H, p->ldh, ex->beta, s);
    if (p->step == GMRES_STEP_RAW_BASIS) dfl_gmres_scale_inv(iter, ex->nrm, ex->beta, s);
    dfl_gemv_n(p->na, iter, p->Zb ? p->Zb : ex->Q, p->na, ex->beta, tmp, s);
    if (p->Zb) { dfl_daxpy(p->na, 1.0, tmp, x, s); return; }
    DflPcApplyFused(pc, p->na, tmp, NULL, tmp + p->n);
    dfl_daxpy(p->na, 1.0, tmp + p->n, x, s);
}

/* ============================== convergence, progress ===================================== */
b32 DflKrylovConverged(const Krylov* ksp, f64 rnrm, f64 rnrm_init) { return rnrm < ksp->atol || rnrm < (rnrm_init + 1e-16) * ksp->rtol; }

/* the reference's progress line (verbose solvers); restart_cycle > 0: the line of a recomputed true residual */
void DflKrylovPrintProgress(const Krylov* ksp, index_type it, f64 rnrm, f64 rnrm_init, index_type restart_cycle) {
    if (!kext(ksp)->verbose) return;
    fprintf(stdout, "%3d) abs = %6.4e (tol = %6.4e) rel = %6.4e (tol = %6.4e)", it, rnrm, ksp->atol,
            it ? rnrm / (rnrm_init + DBL_EPSILON) : 1.0, ksp->rtol);
    if (restart_cycle > 0) fprintf(stdout, " [restart %d]", restart_cycle);
    fputc('\n', stdout);
    if (it && restart_cycle == 0) fflush(stdout);
}

/* ============================== host reads ================================================= */
/* Host reads without idling the GPU ("lazy" mode: quiet solver, no restarts).  The reference synchronises two to three times
 * per iteration.  Read eagerly, a solve still has: operand probe, ||r0||, one read per convergence check, two at the end --
 * each of them a round trip during which the device sits idle (40-120 us; 0.38 ms of a rank's 8 ms step at 8 ranks).  Lazily:
 *   - the operand probe (tail of b zero? x0 zero?) is ASSUMED to answer what it answered in this solver's previous solve;
 *     the probe still runs, asynchronously, and its result travels with ||r0|| in the first host read of the solve.  A wrong
 *     assumption that would change the result (tail not zero after all, x0 not zero after all) is noticed there, before x
 *     has been touched, and the solve is redone with a synchronous probe (gmres_run returns TRUE);
 *   - a convergence check is enqueued as an asynchronous copy behind iteration k and READ after iteration k + 1 has been
 *     enqueued: the device works on k + 1 while the host looks at k.  On convergence iteration k + 1 is simply not counted:
 *     it has written column k + 1 of H, beta[k + 1 ..] and Q[:, k + 2], none of which the update with k + 1 columns reads;
 *   - a check that falls on the last iteration of the loop, the history and the cancellation flag share the one
 *     synchronisation at the end.
 * Verbose solvers print the reference's lines in the reference's order and keep the eager reads; so do restarted solves
 * (their cycle boundaries read the true residual anyway).  DFL_KRYLOV_EAGER_SYNC=1 forces the eager form (A/B). */
typedef struct HostReads {
    b32 tail_zero, x_is_zero; /* the operand probe's answers this solve runs on */
    b32 assumed;              /* ... are last solve's, still to be verified */
    b32 first_read_done;      /* ||r0|| is on the host (and the assumed answers verified) */
    b32 pend;                 /* a convergence check has been enqueued and not been looked at yet */
    b32 pend_first;           /* ... and the first read of the solve travels with it */
    index_type final_check;   /* beta index whose value decides convergence at the end-of-solve synchronisation, or -1 */
    f64 rnrm_init;
} HostReads;

typedef enum { FIRST_READ_GO_ON, FIRST_READ_REDO, FIRST_READ_R0_ZERO } FirstRead;

static f64 read_scalar(const f64* d) {
    f64 h = 0.0;
    HIPGUARD(hipMemcpyAsync(&h, d, sizeof(f64), D2H, DflStream()));
    HIPGUARD(hipStreamSynchronize(DflStream()));
    return h;
}

/* The operand probe of a solve: synchronous, or (lazy, and the previous solve of this solver left its answers) assumed, with
   the probes themselves enqueued into the slots in front of nrm[].  Partitioned runs keep the matvec of r0 whatever x is: every
   rank has to take the same path through the halo exchange */
static void gmres_probe_or_assume(KrylovExt* ex, Matrix* A, const f64* x, const f64* b, b32 lazy, b32 force_probe, HostReads* hr) {
    const index_type n = MatrixNumRow(A), tail_begin = DflKrylovTailBegin(A);
    const f64* xp = ex->has_comm ? NULL : x;
    hipStream_t s = DflStream();
    memset(hr, 0, sizeof *hr);
    hr->first_read_done = !lazy; hr->final_check = -1;
    if (!(lazy && ex->assume_valid && !force_probe)) {
        DflProbeOperands(b, tail_begin, n, xp, ex->work, &hr->tail_zero, &hr->x_is_zero);
        ex->assume_valid = TRUE; ex->assume_tail_zero = hr->tail_zero; ex->assume_x_zero = hr->x_is_zero;
        return;
    }
    hr->tail_zero = ex->assume_tail_zero; hr->x_is_zero = xp ? ex->assume_x_zero : FALSE; hr->assumed = TRUE;
    if (n > tail_begin) dfl_dnrm2(n - tail_begin, b + tail_begin, ex->nrm_base, ex->work, s);
    else HIPGUARD(hipMemsetAsync(ex->nrm_base, 0, sizeof(f64), s));
    if (xp) dfl_dnrm2(n, xp, ex->nrm_base + 1, ex->work, s);
    else HIPGUARD(hipMemsetAsync(ex->nrm_base + 1, 0, sizeof(f64), s));
}

/* The first host read of a lazy solve: probes + ||r0|| (the five doubles in front of / at nrm[0]) are in h_stat -- copy_now:
   fetched here, synchronously, where nothing has been read yet and the host needs ||r0|| before x is first updated.  A wrong
   assumption that matters -> REDO (x is untouched); r0 = 0 -> x already solves the system (krylov.c:130 would normalise by
   zero), the solve is over */
static FirstRead gmres_first_read(KrylovExt* ex, HostReads* hr, b32 copy_now) {
    hipStream_t s = DflStream();
    if (copy_now) {
        HIPGUARD(hipMemcpyAsync(ex->h_stat, ex->nrm_base, 5 * sizeof(f64), D2H, s));
        HIPGUARD(hipStreamSynchronize(s));
    }
    hr->rnrm_init = ex->stats.rnrm_init = ex->h_stat[4];
    hr->first_read_done = TRUE;
    if (hr->assumed) {
        const b32 tz = ex->h_stat[0] == 0.0, xz = ex->has_comm ? FALSE : ex->h_stat[1] == 0.0;
        const b32 wrong = (hr->tail_zero && !tz) || (hr->x_is_zero && !xz);
        ex->assume_tail_zero = tz; ex->assume_x_zero = xz;
        hr->assumed = FALSE;
        if (wrong) { HIPGUARD(hipStreamSynchronize(s)); return FIRST_READ_REDO; }
    }
    if (hr->rnrm_init != 0.0) return FIRST_READ_GO_ON;
    HIPGUARD(hipStreamSynchronize(s));
    ex->stats.converged = TRUE;
    return FIRST_READ_R0_ZERO;
}

/* eager read of ||r0|| = nrm[0] with the reference's line 0; TRUE: r0 = 0, x already solves the system (the reference would
   normalise by zero here, krylov.c:130) */
static b32 gmres_read_r0(const Krylov* ksp, KrylovExt* ex, HostReads* hr) {
    hr->rnrm_init = ex->stats.rnrm_init = read_scalar(ex->nrm);
    DflKrylovPrintProgress(ksp, 0, hr->rnrm_init, hr->rnrm_init, 0);
    if (hr->rnrm_init == 0.0) ex->stats.converged = TRUE;
    return hr->rnrm_init == 0.0;
}

/* The convergence check behind iteration `iter` of the cycle (`total` over all cycles).  Eager: read beta[iter+1] now, print,
   decide.  Lazy: enqueue the copy (the first read of the solve rides along) and look at it one iteration later; a check on the
   last iteration of the loop is left to the end-of-solve synchronisation.  Returns TRUE when the solve has converged */
static b32 gmres_check(const Krylov* ksp, const GmresPlan* p, KrylovExt* ex, HostReads* hr, index_type iter, index_type total) {
    hipStream_t s = DflStream();
    if (!p->lazy) {
        const f64 rnrm = fabs(read_scalar(ex->beta + iter + 1));
        DflKrylovPrintProgress(ksp, total + 1, rnrm, hr->rnrm_init, 0);
        return DflKrylovConverged(ksp, rnrm, hr->rnrm_init);
    }
    if (iter + 1 >= p->m || total + 1 >= p->maxit) { hr->final_check = iter + 1; return FALSE; }
    if (!hr->first_read_done) {
        HIPGUARD(hipMemcpyAsync(ex->h_stat, ex->nrm_base, 5 * sizeof(f64), D2H, s));
        hr->pend_first = TRUE;
    }
    HIPGUARD(hipMemcpyAsync(ex->h_stat + 8, ex->beta + iter + 1, sizeof(f64), D2H, s));
    HIPGUARD(hipEventRecord(ex->ev_stat, s));
    hr->pend = TRUE;
    return FALSE;
}

/* residual history and (fused-norm forms) the cancellation flag to the host: the one synchronisation at the end of a solve */
static void gmres_end_of_solve(KrylovExt* ex, index_type total, b32 read_flag) {
    hipStream_t s = DflStream();
    const index_type nh = total < 512 ? total : 512;
    int flag[2] = {0, 0}; /* [0] cancellation; [1] a fused block whose q_i came out skew (dfl_gmres_block_fused) */
    if (nh) HIPGUARD(hipMemcpyAsync(ex->stats.res_hist, ex->res_hist, sizeof(f64) * (size_t)nh, D2H, s));
    if (read_flag) {
        HIPGUARD(hipMemcpyAsync(flag, ex->d_flag, sizeof flag, D2H, s));
        HIPGUARD(hipMemsetAsync(ex->d_flag, 0, sizeof flag, s));
    }
    HIPGUARD(hipStreamSynchronize(s));
    ex->stats.fused_norm_cancelled = (flag[0] != 0 ? 1 : 0) | (flag[1] != 0 ? 2 : 0);
}

/* ============================== drivers ==================================================== */
#define COL(base, c) ((base) + (size_t)(c) * (size_t)na) /* column c of a basis with leading dimension na */

/* one solve; TRUE: an assumed probe answer was wrong, nothing has been written to x, run again with force_probe */
static b32 gmres_run(Matrix* A, f64* x, f64* b, Krylov* ksp, b32 force_probe) {
    KrylovExt* ex = kext(ksp);
    PC* pc = (PC*)ksp->pc;
    hipStream_t s = DflStream();
    const index_type n = MatrixNumRow(A), maxit = ksp->max_iter;
    index_type m, ldh;
    DflGmresSizes(ex, maxit, &m, &ldh);
    DflWsEnsure(ex, n, m, ldh, maxit);
    HostReads hr;
    gmres_probe_or_assume(ex, A, x, b, gmres_lazy(ex, maxit), force_probe, &hr);
    const index_type na = hr.tail_zero ? DflKrylovTailBegin(A) : n;
    if (ex->ws_fresh) {
        ex->ws_fresh = FALSE;
        if (!ex->flexible && !ex->no_calibration) ex->Q = DflWsPickBasis(ex, A, pc, ex->Q, maxit, na);
    }
    if (ex->flexible && !ex->Z) ex->Z = ws_vec_malloc((ptrdiff_t)n * m);
    GmresPlan p;
    DflGmresPlanFill(&p, ex, maxit, A, pc, na, FALSE);
    ex->last_step = (int)p.step;
    memset(ex->last_blocks, 0, sizeof ex->last_blocks);
    ex->last_pair_cancelled = 0;
    ex->last_folded = 0;
    ex->last_fused = 0;
    f64 *const Q = ex->Q, *const tmp = ex->tmp;
    b32 converged = FALSE;
    index_type total = 0; /* iterations over all cycles */
    ex->stats.converged = FALSE; ex->stats.iterations = 0;
    for (index_type cycle = 0; !converged && total < maxit; ++cycle) {
        f64* res_hist = ex->res_hist + total; /* history of this cycle */
        index_type iter = 0;
        gmres_clear_recurrence(&p, ex);
        gmres_initial_residual(&p, ex, A, x, b, COL(Q, 0), cycle == 0 && hr.x_is_zero);
        if (cycle > 0) { /* restart: the recomputed true residual decides */
            const f64 rnrm = read_scalar(ex->nrm);
            DflKrylovPrintProgress(ksp, total, rnrm, hr.rnrm_init, cycle);
            if (DflKrylovConverged(ksp, rnrm, hr.rnrm_init)) { converged = TRUE; break; }
        } else if (!p.lazy && gmres_read_r0(ksp, ex, &hr)) return FALSE;
        /* (lazy: ||r0|| reaches the host with the first convergence check, or right before x is first updated) */
        /* the normalisation of Q[:,k] is folded into the preconditioner application that consumes it;
           nrm[k] holds the norm Q[:,k] still has to be divided by */
        while (!converged && iter < m && total < maxit) {
            /* as many iterations at once as fit into the cycle and the iteration cap with no convergence check between them */
            index_type adv = p.block > 1 ? p.block : 1;
            if (adv > m - iter) adv = m - iter;
            if (adv > maxit - total) adv = maxit - total;
            if (adv > ex->check_interval - total % ex->check_interval) adv = ex->check_interval - total % ex->check_interval;
            const b32 last = iter + adv >= m || total + adv >= maxit;
            const int folded_before = ex->last_folded, fused_before = ex->last_fused;
            if (adv > 2) gmres_block(&p, ex, A, pc, iter, (int)adv, res_hist, last);
            else if (adv == 2) gmres_pair(&p, ex, A, pc, iter, res_hist, last);
            else {
                /* 2.0 z = inv(P) Q[:,iter] (FGMRES keeps every z; the fused step has left it in tmp)   2.2 Q[:,iter+1] = A z */
                gmres_apply_operator(&p, ex, A, pc, COL(Q, iter), ex->nrm + iter, p.Zb ? COL(p.Zb, iter) : tmp,
                                     iter > 0 && (p.step == GMRES_STEP_FUSED_UPDATE_PC || p.step == GMRES_STEP_RAW_BASIS),
                                     COL(Q, iter + 1));
                /* 3. classical Gram-Schmidt   4. Givens rotations + residual recurrence */
                gmres_orthogonalise(&p, ex, iter, res_hist, last);
            }
            if (hr.pend) {
                /* the check enqueued behind the PREVIOUS step: the device has the step just enqueued to work on while the host
                   waits for the 8 (+ 40) bytes */
                HIPGUARD(hipEventSynchronize(ex->ev_stat));
                hr.pend = FALSE;
                if (hr.pend_first) {
                    hr.pend_first = FALSE;
                    const FirstRead fr = gmres_first_read(ex, &hr, FALSE);
                    if (fr != FIRST_READ_GO_ON) return fr == FIRST_READ_REDO;
                }
                /* converged: the step enqueued meanwhile (one iteration or several) is not counted */
                if (DflKrylovConverged(ksp, fabs(ex->h_stat[8]), hr.rnrm_init)) {
                    ex->last_folded = folded_before;
                    ex->last_fused = fused_before;
                    converged = TRUE;
                    break;
                }
            }
            if ((total + adv) % ex->check_interval == 0) converged = gmres_check(ksp, &p, ex, &hr, iter + adv - 1, total + adv - 1);
            iter += adv; total += adv;
            ex->last_blocks[adv]++;
        }
        /* (no check is pending here: one on the last iteration of the loop went to final_check instead) */
        if (!hr.first_read_done) { /* a solve shorter than its check interval: nothing has been read yet */
            const FirstRead fr = gmres_first_read(ex, &hr, TRUE);
            if (fr != FIRST_READ_GO_ON) return fr == FIRST_READ_REDO;
        }
        if (iter) {
            /* 5.1 H y = beta   5.2 tmp = Q[:,0:iter] y   5.3 precondition   5.4 x += .   (final check: before trsv overwrites beta) */
            if (hr.final_check >= 0) HIPGUARD(hipMemcpyAsync(ex->h_stat + 9, ex->beta + hr.final_check, sizeof(f64), D2H, s));
            gmres_update_solution(&p, ex, pc, iter, x);
        }
    }
    gmres_end_of_solve(ex, total, ex->fused_norm || p.block > 1);
    if (p.block > 1) { ex->last_pair_cancelled = ex->stats.fused_norm_cancelled; ex->stats.fused_norm_cancelled = FALSE; }
    if (hr.final_check >= 0 && !converged) converged = DflKrylovConverged(ksp, fabs(ex->h_stat[9]), hr.rnrm_init);
    ex->stats.iterations = total; ex->stats.converged = converged;
    return FALSE;
}

/* p(1)-pipelined GMRES (KrylovSetPipelined; off by default; build-defined -- the reference has no multi-GPU path and its
 * AMGX sketch, krylov.c:409-437, no pipelining).  After Ghysels, Ashby, Meerbergen, Vanroose (SIAM J. Sci. Comput. 35, 2013):
 * with B = A M^-1 and the auxiliary basis z_{j+1} = B v_j kept next to V, the product the NEXT Arnoldi step needs follows
 * from one applied to the UN-orthogonalised vector,
 *     B v_{i+1} = ( B z_{i+1} - sum_j h_{j,i} z_{j+1} ) / h_{i+1,i},
 * so the matvec u = B z_{i+1} (preconditioner, halo exchange, SpMV) runs WHILE the one reduction of the step -- the CGS
 * coefficients <z_{i+1}, v_j> together with <z_{i+1}, z_{i+1}>; h_{i+1,i} from the Pythagorean identity as in the fused-norm
 * option -- crosses the ranks: the all-reduce latency (the exposed 20-30 us per iteration of an 8-rank step) hides behind
 * 80+ us of matvec.  The dots and the all-reduce go to a stream of their own when the communicator is stream-ordered (the
 * C-level RCCL one: it exposes halo_stream); with host-side communicators (the torch.distributed callbacks of the gloo
 * tests) everything stays on the library stream: same arithmetic, no overlap.
 * Price: a second basis (memory x2), a third pass over a basis per step (+50 % CGS traffic), one wasted matvec at the end,
 * and the numerics of the z-recurrence plus the Pythagorean norm (cancellation flagged in KrylovStats.fused_norm_cancelled):
 * the residual history follows the reference's to ~1e-8 r0 over 40 steps on the test systems, not to 1e-10.  Fixed
 * (non-flexible) preconditioners only, no restarts; convergence is tested every check interval with an eager read. */
static void gmres_pipelined(Matrix* A, f64* x, f64* b, Krylov* ksp) {
    KrylovExt* ex = kext(ksp);
    PC* pc = (PC*)ksp->pc;
    hipStream_t s = DflStream();
    const index_type n = MatrixNumRow(A), maxit = ksp->max_iter, tail_begin = DflKrylovTailBegin(A);
    index_type m, ldh; /* m == maxit: GMRESSolvePrivate sends restarted solves to gmres_run */
    DflGmresSizes(ex, maxit, &m, &ldh);
    DflWsEnsure(ex, n, m, ldh, maxit);
    ex->ws_fresh = FALSE; /* no placement calibration for this form */
    b32 tail_zero = FALSE, unused = FALSE;
    DflProbeOperands(b, tail_begin, n, NULL, ex->work, &tail_zero, &unused);
    const index_type na = tail_zero ? tail_begin : n;
    if (!ex->Zp || ex->zp_n != n || ex->zp_m != m) {
        DflWsVecFreeAs(ex->Zp, ex->zp_pooled);
        ex->zp_pooled = DflWsInPool();
        ex->Zp = ws_vec_malloc((ptrdiff_t)n * (m + 2));
        ex->zp_n = n; ex->zp_m = m;
    }
    GmresPlan p;
    DflGmresPlanFill(&p, ex, maxit, A, pc, na, TRUE);
    const b32 own_stream = p.dist && ex->comm.halo_stream && ex->comm.halo_stream(ex->comm.ctx) != NULL;
    if (own_stream && !ex->red_stream) {
        ex->red_stream = DflPickConcurrentStream(s); /* a stream that really overlaps the library stream (host/comm_rccl.c) */
        HIPGUARD(hipEventCreateWithFlags(&ex->ev_w, hipEventDisableTiming));
        HIPGUARD(hipEventCreateWithFlags(&ex->ev_h, hipEventDisableTiming));
    }
    hipStream_t rs = own_stream ? ex->red_stream : s;
    f64 *const V = ex->Q, *const Z = ex->Zp, *const tmp = ex->tmp;
    HostReads hr = {.first_read_done = TRUE, .final_check = -1};
    ex->stats.converged = FALSE; ex->stats.iterations = 0;
    gmres_clear_recurrence(&p, ex);
    /* r0 = b - A x, v_0 = r0 / ||r0||, z_1 = B v_0 */
    gmres_initial_residual(&p, ex, A, x, b, COL(V, 0), FALSE);
    if (gmres_read_r0(ksp, ex, &hr)) return;
    dfl_dscal_inv_dev(na, ex->nrm, COL(V, 0), s);
    gmres_apply_operator(&p, ex, A, pc, COL(V, 0), NULL, tmp, FALSE, COL(Z, 1));

    b32 converged = FALSE;
    index_type iter = 0;
    while (!converged && iter < m) {
        const b32 last = iter + 1 >= m;
        f64* const h = ex->H + (size_t)iter * (size_t)ldh;
        /* w = z_{iter+1}, kept in column iter+1 of V as in the reference's loop: the dots then give <w, w> with the h_j */
        dfl_dcopy(na, COL(Z, iter + 1), COL(V, iter + 1), s);
        if (own_stream) {
            HIPGUARD(hipEventRecord(ex->ev_w, s));
            HIPGUARD(hipStreamWaitEvent(rs, ex->ev_w, 0));
        }
        /* the reduction of this step, on its own stream where the communicator allows */
        dfl_cgs_dots(na, iter + 2, V, na, COL(V, iter + 1), h, ex->work, rs);
        if (p.dist) {
            if (own_stream) DflSetStream(rs);
            ex->comm.allreduce_sum(ex->comm.ctx, h, iter + 2);
            if (own_stream) DflSetStream(s);
        }
        if (own_stream) HIPGUARD(hipEventRecord(ex->ev_h, rs));
        /* ... and the matvec of the NEXT step meanwhile: u = B z_{iter+1} (not needed after the last column; ghost rows of Z
           stay zero: nothing ever writes them) */
        if (!last) gmres_apply_operator(&p, ex, A, pc, COL(Z, iter + 1), NULL, tmp, FALSE, COL(Z, iter + 2));
        if (own_stream) HIPGUARD(hipStreamWaitEvent(s, ex->ev_h, 0));
        /* v_{iter+1} = w - V h,  z_{iter+2} = u - Z h  (raw column), then the norm from w.w - sum h^2 + the Givens step */
        DFL_TIMED(DFL_TAG_CGS_UPDATE, dfl_cgs_update(na, iter + 1, V, na, h, COL(V, iter + 1), NULL, 0, ex->work, s));
        if (!last) DFL_TIMED(DFL_TAG_CGS_UPDATE, dfl_cgs_update(na, iter + 1, COL(Z, 1), na, h, COL(Z, iter + 2), NULL, 0, ex->work, s));
        dfl_gmres_givens_pythagoras(iter, ex->nrm + iter + 1, ex->H, ldh, ex->gv, ex->beta, ex->res_hist, ex->d_flag, s);
        dfl_dscal_inv_dev(na, ex->nrm + iter + 1, COL(V, iter + 1), s);
        if (!last) dfl_dscal_inv_dev(na, ex->nrm + iter + 1, COL(Z, iter + 2), s);
        if ((iter + 1) % ex->check_interval == 0) converged = gmres_check(ksp, &p, ex, &hr, iter, iter);
        iter++;
    }
    if (iter) gmres_update_solution(&p, ex, pc, iter, x); /* x += M^-1 V y */
    gmres_end_of_solve(ex, iter, TRUE);
    if (own_stream) HIPGUARD(hipStreamSynchronize(rs));
    ex->stats.iterations = iter; ex->stats.converged = converged;
}

void GMRESSolvePrivate(Matrix* A, f64* x, f64* b, void* ctx) {
    Krylov* ksp = (Krylov*)ctx;
    const KrylovExt* ex = kext(ksp);
    const b32 restarted = ex->restart > 0 && ex->restart < ksp->max_iter;
    if (ex->pipelined && !ex->flexible && !restarted && ksp->max_iter + 2 <= 1024) {
        gmres_pipelined(A, x, b, ksp);
        return;
    }
    if (gmres_run(A, x, b, ksp, FALSE)) {
        const b32 again = gmres_run(A, x, b, ksp, TRUE);
        ASSERT(!again);
        UNUSED(again);
    }
}

/* which Arnoldi step (GmresStep, solver_private.h) the most recent unpipelined GMRES solve of this solver ran; -1: none yet */
int DflKrylovLastGmresStep(Krylov* ksp) {
    return (ksp && ksp->ksp_solve == GMRESSolvePrivate && kext(ksp)) ? kext(ksp)->last_step : -1;
}

/* how the most recent unpipelined GMRES solve of this solver advanced: counts[s] = counted steps of s iterations, s = 1..4
   (counts[0] = 0), and whether a pair or a block raised a flag: bit 0 cancellation (some ||q_i|| < 1e-4 ||p_i'||), bit 1 a fused
   block whose q_i came out less orthogonal than DFL_GMRES_ORTH_TAU */
void DflKrylovLastGmresBlocks(Krylov* ksp, int counts[5], int* cancelled) {
    const KrylovExt* ex = (ksp && ksp->ksp_solve == GMRESSolvePrivate) ? kext(ksp) : NULL;
    if (counts) for (int s = 0; s < 5; ++s) counts[s] = ex ? ex->last_blocks[s] : 0;
    if (cancelled) *cancelled = ex ? ex->last_pair_cancelled : 0;
}
/* how many products of that solve wrote M^-1 of their own output for the product that followed (GmresPlan.fold_pc): every product
   of a counted pair or block but its last; 0 with DFL_GMRES_FOLD_PC=0, single steps, or any other step or preconditioner */
int DflKrylovLastFoldedProducts(Krylov* ksp) {
    return (ksp && ksp->ksp_solve == GMRESSolvePrivate && kext(ksp)) ? kext(ksp)->last_folded : 0;
}
/* how many counted blocks of three or four iterations of that solve ran the update and the fix-up as one pass
   (GmresPlan.fuse_fixup): all of them by default, 0 with DFL_GMRES_FUSE_FIXUP=0 or where no such block runs */
int DflKrylovLastFusedBlocks(Krylov* ksp) {
    return (ksp && ksp->ksp_solve == GMRESSolvePrivate && kext(ksp)) ? kext(ksp)->last_fused : 0;
}
/* the same in pairs and single steps: a counted step of s iterations is floor(s / 2) pairs and s mod 2 single steps */
void DflKrylovLastGmresPairs(Krylov* ksp, int* pairs, int* singles, int* cancelled) {
    int c[5];
    DflKrylovLastGmresBlocks(ksp, c, cancelled);
    if (pairs) *pairs = c[2] + c[3] + 2 * c[4];
    if (singles) *singles = c[1] + c[3];
}

/* the GMRES work space for this matrix as the next KrylovSolve would size it (host/ws_placement.c calibrates it ahead of
   the first solve) */
b32 DflKrylovEnsureWorkspace(Krylov* ksp, Matrix* A, index_type* n_out, index_type* m_out, index_type* ldh_out) {
    if (ksp->ksp_solve != GMRESSolvePrivate) return FALSE;
    *n_out = MatrixNumRow(A);
    DflGmresSizes(kext(ksp), ksp->max_iter, m_out, ldh_out);
    DflWsEnsure(kext(ksp), *n_out, *m_out, *ldh_out, ksp->max_iter);
    return TRUE;
}
