/* Dirichlet rows, preconditioner tree and the Krylov object behind the reference's dirichlet.h / pc.h / krylov.h: setters,
 * CG, the PC tree KrylovSolve builds, KrylovSolve itself.  GMRES lives in host/gmres.c, the placement of its work space in
 * host/ws_placement.c. */
#include <float.h>
#include <math.h>
#include <string.h>
#include <unistd.h>
#include <omp.h>
#include "dedflow.h"
#include "dedflow_kernels.h"
#include "host_private.h"
#include "solver_private.h"

/* ============================== Dirichlet ============================================= */
Dirichlet* DirichletCreate(const Mesh3D* mesh, index_type face_ind, index_type shape) {
    Dirichlet* bc = (Dirichlet*)CdamMallocHost(SIZE_OF(Dirichlet) + SIZE_OF(BCType) * shape);
    memset(bc, 0, sizeof(Dirichlet) + sizeof(BCType) * (size_t)shape);
    bc->mesh = mesh;
    bc->face_ind = face_ind;
    bc->shape = shape;
    bc->buffer_size = (size_t)Mesh3DBoundNumNode(mesh, face_ind);
    bc->buffer = CdamMallocDevice((ptrdiff_t)bc->buffer_size * SIZE_OF(index_type));
    /* bound_node lives on the device (Mesh.c:38-47) */
    if (bc->buffer_size)
        HIPGUARD(hipMemcpy(bc->buffer, Mesh3DBoundNode(mesh, face_ind), bc->buffer_size * sizeof(index_type), D2D));
    return bc;
}

void DirichletDestroy(Dirichlet* bc) {
    if (!bc) return;
    CdamFreeDevice(bc->buffer, 0);
    CdamFreeHost(bc, 0);
}

void DirichletApplyVec(Dirichlet* bc, value_type* b) {
    const Mesh3D* mesh = bc->mesh;
    index_type n = Mesh3DBoundNumNode(mesh, bc->face_ind);
    const index_type* bnode = Mesh3DBoundNode(mesh, bc->face_ind);
    for (index_type ic = 0; ic < bc->shape; ++ic)
        if (bc->bctype[ic] == BC_STRONG) dfl_dirichlet_vec(b, n, bnode, bc->shape, ic, DflStream());
}

void DirichletApplyMat(Dirichlet* bc, Matrix* A) {
    index_type n = Mesh3DBoundNumNode(bc->mesh, bc->face_ind);
    index_type* buffer = (index_type*)bc->buffer;
    value_type* blk = MatrixFSBlockValues(A);
    for (index_type ic = 0; ic < bc->shape; ++ic) {
        if (bc->bctype[ic] != BC_STRONG) continue;
        if (blk) {
            const CSRAttr* spy = ((MatrixFS*)A->data)->spy1x1;
            dfl_bcsr_zero_rows(spy->num_row, spy->row_ptr, spy->col_ind, blk, n, buffer, ic, 1.0, DflStream());
        } else { /* dirichlet.c:54-59 */
            GetRowFromNodeGPU(n, buffer, bc->shape, ic);
            MatrixZeroRow(A, n, buffer, 0, 1.0);
            GetNodeFromRowGPU(n, buffer, bc->shape);
        }
    }
}

/* ============================== PC ===================================================== */
static void none_setup(PC* pc) { UNUSED(pc); }
static void none_apply(PC* pc, value_type* x, value_type* y) { dfl_dcopy(((PCNone*)pc->data)->n, x, y, DflStream()); }
static void none_destroy(PC* pc) { CdamFreeHost(pc->data, SIZE_OF(PCNone)); }

PC* PCCreateNone(Matrix* mat, index_type n) {
    PC* pc = (PC*)CdamMallocHost(SIZE_OF(PC));
    memset(pc, 0, sizeof *pc);
    PCNone* d = (PCNone*)CdamMallocHost(SIZE_OF(PCNone));
    d->n = mat ? MatrixNumRow(mat) : n;
    pc->type = PC_NONE;
    pc->mat = mat;
    pc->data = d;
    pc->op->setup = none_setup;
    pc->op->apply = none_apply;
    pc->op->destroy = none_destroy;
    return pc;
}

static void jacobi_setup(PC* pc) { /* PCJacobiSetup, pc.c:44-85 */
    PCJacobi* d = (PCJacobi*)pc->data;
    Matrix* mat = (Matrix*)pc->mat;
    MatrixGetDiag(mat, (value_type*)d->diag, d->bs);
    if (d->bs == 1) VecPointwiseInv((value_type*)d->diag, d->n);
    else if (d->bs == 3) dfl_block3_invert(d->n / 3, (value_type*)d->diag, DflStream());
    else ASSERT(0 && "PCJacobi: block size must be 1 or 3");
}
static void jacobi_apply(PC* pc, value_type* x, value_type* y) { /* pc.c:93-114 */
    PCJacobi* d = (PCJacobi*)pc->data;
    if (d->bs == 1) VecPointwiseMult(x, (value_type*)d->diag, y, d->n);
    else dfl_block3_apply(d->n / 3, (value_type*)d->diag, x, y, DflStream());
}
static void jacobi_destroy(PC* pc) {
    PCJacobi* d = (PCJacobi*)pc->data;
    CdamFreeDevice(d->diag, 0);
    CdamFreeHost(d, SIZE_OF(PCJacobi));
}

PC* PCCreateJacobi(Matrix* mat, index_type bs, void* handle) {
    PC* pc = (PC*)CdamMallocHost(SIZE_OF(PC));
    memset(pc, 0, sizeof *pc);
    PCJacobi* d = (PCJacobi*)CdamMallocHost(SIZE_OF(PCJacobi));
    d->n = MatrixNumRow(mat);
    d->bs = bs;
    d->diag = CdamMallocDevice(SIZE_OF(value_type) * (ptrdiff_t)d->n * bs);
    pc->type = PC_JACOBI;
    pc->mat = mat;
    pc->data = d;
    pc->cublas_handle = handle;
    pc->op->setup = jacobi_setup;
    pc->op->apply = jacobi_apply;
    pc->op->destroy = jacobi_destroy;
    return pc;
}

/* the tree KrylovSolve builds (krylov.c:439-453): one fused launch instead of four */
b32 DflPcJacobiTreeData(PC* pc, const f64** d33, const f64** d1, index_type* N_out, index_type* nrows) {
    if (!pc || pc->type != PC_DECOMPOSITION) return FALSE;
    PCDecomposition* d = (PCDecomposition*)pc->data;
    if (d->n_sec != 4 || !d->pc[0] || !d->pc[1] || !d->pc[2] || !d->pc[3]) return FALSE;
    if (d->pc[0]->type != PC_JACOBI || d->pc[1]->type != PC_JACOBI || d->pc[2]->type != PC_NONE || d->pc[3]->type != PC_NONE)
        return FALSE;
    const PCJacobi *j0 = (PCJacobi*)d->pc[0]->data, *j1 = (PCJacobi*)d->pc[1]->data;
    const index_type N = j1->n;
    if (j0->bs != 3 || j1->bs != 1 || j0->n != 3 * N) return FALSE;
    if (d->offset[0] != 0 || d->offset[1] != 3 * N || d->offset[2] != 4 * N || d->offset[3] != 5 * N) return FALSE;
    if (((PCNone*)d->pc[2]->data)->n != N || ((PCNone*)d->pc[3]->data)->n != N) return FALSE;
    *N_out = N; *d33 = (const f64*)j0->diag; *d1 = (const f64*)j1->diag;
    *nrows = MatrixFSOwnedRows((Matrix*)pc->mat);
    return TRUE;
}

static void decomposition_setup(PC* pc) {
    PCDecomposition* d = (PCDecomposition*)pc->data;
    const f64 *d33, *d1;
    index_type N, nrows;
    Matrix* A = (Matrix*)pc->mat;
    if (DflPcJacobiTreeData(pc, &d33, &d1, &N, &nrows) && A && MatrixFSBlockValues(A)) {
        /* the tree of krylov.c:439-453 on the block-mode matrix: both diagonal extractions and inversions
           (MatrixGetDiag x2, batched LU, pointwise inverse; pc.c:44-85) in one launch, same arithmetic */
        const CSRAttr* spy = ((MatrixFS*)A->data)->spy1x1;
        dfl_pc_jacobi_setup_rows(nrows, spy->row_ptr, spy->col_ind, MatrixFSBlockValues(A), (value_type*)d33, (value_type*)d1, DflStream());
        return;
    }
    for (index_type i = 0; i < d->n_sec; ++i) PCSetup(d->pc[i]);
}
static void decomposition_apply(PC* pc, value_type* x, value_type* y) {
    PCDecomposition* d = (PCDecomposition*)pc->data;
    const f64 *d33, *d1;
    index_type N, nrows;
    if (DflPcJacobiTreeData(pc, &d33, &d1, &N, &nrows)) {
        dfl_pc_jacobi_apply_rows(nrows, N, 6 * N, d33, d1, x, y, DflStream());
        return;
    }
    for (index_type i = 0; i < d->n_sec; ++i) PCApply(d->pc[i], x + d->offset[i], y + d->offset[i]);
}
static void decomposition_destroy(PC* pc) {
    PCDecomposition* d = (PCDecomposition*)pc->data;
    for (index_type i = 0; i < d->n_sec; ++i) PCDestroy(d->pc[i]);
    CdamFreeHost(d->offset, 0);
    CdamFreeHost(d->pc, 0);
    CdamFreeHost(d, SIZE_OF(PCDecomposition));
}

PC* PCCreateDecomposition(Matrix* mat, index_type n_sec, const index_type* offset, void* handle) {
    PC* pc = (PC*)CdamMallocHost(SIZE_OF(PC));
    memset(pc, 0, sizeof *pc);
    PCDecomposition* d = (PCDecomposition*)CdamMallocHost(SIZE_OF(PCDecomposition));
    memset(d, 0, sizeof *d);
    d->n_sec = n_sec;
    d->offset = (index_type*)CdamMallocHost(SIZE_OF(index_type) * (n_sec + 1));
    memcpy(d->offset, offset, sizeof(index_type) * (size_t)n_sec); /* the reference copies n_sec+1 from an n_sec array (pc.c:124) */
    d->offset[n_sec] = 0;
    d->pc = (PC**)CdamMallocHost(SIZE_OF(PC*) * n_sec);
    memset(d->pc, 0, sizeof(PC*) * (size_t)n_sec);
    pc->type = PC_DECOMPOSITION;
    pc->mat = mat;
    pc->data = d;
    pc->cublas_handle = handle;
    pc->op->setup = decomposition_setup;
    pc->op->apply = decomposition_apply;
    pc->op->destroy = decomposition_destroy;
    return pc;
}

void PCApply(PC* pc, f64* x, f64* y) { pc->op->apply(pc, x, y); }
void PCSetup(PC* pc) { pc->op->setup(pc); }
void PCDestroy(PC* pc) {
    if (!pc) return;
    pc->op->destroy(pc);
    CdamFreeHost(pc, SIZE_OF(PC));
}

/* ============================== Krylov ================================================== */

static Krylov* krylov_init(index_type max_iter, f64 atol, f64 rtol, void* handle) {
    Krylov* ksp = (Krylov*)CdamMallocHost(SIZE_OF(Krylov));
    memset(ksp, 0, sizeof *ksp);
    ksp->max_iter = max_iter;
    ksp->atol = atol;
    ksp->rtol = rtol;
    ksp->handle = handle;
    KrylovExt* x = (KrylovExt*)CdamMallocHost(SIZE_OF(KrylovExt));
    memset(x, 0, sizeof *x);
    x->check_interval = 20; /* krylov.c:281 */
    x->verbose = TRUE;
    x->last_step = -1;
    ksp->ext = x;
    return ksp;
}

const KrylovStats* KrylovGetStats(const Krylov* k) { return &kext(k)->stats; }
void KrylovSetCheckInterval(Krylov* k, index_type n) {
    kext(k)->check_interval = n > 0 ? n : 20;
    kext(k)->check_interval_set = TRUE;
}
void KrylovSetVerbose(Krylov* k, b32 v) { kext(k)->verbose = v; }
void KrylovSetPCType(Krylov* k, PCType type) {
    if (kext(k)->pc_type != type) { /* rebuilt at the next KrylovSolve */
        PCDestroy((PC*)k->pc);
        k->pc = NULL;
    }
    kext(k)->pc_type = type;
}
PC* KrylovGetPC(const Krylov* k) { return (PC*)k->pc; }
void KrylovSetFusedNorm(Krylov* k, b32 on) { kext(k)->fused_norm = on; }
void KrylovSetPipelined(Krylov* k, b32 on) { kext(k)->pipelined = on; }
void KrylovSetRestart(Krylov* k, index_type m) { kext(k)->restart = m; }
void KrylovSetFlexible(Krylov* k, b32 on) {
    kext(k)->flexible = on;
    kext(k)->flexible_user = on;
}
void KrylovSetAMGXConfig(Krylov* k, const char* options) {
    KrylovExt* x = kext(k);
    free(x->amgx_cfg);
    x->amgx_cfg = options ? strdup(options) : NULL;
    if (x->pc_type == PC_AMGX) { /* rebuilt with the new configuration at the next KrylovSolve */
        PCDestroy((PC*)k->pc);
        k->pc = NULL;
    }
}
void KrylovSetMesh(Krylov* k, const Mesh3D* mesh) { kext(k)->mesh = mesh; }
void KrylovSetAggregateSize(Krylov* k, index_type nodes) { kext(k)->agg_size = nodes; }
const DflComm* KrylovGetComm(const Krylov* k) { return kext(k)->has_comm ? &kext(k)->comm : NULL; }
void KrylovSetComm(Krylov* k, const DflComm* comm) {
    KrylovExt* x = kext(k);
    x->has_comm = comm != NULL;
    if (comm) x->comm = *comm;
}

/* Preconditioned conjugate gradients.  The reference's CGSolvePrivate is an empty stub
 * (krylov.c:42-51); BASELINE.json's config 0 asks for "50 CG iters", so this is
 * build-defined: textbook left-preconditioned CG, absolute/relative test on ||r||_2
 * every iteration.  Parity unpinned (no reference behaviour); checked against scipy. */
/* h[0] = a1.b1, h[1] = a2.b2 over all ranks, on the host */
static void cg_dot2(KrylovExt* ex, index_type na, const f64* a1, const f64* b1, const f64* a2, const f64* b2, f64* h) {
    hipStream_t s = DflStream();
    dfl_ddot(na, a1, b1, ex->nrm, ex->work, s);
    dfl_ddot(na, a2, b2, ex->nrm + 1, ex->work, s);
    if (ex->has_comm) ex->comm.allreduce_sum(ex->comm.ctx, ex->nrm, 2);
    HIPGUARD(hipMemcpyAsync(h, ex->nrm, 2 * sizeof(f64), D2H, s));
    HIPGUARD(hipStreamSynchronize(s));
}

static void CGSolvePrivate(Matrix* A, f64* x, f64* b, void* ctx) {
    Krylov* ksp = (Krylov*)ctx;
    KrylovExt* ex = kext(ksp);
    PC* pc = (PC*)ksp->pc;
    hipStream_t s = DflStream();
    const index_type n = MatrixNumRow(A), maxit = ksp->max_iter;
    index_type na = n;
    const b32 dist = ex->has_comm;
    const index_type tail_begin = DflKrylovTailBegin(A);
    DflWsEnsure(ex, n, 3, 32, 3); /* r, z, p, Ap in Q[0..3] */
    if (tail_begin < n) {
        b32 tail_zero = FALSE, unused = FALSE;
        DflProbeOperands(b, tail_begin, n, NULL, ex->work, &tail_zero, &unused);
        if (tail_zero) na = tail_begin;
    }
    f64 *r = ex->Q, *z = ex->Q + (size_t)n, *p = ex->Q + 2 * (size_t)n, *Ap = ex->Q + 3 * (size_t)n;
    f64 h[2], rz, rz_new, pAp, rn, r0;
    dfl_dcopy(na, b, r, s);
    if (dist) ex->comm.halo_exchange(ex->comm.ctx, x);
    MatrixAMVPBY(A, -1.0, x, 1.0, r);
    DflZeroGhostRows(ex, A, r, na);
    index_type it = 0;
    b32 converged = FALSE;
    if (pc) PCApply(pc, r, z); else dfl_dcopy(na, r, z, s);
    dfl_dcopy(na, z, p, s);
    cg_dot2(ex, na, r, z, r, r, h);
    rz = h[0];
    r0 = sqrt(h[1]);
    ex->stats.rnrm_init = r0;
    DflKrylovPrintProgress(ksp, 0, r0, r0, 0);
    if (r0 == 0.0) converged = TRUE; /* x already solves the system: alpha would be 0/0 */
    while (!converged && it < maxit) {
        if (dist) ex->comm.halo_exchange(ex->comm.ctx, p);
        MatrixMatVec(A, p, Ap);
        dfl_ddot(na, p, Ap, ex->nrm, ex->work, s);
        if (dist) ex->comm.allreduce_sum(ex->comm.ctx, ex->nrm, 1);
        HIPGUARD(hipMemcpyAsync(&pAp, ex->nrm, sizeof(f64), D2H, s));
        HIPGUARD(hipStreamSynchronize(s));
        f64 alpha = rz / pAp;
        dfl_daxpy(na, alpha, p, x, s);
        dfl_daxpy(na, -alpha, Ap, r, s);
        if (pc) PCApply(pc, r, z); else dfl_dcopy(na, r, z, s);
        cg_dot2(ex, na, r, z, r, r, h);
        rz_new = h[0];
        rn = sqrt(h[1]);
        if (it < 512) ex->stats.res_hist[it] = rn;
        f64 beta = rz_new / rz;
        rz = rz_new;
        dfl_dscal(na, beta, p, s);
        dfl_daxpy(na, 1.0, z, p, s);
        it++;
        if (it % 20 == 0) DflKrylovPrintProgress(ksp, it, rn, r0, 0);
        converged = DflKrylovConverged(ksp, rn, r0);
    }
    ex->stats.iterations = it;
    ex->stats.converged = converged;
}

Krylov* KrylovCreateCG(index_type max_iter, f64 atol, f64 rtol, void* handle) {
    Krylov* ksp = krylov_init(max_iter, atol, rtol, handle);
    ksp->ksp_solve = CGSolvePrivate;
    return ksp;
}
Krylov* KrylovCreateGMRES(index_type max_iter, f64 atol, f64 rtol, void* handle) {
    Krylov* ksp = krylov_init(max_iter, atol, rtol, handle);
    ksp->ksp_solve = GMRESSolvePrivate;
    return ksp;
}
void KrylovDestroy(Krylov* ksp) {
    if (!ksp) return;
    PCDestroy((PC*)ksp->pc);
    DflWsFree(kext(ksp));
    if (kext(ksp)->h_stat) {
        HIPGUARD(hipHostFree(kext(ksp)->h_stat));
        HIPGUARD(hipEventDestroy(kext(ksp)->ev_stat));
    }
    DflWsVecFreeAs(kext(ksp)->Zp, kext(ksp)->zp_pooled);
    if (kext(ksp)->red_stream) {
        HIPGUARD(hipStreamSynchronize(kext(ksp)->red_stream));
        HIPGUARD(hipEventDestroy(kext(ksp)->ev_w));
        HIPGUARD(hipEventDestroy(kext(ksp)->ev_h));
        HIPGUARD(hipStreamDestroy(kext(ksp)->red_stream));
    }
    free(kext(ksp)->amgx_cfg);
    CdamFreeHost(ksp->ext, SIZE_OF(KrylovExt));
    CdamFreeHost(ksp, SIZE_OF(Krylov));
}

/* the (re)build step of KrylovSolve, krylov.c:386-456: a new PC tree when there is none or the matrix changed */
PC* DflKrylovBuildPC(Krylov* ksp, Matrix* A) {
    PC* pc = (PC*)ksp->pc;
    if (pc == NULL || pc->mat != A) {
        PCDestroy(pc);
        /* PC_TWOLEVEL needs the block-mode matrix, the mesh (node coordinates for the aggregates) and, on a partitioned
           matrix, a communicator that knows its rank; when it cannot be built the solver falls back to PC_ILU0 (block mode) or
           to the reference's tree -- on every rank alike, the conditions are properties of the setup, not of the data */
        KrylovExt* kx = kext(ksp);
        pc = NULL;
        if (kx->pc_type == PC_TWOLEVEL && MatrixFSBlockValues(A) && kx->mesh)
            pc = PCCreateTwoLevelDist(A, kx->mesh, kx->agg_size, kx->has_comm ? &kx->comm : NULL);
        const b32 two_level = pc != NULL;
        if (kx->pc_type == PC_TWOLEVEL && !two_level)
            fprintf(stderr, "KrylovSolve: PC_TWOLEVEL unavailable for this matrix, using %s\n",
                    MatrixFSBlockValues(A) ? "PC_ILU0" : "the reference's Jacobi tree");
        /* convergence test every 20th iteration (krylov.c:281) -- every 4th under PC_TWOLEVEL, where an iteration costs two
           fine-level matvecs, a DILU sweep and a coarse solve and the 8-byte read nothing -- unless the caller chose */
        if (!kx->check_interval_set) kx->check_interval = two_level ? 4 : 20;
        /* the coarse level of PC_TWOLEVEL is solved by an inner Krylov iteration: the PC varies, the outer solver must be
           flexible; a fixed preconditioner gets the plain recurrence back (and its Z basis freed) unless the caller asked */
        kx->flexible = two_level || kx->flexible_user;
        if (!kx->flexible && kx->Z) {
            DflWsVecFreeAs(kx->Z, kx->ws_pooled);
            kx->Z = NULL;
        }
        /* PC_AMGX: the reference's tree with AMG on the pressure block (krylov.c:450), or AMG on a plain CSR matrix.  Refused
           with a communicator (no partitioned AMG; a property of the setup, so every rank falls back alike) */
        PC* amg = NULL;
        const b32 fs_tree = A->type == MAT_TYPE_FS && ((MatrixFS*)A->data)->n_offset >= 4;
        if (!two_level && kx->pc_type == PC_AMGX) {
            if (kx->has_comm) {
                /* no partitioned AMG */
            } else if (fs_tree) {
                MatrixFS* fs = (MatrixFS*)A->data;
                amg = PCCreateAMGX(fs->mat[1 * fs->n_offset + 1], kx->amgx_cfg);
            } else if (A->type == MAT_TYPE_CSR) amg = PCCreateAMGX(A, kx->amgx_cfg);
            if (!amg)
                fprintf(stderr, "KrylovSolve: PC_AMGX unavailable %s, using %s\n", kx->has_comm ? "with a communicator" : "for this matrix",
                        fs_tree ? "the reference's Jacobi tree" : "no preconditioner");
        }
        if (two_level) {
            /* built above */
        } else if (amg && !fs_tree) {
            pc = amg;
        } else if ((kx->pc_type == PC_ILU0 || kx->pc_type == PC_TWOLEVEL) && MatrixFSBlockValues(A)) {
            pc = PCCreateDILU(A);
        } else if (A->type == MAT_TYPE_FS && ((MatrixFS*)A->data)->n_offset >= 4) {
            MatrixFS* fs = (MatrixFS*)A->data;
            index_type n = fs->spy1x1->num_row;
            index_type offset[] = {0 * n, 3 * n, 4 * n, 5 * n};
            Matrix* A00 = fs->mat[0 * fs->n_offset + 0];
            Matrix* A11 = fs->mat[1 * fs->n_offset + 1];
            pc = PCCreateDecomposition(A, 4, offset, ksp->handle);
            ((PCDecomposition*)pc->data)->pc[0] = PCCreateJacobi(A00, 3, ksp->handle);
            ((PCDecomposition*)pc->data)->pc[1] = amg ? amg : PCCreateJacobi(A11, 1, ksp->handle);
            ((PCDecomposition*)pc->data)->pc[2] = PCCreateNone(NULL, n);
            ((PCDecomposition*)pc->data)->pc[3] = PCCreateNone(NULL, n);
        } else {
            pc = PCCreateNone(A, MatrixNumRow(A));
            pc->mat = A;
        }
        ksp->pc = pc;
    }
    return pc;
}

/* KrylovSolve, krylov.c:386-456: (re)build the PC tree when the matrix changes, PCSetup every solve */
void KrylovSolve(Krylov* ksp, Matrix* A, f64* x, f64* b) {
    PC* pc = DflKrylovBuildPC(ksp, A);
    DflRangePush("KrylovSolve");
    PCSetup(pc);
    DflKrylovSolvePrepared(ksp, A, x, b);
    DflRangePop();
}

void DflKrylovMarkInner(Krylov* ksp) { kext(ksp)->no_calibration = TRUE; }

/* the solve alone: ksp->pc exists and has been set up for the current values of A (inner solvers of PC_TWOLEVEL, whose
   coarse matrices change at PCSetup of the outer preconditioner only, not between applications) */
void DflKrylovSolvePrepared(Krylov* ksp, Matrix* A, f64* x, f64* b) {
    ksp->ksp_solve(A, x, b, ksp);
    KrylovStats* st = &kext(ksp)->stats;
    st->total_solves++;
    st->total_converged += st->converged ? 1 : 0;
    st->total_iterations += st->iterations;
}
