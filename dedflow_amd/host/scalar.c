/* Scalar transport of the level set phi and the temperature T (include/dedflow.h, "scalar transport").
 *
 * Per mesh, built at the first use after DflMeshSetScalarTransport: the nodal pattern, the two CSR matrices over it, one GMRES
 * per field and the [2N] residual the F assemblies leave here (DflScalarCaptureResidual, host/assemble.c).  Without a
 * transport nothing of this exists and no call path touches it.  The Jacobian kernel (csrc/k_scalar.hip) sums in the order of
 * the mesh's sorted V2E map (DflMeshSortedV2E), which belongs to the mesh, not to this state. */
#include <string.h>
#include "dedflow.h"
#include "dedflow_kernels.h"
#include "host_private.h"
#include "solver_private.h"

typedef struct ScalarState {
    DflScalarTransport cfg;
    index_type N;
    CSRAttr* spy;            /* nodal pattern of the two matrices */
    Matrix *Jphi, *JT;       /* MAT_TYPE_CSR, own values */
    Krylov *ksp_phi, *ksp_T;
    f64* res;                /* device [2N]: phi / T rows of the last F assembly, Dirichlet rows zeroed */
    f64 *F, *dx;             /* device [6N], [2N]: DflScalarTransportSolve */
    f64 *nrm, *work;         /* device norms [2] + reduction scratch */
    index_type its[2];
} ScalarState;

static ScalarState* st_of(const Mesh3D* mesh) {
    const MeshExt* x = (const MeshExt*)mesh->ext;
    return x ? x->scalar : NULL;
}

void DflScalarFree(ScalarState* st) {
    if (!st) return;
    HIPGUARD(hipStreamSynchronize(DflStream()));
    if (st->ksp_phi) KrylovDestroy(st->ksp_phi);
    if (st->ksp_T) KrylovDestroy(st->ksp_T);
    if (st->Jphi) MatrixDestroy(st->Jphi);
    if (st->JT) MatrixDestroy(st->JT);
    if (st->spy) CSRAttrDestroy(st->spy);
    CdamFreeDevice(st->res, 0);
    CdamFreeDevice(st->F, 0);
    CdamFreeDevice(st->dx, 0);
    CdamFreeDevice(st->nrm, 0);
    CdamFreeDevice(st->work, 0);
    CdamFreeHost(st, SIZE_OF(ScalarState));
}

void DflMeshSetScalarTransport(Mesh3D* mesh, const DflScalarTransport* cfg) {
    MeshExt* x = (MeshExt*)mesh->ext;
    DflScalarFree(x->scalar);
    x->scalar = NULL;
    if (!cfg) return;
    ScalarState* st = (ScalarState*)CdamMallocHost(SIZE_OF(ScalarState));
    memset(st, 0, sizeof *st);
    st->cfg = *cfg;
    if (st->cfg.pc != PC_AMGX) st->cfg.pc = PC_JACOBI;
    if (!(st->cfg.rtol > 0.0)) st->cfg.rtol = 1e-10;
    if (st->cfg.maxit <= 0) st->cfg.maxit = 200;
    st->N = Mesh3DNumNode(mesh);
    st->its[0] = st->its[1] = -1;
    const index_type N = st->N;
    st->res = (f64*)CdamMallocDevice((ptrdiff_t)(2 * N > 0 ? 2 * N : 1) * SIZE_OF(f64));
    HIPGUARD(hipMemsetAsync(st->res, 0, (size_t)2 * N * sizeof(f64), DflStream()));
    x->scalar = st;
}

b32 DflMeshScalarTransportEnabled(const Mesh3D* mesh) { return st_of(mesh) != NULL; }

b32 DflScalarAdvancesT(const Mesh3D* mesh) {
    const ScalarState* st = st_of(mesh);
    return st && st->cfg.T;
}

f64* DflMeshScalarResidual(Mesh3D* mesh) {
    ScalarState* st = st_of(mesh);
    return st ? st->res : NULL;
}

void DflScalarTransportIterations(const Mesh3D* mesh, index_type its[2]) {
    const ScalarState* st = st_of(mesh);
    its[0] = st ? st->its[0] : -1;
    its[1] = st ? st->its[1] : -1;
}

/* zero the entries of the masked boundary groups' nodes in a nodal vector */
static void dirichlet_nodes_vec(const Mesh3D* mesh, index_type mask, f64* v) {
    for (index_type g = 0; g < mesh->num_bound && g < 31; ++g)
        if (mask & (1 << g)) dfl_dirichlet_vec(v, Mesh3DBoundNumNode(mesh, g), Mesh3DBoundNode(mesh, g), 1, 0, DflStream());
}
static void dirichlet_nodes_mat(const Mesh3D* mesh, index_type mask, Matrix* A) {
    for (index_type g = 0; g < mesh->num_bound && g < 31; ++g)
        if (mask & (1 << g)) MatrixZeroRow(A, Mesh3DBoundNumNode(mesh, g), Mesh3DBoundNode(mesh, g), 0, 1.0);
}

/* AssembleSystem, before it zeroes F[4N:6N): keep those rows (host/assemble.c) */
void DflScalarCaptureResidual(Mesh3D* mesh, const f64* F) {
    ScalarState* st = st_of(mesh);
    if (!st || !F) return;
    const index_type N = st->N;
    hipStream_t s = DflStream();
    for (int k = 0; k < 2; ++k) {
        const b32 on = k == 0 ? st->cfg.phi : st->cfg.T;
        f64* r = st->res + (size_t)k * N;
        if (on) HIPGUARD(hipMemcpyAsync(r, F + (size_t)(4 + k) * N, (size_t)N * sizeof(f64), hipMemcpyDeviceToDevice, s));
        else HIPGUARD(hipMemsetAsync(r, 0, (size_t)N * sizeof(f64), s));
    }
    dirichlet_nodes_vec(mesh, st->cfg.dirichlet_phi, st->res);
    dirichlet_nodes_vec(mesh, st->cfg.dirichlet_T, st->res + N);
}

static f64* csr_own_values(Matrix* A) {
    MatrixCSR* c = (MatrixCSR*)A->data;
    ASSERT(A->type == MAT_TYPE_CSR && !c->owner && "DflAssembleScalarJacobian: a MAT_TYPE_CSR matrix with its own values");
    if (!c->val) c->val = (value_type*)CdamMallocDevice((ptrdiff_t)c->attr->nnz * SIZE_OF(value_type));
    return c->val;
}

/* phase_reuse: the Newton driver calls, after its F assembly at the same alpha states (host/phase.c) */
static void assemble_scalar_jacobian(Mesh3D* mesh, f64* wgalpha, Matrix* Jphi, Matrix* JT, b32 phase_reuse) {
    if (!Jphi && !JT) return;
    ScalarState* st = st_of(mesh);
    const Mesh3DData* dev = Mesh3DDevice(mesh);
    const index_type N = Mesh3DNumNode(mesh);
    hipStream_t s = DflStream();
    const index_type *vrow, *vcol;
    DflMeshSortedV2E(mesh, &vrow, &vcol);
    const CSRAttr* ap = Jphi ? ((MatrixCSR*)Jphi->data)->attr : NULL;
    const CSRAttr* at = JT ? ((MatrixCSR*)JT->data)->attr : NULL;
    ASSERT((!ap || (ap->num_row == N && !ap->parent)) && (!at || (at->num_row == N && !at->parent)) &&
           "DflAssembleScalarJacobian: the matrices must lie over the nodal pattern");
    f64* vp = Jphi ? csr_own_values(Jphi) : NULL;
    f64* vt = JT ? csr_own_values(JT) : NULL;
    /* thermal material (include/dedflow.h): the launch that forms JT is the MATERIAL instantiation, which adds the entries jm
       per tet; Jphi gets the same bits from either */
    const dfl_thermal_params* mat = JT ? DflThermalParams(mesh) : NULL;
    const dfl_step_consts* k = DflMeshStepConsts(mesh);
    DflRangePush("AssembleScalarJacobian");
    if (ap && at && ap != at) { /* two pattern objects: one launch each */
        dfl_assemble_scalar_jacobian_dt(N, vrow, vcol, dev->ien, dev->xg, wgalpha, ap->row_ptr, ap->col_ind, vp, NULL, k, s);
        if (mat) dfl_assemble_scalar_jacobian_material_dt(N, vrow, vcol, dev->ien, dev->xg, wgalpha, at->row_ptr, at->col_ind, mat, NULL, vt, k, s);
        else dfl_assemble_scalar_jacobian_dt(N, vrow, vcol, dev->ien, dev->xg, wgalpha, at->row_ptr, at->col_ind, NULL, vt, k, s);
    } else {
        const CSRAttr* a = ap ? ap : at;
        if (mat) dfl_assemble_scalar_jacobian_material_dt(N, vrow, vcol, dev->ien, dev->xg, wgalpha, a->row_ptr, a->col_ind, mat, vp, vt, k, s);
        else dfl_assemble_scalar_jacobian_dt(N, vrow, vcol, dev->ien, dev->xg, wgalpha, a->row_ptr, a->col_ind, vp, vt, k, s);
    }
    /* latent heat (include/dedflow.h, "phase change"): kALPHAM H on the T diagonal, before the Dirichlet unit rows */
    if (JT && ((MeshExt*)mesh->ext)->phase) DflPhaseApplyScalarJacobian(mesh, wgalpha, at, vt, phase_reuse);
    if (st) {
        if (Jphi) dirichlet_nodes_mat(mesh, st->cfg.dirichlet_phi, Jphi);
        if (JT) dirichlet_nodes_mat(mesh, st->cfg.dirichlet_T, JT);
    }
    DflRangePop();
}

void DflAssembleScalarJacobian(Mesh3D* mesh, f64* wgalpha, f64* dwgalpha, Matrix* Jphi, Matrix* JT) {
    UNUSED(dwgalpha);
    assemble_scalar_jacobian(mesh, wgalpha, Jphi, JT, FALSE);
}

static Krylov* field_solver(const ScalarState* st, Matrix* A) {
    Krylov* ksp = KrylovCreateGMRES(st->cfg.maxit, 0.0, st->cfg.rtol, NULL);
    DflKrylovMarkInner(ksp); /* no basis-placement calibration for these solves */
    KrylovSetVerbose(ksp, !DflQuiet());
    if (st->cfg.pc == PC_AMGX) {
        KrylovSetPCType(ksp, PC_AMGX); /* KrylovSolve builds PCCreateAMGX on the CSR matrix */
    } else {
        ksp->pc = PCCreateJacobi(A, 1, NULL); /* a bare CSR matrix would otherwise get PC_NONE */
    }
    return ksp;
}

static void ensure_solvers(Mesh3D* mesh, ScalarState* st) {
    if (st->spy) return;
    st->spy = CSRAttrCreate(mesh);
    st->Jphi = MatrixCreateTypeCSR(st->spy, NULL);
    st->JT = MatrixCreateTypeCSR(st->spy, NULL);
    st->ksp_phi = field_solver(st, st->Jphi);
    st->ksp_T = field_solver(st, st->JT);
}

/* the scalar half of one Newton iteration: both Jacobians at (wgalpha, dwgalpha), both systems solved against the saved
 * residual into dx2[0, N) (phi) and dx2[N, 2N) (T); a field that is not advanced gets a zero increment */
void DflScalarSolveIncrements(Mesh3D* mesh, f64* wgalpha, f64* dwgalpha, f64* dx2) {
    ScalarState* st = st_of(mesh);
    ASSERT(st);
    const index_type N = st->N;
    ensure_solvers(mesh, st);
    UNUSED(dwgalpha);
    assemble_scalar_jacobian(mesh, wgalpha, st->cfg.phi ? st->Jphi : NULL, st->cfg.T ? st->JT : NULL, TRUE);
    HIPGUARD(hipMemsetAsync(dx2, 0, (size_t)2 * N * sizeof(f64), DflStream()));
    if (st->cfg.phi) {
        KrylovSolve(st->ksp_phi, st->Jphi, dx2, st->res);
        st->its[0] = KrylovGetStats(st->ksp_phi)->iterations;
    }
    if (st->cfg.T) {
        KrylovSolve(st->ksp_T, st->JT, dx2 + N, st->res + N);
        st->its[1] = KrylovGetStats(st->ksp_T)->iterations;
    }
    /* exactly zero on the held nodes whatever the preconditioner mixed into them (an AMG aggregate may span both kinds) */
    dirichlet_nodes_vec(mesh, st->cfg.dirichlet_phi, dx2);
    dirichlet_nodes_vec(mesh, st->cfg.dirichlet_T, dx2 + N);
}

/* ||R_phi||, ||R_T|| of the saved residual to the host (synchronises) */
void DflScalarNorms(Mesh3D* mesh, f64* out2) {
    ScalarState* st = st_of(mesh);
    ASSERT(st);
    const index_type N = st->N;
    hipStream_t s = DflStream();
    if (!st->nrm) {
        st->nrm = (f64*)CdamMallocDevice(2 * SIZE_OF(f64));
        st->work = (f64*)CdamMallocDevice((ptrdiff_t)(dfl_reduce_work_size() + 16) * SIZE_OF(f64));
    }
    dfl_dnrm2(N, st->res, st->nrm, st->work, s);
    dfl_dnrm2(N, st->res + N, st->nrm + 1, st->work, s);
    HIPGUARD(hipMemcpyAsync(out2, st->nrm, 2 * sizeof(f64), D2H, s));
    HIPGUARD(hipStreamSynchronize(s));
}

/* scratch of DflScalarTransportSolve (host/driver.c): F [6N] and the increment [2N] */
void DflScalarWork(Mesh3D* mesh, f64** F, f64** dx2) {
    ScalarState* st = st_of(mesh);
    ASSERT(st);
    if (!st->F) {
        st->F = (f64*)CdamMallocDevice((ptrdiff_t)st->N * 6 * SIZE_OF(f64));
        st->dx = (f64*)CdamMallocDevice((ptrdiff_t)st->N * 2 * SIZE_OF(f64));
    }
    *F = st->F;
    *dx2 = st->dx;
}
