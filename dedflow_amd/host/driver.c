/* The immediate caller of the hot path: generalized-alpha predictor / multi-corrector of
 * src/main.c:77-283 (SolveFlowSystem) and the per-step prediction/update of :535-565.
 * Same state algebra (fact1/fact2, :95-97; fac_pred/fac_corr, :535-536), same Newton control
 * (<= 4 iterations, 4-way relative test at 5e-4, :157,271-276), same printed lines.  The reference
 * spells the state algebra as ~10 cuBLAS BLAS-1 passes over 6N-vectors and four Dnrm2 host syncs per
 * Newton iteration; here every group is ONE pass (dfl_alpha_states, which also writes the packed node
 * records of the assembly kernels; dfl_alpha_predict / dfl_alpha_correct; dfl_norms4 + one 32-byte copy).
 * The work vectors live in the mesh (no process-global state). */
#include <math.h>
#include <string.h>
#include "dedflow.h"
#include "dedflow_kernels.h"
#include "host_private.h"

#define BS (6)

typedef struct FlowWork {
    index_type num_node;
    f64 *wgalpha, *dwgalpha, *nrm, *work;
} FlowWork;

/* work vectors of one mesh (kept in its MeshExt: two meshes / two solvers in one process do not collide) */
static FlowWork* fw_get(Mesh3D* mesh) {
    MeshExt* x = (MeshExt*)mesh->ext;
    const index_type N = Mesh3DNumNode(mesh);
    if (x->flow && x->flow->num_node == N) return x->flow;
    DflFreeFlowWork(x->flow);
    FlowWork* fw = (FlowWork*)CdamMallocHost(SIZE_OF(FlowWork));
    fw->wgalpha = (f64*)CdamMallocDevice((ptrdiff_t)N * BS * SIZE_OF(f64));
    fw->dwgalpha = (f64*)CdamMallocDevice((ptrdiff_t)N * BS * SIZE_OF(f64));
    fw->nrm = (f64*)CdamMallocDevice(8 * SIZE_OF(f64));
    fw->work = (f64*)CdamMallocDevice((ptrdiff_t)(dfl_reduce_work_size() + 16) * SIZE_OF(f64));
    fw->num_node = N;
    x->flow = fw;
    return fw;
}
void DflFreeFlowWork(FlowWork* fw) {
    if (!fw) return;
    CdamFreeDevice(fw->wgalpha, 0); CdamFreeDevice(fw->dwgalpha, 0); CdamFreeDevice(fw->nrm, 0); CdamFreeDevice(fw->work, 0);
    CdamFreeHost(fw, SIZE_OF(FlowWork));
}

/* alpha-level states, main.c:107-118 and :242-253: one pass (8 full-vector passes in the reference), which also writes
 * the packed node records the assembly kernels gather from -- the two AssembleSystem calls that follow skip their pack */
static void alpha_states(Mesh3D* mesh, const f64* wgold, const f64* dwgold, const f64* dwg, f64* wgalpha, f64* dwgalpha) {
    const f64 fact1[] = {1.0 - kALPHAM, kALPHAM};
    const dfl_step_consts* k = DflMeshStepConsts(mesh);
    const f64 fact2[] = {k->states_old, k->fact2};
    ((MeshExt*)mesh->ext)->phase_current = FALSE; /* new states: the phase-change coefficients of the old ones are stale */
    f64* const nodep = DflMeshNodeRecords(mesh); /* (allocates the compact (x, u) records of the Jacobian kernel as well) */
    dfl_alpha_states2(Mesh3DNumNode(mesh), wgold, dwgold, dwg, fact1[0], fact1[1], fact2[0], fact2[1], Mesh3DDevice(mesh)->xg, wgalpha,
                      dwgalpha, nodep, ((MeshExt*)mesh->ext)->nodexu, DflStream());
}

static void four_norms(FlowWork* fw, index_type N, const f64* F, f64* out, const DflComm* comm) {
    hipStream_t s = DflStream();
    /* element-partitioned run: ghost entries of F are zero, sums of squares are all-reduced */
    dfl_norms4(N, F, fw->nrm, comm ? 0 : 1, fw->work, s);
    if (comm) comm->allreduce_sum(comm->ctx, fw->nrm, 4);
    HIPGUARD(hipMemcpyAsync(out, fw->nrm, 4 * sizeof(f64), D2H, s));
    HIPGUARD(hipStreamSynchronize(s));
    if (comm) for (int k = 0; k < 4; ++k) out[k] = sqrt(out[k]);
}

/* partitioned run: residual entries of ghost nodes are partial sums that belong to another rank */
static void zero_ghost_residual(index_type N, f64* F, const DflComm* comm) {
    if (!comm) return;
    const index_type no = comm->num_owned_node;
    hipStream_t s = DflStream();
    if (no < N) {
        HIPGUARD(hipMemsetAsync(F + (size_t)no * 3, 0, (size_t)(N - no) * 3 * sizeof(f64), s));
        HIPGUARD(hipMemsetAsync(F + (size_t)N * 3 + no, 0, (size_t)(N - no) * sizeof(f64), s));
    }
}

/* SolveFlowSystem, main.c:77-283.  Returns the number of Newton iterations; rnorm_out[0..3] / rnorm_init_out[0..3]
 * receive the last and the initial residual norms (u, p, phi, T). */
index_type SolveFlowSystem(Mesh3D* mesh, f64* wgold, f64* dwgold, f64* dwg, Matrix* J, f64* F, f64* dx, Krylov* ksp,
                           Dirichlet** bcs, index_type nbc, index_type maxit, f64* rnorm_out, f64* rnorm_init_out) {
    const index_type N = Mesh3DNumNode(mesh);
    const f64 tol = 0.5e-3;
    hipStream_t s = DflStream();
    f64 rnorm[4] = {0, 0, 0, 0}, rnorm_init[4];
    index_type iter = 0;
    b32 converged = FALSE;
    if (maxit <= 0) maxit = 4;
    const DflComm* comm = KrylovGetComm(ksp);
    /* phi / T transport (host/scalar.c): single-GPU only, refused before anything is computed */
    const b32 scalar = DflMeshScalarTransportEnabled(mesh);
    if (scalar && comm) {
        fprintf(stderr, "SolveFlowSystem: the phi / T transport is single-GPU only; the solver has a communicator: solve refused\n");
        return -1;
    }
    if (DflMeshPhaseChangeEnabled(mesh) && comm) {
        fprintf(stderr, "SolveFlowSystem: the phase change is single-GPU only; the solver has a communicator: solve refused\n");
        return -1;
    }
    if (DflMeshThermalMaterialEnabled(mesh) && comm) {
        fprintf(stderr, "SolveFlowSystem: the thermal material is single-GPU only; the solver has a communicator: solve refused\n");
        return -1;
    }
    if (DflMeshFluidMaterialEnabled(mesh) && comm) {
        fprintf(stderr, "SolveFlowSystem: the fluid material is single-GPU only; the solver has a communicator: solve refused\n");
        return -1;
    }
    FlowWork* fw = fw_get(mesh);
    KrylovSetMesh(ksp, mesh); /* node coordinates for aggregation-based preconditioners */
    f64 *wgalpha = fw->wgalpha, *dwgalpha = fw->dwgalpha;
    alpha_states(mesh, wgold, dwgold, dwg, wgalpha, dwgalpha);
    DflAssembleSystemPrepacked(mesh, wgalpha, dwgalpha, F, NULL, bcs, nbc, TRUE);
    zero_ghost_residual(N, F, comm);
    four_norms(fw, N, F, rnorm_init, comm);
    if (scalar) DflScalarNorms(mesh, rnorm_init + 2); /* F[4N:6N) is zero: the phi / T rows were kept aside */
    if (!DflQuiet())
        for (int k = 0; k < 4; ++k)
            fprintf(stdout, "Newton %d) abs = %.17e rel = %6.4e (tol = %6.4e)\n", 0, rnorm_init[k], 1.0, tol);
    if (rnorm_init_out) memcpy(rnorm_init_out, rnorm_init, sizeof rnorm_init);
    for (int k = 0; k < 4; ++k) rnorm_init[k] += 1e-16;
    while (!converged && iter < maxit) {
        DflAssembleSystemPrepacked(mesh, wgalpha, dwgalpha, NULL, J, bcs, nbc, TRUE); /* same states as the residual before */
        HIPGUARD(hipMemsetAsync(dx, 0, (size_t)N * BS * sizeof(f64), s));
        KrylovSolve(ksp, J, dx, F);
        /* F[4N:6N) is zero, so the (u,p) solve runs on its 4N active rows and leaves dx[4N:6N) at the zero it was given;
           the scalar increments go there, at the same alpha states (block-Jacobi Newton) */
        if (scalar) DflScalarSolveIncrements(mesh, wgalpha, dwgalpha, dx + 4 * (size_t)N);
        if (comm) comm->halo_exchange(comm->ctx, dx); /* ghost copies of the increment from their owners */
        dfl_daxpy(N * BS, -1.0, dx, dwg, s); /* dwg -= dx, main.c:226 */
        alpha_states(mesh, wgold, dwgold, dwg, wgalpha, dwgalpha);
        DflAssembleSystemPrepacked(mesh, wgalpha, dwgalpha, F, NULL, bcs, nbc, TRUE);
        zero_ghost_residual(N, F, comm);
        four_norms(fw, N, F, rnorm, comm);
        if (scalar) DflScalarNorms(mesh, rnorm + 2);
        if (!DflQuiet())
            for (int k = 0; k < 4; ++k)
                fprintf(stdout, "Newton %d) abs = %.17e rel = %6.4e (tol = %6.4e)\n", iter + 1, rnorm[k], rnorm[k] / rnorm_init[k], tol);
        if (rnorm[0] < tol * rnorm_init[0] && rnorm[1] < tol * rnorm_init[1] && rnorm[2] < tol * rnorm_init[2] &&
            rnorm[3] < tol * rnorm_init[3])
            converged = TRUE;
        iter++;
    }
    if (rnorm_out) memcpy(rnorm_out, rnorm, sizeof rnorm);
    return iter;
}

/* one time step of main.c:537-565: predictor, Newton solve, corrector; optional DEM sub-steps.  A particle context coupled
 * to this mesh (ParticleContextSetFluidCoupling) instead takes `dem_substeps` fluid sub-steps after the corrector, in the
 * fluid state of the new time level; with two_way, the Newton solve sees the reaction load of the previous step's
 * sub-steps as an external load, and with two-way particle heat (ParticleContextSetHeat) the heat they gave the fluid as a
 * source of the T rows.  With inflow / outflow set on the context (ParticleContextSetInflow / SetOutflow),
 * ParticleContextAdd runs after the predictor and ParticleContextRemove after the particle sub-steps; with capture set
 * (ParticleContextSetCapture) ParticleContextCapture runs just before that Remove, and with its two_way the deposits of
 * the previous step enter the p, momentum and T rows of this step's Newton solve.  With free-surface forces set on the mesh
 * with in_time_step (DflMeshSetSurfaceForces), their load and heat loss at wgold enter the momentum and T rows as well.  With
 * redistancing set on the mesh with every > 0 (DflMeshSetRedistance), every every-th call first redistances phi of wgold.
 * With a volume correction set on the mesh with every > 0 (DflMeshSetVolumeCorrection), every every-th call then shifts phi of
 * wgold back to the target volume, after that redistancing and before anything else looks at phi; with its track_capture, a
 * step that took a pending two-way capture source adds the deposited volume to the target after its Newton solve.
 * With a surface contact set on the coupled context (ParticleContextSetSurfaceContact) every one of those fluid sub-steps also
 * collides the particles with the solid part of the surface phi = level, inside ParticleContextFluidStep: nothing here calls it.
 * With a laser surface set on the coupled context (ParticleContextSetLaserSurface), ParticleContextLaserSurfaceUpdate runs
 * once, before the first particle sub-step, in the state those sub-steps see.
 * With a solidification record set on the mesh with in_time_step (DflMeshSetSolidification), the record is updated with the
 * new wgold and the mesh's time step right after the step has written it; the first such call primes the record at its incoming wgold.
 * With track cross-sections set on the mesh with every > 0 (DflMeshSetTrackSections), every every-th call evaluates them at
 * the new wgold, after that record, whose T_peak they read.
 * With a porosity record set on the mesh with every > 0 (DflMeshSetPorosity), every every-th call evaluates it at the new wgold,
 * after the track cross-sections.
 * With a surface mesh set on the mesh with every > 0 (DflMeshSetSurfaceMesh), every every-th call evaluates it at the new wgold
 * with the field T, after the porosity record. */
index_type DflTimeStep(Mesh3D* mesh, f64* wgold, f64* dwgold, f64* dwg, Matrix* J, f64* F, f64* dx, Krylov* ksp, Dirichlet** bcs,
                       index_type nbc, index_type newton_maxit, ParticleContext* pctx, index_type dem_substeps, f64* rnorm_out,
                       f64* rnorm_init_out) {
    const index_type N = Mesh3DNumNode(mesh);
    hipStream_t s = DflStream();
    const f64 fac_pred = (kGAMMA - 1.0) / kGAMMA;
    const dfl_step_consts* k = DflMeshStepConsts(mesh); /* read once: the step of this call */
    const f64 fac_corr[] = {k->corr_old, k->corr_new};
    const b32 coupled = pctx && DflParticleCoupledMesh(pctx) == mesh;
    if (coupled && KrylovGetComm(ksp)) {
        fprintf(stderr, "DflTimeStep: particle-fluid coupling is single-GPU only; the solver has a communicator: step refused\n");
        return -1;
    }
    if (DflMeshScalarTransportEnabled(mesh) && KrylovGetComm(ksp)) {
        fprintf(stderr, "DflTimeStep: the phi / T transport is single-GPU only; the solver has a communicator: step refused\n");
        return -1;
    }
    if (DflSurfaceInTimeStep(mesh) && KrylovGetComm(ksp)) {
        fprintf(stderr, "DflTimeStep: the free-surface forces are single-GPU only; the solver has a communicator: step refused\n");
        return -1;
    }
    if (DflMeshPhaseChangeEnabled(mesh) && KrylovGetComm(ksp)) {
        fprintf(stderr, "DflTimeStep: the phase change is single-GPU only; the solver has a communicator: step refused\n");
        return -1;
    }
    if (DflMeshThermalMaterialEnabled(mesh) && KrylovGetComm(ksp)) {
        fprintf(stderr, "DflTimeStep: the thermal material is single-GPU only; the solver has a communicator: step refused\n");
        return -1;
    }
    if (DflMeshFluidMaterialEnabled(mesh) && KrylovGetComm(ksp)) {
        fprintf(stderr, "DflTimeStep: the fluid material is single-GPU only; the solver has a communicator: step refused\n");
        return -1;
    }
    if (DflRedistanceInTimeStep(mesh) && KrylovGetComm(ksp)) {
        fprintf(stderr, "DflTimeStep: the level-set redistancing is single-GPU only; the solver has a communicator: step refused\n");
        return -1;
    }
    if (DflVolumeCorrectionInTimeStep(mesh) && KrylovGetComm(ksp)) {
        fprintf(stderr, "DflTimeStep: the level-set volume correction is single-GPU only; the solver has a communicator: step refused\n");
        return -1;
    }
    if (DflSolidificationInTimeStep(mesh) && KrylovGetComm(ksp)) {
        fprintf(stderr, "DflTimeStep: the solidification record is single-GPU only; the solver has a communicator: step refused\n");
        return -1;
    }
    if (DflTrackSectionsInTimeStep(mesh) && KrylovGetComm(ksp)) {
        fprintf(stderr, "DflTimeStep: the track cross-sections are single-GPU only; the solver has a communicator: step refused\n");
        return -1;
    }
    if (DflPorosityInTimeStep(mesh) && KrylovGetComm(ksp)) {
        fprintf(stderr, "DflTimeStep: the porosity record is single-GPU only; the solver has a communicator: step refused\n");
        return -1;
    }
    if (DflMeshSurfaceMeshEnabled(mesh) && DflSurfaceMeshInTimeStep(mesh) && KrylovGetComm(ksp)) {
        fprintf(stderr, "DflTimeStep: the surface mesh is single-GPU only; the solver has a communicator: step refused\n");
        return -1;
    }
    DflRangePush("DflTimeStep");
    /* the solidification record (in_time_step), not primed yet: T_prev is the incoming T, so that this step is booked */
    DflSolidificationTimeStepPrime(mesh, wgold);
    /* every every-th step (DflMeshSetRedistance): phi of wgold becomes the band distance again before the surface load, the
       phase change and the solve look at it */
    DflRedistanceTimeStep(mesh, wgold);
    /* every every-th step (DflMeshSetVolumeCorrection): then phi of wgold is shifted back to the target volume */
    DflVolumeCorrectionTimeStep(mesh, wgold);
    const f64* user_load = DflMeshExternalLoad(mesh);
    const f64* reaction = coupled && DflParticleTwoWay(pctx) ? DflParticlePendingLoad(pctx) : NULL;
    if (reaction) {
        ASSERT(!user_load && "DflTimeStep: a two-way coupled step cannot add to an external load already registered");
        DflMeshSetExternalLoad(mesh, reaction);
    }
    /* the heat the particles gave the fluid in the previous step's sub-steps: a source of the T rows, treated as the load */
    const f64* user_heat = DflMeshHeatSource(mesh);
    const f64* heat = coupled && DflParticleHeatTwoWay(pctx) ? DflParticlePendingHeatSource(pctx) : NULL;
    if (heat) {
        ASSERT(!user_heat && "DflTimeStep: a two-way heat step cannot add to a heat source already registered");
        DflMeshSetHeatSource(mesh, heat);
    }
    /* what the melt pool captured since the last step (two-way capture): the volume rate on the p rows, the momentum and
       heat rates on top of the load and the heat source, in the capture's own buffers */
    const f64* user_vol = DflMeshVolumeSource(mesh);
    f64 *cap_vol = NULL, *cap_load = NULL, *cap_heat = NULL;
    if (coupled && DflCaptureTakePending(pctx, k->dt, &cap_vol, &cap_load, &cap_heat)) {
        ASSERT(!user_vol && "DflTimeStep: a two-way capture step cannot add to a volume source already registered");
        DflMeshSetVolumeSource(mesh, cap_vol);
        if (reaction) dfl_daxpy(3 * N, 1.0, reaction, cap_load, s);
        else ASSERT(!user_load && "DflTimeStep: a two-way capture step cannot add to an external load already registered");
        DflMeshSetExternalLoad(mesh, reaction = cap_load);
        if (cap_heat) {
            if (heat) dfl_daxpy(N, 1.0, heat, cap_heat, s);
            else ASSERT(!user_heat && "DflTimeStep: a two-way capture step cannot add to a heat source already registered");
            DflMeshSetHeatSource(mesh, heat = cap_heat);
        }
    }
    /* the free-surface forces at wgold (in_time_step): surface tension, Marangoni and recoil on top of the load, the surface
       heat loss on top of the heat source, in the mesh's own buffers */
    f64 *surf_load = NULL, *surf_heat = NULL;
    if (DflSurfaceTakeLoad(mesh, wgold, &surf_load, &surf_heat)) {
        if (reaction) dfl_daxpy(3 * N, 1.0, reaction, surf_load, s);
        else ASSERT(!user_load && "DflTimeStep: a free-surface step cannot add to an external load already registered");
        DflMeshSetExternalLoad(mesh, reaction = surf_load);
        if (heat) dfl_daxpy(N, 1.0, heat, surf_heat, s);
        else ASSERT(!user_heat && "DflTimeStep: a free-surface step cannot add to a heat source already registered");
        DflMeshSetHeatSource(mesh, heat = surf_heat);
    }
    dfl_alpha_predict(N, fac_pred, dwg, s);
    if (pctx) ParticleContextAdd(pctx); /* main.c:547-548; a no-op unless inflow is set */
    index_type it = SolveFlowSystem(mesh, wgold, dwgold, dwg, J, F, dx, ksp, bcs, nbc, newton_maxit, rnorm_out, rnorm_init_out);
    if (reaction) DflMeshSetExternalLoad(mesh, user_load);
    if (heat) DflMeshSetHeatSource(mesh, user_heat);
    if (cap_vol) {
        DflMeshSetVolumeSource(mesh, user_vol);
        DflVolumeCorrectionCaptured(mesh, cap_vol, k->dt); /* track_capture: the target follows what was deposited */
    }
    if (pctx && !coupled)
        for (index_type k = 0; k < dem_substeps; ++k) ParticleContextUpdate(pctx); /* coupled step: contact sweep (config 4) */
    dfl_alpha_correct(N, fac_corr[0], fac_corr[1], wgold, dwgold, dwg, s);
    DflSolidificationTimeStep(mesh, wgold); /* the record of this step (in_time_step); reads wgold only */
    DflTrackSectionsTimeStep(mesh, wgold);  /* every every-th step: the cross-sections of the new wgold; reads it only */
    DflPorosityTimeStep(mesh, wgold);       /* every every-th step: the pores of the new wgold; reads it only; nothing when off */
    if (DflMeshSurfaceMeshEnabled(mesh)) DflSurfaceMeshTimeStep(mesh, wgold); /* every every-th step: phi = level with T; reads only */
    if (coupled) DflLaserSurfaceTimeStep(pctx, wgold); /* the laser's snapshot of phi = level; a no-op unless a surface is set */
    if (coupled)
        for (index_type k = 0; k < dem_substeps; ++k) ParticleContextFluidStep(pctx, wgold); /* u at t_{n+1} */
    if (coupled) ParticleContextCapture(pctx, wgold); /* a no-op unless capture is set; before the outflow */
    if (pctx) ParticleContextRemove(pctx); /* main.c:568-569; a no-op unless outflow is set */
    DflRangePop();
    return it;
}

/* one scalar Newton update at the current u (include/dedflow.h): alpha states, residual (its phi / T rows kept by the F
 * assembly), both Jacobians, both solves, dwg[4N:6N) -= dx */
index_type DflScalarTransportSolve(Mesh3D* mesh, f64* wgold, f64* dwgold, f64* dwg, f64* rnorm_out) {
    if (!DflMeshScalarTransportEnabled(mesh)) {
        fprintf(stderr, "DflScalarTransportSolve: no scalar transport is set on this mesh (DflMeshSetScalarTransport)\n");
        return -1;
    }
    const index_type N = Mesh3DNumNode(mesh);
    FlowWork* fw = fw_get(mesh);
    f64 *F, *dx2;
    DflScalarWork(mesh, &F, &dx2);
    DflRangePush("DflScalarTransportSolve");
    alpha_states(mesh, wgold, dwgold, dwg, fw->wgalpha, fw->dwgalpha);
    DflAssembleSystemPrepacked(mesh, fw->wgalpha, fw->dwgalpha, F, NULL, NULL, 0, TRUE);
    DflScalarSolveIncrements(mesh, fw->wgalpha, fw->dwgalpha, dx2);
    dfl_daxpy(2 * N, -1.0, dx2, dwg + 4 * (size_t)N, DflStream());
    if (rnorm_out) DflScalarNorms(mesh, rnorm_out);
    DflRangePop();
    return 0;
}
