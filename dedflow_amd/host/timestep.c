/* The time step of a mesh as a run-time value, and the step limits of a state (include/dedflow.h, "time step").
 *
 * The step lives in MeshExt beside the assembly configuration, as the dfl_step_consts that dfl_step_consts_from_dt derives from
 * it: every kernel launch and every driver factor reads that one struct at the call, so two meshes step differently in one
 * process and the step may change between any two calls.  Nothing cached holds a value derived from dt: the schedules, the
 * face lists, the V2E map, the geometry records and the feature states depend on the mesh and the configuration only, and the
 * packed node records and the phase-change coefficients hold states, not factors.  Those two are still marked stale by the
 * setter, because the alpha states they were formed at belong to the old step.
 *
 * The limits: one launch pair (csrc/k_steplimit.hip), one 64-byte copy back, one synchronisation.  The partials and the result
 * are sized at the first call on a mesh and freed with it. */
#include <math.h>
#include <string.h>

#include "dedflow.h"
#include "dedflow_kernels.h"
#include "host_private.h"

#define kRHO (1.0e3) /* the built-in density of the (u,p) rows, csrc/asm_device.hpp */

typedef struct StepLimitState {
    index_type grid;  /* partial records held: dfl_step_limit_grid(T, 0) */
    f64* dev_v;       /* device: partials [grid][3], then the result [3] */
    index_type* dev_i; /* device: partials [grid][5], then the result [5] */
} StepLimitState;

void DflStepLimitFree(StepLimitState* st) {
    if (!st) return;
    CdamFreeDevice(st->dev_v, 0);
    CdamFreeDevice(st->dev_i, 0);
    CdamFreeHost(st, SIZE_OF(StepLimitState));
}

int DflTimeStepCheck(f64 dt, char* why, size_t why_len) {
    if (!isfinite(dt)) {
        snprintf(why, why_len, "dt is not finite (%g)", dt);
        return 1;
    }
    if (!(dt > 0.0)) {
        snprintf(why, why_len, "dt must be positive, got %g", dt);
        return 2;
    }
    return 0;
}

void DflMeshSetTimeStep(Mesh3D* mesh, f64 dt) {
    char why[160];
    if (DflTimeStepCheck(dt, why, sizeof why)) {
        fprintf(stderr, "DflMeshSetTimeStep: %s; unchanged\n", why);
        return;
    }
    MeshExt* x = (MeshExt*)mesh->ext;
    dfl_step_consts_from_dt(dt, &x->step);
    x->nodep_current = FALSE; /* alpha states of the old step */
    x->phase_current = FALSE;
}

f64 DflMeshTimeStep(const Mesh3D* mesh) { return DflMeshStepConsts(mesh)->dt; }

void DflMeshTimeStepLimits(Mesh3D* mesh, const f64* w, f64 level, DflTimeStepLimits* out) {
    MeshExt* x = (MeshExt*)mesh->ext;
    const Mesh3DData* dev = Mesh3DDevice(mesh);
    const index_type N = Mesh3DNumNode(mesh), T = Mesh3DNumTet(mesh);
    hipStream_t s = DflStream();
    StepLimitState* st = x->steplimit;
    if (!st) {
        st = (StepLimitState*)CdamMallocHost(SIZE_OF(StepLimitState));
        st->grid = dfl_step_limit_grid(T, 0);
        st->dev_v = (f64*)CdamMallocDevice(((ptrdiff_t)st->grid + 1) * 3 * SIZE_OF(f64));
        st->dev_i = (index_type*)CdamMallocDevice(((ptrdiff_t)st->grid + 1) * 5 * SIZE_OF(index_type));
        x->steplimit = st;
    }
    const DflSurfaceForces* sf = DflSurfaceConfig(mesh);
    const DflFluidMaterial* fm = DflFluidConfig(mesh);
    const dfl_step_limit_params prm = {level, sf ? sf->sigma0 : 0.0, sf ? sf->dsigma_dT : 0.0, sf ? sf->T_ref : 0.0};
    f64* out_v = st->dev_v + (size_t)st->grid * 3;
    index_type* out_i = st->dev_i + (size_t)st->grid * 5;
    dfl_step_limits(T, dev->ien, dev->xg, w, N, &prm, 0, st->dev_v, st->dev_i, out_v, out_i, s);
    f64 hv[3];
    index_type hi[5];
    HIPGUARD(hipMemcpyAsync(hv, out_v, sizeof hv, D2H, s));
    HIPGUARD(hipMemcpyAsync(hi, out_i, sizeof hi, D2H, s));
    HIPGUARD(hipStreamSynchronize(s));
    const f64 rho_bar = fm ? 0.5 * (fm->rho_gas + fm->rho_metal) : kRHO;
    memset(out, 0, sizeof *out);
    out->rate_adv = hv[0];
    out->rate_adv_surface = hv[1];
    out->cap_q = hv[2];
    out->tet_adv = hi[0];
    out->tet_surface = hi[1];
    out->tet_cap = hi[2];
    out->num_cut = hi[3];
    out->num_nonfinite = hi[4];
    out->dt_adv = hv[0] > 0.0 ? 1.0 / hv[0] : HUGE_VAL;
    out->dt_surface = hv[1] > 0.0 ? 1.0 / hv[1] : HUGE_VAL;
    out->dt_capillary = hv[2] > 0.0 ? sqrt(rho_bar / (2.0 * M_PI * hv[2])) : HUGE_VAL;
    out->dt = DflMeshTimeStep(mesh);
}
