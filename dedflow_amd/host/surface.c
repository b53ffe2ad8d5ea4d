/* Free-surface forces of the melt pool (build-defined, opt-in; model in include/dedflow.h, kernels in
 * dedflow_amd/csrc/k_surface.hip).  The reference's free surface has no physics.
 *
 * Per mesh, built by DflMeshSetSurfaceForces: the configuration, the one-byte-per-tet band flags (DFL_SURFACE_FLAGS=0: none),
 * and with in_time_step the two buffers DflTimeStep registers.  The node pass sums in the order of the mesh's sorted V2E map
 * (DflMeshSortedV2E), which the Set call has the mesh build if nothing did before.  The kernels read the node coordinates of
 * the mesh at every call, so nothing here goes stale when the nodes move (DflMeshGeometryChanged).  A DflMeshSurfaceLoad is
 * two launches (one without the flags): it allocates nothing and does not wait for the device.  Without a configuration
 * nothing of this exists and no call path touches it. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "dedflow.h"
#include "dedflow_kernels.h"
#include "host_private.h"

typedef struct SurfaceState {
    DflSurfaceForces cfg;
    dfl_surface_params prm;  /* cfg as the kernels take it */
    index_type N, T;
    u8* flag;                /* device [T] band flags of the last call, NULL (DFL_SURFACE_FLAGS=0): the node pass tests the band itself */
    f64 *load, *q_heat;      /* device [3N], [N]: what DflTimeStep registers (in_time_step), else NULL */
} SurfaceState;

static SurfaceState* st_of(const Mesh3D* mesh) {
    const MeshExt* x = (const MeshExt*)mesh->ext;
    return x ? x->surface : NULL;
}

void DflSurfaceFree(SurfaceState* st) {
    if (!st) return;
    HIPGUARD(hipStreamSynchronize(DflStream()));
    CdamFreeDevice(st->flag, 0);
    CdamFreeDevice(st->load, 0);
    CdamFreeDevice(st->q_heat, 0);
    CdamFreeHost(st, SIZE_OF(SurfaceState));
}

int DflSurfaceForcesCheck(const DflSurfaceForces* c, char* why, size_t why_len) {
    const f64 v[] = {c->level, c->eps, c->sigma0, c->dsigma_dT, c->T_ref, c->recoil_p0, c->recoil_a, c->T_boil, c->h_conv,
                     c->emissivity, c->T_amb, c->evap_q0};
    const char* name[] = {"level", "eps", "sigma0", "dsigma_dT", "T_ref", "recoil_p0", "recoil_a", "T_boil", "h_conv",
                          "emissivity", "T_amb", "evap_q0"};
    if (c->side != 1 && c->side != -1) {
        snprintf(why, why_len, "side must be +1 or -1, got %d", (int)c->side);
        return 1;
    }
    for (int k = 0; k < 12; ++k)
        if (!isfinite(v[k])) {
            snprintf(why, why_len, "%s is not finite (%g)", name[k], v[k]);
            return 2;
        }
    if (!(c->eps > 0.0)) {
        snprintf(why, why_len, "eps must be positive, got %g", c->eps);
        return 3;
    }
    if ((c->recoil_p0 > 0.0 || c->evap_q0 > 0.0) && !(c->T_boil > 0.0)) {
        snprintf(why, why_len, "T_boil must be positive while recoil or evaporation is on, got %g", c->T_boil);
        return 4;
    }
    return 0;
}

void DflMeshSetSurfaceForces(Mesh3D* mesh, const DflSurfaceForces* cfg) {
    MeshExt* x = (MeshExt*)mesh->ext;
    if (!cfg) {
        DflSurfaceFree(x->surface);
        x->surface = NULL;
        return;
    }
    char why[160];
    if (DflSurfaceForcesCheck(cfg, why, sizeof why)) {
        fprintf(stderr, "DflMeshSetSurfaceForces: %s; unchanged\n", why);
        return;
    }
    SurfaceState* st = x->surface;
    const index_type N = Mesh3DNumNode(mesh), T = Mesh3DNumTet(mesh);
    const index_type *vrow, *vcol;
    DflMeshSortedV2E(mesh, &vrow, &vcol); /* built here: no load call allocates or waits */
    if (!st) {
        st = (SurfaceState*)CdamMallocHost(SIZE_OF(SurfaceState));
        memset(st, 0, sizeof *st);
        st->N = N;
        st->T = T;
        x->surface = st;
    }
    st->cfg = *cfg;
    const dfl_surface_params prm = {cfg->level,     (f64)cfg->side, cfg->eps,    cfg->sigma0, cfg->dsigma_dT,  cfg->T_ref, cfg->recoil_p0,
                                    cfg->recoil_a,  cfg->T_boil,    cfg->h_conv, cfg->emissivity, cfg->T_amb, cfg->evap_q0};
    st->prm = prm;
    const char* env = getenv("DFL_SURFACE_FLAGS");
    DflTetFlagsMatch(&st->flag, T, !(env && env[0] == '0')); /* on: the band pass in front pays at bench size */
    if (cfg->in_time_step && !st->load) {
        st->load = (f64*)CdamMallocDevice((ptrdiff_t)(N > 0 ? N : 1) * 3 * SIZE_OF(f64));
        st->q_heat = (f64*)CdamMallocDevice((ptrdiff_t)(N > 0 ? N : 1) * SIZE_OF(f64));
    }
    HIPGUARD(hipStreamSynchronize(DflStream()));
}

b32 DflMeshSurfaceForcesEnabled(const Mesh3D* mesh) { return st_of(mesh) != NULL; }
const DflSurfaceForces* DflSurfaceConfig(const Mesh3D* mesh) { return st_of(mesh) ? &st_of(mesh)->cfg : NULL; }

void DflMeshSurfaceLoad(Mesh3D* mesh, const f64* w, f64* load, f64* q_heat, f64* area) {
    SurfaceState* st = st_of(mesh);
    if (!st) {
        fprintf(stderr, "DflMeshSurfaceLoad: no free-surface forces are set on this mesh (DflMeshSetSurfaceForces)\n");
        return;
    }
    const Mesh3DData* dev = Mesh3DDevice(mesh);
    hipStream_t s = DflStream();
    const index_type *vrow, *vcol;
    DflMeshSortedV2E(mesh, &vrow, &vcol);
    DflRangePush("DflMeshSurfaceLoad");
    if (st->flag) dfl_surface_flag_tets(st->T, dev->ien, dev->xg, w, st->N, &st->prm, st->flag, s);
    dfl_surface_load(st->N, vrow, vcol, dev->ien, dev->xg, w, &st->prm, st->flag, load, q_heat, area, s);
    DflRangePop();
}

b32 DflSurfaceInTimeStep(const Mesh3D* mesh) {
    const SurfaceState* st = st_of(mesh);
    return st && st->cfg.in_time_step;
}

b32 DflSurfaceTakeLoad(Mesh3D* mesh, const f64* w, f64** load, f64** q_heat) {
    SurfaceState* st = st_of(mesh);
    if (!st || !st->cfg.in_time_step) return FALSE;
    DflMeshSurfaceLoad(mesh, w, st->load, st->q_heat, NULL);
    *load = st->load;
    *q_heat = st->q_heat;
    return TRUE;
}
