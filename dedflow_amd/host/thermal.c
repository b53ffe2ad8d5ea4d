/* Thermal material: conductivity and heat capacity of the T rows follow phi and the liquid fraction (build-defined, opt-in;
 * model in include/dedflow.h, "thermal material", kernels in dedflow_amd/csrc/k_thermal.hip and k_scalar.hip).  The
 * reference's heat equation has one material.
 *
 * Per mesh, built by DflMeshSetThermalMaterial: the configuration and its kernel form.  The row pass sums in the order of the
 * mesh's sorted V2E map (DflMeshSortedV2E), which the Set call has the mesh build if nothing did before, and adds straight
 * into the T rows of F, so the state owns no device buffer; the kernels read the node coordinates at every call, so nothing
 * here goes stale when the nodes move.  The F hook is one launch, the Jacobian is the scalar transport's own launch in its
 * MATERIAL instantiation.  Nothing is allocated per call and nothing waits for the device.  Without a configuration nothing
 * of this exists and no call path touches it. */
#include <math.h>
#include <stdio.h>
#include <string.h>
#include "dedflow.h"
#include "dedflow_kernels.h"
#include "host_private.h"

typedef struct ThermalState {
    DflThermalMaterial cfg;
    dfl_thermal_params prm; /* cfg as the kernels take it */
    index_type N;
} ThermalState;

static ThermalState* st_of(const Mesh3D* mesh) {
    const MeshExt* x = (const MeshExt*)mesh->ext;
    return x ? x->thermal : NULL;
}

void DflThermalFree(ThermalState* st) {
    if (!st) return;
    HIPGUARD(hipStreamSynchronize(DflStream())); /* a launch in flight holds the parameters by value, but the V2E map by pointer */
    CdamFreeHost(st, SIZE_OF(ThermalState));
}

int DflThermalMaterialCheck(const DflThermalMaterial* c, char* why, size_t why_len) {
    const f64 v[] = {c->k_gas, c->k_solid, c->k_liquid, c->c_gas, c->c_metal, c->T_solidus, c->T_liquidus, c->level, c->eps};
    const char* name[] = {"k_gas", "k_solid", "k_liquid", "c_gas", "c_metal", "T_solidus", "T_liquidus", "level", "eps"};
    for (int k = 0; k < 9; ++k)
        if (!isfinite(v[k])) {
            snprintf(why, why_len, "%s is not finite (%g)", name[k], v[k]);
            return 1;
        }
    for (int k = 0; k < 5; ++k)
        if (!(v[k] > 0.0)) {
            snprintf(why, why_len, "%s must be positive, got %g", name[k], v[k]);
            return 2;
        }
    if (c->k_liquid != c->k_solid && !(c->T_liquidus > c->T_solidus)) {
        snprintf(why, why_len, "T_liquidus must lie above T_solidus while k_liquid differs from k_solid, got %g <= %g",
                 c->T_liquidus, c->T_solidus);
        return 3;
    }
    if (c->use_phi && c->side != 1 && c->side != -1) {
        snprintf(why, why_len, "side must be +1 or -1 with use_phi, got %d", (int)c->side);
        return 4;
    }
    if (c->use_phi && !(c->eps > 0.0)) {
        snprintf(why, why_len, "eps must be positive with use_phi, got %g", c->eps);
        return 5;
    }
    return 0;
}

void DflMeshSetThermalMaterial(Mesh3D* mesh, const DflThermalMaterial* cfg) {
    MeshExt* x = (MeshExt*)mesh->ext;
    if (!cfg) {
        DflThermalFree(x->thermal);
        x->thermal = NULL;
        return;
    }
    char why[200];
    if (DflThermalMaterialCheck(cfg, why, sizeof why)) {
        fprintf(stderr, "DflMeshSetThermalMaterial: %s; unchanged\n", why);
        return;
    }
    ThermalState* st = x->thermal;
    const index_type *vrow, *vcol;
    DflMeshSortedV2E(mesh, &vrow, &vcol); /* built here: no later call allocates or waits */
    if (!st) {
        st = (ThermalState*)CdamMallocHost(SIZE_OF(ThermalState));
        memset(st, 0, sizeof *st);
        st->N = Mesh3DNumNode(mesh);
        x->thermal = st;
    }
    st->cfg = *cfg;
    const dfl_thermal_params prm = {cfg->k_gas,     cfg->k_solid,    cfg->k_liquid, cfg->c_gas,     cfg->c_metal,        cfg->T_solidus,
                                    cfg->T_liquidus, cfg->level,      (f64)cfg->side, cfg->eps,      cfg->use_phi ? 1 : 0};
    st->prm = prm;
    HIPGUARD(hipStreamSynchronize(DflStream()));
}

b32 DflMeshThermalMaterialEnabled(const Mesh3D* mesh) { return st_of(mesh) != NULL; }

const dfl_thermal_params* DflThermalParams(const Mesh3D* mesh) {
    const ThermalState* st = st_of(mesh);
    return st ? &st->prm : NULL;
}

void DflMeshThermalRows(Mesh3D* mesh, const f64* w, const f64* dw, f64* r, f64* Kn, f64* Cn) {
    ThermalState* st = st_of(mesh);
    if (!st) {
        fprintf(stderr, "DflMeshThermalRows: no thermal material is set on this mesh (DflMeshSetThermalMaterial)\n");
        return;
    }
    if (!r && !Kn && !Cn) return;
    const Mesh3DData* dev = Mesh3DDevice(mesh);
    const index_type *vrow, *vcol;
    DflMeshSortedV2E(mesh, &vrow, &vcol);
    DflRangePush("DflMeshThermalRows");
    dfl_thermal_rows(st->N, vrow, vcol, dev->ien, dev->xg, w, dw, &st->prm, r, Kn, Cn, DflStream());
    DflRangePop();
}

void DflThermalApplyRows(Mesh3D* mesh, const f64* wgalpha, const f64* dwgalpha, f64* F) {
    ThermalState* st = st_of(mesh);
    if (!st || !F || !DflScalarAdvancesT(mesh)) return;
    const Mesh3DData* dev = Mesh3DDevice(mesh);
    const index_type *vrow, *vcol;
    DflMeshSortedV2E(mesh, &vrow, &vcol);
    DflRangePush("ThermalMaterial(F)");
    dfl_thermal_add_rows(st->N, vrow, vcol, dev->ien, dev->xg, wgalpha, dwgalpha, &st->prm, F + 5 * (size_t)st->N, DflStream());
    DflRangePop();
}
