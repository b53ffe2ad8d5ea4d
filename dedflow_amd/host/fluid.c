/* Fluid material: density, viscosity and body force of the (u,p) rows follow phi and T (build-defined, opt-in; model in
 * include/dedflow.h, "fluid material", kernels in dedflow_amd/csrc/k_fluid.hip).  The reference's momentum rows belong to one
 * fluid without weight.
 *
 * Per mesh, built by DflMeshSetFluidMaterial: the configuration and its kernel form.  Both passes sum in the order of the
 * mesh's sorted V2E map (DflMeshSortedV2E), which the Set call has the mesh build if nothing did before, and add straight
 * into F and into the block values of J, so the state owns no device buffer; the kernels read the node coordinates at every
 * call, so nothing here goes stale when the nodes move.  The F hook is one launch and the J hook is one launch.  Nothing is
 * allocated per call and nothing waits for the device.  Without a configuration nothing of this exists and no call path
 * touches it. */
#include <math.h>
#include <stdio.h>
#include <string.h>
#include "dedflow.h"
#include "dedflow_kernels.h"
#include "host_private.h"

typedef struct FluidState {
    DflFluidMaterial cfg;
    dfl_fluid_params prm; /* cfg as the kernels take it */
    index_type N;
} FluidState;

static FluidState* st_of(const Mesh3D* mesh) {
    const MeshExt* x = (const MeshExt*)mesh->ext;
    return x ? x->fluid : NULL;
}

void DflFluidFree(FluidState* st) {
    if (!st) return;
    HIPGUARD(hipStreamSynchronize(DflStream())); /* a launch in flight holds the parameters by value, but the V2E map by pointer */
    CdamFreeHost(st, SIZE_OF(FluidState));
}

int DflFluidMaterialCheck(const DflFluidMaterial* c, char* why, size_t why_len) {
    const f64 v[] = {c->rho_gas,    c->rho_metal,  c->mu_gas, c->mu_metal, c->gravity[0], c->gravity[1],
                     c->gravity[2], c->beta,       c->T_ref,  c->level,    c->eps};
    const char* name[] = {"rho_gas",    "rho_metal", "mu_gas", "mu_metal", "gravity[0]", "gravity[1]",
                          "gravity[2]", "beta",      "T_ref",  "level",    "eps"};
    for (int k = 0; k < 11; ++k)
        if (!isfinite(v[k])) {
            snprintf(why, why_len, "%s is not finite (%g)", name[k], v[k]);
            return 1;
        }
    for (int k = 0; k < 4; ++k)
        if (!(v[k] > 0.0)) {
            snprintf(why, why_len, "%s must be positive, got %g", name[k], v[k]);
            return 2;
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

void DflMeshSetFluidMaterial(Mesh3D* mesh, const DflFluidMaterial* cfg) {
    MeshExt* x = (MeshExt*)mesh->ext;
    if (!cfg) {
        DflFluidFree(x->fluid);
        x->fluid = NULL;
        return;
    }
    char why[200];
    if (DflFluidMaterialCheck(cfg, why, sizeof why)) {
        fprintf(stderr, "DflMeshSetFluidMaterial: %s; unchanged\n", why);
        return;
    }
    FluidState* st = x->fluid;
    const index_type *vrow, *vcol;
    DflMeshSortedV2E(mesh, &vrow, &vcol); /* built here: no later call allocates or waits */
    if (!st) {
        st = (FluidState*)CdamMallocHost(SIZE_OF(FluidState));
        memset(st, 0, sizeof *st);
        st->N = Mesh3DNumNode(mesh);
        x->fluid = st;
    }
    st->cfg = *cfg;
    const dfl_fluid_params prm = {cfg->rho_gas, cfg->rho_metal, cfg->mu_gas, cfg->mu_metal,
                                  {cfg->gravity[0], cfg->gravity[1], cfg->gravity[2]},
                                  cfg->beta,    cfg->T_ref,     cfg->level,  (f64)cfg->side, cfg->eps, cfg->use_phi ? 1 : 0};
    st->prm = prm;
    HIPGUARD(hipStreamSynchronize(DflStream()));
}

b32 DflMeshFluidMaterialEnabled(const Mesh3D* mesh) { return st_of(mesh) != NULL; }
const DflFluidMaterial* DflFluidConfig(const Mesh3D* mesh) { return st_of(mesh) ? &st_of(mesh)->cfg : NULL; }

void DflMeshFluidRows(Mesh3D* mesh, const f64* w, const f64* dw, f64* r, f64* Rn, f64* Mn) {
    FluidState* st = st_of(mesh);
    if (!st) {
        fprintf(stderr, "DflMeshFluidRows: no fluid material is set on this mesh (DflMeshSetFluidMaterial)\n");
        return;
    }
    if (!r && !Rn && !Mn) return;
    const Mesh3DData* dev = Mesh3DDevice(mesh);
    const index_type *vrow, *vcol;
    DflMeshSortedV2E(mesh, &vrow, &vcol);
    DflRangePush("DflMeshFluidRows");
    dfl_fluid_rows_dt(st->N, vrow, vcol, dev->ien, dev->xg, w, dw, &st->prm, r, Rn, Mn, DflMeshStepConsts(mesh), DflStream());
    DflRangePop();
}

void DflFluidApplySystem(Mesh3D* mesh, const f64* wgalpha, const f64* dwgalpha, f64* F, Matrix* J) {
    FluidState* st = st_of(mesh);
    if (!st || (!F && !J)) return;
    const Mesh3DData* dev = Mesh3DDevice(mesh);
    const index_type *vrow, *vcol;
    DflMeshSortedV2E(mesh, &vrow, &vcol);
    DflRangePush("FluidMaterial(F,J)");
    if (F) dfl_fluid_add_rows_dt(st->N, vrow, vcol, dev->ien, dev->xg, wgalpha, dwgalpha, &st->prm, F, DflMeshStepConsts(mesh), DflStream());
    if (J) {
        value_type* val = MatrixFSBlockValues(J);
        if (!val) {
            fprintf(stderr, "DflMeshSetFluidMaterial: the Jacobian correction needs the block layout of the (u,p) matrix; this J "
                            "keeps the reference layout (MatrixFSUseReferenceLayout)\n");
            ASSERT(FALSE && "fluid material with a reference-layout FS matrix");
        }
        const CSRAttr* spy = ((MatrixFS*)J->data)->spy1x1;
        dfl_fluid_add_jacobian_dt(st->N, vrow, vcol, dev->ien, dev->xg, wgalpha, spy->row_ptr, spy->col_ind, &st->prm, val,
                                  DflMeshStepConsts(mesh), DflStream());
    }
    DflRangePop();
}
