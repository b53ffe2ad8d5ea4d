/* Melting and solidification: latent heat and mushy-zone drag (build-defined, opt-in; model in include/dedflow.h, "phase
 * change", kernels in dedflow_amd/csrc/k_phase.hip).  The reference's fluid has one phase.
 *
 * Per mesh, built by DflMeshSetPhaseChange: the configuration, the one-byte-per-tet flags (only with DFL_PHASE_FLAGS=1), the
 * nodal D, H and G the assemblies and the statistics use, and the reduction scratch.  The node pass sums in the order of the
 * mesh's sorted V2E map (DflMeshSortedV2E), which the Set call has the mesh build if nothing did before.  The kernels read
 * the node coordinates of the mesh at every call, so nothing here goes stale when the nodes move (DflMeshGeometryChanged).  A coefficient pass is one launch (two with the flags); the assembly hooks add one apply
 * launch each.  Nothing is allocated per call and only DflMeshPhaseChangeStats waits for the device.  Without a
 * configuration nothing of this exists and no call path touches it. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "dedflow.h"
#include "dedflow_kernels.h"
#include "host_private.h"

typedef struct PhaseState {
    DflPhaseChange cfg;
    dfl_phase_params prm;    /* cfg as the kernels take it */
    index_type N, T;
    u8* flag;                /* device [T] flags of the last pass (DFL_PHASE_FLAGS=1), NULL: the node pass decides itself */
    f64 *D, *H, *G;          /* device [N] each: D, H of the last assembly hook, G of the last statistics */
    f64 *work, *out;         /* device reduction scratch and the 9 statistics */
} PhaseState;

static PhaseState* st_of(const Mesh3D* mesh) {
    const MeshExt* x = (const MeshExt*)mesh->ext;
    return x ? x->phase : NULL;
}

void DflPhaseFree(PhaseState* st) {
    if (!st) return;
    HIPGUARD(hipStreamSynchronize(DflStream()));
    CdamFreeDevice(st->flag, 0);
    CdamFreeDevice(st->D, 0);
    CdamFreeDevice(st->H, 0);
    CdamFreeDevice(st->G, 0);
    CdamFreeDevice(st->work, 0);
    CdamFreeDevice(st->out, 0);
    CdamFreeHost(st, SIZE_OF(PhaseState));
}

int DflPhaseChangeCheck(const DflPhaseChange* c, char* why, size_t why_len) {
    const f64 v[] = {c->T_solidus, c->T_liquidus, c->latent, c->darcy_c, c->darcy_b, c->level, c->eps};
    const char* name[] = {"T_solidus", "T_liquidus", "latent", "darcy_c", "darcy_b", "level", "eps"};
    for (int k = 0; k < 7; ++k)
        if (!isfinite(v[k])) {
            snprintf(why, why_len, "%s is not finite (%g)", name[k], v[k]);
            return 1;
        }
    if (!(c->T_liquidus > c->T_solidus)) {
        snprintf(why, why_len, "T_liquidus must lie above T_solidus, got %g <= %g", c->T_liquidus, c->T_solidus);
        return 2;
    }
    if (c->darcy_c > 0.0 && !(c->darcy_b > 0.0)) {
        snprintf(why, why_len, "darcy_b must be positive while the drag is on, got %g", c->darcy_b);
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

void DflMeshSetPhaseChange(Mesh3D* mesh, const DflPhaseChange* cfg) {
    MeshExt* x = (MeshExt*)mesh->ext;
    x->phase_current = FALSE;
    if (!cfg) {
        DflPhaseFree(x->phase);
        x->phase = NULL;
        return;
    }
    char why[160];
    if (DflPhaseChangeCheck(cfg, why, sizeof why)) {
        fprintf(stderr, "DflMeshSetPhaseChange: %s; unchanged\n", why);
        return;
    }
    PhaseState* st = x->phase;
    const index_type N = Mesh3DNumNode(mesh), T = Mesh3DNumTet(mesh);
    const index_type *vrow, *vcol;
    DflMeshSortedV2E(mesh, &vrow, &vcol); /* built here: no coefficient pass allocates or waits */
    if (!st) {
        st = (PhaseState*)CdamMallocHost(SIZE_OF(PhaseState));
        memset(st, 0, sizeof *st);
        st->N = N;
        st->T = T;
        const ptrdiff_t nb = (ptrdiff_t)(N > 0 ? N : 1) * SIZE_OF(f64);
        st->D = (f64*)CdamMallocDevice(nb);
        st->H = (f64*)CdamMallocDevice(nb);
        st->G = (f64*)CdamMallocDevice(nb);
        st->work = (f64*)CdamMallocDevice((ptrdiff_t)dfl_phase_stats_work_size() * SIZE_OF(f64));
        st->out = (f64*)CdamMallocDevice(9 * SIZE_OF(f64));
        x->phase = st;
    }
    st->cfg = *cfg;
    const dfl_phase_params prm = {cfg->T_solidus, cfg->T_liquidus, cfg->latent, cfg->darcy_c, cfg->darcy_b,
                                  cfg->level,     (f64)cfg->side,  cfg->eps,    cfg->use_phi ? 1 : 0};
    st->prm = prm;
    const char* env = getenv("DFL_PHASE_FLAGS");
    /* off unless DFL_PHASE_FLAGS=1: most tets stay (the whole substrate is solid), so the pass in front costs more than it
       saves at bench size ("phase change"); DFL_PHASE_FLAGS=0 is the default spelled out */
    DflTetFlagsMatch(&st->flag, T, env && env[0] == '1');
    HIPGUARD(hipStreamSynchronize(DflStream()));
}

b32 DflMeshPhaseChangeEnabled(const Mesh3D* mesh) { return st_of(mesh) != NULL; }

static void coefficients(PhaseState* st, Mesh3D* mesh, const f64* w, f64* D, f64* H, f64* G) {
    const Mesh3DData* dev = Mesh3DDevice(mesh);
    hipStream_t s = DflStream();
    const index_type *vrow, *vcol;
    DflMeshSortedV2E(mesh, &vrow, &vcol);
    if (st->flag) dfl_phase_flag_tets(st->T, dev->ien, dev->xg, w, st->N, &st->prm, st->flag, s);
    dfl_phase_coefficients(st->N, vrow, vcol, dev->ien, dev->xg, w, &st->prm, st->flag, D, H, G, s);
}

void DflMeshPhaseCoefficients(Mesh3D* mesh, const f64* w, f64* D, f64* H, f64* G) {
    PhaseState* st = st_of(mesh);
    if (!st) {
        fprintf(stderr, "DflMeshPhaseCoefficients: no phase change is set on this mesh (DflMeshSetPhaseChange)\n");
        return;
    }
    if (!D && !H && !G) return;
    DflRangePush("DflMeshPhaseCoefficients");
    coefficients(st, mesh, w, D, H, G);
    DflRangePop();
}

void DflMeshPhaseChangeStats(Mesh3D* mesh, const f64* w, DflPhaseChangeStats* out) {
    PhaseState* st = st_of(mesh);
    f64 h[9] = {0.0, -HUGE_VAL, 0.0, HUGE_VAL, HUGE_VAL, HUGE_VAL, -HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    if (!st) fprintf(stderr, "DflMeshPhaseChangeStats: no phase change is set on this mesh (DflMeshSetPhaseChange)\n");
    if (st && st->N > 0) {
        hipStream_t s = DflStream();
        DflRangePush("DflMeshPhaseChangeStats");
        coefficients(st, mesh, w, NULL, NULL, st->G);
        dfl_phase_stats(st->N, Mesh3DDevice(mesh)->xg, w, st->G, &st->prm, st->work, st->out, s);
        HIPGUARD(hipMemcpyAsync(h, st->out, sizeof h, D2H, s));
        HIPGUARD(hipStreamSynchronize(s));
        DflRangePop();
    }
    out->liquid_volume = h[0];
    out->T_max = h[1];
    out->molten = (int64_t)h[2];
    for (int d = 0; d < 3; ++d) {
        out->lo[d] = h[3 + d];
        out->hi[d] = h[6 + d];
    }
}

/* D and H at the alpha states of this assembly, into the state's own buffers.  `reuse`: the caller is the Newton driver and
 * MeshExt.phase_current says whether an earlier assembly of the same alpha states left them there */
static void ensure_coefficients(Mesh3D* mesh, PhaseState* st, const f64* wgalpha, b32 reuse) {
    MeshExt* x = (MeshExt*)mesh->ext;
    if (!(reuse && x->phase_current)) coefficients(st, mesh, wgalpha, st->D, st->H, NULL);
    x->phase_current = reuse;
}

void DflPhaseApplySystem(Mesh3D* mesh, const f64* wgalpha, const f64* dwgalpha, f64* F, Matrix* J, b32 reuse) {
    PhaseState* st = st_of(mesh);
    if (!st || (!F && !J)) return;
    const b32 drag = st->cfg.darcy_c > 0.0, latent = st->cfg.latent > 0.0;
    if (!drag && !(latent && F)) return;
    hipStream_t s = DflStream();
    DflRangePush("PhaseChange(F,J)");
    ensure_coefficients(mesh, st, wgalpha, reuse);
    if (F) dfl_phase_apply_F(st->N, drag ? st->D : NULL, latent ? st->H : NULL, wgalpha, dwgalpha, F, s);
    if (J && drag) {
        value_type* val = MatrixFSBlockValues(J);
        if (!val) {
            fprintf(stderr, "DflMeshSetPhaseChange: the drag needs the block layout of the (u,p) matrix; this J keeps the "
                            "reference layout (MatrixFSUseReferenceLayout)\n");
            ASSERT(FALSE && "phase-change drag with a reference-layout FS matrix");
        }
        const CSRAttr* spy = ((MatrixFS*)J->data)->spy1x1;
        dfl_phase_apply_J(st->N, spy->row_ptr, spy->col_ind, st->D, DflMeshStepConsts(mesh)->fact2, val, s);
    }
    DflRangePop();
}

void DflPhaseApplyScalarJacobian(Mesh3D* mesh, const f64* wgalpha, const CSRAttr* attr, f64* val_T, b32 reuse) {
    PhaseState* st = st_of(mesh);
    if (!st || !val_T || !(st->cfg.latent > 0.0)) return;
    ensure_coefficients(mesh, st, wgalpha, reuse);
    dfl_phase_apply_JT(st->N, attr->row_ptr, attr->col_ind, st->H, kALPHAM, val_T, DflStream());
}
