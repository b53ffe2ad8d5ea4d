/* Solid-surface contact (build-defined, opt-in; model in include/dedflow.h, kernel in dedflow_amd/csrc/k_surface_contact.hip).
 * The reference's particle hooks are empty; its particles never meet the level set.
 *
 * State of a context with the contact on (ParticleExt.surface_contact): the configuration, 16 KiB of device counters with
 * a host copy for the Stats call, and one number on the device computed from the coupled mesh, grad_max >= |grad N_k| over
 * its tets, which lets the kernel drop a particle far on the gas side before it gathers T and the coordinates.  grad_max is
 * one pass over the tets (dfl_surface_grad_max) at Set, when the coupling changes, and in the first sub-step after
 * DflMeshGeometryChanged.  A sub-step is one launch (two and a memset in that first sub-step): nothing is allocated or copied
 * and nothing waits for the device; only ParticleContextSurfaceContactStats reads the counters. */
#include <math.h>
#include <stdio.h>
#include <string.h>
#include "dedflow.h"
#include "dedflow_kernels.h"
#include "host_private.h"

static SurfaceContactState* state(const ParticleContext* ctx) { return ((ParticleExt*)ctx->ext)->surface_contact; }

int DflSurfaceContactCheck(const DflSurfaceContact* c, char* why, size_t why_len) {
    if (!(c->side == 1 || c->side == -1)) {
        snprintf(why, why_len, "side must be +1 or -1, got %d", (int)c->side);
        return 1;
    }
    if (!isfinite(c->level)) {
        snprintf(why, why_len, "level must be finite, got %g", c->level);
        return 2;
    }
    if (isnan(c->T_solid)) {
        snprintf(why, why_len, "T_solid must not be a NaN (HUGE_VAL: contact everywhere)");
        return 3;
    }
    return 0;
}

void DflSurfaceContactFree(ParticleContext* ctx) {
    SurfaceContactState* k = state(ctx);
    if (!k) return;
    HIPGUARD(hipStreamSynchronize(DflStream()));
    CdamFreeDevice(k->cnt, 0);
    CdamFreeDevice(k->grad_max, 0);
    CdamFreeHost(k->host, SIZE_OF(dfl_surface_counters));
    CdamFreeHost(k, SIZE_OF(SurfaceContactState));
    ((ParticleExt*)ctx->ext)->surface_contact = NULL;
}

/* the bound of the early exit for this mesh as it is now: a memset and one launch over the tets, nothing waits */
static void mesh_bound(SurfaceContactState* k, Mesh3D* mesh) {
    const Mesh3DData* dev = Mesh3DDevice(mesh);
    k->geom_epoch = ((MeshExt*)mesh->ext)->geom_epoch;
    dfl_surface_grad_max(Mesh3DNumTet(mesh), dev->ien, dev->xg, k->grad_max, DflStream());
}

void ParticleContextSetSurfaceContact(ParticleContext* ctx, const DflSurfaceContact* cfg) {
    ParticleExt* x = (ParticleExt*)ctx->ext;
    if (!cfg) {
        DflSurfaceContactFree(ctx);
        return;
    }
    char why[160];
    if (DflSurfaceContactCheck(cfg, why, sizeof why)) {
        fprintf(stderr, "ParticleContextSetSurfaceContact: %s; unchanged\n", why);
        return;
    }
    if (!x->couple) {
        fprintf(stderr, "ParticleContextSetSurfaceContact: the context is not coupled to a mesh (ParticleContextSetFluidCoupling); unchanged\n");
        return;
    }
    SurfaceContactState* k = x->surface_contact;
    if (!k) {
        k = (SurfaceContactState*)CdamMallocHost(SIZE_OF(SurfaceContactState));
        memset(k, 0, sizeof *k);
        k->cnt = (dfl_surface_counters*)CdamMallocDevice(SIZE_OF(dfl_surface_counters));
        k->host = (dfl_surface_counters*)CdamMallocHost(SIZE_OF(dfl_surface_counters));
        k->grad_max = (f64*)CdamMallocDevice(SIZE_OF(f64));
        x->surface_contact = k;
        mesh_bound(k, x->couple->mesh);
    }
    k->cfg = *cfg;
    k->cur = 0;
    HIPGUARD(hipMemsetAsync(k->cnt, 0, sizeof(dfl_surface_counters), DflStream()));
}

b32 DflParticleSurfaceContactOn(const ParticleContext* ctx) { return state(ctx) != NULL; }

void DflSurfaceContactCouplingChanged(ParticleContext* ctx) {
    SurfaceContactState* k = state(ctx);
    if (!k) return;
    const CoupleState* c = ((ParticleExt*)ctx->ext)->couple;
    if (!c) DflSurfaceContactFree(ctx);
    else mesh_bound(k, c->mesh);
}

void DflSurfaceContactApply(ParticleContext* ctx, const f64* w) {
    ParticleExt* x = (ParticleExt*)ctx->ext;
    SurfaceContactState* k = x->surface_contact;
    CoupleState* c = x->couple;
    if (!k || !c) return;
    if (k->geom_epoch != ((MeshExt*)c->mesh->ext)->geom_epoch) mesh_bound(k, c->mesh); /* the nodes moved */
    const Mesh3DData* dev = Mesh3DDevice(c->mesh);
    k->cur = 1 - k->cur;
    int slot = DflProfileBegin(DFL_TAG_SMALL + 6);
    dfl_surface_contact(ctx->num_particle, c->tet, c->lambda, dev->ien, dev->xg, w, c->N, ArrayData(ParticleCTXDeviceVel(ctx)),
                        x->omega, ParticleMass(ctx), ParticleRadius(ctx), DflSizes(x), x->kn, x->gamma_n, DflFrictionLaw(ctx),
                        k->cfg.level, (f64)k->cfg.side, k->cfg.T_solid, k->grad_max, DflFrictionHistoryCurrent(x), k->cnt, k->cur,
                        ArrayData(ParticleCTXDeviceAcc(ctx)), x->alpha, DflStream());
    DflProfileEnd(slot);
}

void DflSurfaceContactTestNoEarlyExit(ParticleContext* ctx) {
    SurfaceContactState* k = state(ctx);
    if (k) HIPGUARD(hipMemsetAsync(k->grad_max, 0, sizeof(f64), DflStream())); /* 0: "not known", nothing leaves early */
}

void ParticleContextSurfaceContactStats(const ParticleContext* ctx, DflSurfaceContactStats* out) {
    const SurfaceContactState* k = state(ctx);
    memset(out, 0, sizeof *out);
    if (!k) return;
    const dfl_surface_counters* h = k->host;
    HIPGUARD(hipStreamSynchronize(DflStream()));
    HIPGUARD(hipMemcpy(k->host, k->cnt, sizeof *h, D2H));
    for (int s = 0; s < DFL_SURFACE_SLOTS; ++s) {
        const unsigned long long c = h->step[k->cur][s * DFL_SURFACE_SLOT_STRIDE];
        out->last += (index_type)(c & 0xffffffffull);
        out->buried += (index_type)(c >> 32);
    }
    out->total = (int64_t)h->total + out->last; /* the last launch folded every earlier sub-step into total */
}

void DflSurfaceContactCopy(ParticleContext* dst, const ParticleContext* src) {
    const SurfaceContactState* ks = state(src);
    if (!ks) {
        if (state(dst)) ParticleContextSetSurfaceContact(dst, NULL);
        return;
    }
    /* the configuration only; an uncoupled dst cannot collide with a surface and stays as it is */
    if (((ParticleExt*)dst->ext)->couple) ParticleContextSetSurfaceContact(dst, &ks->cfg);
}
