/* Particle heat transfer (build-defined, opt-in; model in include/dedflow.h, kernels in dedflow_amd/csrc/k_heat.hip).
 * The reference's particle hooks are empty and its T equation has no source.
 *
 * State of a context with heat on (ParticleExt.heat): per particle the temperature, the energy the fluid gave it since the
 * last ParticleContextHeatSource and the last heat rate, plus two scratch arrays of the sub-step (conduction rate by id,
 * temperatures in the sweep's cell order); per node of the coupled mesh (allocated when heat or the coupling is set) the
 * source DflTimeStep registers and the share of removed particles.  A sub-step launches gather + conduction (k_p > 0) and
 * the update; it allocates nothing, waits for nothing and never writes coord / vel / acc / omega. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "dedflow.h"
#include "dedflow_kernels.h"
#include "host_private.h"

static HeatState* heat(const ParticleContext* ctx) { return ((ParticleExt*)ctx->ext)->heat; }

void DflHeatFree(ParticleContext* ctx) {
    HeatState* h = heat(ctx);
    if (!h) return;
    HIPGUARD(hipStreamSynchronize(DflStream()));
    DflParticleFieldsFree(ctx, DFL_PF_HEAT);
    CdamFreeDevice(h->source, 0); CdamFreeDevice(h->rem_q, 0);
    CdamFreeHost(h, SIZE_OF(HeatState));
    ((ParticleExt*)ctx->ext)->heat = NULL;
}

static void node_buffers(HeatState* h, index_type N);

/* e = 0, time = 0, nothing pending from removed particles */
static void clear_pending(HeatState* h, index_type P) {
    hipStream_t s = DflStream();
    HIPGUARD(hipMemsetAsync(h->e, 0, (size_t)(P > 0 ? P : 1) * sizeof(f64), s));
    if (h->rem_q) HIPGUARD(hipMemsetAsync(h->rem_q, 0, (size_t)h->N * sizeof(f64), s));
    h->rem_pending = FALSE;
    h->time = 0.0;
}

void ParticleContextSetHeat(ParticleContext* ctx, const DflParticleHeat* cfg) {
    ParticleExt* x = (ParticleExt*)ctx->ext;
    if (!cfg) {
        DflLaserFree(ctx); /* the laser heats through the heat update: it goes with it */
        DflHeatFree(ctx);
        return;
    }
    if (!(cfg->cp_p > 0.0 && isfinite(cfg->cp_p) && isfinite(cfg->T_init))) {
        fprintf(stderr, "ParticleContextSetHeat: need cp_p > 0 and a finite T_init, got %g, %g; unchanged\n", cfg->cp_p, cfg->T_init);
        return;
    }
    HeatState* h = x->heat;
    const index_type P = ctx->num_particle;
    if (!h) {
        h = (HeatState*)CdamMallocHost(SIZE_OF(HeatState));
        memset(h, 0, sizeof *h);
        x->heat = h;
        DflParticleFieldsAlloc(ctx, DFL_PF_HEAT);
    }
    h->cfg = *cfg;
    h->cp_f = cfg->cp_f > 0.0 ? cfg->cp_f : 1.0;  /* kCP, assemble.cu:36 */
    h->k_f = cfg->k_f > 0.0 ? cfg->k_f : 0.66;    /* kKAPPA */
    hipStream_t s = DflStream();
    dfl_heat_fill(0, P, cfg->T_init, h->temp, h->rate, h->e, s);
    if (x->couple) node_buffers(h, x->couple->N); /* sized here and when the coupling changes: no sub-step allocates */
    clear_pending(h, P);
}

f64* ParticleContextTemperature(ParticleContext* ctx) { return heat(ctx) ? heat(ctx)->temp : NULL; }
const f64* ParticleContextHeatRate(const ParticleContext* ctx) { return heat(ctx) ? heat(ctx)->rate : NULL; }
const f64* DflParticlePendingEnergy(const ParticleContext* ctx) { return heat(ctx) ? heat(ctx)->e : NULL; }
const f64* DflParticleConductionRate(const ParticleContext* ctx) { return heat(ctx) ? heat(ctx)->q : NULL; }

/* the per-node buffers for a mesh of N nodes (allocated once per coupled mesh) */
static void node_buffers(HeatState* h, index_type N) {
    if (h->N == N && h->source) return;
    HIPGUARD(hipStreamSynchronize(DflStream()));
    CdamFreeDevice(h->source, 0); CdamFreeDevice(h->rem_q, 0);
    h->source = (f64*)CdamMallocDevice((ptrdiff_t)(N > 0 ? N : 1) * SIZE_OF(f64));
    h->rem_q = (f64*)CdamMallocDevice((ptrdiff_t)(N > 0 ? N : 1) * SIZE_OF(f64));
    HIPGUARD(hipMemsetAsync(h->rem_q, 0, (size_t)(N > 0 ? N : 1) * sizeof(f64), DflStream()));
    h->N = N;
    h->rem_pending = FALSE;
}

void DflHeatCouplingChanged(ParticleContext* ctx) {
    HeatState* h = heat(ctx);
    if (!h) return;
    const CoupleState* c = ((ParticleExt*)ctx->ext)->couple;
    if (c) node_buffers(h, c->N);
    clear_pending(h, ctx->num_particle);
    DflLaserCouplingChanged(ctx); /* the substrate of the new mesh; a no-op without a laser */
}

void DflHeatStep(ParticleContext* ctx, const f64* w) {
    ParticleExt* x = (ParticleExt*)ctx->ext;
    HeatState* h = x->heat;
    const index_type P = ctx->num_particle;
    hipStream_t s = DflStream();
    if (x->laser) DflLaserStep(ctx, x->dt); /* the absorbed power of this sub-step, before the update that spends it */
    DflRangePush("ParticleContextHeatStep");
    int slot = DflProfileBegin(DFL_TAG_SMALL + 5);
    const b32 conduct = h->cfg.k_p > 0.0 && P > 0;
    if (conduct) {
        const f64 R = x->radius ? x->rmax : ParticleRadius(ctx);
        dfl_heat_gather(P, x->order, h->temp, h->sorted_t, s);
        if (x->walls)
            dfl_heat_conduction_grid(P, x->sorted, R, DflSizes(x), *DflWallsParticleGrid(ctx), x->order, x->cell_start, h->sorted_t,
                                     h->cfg.k_p, h->q, s);
        else
            dfl_heat_conduction(P, x->sorted, R, DflSizes(x), x->cell, x->ncell, x->order, x->cell_start, h->sorted_t, h->cfg.k_p,
                                h->q, s);
    }
    CoupleState* c = w ? x->couple : NULL;
    const f64 rho_f = c ? c->cfg.rho_f : 0.0, mu_f = c ? c->cfg.mu_f : 1.0;
    const f64 pr13 = cbrt(h->cp_f * mu_f / h->k_f);
    dfl_heat_update(P, c ? c->tet : NULL, c ? c->lambda : NULL, c ? Mesh3DDevice(c->mesh)->ien : NULL, c ? w : NULL, c ? c->N : 0,
                    ParticleMass(ctx), ParticleRadius(ctx), x->mass, x->radius, ArrayData(ParticleCTXDeviceVel(ctx)), h->cfg.cp_p,
                    h->k_f, rho_f, mu_f, pr13, x->dt, conduct ? h->q : NULL, ParticleContextLaserRate(ctx), h->temp, h->rate, h->e, s);
    if (c) h->time += x->dt;
    DflProfileEnd(slot);
    DflRangePop();
}

void ParticleContextHeatStep(ParticleContext* ctx, const f64* w) {
    ParticleExt* x = (ParticleExt*)ctx->ext;
    ASSERT(x->heat && "ParticleContextHeatStep: heat is off (ParticleContextSetHeat)");
    if (!x->heat) return;
    /* a bare call brings its own geometry: the cell sort when no sweep is valid for these particles (never the forces), and
       the particles' tets at their current positions */
    if (x->heat->cfg.k_p > 0.0 && !(x->order_valid && x->sort_valid && x->cap_particle >= ctx->num_particle)) DflDemBuildCells(ctx);
    if (w && x->couple) ParticleContextLocate(ctx);
    DflHeatStep(ctx, w);
}

b32 DflHeatPending(const ParticleContext* ctx) {
    const HeatState* h = heat(ctx);
    return h && ((ParticleExt*)ctx->ext)->couple && (h->time > 0.0 || DflLaserPending(ctx));
}

void ParticleContextHeatSource(ParticleContext* ctx, f64* q) {
    ParticleExt* x = (ParticleExt*)ctx->ext;
    HeatState* h = x->heat;
    CoupleState* c = x->couple;
    ASSERT(h && c && "ParticleContextHeatSource: needs heat on and a coupled context");
    if (!h || !c) return;
    hipStream_t s = DflStream();
    if (h->time <= 0.0) {
        HIPGUARD(hipMemsetAsync(q, 0, (size_t)c->N * sizeof(f64), s));
        DflLaserAddSource(ctx, q); /* the laser's substrate power of bare laser steps or uncoupled sub-steps */
        return;
    }
    DflRangePush("ParticleContextHeatSource");
    const index_type P = ctx->num_particle;
    DflCoupleNodeScatter(ctx, c->tet, h->e, 1, 1.0 / h->time, q);
    if (h->rem_pending) { /* the energy of the particles removed since the last call */
        dfl_daxpy(c->N, 1.0 / h->time, h->rem_q, q, s);
        HIPGUARD(hipMemsetAsync(h->rem_q, 0, (size_t)c->N * sizeof(f64), s));
        h->rem_pending = FALSE;
    }
    HIPGUARD(hipMemsetAsync(h->e, 0, (size_t)(P > 0 ? P : 1) * sizeof(f64), s));
    h->time = 0.0;
    DflLaserAddSource(ctx, q); /* + the substrate's laser energy / its time; a no-op without a laser */
    DflRangePop();
}

void DflHeatAccumulateRemoved(ParticleContext* ctx, const index_type* rtet) {
    ParticleExt* x = (ParticleExt*)ctx->ext;
    HeatState* h = x->heat;
    CoupleState* c = x->couple;
    hipStream_t s = DflStream();
    /* the pattern of the source, restricted to the removed particles: rem_tmp = -sum lambda e, then rem_q += it */
    DflCoupleNodeScatter(ctx, rtet, h->e, 1, 1.0, c->rem_tmp);
    dfl_daxpy(c->N, 1.0, c->rem_tmp, h->rem_q, s);
    h->rem_pending = TRUE;
}

b32 DflParticleHeatTwoWay(const ParticleContext* ctx) { return heat(ctx) ? heat(ctx)->cfg.two_way : FALSE; }

f64* DflParticlePendingHeatSource(ParticleContext* ctx) {
    HeatState* h = heat(ctx);
    if (!DflHeatPending(ctx)) return NULL;
    ParticleContextHeatSource(ctx, h->source);
    return h->source;
}

void DflHeatCopy(ParticleContext* dst, const ParticleContext* src) {
    const HeatState* hs = heat(src);
    if (!hs) {
        if (heat(dst)) ParticleContextSetHeat(dst, NULL);
        return;
    }
    ParticleContextSetHeat(dst, &hs->cfg);
    HeatState* hd = heat(dst);
    const size_t bytes = (size_t)src->num_particle * sizeof(f64);
    hipStream_t s = DflStream();
    if (bytes) {
        HIPGUARD(hipMemcpyAsync(hd->temp, hs->temp, bytes, D2D, s));
        HIPGUARD(hipMemcpyAsync(hd->e, hs->e, bytes, D2D, s));
        HIPGUARD(hipMemcpyAsync(hd->rate, hs->rate, bytes, D2D, s));
    }
    hd->time = hs->time;
    if (hs->rem_pending && ((ParticleExt*)dst->ext)->couple && ((ParticleExt*)dst->ext)->couple->N == hs->N) {
        node_buffers(hd, hs->N);
        HIPGUARD(hipMemcpyAsync(hd->rem_q, hs->rem_q, (size_t)hs->N * sizeof(f64), D2D, s));
        hd->rem_pending = TRUE;
    }
}
