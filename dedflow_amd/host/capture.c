/* Melt-pool capture (build-defined, opt-in; model in include/dedflow.h, kernels in dedflow_amd/csrc/k_capture.hip and the
 * <5> node pass of k_couple.hip).  The reference's particle hooks are empty and its continuity rows have no source.
 *
 * State of a context with capture on (ParticleExt.capture): the configuration, one per-particle scratch array (the
 * deposits of the last call, a row of host/pfields.c) and per node of the coupled mesh the accumulator A[N][5], one call's
 * node sums and the three buffers DflTimeStep registers.  A capture call is a ParticleContextRemove with another flag
 * kernel plus one sort and one node pass: it reads the new count back (4 bytes), allocates nothing, and stops there when
 * nothing was captured. */
#include <math.h>
#include <stdio.h>
#include <string.h>
#include "dedflow.h"
#include "dedflow_kernels.h"
#include "host_private.h"

static CaptureState* state(const ParticleContext* ctx) { return ((ParticleExt*)ctx->ext)->capture; }

static void free_node_buffers(CaptureState* k) {
    CdamFreeDevice(k->A, 0); CdamFreeDevice(k->A_tmp, 0);
    CdamFreeDevice(k->q_vol, 0); CdamFreeDevice(k->load, 0); CdamFreeDevice(k->q_heat, 0);
    k->A = k->A_tmp = k->q_vol = k->load = k->q_heat = NULL;
    k->N = 0;
}

void DflCaptureFree(ParticleContext* ctx) {
    CaptureState* k = state(ctx);
    if (!k) return;
    HIPGUARD(hipStreamSynchronize(DflStream()));
    DflParticleFieldsFree(ctx, DFL_PF_CAPTURE);
    free_node_buffers(k);
    CdamFreeHost(k, SIZE_OF(CaptureState));
    ((ParticleExt*)ctx->ext)->capture = NULL;
}

/* the per-node buffers for a mesh of N nodes, A zero and nothing pending */
static void node_buffers(CaptureState* k, index_type N) {
    const ptrdiff_t n = N > 0 ? N : 1;
    if (k->N != N || !k->A) {
        HIPGUARD(hipStreamSynchronize(DflStream()));
        free_node_buffers(k);
        k->A = (f64*)CdamMallocDevice(n * 5 * SIZE_OF(f64));
        k->A_tmp = (f64*)CdamMallocDevice(n * 5 * SIZE_OF(f64));
        k->q_vol = (f64*)CdamMallocDevice(n * SIZE_OF(f64));
        k->load = (f64*)CdamMallocDevice(n * 3 * SIZE_OF(f64));
        k->q_heat = (f64*)CdamMallocDevice(n * SIZE_OF(f64));
        k->N = N;
    }
    HIPGUARD(hipMemsetAsync(k->A, 0, (size_t)n * 5 * sizeof(f64), DflStream()));
    k->pending = k->heat_pending = FALSE;
}

void ParticleContextSetCapture(ParticleContext* ctx, const DflParticleCapture* cfg) {
    ParticleExt* x = (ParticleExt*)ctx->ext;
    if (!cfg) {
        DflCaptureFree(ctx);
        return;
    }
    if (!((cfg->side == 1 || cfg->side == -1) && cfg->reach >= 0.0 && isfinite(cfg->reach))) {
        fprintf(stderr, "ParticleContextSetCapture: need side +1 or -1 and a finite reach >= 0, got %d, %g; unchanged\n", (int)cfg->side,
                cfg->reach);
        return;
    }
    if (!x->couple) {
        fprintf(stderr, "ParticleContextSetCapture: the context is not coupled to a mesh (ParticleContextSetFluidCoupling); unchanged\n");
        return;
    }
    CaptureState* k = x->capture;
    if (!k) {
        k = (CaptureState*)CdamMallocHost(SIZE_OF(CaptureState));
        memset(k, 0, sizeof *k);
        x->capture = k;
        DflParticleFieldsAlloc(ctx, DFL_PF_CAPTURE);
        node_buffers(k, x->couple->N);
    }
    k->cfg = *cfg;
    DflFlowState(ctx);        /* the tags and the compaction's scratch, as the first Set*flow call */
    DflFlowEnsureSpares(ctx); /* sized here: no capture call allocates */
}

b32 DflParticleCaptureOn(const ParticleContext* ctx) { return state(ctx) != NULL; }

void DflCaptureCouplingChanged(ParticleContext* ctx) {
    CaptureState* k = state(ctx);
    const CoupleState* c = ((ParticleExt*)ctx->ext)->couple;
    if (k && c) node_buffers(k, c->N); /* uncoupled: capture calls do nothing until the context is coupled again */
}

index_type ParticleContextCapture(ParticleContext* ctx, const f64* w) {
    ParticleExt* x = (ParticleExt*)ctx->ext;
    CaptureState* k = x->capture;
    CoupleState* c = x->couple;
    if (!k || !c || k->N != c->N) return 0;
    FlowState* f = x->flow;
    k->stats.last = 0;
    ParticleContextLocate(ctx);
    const index_type P = ctx->num_particle;
    if (P <= 0) return 0;
    DflRangePush("ParticleContextCapture");
    hipStream_t s = DflStream();
    DflFlowEnsureSpares(ctx);
    const Mesh3DData* dev = Mesh3DDevice(c->mesh);
    const HeatState* h = x->heat;
    dfl_capture_flag(P, c->tet, c->lambda, dev->ien, dev->xg, w, c->N, ArrayData(ParticleCTXDeviceVel(ctx)), h ? h->temp : NULL,
                     ParticleMass(ctx), ParticleRadius(ctx), x->mass, x->radius, c->cfg.rho_f, h ? h->cfg.cp_p : 0.0, k->cfg.level,
                     (f64)k->cfg.side, k->cfg.reach, k->cfg.T_melt, f->keep, f->rtet, k->dep, s);
    dfl_exclusive_scan_i32(P, f->keep, f->newid, f->scan_tmp, f->scan_bytes, s);
    const index_type Pn = DflReadDeviceIndex(f->newid + P);
    if (Pn == P) {
        DflRangePop();
        return 0;
    }
    /* before the compaction moves imp, e and lambda: what was pending on the captured particles goes where
       ParticleContextRemove sends it, then their deposits to the nodes, one sort and one pass for the five components */
    if (c->imp_time > 0.0) DflCoupleAccumulateRemoved(ctx, f->rtet);
    if (DflHeatPending(ctx) && h->time > 0.0) DflHeatAccumulateRemoved(ctx, f->rtet);
    dfl_couple_sort_by_tet(P, c->T, f->rtet, c->tcount, c->rank, c->tstart, c->slot, c->members, c->scan_tmp, c->scan_bytes, s);
    const index_type *vrow, *vcol;
    DflMeshSortedV2E(c->mesh, &vrow, &vcol);
    dfl_couple_node_deposit(c->N, vrow, vcol, dev->ien, c->tstart, c->members, c->lambda, k->dep, -1.0, k->A_tmp, s);
    dfl_daxpy(5 * c->N, 1.0, k->A_tmp, k->A, s);
    k->pending = TRUE;
    if (h) k->heat_pending = TRUE;
    DflFlowCompact(ctx, Pn);
    k->stats.last = P - Pn;
    k->stats.captured += P - Pn;
    DflRangePop();
    return P - Pn;
}

void ParticleContextCaptureSource(ParticleContext* ctx, f64 time, f64* q_vol, f64* load, f64* q_heat) {
    CaptureState* k = state(ctx);
    ASSERT(k && "ParticleContextCaptureSource: capture is off (ParticleContextSetCapture)");
    ASSERT(time > 0.0 && "ParticleContextCaptureSource: the time window must be positive");
    if (!k || !(time > 0.0)) return;
    hipStream_t s = DflStream();
    const size_t N = (size_t)k->N;
    if (!k->pending) {
        if (q_vol) HIPGUARD(hipMemsetAsync(q_vol, 0, N * sizeof(f64), s));
        if (load) HIPGUARD(hipMemsetAsync(load, 0, N * 3 * sizeof(f64), s));
        if (q_heat) HIPGUARD(hipMemsetAsync(q_heat, 0, N * sizeof(f64), s));
        return;
    }
    dfl_capture_source(k->N, k->A, time, q_vol, load, q_heat, s);
    HIPGUARD(hipMemsetAsync(k->A, 0, (N > 0 ? N : 1) * 5 * sizeof(f64), s));
    k->pending = k->heat_pending = FALSE;
}

b32 DflCaptureTakePending(ParticleContext* ctx, f64 time, f64** q_vol, f64** load, f64** q_heat) {
    CaptureState* k = state(ctx);
    if (!k || !k->cfg.two_way || !k->pending) return FALSE;
    *q_vol = k->q_vol;
    *load = k->load;
    *q_heat = k->heat_pending ? k->q_heat : NULL;
    ParticleContextCaptureSource(ctx, time, *q_vol, *load, *q_heat);
    return TRUE;
}

void ParticleContextCaptureStats(const ParticleContext* ctx, DflParticleCaptureStats* out) {
    const CaptureState* k = state(ctx);
    if (k) *out = k->stats;
    else memset(out, 0, sizeof *out);
}

void DflCaptureCopy(ParticleContext* dst, const ParticleContext* src) {
    const CaptureState* ks = state(src);
    if (!ks) {
        if (state(dst)) ParticleContextSetCapture(dst, NULL);
        return;
    }
    /* the configuration only: what is pending in src stays there.  An uncoupled dst cannot capture and stays as it is */
    if (((ParticleExt*)dst->ext)->couple) ParticleContextSetCapture(dst, &ks->cfg);
}
