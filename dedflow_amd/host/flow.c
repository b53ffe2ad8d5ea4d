/* Particle inflow and outflow: ParticleContextAdd and ParticleContextRemove (build-defined: empty hooks in the reference,
 * Particle.c:120-130; model in include/dedflow.h, kernels in dedflow_amd/csrc/k_flow.hip).
 *
 * Every per-particle buffer of a context is sized to its capacity x->cap >= num_particle; which buffers there are is the
 * table of host/pfields.c, and nothing here names a field of another feature.  Remove scatters the survivors of every
 * carried field into spare buffers of the same capacity and swaps the pointers (the friction history into the other ping-pong row
 * set, which flips); Add appends in place after growing the capacity by x1.5 when it must.  Each call reads the new count
 * back (4 bytes) and allocates nothing unless the capacity grows. */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "dedflow.h"
#include "dedflow_kernels.h"
#include "host_private.h"

static void free_slots(FlowState* f) {
    CdamFreeDevice(f->blocked, 0); CdamFreeDevice(f->slot, 0); CdamFreeDevice(f->slot_out, 0);
    CdamFreeDevice(f->key, 0); CdamFreeDevice(f->key_out, 0); CdamFreeDevice(f->sort_tmp, 0);
    f->blocked = f->slot = f->slot_out = NULL;
    f->key = f->key_out = NULL;
    f->sort_tmp = NULL;
}

static void free_spares(FlowState* f) {
    for (int e = 0; e < DFL_FLOW_MAX_FIELDS; ++e) {
        CdamFreeDevice(f->spare[e], 0);
        f->spare[e] = NULL;
    }
}

/* the spare a compaction writes `row` into: one of the row's element size that no earlier row of this walk took (bit e of
 * *taken: spare e is taken), allocated at the context's capacity when there is none */
static void** spare_of(FlowState* f, const DflPField* row, index_type cap, unsigned* taken) {
    int e = 0, empty = -1;
    for (; e < DFL_FLOW_MAX_FIELDS; ++e) {
        if (f->spare[e] && f->spare_bytes[e] == row->bytes && !(*taken >> e & 1)) break;
        if (!f->spare[e] && empty < 0) empty = e;
    }
    if (e == DFL_FLOW_MAX_FIELDS) {
        ASSERT(empty >= 0 && "more carried per-particle fields than DFL_FLOW_MAX_FIELDS");
        e = empty;
        f->spare[e] = DflParticleFieldAlloc(row, cap);
        f->spare_bytes[e] = row->bytes;
    }
    *taken |= 1u << e;
    return &f->spare[e];
}

/* the spares the next compaction writes, for the state that is on now */
void DflFlowEnsureSpares(ParticleContext* ctx) {
    ParticleExt* x = (ParticleExt*)ctx->ext;
    DflPField rows[DFL_PF_MAX_ROWS];
    const int nrow = DflParticleFields(ctx, DflParticleLiveFeatures(ctx), rows);
    unsigned taken = 0;
    for (int r = 0; r < nrow; ++r)
        if (rows[r].kind == DFL_PF_CARRIED) spare_of(x->flow, &rows[r], x->cap, &taken);
}

static void alloc_scan(FlowState* f, index_type cap) {
    f->scan_bytes = dfl_scan_temp_bytes(cap > 0 ? cap : 1);
    f->scan_tmp = CdamMallocDevice((ptrdiff_t)f->scan_bytes);
}

void DflFlowFree(ParticleContext* ctx) {
    FlowState* f = ((ParticleExt*)ctx->ext)->flow;
    if (!f) return;
    HIPGUARD(hipStreamSynchronize(DflStream()));
    free_slots(f);
    free_spares(f);
    DflParticleFieldsFree(ctx, DFL_PF_FLOW);
    CdamFreeDevice(f->scan_tmp, 0); CdamFreeDevice(f->count, 0);
    CdamFreeHost(f, SIZE_OF(FlowState));
    ((ParticleExt*)ctx->ext)->flow = NULL;
}

/* the flow state of a context: created (tags 0 .. P-1) at the first Set call */
FlowState* DflFlowState(ParticleContext* ctx) {
    ParticleExt* x = (ParticleExt*)ctx->ext;
    if (x->flow) return x->flow;
    const index_type P = ctx->num_particle;
    FlowState* f = (FlowState*)CdamMallocHost(SIZE_OF(FlowState));
    memset(f, 0, sizeof *f);
    x->flow = f;
    DflParticleFieldsAlloc(ctx, DFL_PF_FLOW);
    f->count = (index_type*)CdamMallocDevice(SIZE_OF(index_type));
    alloc_scan(f, x->cap);
    int64_t* h = (int64_t*)malloc((size_t)(P > 0 ? P : 1) * sizeof(int64_t));
    for (index_type i = 0; i < P; ++i) h[i] = i;
    HIPGUARD(hipStreamSynchronize(DflStream()));
    if (P > 0) HIPGUARD(hipMemcpy(f->tag, h, (size_t)P * sizeof(int64_t), H2D));
    free(h);
    f->next_tag = P;
    return f;
}

/* capacity >= need: every buffer sized by the particle count, the live entries carried */
static void grow(ParticleContext* ctx, index_type need) {
    ParticleExt* x = (ParticleExt*)ctx->ext;
    FlowState* f = x->flow;
    if (need <= x->cap) return;
    const int64_t want = (int64_t)x->cap + x->cap / 2;
    const index_type cap = want > need ? (want < INT32_MAX / DFL_DEM_MAX_HISTORY ? (index_type)want : need) : need;
    const index_type P = ctx->num_particle;
    hipStream_t s = DflStream();
    HIPGUARD(hipStreamSynchronize(s));
    DflPField rows[DFL_PF_MAX_ROWS];
    const int nrow = DflParticleFields(ctx, DflParticleLiveFeatures(ctx), rows);
    for (int r = 0; r < nrow; ++r) { /* stream-ordered: the copy, then the old buffer goes */
        void* old = *rows[r].ptr;
        *rows[r].ptr = DflParticleFieldAlloc(&rows[r], cap);
        if (rows[r].kind != DFL_PF_SCRATCH && P > 0)
            HIPGUARD(hipMemcpyAsync(*rows[r].ptr, old, (size_t)P * rows[r].bytes, hipMemcpyDeviceToDevice, s));
        CdamFreeDevice(old, 0);
    }
    for (int k = 0; k < 3; ++k) {
        Array* h = ctx->h_arr[k];
        f64* hd = (f64*)CdamMallocHost((ptrdiff_t)cap * 3 * SIZE_OF(f64));
        memset(hd, 0, (size_t)cap * 3 * sizeof(f64));
        if (P > 0) memcpy(hd, h->data, (size_t)P * 3 * sizeof(f64));
        CdamFreeHost(h->data, (ptrdiff_t)x->cap * 3 * SIZE_OF(f64));
        h->data = hd;
    }
    CdamFreeDevice(f->scan_tmp, 0);
    alloc_scan(f, cap);
    free_spares(f);
    x->cap = cap;
    DflLaserCapacityChanged(ctx); /* its bins are sized with the capacity too */
    if (f->out_on || x->capture) DflFlowEnsureSpares(ctx);
}

static void set_count(ParticleContext* ctx, index_type P) {
    ParticleExt* x = (ParticleExt*)ctx->ext;
    ctx->num_particle = P;
    for (int k = 0; k < 3; ++k) ctx->h_arr[k]->len = ctx->d_arr[k]->len = 3 * P;
    if (x->couple) x->couple->P = P;
    x->order_valid = x->sort_valid = FALSE; /* the sweep's permutation holds the old ids */
}

void ParticleContextSetOutflow(ParticleContext* ctx, const DflParticleOutflow* cfg) {
    ParticleExt* x = (ParticleExt*)ctx->ext;
    if (!cfg) {
        if (x->flow) x->flow->out_on = FALSE;
        return;
    }
    ASSERT(cfg->num_planes >= 0 && cfg->num_planes <= DFL_OUTFLOW_MAX_PLANES && "ParticleContextSetOutflow: num_planes");
    FlowState* f = DflFlowState(ctx);
    f->out = *cfg;
    f->out_on = TRUE;
    DflFlowEnsureSpares(ctx);
}

static f64 norm3(const f64* a) { return sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]); }

/* the slot lattice of include/dedflow.h for radius R (slot buffers sized to it) */
static void build_inlet(FlowState* f, f64 R) {
    const DflParticleInflow* in = &f->in;
    dfl_inlet* L = &f->inlet;
    memset(L, 0, sizeof *L);
    const f64 lu = norm3(in->edge_u), lv = norm3(in->edge_v);
    const f64 nuf = R > 0.0 ? floor(lu / (2.0 * R)) : 0.0, nvf = R > 0.0 ? floor(lv / (2.0 * R)) : 0.0;
    ASSERT(nuf * nvf <= (f64)(1 << 24) && "ParticleContextSetInflow: more than 2^24 inlet slots");
    L->nu = (index_type)nuf;
    L->nv = (index_type)nvf;
    const f64 jitter = in->jitter < 0.0 ? 0.0 : (in->jitter > 1.0 ? 1.0 : in->jitter);
    if (L->nu > 0 && L->nv > 0) {
        L->ju = jitter * (0.5 * (lu / (f64)L->nu - 2.0 * R));
        L->jv = jitter * (0.5 * (lv / (f64)L->nv - 2.0 * R));
        L->pitch_u = lu / (f64)L->nu;
        L->pitch_v = lv / (f64)L->nv;
        for (int d = 0; d < 3; ++d) {
            L->pu[d] = in->edge_u[d] / (f64)L->nu;
            L->pv[d] = in->edge_v[d] / (f64)L->nv;
            L->base[d] = (in->origin[d] + 0.5 * L->pu[d]) + 0.5 * L->pv[d];
            L->uhat[d] = in->edge_u[d] / lu;
            L->vhat[d] = in->edge_v[d] / lv;
            L->ou[d] = L->uhat[d] * L->ju;
            L->ov[d] = L->vhat[d] * L->jv;
            L->o[d] = in->origin[d];
        }
        const f64* a = L->uhat;
        const f64* b = L->vhat;
        f64 n[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
        const f64 ln = norm3(n);
        for (int d = 0; d < 3; ++d) L->nrm[d] = n[d] / ln;
        const f64 om = fmax(fabs(in->origin[0]), fmax(fabs(in->origin[1]), fabs(in->origin[2])));
        L->plane_tol = 1e-9 * (om + lu + lv + R);
    }
    for (int d = 0; d < 3; ++d) L->vel[d] = in->vel[d];
    L->seed = in->seed;
    f->inlet_R = R;
    const index_type nslot = L->nu * L->nv;
    if (nslot != f->nslot || !f->blocked) {
        HIPGUARD(hipStreamSynchronize(DflStream()));
        free_slots(f);
        const ptrdiff_t n = nslot > 0 ? nslot : 1;
        f->blocked = (index_type*)CdamMallocDevice(n * SIZE_OF(index_type));
        f->slot = (index_type*)CdamMallocDevice(n * SIZE_OF(index_type));
        f->slot_out = (index_type*)CdamMallocDevice(n * SIZE_OF(index_type));
        f->key = (uint64_t*)CdamMallocDevice(n * SIZE_OF(uint64_t));
        f->key_out = (uint64_t*)CdamMallocDevice(n * SIZE_OF(uint64_t));
        f->sort_bytes = dfl_inflow_select_temp_bytes(nslot);
        f->sort_tmp = CdamMallocDevice((ptrdiff_t)f->sort_bytes);
        f->nslot = nslot;
    }
}

void ParticleContextSetInflow(ParticleContext* ctx, const DflParticleInflow* cfg) {
    ParticleExt* x = (ParticleExt*)ctx->ext;
    if (!cfg) {
        if (x->flow) x->flow->in_on = FALSE;
        return;
    }
    const f64 uv = (cfg->edge_u[0] * cfg->edge_v[0] + cfg->edge_u[1] * cfg->edge_v[1]) + cfg->edge_u[2] * cfg->edge_v[2];
    ASSERT(fabs(uv) <= 1e-9 * norm3(cfg->edge_u) * norm3(cfg->edge_v) && "ParticleContextSetInflow: edge_u must be perpendicular to edge_v");
    ASSERT(cfg->per_call >= 0.0 && "ParticleContextSetInflow: per_call must not be negative");
    FlowState* f = DflFlowState(ctx);
    f->in = *cfg;
    f->in_on = TRUE;
    f->call = 0;
    f->credit = 0.0;
    f64 r_lo, r_hi;
    DflInflowRadii(ctx, &r_lo, &r_hi);
    build_inlet(f, x->radius ? r_hi : ParticleRadius(ctx));
}

void ParticleContextRemove(ParticleContext* ctx) {
    ParticleExt* x = (ParticleExt*)ctx->ext;
    FlowState* f = x->flow;
    if (!f || !f->out_on) return;
    CoupleState* c = x->couple;
    const b32 by_mesh = f->out.outside_mesh && c;
    if (by_mesh) ParticleContextLocate(ctx); /* tet -1 also means "not located yet" */
    const index_type P = ctx->num_particle;
    if (P <= 0) return;
    DflRangePush("ParticleContextRemove");
    hipStream_t s = DflStream();
    DflFlowEnsureSpares(ctx);
    dfl_outflow_planes pl;
    memset(&pl, 0, sizeof pl);
    pl.num = f->out.num_planes;
    memcpy(pl.plane, f->out.plane, sizeof pl.plane);
    const b32 pending = c && c->imp_time > 0.0;
    const b32 heat_pending = DflHeatPending(ctx) && x->heat->time > 0.0; /* the laser's substrate energy is per node */
    dfl_flow_flag(P, ArrayData(ParticleCTXDeviceCoord(ctx)), pl, c ? c->tet : NULL, by_mesh ? 1 : 0, f->keep,
                  pending || heat_pending ? f->rtet : NULL, s);
    dfl_exclusive_scan_i32(P, f->keep, f->newid, f->scan_tmp, f->scan_bytes, s);
    const index_type Pn = DflReadDeviceIndex(f->newid + P);
    if (Pn == P) {
        DflRangePop();
        return;
    }
    if (pending) DflCoupleAccumulateRemoved(ctx, f->rtet); /* before the compaction moves imp and lambda */
    if (heat_pending) DflHeatAccumulateRemoved(ctx, f->rtet);
    DflFlowCompact(ctx, Pn);
    f->stats.removed += P - Pn;
    DflRangePop();
}

void DflFlowCompact(ParticleContext* ctx, index_type Pn) {
    ParticleExt* x = (ParticleExt*)ctx->ext;
    FlowState* f = x->flow;
    const index_type P = ctx->num_particle;
    hipStream_t s = DflStream();
    /* every carried field into a spare, grouped by element size; the swap in the same walk: the compacted copy becomes the
       live buffer, the old one the spare */
    static const int group_bytes[4] = {4, 8, 24, 32};
    DflPField rows[DFL_PF_MAX_ROWS];
    const int nrow = DflParticleFields(ctx, DflParticleLiveFeatures(ctx), rows);
    dfl_flow_fields fl;
    memset(&fl, 0, sizeof fl);
    unsigned taken = 0;
    int n = 0, carried = 0;
    for (int g = 0; g < 4; ++g) {
        fl.first[g] = n;
        for (int r = 0; r < nrow; ++r) {
            if (rows[r].kind != DFL_PF_CARRIED || rows[r].bytes != group_bytes[g]) continue;
            void** spare = spare_of(f, &rows[r], x->cap, &taken);
            fl.pair[n].src = *rows[r].ptr;
            fl.pair[n].dst = *spare;
            *spare = *rows[r].ptr;
            *rows[r].ptr = fl.pair[n].dst;
            ++n;
        }
    }
    fl.first[4] = n;
    for (int r = 0; r < nrow; ++r) carried += rows[r].kind == DFL_PF_CARRIED;
    ASSERT(n == carried && "a carried per-particle field whose element size the compaction kernel has no copy path for");
    const int cur = x->hist_cur;
    if (x->omega) { /* the rows the next sweep reads move into the other row set, which becomes the current one */
        fl.hrow_src = x->hist[cur];
        fl.hcount_src = x->hist_count[cur];
        fl.hrow_dst = x->hist[1 - cur];
        fl.hcount_dst = x->hist_count[1 - cur];
    }
    dfl_flow_compact(P, f->keep, f->newid, fl, s);
    if (x->omega) x->hist_cur = 1 - cur;
    set_count(ctx, Pn);
}

void ParticleContextAdd(ParticleContext* ctx) {
    ParticleExt* x = (ParticleExt*)ctx->ext;
    FlowState* f = x->flow;
    if (!f || !f->in_on) return;
    f64 r_lo, r_hi; /* polydisperse: the lattice is built for r_hi */
    DflInflowRadii(ctx, &r_lo, &r_hi);
    const f64 R = x->radius ? r_hi : ParticleRadius(ctx);
    if (x->radius && r_hi > x->rmax) { /* inserted at ParticleRadius without SetInflowSizes */
        x->rmax = r_hi;
        x->sort_valid = FALSE;
    }
    if (R != f->inlet_R) build_inlet(f, R);
    f->inlet.call = f->call++;
    f->credit += f->in.per_call;
    f64 want_f = floor(f->credit);
    f->credit -= want_f;
    const index_type P = ctx->num_particle;
    const f64 room = f->in.max_particles > P ? (f64)(f->in.max_particles - P) : 0.0;
    if (want_f > room) want_f = room;
    const index_type want = (index_type)want_f;
    if (want <= 0) return;
    const index_type n_try = want < f->nslot ? want : f->nslot;
    if (n_try <= 0) {
        f->stats.blocked += want;
        return;
    }
    DflRangePush("ParticleContextAdd");
    hipStream_t s = DflStream();
    grow(ctx, P + n_try);
    CoupleState* c = x->couple;
    dfl_inflow_block(P, ArrayData(ParticleCTXDeviceCoord(ctx)), f->inlet, R, x->radius, r_lo, r_hi, f->blocked, s);
    dfl_inflow_select(f->inlet, f->blocked, f->key, f->key_out, f->slot, f->slot_out, f->sort_tmp, f->sort_bytes, s);
    dfl_inflow_append(P, n_try, f->inlet, f->key_out, f->slot_out, f->next_tag, ArrayData(ParticleCTXDeviceCoord(ctx)),
                      ArrayData(ParticleCTXDeviceVel(ctx)), ArrayData(ParticleCTXDeviceAcc(ctx)), f->tag, x->omega, x->alpha,
                      x->omega ? x->hist_count[x->hist_cur] : NULL, c ? c->tet : NULL, c ? c->lambda : NULL, c ? c->imp : NULL,
                      x->radius, x->mass, r_lo, r_hi, ParticleRadius(ctx), ParticleMass(ctx), f->count, s);
    const index_type n = DflReadDeviceIndex(f->count);
    f->next_tag += n;
    f->stats.inserted += n;
    f->stats.blocked += want - n;
    if (n > 0 && x->heat) /* inserted particles start at T_init with nothing pending */
        dfl_heat_fill(P, n, x->heat->cfg.T_init, x->heat->temp, x->heat->rate, x->heat->e, s);
    if (n > 0) set_count(ctx, P + n);
    DflRangePop();
}

void ParticleContextFlowStats(const ParticleContext* ctx, DflParticleFlowStats* out) {
    const FlowState* f = ((const ParticleExt*)ctx->ext)->flow;
    if (f) *out = f->stats;
    else memset(out, 0, sizeof *out);
}

const int64_t* ParticleContextTag(const ParticleContext* ctx) {
    const FlowState* f = ((const ParticleExt*)ctx->ext)->flow;
    return f ? f->tag : NULL;
}
