/* The per-particle device arrays of a ParticleContext, in one table: the single place that knows which feature owns which
 * array, how many bytes a particle has in it and whether its entries follow the particle.  Every feature allocates and
 * frees its arrays through the table, and host/flow.c -- the one file that changes the particle count -- grows, compacts
 * and swaps them from it.  A new per-particle quantity adds one row here and its initial value on append
 * (inflow_append_kernel, or a fill after it as dfl_heat_fill).  The host mirrors h_arr[k] are host memory and stay out. */
#include "dedflow.h"
#include "dedflow_kernels.h"
#include "host_private.h"

unsigned DflParticleLiveFeatures(const ParticleContext* ctx) {
    const ParticleExt* x = (const ParticleExt*)ctx->ext;
    return DFL_PF_BASE | (x->omega ? DFL_PF_FRICTION : 0) | (x->radius ? DFL_PF_SIZES : 0) | (x->heat ? DFL_PF_HEAT : 0) |
           (x->couple ? DFL_PF_COUPLE : 0) | (x->laser ? DFL_PF_LASER : 0) | (x->flow ? DFL_PF_FLOW : 0) |
           (x->capture ? DFL_PF_CAPTURE : 0);
}

int DflParticleFields(ParticleContext* ctx, unsigned features, DflPField* rows) {
    ParticleExt* x = (ParticleExt*)ctx->ext;
    int n = 0;
#define ROW(kind_, owner, bytes_, extra_) \
    (rows[n].ptr = (void**)&(owner), rows[n].bytes = (int)(bytes_), rows[n].kind = (kind_), rows[n].extra = (extra_), ++n)
#define CARRIED(owner, bytes_) ROW(DFL_PF_CARRIED, owner, bytes_, 0)
#define SCRATCH(owner, bytes_) ROW(DFL_PF_SCRATCH, owner, bytes_, 0)
    if (features & DFL_PF_BASE)
        for (int k = 0; k < 3; ++k) CARRIED(ctx->d_arr[k]->data, 3 * sizeof(f64)); /* coord, vel, acc */
    if (features & DFL_PF_FRICTION) {
        CARRIED(x->omega, 3 * sizeof(f64));
        CARRIED(x->alpha, 3 * sizeof(f64));
        SCRATCH(x->sorted_w, 3 * sizeof(f64));
        for (int k = 0; k < 2; ++k) { /* ping-pong: a compaction remaps the partner keys into the other set and flips hist_cur */
            ROW(DFL_PF_HISTORY, x->hist[k], DFL_DEM_MAX_HISTORY * sizeof(dfl_contact_hist), 0);
            ROW(DFL_PF_HISTORY, x->hist_count[k], sizeof(index_type), 0);
        }
    }
    if (features & DFL_PF_SIZES) {
        CARRIED(x->radius, sizeof(f64));
        CARRIED(x->mass, sizeof(f64));
        SCRATCH(x->sorted_r, sizeof(f64));
    }
    if (features & DFL_PF_HEAT) {
        HeatState* h = x->heat;
        CARRIED(h->temp, sizeof(f64));
        CARRIED(h->e, sizeof(f64));
        CARRIED(h->rate, sizeof(f64));
        SCRATCH(h->q, sizeof(f64));
        SCRATCH(h->sorted_t, sizeof(f64));
    }
    if (features & DFL_PF_COUPLE) {
        CoupleState* c = x->couple;
        CARRIED(c->tet, sizeof(index_type));
        CARRIED(c->lambda, 4 * sizeof(f64));
        CARRIED(c->imp, 3 * sizeof(f64));
        SCRATCH(c->rank, sizeof(index_type));
        SCRATCH(c->slot, sizeof(index_type));
        SCRATCH(c->members, sizeof(index_type));
    }
    if (features & DFL_PF_LASER) { /* the absorbed power is rewritten by every laser step: nothing to carry */
        LaserState* l = x->laser;
        SCRATCH(l->rate, sizeof(f64));
        SCRATCH(l->sorted, 6 * sizeof(f64));
        SCRATCH(l->sorted_r, sizeof(f64));
        SCRATCH(l->k_tau, sizeof(f64));
        SCRATCH(l->cell_of, sizeof(index_type));
        SCRATCH(l->rank, sizeof(index_type));
        SCRATCH(l->slot, sizeof(index_type));
        SCRATCH(l->order, sizeof(index_type));
        SCRATCH(l->k_id, sizeof(index_type));
    }
    if (features & DFL_PF_FLOW) {
        FlowState* f = x->flow;
        CARRIED(f->tag, sizeof(int64_t));
        SCRATCH(f->keep, sizeof(index_type));
        ROW(DFL_PF_SCRATCH, f->newid, sizeof(index_type), 1); /* the exclusive scan of keep and its total */
        SCRATCH(f->rtet, sizeof(index_type));
    }
    if (features & DFL_PF_CAPTURE) SCRATCH(x->capture->dep, 5 * sizeof(f64)); /* rewritten by every capture call */
#undef SCRATCH
#undef CARRIED
#undef ROW
    ASSERT(n <= DFL_PF_MAX_ROWS);
    return n;
}

void* DflParticleFieldAlloc(const DflPField* row, index_type cap) {
    return CdamMallocDevice(((ptrdiff_t)(cap > 0 ? cap : 1) + row->extra) * row->bytes);
}

void DflParticleFieldsAlloc(ParticleContext* ctx, unsigned feature) {
    DflPField rows[DFL_PF_MAX_ROWS];
    const int n = DflParticleFields(ctx, feature, rows);
    for (int r = 0; r < n; ++r) *rows[r].ptr = DflParticleFieldAlloc(&rows[r], ((ParticleExt*)ctx->ext)->cap);
}

void DflParticleFieldsFree(ParticleContext* ctx, unsigned feature) {
    DflPField rows[DFL_PF_MAX_ROWS];
    const int n = DflParticleFields(ctx, feature, rows);
    for (int r = 0; r < n; ++r) {
        CdamFreeDevice(*rows[r].ptr, 0);
        *rows[r].ptr = NULL;
    }
}

index_type DflReadDeviceIndex(const index_type* d) {
    index_type n = 0;
    hipStream_t s = DflStream();
    HIPGUARD(hipMemcpyAsync(&n, d, sizeof n, D2H, s));
    HIPGUARD(hipStreamSynchronize(s));
    return n;
}
