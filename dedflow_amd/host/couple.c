/* Particle-fluid coupling (build-defined; model and sign conventions in include/dedflow.h, kernels in
 * dedflow_amd/csrc/k_couple.hip).  The reference keeps the hooks (SolveParticleSystem, ParticleContextUpdate in its time
 * loop) commented out and has no physics behind them.
 *
 * Per coupled mesh, built once at ParticleContextSetFluidCoupling: the tet neighbour table (on the device, from the mesh's
 * sorted V2E map, DflMeshSortedV2E, which the reaction scatter walks in that order too) and a uniform seed
 * grid over the bounding box (on the host: per cell the tet whose centroid is nearest the cell centre, empty cells filled
 * breadth-first from their neighbours).  Per particle: tet, lambda[4], impulse[3].  Per call nothing is allocated and
 * nothing waits for the device. */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "dedflow.h"
#include "dedflow_kernels.h"
#include "host_private.h"


static CoupleState* state(const ParticleContext* ctx) { return ((ParticleExt*)ctx->ext)->couple; }

void DflCoupleFree(ParticleContext* ctx) {
    CoupleState* c = state(ctx);
    if (!c) return;
    HIPGUARD(hipStreamSynchronize(DflStream()));
    DflParticleFieldsFree(ctx, DFL_PF_COUPLE);
    CdamFreeDevice(c->nbr, 0); CdamFreeDevice(c->seed, 0);
    CdamFreeDevice(c->lost, 0); CdamFreeDevice(c->tcount, 0); CdamFreeDevice(c->tstart, 0); CdamFreeDevice(c->scan_tmp, 0);
    CdamFreeDevice(c->load, 0); CdamFreeDevice(c->rem_load, 0); CdamFreeDevice(c->rem_tmp, 0);
    CdamFreeHost(c, SIZE_OF(CoupleState));
    ((ParticleExt*)ctx->ext)->couple = NULL;
}

/* seed grid: gdim^3 cells over the bounding box (about 8 tets per cell), each holding the tet whose centroid lies nearest
 * the cell centre (lowest id on a tie); cells without a centroid take the tet of the nearest filled cell, breadth-first in
 * cell order (deterministic) */
static void build_seed_grid(CoupleState* c, const f64* xg, const index_type* ien) {
    const index_type N = c->N, T = c->T;
    f64 lo[3], hi[3];
    DflNodeBounds(xg, N, lo, hi);
    index_type g = (index_type)floor(cbrt((f64)T / 8.0));
    if (g < 1) g = 1;
    if (g > 128) g = 128;
    const size_t ncell = (size_t)g * g * g;
    for (int d = 0; d < 3; ++d) {
        const f64 ext = hi[d] > lo[d] ? hi[d] - lo[d] : 1.0;
        c->lo[d] = lo[d];
        c->inv_h[d] = (f64)g / ext;
    }
    index_type* seed = (index_type*)malloc(ncell * sizeof(index_type));
    f64* best = (f64*)malloc(ncell * sizeof(f64));
    size_t* queue = (size_t*)malloc(ncell * sizeof(size_t));
    for (size_t k = 0; k < ncell; ++k) {
        seed[k] = -1;
        best[k] = HUGE_VAL;
    }
    for (index_type t = 0; t < T; ++t) {
        f64 cen[3] = {0.0, 0.0, 0.0};
        for (int b = 0; b < 4; ++b)
            for (int d = 0; d < 3; ++d) cen[d] += 0.25 * xg[3 * (size_t)ien[4 * (size_t)t + b] + d];
        index_type cc[3];
        f64 dist = 0.0;
        for (int d = 0; d < 3; ++d) {
            f64 q = floor((cen[d] - c->lo[d]) * c->inv_h[d]);
            cc[d] = q < 0 ? 0 : (q >= g ? g - 1 : (index_type)q);
            const f64 mid = c->lo[d] + (cc[d] + 0.5) / c->inv_h[d];
            dist += (cen[d] - mid) * (cen[d] - mid);
        }
        const size_t k = (size_t)cc[0] + (size_t)g * ((size_t)cc[1] + (size_t)g * cc[2]);
        if (dist < best[k]) { /* ascending t: the lowest id wins a tie */
            best[k] = dist;
            seed[k] = t;
        }
    }
    size_t head = 0, tail = 0;
    for (size_t k = 0; k < ncell; ++k)
        if (seed[k] >= 0) queue[tail++] = k;
    while (head < tail) {
        const size_t k = queue[head++];
        const index_type cx = (index_type)(k % g), cy = (index_type)((k / g) % g), cz = (index_type)(k / ((size_t)g * g));
        const index_type nb[6][3] = {{cx - 1, cy, cz}, {cx + 1, cy, cz}, {cx, cy - 1, cz}, {cx, cy + 1, cz}, {cx, cy, cz - 1}, {cx, cy, cz + 1}};
        for (int j = 0; j < 6; ++j) {
            if (nb[j][0] < 0 || nb[j][0] >= g || nb[j][1] < 0 || nb[j][1] >= g || nb[j][2] < 0 || nb[j][2] >= g) continue;
            const size_t q = (size_t)nb[j][0] + (size_t)g * ((size_t)nb[j][1] + (size_t)g * nb[j][2]);
            if (seed[q] >= 0) continue;
            seed[q] = seed[k];
            queue[tail++] = q;
        }
    }
    c->gdim = g;
    c->seed = (index_type*)CdamMallocDevice((ptrdiff_t)ncell * SIZE_OF(index_type));
    HIPGUARD(hipMemcpy(c->seed, seed, ncell * sizeof(index_type), H2D));
    free(queue);
    free(best);
    free(seed);
}

static void build_mesh_tables(CoupleState* c, Mesh3D* mesh) {
    const Mesh3DData* dev = Mesh3DDevice(mesh);
    const index_type N = c->N, T = c->T;
    hipStream_t s = DflStream();
    const index_type *vrow, *vcol;
    DflMeshSortedV2E(mesh, &vrow, &vcol);
    c->nbr = (index_type*)CdamMallocDevice((ptrdiff_t)(T > 0 ? T : 1) * 4 * SIZE_OF(index_type));
    dfl_couple_neighbours(T, dev->ien, vrow, vcol, c->nbr, s);
    /* the seed grid from a host copy of the device mesh (what the kernels will read) */
    f64* xg = (f64*)malloc((size_t)N * 3 * sizeof(f64) + 8);
    index_type* ien = (index_type*)malloc((size_t)T * 4 * sizeof(index_type) + 8);
    HIPGUARD(hipMemcpy(xg, dev->xg, (size_t)N * 3 * sizeof(f64), D2H));
    HIPGUARD(hipMemcpy(ien, dev->ien, (size_t)T * 4 * sizeof(index_type), D2H));
    build_seed_grid(c, xg, ien);
    free(ien);
    free(xg);
    c->tcount = (index_type*)CdamMallocDevice((ptrdiff_t)(T > 0 ? T : 1) * SIZE_OF(index_type));
    c->tstart = (index_type*)CdamMallocDevice(((ptrdiff_t)T + 1) * SIZE_OF(index_type));
    c->scan_bytes = dfl_scan_temp_bytes(T);
    c->scan_tmp = CdamMallocDevice((ptrdiff_t)c->scan_bytes);
    c->load = (f64*)CdamMallocDevice((ptrdiff_t)(N > 0 ? N : 1) * 3 * SIZE_OF(f64));
    c->rem_load = (f64*)CdamMallocDevice((ptrdiff_t)(N > 0 ? N : 1) * 3 * SIZE_OF(f64));
    c->rem_tmp = (f64*)CdamMallocDevice((ptrdiff_t)(N > 0 ? N : 1) * 3 * SIZE_OF(f64));
    HIPGUARD(hipStreamSynchronize(s));
}

void ParticleContextSetFluidCoupling(ParticleContext* ctx, Mesh3D* mesh, const DflFluidCoupling* cfg) {
    ParticleExt* x = (ParticleExt*)ctx->ext;
    const index_type P = ctx->num_particle;
    CoupleState* c = x->couple;
    if (c && (!mesh || c->mesh != mesh || c->N != Mesh3DNumNode(mesh) || c->T != Mesh3DNumTet(mesh) || c->P != P)) {
        DflCoupleFree(ctx);
        c = NULL;
    }
    if (!mesh) {
        DflHeatCouplingChanged(ctx);
        DflCaptureCouplingChanged(ctx);
        DflSurfaceContactCouplingChanged(ctx);
        return;
    }
    if (Mesh3DNumTet(mesh) <= 0) {
        fprintf(stderr, "ParticleContextSetFluidCoupling: the mesh has no tets; coupling stays off\n");
        DflSurfaceContactCouplingChanged(ctx);
        return;
    }
    if (!c) {
        c = (CoupleState*)CdamMallocHost(SIZE_OF(CoupleState));
        memset(c, 0, sizeof *c);
        c->mesh = mesh;
        c->N = Mesh3DNumNode(mesh);
        c->T = Mesh3DNumTet(mesh);
        c->P = P;
        build_mesh_tables(c, mesh);
        c->lost = (index_type*)CdamMallocDevice(SIZE_OF(index_type));
        const char* e = getenv("DFL_COUPLE_CELL_ORDER");
        c->use_order = !(e && e[0] == '0');
        x->couple = c;
        DflParticleFieldsAlloc(ctx, DFL_PF_COUPLE);
    }
    DflFluidCoupling def = {1.0e3, 10.0 / 3.0, {0.0, 0.0, 0.0}, FALSE}; /* kRHO, kMU of assemble.cu:35,40 */
    c->cfg = cfg ? *cfg : def;
    hipStream_t s = DflStream();
    HIPGUARD(hipMemsetAsync(c->tet, 0xff, (size_t)(P > 0 ? P : 1) * sizeof(index_type), s)); /* -1: start from the seed grid */
    HIPGUARD(hipMemsetAsync(c->lambda, 0, (size_t)(P > 0 ? P : 1) * 4 * sizeof(f64), s));
    HIPGUARD(hipMemsetAsync(c->imp, 0, (size_t)(P > 0 ? P : 1) * 3 * sizeof(f64), s));
    HIPGUARD(hipMemsetAsync(c->lost, 0, sizeof(index_type), s));
    HIPGUARD(hipMemsetAsync(c->rem_load, 0, (size_t)(c->N > 0 ? c->N : 1) * 3 * sizeof(f64), s));
    c->rem_pending = FALSE;
    c->imp_time = 0.0;
    DflHeatCouplingChanged(ctx);
    DflCaptureCouplingChanged(ctx);
    DflSurfaceContactCouplingChanged(ctx);
}

/* the thread -> particle map of the walk: the contact sweep's (cell, id) order when it has run since the particle count
 * last changed (any permutation is correct; neighbouring lanes then walk neighbouring tets: 10.7 / 28 us from history /
 * cold against 11.4 / 33 us in particle-id order at 1M tets and 100k particles), else particle order */
static const index_type* particle_order(const ParticleContext* ctx, const CoupleState* c) {
    const ParticleExt* x = (const ParticleExt*)ctx->ext;
    return c->use_order && x->order && x->order_valid && x->cap_particle >= ctx->num_particle ? x->order : NULL;
}

void ParticleContextLocate(ParticleContext* ctx) {
    CoupleState* c = state(ctx);
    ASSERT(c && "ParticleContextLocate: the context is not coupled to a mesh");
    if (!c) return;
    const Mesh3DData* dev = Mesh3DDevice(c->mesh);
    int slot = DflProfileBegin(DFL_TAG_SMALL + 2);
    dfl_couple_locate(ctx->num_particle, particle_order(ctx, c), ArrayData(ParticleCTXDeviceCoord(ctx)), dev->xg, dev->ien, c->nbr,
                      c->seed, c->lo, c->inv_h, c->gdim, c->tet, c->lambda, c->lost, DflStream());
    DflProfileEnd(slot);
}

const index_type* ParticleContextTet(const ParticleContext* ctx) { return state(ctx) ? state(ctx)->tet : NULL; }
const f64* ParticleContextBarycentric(const ParticleContext* ctx) { return state(ctx) ? state(ctx)->lambda : NULL; }

index_type ParticleContextLostCount(const ParticleContext* ctx) {
    const CoupleState* c = state(ctx);
    return c ? DflReadDeviceIndex(c->lost) : 0;
}

void ParticleContextFluidStep(ParticleContext* ctx, const f64* w) {
    CoupleState* c = state(ctx);
    ASSERT(c && "ParticleContextFluidStep: the context is not coupled to a mesh");
    if (!c) return;
    ParticleExt* x = (ParticleExt*)ctx->ext;
    DflRangePush("ParticleContextFluidStep");
    ParticleContextComputeForces(ctx);
    ParticleContextLocate(ctx);
    if (x->surface_contact) DflSurfaceContactApply(ctx, w); /* acc, alpha and the rows of the sweep above, before the drag */
    int slot = DflProfileBegin(DFL_TAG_SMALL + 3);
    /* particle-id order: the kernel's contiguous per-particle reads and writes outweigh the gather locality of the cell
       order (1M tets, 100k particles: 14.2 us in id order, 23.4 us in cell order; tools/probe_coupling.py) */
    dfl_couple_fluid_step(ctx->num_particle, NULL, c->tet, c->lambda, Mesh3DDevice(c->mesh)->ien, w, ParticleMass(ctx),
                          ParticleRadius(ctx), x->mass, x->radius, c->cfg.rho_f, c->cfg.mu_f, c->cfg.gravity, x->dt,
                          ArrayData(ParticleCTXDeviceCoord(ctx)), ArrayData(ParticleCTXDeviceVel(ctx)),
                          ArrayData(ParticleCTXDeviceAcc(ctx)), c->imp, DflStream());
    DflProfileEnd(slot);
    if (x->omega) dfl_dem_spin(ctx->num_particle, x->dt, x->omega, x->alpha, DflStream()); /* the fluid exerts no torque */
    c->imp_time += x->dt;
    if (x->heat) DflHeatStep(ctx, w); /* conduction over this sweep's contacts, convection at the new velocity */
    DflRangePop();
}

void DflCoupleNodeScatter(ParticleContext* ctx, const index_type* tet, const f64* val, int ncomp, f64 scale, f64* out) {
    CoupleState* c = state(ctx);
    hipStream_t s = DflStream();
    const index_type* ien = Mesh3DDevice(c->mesh)->ien;
    const index_type *vrow, *vcol;
    DflMeshSortedV2E(c->mesh, &vrow, &vcol);
    dfl_couple_sort_by_tet(ctx->num_particle, c->T, tet, c->tcount, c->rank, c->tstart, c->slot, c->members, c->scan_tmp,
                           c->scan_bytes, s);
    if (ncomp == 3) dfl_couple_node_load(c->N, vrow, vcol, ien, c->tstart, c->members, c->lambda, val, scale, out, s);
    else dfl_couple_node_scalar(c->N, vrow, vcol, ien, c->tstart, c->members, c->lambda, val, scale, out, s);
}

void ParticleContextReactionLoad(ParticleContext* ctx, f64* load) {
    CoupleState* c = state(ctx);
    ASSERT(c && "ParticleContextReactionLoad: the context is not coupled to a mesh");
    if (!c) return;
    hipStream_t s = DflStream();
    if (c->imp_time <= 0.0) {
        HIPGUARD(hipMemsetAsync(load, 0, (size_t)c->N * 3 * sizeof(f64), s));
        return;
    }
    DflRangePush("ParticleContextReactionLoad");
    int slot = DflProfileBegin(DFL_TAG_SMALL + 4);
    const index_type P = ctx->num_particle;
    DflCoupleNodeScatter(ctx, c->tet, c->imp, 3, 1.0 / c->imp_time, load);
    if (c->rem_pending) { /* the impulse of the particles removed since the last call (ParticleContextRemove) */
        dfl_daxpy(c->N * 3, 1.0 / c->imp_time, c->rem_load, load, s);
        HIPGUARD(hipMemsetAsync(c->rem_load, 0, (size_t)c->N * 3 * sizeof(f64), s));
        c->rem_pending = FALSE;
    }
    HIPGUARD(hipMemsetAsync(c->imp, 0, (size_t)(P > 0 ? P : 1) * 3 * sizeof(f64), s));
    DflProfileEnd(slot);
    c->imp_time = 0.0;
    DflRangePop();
}

void DflCoupleAccumulateRemoved(ParticleContext* ctx, const index_type* rtet) {
    CoupleState* c = state(ctx);
    hipStream_t s = DflStream();
    /* the pattern of the reaction load, restricted to the removed particles: rem_tmp = -sum lambda imp, then rem_load += it */
    DflCoupleNodeScatter(ctx, rtet, c->imp, 3, 1.0, c->rem_tmp);
    dfl_daxpy(c->N * 3, 1.0, c->rem_tmp, c->rem_load, s);
    c->rem_pending = TRUE;
}

Mesh3D* DflParticleCoupledMesh(const ParticleContext* ctx) { return state(ctx) ? state(ctx)->mesh : NULL; }
b32 DflParticleTwoWay(const ParticleContext* ctx) { return state(ctx) ? state(ctx)->cfg.two_way : FALSE; }
f64* DflParticlePendingLoad(ParticleContext* ctx) {
    CoupleState* c = state(ctx);
    if (!c || c->imp_time <= 0.0) return NULL;
    ParticleContextReactionLoad(ctx, c->load);
    return c->load;
}
