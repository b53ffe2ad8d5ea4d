/* ParticleContext behind src/Particle.h:13-35.  The reference provides storage only
 * (coord / vel / acc, host + device, mass 1.0, radius 0.1 hard-coded, Particle.c:8-26) and
 * empty Add/Update/Remove hooks (:120-130).  The contact sweep is build-defined
 * (dedflow_amd/csrc/k_dem.hip): ParticleContextComputeForces = cell list + force kernel,
 * ParticleContextUpdate = forces + semi-implicit Euler step.  With walls from a mesh (ParticleContextSetWallMesh) the sweep
 * runs in host/walls.c instead.  With friction on (ParticleContextSetFriction) both sweeps run their friction kernels,
 * which read the previous sweep's contact history and write the next one into the other of two buffers. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "dedflow.h"
#include "dedflow_kernels.h"
#include "host_private.h"

ParticleContext* ParticleContextCreate(index_type num_particle) {
    ParticleContext* ctx = (ParticleContext*)CdamMallocHost(SIZE_OF(ParticleContext));
    memset(ctx, 0, sizeof *ctx);
    ctx->num_particle = num_particle;
    ctx->num_pointwise_dof = 9;
    for (int k = 0; k < 3; ++k) {
        ctx->h_arr[k] = ArrayCreateHost(num_particle * 3);
        ctx->d_arr[k] = ArrayCreateDevice(num_particle * 3);
    }
    ParticleMass(ctx) = 1.0;   /* Particle.c:23-24 */
    ParticleRadius(ctx) = 0.1;
    ParticleExt* x = (ParticleExt*)CdamMallocHost(SIZE_OF(ParticleExt));
    memset(x, 0, sizeof *x);
    x->kn = 1.0e4;
    x->gamma_n = 1.0;
    x->dt = 1.0e-4;
    x->cap = num_particle;
    ctx->ext = x;
    return ctx;
}

void ParticleContextDestroy(ParticleContext* ctx) {
    if (!ctx) return;
    ParticleExt* x = (ParticleExt*)ctx->ext;
    for (int k = 0; k < 3; ++k) {
        if (x) ctx->h_arr[k]->len = ctx->d_arr[k]->len = 3 * x->cap; /* the size they were allocated with */
        ArrayDestroy(ctx->h_arr[k]);
        ArrayDestroy(ctx->d_arr[k]);
    }
    if (x) {
        CdamFreeDevice(x->cell_of, 0); CdamFreeDevice(x->rank, 0); CdamFreeDevice(x->slot, 0); CdamFreeDevice(x->order, 0); CdamFreeDevice(x->sorted, 0);
        CdamFreeDevice(x->count, 0); CdamFreeDevice(x->cell_start, 0); CdamFreeDevice(x->chunk_sum, 0);
        DflCoupleFree(ctx);
        DflWallsFree(x->walls);
        ParticleContextSetFriction(ctx, NULL);
        DflCaptureFree(ctx);
        DflSurfaceContactFree(ctx);
        DflFlowFree(ctx);
        ParticleContextSetSizes(ctx, NULL, NULL);
        DflLaserFree(ctx);
        DflHeatFree(ctx);
        CdamFreeHost(x, SIZE_OF(ParticleExt));
    }
    CdamFreeHost(ctx, SIZE_OF(ParticleContext));
}

void ParticleContextCopy(ParticleContext* dst, const ParticleContext* src) {
    ASSERT(dst && src && dst->num_particle == src->num_particle);
    for (int k = 0; k < 3; ++k) {
        ArrayCopy(dst->h_arr[k], src->h_arr[k], H2H);
        ArrayCopy(dst->d_arr[k], src->d_arr[k], D2D);
    }
    DflHeatCopy(dst, src); /* the thermal state travels too */
    DflCaptureCopy(dst, src); /* the capture configuration (nothing pending) */
    DflSurfaceContactCopy(dst, src); /* the surface-contact configuration (not the counters) */
    /* the sizes travel with the particles (the inflow radius range is configuration and stays) */
    const ParticleExt* xs = (const ParticleExt*)src->ext;
    ParticleExt* xd = (ParticleExt*)dst->ext;
    if (!xs->radius) {
        if (xd->radius) ParticleContextSetSizes(dst, NULL, NULL);
        DflLaserCopy(dst, src);
        return;
    }
    const index_type P = src->num_particle;
    f64* h = (f64*)malloc((size_t)(P > 0 ? 2 * P : 1) * sizeof(f64));
    HIPGUARD(hipStreamSynchronize(DflStream()));
    if (P > 0) {
        HIPGUARD(hipMemcpy(h, xs->radius, (size_t)P * sizeof(f64), D2H));
        HIPGUARD(hipMemcpy(h + P, xs->mass, (size_t)P * sizeof(f64), D2H));
    }
    ParticleContextSetSizes(dst, h, h + P);
    if (xd->radius && xs->rmax > xd->rmax) xd->rmax = xs->rmax;
    free(h);
    DflLaserCopy(dst, src); /* the configuration and the elapsed scan time (after the sizes: h >= 2 Rmax) */
}
void ParticleContextUpdateHost(ParticleContext* ctx) {
    for (int k = 0; k < 3; ++k) ArrayCopy(ctx->h_arr[k], ctx->d_arr[k], D2H);
}
void ParticleContextUpdateDevice(ParticleContext* ctx) {
    for (int k = 0; k < 3; ++k) ArrayCopy(ctx->d_arr[k], ctx->h_arr[k], H2D);
}

void ParticleContextSetContactModel(ParticleContext* ctx, f64 kn, f64 gamma_n, f64 dt) {
    ParticleExt* x = (ParticleExt*)ctx->ext;
    x->kn = kn;
    x->gamma_n = gamma_n;
    x->dt = dt;
}

void DflDemReserve(ParticleExt* x, index_type P, index_type nbin) {
    if (x->cap_particle < P) {
        if (P < x->cap) P = x->cap; /* the context's capacity (grows geometrically under ParticleContextAdd) */
        CdamFreeDevice(x->cell_of, 0); CdamFreeDevice(x->rank, 0); CdamFreeDevice(x->slot, 0); CdamFreeDevice(x->order, 0); CdamFreeDevice(x->sorted, 0);
        x->cell_of = (index_type*)CdamMallocDevice((ptrdiff_t)P * SIZE_OF(index_type));
        x->rank = (index_type*)CdamMallocDevice((ptrdiff_t)P * SIZE_OF(index_type));
        x->slot = (index_type*)CdamMallocDevice((ptrdiff_t)P * SIZE_OF(index_type));
        x->order = (index_type*)CdamMallocDevice((ptrdiff_t)P * SIZE_OF(index_type));
        x->sorted = (f64*)CdamMallocDevice((ptrdiff_t)P * 6 * SIZE_OF(f64));
        x->cap_particle = P;
    }
    if (x->cap_cell < nbin + 1) { /* zero-filled by the allocator; every sweep leaves count zeroed again (chunk_sum is plain scratch) */
        CdamFreeDevice(x->count, 0); CdamFreeDevice(x->cell_start, 0); CdamFreeDevice(x->chunk_sum, 0);
        x->count = (index_type*)CdamMallocDevice(((ptrdiff_t)nbin + 1) * SIZE_OF(index_type));
        x->cell_start = (index_type*)CdamMallocDevice(((ptrdiff_t)nbin + 1) * SIZE_OF(index_type));
        x->chunk_sum = (index_type*)CdamMallocDevice((ptrdiff_t)dfl_scan_num_chunks(nbin) * SIZE_OF(index_type));
        x->cap_cell = nbin + 1;
    }
}

/* the cell sort of the unit-box sweep */
static void box_build_cells(ParticleContext* ctx) {
    ParticleExt* x = (ParticleExt*)ctx->ext;
    const index_type P = ctx->num_particle;
    const f64 R = x->radius ? x->rmax : ParticleRadius(ctx); /* polydisperse: the grid is built for Rmax */
    /* cell edge >= 4R: the interaction range of a particle covers at most two cells per axis; and not (much) finer than a few
       particles per cell -- the scan over the cells is what an over-fine grid pays for (125^3 cells for 100k particles cost
       14 us of scan; 58^3 cells 4 us, and the force kernel still tests only ~1.5 neighbours per particle) */
    index_type ncell = (index_type)floor(1.0 / (4.0 * R));
    const index_type by_count = (index_type)floor(cbrt(2.0 * (f64)P) + 0.5); /* about half a particle per cell */
    if (ncell > by_count) ncell = by_count;
    if (ncell < 1) ncell = 1;
    if (ncell > 256) ncell = 256; /* 2^24 cells at most (the dense cell arrays) */
    const f64 cell = 1.0 / (f64)ncell; /* >= 4R */
    const index_type ncell3 = ncell * ncell * ncell;
    DflDemReserve(x, P, ncell3);
    x->cell = cell;
    x->ncell = ncell;
    dfl_dem_build_cells(P, ArrayData(ParticleCTXDeviceCoord(ctx)), ArrayData(ParticleCTXDeviceVel(ctx)), x->omega, x->radius, cell,
                        ncell, x->cell_of, x->rank, x->count, x->chunk_sum, x->cell_start, x->slot, x->order, x->sorted, x->sorted_w,
                        x->sorted_r, DflStream());
    x->order_valid = x->sort_valid = TRUE;
}

void DflDemBuildCells(ParticleContext* ctx) {
    if (((ParticleExt*)ctx->ext)->walls) DflWallsBuildCells(ctx);
    else box_build_cells(ctx);
}

void ParticleContextComputeForces(ParticleContext* ctx) {
    ParticleExt* x = (ParticleExt*)ctx->ext;
    if (x->walls) {
        DflWallsComputeForces(ctx);
        return;
    }
    const index_type P = ctx->num_particle;
    const f64 R = x->radius ? x->rmax : ParticleRadius(ctx);
    hipStream_t s = DflStream();
    DflRangePush("ParticleContextComputeForces");
    box_build_cells(ctx);
    f64* acc = ArrayData(ParticleCTXDeviceAcc(ctx));
    int slot = DflProfileBegin(DFL_TAG_SMALL + 1);
    dfl_dem_forces(P, x->sorted, x->sorted_w, R, ParticleMass(ctx), DflSizes(x), x->kn, x->gamma_n, DflFrictionLaw(ctx), x->cell,
                   x->ncell, x->order, x->cell_start, DflFrictionHistory(x), acc, x->alpha, s);
    DflProfileEnd(slot);
    DflRangePop();
}

void ParticleContextUpdate(ParticleContext* ctx) {
    ParticleExt* x = (ParticleExt*)ctx->ext;
    ParticleContextComputeForces(ctx);
    const b32 gravity = x->gravity[0] != 0.0 || x->gravity[1] != 0.0 || x->gravity[2] != 0.0;
    if (x->omega || gravity)
        dfl_dem_integrate_spin(ctx->num_particle, x->dt, x->gravity, ArrayData(ParticleCTXDeviceCoord(ctx)),
                               ArrayData(ParticleCTXDeviceVel(ctx)), ArrayData(ParticleCTXDeviceAcc(ctx)), x->omega, x->alpha,
                               DflStream());
    else
        dfl_dem_integrate(ctx->num_particle, x->dt, ArrayData(ParticleCTXDeviceCoord(ctx)), ArrayData(ParticleCTXDeviceVel(ctx)),
                          ArrayData(ParticleCTXDeviceAcc(ctx)), DflStream());
    if (x->heat) DflHeatStep(ctx, NULL); /* conduction over this sweep's contacts */
}

/* ---- contact friction and rotation (model in include/dedflow.h) ---- */

static void clear_history(ParticleExt* x, index_type P) {
    hipStream_t s = DflStream();
    for (int k = 0; k < 2; ++k) HIPGUARD(hipMemsetAsync(x->hist_count[k], 0, (size_t)(P > 0 ? P : 1) * sizeof(index_type), s));
    HIPGUARD(hipMemsetAsync(x->overflow, 0, sizeof(index_type), s));
    x->hist_cur = 0;
}

void ParticleContextSetFriction(ParticleContext* ctx, const DflContactFriction* cfg) {
    ParticleExt* x = (ParticleExt*)ctx->ext;
    const index_type P = ctx->num_particle;
    if (!cfg) {
        if (!x->omega) return;
        HIPGUARD(hipStreamSynchronize(DflStream()));
        DflParticleFieldsFree(ctx, DFL_PF_FRICTION);
        CdamFreeDevice(x->overflow, 0);
        x->overflow = NULL;
        return;
    }
    ASSERT(cfg->mu >= 0.0 && "ParticleContextSetFriction: mu must not be negative");
    x->law.mu = cfg->mu;
    x->law.kt = cfg->kt > 0.0 ? cfg->kt : 2.0 / 7.0 * x->kn;
    x->law.gamma_t = cfg->gamma_t >= 0.0 ? cfg->gamma_t : x->gamma_n;
    if (!x->omega) {
        hipStream_t s = DflStream();
        const size_t n = (size_t)(x->cap > 0 ? x->cap : 1);
        DflParticleFieldsAlloc(ctx, DFL_PF_FRICTION);
        x->overflow = (index_type*)CdamMallocDevice(SIZE_OF(index_type));
        HIPGUARD(hipMemsetAsync(x->omega, 0, n * 3 * sizeof(f64), s));
        HIPGUARD(hipMemsetAsync(x->alpha, 0, n * 3 * sizeof(f64), s));
    }
    clear_history(x, P);
}

void DflFrictionClearHistory(ParticleContext* ctx) {
    ParticleExt* x = (ParticleExt*)ctx->ext;
    if (x->omega) clear_history(x, ctx->num_particle);
}

dfl_friction_law DflFrictionLaw(const ParticleContext* ctx) {
    const ParticleExt* x = (const ParticleExt*)ctx->ext;
    dfl_friction_law law = x->law;
    const f64 R = ParticleRadius(ctx);
    law.dt = x->dt;
    law.inertia = 0.4 * ParticleMass(ctx) * R * R;
    return law;
}

dfl_contact_history DflFrictionHistory(ParticleExt* x) {
    dfl_contact_history h = {NULL, NULL, NULL, NULL, NULL};
    if (!x->omega) return h;
    const int a = x->hist_cur, b = 1 - a;
    h.old_row = x->hist[a];
    h.old_count = x->hist_count[a];
    h.new_row = x->hist[b];
    h.new_count = x->hist_count[b];
    h.overflow = x->overflow;
    x->hist_cur = b;
    return h;
}

dfl_contact_history DflFrictionHistoryCurrent(const ParticleExt* x) {
    dfl_contact_history h = {NULL, NULL, NULL, NULL, NULL};
    if (!x->omega) return h;
    const int b = x->hist_cur, a = 1 - b;
    h.old_row = x->hist[a];
    h.old_count = x->hist_count[a];
    h.new_row = x->hist[b];
    h.new_count = x->hist_count[b];
    h.overflow = x->overflow;
    return h;
}

void ParticleContextFrictionHistory(const ParticleContext* ctx, const void** rows, const index_type** counts) {
    const ParticleExt* x = (const ParticleExt*)ctx->ext;
    *rows = x->omega ? (const void*)x->hist[x->hist_cur] : NULL;
    *counts = x->omega ? x->hist_count[x->hist_cur] : NULL;
}

f64* ParticleContextAngularVelocity(ParticleContext* ctx) { return ((ParticleExt*)ctx->ext)->omega; }
const f64* ParticleContextAngularAcc(const ParticleContext* ctx) { return ((const ParticleExt*)ctx->ext)->alpha; }

index_type ParticleContextFrictionOverflowCount(const ParticleContext* ctx) {
    const ParticleExt* x = (const ParticleExt*)ctx->ext;
    return x->overflow ? DflReadDeviceIndex(x->overflow) : 0;
}

void ParticleContextSetGravity(ParticleContext* ctx, const f64 g[3]) {
    ParticleExt* x = (ParticleExt*)ctx->ext;
    for (int d = 0; d < 3; ++d) x->gravity[d] = g ? g[d] : 0.0;
}

/* ---- polydisperse particles (model in include/dedflow.h) ---- */

dfl_sizes DflSizes(const ParticleExt* x) {
    dfl_sizes sz;
    sz.radius = x->radius;
    sz.mass = x->mass;
    sz.sorted_r = x->sorted_r;
    sz.rmax = x->rmax;
    return sz;
}

void DflInflowRadii(const ParticleContext* ctx, f64* r_lo, f64* r_hi) {
    const ParticleExt* x = (const ParticleExt*)ctx->ext;
    *r_lo = x->in_sizes ? x->in_r_lo : ParticleRadius(ctx);
    *r_hi = x->in_sizes ? x->in_r_hi : ParticleRadius(ctx);
}

static void free_sizes(ParticleContext* ctx) {
    ParticleExt* x = (ParticleExt*)ctx->ext;
    if (!x->radius) return;
    HIPGUARD(hipStreamSynchronize(DflStream()));
    DflParticleFieldsFree(ctx, DFL_PF_SIZES);
    x->in_sizes = FALSE;
    x->sort_valid = FALSE; /* the sorted copies and the grid were those of the per-particle sizes */
    x->rmax = 0.0;
}

void ParticleContextSetSizes(ParticleContext* ctx, const f64* radius, const f64* mass) {
    ParticleExt* x = (ParticleExt*)ctx->ext;
    if (!radius) {
        free_sizes(ctx);
        return;
    }
    const index_type P = ctx->num_particle;
    const f64 R = ParticleRadius(ctx), M = ParticleMass(ctx);
    f64 rmax = 0.0;
    for (index_type i = 0; i < P; ++i) {
        if (!(radius[i] > 0.0 && isfinite(radius[i])) || (mass && !(mass[i] > 0.0 && isfinite(mass[i])))) {
            fprintf(stderr, "ParticleContextSetSizes: particle %d has radius %g, mass %g; the sizes stay as they were\n", (int)i,
                    radius[i], mass ? mass[i] : 0.0);
            return;
        }
        if (radius[i] > rmax) rmax = radius[i];
    }
    if (!mass && !(R > 0.0 && M > 0.0)) {
        fprintf(stderr, "ParticleContextSetSizes: no masses and no positive reference particle; the sizes stay as they were\n");
        return;
    }
    f64* m = (f64*)malloc((size_t)(P > 0 ? P : 1) * sizeof(f64));
    for (index_type i = 0; i < P; ++i) {
        if (mass) {
            m[i] = mass[i];
        } else {
            const f64 q = radius[i] / R; /* the reference particle's density; q = 1 gives M exactly */
            m[i] = M * ((q * q) * q);
        }
    }
    if (!x->radius) DflParticleFieldsAlloc(ctx, DFL_PF_SIZES);
    HIPGUARD(hipStreamSynchronize(DflStream()));
    if (P > 0) {
        HIPGUARD(hipMemcpy(x->radius, radius, (size_t)P * sizeof(f64), H2D));
        HIPGUARD(hipMemcpy(x->mass, m, (size_t)P * sizeof(f64), H2D));
    }
    free(m);
    if (x->in_sizes && x->in_r_hi > rmax) rmax = x->in_r_hi;
    if (P == 0 && rmax == 0.0) rmax = R;
    x->rmax = rmax;
    x->sort_valid = FALSE; /* sorted_r and the grid of the last sweep are not these sizes' */
}

void ParticleContextSetInflowSizes(ParticleContext* ctx, f64 r_lo, f64 r_hi) {
    ParticleExt* x = (ParticleExt*)ctx->ext;
    if (!(r_lo > 0.0 && r_lo <= r_hi && isfinite(r_hi))) {
        fprintf(stderr, "ParticleContextSetInflowSizes: need 0 < r_lo <= r_hi, got %g, %g; unchanged\n", r_lo, r_hi);
        return;
    }
    if (!x->radius) { /* a monodisperse context becomes polydisperse: every particle keeps R and M */
        const index_type P = ctx->num_particle;
        f64* r = (f64*)calloc((size_t)(P > 0 ? P : 1), sizeof(f64));
        for (index_type i = 0; i < P; ++i) r[i] = ParticleRadius(ctx);
        ParticleContextSetSizes(ctx, r, NULL);
        free(r);
        if (!x->radius) return;
        if (P == 0) x->rmax = ParticleRadius(ctx);
    }
    x->in_sizes = TRUE;
    x->in_r_lo = r_lo;
    x->in_r_hi = r_hi;
    if (r_hi > x->rmax) {
        x->rmax = r_hi;
        x->sort_valid = FALSE; /* the grid is built for Rmax */
    }
}

const f64* ParticleContextRadii(const ParticleContext* ctx) { return ((const ParticleExt*)ctx->ext)->radius; }
const f64* ParticleContextMasses(const ParticleContext* ctx) { return ((const ParticleExt*)ctx->ext)->mass; }

f64 ParticleContextMaxRadius(const ParticleContext* ctx) {
    const ParticleExt* x = (const ParticleExt*)ctx->ext;
    return x->radius ? x->rmax : ParticleRadius(ctx);
}
