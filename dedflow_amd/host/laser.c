/* Laser energy deposition (build-defined, opt-in; model in include/dedflow.h, kernels in dedflow_amd/csrc/k_laser.hip).
 * The reference's T equation has no source term.
 *
 * State of a context with a laser (ParticleExt.laser): the configuration with the normalised direction and the transverse
 * frame, the elapsed scan time; per column the weights, the hit keys, the transmitted power, the hit face and the tally
 * partials, plus the bins of the column sort; per particle (the context's capacity) the absorbed power by id and the
 * scratch of the column sort -- its own, so that the contact sweep's order / cell_start survive for the conduction of the
 * same sub-step; per substrate node the power of the last step and the energy since the last heat source.  The substrate
 * list -- the faces of the coupled mesh in the masked groups with n . dir < 0, as the wall records of host/walls.c, and
 * per node of those faces the list of its faces -- is built once per (coupled mesh, mask, direction): at
 * ParticleContextSetLaser and when the coupling changes.  A step launches hit (substrate only), bin + cell sort, columns,
 * deposit (substrate only) and tally; it allocates nothing and does not wait for the device.  With a laser surface set
 * (host/laser_surface.c) and a snapshot taken, the facets of phi = level follow the boundary records in one candidate list,
 * and the step adds the surface deposit; without one, the step's launches and their arguments are what they were. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "dedflow.h"
#include "dedflow_kernels.h"
#include "host_private.h"

#define LASER_MAX_COLUMNS 256
#define LASER_MAX_FACES (1 << 24)

static LaserState* laser(const ParticleContext* ctx) { return ((ParticleExt*)ctx->ext)->laser; }

static void free_substrate(LaserState* l) {
    CdamFreeDevice(l->tri, 0); CdamFreeDevice(l->snode, 0); CdamFreeDevice(l->soff, 0); CdamFreeDevice(l->sface, 0);
    CdamFreeDevice(l->power, 0); CdamFreeDevice(l->energy, 0);
    l->tri = NULL;
    l->snode = l->soff = l->sface = NULL;
    l->power = l->energy = NULL;
    l->nf = l->ns = 0;
    l->time = 0.0;
}

void DflLaserFree(ParticleContext* ctx) {
    ParticleExt* x = (ParticleExt*)ctx->ext;
    LaserState* l = x->laser;
    if (!l) return;
    HIPGUARD(hipStreamSynchronize(DflStream()));
    DflParticleFieldsFree(ctx, DFL_PF_LASER);
    DflLaserSurfaceFree(l);
    CdamFreeDevice(l->count, 0); CdamFreeDevice(l->cell_start, 0); CdamFreeDevice(l->chunk_sum, 0);
    free_substrate(l);
    CdamFreeDevice(l->gw, 0);
    CdamFreeDevice(l->colkey, 0); CdamFreeDevice(l->col_T, 0); CdamFreeDevice(l->part, 0); CdamFreeDevice(l->tally, 0);
    CdamFreeDevice(l->col_face, 0);
    CdamFreeHost(l, SIZE_OF(LaserState));
    x->laser = NULL;
}

/* what the capacity sizes beside the table's per-particle buffers: the bins of the column sort; and a zero rate */
static void bin_buffers(LaserState* l, index_type cap) {
    const ptrdiff_t n = cap > 0 ? cap : 1;
    CdamFreeDevice(l->count, 0); CdamFreeDevice(l->cell_start, 0); CdamFreeDevice(l->chunk_sum, 0);
    hipStream_t s = DflStream();
    HIPGUARD(hipMemsetAsync(l->rate, 0, (size_t)n * sizeof(f64), s));
    /* the bins: every column, then one per 2^DFL_LASER_OUTSIDE_SHIFT particle ids for the particles outside the grid */
    const index_type nbin = l->ncol + (index_type)((n - 1) >> DFL_LASER_OUTSIDE_SHIFT) + 1;
    const index_type nchunk = dfl_scan_num_chunks(nbin);
    l->count = (index_type*)CdamMallocDevice(((ptrdiff_t)nbin + 1) * SIZE_OF(index_type));
    l->cell_start = (index_type*)CdamMallocDevice(((ptrdiff_t)nbin + 1) * SIZE_OF(index_type));
    l->chunk_sum = (index_type*)CdamMallocDevice((ptrdiff_t)nchunk * SIZE_OF(index_type));
    HIPGUARD(hipMemsetAsync(l->count, 0, ((size_t)nbin + 1) * sizeof(index_type), s)); /* every sort leaves it zeroed again */
    HIPGUARD(hipMemsetAsync(l->cell_start, 0, ((size_t)nbin + 1) * sizeof(index_type), s));
    HIPGUARD(hipMemsetAsync(l->chunk_sum, 0, (size_t)nchunk * sizeof(index_type), s));
    l->nbin = nbin;
}

/* the weights and per-column outputs of an n x n grid */
static void column_buffers(LaserState* l) {
    const index_type n = l->n, ncol = l->ncol;
    const f64 w = l->cfg.w, h = l->cfg.h;
    f64* g = (f64*)malloc((size_t)2 * n * sizeof(f64));
    f64 prev = erf((M_SQRT2 * ((f64)(-n / 2) * h)) / w);
    for (index_type i = 0; i < n; ++i) {
        const f64 next = erf((M_SQRT2 * ((f64)(i + 1 - n / 2) * h)) / w);
        g[i] = g[n + i] = next - prev;
        prev = next;
    }
    l->gw = (f64*)CdamMallocDevice((ptrdiff_t)2 * n * SIZE_OF(f64));
    HIPGUARD(hipMemcpy(l->gw, g, (size_t)2 * n * sizeof(f64), H2D));
    free(g);
    l->colkey = (uint64_t*)CdamMallocDevice((ptrdiff_t)ncol * SIZE_OF(uint64_t));
    l->col_T = (f64*)CdamMallocDevice((ptrdiff_t)ncol * SIZE_OF(f64));
    l->part = (f64*)CdamMallocDevice((ptrdiff_t)ncol * 6 * SIZE_OF(f64));
    l->tally = (f64*)CdamMallocDevice(6 * SIZE_OF(f64));
    l->col_face = (index_type*)CdamMallocDevice((ptrdiff_t)ncol * SIZE_OF(index_type));
    hipStream_t s = DflStream();
    HIPGUARD(hipMemsetAsync(l->colkey, 0xff, (size_t)ncol * sizeof(uint64_t), s)); /* no hit; rewritten only with a substrate */
    HIPGUARD(hipMemsetAsync(l->col_T, 0, (size_t)ncol * sizeof(f64), s));
    HIPGUARD(hipMemsetAsync(l->col_face, 0xff, (size_t)ncol * sizeof(index_type), s));
    HIPGUARD(hipMemsetAsync(l->tally, 0, 6 * sizeof(f64), s));
}

static int cmp_node_entry(const void* a, const void* b) {
    const int64_t x = *(const int64_t*)a, y = *(const int64_t*)b;
    return (x > y) - (x < y);
}

/* the substrate list of the coupled mesh (none when uncoupled or the mask is 0); nothing pending afterwards */
static void build_substrate(ParticleContext* ctx, LaserState* l) {
    HIPGUARD(hipStreamSynchronize(DflStream()));
    free_substrate(l);
    /* no face, no hit: the keys of the last step name faces of the list that has just gone (only a step with candidate
       faces rewrites them) */
    HIPGUARD(hipMemsetAsync(l->colkey, 0xff, (size_t)l->ncol * sizeof(uint64_t), DflStream()));
    Mesh3D* mesh = DflParticleCoupledMesh(ctx);
    if (!mesh || l->cfg.substrate_groups == 0) return;
    index_type nall = 0;
    f64 lo[3], hi[3];
    dfl_wall_tri* all = DflMeshBoundaryTris(mesh, l->cfg.substrate_groups, &nall, lo, hi, NULL);
    index_type nf = 0;
    l->vdmin = HUGE_VAL;
    l->vdmax = -HUGE_VAL;
    for (index_type t = 0; t < nall; ++t) { /* ascending record id; the record keeps its id */
        const f64* nn = all[t].n;
        if (!((nn[0] * l->dir[0] + nn[1] * l->dir[1]) + nn[2] * l->dir[2] < 0.0)) continue;
        all[nf] = all[t];
        for (int k = 0; k < 3; ++k) {
            const f64* v = all[nf].v + 3 * k;
            const f64 vd = (v[0] * l->dir[0] + v[1] * l->dir[1]) + v[2] * l->dir[2];
            if (vd < l->vdmin) l->vdmin = vd;
            if (vd > l->vdmax) l->vdmax = vd;
        }
        ++nf;
    }
    if (nf > LASER_MAX_FACES) {
        fprintf(stderr, "ParticleContextSetLaser: %d candidate substrate faces, at most %d; the beam misses the substrate\n", (int)nf,
                LASER_MAX_FACES);
        nf = 0;
    }
    if (nf == 0) {
        free(all);
        return;
    }
    /* (node, face, local vertex) sorted by node then face: the distinct nodes and, per node, its faces ascending */
    int64_t* ent = (int64_t*)malloc((size_t)3 * nf * sizeof(int64_t));
    for (index_type f = 0; f < nf; ++f)
        for (int k = 0; k < 3; ++k) ent[3 * (size_t)f + k] = ((int64_t)all[f].node[k] << 32) | (int64_t)(4 * f + k);
    qsort(ent, (size_t)3 * nf, sizeof(int64_t), cmp_node_entry);
    index_type* snode = (index_type*)malloc((size_t)3 * nf * sizeof(index_type));
    index_type* soff = (index_type*)malloc(((size_t)3 * nf + 1) * sizeof(index_type));
    index_type* sface = (index_type*)malloc((size_t)3 * nf * sizeof(index_type));
    index_type ns = 0;
    for (index_type e = 0; e < 3 * nf; ++e) {
        const index_type node = (index_type)(ent[e] >> 32);
        if (ns == 0 || snode[ns - 1] != node) {
            snode[ns] = node;
            soff[ns] = e;
            ++ns;
        }
        sface[e] = (index_type)(ent[e] & 0xffffffff);
    }
    soff[ns] = 3 * nf;
    l->tri = (dfl_wall_tri*)CdamMallocDevice((ptrdiff_t)nf * SIZE_OF(dfl_wall_tri));
    l->snode = (index_type*)CdamMallocDevice((ptrdiff_t)ns * SIZE_OF(index_type));
    l->soff = (index_type*)CdamMallocDevice(((ptrdiff_t)ns + 1) * SIZE_OF(index_type));
    l->sface = (index_type*)CdamMallocDevice((ptrdiff_t)3 * nf * SIZE_OF(index_type));
    l->power = (f64*)CdamMallocDevice((ptrdiff_t)ns * SIZE_OF(f64));
    l->energy = (f64*)CdamMallocDevice((ptrdiff_t)ns * SIZE_OF(f64));
    HIPGUARD(hipMemcpy(l->tri, all, (size_t)nf * sizeof(dfl_wall_tri), H2D));
    HIPGUARD(hipMemcpy(l->snode, snode, (size_t)ns * sizeof(index_type), H2D));
    HIPGUARD(hipMemcpy(l->soff, soff, ((size_t)ns + 1) * sizeof(index_type), H2D));
    HIPGUARD(hipMemcpy(l->sface, sface, (size_t)3 * nf * sizeof(index_type), H2D));
    HIPGUARD(hipMemset(l->power, 0, (size_t)ns * sizeof(f64)));
    HIPGUARD(hipMemset(l->energy, 0, (size_t)ns * sizeof(f64)));
    l->nf = nf;
    l->ns = ns;
    free(sface);
    free(soff);
    free(snode);
    free(ent);
    free(all);
}

void ParticleContextSetLaser(ParticleContext* ctx, const DflLaser* cfg) {
    ParticleExt* x = (ParticleExt*)ctx->ext;
    if (!cfg) {
        DflLaserFree(ctx);
        return;
    }
    if (!x->heat) {
        fprintf(stderr, "ParticleContextSetLaser: particle heat is off (ParticleContextSetHeat); unchanged\n");
        return;
    }
    const f64* d = cfg->dir;
    const f64 len = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    if (!(len > 0.0 && isfinite(len))) {
        fprintf(stderr, "ParticleContextSetLaser: the direction is zero or not finite; unchanged\n");
        return;
    }
    b32 finite = TRUE;
    for (int k = 0; k < 3; ++k) finite = finite && isfinite(cfg->origin[k]) && isfinite(cfg->scan_vel[k]);
    if (!(finite && cfg->power >= 0.0 && isfinite(cfg->power) && cfg->w > 0.0 && isfinite(cfg->w) && cfg->h > 0.0 && isfinite(cfg->h) &&
          cfg->r_cut > 0.0 && isfinite(cfg->r_cut) && cfg->eta_p >= 0.0 && cfg->eta_p <= 1.0 && cfg->eta_s >= 0.0 && cfg->eta_s <= 1.0)) {
        fprintf(stderr, "ParticleContextSetLaser: need finite origin and scan_vel, power >= 0, w, h, r_cut > 0 and eta_p, eta_s in [0, 1]; unchanged\n");
        return;
    }
    const f64 nside = 2.0 * ceil(cfg->r_cut / cfg->h);
    if (!(nside <= (f64)LASER_MAX_COLUMNS)) {
        fprintf(stderr, "ParticleContextSetLaser: r_cut / h gives %g columns per side, at most %d; unchanged\n", nside, LASER_MAX_COLUMNS);
        return;
    }
    const f64 rmax = ParticleContextMaxRadius(ctx);
    if (!(cfg->h >= 2.0 * rmax)) {
        fprintf(stderr, "ParticleContextSetLaser: column edge h = %g is below 2 Rmax = %g; unchanged\n", cfg->h, 2.0 * rmax);
        return;
    }
    /* a laser surface set on the context keeps its configuration and loses its snapshot (host/laser_surface.c) */
    const b32 had_surface = x->laser && x->laser->surf;
    const b32 had_reflection = had_surface && x->laser->surf->refl;
    DflLaserSurface surface;
    DflLaserReflection reflection;
    if (had_surface) surface = x->laser->surf->cfg;
    if (had_reflection) reflection = x->laser->surf->refl->cfg;
    DflLaserFree(ctx);
    LaserState* l = (LaserState*)CdamMallocHost(SIZE_OF(LaserState));
    memset(l, 0, sizeof *l);
    l->cfg = *cfg;
    for (int k = 0; k < 3; ++k) l->dir[k] = d[k] / len;
    int axis = 0; /* the coordinate axis least aligned with dir, the lowest on a tie */
    for (int k = 1; k < 3; ++k)
        if (fabs(l->dir[k]) < fabs(l->dir[axis])) axis = k;
    f64 t[3];
    for (int k = 0; k < 3; ++k) t[k] = (k == axis ? 1.0 : 0.0) - l->dir[axis] * l->dir[k];
    const f64 tl = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
    for (int k = 0; k < 3; ++k) l->e1[k] = t[k] / tl;
    l->e2[0] = l->dir[1] * l->e1[2] - l->dir[2] * l->e1[1];
    l->e2[1] = l->dir[2] * l->e1[0] - l->dir[0] * l->e1[2];
    l->e2[2] = l->dir[0] * l->e1[1] - l->dir[1] * l->e1[0];
    l->n = (index_type)nside;
    l->ncol = l->n * l->n;
    column_buffers(l);
    x->laser = l;
    DflParticleFieldsAlloc(ctx, DFL_PF_LASER);
    bin_buffers(l, x->cap);
    build_substrate(ctx, l);
    if (had_surface) DflLaserSurfaceInstall(ctx, &surface);
    if (had_reflection) DflLaserReflectInstall(l, &reflection);
}

void DflLaserCouplingChanged(ParticleContext* ctx) {
    LaserState* l = laser(ctx);
    if (l) build_substrate(ctx, l);
    DflLaserSurfaceCouplingChanged(ctx);
}

void DflLaserCapacityChanged(ParticleContext* ctx) {
    LaserState* l = laser(ctx);
    if (l) bin_buffers(l, ((ParticleExt*)ctx->ext)->cap);
}

void DflLaserCopy(ParticleContext* dst, const ParticleContext* src) {
    const LaserState* ls = laser(src);
    if (!ls) {
        DflLaserFree(dst);
        return;
    }
    ParticleContextSetLaser(dst, &ls->cfg);
    if (!laser(dst)) return;
    laser(dst)->t = ls->t;
    if (ls->surf) {
        DflLaserSurfaceInstall(dst, &ls->surf->cfg); /* the configuration, not the snapshot or pending energy */
        if (ls->surf->refl) DflLaserReflectInstall(laser(dst), &ls->surf->refl->cfg);
        else DflLaserReflectFree(laser(dst)->surf);
    } else ParticleContextSetLaserSurface(dst, NULL);
}

void DflLaserStep(ParticleContext* ctx, f64 dt) {
    ParticleExt* x = (ParticleExt*)ctx->ext;
    LaserState* l = x->laser;
    const index_type P = ctx->num_particle;
    hipStream_t s = DflStream();
    DflRangePush("ParticleContextLaserStep");
    l->t += dt;
    dfl_laser_beam b;
    for (int k = 0; k < 3; ++k) {
        b.o[k] = l->cfg.origin[k] + l->cfg.scan_vel[k] * l->t;
        b.e1[k] = l->e1[k];
        b.e2[k] = l->e2[k];
        b.dir[k] = l->dir[k];
    }
    b.h = l->cfg.h;
    b.area = l->cfg.h * l->cfg.h;
    b.n = l->n;
    /* with a snapshot of the level-set surface its facets follow the boundary records in one candidate list; with a surface
       set the depth range is that of the mesh's bounding box (host/laser_surface.c) */
    const LaserSurface* sf = l->surf;
    const index_type nfs = sf && sf->nf > 0 ? sf->nf : 0;
    const dfl_wall_tri* tri = nfs > 0 ? sf->cand : l->tri;
    if (l->nf + nfs > 0) { /* depths on a 2^-40 grid of the candidates' range as seen from this step's origin */
        const f64 vdmin = sf ? sf->vdmin : l->vdmin, vdmax = sf ? sf->vdmax : l->vdmax;
        const f64 od = (b.o[0] * b.dir[0] + b.o[1] * b.dir[1]) + b.o[2] * b.dir[2];
        const f64 range = vdmax - vdmin;
        f64 pad = 1e-6 * (range + fabs(vdmin) + fabs(vdmax) + fabs(od));
        if (!(pad > 0.0)) pad = 1.0;
        dfl_laser_hit(l->nf + nfs, tri, b, (vdmin - od) - pad, 1099511627776.0 / (range + 2.0 * pad), l->colkey, s);
    }
    if (P > 0) {
        dfl_laser_bin(P, ArrayData(ParticleCTXDeviceCoord(ctx)), b, l->cell_of, l->rank, l->count, l->rate, s);
        dfl_dem_sort_binned(P, l->nbin, ArrayData(ParticleCTXDeviceCoord(ctx)), ArrayData(ParticleCTXDeviceVel(ctx)), NULL,
                            x->radius, l->cell_of, l->rank, l->count, l->chunk_sum, l->cell_start, l->slot, l->order, l->sorted, NULL,
                            l->sorted_r, s);
    }
    dfl_laser_columns(P, b, l->cfg.power, l->cfg.eta_p, l->cfg.eta_s, l->gw, l->cell_start, l->order, l->sorted,
                      x->radius ? l->sorted_r : NULL, ParticleRadius(ctx), tri, l->colkey, l->k_tau, l->k_id, l->rate, l->col_T,
                      l->col_face, l->part, s);
    if (l->ns > 0) dfl_laser_deposit(l->ns, l->soff, l->sface, tri, b, l->cfg.eta_s, dt, l->colkey, l->col_T, l->power, l->energy, s);
    if (nfs > 0) DflLaserSurfaceDeposit(l, b, dt);
    else if (sf && sf->refl) DflLaserReflectIdle(l); /* no facets, no ray: the reflection tally of this step is zero */
    if (l->ns > 0 || nfs > 0) l->time += dt;
    dfl_laser_tally(l->ncol, l->cfg.power, l->part, l->tally, s);
    DflRangePop();
}

void ParticleContextLaserStep(ParticleContext* ctx, f64 dt) {
    ASSERT(laser(ctx) && "ParticleContextLaserStep: the laser is off (ParticleContextSetLaser)");
    if (laser(ctx)) DflLaserStep(ctx, dt);
}

const f64* ParticleContextLaserRate(const ParticleContext* ctx) { return laser(ctx) ? laser(ctx)->rate : NULL; }

void ParticleContextLaserTally(ParticleContext* ctx, DflLaserTally* out) {
    const LaserState* l = laser(ctx);
    memset(out, 0, sizeof *out);
    if (!l) return;
    f64 v[6];
    hipStream_t s = DflStream();
    HIPGUARD(hipMemcpyAsync(v, l->tally, sizeof v, D2H, s));
    HIPGUARD(hipStreamSynchronize(s));
    out->outside = v[0];
    out->absorbed_particles = v[1];
    out->scattered = v[2];
    out->substrate = v[3];
    out->reflected = v[4];
    out->missed = v[5];
}

index_type ParticleContextLaserColumns(const ParticleContext* ctx, const f64** transmitted, const index_type** face) {
    const LaserState* l = laser(ctx);
    *transmitted = l ? l->col_T : NULL;
    *face = l ? l->col_face : NULL;
    return l ? l->ncol : 0;
}

b32 DflLaserPending(const ParticleContext* ctx) {
    const LaserState* l = laser(ctx);
    return l && (l->ns > 0 || (l->surf && (l->surf->dirty || l->surf->carry_on))) && l->time > 0.0;
}

void DflLaserAddSource(ParticleContext* ctx, f64* q) {
    LaserState* l = laser(ctx);
    if (!DflLaserPending(ctx)) return;
    dfl_laser_source_add(l->ns, l->snode, 1.0 / l->time, l->energy, q, DflStream());
    DflLaserSurfaceAddSource(l, q);
    l->time = 0.0;
}
