/* The laser's transmitted beam on the level-set surface phi = level (build-defined, opt-in; model in include/dedflow.h,
 * "laser on the level-set surface", kernels in dedflow_amd/csrc/k_laser_surface.hip).
 *
 * State (LaserState.surf, NULL when off): the configuration; per coupled mesh the workgroup counts of the tet passes and
 * the depth range of the node bounding box; the snapshot of the last Update -- the facets, their tets, (i, j, t) per
 * vertex, the candidate list of the laser (boundary records, then the facets as records), the distinct nodes of the facets'
 * tets with the slot of every (facet, local node) -- and, keyed by that node list, the nodal power of the last step and the
 * energy since the last heat source; per column grid the deposit records.  Update reads the facet count back once and
 * grows the facet-sized lists when the count exceeds their capacity; a laser step allocates nothing and does not wait.
 * Energy still pending when an Update replaces the node list moves to a dense [N] array first (allocated at the first such
 * Update) and reaches the next heat source from there. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "dedflow.h"
#include "dedflow_kernels.h"
#include "host_private.h"

#define LASER_MAX_RECORDS (1 << 24)
#define LASER_SURFACE_FIRST_CAP 128 /* facets the lists hold before the first Update that needs more */

static LaserState* laser(const ParticleContext* ctx) { return ((ParticleExt*)ctx->ext)->laser; }

static void free_lists(LaserSurface* s) {
    CdamFreeDevice(s->facets, 0); CdamFreeDevice(s->ft, 0); CdamFreeDevice(s->ftet, 0); CdamFreeDevice(s->fij, 0);
    CdamFreeDevice(s->nkey, 0); CdamFreeDevice(s->nkey_out, 0); CdamFreeDevice(s->nrec, 0); CdamFreeDevice(s->nrec_out, 0);
    CdamFreeDevice(s->nflag, 0); CdamFreeDevice(s->nstart, 0); CdamFreeDevice(s->fslot, 0); CdamFreeDevice(s->unode, 0);
    CdamFreeDevice(s->power, 0); CdamFreeDevice(s->energy, 0); CdamFreeDevice(s->temp, 0);
    s->facets = s->ft = s->power = s->energy = NULL;
    s->ftet = s->fij = s->nrec = s->nrec_out = s->nflag = s->nstart = s->fslot = s->unode = NULL;
    s->nkey = s->nkey_out = NULL;
    s->temp = NULL;
    s->cap = 0;
}

static void free_mesh_buffers(LaserSurface* s) {
    free_lists(s);
    DflBlockScanFree(&s->scan);
    CdamFreeDevice(s->cand, 0); CdamFreeDevice(s->carry, 0);
    s->cand = NULL;
    s->carry = NULL;
    s->cap_cand = 0;
    s->carry_on = s->dirty = FALSE;
    s->nf = -1;
    s->nn = 0;
    s->nfb = 0;
    s->mesh = NULL;
    s->N = s->T = 0;
}

/* the lists sized by the facet capacity (with the scan scratch of the 4 cap node heads and the sort scratch, which also
 * serves the 4 ncol deposit records) */
static void alloc_lists(LaserSurface* s, index_type cap, index_type ncol) {
    free_lists(s);
    const ptrdiff_t c = cap, c4 = 4 * (ptrdiff_t)cap;
    s->cap = cap;
    s->facets = (f64*)CdamMallocDevice(c * 9 * SIZE_OF(f64));
    s->ft = (f64*)CdamMallocDevice(c * 3 * SIZE_OF(f64));
    s->ftet = (index_type*)CdamMallocDevice(c * SIZE_OF(index_type));
    s->fij = (index_type*)CdamMallocDevice(c * SIZE_OF(index_type));
    s->nkey = (uint32_t*)CdamMallocDevice(c4 * SIZE_OF(uint32_t));
    s->nkey_out = (uint32_t*)CdamMallocDevice(c4 * SIZE_OF(uint32_t));
    s->nrec = (index_type*)CdamMallocDevice(c4 * SIZE_OF(index_type));
    s->nrec_out = (index_type*)CdamMallocDevice(c4 * SIZE_OF(index_type));
    s->nflag = (index_type*)CdamMallocDevice(c4 * SIZE_OF(index_type));
    s->nstart = (index_type*)CdamMallocDevice((c4 + 1) * SIZE_OF(index_type));
    s->fslot = (index_type*)CdamMallocDevice(c4 * SIZE_OF(index_type));
    s->unode = (index_type*)CdamMallocDevice(c4 * SIZE_OF(index_type));
    s->power = (f64*)CdamMallocDevice(c4 * SIZE_OF(f64));
    s->energy = (f64*)CdamMallocDevice(c4 * SIZE_OF(f64));
    DflBlockScanReserve(&s->scan, (index_type)c4);
    s->temp_bytes = dfl_laser_surface_temp_bytes((index_type)c4, 4 * ncol);
    s->temp = CdamMallocDevice((ptrdiff_t)s->temp_bytes);
}

/* the buffers of the coupled mesh (none when uncoupled) and the depth range of its node bounding box; no snapshot, nothing
 * pending afterwards.  Synchronises */
static void bind_mesh(ParticleContext* ctx, LaserState* l, LaserSurface* s) {
    hipStream_t st = DflStream();
    HIPGUARD(hipStreamSynchronize(st));
    free_mesh_buffers(s);
    /* the keys of the last step may name facets of the list that has just gone */
    HIPGUARD(hipMemsetAsync(l->colkey, 0xff, (size_t)l->ncol * sizeof(uint64_t), st));
    s->vdmin = s->vdmax = 0.0;
    Mesh3D* mesh = DflParticleCoupledMesh(ctx);
    if (!mesh) {
        DflLaserReflectMeshChanged(s);
        return;
    }
    const index_type N = Mesh3DNumNode(mesh), T = Mesh3DNumTet(mesh);
    s->mesh = mesh;
    s->N = N;
    s->T = T;
    DflLaserReflectMeshChanged(s);
    DflBlockScanAlloc(&s->scan, T, 0);
    alloc_lists(s, LASER_SURFACE_FIRST_CAP, l->ncol);
    if (N > 0) {
        f64 lo[3], hi[3];
        DflMeshNodeBounds(mesh, lo, hi);
        s->vdmin = HUGE_VAL;
        s->vdmax = -HUGE_VAL;
        for (int k = 0; k < 8; ++k) {
            const f64 c[3] = {k & 1 ? hi[0] : lo[0], k & 2 ? hi[1] : lo[1], k & 4 ? hi[2] : lo[2]};
            const f64 vd = (c[0] * l->dir[0] + c[1] * l->dir[1]) + c[2] * l->dir[2];
            if (vd < s->vdmin) s->vdmin = vd;
            if (vd > s->vdmax) s->vdmax = vd;
        }
    }
}

void DflLaserSurfaceFree(LaserState* l) {
    LaserSurface* s = l->surf;
    if (!s) return;
    HIPGUARD(hipStreamSynchronize(DflStream()));
    DflLaserReflectFree(s);
    free_mesh_buffers(s);
    CdamFreeDevice(s->rkey, 0); CdamFreeDevice(s->rkey_out, 0); CdamFreeDevice(s->rval, 0);
    CdamFreeHost(s, SIZE_OF(LaserSurface));
    l->surf = NULL;
}

void DflLaserSurfaceInstall(ParticleContext* ctx, const DflLaserSurface* cfg) {
    LaserState* l = laser(ctx);
    const DflLaserSurface keep = *cfg; /* (cfg may live in the state that goes) */
    const b32 had_reflection = l->surf && l->surf->refl; /* a reflection keeps its configuration, not its lists */
    DflLaserReflection reflection;
    if (had_reflection) reflection = l->surf->refl->cfg;
    DflLaserSurfaceFree(l);
    LaserSurface* s = (LaserSurface*)CdamMallocHost(SIZE_OF(LaserSurface));
    memset(s, 0, sizeof *s);
    s->cfg = keep;
    s->nf = -1;
    const ptrdiff_t r4 = 4 * (ptrdiff_t)l->ncol;
    s->rkey = (uint64_t*)CdamMallocDevice(r4 * SIZE_OF(uint64_t));
    s->rkey_out = (uint64_t*)CdamMallocDevice(r4 * SIZE_OF(uint64_t));
    s->rval = (f64*)CdamMallocDevice(r4 * SIZE_OF(f64));
    l->surf = s;
    bind_mesh(ctx, l, s);
    if (had_reflection) DflLaserReflectInstall(l, &reflection);
}

void ParticleContextSetLaserSurface(ParticleContext* ctx, const DflLaserSurface* cfg) {
    LaserState* l = laser(ctx);
    if (!cfg) {
        if (l && l->surf) {
            DflLaserSurfaceFree(l);
            HIPGUARD(hipMemsetAsync(l->colkey, 0xff, (size_t)l->ncol * sizeof(uint64_t), DflStream()));
        }
        return;
    }
    if (!l) {
        fprintf(stderr, "ParticleContextSetLaserSurface: the laser is off (ParticleContextSetLaser); unchanged\n");
        return;
    }
    if (!DflParticleCoupledMesh(ctx)) {
        fprintf(stderr, "ParticleContextSetLaserSurface: the context is not coupled to a mesh (ParticleContextSetFluidCoupling); unchanged\n");
        return;
    }
    if (cfg->side != 1 && cfg->side != -1) {
        fprintf(stderr, "ParticleContextSetLaserSurface: side must be +1 or -1, got %d; unchanged\n", (int)cfg->side);
        return;
    }
    if (!isfinite(cfg->level)) {
        fprintf(stderr, "ParticleContextSetLaserSurface: level is not finite (%g); unchanged\n", cfg->level);
        return;
    }
    DflLaserSurfaceInstall(ctx, cfg);
}

void DflLaserSurfaceCouplingChanged(ParticleContext* ctx) {
    LaserState* l = laser(ctx);
    if (l && l->surf) bind_mesh(ctx, l, l->surf);
}

/* the snapshot goes (nf as given: 0, or -1 for "no Update yet"): energy keyed by its node list moves to the dense array
 * first, the reflection lists go with it, and no key names a facet that goes */
void DflLaserSurfaceDropSnapshot(LaserState* l, index_type nf) {
    LaserSurface* s = l->surf;
    hipStream_t st = DflStream();
    if (s->nf > 0 && s->dirty) {
        if (!s->carry) {
            s->carry = (f64*)CdamMallocDevice((ptrdiff_t)s->N * SIZE_OF(f64));
            HIPGUARD(hipMemsetAsync(s->carry, 0, (size_t)s->N * sizeof(f64), st));
        }
        dfl_laser_surface_carry(4 * s->nn, s->nstart + 4 * (size_t)s->nn, s->unode, s->energy, s->carry, st);
        s->carry_on = TRUE;
    }
    s->dirty = FALSE;
    s->nf = nf;
    s->nn = 0;
    DflLaserReflectDropLists(s);
    HIPGUARD(hipMemsetAsync(l->colkey, 0xff, (size_t)l->ncol * sizeof(uint64_t), st));
}

index_type ParticleContextLaserSurfaceUpdate(ParticleContext* ctx, const f64* w) {
    LaserState* l = laser(ctx);
    LaserSurface* s = l ? l->surf : NULL;
    if (!s) return -1;
    hipStream_t st = DflStream();
    DflRangePush("ParticleContextLaserSurfaceUpdate");
    DflLaserSurfaceDropSnapshot(l, 0);
    s->nfb = l->nf;
    if (!s->mesh || s->N <= 0 || s->T <= 0) {
        DflRangePop();
        return 0;
    }
    const Mesh3DData* dev = Mesh3DDevice(s->mesh);
    dfl_laser_surface_count(s->T, dev->ien, dev->xg, w, s->N, s->cfg.level, s->cfg.side, l->dir, s->scan.count, st);
    index_type nf = 0, nr = 0;
    DflBlockScanEnqueue(&s->scan, &nf, st);
    if (s->refl) DflLaserReflectCount(l, w, &nr);
    HIPGUARD(hipStreamSynchronize(st)); /* the one synchronisation: the count (and that of the reflection list) */
    if (nf <= 0) {
        DflRangePop();
        return nf < 0 ? -1 : 0;
    }
    if ((int64_t)l->nf + nf > LASER_MAX_RECORDS) {
        fprintf(stderr, "ParticleContextLaserSurfaceUpdate: %d boundary candidates and %d facets, at most %d records; the facets "
                        "are dropped\n", (int)l->nf, (int)nf, LASER_MAX_RECORDS);
        DflRangePop();
        return nf;
    }
    if (s->refl && nr > LASER_MAX_RECORDS) {
        fprintf(stderr, "ParticleContextLaserSurfaceUpdate: %d facets in the reflection list, at most %d; no ray is reflected\n", (int)nr,
                LASER_MAX_RECORDS);
        nr = 0;
    }
    /* with a reflection list the node list covers the tets of all its facets (the candidates are among them) */
    const b32 with_r = s->refl && nr >= nf;
    const index_type nn = with_r ? nr : nf;
    if (nn > s->cap) alloc_lists(s, DflGrowCap(nn), l->ncol);
    if (l->nf + nf > s->cap_cand) {
        CdamFreeDevice(s->cand, 0);
        s->cap_cand = l->nf + (nf > s->cap ? nf : s->cap);
        s->cand = (dfl_wall_tri*)CdamMallocDevice((ptrdiff_t)s->cap_cand * SIZE_OF(dfl_wall_tri));
    }
    if (l->nf > 0) HIPGUARD(hipMemcpyAsync(s->cand, l->tri, (size_t)l->nf * sizeof(dfl_wall_tri), hipMemcpyDeviceToDevice, st));
    dfl_laser_surface_emit(s->T, dev->ien, dev->xg, w, s->N, s->cfg.level, s->cfg.side, l->dir, s->scan.base, s->cand + l->nf, s->facets,
                           s->ftet, s->fij, s->ft, nf, st);
    if (with_r) DflLaserReflectEmit(l, w, nr);
    dfl_laser_surface_nodes(nn, dev->ien, with_r ? s->refl->tet : s->ftet, s->nkey, s->nkey_out, s->nrec, s->nrec_out, s->nflag, s->scan.chunk_sum, s->nstart,
                            s->fslot, s->unode, s->temp, s->temp_bytes, st);
    HIPGUARD(hipMemsetAsync(s->power, 0, (size_t)4 * nn * sizeof(f64), st));
    HIPGUARD(hipMemsetAsync(s->energy, 0, (size_t)4 * nn * sizeof(f64), st));
    s->nf = nf;
    s->nn = nn;
    DflRangePop();
    return nf;
}

index_type ParticleContextLaserSurfaceFacets(const ParticleContext* ctx, const f64** facets, const index_type** tet) {
    const LaserState* l = laser(ctx);
    const LaserSurface* s = l ? l->surf : NULL;
    const b32 any = s && s->nf > 0;
    if (facets) *facets = any ? s->facets : NULL;
    if (tet) *tet = any ? s->ftet : NULL;
    return s ? (s->nf > 0 ? s->nf : 0) : -1;
}

void ParticleContextLaserSurfacePower(ParticleContext* ctx, f64* q) {
    LaserState* l = laser(ctx);
    LaserSurface* s = l ? l->surf : NULL;
    if (!s) {
        fprintf(stderr, "ParticleContextLaserSurfacePower: no laser surface is set on this context (ParticleContextSetLaserSurface)\n");
        return;
    }
    const index_type nmax = s->nf > 0 ? 4 * s->nn : 0;
    dfl_laser_surface_power(s->N, nmax, nmax ? s->nstart + nmax : NULL, s->unode, s->power, q, DflStream());
}

void DflLaserSurfaceDeposit(LaserState* l, dfl_laser_beam b, f64 dt) {
    LaserSurface* s = l->surf;
    if (s->refl && s->refl->nr > 0) {
        DflLaserReflectDeposit(l, b, dt);
        s->dirty = TRUE;
        return;
    }
    if (s->refl) DflLaserReflectIdle(l);
    dfl_laser_surface_deposit(b, l->colkey, s->nfb, s->nf, s->cand, s->fij, s->ft, s->fslot, l->cfg.eta_s, dt, l->col_T, s->rkey,
                              s->rkey_out, s->rval, s->power, s->energy, s->temp, s->temp_bytes, DflStream());
    s->dirty = TRUE;
}

void DflLaserSurfaceAddSource(LaserState* l, f64* q) {
    LaserSurface* s = l->surf;
    if (!s || !(l->time > 0.0)) return;
    hipStream_t st = DflStream();
    if (s->dirty && s->nf > 0)
        dfl_laser_surface_source_add(4 * s->nn, s->nstart + 4 * (size_t)s->nn, s->unode, 1.0 / l->time, s->energy, q, st);
    if (s->carry_on) dfl_laser_surface_carry_add(s->N, 1.0 / l->time, s->carry, q, st);
    s->dirty = s->carry_on = FALSE;
}

void DflLaserSurfaceTimeStep(ParticleContext* ctx, const f64* w) {
    const LaserState* l = laser(ctx);
    if (l && l->surf) ParticleContextLaserSurfaceUpdate(ctx, w);
}
