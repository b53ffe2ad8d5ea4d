/* The laser's reflections on the level-set surface (build-defined, opt-in; model in include/dedflow.h, "laser reflections",
 * kernels in dedflow_amd/csrc/k_laser_reflect.hip).
 *
 * State (LaserSurface.refl, NULL when off): the configuration; the reflection list R of the last Update -- facets, tets,
 * gradients, (i, j, t) per vertex --; per (bounce, column) the facet, absorbed power and weights of the last step, per column
 * the power that escaped or remained, the deposit records, and the reflection tally on the device.  With a reflection set,
 * ParticleContextLaserSurfaceUpdate (host/laser_surface.c) also counts and emits R -- its total rides on Update's one
 * synchronisation -- and builds the surface's node list over the tets of R, so fslot is indexed by R.  A laser step allocates
 * nothing and does not wait: trace, records, sort, sum, tally. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "dedflow.h"
#include "dedflow_kernels.h"
#include "host_private.h"

#define LASER_REFLECT_FIRST_CAP 128
#define LASER_REFLECT_NTALLY 20
#define LASER_REFLECT_GROUP 64 /* lanes per ray: a wave; DESIGN.md has the measurement against 16 */

static LaserState* laser(const ParticleContext* ctx) { return ((ParticleExt*)ctx->ext)->laser; }
static LaserReflect* reflect(const ParticleContext* ctx) {
    const LaserState* l = laser(ctx);
    return l && l->surf ? l->surf->refl : NULL;
}

int DflLaserReflectionCheck(const DflLaserReflection* cfg, char* why, size_t why_len) {
    const char* msg = NULL;
    char buf[128];
    if (!cfg) msg = "no configuration";
    else if (cfg->max_bounce < 1 || cfg->max_bounce > 8) {
        snprintf(buf, sizeof buf, "max_bounce must be in 1..8, got %d", (int)cfg->max_bounce);
        msg = buf;
    } else if (cfg->model != 0 && cfg->model != 1) {
        snprintf(buf, sizeof buf, "model must be 0 or 1, got %d", (int)cfg->model);
        msg = buf;
    } else if (cfg->model == 1 && !(isfinite(cfg->eps) && cfg->eps > 0.0)) {
        snprintf(buf, sizeof buf, "eps must be finite and > 0 under model 1, got %g", cfg->eps);
        msg = buf;
    }
    if (why && why_len > 0) snprintf(why, why_len, "%s", msg ? msg : "");
    return msg ? 1 : 0;
}

static void free_cells(LaserReflect* r) {
    CdamFreeDevice(r->cell_count, 0); CdamFreeDevice(r->cell_start, 0); CdamFreeDevice(r->cell_chunk, 0);
    CdamFreeDevice(r->cell_entry, 0);
    r->cell_count = r->cell_start = r->cell_chunk = r->cell_entry = NULL;
    r->ncell = r->cap_cell = r->nentry = r->cap_entry = 0;
}

static void free_lists(LaserReflect* r) {
    CdamFreeDevice(r->facets, 0); CdamFreeDevice(r->grad, 0); CdamFreeDevice(r->ft, 0);
    CdamFreeDevice(r->tet, 0); CdamFreeDevice(r->fij, 0);
    r->facets = r->grad = r->ft = NULL;
    r->tet = r->fij = NULL;
    r->cap = r->nr = 0;
}

static void alloc_lists(LaserReflect* r, index_type cap) {
    free_lists(r);
    const ptrdiff_t c = cap;
    r->cap = cap;
    r->facets = (f64*)CdamMallocDevice(c * 9 * SIZE_OF(f64));
    r->grad = (f64*)CdamMallocDevice(c * 3 * SIZE_OF(f64));
    r->ft = (f64*)CdamMallocDevice(c * 3 * SIZE_OF(f64));
    r->tet = (index_type*)CdamMallocDevice(c * SIZE_OF(index_type));
    r->fij = (index_type*)CdamMallocDevice(c * SIZE_OF(index_type));
}

void DflLaserReflectFree(LaserSurface* s) {
    LaserReflect* r = s ? s->refl : NULL;
    if (!r) return;
    HIPGUARD(hipStreamSynchronize(DflStream()));
    free_lists(r);
    free_cells(r);
    CdamFreeDevice(r->visited, 0);
    DflBlockScanFree(&r->scan);
    CdamFreeDevice(r->hit_facet, 0); CdamFreeDevice(r->hit_abs, 0); CdamFreeDevice(r->hit_w, 0); CdamFreeDevice(r->ray_end, 0);
    CdamFreeDevice(r->rkey, 0); CdamFreeDevice(r->rkey_out, 0); CdamFreeDevice(r->rval, 0); CdamFreeDevice(r->temp, 0);
    CdamFreeDevice(r->tally, 0);
    CdamFreeHost(r, SIZE_OF(LaserReflect));
    s->refl = NULL;
}

void DflLaserReflectDropLists(LaserSurface* s) {
    if (!s->refl) return;
    s->refl->nr = 0;
    s->refl->ncell = s->refl->nentry = 0;
    s->refl->stepped = FALSE;
}

void DflLaserReflectMeshChanged(LaserSurface* s) {
    LaserReflect* r = s->refl;
    if (!r) return;
    HIPGUARD(hipStreamSynchronize(DflStream()));
    free_lists(r);
    free_cells(r);
    DflBlockScanFree(&r->scan);
    r->stepped = FALSE;
    HIPGUARD(hipMemsetAsync(r->tally, 0, LASER_REFLECT_NTALLY * sizeof(f64), DflStream()));
    if (!s->mesh) return;
    DflBlockScanAlloc(&r->scan, s->T, 0);
    alloc_lists(r, LASER_REFLECT_FIRST_CAP);
    if (s->N > 0) DflMeshNodeBounds(s->mesh, r->lo, r->hi);
}

/* the grid of this Update: n cells per axis, from DFL_LASER_REFLECT_CELLS or about two facets per cell of a surface that
 * crosses the box once (nr ~ 2 n^2 facets lie in ~ n^2 of the n^3 cells), n <= 128 */
static void build_cells(LaserState* l, index_type nr) {
    LaserReflect* r = l->surf->refl;
    hipStream_t st = DflStream();
    index_type n = r->cells_env;
    if (n <= 0) {
        n = (index_type)ceil(sqrt((f64)nr / 4.0));
        n = n < 1 ? 1 : (n > 128 ? 128 : n);
    }
    for (int k = 0; k < 3; ++k) {
        const f64 ext = r->hi[k] - r->lo[k];
        r->grid.lo[k] = r->lo[k];
        r->grid.n[k] = ext > 0.0 && isfinite(ext) ? n : 1;
        r->grid.inv[k] = ext > 0.0 && isfinite(ext) ? (f64)n / ext : 1.0;
    }
    const index_type ncell = r->grid.n[0] * r->grid.n[1] * r->grid.n[2];
    if (ncell > r->cap_cell) {
        CdamFreeDevice(r->cell_count, 0); CdamFreeDevice(r->cell_start, 0); CdamFreeDevice(r->cell_chunk, 0);
        r->cap_cell = ncell;
        r->cell_count = (index_type*)CdamMallocDevice((ptrdiff_t)ncell * SIZE_OF(index_type));
        r->cell_start = (index_type*)CdamMallocDevice(((ptrdiff_t)ncell + 1) * SIZE_OF(index_type));
        r->cell_chunk = (index_type*)CdamMallocDevice((ptrdiff_t)dfl_scan_num_chunks(ncell) * SIZE_OF(index_type));
    }
    HIPGUARD(hipMemsetAsync(r->cell_count, 0, (size_t)ncell * sizeof(index_type), st));
    dfl_laser_reflect_cells_count(nr, r->facets, r->grid, r->cell_count, st);
    dfl_scan_counts(ncell, r->cell_count, r->cell_chunk, r->cell_start, st);
    index_type total = 0;
    HIPGUARD(hipMemcpyAsync(&total, r->cell_start + ncell, sizeof total, D2H, st));
    HIPGUARD(hipStreamSynchronize(st)); /* one more read of four bytes, in Update only: the entries */
    if (total > r->cap_entry) {
        CdamFreeDevice(r->cell_entry, 0);
        r->cap_entry = DflGrowCap(total);
        r->cell_entry = (index_type*)CdamMallocDevice((ptrdiff_t)r->cap_entry * SIZE_OF(index_type));
    }
    dfl_laser_reflect_cells_emit(nr, r->facets, r->grid, r->cell_start, r->cell_count, r->cell_entry, total, st);
    r->ncell = ncell;
    r->nentry = total;
}

static index_type env_int(const char* name, index_type lo, index_type hi, index_type dflt) {
    const char* env = getenv(name);
    if (!env || !*env) return dflt;
    char* end = NULL;
    const long v = strtol(env, &end, 10);
    if (end == env || *end || v < lo || v > hi) {
        fprintf(stderr, "ParticleContextSetLaserReflection: %s must be an integer in %d..%d, got '%s'; ignored\n", name, (int)lo, (int)hi, env);
        return dflt;
    }
    return (index_type)v;
}

/* the node list of a snapshot taken without R does not cover R's tets, and fslot of one taken with R is indexed by R: setting
 * or clearing a reflection drops the snapshot (pending energy is kept) */
static void drop_snapshot(LaserState* l) { DflLaserSurfaceDropSnapshot(l, l->surf->nf > 0 ? 0 : l->surf->nf); }

void DflLaserReflectInstall(LaserState* l, const DflLaserReflection* cfg) {
    LaserSurface* s = l->surf;
    const DflLaserReflection keep = *cfg; /* (cfg may live in the state that goes) */
    DflLaserReflectFree(s);
    drop_snapshot(l);
    LaserReflect* r = (LaserReflect*)CdamMallocHost(SIZE_OF(LaserReflect));
    memset(r, 0, sizeof *r);
    r->cfg = keep;
    r->nhit = (keep.max_bounce + 1) * l->ncol;
    const ptrdiff_t nh = r->nhit;
    r->hit_facet = (index_type*)CdamMallocDevice(nh * SIZE_OF(index_type));
    r->hit_abs = (f64*)CdamMallocDevice(nh * SIZE_OF(f64));
    r->hit_w = (f64*)CdamMallocDevice(nh * 3 * SIZE_OF(f64));
    r->ray_end = (f64*)CdamMallocDevice((ptrdiff_t)2 * l->ncol * SIZE_OF(f64));
    r->rkey = (uint64_t*)CdamMallocDevice(nh * 4 * SIZE_OF(uint64_t));
    r->rkey_out = (uint64_t*)CdamMallocDevice(nh * 4 * SIZE_OF(uint64_t));
    r->rval = (f64*)CdamMallocDevice(nh * 4 * SIZE_OF(f64));
    r->temp_bytes = dfl_laser_reflect_temp_bytes(4 * r->nhit);
    r->temp = CdamMallocDevice((ptrdiff_t)r->temp_bytes);
    r->tally = (f64*)CdamMallocDevice(LASER_REFLECT_NTALLY * SIZE_OF(f64));
    r->visited = (f64*)CdamMallocDevice((ptrdiff_t)l->ncol * SIZE_OF(f64));
    HIPGUARD(hipMemsetAsync(r->visited, 0, (size_t)l->ncol * sizeof(f64), DflStream()));
    r->cells_env = env_int("DFL_LASER_REFLECT_CELLS", 0, 256, 0); /* 0: sized from the facet count; -1 is not accepted */
    r->group = env_int("DFL_LASER_REFLECT_GROUP", 16, 64, LASER_REFLECT_GROUP);
    if (r->group != 16 && r->group != 64) r->group = LASER_REFLECT_GROUP;
    s->refl = r;
    DflLaserReflectMeshChanged(s);
}

void ParticleContextSetLaserReflection(ParticleContext* ctx, const DflLaserReflection* cfg) {
    LaserState* l = laser(ctx);
    if (!cfg) {
        if (l && l->surf && l->surf->refl) {
            DflLaserReflectFree(l->surf);
            drop_snapshot(l); /* its node list and slots were those of R */
        }
        return;
    }
    if (!l) {
        fprintf(stderr, "ParticleContextSetLaserReflection: the laser is off (ParticleContextSetLaser); unchanged\n");
        return;
    }
    if (!l->surf) {
        fprintf(stderr, "ParticleContextSetLaserReflection: the laser surface is off (ParticleContextSetLaserSurface); unchanged\n");
        return;
    }
    char why[128];
    if (DflLaserReflectionCheck(cfg, why, sizeof why)) {
        fprintf(stderr, "ParticleContextSetLaserReflection: %s; unchanged\n", why);
        return;
    }
    DflLaserReflectInstall(l, cfg);
}

void DflLaserReflectCount(LaserState* l, const f64* w, index_type* nr) {
    LaserSurface* s = l->surf;
    LaserReflect* r = s->refl;
    const Mesh3DData* dev = Mesh3DDevice(s->mesh);
    hipStream_t st = DflStream();
    dfl_laser_reflect_count(s->T, dev->ien, dev->xg, w, s->N, s->cfg.level, r->scan.count, st);
    DflBlockScanEnqueue(&r->scan, nr, st);
}

void DflLaserReflectEmit(LaserState* l, const f64* w, index_type nr) {
    LaserSurface* s = l->surf;
    LaserReflect* r = s->refl;
    const Mesh3DData* dev = Mesh3DDevice(s->mesh);
    if (nr > r->cap) alloc_lists(r, DflGrowCap(nr));
    dfl_laser_reflect_emit(s->T, dev->ien, dev->xg, w, s->N, s->cfg.level, r->scan.base, r->facets, r->tet, r->grad, r->fij, r->ft, nr,
                           DflStream());
    r->nr = nr;
    build_cells(l, nr);
}

void DflLaserReflectDeposit(LaserState* l, dfl_laser_beam b, f64 dt) {
    LaserSurface* s = l->surf;
    LaserReflect* r = s->refl;
    hipStream_t st = DflStream();
    dfl_laser_reflect_trace_grid(b, l->colkey, s->nfb, s->nf, s->cand, s->ftet, r->nr, r->facets, r->tet, r->grad, s->cfg.side,
                                 r->cfg.model, r->cfg.max_bounce, l->cfg.eta_s, r->cfg.eps, l->col_T, r->hit_facet, r->hit_abs, r->hit_w,
                                 r->ray_end, l->part, r->grid, r->ncell > 0 ? r->cell_start : NULL, r->cell_entry, r->group, r->visited, st);
    dfl_laser_reflect_deposit(r->nhit, r->hit_facet, r->hit_abs, r->hit_w, r->nr, r->fij, r->ft, s->fslot, dt, r->rkey, r->rkey_out,
                              r->rval, s->power, s->energy, r->temp, r->temp_bytes, st);
    dfl_laser_reflect_tally(l->ncol, r->cfg.max_bounce, r->hit_facet, r->hit_abs, r->ray_end, r->tally, st);
    r->stepped = TRUE;
}

void DflLaserReflectIdle(LaserState* l) {
    LaserReflect* r = l->surf->refl;
    HIPGUARD(hipMemsetAsync(r->tally, 0, LASER_REFLECT_NTALLY * sizeof(f64), DflStream()));
    r->stepped = FALSE;
}

void ParticleContextLaserReflectionTally(ParticleContext* ctx, DflLaserReflectionTally* out) {
    const LaserReflect* r = reflect(ctx);
    memset(out, 0, sizeof *out);
    if (!r) return;
    f64 v[LASER_REFLECT_NTALLY];
    hipStream_t st = DflStream();
    HIPGUARD(hipMemcpyAsync(v, r->tally, sizeof v, D2H, st));
    HIPGUARD(hipStreamSynchronize(st));
    for (int b = 0; b < 9; ++b) {
        out->absorbed[b] = v[b];
        out->rays[b] = (index_type)v[11 + b];
    }
    out->escaped = v[9];
    out->remaining = v[10];
}

void DflLaserReflectionGridStats(ParticleContext* ctx, index_type* entries, index_type* cells, f64* mean_visited, f64* max_visited) {
    const LaserReflect* r = reflect(ctx);
    *entries = *cells = 0;
    *mean_visited = *max_visited = 0.0;
    if (!r) return;
    const index_type ncol = laser(ctx)->ncol;
    f64* v = (f64*)malloc((size_t)ncol * sizeof(f64));
    HIPGUARD(hipMemcpy(v, r->visited, (size_t)ncol * sizeof(f64), D2H));
    f64 sum = 0.0;
    index_type rays = 0;
    for (index_type c = 0; c < ncol; ++c)
        if (v[c] > 0.0) {
            sum += v[c];
            ++rays;
            if (v[c] > *max_visited) *max_visited = v[c];
        }
    free(v);
    *mean_visited = rays ? sum / rays : 0.0;
    *entries = r->nentry;
    *cells = r->ncell;
}

index_type ParticleContextLaserReflectionRays(const ParticleContext* ctx, const index_type** facet, const f64** absorbed) {
    const LaserReflect* r = reflect(ctx);
    const b32 any = r && r->stepped;
    if (facet) *facet = any ? r->hit_facet : NULL;
    if (absorbed) *absorbed = any ? r->hit_abs : NULL;
    return r ? (any ? r->nhit : 0) : 0;
}

index_type ParticleContextLaserReflectionFacets(const ParticleContext* ctx, const f64** facets, const index_type** tet, const f64** grad) {
    const LaserReflect* r = reflect(ctx);
    const b32 any = r && r->nr > 0;
    if (facets) *facets = any ? r->facets : NULL;
    if (tet) *tet = any ? r->tet : NULL;
    if (grad) *grad = any ? r->grad : NULL;
    return r ? r->nr : -1;
}
