/* DEM walls from the boundary faces of a tet mesh (build-defined; contact model and de-duplication rule in
 * include/dedflow.h, kernels in dedflow_amd/csrc/k_walls.hip).
 *
 * At ParticleContextSetWallMesh, on the host: the faces of the masked groups become packed 128-byte records (vertices in
 * ascending local index of the parent tet, normal oriented towards the tet's opposite vertex, the node ids); the record
 * id is the position in group order.  At that call and again whenever ParticleRadius (Rmax when polydisperse) changes (a host-side comparison per
 * sweep): the particle grid and the wall grid over the bounding box padded by R.  Also at that call, for the contact keys of
 * the friction sweep: the plane id of every record (sort by the rounded plane, then de-duplication rule 1 within runs).  The wall grid is built on the host: it
 * is a one-time O(faces) job, and walking the faces in id order fills every cell's list in ascending id without a sort.
 * Per sweep nothing is allocated and nothing waits for the device. */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "dedflow.h"
#include "dedflow_kernels.h"
#include "host_private.h"

typedef struct WallState {
    index_type nf;
    dfl_wall_tri* h_tri;         /* host [nf] */
    dfl_wall_tri* tri;           /* device [nf] */
    f64 lo[3], hi[3];            /* bounding box of the mesh nodes */
    f64 scale;                   /* its diagonal: plane and distance tolerances are 1e-12 of it */
    f64 edge;                    /* median wall edge length */
    f64 R;                       /* radius the grids were built for (negative: none yet) */
    index_type P;
    dfl_grid3 pgrid, wgrid;
    index_type *wstart, *wlist;  /* device [wcells + 1], [entries] */
    index_type* plane;           /* device [nf]: plane id of every record (friction contact keys) */
    index_type* dropped;         /* device [1] */
} WallState;

#define WALL_GRID_MAX_CELLS (1 << 22)
#define PARTICLE_GRID_MAX_CELLS (1 << 24)

void DflWallsFree(WallState* w) {
    if (!w) return;
    HIPGUARD(hipStreamSynchronize(DflStream()));
    CdamFreeDevice(w->tri, 0); CdamFreeDevice(w->plane, 0); CdamFreeDevice(w->wstart, 0); CdamFreeDevice(w->wlist, 0); CdamFreeDevice(w->dropped, 0);
    free(w->h_tri);
    CdamFreeHost(w, SIZE_OF(WallState));
}

static int cmp_f64(const void* a, const void* b) {
    const f64 x = *(const f64*)a, y = *(const f64*)b;
    return (x > y) - (x < y);
}

static index_type clamp_cell(f64 v, index_type n) {
    const f64 c = floor(v);
    return c < 0.0 ? 0 : (c >= (f64)n ? n - 1 : (index_type)c);
}

/* the bounding box padded by R: origin and extent */
static void padded_box(const WallState* w, f64 R, f64 glo[3], f64 ext[3]) {
    for (int d = 0; d < 3; ++d) {
        glo[d] = w->lo[d] - R;
        ext[d] = (w->hi[d] - w->lo[d]) + 2.0 * R;
        if (!(ext[d] > 0.0)) ext[d] = 1.0;
    }
}

/* the particle grid: cell edge >= 4R per axis and about half a particle per cell, as the unit-box grid, over the bounding
 * box padded by R, with its cell count capped.  Host arithmetic only: a particle count change rebuilds just this */
static void build_particle_grid(WallState* w, f64 R, index_type P) {
    f64 glo[3], ext[3];
    padded_box(w, R, glo, ext);
    const f64 vol = ext[0] * ext[1] * ext[2];
    f64 h = cbrt(vol / (2.0 * (f64)(P > 0 ? P : 1)));
    if (h < 4.0 * R) h = 4.0 * R;
    for (;;) {
        f64 cells = 1.0;
        for (int d = 0; d < 3; ++d) {
            f64 n = floor(ext[d] / h);
            w->pgrid.n[d] = n < 1.0 ? 1 : (index_type)n;
            cells *= w->pgrid.n[d];
        }
        if (cells <= (f64)PARTICLE_GRID_MAX_CELLS) break;
        h *= 1.05;
    }
    for (int d = 0; d < 3; ++d) {
        w->pgrid.lo[d] = glo[d];
        w->pgrid.inv[d] = (f64)w->pgrid.n[d] / ext[d];
    }
    w->P = P;
}

/* the wall grid: cubic cells of max(2R, median wall edge) over the same padded box, with its cell count capped; the lists
 * are built on the host and uploaded (synchronises) */
static void build_wall_grid(WallState* w, f64 R) {
    f64 glo[3], ext[3];
    padded_box(w, R, glo, ext);
    f64 hw = w->edge > 2.0 * R ? w->edge : 2.0 * R;
    for (;;) {
        f64 cells = 1.0;
        for (int d = 0; d < 3; ++d) {
            f64 n = ceil(ext[d] / hw);
            w->wgrid.n[d] = n < 1.0 ? 1 : (index_type)n;
            cells *= w->wgrid.n[d];
        }
        if (cells <= (f64)WALL_GRID_MAX_CELLS) break;
        hw *= 1.05;
    }
    for (int d = 0; d < 3; ++d) {
        w->wgrid.lo[d] = glo[d];
        w->wgrid.inv[d] = 1.0 / hw;
    }
    const dfl_grid3* g = &w->wgrid;
    const size_t ncell = (size_t)g->n[0] * g->n[1] * g->n[2];
    index_type* start = (index_type*)calloc(ncell + 1, sizeof(index_type));
    /* a triangle is listed in every cell its bounding box expanded by R (and a hair, against rounding) overlaps */
    const f64 pad = R * (1.0 + 1e-9) + 1e-12 * w->scale;
    index_type (*range)[6] = (index_type(*)[6])malloc((size_t)(w->nf > 0 ? w->nf : 1) * sizeof *range);
    for (index_type t = 0; t < w->nf; ++t) {
        const f64* v = w->h_tri[t].v;
        for (int d = 0; d < 3; ++d) {
            f64 mn = v[d], mx = v[d];
            for (int k = 1; k < 3; ++k) {
                if (v[3 * k + d] < mn) mn = v[3 * k + d];
                if (v[3 * k + d] > mx) mx = v[3 * k + d];
            }
            range[t][2 * d] = clamp_cell((mn - pad - g->lo[d]) * g->inv[d], g->n[d]);
            range[t][2 * d + 1] = clamp_cell((mx + pad - g->lo[d]) * g->inv[d], g->n[d]);
        }
        for (index_type k = range[t][4]; k <= range[t][5]; ++k)
            for (index_type j = range[t][2]; j <= range[t][3]; ++j)
                for (index_type i = range[t][0]; i <= range[t][1]; ++i)
                    start[(size_t)i + (size_t)g->n[0] * ((size_t)j + (size_t)g->n[1] * k) + 1] += 1;
    }
    for (size_t c = 0; c < ncell; ++c) start[c + 1] += start[c];
    const index_type entries = start[ncell];
    index_type* list = (index_type*)malloc((size_t)(entries > 0 ? entries : 1) * sizeof(index_type));
    index_type* fill = (index_type*)malloc(ncell * sizeof(index_type));
    memcpy(fill, start, ncell * sizeof(index_type));
    for (index_type t = 0; t < w->nf; ++t) /* ascending t: every cell's list ascending */
        for (index_type k = range[t][4]; k <= range[t][5]; ++k)
            for (index_type j = range[t][2]; j <= range[t][3]; ++j)
                for (index_type i = range[t][0]; i <= range[t][1]; ++i)
                    list[fill[(size_t)i + (size_t)g->n[0] * ((size_t)j + (size_t)g->n[1] * k)]++] = t;
    HIPGUARD(hipStreamSynchronize(DflStream()));
    CdamFreeDevice(w->wstart, 0);
    CdamFreeDevice(w->wlist, 0);
    w->wstart = (index_type*)CdamMallocDevice((ptrdiff_t)(ncell + 1) * SIZE_OF(index_type));
    w->wlist = (index_type*)CdamMallocDevice((ptrdiff_t)(entries > 0 ? entries : 1) * SIZE_OF(index_type));
    HIPGUARD(hipMemcpy(w->wstart, start, (ncell + 1) * sizeof(index_type), H2D));
    HIPGUARD(hipMemcpy(w->wlist, list, (size_t)(entries > 0 ? entries : 1) * sizeof(index_type), H2D));
    free(fill);
    free(list);
    free(range);
    free(start);
    w->R = R;
}

static void build_grids(WallState* w, f64 R, index_type P) {
    build_particle_grid(w, R, P);
    build_wall_grid(w, R);
}

/* plane ids: the smallest record id among the records whose plane equals this one under de-duplication rule 1 (normals
 * equal to 1e-12, offsets to tol).  The records are sorted by their plane rounded to a grid much coarser than those
 * tolerances (2^-30 on the normal, 2^10 tol on the offset), then by id; within a run of equal rounded planes every record
 * joins the first earlier group of the run it matches.  Rounding noise splits a plane only when it straddles a grid line */
typedef struct PlaneKey {
    int64_t q[4];
    index_type id;
} PlaneKey;

static int cmp_plane_key(const void* a, const void* b) {
    const PlaneKey* x = (const PlaneKey*)a;
    const PlaneKey* y = (const PlaneKey*)b;
    for (int k = 0; k < 4; ++k)
        if (x->q[k] != y->q[k]) return x->q[k] < y->q[k] ? -1 : 1;
    return (x->id > y->id) - (x->id < y->id);
}

static b32 same_plane(const dfl_wall_tri* a, const dfl_wall_tri* b, f64 tol) {
    return fabs(a->n[0] - b->n[0]) <= 1e-12 && fabs(a->n[1] - b->n[1]) <= 1e-12 && fabs(a->n[2] - b->n[2]) <= 1e-12 &&
           fabs(a->off - b->off) <= tol;
}

static void plane_ids(const dfl_wall_tri* tri, index_type nf, f64 tol, index_type* plane) {
    PlaneKey* key = (PlaneKey*)malloc((size_t)(nf > 0 ? nf : 1) * sizeof(PlaneKey));
    const f64 qn = 1073741824.0, qo = 1.0 / (1024.0 * (tol > 0.0 ? tol : 1e-300));
    for (index_type t = 0; t < nf; ++t) {
        for (int d = 0; d < 3; ++d) key[t].q[d] = (int64_t)llround(tri[t].n[d] * qn);
        key[t].q[3] = (int64_t)llround(tri[t].off * qo);
        key[t].id = t;
    }
    qsort(key, (size_t)nf, sizeof(PlaneKey), cmp_plane_key);
    for (index_type a = 0; a < nf;) {
        index_type b = a + 1;
        while (b < nf && memcmp(key[b].q, key[a].q, sizeof key[a].q) == 0) ++b;
        /* run [a, b), ascending id: a record is a group leader unless it matches an earlier leader of the run */
        for (index_type r = a; r < b; ++r) {
            const index_type t = key[r].id;
            plane[t] = t;
            for (index_type u = a; u < r; ++u) {
                const index_type l = key[u].id;
                if (plane[l] == l && same_plane(&tri[l], &tri[t], tol)) {
                    plane[t] = l;
                    break;
                }
            }
        }
        a = b;
    }
    free(key);
}

/* the boundary faces of the masked groups as packed records, in group order (the record id), from host copies of what the
 * device holds (synchronises); also the bounding box of the mesh nodes and, when asked for, the 3 nf edge lengths.  The
 * caller frees both with free().  Shared with the laser's substrate list (host/laser.c) */
dfl_wall_tri* DflMeshBoundaryTris(Mesh3D* mesh, index_type group_mask, index_type* nf_out, f64 lo[3], f64 hi[3], f64** edges_out) {
    const index_type N = Mesh3DNumNode(mesh), T = Mesh3DNumTet(mesh);
    const index_type nb = mesh->num_bound;
    const index_type nfall = nb > 0 ? mesh->bound_elem_offset[nb] : 0;
    /* host copies of what the device holds */
    hipStream_t s = DflStream();
    HIPGUARD(hipStreamSynchronize(s));
    f64* xg = (f64*)malloc((size_t)N * 3 * sizeof(f64));
    index_type* ien = (index_type*)malloc((size_t)T * 4 * sizeof(index_type));
    index_type* f2e = (index_type*)malloc((size_t)(nfall > 0 ? nfall : 1) * sizeof(index_type));
    index_type* forn = (index_type*)malloc((size_t)(nfall > 0 ? nfall : 1) * sizeof(index_type));
    HIPGUARD(hipMemcpy(xg, Mesh3DDevice(mesh)->xg, (size_t)N * 3 * sizeof(f64), D2H));
    HIPGUARD(hipMemcpy(ien, Mesh3DDevice(mesh)->ien, (size_t)T * 4 * sizeof(index_type), D2H));
    if (nfall > 0) {
        HIPGUARD(hipMemcpy(f2e, mesh->bound_f2e, (size_t)nfall * sizeof(index_type), D2H));
        HIPGUARD(hipMemcpy(forn, mesh->bound_forn, (size_t)nfall * sizeof(index_type), D2H));
    }
    DflNodeBounds(xg, N, lo, hi);
    index_type nf = 0;
    for (index_type g = 0; g < nb && g < 31; ++g)
        if (group_mask >> g & 1) nf += mesh->bound_elem_offset[g + 1] - mesh->bound_elem_offset[g];
    dfl_wall_tri* tri = (dfl_wall_tri*)calloc((size_t)(nf > 0 ? nf : 1), sizeof(dfl_wall_tri));
    f64* edges = (f64*)malloc((size_t)(nf > 0 ? 3 * nf : 1) * sizeof(f64));
    index_type id = 0;
    for (index_type g = 0; g < nb && g < 31; ++g) {
        if (!(group_mask >> g & 1)) continue;
        for (index_type e = mesh->bound_elem_offset[g]; e < mesh->bound_elem_offset[g + 1]; ++e, ++id) {
            dfl_wall_tri* r = &tri[id];
            const index_type* tv = ien + 4 * (size_t)f2e[e];
            const index_type opp = tv[forn[e]];
            for (int k = 0, j = 0; k < 4; ++k) {
                if (k == forn[e]) continue;
                r->node[j] = tv[k];
                for (int d = 0; d < 3; ++d) r->v[3 * j + d] = xg[3 * (size_t)tv[k] + d];
                ++j;
            }
            f64 ab[3], ac[3], ao[3];
            for (int d = 0; d < 3; ++d) {
                ab[d] = r->v[3 + d] - r->v[d];
                ac[d] = r->v[6 + d] - r->v[d];
                ao[d] = xg[3 * (size_t)opp + d] - r->v[d];
            }
            f64 n[3] = {ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]};
            const f64 len = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
            const f64 sgn = (n[0] * ao[0] + n[1] * ao[1] + n[2] * ao[2]) < 0.0 ? -1.0 : 1.0; /* inward: towards opp */
            for (int d = 0; d < 3; ++d) r->n[d] = len > 0.0 ? sgn * n[d] / len : 0.0;
            r->off = r->n[0] * r->v[0] + r->n[1] * r->v[1] + r->n[2] * r->v[2];
            r->id = id;
            for (int k = 0; k < 3; ++k) {
                const f64* p = r->v + 3 * k;
                const f64* q = r->v + 3 * ((k + 1) % 3);
                edges[3 * (size_t)id + k] = sqrt((p[0] - q[0]) * (p[0] - q[0]) + (p[1] - q[1]) * (p[1] - q[1]) + (p[2] - q[2]) * (p[2] - q[2]));
            }
        }
    }
    free(forn);
    free(f2e);
    free(ien);
    free(xg);
    if (edges_out) *edges_out = edges;
    else free(edges);
    *nf_out = nf;
    return tri;
}

void ParticleContextSetWallMesh(ParticleContext* ctx, Mesh3D* mesh, index_type group_mask) {
    ParticleExt* x = (ParticleExt*)ctx->ext;
    DflWallsFree(x->walls);
    x->walls = NULL;
    x->sort_valid = FALSE;        /* the last cell sort was on the other grid */
    DflFrictionClearHistory(ctx); /* the keys of the wall contacts change meaning */
    if (!mesh) return;
    const index_type N = Mesh3DNumNode(mesh), T = Mesh3DNumTet(mesh);
    if (N <= 0 || T <= 0) {
        fprintf(stderr, "ParticleContextSetWallMesh: the mesh has no tets; the walls stay the unit box\n");
        return;
    }
    WallState* w = (WallState*)CdamMallocHost(SIZE_OF(WallState));
    memset(w, 0, sizeof *w);
    f64* edges = NULL;
    index_type nf = 0;
    w->h_tri = DflMeshBoundaryTris(mesh, group_mask, &nf, w->lo, w->hi, &edges);
    w->nf = nf;
    w->scale = sqrt((w->hi[0] - w->lo[0]) * (w->hi[0] - w->lo[0]) + (w->hi[1] - w->lo[1]) * (w->hi[1] - w->lo[1]) +
                    (w->hi[2] - w->lo[2]) * (w->hi[2] - w->lo[2]));
    if (nf > 0) {
        qsort(edges, 3 * (size_t)nf, sizeof(f64), cmp_f64);
        w->edge = edges[3 * (size_t)nf / 2];
    } else {
        w->edge = w->scale;
    }
    free(edges);
    w->tri = (dfl_wall_tri*)CdamMallocDevice((ptrdiff_t)(nf > 0 ? nf : 1) * SIZE_OF(dfl_wall_tri));
    HIPGUARD(hipMemcpy(w->tri, w->h_tri, (size_t)(nf > 0 ? nf : 1) * sizeof(dfl_wall_tri), H2D));
    index_type* h_plane = (index_type*)malloc((size_t)(nf > 0 ? nf : 1) * sizeof(index_type));
    plane_ids(w->h_tri, nf, 1e-12 * w->scale, h_plane);
    w->plane = (index_type*)CdamMallocDevice((ptrdiff_t)(nf > 0 ? nf : 1) * SIZE_OF(index_type));
    HIPGUARD(hipMemcpy(w->plane, h_plane, (size_t)(nf > 0 ? nf : 1) * sizeof(index_type), H2D));
    free(h_plane);
    w->dropped = (index_type*)CdamMallocDevice(SIZE_OF(index_type));
    HIPGUARD(hipMemset(w->dropped, 0, sizeof(index_type)));
    build_grids(w, ParticleContextMaxRadius(ctx), ctx->num_particle);
    x->walls = w;
}

index_type ParticleContextWallDroppedCount(const ParticleContext* ctx) {
    const WallState* w = ((const ParticleExt*)ctx->ext)->walls;
    if (!w) return 0;
    index_type n = 0;
    hipStream_t s = DflStream();
    HIPGUARD(hipMemcpyAsync(&n, w->dropped, sizeof n, D2H, s));
    HIPGUARD(hipStreamSynchronize(s));
    return n;
}

void DflWallsBuildCells(ParticleContext* ctx) {
    ParticleExt* x = (ParticleExt*)ctx->ext;
    WallState* w = x->walls;
    const index_type P = ctx->num_particle;
    const f64 R = ParticleContextMaxRadius(ctx); /* Rmax of a polydisperse context */
    if (R != w->R) build_grids(w, R, P);
    else if (P != w->P) build_particle_grid(w, R, P); /* ParticleContextAdd / Remove: the walls stay */
    const index_type ncell3 = w->pgrid.n[0] * w->pgrid.n[1] * w->pgrid.n[2];
    DflDemReserve(x, P, ncell3 + 1); /* + the bin of the particles outside the grid */
    dfl_walls_build_cells(P, ArrayData(ParticleCTXDeviceCoord(ctx)), ArrayData(ParticleCTXDeviceVel(ctx)), x->omega, x->radius,
                          w->pgrid, x->cell_of, x->rank, x->count, x->chunk_sum, x->cell_start, x->slot, x->order, x->sorted,
                          x->sorted_w, x->sorted_r, DflStream());
    x->order_valid = x->sort_valid = TRUE;
}

const dfl_grid3* DflWallsParticleGrid(const ParticleContext* ctx) { return &((const ParticleExt*)ctx->ext)->walls->pgrid; }

void DflWallsComputeForces(ParticleContext* ctx) {
    ParticleExt* x = (ParticleExt*)ctx->ext;
    WallState* w = x->walls;
    const index_type P = ctx->num_particle;
    const f64 R = ParticleContextMaxRadius(ctx);
    hipStream_t s = DflStream();
    DflRangePush("ParticleContextComputeForces");
    DflWallsBuildCells(ctx);
    f64* acc = ArrayData(ParticleCTXDeviceAcc(ctx));
    int slot = DflProfileBegin(DFL_TAG_SMALL + 1);
    dfl_walls_forces(P, x->sorted, x->sorted_w, R, ParticleMass(ctx), DflSizes(x), x->kn, x->gamma_n, DflFrictionLaw(ctx), w->pgrid,
                     x->order, x->cell_start, w->tri, w->plane, w->wgrid, w->wstart, w->wlist, 1e-12 * w->scale, w->dropped,
                     DflFrictionHistory(x), acc, x->alpha, s);
    DflProfileEnd(slot);
    DflRangePop();
}
