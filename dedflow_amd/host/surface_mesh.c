/* Surface mesh: the surface phi = level as one indexed triangle mesh, one vertex per cut mesh edge, oriented out of the metal,
 * with nodal fields at the vertices (build-defined, opt-in; model in include/dedflow.h, "surface mesh", kernels in
 * dedflow_amd/csrc/k_surface_mesh.hip).  The reference has nothing of the kind.
 *
 * Per mesh, built by DflMeshSetSurfaceMesh: the configuration, the [T] codes, the workgroup counts with their scan, one device
 * record of the totals with its pinned host copy, and the lists.  An evaluation enqueues the count pass, copies the totals and
 * waits once; the lists grow when a count exceeds their capacity and nothing is allocated otherwise; then emit, sort, weld,
 * orient and sum, and the totals are copied again for the vertex count and the area (read after the next synchronisation).
 * The state w is never written.  Without a configuration nothing of this exists and no call path touches it. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "dedflow.h"
#include "dedflow_kernels.h"
#include "host_private.h"

typedef struct SurfaceMeshState {
    DflSurfaceMesh cfg;
    dfl_surface_mesh_params prm;      /* cfg as the kernels take it */
    index_type N, T, nblk;
    u8* code;                         /* device [T] */
    index_type *count, *start;        /* device [2 nblk], [2 nblk + 1] */
    index_type* chunk_sum;            /* device: that scan's scratch */
    dfl_surface_mesh_totals* tot;     /* device [1] */
    dfl_surface_mesh_totals* h_tot;   /* pinned host [1]: valid after a synchronisation */
    /* the key lists, cap_key rows: one key per cut edge of every emitting tet, which bounds the vertices */
    index_type cap_key;
    uint64_t *key, *key_out;          /* device [cap_key]; key holds the unique list after an evaluation */
    index_type *kcount, *kbase, *kchunk; /* device: the run heads per workgroup, their scan and its scratch */
    f64 *verts, *t;                   /* device [cap_key][3], [cap_key] */
    index_type* edge;                 /* device [cap_key][2] */
    f64* vals;                        /* device [cap_vals] >= cap_key x the fields of any evaluation so far */
    int64_t cap_vals;
    void* temp;                       /* radix sort scratch */
    int64_t temp_bytes;
    /* the triangle lists, cap_tri rows */
    index_type cap_tri;
    index_type *tris, *tri_tet;       /* device [cap_tri][3], [cap_tri] */
    f64* part;                        /* device [ceil(cap_tri / 256)] */
    index_type K;                     /* fields of the last evaluation */
    index_type steps;                 /* DflTimeStep calls since the Set call */
    index_type launches;              /* of the last evaluation */
    index_type grows;                 /* evaluations that allocated */
} SurfaceMeshState;

static SurfaceMeshState* st_of(const Mesh3D* mesh) {
    const MeshExt* x = (const MeshExt*)mesh->ext;
    return x ? x->surface_mesh : NULL;
}

static void free_key_lists(SurfaceMeshState* st) {
    CdamFreeDevice(st->key, 0);
    CdamFreeDevice(st->key_out, 0);
    CdamFreeDevice(st->kcount, 0);
    CdamFreeDevice(st->kbase, 0);
    CdamFreeDevice(st->kchunk, 0);
    CdamFreeDevice(st->verts, 0);
    CdamFreeDevice(st->t, 0);
    CdamFreeDevice(st->edge, 0);
    st->key = st->key_out = NULL;
    st->kcount = st->kbase = st->kchunk = st->edge = NULL;
    st->verts = st->t = NULL;
}

static void alloc_key_lists(SurfaceMeshState* st, index_type cap) {
    st->cap_key = cap > 0 ? cap : 1;
    const ptrdiff_t n = st->cap_key;
    const index_type per = dfl_tets_per_block(), nkb = (st->cap_key + per - 1) / per;
    st->key = (uint64_t*)CdamMallocDevice(n * SIZE_OF(uint64_t));
    st->key_out = (uint64_t*)CdamMallocDevice(n * SIZE_OF(uint64_t));
    st->kcount = (index_type*)CdamMallocDevice((ptrdiff_t)nkb * SIZE_OF(index_type));
    st->kbase = (index_type*)CdamMallocDevice(((ptrdiff_t)nkb + 1) * SIZE_OF(index_type));
    st->kchunk = (index_type*)CdamMallocDevice((ptrdiff_t)dfl_scan_num_chunks(nkb) * SIZE_OF(index_type));
    st->verts = (f64*)CdamMallocDevice(n * 3 * SIZE_OF(f64));
    st->t = (f64*)CdamMallocDevice(n * SIZE_OF(f64));
    st->edge = (index_type*)CdamMallocDevice(n * 2 * SIZE_OF(index_type));
}

static void free_tri_lists(SurfaceMeshState* st) {
    CdamFreeDevice(st->tris, 0);
    CdamFreeDevice(st->tri_tet, 0);
    CdamFreeDevice(st->part, 0);
    st->tris = st->tri_tet = NULL;
    st->part = NULL;
}

static void alloc_tri_lists(SurfaceMeshState* st, index_type cap) {
    st->cap_tri = cap > 0 ? cap : 1;
    const ptrdiff_t n = st->cap_tri;
    const index_type per = dfl_tets_per_block();
    st->tris = (index_type*)CdamMallocDevice(n * 3 * SIZE_OF(index_type));
    st->tri_tet = (index_type*)CdamMallocDevice(n * SIZE_OF(index_type));
    st->part = (f64*)CdamMallocDevice((ptrdiff_t)((st->cap_tri + per - 1) / per) * SIZE_OF(f64));
}

void DflSurfaceMeshFree(SurfaceMeshState* st) {
    if (!st) return;
    HIPGUARD(hipStreamSynchronize(DflStream()));
    CdamFreeDevice(st->code, 0);
    CdamFreeDevice(st->count, 0);
    CdamFreeDevice(st->start, 0);
    CdamFreeDevice(st->chunk_sum, 0);
    CdamFreeDevice(st->tot, 0);
    if (st->h_tot) HIPGUARD(hipHostFree(st->h_tot));
    free_key_lists(st);
    free_tri_lists(st);
    CdamFreeDevice(st->vals, 0);
    CdamFreeDevice(st->temp, 0);
    CdamFreeHost(st, SIZE_OF(SurfaceMeshState));
}

int DflSurfaceMeshCheck(const DflSurfaceMesh* c, char* why, size_t why_len) {
    if (!isfinite(c->level)) {
        snprintf(why, why_len, "level is not finite (%g)", c->level);
        return 1;
    }
    if (c->side != 1 && c->side != -1) {
        snprintf(why, why_len, "side must be +1 or -1, got %d", (int)c->side);
        return 2;
    }
    if (c->every < 0) {
        snprintf(why, why_len, "every must not be negative, got %d", (int)c->every);
        return 3;
    }
    return 0;
}

void DflMeshSetSurfaceMesh(Mesh3D* mesh, const DflSurfaceMesh* cfg) {
    MeshExt* x = (MeshExt*)mesh->ext;
    if (!cfg) {
        DflSurfaceMeshFree(x->surface_mesh);
        x->surface_mesh = NULL;
        return;
    }
    char why[160];
    if (DflSurfaceMeshCheck(cfg, why, sizeof why)) {
        fprintf(stderr, "DflMeshSetSurfaceMesh: %s; unchanged\n", why);
        return;
    }
    HIPGUARD(hipStreamSynchronize(DflStream()));
    SurfaceMeshState* st = x->surface_mesh;
    if (!st) {
        st = (SurfaceMeshState*)CdamMallocHost(SIZE_OF(SurfaceMeshState));
        memset(st, 0, sizeof *st);
        st->N = Mesh3DNumNode(mesh);
        st->T = Mesh3DNumTet(mesh);
        const index_type per = dfl_tets_per_block();
        st->nblk = (st->T + per - 1) / per;
        const ptrdiff_t nt = st->T > 0 ? st->T : 1, nb = st->nblk > 0 ? st->nblk : 1;
        st->code = (u8*)CdamMallocDevice(nt);
        st->count = (index_type*)CdamMallocDevice(2 * nb * SIZE_OF(index_type));
        st->start = (index_type*)CdamMallocDevice((2 * nb + 1) * SIZE_OF(index_type));
        st->chunk_sum = (index_type*)CdamMallocDevice((ptrdiff_t)dfl_scan_num_chunks((index_type)(2 * nb)) * SIZE_OF(index_type));
        st->tot = (dfl_surface_mesh_totals*)CdamMallocDevice(SIZE_OF(dfl_surface_mesh_totals));
        HIPGUARD(hipHostMalloc((void**)&st->h_tot, sizeof(dfl_surface_mesh_totals), hipHostMallocDefault));
        alloc_key_lists(st, 1024);
        alloc_tri_lists(st, 1024);
        st->temp_bytes = dfl_surface_mesh_temp_bytes(st->N, st->cap_key);
        st->temp = CdamMallocDevice((ptrdiff_t)st->temp_bytes);
        x->surface_mesh = st;
    }
    st->cfg = *cfg;
    st->prm.level = cfg->level;
    st->prm.side = (f64)cfg->side;
    st->steps = 0;
    st->launches = 0;
    st->K = 0;
    memset(st->h_tot, 0, sizeof *st->h_tot); /* no evaluation yet: an empty mesh */
}

b32 DflMeshSurfaceMeshEnabled(const Mesh3D* mesh) { return st_of(mesh) != NULL; }

index_type DflMeshSurfaceMesh(Mesh3D* mesh, const f64* w, const f64* const* fields, index_type num_fields) {
    SurfaceMeshState* st = st_of(mesh);
    if (!st) {
        fprintf(stderr, "DflMeshSurfaceMesh: no surface mesh is set on this mesh (DflMeshSetSurfaceMesh)\n");
        return -1;
    }
    if (num_fields < 0 || num_fields > DFL_SURFACE_MESH_MAX_FIELDS || (num_fields > 0 && !fields)) {
        fprintf(stderr, "DflMeshSurfaceMesh: num_fields must be in [0, %d] with that many arrays, got %d; nothing evaluated\n",
                DFL_SURFACE_MESH_MAX_FIELDS, (int)num_fields);
        return -1;
    }
    if (st->T <= 0 || st->N <= 0) return 0;
    hipStream_t s = DflStream();
    const Mesh3DData* dev = Mesh3DDevice(mesh);
    DflRangePush("DflMeshSurfaceMesh");
    int n = dfl_surface_mesh_count(st->N, st->T, dev->ien, dev->xg, w, &st->prm, st->code, st->count, st->start, st->chunk_sum,
                                   st->tot, s);
    HIPGUARD(hipMemcpyAsync(st->h_tot, st->tot, sizeof *st->h_tot, D2H, s));
    HIPGUARD(hipStreamSynchronize(s)); /* the one wait: the triangle and key counts (and the bad and degenerate counts) */
    const index_type nt = st->h_tot->count[0], nkeys = st->h_tot->count[1];
    b32 grew = FALSE;
    if (nkeys > st->cap_key) {
        free_key_lists(st);
        alloc_key_lists(st, DflGrowCap(nkeys));
        grew = TRUE;
    }
    if (nt > st->cap_tri) {
        free_tri_lists(st);
        alloc_tri_lists(st, DflGrowCap(nt));
        grew = TRUE;
    }
    if ((int64_t)st->cap_key * num_fields > st->cap_vals) {
        CdamFreeDevice(st->vals, 0);
        st->cap_vals = (int64_t)st->cap_key * num_fields;
        st->vals = (f64*)CdamMallocDevice((ptrdiff_t)st->cap_vals * SIZE_OF(f64));
        grew = TRUE;
    }
    /* rocprim's scratch is not monotone in the key count across its algorithms: sized for the count at hand */
    const int64_t need = nkeys > 0 ? dfl_surface_mesh_temp_bytes(st->N, nkeys) : 0;
    if (need > st->temp_bytes) {
        CdamFreeDevice(st->temp, 0);
        const int64_t at_cap = dfl_surface_mesh_temp_bytes(st->N, st->cap_key);
        st->temp_bytes = need > at_cap ? need : at_cap;
        st->temp = CdamMallocDevice((ptrdiff_t)st->temp_bytes);
        grew = TRUE;
    }
    if (grew) st->grows++;
    n += dfl_surface_mesh_build(st->N, st->T, dev->ien, dev->xg, w, &st->prm, st->code, st->start, nt, nkeys, st->key, st->key_out,
                                st->cap_key, st->temp, st->temp_bytes, st->kcount, st->kbase, st->kchunk, fields, num_fields,
                                st->verts, st->edge, st->t, st->vals, st->tris, st->tri_tet, st->cap_tri, st->part, st->tot, s);
    /* the vertex count and the area: read after the next synchronisation (Stats, Arrays, Copy) */
    HIPGUARD(hipMemcpyAsync(st->h_tot, st->tot, sizeof *st->h_tot, D2H, s));
    st->K = num_fields;
    st->launches = n;
    DflRangePop();
    return nt;
}

void DflMeshSurfaceMeshStats(Mesh3D* mesh, DflSurfaceMeshStats* out) {
    const SurfaceMeshState* st = st_of(mesh);
    if (!st) {
        fprintf(stderr, "DflMeshSurfaceMeshStats: no surface mesh is set on this mesh (DflMeshSetSurfaceMesh)\n");
        return;
    }
    HIPGUARD(hipStreamSynchronize(DflStream()));
    const dfl_surface_mesh_totals* t = st->h_tot;
    out->triangles = t->count[0];
    out->vertices = t->count[2];
    out->bad_nodes = t->count[3];
    out->bad_tets = t->count[4];
    out->degenerate_tets = t->count[5];
    out->fields = st->K;
    out->area = t->area;
}

index_type DflMeshSurfaceMeshArrays(Mesh3D* mesh, const f64** verts, const index_type** edge, const f64** t, const f64** vals,
                                    const index_type** tris, const index_type** tri_tet, index_type* nv) {
    const SurfaceMeshState* st = st_of(mesh);
    if (st) HIPGUARD(hipStreamSynchronize(DflStream()));
    if (verts) *verts = st ? st->verts : NULL;
    if (edge) *edge = st ? st->edge : NULL;
    if (t) *t = st ? st->t : NULL;
    if (vals) *vals = st && st->K > 0 ? st->vals : NULL;
    if (tris) *tris = st ? st->tris : NULL;
    if (tri_tet) *tri_tet = st ? st->tri_tet : NULL;
    if (nv) *nv = st ? st->h_tot->count[2] : 0;
    return st ? st->h_tot->count[0] : 0;
}

void DflMeshSurfaceMeshCopy(Mesh3D* mesh, f64* verts, f64* vals, index_type* tris) {
    const SurfaceMeshState* st = st_of(mesh);
    if (!st) {
        fprintf(stderr, "DflMeshSurfaceMeshCopy: no surface mesh is set on this mesh (DflMeshSetSurfaceMesh)\n");
        return;
    }
    HIPGUARD(hipStreamSynchronize(DflStream()));
    const size_t nt = (size_t)st->h_tot->count[0], nv = (size_t)st->h_tot->count[2];
    if (verts && nv) HIPGUARD(hipMemcpy(verts, st->verts, nv * 3 * sizeof(f64), D2H));
    if (vals && nv && st->K > 0) HIPGUARD(hipMemcpy(vals, st->vals, nv * (size_t)st->K * sizeof(f64), D2H));
    if (tris && nt) HIPGUARD(hipMemcpy(tris, st->tris, nt * 3 * sizeof(index_type), D2H));
}

index_type DflSurfaceMeshTestLaunches(const Mesh3D* mesh) {
    const SurfaceMeshState* st = st_of(mesh);
    return st ? st->launches : 0;
}

index_type DflSurfaceMeshTestGrows(const Mesh3D* mesh, index_type* cap_key, index_type* cap_tri) {
    const SurfaceMeshState* st = st_of(mesh);
    if (cap_key) *cap_key = st ? st->cap_key : 0;
    if (cap_tri) *cap_tri = st ? st->cap_tri : 0;
    return st ? st->grows : 0;
}

b32 DflSurfaceMeshInTimeStep(const Mesh3D* mesh) {
    const SurfaceMeshState* st = st_of(mesh);
    return st && st->cfg.every > 0;
}

/* DflTimeStep: counts the call; on every every-th since the Set call evaluates at wgold with the field T */
void DflSurfaceMeshTimeStep(Mesh3D* mesh, const f64* wgold) {
    SurfaceMeshState* st = st_of(mesh);
    if (!st || st->cfg.every <= 0) return;
    if (++st->steps % st->cfg.every != 0) return;
    const f64* T = wgold + 5 * (ptrdiff_t)st->N;
    DflMeshSurfaceMesh(mesh, wgold, &T, 1);
}
