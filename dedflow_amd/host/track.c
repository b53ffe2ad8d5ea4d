/* Track cross-sections: bead height, width, depth and dilution of the frozen track at up to 64 parallel planes (build-defined,
 * opt-in; model in include/dedflow.h, "track cross-sections", kernels in dedflow_amd/csrc/k_track.hip).  The reference has
 * nothing of the kind.
 *
 * Per mesh, built by DflMeshSetTrackSections: the configuration and the frame made of it, the station-major workgroup counts
 * with their scan, the pair list, the reduction records, and pinned host copies of the 65 segment offsets and of the result.
 * An evaluation is count, the two launches of the scan, the offsets, then one wait for the 65 offsets; the list and the records
 * grow when a count exceeds their capacity and nothing is allocated otherwise; then emit, evaluate, reduce and one copy of the
 * result, which DflMeshTrackSectionsResult waits for.  The state w is never written.  Without a configuration nothing of this
 * exists and no call path touches it. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "dedflow.h"
#include "dedflow_kernels.h"
#include "host_private.h"

#define TS_MAXS DFL_TRACK_MAX_STATION
#define TS_NV DFL_TRACK_NSTAT

typedef struct TrackState {
    DflTrackSections cfg;
    dfl_track_params prm;             /* cfg as the kernels take it */
    index_type N, T, nblk;
    index_type ns_alloc;              /* stations count / base / chunk_sum are sized for */
    index_type *count, *base;         /* device [ns nblk], [ns nblk + 1], station-major */
    index_type* chunk_sum;            /* device: the scan's scratch */
    index_type* off;                  /* device [65]: the segment offsets of the last evaluation */
    index_type* h_off;                /* pinned host [65] */
    index_type* list;                 /* device [cap]: the pair list, tet ids, by station then tet */
    index_type cap;
    f64* part;                        /* device [cap_part][TS_NV] */
    index_type cap_part;
    f64* out;                         /* device [TS_MAXS][TS_NV] */
    f64* h_out;                       /* pinned host [TS_MAXS][TS_NV]: valid after a synchronisation */
    index_type steps;                 /* DflTimeStep calls since the Set call */
    int64_t evaluations;
} TrackState;

static TrackState* st_of(const Mesh3D* mesh) {
    const MeshExt* x = (const MeshExt*)mesh->ext;
    return x ? x->track : NULL;
}

static void free_scan(TrackState* st) {
    CdamFreeDevice(st->count, 0);
    CdamFreeDevice(st->base, 0);
    CdamFreeDevice(st->chunk_sum, 0);
    st->count = st->base = st->chunk_sum = NULL;
}

void DflTrackSectionsFree(TrackState* st) {
    if (!st) return;
    HIPGUARD(hipStreamSynchronize(DflStream()));
    free_scan(st);
    CdamFreeDevice(st->off, 0);
    if (st->h_off) HIPGUARD(hipHostFree(st->h_off));
    CdamFreeDevice(st->list, 0);
    CdamFreeDevice(st->part, 0);
    CdamFreeDevice(st->out, 0);
    if (st->h_out) HIPGUARD(hipHostFree(st->h_out));
    CdamFreeHost(st, SIZE_OF(TrackState));
}

static f64 dot3(const f64* a, const f64* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

/* n, u, t of the configuration; 0, or which of the two lengths is not a positive finite number */
static int frame(const DflTrackSections* c, f64* n, f64* u, f64* t) {
    const f64 nn = sqrt(dot3(c->normal, c->normal));
    if (!(nn > 0.0) || !isfinite(nn)) return 1;
    for (int d = 0; d < 3; ++d) n[d] = c->normal[d] / nn;
    const f64 along = dot3(c->up, n);
    for (int d = 0; d < 3; ++d) u[d] = c->up[d] - along * n[d];
    const f64 uu = sqrt(dot3(u, u));
    if (!(uu > 0.0) || !isfinite(uu)) return 2;
    for (int d = 0; d < 3; ++d) u[d] = u[d] / uu;
    t[0] = u[1] * n[2] - u[2] * n[1];
    t[1] = u[2] * n[0] - u[0] * n[2];
    t[2] = u[0] * n[1] - u[1] * n[0];
    return 0;
}

int DflTrackSectionsCheck(const DflTrackSections* c, char* why, size_t why_len) {
    static const char* const names[3] = {"origin", "normal", "up"};
    const f64* const vecs[3] = {c->origin, c->normal, c->up};
    for (int v = 0; v < 3; ++v)
        for (int d = 0; d < 3; ++d)
            if (!isfinite(vecs[v][d])) {
                snprintf(why, why_len, "%s[%d] is not finite (%g)", names[v], d, vecs[v][d]);
                return 1 + v;
            }
    f64 n[3], u[3], t[3];
    const int bad = frame(c, n, u, t);
    if (bad == 1) {
        snprintf(why, why_len, "normal has no length");
        return 4;
    }
    if (bad == 2) {
        snprintf(why, why_len, "up is parallel to normal: no build direction is left");
        return 5;
    }
    if (c->num_station < 1 || c->num_station > TS_MAXS) {
        snprintf(why, why_len, "num_station must be in [1, %d], got %d", TS_MAXS, (int)c->num_station);
        return 6;
    }
    for (index_type k = 0; k < c->num_station; ++k) {
        if (!isfinite(c->station[k])) {
            snprintf(why, why_len, "station[%d] is not finite (%g)", (int)k, c->station[k]);
            return 7;
        }
        if (k > 0 && !(c->station[k] > c->station[k - 1])) {
            snprintf(why, why_len, "station must ascend strictly: station[%d] = %g after %g", (int)k, c->station[k], c->station[k - 1]);
            return 8;
        }
    }
    if (!isfinite(c->level)) {
        snprintf(why, why_len, "level is not finite (%g)", c->level);
        return 9;
    }
    if (c->side != 1 && c->side != -1) {
        snprintf(why, why_len, "side must be +1 or -1, got %d", (int)c->side);
        return 10;
    }
    if (!isfinite(c->T_fuse)) {
        snprintf(why, why_len, "T_fuse is not finite (%g)", c->T_fuse);
        return 11;
    }
    if (c->every < 0) {
        snprintf(why, why_len, "every must not be negative, got %d", (int)c->every);
        return 12;
    }
    return 0;
}

/* the result of "no evaluation yet": no pairs, the empty-set values */
static void clear_result(TrackState* st) {
    for (int k = 0; k <= TS_MAXS; ++k) st->h_off[k] = 0;
    for (int k = 0; k < TS_MAXS; ++k)
        for (int j = 0; j < TS_NV; ++j) st->h_out[k * TS_NV + j] = j < 3 ? 0.0 : (j == 5 || j == 7) ? HUGE_VAL : -HUGE_VAL;
}

void DflMeshSetTrackSections(Mesh3D* mesh, const DflTrackSections* cfg) {
    MeshExt* x = (MeshExt*)mesh->ext;
    if (!cfg) {
        DflTrackSectionsFree(x->track);
        x->track = NULL;
        return;
    }
    char why[160];
    if (DflTrackSectionsCheck(cfg, why, sizeof why)) {
        fprintf(stderr, "DflMeshSetTrackSections: %s; unchanged\n", why);
        return;
    }
    hipStream_t s = DflStream();
    HIPGUARD(hipStreamSynchronize(s));
    TrackState* st = x->track;
    if (!st) {
        st = (TrackState*)CdamMallocHost(SIZE_OF(TrackState));
        memset(st, 0, sizeof *st);
        st->N = Mesh3DNumNode(mesh);
        st->T = Mesh3DNumTet(mesh);
        const index_type per = dfl_tets_per_block();
        st->nblk = (st->T + per - 1) / per;
        st->off = (index_type*)CdamMallocDevice((TS_MAXS + 1) * SIZE_OF(index_type));
        HIPGUARD(hipHostMalloc((void**)&st->h_off, (TS_MAXS + 1) * sizeof(index_type), hipHostMallocDefault));
        st->cap = 1024;
        st->list = (index_type*)CdamMallocDevice((ptrdiff_t)st->cap * SIZE_OF(index_type));
        st->cap_part = TS_MAXS;
        st->part = (f64*)CdamMallocDevice((ptrdiff_t)st->cap_part * TS_NV * SIZE_OF(f64));
        st->out = (f64*)CdamMallocDevice(TS_MAXS * TS_NV * SIZE_OF(f64));
        HIPGUARD(hipHostMalloc((void**)&st->h_out, TS_MAXS * TS_NV * sizeof(f64), hipHostMallocDefault));
        x->track = st;
    }
    const index_type ns = cfg->num_station;
    if (ns > st->ns_alloc) {
        free_scan(st);
        const ptrdiff_t n = (ptrdiff_t)ns * (st->nblk > 0 ? st->nblk : 1);
        st->count = (index_type*)CdamMallocDevice(n * SIZE_OF(index_type));
        st->base = (index_type*)CdamMallocDevice((n + 1) * SIZE_OF(index_type));
        st->chunk_sum = (index_type*)CdamMallocDevice((ptrdiff_t)dfl_scan_num_chunks((index_type)n) * SIZE_OF(index_type));
        HIPGUARD(hipMemsetAsync(st->count, 0, (size_t)n * sizeof(index_type), s)); /* every scan leaves it zero again */
        st->ns_alloc = ns;
    }
    st->cfg = *cfg;
    dfl_track_params* p = &st->prm;
    memset(p, 0, sizeof *p);
    frame(cfg, p->n, p->u, p->t);
    for (int d = 0; d < 3; ++d) p->o[d] = cfg->origin[d];
    p->level = cfg->level;
    p->side = (f64)cfg->side;
    p->T_fuse = cfg->T_fuse;
    p->num_station = ns;
    for (index_type k = 0; k < ns; ++k) p->c[k] = cfg->station[k];
    st->steps = 0;
    st->evaluations = 0;
    clear_result(st);
    HIPGUARD(hipStreamSynchronize(s));
}

b32 DflMeshTrackSectionsEnabled(const Mesh3D* mesh) { return st_of(mesh) != NULL; }

index_type DflMeshTrackSectionsStations(const Mesh3D* mesh) {
    const TrackState* st = st_of(mesh);
    return st ? st->prm.num_station : 0;
}

void DflMeshTrackSections(Mesh3D* mesh, const f64* w, const f64* T_peak) {
    TrackState* st = st_of(mesh);
    if (!st) {
        fprintf(stderr, "DflMeshTrackSections: no track sections are set on this mesh (DflMeshSetTrackSections)\n");
        return;
    }
    if (st->T <= 0 || st->N <= 0) return;
    if (!T_peak) DflMeshSolidificationFields(mesh, NULL, NULL, NULL, &T_peak, NULL, NULL); /* NULL again without a record */
    hipStream_t s = DflStream();
    const Mesh3DData* dev = Mesh3DDevice(mesh);
    const index_type ns = st->prm.num_station, n = ns * st->nblk;
    DflRangePush("DflMeshTrackSections");
    dfl_track_count(st->T, dev->ien, dev->xg, w, st->N, &st->prm, st->nblk, st->count, s);
    dfl_scan_counts(n, st->count, st->chunk_sum, st->base, s);
    dfl_track_offsets(ns, st->nblk, st->base, st->off, s);
    HIPGUARD(hipMemcpyAsync(st->h_off, st->off, (TS_MAXS + 1) * sizeof(index_type), D2H, s));
    HIPGUARD(hipStreamSynchronize(s)); /* the one wait: the pair counts */
    const index_type total = st->h_off[ns];
    index_type longest = 0;
    for (index_type k = 0; k < ns; ++k) {
        const index_type seg = st->h_off[k + 1] - st->h_off[k];
        if (seg > longest) longest = seg;
    }
    const index_type per = dfl_tets_per_block(), max_chunk = (longest + per - 1) / per;
    if (total > st->cap) {
        CdamFreeDevice(st->list, 0);
        st->cap = DflGrowCap(total);
        st->list = (index_type*)CdamMallocDevice((ptrdiff_t)st->cap * SIZE_OF(index_type));
    }
    if ((int64_t)ns * max_chunk > st->cap_part) {
        CdamFreeDevice(st->part, 0);
        st->cap_part = DflGrowCap(ns * max_chunk);
        st->part = (f64*)CdamMallocDevice((ptrdiff_t)st->cap_part * TS_NV * SIZE_OF(f64));
    }
    if (total > 0) dfl_track_emit(st->T, dev->ien, dev->xg, w, st->N, &st->prm, st->nblk, st->base, st->list, st->cap, s);
    dfl_track_eval(max_chunk, st->off, st->list, dev->ien, dev->xg, w, st->N, T_peak, &st->prm, st->part, st->out, s);
    HIPGUARD(hipMemcpyAsync(st->h_out, st->out, (size_t)ns * TS_NV * sizeof(f64), D2H, s));
    st->evaluations++;
    DflRangePop();
}

void DflMeshTrackSectionsResult(Mesh3D* mesh, DflTrackSection* out) {
    const TrackState* st = st_of(mesh);
    if (!st) {
        fprintf(stderr, "DflMeshTrackSectionsResult: no track sections are set on this mesh (DflMeshSetTrackSections)\n");
        return;
    }
    HIPGUARD(hipStreamSynchronize(DflStream()));
    for (index_type k = 0; k < st->prm.num_station; ++k) {
        const f64* h = st->h_out + (size_t)k * TS_NV;
        DflTrackSection* r = out + k;
        r->area_clad = h[0];
        r->area_fused = h[1];
        r->area_scale = h[2];
        /* (+ 0.0: a zero extent is +0.0 whichever of -0.0 and +0.0 the fixed tree met first) */
        r->height = h[3] + 0.0;
        r->depth = h[4] + 0.0;
        r->y_lo_clad = h[5] + 0.0;
        r->y_hi_clad = h[6] + 0.0;
        r->y_lo_fused = h[7] + 0.0;
        r->y_hi_fused = h[8] + 0.0;
        r->pairs = (int64_t)st->h_off[k + 1] - (int64_t)st->h_off[k];
        const f64 both = r->area_clad + r->area_fused;
        r->dilution = both > 0.0 ? r->area_fused / both : 0.0;
    }
}

/* the pair list of the last evaluation on the device and its 65 segment offsets (tests, probes); returns the total */
index_type DflTrackSectionsTestPairs(const Mesh3D* mesh, const index_type** list, index_type* off65) {
    const TrackState* st = st_of(mesh);
    if (list) *list = st ? st->list : NULL;
    if (!st) return 0;
    HIPGUARD(hipStreamSynchronize(DflStream()));
    if (off65) memcpy(off65, st->h_off, (TS_MAXS + 1) * sizeof(index_type));
    return st->h_off[TS_MAXS];
}

/* the capacities of the pair list and of the reduction records (tests: a smaller evaluation reuses both) */
void DflTrackSectionsTestCapacity(const Mesh3D* mesh, index_type* cap_list, index_type* cap_part) {
    const TrackState* st = st_of(mesh);
    *cap_list = st ? st->cap : 0;
    *cap_part = st ? st->cap_part : 0;
}

b32 DflTrackSectionsInTimeStep(const Mesh3D* mesh) {
    const TrackState* st = st_of(mesh);
    return st && st->cfg.every > 0;
}

/* DflTimeStep: counts the call; on every every-th since the Set call evaluates at wgold */
void DflTrackSectionsTimeStep(Mesh3D* mesh, const f64* wgold) {
    TrackState* st = st_of(mesh);
    if (!st || st->cfg.every <= 0) return;
    if (++st->steps % st->cfg.every != 0) return;
    DflMeshTrackSections(mesh, wgold, NULL);
}
