/* Level-set volume correction: the global shift of phi that restores the volume of {phi > level} (build-defined, opt-in; model
 * in include/dedflow.h, "level-set volume correction", kernels in dedflow_amd/csrc/k_volume.hip).  The reference lets the
 * volume drift.
 *
 * Per mesh, built by DflMeshSetVolumeCorrection: the configuration, the target, the scan and reduction scratch and the band
 * list (tet ids) of the last call.  A call waits for the device once after the pass over all tets (five sums and the band-tet count)
 * and once per K-section pass (K sums); it grows the band list when the count exceeds the capacity and allocates nothing
 * otherwise.  Without a configuration nothing of this exists and no call path touches it. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "dedflow.h"
#include "dedflow_kernels.h"
#include "host_private.h"

#define VC_K DFL_VOLUME_K
#define VC_PASSES 12

typedef struct VolumeState {
    DflVolumeCorrection cfg;
    index_type N, T;
    index_type pass_limit;            /* DFL_VOLUME_PASSES as the Set call read it */
    f64 target;                       /* NaN: the next call records it */
    DflBlockScan scan;                /* the band-tet counts of the tet passes */
    f64 *part, *out;                  /* device [max(VC_K nblk, dfl_node_reduce_max_part())], [VC_K] */
    index_type* list;                 /* device [cap]: the band list, tet ids */
    index_type cap;
    DflVolumeCorrectionStats last;    /* status -1: no call yet */
    index_type steps;                 /* DflTimeStep calls since the Set call */
} VolumeState;

static VolumeState* st_of(const Mesh3D* mesh) {
    const MeshExt* x = (const MeshExt*)mesh->ext;
    return x ? x->volume : NULL;
}

void DflVolumeCorrectionFree(VolumeState* st) {
    if (!st) return;
    HIPGUARD(hipStreamSynchronize(DflStream()));
    DflBlockScanFree(&st->scan);
    CdamFreeDevice(st->part, 0);
    CdamFreeDevice(st->out, 0);
    CdamFreeDevice(st->list, 0);
    CdamFreeHost(st, SIZE_OF(VolumeState));
}

int DflVolumeCorrectionCheck(const DflVolumeCorrection* c, char* why, size_t why_len) {
    if (!isfinite(c->level)) {
        snprintf(why, why_len, "level is not finite (%g)", c->level);
        return 1;
    }
    if (!isfinite(c->max_shift)) {
        snprintf(why, why_len, "max_shift is not finite (%g)", c->max_shift);
        return 2;
    }
    if (!(c->max_shift > 0.0)) {
        snprintf(why, why_len, "max_shift must be positive, got %g", c->max_shift);
        return 3;
    }
    if (!isfinite(c->tol)) {
        snprintf(why, why_len, "tol is not finite (%g)", c->tol);
        return 4;
    }
    if (c->tol < 0.0) {
        snprintf(why, why_len, "tol must not be negative, got %g", c->tol);
        return 5;
    }
    if (c->side != 1 && c->side != -1) {
        snprintf(why, why_len, "side must be +1 or -1, got %d", (int)c->side);
        return 6;
    }
    if (c->every < 0) {
        snprintf(why, why_len, "every must not be negative, got %d", (int)c->every);
        return 7;
    }
    if (isinf(c->target)) {
        snprintf(why, why_len, "target is infinite (%g)", c->target);
        return 8;
    }
    return 0;
}

static void clear_stats(VolumeState* st) {
    memset(&st->last, 0, sizeof st->last);
    st->last.status = -1;
}

void DflMeshSetVolumeCorrection(Mesh3D* mesh, const DflVolumeCorrection* cfg) {
    MeshExt* x = (MeshExt*)mesh->ext;
    if (!cfg) {
        DflVolumeCorrectionFree(x->volume);
        x->volume = NULL;
        return;
    }
    char why[160];
    if (DflVolumeCorrectionCheck(cfg, why, sizeof why)) {
        fprintf(stderr, "DflMeshSetVolumeCorrection: %s; unchanged\n", why);
        return;
    }
    long limit = VC_PASSES;
    const char* env = getenv("DFL_VOLUME_PASSES");
    if (env && env[0]) {
        char* end = NULL;
        limit = strtol(env, &end, 10);
        if (end == env || *end || limit < 1 || limit > 1000) {
            fprintf(stderr, "DflMeshSetVolumeCorrection: DFL_VOLUME_PASSES must be an integer in [1, 1000], got \"%s\"; unchanged\n", env);
            return;
        }
    }
    VolumeState* st = x->volume;
    if (!st) {
        st = (VolumeState*)CdamMallocHost(SIZE_OF(VolumeState));
        memset(st, 0, sizeof *st);
        st->N = Mesh3DNumNode(mesh);
        st->T = Mesh3DNumTet(mesh);
        DflBlockScanAlloc(&st->scan, st->T, 0);
        const ptrdiff_t nb = st->scan.nblk > 0 ? st->scan.nblk : 1, most = dfl_node_reduce_max_part();
        st->part = (f64*)CdamMallocDevice((VC_K * nb > most ? VC_K * nb : most) * SIZE_OF(f64));
        st->out = (f64*)CdamMallocDevice(VC_K * SIZE_OF(f64));
        st->cap = 1024;
        st->list = (index_type*)CdamMallocDevice((ptrdiff_t)st->cap * SIZE_OF(index_type));
        x->volume = st;
    }
    st->cfg = *cfg;
    st->pass_limit = (index_type)limit;
    st->target = cfg->target;
    st->steps = 0;
    clear_stats(st);
    HIPGUARD(hipStreamSynchronize(DflStream()));
}

b32 DflMeshVolumeCorrectionEnabled(const Mesh3D* mesh) { return st_of(mesh) != NULL; }

b32 DflVolumeCorrectionInTimeStep(const Mesh3D* mesh) {
    const VolumeState* st = st_of(mesh);
    return st && st->cfg.every > 0;
}

typedef struct Point {
    f64 c, V;
} Point;

/* the K candidates of a pass over the bracket [a, b]: the K - 1 section points and the trial, ascending */
static void candidates(Point a, Point b, f64 target, f64* cand) {
    const f64 wdt = (b.c - a.c) / (f64)VC_K;
    f64 trial = a.V > b.V ? a.c + (b.c - a.c) * ((a.V - target) / (a.V - b.V)) : a.c + 0.5 * (b.c - a.c);
    if (!(trial >= a.c)) trial = a.c;
    if (trial > b.c) trial = b.c;
    int n = 0;
    b32 placed = FALSE;
    for (int k = 1; k < VC_K; ++k) {
        const f64 u = a.c + (f64)k * wdt;
        if (!placed && trial <= u) {
            cand[n++] = trial;
            placed = TRUE;
        }
        cand[n++] = u;
    }
    if (!placed) cand[n++] = trial;
}

index_type DflMeshVolumeCorrect(Mesh3D* mesh, f64* w) {
    VolumeState* st = st_of(mesh);
    if (!st) {
        fprintf(stderr, "DflMeshVolumeCorrect: no volume correction is set on this mesh (DflMeshSetVolumeCorrection)\n");
        return -1;
    }
    hipStream_t s = DflStream();
    const f64 level = st->cfg.level, lo = level - st->cfg.max_shift, hi = level + st->cfg.max_shift;
    DflVolumeCorrectionStats* r = &st->last;
    f64 h[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    index_type nb = 0;
    DflRangePush("DflMeshVolumeCorrect");
    if (st->N > 0 && st->T > 0) {
        const Mesh3DData* dev = Mesh3DDevice(mesh);
        dfl_volume_classify(st->T, dev->ien, dev->xg, w, st->N, level, lo, hi, st->scan.count, st->part, st->out, s);
        DflBlockScanEnqueue(&st->scan, &nb, s);
        HIPGUARD(hipMemcpyAsync(h, st->out, sizeof h, D2H, s));
        HIPGUARD(hipStreamSynchronize(s));
    }
    const f64 V_in = h[0], V_mesh = h[4];
    const Point at_level = {level, V_in + h[1]}, at_lo = {lo, V_in + h[2]}, at_hi = {hi, V_in + h[3]};
    if (isnan(st->target)) st->target = at_level.V; /* the first call records it: status 1 below */
    const f64 target = st->target, tolV = st->cfg.tol * V_mesh;
    memset(r, 0, sizeof *r);
    r->band_tets = nb;
    r->target = target;
    r->volume_before = r->volume_after = at_level.V;
    r->volume_mesh = V_mesh;
    if (fabs(at_level.V - target) <= tolV) {
        r->status = 1;
    } else if (!(target <= at_lo.V && target >= at_hi.V)) {
        r->status = 2;
    } else {
        Point a = target > at_level.V ? at_lo : at_level, b = target > at_level.V ? at_level : at_hi;
        Point best = fabs(a.V - target) <= fabs(b.V - target) ? a : b;
        if (nb > st->cap) {
            CdamFreeDevice(st->list, 0);
            st->cap = DflGrowCap(nb);
            st->list = (index_type*)CdamMallocDevice((ptrdiff_t)st->cap * SIZE_OF(index_type));
        }
        const Mesh3DData* dev = Mesh3DDevice(mesh);
        dfl_volume_emit(st->T, dev->ien, w, st->N, lo, hi, st->scan.base, st->list, st->cap, s);
        r->status = 3;
        while (fabs(best.V - target) > tolV && r->passes < st->pass_limit) {
            Point p[VC_K + 2];
            f64 cand[VC_K], V[VC_K];
            candidates(a, b, target, cand);
            dfl_volume_eval(nb, st->list, dev->ien, dev->xg, w, st->N, cand, st->part, st->out, s);
            HIPGUARD(hipMemcpyAsync(V, st->out, sizeof V, D2H, s));
            HIPGUARD(hipStreamSynchronize(s));
            r->passes++;
            p[0] = a;
            p[VC_K + 1] = b;
            for (int k = 0; k < VC_K; ++k) {
                p[k + 1].c = cand[k];
                p[k + 1].V = V_in + V[k];
                if (fabs(p[k + 1].V - target) < fabs(best.V - target)) best = p[k + 1];
            }
            int j = 0;
            while (j < VC_K && !(p[j + 1].V <= target)) ++j; /* the first sub-interval whose right end is at or below the target */
            a = p[j];
            b = p[j + 1];
        }
        if (fabs(best.V - target) <= tolV) r->status = 0;
        r->shift = level - best.c;
        r->volume_after = best.V;
        if (r->shift != 0.0) dfl_volume_shift(st->N, w, r->shift, s);
    }
    DflRangePop();
    return r->status;
}

void DflMeshVolumeCorrectionStats(Mesh3D* mesh, DflVolumeCorrectionStats* out) {
    const VolumeState* st = st_of(mesh);
    memset(out, 0, sizeof *out);
    out->status = -1;
    if (!st) {
        fprintf(stderr, "DflMeshVolumeCorrectionStats: no volume correction is set on this mesh (DflMeshSetVolumeCorrection)\n");
        return;
    }
    *out = st->last;
}

f64 DflMeshVolumeCorrectionTarget(const Mesh3D* mesh) {
    const VolumeState* st = st_of(mesh);
    return st ? st->target : NAN;
}

void DflMeshVolumeCorrectionSetTarget(Mesh3D* mesh, f64 volume) {
    VolumeState* st = st_of(mesh);
    if (!st) {
        fprintf(stderr, "DflMeshVolumeCorrectionSetTarget: no volume correction is set on this mesh (DflMeshSetVolumeCorrection)\n");
        return;
    }
    if (isinf(volume)) {
        fprintf(stderr, "DflMeshVolumeCorrectionSetTarget: target is infinite (%g); unchanged\n", volume);
        return;
    }
    st->target = volume;
}

void DflMeshVolumeCorrectionAddTarget(Mesh3D* mesh, f64 dV) {
    VolumeState* st = st_of(mesh);
    if (!st) {
        fprintf(stderr, "DflMeshVolumeCorrectionAddTarget: no volume correction is set on this mesh (DflMeshSetVolumeCorrection)\n");
        return;
    }
    if (!isfinite(dV)) {
        fprintf(stderr, "DflMeshVolumeCorrectionAddTarget: dV is not finite (%g); unchanged\n", dV);
        return;
    }
    st->target += dV; /* (an unset target stays unset: the recording call sees the state with the deposit in it) */
}

/* DflTimeStep: counts the call; on every every-th since the Set call corrects wgold */
void DflVolumeCorrectionTimeStep(Mesh3D* mesh, f64* wgold) {
    VolumeState* st = st_of(mesh);
    if (!st || st->cfg.every <= 0) return;
    if (++st->steps % st->cfg.every != 0) return;
    DflMeshVolumeCorrect(mesh, wgold);
}

/* DflTimeStep, after the Newton solve of a step that took the capture's volume source q_vol (device [N], a rate over
 * `time`): with track_capture the target grows by side time sum q_vol */
void DflVolumeCorrectionCaptured(Mesh3D* mesh, const f64* q_vol, f64 time) {
    VolumeState* st = st_of(mesh);
    if (!st || !st->cfg.track_capture || st->N <= 0) return;
    hipStream_t s = DflStream();
    f64 sum = 0.0;
    dfl_volume_node_sum(st->N, q_vol, st->part, st->out, s);
    HIPGUARD(hipMemcpyAsync(&sum, st->out, sizeof sum, D2H, s));
    HIPGUARD(hipStreamSynchronize(s));
    st->target += (f64)st->cfg.side * time * sum;
}
