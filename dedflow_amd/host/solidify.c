/* Solidification record: per node the time, cooling rate and thermal gradient of its last freezing, peak temperature, time
 * spent liquid and remelts (build-defined, opt-in; model in include/dedflow.h, "solidification record", kernels in
 * dedflow_amd/csrc/k_solidify.hip).  The reference keeps no such record.
 *
 * Per mesh, built by DflMeshSetSolidification: the configuration, the record arrays, the workgroup counts of the event pass
 * with their scan (DflBlockScan over the node workgroups), the event list, the reduction scratch and one pinned host word the
 * list length is copied to.  The gradient pass sums in the order of the mesh's sorted V2E map (DflMeshSortedV2E), which the
 * Set call has the mesh build if nothing did before and which stays the mesh's when this feature is cleared.  The kernels read
 * the node coordinates of the mesh at every call, so nothing here goes stale when the nodes move (DflMeshGeometryChanged).
 * An update is five launches (count, the two of the scan, events, gradient) and one 4-byte copy; nothing is allocated per
 * call and only DflMeshSolidificationEvents and DflMeshSolidificationStats wait for the device.  The state w is never
 * written.  Without a configuration nothing of this exists and no call path touches it. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "dedflow.h"
#include "dedflow_kernels.h"
#include "host_private.h"

#define SO_NSTAT 11

typedef struct SolidifyState {
    DflSolidification cfg;
    dfl_solid_params prm;      /* cfg as the kernels take it */
    index_type N;
    f64 *T_prev, *T_peak, *t_liquid, *t_solid, *cool, *grad3; /* device [N] each, grad3 [3N] */
    index_type* melts;         /* device [N] */
    u8* metal;                 /* device [N]: the metal flag of every node as its last update saw it */
    DflBlockScan scan;         /* the freeze-event counts of the node workgroups; base[nblk] is the list length */
    index_type* melt_count;    /* device [nblk]: the melt-event counts of the last update */
    index_type* list;          /* device [N]: the nodes frozen by the last update, ascending */
    index_type* h_events;      /* pinned host word: the list length of the last update, valid after a synchronisation */
    f64 *work, *out;           /* device reduction scratch and the SO_NSTAT statistics */
    f64 t;                     /* elapsed time */
    int64_t updates;
    b32 primed;
} SolidifyState;

static SolidifyState* st_of(const Mesh3D* mesh) {
    const MeshExt* x = (const MeshExt*)mesh->ext;
    return x ? x->solidify : NULL;
}

void DflSolidificationFree(SolidifyState* st) {
    if (!st) return;
    HIPGUARD(hipStreamSynchronize(DflStream()));
    CdamFreeDevice(st->T_prev, 0);
    CdamFreeDevice(st->T_peak, 0);
    CdamFreeDevice(st->t_liquid, 0);
    CdamFreeDevice(st->t_solid, 0);
    CdamFreeDevice(st->cool, 0);
    CdamFreeDevice(st->grad3, 0);
    CdamFreeDevice(st->melts, 0);
    CdamFreeDevice(st->metal, 0);
    DflBlockScanFree(&st->scan);
    CdamFreeDevice(st->melt_count, 0);
    CdamFreeDevice(st->list, 0);
    if (st->h_events) HIPGUARD(hipHostFree(st->h_events));
    CdamFreeDevice(st->work, 0);
    CdamFreeDevice(st->out, 0);
    CdamFreeHost(st, SIZE_OF(SolidifyState));
}

int DflSolidificationCheck(const DflSolidification* c, char* why, size_t why_len) {
    if (!isfinite(c->T_front)) {
        snprintf(why, why_len, "T_front is not finite (%g)", c->T_front);
        return 1;
    }
    if (!isfinite(c->level)) {
        snprintf(why, why_len, "level is not finite (%g)", c->level);
        return 2;
    }
    if (c->use_phi && c->side != 1 && c->side != -1) {
        snprintf(why, why_len, "side must be +1 or -1 with use_phi, got %d", (int)c->side);
        return 3;
    }
    return 0;
}

/* the record to its initial values, the event list empty, time 0, unprimed; enqueues only */
static void reset(SolidifyState* st) {
    hipStream_t s = DflStream();
    dfl_solid_reset(st->N, st->T_prev, st->T_peak, st->t_liquid, st->melts, st->t_solid, st->cool, st->grad3, st->metal, s);
    const size_t nb = st->scan.nblk > 0 ? (size_t)st->scan.nblk : 1;
    HIPGUARD(hipMemsetAsync(st->scan.count, 0, nb * sizeof(index_type), s));
    HIPGUARD(hipMemsetAsync(st->scan.base, 0, (nb + 1) * sizeof(index_type), s));
    HIPGUARD(hipMemsetAsync(st->melt_count, 0, nb * sizeof(index_type), s));
    HIPGUARD(hipMemcpyAsync(st->h_events, st->scan.base + st->scan.nblk, sizeof(index_type), D2H, s));
    st->t = 0.0;
    st->updates = 0;
    st->primed = FALSE;
}

void DflMeshSetSolidification(Mesh3D* mesh, const DflSolidification* cfg) {
    MeshExt* x = (MeshExt*)mesh->ext;
    if (!cfg) {
        DflSolidificationFree(x->solidify);
        x->solidify = NULL;
        return;
    }
    char why[160];
    if (DflSolidificationCheck(cfg, why, sizeof why)) {
        fprintf(stderr, "DflMeshSetSolidification: %s; unchanged\n", why);
        return;
    }
    SolidifyState* st = x->solidify;
    const index_type N = Mesh3DNumNode(mesh);
    const index_type *vrow, *vcol;
    DflMeshSortedV2E(mesh, &vrow, &vcol); /* built here: no update allocates or waits */
    if (!st) {
        st = (SolidifyState*)CdamMallocHost(SIZE_OF(SolidifyState));
        memset(st, 0, sizeof *st);
        st->N = N;
        const ptrdiff_t n1 = N > 0 ? N : 1, nb = n1 * SIZE_OF(f64);
        st->T_prev = (f64*)CdamMallocDevice(nb);
        st->T_peak = (f64*)CdamMallocDevice(nb);
        st->t_liquid = (f64*)CdamMallocDevice(nb);
        st->t_solid = (f64*)CdamMallocDevice(nb);
        st->cool = (f64*)CdamMallocDevice(nb);
        st->grad3 = (f64*)CdamMallocDevice(3 * nb);
        st->melts = (index_type*)CdamMallocDevice(n1 * SIZE_OF(index_type));
        st->metal = (u8*)CdamMallocDevice(n1);
        DflBlockScanAlloc(&st->scan, N, 0); /* one count per workgroup of the per-node kernels */
        st->melt_count = (index_type*)CdamMallocDevice((ptrdiff_t)(st->scan.nblk > 0 ? st->scan.nblk : 1) * SIZE_OF(index_type));
        st->list = (index_type*)CdamMallocDevice(n1 * SIZE_OF(index_type));
        HIPGUARD(hipHostMalloc((void**)&st->h_events, sizeof(index_type), hipHostMallocDefault));
        *st->h_events = 0;
        st->work = (f64*)CdamMallocDevice((ptrdiff_t)dfl_solid_stats_work_size() * SIZE_OF(f64));
        st->out = (f64*)CdamMallocDevice(SO_NSTAT * SIZE_OF(f64));
        x->solidify = st;
    }
    st->cfg = *cfg;
    const dfl_solid_params prm = {cfg->T_front, cfg->level, (f64)cfg->side, cfg->use_phi ? 1 : 0};
    st->prm = prm;
    reset(st);
    HIPGUARD(hipStreamSynchronize(DflStream()));
}

b32 DflMeshSolidificationEnabled(const Mesh3D* mesh) { return st_of(mesh) != NULL; }

void DflMeshSolidificationReset(Mesh3D* mesh) {
    SolidifyState* st = st_of(mesh);
    if (!st) {
        fprintf(stderr, "DflMeshSolidificationReset: no solidification record is set on this mesh (DflMeshSetSolidification)\n");
        return;
    }
    reset(st);
}

void DflMeshSolidificationUpdate(Mesh3D* mesh, const f64* w, f64 dt) {
    SolidifyState* st = st_of(mesh);
    if (!st) {
        fprintf(stderr, "DflMeshSolidificationUpdate: no solidification record is set on this mesh (DflMeshSetSolidification)\n");
        return;
    }
    if (!isfinite(dt) || !(dt > 0.0)) {
        fprintf(stderr, "DflMeshSolidificationUpdate: dt must be finite and positive, got %g; unchanged\n", dt);
        return;
    }
    hipStream_t s = DflStream();
    DflRangePush("DflMeshSolidificationUpdate");
    st->updates++;
    if (!st->primed) {
        /* (the event list is already empty: Set, Reset) */
        dfl_solid_prime(st->N, w, &st->prm, st->T_prev, st->T_peak, st->metal, s);
        st->primed = TRUE;
    } else {
        const Mesh3DData* dev = Mesh3DDevice(mesh);
        const index_type *vrow, *vcol;
        DflMeshSortedV2E(mesh, &vrow, &vcol);
        dfl_solid_count(st->N, w, &st->prm, dt, st->T_prev, st->scan.count, st->melt_count, s);
        DflBlockScanEnqueue(&st->scan, st->h_events, s);
        dfl_solid_events(st->N, w, &st->prm, st->t, dt, st->scan.base, st->T_prev, st->T_peak, st->t_liquid, st->melts, st->t_solid,
                         st->cool, st->grad3, st->metal, st->list, s);
        dfl_solid_gradient(st->N, st->scan.base + st->scan.nblk, st->list, vrow, vcol, dev->ien, dev->xg, w, &st->prm, st->grad3, s);
        st->t += dt;
    }
    DflRangePop();
}

void DflMeshSolidificationFields(const Mesh3D* mesh, const f64** t_solid, const f64** grad3, const f64** cool, const f64** T_peak,
                                 const f64** t_liquid, const index_type** melts) {
    const SolidifyState* st = st_of(mesh);
    if (t_solid) *t_solid = st ? st->t_solid : NULL;
    if (grad3) *grad3 = st ? st->grad3 : NULL;
    if (cool) *cool = st ? st->cool : NULL;
    if (T_peak) *T_peak = st ? st->T_peak : NULL;
    if (t_liquid) *t_liquid = st ? st->t_liquid : NULL;
    if (melts) *melts = st ? st->melts : NULL;
}

index_type DflMeshSolidificationEvents(const Mesh3D* mesh, const index_type** nodes) {
    const SolidifyState* st = st_of(mesh);
    if (nodes) *nodes = st ? st->list : NULL;
    if (!st) return 0;
    HIPGUARD(hipStreamSynchronize(DflStream()));
    return *st->h_events;
}

/* T_prev and the metal flags, for the tests and the probes */
void DflSolidificationTestFields(const Mesh3D* mesh, const f64** T_prev, const u8** metal) {
    const SolidifyState* st = st_of(mesh);
    if (T_prev) *T_prev = st ? st->T_prev : NULL;
    if (metal) *metal = st ? st->metal : NULL;
}

void DflMeshSolidificationStats(Mesh3D* mesh, DflSolidificationStats* out) {
    SolidifyState* st = st_of(mesh);
    f64 h[SO_NSTAT] = {0.0, 0.0, 0.0, 0.0, HUGE_VAL, -HUGE_VAL, HUGE_VAL, -HUGE_VAL, HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    if (!st) fprintf(stderr, "DflMeshSolidificationStats: no solidification record is set on this mesh (DflMeshSetSolidification)\n");
    if (st && st->N > 0) {
        hipStream_t s = DflStream();
        DflRangePush("DflMeshSolidificationStats");
        dfl_solid_stats(st->N, st->cfg.T_front, st->T_prev, st->T_peak, st->t_solid, st->cool, st->grad3, st->metal, st->scan.nblk,
                        st->scan.base + st->scan.nblk, st->melt_count, st->work, st->out, s);
        HIPGUARD(hipMemcpyAsync(h, st->out, sizeof h, D2H, s));
        HIPGUARD(hipStreamSynchronize(s));
        DflRangePop();
    }
    out->time = st ? st->t : 0.0;
    out->updates = st ? st->updates : 0;
    out->frozen = (int64_t)h[0];
    out->liquid = (int64_t)h[1];
    out->freeze_events_last = (int64_t)h[2];
    out->melt_events_last = (int64_t)h[3];
    out->G_min = h[4];
    out->G_max = h[5];
    out->cool_min = h[6];
    out->cool_max = h[7];
    out->R_min = h[8];
    out->R_max = h[9];
    out->T_peak_max = h[10];
}

b32 DflSolidificationInTimeStep(const Mesh3D* mesh) {
    const SolidifyState* st = st_of(mesh);
    return st && st->cfg.in_time_step;
}

void DflSolidificationTimeStepPrime(Mesh3D* mesh, const f64* wgold) {
    SolidifyState* st = st_of(mesh);
    if (!st || !st->cfg.in_time_step || st->primed) return;
    DflMeshSolidificationUpdate(mesh, wgold, DflMeshTimeStep(mesh));
}

void DflSolidificationTimeStep(Mesh3D* mesh, const f64* wgold) {
    if (DflSolidificationInTimeStep(mesh)) DflMeshSolidificationUpdate(mesh, wgold, DflMeshTimeStep(mesh));
}
