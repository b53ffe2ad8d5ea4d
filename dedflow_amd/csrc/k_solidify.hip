// The solidification record for gfx950: per node the time, cooling rate and recovered thermal gradient of its last
// freezing, the peak temperature, the time spent liquid and the number of remelts (build-defined: the reference keeps no such
// record; model in include/dedflow.h, "solidification record").  Passive: the state w is read and never written.
//
//   solid_events_kernel<false>  one thread per node: decides freeze / melt event from (T_prev, T, phi) and writes nothing but
//                       the two counts of its workgroup (block_count_256).  The host scans the freeze counts with
//                       dfl_scan_counts (k_scan.hip); the melt counts ride along in an array of their own.
//   solid_events_kernel<true>   one thread per node again, the same decision from the same numbers: every elementwise update of
//                       the record, and the freeze-event nodes into the list at blk_base[b] + block_scan_incl_256 - 1, which
//                       is ascending node order.  A melt event clears the node's record, grad3 included.
//   solid_gradient_kernel   the node gather of node_gather.hpp in its row-mapping form over the listed nodes only, four sums
//                       per node (S_0, S_1, S_2, V).  The grid strides over the list and reads its length on the device, so
//                       the host never waits for the count.  A lane gathers its tet's ien line, four T, 4 x 24 B of
//                       coordinates (with use_phi four phi); lanes 0..2 of a group take V from lane 3 by a shuffle inside the
//                       group and write one component each.
//   solid_stats_stage1  two-stage fixed-order reduction over the nodes: block_tree_256, then block_reduce_kernel (block_ops.hpp).
//   solid_reset_kernel / solid_prime_kernel   the initial values; T_prev = T and T_peak of the priming update.
//
// No float atomics, every output written once by the lane that owns it, nothing allocated.  Both passes of the event kernel
// must take the same decision and the numpy model reproduces every elementwise bit: the whole file is compiled without fused
// multiply-add (as the geometry of tet_levelset.hpp is wherever it is included).
//
// HBM view per update: the event passes read 2 x (16 B, with use_phi 24 B) per node and write at most 25 B per node that has a
// finite T (T_prev, T_peak, t_liquid, the metal byte) and 24 B more at an event (t_solid, cool and the list entry or melts; a
// melt also zeroes its 24 B of grad3); the gradient pass reads 4 B per listed node and per (listed node, tet) pair 4 B of
// V2E, 16 B of ien, 32 B of T and 96 B of coordinates (with use_phi 32 B of phi more) gathered through L2, and writes 24 B per
// listed node.
#include "block_ops.hpp"
#include "node_gather.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int SO_BLK = BLOCK_OPS_BLK;   // the one-thread-per-node and reduction kernels
constexpr int SO_NSTAT = 11;            // frozen, liquid, freeze events, melt events, G / cool / R min and max, T_peak_max
constexpr int SO_GRAD_GRID = 1024;      // most workgroups of the gradient pass: 16 listed nodes each per trip over the list

struct SolidNode {   // what one update does to one node
    bool valid;      // T is not a NaN: the node is updated at all
    bool metal, freeze, melt;
    double Tn, add_liquid, theta;
    double Tp;
};

__device__ __forceinline__ SolidNode solid_node(long long a, I N, const T* __restrict__ w, const T* __restrict__ T_prev,
                                                const dfl_solid_params& p, double dt) {
    SolidNode s;
    s.Tn = w[5LL * N + a];
    s.valid = s.Tn == s.Tn;
    s.metal = s.freeze = s.melt = false;
    s.add_liquid = s.theta = 0.0;
    s.Tp = 0.0;
    if (!s.valid) return s;
    s.Tp = T_prev[a];
    s.metal = !p.use_phi || p.side * (w[4LL * N + a] - p.level) > 0.0;
    const bool above_p = s.Tp >= p.T_front, above_n = s.Tn >= p.T_front;
    if (!s.metal) return s;
    if (above_p && above_n) {
        s.add_liquid = dt;
    } else if (above_p) {
        s.freeze = true;
        s.theta = (s.Tp - p.T_front) / (s.Tp - s.Tn);
        s.add_liquid = s.theta * dt;
    } else if (above_n) {
        s.melt = true;
        s.add_liquid = (1.0 - (p.T_front - s.Tp) / (s.Tn - s.Tp)) * dt;
    }
    return s;
}

template <bool EMIT>
__global__ __launch_bounds__(SO_BLK) void solid_events_kernel(I N, const T* __restrict__ w, const dfl_solid_params p, double t,
                                                               double dt, const I* __restrict__ blk_base, I* __restrict__ blk_count,
                                                               I* __restrict__ melt_count, T* __restrict__ T_prev,
                                                               T* __restrict__ T_peak, T* __restrict__ t_liquid,
                                                               I* __restrict__ melts, T* __restrict__ t_solid, T* __restrict__ cool,
                                                               T* __restrict__ grad3, unsigned char* __restrict__ metal,
                                                               I* __restrict__ list) {
    const long long a = (long long)blockIdx.x * SO_BLK + threadIdx.x;
    SolidNode s;
    s.valid = s.freeze = s.melt = false;
    if (a < N) s = solid_node(a, N, w, T_prev, p, dt);
    if (!EMIT) {
        __shared__ int s_cnt[2][4];
        block_count_256(s.freeze ? 1 : 0, s_cnt[0]);
        block_count_256(s.melt ? 1 : 0, s_cnt[1]);
        __syncthreads();
        if (threadIdx.x == 0) {
            blk_count[blockIdx.x] = block_count_read(s_cnt[0]);
            melt_count[blockIdx.x] = block_count_read(s_cnt[1]);
        }
        return;
    }
    __shared__ int s_scan[SO_BLK];
    if (s.valid) {
        T_peak[a] = fmax(T_peak[a], s.Tn);
        metal[a] = s.metal ? 1 : 0;
        if (s.add_liquid != 0.0) t_liquid[a] = t_liquid[a] + s.add_liquid;
        if (s.freeze) {
            const double part = s.theta * dt;
            t_solid[a] = t + part;
            cool[a] = (s.Tp - s.Tn) / dt;
        }
        if (s.melt) {
            melts[a] = melts[a] + 1;
            t_solid[a] = __builtin_nan("");
            cool[a] = 0.0;
#pragma unroll
            for (int d = 0; d < 3; ++d) grad3[3 * a + d] = 0.0;
        }
        T_prev[a] = s.Tn;
    }
    const int incl = block_scan_incl_256(s.freeze ? 1 : 0, s_scan);
    if (!s.freeze) return;  // (after the last barrier)
    const long long id = (long long)blk_base[blockIdx.x] + (incl - 1);
    if (id < N) list[id] = (I)a;  // (always: the list holds N entries)
}

__global__ __launch_bounds__(NG_BLK) void solid_gradient_kernel(const I* __restrict__ count, const I* __restrict__ list, I N,
                                                                 const I* __restrict__ vrow, const I* __restrict__ vcol,
                                                                 const I* __restrict__ ien, const T* __restrict__ xg,
                                                                 const T* __restrict__ w, const dfl_solid_params p,
                                                                 T* __restrict__ grad3) {
    const long long n = min(*count, N);  // the same in every lane of the grid: the trips below are workgroup-uniform
    const long long stride = (long long)gridDim.x * NG_ROWS;
    for (long long k0 = (long long)blockIdx.x * NG_ROWS; k0 < n; k0 += stride) {
        const long long k = k0 + threadIdx.x / NG_LANES;
        const bool live = k < n;
        const I node = live ? list[k] : 0;
        const NodeSum s = node_gather_row<4>(node, live, vrow, vcol, [&](I e, I, double* out) {
            const int4 n4 = reinterpret_cast<const int4*>(ien)[e];
            const long long nd[4] = {n4.x, n4.y, n4.z, n4.w};
            double x[12], Tn[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                Tn[b] = w[5LL * N + nd[b]];
#pragma unroll
                for (int d = 0; d < 3; ++d) x[b * 3 + d] = xg[nd[b] * 3 + d];
            }
            TetCross c;
            tet_cross(x, c);
            const double ad = fabs(c.det);
            if (!(ad > 0.0)) return false;
            if (p.use_phi) {
                const T* phi = w + 4LL * N;
                const double mean = ((phi[nd[0]] + phi[nd[1]]) + (phi[nd[2]] + phi[nd[3]])) * 0.25;
                if (!(p.side * (mean - p.level) > 0.0)) return false;
            }
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const double g1 = c.c23[d] / c.det, g2 = c.c31[d] / c.det, g3 = c.c12[d] / c.det;
                const double g0 = -((g1 + g2) + g3);
                const double ge = ((Tn[0] * g0 + Tn[1] * g1) + Tn[2] * g2) + Tn[3] * g3;
                out[d] = ad * ge;
            }
            out[3] = ad;
            return true;
        });
        const double V = __shfl(s.acc, 3, NG_LANES);  // lane 3 of this lane's own group
        if (s.live && s.g < 3) grad3[3LL * s.row + s.g] = V > 0.0 ? s.acc / V : 0.0;
    }
}

__global__ __launch_bounds__(SO_BLK) void solid_reset_kernel(I N, T* __restrict__ T_prev, T* __restrict__ T_peak,
                                                              T* __restrict__ t_liquid, I* __restrict__ melts,
                                                              T* __restrict__ t_solid, T* __restrict__ cool, T* __restrict__ grad3,
                                                              unsigned char* __restrict__ metal) {
    const long long a = (long long)blockIdx.x * SO_BLK + threadIdx.x;
    if (a >= N) return;
    T_prev[a] = __builtin_nan("");
    T_peak[a] = -HUGE_VAL;
    t_liquid[a] = 0.0;
    melts[a] = 0;
    t_solid[a] = __builtin_nan("");
    cool[a] = 0.0;
#pragma unroll
    for (int d = 0; d < 3; ++d) grad3[3 * a + d] = 0.0;
    metal[a] = 0;
}

__global__ __launch_bounds__(SO_BLK) void solid_prime_kernel(I N, const T* __restrict__ w, const dfl_solid_params p,
                                                              T* __restrict__ T_prev, T* __restrict__ T_peak,
                                                              unsigned char* __restrict__ metal) {
    const long long a = (long long)blockIdx.x * SO_BLK + threadIdx.x;
    if (a >= N) return;
    const double Tn = w[5LL * N + a];
    T_prev[a] = Tn;
    T_peak[a] = fmax(T_peak[a], Tn);
    metal[a] = (!p.use_phi || p.side * (w[4LL * N + a] - p.level) > 0.0) ? 1 : 0;
}

// the statistics: sums (0..3), then (min, max) of G, cool and R, then the maximum of T_peak; a + b in this order, fmax / fmin
// drop a NaN
struct MergeSolid {
    __device__ __forceinline__ static bool is_sum(int j) { return j < 4; }
    __device__ __forceinline__ static bool is_max(int j) { return j == 10 || (j & 1); }
    __device__ __forceinline__ double operator()(int j, double a, double b) const {
        return is_sum(j) ? a + b : is_max(j) ? fmax(a, b) : fmin(a, b);
    }
    __device__ __forceinline__ double identity(int j) const { return is_sum(j) ? 0.0 : is_max(j) ? -HUGE_VAL : HUGE_VAL; }
};

struct SolidStat {  // (a struct, as Stat of k_phase.hip)
    double v[SO_NSTAT];
};
__device__ __forceinline__ SolidStat solid_stat_identity() {
    SolidStat s;
#pragma unroll
    for (int k = 0; k < SO_NSTAT; ++k) s.v[k] = MergeSolid().identity(k);
    return s;
}

__global__ __launch_bounds__(SO_BLK) void solid_stats_stage1(I N, double T_front, const T* __restrict__ T_prev,
                                                              const T* __restrict__ T_peak, const T* __restrict__ t_solid,
                                                              const T* __restrict__ cool, const T* __restrict__ grad3,
                                                              const unsigned char* __restrict__ metal, I nblk,
                                                              const I* __restrict__ freeze_total, const I* __restrict__ melt_count,
                                                              T* __restrict__ part) {
    __shared__ double lds[4][SO_NSTAT];
    const MergeSolid merge;
    SolidStat s = solid_stat_identity();
    const long long stride = (long long)gridDim.x * SO_BLK, first = (long long)blockIdx.x * SO_BLK + threadIdx.x;
    for (long long a = first; a < N; a += stride) {
        SolidStat o = solid_stat_identity();
        const double ts = t_solid[a];
        if (ts == ts) {
            const double g0 = grad3[3 * a], g1 = grad3[3 * a + 1], g2 = grad3[3 * a + 2], c = cool[a];
            const double G = sqrt((g0 * g0 + g1 * g1) + g2 * g2);
            const double R = G > 0.0 ? c / G : 0.0;
            o.v[0] = 1.0;
            o.v[4] = o.v[5] = G;
            o.v[6] = o.v[7] = c;
            o.v[8] = o.v[9] = R;
        }
        if (metal[a]) {
            if (T_prev[a] >= T_front) o.v[1] = 1.0;
            o.v[10] = T_peak[a];
        }
#pragma unroll
        for (int k = 0; k < SO_NSTAT; ++k) s.v[k] = merge(k, s.v[k], o.v[k]);
    }
    for (long long b = first; b < nblk; b += stride) s.v[3] = s.v[3] + (double)melt_count[b];  // integers: exact in any order
    if (first == 0) s.v[2] = s.v[2] + (double)*freeze_total;
    block_tree_256<SO_NSTAT>(s.v, merge, lds);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < SO_NSTAT; ++k) part[(long long)blockIdx.x * SO_NSTAT + k] = s.v[k];
}

}  // namespace

extern "C" {

void dfl_solid_reset(I N, T* T_prev, T* T_peak, T* t_liquid, I* melts, T* t_solid, T* cool, T* grad3, unsigned char* metal,
                     void* stream) {
    if (N <= 0) return;
    solid_reset_kernel<<<ceil_div(N, SO_BLK), SO_BLK, 0, S(stream)>>>(N, T_prev, T_peak, t_liquid, melts, t_solid, cool, grad3, metal);
    DFL_LAUNCH_CHECK();
}

void dfl_solid_prime(I N, const T* w, const dfl_solid_params* prm, T* T_prev, T* T_peak, unsigned char* metal, void* stream) {
    if (N <= 0) return;
    solid_prime_kernel<<<ceil_div(N, SO_BLK), SO_BLK, 0, S(stream)>>>(N, w, *prm, T_prev, T_peak, metal);
    DFL_LAUNCH_CHECK();
}

void dfl_solid_count(I N, const T* w, const dfl_solid_params* prm, T dt, const T* T_prev, I* blk_count, I* melt_count, void* stream) {
    if (N <= 0) return;
    solid_events_kernel<false><<<ceil_div(N, SO_BLK), SO_BLK, 0, S(stream)>>>(
        N, w, *prm, 0.0, dt, nullptr, blk_count, melt_count, const_cast<T*>(T_prev), nullptr, nullptr, nullptr, nullptr, nullptr,
        nullptr, nullptr, nullptr);
    DFL_LAUNCH_CHECK();
}

void dfl_solid_events(I N, const T* w, const dfl_solid_params* prm, T t, T dt, const I* blk_base, T* T_prev, T* T_peak, T* t_liquid,
                      I* melts, T* t_solid, T* cool, T* grad3, unsigned char* metal, I* list, void* stream) {
    if (N <= 0) return;
    solid_events_kernel<true><<<ceil_div(N, SO_BLK), SO_BLK, 0, S(stream)>>>(N, w, *prm, t, dt, blk_base, nullptr, nullptr, T_prev,
                                                                             T_peak, t_liquid, melts, t_solid, cool, grad3, metal,
                                                                             list);
    DFL_LAUNCH_CHECK();
}

void dfl_solid_gradient(I N, const I* count, const I* list, const I* vrow, const I* vcol, const I* ien, const T* xg, const T* w,
                        const dfl_solid_params* prm, T* grad3, void* stream) {
    if (N <= 0) return;
    const int full = ceil_div(N, NG_ROWS);
    solid_gradient_kernel<<<full < SO_GRAD_GRID ? full : SO_GRAD_GRID, NG_BLK, 0, S(stream)>>>(count, list, N, vrow, vcol, ien, xg,
                                                                                               w, *prm, grad3);
    DFL_LAUNCH_CHECK();
}

I dfl_solid_stats_work_size(void) { return NODE_REDUCE_MAX_PART * SO_NSTAT; }

void dfl_solid_stats(I N, T T_front, const T* T_prev, const T* T_peak, const T* t_solid, const T* cool, const T* grad3,
                     const unsigned char* metal, I nblk, const I* freeze_total, const I* melt_count, T* work, T* out11,
                     void* stream) {
    if (N <= 0) return;
    const int g = node_reduce_grid(N);
    solid_stats_stage1<<<g, SO_BLK, 0, S(stream)>>>(N, T_front, T_prev, T_peak, t_solid, cool, grad3, metal, nblk, freeze_total,
                                                    melt_count, work);
    block_reduce<SO_NSTAT>(g, work, out11, MergeSolid(), stream);
    DFL_LAUNCH_CHECK();
}

}  // extern "C"
