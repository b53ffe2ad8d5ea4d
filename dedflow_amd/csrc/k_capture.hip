// Melt-pool capture for gfx950: the capture decision and the deposits of the captured particles (build-defined: the
// reference's particle hooks are empty; model in include/dedflow.h, "melt-pool capture").
//
// capture_flag_kernel is the drag kernel's gather pattern (k_couple.hip): a particle reads its tet, its four weights, the
// four node ids and per node the 24 B velocity, phi, T and the 24 B coordinates, all at random; it is latency-bound at the
// particle counts of a powder stream, so it runs one thread per particle in id order (what measured best for the drag
// kernel: contiguous per-particle reads and writes), without LDS and without atomics.  The node sums run in
// couple_node_kernel<5> (k_couple.hip) after the sort by tet; the compaction is flow_compact_kernel (k_flow.hip).
#include "tet_levelset.hpp"

namespace {

constexpr int BLK = 256;

// u_f exactly as couple_fluid_kernel computes it: the same expression under the same contraction mode (this helper stands
// above the pragma below on purpose)
__device__ __forceinline__ void fluid_velocity(const T* __restrict__ w, const long long n[4], const double l[4], double uf[3]) {
    uf[0] = uf[1] = uf[2] = 0.0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
#pragma unroll
        for (int d = 0; d < 3; ++d) uf[d] += l[b] * w[3 * n[b] + d];
    }
}

}  // namespace

// the decision's operation order is part of the model: no fused multiply-add from here on
#pragma clang fp contract(off)

namespace {

// POLY: mass and radius of particle i are m[i] and r[i]
template <bool POLY>
__global__ __launch_bounds__(BLK) void capture_flag_kernel(I P, const I* __restrict__ tet, const T* __restrict__ lambda,
                                                          const I* __restrict__ ien, const T* __restrict__ xg,
                                                          const T* __restrict__ w, I N, const T* __restrict__ vel,
                                                          const T* __restrict__ temp, T mass_, T radius_, const T* __restrict__ m,
                                                          const T* __restrict__ r, T rho_f, T cp_p, T level, T side, T reach,
                                                          T T_melt, I* __restrict__ keep, I* __restrict__ rtet,
                                                          T* __restrict__ dep) {
    const long long i = (long long)blockIdx.x * BLK + threadIdx.x;
    if (i >= P) return;
    const int t = tet[i];
    bool captured = false;
    double out[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (t >= 0) {
        long long n[4];
        double l[4], phi[4], tf[4], x[12];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            n[b] = ien[4LL * t + b];
            l[b] = lambda[4 * i + b];
            phi[b] = w[4LL * N + n[b]];
            tf[b] = w[5LL * N + n[b]];
#pragma unroll
            for (int d = 0; d < 3; ++d) x[3 * b + d] = xg[3 * n[b] + d];
        }
        const double phi_p = tet_interp(l, phi), T_f = tet_interp(l, tf);
        TetCross c;
        tet_cross(x, c);
        double g[3], gn, dist[4];  // the decision needs |g| only
        tet_levelset(c, phi, level, g, gn, dist);
        const double mass = POLY ? m[i] : mass_, radius = POLY ? r[i] : radius_;
        const double reach_c = side * (phi_p - level) + (reach * radius) * gn;
        captured = reach_c >= 0.0 && T_f >= T_melt;  // (a NaN compares false: it captures nothing)
        if (captured) {
            double uf[3];
            fluid_velocity(w, n, l, uf);
            out[0] = mass / rho_f;
#pragma unroll
            for (int d = 0; d < 3; ++d) out[1 + d] = mass * (vel[3 * i + d] - uf[d]);
            if (temp) out[4] = (mass * cp_p) * (temp[i] - T_f);
        }
    }
    keep[i] = captured ? 0 : 1;
    rtet[i] = captured ? t : -1;
#pragma unroll
    for (int d = 0; d < 5; ++d) dep[5 * i + d] = out[d];
}

__global__ __launch_bounds__(BLK) void capture_source_kernel(I N, const T* __restrict__ A, T time, T* __restrict__ q_vol,
                                                            T* __restrict__ load, T* __restrict__ q_heat) {
    const long long a = (long long)blockIdx.x * BLK + threadIdx.x;
    if (a >= N) return;
    if (q_vol) q_vol[a] = A[5 * a] / time;
    if (load) {
#pragma unroll
        for (int d = 0; d < 3; ++d) load[3 * a + d] = A[5 * a + 1 + d] / time;
    }
    if (q_heat) q_heat[a] = A[5 * a + 4] / time;
}

}  // namespace

extern "C" {

void dfl_capture_flag(I P, const I* tet, const T* lambda, const I* ien, const T* xg, const T* w, I N, const T* vel, const T* temp,
                      T mass, T radius, const T* mass_i, const T* radius_i, T rho_f, T cp_p, T level, T side, T reach, T T_melt,
                      I* keep, I* rtet, T* dep, void* stream) {
    if (P <= 0) return;
    if (radius_i)
        capture_flag_kernel<true><<<ceil_div(P, BLK), BLK, 0, S(stream)>>>(P, tet, lambda, ien, xg, w, N, vel, temp, 0.0, 0.0, mass_i,
                                                                         radius_i, rho_f, cp_p, level, side, reach, T_melt, keep,
                                                                         rtet, dep);
    else
        capture_flag_kernel<false><<<ceil_div(P, BLK), BLK, 0, S(stream)>>>(P, tet, lambda, ien, xg, w, N, vel, temp, mass, radius,
                                                                          nullptr, nullptr, rho_f, cp_p, level, side, reach, T_melt,
                                                                          keep, rtet, dep);
    DFL_LAUNCH_CHECK();
}

void dfl_capture_source(I N, const T* A, T time, T* q_vol, T* load, T* q_heat, void* stream) {
    if (N <= 0) return;
    capture_source_kernel<<<ceil_div(N, BLK), BLK, 0, S(stream)>>>(N, A, time, q_vol, load, q_heat);
    DFL_LAUNCH_CHECK();
}

}  // extern "C"
