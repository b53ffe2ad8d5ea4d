// Free-surface forces of the melt pool for gfx950: surface tension and Marangoni stress, recoil pressure and the surface
// heat loss of a smeared interface phi = level (build-defined: the reference's free surface has no physics; model in
// include/dedflow.h, "free-surface forces").
//
//   surface_node_kernel   the node gather of node_gather.hpp with five sums per node (f_a[3], heat_a, area_a).  A lane
//                         gathers its tet's ien line, four phi and the 4 x 24 B of coordinates and leaves at the band test;
//                         with the flag pass below it leaves after one byte instead.  A lane that stays gathers the four T
//                         and evaluates the five values of its own node.  With a thin band almost every trip of a wave
//                         skips the hand-over.
//   surface_flag_kernel   one thread per tet: the same gathers and the same band test once per tet instead of four times,
//                         one byte out.  The node pass then reads 1 B per (node, tet) pair from a [T] array that stays in L2
//                         in place of 144 B of gathers.
//
// The band test decides what is evaluated, so both kernels must take the same decision from the same numbers: the whole file
// is compiled without fused multiply-add (as the geometry of tet_levelset.hpp is wherever it is included), which makes
// tet_band the same IEEE operations wherever it is inlined.
//
// HBM view per call: V2E (4 B x (N + 4T)) + 40 B x N written; without flags per (node, tet) pair 16 B of ien, 32 B of phi and
// 96 B of coordinates gathered through L2; with flags those 144 B once per tet, T bytes written and 4T bytes read back.
#include "node_gather.hpp"

#pragma clang fp contract(off)

namespace {

constexpr double kSB = 5.670374419e-8;

struct TetBand {
    TetCross c;
    double g[3], gn;  // sum_a phi_a grad N_a and its norm
    double d[4];      // (phi_a - level) / |g|
};

// the tet's constant gradient and the band test; false: the tet contributes nothing (a NaN anywhere compares false at
// |g| > 0)
__device__ __forceinline__ bool tet_band(const double* x, const double* phi, double level, double eps, TetBand& b) {
    tet_cross(x, b.c);
    if (!tet_levelset(b.c, phi, level, b.g, b.gn, b.d)) return false;
    bool above = true, below = true;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        above = above && b.d[a] >= eps;
        below = below && b.d[a] <= -eps;
    }
    return !(above || below);
}

__device__ __forceinline__ void gather_tet(const int4 n4, const T* __restrict__ xg, const T* __restrict__ w, I N, double* x,
                                           double* phi) {
    const long long n[4] = {n4.x, n4.y, n4.z, n4.w};
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        phi[b] = w[4LL * N + n[b]];
#pragma unroll
        for (int d = 0; d < 3; ++d) x[b * 3 + d] = xg[n[b] * 3 + d];
    }
}

// out = (f_a[0..2], heat_a, area_a) of local node la of a tet inside the band
__device__ __forceinline__ void tet_node_terms(const TetBand& b, const double* Tn, int la, const dfl_surface_params& p, double* out) {
    double gN[3], n[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double c = la == 0 ? -((b.c.c23[k] + b.c.c31[k]) + b.c.c12[k]) : la == 1 ? b.c.c23[k] : la == 2 ? b.c.c31[k] : b.c.c12[k];
        gN[k] = c / b.c.det;
        n[k] = b.g[k] / b.gn;
    }
    const double ndg = (n[0] * gN[0] + n[1] * gN[1]) + n[2] * gN[2];
    const double wdet = GW * fabs(b.c.det);
    const bool vapour = p.recoil_p0 > 0.0 || p.evap_q0 > 0.0;
    double S = 0.0, P = 0.0, H = 0.0, A = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double dq = interp_q(q, b.d), Tq = interp_q(q, Tn);
        const double t = dq / p.eps;
        const double u = 1.0 - t * t;
        const double delta = fabs(t) < 1.0 ? 15.0 / (16.0 * p.eps) * (u * u) : 0.0;
        const double W = wdet * delta;
        const double sigma = fmax(0.0, p.sigma0 + p.dsigma_dT * (Tq - p.T_ref));
        const bool hot = vapour && Tq > 0.0;
        const double E = hot ? exp(p.recoil_a * (1.0 - p.T_boil / Tq)) : 0.0;
        const double pq = p.recoil_p0 > 0.0 ? p.recoil_p0 * E : 0.0;
        const double T2 = Tq * Tq, A2 = p.T_amb * p.T_amb;
        double loss = p.h_conv > 0.0 ? p.h_conv * (Tq - p.T_amb) : 0.0;
        loss += p.emissivity > 0.0 ? p.emissivity * kSB * (T2 * T2 - A2 * A2) : 0.0;
        loss += p.evap_q0 > 0.0 && hot ? p.evap_q0 * E * sqrt(p.T_boil / Tq) : 0.0;
        const double Ws = W * shl(la, q);
        S += W * sigma;
        P += Ws * pq;
        H += Ws * loss;
        A += Ws;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = -S * (gN[k] - n[k] * ndg) + p.side * n[k] * P;
    out[3] = -H;
    out[4] = A;
}

template <bool FLAGS>
__global__ __launch_bounds__(NG_BLK) void surface_node_kernel(I N, const I* __restrict__ vrow, const I* __restrict__ vcol,
                                                               const I* __restrict__ ien, const T* __restrict__ xg,
                                                               const T* __restrict__ w, const dfl_surface_params p,
                                                               const unsigned char* __restrict__ flag, T* __restrict__ load,
                                                               T* __restrict__ q_heat, T* __restrict__ area) {
    const NodeSum s = node_gather_sum<5>(N, vrow, vcol, [&](I e, I row, double* out) {
        if (FLAGS && !flag[e]) return false;
        const int4 n4 = reinterpret_cast<const int4*>(ien)[e];
        double x[12], phi[4];
        gather_tet(n4, xg, w, N, x, phi);
        TetBand b;
        if (!tet_band(x, phi, p.level, p.eps, b)) return false;
        const double Tn[4] = {w[5LL * N + n4.x], w[5LL * N + n4.y], w[5LL * N + n4.z], w[5LL * N + n4.w]};
        const int la = n4.x == row ? 0 : n4.y == row ? 1 : n4.z == row ? 2 : 3;
        tet_node_terms(b, Tn, la, p, out);
        return true;
    });
    if (s.live) {
        if (s.g < 3) {
            if (load) load[(long long)s.row * 3 + s.g] = s.acc;
        } else if (s.g == 3) {
            if (q_heat) q_heat[s.row] = s.acc;
        } else if (s.g == 4) {
            if (area) area[s.row] = s.acc;
        }
    }
}

__global__ __launch_bounds__(NG_BLK) void surface_flag_kernel(I NT, const I* __restrict__ ien, const T* __restrict__ xg,
                                                               const T* __restrict__ w, I N, const dfl_surface_params p,
                                                               unsigned char* __restrict__ flag) {
    const long long e = (long long)blockIdx.x * NG_BLK + threadIdx.x;
    if (e >= NT) return;
    const int4 n4 = reinterpret_cast<const int4*>(ien)[e];
    double x[12], phi[4];
    gather_tet(n4, xg, w, N, x, phi);
    TetBand b;
    flag[e] = tet_band(x, phi, p.level, p.eps, b) ? 1 : 0;
}

}  // namespace

extern "C" {

void dfl_surface_flag_tets(I NT, const I* ien, const T* xg, const T* w, I N, const dfl_surface_params* prm, unsigned char* flag,
                           void* stream) {
    if (NT <= 0) return;
    surface_flag_kernel<<<ceil_div(NT, NG_BLK), NG_BLK, 0, S(stream)>>>(NT, ien, xg, w, N, *prm, flag);
    DFL_LAUNCH_CHECK();
}

void dfl_surface_load(I N, const I* vrow, const I* vcol, const I* ien, const T* xg, const T* w, const dfl_surface_params* prm,
                      const unsigned char* flag, T* load, T* q_heat, T* area, void* stream) {
    if (N <= 0 || (!load && !q_heat && !area)) return;
    if (flag)
        surface_node_kernel<true><<<ceil_div(N, NG_ROWS), NG_BLK, 0, S(stream)>>>(N, vrow, vcol, ien, xg, w, *prm, flag, load,
                                                                                 q_heat, area);
    else
        surface_node_kernel<false><<<ceil_div(N, NG_ROWS), NG_BLK, 0, S(stream)>>>(N, vrow, vcol, ien, xg, w, *prm, flag, load,
                                                                                  q_heat, area);
    DFL_LAUNCH_CHECK();
}

}  // extern "C"
