// Free-surface forces of the melt pool for gfx950: surface tension and Marangoni stress, recoil pressure and the surface
// heat loss of a smeared interface phi = level (build-defined: the reference's free surface has no physics; model in
// include/dedflow.h, "free-surface forces").
//
//   surface_node_kernel   row gather, the pattern of scalar_jac_row_kernel (k_scalar.hip): a group of 16 lanes owns node a
//                         (16 nodes per 256-thread workgroup).  Lane j of the group takes tet j of a's V2E list (ascending
//                         tet id), gathers the tet's ien line, four phi and the 4 x 24 B of coordinates and leaves at the
//                         band test; with the flag pass below it leaves after one byte instead.  A lane that stays gathers
//                         the four T, evaluates the five values of its own node (f_a[3], heat_a, area_a) and parks them in
//                         LDS; lanes 0-4 of the group each own one of the five sums and add the parked values in list
//                         order.  A wave none of whose lanes stays skips the LDS hand-over (a wave-uniform branch): with a
//                         thin band that is almost every trip.  More than 16 tets per node: more trips.  No atomics, every
//                         output written once (no zero pass), fixed summation order starting from +0.0 (a tet that left adds
//                         nothing, which for a sum that started at +0.0 is the same bits as adding its +0.0): bitwise
//                         reproducible and independent of the assembly schedule.
//   surface_flag_kernel   one thread per tet: the same gathers and the same band test once per tet instead of four times,
//                         one byte out.  The node pass then reads 1 B per (node, tet) pair from a [T] array that stays in L2
//                         in place of 144 B of gathers.
//
// The band test decides what is evaluated, so both kernels must take the same decision from the same numbers: the whole file
// is compiled without fused multiply-add, which makes tet_band the same IEEE operations wherever it is inlined.
//
// HBM view per call: V2E (4 B x (N + 4T)) + 40 B x N written; without flags per (node, tet) pair 16 B of ien, 32 B of phi and
// 96 B of coordinates gathered through L2; with flags those 144 B once per tet, T bytes written and 4T bytes read back.
#include "asm_device.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int SF_BLK = 256;
constexpr int SF_G = 16;                // lanes per node (a Kuhn-cube interior node has 24 tets: two trips)
constexpr int SF_ROWS = SF_BLK / SF_G;  // nodes per workgroup
constexpr double kSB = 5.670374419e-8;

struct TetBand {
    double c23[3], c31[3], c12[3], det;  // grad N_1 = c23 / det, grad N_2 = c31 / det, grad N_3 = c12 / det
    double g[3], gn;                     // sum_a phi_a grad N_a and its norm
    double d[4];                         // (phi_a - level) / |g|
};

// the tet's constant gradient in the closed form of the capture kernel (k_capture.hip) and the band test; false: the tet
// contributes nothing (a NaN anywhere compares false at |g| > 0)
__device__ __forceinline__ bool tet_band(const double* x, const double* phi, double level, double eps, TetBand& b) {
    const double e1[3] = {x[3] - x[0], x[4] - x[1], x[5] - x[2]};
    const double e2[3] = {x[6] - x[0], x[7] - x[1], x[8] - x[2]};
    const double e3[3] = {x[9] - x[0], x[10] - x[1], x[11] - x[2]};
    b.c23[0] = e2[1] * e3[2] - e2[2] * e3[1]; b.c23[1] = e2[2] * e3[0] - e2[0] * e3[2]; b.c23[2] = e2[0] * e3[1] - e2[1] * e3[0];
    b.c31[0] = e3[1] * e1[2] - e3[2] * e1[1]; b.c31[1] = e3[2] * e1[0] - e3[0] * e1[2]; b.c31[2] = e3[0] * e1[1] - e3[1] * e1[0];
    b.c12[0] = e1[1] * e2[2] - e1[2] * e2[1]; b.c12[1] = e1[2] * e2[0] - e1[0] * e2[2]; b.c12[2] = e1[0] * e2[1] - e1[1] * e2[0];
    b.det = (e1[0] * b.c23[0] + e1[1] * b.c23[1]) + e1[2] * b.c23[2];
    const double d1 = phi[1] - phi[0], d2 = phi[2] - phi[0], d3 = phi[3] - phi[0];
#pragma unroll
    for (int k = 0; k < 3; ++k) b.g[k] = ((d1 * b.c23[k] + d2 * b.c31[k]) + d3 * b.c12[k]) / b.det;
    b.gn = sqrt((b.g[0] * b.g[0] + b.g[1] * b.g[1]) + b.g[2] * b.g[2]);
    if (!(b.gn > 0.0)) return false;
    bool above = true, below = true;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        b.d[a] = (phi[a] - level) / b.gn;
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

__device__ __forceinline__ double interp_q(int q, const double* f) {
    return ((shl(0, q) * f[0] + shl(1, q) * f[1]) + shl(2, q) * f[2]) + shl(3, q) * f[3];
}

// out = (f_a[0..2], heat_a, area_a) of local node la of a tet inside the band
__device__ __forceinline__ void tet_node_terms(const TetBand& b, const double* Tn, int la, const dfl_surface_params& p, double* out) {
    double gN[3], n[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double c = la == 0 ? -((b.c23[k] + b.c31[k]) + b.c12[k]) : la == 1 ? b.c23[k] : la == 2 ? b.c31[k] : b.c12[k];
        gN[k] = c / b.det;
        n[k] = b.g[k] / b.gn;
    }
    const double ndg = (n[0] * gN[0] + n[1] * gN[1]) + n[2] * gN[2];
    const double wdet = GW * fabs(b.det);
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

__device__ __forceinline__ int wave_max(int v) {  // the node groups of one wave share trips
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, WAVE));
    return v;
}

template <bool FLAGS>
__global__ __launch_bounds__(SF_BLK) void surface_node_kernel(I N, const I* __restrict__ vrow, const I* __restrict__ vcol,
                                                               const I* __restrict__ ien, const T* __restrict__ xg,
                                                               const T* __restrict__ w, const dfl_surface_params p,
                                                               const unsigned char* __restrict__ flag, T* __restrict__ load,
                                                               T* __restrict__ q_heat, T* __restrict__ area) {
    __shared__ double s_val[5][SF_BLK];
    const int t = threadIdx.x;
    const int g = t & (SF_G - 1);
    const int gbase = t & ~(SF_G - 1);
    const long long row_ll = (long long)blockIdx.x * SF_ROWS + t / SF_G;
    const bool live = row_ll < N;
    const I row = live ? (I)row_ll : 0;
    const I e0 = live ? vrow[row] : 0, ne = live ? vrow[row + 1] - e0 : 0;
    const int ne_w = wave_max(ne);
    double acc = 0.0;  // lane g < 5 of the group owns component g of the node
    for (int jc = 0; jc < ne_w; jc += SF_G) {
        const int j = jc + g;
        bool stays = false;
        double out[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        if (j < ne) {
            const I e = vcol[e0 + j];
            if (!FLAGS || flag[e]) {
                const int4 n4 = reinterpret_cast<const int4*>(ien)[e];
                double x[12], phi[4];
                gather_tet(n4, xg, w, N, x, phi);
                TetBand b;
                if (tet_band(x, phi, p.level, p.eps, b)) {
                    const double Tn[4] = {w[5LL * N + n4.x], w[5LL * N + n4.y], w[5LL * N + n4.z], w[5LL * N + n4.w]};
                    const int la = n4.x == row ? 0 : n4.y == row ? 1 : n4.z == row ? 2 : 3;
                    tet_node_terms(b, Tn, la, p, out);
                    stays = true;
                }
            }
        }
        if (__any(stays)) {  // the same in every lane of the wave: the hand-over below is a wave barrier
#pragma unroll
            for (int c = 0; c < 5; ++c) s_val[c][t] = out[c];
            WAVE_SYNC();
            const int nj = min(SF_G, (int)ne - jc);
            if (g < 5)
                for (int jj = 0; jj < nj; ++jj) acc += s_val[g][gbase + jj];  // V2E order: ascending tet id
            WAVE_SYNC();  // the parked values are consumed before the next trip overwrites them
        }
    }
    if (live) {
        if (g < 3) {
            if (load) load[(long long)row * 3 + g] = acc;
        } else if (g == 3) {
            if (q_heat) q_heat[row] = acc;
        } else if (g == 4) {
            if (area) area[row] = acc;
        }
    }
}

__global__ __launch_bounds__(SF_BLK) void surface_flag_kernel(I NT, const I* __restrict__ ien, const T* __restrict__ xg,
                                                               const T* __restrict__ w, I N, const dfl_surface_params p,
                                                               unsigned char* __restrict__ flag) {
    const long long e = (long long)blockIdx.x * SF_BLK + threadIdx.x;
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
    surface_flag_kernel<<<ceil_div(NT, SF_BLK), SF_BLK, 0, S(stream)>>>(NT, ien, xg, w, N, *prm, flag);
    DFL_LAUNCH_CHECK();
}

void dfl_surface_load(I N, const I* vrow, const I* vcol, const I* ien, const T* xg, const T* w, const dfl_surface_params* prm,
                      const unsigned char* flag, T* load, T* q_heat, T* area, void* stream) {
    if (N <= 0 || (!load && !q_heat && !area)) return;
    if (flag)
        surface_node_kernel<true><<<ceil_div(N, SF_ROWS), SF_BLK, 0, S(stream)>>>(N, vrow, vcol, ien, xg, w, *prm, flag, load,
                                                                                 q_heat, area);
    else
        surface_node_kernel<false><<<ceil_div(N, SF_ROWS), SF_BLK, 0, S(stream)>>>(N, vrow, vcol, ien, xg, w, *prm, flag, load,
                                                                                  q_heat, area);
    DFL_LAUNCH_CHECK();
}

}  // extern "C"
