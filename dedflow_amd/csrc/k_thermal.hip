// Two-material heat equation for gfx950: the T rows that turn the Galerkin part of the heat equation from the one material
// of the assembly (kKAPPA, kRHO kCP) into conductivity and heat capacity that follow phi and the liquid fraction
// (build-defined: the reference has one material; model in include/dedflow.h, "thermal material").  The matching entries of
// the T Jacobian are added inside scalar_jac_row_kernel<true> (k_scalar.hip) from the same coefficients (thermal_coeff.hpp).
//
//   thermal_rows_kernel<NC>   the node gather of node_gather.hpp.  A lane gathers its tet's ien line, the 4 x 24 B of
//                             coordinates, the four T and (with use_phi) phi, the 4 x 24 B of velocities and the four dT,
//                             forms k_q and c_q at the four quadrature points and evaluates the share of its own node:
//                             NC = 1: r_a alone (the assembly path; a tet whose eight differences dk_q, dc_q are all exactly 0
//                             leaves early and parks +0.0), NC = 3: r_a, Kn_a, Cn_a (the stand-alone call; Kn and Cn are
//                             totals, so no tet leaves).  With `add` the owner lane adds its sum to add[row] (the T rows of F,
//                             sum rounded first) instead of writing r[row]: the hook needs no buffer and no second launch.
//
// The whole file is compiled without fused multiply-add, as k_phase.hip is.
//
// HBM view per call: V2E (4 B x (N + 4T)) + 8 B x N per output; per (node, tet) pair 16 B of ien, 96 B of coordinates, 96 B of
// velocities and 64 B of T and dT (with use_phi 32 B of phi more) gathered through L2.
#include "thermal_coeff.hpp"

#pragma clang fp contract(off)

namespace {

// out[0] = r_a, and with NC = 3 out[1] = Kn_a, out[2] = Cn_a, of local node la
template <int NC>
__device__ __forceinline__ bool thermal_tet_node(const int4 n4, I row, I N, const T* __restrict__ xg, const T* __restrict__ w,
                                                 const T* __restrict__ dw, const dfl_thermal_params& p, double* out) {
    const long long n[4] = {n4.x, n4.y, n4.z, n4.w};
    double x[12], phi[4], Tn[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        phi[b] = p.use_phi ? w[4LL * N + n[b]] : 0.0;
        Tn[b] = w[5LL * N + n[b]];
#pragma unroll
        for (int d = 0; d < 3; ++d) x[b * 3 + d] = xg[n[b] * 3 + d];
    }
    TetCross c;
    tet_cross(x, c);
    double m[4], kq[4], cq[4], dk[4], dc[4];
    thermal_metal_fraction(c, phi, p, m);
    thermal_kc(m, Tn, p, kq, cq);
    const bool any = thermal_differences(kq, cq, dk, dc);
    if (NC == 1 && !any) return false;
    const int la = n4.x == row ? 0 : n4.y == row ? 1 : n4.z == row ? 2 : 3;
    const double wdet = GW * fabs(c.det);
    // gT = sum_b T_b grad N_b, in the closed form of tet_levelset's g; ga = grad N_la
    const double t1 = Tn[1] - Tn[0], t2 = Tn[2] - Tn[0], t3 = Tn[3] - Tn[0];
    double gT[3], ga[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        gT[k] = ((t1 * c.c23[k] + t2 * c.c31[k]) + t3 * c.c12[k]) / c.det;
        const double s = la == 0 ? -((c.c23[k] + c.c31[k]) + c.c12[k]) : la == 1 ? c.c23[k] : la == 2 ? c.c31[k] : c.c12[k];
        ga[k] = s / c.det;
    }
    const double cond = (ga[0] * gT[0] + ga[1] * gT[1]) + ga[2] * gT[2];
    double dT[4], ud[3][4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        dT[b] = dw[5LL * N + n[b]];
#pragma unroll
        for (int d = 0; d < 3; ++d) ud[d][b] = w[n[b] * 3 + d];
    }
    double r = 0.0, K = 0.0, C = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double adv = (interp_q(q, ud[0]) * gT[0] + interp_q(q, ud[1]) * gT[1]) + interp_q(q, ud[2]) * gT[2];
        const double na = shl(la, q);
        if (any) r += wdet * ((dc[q] * na) * (interp_q(q, dT) + adv) + dk[q] * cond);  // (the same r whatever NC)
        if (NC == 3) {
            K += (wdet * na) * kq[q];
            C += (wdet * na) * cq[q];
        }
    }
    out[0] = r;
    if (NC == 3) {
        out[1] = K;
        out[2] = C;
    }
    return true;
}

template <int NC>
__global__ __launch_bounds__(NG_BLK) void thermal_rows_kernel(I N, const I* __restrict__ vrow, const I* __restrict__ vcol,
                                                               const I* __restrict__ ien, const T* __restrict__ xg,
                                                               const T* __restrict__ w, const T* __restrict__ dw,
                                                               const dfl_thermal_params p, T* __restrict__ r, T* __restrict__ Kn,
                                                               T* __restrict__ Cn, T* __restrict__ add) {
    const NodeSum s = node_gather_sum<NC>(N, vrow, vcol, [&](I e, I row, double* out) {
        return thermal_tet_node<NC>(reinterpret_cast<const int4*>(ien)[e], row, N, xg, w, dw, p, out);
    });
    if (!s.live) return;
    if (s.g == 0) {
        if (add) add[s.row] = add[s.row] + s.acc;
        else if (r) r[s.row] = s.acc;
    } else if (NC == 3 && s.g == 1) {
        if (Kn) Kn[s.row] = s.acc;
    } else if (NC == 3 && s.g == 2) {
        if (Cn) Cn[s.row] = s.acc;
    }
}

}  // namespace

extern "C" {

void dfl_thermal_rows(I N, const I* vrow, const I* vcol, const I* ien, const T* xg, const T* w, const T* dw,
                      const dfl_thermal_params* prm, T* r, T* Kn, T* Cn, void* stream) {
    if (N <= 0 || (!r && !Kn && !Cn)) return;
    if (Kn || Cn)
        thermal_rows_kernel<3><<<ceil_div(N, NG_ROWS), NG_BLK, 0, S(stream)>>>(N, vrow, vcol, ien, xg, w, dw, *prm, r, Kn, Cn, nullptr);
    else
        thermal_rows_kernel<1><<<ceil_div(N, NG_ROWS), NG_BLK, 0, S(stream)>>>(N, vrow, vcol, ien, xg, w, dw, *prm, r, nullptr, nullptr,
                                                                              nullptr);
    DFL_LAUNCH_CHECK();
}

void dfl_thermal_add_rows(I N, const I* vrow, const I* vcol, const I* ien, const T* xg, const T* wgalpha, const T* dwgalpha,
                          const dfl_thermal_params* prm, T* FT, void* stream) {
    if (N <= 0 || !FT) return;
    thermal_rows_kernel<1><<<ceil_div(N, NG_ROWS), NG_BLK, 0, S(stream)>>>(N, vrow, vcol, ien, xg, wgalpha, dwgalpha, *prm, nullptr,
                                                                          nullptr, nullptr, FT);
    DFL_LAUNCH_CHECK();
}

}  // extern "C"
