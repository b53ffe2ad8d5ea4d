// The two-material coefficients of one tet (include/dedflow.h, "thermal material"): the metal fraction m_q, the liquid
// fraction fl_q and from them the differences dk_q = k_q - kKAPPA and dc_q = c_q - kRHO kCP at the four quadrature points.
// Shared by the row pass (k_thermal.hip) and the T Jacobian (k_scalar.hip), which must freeze the same coefficients: every
// function switches fused multiply-add off for its own body, as tet_levelset.hpp does, so both form them from the same IEEE
// operations whatever the contraction mode of the file around them.
#pragma once
#include "node_gather.hpp"

namespace {

// m[q] = Hs(side d_q / eps) from the tet's cross products and its four phi, by the rules of the phase-change section
// (a tet with !(|g| > 0): one value from the mean); without use_phi 1
__device__ __forceinline__ void thermal_metal_fraction(const TetCross& c, const double* phi, const dfl_thermal_params& p, double* m) {
#pragma clang fp contract(off)
#pragma unroll
    for (int q = 0; q < 4; ++q) m[q] = 1.0;
    if (!p.use_phi) return;
    double g[3], gn, d[4];
    if (tet_levelset(c, phi, p.level, g, gn, d)) {
#pragma unroll
        for (int q = 0; q < 4; ++q) m[q] = smooth_step(p.side * interp_q(q, d) / p.eps);
    } else {
        const double mean = ((phi[0] + phi[1]) + (phi[2] + phi[3])) * 0.25;
        const double mflat = p.side * (mean - p.level) > 0.0 ? 1.0 : 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) m[q] = mflat;
    }
}

// k_q and c_q from m_q and the four nodal T (read only when k_liquid != k_solid; a NaN T_q gives fl_q = 0)
__device__ __forceinline__ void thermal_kc(const double* m, const double* Tn, const dfl_thermal_params& p, double* kq, double* cq) {
#pragma clang fp contract(off)
    const bool melts = p.k_liquid != p.k_solid;
    const double range = p.T_liquidus - p.T_solidus;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        double fl = 0.0;
        if (melts) {
            const double s = fmin(1.0, fmax(0.0, (interp_q(q, Tn) - p.T_solidus) / range));  // a NaN clamps to 0
            fl = (s * s) * (3.0 - 2.0 * s);
        }
        kq[q] = p.k_gas + m[q] * ((p.k_solid + fl * (p.k_liquid - p.k_solid)) - p.k_gas);
        cq[q] = p.c_gas + m[q] * (p.c_metal - p.c_gas);
    }
}

// dk[q], dc[q]; returns whether any of the eight is not exactly 0 (a NaN counts as not 0)
__device__ __forceinline__ bool thermal_differences(const double* kq, const double* cq, double* dk, double* dc) {
    bool any = false;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        dk[q] = kq[q] - kKAPPA;
        dc[q] = cq[q] - kRHO * kCP;
        any = any || dk[q] != 0.0 || dc[q] != 0.0;
    }
    return any;
}

}  // namespace
