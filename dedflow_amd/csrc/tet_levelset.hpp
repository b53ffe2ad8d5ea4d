// The level-set geometry of one linear tet in closed form, shared by the capture decision (k_capture.hip), the solid-surface contact (k_surface_contact.hip), the free-surface
// band (k_surface.hip), the phase-change metal fraction (k_phase.hip) and the thermal material (thermal_coeff.hpp).  The
// operation order is part of the model (two kernels must take the same decision from the same numbers, and the numpy models
// reproduce it): every function switches
// fused multiply-add off for its own body, so the IEEE operations and their association do not depend on where this header
// is included or on the contraction mode of the file around it.
#pragma once
#include "dfl_common.hpp"

namespace {

// I(f) = ((l_0 f_0 + l_1 f_1) + l_2 f_2) + l_3 f_3: a nodal field at a point with barycentric weights l
__device__ __forceinline__ double tet_interp(const double* l, const double* f) {
#pragma clang fp contract(off)
    return ((l[0] * f[0] + l[1] * f[1]) + l[2] * f[2]) + l[3] * f[3];
}

struct TetCross {
    double c23[3], c31[3], c12[3], det;  // grad N_1 = c23 / det, grad N_2 = c31 / det, grad N_3 = c12 / det
};

// edge vectors e_k = x_k - x_0 of the vertices x[a*3+d], c23 = e2 x e3, c31 = e3 x e1, c12 = e1 x e2, det = e1 . c23
__device__ __forceinline__ void tet_cross(const double* x, TetCross& t) {
#pragma clang fp contract(off)
    const double e1[3] = {x[3] - x[0], x[4] - x[1], x[5] - x[2]};
    const double e2[3] = {x[6] - x[0], x[7] - x[1], x[8] - x[2]};
    const double e3[3] = {x[9] - x[0], x[10] - x[1], x[11] - x[2]};
    t.c23[0] = e2[1] * e3[2] - e2[2] * e3[1]; t.c23[1] = e2[2] * e3[0] - e2[0] * e3[2]; t.c23[2] = e2[0] * e3[1] - e2[1] * e3[0];
    t.c31[0] = e3[1] * e1[2] - e3[2] * e1[1]; t.c31[1] = e3[2] * e1[0] - e3[0] * e1[2]; t.c31[2] = e3[0] * e1[1] - e3[1] * e1[0];
    t.c12[0] = e1[1] * e2[2] - e1[2] * e2[1]; t.c12[1] = e1[2] * e2[0] - e1[0] * e2[2]; t.c12[2] = e1[0] * e2[1] - e1[1] * e2[0];
    t.det = (e1[0] * t.c23[0] + e1[1] * t.c23[1]) + e1[2] * t.c23[2];
}

// g = sum_a phi_a grad N_a = ((phi_1 - phi_0) c23 + (phi_2 - phi_0) c31 + (phi_3 - phi_0) c12) / det and gn = |g|; where
// gn > 0 also the signed distances d[a] = (phi_a - level) / gn.  Returns gn > 0 (a NaN anywhere compares false)
__device__ __forceinline__ bool tet_levelset(const TetCross& t, const double* phi, double level, double* g, double& gn, double* d) {
#pragma clang fp contract(off)
    const double d1 = phi[1] - phi[0], d2 = phi[2] - phi[0], d3 = phi[3] - phi[0];
#pragma unroll
    for (int k = 0; k < 3; ++k) g[k] = ((d1 * t.c23[k] + d2 * t.c31[k]) + d3 * t.c12[k]) / t.det;
    gn = sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
    if (!(gn > 0.0)) return false;
#pragma unroll
    for (int a = 0; a < 4; ++a) d[a] = (phi[a] - level) / gn;
    return true;
}

// Hs: the integral of the biweight kernel, the metal fraction of the phase-change and thermal-material sections; a NaN gives 0
__device__ __forceinline__ double smooth_step(double t) {
#pragma clang fp contract(off)
    if (!(t > -1.0)) return 0.0;
    if (t >= 1.0) return 1.0;
    const double t2 = t * t, t3 = t2 * t;
    return 0.5 + 0.9375 * ((t - (2.0 / 3.0) * t3) + 0.2 * (t3 * t2));
}

}  // namespace
