// The ray geometry of the laser's reflections (k_laser_reflect.hip; model in include/dedflow.h, "laser reflections"): the
// absorptivity of a hit, the specular reflection, and a ray against a triangle (Moeller-Trumbore in the header's fixed order).
// As in laser_geom.hpp the operation order is part of the model (tests/laser_reflection_model.py decides alike): every
// function switches fused multiply-add off for its own body, every dot product is (a0 b0 + a1 b1) + a2 b2, the cross
// products are in the order of laser_geom.hpp / level_facets.hpp, and a comparison with a NaN never wins.
#pragma once
#include "dfl_common.hpp"

namespace {

__device__ __forceinline__ double lr_dot(const double* a, const double* b) {
#pragma clang fp contract(off)
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}
__device__ __forceinline__ void lr_cross(const double* a, const double* b, double* c) {
#pragma clang fp contract(off)
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}

// c = |d . g| / sqrt((g . g) (d . d)); model 0: A = eta_s; model 1: the Fresnel approximation with eps
__device__ __forceinline__ double lr_absorptivity(int model, double eta_s, double eps, const double* d, const double* g) {
#pragma clang fp contract(off)
    if (model == 0) return eta_s;
    const double c = fabs(lr_dot(d, g)) / sqrt(lr_dot(g, g) * lr_dot(d, d));
    const double ec = eps * c, e2 = eps * eps, c2 = 2.0 * (c * c), tec = 2.0 * ec;
    const double m = 1.0 - ec, q = 1.0 + ec;
    const double r1 = (1.0 + m * m) / (1.0 + q * q);
    const double r2 = ((e2 - tec) + c2) / ((e2 + tec) + c2);
    return 1.0 - (r1 + r2) / 2.0;
}

// d' = d - (2 (d . g) / (g . g)) g
__device__ __forceinline__ void lr_reflect(const double* d, const double* g, double* r) {
#pragma clang fp contract(off)
    const double f = (2.0 * lr_dot(d, g)) / lr_dot(g, g);
#pragma unroll
    for (int k = 0; k < 3; ++k) r[k] = d[k] - f * g[k];
}

// the ray (X, d) against the triangle F = (A, B, C): a hit iff det != 0, u >= 0, v >= 0, u + v <= 1 and tau > 0
__device__ __forceinline__ bool lr_ray_triangle(const double* X, const double* d, const double* F, double& u, double& v, double& tau) {
#pragma clang fp contract(off)
    double e1[3], e2[3], p[3], s[3], q[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        e1[k] = F[3 + k] - F[k];
        e2[k] = F[6 + k] - F[k];
    }
    lr_cross(d, e2, p);
    const double det = lr_dot(e1, p);
    if (det == 0.0) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] = X[k] - F[k];
    u = lr_dot(s, p) / det;
    lr_cross(s, e1, q);
    v = lr_dot(d, q) / det;
    tau = lr_dot(e2, q) / det;
    return u >= 0.0 && v >= 0.0 && u + v <= 1.0 && tau > 0.0;
}

// ((w0 A + w1 B) + w2 C) of the triangle F
__device__ __forceinline__ void lr_point(const double* F, double w0, double w1, double w2, double* X) {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < 3; ++k) X[k] = (w0 * F[k] + w1 * F[3 + k]) + w2 * F[6 + k];
}

}  // namespace
