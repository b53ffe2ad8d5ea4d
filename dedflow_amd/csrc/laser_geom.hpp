// The beam-frame geometry of the laser kernels (k_laser.hip, k_laser_surface.hip): projection of a candidate triangle, the
// columns under it, the column-centre ray against it.  The operation order is part of the model (tests/laser_model.py bins
// and hits alike): every function switches fused multiply-add off for its own body.
#pragma once
#include "dfl_common.hpp"

namespace {

__device__ __forceinline__ double dot3(const double* a, double x, double y, double z) {
#pragma clang fp contract(off)
    return (x * a[0] + y * a[1]) + z * a[2];
}

// a candidate face in the beam frame: transverse coordinates and depth of its vertices
struct Proj {
    double u[3], v[3], s[3];
};

__device__ __forceinline__ void project(const dfl_wall_tri* __restrict__ t, const dfl_laser_beam& b, Proj& p) {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double dx = t->v[3 * k] - b.o[0], dy = t->v[3 * k + 1] - b.o[1], dz = t->v[3 * k + 2] - b.o[2];
        p.u[k] = dot3(b.e1, dx, dy, dz);
        p.v[k] = dot3(b.e2, dx, dy, dz);
        p.s[k] = dot3(b.dir, dx, dy, dz);
    }
}

// columns whose centre can lie in the projected bounding box (one column of slack per side; the exact test follows)
__device__ __forceinline__ void column_range(const Proj& p, const dfl_laser_beam& b, int& i0, int& i1, int& j0, int& j1) {
#pragma clang fp contract(off)
    const double half = (double)(b.n / 2), top = (double)(b.n - 1);
    const double ulo = fmin(p.u[0], fmin(p.u[1], p.u[2])), uhi = fmax(p.u[0], fmax(p.u[1], p.u[2]));
    const double vlo = fmin(p.v[0], fmin(p.v[1], p.v[2])), vhi = fmax(p.v[0], fmax(p.v[1], p.v[2]));
    i0 = (int)fmin(fmax(floor(ulo / b.h - 0.5) + half, 0.0), top + 1.0);
    i1 = (int)fmax(fmin(ceil(uhi / b.h - 0.5) + half, top), -1.0);
    j0 = (int)fmin(fmax(floor(vlo / b.h - 0.5) + half, 0.0), top + 1.0);
    j1 = (int)fmax(fmin(ceil(vhi / b.h - 0.5) + half, top), -1.0);
}

__device__ __forceinline__ double column_centre(int i, const dfl_laser_beam& b) {
#pragma clang fp contract(off)
    return ((double)(i - b.n / 2) + 0.5) * b.h;
}

// the centre ray (cu, cv) against the projected triangle, edges included; barycentric weights and depth of the hit point
__device__ __forceinline__ bool tri_hit(const Proj& p, double cu, double cv, double* w, double& s) {
#pragma clang fp contract(off)
    const double a0 = p.u[0] - cu, a1 = p.u[1] - cu, a2 = p.u[2] - cu;
    const double b0 = p.v[0] - cv, b1 = p.v[1] - cv, b2 = p.v[2] - cv;
    const double w0 = a1 * b2 - a2 * b1, w1 = a2 * b0 - a0 * b2, w2 = a0 * b1 - a1 * b0;
    const double sum = (w0 + w1) + w2;
    if (sum == 0.0) return false;
    if (!((w0 >= 0.0 && w1 >= 0.0 && w2 >= 0.0) || (w0 <= 0.0 && w1 <= 0.0 && w2 <= 0.0))) return false;
    w[0] = w0 / sum; w[1] = w1 / sum; w[2] = w2 / sum;
    s = (w[0] * p.s[0] + w[1] * p.s[1]) + w[2] * p.s[2];
    return true;
}

}  // namespace
