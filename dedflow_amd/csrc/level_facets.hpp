// The piecewise-linear surface phi = level inside one linear tet, and the distance of a point to one of its triangles, in
// closed form (model in include/dedflow.h, "level-set redistancing"; kernels in k_redistance.hip).  As in tet_levelset.hpp the
// operation order is part of the model (tests/redistance_model.py reproduces it to the last bit): every function switches
// fused multiply-add off for its own body, every dot product is associated (x0 y0 + x1 y1) + x2 y2, and a comparison with
// a NaN never wins.
#pragma once
#include "tet_levelset.hpp"

namespace {

__device__ __forceinline__ double lf_dot(const double* a, const double* b) {
#pragma clang fp contract(off)
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}
__device__ __forceinline__ void lf_sub(const double* a, const double* b, double* c) {
    c[0] = a[0] - b[0]; c[1] = a[1] - b[1]; c[2] = a[2] - b[2];
}
__device__ __forceinline__ void lf_cross(const double* a, const double* b, double* c) {
#pragma clang fp contract(off)
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}
// entry d of vertex i / value of vertex i, by comparison: the local index is data, the arrays stay in registers
__device__ __forceinline__ double lf_pick(const double* x, int i, int d) {
    const double x0 = x[d], x1 = x[3 + d], x2 = x[6 + d], x3 = x[9 + d];  // (loaded first: the selection is on values)
    return i == 0 ? x0 : i == 1 ? x1 : i == 2 ? x2 : x3;
}
__device__ __forceinline__ double lf_pick1(const double* f, int i) {
    const double f0 = f[0], f1 = f[1], f2 = f[2], f3 = f[3];
    return i == 0 ? f0 : i == 1 ? f1 : i == 2 ? f2 : f3;
}

// bit a set: node a is positive, f_a > 0 (a NaN is not)
__device__ __forceinline__ int lf_positive_mask(const double* f) {
    return (f[0] > 0.0 ? 1 : 0) | (f[1] > 0.0 ? 2 : 0) | (f[2] > 0.0 ? 4 : 0) | (f[3] > 0.0 ? 8 : 0);
}
// triangles of the surface in a tet with this mask: 0 (no or four positive nodes), 1 or 2 (two positive nodes: a quad)
__device__ __forceinline__ int lf_facet_count(int mask) {
    const int np = __popc(mask);
    return np == 0 || np == 4 ? 0 : np == 2 ? 2 : 1;
}

// the coordinates of the tet's nodes: x[b * 3 + d] of local node b
__device__ __forceinline__ void lf_gather_tet(const int4 n4, const double* __restrict__ xg, double* x) {
    const long long n[4] = {n4.x, n4.y, n4.z, n4.w};
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int d = 0; d < 3; ++d) x[b * 3 + d] = xg[n[b] * 3 + d];
}
// phi of the tet's nodes and f = phi - level; returns the mask of the positive nodes
__device__ __forceinline__ int lf_levels(const int4 n4, const double* __restrict__ phi_g, double level, double* phi, double* f) {
    phi[0] = phi_g[n4.x]; phi[1] = phi_g[n4.y]; phi[2] = phi_g[n4.z]; phi[3] = phi_g[n4.w];
#pragma unroll
    for (int a = 0; a < 4; ++a) f[a] = phi[a] - level;
    return lf_positive_mask(f);
}

// P_ij = x_i + t (x_j - x_i), t = f_i / (f_i - f_j): the crossing point of edge (i positive, j not)
__device__ __forceinline__ void lf_cross_point(const double* x, const double* f, int i, int j, double* P) {
#pragma clang fp contract(off)
    const double fi = lf_pick1(f, i);
    const double t = fi / (fi - lf_pick1(f, j));
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double xi = lf_pick(x, i, d);
        P[d] = xi + t * (lf_pick(x, j, d) - xi);
    }
}

// the two positive nodes a < b and the two others c < d of a mask with two bits
__device__ __forceinline__ void lf_pairs(int mask, int& a, int& b, int& c, int& d) {
    a = __ffs(mask) - 1;
    b = 31 - __clz(mask);
    const int rest = ~mask & 15;
    c = __ffs(rest) - 1;
    d = 31 - __clz(rest);
}

// the facets of one tet (vertices x[a*3+d], f_a = phi_a - level) into out[k*9 ..], k < the returned count:
//   one positive node i: (P_ij), j over the three others in local order;  three: (P_ij), i over the positives in local order;
//   two, a < b, the others c < d: the quad P_ac, P_ad, P_bd, P_bc as (0, 1, 2) and (0, 2, 3)
__device__ __forceinline__ int lf_tet_facets(const double* x, const double* f, int mask, double* out) {
    const int np = __popc(mask);
    if (np == 0 || np == 4) return 0;
    if (np == 2) {
        int a, b, c, d;
        lf_pairs(mask, a, b, c, d);
        double Q[12];
        lf_cross_point(x, f, a, c, Q);
        lf_cross_point(x, f, a, d, Q + 3);
        lf_cross_point(x, f, b, d, Q + 6);
        lf_cross_point(x, f, b, c, Q + 9);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            out[k] = Q[k]; out[3 + k] = Q[3 + k]; out[6 + k] = Q[6 + k];
            out[9 + k] = Q[k]; out[12 + k] = Q[6 + k]; out[15 + k] = Q[9 + k];
        }
        return 2;
    }
    const int lone = np == 1 ? __ffs(mask) - 1 : __ffs(~mask & 15) - 1;  // the one positive, or the one that is not
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int o = k + (k >= lone ? 1 : 0);  // the three others in local order
        if (np == 1) lf_cross_point(x, f, lone, o, out + 3 * k);
        else lf_cross_point(x, f, o, lone, out + 3 * k);
    }
    return 1;
}

// lf_cross_point that also returns t: the weights of P_ij in the tet are 1 - t at node i, t at node j
__device__ __forceinline__ double lf_cross_point_t(const double* x, const double* f, int i, int j, double* P) {
#pragma clang fp contract(off)
    const double fi = lf_pick1(f, i);
    const double t = fi / (fi - lf_pick1(f, j));
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double xi = lf_pick(x, i, d);
        P[d] = xi + t * (lf_pick(x, j, d) - xi);
    }
    return t;
}

// lf_tet_facets (the same facets, bit for bit) with the edge of every vertex: vertex v of facet k is P_ij with
// i | j << 2 in bits [4 v, 4 v + 4) of ij[k], and t in tt[3 k + v] (the laser's surface deposit, k_laser_surface.hip)
__device__ __forceinline__ int lf_tet_facets_ijt(const double* x, const double* f, int mask, double* out, int* ij, double* tt) {
    const int np = __popc(mask);
    if (np == 0 || np == 4) return 0;
    if (np == 2) {
        int a, b, c, d;
        lf_pairs(mask, a, b, c, d);
        double Q[12], tq[4];
        tq[0] = lf_cross_point_t(x, f, a, c, Q);
        tq[1] = lf_cross_point_t(x, f, a, d, Q + 3);
        tq[2] = lf_cross_point_t(x, f, b, d, Q + 6);
        tq[3] = lf_cross_point_t(x, f, b, c, Q + 9);
        const int e0 = a | c << 2, e1 = a | d << 2, e2 = b | d << 2, e3 = b | c << 2;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            out[k] = Q[k]; out[3 + k] = Q[3 + k]; out[6 + k] = Q[6 + k];
            out[9 + k] = Q[k]; out[12 + k] = Q[6 + k]; out[15 + k] = Q[9 + k];
        }
        ij[0] = e0 | e1 << 4 | e2 << 8;
        ij[1] = e0 | e2 << 4 | e3 << 8;
        tt[0] = tq[0]; tt[1] = tq[1]; tt[2] = tq[2];
        tt[3] = tq[0]; tt[4] = tq[2]; tt[5] = tq[3];
        return 2;
    }
    const int lone = np == 1 ? __ffs(mask) - 1 : __ffs(~mask & 15) - 1;
    int e = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int o = k + (k >= lone ? 1 : 0);
        const int i = np == 1 ? lone : o, j = np == 1 ? o : lone;
        tt[k] = lf_cross_point_t(x, f, i, j, out + 3 * k);
        e |= (i | j << 2) << (4 * k);
    }
    ij[0] = e;
    return 1;
}

// det(q1 - q0, q2 - q0, q3 - q0) in the association of tet_cross
__device__ __forceinline__ double lf_det4(const double* q0, const double* q1, const double* q2, const double* q3) {
    double e1[3], e2[3], e3[3], c[3];
    lf_sub(q1, q0, e1); lf_sub(q2, q0, e2); lf_sub(q3, q0, e3);
    lf_cross(e2, e3, c);
    return lf_dot(e1, c);
}

// volume of {phi > level} inside the tet, det = the tet's own determinant (tet_cross):
//   no positive node 0, four |det| / 6;
//   one (i): the corner tet (x_i, P_ij) -> |det4| / 6;   three (j not positive): |det| / 6 - |det4(x_j, P_ij)| / 6;
//   two (a < b, others c < d): the wedge u = (x_a, P_ac, P_ad), v = (x_b, P_bc, P_bd) as the three tets
//   (u0 u1 u2 v0), (u1 u2 v0 v1), (u2 v0 v1 v2): ((|det4| + |det4|) + |det4|) / 6
__device__ __forceinline__ double lf_positive_volume(const double* x, const double* f, int mask, double det) {
#pragma clang fp contract(off)
    const int np = __popc(mask);
    if (np == 0) return 0.0;
    if (np == 4) return fabs(det) / 6.0;
    if (np == 2) {
        int a, b, c, d;
        lf_pairs(mask, a, b, c, d);
        double u0[3], v0[3], u1[3], u2[3], v1[3], v2[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            u0[k] = lf_pick(x, a, k);
            v0[k] = lf_pick(x, b, k);
        }
        lf_cross_point(x, f, a, c, u1);
        lf_cross_point(x, f, a, d, u2);
        lf_cross_point(x, f, b, c, v1);
        lf_cross_point(x, f, b, d, v2);
        return ((fabs(lf_det4(u0, u1, u2, v0)) + fabs(lf_det4(u1, u2, v0, v1))) + fabs(lf_det4(u2, v0, v1, v2))) / 6.0;
    }
    const int lone = np == 1 ? __ffs(mask) - 1 : __ffs(~mask & 15) - 1;
    double q0[3], P[9];
#pragma unroll
    for (int k = 0; k < 3; ++k) q0[k] = lf_pick(x, lone, k);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int o = k + (k >= lone ? 1 : 0);
        if (np == 1) lf_cross_point(x, f, lone, o, P + 3 * k);
        else lf_cross_point(x, f, o, lone, P + 3 * k);
    }
    const double corner = fabs(lf_det4(q0, P, P + 3, P + 6)) / 6.0;
    return np == 1 ? corner : fabs(det) / 6.0 - corner;
}

// squared distance of p to the segment U V; only where e . e > 0
__device__ __forceinline__ void lf_segment(const double* p, const double* U, const double* V, double& best) {
#pragma clang fp contract(off)
    double e[3], w[3], r[3];
    lf_sub(V, U, e);
    const double ee = lf_dot(e, e);
    if (!(ee > 0.0)) return;
    lf_sub(p, U, w);
    double t = lf_dot(w, e) / ee;
    t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
#pragma unroll
    for (int d = 0; d < 3; ++d) r[d] = p[d] - (U[d] + t * e[d]);
    const double d2 = lf_dot(r, r);
    if (d2 < best) best = d2;
}

// squared distance of p to the triangle F = (A, B, C): the minimum of the three vertex distances, the three segment
// distances and, where the projection falls inside, the plane distance
__device__ __forceinline__ double lf_point_facet_dist2(const double* p, const double* F) {
#pragma clang fp contract(off)
    const double *A = F, *B = F + 3, *C = F + 6;
    double best = HUGE_VAL, r[3];
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        lf_sub(p, F + 3 * v, r);
        const double d2 = lf_dot(r, r);
        if (d2 < best) best = d2;
    }
    lf_segment(p, A, B, best);
    lf_segment(p, B, C, best);
    lf_segment(p, C, A, best);
    double ab[3], ac[3], n[3], w[3], c1[3], c2[3];
    lf_sub(B, A, ab);
    lf_sub(C, A, ac);
    lf_cross(ab, ac, n);
    const double nn = lf_dot(n, n);
    if (nn > 0.0) {
        lf_sub(p, A, w);
        lf_cross(w, ac, c1);
        lf_cross(ab, w, c2);
        const double b1 = lf_dot(c1, n), b2 = lf_dot(c2, n);
        if (b1 >= 0.0 && b2 >= 0.0 && b1 + b2 <= nn) {
            const double s = lf_dot(w, n);
            const double d2 = (s * s) / nn;
            if (d2 < best) best = d2;
        }
    }
    return best;
}

}  // namespace
