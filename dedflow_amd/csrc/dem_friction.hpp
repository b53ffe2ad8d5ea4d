// Tangential contact law with history (Cundall-Strack), shared by the friction variants of the unit-box sweep
// (k_dem.hip) and the mesh-wall sweep (k_walls.hip).  The model, the contact keys and the capacity rule are stated in
// include/dedflow.h ("contact friction").
//
// One thread owns one particle: it reads only its own row of the previous sweep's history and writes only its own new
// row, in the kernel's fixed contact visit order, so the rows (and the forces) are bitwise reproducible.  The old row is
// streamed from memory for every lookup -- no runtime-indexed private copy, which would live in scratch.  A lookup
// starts at the entry the contact would take in the new row: when the contact order did not change since the last sweep
// (the usual case) the first probe hits.
#pragma once
#include "dfl_common.hpp"

namespace dfl_friction {

// kind in the two high bits (include/dedflow.h, contact keys)
constexpr uint64_t KEY_PARTNER = 0ull << 62;  // | partner particle id
constexpr uint64_t KEY_WALL = 1ull << 62;     // | 2 axis + side (unit box) or plane id (mesh)
constexpr uint64_t KEY_EDGE = 2ull << 62;     // | n0 << 31 | n1, n0 < n1
constexpr uint64_t KEY_VERTEX = 3ull << 62;   // | node id
constexpr uint64_t KEY_SURFACE = KEY_WALL | (1ull << 61);  // the surface phi = level (k_surface_contact.hip)

__device__ __forceinline__ uint64_t edge_key(int n0, int n1) { return KEY_EDGE | ((uint64_t)n0 << 31) | (uint64_t)n1; }

struct Contacts {
    const dfl_contact_hist* old;  // the particle's row of the previous sweep
    dfl_contact_hist* out;        // its row of this sweep
    int nold, nnew, over;
    double f[3], tau[3];
};

__device__ __forceinline__ void begin(Contacts& c, const dfl_contact_history& h, long long i) {
    c.old = h.old_row + i * DFL_DEM_MAX_HISTORY;
    c.out = h.new_row + i * DFL_DEM_MAX_HISTORY;
    c.nold = h.old_count[i];
    c.nnew = 0;
    c.over = 0;
    c.f[0] = c.f[1] = c.f[2] = 0.0;
    c.tau[0] = c.tau[1] = c.tau[2] = 0.0;
}

// one contact: unit normal n towards the particle, normal force fn (unclamped), lever ell; v and w are the particle's
// velocity and angular velocity relative to the partner (pair: v_i - v_j and w_i + w_j; wall at rest: v and w).
// LEVER (a pair of unequal radii): w is the lever velocity ell_a w_a x n + ell_b w_b x n itself, already evaluated in the
// pair's id order (lever_velocity), and ell is particle i's own lever, used for the torque only
template <bool LEVER = false>
__device__ __forceinline__ void contact(Contacts& c, const dfl_friction_law& L, uint64_t key, const double* n, double fn,
                                        double ell, const double* v, const double* w) {
    // contact-point velocity v - ell w x n and its tangential part
    double vr0, vr1, vr2;
    if (LEVER) {
        vr0 = v[0] - w[0]; vr1 = v[1] - w[1]; vr2 = v[2] - w[2];
    } else {
        vr0 = v[0] - ell * (w[1] * n[2] - w[2] * n[1]);
        vr1 = v[1] - ell * (w[2] * n[0] - w[0] * n[2]);
        vr2 = v[2] - ell * (w[0] * n[1] - w[1] * n[0]);
    }
    const double vrn = vr0 * n[0] + vr1 * n[1] + vr2 * n[2];
    const double vt0 = vr0 - vrn * n[0], vt1 = vr1 - vrn * n[1], vt2 = vr2 - vrn * n[2];
    double x0 = 0.0, x1 = 0.0, x2 = 0.0;
    const bool keep = c.nnew < DFL_DEM_MAX_HISTORY;
    if (keep) {
        const int start = c.nnew < c.nold ? c.nnew : 0;
        for (int k = 0; k < c.nold; ++k) {
            int e = start + k;
            if (e >= c.nold) e -= c.nold;
            if (c.old[e].key == key) {
                x0 = c.old[e].xi[0]; x1 = c.old[e].xi[1]; x2 = c.old[e].xi[2];
                break;
            }
        }
        // rotate the spring onto the current tangent plane, keeping its length
        const double xn = x0 * n[0] + x1 * n[1] + x2 * n[2];
        const double p0 = x0 - xn * n[0], p1 = x1 - xn * n[1], p2 = x2 - xn * n[2];
        const double pp = p0 * p0 + p1 * p1 + p2 * p2;
        if (pp > 0.0) {
            const double sc = sqrt(x0 * x0 + x1 * x1 + x2 * x2) / sqrt(pp);
            x0 = p0 * sc; x1 = p1 * sc; x2 = p2 * sc;
        } else {
            x0 = x1 = x2 = 0.0;
        }
    }
    x0 += vt0 * L.dt; x1 += vt1 * L.dt; x2 += vt2 * L.dt;
    double F0 = -L.kt * x0 - L.gamma_t * vt0, F1 = -L.kt * x1 - L.gamma_t * vt1, F2 = -L.kt * x2 - L.gamma_t * vt2;
    const double cap = L.mu * fmax(fn, 0.0);
    const double Fm = sqrt(F0 * F0 + F1 * F1 + F2 * F2);
    if (Fm > cap) {  // sliding: Coulomb cap, spring kept consistent with it
        const double sc = cap / Fm;
        F0 *= sc; F1 *= sc; F2 *= sc;
        x0 = -(F0 + L.gamma_t * vt0) / L.kt;
        x1 = -(F1 + L.gamma_t * vt1) / L.kt;
        x2 = -(F2 + L.gamma_t * vt2) / L.kt;
    }
    if (keep) {
        dfl_contact_hist* o = c.out + c.nnew;
        o->key = key;
        o->xi[0] = x0; o->xi[1] = x1; o->xi[2] = x2;
        ++c.nnew;
    } else {
        ++c.over;
    }
    c.f[0] += fn * n[0] + F0;
    c.f[1] += fn * n[1] + F1;
    c.f[2] += fn * n[2] + F2;
    // torque (-ell n) x F
    const double a0 = -ell * n[0], a1 = -ell * n[1], a2 = -ell * n[2];
    c.tau[0] += a1 * F2 - a2 * F1;
    c.tau[1] += a2 * F0 - a0 * F2;
    c.tau[2] += a0 * F1 - a1 * F0;
}

// lever velocity of a pair of unequal radii: ell_a (w_a x n) + ell_b (w_b x n), a the smaller particle id.  Both particles
// of the pair evaluate the same expression with n (and so every term) negated: the results are exact negations
__device__ __forceinline__ void lever_velocity(double ell_a, const double* wa, double ell_b, const double* wb, const double* n,
                                               double* lw) {
    lw[0] = ell_a * (wa[1] * n[2] - wa[2] * n[1]) + ell_b * (wb[1] * n[2] - wb[2] * n[1]);
    lw[1] = ell_a * (wa[2] * n[0] - wa[0] * n[2]) + ell_b * (wb[2] * n[0] - wb[0] * n[2]);
    lw[2] = ell_a * (wa[0] * n[1] - wa[1] * n[0]) + ell_b * (wb[0] * n[1] - wb[1] * n[0]);
}

// acc, alpha and the live count of particle i; one atomic per particle that overflowed
__device__ __forceinline__ void finish(const Contacts& c, const dfl_contact_history& h, long long i, double mass, double inertia,
                                      T* __restrict__ acc, T* __restrict__ alpha) {
    const double im = 1.0 / mass, ii = 1.0 / inertia;
    acc[3 * i] = c.f[0] * im; acc[3 * i + 1] = c.f[1] * im; acc[3 * i + 2] = c.f[2] * im;
    alpha[3 * i] = c.tau[0] * ii; alpha[3 * i + 1] = c.tau[1] * ii; alpha[3 * i + 2] = c.tau[2] * ii;
    h.new_count[i] = c.nnew;
    if (c.over) atomicAdd(h.overflow, c.over);
}

}  // namespace dfl_friction
