// The parts of the DEM contact sweep that the unit-box kernel (k_dem.hip) and the mesh-wall kernel (k_walls.hip) share:
// the cell list a particle searches, the neighbour-pair loop, and what is done with a contact (the sink).
//
// Every force kernel is: load the particle, pair_contacts(), its own walls, sink.finish().  The two template flags are
//   POLY      per-particle radius sz.sorted_r[slot] and mass sz.mass[id] instead of the scalars R and mass; the search
//             range is r_i + sz.rmax.  With every radius R and every mass m the operations are those of the one-size
//             law: (R + R) == 2R and (R + R)^2 == 4 R R exactly
//   FRICTION  the tangential law with history and the torque (dem_friction.hpp) on top of the normal force
// A contact's arithmetic is written once here and is the same in every kernel: the tests compare the variants bit for bit.
#pragma once
#include <type_traits>
#include "dfl_common.hpp"
#include "dem_friction.hpp"

namespace dfl_dem {

__device__ __forceinline__ int cell_coord(double x, double inv_cell, int ncell) {
    int c = (int)floor(x * inv_cell);
    return c < 0 ? 0 : (c >= ncell ? ncell - 1 : c);
}

__device__ __forceinline__ int grid_coord(double x, double lo, double inv, int n) {
    int c = (int)floor((x - lo) * inv);
    return c < 0 ? 0 : (c >= n ? n - 1 : c);
}

// the cell list of the unit box: ncell^3 cells of edge 1 / inv_cell; a coordinate outside falls into the edge cell, in
// the bin kernel as well
struct BoxGrid {
    double inv_cell;
    int ncell;
    __device__ __forceinline__ int coord(int, double x) const { return cell_coord(x, inv_cell, ncell); }
    __device__ __forceinline__ int n(int) const { return ncell; }
};

// the cell list over a mesh: a search range is clamped to the grid, but the bin kernel sends a centre outside it to an
// extra bin behind every cell, which no range reaches
struct MeshGrid {
    dfl_grid3 g;
    __device__ __forceinline__ int coord(int a, double x) const { return grid_coord(x, g.lo[a], g.inv[a], g.n[a]); }
    __device__ __forceinline__ int n(int a) const { return g.n[a]; }
};

// the particle of a thread: sorted slot s, particle id i, radius r (the scalar R when not POLY), position, velocity and,
// with friction, angular velocity
struct Particle {
    int s;
    long long i;
    double r, p[3], v[3], w[3];
};

template <bool FRICTION>
__device__ __forceinline__ void load_state(Particle& a, const T* __restrict__ sorted, const T* __restrict__ sorted_w) {
    const T* me = sorted + (long long)a.s * 6;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        a.p[d] = me[d];
        a.v[d] = me[3 + d];
        a.w[d] = FRICTION ? sorted_w[3 * (long long)a.s + d] : 0.0;
    }
}

// Frictionless sink: the sum of fn n
template <bool POLY>
struct NormalSink {
    double f[3];

    __device__ __forceinline__ NormalSink(const Particle&, const dfl_friction_law&, const dfl_contact_history&, const T*, const I*)
        : f{0.0, 0.0, 0.0} {}

    __device__ __forceinline__ void add(const double* n, double fn) {
        f[0] += fn * n[0]; f[1] += fn * n[1]; f[2] += fn * n[2];
    }
    __device__ __forceinline__ void pair(const Particle&, int, double, double, const double* n, const double*, double fn) {
        add(n, fn);
    }
    __device__ __forceinline__ void wall(const Particle&, uint64_t, const double* n, double, double fn) { add(n, fn); }

    __device__ __forceinline__ void finish(const Particle& a, double mass, const dfl_sizes& sz, T* __restrict__ acc, T*) {
        const double im = 1.0 / (POLY ? sz.mass[a.i] : mass);
        acc[3 * a.i] = f[0] * im; acc[3 * a.i + 1] = f[1] * im; acc[3 * a.i + 2] = f[2] * im;
    }
};

// Friction sink: every contact goes through dfl_friction::contact, which also sums the normal forces; the particle's new
// history row is written in the visit order
template <bool POLY>
struct FrictionSink {
    dfl_friction::Contacts c;
    const dfl_friction_law& law;
    const dfl_contact_history& hist;
    const T* __restrict__ sorted_w;
    const I* __restrict__ order;

    __device__ __forceinline__ FrictionSink(const Particle& a, const dfl_friction_law& law_, const dfl_contact_history& hist_,
                                            const T* sorted_w_, const I* order_)
        : law(law_), hist(hist_), sorted_w(sorted_w_), order(order_) {
        dfl_friction::begin(c, hist, a.i);
    }

    // the partner in slot t, radius rj (POLY only), centres dist apart, n towards a, dv = v_a - v_t
    __device__ __forceinline__ void pair(const Particle& a, int t, double rj, double dist, const double* n, const double* dv,
                                         double fn) {
        const T* ow = sorted_w + (long long)t * 3;
        const long long j = order[t];
        if (POLY && a.r != rj) {
            // unequal radii: the levers ell_i = (dist + (r_i - r_j)) / 2, and the lever velocity in the pair's id order
            const double ell_i = 0.5 * (dist + (a.r - rj)), ell_j = 0.5 * (dist + (rj - a.r));
            // operands picked first, then ONE evaluation: both particles run the same instructions on them
            const bool a_is_i = a.i < j;
            const double wa[3] = {a_is_i ? a.w[0] : ow[0], a_is_i ? a.w[1] : ow[1], a_is_i ? a.w[2] : ow[2]};
            const double wb[3] = {a_is_i ? ow[0] : a.w[0], a_is_i ? ow[1] : a.w[1], a_is_i ? ow[2] : a.w[2]};
            double lw[3];
            dfl_friction::lever_velocity(a_is_i ? ell_i : ell_j, wa, a_is_i ? ell_j : ell_i, wb, n, lw);
            dfl_friction::contact<true>(c, law, dfl_friction::KEY_PARTNER | (uint64_t)j, n, fn, ell_i, dv, lw);
            return;
        }
        const double ws[3] = {a.w[0] + ow[0], a.w[1] + ow[1], a.w[2] + ow[2]};
        dfl_friction::contact(c, law, dfl_friction::KEY_PARTNER | (uint64_t)j, n, fn, 0.5 * dist, dv, ws);
    }

    // a wall at rest: overlap delta, lever r - delta
    __device__ __forceinline__ void wall(const Particle& a, uint64_t key, const double* n, double delta, double fn) {
        dfl_friction::contact(c, law, key, n, fn, fmax(a.r - delta, 0.0), a.v, a.w);
    }

    __device__ __forceinline__ void finish(const Particle& a, double mass, const dfl_sizes& sz, T* __restrict__ acc,
                                           T* __restrict__ alpha) {
        const double m = POLY ? sz.mass[a.i] : mass;
        dfl_friction::finish(c, hist, a.i, m, POLY ? 0.4 * m * a.r * a.r : law.inertia, acc, alpha);
    }
};

template <bool POLY, bool FRICTION>
using Sink = std::conditional_t<FRICTION, FrictionSink<POLY>, NormalSink<POLY>>;

// The neighbour pairs of particle a, in the fixed order of the sorted copies: cells z, then y, then the x-neighbour cells,
// which are one contiguous run (ascending cell, then particle id).  The search range covers at most two cells per axis
// (cell edge >= 4R, or 4 rmax).  Linear spring-dashpot normal force fn = kn * overlap - gn * (dv . n) along n
template <bool POLY, class Grid, class SinkT>
__device__ __forceinline__ void pair_contacts(const Particle& a, const Grid& grid, const T* __restrict__ sorted,
                                              const I* __restrict__ cell_start, double kn, double gn, const dfl_sizes& sz,
                                              SinkT& sink) {
    const double rng = POLY ? a.r + sz.rmax : 2.0 * a.r;
    const int x0 = grid.coord(0, a.p[0] - rng), x1 = grid.coord(0, a.p[0] + rng);
    const int y0 = grid.coord(1, a.p[1] - rng), y1 = grid.coord(1, a.p[1] + rng);
    const int z0 = grid.coord(2, a.p[2] - rng), z1 = grid.coord(2, a.p[2] + rng);
    const double d2max = 4.0 * a.r * a.r;
    for (int z = z0; z <= z1; ++z) {
        for (int y = y0; y <= y1; ++y) {
            const int c0 = x0 + grid.n(0) * (y + grid.n(1) * z), c1 = x1 + grid.n(0) * (y + grid.n(1) * z);
            for (int t = cell_start[c0]; t < cell_start[c1 + 1]; ++t) {
                if (t == a.s) continue;
                const T* o = sorted + (long long)t * 6;
                const double rx = a.p[0] - o[0], ry = a.p[1] - o[1], rz = a.p[2] - o[2];
                const double d2 = rx * rx + ry * ry + rz * rz;
                const double rj = POLY ? sz.sorted_r[t] : 0.0;
                const double rs = POLY ? a.r + rj : 0.0;
                if (d2 >= (POLY ? rs * rs : d2max) || d2 == 0.0) continue;
                const double dist = sqrt(d2), inv = 1.0 / dist;
                const double n[3] = {rx * inv, ry * inv, rz * inv};
                const double dv[3] = {a.v[0] - o[3], a.v[1] - o[4], a.v[2] - o[5]};
                const double vn = dv[0] * n[0] + dv[1] * n[1] + dv[2] * n[2];
                const double fn = kn * ((POLY ? rs : 2.0 * a.r) - dist) - gn * vn;
                sink.pair(a, t, rj, dist, n, dv, fn);
            }
        }
    }
}

}  // namespace dfl_dem
