// DEM particle contact-force sweep for gfx950: the cell sort, the force kernel of the unit box and the integrators.
//
// BUILD-DEFINED: the reference's Particle.c is a storage container (coord/vel/acc arrays,
// mass 1.0, radius 0.1) whose Add/Update/Remove hooks are empty and whose calls in the time
// loop are commented out (src/Particle.c:120-130, src/main.c:547-569).
// BASELINE.json nevertheless names "the DEM particle contact-force sweep", so the behaviour
// is specified here (and, for the opt-in parts, in include/dedflow.h):
//   spheres of radius R and mass m, or with per-particle r_i and m_i (POLY); linear spring-dashpot normal contact
//       overlap d = r_i + r_j - |xi - xj| > 0,  n = (xi - xj)/|xi - xj|
//       F_ij = (kn * d - gn * ((vi - vj) . n)) n          acc_i = sum_j F_ij / m_i
//   plus the same law against the six walls of the unit box (d = r_i - distance to wall), and optionally (FRICTION) the
//   tangential law with history and the particles' rotation (dem_friction.hpp).
// Neighbour search: uniform cell list, cell edge >= 4R (4 rmax when POLY; a particle's interaction range then covers at
// most two cells per axis), particles sorted by (cell, particle id)
// (counting sort + per-cell ordering => fixed summation order => bitwise reproducible forces).
// The pair loop and the two contact laws are in dem_sweep.hpp, shared with the mesh-wall sweep (k_walls.hip).
// HBM-bound: (48 read + 24 write) B per particle + 24 B per tested neighbour.
#include "dfl_common.hpp"
#include "dem_sweep.hpp"

namespace {

constexpr int BLK = 256;

using dfl_dem::cell_coord;

// The whole sweep is six small dependent launches on the library stream, no allocation, no host round trip:
//   bin    cell of every particle; count[cell]++ (integer atomics: the COUNTS are deterministic, the returned ranks are
//          not -- the segment sort below removes that freedom).  The grid is sized for a few particles per cell, so the
//          atomics are nearly uncontended (a per-chunk counter bumped by every particle cost 18 us of serialised atomics)
//   chunk  total of every 1024-cell chunk (this launch and the next are dfl_scan_counts, k_scan.hip)
//   scan   cell_start = exclusive scan of count (every block adds up the chunk totals before it), count zeroed
//   place  slot[cell_start[cell] + rank] = particle (arrival order)
//   sort   every particle finds its place among the few members of its cell (number of members with a smaller id => the
//          neighbour loops visit particles in a FIXED order: bitwise reproducible forces) and writes its own sorted copy of
//          position / velocity, so that the force kernel streams contiguous runs instead of gathering through order[]
//   force  one thread per sorted slot over the 9 contiguous 3-cell runs around it
__global__ __launch_bounds__(BLK) void dem_bin_kernel(I P, const T* __restrict__ coord, T inv_cell, I ncell, I* __restrict__ cell_of,
                                                     I* __restrict__ rank, I* __restrict__ count) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i >= P) return;
    const int cx = cell_coord(coord[3 * i], inv_cell, ncell);
    const int cy = cell_coord(coord[3 * i + 1], inv_cell, ncell);
    const int cz = cell_coord(coord[3 * i + 2], inv_cell, ncell);
    const int c = cx + ncell * (cy + ncell * cz);
    cell_of[i] = c;
    rank[i] = atomicAdd(&count[c], 1);
}

__global__ __launch_bounds__(BLK) void dem_place_kernel(I P, const I* __restrict__ cell_of, const I* __restrict__ rank,
                                                       const I* __restrict__ cell_start, I* __restrict__ slot) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i >= P) return;
    slot[cell_start[cell_of[i]] + rank[i]] = i;
}

// omega != NULL (friction on): also sorted_w[P][3]; radius != NULL (polydisperse): also sorted_r[P] -- separate arrays, the
// frictionless one-size kernels keep their 48-byte records
__global__ __launch_bounds__(BLK) void dem_sort_cells_kernel(I P, const I* __restrict__ cell_of, const I* __restrict__ cell_start,
                                                            const I* __restrict__ slot, I* __restrict__ order,
                                                            const T* __restrict__ coord, const T* __restrict__ vel,
                                                            const T* __restrict__ omega, const T* __restrict__ radius,
                                                            T* __restrict__ sorted /*[P][6]*/, T* __restrict__ sorted_w,
                                                            T* __restrict__ sorted_r) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i >= P) return;
    const int c = cell_of[i];
    const int lo = cell_start[c], hi = cell_start[c + 1];
    int r = 0;
    for (int a = lo; a < hi; ++a) r += slot[a] < i;  // a handful of members per cell
    const long long pos = lo + r;
    order[pos] = i;
    T* o = sorted + pos * 6;
    o[0] = coord[3 * i]; o[1] = coord[3 * i + 1]; o[2] = coord[3 * i + 2];
    o[3] = vel[3 * i]; o[4] = vel[3 * i + 1]; o[5] = vel[3 * i + 2];
    if (radius) sorted_r[pos] = radius[i];
    if (omega) {
        T* w = sorted_w + pos * 3;
        w[0] = omega[3 * i]; w[1] = omega[3 * i + 1]; w[2] = omega[3 * i + 2];
    }
}

// The force kernel of the unit box: pairs, then the six walls (axis 0..2, side lo then hi); writes acc and, with FRICTION,
// alpha and the particle's new history row.  POLY and FRICTION: dem_sweep.hpp; the arguments a variant does not use
// (sorted_w, law, hist, alpha; R, mass; sz) are not read
template <bool POLY, bool FRICTION>
__global__ __launch_bounds__(BLK) void dem_force_kernel(I P, const T* __restrict__ sorted, const T* __restrict__ sorted_w, T R,
                                                       T mass, dfl_sizes sz, T kn, T gn, dfl_friction_law law, T inv_cell,
                                                       I ncell, const I* __restrict__ order, const I* __restrict__ cell_start,
                                                       dfl_contact_history hist, T* __restrict__ acc, T* __restrict__ alpha) {
    dfl_dem::Particle a;
    a.s = blockIdx.x * BLK + threadIdx.x;
    if (a.s >= P) return;
    a.i = order[a.s];
    a.r = POLY ? sz.sorted_r[a.s] : R;
    dfl_dem::load_state<FRICTION>(a, sorted, sorted_w);
    dfl_dem::Sink<POLY, FRICTION> sink(a, law, hist, sorted_w, order);
    dfl_dem::pair_contacts<POLY>(a, dfl_dem::BoxGrid{inv_cell, ncell}, sorted, cell_start, kn, gn, sz, sink);
    // the frictionless kernel sums its wall forces apart from its pair forces and adds the two sums
    double fw[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int d = 0; d < 3; ++d) {
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            // overlap with the wall x_d = 0 (normal +e_d) or x_d = 1 (normal -e_d)
            const double delta = side == 0 ? a.r - a.p[d] : a.p[d] + a.r - 1.0;
            if (!(delta > 0.0)) continue;
            if constexpr (FRICTION) {
                double n[3] = {0.0, 0.0, 0.0};
                n[d] = side == 0 ? 1.0 : -1.0;
                sink.wall(a, dfl_friction::KEY_WALL | (uint64_t)(2 * d + side), n, delta, kn * delta - gn * (a.v[d] * n[d]));
            } else if (side == 0) {
                fw[d] += kn * delta - gn * a.v[d];
            } else {
                fw[d] -= kn * delta + gn * a.v[d];
            }
        }
    }
    if constexpr (!FRICTION) {
#pragma unroll
        for (int d = 0; d < 3; ++d) sink.f[d] += fw[d];
    }
    sink.finish(a, mass, sz, acc, alpha);
}

// semi-implicit Euler: v += dt a ; x += dt v
__global__ void dem_integrate_kernel(I n3, T dt, T* __restrict__ coord, T* __restrict__ vel, const T* __restrict__ acc) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i >= n3) return;
    const double v = vel[i] + dt * acc[i];
    vel[i] = v;
    coord[i] += dt * v;
}

// semi-implicit Euler with a body acceleration g and rotation: v += dt (a + g) ; x += dt v ; omega += dt alpha
__global__ __launch_bounds__(BLK) void dem_integrate_spin_kernel(I P, T dt, T gx, T gy, T gz, T* __restrict__ coord,
                                                                T* __restrict__ vel, const T* __restrict__ acc,
                                                                T* __restrict__ omega, const T* __restrict__ alpha) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i >= P) return;
    const double g[3] = {gx, gy, gz};
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const long long k = 3 * (long long)i + d;
        const double v = vel[k] + dt * (acc[k] + g[d]);
        vel[k] = v;
        coord[k] += dt * v;
    }
    if (omega) {
#pragma unroll
        for (int d = 0; d < 3; ++d) omega[3 * (long long)i + d] += dt * alpha[3 * (long long)i + d];
    }
}

// omega += dt alpha (after the coupled sub-step, whose kernel integrates v and x)
__global__ void dem_spin_kernel(I n3, T dt, T* __restrict__ omega, const T* __restrict__ alpha) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i >= n3) return;
    omega[i] += dt * alpha[i];
}

}  // namespace

extern "C" {

// count[ncell3 + 1] must be zero on entry (it is again on return); chunk_sum[dfl_scan_num_chunks] and slot[P] are scratch
// chunk / scan / place / sort after a bin pass that left cell_of, rank and count[nbin] (the wall sweep, k_walls.hip, bins
// with its own kernel)
void dfl_dem_sort_binned(I P, I nbin, const T* coord, const T* vel, const T* omega, const T* radius, I* cell_of, I* rank, I* count,
                         I* chunk_sum, I* cell_start, I* slot, I* order, T* sorted, T* sorted_w, T* sorted_r, void* stream) {
    dfl_scan_counts(nbin, count, chunk_sum, cell_start, stream);
    dem_place_kernel<<<ceil_div(P, BLK), BLK, 0, S(stream)>>>(P, cell_of, rank, cell_start, slot);
    dem_sort_cells_kernel<<<ceil_div(P, BLK), BLK, 0, S(stream)>>>(P, cell_of, cell_start, slot, order, coord, vel, omega, radius,
                                                                 sorted, sorted_w, sorted_r);
    DFL_LAUNCH_CHECK();
}

void dfl_dem_build_cells(I P, const T* coord, const T* vel, const T* omega, const T* radius, T cell, I ncell, I* cell_of, I* rank,
                         I* count, I* chunk_sum, I* cell_start, I* slot, I* order, T* sorted, T* sorted_w, T* sorted_r,
                         void* stream) {
    if (P <= 0) return;
    const I ncell3 = ncell * ncell * ncell;
    dem_bin_kernel<<<ceil_div(P, BLK), BLK, 0, S(stream)>>>(P, coord, 1.0 / cell, ncell, cell_of, rank, count);
    dfl_dem_sort_binned(P, ncell3, coord, vel, omega, radius, cell_of, rank, count, chunk_sum, cell_start, slot, order, sorted,
                        sorted_w, sorted_r, stream);
}

void dfl_dem_forces(I P, const T* sorted, const T* sorted_w, T radius, T mass, dfl_sizes sz, T kn, T gamma_n, dfl_friction_law law,
                    T cell, I ncell, const I* order, const I* cell_start, dfl_contact_history hist, T* acc, T* alpha,
                    void* stream) {
    if (P <= 0) return;
    const auto kernel = sz.sorted_r ? (sorted_w ? dem_force_kernel<true, true> : dem_force_kernel<true, false>)
                                    : (sorted_w ? dem_force_kernel<false, true> : dem_force_kernel<false, false>);
    kernel<<<ceil_div(P, BLK), BLK, 0, S(stream)>>>(P, sorted, sorted_w, radius, mass, sz, kn, gamma_n, law, 1.0 / cell, ncell, order,
                                                  cell_start, hist, acc, alpha);
    DFL_LAUNCH_CHECK();
}

void dfl_dem_integrate(I P, T dt, T* coord, T* vel, const T* acc, void* stream) {
    if (P <= 0) return;
    dem_integrate_kernel<<<ceil_div((long long)P * 3, BLK), BLK, 0, S(stream)>>>(3 * P, dt, coord, vel, acc);
    DFL_LAUNCH_CHECK();
}

void dfl_dem_integrate_spin(I P, T dt, const T* g, T* coord, T* vel, const T* acc, T* omega, const T* alpha, void* stream) {
    if (P <= 0) return;
    dem_integrate_spin_kernel<<<ceil_div(P, BLK), BLK, 0, S(stream)>>>(P, dt, g[0], g[1], g[2], coord, vel, acc, omega, alpha);
    DFL_LAUNCH_CHECK();
}

void dfl_dem_spin(I P, T dt, T* omega, const T* alpha, void* stream) {
    if (P <= 0) return;
    dem_spin_kernel<<<ceil_div((long long)P * 3, BLK), BLK, 0, S(stream)>>>(3 * P, dt, omega, alpha);
    DFL_LAUNCH_CHECK();
}

}  // extern "C"
