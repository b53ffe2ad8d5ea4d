// Particle heat transfer for gfx950: contact conduction between touching particles, convection with the fluid, the
// implicit temperature update.  BUILD-DEFINED and opt-in (the reference's particle hooks are empty); the model is stated in
// include/dedflow.h, "particle heat transfer".
//
// One thermal sub-step is three small dependent launches behind the mechanical sub-step, which they do not touch:
//   gather      sorted_t[s] = temp[order[s]]: the temperatures in the contact sweep's cell order, so that the conduction
//               kernel streams its partners' temperatures next to their sorted positions
//   conduction  one thread per sorted slot over dfl_dem::pair_contacts (the pair loop of the force kernels: same sorted
//               copies, same cell list, same overlap test) with a HeatSink: q[i] = sum_j H_ij (T_j - T_i), visit order =
//               the pair loop's => bitwise reproducible; both partners evaluate H with commutative operations on (r_i, r_j)
//               and get exactly opposite heat
//   update      one thread per particle in id order (contiguous per-particle reads and writes, as the drag kernel):
//               gathers the 4 node temperatures and velocities of its tet, Ranz-Marshall Nu, the implicit update, the
//               heat rate and the energy the fluid gave
// The node heat source is the scalar instance of the reaction-load scatter (k_couple.hip, couple_node_kernel<1>).
// All of it is latency-bound at 10^5 particles: (8 + 8) B per particle for the gather, 48 + 8 B per tested neighbour for
// the conduction, 4 gathered node records for the update.
#include "dfl_common.hpp"
#include "dem_sweep.hpp"

namespace {

constexpr int BLK = 256;

__global__ __launch_bounds__(BLK) void heat_gather_kernel(I P, const I* __restrict__ order, const T* __restrict__ temp,
                                                         T* __restrict__ sorted_t) {
    const int s = blockIdx.x * BLK + threadIdx.x;
    if (s >= P) return;
    sorted_t[s] = temp[order[s]];
}

// Conduction sink of the pair loop: Batchelor-O'Brien conductance of the contact circle, H = 2 k_p sqrt(r* delta) with
// r* = r_i r_j / (r_i + r_j), delta = (r_i + r_j) - dist.  Sums and products of (r_i, r_j) only: the partner computes the
// same H bit for bit, and (T_j - T_i) is the exact negation of its (T_i - T_j)
template <bool POLY>
struct HeatSink {
    double q, ti, two_kp;
    const T* __restrict__ sorted_t;

    __device__ __forceinline__ void pair(const dfl_dem::Particle& a, int t, double rj_, double dist, const double*, const double*,
                                         double) {
        const double rj = POLY ? rj_ : a.r;
        const double rs = a.r + rj;
        const double rstar = (a.r * rj) / rs;
        const double h = two_kp * sqrt(rstar * (rs - dist));
        q += h * (sorted_t[t] - ti);
    }
};

// q[i] = conduction heat rate into particle i.  nbin_in = the number of cells a neighbour loop can reach: the slots from
// cell_start[nbin_in] on are the particles outside a mesh grid (none on the unit box), which have no partner
template <bool POLY, class Grid>
__global__ __launch_bounds__(BLK) void heat_conduction_kernel(I P, const T* __restrict__ sorted, T R, dfl_sizes sz, Grid grid,
                                                             I nbin_in, const I* __restrict__ order,
                                                             const I* __restrict__ cell_start, const T* __restrict__ sorted_t,
                                                             T two_kp, T* __restrict__ q) {
    dfl_dem::Particle a;
    a.s = blockIdx.x * BLK + threadIdx.x;
    if (a.s >= P) return;
    a.i = order[a.s];
    if (a.s >= cell_start[nbin_in]) {
        q[a.i] = 0.0;
        return;
    }
    a.r = POLY ? sz.sorted_r[a.s] : R;
    dfl_dem::load_state<false>(a, sorted, nullptr);
    HeatSink<POLY> sink{0.0, sorted_t[a.s], two_kp, sorted_t};
    dfl_dem::pair_contacts<POLY>(a, grid, sorted, cell_start, 0.0, 0.0, sz, sink);
    q[a.i] = sink.q;
}

// The thermal update of particle i (include/dedflow.h): with a fluid state and a tet, convection implicit in T_i;
// else conduction only.  q may be NULL (no contact conduction); w NULL or tet NULL: uncoupled.  POLY: m[i], r[i].  LASER:
// the absorbed laser power p[i] joins q[i] (k_laser.hip); without it the arithmetic is that of a context with no laser
template <bool POLY, bool LASER>
__global__ __launch_bounds__(BLK) void heat_update_kernel(I P, const I* __restrict__ tet, const T* __restrict__ lambda,
                                                         const I* __restrict__ ien, const T* __restrict__ w, I N, T mass_,
                                                         T radius_, const T* __restrict__ m, const T* __restrict__ r,
                                                         const T* __restrict__ vel, T cp_p, T k_f, T rho_f, T mu_f, T pr13, T dt,
                                                         const T* __restrict__ q, const T* __restrict__ p,
                                                         T* __restrict__ temp, T* __restrict__ rate, T* __restrict__ e) {
    const long long i = (long long)blockIdx.x * BLK + threadIdx.x;
    if (i >= P) return;
    const double mass = POLY ? m[i] : mass_, radius = POLY ? r[i] : radius_;
    const double cap = mass * cp_p;
    const double ti = temp[i];
    double qc;
    if constexpr (LASER) qc = ((q ? q[i] : 0.0) + p[i]) / cap;
    else qc = q ? q[i] / cap : 0.0;
    const int t = (w && tet) ? tet[i] : -1;
    double tn;
    if (t >= 0) {
        double tf = 0.0, uf[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const double l = lambda[4 * i + b];
            const long long n = ien[4LL * t + b];
            tf += l * w[5LL * N + n];
#pragma unroll
            for (int d = 0; d < 3; ++d) uf[d] += l * w[3 * n + d];
        }
        const double diam = 2.0 * radius;
        const double sx = uf[0] - vel[3 * i], sy = uf[1] - vel[3 * i + 1], sz = uf[2] - vel[3 * i + 2];
        const double re = rho_f * sqrt(sx * sx + sy * sy + sz * sz) * diam / mu_f;
        const double nu = 2.0 + 0.6 * sqrt(re) * pr13;
        const double itau = (nu * k_f * M_PI * diam) / cap;  // 1 / tau_T
        tn = (ti + dt * (qc + tf * itau)) / (1.0 + dt * itau);
        e[i] += dt * cap * (tf - tn) * itau;
    } else {
        tn = ti + dt * qc;
    }
    temp[i] = tn;
    rate[i] = dt != 0.0 ? cap * (tn - ti) / dt : 0.0;  // a zero step moves no heat
}

// the thermal state of the particles ParticleContextAdd has just appended at ids [first, first + count)
__global__ __launch_bounds__(BLK) void heat_fill_kernel(I first, I count, T t_init, T* __restrict__ temp, T* __restrict__ rate,
                                                       T* __restrict__ e) {
    const int k = blockIdx.x * BLK + threadIdx.x;
    if (k >= count) return;
    temp[first + k] = t_init;
    rate[first + k] = 0.0;
    e[first + k] = 0.0;
}

}  // namespace

extern "C" {

void dfl_heat_gather(I P, const I* order, const T* temp, T* sorted_t, void* stream) {
    if (P <= 0) return;
    heat_gather_kernel<<<ceil_div(P, BLK), BLK, 0, S(stream)>>>(P, order, temp, sorted_t);
    DFL_LAUNCH_CHECK();
}

void dfl_heat_conduction(I P, const T* sorted, T radius, dfl_sizes sz, T cell, I ncell, const I* order, const I* cell_start,
                         const T* sorted_t, T k_p, T* q, void* stream) {
    if (P <= 0) return;
    const dfl_dem::BoxGrid g{1.0 / cell, ncell};
    const I nbin = ncell * ncell * ncell;
    const auto kernel = sz.sorted_r ? heat_conduction_kernel<true, dfl_dem::BoxGrid> : heat_conduction_kernel<false, dfl_dem::BoxGrid>;
    kernel<<<ceil_div(P, BLK), BLK, 0, S(stream)>>>(P, sorted, radius, sz, g, nbin, order, cell_start, sorted_t, 2.0 * k_p, q);
    DFL_LAUNCH_CHECK();
}

void dfl_heat_conduction_grid(I P, const T* sorted, T radius, dfl_sizes sz, dfl_grid3 grid, const I* order, const I* cell_start,
                              const T* sorted_t, T k_p, T* q, void* stream) {
    if (P <= 0) return;
    const dfl_dem::MeshGrid g{grid};
    const I nbin = grid.n[0] * grid.n[1] * grid.n[2];
    const auto kernel = sz.sorted_r ? heat_conduction_kernel<true, dfl_dem::MeshGrid> : heat_conduction_kernel<false, dfl_dem::MeshGrid>;
    kernel<<<ceil_div(P, BLK), BLK, 0, S(stream)>>>(P, sorted, radius, sz, g, nbin, order, cell_start, sorted_t, 2.0 * k_p, q);
    DFL_LAUNCH_CHECK();
}

void dfl_heat_update(I P, const I* tet, const T* lambda, const I* ien, const T* w, I N, T mass, T radius, const T* m, const T* r,
                     const T* vel, T cp_p, T k_f, T rho_f, T mu_f, T pr13, T dt, const T* q, const T* laser, T* temp, T* rate, T* e,
                     void* stream) {
    if (P <= 0) return;
    const auto kernel = laser ? (m ? heat_update_kernel<true, true> : heat_update_kernel<false, true>)
                              : (m ? heat_update_kernel<true, false> : heat_update_kernel<false, false>);
    kernel<<<ceil_div(P, BLK), BLK, 0, S(stream)>>>(P, tet, lambda, ien, w, N, mass, radius, m, r, vel, cp_p, k_f, rho_f, mu_f, pr13,
                                                  dt, q, laser, temp, rate, e);
    DFL_LAUNCH_CHECK();
}

void dfl_heat_fill(I first, I count, T t_init, T* temp, T* rate, T* e, void* stream) {
    if (count <= 0) return;
    heat_fill_kernel<<<ceil_div(count, BLK), BLK, 0, S(stream)>>>(first, count, t_init, temp, rate, e);
    DFL_LAUNCH_CHECK();
}

}  // extern "C"
