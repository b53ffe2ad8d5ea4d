// Particle-fluid coupling for gfx950: point location on the tet mesh, drag + gravity sub-step, reaction load.
//
// BUILD-DEFINED, like the contact sweep of k_dem.hip: the reference keeps SolveParticleSystem / ParticleContextUpdate
// commented out of its time loop and has no coupling physics.  The model (include/dedflow.h, "particle-fluid coupling"):
//   location   remembering visibility walk over the tet neighbour table from the previous tet or a seed-grid tet;
//              exact for convex domains (a point behind a boundary face is outside), every walk capped at DFL_COUPLE_MAX_WALK
//   drag       Schiller-Naumann, integrated implicitly in v with the factor f lagged (stable for any dt / tau)
//   reaction   the drag impulse of every particle, spread to the nodes of its tet with the barycentric weights, summed in a
//              fixed order (particles counting-sorted by tet, stable by id; nodes walk their sorted V2E lists): no float
//              atomics, bitwise reproducible
// All of it is gather-bound: a particle reads 4 vertex records of 24 B (location), 4 nodal velocities of 24 B (drag) at
// random; the node pass reads its V2E list and the few particles per tet.
#include "dfl_common.hpp"

namespace {

constexpr int BLK = 256;
constexpr double LAMBDA_EPS = 1e-12;

// sort every node's V2E list ascending (GenerateV2EMapColTetGPU fills them in arrival order); a few dozen entries per node
__global__ __launch_bounds__(BLK) void couple_v2e_sort_kernel(I N, const I* __restrict__ vrow, I* __restrict__ vcol) {
    const int a = blockIdx.x * BLK + threadIdx.x;
    if (a >= N) return;
    const int lo = vrow[a], hi = vrow[a + 1];
    for (int i = lo + 1; i < hi; ++i) {
        const int v = vcol[i];
        int j = i - 1;
        while (j >= lo && vcol[j] > v) {
            vcol[j + 1] = vcol[j];
            --j;
        }
        vcol[j + 1] = v;
    }
}

// nbr[4t + k] = the tet across the face of t opposite local vertex k (it shares the face's three vertices), -1 on the boundary
__global__ __launch_bounds__(BLK) void couple_nbr_kernel(I T_, const I* __restrict__ ien, const I* __restrict__ vrow,
                                                        const I* __restrict__ vcol, I* __restrict__ nbr) {
    const long long tk = (long long)blockIdx.x * BLK + threadIdx.x;
    if (tk >= 4LL * T_) return;
    const int t = (int)(tk >> 2), k = (int)(tk & 3);
    int f[3], m = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j != k) f[m++] = ien[4LL * t + j];
    int found = -1;
    for (int q = vrow[f[0]]; q < vrow[f[0] + 1]; ++q) {  // ascending: the lowest id wins on a non-conforming mesh
        const int e = vcol[q];
        if (e == t) continue;
        const int* v = ien + 4LL * e;
        bool h1 = false, h2 = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            h1 |= v[j] == f[1];
            h2 |= v[j] == f[2];
        }
        if (h1 && h2) {
            found = e;
            break;
        }
    }
    nbr[tk] = found;
}

// barycentric coordinates of p in the tet (x0, x1, x2, x3): lambda_k = signed volume with vertex k replaced by p / volume
__device__ __forceinline__ void barycentric(const double* x, const double p[3], double lam[4]) {
    const double e1[3] = {x[3] - x[0], x[4] - x[1], x[5] - x[2]};
    const double e2[3] = {x[6] - x[0], x[7] - x[1], x[8] - x[2]};
    const double e3[3] = {x[9] - x[0], x[10] - x[1], x[11] - x[2]};
    const double r[3] = {p[0] - x[0], p[1] - x[1], p[2] - x[2]};
    const double c23[3] = {e2[1] * e3[2] - e2[2] * e3[1], e2[2] * e3[0] - e2[0] * e3[2], e2[0] * e3[1] - e2[1] * e3[0]};
    const double c31[3] = {e3[1] * e1[2] - e3[2] * e1[1], e3[2] * e1[0] - e3[0] * e1[2], e3[0] * e1[1] - e3[1] * e1[0]};
    const double c12[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double inv = 1.0 / (e1[0] * c23[0] + e1[1] * c23[1] + e1[2] * c23[2]);
    lam[1] = (r[0] * c23[0] + r[1] * c23[1] + r[2] * c23[2]) * inv;
    lam[2] = (r[0] * c31[0] + r[1] * c31[1] + r[2] * c31[2]) * inv;
    lam[3] = (r[0] * c12[0] + r[1] * c12[1] + r[2] * c12[2]) * inv;
    lam[0] = 1.0 - lam[1] - lam[2] - lam[3];
}

__device__ __forceinline__ unsigned mix32(unsigned h) {
    h ^= h >> 16; h *= 0x7feb352du;
    h ^= h >> 15; h *= 0x846ca68bu;
    h ^= h >> 16;
    return h;
}

__device__ __forceinline__ int grid_coord(double x, double lo, double inv_h, int g) {
    const double c = floor((x - lo) * inv_h);
    return c >= (double)g ? g - 1 : (c >= 1.0 ? (int)c : 0);  // a NaN compares false twice: cell 0, and is never converted
}

// one thread per particle (in the contact sweep's cell order when `order` is given): walk from the previous tet, or from
// the seed-grid tet of the particle's grid cell, across the face with the most negative lambda.  Only faces with an inner
// neighbour are crossed; a tet whose negative faces are all boundary faces means "outside" (exact for convex domains).
// When several inner faces are negative, one step in four takes a hashed one instead of the most negative (breaks cycles).
__global__ __launch_bounds__(BLK) void couple_locate_kernel(I P, const I* __restrict__ order, const T* __restrict__ coord,
                                                           const T* __restrict__ xg, const I* __restrict__ ien,
                                                           const I* __restrict__ nbr, const I* __restrict__ seed, T lo0, T lo1,
                                                           T lo2, T inv_h0, T inv_h1, T inv_h2, I gdim, I* __restrict__ tet,
                                                           T* __restrict__ lambda, I* __restrict__ lost) {
    const int s = blockIdx.x * BLK + threadIdx.x;
    if (s >= P) return;
    const int i = order ? order[s] : s;
    const double p[3] = {coord[3LL * i], coord[3LL * i + 1], coord[3LL * i + 2]};
    int t = tet[i];
    if (t < 0) {
        const int cx = grid_coord(p[0], lo0, inv_h0, gdim), cy = grid_coord(p[1], lo1, inv_h1, gdim),
                  cz = grid_coord(p[2], lo2, inv_h2, gdim);
        t = seed[cx + gdim * (cy + gdim * cz)];
    }
    const bool finite = isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);
    double lam[4] = {0.0, 0.0, 0.0, 0.0};
    int result = t < 0 ? -1 : -2;  // (a seed grid without a tet: a mesh without tets)
    for (int step = 0; t >= 0 && step < DFL_COUPLE_MAX_WALK; ++step) {
        double x[12];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const long long v = ien[4LL * t + b];
#pragma unroll
            for (int d = 0; d < 3; ++d) x[3 * b + d] = xg[3 * v + d];
        }
        barycentric(x, p, lam);
        // every lambda by comparison: fmin drops a NaN, and a tet must never accept a lambda that is one
        if (lam[0] >= -LAMBDA_EPS && lam[1] >= -LAMBDA_EPS && lam[2] >= -LAMBDA_EPS && lam[3] >= -LAMBDA_EPS) {
            result = t;
            break;
        }
        if (!finite) {  // no tet accepts an inf or a NaN (lambda_1..3 are none of them finite); outside, and no walk on them
            result = -1;
            break;
        }
        int nb[4], cand[4], ncand = 0, best = -1;
        double bestl = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            nb[k] = nbr[4LL * t + k];
            if (lam[k] < -LAMBDA_EPS && nb[k] >= 0) {
                cand[ncand++] = k;
                if (best < 0 || lam[k] < bestl) {
                    best = k;
                    bestl = lam[k];
                }
            }
        }
        if (ncand == 0) {  // behind boundary faces only
            result = -1;
            break;
        }
        if (ncand > 1) {
            const unsigned h = mix32((unsigned)i * 0x9e3779b9u ^ (unsigned)step);
            if ((h & 3u) == 0u) best = cand[(h >> 2) % (unsigned)ncand];
        }
        t = nb[best];
    }
    if (result == -2) atomicAdd(lost, 1);
    tet[i] = result;
#pragma unroll
    for (int k = 0; k < 4; ++k) lambda[4LL * i + k] = result >= 0 ? lam[k] : 0.0;
}

// fluid sub-step of one particle: u_f = sum_a lambda_a u(node_a); Schiller-Naumann drag integrated implicitly in v
// (f lagged), gravity reduced by buoyancy; outside the fluid (tet < 0) gravity only.  acc <- the applied acceleration,
// imp += the drag impulse of the step (for the reaction load).  POLY: mass and radius of particle i are m[i] and r[i]
template <bool POLY>
__global__ __launch_bounds__(BLK) void couple_fluid_kernel(I P, const I* __restrict__ order, const I* __restrict__ tet,
                                                          const T* __restrict__ lambda, const I* __restrict__ ien,
                                                          const T* __restrict__ w, T mass_, T radius_, T rho_f, T mu_f, T g0,
                                                          T g1, T g2, T dt, T* __restrict__ coord, T* __restrict__ vel,
                                                          T* __restrict__ acc, T* __restrict__ imp, const T* __restrict__ m,
                                                          const T* __restrict__ r) {
    const int s = blockIdx.x * BLK + threadIdx.x;
    if (s >= P) return;
    const long long i = order ? order[s] : s;
    const double g[3] = {g0, g1, g2};
    double v[3], a[3], vn[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        v[d] = vel[3 * i + d];
        a[d] = acc[3 * i + d];
    }
    const int t = tet[i];
    if (t >= 0) {
        const double mass = POLY ? m[i] : mass_, radius = POLY ? r[i] : radius_;
        double uf[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const double l = lambda[4 * i + b];
            const long long n = ien[4LL * t + b];
#pragma unroll
            for (int d = 0; d < 3; ++d) uf[d] += l * w[3 * n + d];
        }
        const double diam = 2.0 * radius;
        const double rho_p = mass / (4.0 / 3.0 * M_PI * radius * radius * radius);
        const double sx = uf[0] - v[0], sy = uf[1] - v[1], sz = uf[2] - v[2];
        const double re = rho_f * sqrt(sx * sx + sy * sy + sz * sz) * diam / mu_f;
        const double f = re <= 1000.0 ? 1.0 + 0.15 * pow(re, 0.687) : 0.44 * re / 24.0;
        const double tau = rho_p * diam * diam / (18.0 * mu_f);
        const double k = f / tau;
        const double buoy = 1.0 - rho_f / rho_p;
        const double den = 1.0 / (1.0 + dt * k);
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            vn[d] = (v[d] + dt * (a[d] + buoy * g[d] + k * uf[d])) * den;
            imp[3 * i + d] += mass * k * (uf[d] - vn[d]) * dt;
        }
    } else {
#pragma unroll
        for (int d = 0; d < 3; ++d) vn[d] = v[d] + dt * (a[d] + g[d]);
    }
    const double idt = 1.0 / dt;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        vel[3 * i + d] = vn[d];
        coord[3 * i + d] += dt * vn[d];
        acc[3 * i + d] = (vn[d] - v[d]) * idt;
    }
}

// counting sort of the located particles by tet: count (integer atomics: the counts are deterministic, the ranks are not),
// place at tstart + rank, then each particle takes the position of its id among its tet's members (stable by id)
__global__ __launch_bounds__(BLK) void couple_count_kernel(I P, const I* __restrict__ tet, I* __restrict__ tcount,
                                                          I* __restrict__ rank) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i >= P) return;
    const int t = tet[i];
    rank[i] = t >= 0 ? atomicAdd(&tcount[t], 1) : -1;
}

__global__ __launch_bounds__(BLK) void couple_place_kernel(I P, const I* __restrict__ tet, const I* __restrict__ tstart,
                                                          const I* __restrict__ rank, I* __restrict__ slot, I* __restrict__ tcount) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i >= P) return;
    const int t = tet[i];
    if (t < 0) return;
    slot[tstart[t] + rank[i]] = i;
    tcount[t] = 0;  // the scan has consumed the counts: zero again for the next call
}

__global__ __launch_bounds__(BLK) void couple_stable_kernel(I P, const I* __restrict__ tet, const I* __restrict__ tstart,
                                                           const I* __restrict__ slot, I* __restrict__ members) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i >= P) return;
    const int t = tet[i];
    if (t < 0) return;
    const int lo = tstart[t], hi = tstart[t + 1];
    int r = 0;
    for (int q = lo; q < hi; ++q) r += slot[q] < i;
    members[lo + r] = i;
}

// load[C a + d] = -scale * sum over the tets e of node a (ascending) and the particles p of e (ascending id) of
// lambda_{p, k(a, e)} imp[p][d], d < C.  C = 3: the reaction load of the drag impulses; C = 1: the heat source of the
// particles' pending energy (k_heat.hip); C = 5: the deposits of captured particles (k_capture.hip)
template <int C>
__global__ __launch_bounds__(BLK) void couple_node_kernel(I N, const I* __restrict__ vrow, const I* __restrict__ vcol,
                                                         const I* __restrict__ ien, const I* __restrict__ tstart,
                                                         const I* __restrict__ members, const T* __restrict__ lambda,
                                                         const T* __restrict__ imp, T scale, T* __restrict__ load) {
    const int a = blockIdx.x * BLK + threadIdx.x;
    if (a >= N) return;
    double s[C];
#pragma unroll
    for (int d = 0; d < C; ++d) s[d] = 0.0;
    for (int q = vrow[a]; q < vrow[a + 1]; ++q) {
        const int e = vcol[q];
        const int lo = tstart[e], hi = tstart[e + 1];
        if (lo == hi) continue;
        int k = 0;
#pragma unroll
        for (int j = 1; j < 4; ++j)
            if (ien[4LL * e + j] == a) k = j;
        for (int m = lo; m < hi; ++m) {
            const long long p = members[m];
            const double l = lambda[4 * p + k];
#pragma unroll
            for (int d = 0; d < C; ++d) s[d] += l * imp[C * p + d];
        }
    }
#pragma unroll
    for (int d = 0; d < C; ++d) load[(long long)C * a + d] = -scale * s[d];
}

}  // namespace

extern "C" {

void dfl_couple_sort_v2e(I N, const I* vrow, I* vcol, void* stream) {
    if (N <= 0) return;
    couple_v2e_sort_kernel<<<ceil_div(N, BLK), BLK, 0, S(stream)>>>(N, vrow, vcol);
    DFL_LAUNCH_CHECK();
}

void dfl_couple_neighbours(I T_, const I* ien, const I* vrow, const I* vcol, I* nbr, void* stream) {
    if (T_ <= 0) return;
    couple_nbr_kernel<<<ceil_div(4LL * T_, BLK), BLK, 0, S(stream)>>>(T_, ien, vrow, vcol, nbr);
    DFL_LAUNCH_CHECK();
}

void dfl_couple_locate(I P, const I* order, const T* coord, const T* xg, const I* ien, const I* nbr, const I* seed,
                       const T* grid_lo, const T* grid_inv_h, I grid_dim, I* tet, T* lambda, I* lost, void* stream) {
    if (P <= 0) return;
    couple_locate_kernel<<<ceil_div(P, BLK), BLK, 0, S(stream)>>>(P, order, coord, xg, ien, nbr, seed, grid_lo[0], grid_lo[1],
                                                                grid_lo[2], grid_inv_h[0], grid_inv_h[1], grid_inv_h[2],
                                                                grid_dim, tet, lambda, lost);
    DFL_LAUNCH_CHECK();
}

void dfl_couple_fluid_step(I P, const I* order, const I* tet, const T* lambda, const I* ien, const T* w, T mass, T radius,
                           const T* mass_i, const T* radius_i, T rho_f, T mu_f, const T* gravity, T dt, T* coord, T* vel, T* acc,
                           T* imp, void* stream) {
    if (P <= 0) return;
    if (radius_i)
        couple_fluid_kernel<true><<<ceil_div(P, BLK), BLK, 0, S(stream)>>>(P, order, tet, lambda, ien, w, 0.0, 0.0, rho_f, mu_f,
                                                                         gravity[0], gravity[1], gravity[2], dt, coord, vel, acc,
                                                                         imp, mass_i, radius_i);
    else
        couple_fluid_kernel<false><<<ceil_div(P, BLK), BLK, 0, S(stream)>>>(P, order, tet, lambda, ien, w, mass, radius, rho_f, mu_f,
                                                                          gravity[0], gravity[1], gravity[2], dt, coord, vel, acc,
                                                                          imp, nullptr, nullptr);
    DFL_LAUNCH_CHECK();
}

void dfl_couple_sort_by_tet(I P, I T_, const I* tet, I* tcount, I* rank, I* tstart, I* slot, I* members, void* scan_temp,
                            int64_t scan_temp_bytes, void* stream) {
    if (P > 0) couple_count_kernel<<<ceil_div(P, BLK), BLK, 0, S(stream)>>>(P, tet, tcount, rank);
    dfl_exclusive_scan_i32(T_, tcount, tstart, scan_temp, scan_temp_bytes, stream);
    if (P > 0) {
        couple_place_kernel<<<ceil_div(P, BLK), BLK, 0, S(stream)>>>(P, tet, tstart, rank, slot, tcount);
        couple_stable_kernel<<<ceil_div(P, BLK), BLK, 0, S(stream)>>>(P, tet, tstart, slot, members);
    }
    DFL_LAUNCH_CHECK();
}

void dfl_couple_node_load(I N, const I* vrow, const I* vcol, const I* ien, const I* tstart, const I* members, const T* lambda,
                          const T* imp, T scale, T* load, void* stream) {
    if (N <= 0) return;
    couple_node_kernel<3><<<ceil_div(N, BLK), BLK, 0, S(stream)>>>(N, vrow, vcol, ien, tstart, members, lambda, imp, scale, load);
    DFL_LAUNCH_CHECK();
}

void dfl_couple_node_scalar(I N, const I* vrow, const I* vcol, const I* ien, const I* tstart, const I* members, const T* lambda,
                            const T* e, T scale, T* out, void* stream) {
    if (N <= 0) return;
    couple_node_kernel<1><<<ceil_div(N, BLK), BLK, 0, S(stream)>>>(N, vrow, vcol, ien, tstart, members, lambda, e, scale, out);
    DFL_LAUNCH_CHECK();
}

void dfl_couple_node_deposit(I N, const I* vrow, const I* vcol, const I* ien, const I* tstart, const I* members, const T* lambda,
                             const T* dep, T scale, T* out, void* stream) {
    if (N <= 0) return;
    couple_node_kernel<5><<<ceil_div(N, BLK), BLK, 0, S(stream)>>>(N, vrow, vcol, ien, tstart, members, lambda, dep, scale, out);
    DFL_LAUNCH_CHECK();
}

}  // extern "C"
