// Solid-surface contact for gfx950: every particle against the implicit surface phi = level where the fluid counts as solid
// (build-defined, opt-in: ParticleContextSetSurfaceContact; the model and its operation order are stated in
// include/dedflow.h, "solid-surface contact").
//
// One launch per coupled sub-step, one thread per particle in id order, as the drag and capture kernels (k_couple.hip,
// k_capture.hip): tet, weights, acc, alpha and the history row of a particle are contiguous per particle, the node data
// are gathered at random, and at the particle counts of a powder stream the kernel is bound by the latency of its two
// dependent gathers (tet -> ien -> nodes), not by bytes.  The gathers are ordered so that the common particle, far away on
// the gas side, leaves after the first: ien, lambda and phi give f = phi_p - level and the spread of phi over the tet;
// |g| <= (|phi_1 - phi_0| + |phi_2 - phi_0| + |phi_3 - phi_0|) grad_max with grad_max >= |grad N_k| over the mesh (one pass
// over the tets at Set), so q > r spread grad_max proves s = q / |g| > r without T and without the twelve coordinates.  The bound only
// skips work: every particle that passes it takes the full decision.  Integer atomics only (the counters, one per
// workgroup, and the sweeps' overflow count); LDS for those four counts only; a particle without contact is not written at all.
#include "dfl_common.hpp"

// the operation order is part of the model, through the friction law too: no fused multiply-add from here on
#pragma clang fp contract(off)

#include "dem_friction.hpp"
#include "tet_levelset.hpp"

namespace {

constexpr int BLK = 256;
constexpr int MAXH = DFL_DEM_MAX_HISTORY;
constexpr double FAR_MARGIN = 1.0 + 1e-6;  // far above the roundings of q, the spread and grad_max

// |x| as an integer that orders like |x|, with every NaN above +inf: a maximum over these never loses a NaN
__device__ __forceinline__ unsigned long long abs_bits(double x) { return (unsigned long long)__double_as_longlong(fabs(x)); }

// grad_max = the largest |c_k| / |det| (k = 1, 2, 3) over the tets, from the very tet_cross() the contact kernel divides by:
// its computed g = sum_k d_k c_k / det then obeys |g| <= (|d_1| + |d_2| + |d_3|) grad_max to a few roundings whatever
// the shape of the tet.  A degenerate tet or a coordinate that is not finite leaves inf or a NaN, and nothing leaves early
__global__ __launch_bounds__(BLK) void surface_grad_max_kernel(I T_, const I* __restrict__ ien, const T* __restrict__ xg,
                                                              unsigned long long* __restrict__ out) {
    const long long t = (long long)blockIdx.x * BLK + threadIdx.x;
    unsigned long long best = 0;
    if (t < T_) {
        double x[12];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const long long n = ien[4 * t + b];
#pragma unroll
            for (int d = 0; d < 3; ++d) x[3 * b + d] = xg[3 * n + d];
        }
        TetCross c;
        tet_cross(x, c);
        const double* ck[3] = {c.c23, c.c31, c.c12};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const unsigned long long g = abs_bits(sqrt((ck[k][0] * ck[k][0] + ck[k][1] * ck[k][1]) + ck[k][2] * ck[k][2]) / c.det);
            best = g > best ? g : best;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(best, off, WAVE);
        best = o > best ? o : best;
    }
    __shared__ unsigned long long wave_best[BLK / WAVE];
    if ((threadIdx.x & (WAVE - 1)) == 0) wave_best[threadIdx.x / WAVE] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < BLK / WAVE; ++k) best = wave_best[k] > best ? wave_best[k] : best;
        atomicMax(out, best);  // one per workgroup, once per mesh
    }
}

// POLY: radius and mass of particle i are sz.radius[i] and sz.mass[i].  FRICTION: the tangential law with history and the
// torque on top of the normal force
template <bool POLY, bool FRICTION>
__global__ __launch_bounds__(BLK) void surface_contact_kernel(I P, const I* __restrict__ tet, const T* __restrict__ lambda,
                                                             const I* __restrict__ ien, const T* __restrict__ xg,
                                                             const T* __restrict__ w, I N, const T* __restrict__ vel,
                                                             const T* __restrict__ omega, T mass_, T radius_, dfl_sizes sz, T kn,
                                                             T gn, dfl_friction_law law, T level, T side, T T_solid,
                                                             const T* __restrict__ grad_max_,
                                                             dfl_contact_history hist, dfl_surface_counters* __restrict__ cnt,
                                                             int cur, T* __restrict__ acc, T* __restrict__ alpha) {
    const long long i = (long long)blockIdx.x * BLK + threadIdx.x;
    if (i < DFL_SURFACE_SLOTS) {  // (one full wave) the counts of the launch before this one are complete: into the total,
                                  // and cleared for the next launch
        unsigned long long* old = &cnt->step[1 - cur][i * DFL_SURFACE_SLOT_STRIDE];
        unsigned c = (unsigned)(*old & 0xffffffffull);
        *old = 0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, WAVE);
        if (i == 0) cnt->total += (long long)c;
    }
    bool contact = false, buried = false;
    const int t = i < P ? tet[i] : -1;
    if (t >= 0) {
        long long n[4];
        double l[4], phi[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            n[b] = ien[4LL * t + b];
            l[b] = lambda[4 * i + b];
            phi[b] = w[4LL * N + n[b]];
        }
        const double radius = POLY ? sz.radius[i] : radius_;
        // contiguous per particle: read with the first gather, not in a round of its own behind the decision
        const double v[3] = {vel[3 * i], vel[3 * i + 1], vel[3 * i + 2]};
        const double q = -(side * (tet_interp(l, phi) - level));
        const double spread = (fabs(phi[1] - phi[0]) + fabs(phi[2] - phi[0])) + fabs(phi[3] - phi[0]);
        // (a NaN compares false and takes the full decision, which refuses it)
        const double grad_max = *grad_max_;
        const bool far = grad_max > 0.0 && q > (radius * (spread * grad_max)) * FAR_MARGIN;
        if (!far) {
            double tf[4], x[12];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                tf[b] = w[5LL * N + n[b]];
#pragma unroll
                for (int d = 0; d < 3; ++d) x[3 * b + d] = xg[3 * n[b] + d];
            }
            const double T_f = tet_interp(l, tf);
            TetCross c;
            tet_cross(x, c);
            double g[3], gnorm, dist[4];
            if (tet_levelset(c, phi, level, g, gnorm, dist) && T_f < T_solid) {
                const double s = q / gnorm;
                contact = s > -radius && s < radius;
                buried = s <= -radius;
                if (contact) {
                    const double nrm[3] = {(-(side * g[0])) / gnorm, (-(side * g[1])) / gnorm, (-(side * g[2])) / gnorm};
                    const double delta = radius - s;
                    const double vn = (v[0] * nrm[0] + v[1] * nrm[1]) + v[2] * nrm[2];
                    const double fn = kn * delta - gn * vn;
                    const double mass = POLY ? sz.mass[i] : mass_;
                    const double im = 1.0 / mass;
                    if (FRICTION) {
                        // the previous sweep's row for the lookup; the row this sub-step's sweep wrote, at its count
                        dfl_friction::Contacts k;
                        k.old = hist.old_row + i * MAXH;
                        k.out = hist.new_row + i * MAXH;
                        k.nold = hist.old_count[i];
                        k.nnew = hist.new_count[i];
                        k.over = 0;
                        k.f[0] = k.f[1] = k.f[2] = 0.0;
                        k.tau[0] = k.tau[1] = k.tau[2] = 0.0;
                        const double om[3] = {omega[3 * i], omega[3 * i + 1], omega[3 * i + 2]};
                        dfl_friction::contact(k, law, dfl_friction::KEY_SURFACE, nrm, fn, fmax(radius - delta, 0.0), v, om);
                        const double ii = 1.0 / (POLY ? 0.4 * mass * radius * radius : law.inertia);
#pragma unroll
                        for (int d = 0; d < 3; ++d) {
                            acc[3 * i + d] += k.f[d] * im;
                            alpha[3 * i + d] += k.tau[d] * ii;
                        }
                        hist.new_count[i] = k.nnew;
                        if (k.over) atomicAdd(hist.overflow, k.over);
                    } else {
#pragma unroll
                        for (int d = 0; d < 3; ++d) acc[3 * i + d] += (fn * nrm[d]) * im;
                    }
                }
            }
        }
    }
    // one atomic per workgroup that has anything to count, in contact in the low and buried in the high 32 bits, spread over
    // DFL_SURFACE_SLOTS cache lines: device-scope atomics on one address serialise across the whole chip (one per wave on one
    // counter cost more than the rest of the kernel)
    __shared__ unsigned long long wave_count[BLK / WAVE];
    const unsigned long long mc = __ballot(contact), mb = __ballot(buried);
    if ((threadIdx.x & (WAVE - 1)) == 0)
        wave_count[threadIdx.x / WAVE] = (unsigned long long)__popcll(mc) | ((unsigned long long)__popcll(mb) << 32);
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long c = (wave_count[0] + wave_count[1]) + (wave_count[2] + wave_count[3]);
        if (c) atomicAdd(&cnt->step[cur][(blockIdx.x % DFL_SURFACE_SLOTS) * DFL_SURFACE_SLOT_STRIDE], c);
    }
}

}  // namespace

extern "C" {

void dfl_surface_grad_max(I T_, const I* ien, const T* xg, T* grad_max, void* stream) {
    DFL_GUARD(hipMemsetAsync(grad_max, 0, sizeof(T), S(stream)));
    if (T_ <= 0) return;
    surface_grad_max_kernel<<<ceil_div(T_, BLK), BLK, 0, S(stream)>>>(T_, ien, xg, reinterpret_cast<unsigned long long*>(grad_max));
    DFL_LAUNCH_CHECK();
}

void dfl_surface_contact(I P, const I* tet, const T* lambda, const I* ien, const T* xg, const T* w, I N, const T* vel, const T* omega,
                         T mass, T radius, dfl_sizes sz, T kn, T gamma_n, dfl_friction_law law, T level, T side, T T_solid,
                         const T* grad_max, dfl_contact_history hist, dfl_surface_counters* cnt, int cur, T* acc, T* alpha, void* stream) {
    const auto kernel = sz.radius ? (omega ? surface_contact_kernel<true, true> : surface_contact_kernel<true, false>)
                                  : (omega ? surface_contact_kernel<false, true> : surface_contact_kernel<false, false>);
    // P = 0 still launches one workgroup: the counters of the sub-step are those of no particle
    kernel<<<P > 0 ? ceil_div(P, BLK) : 1, BLK, 0, S(stream)>>>(P, tet, lambda, ien, xg, w, N, vel, omega, mass, radius, sz, kn,
                                                                gamma_n, law, level, side, T_solid, grad_max, hist, cnt, cur, acc, alpha);
    DFL_LAUNCH_CHECK();
}

}  // extern "C"
