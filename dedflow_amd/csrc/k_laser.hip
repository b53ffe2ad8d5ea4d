// Laser energy deposition for gfx950: powder shadowing per beam column, in-flight heating, the substrate flux.
// BUILD-DEFINED and opt-in (the reference has no source in its T equation); the model is stated in include/dedflow.h,
// "laser energy deposition".
//
// One laser step is a handful of small dependent launches on the library stream; it allocates nothing and waits for nothing:
//   hit      (substrate only) one thread per candidate face: the columns under the face's projected bounding box, the
//            column centre against the projected triangle, 64-bit atomicMin of (depth on a 2^-40 grid << 24 | face).
//            Integer atomics: the winner does not depend on the order of arrival
//   bin      one thread per particle: the column holding the projection of its centre.  A particle outside the grid gets
//            rate 0 here and one of the extra bins behind the columns, n^2 + id / 8: a single extra bin, as the wall sweep
//            has, would hold most of the cloud under a narrow beam, and both the bin pass's counter and the per-bin
//            ordering of the cell sort are built for a handful of members (100k particles, 94% outside: the records
//            labelled single_outside_bin in profiles/laser_M55.jsonl, 1.1 ms of serialised atomics in the bin pass and
//            5 ms in dem_sort_cells_kernel).  The extra bins add P / 8 entries to the sort's scan.  Then the cell sort of the contact sweep
//            (dfl_dem_sort_binned) on the laser's own scratch leaves the column runs in (column, id) order with sorted
//            copies of position and radius
//   column   THE HOT KERNEL: one wavefront per column, four columns per 256-thread workgroup.  The run (s, id, A/a) goes
//            into LDS (20 B per entry, 512 entries per wave, 40 KB per workgroup), is sorted by (s, id) with a bitonic
//            network (each compare-exchange touches two entries of one lane: no bank conflict beyond the 2-way of a
//            64-bit access), then scanned 64 entries at a time: a Hillis-Steele scan over the lanes (__shfl_up, fixed
//            tree) plus the carry of the chunks before.  exp / expm1 per particle, laser_rate written by id, the column's
//            transmitted power, hit face and six tally partials by lane 0.  A run longer than the LDS cap takes the
//            fallback: every entry counts the entries before it (tiles of the run staged in LDS), writes (A/a, id) at its
//            rank into global scratch, and the same chunked scan reads that: O(len^2) compares, same summation order, so
//            the result does not depend on which path ran.  No floating-point atomics; every output is written once; the
//            order of every sum is fixed by (s, id) => bitwise reproducible, and invariant under a permutation of the
//            ids wherever depths are distinct.
//   deposit  one thread per substrate node over its faces (ascending) and the columns under each (ascending): the columns
//            the face won give eta_s T_c times the node's barycentric weight; written, not accumulated by atomics
//   tally    one workgroup: fixed-tree reduction of the per-column partials into six doubles on the device
// The projection arithmetic is written without fused multiply-add, so that a float64 model bins alike.
#include "laser_geom.hpp"
#include <climits>

#pragma clang fp contract(off)

namespace {

constexpr int BLK = 256;
constexpr int CAP = 512;         // entries of one column run sorted in LDS
constexpr int FACE_BITS = 24;    // low bits of a hit key: the candidate face; the depth grid has 40 bits
constexpr unsigned long long NO_HIT = ~0ull;

// the lanes of ONE wave exchange data through LDS / their own global scratch: order the accesses, no s_barrier
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__global__ __launch_bounds__(BLK) void laser_bin_kernel(I P, const T* __restrict__ coord, dfl_laser_beam b, I* __restrict__ cell_of,
                                                       I* __restrict__ rank, I* __restrict__ count, T* __restrict__ rate) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i >= P) return;
    const double dx = coord[3 * i] - b.o[0], dy = coord[3 * i + 1] - b.o[1], dz = coord[3 * i + 2] - b.o[2];
    const double qu = floor(dot3(b.e1, dx, dy, dz) / b.h), qv = floor(dot3(b.e2, dx, dy, dz) / b.h);
    const double half = (double)(b.n / 2);
    int c = b.n * b.n + (i >> DFL_LASER_OUTSIDE_SHIFT);  // outside the grid: unlit, an extra bin behind the columns
    if (qu >= -half && qu < half && qv >= -half && qv < half) c = ((int)qu + b.n / 2) + b.n * ((int)qv + b.n / 2);
    else rate[i] = 0.0;
    cell_of[i] = c;
    rank[i] = atomicAdd(&count[c], 1);
}

__global__ __launch_bounds__(BLK) void laser_hit_kernel(I nf, const dfl_wall_tri* __restrict__ tri, dfl_laser_beam b, T s_lo, T scale,
                                                       unsigned long long* __restrict__ colkey) {
    const int f = blockIdx.x * BLK + threadIdx.x;
    if (f >= nf) return;
    Proj p;
    project(tri + f, b, p);
    int i0, i1, j0, j1;
    column_range(p, b, i0, i1, j0, j1);
    for (int j = j0; j <= j1; ++j)
        for (int i = i0; i <= i1; ++i) {  // 0 <= i, j < n by column_range
            double w[3], s;
            if (!tri_hit(p, column_centre(i, b), column_centre(j, b), w, s)) continue;
            const double q = fmin(fmax((s - s_lo) * scale, 0.0), 1099511627775.0);  // 2^40 - 1
            atomicMin(&colkey[i + b.n * j], ((unsigned long long)q << FACE_BITS) | (unsigned long long)f);
        }
}

__device__ __forceinline__ bool before(double sa, int ia, double sb, int ib) { return sa < sb || (sa == sb && ia < ib); }

template <bool POLY>
__global__ __launch_bounds__(BLK) void laser_column_kernel(I P, dfl_laser_beam b, T power4, T eta_p, T eta_s, const T* __restrict__ gw,
                                                          const I* __restrict__ cell_start, const I* __restrict__ order,
                                                          const T* __restrict__ sorted, const T* __restrict__ sorted_r, T radius,
                                                          const dfl_wall_tri* __restrict__ tri,
                                                          const unsigned long long* __restrict__ colkey, T* __restrict__ k_tau,
                                                          I* __restrict__ k_id, T* __restrict__ rate, T* __restrict__ col_T,
                                                          I* __restrict__ col_face, T* __restrict__ part) {
    __shared__ double s_s[BLK / WAVE][CAP];
    __shared__ double s_tau[BLK / WAVE][CAP];
    __shared__ int s_id[BLK / WAVE][CAP];
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    const int ncol = b.n * b.n;
    const int c = blockIdx.x * (BLK / WAVE) + wv;
    if (c >= ncol) return;  // a whole wave leaves: the kernel has no workgroup barrier
    const int ci = c % b.n, cj = c / b.n;
    const double pc = (power4 * gw[ci]) * gw[b.n + cj];
    // the substrate hit of this column's centre ray (every lane computes the same)
    const unsigned long long key = colkey[c];
    const bool has_hit = key != NO_HIT && tri != nullptr;  // (the host clears the keys with the face list; never read through NULL)
    double s_hit = 0.0;
    int face = -1;
    if (has_hit) {
        const dfl_wall_tri* t = tri + (int)(key & ((1ull << FACE_BITS) - 1));
        Proj p;
        project(t, b, p);
        double w[3];
        tri_hit(p, column_centre(ci, b), column_centre(cj, b), w, s_hit);
        face = t->id;
    }
    const int lo = P > 0 ? cell_start[c] : 0;
    const int len = P > 0 ? cell_start[c + 1] - lo : 0;
    const double inv_a = 1.0 / b.area;
    double* ss = s_s[wv];
    double* st = s_tau[wv];
    int* si = s_id[wv];
    const bool long_run = len > CAP;
    // depth and optical depth A/a of run entry k; a particle deeper than the hit is unlit: it intercepts nothing
    auto load = [&](int k, double& s, double& tau) {
        const T* x = sorted + 6LL * (lo + k);
        s = dot3(b.dir, x[0] - b.o[0], x[1] - b.o[1], x[2] - b.o[2]);
        const double r = POLY ? sorted_r[lo + k] : radius;
        tau = (has_hit && s > s_hit) ? 0.0 : (M_PI * (r * r)) * inv_a;
    };
    if (!long_run) {
        int m = 2;
        while (m < len) m <<= 1;
        for (int k = lane; k < m; k += WAVE) {
            double s = HUGE_VAL, tau = 0.0;
            int id = INT_MAX;
            if (k < len) {
                load(k, s, tau);
                id = order[lo + k];
            }
            ss[k] = s; st[k] = tau; si[k] = id;
        }
        wave_sync();
        if (len > 1)
            for (int size = 2; size <= m; size <<= 1)
                for (int j = size >> 1; j > 0; j >>= 1) {
                    for (int t = lane; t < m / 2; t += WAVE) {
                        const int i0 = ((t & ~(j - 1)) << 1) | (t & (j - 1)), i1 = i0 | j;
                        const double sa = ss[i0], sb = ss[i1];
                        const int ia = si[i0], ib = si[i1];
                        const bool up = (i0 & size) == 0;
                        if (up ? before(sb, ib, sa, ia) : before(sa, ia, sb, ib)) {
                            const double ta = st[i0], tb = st[i1];
                            ss[i0] = sb; ss[i1] = sa; si[i0] = ib; si[i1] = ia; st[i0] = tb; st[i1] = ta;
                        }
                    }
                    wave_sync();
                }
    } else {
        // fallback: the rank of every entry by counting, over tiles of the run staged in LDS; (tau, id) to global scratch
        for (int kb = 0; kb < len; kb += WAVE) {
            const int k = kb + lane;
            double s = HUGE_VAL, tau = 0.0;
            int id = INT_MAX, r = 0;
            if (k < len) {
                load(k, s, tau);
                id = order[lo + k];
            }
            for (int tb = 0; tb < len; tb += CAP) {
                const int tl = min(CAP, len - tb);
                wave_sync();  // the previous tile has been read
                for (int q = lane; q < tl; q += WAVE) {
                    double s2, t2;
                    load(tb + q, s2, t2);
                    ss[q] = s2;
                    si[q] = order[lo + tb + q];
                }
                wave_sync();
                for (int q = 0; q < tl; ++q) r += before(ss[q], si[q], s, id) ? 1 : 0;
            }
            if (k < len) {  // ranks are a permutation of [0, len): (s, id) are distinct
                k_tau[lo + r] = tau;
                k_id[lo + r] = id;
            }
        }
        wave_sync();
    }
    // exclusive prefix of the optical depth in (s, id) order, 64 entries at a time
    double carry = 0.0, absorbed = 0.0, scattered = 0.0;
    for (int kb = 0; kb < len; kb += WAVE) {
        const int k = kb + lane;
        double tau = 0.0;
        int id = -1;
        if (k < len) {
            tau = long_run ? k_tau[lo + k] : st[k];
            id = long_run ? k_id[lo + k] : si[k];
        }
        double v = tau;
#pragma unroll
        for (int off = 1; off < WAVE; off <<= 1) {
            const double t = __shfl_up(v, off, WAVE);
            if (lane >= off) v += t;
        }
        const double ex = __shfl_up(v, 1, WAVE);
        const double prefix = carry + (lane == 0 ? 0.0 : ex);
        carry = carry + __shfl(v, WAVE - 1, WAVE);
        // non-finite coordinates are not supported: a NaN depth compares false both ways, so the order and, in the fallback,
        // the ranks of its column are meaningless.  The guard only keeps every write inside the arrays
        if (k < len && (unsigned)id < (unsigned)P) {
            const double p_in = pc * exp(-prefix);
            const double got = p_in * (0.0 - expm1(-tau));  // (0 - x, not -x: an unlit particle, tau = 0, gets +0.0 and not -0.0)
            const double mine = eta_p * got;
            rate[id] = mine;
            absorbed += mine;
            scattered += got - mine;
        }
    }
    absorbed = wave_sum(absorbed);
    scattered = wave_sum(scattered);
    if (lane == 0) {
        const double tc = pc * exp(-carry);
        const double sub = has_hit ? eta_s * tc : 0.0;
        col_T[c] = tc;
        col_face[c] = face;
        part[c] = pc;
        part[ncol + c] = absorbed;
        part[2 * ncol + c] = scattered;
        part[3 * ncol + c] = sub;
        part[4 * ncol + c] = has_hit ? (1.0 - eta_s) * tc : 0.0;
        part[5 * ncol + c] = has_hit ? 0.0 : tc;
    }
}

__global__ __launch_bounds__(BLK) void laser_deposit_kernel(I ns, const I* __restrict__ soff, const I* __restrict__ sface,
                                                           const dfl_wall_tri* __restrict__ tri, dfl_laser_beam b, T eta_s, T dt,
                                                           const unsigned long long* __restrict__ colkey,
                                                           const T* __restrict__ col_T, T* __restrict__ power,
                                                           T* __restrict__ energy) {
    const int a = blockIdx.x * BLK + threadIdx.x;
    if (a >= ns) return;
    double acc = 0.0;
    for (int e = soff[a]; e < soff[a + 1]; ++e) {  // ascending face
        const int f = sface[e] >> 2, kv = sface[e] & 3;
        Proj p;
        project(tri + f, b, p);
        int i0, i1, j0, j1;
        column_range(p, b, i0, i1, j0, j1);
        for (int j = j0; j <= j1; ++j)
            for (int i = i0; i <= i1; ++i) {  // ascending column
                const unsigned long long key = colkey[i + b.n * j];
                if (key == NO_HIT || (int)(key & ((1ull << FACE_BITS) - 1)) != f) continue;
                double w[3], s;
                if (!tri_hit(p, column_centre(i, b), column_centre(j, b), w, s)) continue;
                acc += (eta_s * col_T[i + b.n * j]) * w[kv];
            }
    }
    power[a] = acc;
    energy[a] += dt * acc;  // this thread owns the node
}

// out[0..6) = outside, absorbed_particles, scattered, substrate, reflected, missed; thread t sums columns t, t + 256, ...
__global__ __launch_bounds__(BLK) void laser_tally_kernel(I ncol, T power, const T* __restrict__ part, T* __restrict__ out) {
    __shared__ double s_part[6][BLK];
    const int t = threadIdx.x;
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int c = t; c < ncol; c += BLK)
#pragma unroll
        for (int q = 0; q < 6; ++q) acc[q] += part[(long long)q * ncol + c];
#pragma unroll
    for (int q = 0; q < 6; ++q) s_part[q][t] = acc[q];
    __syncthreads();
    for (int off = BLK / 2; off > 0; off >>= 1) {
        if (t < off)
#pragma unroll
            for (int q = 0; q < 6; ++q) s_part[q][t] += s_part[q][t + off];
        __syncthreads();
    }
    if (t == 0) {
        out[0] = power - s_part[0][0];
        for (int q = 1; q < 6; ++q) out[q] = s_part[q][0];
    }
}

__global__ __launch_bounds__(BLK) void laser_source_add_kernel(I ns, const I* __restrict__ snode, T inv_time, T* __restrict__ energy,
                                                              T* __restrict__ q) {
    const int a = blockIdx.x * BLK + threadIdx.x;
    if (a >= ns) return;
    q[snode[a]] += energy[a] * inv_time;  // the substrate nodes are distinct
    energy[a] = 0.0;
}

}  // namespace

extern "C" {

I dfl_laser_column_cap(void) { return CAP; }

void dfl_laser_bin(I P, const T* coord, dfl_laser_beam b, I* cell_of, I* rank, I* count, T* rate, void* stream) {
    if (P <= 0) return;
    laser_bin_kernel<<<ceil_div(P, BLK), BLK, 0, S(stream)>>>(P, coord, b, cell_of, rank, count, rate);
    DFL_LAUNCH_CHECK();
}

void dfl_laser_hit(I nf, const dfl_wall_tri* tri, dfl_laser_beam b, T s_lo, T scale, uint64_t* colkey, void* stream) {
    DFL_GUARD(hipMemsetAsync(colkey, 0xff, (size_t)b.n * b.n * sizeof(uint64_t), S(stream)));
    if (nf <= 0) return;
    laser_hit_kernel<<<ceil_div(nf, BLK), BLK, 0, S(stream)>>>(nf, tri, b, s_lo, scale, (unsigned long long*)colkey);
    DFL_LAUNCH_CHECK();
}

void dfl_laser_columns(I P, dfl_laser_beam b, T power, T eta_p, T eta_s, const T* gw, const I* cell_start, const I* order,
                       const T* sorted, const T* sorted_r, T radius, const dfl_wall_tri* tri, const uint64_t* colkey, T* k_tau,
                       I* k_id, T* rate, T* col_T, I* col_face, T* part, void* stream) {
    const int ncol = b.n * b.n;
    const auto kernel = sorted_r ? laser_column_kernel<true> : laser_column_kernel<false>;
    kernel<<<ceil_div(ncol, BLK / WAVE), BLK, 0, S(stream)>>>(P, b, power / 4.0, eta_p, eta_s, gw, cell_start, order, sorted, sorted_r,
                                                             radius, tri, (const unsigned long long*)colkey, k_tau, k_id, rate,
                                                             col_T, col_face, part);
    DFL_LAUNCH_CHECK();
}

void dfl_laser_deposit(I ns, const I* soff, const I* sface, const dfl_wall_tri* tri, dfl_laser_beam b, T eta_s, T dt,
                       const uint64_t* colkey, const T* col_T, T* power, T* energy, void* stream) {
    if (ns <= 0) return;
    laser_deposit_kernel<<<ceil_div(ns, BLK), BLK, 0, S(stream)>>>(ns, soff, sface, tri, b, eta_s, dt,
                                                                 (const unsigned long long*)colkey, col_T, power, energy);
    DFL_LAUNCH_CHECK();
}

void dfl_laser_tally(I ncol, T power, const T* part, T* tally, void* stream) {
    laser_tally_kernel<<<1, BLK, 0, S(stream)>>>(ncol, power, part, tally);
    DFL_LAUNCH_CHECK();
}

void dfl_laser_source_add(I ns, const I* snode, T inv_time, T* energy, T* q, void* stream) {
    if (ns <= 0) return;
    laser_source_add_kernel<<<ceil_div(ns, BLK), BLK, 0, S(stream)>>>(ns, snode, inv_time, energy, q);
    DFL_LAUNCH_CHECK();
}

}  // extern "C"
