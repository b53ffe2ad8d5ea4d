// Track cross-sections for gfx950: the cut of the frozen track by up to 64 parallel planes, per plane the clad and fused
// areas, bead height, penetration depth and the widths (build-defined; model in include/dedflow.h, "track cross-sections").
// Passive: the state w is read and never written.
//
//   ts_pairs_kernel<false>  one thread per tet: gathers xg and phi through ien and forms the 64-bit mask of the stations the tet
//                       pairs with (ts_tet_stations).  One __syncthreads_or: a workgroup that meets no station leaves here,
//                       having written nothing (its counts are the zeros the last scan left).  Otherwise the masks are ORed
//                       over the workgroup (xor shuffles, four words through LDS) and, for the set bits only, one 64-wide
//                       __ballot per wave and the four wave totals through LDS give count[k * nblk + workgroup].  The host
//                       scans the station-major counts with dfl_scan_counts (k_scan.hip).
//   ts_pairs_kernel<true>   the same decisions from the same function; the tet id goes to list[base[k * nblk + workgroup] + rank],
//                       rank = popcount of the lower lanes of the same ballot + the totals of the lower waves: ascending tet
//                       id inside every station by construction, whatever the arrival order.
//   ts_offsets_kernel   off[k] = base[k * nblk], the 65 segment offsets (the total from num_station on)
//   ts_eval_kernel      grid (chunks of 256 pairs, station), one thread per pair: the facets of lf_tet_facets_ijt with
//                       f := sigma, (y, h, f, g) carried to the vertices, three Sutherland-Hodgman clips per polygon kept in
//                       registers (every index static after unrolling: a vertex is put at the running count by a select
//                       chain), 9 components through block_tree_256 with MergeTrack to [station][chunk][9]
//   ts_reduce_kernel    one workgroup per station: block_reduce_kernel's loop and tree over the station's chunks
//
// No atomics, on floats or on integers; every sum has a fixed order.  The file is compiled without fused multiply-add, as
// level_facets.hpp is wherever it is included.
#include "block_ops.hpp"
#include "level_facets.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int TS_BLK = BLOCK_OPS_BLK;
constexpr int TS_NV = DFL_TRACK_NSTAT;
constexpr int TS_MAXS = DFL_TRACK_MAX_STATION;
enum { TS_Y = 0, TS_H = 1, TS_F = 2, TS_G = 3, TS_NQ = 4 };

// (x - o) . d with x - o formed first
__device__ __forceinline__ double ts_along(const double* x, const double* o, const double* d) {
    const double r[3] = {x[0] - o[0], x[1] - o[1], x[2] - o[2]};
    return lf_dot(r, d);
}
// f_a = side (phi_a - level): the difference of lf_levels, negated for side = -1
__device__ __forceinline__ void ts_metal(const int4 n4, const T* __restrict__ phi_g, const dfl_track_params& p, double* f) {
    double phi[4];
    lf_levels(n4, phi_g, p.level, phi, f);
    if (p.side < 0.0) {
#pragma unroll
        for (int a = 0; a < 4; ++a) f[a] = -f[a];
    }
}

// bit k set: tet e and station k form a pair.  The mask of sigma_a = s_a - c_k > 0 is that of s_a > c_k (the sign of an IEEE
// difference is exact), so it is neither 0 nor 15 exactly when the largest s_a is > c_k and not every s_a is: two
// comparisons per station with hi = the largest s_a that is no NaN and lo = the smallest, -inf as soon as one is a NaN
__device__ __forceinline__ unsigned long long ts_tet_stations(long long e, I NT, const I* __restrict__ ien, const T* __restrict__ xg,
                                                              const T* __restrict__ phi_g, const dfl_track_params& p) {
    if (e >= NT) return 0ull;
    const int4 n4 = reinterpret_cast<const int4*>(ien)[e];
    double x[12], f[4];
    lf_gather_tet(n4, xg, x);
    ts_metal(n4, phi_g, p, f);
    if (lf_positive_mask(f) == 0) return 0ull;
    double hi = -HUGE_VAL, lo = HUGE_VAL;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const double s = ts_along(x + 3 * a, p.o, p.n);
        if (s > hi) hi = s;
        lo = s == s ? (s < lo ? s : lo) : -HUGE_VAL;
    }
    unsigned long long m = 0ull;
    for (int k = 0; k < p.num_station; ++k) {
        const double c = p.c[k];
        if (hi > c && !(lo > c)) m |= 1ull << k;
    }
    return m;
}

template <bool EMIT>
__global__ __launch_bounds__(TS_BLK) void ts_pairs_kernel(I NT, const I* __restrict__ ien, const T* __restrict__ xg,
                                                           const T* __restrict__ w, I N, const dfl_track_params p, I nblk,
                                                           const I* __restrict__ base, I* __restrict__ count,
                                                           I* __restrict__ list, I cap) {
    __shared__ unsigned long long s_or[4];
    __shared__ int s_cnt[TS_MAXS][4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long e = (long long)blockIdx.x * TS_BLK + threadIdx.x;
    const unsigned long long m = ts_tet_stations(e, NT, ien, xg, w + 4LL * N, p);
    if (!__syncthreads_or(m != 0ull)) return;  // most workgroups: no station cuts a metal tet of theirs
    unsigned long long wm = m;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) wm |= __shfl_xor(wm, off, WAVE);
    if (lane == 0) s_or[wv] = wm;
    __syncthreads();
    const unsigned long long any = (s_or[0] | s_or[1]) | (s_or[2] | s_or[3]);
    // (uniform by value; through readfirstlane the loops below are scalar)
    const unsigned long long all = (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(any >> 32)) << 32 |
                                   (unsigned)__builtin_amdgcn_readfirstlane((int)any);
    for (unsigned long long rest = all; rest; rest &= rest - 1) {
        const int k = __ffsll((long long)rest) - 1;
        const unsigned long long b = __ballot((m >> k) & 1ull);
        if (lane == 0) s_cnt[k][wv] = __popcll(b);
    }
    __syncthreads();
    if (!EMIT) {
        const int k = threadIdx.x;
        if (k < p.num_station && ((all >> k) & 1ull))
            count[(long long)k * nblk + blockIdx.x] = (s_cnt[k][0] + s_cnt[k][1]) + (s_cnt[k][2] + s_cnt[k][3]);
        return;
    }
    const unsigned long long below = lane == 0 ? 0ull : ~0ull >> (64 - lane);
    for (unsigned long long rest = all; rest; rest &= rest - 1) {
        const int k = __ffsll((long long)rest) - 1;
        const unsigned long long b = __ballot((m >> k) & 1ull);
        if (!((m >> k) & 1ull)) continue;
        int rank = __popcll(b & below);
        for (int v = 0; v < wv; ++v) rank += s_cnt[k][v];
        const long long id = (long long)base[(long long)k * nblk + blockIdx.x] + rank;
        if (id < cap) list[id] = (I)e;  // (always: the host sized the list)
    }
}

__global__ void ts_offsets_kernel(int ns, I nblk, const I* __restrict__ base, I* __restrict__ off) {
    const int k = threadIdx.x;
    if (k <= TS_MAXS) off[k] = base[(long long)(k < ns ? k : ns) * nblk];
}

// ---- the cut of one pair ----------------------------------------------------------------------------------------------------

struct TsPositive {
    __device__ __forceinline__ bool operator()(double q) const { return q > 0.0; }
};
struct TsNotPositive {
    __device__ __forceinline__ bool operator()(double q) const { return !(q > 0.0); }
};
struct TsNotNegative {
    __device__ __forceinline__ bool operator()(double q) const { return q >= 0.0; }
};

// vertex v into slot n of out (a select chain: n is data, the arrays stay in registers); a vertex beyond the NO slots is
// dropped.  Returns the new count
template <int NO>
__device__ __forceinline__ int ts_put(double (&out)[TS_NQ][NO], int n, const double* v) {
#pragma unroll
    for (int k = 0; k < NO; ++k)
#pragma unroll
        for (int c = 0; c < TS_NQ; ++c) out[c][k] = k == n ? v[c] : out[c][k];  // (a select per slot, never a store at n)
    return n < NO ? n + 1 : n;
}

// Sutherland-Hodgman against inside(q[COMP]): walking the edges U -> V of in[.][0 .. nin) in order, U goes out when it is
// inside, then the crossing when exactly one of U, V is: A + tau (B - A) from the inside vertex A towards the outside B,
// tau = q_A / (q_A - q_B), for all four carried quantities
template <int COMP, int NI, class Inside>
__device__ __forceinline__ int ts_clip(const double (&in)[TS_NQ][NI], int nin, Inside inside, double (&out)[TS_NQ][NI + 1]) {
#pragma unroll
    for (int c = 0; c < TS_NQ; ++c)
#pragma unroll
        for (int k = 0; k < NI + 1; ++k) out[c][k] = 0.0;
    int n = 0;
#pragma unroll
    for (int e = 0; e < NI; ++e) {
        if (e < nin) {
            double U[TS_NQ], V[TS_NQ];
#pragma unroll
            for (int c = 0; c < TS_NQ; ++c) {
                U[c] = in[c][e];
                V[c] = (e + 1 < NI && e + 1 < nin) ? in[c][e + 1 < NI ? e + 1 : 0] : in[c][0];
            }
            const bool iu = inside(U[COMP]), iv = inside(V[COMP]);
            if (iu) n = ts_put<NI + 1>(out, n, U);
            if (iu != iv) {
                double X[TS_NQ];
                const double qa = iu ? U[COMP] : V[COMP], qb = iu ? V[COMP] : U[COMP];
                const double tau = qa / (qa - qb);
#pragma unroll
                for (int c = 0; c < TS_NQ; ++c) {
                    const double A = iu ? U[c] : V[c], B = iu ? V[c] : U[c];
                    X[c] = A + tau * (B - A);
                }
                n = ts_put<NI + 1>(out, n, X);
            }
        }
    }
    return n;
}

// the shoelace fan from vertex 0, an absolute value per fan triangle, summed from +0.0 in fan order; a NaN sum counts 0
template <int NP>
__device__ __forceinline__ double ts_area(const double (&P)[TS_NQ][NP], int n) {
    double area = 0.0;
#pragma unroll
    for (int k = 1; k + 1 < NP; ++k)
        if (k + 1 < n) {
            const double ay = P[TS_Y][k] - P[TS_Y][0], ah = P[TS_H][k] - P[TS_H][0];
            const double by = P[TS_Y][k + 1] - P[TS_Y][0], bh = P[TS_H][k + 1] - P[TS_H][0];
            area = area + 0.5 * fabs(ay * bh - by * ah);
        }
    return area == area ? area : 0.0;
}

// a NaN never wins
__device__ __forceinline__ void ts_max(double& cur, double v) { if (v > cur) cur = v; }
__device__ __forceinline__ void ts_min(double& cur, double v) { if (v < cur) cur = v; }

// components: 0 area_clad, 1 area_fused, 2 area_scale (sums); 3 height, 4 depth (max); 5 y_lo_clad (min), 6 y_hi_clad (max),
// 7 y_lo_fused (min), 8 y_hi_fused (max)
struct MergeTrack {
    __device__ __forceinline__ static bool is_sum(int j) { return j < 3; }
    __device__ __forceinline__ static bool is_min(int j) { return j == 5 || j == 7; }
    __device__ __forceinline__ double operator()(int j, double a, double b) const {
        return is_sum(j) ? a + b : is_min(j) ? (b < a ? b : a) : (b > a ? b : a);
    }
    __device__ __forceinline__ double identity(int j) const { return is_sum(j) ? 0.0 : is_min(j) ? HUGE_VAL : -HUGE_VAL; }
};

__global__ __launch_bounds__(TS_BLK) void ts_eval_kernel(const I* __restrict__ off, const I* __restrict__ list,
                                                          const I* __restrict__ ien, const T* __restrict__ xg,
                                                          const T* __restrict__ w, I N, const T* __restrict__ T_peak,
                                                          const dfl_track_params p, I stride, T* __restrict__ part) {
    __shared__ double lds[4][TS_NV];
    const int k = blockIdx.y;
    const long long seg0 = off[k], seg = off[k + 1] - seg0;
    if ((long long)blockIdx.x * TS_BLK >= seg) return;  // (the whole workgroup: the second stage reads ceil(seg / 256) records)
    const long long i = (long long)blockIdx.x * TS_BLK + threadIdx.x;
    const MergeTrack merge;
    double v[TS_NV];
#pragma unroll
    for (int j = 0; j < TS_NV; ++j) v[j] = merge.identity(j);
    if (i < seg) {
        const int4 n4 = reinterpret_cast<const int4*>(ien)[list[seg0 + i]];
        const long long nd[4] = {n4.x, n4.y, n4.z, n4.w};
        double x[12], q[TS_NQ][4], sigma[4];
        lf_gather_tet(n4, xg, x);
        ts_metal(n4, w + 4LL * N, p, q[TS_F]);
        const double c = p.c[k];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            sigma[a] = ts_along(x + 3 * a, p.o, p.n) - c;
            q[TS_Y][a] = ts_along(x + 3 * a, p.o, p.t);
            q[TS_H][a] = ts_along(x + 3 * a, p.o, p.u);
            q[TS_G][a] = T_peak ? T_peak[nd[a]] - p.T_fuse : -HUGE_VAL;
        }
        double P3[18], tt[6];
        int ij[2] = {0, 0};
        const int nf = lf_tet_facets_ijt(x, sigma, lf_positive_mask(sigma), P3, ij, tt);  // (the points themselves are not used)
#pragma unroll
        for (int kf = 0; kf < 2; ++kf) {
            if (kf < nf) {
                double tri[TS_NQ][3];
#pragma unroll
                for (int vtx = 0; vtx < 3; ++vtx) {
                    const int a = (ij[kf] >> (4 * vtx)) & 3, b = (ij[kf] >> (4 * vtx + 2)) & 3;
                    const double t = tt[3 * kf + vtx];
#pragma unroll
                    for (int cq = 0; cq < TS_NQ; ++cq) {
                        const double qa = lf_pick1(q[cq], a);
                        tri[cq][vtx] = qa + t * (lf_pick1(q[cq], b) - qa);
                    }
                }
                v[2] = v[2] + ts_area<3>(tri, 3);
                double metal[TS_NQ][4];
                const int nm = ts_clip<TS_F, 3>(tri, 3, TsPositive(), metal);
                {
                    double clad[TS_NQ][5];
                    const int nc = ts_clip<TS_H, 4>(metal, nm, TsPositive(), clad);
                    if (nc >= 3) {
                        v[0] = v[0] + ts_area<5>(clad, nc);
#pragma unroll
                        for (int s = 0; s < 5; ++s)
                            if (s < nc) {
                                ts_max(v[3], clad[TS_H][s]);
                                ts_min(v[5], clad[TS_Y][s]);
                                ts_max(v[6], clad[TS_Y][s]);
                            }
                    }
                }
                {
                    double under[TS_NQ][5], fused[TS_NQ][6];
                    const int nu = ts_clip<TS_H, 4>(metal, nm, TsNotPositive(), under);
                    const int nz = ts_clip<TS_G, 5>(under, nu, TsNotNegative(), fused);
                    if (nz >= 3) {
                        v[1] = v[1] + ts_area<6>(fused, nz);
#pragma unroll
                        for (int s = 0; s < 6; ++s)
                            if (s < nz) {
                                ts_max(v[4], -fused[TS_H][s]);
                                ts_min(v[7], fused[TS_Y][s]);
                                ts_max(v[8], fused[TS_Y][s]);
                            }
                    }
                }
            }
        }
    }
    block_tree_256<TS_NV>(v, merge, lds);
    if (threadIdx.x == 0) {
        T* dst = part + ((long long)k * stride + blockIdx.x) * TS_NV;
#pragma unroll
        for (int j = 0; j < TS_NV; ++j) dst[j] = v[j];
    }
}

// the second stage of station blockIdx.x: block_reduce_kernel's loop and tree over the station's ceil(seg / 256) records
__global__ __launch_bounds__(TS_BLK) void ts_reduce_kernel(const I* __restrict__ off, I stride, const T* __restrict__ part,
                                                            T* __restrict__ out) {
    __shared__ double lds[4][TS_NV];
    const int k = blockIdx.x;
    const long long seg = off[k + 1] - off[k], npart = (seg + TS_BLK - 1) / TS_BLK;
    const T* src = part + (long long)k * stride * TS_NV;
    const MergeTrack merge;
    double v[TS_NV];
#pragma unroll
    for (int j = 0; j < TS_NV; ++j) v[j] = merge.identity(j);
    for (long long i = threadIdx.x; i < npart && i < stride; i += TS_BLK)
#pragma unroll
        for (int j = 0; j < TS_NV; ++j) v[j] = merge(j, v[j], src[TS_NV * i + j]);
    block_tree_256<TS_NV>(v, merge, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < TS_NV; ++j) out[(long long)k * TS_NV + j] = v[j];
    }
}

}  // namespace

extern "C" {

void dfl_track_count(I NT, const I* ien, const T* xg, const T* w, I N, const dfl_track_params* prm, I nblk, I* count,
                     void* stream) {
    if (NT <= 0) return;
    ts_pairs_kernel<false><<<ceil_div(NT, TS_BLK), TS_BLK, 0, S(stream)>>>(NT, ien, xg, w, N, *prm, nblk, nullptr, count, nullptr, 0);
    DFL_LAUNCH_CHECK();
}

void dfl_track_offsets(I num_station, I nblk, const I* base, I* off65, void* stream) {
    ts_offsets_kernel<<<1, 128, 0, S(stream)>>>(num_station, nblk, base, off65);
    DFL_LAUNCH_CHECK();
}

void dfl_track_emit(I NT, const I* ien, const T* xg, const T* w, I N, const dfl_track_params* prm, I nblk, const I* base, I* list,
                    I cap, void* stream) {
    if (NT <= 0) return;
    ts_pairs_kernel<true><<<ceil_div(NT, TS_BLK), TS_BLK, 0, S(stream)>>>(NT, ien, xg, w, N, *prm, nblk, base, nullptr, list, cap);
    DFL_LAUNCH_CHECK();
}

void dfl_track_eval(I max_chunk, const I* off65, const I* list, const I* ien, const T* xg, const T* w, I N, const T* T_peak,
                    const dfl_track_params* prm, T* part, T* out, void* stream) {
    const int ns = prm->num_station;
    if (ns <= 0) return;
    if (max_chunk > 0) {
        ts_eval_kernel<<<dim3(max_chunk, ns), TS_BLK, 0, S(stream)>>>(off65, list, ien, xg, w, N, T_peak, *prm, max_chunk, part);
    }
    ts_reduce_kernel<<<ns, TS_BLK, 0, S(stream)>>>(off65, max_chunk, part, out);
    DFL_LAUNCH_CHECK();
}

}  // extern "C"
