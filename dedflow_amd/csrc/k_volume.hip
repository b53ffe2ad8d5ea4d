// Level-set volume correction for gfx950: the global shift of phi that restores the volume of {phi > level} (build-defined;
// model in include/dedflow.h, "level-set volume correction"; the per-tet volume is lf_positive_volume of level_facets.hpp).
//
//   vc_classify_kernel   one thread per tet, as rd_cut_kernel.  A tet whose four phi are > hi = level + max_shift is inside for
//                        every candidate: |det| / 6 into V_in.  A tet with no phi > lo = level - max_shift adds nothing.  Every
//                        other tet is a band tet: its volume at level, lo and hi, and one count.  Five sums (V_in, the three
//                        band volumes, the mesh volume) go through a fixed tree to [workgroup][5]; the band count of the
//                        workgroup is level 1 of the scan that makes the band index the ascending-tet order.
//   vc_emit_kernel       one thread per tet again, four phi only: band index = blk_base[b] + the exclusive scan inside the
//                        workgroup; writes the tet id.  The scan of the workgroup counts is dfl_redistance_scan.
//   vc_eval_kernel       one thread per band tet: gathers the tet through its id and keeps the volume of {phi > c_k} at the
//                        VC_K candidates of one K-section pass in VC_K registers; xor shuffles in the wave, then the four
//                        waves in order, to [workgroup][VC_K].  Plain loads: the band's nodes and ien rows are read once per
//                        pass and stay in the caches from one pass to the next.
//   vc_reduce_kernel     the second fixed-order stage, one workgroup: NV sums over the workgroup partials.
//   vc_shift_kernel      one thread per node: phi += delta as one rounded addition; a NaN is not written.
//   vc_node_sum_kernel   the sum of a nodal array to at most 1024 partials (the captured volume rate), then vc_reduce_kernel.
//
// No float atomics anywhere: every sum has a fixed order, so the result is bitwise reproducible.  The file is compiled
// without fused multiply-add, as level_facets.hpp is wherever it is included.
#include "level_facets.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int VC_BLK = 256;
constexpr int VC_K = DFL_VOLUME_K;
constexpr int VC_CLS = 5;          // sums of the classification pass
constexpr int VC_MAX_PART = 1024;  // partials of a node sum

struct VcCand {
    double c[VC_K];
};

// 2: inside for every candidate in [lo, hi], 1: band, 0: adds nothing (a NaN is not positive)
__device__ __forceinline__ int vc_class(const double* phi, double lo, double hi) {
    if (phi[0] > hi && phi[1] > hi && phi[2] > hi && phi[3] > hi) return 2;
    return (phi[0] > lo || phi[1] > lo || phi[2] > lo || phi[3] > lo) ? 1 : 0;
}

// the volume of {phi > c} inside the tet as the redistancing statistics form it; a NaN adds 0
__device__ __forceinline__ double vc_volume(const double* x, const double* phi, double c, double det) {
    double f[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) f[a] = phi[a] - c;
    const double v = lf_positive_volume(x, f, lf_positive_mask(f), det);
    return v == v ? v : 0.0;
}

__device__ __forceinline__ void vc_load(const int4 n4, const T* __restrict__ xg, const T* __restrict__ phi_g, double* x, double* phi) {
    const long long n[4] = {n4.x, n4.y, n4.z, n4.w};
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        phi[b] = phi_g[n[b]];
#pragma unroll
        for (int d = 0; d < 3; ++d) x[b * 3 + d] = xg[n[b] * 3 + d];
    }
}

// NV sums over the 256 threads of a workgroup in a fixed tree: xor shuffles in the wave, then the four waves in order; valid
// in thread 0
template <int NV>
__device__ __forceinline__ void vc_block_sums(double* v, double (*lds)[NV]) {
#pragma unroll
    for (int j = 0; j < NV; ++j)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[j] = v[j] + __shfl_xor(v[j], off, WAVE);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) lds[wv][j] = v[j];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j)
            for (int i = 1; i < 4; ++i) v[j] = v[j] + lds[i][j];
    }
}

__global__ __launch_bounds__(VC_BLK) void vc_classify_kernel(I NT, const I* __restrict__ ien, const T* __restrict__ xg,
                                                              const T* __restrict__ w, I N, double level, double lo, double hi,
                                                              I* __restrict__ blk_count, T* __restrict__ part) {
    __shared__ double lds[4][VC_CLS];
    __shared__ int s_cnt[4];
    const long long e = (long long)blockIdx.x * VC_BLK + threadIdx.x;
    double v[VC_CLS] = {0.0, 0.0, 0.0, 0.0, 0.0};  // V_in, band at level, band at lo, band at hi, mesh
    int band = 0;
    if (e < NT) {
        const int4 n4 = reinterpret_cast<const int4*>(ien)[e];
        double x[12], phi[4];
        vc_load(n4, xg, w + 4LL * N, x, phi);
        TetCross c;
        tet_cross(x, c);
        const double full = fabs(c.det) / 6.0;
        v[4] = full;
        const int cls = vc_class(phi, lo, hi);
        if (cls == 2) v[0] = full;
        if (cls == 1) {
            band = 1;
            v[1] = vc_volume(x, phi, level, c.det);
            v[2] = vc_volume(x, phi, lo, c.det);
            v[3] = vc_volume(x, phi, hi, c.det);
        }
    }
    int cnt = band;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, WAVE);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = cnt;
    vc_block_sums<VC_CLS>(v, lds);  // (its barrier also publishes s_cnt)
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < VC_CLS; ++j) part[(long long)VC_CLS * blockIdx.x + j] = v[j];
        blk_count[blockIdx.x] = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
    }
}

__global__ __launch_bounds__(VC_BLK) void vc_emit_kernel(I NT, const I* __restrict__ ien, const T* __restrict__ w, I N, double lo,
                                                          double hi, const I* __restrict__ blk_base, I* __restrict__ list, I cap) {
    __shared__ int s_scan[VC_BLK];
    const int t = threadIdx.x;
    const long long e = (long long)blockIdx.x * VC_BLK + t;
    int band = 0;
    if (e < NT) {
        const int4 n4 = reinterpret_cast<const int4*>(ien)[e];
        const T* phi_g = w + 4LL * N;
        const double phi[4] = {phi_g[n4.x], phi_g[n4.y], phi_g[n4.z], phi_g[n4.w]};
        band = vc_class(phi, lo, hi) == 1;
    }
    s_scan[t] = band;
    __syncthreads();
    for (int off = 1; off < VC_BLK; off <<= 1) {  // Hillis-Steele inclusive scan
        const int add = t >= off ? s_scan[t - off] : 0;
        __syncthreads();
        s_scan[t] += add;
        __syncthreads();
    }
    if (!band) return;  // (after the last barrier)
    const long long id = (long long)blk_base[blockIdx.x] + (s_scan[t] - 1);
    if (id < cap) list[id] = (I)e;  // (always: the host sized the list)
}

__global__ __launch_bounds__(VC_BLK) void vc_eval_kernel(I nband, const I* __restrict__ list, const I* __restrict__ ien,
                                                          const T* __restrict__ xg, const T* __restrict__ w, I N,
                                                          const VcCand cand, T* __restrict__ part) {
    __shared__ double lds[4][VC_K];
    const long long i = (long long)blockIdx.x * VC_BLK + threadIdx.x;
    double v[VC_K];
#pragma unroll
    for (int k = 0; k < VC_K; ++k) v[k] = 0.0;
    if (i < nband) {
        double x[12], phi[4];
        vc_load(reinterpret_cast<const int4*>(ien)[list[i]], xg, w + 4LL * N, x, phi);
        TetCross c;
        tet_cross(x, c);
#pragma unroll
        for (int k = 0; k < VC_K; ++k) v[k] = vc_volume(x, phi, cand.c[k], c.det);
    }
    vc_block_sums<VC_K>(v, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < VC_K; ++k) part[(long long)VC_K * blockIdx.x + k] = v[k];
    }
}

// out[j] = sum over i < npart of part[NV i + j], in a fixed order
template <int NV>
__global__ __launch_bounds__(VC_BLK) void vc_reduce_kernel(I npart, const T* __restrict__ part, T* __restrict__ out) {
    __shared__ double lds[4][NV];
    double v[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = 0.0;
    for (long long i = threadIdx.x; i < npart; i += VC_BLK)
#pragma unroll
        for (int j = 0; j < NV; ++j) v[j] = v[j] + part[NV * i + j];
    vc_block_sums<NV>(v, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) out[j] = v[j];
    }
}

__global__ __launch_bounds__(VC_BLK) void vc_shift_kernel(I N, T* __restrict__ phi, double delta) {
    const long long a = (long long)blockIdx.x * VC_BLK + threadIdx.x;
    if (a >= N) return;
    const double old = phi[a];
    if (old == old) phi[a] = old + delta;
}

__global__ __launch_bounds__(VC_BLK) void vc_node_sum_kernel(I N, const T* __restrict__ q, T* __restrict__ part) {
    __shared__ double lds[4][1];
    double v[1] = {0.0};
    const long long stride = (long long)gridDim.x * VC_BLK;
    for (long long a = (long long)blockIdx.x * VC_BLK + threadIdx.x; a < N; a += stride) v[0] = v[0] + q[a];
    vc_block_sums<1>(v, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = v[0];
}

}  // namespace

extern "C" {

void dfl_volume_classify(I NT, const I* ien, const T* xg, const T* w, I N, T level, T lo, T hi, I* blk_count, T* part, T* out5,
                         void* stream) {
    if (NT <= 0) return;
    const int nblk = ceil_div(NT, VC_BLK);
    vc_classify_kernel<<<nblk, VC_BLK, 0, S(stream)>>>(NT, ien, xg, w, N, level, lo, hi, blk_count, part);
    vc_reduce_kernel<VC_CLS><<<1, VC_BLK, 0, S(stream)>>>(nblk, part, out5);
    DFL_LAUNCH_CHECK();
}

void dfl_volume_emit(I NT, const I* ien, const T* w, I N, T lo, T hi, const I* blk_base, I* list, I cap, void* stream) {
    if (NT <= 0) return;
    vc_emit_kernel<<<ceil_div(NT, VC_BLK), VC_BLK, 0, S(stream)>>>(NT, ien, w, N, lo, hi, blk_base, list, cap);
    DFL_LAUNCH_CHECK();
}

void dfl_volume_eval(I nband, const I* list, const I* ien, const T* xg, const T* w, I N, const T* cand, T* part, T* outK,
                     void* stream) {
    if (nband <= 0) return;
    VcCand c;
    for (int k = 0; k < VC_K; ++k) c.c[k] = cand[k];
    const int nblk = ceil_div(nband, VC_BLK);
    vc_eval_kernel<<<nblk, VC_BLK, 0, S(stream)>>>(nband, list, ien, xg, w, N, c, part);
    vc_reduce_kernel<VC_K><<<1, VC_BLK, 0, S(stream)>>>(nblk, part, outK);
    DFL_LAUNCH_CHECK();
}

void dfl_volume_shift(I N, T* w, T delta, void* stream) {
    if (N <= 0) return;
    vc_shift_kernel<<<ceil_div(N, VC_BLK), VC_BLK, 0, S(stream)>>>(N, w + 4LL * N, delta);
    DFL_LAUNCH_CHECK();
}

void dfl_volume_node_sum(I N, const T* q, T* work, T* out1, void* stream) {
    if (N <= 0) return;
    int g = ceil_div(N, VC_BLK * 8);
    if (g > VC_MAX_PART) g = VC_MAX_PART;
    vc_node_sum_kernel<<<g, VC_BLK, 0, S(stream)>>>(N, q, work);
    vc_reduce_kernel<1><<<1, VC_BLK, 0, S(stream)>>>(g, work, out1);
    DFL_LAUNCH_CHECK();
}

}  // extern "C"
