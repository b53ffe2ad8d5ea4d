// Level-set volume correction for gfx950: the global shift of phi that restores the volume of {phi > level} (build-defined;
// model in include/dedflow.h, "level-set volume correction"; the per-tet volume is lf_positive_volume of level_facets.hpp).
//
//   vc_classify_kernel   one thread per tet, as rd_cut_kernel.  A tet whose four phi are > hi = level + max_shift is inside for
//                        every candidate: |det| / 6 into V_in.  A tet with no phi > lo = level - max_shift adds nothing.  Every
//                        other tet is a band tet: its volume at level, lo and hi, and one count.  Five sums (V_in, the three
//                        band volumes, the mesh volume) go through the fixed tree block_tree_256 (block_ops.hpp) to
//                        [workgroup][5]; the band count of the workgroup (block_count_256) is level 1 of the scan that makes
//                        the band index the ascending-tet order.
//   vc_emit_kernel       one thread per tet again, four phi only: band index = blk_base[b] + block_scan_incl_256 inside the
//                        workgroup; writes the tet id.  The host scans the workgroup counts with dfl_scan_counts (k_scan.hip).
//   vc_eval_kernel       one thread per band tet: gathers the tet through its id and keeps the volume of {phi > c_k} at the
//                        VC_K candidates of one K-section pass in VC_K registers; the same tree to [workgroup][VC_K].  Plain
//                        loads: the band's nodes and ien rows are read once per pass and stay in the caches from one pass to
//                        the next.
//   block_reduce_kernel  (block_ops.hpp) the second fixed-order stage, one workgroup: NV sums over the workgroup partials.
//   vc_shift_kernel      one thread per node: phi += delta as one rounded addition; a NaN is not written.
//   vc_node_sum_kernel   the sum of a nodal array to at most 1024 partials (the captured volume rate), then the second stage.
//
// No float atomics anywhere: every sum has a fixed order, so the result is bitwise reproducible.  The file is compiled
// without fused multiply-add, as level_facets.hpp is wherever it is included.
#include "block_ops.hpp"
#include "level_facets.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int VC_BLK = BLOCK_OPS_BLK;
constexpr int VC_K = DFL_VOLUME_K;
constexpr int VC_CLS = 5;          // sums of the classification pass

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
    double f[4];  // (the candidates form their own phi - c)
    lf_gather_tet(n4, xg, x);
    lf_levels(n4, phi_g, 0.0, phi, f);
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
    block_count_256(band, s_cnt);
    block_tree_256<VC_CLS>(v, MergeSum(), lds);  // (its barrier also publishes s_cnt)
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < VC_CLS; ++j) part[(long long)VC_CLS * blockIdx.x + j] = v[j];
        blk_count[blockIdx.x] = block_count_read(s_cnt);
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
    const int incl = block_scan_incl_256(band, s_scan);
    if (!band) return;  // (after the last barrier)
    const long long id = (long long)blk_base[blockIdx.x] + (incl - 1);
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
    block_tree_256<VC_K>(v, MergeSum(), lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < VC_K; ++k) part[(long long)VC_K * blockIdx.x + k] = v[k];
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
    block_tree_256<1>(v, MergeSum(), lds);
    if (threadIdx.x == 0) part[blockIdx.x] = v[0];
}

}  // namespace

extern "C" {

void dfl_volume_classify(I NT, const I* ien, const T* xg, const T* w, I N, T level, T lo, T hi, I* blk_count, T* part, T* out5,
                         void* stream) {
    if (NT <= 0) return;
    const int nblk = ceil_div(NT, VC_BLK);
    vc_classify_kernel<<<nblk, VC_BLK, 0, S(stream)>>>(NT, ien, xg, w, N, level, lo, hi, blk_count, part);
    block_reduce<VC_CLS>(nblk, part, out5, MergeSum(), stream);
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
    block_reduce<VC_K>(nblk, part, outK, MergeSum(), stream);
    DFL_LAUNCH_CHECK();
}

void dfl_volume_shift(I N, T* w, T delta, void* stream) {
    if (N <= 0) return;
    vc_shift_kernel<<<ceil_div(N, VC_BLK), VC_BLK, 0, S(stream)>>>(N, w + 4LL * N, delta);
    DFL_LAUNCH_CHECK();
}

void dfl_volume_node_sum(I N, const T* q, T* work, T* out1, void* stream) {
    if (N <= 0) return;
    const int g = node_reduce_grid(N);
    vc_node_sum_kernel<<<g, VC_BLK, 0, S(stream)>>>(N, q, work);
    block_reduce<1>(g, work, out1, MergeSum(), stream);
    DFL_LAUNCH_CHECK();
}

}  // extern "C"
