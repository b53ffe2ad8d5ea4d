// Workgroup-wide integer counts and scans and fixed-order reductions for 256-thread workgroups: the one copy of every idiom
// the "count per workgroup -> scan (k_scan.hip) -> emit in ascending order" passes and the two-stage statistics share
// (k_redistance.hip, k_volume.hip, k_laser_surface.hip, k_phase.hip, k_solidify.hip, k_scan.hip).  Results that must stay bitwise
// reproducible depend on the association written here:
//   block_tree_256    ((w0 o w1) o w2) o w3 after the xor shuffles inside every wave
//   block_sum_256     of dfl_common.hpp is another tree, (w0 + w1) + (w2 + w3): the Krylov kernels keep it
#pragma once
#include "dfl_common.hpp"

constexpr int BLOCK_OPS_BLK = 256;
constexpr int NODE_REDUCE_WORK = 8;         // entries per thread the grid of a stage-1 node reduction is sized for
constexpr int NODE_REDUCE_MAX_PART = 1024;  // its largest grid: partials the one-workgroup second stage reads

// grid of the first stage of a two-stage reduction over N entries
static inline int node_reduce_grid(long long N) {
    const int g = ceil_div(N, BLOCK_OPS_BLK * NODE_REDUCE_WORK);
    return g > NODE_REDUCE_MAX_PART ? NODE_REDUCE_MAX_PART : g;
}

// sum of v over the workgroup, first half: lane 0 of every wave stores its wave's total in s_cnt4[wave].  The caller's next
// barrier publishes the four totals; block_count_read forms the sum after it
__device__ __forceinline__ void block_count_256(int v, int* s_cnt4) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
    if ((threadIdx.x & 63) == 0) s_cnt4[threadIdx.x >> 6] = v;
}
__device__ __forceinline__ int block_count_read(const int* s_cnt4) { return (s_cnt4[0] + s_cnt4[1]) + (s_cnt4[2] + s_cnt4[3]); }

// Hillis-Steele inclusive scan of v over the 256 threads through s_scan[256]; ends after its last barrier, so a thread may
// return right behind it
__device__ __forceinline__ int block_scan_incl_256(int v, int* s_scan) {
    const int t = threadIdx.x;
    s_scan[t] = v;
    __syncthreads();
    for (int off = 1; off < BLOCK_OPS_BLK; off <<= 1) {
        const int add = t >= off ? s_scan[t - off] : 0;
        __syncthreads();
        s_scan[t] += add;
        __syncthreads();
    }
    return s_scan[t];
}

// merge functors: merge(j, a, b) combines component j in this operand order, identity(j) starts a second stage
struct MergeSum {
    __device__ __forceinline__ double operator()(int, double a, double b) const { return a + b; }
    __device__ __forceinline__ double identity(int) const { return 0.0; }
};

// v[0 .. NV) merged over the 256 threads of a workgroup in a fixed tree: xor shuffles in the wave, then waves 1, 2, 3 into
// wave 0 in that order by thread 0; valid in thread 0.  One barrier
template <int NV, class Merge>
__device__ __forceinline__ void block_tree_256(double* v, Merge merge, double (*lds)[NV]) {
#pragma unroll
    for (int j = 0; j < NV; ++j)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[j] = merge(j, v[j], __shfl_xor(v[j], off, WAVE));
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) lds[wv][j] = v[j];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < NV; ++j) v[j] = merge(j, v[j], lds[i][j]);
    }
}

// the second stage, one workgroup: out[j] = merge over i < npart of part[NV i + j], thread t taking i = t, t + 256, ...
template <int NV, class Merge>
__global__ __launch_bounds__(BLOCK_OPS_BLK) void block_reduce_kernel(I npart, const T* __restrict__ part, T* __restrict__ out,
                                                                      Merge merge) {
    __shared__ double lds[4][NV];
    double v[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = merge.identity(j);
    for (long long i = threadIdx.x; i < npart; i += BLOCK_OPS_BLK)
#pragma unroll
        for (int j = 0; j < NV; ++j) v[j] = merge(j, v[j], part[NV * i + j]);
    block_tree_256<NV>(v, merge, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) out[j] = v[j];
    }
}

template <int NV, class Merge>
static inline void block_reduce(I npart, const T* part, T* out, Merge merge, void* stream) {
    block_reduce_kernel<NV><<<1, BLOCK_OPS_BLK, 0, S(stream)>>>(npart, part, out, merge);
}
