// The chunked exclusive scan of integer counts for gfx950: the one scan behind the DEM cell sort (k_dem.hip, k_walls.hip,
// the laser's column bins), the workgroup counts of the count -> scan -> emit passes (k_redistance.hip, k_volume.hip,
// k_laser_surface.hip, k_solidify.hip), the redistancing cells and the laser surface's node heads.
//
//   scan_chunk_sum_kernel   total of every 1024-entry chunk
//   scan_chunk_kernel       workgroup b owns [b * 1024, (b + 1) * 1024): adds up the chunk totals before it, scans its own
//                           entries (four per thread, then block_scan_incl_256 over the thread sums), zeroes them
// Two dependent launches, no allocation, no host round trip; integer sums only, so the result has no order to keep.
#include "block_ops.hpp"

namespace {

constexpr int BLK = BLOCK_OPS_BLK;
constexpr int SCAN_CHUNK = 4 * BLK;  // entries per workgroup

// sum of v over the workgroup through s_part[256]; every thread returns it
__device__ __forceinline__ int scan_block_total(int v, int* s_part) {
    const int t = threadIdx.x;
    s_part[t] = v;
    __syncthreads();
    for (int off = BLK / 2; off > 0; off >>= 1) {
        if (t < off) s_part[t] += s_part[t + off];
        __syncthreads();
    }
    const int total = s_part[0];
    __syncthreads();
    return total;
}

__global__ __launch_bounds__(BLK) void scan_chunk_sum_kernel(I n, const I* __restrict__ count, I* __restrict__ chunk_sum) {
    __shared__ int s_part[BLK];
    const long long c0 = (long long)blockIdx.x * SCAN_CHUNK + 4 * threadIdx.x;
    int v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) v += (c0 + k < n) ? count[c0 + k] : 0;
    const int total = scan_block_total(v, s_part);
    if (threadIdx.x == 0) chunk_sum[blockIdx.x] = total;
}

// start[0 .. n] = exclusive scan of count[0 .. n) (start[n] = total), count zeroed
__global__ __launch_bounds__(BLK) void scan_chunk_kernel(I n, I* __restrict__ count, const I* __restrict__ chunk_sum,
                                                          I* __restrict__ start) {
    __shared__ int s_part[BLK];
    const int t = threadIdx.x, b = blockIdx.x;
    int acc = 0;
    for (int k = t; k < b; k += BLK) acc += chunk_sum[k];
    const int base = scan_block_total(acc, s_part);
    const long long c0 = (long long)b * SCAN_CHUNK + 4 * t;  // 4 consecutive entries per thread
    int v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[k] = (c0 + k < n) ? count[c0 + k] : 0;
        if (c0 + k < n) count[c0 + k] = 0;  // ready for the next pass
    }
    const int mine = (v[0] + v[1]) + (v[2] + v[3]);
    int run = base + block_scan_incl_256(mine, s_part) - mine;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (c0 + k <= n) start[c0 + k] = run;
        run += v[k];
    }
}

}  // namespace

extern "C" {

I dfl_tets_per_block(void) { return BLOCK_OPS_BLK; }

I dfl_node_reduce_max_part(void) { return NODE_REDUCE_MAX_PART; }

I dfl_scan_num_chunks(I n) { return (I)ceil_div((long long)n + 1, SCAN_CHUNK); }

void dfl_scan_counts(I n, I* count, I* chunk_sum, I* start, void* stream) {
    if (n < 0) return;
    const I nchunk = dfl_scan_num_chunks(n);
    scan_chunk_sum_kernel<<<nchunk, BLK, 0, S(stream)>>>(n, count, chunk_sum);
    scan_chunk_kernel<<<nchunk, BLK, 0, S(stream)>>>(n, count, chunk_sum, start);
    DFL_LAUNCH_CHECK();
}

}  // extern "C"
