// Level-set redistancing for gfx950: the exact distance of every node to the piecewise-linear surface phi = level inside a
// band (build-defined; model in include/dedflow.h, "level-set redistancing"; geometry in level_facets.hpp).
//
//   rd_cut_kernel        one thread per tet.  The volume of {phi > level} in the tet and, for a cut tet, ||g| - 1| go through a
//                        fixed tree to one (sum, max) pair per workgroup.  COUNT: also the number of facets of the workgroup
//                        (level 1 of the scan that makes the facet index the ascending-tet order) and, per facet, count[c]++
//                        for every cell its bounding box overlaps.  Only a tet with a positive node gathers coordinates.
//   rd_chunk_sum / rd_scan   the exclusive scan of the DEM cell sort (k_dem.hip): 1024 entries per workgroup, every workgroup
//                        adds up the chunk totals before it.  Used for the workgroup facet counts and for the cells.
//   rd_emit_kernel       one thread per tet again: facet index = blk_base[b] + the exclusive scan inside the workgroup;
//                        writes the 9 doubles and enters the index into its cells (integer atomic on the cell's fill count:
//                        the order inside a cell is free because the result is a minimum).
//   rd_node_count_kernel one thread per node: the entries of the 27 cells around it as nine three-cell runs of cell_start.
//                        None (about 95 % at bench size): written at once.  Else compacted: wave ballot, one integer atomic
//                        per wave, order free.
//   rd_node_dist_kernel  16 lanes per compacted node (the NG_LANES idiom of node_gather.hpp), the groups stride the list.  The
//                        lanes stride the entries of a run, each keeps a running minimum of d^2; four xor-shuffles; lane 0
//                        writes.  The trip counts are uniform inside a group, so the shuffles only ever meet active lanes.
//   rd_node_stats / rd_reduce   two-stage fixed-order (sum, max) reductions (the scheme of k_phase.hip's statistics).
//
// No float atomics anywhere.  The same facet may sit in several of a node's 27 cells: it is evaluated again, which a
// minimum does not see.  The file is compiled without fused multiply-add, as level_facets.hpp is wherever it is included.
#include "level_facets.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int RD_BLK = 256;
constexpr int RD_CHUNK = 1024;     // entries per scan workgroup
constexpr int RD_LANES = 16;       // lanes per compacted node
constexpr int RD_MAX_PART = 1024;  // partial pairs of a node reduction
constexpr int RD_MAX_GROUP_BLOCKS = 2048;

typedef dfl_redistance_grid Grid;

// cell of a finite coordinate
__device__ __forceinline__ int rd_cell(double x, double lo, double inv_h, int n) {
    double u = floor((x - lo) * inv_h);
    u = u < 0.0 ? 0.0 : (u > (double)(n - 1) ? (double)(n - 1) : u);
    return (int)u;
}

// the cell range of the bounding box of a facet's finite vertices: a vertex with a NaN or infinite coordinate (a NaN phi at
// a node of the tet) cannot win, nor can a segment that ends in it, but the other vertices and the segment between them
// still count.  false: no vertex is finite and the facet enters no cell
__device__ __forceinline__ bool rd_facet_cells(const double* F, const Grid& g, int* lo, int* hi) {
    double mn[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, mx[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    bool any = false;
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        const double* V = F + 3 * v;
        if (fabs(V[0]) < HUGE_VAL && fabs(V[1]) < HUGE_VAL && fabs(V[2]) < HUGE_VAL) {
            any = true;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                mn[d] = fmin(mn[d], V[d]);
                mx[d] = fmax(mx[d], V[d]);
            }
        }
    }
    if (!any) return false;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        lo[d] = rd_cell(mn[d], g.lo[d], g.inv_h, g.n[d]);
        hi[d] = rd_cell(mx[d], g.lo[d], g.inv_h, g.n[d]);
    }
    return true;
}

__device__ __forceinline__ void rd_gather(const int4 n4, const T* __restrict__ xg, double* x) {
    const long long n[4] = {n4.x, n4.y, n4.z, n4.w};
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int d = 0; d < 3; ++d) x[b * 3 + d] = xg[n[b] * 3 + d];
}

// phi of the tet's nodes and f = phi - level; returns the mask of the positive nodes
__device__ __forceinline__ int rd_levels(const int4 n4, const T* __restrict__ phi_g, double level, double* phi, double* f) {
    phi[0] = phi_g[n4.x]; phi[1] = phi_g[n4.y]; phi[2] = phi_g[n4.z]; phi[3] = phi_g[n4.w];
#pragma unroll
    for (int a = 0; a < 4; ++a) f[a] = phi[a] - level;
    return lf_positive_mask(f);
}

struct Pair {
    double s, m;  // a sum and a maximum (of values >= 0; fmax passes over a NaN)
};
__device__ __forceinline__ void pair_merge(Pair& a, const Pair& b) {
    a.s = a.s + b.s;
    a.m = fmax(a.m, b.m);
}
// fixed tree over the 256 threads of a workgroup: xor shuffles in the wave, then the four waves in order; valid in thread 0
__device__ __forceinline__ Pair pair_block(Pair p, double (*lds)[2]) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        Pair o;
        o.s = __shfl_xor(p.s, off, WAVE);
        o.m = __shfl_xor(p.m, off, WAVE);
        pair_merge(p, o);
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) {
        lds[wv][0] = p.s;
        lds[wv][1] = p.m;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int i = 1; i < 4; ++i) {
            Pair o = {lds[i][0], lds[i][1]};
            pair_merge(p, o);
        }
    return p;
}

template <bool COUNT>
__global__ __launch_bounds__(RD_BLK) void rd_cut_kernel(I NT, const I* __restrict__ ien, const T* __restrict__ xg,
                                                         const T* __restrict__ w, I N, double level, const Grid g,
                                                         I* __restrict__ blk_count, I* __restrict__ cell_count,
                                                         T* __restrict__ part) {
    __shared__ double lds[4][2];
    __shared__ int s_cnt[4];
    const long long e = (long long)blockIdx.x * RD_BLK + threadIdx.x;
    Pair p = {0.0, 0.0};
    int nf = 0;
    if (e < NT) {
        const int4 n4 = reinterpret_cast<const int4*>(ien)[e];
        double phi[4], f[4];
        const int mask = rd_levels(n4, w + 4LL * N, level, phi, f);
        if (mask) {
            double x[12];
            rd_gather(n4, xg, x);
            TetCross c;
            tet_cross(x, c);
            const double vol = lf_positive_volume(x, f, mask, c.det);
            p.s = vol == vol ? vol : 0.0;  // a NaN phi at a node of a cut tet: the tet adds nothing
            if (mask != 15) {
                double gr[3], gn, dd[4];
                tet_levelset(c, phi, level, gr, gn, dd);
                p.m = fabs(gn - 1.0);
                if (COUNT) {
                    double F[18];
                    nf = lf_tet_facets(x, f, mask, F);
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        int lo[3], hi[3];
                        if (k >= nf || !rd_facet_cells(F + 9 * k, g, lo, hi)) continue;
                        for (int cz = lo[2]; cz <= hi[2]; ++cz)
                            for (int cy = lo[1]; cy <= hi[1]; ++cy)
                                for (int cx = lo[0]; cx <= hi[0]; ++cx) atomicAdd(&cell_count[cx + g.n[0] * (cy + g.n[1] * cz)], 1);
                    }
                }
            }
        }
    }
    if (COUNT) {
        int cnt = nf;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, WAVE);
        if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = cnt;
    }
    p = pair_block(p, lds);  // (its barrier also publishes s_cnt)
    if (threadIdx.x == 0) {
        part[2LL * blockIdx.x] = p.s;
        part[2LL * blockIdx.x + 1] = p.m;
        if (COUNT) blk_count[blockIdx.x] = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
    }
}

// total of every 1024-entry chunk
__global__ __launch_bounds__(RD_BLK) void rd_chunk_sum_kernel(I n, const I* __restrict__ count, I* __restrict__ chunk_sum) {
    __shared__ int s_part[RD_BLK];
    const int t = threadIdx.x;
    const long long c0 = (long long)blockIdx.x * RD_CHUNK + 4 * t;
    int v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) v += (c0 + k < n) ? count[c0 + k] : 0;
    s_part[t] = v;
    __syncthreads();
    for (int off = RD_BLK / 2; off > 0; off >>= 1) {
        if (t < off) s_part[t] += s_part[t + off];
        __syncthreads();
    }
    if (t == 0) chunk_sum[blockIdx.x] = s_part[0];
}

// start[0 .. n] = exclusive scan of count[0 .. n) (start[n] = total), count zeroed; workgroup b owns [b * 1024, (b + 1) * 1024)
__global__ __launch_bounds__(RD_BLK) void rd_scan_kernel(I n, I* __restrict__ count, const I* __restrict__ chunk_sum,
                                                          I* __restrict__ start) {
    __shared__ int s_part[RD_BLK];
    __shared__ int s_base;
    const int t = threadIdx.x, b = blockIdx.x;
    int acc = 0;
    for (int k = t; k < b; k += RD_BLK) acc += chunk_sum[k];
    s_part[t] = acc;
    __syncthreads();
    for (int off = RD_BLK / 2; off > 0; off >>= 1) {
        if (t < off) s_part[t] += s_part[t + off];
        __syncthreads();
    }
    if (t == 0) s_base = s_part[0];
    __syncthreads();
    const int base = s_base;
    __syncthreads();
    const long long c0 = (long long)b * RD_CHUNK + 4 * t;
    int v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[k] = (c0 + k < n) ? count[c0 + k] : 0;
        if (c0 + k < n) count[c0 + k] = 0;
    }
    const int mine = (v[0] + v[1]) + (v[2] + v[3]);
    s_part[t] = mine;
    __syncthreads();
    for (int off = 1; off < RD_BLK; off <<= 1) {  // Hillis-Steele inclusive scan of the 256 thread sums
        const int add = t >= off ? s_part[t - off] : 0;
        __syncthreads();
        s_part[t] += add;
        __syncthreads();
    }
    int run = base + s_part[t] - mine;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (c0 + k <= n) start[c0 + k] = run;
        run += v[k];
    }
}

__global__ __launch_bounds__(RD_BLK) void rd_emit_kernel(I NT, const I* __restrict__ ien, const T* __restrict__ xg,
                                                          const T* __restrict__ w, I N, double level, const Grid g,
                                                          const I* __restrict__ blk_base, const I* __restrict__ cell_start,
                                                          I* __restrict__ cell_fill, T* __restrict__ facets, I cap_facets,
                                                          I* __restrict__ entries, I cap_entries) {
    __shared__ int s_scan[RD_BLK];
    const int t = threadIdx.x;
    const long long e = (long long)blockIdx.x * RD_BLK + t;
    int4 n4 = {0, 0, 0, 0};
    double phi[4], f[4];
    int mask = 0;
    if (e < NT) {
        n4 = reinterpret_cast<const int4*>(ien)[e];
        mask = rd_levels(n4, w + 4LL * N, level, phi, f);
    }
    const int nf = lf_facet_count(mask);
    s_scan[t] = nf;
    __syncthreads();
    for (int off = 1; off < RD_BLK; off <<= 1) {
        const int add = t >= off ? s_scan[t - off] : 0;
        __syncthreads();
        s_scan[t] += add;
        __syncthreads();
    }
    if (!nf) return;  // (after the last barrier)
    const long long first = (long long)blk_base[blockIdx.x] + (s_scan[t] - nf);
    double x[12], F[18];
    rd_gather(n4, xg, x);
    lf_tet_facets(x, f, mask, F);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const long long id = first + k;
        if (k >= nf || id >= cap_facets) continue;
        const double* Fk = F + 9 * k;
#pragma unroll
        for (int q = 0; q < 9; ++q) facets[id * 9 + q] = Fk[q];
        int lo[3], hi[3];
        if (!rd_facet_cells(Fk, g, lo, hi)) continue;
        for (int cz = lo[2]; cz <= hi[2]; ++cz)
            for (int cy = lo[1]; cy <= hi[1]; ++cy)
                for (int cx = lo[0]; cx <= hi[0]; ++cx) {
                    const int c = cx + g.n[0] * (cy + g.n[1] * cz);
                    const long long pos = (long long)cell_start[c] + atomicAdd(&cell_fill[c], 1);
                    if (pos < cap_entries) entries[pos] = (I)id;
                }
    }
}

// the cell of a node and its x range: the 27 cells around it are the nine runs r = (y, z) of three contiguous cells
struct NodeCell {
    int x0, x1, cy, cz;
};
__device__ __forceinline__ NodeCell rd_node_cell(const double* p, const Grid& g) {
    const int cx = rd_cell(p[0], g.lo[0], g.inv_h, g.n[0]);
    NodeCell c;
    c.x0 = max(cx - 1, 0);
    c.x1 = min(cx + 1, g.n[0] - 1);
    c.cy = rd_cell(p[1], g.lo[1], g.inv_h, g.n[1]);
    c.cz = rd_cell(p[2], g.lo[2], g.inv_h, g.n[2]);
    return c;
}
// run r < 9 covers the entries [lo, hi) (empty outside the grid)
__device__ __forceinline__ void rd_run(const NodeCell& c, int r, const Grid& g, const I* __restrict__ cell_start, int& lo, int& hi) {
    const int y = c.cy + r % 3 - 1, z = c.cz + r / 3 - 1;
    lo = hi = 0;
    if (y < 0 || y >= g.n[1] || z < 0 || z >= g.n[2]) return;
    const int row = g.n[0] * (y + g.n[1] * z);
    lo = cell_start[row + c.x0];
    hi = cell_start[row + c.x1 + 1];
}

__global__ __launch_bounds__(RD_BLK) void rd_node_count_kernel(I N, const T* __restrict__ xg, T* __restrict__ w, double level,
                                                                double band, const Grid g, const I* __restrict__ cell_start,
                                                                const unsigned char* __restrict__ hold, I* __restrict__ ncand,
                                                                I* __restrict__ list, T* __restrict__ chg) {
    const long long a = (long long)blockIdx.x * RD_BLK + threadIdx.x;
    bool cand = false;
    if (a < N) {
        const double p[3] = {xg[3 * a], xg[3 * a + 1], xg[3 * a + 2]};
        const NodeCell c = rd_node_cell(p, g);
        int total = 0;
#pragma unroll
        for (int r = 0; r < 9; ++r) {
            int lo, hi;
            rd_run(c, r, g, cell_start, lo, hi);
            total += hi - lo;
        }
        if (total > 0) {
            cand = true;
        } else {  // no facet within the band: level +- band, and not a band node
            const double old = w[4LL * N + a];
            chg[a] = -1.0;
            if (old == old && !(hold && hold[a])) w[4LL * N + a] = level + (old - level > 0.0 ? band : -band);
        }
    }
    const unsigned long long m = __ballot(cand);
    if (m) {  // wave-uniform
        const int lane = threadIdx.x & 63;
        int base = 0;
        if (lane == 0) base = atomicAdd(ncand, __popcll(m));
        base = __shfl(base, 0, WAVE);
        if (cand) list[base + __popcll(m & ((1ull << lane) - 1ull))] = (I)a;
    }
}

__global__ __launch_bounds__(RD_BLK) void rd_node_dist_kernel(I N, const T* __restrict__ xg, T* __restrict__ w, double level,
                                                               double band, const Grid g, const I* __restrict__ cell_start,
                                                               const I* __restrict__ entries, const T* __restrict__ facets,
                                                               I cap_facets, const unsigned char* __restrict__ hold,
                                                               const I* __restrict__ ncand, const I* __restrict__ list,
                                                               T* __restrict__ chg) {
    const int l = threadIdx.x & (RD_LANES - 1);
    const long long ngroup = (long long)gridDim.x * (RD_BLK / RD_LANES);
    const I nc = min(*ncand, N);
    for (long long i = (long long)blockIdx.x * (RD_BLK / RD_LANES) + threadIdx.x / RD_LANES; i < nc; i += ngroup) {
        const long long a = list[i];
        const double p[3] = {xg[3 * a], xg[3 * a + 1], xg[3 * a + 2]};
        const NodeCell c = rd_node_cell(p, g);
        double best = HUGE_VAL;
#pragma unroll 1
        for (int r = 0; r < 9; ++r) {
            int lo, hi;
            rd_run(c, r, g, cell_start, lo, hi);
            for (int k = lo + l; k < hi; k += RD_LANES) {
                const I fi = entries[k];
                if ((unsigned)fi >= (unsigned)cap_facets) continue;  // (never: the host sized both lists)
                const double* Fg = facets + 9LL * fi;
                double F[9];
#pragma unroll
                for (int q = 0; q < 9; ++q) F[q] = Fg[q];
                const double d2 = lf_point_facet_dist2(p, F);
                if (d2 < best) best = d2;
            }
        }
#pragma unroll
        for (int off = RD_LANES / 2; off > 0; off >>= 1) {
            const double o = __shfl_xor(best, off, RD_LANES);
            if (o < best) best = o;
        }
        if (l == 0) {
            const double d = sqrt(best), old = w[4LL * N + a];
            const bool in_band = d < band;
            const double m = in_band ? d : band;
            const double now = level + (old - level > 0.0 ? m : -m);
            const bool kept = !(old == old) || (hold && hold[a]);
            if (!kept) w[4LL * N + a] = now;
            chg[a] = in_band ? (kept ? 0.0 : fabs(now - old)) : -1.0;
        }
    }
}

__global__ __launch_bounds__(RD_BLK) void rd_node_stats_kernel(I N, const T* __restrict__ chg, T* __restrict__ part) {
    __shared__ double lds[4][2];
    Pair p = {0.0, 0.0};
    const long long stride = (long long)gridDim.x * RD_BLK;
    for (long long a = (long long)blockIdx.x * RD_BLK + threadIdx.x; a < N; a += stride) {
        const double c = chg[a];
        if (c >= 0.0) {
            const Pair o = {1.0, c};
            pair_merge(p, o);
        }
    }
    p = pair_block(p, lds);
    if (threadIdx.x == 0) {
        part[2LL * blockIdx.x] = p.s;
        part[2LL * blockIdx.x + 1] = p.m;
    }
}

__global__ __launch_bounds__(RD_BLK) void rd_reduce_kernel(I npart, const T* __restrict__ part, T* __restrict__ out2) {
    __shared__ double lds[4][2];
    Pair p = {0.0, 0.0};
    for (long long i = threadIdx.x; i < npart; i += RD_BLK) {
        const Pair o = {part[2 * i], part[2 * i + 1]};
        pair_merge(p, o);
    }
    p = pair_block(p, lds);
    if (threadIdx.x == 0) {
        out2[0] = p.s;
        out2[1] = p.m;
    }
}

}  // namespace

extern "C" {

I dfl_redistance_tets_per_block(void) { return RD_BLK; }

void dfl_redistance_cut(I NT, const I* ien, const T* xg, const T* w, I N, T level, const dfl_redistance_grid* grid, I* blk_count,
                        I* cell_count, T* part, void* stream) {
    if (NT <= 0) return;
    if (blk_count)
        rd_cut_kernel<true><<<ceil_div(NT, RD_BLK), RD_BLK, 0, S(stream)>>>(NT, ien, xg, w, N, level, *grid, blk_count, cell_count, part);
    else {
        const Grid none = {{0.0, 0.0, 0.0}, 0.0, {1, 1, 1}};
        rd_cut_kernel<false><<<ceil_div(NT, RD_BLK), RD_BLK, 0, S(stream)>>>(NT, ien, xg, w, N, level, grid ? *grid : none, nullptr,
                                                                            nullptr, part);
    }
    DFL_LAUNCH_CHECK();
}

void dfl_redistance_scan(I n, I* count, I* chunk_sum, I* start, void* stream) {
    if (n < 0) return;
    const int nchunk = ceil_div((long long)n + 1, RD_CHUNK);
    rd_chunk_sum_kernel<<<nchunk, RD_BLK, 0, S(stream)>>>(n, count, chunk_sum);
    rd_scan_kernel<<<nchunk, RD_BLK, 0, S(stream)>>>(n, count, chunk_sum, start);
    DFL_LAUNCH_CHECK();
}

void dfl_redistance_emit(I NT, const I* ien, const T* xg, const T* w, I N, T level, const dfl_redistance_grid* grid,
                         const I* blk_base, const I* cell_start, I* cell_fill, T* facets, I cap_facets, I* entries, I cap_entries,
                         void* stream) {
    if (NT <= 0) return;
    rd_emit_kernel<<<ceil_div(NT, RD_BLK), RD_BLK, 0, S(stream)>>>(NT, ien, xg, w, N, level, *grid, blk_base, cell_start, cell_fill,
                                                                  facets, cap_facets, entries, cap_entries);
    DFL_LAUNCH_CHECK();
}

void dfl_redistance_nodes(I N, const T* xg, T* w, T level, T band, const dfl_redistance_grid* grid, const I* cell_start,
                          const I* entries, const T* facets, I cap_facets, const unsigned char* hold, I* ncand, I* list, T* chg,
                          void* stream) {
    if (N <= 0) return;
    rd_node_count_kernel<<<ceil_div(N, RD_BLK), RD_BLK, 0, S(stream)>>>(N, xg, w, level, band, *grid, cell_start, hold, ncand, list, chg);
    int nb = ceil_div(N, RD_BLK / RD_LANES);
    if (nb > RD_MAX_GROUP_BLOCKS) nb = RD_MAX_GROUP_BLOCKS;
    rd_node_dist_kernel<<<nb, RD_BLK, 0, S(stream)>>>(N, xg, w, level, band, *grid, cell_start, entries, facets, cap_facets, hold, ncand,
                                                      list, chg);
    DFL_LAUNCH_CHECK();
}

void dfl_redistance_node_stats(I N, const T* chg, T* work, T* out2, void* stream) {
    if (N <= 0) return;
    int g = ceil_div(N, RD_BLK * 8);
    if (g > RD_MAX_PART) g = RD_MAX_PART;
    rd_node_stats_kernel<<<g, RD_BLK, 0, S(stream)>>>(N, chg, work);
    rd_reduce_kernel<<<1, RD_BLK, 0, S(stream)>>>(g, work, out2);
    DFL_LAUNCH_CHECK();
}

void dfl_redistance_reduce(I npart, const T* part, T* out2, void* stream) {
    if (npart <= 0) return;
    rd_reduce_kernel<<<1, RD_BLK, 0, S(stream)>>>(npart, part, out2);
    DFL_LAUNCH_CHECK();
}

}  // extern "C"
