// Level-set redistancing for gfx950: the exact distance of every node to the piecewise-linear surface phi = level inside a
// band (build-defined; model in include/dedflow.h, "level-set redistancing"; geometry in level_facets.hpp).
//
//   rd_cut_kernel        one thread per tet.  The volume of {phi > level} in the tet and, for a cut tet, ||g| - 1| go through a
//                        fixed tree (block_tree_256 of block_ops.hpp) to one (sum, max) pair per workgroup.  COUNT: also the
//                        number of facets of the workgroup (block_count_256; level 1 of the scan that makes the facet index
//                        the ascending-tet order) and, per facet, count[c]++ for every cell its bounding box overlaps.  Only a
//                        tet with a positive node gathers coordinates.  The host scans the workgroup counts and the cells
//                        with dfl_scan_counts (k_scan.hip).
//   rd_emit_kernel       one thread per tet again: facet index = blk_base[b] + block_scan_incl_256 inside the workgroup;
//                        writes the 9 doubles and enters the index into its cells (integer atomic on the cell's fill count:
//                        the order inside a cell is free because the result is a minimum).
//   rd_node_count_kernel one thread per node: the entries of the 27 cells around it as nine three-cell runs of cell_start.
//                        None (about 95 % at bench size): written at once.  Else compacted: wave ballot, one integer atomic
//                        per wave, order free.
//   rd_node_dist_kernel  16 lanes per compacted node (the NG_LANES idiom of node_gather.hpp), the groups stride the list.  The
//                        lanes stride the entries of a run, each keeps a running minimum of d^2; four xor-shuffles; lane 0
//                        writes.  The trip counts are uniform inside a group, so the shuffles only ever meet active lanes.
//   rd_node_stats, then block_reduce_kernel   two-stage fixed-order (sum, max) reductions.
//
// No float atomics anywhere.  The same facet may sit in several of a node's 27 cells: it is evaluated again, which a
// minimum does not see.  The file is compiled without fused multiply-add, as level_facets.hpp is wherever it is included.
#include "block_ops.hpp"
#include "level_facets.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int RD_BLK = BLOCK_OPS_BLK;
constexpr int RD_LANES = 16;       // lanes per compacted node
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

// a sum and a maximum (of values >= 0; fmax passes over a NaN)
struct MergePair {
    __device__ __forceinline__ double operator()(int j, double a, double b) const { return j == 0 ? a + b : fmax(a, b); }
    __device__ __forceinline__ double identity(int) const { return 0.0; }
};

template <bool COUNT>
__global__ __launch_bounds__(RD_BLK) void rd_cut_kernel(I NT, const I* __restrict__ ien, const T* __restrict__ xg,
                                                         const T* __restrict__ w, I N, double level, const Grid g,
                                                         I* __restrict__ blk_count, I* __restrict__ cell_count,
                                                         T* __restrict__ part) {
    __shared__ double lds[4][2];
    __shared__ int s_cnt[4];
    const long long e = (long long)blockIdx.x * RD_BLK + threadIdx.x;
    double p[2] = {0.0, 0.0};  // volume, | |g| - 1 |
    int nf = 0;
    if (e < NT) {
        const int4 n4 = reinterpret_cast<const int4*>(ien)[e];
        double phi[4], f[4];
        const int mask = lf_levels(n4, w + 4LL * N, level, phi, f);
        if (mask) {
            double x[12];
            lf_gather_tet(n4, xg, x);
            TetCross c;
            tet_cross(x, c);
            const double vol = lf_positive_volume(x, f, mask, c.det);
            p[0] = vol == vol ? vol : 0.0;  // a NaN phi at a node of a cut tet: the tet adds nothing
            if (mask != 15) {
                double gr[3], gn, dd[4];
                tet_levelset(c, phi, level, gr, gn, dd);
                p[1] = fabs(gn - 1.0);
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
    if (COUNT) block_count_256(nf, s_cnt);
    block_tree_256<2>(p, MergePair(), lds);  // (its barrier also publishes s_cnt)
    if (threadIdx.x == 0) {
        part[2LL * blockIdx.x] = p[0];
        part[2LL * blockIdx.x + 1] = p[1];
        if (COUNT) blk_count[blockIdx.x] = block_count_read(s_cnt);
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
        mask = lf_levels(n4, w + 4LL * N, level, phi, f);
    }
    const int nf = lf_facet_count(mask);
    const int incl = block_scan_incl_256(nf, s_scan);
    if (!nf) return;  // (after the last barrier)
    const long long first = (long long)blk_base[blockIdx.x] + (incl - nf);
    double x[12], F[18];
    lf_gather_tet(n4, xg, x);
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
    const MergePair merge;
    double p[2] = {0.0, 0.0};  // band nodes, largest change
    const long long stride = (long long)gridDim.x * RD_BLK;
    for (long long a = (long long)blockIdx.x * RD_BLK + threadIdx.x; a < N; a += stride) {
        const double c = chg[a];
        if (c >= 0.0) {
            p[0] = merge(0, p[0], 1.0);
            p[1] = merge(1, p[1], c);
        }
    }
    block_tree_256<2>(p, merge, lds);
    if (threadIdx.x == 0) {
        part[2LL * blockIdx.x] = p[0];
        part[2LL * blockIdx.x + 1] = p[1];
    }
}

}  // namespace

extern "C" {

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
    const int g = node_reduce_grid(N);
    rd_node_stats_kernel<<<g, RD_BLK, 0, S(stream)>>>(N, chg, work);
    block_reduce<2>(g, work, out2, MergePair(), stream);
    DFL_LAUNCH_CHECK();
}

void dfl_redistance_reduce(I npart, const T* part, T* out2, void* stream) {
    if (npart <= 0) return;
    block_reduce<2>(npart, part, out2, MergePair(), stream);
    DFL_LAUNCH_CHECK();
}

}  // extern "C"
