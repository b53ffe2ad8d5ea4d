// The laser's reflections on the melt surface phi = level, for gfx950 (build-defined, opt-in; model in include/dedflow.h,
// "laser reflections"; host side in host/laser_reflect.c).  The facets come from level_facets.hpp, the tet gradient from
// tet_levelset.hpp, the primary hit from laser_geom.hpp, the ray geometry from laser_reflect_geom.hpp: included, not copied.
//
// Reflection list R (ParticleContextLaserSurfaceUpdate with a reflection set), O(tets):
//   lr_count_kernel   one thread per tet: the facets of the tet with |g| > 0 and nine finite coordinates -- the candidates of
//                     k_laser_surface.hip without the side filter --, summed per workgroup, scanned by dfl_scan_counts
//   lr_emit_kernel    the same decision from the same numbers: facet index = blk_base[b] + the scan inside the workgroup;
//                     writes the 9 doubles, the tet, its gradient, the edge (i, j) and t of every vertex.  The node slots of
//                     R's tets are dfl_laser_surface_nodes on R's tet list
// One laser step, after the unchanged hit and column kernels:
//   lr_cell_*         (Update) a uniform grid over the node bounding box: every facet of R entered into every cell that the box
//                     of its vertices overlaps; integer atomics for the counts and arrival positions only
//   lr_trace_kernel   one lane group (16 lanes or a wave) per column.  A column whose primary hit is a facet starts a ray at
//                     the hit point; at every hit the group books the absorbed share, reflects, and looks for the next
//                     facet: it walks the layers of cells along the ray's dominant axis, in each the rectangle the ray's
//                     entry and exit points span padded by one cell, and stops one layer behind the best hit; the lanes
//                     stride a cell's entries, each keeps its (tau, index) minimum, xor shuffles merge them (smaller tau,
//                     then lower index): the minimum over all of R, which the kernel takes directly when it gets no grid.  The winner's (u, v) are recomputed by every lane from the winner's index: the same
//                     operations, the same bits.  Writes per (bounce, column) the facet, the absorbed power and the weights,
//                     per column the escaped / remaining power, and the column's substrate / reflected tally partials
//   lr_record_kernel  one thread per (bounce, column): four records (slot of local node a, ((b n n + c) 4 + a)) with the value
//                     absorbed lambda_a; other (b, c) write a key that sorts last
//   (radix sort of the (max_bounce + 1) 4 n^2 keys)
//   lr_sum_kernel     the head of a run sums it from +0.0 in ascending record id -- bounce-major, then column -- and owns the
//                     slot.  No floating-point atomics; bitwise reproducible
//   lr_tally_kernel   one workgroup: thread t sums columns t, t + 256, ... then block_tree_256
#include "block_ops.hpp"
#include "laser_geom.hpp"
#include "laser_reflect_geom.hpp"
#include "level_facets.hpp"
#include <cstring>
#include <rocprim/rocprim.hpp>

#pragma clang fp contract(off)

namespace {

constexpr int BLK = 256;
constexpr int FACE_BITS = 24;  // as k_laser.hip: low bits of a hit key
constexpr unsigned long long NO_HIT = ~0ull;
constexpr int REC_BITS = 22;   // low bits of a deposit key: ((b n n + c) 4 + a) < 9 * 4 * 256^2 < 2^22
constexpr int KEY_BITS = 49;   // slot < 4 * 2^24 above them; the key of a (b, c) without a hit is 2^48
constexpr unsigned long long NO_REC = 1ull << (KEY_BITS - 1);
constexpr int MAXB = 8;
constexpr int NTALLY = 2 * (MAXB + 1) + 2;  // absorbed[9], escaped, remaining, rays[9]

// the facets of one tet that belong to R: bit k of the result = facet k (of lf_tet_facets); g is the tet's gradient
__device__ __forceinline__ int lr_tet_facets(const int4 n4, const T* __restrict__ xg, const T* __restrict__ phi_g, double level,
                                              double* F, int* ij, double* tt, double* g) {
    double phi[4], f[4];
    const int mask = lf_levels(n4, phi_g, level, phi, f);
    if (!lf_facet_count(mask)) return 0;
    double x[12];
    lf_gather_tet(n4, xg, x);
    TetCross c;
    tet_cross(x, c);
    double gn, dd[4];
    if (!tet_levelset(c, phi, level, g, gn, dd)) return 0;  // |g| > 0; a NaN is not
    const int nf = lf_tet_facets_ijt(x, f, mask, F, ij, tt);
    int keep = 0;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (k >= nf) continue;
        bool finite = true;
#pragma unroll
        for (int q = 0; q < 9; ++q) finite = finite && fabs(F[9 * k + q]) < HUGE_VAL;
        if (finite) keep |= 1 << k;
    }
    return keep;
}

__global__ __launch_bounds__(BLK) void lr_count_kernel(I NT, const I* __restrict__ ien, const T* __restrict__ xg,
                                                        const T* __restrict__ w, I N, double level, I* __restrict__ blk_count) {
    __shared__ int s_cnt[BLK / WAVE];
    const long long e = (long long)blockIdx.x * BLK + threadIdx.x;
    int cnt = 0;
    if (e < NT) {
        double F[18], tt[6], g[3];
        int ij[2];
        cnt = __popc(lr_tet_facets(reinterpret_cast<const int4*>(ien)[e], xg, w + 4LL * N, level, F, ij, tt, g));
    }
    block_count_256(cnt, s_cnt);
    __syncthreads();
    if (threadIdx.x == 0) blk_count[blockIdx.x] = block_count_read(s_cnt);
}

__global__ __launch_bounds__(BLK) void lr_emit_kernel(I NT, const I* __restrict__ ien, const T* __restrict__ xg,
                                                       const T* __restrict__ w, I N, double level, const I* __restrict__ blk_base,
                                                       T* __restrict__ facets, I* __restrict__ rtet, T* __restrict__ rgrad,
                                                       I* __restrict__ rij, T* __restrict__ rt, I cap) {
    __shared__ int s_scan[BLK];
    const int t = threadIdx.x;
    const long long e = (long long)blockIdx.x * BLK + t;
    double F[18], tt[6], g[3] = {0.0, 0.0, 0.0};
    int ij[2] = {0, 0}, keep = 0;
    if (e < NT) keep = lr_tet_facets(reinterpret_cast<const int4*>(ien)[e], xg, w + 4LL * N, level, F, ij, tt, g);
    const int cnt = __popc(keep);
    const int incl = block_scan_incl_256(cnt, s_scan);
    if (!cnt) return;  // (after the last barrier)
    long long id = (long long)blk_base[blockIdx.x] + (incl - cnt);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (!((keep >> k) & 1)) continue;
        if (id < cap) {
#pragma unroll
            for (int q = 0; q < 9; ++q) facets[id * 9 + q] = F[9 * k + q];
            rtet[id] = (I)e;
            rij[id] = ij[k];
#pragma unroll
            for (int v = 0; v < 3; ++v) {
                rgrad[id * 3 + v] = g[v];
                rt[id * 3 + v] = tt[3 * k + v];
            }
        }
        ++id;
    }
}

struct ReflectArgs {
    int model, max_bounce;
    double eta_s, eps, side;
};

// cell of a coordinate along axis k, clamped into the grid; a NaN gives cell 0 (fmax)
__device__ __forceinline__ int lr_cell(const dfl_grid3& gr, int k, double x) {
    return (int)fmin(fmax(floor((x - gr.lo[k]) * gr.inv[k]), 0.0), (double)(gr.n[k] - 1));
}

// the cells that the box of a facet's vertices overlaps
__device__ __forceinline__ void lr_facet_cells(const dfl_grid3& gr, const T* __restrict__ F, int* c0, int* c1) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        c0[k] = lr_cell(gr, k, fmin(F[k], fmin(F[3 + k], F[6 + k])));
        c1[k] = lr_cell(gr, k, fmax(F[k], fmax(F[3 + k], F[6 + k])));
    }
}

// one thread per facet: count[cell] += 1 for every cell its box overlaps (integer atomics on the counts only, as rd_cut_kernel)
__global__ __launch_bounds__(BLK) void lr_cell_count_kernel(I nr, const T* __restrict__ facets, dfl_grid3 gr, I* __restrict__ count) {
    const int f = blockIdx.x * BLK + threadIdx.x;
    if (f >= nr) return;
    int c0[3], c1[3];
    lr_facet_cells(gr, facets + 9LL * f, c0, c1);
    for (int z = c0[2]; z <= c1[2]; ++z)
        for (int y = c0[1]; y <= c1[1]; ++y)
            for (int x = c0[0]; x <= c1[0]; ++x) atomicAdd(&count[((long long)z * gr.n[1] + y) * gr.n[0] + x], 1);
}

// the same cells again: entry[start[cell] + arrival] = facet.  The order inside a cell is free: the trace takes a minimum
// over (tau, index).  cursor is zero on entry (dfl_scan_counts leaves the counts so)
__global__ __launch_bounds__(BLK) void lr_cell_emit_kernel(I nr, const T* __restrict__ facets, dfl_grid3 gr, const I* __restrict__ start,
                                                            I* __restrict__ cursor, I* __restrict__ entry, I cap) {
    const int f = blockIdx.x * BLK + threadIdx.x;
    if (f >= nr) return;
    int c0[3], c1[3];
    lr_facet_cells(gr, facets + 9LL * f, c0, c1);
    for (int z = c0[2]; z <= c1[2]; ++z)
        for (int y = c0[1]; y <= c1[1]; ++y)
            for (int x = c0[0]; x <= c1[0]; ++x) {
                const long long c = ((long long)z * gr.n[1] + y) * gr.n[0] + x;
                const long long e = (long long)start[c] + atomicAdd(&cursor[c], 1);
                if (e < cap) entry[e] = f;
            }
}

// the running (tau, index) minimum of one lane: the smaller tau, on a tie the lower index
__device__ __forceinline__ void lr_keep(double tau, int f, double& best, int& bi) {
    if (tau < best || (tau == best && f < bi)) {
        best = tau;
        bi = f;
    }
}

// facet f against the ray (X, d) leaving tet t0; feeds the lane's minimum
__device__ __forceinline__ void lr_test(int f, int t0, const double* X, const double* d, double side, const T* __restrict__ facets,
                                        const I* __restrict__ rtet, const T* __restrict__ rgrad, double& best, int& bi) {
    if (rtet[f] == t0) return;
    const double gf[3] = {rgrad[3LL * f], rgrad[3LL * f + 1], rgrad[3LL * f + 2]};
    if (!(side * lr_dot(gf, d) > 0.0)) return;  // the ray enters the metal there; a NaN is not greater
    double F[9], u, v, tau;
#pragma unroll
    for (int q = 0; q < 9; ++q) F[q] = facets[9LL * f + q];
    if (!lr_ray_triangle(X, d, F, u, v, tau)) return;
    lr_keep(tau, f, best, bi);
}

// first index of R whose tet is >= tet (R is in ascending tet id)
__device__ __forceinline__ int lr_lower_bound(const I* __restrict__ rtet, int nr, int tet) {
    int lo = 0, hi = nr;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (rtet[mid] < tet) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

template <int G>
__global__ __launch_bounds__(BLK) void lr_trace_kernel(dfl_laser_beam b, const unsigned long long* __restrict__ colkey, I nfb, I nfs,
                                                        const dfl_wall_tri* __restrict__ cand, const I* __restrict__ ftet, I nr,
                                                        const T* __restrict__ facets, const I* __restrict__ rtet,
                                                        const T* __restrict__ rgrad, ReflectArgs ra, const T* __restrict__ col_T,
                                                        I* __restrict__ hit_facet, T* __restrict__ hit_abs, T* __restrict__ hit_w,
                                                        T* __restrict__ ray_end, T* __restrict__ part, dfl_grid3 gr,
                                                        const I* __restrict__ cell_start, const I* __restrict__ cell_entry,
                                                        T* __restrict__ visited) {
    const int ncol = b.n * b.n;
    const int lane = threadIdx.x & (G - 1);
    const int c = blockIdx.x * (BLK / G) + threadIdx.x / G;
    if (c >= ncol) return;  // (whole lane groups: no barrier below, and the shuffles stay inside a group)
    double nvisit = 0.0;
    const int nb = ra.max_bounce + 1;
    // everything up to the facet loop is wave-uniform: every lane computes the same numbers
    const unsigned long long hk = colkey[c];
    const long long idx = (long long)(hk & ((1ull << FACE_BITS) - 1));
    const long long k = idx - nfb;
    double w[3] = {0.0, 0.0, 0.0}, s;
    bool hit = hk != NO_HIT && k >= 0 && k < nfs;
    if (hit) {
        Proj p;
        project(cand + idx, b, p);
        hit = tri_hit(p, column_centre(c % b.n, b), column_centre(c / b.n, b), w, s);  // (true: the hit kernel found it so)
    }
    int r = -1;
    if (hit) {
        const int tet = ftet[k];
        r = lr_lower_bound(rtet, nr, tet) + ((k > 0 && ftet[k - 1] == tet) ? 1 : 0);  // a quad's second triangle follows its first
        hit = r < nr && rtet[r] == tet;                                               // (true: the candidates are a subset of R)
    }
    int bounce = 0;
    double escaped = 0.0, remaining = 0.0;
    if (hit) {
        double X[3], d[3] = {b.dir[0], b.dir[1], b.dir[2]};
        lr_point(facets + 9LL * r, w[0], w[1], w[2], X);
        double p = col_T[c], sub = 0.0;
        for (;;) {
            const double g[3] = {rgrad[3LL * r], rgrad[3LL * r + 1], rgrad[3LL * r + 2]};
            const double A = lr_absorptivity(ra.model, ra.eta_s, ra.eps, d, g);
            const double ab = A * p;
            p = p - ab;
            sub = bounce == 0 ? ab : sub + ab;
            if (lane == 0) {
                const long long o = (long long)bounce * ncol + c;
                hit_facet[o] = r;
                hit_abs[o] = ab;
                hit_w[3 * o] = w[0]; hit_w[3 * o + 1] = w[1]; hit_w[3 * o + 2] = w[2];
            }
            ++bounce;
            if (bounce == nb) {
                remaining = p;
                break;
            }
            double dn[3];
            lr_reflect(d, g, dn);
            d[0] = dn[0]; d[1] = dn[1]; d[2] = dn[2];
            const int t0 = rtet[r];
            double best = HUGE_VAL;
            int bi = 0x7fffffff;
            if (!cell_start) {  // no grid: all of R
                for (int f = lane; f < nr; f += G) lr_test(f, t0, X, d, ra.side, facets, rtet, rgrad, best, bi);
                nvisit += (double)nr;
            } else {
                // the layers of cells along the ray's dominant axis a, from the layer behind the ray's start; in each the
                // rectangle of cells that the ray's entry and exit points span, padded by one cell; stop only after the
                // layer behind the one in which the best tau so far lies
                int a = 0;
                if (fabs(d[1]) > fabs(d[a])) a = 1;
                if (fabs(d[2]) > fabs(d[a])) a = 2;
                const int p1 = (a + 1) % 3, p2 = (a + 2) % 3;
                const int step = d[a] > 0.0 ? 1 : -1;  // (d[a] != 0 unless d is zero or NaN: then nothing is hit anyway)
                int L = lr_cell(gr, a, X[a]) - step;
                for (; L >= -1 && L <= gr.n[a]; L += step) {
                    if (L < 0 || L >= gr.n[a]) {
                        if ((L < 0) == (step < 0)) break;  // left the grid
                        continue;                            // (the padded layer behind the start)
                    }
                    const double ta = ((gr.lo[a] + (double)L / gr.inv[a]) - X[a]) / d[a];
                    const double tb = ((gr.lo[a] + (double)(L + 1) / gr.inv[a]) - X[a]) / d[a];
                    const double t0r = fmax(fmin(ta, tb), 0.0), t1r = fmax(fmax(ta, tb), 0.0);
                    // (both ends clamped into the grid: a ray beside the grid walks its boundary cells, which is only more)
                    const double q0 = ((X[p1] + t0r * d[p1]) - gr.lo[p1]) * gr.inv[p1], q1 = ((X[p1] + t1r * d[p1]) - gr.lo[p1]) * gr.inv[p1];
                    const double r0 = ((X[p2] + t0r * d[p2]) - gr.lo[p2]) * gr.inv[p2], r1 = ((X[p2] + t1r * d[p2]) - gr.lo[p2]) * gr.inv[p2];
                    const double top1 = (double)(gr.n[p1] - 1), top2 = (double)(gr.n[p2] - 1);
                    const int lo1 = (int)fmin(fmax(floor(fmin(q0, q1)) - 1.0, 0.0), top1), hi1 = (int)fmin(fmax(floor(fmax(q0, q1)) + 1.0, 0.0), top1);
                    const int lo2 = (int)fmin(fmax(floor(fmin(r0, r1)) - 1.0, 0.0), top2), hi2 = (int)fmin(fmax(floor(fmax(r0, r1)) + 1.0, 0.0), top2);
                    for (int i2 = lo2; i2 <= hi2; ++i2)
                        for (int i1 = lo1; i1 <= hi1; ++i1) {
                            int ix[3];
                            ix[a] = L; ix[p1] = i1; ix[p2] = i2;
                            const long long cell = ((long long)ix[2] * gr.n[1] + ix[1]) * gr.n[0] + ix[0];
                            const int e0 = cell_start[cell], e1 = cell_start[cell + 1];
                            for (int e = e0 + lane; e < e1; e += G) lr_test(cell_entry[e], t0, X, d, ra.side, facets, rtet, rgrad, best, bi);
                            nvisit += (double)(e1 - e0);
                        }
                    // the group's best so far decides whether to stop
                    double gb = best;
#pragma unroll
                    for (int off = G / 2; off > 0; off >>= 1) gb = fmin(gb, __shfl_xor(gb, off, G));
                    if (gb < HUGE_VAL) {
                        const int Lb = lr_cell(gr, a, X[a] + gb * d[a]);
                        if (step > 0 ? L > Lb : L < Lb) break;
                    }
                }
            }
#pragma unroll
            for (int off = G / 2; off > 0; off >>= 1) {
                const double ot = __shfl_xor(best, off, G);
                const int oi = __shfl_xor(bi, off, G);
                lr_keep(ot, oi, best, bi);
            }
            if (bi == 0x7fffffff) {
                escaped = p;
                break;
            }
            r = bi;
            double F[9], u, v, tau;
#pragma unroll
            for (int q = 0; q < 9; ++q) F[q] = facets[9LL * r + q];
            lr_ray_triangle(X, d, F, u, v, tau);  // the winner's own numbers again
            w[0] = (1.0 - u) - v; w[1] = u; w[2] = v;
            lr_point(F, w[0], w[1], w[2], X);
        }
        // a model-0 ray that found no second facet keeps the column kernel's partials, eta_s T_c and (1 - eta_s) T_c: the
        // six-entry tally of a surface without a second hit has the bits of a step without reflections
        if (lane == 0 && !(ra.model == 0 && bounce == 1 && bounce < nb)) {
            part[3LL * ncol + c] = sub;
            part[4LL * ncol + c] = escaped + remaining;  // one of them is +0.0
        }
    }
    if (lane == 0) {
        for (int q = bounce; q < nb; ++q) {
            const long long o = (long long)q * ncol + c;
            hit_facet[o] = -1;
            hit_abs[o] = 0.0;
            hit_w[3 * o] = hit_w[3 * o + 1] = hit_w[3 * o + 2] = 0.0;
        }
        ray_end[c] = escaped;
        ray_end[ncol + c] = remaining;
        if (visited) visited[c] = nvisit;
    }
}

__global__ __launch_bounds__(BLK) void lr_record_kernel(I nrec, const I* __restrict__ hit_facet, const T* __restrict__ hit_abs,
                                                         const T* __restrict__ hit_w, I nr, const I* __restrict__ rij,
                                                         const T* __restrict__ rt, const I* __restrict__ fslot,
                                                         unsigned long long* __restrict__ key, T* __restrict__ val) {
    const int o = blockIdx.x * BLK + threadIdx.x;  // b n n + c
    if (o >= nrec) return;
    const int k = hit_facet[o];
    if (k < 0 || k >= nr) {
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            key[4LL * o + a] = NO_REC;
            val[4LL * o + a] = 0.0;
        }
        return;
    }
    const int e = rij[k];
    const double t0 = rt[3LL * k], t1 = rt[3LL * k + 1], t2 = rt[3LL * k + 2];
    const double w0 = hit_w[3LL * o], w1 = hit_w[3LL * o + 1], w2 = hit_w[3LL * o + 2];
    const double pw = hit_abs[o];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        // weight of facet vertex v at local node a: 1 - t at i, t at j, 0 elsewhere (as ls_record_kernel)
        const double c0 = a == (e & 3) ? 1.0 - t0 : (a == ((e >> 2) & 3) ? t0 : 0.0);
        const double c1 = a == ((e >> 4) & 3) ? 1.0 - t1 : (a == ((e >> 6) & 3) ? t1 : 0.0);
        const double c2 = a == ((e >> 8) & 3) ? 1.0 - t2 : (a == ((e >> 10) & 3) ? t2 : 0.0);
        const double lambda = (w0 * c0 + w1 * c1) + w2 * c2;
        key[4LL * o + a] = ((unsigned long long)(unsigned)fslot[4LL * k + a] << REC_BITS) | (unsigned long long)(4LL * o + a);
        val[4LL * o + a] = pw * lambda;
    }
}

__global__ __launch_bounds__(BLK) void lr_sum_kernel(I n, const unsigned long long* __restrict__ key, const T* __restrict__ val, T dt,
                                                      I nslot, T* __restrict__ power, T* __restrict__ energy) {
    const int p = blockIdx.x * BLK + threadIdx.x;
    if (p >= n) return;
    const unsigned long long kp = key[p];
    if (kp >= NO_REC) return;
    const unsigned long long slot = kp >> REC_BITS;
    if (p > 0 && (key[p - 1] >> REC_BITS) == slot) return;  // not the head of its run
    if (slot >= (unsigned long long)nslot) return;          // (never: the slots are those of the snapshot)
    double acc = 0.0;
    for (int q = p; q < n; ++q) {  // ascending record id: bounce-major, then column
        const unsigned long long kq = key[q];
        if ((kq >> REC_BITS) != slot) break;
        acc += val[kq & ((1ull << REC_BITS) - 1)];
    }
    power[slot] = acc;
    energy[slot] += dt * acc;  // this thread owns the slot
}

// out[0 .. 9) absorbed per bounce, out[9] escaped, out[10] remaining, out[11 .. 20) rays per bounce (as doubles: exact)
__global__ __launch_bounds__(BLK) void lr_tally_kernel(I ncol, I nb, const I* __restrict__ hit_facet, const T* __restrict__ hit_abs,
                                                        const T* __restrict__ ray_end, T* __restrict__ out) {
    __shared__ double lds[4][NTALLY];
    double v[NTALLY];
#pragma unroll
    for (int j = 0; j < NTALLY; ++j) v[j] = 0.0;
    for (int c = threadIdx.x; c < ncol; c += BLK) {
#pragma unroll
        for (int q = 0; q <= MAXB; ++q) {
            if (q >= nb) continue;
            const long long o = (long long)q * ncol + c;
            v[q] += hit_abs[o];
            v[MAXB + 3 + q] += hit_facet[o] >= 0 ? 1.0 : 0.0;
        }
        v[MAXB + 1] += ray_end[c];
        v[MAXB + 2] += ray_end[ncol + c];
    }
    block_tree_256<NTALLY>(v, MergeSum(), lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < NTALLY; ++j) out[j] = v[j];
    }
}

}  // namespace

extern "C" {

int64_t dfl_laser_reflect_temp_bytes(I n_records) {
    size_t b = 0;
    (void)rocprim::radix_sort_keys(nullptr, b, (const unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                   (size_t)(n_records > 0 ? n_records : 1), 0, KEY_BITS);
    return (int64_t)b + 16;
}

void dfl_laser_reflect_count(I NT, const I* ien, const T* xg, const T* w, I N, T level, I* blk_count, void* stream) {
    if (NT <= 0) return;
    lr_count_kernel<<<ceil_div(NT, BLK), BLK, 0, S(stream)>>>(NT, ien, xg, w, N, level, blk_count);
    DFL_LAUNCH_CHECK();
}

void dfl_laser_reflect_emit(I NT, const I* ien, const T* xg, const T* w, I N, T level, const I* blk_base, T* facets, I* tet, T* grad,
                            I* ij, T* t, I cap, void* stream) {
    if (NT <= 0) return;
    lr_emit_kernel<<<ceil_div(NT, BLK), BLK, 0, S(stream)>>>(NT, ien, xg, w, N, level, blk_base, facets, tet, grad, ij, t, cap);
    DFL_LAUNCH_CHECK();
}

void dfl_laser_reflect_cells_count(I nr, const T* facets, dfl_grid3 grid, I* count, void* stream) {
    if (nr <= 0) return;
    lr_cell_count_kernel<<<ceil_div(nr, BLK), BLK, 0, S(stream)>>>(nr, facets, grid, count);
    DFL_LAUNCH_CHECK();
}

void dfl_laser_reflect_cells_emit(I nr, const T* facets, dfl_grid3 grid, const I* start, I* cursor, I* entry, I cap, void* stream) {
    if (nr <= 0) return;
    lr_cell_emit_kernel<<<ceil_div(nr, BLK), BLK, 0, S(stream)>>>(nr, facets, grid, start, cursor, entry, cap);
    DFL_LAUNCH_CHECK();
}

void dfl_laser_reflect_trace(dfl_laser_beam b, const uint64_t* colkey, I nfb, I nfs, const dfl_wall_tri* cand, const I* ftet, I nr,
                             const T* facets, const I* rtet, const T* rgrad, I side, I model, I max_bounce, T eta_s, T eps,
                             const T* col_T, I* hit_facet, T* hit_abs, T* hit_w, T* ray_end, T* part, void* stream) {
    dfl_grid3 none;
    memset(&none, 0, sizeof none);
    dfl_laser_reflect_trace_grid(b, colkey, nfb, nfs, cand, ftet, nr, facets, rtet, rgrad, side, model, max_bounce, eta_s, eps, col_T,
                                 hit_facet, hit_abs, hit_w, ray_end, part, none, nullptr, nullptr, 64, nullptr, stream);
}

void dfl_laser_reflect_trace_grid(dfl_laser_beam b, const uint64_t* colkey, I nfb, I nfs, const dfl_wall_tri* cand, const I* ftet, I nr,
                                  const T* facets, const I* rtet, const T* rgrad, I side, I model, I max_bounce, T eta_s, T eps,
                                  const T* col_T, I* hit_facet, T* hit_abs, T* hit_w, T* ray_end, T* part, dfl_grid3 grid,
                                  const I* cell_start, const I* cell_entry, I group, T* visited, void* stream) {
    const I ncol = b.n * b.n;
    if (ncol <= 0 || max_bounce < 1 || max_bounce > MAXB) return;
    ReflectArgs ra;
    ra.model = model;
    ra.max_bounce = max_bounce;
    ra.eta_s = eta_s;
    ra.eps = eps;
    ra.side = (double)side;
    if (group == 16)
        lr_trace_kernel<16><<<ceil_div(ncol, BLK / 16), BLK, 0, S(stream)>>>(b, (const unsigned long long*)colkey, nfb, nr > 0 ? nfs : 0,
                                                                             cand, ftet, nr, facets, rtet, rgrad, ra, col_T, hit_facet,
                                                                             hit_abs, hit_w, ray_end, part, grid, cell_start, cell_entry,
                                                                             visited);
    else
        lr_trace_kernel<64><<<ceil_div(ncol, BLK / 64), BLK, 0, S(stream)>>>(b, (const unsigned long long*)colkey, nfb, nr > 0 ? nfs : 0,
                                                                             cand, ftet, nr, facets, rtet, rgrad, ra, col_T, hit_facet,
                                                                             hit_abs, hit_w, ray_end, part, grid, cell_start, cell_entry,
                                                                             visited);
    DFL_LAUNCH_CHECK();
}

void dfl_laser_reflect_deposit(I nrec, const I* hit_facet, const T* hit_abs, const T* hit_w, I nr, const I* ij, const T* t,
                               const I* fslot, T dt, uint64_t* key, uint64_t* key_out, T* val, T* power, T* energy, void* temp,
                               int64_t temp_bytes, void* stream) {
    if (nrec <= 0 || nr <= 0) return;
    DFL_GUARD(hipMemsetAsync(power, 0, (size_t)4 * nr * sizeof(T), S(stream)));
    lr_record_kernel<<<ceil_div(nrec, BLK), BLK, 0, S(stream)>>>(nrec, hit_facet, hit_abs, hit_w, nr, ij, t, fslot,
                                                                (unsigned long long*)key, val);
    DFL_LAUNCH_CHECK();
    size_t bytes = (size_t)temp_bytes;
    DFL_GUARD(rocprim::radix_sort_keys(temp, bytes, (unsigned long long*)key, (unsigned long long*)key_out, (size_t)4 * nrec, 0,
                                       KEY_BITS, S(stream)));
    lr_sum_kernel<<<ceil_div(4 * nrec, BLK), BLK, 0, S(stream)>>>(4 * nrec, (const unsigned long long*)key_out, val, dt, 4 * nr, power,
                                                                 energy);
    DFL_LAUNCH_CHECK();
}

void dfl_laser_reflect_tally(I ncol, I max_bounce, const I* hit_facet, const T* hit_abs, const T* ray_end, T* out, void* stream) {
    if (max_bounce < 1 || max_bounce > MAXB) return;
    lr_tally_kernel<<<1, BLK, 0, S(stream)>>>(ncol, max_bounce + 1, hit_facet, hit_abs, ray_end, out);
    DFL_LAUNCH_CHECK();
}

}  // extern "C"
