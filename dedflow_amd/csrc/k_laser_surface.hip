// The laser's transmitted beam on the melt surface phi = level, for gfx950 (build-defined, opt-in; model in include/dedflow.h,
// "laser on the level-set surface"; host side in host/laser_surface.c).  The facets come from level_facets.hpp, the tet
// gradient from tet_levelset.hpp, the beam-frame geometry from laser_geom.hpp: included, not copied.
//
// Snapshot (ParticleContextLaserSurfaceUpdate), O(tets):
//   ls_count_kernel   one thread per tet: the facets of the tet that are candidates (the beam enters the metal there:
//                     side (g . dir) > 0, |g| > 0, nine finite coordinates), summed per workgroup (block_count_256 of
//                     block_ops.hpp).  The workgroup counts go through dfl_scan_counts (k_scan.hip): the list is in
//                     ascending tet order, a quad's first triangle first.  Stable by construction: no atomic decides a position
//   ls_emit_kernel    one thread per tet again, the same decision from the same numbers: facet index = blk_base[b] +
//                     block_scan_incl_256 inside the workgroup.  Writes the 9 doubles, the tet, the edge (i, j) and t of every
//                     vertex, and the facet as a dfl_wall_tri record (id = -2 - tet) behind the boundary records of the
//                     laser's candidate list, so that laser_hit_kernel / laser_column_kernel see one list
//   ls_node_*         the distinct nodes of the candidate facets' tets: the (node, 4 facet + local node) pairs sorted by
//                     node (rocprim radix sort, deterministic), run heads counted by the same scan -> slot of every
//                     (facet, local node) and the compact node list.  Nodal power and energy live on that list
// Deposit (one laser step), O(columns + candidates), nothing of size N or T:
//   ls_record_kernel  one thread per column: a column won by facet k writes four records (slot of local node a, 4 c + a)
//                     with the value (eta_s T_c) lambda_a, lambda_a = (w_0 c_0a + w_1 c_1a) + w_2 c_2a; the weights w
//                     are tri_hit's of the same record the column kernel used.  Other columns write a key that sorts last
//   (radix sort of the 4 n^2 keys)
//   ls_sum_kernel     one thread per sorted record; the head of a run sums it from +0.0 in ascending column id (a node is
//                     at most one local node of a column's tet), writes power[slot] and adds dt power to energy[slot]: it
//                     owns the slot.  No floating-point atomics; the order is fixed => bitwise reproducible
//   ls_source_add / ls_power / ls_carry   q[node] += energy / time; the dense scatter of power; and pending energy moved to
//                     a dense array when a new snapshot replaces the node list it was keyed by
#include "block_ops.hpp"
#include "laser_geom.hpp"
#include "level_facets.hpp"
#include <cstring>
#include <rocprim/rocprim.hpp>

#pragma clang fp contract(off)

namespace {

constexpr int BLK = 256;
constexpr int FACE_BITS = 24;  // as k_laser.hip: low bits of a hit key
constexpr unsigned long long NO_HIT = ~0ull;
constexpr int REC_BITS = 20;   // low bits of a deposit key: 4 column + local node (at most 4 * 256^2 = 2^18 records)
constexpr int KEY_BITS = 47;   // slot < 4 * 2^24 above them; the key of a column without a surface hit is 2^46
constexpr unsigned long long NO_REC = 1ull << (KEY_BITS - 1);

struct Dir3 {
    double d[3];
};

// the candidate facets of one tet: bit k of the result = facet k (of lf_tet_facets) is a candidate
__device__ __forceinline__ int ls_tet_candidates(const int4 n4, const T* __restrict__ xg, const T* __restrict__ phi_g, double level,
                                                  double side, const Dir3& dir, double* F, int* ij, double* tt) {
    double phi[4], f[4];
    const int mask = lf_levels(n4, phi_g, level, phi, f);
    if (!lf_facet_count(mask)) return 0;
    double x[12];
    lf_gather_tet(n4, xg, x);
    TetCross c;
    tet_cross(x, c);
    double g[3], gn, dd[4];
    if (!tet_levelset(c, phi, level, g, gn, dd)) return 0;  // |g| > 0; a NaN is not
    const double gd = (g[0] * dir.d[0] + g[1] * dir.d[1]) + g[2] * dir.d[2];
    if (!(side * gd > 0.0)) return 0;                        // the beam enters the metal; a NaN is not greater
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

__global__ __launch_bounds__(BLK) void ls_count_kernel(I NT, const I* __restrict__ ien, const T* __restrict__ xg,
                                                        const T* __restrict__ w, I N, double level, double side, Dir3 dir,
                                                        I* __restrict__ blk_count) {
    __shared__ int s_cnt[BLK / WAVE];
    const long long e = (long long)blockIdx.x * BLK + threadIdx.x;
    int cnt = 0;
    if (e < NT) {
        double F[18], tt[6];
        int ij[2];
        cnt = __popc(ls_tet_candidates(reinterpret_cast<const int4*>(ien)[e], xg, w + 4LL * N, level, side, dir, F, ij, tt));
    }
    block_count_256(cnt, s_cnt);
    __syncthreads();
    if (threadIdx.x == 0) blk_count[blockIdx.x] = block_count_read(s_cnt);
}

__global__ __launch_bounds__(BLK) void ls_emit_kernel(I NT, const I* __restrict__ ien, const T* __restrict__ xg,
                                                       const T* __restrict__ w, I N, double level, double side, Dir3 dir,
                                                       const I* __restrict__ blk_base, dfl_wall_tri* __restrict__ cand,
                                                       T* __restrict__ facets, I* __restrict__ ftet, I* __restrict__ fij,
                                                       T* __restrict__ ft, I cap) {
    __shared__ int s_scan[BLK];
    const int t = threadIdx.x;
    const long long e = (long long)blockIdx.x * BLK + t;
    double F[18], tt[6];
    int ij[2] = {0, 0}, keep = 0;
    if (e < NT) keep = ls_tet_candidates(reinterpret_cast<const int4*>(ien)[e], xg, w + 4LL * N, level, side, dir, F, ij, tt);
    const int cnt = __popc(keep);
    const int incl = block_scan_incl_256(cnt, s_scan);
    if (!cnt) return;  // (after the last barrier)
    long long id = (long long)blk_base[blockIdx.x] + (incl - cnt);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (!((keep >> k) & 1)) continue;
        if (id < cap) {
            dfl_wall_tri r;
#pragma unroll
            for (int q = 0; q < 9; ++q) {
                r.v[q] = F[9 * k + q];
                facets[id * 9 + q] = F[9 * k + q];
            }
            r.n[0] = r.n[1] = r.n[2] = 0.0;  // (a facet record is only ever projected)
            r.off = r.pad = 0.0;
            r.node[0] = r.node[1] = r.node[2] = -1;
            r.id = -2 - (I)e;
            cand[id] = r;
            ftet[id] = (I)e;
            fij[id] = ij[k];
#pragma unroll
            for (int v = 0; v < 3; ++v) ft[id * 3 + v] = tt[3 * k + v];
        }
        ++id;
    }
}

__global__ __launch_bounds__(BLK) void ls_node_keys_kernel(I n, const I* __restrict__ ien, const I* __restrict__ ftet,
                                                            unsigned* __restrict__ key, I* __restrict__ rec) {
    const int r = blockIdx.x * BLK + threadIdx.x;
    if (r >= n) return;
    key[r] = (unsigned)ien[4LL * ftet[r >> 2] + (r & 3)];
    rec[r] = r;
}

__global__ __launch_bounds__(BLK) void ls_node_head_kernel(I n, const unsigned* __restrict__ key, I* __restrict__ flag) {
    const int p = blockIdx.x * BLK + threadIdx.x;
    if (p >= n) return;
    flag[p] = (p == 0 || key[p] != key[p - 1]) ? 1 : 0;
}

// start = the exclusive scan of the head flags: the slot of sorted entry p is the number of heads up to and including p, - 1
__global__ __launch_bounds__(BLK) void ls_node_slot_kernel(I n, const unsigned* __restrict__ key, const I* __restrict__ rec,
                                                            const I* __restrict__ start, I* __restrict__ fslot,
                                                            I* __restrict__ unode) {
    const int p = blockIdx.x * BLK + threadIdx.x;
    if (p >= n) return;
    const bool head = p == 0 || key[p] != key[p - 1];
    const int u = start[p] + (head ? 1 : 0) - 1;
    fslot[rec[p]] = u;
    if (head) unode[u] = (I)key[p];
}

__global__ __launch_bounds__(BLK) void ls_record_kernel(dfl_laser_beam b, const unsigned long long* __restrict__ colkey, I nfb, I nfs,
                                                         const dfl_wall_tri* __restrict__ cand, const I* __restrict__ fij,
                                                         const T* __restrict__ ft, const I* __restrict__ fslot, T eta_s,
                                                         const T* __restrict__ col_T, unsigned long long* __restrict__ key,
                                                         T* __restrict__ val) {
    const int c = blockIdx.x * BLK + threadIdx.x;
    if (c >= b.n * b.n) return;
    const unsigned long long hk = colkey[c];
    const long long idx = (long long)(hk & ((1ull << FACE_BITS) - 1));
    const long long k = idx - nfb;
    double w[3], s;
    bool hit = hk != NO_HIT && k >= 0 && k < nfs;
    if (hit) {
        Proj p;
        project(cand + idx, b, p);
        hit = tri_hit(p, column_centre(c % b.n, b), column_centre(c / b.n, b), w, s);  // (true: the hit kernel found it so)
    }
    if (!hit) {
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            key[4 * c + a] = NO_REC;
            val[4 * c + a] = 0.0;
        }
        return;
    }
    const int e = fij[k];
    const double t0 = ft[3 * k], t1 = ft[3 * k + 1], t2 = ft[3 * k + 2];
    const double pw = eta_s * col_T[c];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        // weight of facet vertex v at local node a: 1 - t at i, t at j, 0 elsewhere
        const double c0 = a == (e & 3) ? 1.0 - t0 : (a == ((e >> 2) & 3) ? t0 : 0.0);
        const double c1 = a == ((e >> 4) & 3) ? 1.0 - t1 : (a == ((e >> 6) & 3) ? t1 : 0.0);
        const double c2 = a == ((e >> 8) & 3) ? 1.0 - t2 : (a == ((e >> 10) & 3) ? t2 : 0.0);
        const double lambda = (w[0] * c0 + w[1] * c1) + w[2] * c2;
        key[4 * c + a] = ((unsigned long long)(unsigned)fslot[4 * k + a] << REC_BITS) | (unsigned long long)(4 * c + a);
        val[4 * c + a] = pw * lambda;
    }
}

__global__ __launch_bounds__(BLK) void ls_sum_kernel(I n, const unsigned long long* __restrict__ key, const T* __restrict__ val, T dt,
                                                      I nslot, T* __restrict__ power, T* __restrict__ energy) {
    const int p = blockIdx.x * BLK + threadIdx.x;
    if (p >= n) return;
    const unsigned long long kp = key[p];
    if (kp >= NO_REC) return;
    const unsigned long long slot = kp >> REC_BITS;
    if (p > 0 && (key[p - 1] >> REC_BITS) == slot) return;  // not the head of its run
    if (slot >= (unsigned long long)nslot) return;          // (never: the slots are those of the snapshot)
    double acc = 0.0;
    for (int q = p; q < n; ++q) {  // ascending column id
        const unsigned long long kq = key[q];
        if ((kq >> REC_BITS) != slot) break;
        acc += val[kq & ((1ull << REC_BITS) - 1)];
    }
    power[slot] = acc;
    energy[slot] += dt * acc;  // this thread owns the slot
}

__global__ __launch_bounds__(BLK) void ls_source_add_kernel(I nmax, const I* __restrict__ nu, const I* __restrict__ unode, T inv_time,
                                                             T* __restrict__ energy, T* __restrict__ q) {
    const int a = blockIdx.x * BLK + threadIdx.x;
    if (a >= nmax || a >= *nu) return;
    q[unode[a]] += energy[a] * inv_time;  // the nodes of the list are distinct
    energy[a] = 0.0;
}

__global__ __launch_bounds__(BLK) void ls_power_kernel(I nmax, const I* __restrict__ nu, const I* __restrict__ unode,
                                                        const T* __restrict__ power, T* __restrict__ q) {
    const int a = blockIdx.x * BLK + threadIdx.x;
    if (a >= nmax || a >= *nu) return;
    q[unode[a]] = power[a];
}

__global__ __launch_bounds__(BLK) void ls_carry_kernel(I nmax, const I* __restrict__ nu, const I* __restrict__ unode,
                                                        T* __restrict__ energy, T* __restrict__ carry) {
    const int a = blockIdx.x * BLK + threadIdx.x;
    if (a >= nmax || a >= *nu) return;
    carry[unode[a]] += energy[a];
    energy[a] = 0.0;
}

__global__ __launch_bounds__(BLK) void ls_carry_add_kernel(I N, T inv_time, T* __restrict__ carry, T* __restrict__ q) {
    const long long a = (long long)blockIdx.x * BLK + threadIdx.x;
    if (a >= N) return;
    q[a] += carry[a] * inv_time;
    carry[a] = 0.0;
}

Dir3 dir3(const T* d) {
    Dir3 r = {{d[0], d[1], d[2]}};
    return r;
}

}  // namespace

extern "C" {

int64_t dfl_laser_surface_temp_bytes(I n_node_keys, I n_records) {
    size_t a = 0, b = 0;
    (void)rocprim::radix_sort_pairs(nullptr, a, (const unsigned*)nullptr, (unsigned*)nullptr, (const I*)nullptr, (I*)nullptr,
                                    (size_t)(n_node_keys > 0 ? n_node_keys : 1));
    (void)rocprim::radix_sort_keys(nullptr, b, (const unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                   (size_t)(n_records > 0 ? n_records : 1), 0, KEY_BITS);
    return (int64_t)(a > b ? a : b) + 16;
}

void dfl_laser_surface_count(I NT, const I* ien, const T* xg, const T* w, I N, T level, I side, const T* dir, I* blk_count,
                             void* stream) {
    if (NT <= 0) return;
    ls_count_kernel<<<ceil_div(NT, BLK), BLK, 0, S(stream)>>>(NT, ien, xg, w, N, level, (double)side, dir3(dir), blk_count);
    DFL_LAUNCH_CHECK();
}

void dfl_laser_surface_emit(I NT, const I* ien, const T* xg, const T* w, I N, T level, I side, const T* dir, const I* blk_base,
                            dfl_wall_tri* cand, T* facets, I* tet, I* ij, T* t, I cap, void* stream) {
    if (NT <= 0) return;
    ls_emit_kernel<<<ceil_div(NT, BLK), BLK, 0, S(stream)>>>(NT, ien, xg, w, N, level, (double)side, dir3(dir), blk_base, cand, facets,
                                                            tet, ij, t, cap);
    DFL_LAUNCH_CHECK();
}

void dfl_laser_surface_nodes(I nfs, const I* ien, const I* tet, uint32_t* key, uint32_t* key_out, I* rec, I* rec_out, I* flag,
                             I* chunk_sum, I* start, I* fslot, I* unode, void* temp, int64_t temp_bytes, void* stream) {
    if (nfs <= 0) return;
    const I n = 4 * nfs;
    ls_node_keys_kernel<<<ceil_div(n, BLK), BLK, 0, S(stream)>>>(n, ien, tet, key, rec);
    DFL_LAUNCH_CHECK();
    size_t bytes = (size_t)temp_bytes;
    DFL_GUARD(rocprim::radix_sort_pairs(temp, bytes, key, key_out, rec, rec_out, (size_t)n, 0, 32, S(stream)));
    ls_node_head_kernel<<<ceil_div(n, BLK), BLK, 0, S(stream)>>>(n, key_out, flag);
    DFL_LAUNCH_CHECK();
    dfl_scan_counts(n, flag, chunk_sum, start, stream);
    ls_node_slot_kernel<<<ceil_div(n, BLK), BLK, 0, S(stream)>>>(n, key_out, rec_out, start, fslot, unode);
    DFL_LAUNCH_CHECK();
}

void dfl_laser_surface_deposit(dfl_laser_beam b, const uint64_t* colkey, I nfb, I nfs, const dfl_wall_tri* cand, const I* ij,
                               const T* t, const I* fslot, T eta_s, T dt, const T* col_T, uint64_t* key, uint64_t* key_out, T* val,
                               T* power, T* energy, void* temp, int64_t temp_bytes, void* stream) {
    const I ncol = b.n * b.n;
    if (ncol <= 0 || nfs <= 0) return;
    DFL_GUARD(hipMemsetAsync(power, 0, (size_t)4 * nfs * sizeof(T), S(stream)));
    ls_record_kernel<<<ceil_div(ncol, BLK), BLK, 0, S(stream)>>>(b, (const unsigned long long*)colkey, nfb, nfs, cand, ij, t, fslot, eta_s,
                                                                col_T, (unsigned long long*)key, val);
    DFL_LAUNCH_CHECK();
    size_t bytes = (size_t)temp_bytes;
    DFL_GUARD(rocprim::radix_sort_keys(temp, bytes, (unsigned long long*)key, (unsigned long long*)key_out, (size_t)4 * ncol, 0,
                                       KEY_BITS, S(stream)));
    ls_sum_kernel<<<ceil_div(4 * ncol, BLK), BLK, 0, S(stream)>>>(4 * ncol, (const unsigned long long*)key_out, val, dt, 4 * nfs, power,
                                                                 energy);
    DFL_LAUNCH_CHECK();
}

void dfl_laser_surface_source_add(I nmax, const I* nu, const I* unode, T inv_time, T* energy, T* q, void* stream) {
    if (nmax <= 0) return;
    ls_source_add_kernel<<<ceil_div(nmax, BLK), BLK, 0, S(stream)>>>(nmax, nu, unode, inv_time, energy, q);
    DFL_LAUNCH_CHECK();
}

void dfl_laser_surface_power(I N, I nmax, const I* nu, const I* unode, const T* power, T* q, void* stream) {
    if (N <= 0) return;
    DFL_GUARD(hipMemsetAsync(q, 0, (size_t)N * sizeof(T), S(stream)));
    if (nmax <= 0) return;
    ls_power_kernel<<<ceil_div(nmax, BLK), BLK, 0, S(stream)>>>(nmax, nu, unode, power, q);
    DFL_LAUNCH_CHECK();
}

void dfl_laser_surface_carry(I nmax, const I* nu, const I* unode, T* energy, T* carry, void* stream) {
    if (nmax <= 0) return;
    ls_carry_kernel<<<ceil_div(nmax, BLK), BLK, 0, S(stream)>>>(nmax, nu, unode, energy, carry);
    DFL_LAUNCH_CHECK();
}

void dfl_laser_surface_carry_add(I N, T inv_time, T* carry, T* q, void* stream) {
    if (N <= 0) return;
    ls_carry_add_kernel<<<ceil_div(N, BLK), BLK, 0, S(stream)>>>(N, inv_time, carry, q);
    DFL_LAUNCH_CHECK();
}

}  // extern "C"
