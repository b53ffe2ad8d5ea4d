// Surface mesh for gfx950: the surface phi = level as one indexed triangle mesh, one vertex per cut mesh edge, every triangle
// oriented out of the metal, with nodal fields interpolated to the vertices (build-defined; model in include/dedflow.h,
// "surface mesh").  Passive: the state w is read and never written.  The sorted variant ("Surface mesh").
//
//   sm_bad_nodes_kernel   one thread per node: the nodes whose phi is not finite, counted
//   sm_classify_kernel    one thread per tet: code[e] = 0 for a tet that emits nothing (a bad node: counted; not cut; cut with a
//                         determinant that is zero or not finite: counted), else the mask of its metal nodes | 16 where the
//                         determinant is negative.  The coordinates are gathered for the cut tets only.  Per workgroup the
//                         triangles into count[b] and the edge keys into count[nblk + b]: one scan (k_scan.hip) of the 2 nblk
//                         counts gives both offsets, start[nblk] = triangles, start[2 nblk] - start[nblk] = keys
//   sm_counts_kernel      both totals beside the other counters: one read-back carries all of them
//   sm_emit_kernel        one thread per tet, from code[] alone: one block scan of the packed pair (triangles, keys); tri_tet at
//                         the tet's triangle offset, and the keys min(i, j) << bits | max(i, j), bits = ceil(log2 N), of its three
//                         or four cut edges at its key offset.  rocprim's radix sort over the 2 bits significant bits: equal
//                         keys are equal edges, so the result does not depend on the sort's own order
//   sm_head_count_kernel  one thread per sorted key: the heads of the runs per workgroup -> scan
//   sm_vertex_kernel      the same heads: the rank of a head is its vertex id.  The head writes the key, the edge with the metal
//                         node first, t, the crossing point and the K field values
//   sm_tri_kernel         one thread per triangle k: its tet tri_tet[k], the second of a quad where tri_tet[k - 1] is the same
//                         tet; the tet's levels and coordinates gathered once more (only cut tets are read); the three keys
//                         looked up in the unique list by binary search; the second and third index swapped by the table over
//                         (mask, determinant sign); the area through block_tree_256 to part[workgroup]
//   block_reduce          the workgroups' areas in the second stage's fixed tree
//   sm_finish_kernel      the vertex count beside the other counters
//
// No float atomics: the one sum has a fixed order.  Integer atomics carry counts only.  The file is compiled without fused
// multiply-add, as level_facets.hpp is wherever it is included.
#include "block_ops.hpp"
#include "level_facets.hpp"
#include <cstring>
#include <rocprim/rocprim.hpp>

#pragma clang fp contract(off)

namespace {

constexpr int SM_BLK = BLOCK_OPS_BLK;
enum { SM_TRIS = 0, SM_KEYS = 1, SM_VERTS = 2, SM_BAD_NODES = 3, SM_BAD_TETS = 4, SM_DEGENERATE = 5 };
typedef unsigned long long U64;

// bit m: in a tet with a positive determinant and the metal nodes of mask m, the facets of lf_tet_facets turn their normal
// (B - A) x (C - A) into the metal, so the second and third vertex are swapped; a negative determinant inverts the answer.
// The decision uses nothing that was rounded: inside one mask and one determinant sign the triangle cannot turn over while
// the signs of f are strict (tests/surface_mesh_model.py derives the table from geometry and checks it)
constexpr unsigned SM_SWAP = 0x4D24u;

struct SmFields {
    const T* q[DFL_SURFACE_MESH_MAX_FIELDS];
};

__device__ __forceinline__ bool sm_finite(double v) { return fabs(v) < HUGE_VAL; }

// f = phi - level, negated for side = -1
__device__ __forceinline__ double sm_level(double ph, double level, double side) {
    const double f = ph - level;
    return side < 0.0 ? -f : f;
}

// the local (i, j), i metal, of the tet's three or four crossing points in the order of lf_tet_facets; returns their number
__device__ __forceinline__ int sm_edges(int mask, int* ei, int* ej) {
    const int np = __popc(mask);
    if (np == 2) {
        int a, b, c, d;
        lf_pairs(mask, a, b, c, d);
        ei[0] = a; ej[0] = c;
        ei[1] = a; ej[1] = d;
        ei[2] = b; ej[2] = d;
        ei[3] = b; ej[3] = c;
        return 4;
    }
    const int lone = np == 1 ? __ffs(mask) - 1 : __ffs(~mask & 15) - 1;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int o = k + (k >= lone ? 1 : 0);
        ei[k] = np == 1 ? lone : o;
        ej[k] = np == 1 ? o : lone;
    }
    ei[3] = ej[3] = 0;
    return 3;
}

__device__ __forceinline__ int sm_pick_node(const int4 n4, int a) { return a == 0 ? n4.x : a == 1 ? n4.y : a == 2 ? n4.z : n4.w; }

__device__ __forceinline__ U64 sm_key(int ni, int nj, int bits) {
    const unsigned lo = ni < nj ? ni : nj, hi = ni < nj ? nj : ni;
    return (U64)lo << bits | (U64)hi;
}

__global__ __launch_bounds__(SM_BLK) void sm_bad_nodes_kernel(I N, const T* __restrict__ phi, I* __restrict__ cnt) {
    __shared__ int s_cnt[4];
    const long long a = (long long)blockIdx.x * SM_BLK + threadIdx.x;
    block_count_256(a < N && !sm_finite(phi[a]) ? 1 : 0, s_cnt);
    __syncthreads();
    if (threadIdx.x == 0) {
        const int n = block_count_read(s_cnt);
        if (n) atomicAdd(cnt + SM_BAD_NODES, n);
    }
}

__global__ __launch_bounds__(SM_BLK) void sm_classify_kernel(I NT, const I* __restrict__ ien, const T* __restrict__ xg,
                                                              const T* __restrict__ phi_g, I N, double level, double side,
                                                              unsigned char* __restrict__ code, I nblk, I* __restrict__ count,
                                                              I* __restrict__ cnt) {
    __shared__ int s_tri[4], s_key[4], s_bad[4], s_deg[4];
    const long long e = (long long)blockIdx.x * SM_BLK + threadIdx.x;
    int ntri = 0, bad = 0, deg = 0;
    if (e < NT) {
        const int4 n4 = reinterpret_cast<const int4*>(ien)[e];
        int c = 0;
        if ((unsigned)n4.x >= (unsigned)N || (unsigned)n4.y >= (unsigned)N || (unsigned)n4.z >= (unsigned)N ||
            (unsigned)n4.w >= (unsigned)N) {
            bad = 1;  // (never: ien holds node ids)
        } else {
            const double ph[4] = {phi_g[n4.x], phi_g[n4.y], phi_g[n4.z], phi_g[n4.w]};
            bad = !(sm_finite(ph[0]) && sm_finite(ph[1]) && sm_finite(ph[2]) && sm_finite(ph[3]));
            if (!bad) {
                double f[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) f[a] = sm_level(ph[a], level, side);
                const int mask = lf_positive_mask(f);
                ntri = lf_facet_count(mask);
                if (ntri) {
                    double x[12];
                    lf_gather_tet(n4, xg, x);
                    TetCross tc;
                    tet_cross(x, tc);
                    if (tc.det != 0.0 && sm_finite(tc.det)) {
                        c = mask | (tc.det < 0.0 ? 16 : 0);
                    } else {
                        deg = 1;
                        ntri = 0;
                    }
                }
            }
        }
        code[e] = (unsigned char)c;
    }
    block_count_256(ntri, s_tri);
    block_count_256(ntri == 2 ? 4 : ntri == 1 ? 3 : 0, s_key);
    block_count_256(bad, s_bad);
    block_count_256(deg, s_deg);
    __syncthreads();
    if (threadIdx.x == 0) {
        count[blockIdx.x] = block_count_read(s_tri);
        count[nblk + blockIdx.x] = block_count_read(s_key);
        const int nb = block_count_read(s_bad), nd = block_count_read(s_deg);
        if (nb) atomicAdd(cnt + SM_BAD_TETS, nb);
        if (nd) atomicAdd(cnt + SM_DEGENERATE, nd);
    }
}

__global__ void sm_counts_kernel(const I* __restrict__ start, I nblk, I* __restrict__ cnt) {
    if (threadIdx.x == 0) cnt[SM_TRIS] = start[nblk];
    if (threadIdx.x == 1) cnt[SM_KEYS] = start[2LL * nblk] - start[nblk];
}

__global__ __launch_bounds__(SM_BLK) void sm_emit_kernel(I NT, const I* __restrict__ ien, const unsigned char* __restrict__ code,
                                                          const I* __restrict__ start, I nblk, int bits, U64* __restrict__ key,
                                                          I capk, I* __restrict__ tri_tet, I capt) {
    __shared__ int s_scan[SM_BLK];
    const long long e = (long long)blockIdx.x * SM_BLK + threadIdx.x;
    const int mask = e < NT ? (code[e] & 15) : 0;
    const int ntri = lf_facet_count(mask);
    const int nkey = ntri == 2 ? 4 : ntri == 1 ? 3 : 0;
    const int packed = ntri | nkey << 16;  // (at most 512 and 1024 per workgroup)
    const int excl = block_scan_incl_256(packed, s_scan) - packed;
    if (!ntri) return;  // (after the last barrier)
    const long long toff = (long long)start[blockIdx.x] + (excl & 0xffff);
    const long long koff = (long long)(start[nblk + blockIdx.x] - start[nblk]) + (excl >> 16);
    for (int k = 0; k < ntri; ++k)
        if (toff + k < capt) tri_tet[toff + k] = (I)e;  // (always: the host sized the lists)
    const int4 n4 = reinterpret_cast<const int4*>(ien)[e];
    int ei[4], ej[4];
    sm_edges(mask, ei, ej);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < nkey && koff + k < capk) key[koff + k] = sm_key(sm_pick_node(n4, ei[k]), sm_pick_node(n4, ej[k]), bits);
}

__device__ __forceinline__ int sm_is_head(long long p, I n, const U64* __restrict__ key) {
    return p < n && (p == 0 || key[p - 1] != key[p]) ? 1 : 0;
}

__global__ __launch_bounds__(SM_BLK) void sm_head_count_kernel(I n, const U64* __restrict__ key, I* __restrict__ count) {
    __shared__ int s_cnt[4];
    const long long p = (long long)blockIdx.x * SM_BLK + threadIdx.x;
    block_count_256(sm_is_head(p, n, key), s_cnt);
    __syncthreads();
    if (threadIdx.x == 0) count[blockIdx.x] = block_count_read(s_cnt);
}

__global__ __launch_bounds__(SM_BLK) void sm_vertex_kernel(I n, const U64* __restrict__ key, const I* __restrict__ base, int bits,
                                                            const T* __restrict__ xg, const T* __restrict__ phi_g, double level,
                                                            double side, SmFields fields, int K, U64* __restrict__ ukey,
                                                            T* __restrict__ verts, I* __restrict__ edge, T* __restrict__ tv,
                                                            T* __restrict__ vals, I capv) {
    __shared__ int s_scan[SM_BLK];
    const long long p = (long long)blockIdx.x * SM_BLK + threadIdx.x;
    const int head = sm_is_head(p, n, key);
    const int incl = block_scan_incl_256(head, s_scan);
    if (!head) return;  // (after the last barrier)
    const long long v = (long long)base[blockIdx.x] + (incl - 1);
    if (v >= capv) return;  // (never: the host sized the lists for n vertices)
    const U64 k = key[p];
    const long long lo = (long long)(k >> bits), hi = (long long)(k & ((1ull << bits) - 1ull));
    const double flo = sm_level(phi_g[lo], level, side), fhi = sm_level(phi_g[hi], level, side);
    const bool lo_metal = flo > 0.0;
    const long long i = lo_metal ? lo : hi, j = lo_metal ? hi : lo;
    const double fi = lo_metal ? flo : fhi, fj = lo_metal ? fhi : flo;
    const double t = fi / (fi - fj);
    ukey[v] = k;
    edge[2 * v] = (I)i;
    edge[2 * v + 1] = (I)j;
    tv[v] = t;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double xi = xg[3 * i + d];
        verts[3 * v + d] = xi + t * (xg[3 * j + d] - xi);
    }
    for (int q = 0; q < K; ++q) {
        const double qi = fields.q[q][i];
        vals[v * K + q] = qi + t * (fields.q[q][j] - qi);
    }
}

// the rank of k in the ascending ukey[0 .. nv), -1 when it is not there (never)
__device__ __forceinline__ I sm_find(const U64* __restrict__ ukey, I nv, U64 k) {
    I lo = 0, hi = nv;
    while (lo < hi) {
        const I mid = lo + ((hi - lo) >> 1);
        if (ukey[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    return lo < nv && ukey[lo] == k ? lo : -1;
}

__global__ __launch_bounds__(SM_BLK) void sm_tri_kernel(I nt, const I* __restrict__ tri_tet, const I* __restrict__ ien,
                                                         const unsigned char* __restrict__ code, const T* __restrict__ xg,
                                                         const T* __restrict__ phi_g, double level, double side,
                                                         const U64* __restrict__ ukey, const I* __restrict__ nv_ptr, I capv,
                                                         int bits, I* __restrict__ tris, T* __restrict__ part) {
    __shared__ double lds[4][1];
    const long long k = (long long)blockIdx.x * SM_BLK + threadIdx.x;
    double v[1] = {0.0};
    if (k < nt) {
        const I nv = *nv_ptr < capv ? *nv_ptr : capv;
        const I e = tri_tet[k];
        const bool second = k > 0 && tri_tet[k - 1] == e;
        const int c = code[e], mask = c & 15;
        const int4 n4 = reinterpret_cast<const int4*>(ien)[e];
        double x[12], f[4];
        lf_gather_tet(n4, xg, x);
        f[0] = sm_level(phi_g[n4.x], level, side);
        f[1] = sm_level(phi_g[n4.y], level, side);
        f[2] = sm_level(phi_g[n4.z], level, side);
        f[3] = sm_level(phi_g[n4.w], level, side);
        int ei[4], ej[4];
        sm_edges(mask, ei, ej);
        const bool swap = (((SM_SWAP >> mask) & 1u) != 0u) != ((c & 16) != 0);
        // the corners (0, 1, 2), of a quad's second triangle (0, 2, 3); then the swap of the second and third
        const int c1 = second ? 2 : 1, c2 = second ? 3 : 2;
        const int corner[3] = {0, swap ? c2 : c1, swap ? c1 : c2};
        double P[9];
        I id[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int cq = corner[q];
            const int i = cq == 0 ? ei[0] : cq == 1 ? ei[1] : cq == 2 ? ei[2] : ei[3];
            const int j = cq == 0 ? ej[0] : cq == 1 ? ej[1] : cq == 2 ? ej[2] : ej[3];
            lf_cross_point(x, f, i, j, P + 3 * q);
            id[q] = sm_find(ukey, nv, sm_key(sm_pick_node(n4, i), sm_pick_node(n4, j), bits));
        }
        tris[3 * k] = id[0];
        tris[3 * k + 1] = id[1];
        tris[3 * k + 2] = id[2];
        double ab[3], ac[3], nrm[3];
        lf_sub(P + 3, P, ab);
        lf_sub(P + 6, P, ac);
        lf_cross(ab, ac, nrm);
        v[0] = 0.5 * sqrt(lf_dot(nrm, nrm));
    }
    block_tree_256<1>(v, MergeSum(), lds);
    if (threadIdx.x == 0) part[blockIdx.x] = v[0];
}

__global__ void sm_finish_kernel(const I* __restrict__ nv_ptr, I* __restrict__ cnt) {
    if (threadIdx.x == 0) cnt[SM_VERTS] = *nv_ptr;
}

int sm_bits(I N) {
    int b = 1;
    while (b < 31 && (1LL << b) < (long long)N) ++b;
    return b;
}

}  // namespace

extern "C" {

I dfl_surface_mesh_sort_block(void) {
    // rocprim sorts up to this many 8-byte keys in one workgroup and switches algorithm above it
    using cfg = rocprim::detail::radix_sort_block_sort_config_base<U64, rocprim::empty_type>::type;
    return (I)((cfg::block_size < 256u ? cfg::block_size : 256u) * (cfg::items_per_thread < 4u ? cfg::items_per_thread : 4u));
}

int64_t dfl_surface_mesh_temp_bytes(I N, I n) {
    size_t b = 0;
    (void)rocprim::radix_sort_keys(nullptr, b, (const U64*)nullptr, (U64*)nullptr, (size_t)(n > 0 ? n : 1), 0, 2 * sm_bits(N));
    return (int64_t)b + 16;
}

int dfl_surface_mesh_count(I N, I NT, const I* ien, const T* xg, const T* w, const dfl_surface_mesh_params* prm,
                           unsigned char* code, I* count, I* start, I* chunk_sum, dfl_surface_mesh_totals* tot, void* stream) {
    if (N <= 0 || NT <= 0) return 0;
    hipStream_t s = S(stream);
    const int nblk = ceil_div(NT, SM_BLK);
    const T* phi = w + 4LL * N;
    DFL_GUARD(hipMemsetAsync(tot, 0, sizeof *tot, s));
    sm_bad_nodes_kernel<<<ceil_div(N, SM_BLK), SM_BLK, 0, s>>>(N, phi, tot->count);
    sm_classify_kernel<<<nblk, SM_BLK, 0, s>>>(NT, ien, xg, phi, N, prm->level, prm->side, code, nblk, count, tot->count);
    dfl_scan_counts(2 * nblk, count, chunk_sum, start, stream);
    sm_counts_kernel<<<1, 64, 0, s>>>(start, nblk, tot->count);
    DFL_LAUNCH_CHECK();
    return 5;
}

int dfl_surface_mesh_build(I N, I NT, const I* ien, const T* xg, const T* w, const dfl_surface_mesh_params* prm,
                           const unsigned char* code, const I* start, I nt, I nkeys, uint64_t* key, uint64_t* key_out, I capk,
                           void* temp, int64_t temp_bytes, I* kcount, I* kbase, I* kchunk, const T* const* fields, I num_fields,
                           T* verts, I* edge, T* t, T* vals, I* tris, I* tri_tet, I capt, T* part, dfl_surface_mesh_totals* tot,
                           void* stream) {
    if (N <= 0 || NT <= 0 || nt <= 0 || nkeys <= 0) return 0;
    if (nt > capt || nkeys > capk || num_fields < 0 || num_fields > DFL_SURFACE_MESH_MAX_FIELDS ||
        dfl_surface_mesh_temp_bytes(N, nkeys) > temp_bytes) {  // (never: the host sized everything)
        DFL_GUARD(hipErrorInvalidValue);
        return 0;
    }
    hipStream_t s = S(stream);
    const int nblk = ceil_div(NT, SM_BLK), nkb = ceil_div(nkeys, SM_BLK), ntb = ceil_div(nt, SM_BLK);
    const int bits = sm_bits(N);
    const T* phi = w + 4LL * N;
    SmFields fl;
    for (int q = 0; q < DFL_SURFACE_MESH_MAX_FIELDS; ++q) fl.q[q] = q < num_fields ? fields[q] : nullptr;
    sm_emit_kernel<<<nblk, SM_BLK, 0, s>>>(NT, ien, code, start, nblk, bits, (U64*)key, capk, tri_tet, capt);
    DFL_LAUNCH_CHECK();
    size_t bytes = (size_t)temp_bytes;
    DFL_GUARD(rocprim::radix_sort_keys(temp, bytes, (U64*)key, (U64*)key_out, (size_t)nkeys, 0, 2 * bits, s));
    sm_head_count_kernel<<<nkb, SM_BLK, 0, s>>>(nkeys, (const U64*)key_out, kcount);
    dfl_scan_counts(nkb, kcount, kchunk, kbase, stream);
    // the unsorted keys are dead: their buffer takes the unique list
    sm_vertex_kernel<<<nkb, SM_BLK, 0, s>>>(nkeys, (const U64*)key_out, kbase, bits, xg, phi, prm->level, prm->side, fl,
                                            (int)num_fields, (U64*)key, verts, edge, t, vals, capk);
    sm_tri_kernel<<<ntb, SM_BLK, 0, s>>>(nt, tri_tet, ien, code, xg, phi, prm->level, prm->side, (const U64*)key, kbase + nkb,
                                         capk, bits, tris, part);
    block_reduce<1>(ntb, part, &tot->area, MergeSum(), stream);
    sm_finish_kernel<<<1, 64, 0, s>>>(kbase + nkb, tot->count);
    DFL_LAUNCH_CHECK();
    return 9;  // (the sort counts as one)
}

}  // extern "C"
