// Porosity record for gfx950: the connected components of the gas region {side (phi - level) <= 0} over the mesh graph, which
// of them touch the atmosphere, and per closed component (a pore) its volume, box and wall temperatures (build-defined; model
// in include/dedflow.h, "porosity record").  Passive: the state w is read and never written.
//
//   por_init_kernel        the max_pores rows get their empty values (sums 0, minima +inf, maxima -inf), the counters 0
//   por_classify_kernel    one thread per node: parent[a] = a for gas, -1 for metal, -2 for a phi that is not finite (counted)
//   por_hook_kernel        one thread per tet: a lock-free union-find over parent[] joins the gas nodes of a tet without a bad
//                          node.  find walks the parents with pointer halving; unite hooks the larger root under the smaller
//                          with a compare-and-swap and, when it lost, goes on from the value the CAS returned.  Every access
//                          to parent[] in this launch is an agent-scope relaxed atomic.
//   por_flatten_kernel     one thread per node, the next launch, plain loads: label[a] = the root = the component's minimum
//   por_open_kernel        one thread per boundary face of the open groups: open[label] = 1 at the face's gas nodes
//   por_root_count / emit  count -> scan (k_scan.hip) -> emit over the nodes: the pore roots in ascending id get their rank,
//                          and row rank its label; the components are counted on the way
//   por_node_kernel        one thread per node: pore[a] = the rank of its pore; nodes and the box of its row (integer atomics)
//   por_tet_kernel         one thread per tet: the metal, open and pore volumes through block_tree_256 to [workgroup][3], the
//                          bad tets counted, the closed tets counted per workgroup for the second count -> scan -> emit
//   por_counts_kernel      pores and closed tets beside the other counters: one read-back carries all of them
//   por_tet_emit_kernel    the keys (rank << 32 | tet) of the closed tets in ascending tet id; rocprim's radix sort of the whole
//                          keys, which are distinct: ascending rank, ascending tet ids inside every run, in one possible order
//   por_eval_kernel        one thread per sorted key: the tet's gas volume and |det| / 6 into vals; crossing points into the
//                          box and the metal nodes' T into the extremes of its row (ordered-bit integer atomics)
//   por_sum_kernel         the head of every run sums its run from +0.0 in order and counts it: it owns the row's sums
//
// Why the union-find ends and is right in every interleaving: parent[a] <= a holds for a gas node at every moment (classify
// writes a; a hook writes lo < hi at a root hi; halving writes a grandparent, which is smaller still), so every walk visits
// strictly decreasing ids, and the two roots a failed CAS goes on from are smaller than the one it failed on.  No thread waits
// for another: a CAS that fails means another thread wrote a smaller parent.  A root is only ever changed by a CAS that
// expects the root itself, and that CAS acts on the one copy of the word at the memory side; a load may return an older value
// of a word, which is an ancestor-or-equal in the same set then as now and at worst lengthens the walk or fails a CAS.  The
// agent scope is what makes the loads reach beyond the reading CU's L1, which no other CU's store ever refreshes.
//
// No float atomics: every sum has a fixed order.  Integer atomics carry counts and extremes, which no order changes.  The file
// is compiled without fused multiply-add, as level_facets.hpp is wherever it is included.
#include "block_ops.hpp"
#include "level_facets.hpp"
#include <cstring>
#include <rocprim/rocprim.hpp>

#pragma clang fp contract(off)

namespace {

constexpr int PO_BLK = BLOCK_OPS_BLK;
constexpr int PO_NVOL = 3;  // metal, open, pores
enum { PO_COMPONENTS = 0, PO_PORES = 1, PO_CLOSED = 2, PO_BAD_NODES = 3, PO_BAD_TETS = 4 };
enum { PO_METAL = -1, PO_BAD = -2 };
typedef unsigned long long U64;

// a double as an unsigned integer of the same order (-inf lowest); a NaN is never encoded
__device__ __forceinline__ U64 po_key(double v) {
    const U64 u = (U64)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
// a NaN never wins
__device__ __forceinline__ void po_min(U64* cell, double v) { if (v == v) atomicMin(cell, po_key(v)); }
__device__ __forceinline__ void po_max(U64* cell, double v) { if (v == v) atomicMax(cell, po_key(v)); }

__global__ __launch_bounds__(PO_BLK) void por_init_kernel(I max_pores, dfl_pore_row* __restrict__ rows, dfl_porosity_totals* __restrict__ tot) {
    const long long r = (long long)blockIdx.x * PO_BLK + threadIdx.x;
    if (r < DFL_POROSITY_NCOUNT) tot->count[r] = 0;
    if (r >= max_pores) return;
    dfl_pore_row row;
    row.label = -1; row.nodes = 0; row.tets = 0; row.pad = 0;
    row.volume = 0.0; row.volume_scale = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) row.ext[k] = (k < 3 || k == 6) ? po_key(HUGE_VAL) : po_key(-HUGE_VAL);
    rows[r] = row;
}

__global__ __launch_bounds__(PO_BLK) void por_classify_kernel(I N, const T* __restrict__ phi, double level, double side,
                                                               I* __restrict__ parent, I* __restrict__ open, I* __restrict__ cnt) {
    __shared__ int s_cnt[4];
    const long long a = (long long)blockIdx.x * PO_BLK + threadIdx.x;
    int bad = 0;
    if (a < N) {
        const double ph = phi[a];
        double f = ph - level;
        if (side < 0.0) f = -f;
        bad = !(fabs(ph) < HUGE_VAL);  // NaN or infinite
        parent[a] = bad ? PO_BAD : (f > 0.0 ? PO_METAL : (I)a);
        open[a] = 0;
    }
    block_count_256(bad, s_cnt);
    __syncthreads();
    if (threadIdx.x == 0) {
        const int n = block_count_read(s_cnt);
        if (n) atomicAdd(cnt + PO_BAD_NODES, n);
    }
}

// ---- the union-find of the hook launch: agent-scope relaxed atomics only ---------------------------------------------------------
__device__ __forceinline__ I po_load(I* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// true when *p was `expect` and is now v; otherwise expect holds what *p was
__device__ __forceinline__ bool po_cas(I* p, I& expect, I v) {
    return __hip_atomic_compare_exchange_strong(p, &expect, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root above gas node x as far as this thread can see.  p is a parent of x that was read: p <= x, and the walk goes on only
// while p < x, so the ids it visits fall strictly (a value outside 0 .. x - 1 ends it).  On the way x's parent becomes its
// grandparent unless somebody changed it meanwhile
__device__ __forceinline__ I po_find(I* parent, I x) {
    I p = po_load(parent + x);
    while ((unsigned)p < (unsigned)x) {
        const I gp = po_load(parent + p);
        if ((unsigned)gp >= (unsigned)p) return p;  // p is a root
        I expect = p;
        po_cas(parent + x, expect, gp);
        x = p;
        p = gp;
    }
    return x;
}

// joins the sets of gas nodes a and b: the larger root goes under the smaller.  A CAS that lost returns the parent somebody
// gave that root, which is smaller than the root: the larger of the two roots falls strictly from one round to the next
__device__ __forceinline__ void po_unite(I* parent, I a, I b) {
    I ra = po_find(parent, a), rb = po_find(parent, b);
    while (ra != rb) {
        const I hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
        I expect = hi;
        if (po_cas(parent + hi, expect, lo)) return;
        if ((unsigned)expect >= (unsigned)hi) return;  // (never: a parent is below its node)
        ra = po_find(parent, expect);
        rb = po_find(parent, lo);
    }
}

__global__ __launch_bounds__(PO_BLK) void por_hook_kernel(I NT, const I* __restrict__ ien, I N, I* parent) {
    const long long e = (long long)blockIdx.x * PO_BLK + threadIdx.x;
    if (e >= NT) return;
    const int4 n4 = reinterpret_cast<const int4*>(ien)[e];
    const I nd[4] = {n4.x, n4.y, n4.z, n4.w};
    I first = -1;
    int ngas = 0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        if ((unsigned)nd[a] >= (unsigned)N) return;  // (never: ien holds node ids)
        const I p = po_load(parent + nd[a]);
        if (p == PO_BAD) return;  // a tet with a bad node joins nothing
        if (p >= 0) {
            if (first < 0) first = nd[a];
            ++ngas;
        }
    }
    if (ngas < 2) return;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const I p = po_load(parent + nd[a]);  // (a code never changes: >= 0 still means gas)
        if (p >= 0 && nd[a] != first) po_unite(parent, first, nd[a]);
    }
}

// the launch after the hooks: parent[] is final and read plainly
__global__ __launch_bounds__(PO_BLK) void por_flatten_kernel(I N, const I* __restrict__ parent, I* __restrict__ label) {
    const long long a = (long long)blockIdx.x * PO_BLK + threadIdx.x;
    if (a >= N) return;
    I x = (I)a, p = parent[a];
    if (p >= 0) {
        while ((unsigned)p < (unsigned)x) {
            x = p;
            p = parent[x];
        }
        p = x;
    }
    label[a] = p;
}

__global__ __launch_bounds__(PO_BLK) void por_open_kernel(I nof, const I* __restrict__ oface, const I* __restrict__ f2e,
                                                           const I* __restrict__ forn, I NT, const I* __restrict__ ien,
                                                           const I* __restrict__ label, I* __restrict__ open) {
    const long long i = (long long)blockIdx.x * PO_BLK + threadIdx.x;
    if (i >= nof) return;
    const I f = oface[i];
    const I e = f2e[f], o = forn[f];
    if ((unsigned)e >= (unsigned)NT) return;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        if (a == o) continue;
        const I l = label[ien[4LL * e + a]];
        if (l >= 0) open[l] = 1;
    }
}

__device__ __forceinline__ bool po_is_pore_root(long long a, I N, const I* __restrict__ label, const I* __restrict__ open) {
    return a < N && label[a] == (I)a && !open[a];
}

__global__ __launch_bounds__(PO_BLK) void por_root_count_kernel(I N, const I* __restrict__ label, const I* __restrict__ open,
                                                                 I* __restrict__ count, I* __restrict__ cnt) {
    __shared__ int s_pore[4], s_comp[4];
    const long long a = (long long)blockIdx.x * PO_BLK + threadIdx.x;
    block_count_256(po_is_pore_root(a, N, label, open) ? 1 : 0, s_pore);
    block_count_256((a < N && label[a] == (I)a) ? 1 : 0, s_comp);
    __syncthreads();
    if (threadIdx.x == 0) {
        count[blockIdx.x] = block_count_read(s_pore);
        const int n = block_count_read(s_comp);
        if (n) atomicAdd(cnt + PO_COMPONENTS, n);
    }
}

__global__ __launch_bounds__(PO_BLK) void por_root_emit_kernel(I N, const I* __restrict__ label, const I* __restrict__ open,
                                                                const I* __restrict__ base, I* __restrict__ rank,
                                                                dfl_pore_row* __restrict__ rows, I max_pores) {
    __shared__ int s_scan[PO_BLK];
    const long long a = (long long)blockIdx.x * PO_BLK + threadIdx.x;
    const int root = po_is_pore_root(a, N, label, open) ? 1 : 0;
    const int incl = block_scan_incl_256(root, s_scan);
    if (!root) return;  // (after the last barrier)
    const I r = base[blockIdx.x] + (incl - 1);
    rank[a] = r;
    if (r < max_pores) rows[r].label = (I)a;
}

__global__ __launch_bounds__(PO_BLK) void por_node_kernel(I N, const I* __restrict__ label, const I* __restrict__ open,
                                                           const I* __restrict__ rank, const T* __restrict__ xg,
                                                           I* __restrict__ pore, dfl_pore_row* rows, I max_pores) {
    const long long a = (long long)blockIdx.x * PO_BLK + threadIdx.x;
    if (a >= N) return;
    const I l = label[a];
    if (l < 0 || open[l]) {
        pore[a] = -1;
        return;
    }
    const I r = rank[l];
    pore[a] = r;
    if (r >= max_pores) return;
    atomicAdd(&rows[r].nodes, 1);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double x = xg[3 * a + d];
        po_min((U64*)&rows[r].ext[d], x);
        po_max((U64*)&rows[r].ext[3 + d], x);
    }
}

// f_a = phi_a - level, negated for side = -1
__device__ __forceinline__ void po_levels(const int4 n4, const T* __restrict__ phi_g, double level, double side, double* f) {
    double phi[4];
    lf_levels(n4, phi_g, level, phi, f);
    if (side < 0.0) {
#pragma unroll
        for (int a = 0; a < 4; ++a) f[a] = -f[a];
    }
}

// the labels of a tet's nodes; -1: a bad node among them, 0: four metal nodes, 1: gas nodes, comp = their component
__device__ __forceinline__ int po_tet_class(const int4 n4, const I* __restrict__ label, I& comp) {
    const I l[4] = {label[n4.x], label[n4.y], label[n4.z], label[n4.w]};
    comp = -1;
    int cls = 0;
#pragma unroll
    for (int a = 3; a >= 0; --a) {
        if (l[a] == PO_BAD) return -1;
        if (l[a] >= 0) {
            comp = l[a];
            cls = 1;
        }
    }
    return cls;
}

// the tet's |det| / 6, the metal volume in it and the gas volume |det| / 6 - metal; a NaN adds 0
__device__ __forceinline__ void po_tet_volumes(const double* x, const double* f, double& full, double& metal, double& gas) {
    TetCross c;
    tet_cross(x, c);
    full = fabs(c.det) / 6.0;
    const double pv = lf_positive_volume(x, f, lf_positive_mask(f), c.det);
    metal = pv == pv ? pv : 0.0;
    const double g = full - pv;
    gas = g == g ? g : 0.0;
}

__global__ __launch_bounds__(PO_BLK) void por_tet_kernel(I NT, const I* __restrict__ ien, const T* __restrict__ xg,
                                                          const T* __restrict__ w, I N, double level, double side,
                                                          const I* __restrict__ label, const I* __restrict__ open,
                                                          I* __restrict__ count, T* __restrict__ part, I* __restrict__ cnt) {
    __shared__ double lds[4][PO_NVOL];
    __shared__ int s_closed[4], s_bad[4];
    const long long e = (long long)blockIdx.x * PO_BLK + threadIdx.x;
    double v[PO_NVOL] = {0.0, 0.0, 0.0};
    int closed = 0, bad = 0;
    if (e < NT) {
        const int4 n4 = reinterpret_cast<const int4*>(ien)[e];
        I comp;
        const int cls = po_tet_class(n4, label, comp);
        bad = cls < 0;
        if (!bad) {
            double x[12], f[4], full, metal, gas;
            lf_gather_tet(n4, xg, x);
            po_levels(n4, w + 4LL * N, level, side, f);
            po_tet_volumes(x, f, full, metal, gas);
            v[0] = metal;
            if (cls == 1) {
                closed = !open[comp];
                v[closed ? 2 : 1] = gas;
            }
        }
    }
    block_count_256(closed, s_closed);
    block_count_256(bad, s_bad);
    block_tree_256<PO_NVOL>(v, MergeSum(), lds);  // (its barrier also publishes the counts)
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < PO_NVOL; ++j) part[(long long)PO_NVOL * blockIdx.x + j] = v[j];
        count[blockIdx.x] = block_count_read(s_closed);
        const int n = block_count_read(s_bad);
        if (n) atomicAdd(cnt + PO_BAD_TETS, n);
    }
}

__global__ void por_counts_kernel(const I* __restrict__ node_total, const I* __restrict__ tet_total, I* __restrict__ cnt) {
    if (threadIdx.x == 0) cnt[PO_PORES] = *node_total;
    if (threadIdx.x == 1) cnt[PO_CLOSED] = *tet_total;
}

__global__ __launch_bounds__(PO_BLK) void por_tet_emit_kernel(I NT, const I* __restrict__ ien, const I* __restrict__ label,
                                                               const I* __restrict__ open, const I* __restrict__ pore,
                                                               const I* __restrict__ base, U64* __restrict__ key, I cap) {
    __shared__ int s_scan[PO_BLK];
    const long long e = (long long)blockIdx.x * PO_BLK + threadIdx.x;
    int closed = 0;
    I r = 0;
    if (e < NT) {
        const int4 n4 = reinterpret_cast<const int4*>(ien)[e];
        I comp;
        if (po_tet_class(n4, label, comp) == 1 && !open[comp]) {
            closed = 1;
            r = pore[comp];  // the root is a node of its pore
        }
    }
    const int incl = block_scan_incl_256(closed, s_scan);
    if (!closed) return;  // (after the last barrier)
    const long long id = (long long)base[blockIdx.x] + (incl - 1);
    if (id < cap) key[id] = (U64)(unsigned)r << 32 | (U64)(unsigned)e;  // (always: the host sized the list)
}

__global__ __launch_bounds__(PO_BLK) void por_eval_kernel(I n, const U64* __restrict__ key, const I* __restrict__ ien,
                                                           const T* __restrict__ xg, const T* __restrict__ w, I N, double level,
                                                           double side, T* __restrict__ vals, dfl_pore_row* rows, I max_pores) {
    const long long p = (long long)blockIdx.x * PO_BLK + threadIdx.x;
    if (p >= n) return;
    const U64 k = key[p];
    const I e = (I)(unsigned)k, r = (I)(k >> 32);
    const int4 n4 = reinterpret_cast<const int4*>(ien)[e];
    const long long nd[4] = {n4.x, n4.y, n4.z, n4.w};
    double x[12], f[4], full, metal, gas;
    lf_gather_tet(n4, xg, x);
    po_levels(n4, w + 4LL * N, level, side, f);
    po_tet_volumes(x, f, full, metal, gas);
    vals[2 * p] = gas;
    vals[2 * p + 1] = full;
    if (r >= max_pores) return;
    const int mask = lf_positive_mask(f);
    U64* ext = (U64*)rows[r].ext;
    const T* Tg = w + 5LL * N;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (!((mask >> j) & 1)) continue;  // j metal
        const double Tj = Tg[nd[j]];
        po_min(ext + 6, Tj);
        po_max(ext + 7, Tj);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if ((mask >> i) & 1) continue;  // i gas: the crossing point of the edge from i to j
            double P[3];
            lf_cross_point(x, f, i, j, P);
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                po_min(ext + d, P[d]);
                po_max(ext + 3 + d, P[d]);
            }
        }
    }
}

__global__ __launch_bounds__(PO_BLK) void por_sum_kernel(I n, const U64* __restrict__ key, const T* __restrict__ vals,
                                                          dfl_pore_row* __restrict__ rows, I max_pores) {
    const long long p = (long long)blockIdx.x * PO_BLK + threadIdx.x;
    if (p >= n) return;
    const I r = (I)(key[p] >> 32);
    if (r >= max_pores || (p > 0 && (I)(key[p - 1] >> 32) == r)) return;  // not the head of a listed run
    double vol = 0.0, scale = 0.0;
    I tets = 0;
    for (long long q = p; q < n && (I)(key[q] >> 32) == r; ++q) {
        vol = vol + vals[2 * q];
        scale = scale + vals[2 * q + 1];
        ++tets;
    }
    rows[r].volume = vol;
    rows[r].volume_scale = scale;
    rows[r].tets = tets;
}

}  // namespace

extern "C" {

int64_t dfl_porosity_temp_bytes(I n) {
    size_t b = 0;
    (void)rocprim::radix_sort_keys(nullptr, b, (const U64*)nullptr, (U64*)nullptr, (size_t)(n > 0 ? n : 1), 0, 64);
    return (int64_t)b + 16;
}

int dfl_porosity_label(I N, I NT, const I* ien, const T* w, const dfl_porosity_params* prm, I nof, const I* oface, const I* f2e,
                       const I* forn, I* parent, I* label, I* open, dfl_pore_row* rows, dfl_porosity_totals* tot, void* stream) {
    if (N <= 0) return 0;
    hipStream_t s = S(stream);
    int launches = 4;
    const int need = prm->max_pores > DFL_POROSITY_NCOUNT ? prm->max_pores : DFL_POROSITY_NCOUNT;
    por_init_kernel<<<ceil_div(need, PO_BLK), PO_BLK, 0, s>>>(prm->max_pores, rows, tot);
    por_classify_kernel<<<ceil_div(N, PO_BLK), PO_BLK, 0, s>>>(N, w + 4LL * N, prm->level, prm->side, parent, open, tot->count);
    por_hook_kernel<<<ceil_div(NT > 0 ? NT : 1, PO_BLK), PO_BLK, 0, s>>>(NT, ien, N, parent);
    por_flatten_kernel<<<ceil_div(N, PO_BLK), PO_BLK, 0, s>>>(N, parent, label);
    if (nof > 0) {
        por_open_kernel<<<ceil_div(nof, PO_BLK), PO_BLK, 0, s>>>(nof, oface, f2e, forn, NT, ien, label, open);
        ++launches;
    }
    DFL_LAUNCH_CHECK();
    return launches;
}

int dfl_porosity_rank(I N, const T* xg, const dfl_porosity_params* prm, const I* label, const I* open, I* count, I* base,
                      I* chunk_sum, I* rank, I* pore, dfl_pore_row* rows, dfl_porosity_totals* tot, void* stream) {
    if (N <= 0) return 0;
    hipStream_t s = S(stream);
    const int nblk = ceil_div(N, PO_BLK);
    por_root_count_kernel<<<nblk, PO_BLK, 0, s>>>(N, label, open, count, tot->count);
    dfl_scan_counts(nblk, count, chunk_sum, base, stream);
    por_root_emit_kernel<<<nblk, PO_BLK, 0, s>>>(N, label, open, base, rank, rows, prm->max_pores);
    por_node_kernel<<<nblk, PO_BLK, 0, s>>>(N, label, open, rank, xg, pore, rows, prm->max_pores);
    DFL_LAUNCH_CHECK();
    return 5;
}

int dfl_porosity_tets(I NT, const I* ien, const T* xg, const T* w, I N, const dfl_porosity_params* prm, const I* label,
                      const I* open, I nblk_node, const I* node_base, I* count, I* base, I* chunk_sum, T* part,
                      dfl_porosity_totals* tot, void* stream) {
    if (NT <= 0 || N <= 0) return 0;
    hipStream_t s = S(stream);
    const int nblk = ceil_div(NT, PO_BLK);
    por_tet_kernel<<<nblk, PO_BLK, 0, s>>>(NT, ien, xg, w, N, prm->level, prm->side, label, open, count, part, tot->count);
    dfl_scan_counts(nblk, count, chunk_sum, base, stream);
    block_reduce<PO_NVOL>(nblk, part, tot->volume, MergeSum(), stream);
    por_counts_kernel<<<1, 64, 0, s>>>(node_base + nblk_node, base + nblk, tot->count);
    DFL_LAUNCH_CHECK();
    return 5;
}

int dfl_porosity_pores(I NT, const I* ien, const T* xg, const T* w, I N, const dfl_porosity_params* prm, const I* label,
                       const I* open, const I* pore, const I* base, I nclosed, uint64_t* key, uint64_t* key_out, I cap, T* vals,
                       void* temp, int64_t temp_bytes, dfl_pore_row* rows, void* stream) {
    if (NT <= 0 || N <= 0) return 0;
    hipStream_t s = S(stream);
    const I n = nclosed < cap ? nclosed : cap;
    por_tet_emit_kernel<<<ceil_div(NT, PO_BLK), PO_BLK, 0, s>>>(NT, ien, label, open, pore, base, (U64*)key, cap);
    DFL_LAUNCH_CHECK();
    if (n > 0) {
        size_t bytes = (size_t)temp_bytes;
        if (dfl_porosity_temp_bytes(n) > temp_bytes) {  // (never: the host sized temp for cap >= n keys)
            DFL_GUARD(hipErrorInvalidValue);
            return 1;
        }
        DFL_GUARD(rocprim::radix_sort_keys(temp, bytes, (U64*)key, (U64*)key_out, (size_t)n, 0, 64, s));
    }
    const int grid = ceil_div(n > 0 ? n : 1, PO_BLK);
    por_eval_kernel<<<grid, PO_BLK, 0, s>>>(n, (const U64*)key_out, ien, xg, w, N, prm->level, prm->side, vals, rows, prm->max_pores);
    por_sum_kernel<<<grid, PO_BLK, 0, s>>>(n, (const U64*)key_out, vals, rows, prm->max_pores);
    DFL_LAUNCH_CHECK();
    return 4;  // (the sort counts as one)
}

}  // extern "C"
