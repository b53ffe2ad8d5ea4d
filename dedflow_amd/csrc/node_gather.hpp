// The node gather over the sorted V2E map (one per mesh, host/mesh.c: every node's tets in ascending tet id), shared by the
// free-surface pass (k_surface.hip), the phase-change pass (k_phase.hip), the thermal-material rows (k_thermal.hip), the
// solidification record's gradient over a node list (k_solidify.hip) and, for its shape and trip count, the scalar Jacobian rows
// (k_scalar.hip).
//
// A group of NG_LANES = 16 lanes owns node a (NG_ROWS = 16 nodes per 256-thread workgroup; a Kuhn-cube interior node has 24
// tets: two trips).  Lane j of the group takes tet j of a's list and evaluates the NC values of its own node, or leaves
// early with nothing.  The values are parked in LDS and lanes 0 .. NC-1 of the group each own one of the NC sums and add the
// parked values in list order.  More than 16 tets per node: more trips.
//
// Why the result is bitwise reproducible and independent of the assembly schedule:
//   - no atomics, and every output is written once by the lane that owns it (no zero pass);
//   - the summation order is fixed: ascending tet id, starting from +0.0.  A tet that left parks +0.0, and a trip in which
//     no lane of the wave stays is skipped altogether; for a sum that started at +0.0 and whose skipped terms are all +0.0
//     that is the same bits as adding them;
//   - the four groups of a wave take the same number of trips (wave_max) and the hand-over branch is taken on __any, so it
//     is wave-uniform and the two WAVE_SYNCs inside it are barriers every lane of the wave reaches: the first orders the
//     parking before the sums, the second the sums before the next trip overwrites the parked values.  A group's LDS slots
//     are written and read by its own wave only, so no workgroup barrier is needed.
#pragma once
#include "asm_device.hpp"
#include "tet_levelset.hpp"

namespace {

constexpr int NG_BLK = 256;
constexpr int NG_LANES = 16;                // lanes per node
constexpr int NG_ROWS = NG_BLK / NG_LANES;  // nodes per workgroup

__device__ __forceinline__ int wave_max(int v) {  // the node groups of one wave share trips
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, WAVE));
    return v;
}

// f at quadrature point q of the assembly's four-point rule, in this association
__device__ __forceinline__ double interp_q(int q, const double* f) {
#pragma clang fp contract(off)
    return ((shl(0, q) * f[0] + shl(1, q) * f[1]) + shl(2, q) * f[2]) + shl(3, q) * f[3];
}

struct NodeSum {
    I row;      // the node of this lane's group (0 when !live)
    bool live;  // row < N
    int g;      // lane within the group; with g < NC, acc is component g of the node
    double acc;
};

// eval(e, row, out[NC]) -> stays: the NC values of node `row` from tet e into out (which arrives as +0.0), false: the tet
// adds nothing.  The row-mapping form: the caller says which node this lane's group owns (the same for the 16 lanes of a
// group; !live: none) -- the k-th entry of a node list, say (k_solidify.hip).  It may be called again and again by the same
// workgroup: a group's parked values are consumed before the call returns.  NG_BLK threads; NC * NG_BLK * 8 bytes of LDS.
template <int NC, class Eval>
__device__ __forceinline__ NodeSum node_gather_row(I row, bool live, const I* __restrict__ vrow, const I* __restrict__ vcol,
                                                   Eval eval) {
    __shared__ double s_val[NC][NG_BLK];
    const int t = threadIdx.x;
    const int gbase = t & ~(NG_LANES - 1);
    NodeSum r;
    r.g = t & (NG_LANES - 1);
    r.live = live;
    r.row = r.live ? row : 0;
    r.acc = 0.0;
    const I e0 = r.live ? vrow[r.row] : 0, ne = r.live ? vrow[r.row + 1] - e0 : 0;
    const int ne_w = wave_max(ne);
    for (int jc = 0; jc < ne_w; jc += NG_LANES) {
        const int j = jc + r.g;
        bool stays = false;
        double out[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) out[c] = 0.0;
        if (j < ne) stays = eval(vcol[e0 + j], r.row, out);
        if (__any(stays)) {  // the same in every lane of the wave: the hand-over below is a wave barrier
#pragma unroll
            for (int c = 0; c < NC; ++c) s_val[c][t] = out[c];
            WAVE_SYNC();
            const int nj = min(NG_LANES, (int)ne - jc);
            if (r.g < NC)
                for (int jj = 0; jj < nj; ++jj) r.acc += s_val[r.g][gbase + jj];  // V2E order: ascending tet id
            WAVE_SYNC();  // the parked values are consumed before the next trip overwrites them
        }
    }
    return r;
}

// the form of the passes over all nodes: group t / NG_LANES of workgroup b owns node b * NG_ROWS + t / NG_LANES.  Launch with
// NG_BLK threads and ceil(N / NG_ROWS) workgroups
template <int NC, class Eval>
__device__ __forceinline__ NodeSum node_gather_sum(I N, const I* __restrict__ vrow, const I* __restrict__ vcol, Eval eval) {
    const long long row_ll = (long long)blockIdx.x * NG_ROWS + threadIdx.x / NG_LANES;
    return node_gather_row<NC>((I)row_ll, row_ll < N, vrow, vcol, eval);
}

}  // namespace
