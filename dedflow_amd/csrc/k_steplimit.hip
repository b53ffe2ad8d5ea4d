// Time-step limits for gfx950 (include/dedflow.h, "time step"): per tet the advective rate r_e = max_a |ubar . grad N_a|, the
// inverse squared altitude m_e = max_a |grad N_a|^2 and, on the tets the surface phi = level cuts, the capillary quantity
// q_e = sigma_e m_e sqrt(m_e); over the mesh the three maxima, the lowest tet id that attains each, and two counts.
//
//   step_limit_partials_kernel   one pass over the tets in id order, a grid-stride loop over 256-tet workgroups: thread t of
//                                workgroup b takes tets 256 (b + k grid) + t, k = 0, 1, ..., ascending, and keeps per maximum its
//                                largest value and the first (lowest) tet that gave it.  The workgroup's result goes through
//                                the fixed tree of block_ops.hpp twice: the maxima and the counts, then -- against the finished
//                                maxima -- the lowest id among the threads that hold them.
//   step_limit_finish_kernel     one workgroup, the same two trees over the partials.
//
// No floating-point atomics, no atomics at all: a maximum is exact in any order and "the lowest tet id that attains it" does
// not depend on the order either, so the result is bitwise reproducible and independent of the grid.  Inside a workgroup
// an absent candidate carries the value -1 (every real one is >= 0) and the id -1; it is written out as (0, -1).
//
// Every per-tet formula is written operation by operation with fused multiply-add off (tests/timestep_model.py restates them in
// numpy and the launcher is compared bit for bit).  HBM view: the tet's ien line (16 B) and per vertex 3 coordinates, 3 velocities,
// phi and T gathered through L2 (64 B): the volume-correction classify pass gathers 32 B per vertex.
#include "block_ops.hpp"
#include "tet_levelset.hpp"

namespace {

constexpr int SL_NV = 3;  // rate_adv, rate_adv_surface, cap_q
constexpr int SL_NI = 5;  // tet_adv, tet_surface, tet_cap, num_cut, num_nonfinite
constexpr int SL_MAX_GRID = 2048;
constexpr double SL_NO_ID = 4294967296.0;  // above every tet id: what a thread that does not hold the maximum offers to the min tree

struct MergeMaxSum {  // components 0..2: max (a NaN never gets here), 3..4: sum
    __device__ __forceinline__ double operator()(int j, double a, double b) const { return j < SL_NV ? (b > a ? b : a) : a + b; }
    __device__ __forceinline__ double identity(int j) const { return j < SL_NV ? -1.0 : 0.0; }
};
struct MergeMin {
    __device__ __forceinline__ double operator()(int, double a, double b) const { return b < a ? b : a; }
    __device__ __forceinline__ double identity(int) const { return SL_NO_ID; }
};

__device__ __forceinline__ bool finite_d(double v) { return fabs(v) <= 1.7976931348623157e308; }  // false for NaN and +-inf

// a candidate (v, id) into the running (best, best_id): strictly larger wins, an equal value keeps the lower id
__device__ __forceinline__ void offer(double v, int id, double& best, int& best_id) {
    if (v > best || (v == best && id >= 0 && (best_id < 0 || id < best_id))) {
        best = v;
        best_id = id;
    }
}

// the workgroup's (best[3], id[3], cnt[2]) -> thread 0 writes out_v[3], out_i[5]
__device__ __forceinline__ void block_result(const double* best, const int* id, const double* cnt, double* out_v, int* out_i) {
    __shared__ double lds5[4][SL_NV + 2];
    __shared__ double lds3[4][SL_NV];
    __shared__ double s_max[SL_NV];
    double v[SL_NV + 2] = {best[0], best[1], best[2], cnt[0], cnt[1]};
    block_tree_256<SL_NV + 2>(v, MergeMaxSum{}, lds5);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < SL_NV; ++j) s_max[j] = v[j];
    }
    __syncthreads();
    double cand[SL_NV];
#pragma unroll
    for (int j = 0; j < SL_NV; ++j) cand[j] = (id[j] >= 0 && best[j] == s_max[j]) ? (double)id[j] : SL_NO_ID;
    block_tree_256<SL_NV>(cand, MergeMin{}, lds3);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < SL_NV; ++j) {
            out_i[j] = cand[j] < SL_NO_ID ? (int)cand[j] : -1;
            out_v[j] = out_i[j] < 0 ? 0.0 : v[j];  // absent: 0, which loses to every real candidate's id in offer()
        }
        out_i[3] = (int)v[3];
        out_i[4] = (int)v[4];
    }
}

// r_e, q_e and the two flags of one tet; returns false for a non-finite tet
__device__ __forceinline__ bool step_limit_tet(const int4 n4, I N, const T* __restrict__ xg, const T* __restrict__ w,
                                               const dfl_step_limit_params& p, double& r_e, double& q_e, bool& cut) {
#pragma clang fp contract(off)
    const long long n[4] = {n4.x, n4.y, n4.z, n4.w};
    double x[12], u[4][3], phi[4], Tn[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            x[a * 3 + d] = xg[n[a] * 3 + d];
            u[a][d] = w[n[a] * 3 + d];
        }
        phi[a] = w[4LL * N + n[a]];
        Tn[a] = w[5LL * N + n[a]];
    }
    TetCross c;
    tet_cross(x, c);
    double g[4][3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        g[1][d] = c.c23[d] / c.det;
        g[2][d] = c.c31[d] / c.det;
        g[3][d] = c.c12[d] / c.det;
        g[0][d] = -((g[1][d] + g[2][d]) + g[3][d]);
    }
    double ubar[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) ubar[d] = 0.25 * (((u[0][d] + u[1][d]) + u[2][d]) + u[3][d]);
    const double Tbar = 0.25 * (((Tn[0] + Tn[1]) + Tn[2]) + Tn[3]);
    double f[4];
    bool fin = finite_d(ubar[0]) && finite_d(ubar[1]) && finite_d(ubar[2]) && finite_d(Tbar);
    bool all_pos = true, all_neg = true;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        f[a] = phi[a] - p.level;
        fin = fin && finite_d(f[a]) && finite_d(g[a][0]) && finite_d(g[a][1]) && finite_d(g[a][2]);
        all_pos = all_pos && f[a] > 0.0;
        all_neg = all_neg && f[a] < 0.0;
    }
    if (!fin) return false;
    cut = !all_pos && !all_neg;
    double r = 0.0, m = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const double ca = fabs((ubar[0] * g[a][0] + ubar[1] * g[a][1]) + ubar[2] * g[a][2]);
        const double ma = (g[a][0] * g[a][0] + g[a][1] * g[a][1]) + g[a][2] * g[a][2];
        r = ca > r ? ca : r;
        m = ma > m ? ma : m;
    }
    const double s = p.sigma0 + p.dsigma_dT * (Tbar - p.T_ref);
    const double sigma = s > 0.0 ? s : 0.0;
    r_e = r;
    q_e = sigma * (m * sqrt(m));
    return true;
}

__global__ __launch_bounds__(BLOCK_OPS_BLK) void step_limit_partials_kernel(I T_, const I* __restrict__ ien, const T* __restrict__ xg,
                                                                             const T* __restrict__ w, I N,
                                                                             const dfl_step_limit_params p, T* __restrict__ part_v,
                                                                             I* __restrict__ part_i) {
    double best[SL_NV] = {-1.0, -1.0, -1.0}, cnt[2] = {0.0, 0.0};
    int id[SL_NV] = {-1, -1, -1};
    for (long long e = (long long)blockIdx.x * BLOCK_OPS_BLK + threadIdx.x; e < T_; e += (long long)gridDim.x * BLOCK_OPS_BLK) {
        double r_e, q_e;
        bool cut;
        if (!step_limit_tet(reinterpret_cast<const int4*>(ien)[e], N, xg, w, p, r_e, q_e, cut)) {
            cnt[1] += 1.0;
            continue;
        }
        offer(r_e, (int)e, best[0], id[0]);
        if (cut) {
            cnt[0] += 1.0;
            offer(r_e, (int)e, best[1], id[1]);
            if (q_e >= 0.0) offer(q_e, (int)e, best[2], id[2]);  // (0 inf = NaN for a tet with an overflowing m: it offers nothing)
        }
    }
    block_result(best, id, cnt, part_v + (long long)blockIdx.x * SL_NV, part_i + (long long)blockIdx.x * SL_NI);
}

__global__ __launch_bounds__(BLOCK_OPS_BLK) void step_limit_finish_kernel(I grid, const T* __restrict__ part_v, const I* __restrict__ part_i,
                                                                           T* __restrict__ out_v, I* __restrict__ out_i) {
    double best[SL_NV] = {-1.0, -1.0, -1.0}, cnt[2] = {0.0, 0.0};
    int id[SL_NV] = {-1, -1, -1};
    for (long long i = threadIdx.x; i < grid; i += BLOCK_OPS_BLK) {
#pragma unroll
        for (int j = 0; j < SL_NV; ++j) offer(part_v[i * SL_NV + j], part_i[i * SL_NI + j], best[j], id[j]);
        cnt[0] += (double)part_i[i * SL_NI + 3];
        cnt[1] += (double)part_i[i * SL_NI + 4];
    }
    block_result(best, id, cnt, out_v, out_i);
}

}  // namespace

extern "C" {

I dfl_step_limit_grid(I T_, I max_workgroups) {
    long long g = ((long long)T_ + BLOCK_OPS_BLK - 1) / BLOCK_OPS_BLK;
    const long long cap = max_workgroups > 0 ? max_workgroups : SL_MAX_GRID;
    if (g > cap) g = cap;
    return (I)(g < 1 ? 1 : g);
}

void dfl_step_limit_partials(I T_, const I* ien, const T* xg, const T* w, I N, const dfl_step_limit_params* prm, I grid, T* part_v,
                             I* part_i, void* stream) {
    if (grid <= 0) return;
    step_limit_partials_kernel<<<grid, BLOCK_OPS_BLK, 0, S(stream)>>>(T_, ien, xg, w, N, *prm, part_v, part_i);
    DFL_LAUNCH_CHECK();
}

void dfl_step_limit_finish(I grid, const T* part_v, const I* part_i, T* out_v, I* out_i, void* stream) {
    step_limit_finish_kernel<<<1, BLOCK_OPS_BLK, 0, S(stream)>>>(grid, part_v, part_i, out_v, out_i);
    DFL_LAUNCH_CHECK();
}

void dfl_step_limits(I T_, const I* ien, const T* xg, const T* w, I N, const dfl_step_limit_params* prm, I max_workgroups,
                     T* part_v, I* part_i, T* out_v, I* out_i, void* stream) {
    const I grid = dfl_step_limit_grid(T_, max_workgroups);
    dfl_step_limit_partials(T_, ien, xg, w, N, prm, grid, part_v, part_i, stream);
    dfl_step_limit_finish(grid, part_v, part_i, out_v, out_i, stream);
}

}  // extern "C"
