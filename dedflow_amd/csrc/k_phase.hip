// Melting and solidification for gfx950: the nodal drag coefficient D, latent heat capacity H and liquid volume G of the
// enthalpy-porosity model (build-defined: the reference has one phase; model in include/dedflow.h, "phase change"), their
// row updates of F, J and JT, and the melt-pool statistics.
//
//   phase_node_kernel   the node gather of node_gather.hpp with three sums per node (D_a, H_a, G_a).  A lane gathers its
//                       tet's ien line, the four T, the 4 x 24 B of coordinates (and with use_phi four phi), applies the
//                       skip rules and evaluates the three values of its own node at the four quadrature points.  Every
//                       term is >= +0.0.
//   phase_flag_kernel   one thread per tet: the skip rules once per tet instead of four times, one byte out (bit 0: adds to
//                       D / H, bit 1: adds to G).  The node pass then reads that byte first and a lane whose byte is 0
//                       leaves without gathering.  Optional (DFL_PHASE_FLAGS=1, host/phase.c): unlike the surface band most
//                       tets stay (the whole substrate is solid), and at bench size the pass costs more than it saves.
//   phase_apply_F / _J / _JT   one thread per node: F += D u and H dT; fact2 D on the (d, d) entries of the node's diagonal
//                       4x4 block, kALPHAM H on the diagonal of the scalar T Jacobian (the diagonal by binary search in the
//                       ascending col_ind row).  Products are rounded before the add.
//   phase_stats_*       two-stage fixed-order reduction over the nodes: block_tree_256, then block_reduce_kernel (block_ops.hpp).
//
// The skip rules decide what is evaluated, so both kernels must take the same decision from the same numbers: the whole
// file is compiled without fused multiply-add (as the geometry of tet_levelset.hpp is wherever it is included), and
// tet_parts is the one function that decides.
//
// HBM view per coefficient call: V2E (4 B x (N + 4T)) + 8 B x N per output written; per (node, tet) pair 16 B of ien, 32 B
// of T and 96 B of coordinates (with use_phi 32 B of phi more) gathered through L2; the flag pass gathers the same once per
// tet, writes T bytes and the node pass reads 4T of them back.
#include "block_ops.hpp"
#include "node_gather.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int PH_BLK = BLOCK_OPS_BLK;  // the one-thread-per-node and reduction kernels
constexpr int PH_NSTAT = 9;            // liquid volume, T_max, molten count, lo[3], hi[3]

struct TetPhase {
    double det;
    double d[4];   // (phi_a - level) / |g| (use_phi and |g| > 0)
    bool flat;     // use_phi and !(|g| > 0): one metal fraction for the tet
    double mflat;
};

// det and, with use_phi, the signed distances of the four nodes
__device__ __forceinline__ void tet_geometry(const double* x, const double* phi, const dfl_phase_params& p, TetPhase& b) {
    TetCross c;
    tet_cross(x, c);
    b.det = c.det;
    b.flat = false;
    b.mflat = 1.0;
    if (!p.use_phi) return;
    double g[3], gn;
    if (!tet_levelset(c, phi, p.level, g, gn, b.d)) {
        const double mean = ((phi[0] + phi[1]) + (phi[2] + phi[3])) * 0.25;
        b.flat = true;
        b.mflat = p.side * (mean - p.level) > 0.0 ? 1.0 : 0.0;
    }
}

// the skip rules: bit 0 = the tet adds to D / H, bit 1 = it adds to G
__device__ __forceinline__ int tet_parts(const TetPhase& b, const double* Tn, const dfl_phase_params& p) {
    if (p.use_phi) {
        if (b.flat) {
            if (b.mflat == 0.0) return 0;
        } else {
            bool gas = true;
#pragma unroll
            for (int a = 0; a < 4; ++a) gas = gas && p.side * b.d[a] <= -p.eps;
            if (gas) return 0;
        }
    }
    bool liquid = true, solid = true;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        liquid = liquid && Tn[a] >= p.T_liquidus;
        solid = solid && Tn[a] <= p.T_solidus;
    }
    const bool coeff = p.darcy_c > 0.0 || p.latent > 0.0;
    return (coeff && !liquid ? 1 : 0) | (!solid ? 2 : 0);
}

// s, fl, fl' and C of one temperature
__device__ __forceinline__ void liquid_fraction(double Tq, const dfl_phase_params& p, double& fl, double& dfl, double& C) {
    const double range = p.T_liquidus - p.T_solidus;
    const double s = fmin(1.0, fmax(0.0, (Tq - p.T_solidus) / range));  // a NaN clamps to 0
    const bool nan = !(Tq == Tq);
    fl = (s * s) * (3.0 - 2.0 * s);
    dfl = (6.0 * s) * (1.0 - s) / range;
    const double r = 1.0 - fl;
    C = nan || !(p.darcy_c > 0.0) ? 0.0 : p.darcy_c * (r * r) / ((fl * fl) * fl + p.darcy_b);
}

// out = (D_a, H_a, G_a) of local node la
__device__ __forceinline__ void tet_node_terms(const TetPhase& b, const double* Tn, int la, int parts, const dfl_phase_params& p,
                                               double* out) {
    const double wdet = GW * fabs(b.det);
    const bool lat = p.latent > 0.0;
    double D = 0.0, H = 0.0, G = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double Tq = interp_q(q, Tn);
        double m = b.mflat;
        if (p.use_phi && !b.flat) m = smooth_step(p.side * interp_q(q, b.d) / p.eps);
        double fl, dfl, C;
        liquid_fraction(Tq, p, fl, dfl, C);
        const double Wm = (wdet * shl(la, q)) * m;
        if (parts & 1) {
            D += Wm * C;
            if (lat) H += Wm * (p.latent * dfl);
        }
        if (parts & 2) G += Wm * fl;
    }
    out[0] = D;
    out[1] = H;
    out[2] = G;
}

__device__ __forceinline__ void gather_tet(const int4 n4, const T* __restrict__ xg, const T* __restrict__ w, I N, bool use_phi,
                                           double* x, double* phi, double* Tn) {
    const long long n[4] = {n4.x, n4.y, n4.z, n4.w};
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        phi[b] = use_phi ? w[4LL * N + n[b]] : 0.0;
        Tn[b] = w[5LL * N + n[b]];
#pragma unroll
        for (int d = 0; d < 3; ++d) x[b * 3 + d] = xg[n[b] * 3 + d];
    }
}

template <bool FLAGS>
__global__ __launch_bounds__(NG_BLK) void phase_node_kernel(I N, const I* __restrict__ vrow, const I* __restrict__ vcol,
                                                             const I* __restrict__ ien, const T* __restrict__ xg,
                                                             const T* __restrict__ w, const dfl_phase_params p,
                                                             const unsigned char* __restrict__ flag, T* __restrict__ D,
                                                             T* __restrict__ H, T* __restrict__ G) {
    const NodeSum s = node_gather_sum<3>(N, vrow, vcol, [&](I e, I row, double* out) {
        int parts = FLAGS ? flag[e] : 3;
        if (!parts) return false;
        const int4 n4 = reinterpret_cast<const int4*>(ien)[e];
        double x[12], phi[4], Tn[4];
        gather_tet(n4, xg, w, N, p.use_phi != 0, x, phi, Tn);
        TetPhase b;
        tet_geometry(x, phi, p, b);
        if (!FLAGS) parts = tet_parts(b, Tn, p);
        if (!parts) return false;
        const int la = n4.x == row ? 0 : n4.y == row ? 1 : n4.z == row ? 2 : 3;
        tet_node_terms(b, Tn, la, parts, p, out);
        return true;
    });
    if (s.live) {
        if (s.g == 0) {
            if (D) D[s.row] = s.acc;
        } else if (s.g == 1) {
            if (H) H[s.row] = s.acc;
        } else if (s.g == 2) {
            if (G) G[s.row] = s.acc;
        }
    }
}

__global__ __launch_bounds__(PH_BLK) void phase_flag_kernel(I NT, const I* __restrict__ ien, const T* __restrict__ xg,
                                                             const T* __restrict__ w, I N, const dfl_phase_params p,
                                                             unsigned char* __restrict__ flag) {
    const long long e = (long long)blockIdx.x * PH_BLK + threadIdx.x;
    if (e >= NT) return;
    const int4 n4 = reinterpret_cast<const int4*>(ien)[e];
    double x[12], phi[4], Tn[4];
    gather_tet(n4, xg, w, N, p.use_phi != 0, x, phi, Tn);
    TetPhase b;
    tet_geometry(x, phi, p, b);
    flag[e] = (unsigned char)tet_parts(b, Tn, p);
}

// R[3a + d] += D_a u_a[d], R[5N + a] += H_a dT_a
__global__ __launch_bounds__(PH_BLK) void phase_apply_F_kernel(I N, const T* __restrict__ D, const T* __restrict__ H,
                                                                const T* __restrict__ wgalpha, const T* __restrict__ dwgalpha,
                                                                T* __restrict__ F) {
    const long long a = (long long)blockIdx.x * PH_BLK + threadIdx.x;
    if (a >= N) return;
    if (D) {
        const double Da = D[a];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double add = Da * wgalpha[3 * a + d];
            F[3 * a + d] = F[3 * a + d] + add;
        }
    }
    if (H) {
        const double add = H[a] * dwgalpha[5LL * N + a];
        F[5LL * N + a] = F[5LL * N + a] + add;
    }
}

// position of column `a` in row `a` of an ascending pattern, -1: not stored
__device__ __forceinline__ long long find_diagonal(const I* __restrict__ row_ptr, const I* __restrict__ col_ind, I a) {
    I lo = row_ptr[a], hi = row_ptr[a + 1] - 1;
    while (lo <= hi) {
        const I mid = lo + ((hi - lo) >> 1);
        const I c = col_ind[mid];
        if (c == a) return mid;
        if (c < a) lo = mid + 1;
        else hi = mid - 1;
    }
    return -1;
}

template <int BSZ>  // 16: the (d, d), d < 3 entries of the 4x4 block get coef * v[a]; 1: the scalar diagonal
__global__ __launch_bounds__(PH_BLK) void phase_apply_diag_kernel(I N, const I* __restrict__ row_ptr, const I* __restrict__ col_ind,
                                                                   const T* __restrict__ v, double coef, T* __restrict__ val) {
    const long long a = (long long)blockIdx.x * PH_BLK + threadIdx.x;
    if (a >= N) return;
    const long long k = find_diagonal(row_ptr, col_ind, (I)a);
    if (k < 0) return;
    const double add = coef * v[a];
    if (BSZ == 16) {
#pragma unroll
        for (int d = 0; d < 3; ++d) val[k * 16 + d * 5] = val[k * 16 + d * 5] + add;
    } else {
        val[k] = val[k] + add;
    }
}

// the nine statistics: sums (liquid volume, molten count), maxima (T_max, hi) and minima (lo); a + b in this order, fmax /
// fmin drop a NaN
struct MergeStat {
    __device__ __forceinline__ static bool is_sum(int j) { return j == 0 || j == 2; }
    __device__ __forceinline__ static bool is_max(int j) { return j == 1 || j >= 6; }
    __device__ __forceinline__ double operator()(int j, double a, double b) const {
        return is_sum(j) ? a + b : is_max(j) ? fmax(a, b) : fmin(a, b);
    }
    __device__ __forceinline__ double identity(int j) const { return is_sum(j) ? 0.0 : is_max(j) ? -HUGE_VAL : HUGE_VAL; }
};

struct Stat {  // (a struct: with bare arrays phase_stats_stage1 takes 80 VGPRs, not 46, and loses two waves of occupancy)
    double v[PH_NSTAT];
};
__device__ __forceinline__ Stat stat_identity() {
    Stat s;
#pragma unroll
    for (int k = 0; k < PH_NSTAT; ++k) s.v[k] = MergeStat().identity(k);
    return s;
}

__global__ __launch_bounds__(PH_BLK) void phase_stats_stage1(I N, const T* __restrict__ xg, const T* __restrict__ w,
                                                              const T* __restrict__ G, const dfl_phase_params p,
                                                              T* __restrict__ part) {
    __shared__ double lds[4][PH_NSTAT];
    const MergeStat merge;
    Stat s = stat_identity();
    const long long stride = (long long)gridDim.x * PH_BLK;
    for (long long a = (long long)blockIdx.x * PH_BLK + threadIdx.x; a < N; a += stride) {
        const double Ta = w[5LL * N + a];
        const bool metal = !p.use_phi || p.side * (w[4LL * N + a] - p.level) > 0.0;
        double fl, dfl, C;
        liquid_fraction(Ta, p, fl, dfl, C);
        Stat o = stat_identity();
        o.v[0] = G[a];
        if (metal) o.v[1] = Ta;
        if (metal && fl >= 0.5) {
            o.v[2] = 1.0;
#pragma unroll
            for (int d = 0; d < 3; ++d) o.v[3 + d] = o.v[6 + d] = xg[3 * a + d];
        }
#pragma unroll
        for (int k = 0; k < PH_NSTAT; ++k) s.v[k] = merge(k, s.v[k], o.v[k]);
    }
    block_tree_256<PH_NSTAT>(s.v, merge, lds);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < PH_NSTAT; ++k) part[(long long)blockIdx.x * PH_NSTAT + k] = s.v[k];
}

}  // namespace

extern "C" {

void dfl_phase_flag_tets(I NT, const I* ien, const T* xg, const T* w, I N, const dfl_phase_params* prm, unsigned char* flag,
                         void* stream) {
    if (NT <= 0) return;
    phase_flag_kernel<<<ceil_div(NT, PH_BLK), PH_BLK, 0, S(stream)>>>(NT, ien, xg, w, N, *prm, flag);
    DFL_LAUNCH_CHECK();
}

void dfl_phase_coefficients(I N, const I* vrow, const I* vcol, const I* ien, const T* xg, const T* w, const dfl_phase_params* prm,
                            const unsigned char* flag, T* D, T* H, T* G, void* stream) {
    if (N <= 0 || (!D && !H && !G)) return;
    if (flag)
        phase_node_kernel<true><<<ceil_div(N, NG_ROWS), NG_BLK, 0, S(stream)>>>(N, vrow, vcol, ien, xg, w, *prm, flag, D, H, G);
    else
        phase_node_kernel<false><<<ceil_div(N, NG_ROWS), NG_BLK, 0, S(stream)>>>(N, vrow, vcol, ien, xg, w, *prm, flag, D, H, G);
    DFL_LAUNCH_CHECK();
}

void dfl_phase_apply_F(I N, const T* D, const T* H, const T* wgalpha, const T* dwgalpha, T* F, void* stream) {
    if (N <= 0 || (!D && !H)) return;
    phase_apply_F_kernel<<<ceil_div(N, PH_BLK), PH_BLK, 0, S(stream)>>>(N, D, H, wgalpha, dwgalpha, F);
    DFL_LAUNCH_CHECK();
}

void dfl_phase_apply_J(I N, const I* row_ptr, const I* col_ind, const T* D, T fact2, T* val, void* stream) {
    if (N <= 0) return;
    phase_apply_diag_kernel<16><<<ceil_div(N, PH_BLK), PH_BLK, 0, S(stream)>>>(N, row_ptr, col_ind, D, fact2, val);
    DFL_LAUNCH_CHECK();
}

void dfl_phase_apply_JT(I N, const I* row_ptr, const I* col_ind, const T* H, T alpham, T* val, void* stream) {
    if (N <= 0) return;
    phase_apply_diag_kernel<1><<<ceil_div(N, PH_BLK), PH_BLK, 0, S(stream)>>>(N, row_ptr, col_ind, H, alpham, val);
    DFL_LAUNCH_CHECK();
}

I dfl_phase_stats_work_size(void) { return NODE_REDUCE_MAX_PART * PH_NSTAT; }

void dfl_phase_stats(I N, const T* xg, const T* w, const T* G, const dfl_phase_params* prm, T* work, T* out9, void* stream) {
    if (N <= 0) return;
    const int g = node_reduce_grid(N);
    phase_stats_stage1<<<g, PH_BLK, 0, S(stream)>>>(N, xg, w, G, *prm, work);
    block_reduce<PH_NSTAT>(g, work, out9, MergeStat(), stream);
    DFL_LAUNCH_CHECK();
}

}  // extern "C"
