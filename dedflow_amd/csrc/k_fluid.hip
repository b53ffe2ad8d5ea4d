// Two-fluid momentum and continuity rows for gfx950: the correction that turns the (u,p) rows and Jacobian blocks of the
// one-phase assembly (kRHO, kMU, no body force) into rows with the density rho_q, the viscosity mu_q and the body force f_q
// at every quadrature point (build-defined: the reference has one fluid without weight; model in include/dedflow.h, "fluid
// material").  The base assembly kernels are untouched: base + correction is the two-fluid system.
//
//   fluid_rows_kernel<NC>    the node gather of node_gather.hpp.  A lane gathers its tet's ien line, coordinates, u, du, p,
//                            T and (with use_phi) phi, forms rho_q, mu_q, f_q and evaluates E_a(rho, mu, f) - E_a(kRHO, kMU, 0)
//                            of its own node through one inlined function (fluid_coeff.hpp), the four quadrature points in a
//                            rolled loop so that they share code and registers.  NC = 4: the three momentum rows
//                            and the continuity row (the assembly path: a tet with the built-in coefficients and no force
//                            leaves early and parks +0.0; with `add` the owner lanes add their sums into F: one launch, no
//                            buffer).  NC = 6: also Rn and Mn (totals, so no tet leaves).
//   fluid_jac_row_kernel     the row gather of scalar_jac_row_kernel (k_scalar.hip) with the 4 x 4 block in place of the two
//                            scalars.  A group of 16 lanes owns nodal row a; lane j evaluates the four difference blocks
//                            jm_a0 .. jm_a3 of tet j (64 doubles, kept in registers).  They are handed over in four rounds of
//                            four tets each (lanes 4r .. 4r+3 park in round r), so the LDS of a workgroup is
//                            16 groups x 4 tets x (64 x 8 B + 16 B of node ids) = 33 KiB and four workgroups fit a CU by LDS
//                            (all 64 doubles of all 256 lanes at once would be 128 KiB: one).  Lane k owns nonzero k of the
//                            row, adds the parked blocks whose node is its column in list order -- rounds ascend, and the
//                            tets inside a round ascend, so the order is the V2E order -- and then does the one
//                            read-modify-write of its 16 values.  Parked blocks move as 16-byte LDS accesses.
//
// No atomics, every value written once by its owner, fixed summation order from +0.0: bitwise reproducible and independent
// of the assembly schedule.  The whole file is compiled without fused multiply-add.
#include "fluid_coeff.hpp"

#pragma clang fp contract(off)

namespace {

struct FluidTet {
    TetCross c;
    double rho[4], mu[4], fac[4];  // f_q[i] = gravity[i] fac[q]
};

// gathers coordinates, phi and T of the tet and forms its coefficients
__device__ __forceinline__ void fluid_gather_coefficients(const long long* n, I N, const T* __restrict__ xg, const T* __restrict__ w,
                                                          const dfl_fluid_params& p, FluidTet& t) {
    double x[12], phi[4], Tn[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        phi[b] = p.use_phi ? w[4LL * N + n[b]] : 0.0;
        Tn[b] = p.beta != 0.0 ? w[5LL * N + n[b]] : 0.0;
#pragma unroll
        for (int d = 0; d < 3; ++d) x[b * 3 + d] = xg[n[b] * 3 + d];
    }
    tet_cross(x, t.c);
    fluid_coefficients(t.c, phi, Tn, p, t.rho, t.mu, t.fac);
}

// out[0..2] the momentum rows, out[3] the continuity row, and with NC = 6 out[4] = Rn_a, out[5] = Mn_a, of local node la
template <int NC>
__device__ __forceinline__ bool fluid_tet_node(const StepK& sk, const int4 n4, I row, I N, const T* __restrict__ xg, const T* __restrict__ w,
                                               const T* __restrict__ dw, const dfl_fluid_params& p, double* out) {
    const long long n[4] = {n4.x, n4.y, n4.z, n4.w};
    FluidTet t;
    fluid_gather_coefficients(n, N, xg, w, p, t);
    const bool base = fluid_is_base(t.rho, t.mu, t.fac, p);
    if (NC == 4 && base) return false;
    const int la = n4.x == row ? 0 : n4.y == row ? 1 : n4.z == row ? 2 : 3;
    FluidGeom g;
    fluid_geometry(t.c, g);
    if (!base) {
        FluidFields v;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            v.p[b] = dw[3LL * N + n[b]];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                v.u[b][d] = w[n[b] * 3 + d];
                v.du[b][d] = dw[n[b] * 3 + d];
            }
        }
        FluidRowTet rt;
        fluid_row_tet(g, v, la, rt);
        double E[4] = {0.0, 0.0, 0.0, 0.0}, E0[4] = {0.0, 0.0, 0.0, 0.0};
        const double f0[3] = {0.0, 0.0, 0.0};
#pragma unroll 1
        for (int q = 0; q < 4; ++q) {  // (rolled: the four points share the code and the registers)
            FluidRowPoint pt;
            fluid_row_point(g, v, la, q, pt);
            const double fq = sel4(q, t.fac);
            const double f[3] = {p.gravity[0] * fq, p.gravity[1] * fq, p.gravity[2] * fq};
            fluid_E_add(sk, g, rt, pt, sel4(q, t.rho), sel4(q, t.mu), f, E);
            fluid_E_add(sk, g, rt, pt, kRHO, kMU, f0, E0);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) out[k] = E[k] - E0[k];
    }
    if (NC == 6) {
        double R = 0.0, M = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            R += (g.W * shl(la, q)) * t.rho[q];
            M += (g.W * shl(la, q)) * t.mu[q];
        }
        out[4] = R;
        out[5] = M;
    }
    return true;
}

template <int NC>
__global__ __launch_bounds__(NG_BLK) void fluid_rows_kernel(I N, const I* __restrict__ vrow, const I* __restrict__ vcol,
                                                             const I* __restrict__ ien, const T* __restrict__ xg,
                                                             const T* __restrict__ w, const T* __restrict__ dw,
                                                             const dfl_fluid_params p, T* __restrict__ r, T* __restrict__ Rn,
                                                             T* __restrict__ Mn, T* __restrict__ add, const StepK sk) {
    const NodeSum s = node_gather_sum<NC>(N, vrow, vcol, [&](I e, I row, double* out) {
        return fluid_tet_node<NC>(sk, reinterpret_cast<const int4*>(ien)[e], row, N, xg, w, dw, p, out);
    });
    if (!s.live) return;
    if (s.g < 4) {
        const long long at = s.g < 3 ? 3LL * s.row + s.g : 3LL * N + s.row;
        if (add) add[at] = add[at] + s.acc;
        else if (r) r[at] = s.acc;
    } else if (NC == 6 && s.g == 4) {
        if (Rn) Rn[s.row] = s.acc;
    } else if (NC == 6 && s.g == 5) {
        if (Mn) Mn[s.row] = s.acc;
    }
}

constexpr int FJ_RND = 4;                    // hand-over rounds per trip
constexpr int FJ_TPR = NG_LANES / FJ_RND;    // tets per round and group
constexpr int FJ_SLOTS = NG_ROWS * FJ_TPR;   // parked tets per workgroup

__global__ __launch_bounds__(NG_BLK) void fluid_jac_row_kernel(I N, const I* __restrict__ vrow, const I* __restrict__ vcol,
                                                                const I* __restrict__ ien, const T* __restrict__ xg,
                                                                const T* __restrict__ wg, const I* __restrict__ row_ptr,
                                                                const I* __restrict__ col_ind, const dfl_fluid_params p,
                                                                T* __restrict__ val, const StepK sk) {
    __shared__ int4 s_node[FJ_SLOTS];
    __shared__ double2 s_blk[FJ_SLOTS][4][8];  // [slot][b][pair of entries]
    const int t = threadIdx.x;
    const int g = t & (NG_LANES - 1);
    const int grp = t / NG_LANES;
    const long long row_ll = (long long)blockIdx.x * NG_ROWS + grp;
    const bool live = row_ll < N;
    const I row = live ? (I)row_ll : 0;
    const I e0 = live ? vrow[row] : 0, ne = live ? vrow[row + 1] - e0 : 0;
    const I c0 = live ? row_ptr[row] : 0, nc = live ? row_ptr[row + 1] - c0 : 0;
    const int ne_w = wave_max(ne), nc_w = wave_max(nc);
    for (int kc = 0; kc < nc_w; kc += NG_LANES) {
        const int k = kc + g;
        const I col = k < nc ? col_ind[c0 + k] : -1;
        double S[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) S[e] = 0.0;
        for (int jc = 0; jc < ne_w; jc += NG_LANES) {
            const int j = jc + g;
            int4 n4 = make_int4(-1, -1, -1, -1);
            double jm[4][16];
            bool any = false;
            if (j < ne) {
                n4 = reinterpret_cast<const int4*>(ien)[vcol[e0 + j]];
                const long long n[4] = {n4.x, n4.y, n4.z, n4.w};
                FluidTet tt;
                fluid_gather_coefficients(n, N, xg, wg, p, tt);
                bool same = true;  // (the body force does not enter the Jacobian)
#pragma unroll
                for (int q = 0; q < 4; ++q) same = same && tt.rho[q] == kRHO && tt.mu[q] == kMU;
                any = !same;
                if (any) {
                    const int la = n4.x == row ? 0 : n4.y == row ? 1 : n4.z == row ? 2 : 3;
                    FluidGeom geo;
                    fluid_geometry(tt.c, geo);
                    double u[4][3];
#pragma unroll
                    for (int b = 0; b < 4; ++b)
#pragma unroll
                        for (int d = 0; d < 3; ++d) u[b][d] = wg[n[b] * 3 + d];
                    FluidJacTet jt;
                    fluid_jac_tet(sk, geo, u, tt.rho, tt.mu, jt);
                    const double rho0[4] = {kRHO, kRHO, kRHO, kRHO}, mu0[4] = {kMU, kMU, kMU, kMU};
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        double B[16], B0[16];
                        fluid_tet_B(sk, geo, jt.c, la, b, tt.rho, tt.mu, jt.t0, jt.t1, B);
                        fluid_tet_B(sk, geo, jt.c, la, b, rho0, mu0, jt.t0b, jt.t1b, B0);
#pragma unroll
                        for (int e = 0; e < 16; ++e) jm[b][e] = B[e] - B0[e];
                    }
                }
            }
            if (!__any(any)) continue;  // wave-uniform: every block of this trip is +0.0, and the sums started from +0.0
            if (!any)
#pragma unroll
                for (int b = 0; b < 4; ++b)
#pragma unroll
                    for (int e = 0; e < 16; ++e) jm[b][e] = 0.0;
#pragma unroll 1
            for (int rnd = 0; rnd < FJ_RND; ++rnd) {
                if (jc + rnd * FJ_TPR >= ne_w) break;  // wave-uniform
                const int slot0 = grp * FJ_TPR;
                if (g / FJ_TPR == rnd) {
                    const int slot = slot0 + (g % FJ_TPR);
                    s_node[slot] = n4;
#pragma unroll
                    for (int b = 0; b < 4; ++b)
#pragma unroll
                        for (int e = 0; e < 8; ++e) s_blk[slot][b][e] = make_double2(jm[b][2 * e], jm[b][2 * e + 1]);
                }
                WAVE_SYNC();
                const int nj = min(FJ_TPR, (int)ne - (jc + rnd * FJ_TPR));
                if (col >= 0) {
                    for (int jj = 0; jj < nj; ++jj) {  // V2E order: ascending tet id
                        const int4 m = s_node[slot0 + jj];
                        const int b = m.x == col ? 0 : m.y == col ? 1 : m.z == col ? 2 : m.w == col ? 3 : -1;
                        if (b >= 0) {
#pragma unroll
                            for (int e = 0; e < 8; ++e) {
                                const double2 v = s_blk[slot0 + jj][b][e];
                                S[2 * e] += v.x;
                                S[2 * e + 1] += v.y;
                            }
                        }
                    }
                }
                WAVE_SYNC();  // the parked blocks are consumed before the next round overwrites them
            }
        }
        if (k < nc) {
            double2* dst = reinterpret_cast<double2*>(val + 16LL * (c0 + k));
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                double2 v = dst[e];
                v.x = v.x + S[2 * e];
                v.y = v.y + S[2 * e + 1];
                dst[e] = v;
            }
        }
    }
}

}  // namespace

extern "C" {

void dfl_fluid_rows(I N, const I* vrow, const I* vcol, const I* ien, const T* xg, const T* w, const T* dw,
                    const dfl_fluid_params* prm, T* r, T* Rn, T* Mn, void* stream) {
    dfl_fluid_rows_dt(N, vrow, vcol, ien, xg, w, dw, prm, r, Rn, Mn, dfl_step_consts_default(), stream);
}
void dfl_fluid_rows_dt(I N, const I* vrow, const I* vcol, const I* ien, const T* xg, const T* w, const T* dw,
                       const dfl_fluid_params* prm, T* r, T* Rn, T* Mn, const dfl_step_consts* k, void* stream) {
    if (N <= 0 || (!r && !Rn && !Mn)) return;
    if (Rn || Mn)
        fluid_rows_kernel<6><<<ceil_div(N, NG_ROWS), NG_BLK, 0, S(stream)>>>(N, vrow, vcol, ien, xg, w, dw, *prm, r, Rn, Mn, nullptr, *k);
    else
        fluid_rows_kernel<4><<<ceil_div(N, NG_ROWS), NG_BLK, 0, S(stream)>>>(N, vrow, vcol, ien, xg, w, dw, *prm, r, nullptr, nullptr,
                                                                            nullptr, *k);
    DFL_LAUNCH_CHECK();
}

void dfl_fluid_add_rows(I N, const I* vrow, const I* vcol, const I* ien, const T* xg, const T* wgalpha, const T* dwgalpha,
                        const dfl_fluid_params* prm, T* F, void* stream) {
    dfl_fluid_add_rows_dt(N, vrow, vcol, ien, xg, wgalpha, dwgalpha, prm, F, dfl_step_consts_default(), stream);
}
void dfl_fluid_add_rows_dt(I N, const I* vrow, const I* vcol, const I* ien, const T* xg, const T* wgalpha, const T* dwgalpha,
                           const dfl_fluid_params* prm, T* F, const dfl_step_consts* k, void* stream) {
    if (N <= 0 || !F) return;
    fluid_rows_kernel<4><<<ceil_div(N, NG_ROWS), NG_BLK, 0, S(stream)>>>(N, vrow, vcol, ien, xg, wgalpha, dwgalpha, *prm, nullptr,
                                                                        nullptr, nullptr, F, *k);
    DFL_LAUNCH_CHECK();
}

void dfl_fluid_add_jacobian(I N, const I* vrow, const I* vcol, const I* ien, const T* xg, const T* wgalpha, const I* row_ptr,
                            const I* col_ind, const dfl_fluid_params* prm, T* val, void* stream) {
    dfl_fluid_add_jacobian_dt(N, vrow, vcol, ien, xg, wgalpha, row_ptr, col_ind, prm, val, dfl_step_consts_default(), stream);
}
void dfl_fluid_add_jacobian_dt(I N, const I* vrow, const I* vcol, const I* ien, const T* xg, const T* wgalpha, const I* row_ptr,
                               const I* col_ind, const dfl_fluid_params* prm, T* val, const dfl_step_consts* k, void* stream) {
    if (N <= 0 || !val) return;
    fluid_jac_row_kernel<<<ceil_div(N, NG_ROWS), NG_BLK, 0, S(stream)>>>(N, vrow, vcol, ien, xg, wgalpha, row_ptr, col_ind, *prm, val, *k);
    DFL_LAUNCH_CHECK();
}

}  // extern "C"
