// Scalar transport Jacobians for gfx950: the exact derivatives of the level-set (phi) and temperature (T) rows of the
// element residual (rhs_quad in asm_device.hpp; src/assemble.cu:885-906) with respect to the rates dphi / dT:
//
//   Jphi[a][b] = sum_q w |det J| (N_a + tau2 c_a) (f1 N_b + f2 c_b)
//   JT[a][b]   = sum_q w |det J| [ rho cp (N_a + rho cp tau3 c_a) (f1 N_b + f2 c_b) + f2 kappa gradN_a . gradN_b ]
//
// with c_a = u(q) . gradN_a, tau2 / tau3 as rhs_quad forms them at every quadrature point, f1 = alpha_m and
// f2 = dt alpha_f gamma.  Both depend on the geometry and on u only.  With a thermal material (include/dedflow.h) JT also gets
// the entries jm of that section, from phi and T as well: the MATERIAL instantiation below, in the same single launch.
//
//   scalar_jac_row_kernel   row gather in the shape of node_gather.hpp (its constants and trip count; a Kuhn-cube interior
//                           row has 15 nonzeros and 24 tets): a group of 16 lanes owns one nodal CSR row a.
//                           Phase 1: lane j of the group takes tet j of a's V2E list (ascending tet id), evaluates the
//                           four entries (a, b) of both element matrices and parks them with the tet's node ids in LDS.
//                           Phase 2: lane k of the group owns nonzero k of the row and adds the parked entries whose
//                           node is its column, in V2E order.  More than 16 tets or nonzeros per row: more trips of the
//                           same group.  No atomics, every value written once (no zero pass), fixed summation order:
//                           bitwise reproducible, and independent of the assembly schedule of the (u,p) system.
//
// HBM view per assembly: 2 x 8 B x nnz1 of values written + row_ptr / col_ind (4 B x (N + nnz1)) + V2E (4 B x 4T) + per
// (row, tet) pair the tet's ien line (16 B) and 4 x 48 B of coordinates and velocities gathered through L2 (MATERIAL: 4 x 8 B
// of T more, and with use_phi 4 x 8 B of phi).
#include <type_traits>
#include "thermal_coeff.hpp"

namespace {

// the four entries (la, b) of both element matrices of one tet; la = the local index of the row's node.  MATERIAL: dk / dc =
// the thermal-material differences at the four quadrature points (thermal_coeff.hpp), any = not all of them are 0; the entries
//   jm[b] = sum_q w [ dc_q N_la (f1 N_b + f2 c_b) + f2 dk_q gradN_la . gradN_b ]
// are formed beside the base ones from the same geometry and added to the finished jt[b] (the base is rounded first).  The
// conduction part depends on q through dk_q alone, so it is w kg[b] (sum_q dk_q) / kKAPPA: jm[b] starts from it
template <bool MATERIAL>
__device__ __forceinline__ void scalar_tet_row(const StepK& sk, const double* x, const double* u, int la, double* jp, double* jt,
                                               const double* dk = nullptr, const double* dc = nullptr, bool any = false) {
    double invJ[9], shg[12], G[9], detJ;
    tet_geometry(x, invJ, detJ, shg);
    tet_metric(shg, G);
    double gg = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) gg += G[k] * G[k];
    const double f1 = kALPHAM, f2 = sk.fact2;
    const double t0 = sk.t0;
    const double kappa = kKAPPA / (kRHO * kCP);
    const double rc = kRHO * kCP;
    const double w = GW * detJ;
    double kg[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        jp[b] = 0.0;
        jt[b] = 0.0;
        kg[b] = sk.fact2_kappa * (shg[la * 3] * shg[b * 3] + shg[la * 3 + 1] * shg[b * 3 + 1] + shg[la * 3 + 2] * shg[b * 3 + 2]);
    }
    double jm[4];
    if constexpr (MATERIAL) {
        const double sdk = w * ((((dk[0] + dk[1]) + dk[2]) + dk[3]) * (1.0 / kKAPPA));
#pragma unroll
        for (int b = 0; b < 4; ++b) jm[b] = sdk * kg[b];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        double uq[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            double s = 0.0;
#pragma unroll
            for (int b = 0; b < 4; ++b) s += shl(b, q) * u[b * 3 + d];
            uq[d] = s;
        }
        // u.G.u of GetStabTau (assemble.cu:444-484) exactly as rhs_quad forms it
        double t1 = 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double v = shg[3 + r] * uq[0] + shg[6 + r] * uq[1] + shg[9 + r] * uq[2];
            t1 += v * v;
        }
        const double tau2 = 1.0 / sqrt(t0 + t1);
        const double tau3 = (1.0 / sqrt(t0 + t1 + 3.0 * kappa * kappa * gg)) / rc;
        double c[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) c[b] = uq[0] * shg[b * 3] + uq[1] * shg[b * 3 + 1] + uq[2] * shg[b * 3 + 2];
        const double ca = la == 0 ? c[0] : la == 1 ? c[1] : la == 2 ? c[2] : c[3];
        const double na = shl(la, q);
        const double rp = w * (na + tau2 * ca);
        const double rt = w * rc * (na + rc * tau3 * ca);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const double cb = f1 * shl(b, q) + f2 * c[b];
            jp[b] += rp * cb;
            jt[b] += rt * cb + w * kg[b];
            if constexpr (MATERIAL)
                if (any) jm[b] += ((w * dc[q]) * na) * cb;
        }
    }
    if constexpr (MATERIAL)
        if (any)
#pragma unroll
            for (int b = 0; b < 4; ++b) jt[b] = jt[b] + jm[b];
}

struct NoMaterial {};
template <bool MATERIAL>
using MaterialArg = std::conditional_t<MATERIAL, dfl_thermal_params, NoMaterial>;

// MATERIAL = false is the kernel of the one-material heat equation, unchanged.  MATERIAL = true (include/dedflow.h, "thermal
// material") also gathers the tet's four phi and T beside x and u, forms dk_q / dc_q and parks jt[b] + jm[b]: one launch
template <bool MATERIAL>
__global__ __launch_bounds__(NG_BLK) void scalar_jac_row_kernel(I N, const I* __restrict__ vrow, const I* __restrict__ vcol,
                                                                 const I* __restrict__ ien, const T* __restrict__ xg,
                                                                 const T* __restrict__ wg, const I* __restrict__ row_ptr,
                                                                 const I* __restrict__ col_ind, T* __restrict__ vphi,
                                                                 T* __restrict__ vT, const MaterialArg<MATERIAL> mat, const StepK sk) {
    __shared__ int4 s_node[NG_BLK];
    __shared__ double s_jp[NG_BLK][4];
    __shared__ double s_jt[NG_BLK][4];
    const int t = threadIdx.x;
    const int g = t & (NG_LANES - 1);
    const int gbase = t & ~(NG_LANES - 1);
    const long long row_ll = (long long)blockIdx.x * NG_ROWS + t / NG_LANES;
    const bool live = row_ll < N;
    const I row = live ? (I)row_ll : 0;
    const I e0 = live ? vrow[row] : 0, ne = live ? vrow[row + 1] - e0 : 0;
    const I c0 = live ? row_ptr[row] : 0, nc = live ? row_ptr[row + 1] - c0 : 0;
    // every lane of a wave takes the same trips (the LDS hand-over below is a wave barrier)
    const int ne_w = wave_max(ne), nc_w = wave_max(nc);
    for (int kc = 0; kc < nc_w; kc += NG_LANES) {
        const int k = kc + g;
        const I col = k < nc ? col_ind[c0 + k] : -1;
        double ap = 0.0, at = 0.0;
        for (int jc = 0; jc < ne_w; jc += NG_LANES) {
            const int j = jc + g;
            if (j < ne) {
                const I e = vcol[e0 + j];
                const int4 n4 = reinterpret_cast<const int4*>(ien)[e];
                const int n[4] = {n4.x, n4.y, n4.z, n4.w};
                double x[12], u[12];
#pragma unroll
                for (int b = 0; b < 4; ++b)
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        x[b * 3 + d] = xg[(long long)n[b] * 3 + d];
                        u[b * 3 + d] = wg[(long long)n[b] * 3 + d];
                    }
                const int la = n[0] == row ? 0 : n[1] == row ? 1 : n[2] == row ? 2 : 3;
                double jp[4], jt[4];
                if constexpr (MATERIAL) {
                    double phi[4], Tn[4], m[4], kq[4], cq[4], dk[4], dc[4];
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        phi[b] = mat.use_phi ? wg[4LL * N + n[b]] : 0.0;
                        Tn[b] = wg[5LL * N + n[b]];
                    }
                    TetCross c;
                    if (mat.use_phi) tet_cross(x, c);  // (the metal fraction as the row pass forms it: tet_levelset.hpp)
                    thermal_metal_fraction(c, phi, mat, m);
                    thermal_kc(m, Tn, mat, kq, cq);
                    const bool any = thermal_differences(kq, cq, dk, dc);
                    scalar_tet_row<true>(sk, x, u, la, jp, jt, dk, dc, any);
                } else {
                    scalar_tet_row<false>(sk, x, u, la, jp, jt);
                }
                s_node[t] = n4;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    s_jp[t][b] = jp[b];
                    s_jt[t][b] = jt[b];
                }
            }
            WAVE_SYNC();
            const int nj = min(NG_LANES, (int)ne - jc);
            if (col >= 0) {
                for (int jj = 0; jj < nj; ++jj) {  // V2E order: ascending tet id
                    const int src = gbase + jj;
                    const int4 m = s_node[src];
                    const int b = m.x == col ? 0 : m.y == col ? 1 : m.z == col ? 2 : m.w == col ? 3 : -1;
                    if (b >= 0) {
                        ap += s_jp[src][b];
                        at += s_jt[src][b];
                    }
                }
            }
            WAVE_SYNC();  // the parked entries are consumed before the next trip overwrites them
        }
        if (k < nc) {
            if (vphi) vphi[c0 + k] = ap;
            if (vT) vT[c0 + k] = at;
        }
    }
}

}  // namespace

extern "C" void dfl_assemble_scalar_jacobian(I N, const I* vrow, const I* vcol, const I* ien, const T* xg, const T* wgalpha,
                                             const I* row_ptr, const I* col_ind, T* val_phi, T* val_T, void* stream) {
    dfl_assemble_scalar_jacobian_dt(N, vrow, vcol, ien, xg, wgalpha, row_ptr, col_ind, val_phi, val_T, dfl_step_consts_default(), stream);
}
extern "C" void dfl_assemble_scalar_jacobian_dt(I N, const I* vrow, const I* vcol, const I* ien, const T* xg, const T* wgalpha,
                                                const I* row_ptr, const I* col_ind, T* val_phi, T* val_T,
                                                const dfl_step_consts* k, void* stream) {
    if (N <= 0 || (!val_phi && !val_T)) return;
    scalar_jac_row_kernel<false><<<ceil_div(N, NG_ROWS), NG_BLK, 0, S(stream)>>>(N, vrow, vcol, ien, xg, wgalpha, row_ptr, col_ind,
                                                                                 val_phi, val_T, NoMaterial{}, *k);
    DFL_LAUNCH_CHECK();
}

extern "C" void dfl_assemble_scalar_jacobian_material(I N, const I* vrow, const I* vcol, const I* ien, const T* xg, const T* wgalpha,
                                                      const I* row_ptr, const I* col_ind, const dfl_thermal_params* prm,
                                                      T* val_phi, T* val_T, void* stream) {
    dfl_assemble_scalar_jacobian_material_dt(N, vrow, vcol, ien, xg, wgalpha, row_ptr, col_ind, prm, val_phi, val_T,
                                             dfl_step_consts_default(), stream);
}
extern "C" void dfl_assemble_scalar_jacobian_material_dt(I N, const I* vrow, const I* vcol, const I* ien, const T* xg,
                                                         const T* wgalpha, const I* row_ptr, const I* col_ind,
                                                         const dfl_thermal_params* prm, T* val_phi, T* val_T,
                                                         const dfl_step_consts* k, void* stream) {
    if (N <= 0 || (!val_phi && !val_T)) return;
    scalar_jac_row_kernel<true><<<ceil_div(N, NG_ROWS), NG_BLK, 0, S(stream)>>>(N, vrow, vcol, ien, xg, wgalpha, row_ptr, col_ind,
                                                                                val_phi, val_T, *prm, *k);
    DFL_LAUNCH_CHECK();
}
