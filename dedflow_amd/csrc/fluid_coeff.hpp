// The two-fluid momentum and continuity rows of one tet (include/dedflow.h, "fluid material"): density rho_q, viscosity mu_q
// and body force f_q at the four quadrature points, the element residual E_a(rho, mu, f) of one node and the element Jacobian
// blocks B_ab(rho, mu) of one node pair with the coefficients inside the quadrature sums.  The terms are those of rhs_quad and
// lhs_block_eval (asm_device.hpp) with rho_q for kRHO, mu_q for kMU and f_q for fb.  Shared by the row pass and the Jacobian
// pass of k_fluid.hip; every function switches fused multiply-add off for its own body, so the correction
// E(rho_q, mu_q, f_q) - E(kRHO, kMU, 0), both sides through the same inlined function, is exactly +0.0 for a tet whose
// coefficients are the built-in ones.
#pragma once
#include "thermal_coeff.hpp"

namespace {

// the tet's geometry as the level-set sections form it: grad N_a = cr_a / det from the cross products, W = GW |det|, the
// metric G(i,j) = sum_r dxi_i/dx_r dxi_j/dx_r of the assembly with gg = sum G_ij^2 and tr = G_00 + G_11 + G_22
struct FluidGeom {
    double gN[4][3];
    double W, gg, tr;
};

__device__ __forceinline__ void fluid_geometry(const TetCross& c, FluidGeom& g) {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        g.gN[0][k] = -((c.c23[k] + c.c31[k]) + c.c12[k]) / c.det;
        g.gN[1][k] = c.c23[k] / c.det;
        g.gN[2][k] = c.c31[k] / c.det;
        g.gN[3][k] = c.c12[k] / c.det;
    }
    g.W = GW * fabs(c.det);
    g.gg = 0.0;
    g.tr = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double G = (g.gN[i + 1][0] * g.gN[j + 1][0] + g.gN[i + 1][1] * g.gN[j + 1][1]) + g.gN[i + 1][2] * g.gN[j + 1][2];
            g.gg += G * G;
            if (i == j) g.tr += G;
        }
}

// m_q by the rules of the thermal material (thermal_coeff.hpp), then rho_q, mu_q and the factor fac_q of
// f_q[i] = gravity[i] fac_q; Tn is read only with beta != 0
__device__ __forceinline__ void fluid_coefficients(const TetCross& c, const double* phi, const double* Tn, const dfl_fluid_params& p,
                                                   double* rho, double* mu, double* fac) {
#pragma clang fp contract(off)
    dfl_thermal_params tp = {};
    tp.level = p.level;
    tp.side = p.side;
    tp.eps = p.eps;
    tp.use_phi = p.use_phi;
    double m[4];
    thermal_metal_fraction(c, phi, tp, m);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        rho[q] = p.rho_gas + m[q] * (p.rho_metal - p.rho_gas);
        mu[q] = p.mu_gas + m[q] * (p.mu_metal - p.mu_gas);
        fac[q] = 1.0;
        if (p.beta != 0.0) {
            const double Tq = interp_q(q, Tn);
            if (Tq == Tq) fac[q] = 1.0 - (m[q] * p.beta) * (Tq - p.T_ref);  // a NaN T_q: the factor 1
        }
    }
}

// whether every coefficient is the built-in one and every f_q is zero (a NaN counts as different)
__device__ __forceinline__ bool fluid_is_base(const double* rho, const double* mu, const double* fac, const dfl_fluid_params& p) {
#pragma clang fp contract(off)
    bool same = true;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        same = same && rho[q] == kRHO && mu[q] == kMU && p.gravity[0] * fac[q] == 0.0 && p.gravity[1] * fac[q] == 0.0 &&
               p.gravity[2] * fac[q] == 0.0;
    return same;
}

// the fields of one tet the rows need: u, du [b][d], the pressure p [b] (from the rate vector, as the assembly takes it)
struct FluidFields {
    double u[4][3], du[4][3], p[4];
};

// what the quadrature points of a tet share in the rows: grad[i][d] = d u_i / d x_d, grad p, div u, grad N of the own node
struct FluidRowTet {
    double grad[3][3], gp[3], divu, ga[3];
};

__device__ __forceinline__ void fluid_row_tet(const FluidGeom& g, const FluidFields& v, int la, FluidRowTet& t) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int d = 0; d < 3; ++d)
            t.grad[i][d] = ((g.gN[0][d] * v.u[0][i] + g.gN[1][d] * v.u[1][i]) + g.gN[2][d] * v.u[2][i]) + g.gN[3][d] * v.u[3][i];
        t.gp[i] = ((g.gN[0][i] * v.p[0] + g.gN[1][i] * v.p[1]) + g.gN[2][i] * v.p[2]) + g.gN[3][i] * v.p[3];
    }
    t.divu = (t.grad[0][0] + t.grad[1][1]) + t.grad[2][2];
#pragma unroll
    for (int d = 0; d < 3; ++d) t.ga[d] = la == 0 ? g.gN[0][d] : la == 1 ? g.gN[1][d] : la == 2 ? g.gN[2][d] : g.gN[3][d];
}

// what one quadrature point interpolates from the nodes, the same for both evaluations
struct FluidRowPoint {
    double uq[3], aq[3], pq, t1, na;
};

__device__ __forceinline__ void fluid_row_point(const FluidGeom& g, const FluidFields& v, int la, int q, FluidRowPoint& s) {
#pragma clang fp contract(off)
    double ub[4], ab[4];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            ub[b] = v.u[b][i];
            ab[b] = v.du[b][i];
        }
        s.uq[i] = interp_q(q, ub);
        s.aq[i] = interp_q(q, ab);
    }
    s.pq = interp_q(q, v.p);
    s.t1 = 0.0;  // u.G.u as rhs_quad forms it
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double w = (g.gN[1][k] * s.uq[0] + g.gN[2][k] * s.uq[1]) + g.gN[3][k] * s.uq[2];
        s.t1 += w * w;
    }
    s.na = shl(la, q);
}

// E[0..2] += the momentum rows, E[3] += the continuity row of the own node at one quadrature point (the element residual of
// rhs_quad) with the density r, the viscosity m and the body force f there.  The caller adds the four points in ascending q
// from +0.0, once with (rho_q, mu_q, f_q) and once with (kRHO, kMU, 0), through this one function
__device__ __forceinline__ void fluid_E_add(const StepK& sk, const FluidGeom& g, const FluidRowTet& t, const FluidRowPoint& s, double r, double m,
                                            const double* f, double* E) {
#pragma clang fp contract(off)
    double acc[3], rLi[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) acc[i] = s.aq[i] - f[i];
#pragma unroll
    for (int i = 0; i < 3; ++i)
        rLi[i] = (((r * acc[i] + (r * s.uq[0]) * t.grad[i][0]) + (r * s.uq[1]) * t.grad[i][1]) + (r * s.uq[2]) * t.grad[i][2]) + t.gp[i];
    const double nu = m / r;
    const double y = s.t1 + ((3.0 * nu) * nu) * g.gg;
    const double tau0 = (1.0 / sqrt(sk.t0 + y)) / r;
    const double tau1 = sqrt(y) / g.tr;
    const double diag = r * tau1 * t.divu - s.pq;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double tmp0 = r * acc[i];
#pragma unroll
        for (int d = 0; d < 3; ++d) tmp0 += (r * (s.uq[d] - tau0 * rLi[d])) * t.grad[i][d];
        double bm = s.na * tmp0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double x = m * (t.grad[i][j] + t.grad[j][i]);
            x += ((r * tau0) * rLi[i]) * s.uq[j];
            x -= (((r * tau0) * tau0) * rLi[i]) * rLi[j];
            if (i == j) x += diag;
            bm += t.ga[j] * x;
        }
        E[i] += bm * g.W;
    }
    double bc = s.na * t.divu;
#pragma unroll
    for (int d = 0; d < 3; ++d) bc += (tau0 * rLi[d]) * t.ga[d];
    E[3] += bc * g.W;
}

// v[q] for a q that is not a compile-time constant: selects, no indexed register array
__device__ __forceinline__ double sel4(int q, const double* v) { return q == 0 ? v[0] : q == 1 ? v[1] : q == 2 ? v[2] : v[3]; }

// what the sixteen blocks of a tet share: the convective shape derivatives c_b(q) = u_q . grad N_b and the stabilisation
// parameters at the four quadrature points, the latter with (rho, mu) and with the built-in constants
struct FluidJacTet {
    double c[4][4];              // [q][b]
    double t0[4], t1[4];         // tau0_q, tau1_q with rho_q, mu_q
    double t0b[4], t1b[4];       // with kRHO, kMU
};

__device__ __forceinline__ void fluid_tau(const StepK& sk, double y1, double gg, double tr, double rho, double mu, double& tau0, double& tau1) {
#pragma clang fp contract(off)
    const double nu = mu / rho;
    const double y = y1 + ((3.0 * nu) * nu) * gg;
    tau0 = (1.0 / sqrt(sk.t0 + y)) / rho;
    tau1 = sqrt(y) / tr;
}

__device__ __forceinline__ void fluid_jac_tet(const StepK& sk, const FluidGeom& g, const double (*u)[3], const double* rho, const double* mu,
                                              FluidJacTet& j) {
#pragma clang fp contract(off)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        double uq[3], ub[4];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int b = 0; b < 4; ++b) ub[b] = u[b][i];
            uq[i] = interp_q(q, ub);
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) j.c[q][b] = (uq[0] * g.gN[b][0] + uq[1] * g.gN[b][1]) + uq[2] * g.gN[b][2];
        const double y1 = (j.c[q][1] * j.c[q][1] + j.c[q][2] * j.c[q][2]) + j.c[q][3] * j.c[q][3];  // |J^-1 u_q|^2
        fluid_tau(sk, y1, g.gg, g.tr, rho[q], mu[q], j.t0[q], j.t1[q]);
        fluid_tau(sk, y1, g.gg, g.tr, kRHO, kMU, j.t0b[q], j.t1b[q]);
    }
}

// B[ii * 4 + jj] of node pair (la, lb) (lb a compile-time index after unrolling), coefficients inside the quadrature sums (ascending q, from +0.0)
__device__ __forceinline__ void fluid_tet_B(const StepK& sk, const FluidGeom& g, const double (*cq)[4], int la, int lb, const double* rho,
                                            const double* mu, const double* t0, const double* t1, double* B) {
#pragma clang fp contract(off)
    const double f1 = kALPHAM, f2 = sk.fact2;
    double ga[3];  // (la is the lane's own: selects, no indexed register array)
#pragma unroll
    for (int d = 0; d < 3; ++d) ga[d] = la == 0 ? g.gN[0][d] : la == 1 ? g.gN[1][d] : la == 2 ? g.gN[2][d] : g.gN[3][d];
    const double* gb = g.gN[lb];
    const double eK = (ga[0] * gb[0] + ga[1] * gb[1]) + ga[2] * gb[2];
    double S_d = 0.0, S_mu = 0.0, S_rt1 = 0.0, S_sb = 0.0, S_sa = 0.0, S_rt0ca = 0.0, S_u0 = 0.0, S_t0 = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double sa = shl(la, q), sb = shl(lb, q), cb = cq[q][lb];
        const double ca = la == 0 ? cq[q][0] : la == 1 ? cq[q][1] : la == 2 ? cq[q][2] : cq[q][3];
        const double r = rho[q], rt0 = r * t0[q];
        S_d += ((((f1 * r) * sa) * sb + ((f1 * r) * (rt0 * ca)) * sb) + ((f2 * r) * sa) * cb) + (((f2 * r) * (rt0 * ca)) * cb + (f2 * mu[q]) * eK);
        S_mu += mu[q];
        S_rt1 += r * t1[q];
        S_sb += sb;
        S_sa += sa;
        S_rt0ca += rt0 * ca;
        S_u0 += rt0 * (f1 * sb + f2 * cb);
        S_t0 += t0[q];
    }
    const double diag = g.W * S_d;
    const double cK = (f2 * g.W) * S_mu, cT = (f2 * g.W) * S_rt1;
#pragma unroll
    for (int ii = 0; ii < 3; ++ii)
#pragma unroll
        for (int jj = 0; jj < 3; ++jj) {
            const double t = (cK * ga[jj]) * gb[ii] + (cT * ga[ii]) * gb[jj];
            B[ii * 4 + jj] = ii == jj ? t + diag : t;
        }
    const double cP0 = g.W * S_sb, cP1 = g.W * S_rt0ca;
    const double cU0 = g.W * S_u0, cU1 = (g.W * f2) * S_sa;
#pragma unroll
    for (int ii = 0; ii < 3; ++ii) {
        B[ii * 4 + 3] = cP1 * gb[ii] - cP0 * ga[ii];
        B[12 + ii] = cU0 * ga[ii] + cU1 * gb[ii];
    }
    B[15] = (g.W * eK) * S_t0;
}

}  // namespace
