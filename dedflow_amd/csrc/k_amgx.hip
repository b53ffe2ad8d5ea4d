// Kernels of PC_AMGX (host/pc_amgx.c): setup and V-cycle of a scalar pairwise-aggregation AMG with multicolour-DILU or
// Jacobi smoothing and a dense LU on the coarsest level.
//
// Every row operation is a __device__ function used twice: by the grid kernels of the large levels (one thread per row,
// one launch per colour) and by the two one-workgroup tail kernels that walk all small levels inside one launch with
// __syncthreads between the phases (no grid-wide barrier, no inter-workgroup flag).  Each value is written by exactly one
// thread and every sum runs in a fixed order (row order, host-built lists): two applications are bitwise equal.
#include "dfl_common.hpp"

namespace {

constexpr int BLK = 256;
constexpr int TAIL = 1024;
typedef dfl_amgx_level Lev;

// ---- setup rows ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void galerkin_nz(const Lev& c, const T* __restrict__ vf, I k) {
    double s = 0.0;
    for (I t = c.goff[k]; t < c.goff[k + 1]; ++t) s += vf[c.gidx[t]];
    c.val[k] = s;
}
// E_i = a_ii - sum_{j in N(i), colour(j) < colour(i)} a_ij a_ji / E_j; |E_i| < 1e-12 |a_ii| -> a_ii
__device__ __forceinline__ void dilu_setup_row(const Lev& L, I i, I col) {
    double s = 0.0;
    for (I k = L.rp[i]; k < L.rp[i + 1]; ++k) {
        const I j = L.ci[k], t = L.trans[k];
        if (L.color[j] < col && t >= 0) s += L.val[k] * L.val[t] * L.einv[j];
    }
    const double aii = L.val[L.diag[i]];
    double e = aii - s;
    if (fabs(e) < 1e-12 * fabs(aii)) e = aii;
    L.einv[i] = 1.0 / e;
}
__device__ __forceinline__ void jacobi_setup_row(const Lev& L, I i) { L.einv[i] = 1.0 / L.val[L.diag[i]]; }

// ---- cycle rows ---------------------------------------------------------------------------------------------------------
// forward colour: w_i = ((b_i - (A x)_i) - sum_{colour(j) < col} a_ij w_j) / E_i in one walk over row i
__device__ __forceinline__ void dilu_fwd_row(const Lev& L, const T* __restrict__ b, const T* __restrict__ x, T* w, I i, I col,
                                             bool xz) {
    double ax = 0.0, sl = 0.0;
    for (I k = L.rp[i]; k < L.rp[i + 1]; ++k) {
        const I j = L.ci[k];
        const double a = L.val[k];
        if (!xz) ax += a * x[j];
        if (L.color[j] < col) sl += a * w[j];
    }
    w[i] = ((b[i] - ax) - sl) * L.einv[i];
}
// backward colour: w_i -= E_i^-1 sum_{colour(j) > col} a_ij w_j;  x_i += omega w_i
__device__ __forceinline__ void dilu_bwd_row(const Lev& L, T* x, T* w, I i, I col, double omega, bool xz) {
    double su = 0.0;
    for (I k = L.rp[i]; k < L.rp[i + 1]; ++k) {
        const I j = L.ci[k];
        if (L.color[j] > col) su += L.val[k] * w[j];
    }
    const double z = w[i] - L.einv[i] * su;
    w[i] = z;
    x[i] = (xz ? 0.0 : x[i]) + omega * z;
}
__device__ __forceinline__ void jacobi_row(const Lev& L, const T* __restrict__ b, const T* __restrict__ x, T* __restrict__ xn, I i,
                                           double omega, bool xz) {
    double ax = 0.0;
    if (!xz)
        for (I k = L.rp[i]; k < L.rp[i + 1]; ++k) ax += L.val[k] * x[L.ci[k]];
    xn[i] = (xz ? 0.0 : x[i]) + omega * L.einv[i] * (b[i] - ax);
}
// bc_I = sum over the members m of I (ascending) of (b_m - (A x)_m)
__device__ __forceinline__ void restrict_row(const Lev& L, const T* __restrict__ b, const T* __restrict__ x, T* __restrict__ bc, I c,
                                             bool xz) {
    double s = 0.0;
    for (I t = L.aoff[c]; t < L.aoff[c + 1]; ++t) {
        const I m = L.amem[t];
        double r = b[m];
        if (!xz) {
            double ax = 0.0;
            for (I k = L.rp[m]; k < L.rp[m + 1]; ++k) ax += L.val[k] * x[L.ci[k]];
            r -= ax;
        }
        s += r;
    }
    bc[c] = s;
}
__device__ __forceinline__ void prolong_row(const Lev& L, T* x, const T* __restrict__ xc, I i, bool xz) {
    x[i] = (xz ? 0.0 : x[i]) + xc[L.agg[i]];
}

// ---- grid kernels --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLK) void gather_a11_kernel(I nnz, const T* __restrict__ bv, T* __restrict__ v) {
    const long long k = (long long)blockIdx.x * BLK + threadIdx.x;
    if (k < nnz) v[k] = bv[k * 16 + 15];
}
__global__ __launch_bounds__(BLK) void galerkin_kernel(Lev c, const T* __restrict__ vf) {
    const I k = blockIdx.x * BLK + threadIdx.x;
    if (k < c.nnz) galerkin_nz(c, vf, k);
}
__global__ __launch_bounds__(BLK) void dilu_setup_kernel(Lev L, I s0, I cnt, I col) {
    const I t = blockIdx.x * BLK + threadIdx.x;
    if (t < cnt) dilu_setup_row(L, L.rows[s0 + t], col);
}
__global__ __launch_bounds__(BLK) void jacobi_setup_kernel(Lev L) {
    const I i = blockIdx.x * BLK + threadIdx.x;
    if (i < L.n) jacobi_setup_row(L, i);
}
__global__ __launch_bounds__(BLK) void dilu_fwd_kernel(Lev L, I s0, I cnt, I col, int xz) {
    const I t = blockIdx.x * BLK + threadIdx.x;
    if (t < cnt) dilu_fwd_row(L, L.b, L.x, L.w, L.rows[s0 + t], col, xz != 0);
}
__global__ __launch_bounds__(BLK) void dilu_bwd_kernel(Lev L, I s0, I cnt, I col, double omega, int xz) {
    const I t = blockIdx.x * BLK + threadIdx.x;
    if (t < cnt) dilu_bwd_row(L, L.x, L.w, L.rows[s0 + t], col, omega, xz != 0);
}
__global__ __launch_bounds__(BLK) void jacobi_kernel(Lev L, double omega, int xz) {
    const I i = blockIdx.x * BLK + threadIdx.x;
    if (i < L.n) jacobi_row(L, L.b, L.x, L.w, i, omega, xz != 0);
}
__global__ __launch_bounds__(BLK) void restrict_kernel(Lev L, T* __restrict__ bc, int xz) {
    const I c = blockIdx.x * BLK + threadIdx.x;
    if (c < L.nc) restrict_row(L, L.b, L.x, bc, c, xz != 0);
}
__global__ __launch_bounds__(BLK) void prolong_kernel(Lev L, const T* __restrict__ xc, int xz) {
    const I i = blockIdx.x * BLK + threadIdx.x;
    if (i < L.n) prolong_row(L, L.x, xc, i, xz != 0);
}
__global__ __launch_bounds__(BLK) void residual_kernel(Lev L, const T* __restrict__ r, const T* __restrict__ z, T* __restrict__ t) {
    const I i = blockIdx.x * BLK + threadIdx.x;
    if (i >= L.n) return;
    double ax = 0.0;
    for (I k = L.rp[i]; k < L.rp[i + 1]; ++k) ax += L.val[k] * z[L.ci[k]];
    t[i] = r[i] - ax;
}

// ---- tail (one workgroup) -------------------------------------------------------------------------------------------------
__device__ void tail_smoother_setup(const Lev& L, bool jacobi) {
    if (jacobi) {
        for (I i = threadIdx.x; i < L.n; i += TAIL) jacobi_setup_row(L, i);
        __syncthreads();
        return;
    }
    for (I c = 0; c < L.ncolor; ++c) {
        const I s0 = L.coff[c], cnt = L.coff[c + 1] - s0;
        for (I t = threadIdx.x; t < cnt; t += TAIL) dilu_setup_row(L, L.rows[s0 + t], c);
        __syncthreads();
    }
}

// dense LU with partial pivoting (largest |value|, lowest row on a tie).  A pivot with |u_kk| <= 1e-12 max_{j<=k} |u_jj|
// counts as zero: no elimination with it (its multipliers are 0), and the solve sets its unknown to 0.
__device__ void tail_lu_factor(const Lev& L) {
    __shared__ double sv[TAIL];
    __shared__ I sr[TAIL];
    __shared__ double runmax;
    const I n = L.n, tid = threadIdx.x;
    double* a = L.lu;
    for (long long e = tid; e < (long long)n * n; e += TAIL) a[e] = 0.0;
    __syncthreads();
    for (I i = tid; i < n; i += TAIL)
        for (I k = L.rp[i]; k < L.rp[i + 1]; ++k) a[(long long)i * n + L.ci[k]] = L.val[k];
    if (tid == 0) runmax = 0.0;
    __syncthreads();
    for (I k = 0; k < n; ++k) {
        double bv = -1.0;
        I br = n;
        for (I i = k + tid; i < n; i += TAIL) {
            const double v = fabs(a[(long long)i * n + k]);
            if (v > bv) { bv = v; br = i; }  // ascending i: the first of equal values stays
        }
        sv[tid] = bv;
        sr[tid] = br;
        __syncthreads();
        for (int s = TAIL / 2; s > 0; s >>= 1) {
            if (tid < s) {
                const double v2 = sv[tid + s];
                const I r2 = sr[tid + s];
                if (v2 > sv[tid] || (v2 == sv[tid] && r2 < sr[tid])) { sv[tid] = v2; sr[tid] = r2; }
            }
            __syncthreads();
        }
        const I p = sr[0];
        const double pv = sv[0];
        if (tid == 0) {
            L.piv[k] = p;
            runmax = fmax(runmax, pv);
            L.zpiv[k] = (pv <= 1e-12 * runmax) ? 1 : 0;
        }
        __syncthreads();
        if (p != k)
            for (I j = tid; j < n; j += TAIL) {
                const double t = a[(long long)k * n + j];
                a[(long long)k * n + j] = a[(long long)p * n + j];
                a[(long long)p * n + j] = t;
            }
        __syncthreads();
        const bool zero = L.zpiv[k] != 0;
        const double ukk = a[(long long)k * n + k];
        for (I i = k + 1 + tid; i < n; i += TAIL) a[(long long)i * n + k] = zero ? 0.0 : a[(long long)i * n + k] / ukk;
        __syncthreads();
        if (!zero) {
            const I m = n - k - 1;
            for (long long e = tid; e < (long long)m * m; e += TAIL) {
                const I i = k + 1 + (I)(e / m), j = k + 1 + (I)(e % m);
                a[(long long)i * n + j] -= a[(long long)i * n + k] * a[(long long)k * n + j];
            }
        }
        __syncthreads();
    }
}

__device__ void tail_lu_solve(const Lev& L, const T* b, T* x) {
    const I n = L.n, tid = threadIdx.x;
    const double* a = L.lu;
    for (I i = tid; i < n; i += TAIL) x[i] = b[i];
    __syncthreads();
    if (tid == 0)
        for (I k = 0; k < n; ++k) {
            const I p = L.piv[k];
            if (p != k) { const double t = x[k]; x[k] = x[p]; x[p] = t; }
        }
    __syncthreads();
    for (I k = 0; k < n; ++k) {  // L y = P b, unit diagonal
        const double xk = x[k];
        for (I i = k + 1 + tid; i < n; i += TAIL) x[i] -= a[(long long)i * n + k] * xk;
        __syncthreads();
    }
    for (I k = n - 1; k >= 0; --k) {  // U x = y; zero pivots: x_k = 0
        if (tid == 0) x[k] = L.zpiv[k] ? 0.0 : x[k] / a[(long long)k * n + k];
        __syncthreads();
        const double xk = x[k];
        if (xk != 0.0)
            for (I i = tid; i < k; i += TAIL) x[i] -= a[(long long)i * n + k] * xk;
        __syncthreads();
    }
}

__device__ void tail_smooth(const Lev& L, const T* b, T*& x, T*& w, bool jacobi, double omega, bool xz) {
    if (jacobi) {
        for (I i = threadIdx.x; i < L.n; i += TAIL) jacobi_row(L, b, x, w, i, omega, xz);
        __syncthreads();
        T* t = x;
        x = w;
        w = t;
        return;
    }
    for (I c = 0; c < L.ncolor; ++c) {
        const I s0 = L.coff[c], cnt = L.coff[c + 1] - s0;
        for (I t = threadIdx.x; t < cnt; t += TAIL) dilu_fwd_row(L, b, x, w, L.rows[s0 + t], c, xz);
        __syncthreads();
    }
    for (I c = L.ncolor - 1; c >= 0; --c) {
        const I s0 = L.coff[c], cnt = L.coff[c + 1] - s0;
        for (I t = threadIdx.x; t < cnt; t += TAIL) dilu_bwd_row(L, x, w, L.rows[s0 + t], c, omega, xz);
        __syncthreads();
    }
}

__global__ __launch_bounds__(TAIL) void tail_setup_kernel(const Lev* __restrict__ lev, I l0, I nlev, int jacobi) {
    for (I l = l0; l < nlev; ++l) {
        const Lev L = lev[l];
        if (l >= 1) {
            const T* vf = lev[l - 1].val;
            for (I k = threadIdx.x; k < L.nnz; k += TAIL) galerkin_nz(L, vf, k);
            __syncthreads();
        }
        if (l < nlev - 1) tail_smoother_setup(L, jacobi != 0);
        else tail_lu_factor(L);
    }
}

// where level l's iterate is after `sweeps` smoothing steps that started in x (Jacobi alternates between x and w)
__device__ __forceinline__ T* iterate_after(T* x, T* w, bool jacobi, int sweeps) { return (jacobi && (sweeps & 1)) ? w : x; }

__global__ __launch_bounds__(TAIL) void tail_cycle_kernel(const Lev* __restrict__ lev, I l0, I nlev, int jacobi, int pre, int post,
                                                          double omega, const T* b0, T* x0, T* w0) {
    const bool jac = jacobi != 0;
    // down: presweeps, restriction
    for (I l = l0; l < nlev - 1; ++l) {
        const Lev L = lev[l];
        const T* b = l == l0 ? b0 : L.b;
        T* x = l == l0 ? x0 : L.x;
        T* w = l == l0 ? w0 : L.w;
        for (int s = 0; s < pre; ++s) tail_smooth(L, b, x, w, jac, omega, s == 0);
        T* bc = lev[l + 1].b;
        for (I c = threadIdx.x; c < L.nc; c += TAIL) restrict_row(L, b, x, bc, c, pre == 0);
        __syncthreads();
    }
    {
        const Lev L = lev[nlev - 1];
        tail_lu_solve(L, nlev - 1 == l0 ? b0 : L.b, nlev - 1 == l0 ? x0 : L.x);
    }
    // up: prolongation, postsweeps
    for (I l = nlev - 2; l >= l0; --l) {
        const Lev L = lev[l];
        const T* b = l == l0 ? b0 : L.b;
        T* x = l == l0 ? x0 : L.x;
        T* w = l == l0 ? w0 : L.w;
        if (jac && (pre & 1)) { T* t = x; x = w; w = t; }
        const Lev C = lev[l + 1];
        const T* xc = (l + 1 == nlev - 1) ? C.x : iterate_after(C.x, C.w, jac, pre + post);
        for (I i = threadIdx.x; i < L.n; i += TAIL) prolong_row(L, x, xc, i, pre == 0);
        __syncthreads();
        for (int s = 0; s < post; ++s) tail_smooth(L, b, x, w, jac, omega, false);
    }
}

}  // namespace

extern "C" {

void dfl_amgx_gather_a11(I nnz, const T* block_val, T* val, void* stream) {
    if (nnz <= 0) return;
    gather_a11_kernel<<<ceil_div(nnz, BLK), BLK, 0, S(stream)>>>(nnz, block_val, val);
    DFL_LAUNCH_CHECK();
}
void dfl_amgx_galerkin(Lev c, const T* vf, void* stream) {
    if (c.nnz <= 0) return;
    galerkin_kernel<<<ceil_div(c.nnz, BLK), BLK, 0, S(stream)>>>(c, vf);
    DFL_LAUNCH_CHECK();
}
void dfl_amgx_dilu_setup_color(Lev L, I color, I s0, I cnt, void* stream) {
    if (cnt <= 0) return;
    dilu_setup_kernel<<<ceil_div(cnt, BLK), BLK, 0, S(stream)>>>(L, s0, cnt, color);
    DFL_LAUNCH_CHECK();
}
void dfl_amgx_dilu_forward(Lev L, I color, I s0, I cnt, int x_zero, void* stream) {
    if (cnt <= 0) return;
    dilu_fwd_kernel<<<ceil_div(cnt, BLK), BLK, 0, S(stream)>>>(L, s0, cnt, color, x_zero);
    DFL_LAUNCH_CHECK();
}
void dfl_amgx_dilu_backward(Lev L, I color, I s0, I cnt, T omega, int x_zero, void* stream) {
    if (cnt <= 0) return;
    dilu_bwd_kernel<<<ceil_div(cnt, BLK), BLK, 0, S(stream)>>>(L, s0, cnt, color, omega, x_zero);
    DFL_LAUNCH_CHECK();
}
void dfl_amgx_jacobi_setup(Lev L, void* stream) {
    if (L.n <= 0) return;
    jacobi_setup_kernel<<<ceil_div(L.n, BLK), BLK, 0, S(stream)>>>(L);
    DFL_LAUNCH_CHECK();
}
void dfl_amgx_jacobi_sweep(Lev L, T omega, int x_zero, void* stream) {
    if (L.n <= 0) return;
    jacobi_kernel<<<ceil_div(L.n, BLK), BLK, 0, S(stream)>>>(L, omega, x_zero);
    DFL_LAUNCH_CHECK();
}
void dfl_amgx_restrict(Lev L, Lev c, int x_zero, void* stream) {
    if (L.nc <= 0) return;
    restrict_kernel<<<ceil_div(L.nc, BLK), BLK, 0, S(stream)>>>(L, c.b, x_zero);
    DFL_LAUNCH_CHECK();
}
void dfl_amgx_prolong(Lev L, const T* xc, int x_zero, void* stream) {
    if (L.n <= 0) return;
    prolong_kernel<<<ceil_div(L.n, BLK), BLK, 0, S(stream)>>>(L, xc, x_zero);
    DFL_LAUNCH_CHECK();
}
void dfl_amgx_residual(Lev L, const T* r, const T* z, T* t, void* stream) {
    if (L.n <= 0) return;
    residual_kernel<<<ceil_div(L.n, BLK), BLK, 0, S(stream)>>>(L, r, z, t);
    DFL_LAUNCH_CHECK();
}
void dfl_amgx_tail_setup(const Lev* levels, I l0, I nlev, int jacobi, void* stream) {
    tail_setup_kernel<<<1, TAIL, 0, S(stream)>>>(levels, l0, nlev, jacobi);
    DFL_LAUNCH_CHECK();
}
void dfl_amgx_tail_cycle(const Lev* levels, I l0, I nlev, int jacobi, int presweeps, int postsweeps, T omega, const T* b0, T* x0,
                         T* w0, void* stream) {
    tail_cycle_kernel<<<1, TAIL, 0, S(stream)>>>(levels, l0, nlev, jacobi, presweeps, postsweeps, omega, b0, x0, w0);
    DFL_LAUNCH_CHECK();
}

}  // extern "C"
