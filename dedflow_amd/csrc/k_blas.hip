// BLAS-1, deterministic reductions, fused classical Gram-Schmidt and the GMRES
// small recurrences -- replaces the cuBLAS calls of src/krylov.c:114-319,
// src/main.c:107-130 and the elementwise kernels of src/vec.cu:14-76.
// All of these are HBM-bound streams: 16-byte accesses per lane, grid sized to
// a few blocks per CU, two-stage (order-fixed) reductions instead of atomics so
// that Krylov residual histories are bitwise reproducible run to run.
#include "dfl_common.hpp"
#include <cmath>

static char g_err[512] = "";
void dfl_record_error(hipError_t e, const char* file, int line) {
    snprintf(g_err, sizeof g_err, "HIP error: %s at %s:%d", hipGetErrorString(e), file, line);
    fprintf(stderr, "GPUAssert: %s\n", g_err);
}

namespace {

constexpr int BLK = 256;
constexpr int MAX_PART = 1024;  // stage-1 partials of a reduction

template <class F>
__global__ __launch_bounds__(BLK) void map1(I n, T* x, F f) {
    long long i = (long long)blockIdx.x * BLK + threadIdx.x;
    long long n2 = n >> 1;
    if (i < n2) {
        double2 v = reinterpret_cast<double2*>(x)[i];
        v.x = f(v.x);
        v.y = f(v.y);
        reinterpret_cast<double2*>(x)[i] = v;
    }
    if (i == 0 && (n & 1)) x[n - 1] = f(x[n - 1]);
}

template <class F>
__global__ __launch_bounds__(BLK) void map3(I n, const T* a, const T* b, T* c, F f) {
    long long i = (long long)blockIdx.x * BLK + threadIdx.x;
    long long n2 = n >> 1;
    if (i < n2) {
        double2 u = reinterpret_cast<const double2*>(a)[i];
        double2 v = reinterpret_cast<const double2*>(b)[i];
        double2 r;
        r.x = f(u.x, v.x);
        r.y = f(u.y, v.y);
        reinterpret_cast<double2*>(c)[i] = r;
    }
    if (i == 0 && (n & 1)) c[n - 1] = f(a[n - 1], b[n - 1]);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <class F>
__global__ __launch_bounds__(BLK) void map1_scalar(I n, T* x, F f) {
    long long i = (long long)blockIdx.x * BLK + threadIdx.x;
    if (i < n) x[i] = f(x[i]);
}
template <class F>
__global__ __launch_bounds__(BLK) void map3_scalar(I n, const T* a, const T* b, T* c, F f) {
    long long i = (long long)blockIdx.x * BLK + threadIdx.x;
    if (i < n) c[i] = f(a[i], b[i]);
}

template <class F>
void launch_map1(I n, T* x, F f, void* stream) {
    if (n <= 0) return;
    if (aligned16(x)) map1<<<ceil_div((n >> 1) + 1, BLK), BLK, 0, S(stream)>>>(n, x, f);
    else map1_scalar<<<ceil_div(n, BLK), BLK, 0, S(stream)>>>(n, x, f);
    DFL_LAUNCH_CHECK();
}
template <class F>
void launch_map3(I n, const T* a, const T* b, T* c, F f, void* stream) {
    if (n <= 0) return;
    if (aligned16(a) && aligned16(b) && aligned16(c)) map3<<<ceil_div((n >> 1) + 1, BLK), BLK, 0, S(stream)>>>(n, a, b, c, f);
    else map3_scalar<<<ceil_div(n, BLK), BLK, 0, S(stream)>>>(n, a, b, c, f);
    DFL_LAUNCH_CHECK();
}

// ---- reductions ----------------------------------------------------------------
template <bool DOT>
__global__ __launch_bounds__(BLK) void reduce_stage1(I n, const T* x, const T* y, T* part) {
    __shared__ double lds[4];
    double acc = 0.0;
    const long long stride = (long long)gridDim.x * BLK;
    for (long long i = (long long)blockIdx.x * BLK + threadIdx.x; i < n; i += stride) {
        double a = x[i];
        acc += DOT ? a * y[i] : a * a;
    }
    double r = block_sum_256(acc, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = r;
}

template <bool SQRT>
__global__ __launch_bounds__(BLK) void reduce_stage2(int npart, const T* part, T* out) {
    __shared__ double lds[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < npart; i += BLK) acc += part[i];
    double r = block_sum_256(acc, lds);
    if (threadIdx.x == 0) out[0] = SQRT ? sqrt(r) : r;
}

__global__ __launch_bounds__(BLK) void scal_inv_dev(I n, const T* d_scale, T* x) {
    const double s = 1.0 / d_scale[0];
    long long i = (long long)blockIdx.x * BLK + threadIdx.x;
    long long n2 = n >> 1;
    if (i < n2) {
        double2 v = reinterpret_cast<double2*>(x)[i];
        v.x *= s;
        v.y *= s;
        reinterpret_cast<double2*>(x)[i] = v;
    }
    if (i == 0 && (n & 1)) x[n - 1] *= s;
}

// Krylov basis columns are streamed once per pass (2.3 GB at 10M tets, m = 40): nontemporal
// loads keep them from displacing w and the partial sums in L2 / MALL.
typedef double d2s __attribute__((ext_vector_type(2)));
__device__ __forceinline__ double2 ld_stream(const T* p) {
    const d2s v = __builtin_nontemporal_load(reinterpret_cast<const d2s*>(p));
    return make_double2(v.x, v.y);
}

// ---- fused CGS -------------------------------------------------------------------
// d_h[j] = Q[:,j].w : grid (row blocks, column tiles of CT); each thread owns
// RPT double2 row slots, keeps w in registers across the CT columns of its tile.
constexpr int CT = 8;
constexpr int RPT = 4;                      // double2 slots per thread
constexpr int ROWS_PER_BLOCK = BLK * RPT * 2;  // 2048 rows

__global__ __launch_bounds__(BLK) void cgs_dots_stage1(I n, I ncol, const T* __restrict__ Q, long long ldq,
                                                      const T* __restrict__ w, T* __restrict__ part, int nrb, int ct) {
    __shared__ double lds[4];
    const long long r0 = (long long)blockIdx.x * ROWS_PER_BLOCK;
    const int c0 = blockIdx.y * ct;
    double2 wv[RPT];
    long long row[RPT];
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
        row[i] = r0 + 2LL * threadIdx.x + (long long)i * (2 * BLK);
        if (row[i] + 1 < n) wv[i] = *reinterpret_cast<const double2*>(w + row[i]);
        else { wv[i].x = (row[i] < n) ? w[row[i]] : 0.0; wv[i].y = 0.0; }
    }
    for (int c = 0; c < ct; ++c) {
        const int col = c0 + c;
        if (col >= ncol) break;  // uniform
        const T* q = Q + (long long)col * ldq;
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
            double2 qv;
            if (row[i] + 1 < n) qv = ld_stream(q + row[i]);
            else { qv.x = (row[i] < n) ? q[row[i]] : 0.0; qv.y = 0.0; }
            acc += qv.x * wv[i].x + qv.y * wv[i].y;
        }
        double r = block_sum_256(acc, lds);
        if (threadIdx.x == 0) part[(long long)col * nrb + blockIdx.x] = r;
    }
}

__global__ __launch_bounds__(BLK) void cgs_dots_stage2(int nrb, const T* part, T* d_h) {
    __shared__ double lds[4];
    const T* p = part + (long long)blockIdx.x * nrb;
    double acc = 0.0;
    for (int i = threadIdx.x; i < nrb; i += BLK) acc += p[i];
    double r = block_sum_256(acc, lds);
    if (threadIdx.x == 0) d_h[blockIdx.x] = r;
}

// w -= Q h (SUB) or y = Q c (!SUB); optional partial ||w||^2 per block
constexpr int UPT = 2;  // double2 slots per thread (1 and 4 measured: 0.2093 against 0.2028 ms per CGS kernel)
constexpr int UROWS = BLK * UPT * 2;
template <bool SUB>
__global__ __launch_bounds__(BLK) void cgs_update_kernel(I n, I ncol, const T* __restrict__ Q, long long ldq,
                                                        const T* __restrict__ d_h, T* __restrict__ w, T* __restrict__ part) {
    __shared__ double lds[4];
    __shared__ double sh[128];
    for (int j = threadIdx.x; j < ncol && j < 128; j += BLK) sh[j] = d_h[j];
    __syncthreads();
    const long long blk = blockIdx.x;
    const long long r0 = blk * UROWS;
    long long row[UPT];
    double2 acc[UPT];
#pragma unroll
    for (int i = 0; i < UPT; ++i) {
        row[i] = r0 + 2LL * threadIdx.x + (long long)i * (2 * BLK);
        if (SUB) {
            if (row[i] + 1 < n) acc[i] = *reinterpret_cast<const double2*>(w + row[i]);
            else { acc[i].x = (row[i] < n) ? w[row[i]] : 0.0; acc[i].y = 0.0; }
        } else { acc[i].x = 0.0; acc[i].y = 0.0; }
    }
#pragma unroll 4  // (8 columns in flight: 0.212 against 0.205 ms per CGS kernel -- slower)
    for (int j = 0; j < ncol; ++j) {
        const double h = (j < 128) ? sh[j] : d_h[j];
        const T* q = Q + (long long)j * ldq;
#pragma unroll
        for (int i = 0; i < UPT; ++i) {
            double2 qv;
            if (row[i] + 1 < n) qv = ld_stream(q + row[i]);
            else { qv.x = (row[i] < n) ? q[row[i]] : 0.0; qv.y = 0.0; }
            if (SUB) { acc[i].x -= qv.x * h; acc[i].y -= qv.y * h; }
            else { acc[i].x += qv.x * h; acc[i].y += qv.y * h; }
        }
    }
    double ss = 0.0;
#pragma unroll
    for (int i = 0; i < UPT; ++i) {
        if (row[i] + 1 < n) *reinterpret_cast<double2*>(w + row[i]) = acc[i];
        else if (row[i] < n) w[row[i]] = acc[i].x;
        ss += acc[i].x * acc[i].x + acc[i].y * acc[i].y;
    }
    if (part) {
        double r = block_sum_256(ss, lds);
        if (threadIdx.x == 0 && blk < gridDim.x) part[blk] = r;  // (the bound always holds; kept: the kernel stays as measured)
    }
}

// ---- GMRES recurrences (single lane; O(k) flops) ----------------------------------
__device__ void drotg_dev(double* a, double* b, double* c, double* s) {
    double roe = *b;
    if (fabs(*a) > fabs(*b)) roe = *a;
    double scale = fabs(*a) + fabs(*b), r, z;
    if (scale == 0.0) { *c = 1.0; *s = 0.0; r = 0.0; z = 0.0; }
    else {
        double ta = *a / scale, tb = *b / scale;
        r = scale * sqrt(ta * ta + tb * tb);
        r = (roe < 0.0 ? -1.0 : 1.0) * r;
        *c = *a / r; *s = *b / r; z = 1.0;
        if (fabs(*a) > fabs(*b)) z = *s;
        if (fabs(*b) >= fabs(*a) && *c != 0.0) z = 1.0 / *c;
    }
    *a = r; *b = z;
}

// The Givens step of column `iter` (krylov.c:256-277, krylov_util.cu:5-19), called by a whole workgroup: the column and
// the earlier rotations are staged in LDS with coalesced loads first (a single thread walking them in global memory
// pays one dependent load latency per entry), thread 0 runs the O(iter) recurrence on the staged copy, the column is
// written back by all threads.  `nrm` = ||w||.
constexpr int GIV_MAX = 1024;  // columns longer than this fall back to the in-place walk
__device__ void givens_step_block(I iter, double nrm, T* H, I ldh, T* gv, T* beta, T* res_hist, double* s_col, double* s_gv) {
    T* col = H + (long long)iter * ldh;
    const int t = threadIdx.x, nt = blockDim.x;
    const bool staged = iter + 2 <= GIV_MAX;
    if (staged) {
        for (int i = t; i <= iter; i += nt) s_col[i] = col[i];
        for (int i = t; i < 2 * iter; i += nt) s_gv[i] = gv[i];
        __syncthreads();
    }
    if (t == 0) {
        double* c_ = staged ? s_col : col;
        const double* g_ = staged ? s_gv : gv;
        c_[iter + 1] = nrm;  // H[iter+1, iter] = ||w||, krylov.c:228-230
        for (I i = 0; i < iter; ++i) {  // cublasDrot(n=1), krylov.c:258-263
            const double c = g_[2 * i], s = g_[2 * i + 1];
            const double x = c_[i], y = c_[i + 1];
            c_[i] = c * x + s * y;
            c_[i + 1] = c * y - s * x;
        }
        double gc, gs;
        drotg_dev(&c_[iter], &c_[iter + 1], &gc, &gs);  // :266
        gv[2 * iter] = gc;
        gv[2 * iter + 1] = gs;
        c_[iter + 1] = 0.0;  // :267
        const double b0 = beta[iter];  // krylov_util.cu:5-19
        beta[iter + 1] = -gs * b0;
        beta[iter] = b0 * gc;
        if (res_hist) res_hist[iter] = fabs(beta[iter + 1]);
    }
    if (staged) {
        __syncthreads();
        for (int i = t; i <= iter + 1; i += nt) col[i] = s_col[i];
    }
}

// SQUARED: *d_nrm holds the (all-reduced) squared norm; it is replaced by its square root first
template <bool SQUARED>
__global__ __launch_bounds__(BLK) void gmres_givens_kernel(I iter, T* d_nrm, T* H, I ldh, T* gv, T* beta, T* res_hist) {
    __shared__ double s_col[GIV_MAX], s_gv[2 * GIV_MAX];
    __shared__ double s_nrm;
    if (threadIdx.x == 0) {
        s_nrm = SQUARED ? sqrt(d_nrm[0]) : d_nrm[0];
        if (SQUARED) d_nrm[0] = s_nrm;
    }
    __syncthreads();
    givens_step_block(iter, s_nrm, H, ldh, gv, beta, res_hist, s_col, s_gv);
}

// Partitioned runs, fused-norm option: column `iter` of H holds the all-reduced h_0..h_iter and, in slot iter+1, the
// all-reduced w.w from the SAME reduction; ||w - Q h||^2 = w.w - sum h_j^2 (Q orthonormal), so the second all-reduce of an
// Arnoldi step disappears.  Cancellation makes this unsafe when ||w - Qh|| << ||w||: *d_flag is raised when less than
// 1e-6 of w.w is left (the caller then knows the history is unreliable and can switch the option off).
__global__ __launch_bounds__(BLK) void gmres_givens_pythagoras_kernel(I iter, T* d_nrm, T* H, I ldh, T* gv, T* beta, T* res_hist,
                                                                     int* d_flag) {
    __shared__ double s_col[GIV_MAX], s_gv[2 * GIV_MAX];
    __shared__ double s_nrm;
    if (threadIdx.x == 0) {
        const T* col = H + (long long)iter * ldh;
        const double ww = col[iter + 1];
        double hh = 0.0;
        for (I j = 0; j <= iter; ++j) hh += col[j] * col[j];
        double r = ww - hh;
        if (r < 1e-6 * ww) {
            if (d_flag) *d_flag = 1;
            if (r < 0.0) r = 0.0;
        }
        s_nrm = sqrt(r);
        d_nrm[0] = s_nrm;
    }
    __syncthreads();
    givens_step_block(iter, s_nrm, H, ldh, gv, beta, res_hist, s_col, s_gv);
}

// second stage of ||w||^2 (partials of cgs_update_kernel, same fixed order as reduce_stage2) + square root + the Givens
// step in one launch: one kernel boundary less per Arnoldi step
// raw_col != NULL: the column as it is before the rotations, h[0..iter] and the norm, is kept there (the paired step's
// recurrence reads the un-rotated Hessenberg matrix)
__global__ __launch_bounds__(BLK) void norm_givens_kernel(int npart, const T* part, T* d_nrm, I iter, T* H, I ldh, T* gv, T* beta,
                                                         T* res_hist, T* raw_col) {
    __shared__ double lds[4];
    __shared__ double s_nrm;
    __shared__ double s_col[GIV_MAX], s_gv[2 * GIV_MAX];
    double acc = 0.0;
    for (int i = threadIdx.x; i < npart; i += BLK) acc += part[i];
    const double r = block_sum_256(acc, lds);
    if (threadIdx.x == 0) {
        s_nrm = sqrt(r);
        d_nrm[0] = s_nrm;
        if (raw_col) raw_col[iter + 1] = s_nrm;
    }
    if (raw_col) {
        const T* col = H + (long long)iter * ldh;
        for (int i = threadIdx.x; i <= iter; i += BLK) raw_col[i] = col[i];
    }
    __syncthreads();
    givens_step_block(iter, s_nrm, H, ldh, gv, beta, res_hist, s_col, s_gv);
}

// Partitioned runs with the fused norm and the Jacobi tree: the raw column hraw = [h_0 .. h_iter, w.w] is complete (all-
// reduced) BEFORE the update, so ||w - Q h||^2 = w.w - sum h_j^2 is known up front and three launches collapse into one:
//   cgs_update (w -= Q h)  +  gmres_givens_pythagoras (block 0, on a copy of the column in H)  +  the preconditioner
//   application that opens the NEXT Arnoldi step (q = w / nrm stored as the new basis column, z = M^-1 q).
// One owned node per thread (its 3 velocity rows and its pressure row); every block recomputes the norm from hraw in the
// order of gmres_givens_pythagoras_kernel, so all blocks scale by the same bits.  Ghost rows are never touched (zero).
__global__ __launch_bounds__(BLK) void cgs_update_pc_kernel(I nrows, I N, I ncol, const T* __restrict__ Q, long long ldq,
                                                           const T* __restrict__ hraw, T* __restrict__ w,
                                                           const T* __restrict__ dinv33, const T* __restrict__ dinv1,
                                                           T* __restrict__ z, I iter, T* H, I ldh, T* gv, T* beta, T* res_hist,
                                                           T* d_nrm, int* d_flag, T* __restrict__ z4) {
    __shared__ double sh[GIV_MAX + 2];
    __shared__ double s_col[GIV_MAX], s_gv[2 * GIV_MAX];
    __shared__ double s_nrm;
    for (int j = threadIdx.x; j < ncol + 1 && j < GIV_MAX + 2; j += BLK) sh[j] = hraw[j];
    __syncthreads();
    if (threadIdx.x == 0) {
        const double ww = sh[ncol];
        double hh = 0.0;
        for (I j = 0; j < ncol; ++j) hh += sh[j] * sh[j];
        double r = ww - hh;
        if (r < 1e-6 * ww) {
            if (d_flag && blockIdx.x == 0) *d_flag = 1;
            if (r < 0.0) r = 0.0;
        }
        s_nrm = sqrt(r);
    }
    __syncthreads();
    const double nrm = s_nrm;
    const long long i = (long long)blockIdx.x * BLK + threadIdx.x;
    if (i < nrows) {
        double a0 = w[3 * i], a1 = w[3 * i + 1], a2 = w[3 * i + 2], ap = w[3LL * N + i];
#pragma unroll 4
        for (int j = 0; j < ncol; ++j) {
            const double h = sh[j];
            const T* q = Q + (long long)j * ldq;
            a0 -= __builtin_nontemporal_load(q + 3 * i) * h;
            a1 -= __builtin_nontemporal_load(q + 3 * i + 1) * h;
            a2 -= __builtin_nontemporal_load(q + 3 * i + 2) * h;
            ap -= __builtin_nontemporal_load(q + 3LL * N + i) * h;
        }
        const double s = 1.0 / nrm;
        a0 *= s; a1 *= s; a2 *= s; ap *= s;
        w[3 * i] = a0; w[3 * i + 1] = a1; w[3 * i + 2] = a2; w[3LL * N + i] = ap;
        const T* A = dinv33 + i * 9;
        const double z0 = A[0] * a0 + A[3] * a1 + A[6] * a2, z1 = A[1] * a0 + A[4] * a1 + A[7] * a2;
        const double z2 = A[2] * a0 + A[5] * a1 + A[8] * a2, zp = ap * dinv1[i];
        z[3 * i + 0] = z0;
        z[3 * i + 1] = z1;
        z[3 * i + 2] = z2;
        z[3LL * N + i] = zp;
        if (z4) {  // the interleaved copy the matvec gathers from (dfl_bcsr_spmv_x4)
            double2* o = reinterpret_cast<double2*>(z4 + 4 * i);
            o[0] = make_double2(z0, z1);
            o[1] = make_double2(z2, zp);
        }
    }
    if (blockIdx.x == 0) {  // uniform per block: the barriers inside givens_step_block are safe
        T* col = H + (long long)iter * ldh;
        for (int j = threadIdx.x; j < ncol; j += BLK) col[j] = sh[j];
        if (threadIdx.x == 0) d_nrm[0] = nrm;
        __syncthreads();
        givens_step_block(iter, nrm, H, ldh, gv, beta, res_hist, s_col, s_gv);
    }
}

// ---- raw (unnormalised) basis, one GPU (GMRES_STEP_RAW_BASIS) ---------------------------------------------------------
// Column j of the basis holds r_j = nu_j q_j, nu[] the norms.  The coefficients follow from the raw dots g_j = <r_j, w>:
// h_j = g_j / nu_j goes into H, c_j = h_j / nu_j multiplies r_j in the update.  Same fixed order as cgs_dots_stage2.
__global__ __launch_bounds__(BLK) void cgs_dots_raw_stage2(int nrb, const T* part, const T* __restrict__ nu, T* d_h, T* d_c) {
    __shared__ double lds[4];
    const T* p = part + (long long)blockIdx.x * nrb;
    double acc = 0.0;
    for (int i = threadIdx.x; i < nrb; i += BLK) acc += p[i];
    double r = block_sum_256(acc, lds);
    if (threadIdx.x == 0) {
        const double v = nu[blockIdx.x], h = r / v;
        d_h[blockIdx.x] = h;
        d_c[blockIdx.x] = h / v;
    }
}

// y_j /= nu_j: the triangular-solve result in terms of the raw columns
__global__ __launch_bounds__(BLK) void scale_inv_vec_kernel(I m, const T* __restrict__ nu, T* __restrict__ y) {
    const int j = blockIdx.x * BLK + threadIdx.x;
    if (j < m) y[j] = y[j] / nu[j];
}

// w -= Q c with ||w||^2 partials, as cgs_update_kernel<true>, and (Z4) the Jacobi application of the NEXT Arnoldi step on the
// updated w while it is still in registers: z4[node] = M^-1 w'[node], interleaved for dfl_bcsr_spmv_x4.  A workgroup owns the
// 256 nodes [a, a + 256): 768 u rows at 3a and 256 p rows at 3N + a, 512 double2 slots, two per thread (UPT).  The columns are
// streamed slot-wise with 16-byte nontemporal loads exactly as cgs_update_kernel streams them; the regrouping to one node per
// thread goes through LDS ONCE, after the last column (cgs_update_pc_kernel above maps a node to a thread from the start and
// pays for it with 8-byte column loads).  vec_ok: Q, w 16-byte aligned and ldq even; the p section additionally needs N even.
template <bool Z4>
__global__ __launch_bounds__(BLK) void cgs_update_jacobi_kernel(I N, I ncol, const T* __restrict__ Q, long long ldq,
                                                               const T* __restrict__ d_c, T* __restrict__ w, T* __restrict__ part,
                                                               const T* __restrict__ dinv33, const T* __restrict__ dinv1,
                                                               T* __restrict__ z4, int vec_ok) {
    __shared__ double lds[4];
    __shared__ double sh[128];
    __shared__ double2 sm[Z4 ? BLK * UPT : 1];  // the block's updated rows: [0, 768) u, [768, 1024) p
    for (int j = threadIdx.x; j < ncol && j < 128; j += BLK) sh[j] = d_c[j];
    __syncthreads();
    const long long blk = blockIdx.x;
    const long long a = blk * BLK;
    const long long nb = (N - a < BLK) ? (N - a) : BLK;  // nodes of this block
    long long row[UPT], lim[UPT];
    bool vec[UPT];
    double2 acc[UPT];
#pragma unroll
    for (int i = 0; i < UPT; ++i) {
        const int slot = threadIdx.x + i * BLK;  // slots [0, 384): u rows, [384, 512): p rows
        if (slot < 384) { row[i] = 3 * a + 2LL * slot; lim[i] = 3 * (a + nb); }
        else { row[i] = 3LL * N + a + 2LL * (slot - 384); lim[i] = 3LL * N + a + nb; }
        vec[i] = vec_ok && row[i] + 1 < lim[i] && !(row[i] & 1);
        if (vec[i]) acc[i] = *reinterpret_cast<const double2*>(w + row[i]);
        else { acc[i].x = (row[i] < lim[i]) ? w[row[i]] : 0.0; acc[i].y = (row[i] + 1 < lim[i]) ? w[row[i] + 1] : 0.0; }
    }
#pragma unroll 4
    for (int j = 0; j < ncol; ++j) {
        const double h = (j < 128) ? sh[j] : d_c[j];
        const T* q = Q + (long long)j * ldq;
#pragma unroll
        for (int i = 0; i < UPT; ++i) {
            double2 qv;
            if (vec[i]) qv = ld_stream(q + row[i]);
            else { qv.x = (row[i] < lim[i]) ? q[row[i]] : 0.0; qv.y = (row[i] + 1 < lim[i]) ? q[row[i] + 1] : 0.0; }
            acc[i].x -= qv.x * h; acc[i].y -= qv.y * h;
        }
    }
    double ss = 0.0;
#pragma unroll
    for (int i = 0; i < UPT; ++i) {
        if (vec[i]) *reinterpret_cast<double2*>(w + row[i]) = acc[i];
        else {
            if (row[i] < lim[i]) w[row[i]] = acc[i].x;
            if (row[i] + 1 < lim[i]) w[row[i] + 1] = acc[i].y;
        }
        ss += acc[i].x * acc[i].x + acc[i].y * acc[i].y;
        if (Z4) sm[threadIdx.x + i * BLK] = acc[i];
    }
    const double r = block_sum_256(ss, lds);  // (its barriers also publish sm)
    if (threadIdx.x == 0) part[blk] = r;
    if (Z4) {
        const double* s = reinterpret_cast<const double*>(sm);
        const int t = threadIdx.x;
        if (t < nb) {
            const long long i = a + t;
            const T* A = dinv33 + i * 9;  // column-major image, as pc_apply_kernel (Q7)
            const double x0 = s[3 * t], x1 = s[3 * t + 1], x2 = s[3 * t + 2], xp = s[768 + t];
            const double y0 = A[0] * x0 + A[3] * x1 + A[6] * x2, y1 = A[1] * x0 + A[4] * x1 + A[7] * x2;
            const double y2 = A[2] * x0 + A[5] * x1 + A[8] * x2, yp = xp * dinv1[i];
            double2* o = reinterpret_cast<double2*>(z4 + 4 * i);
            o[0] = make_double2(y0, y1);
            o[1] = make_double2(y2, yp);
        }
    }
}

// ---- two Arnoldi steps per pass over the raw basis (GmresPlan.pair) -----------------------------------------------------
// p1 = B v_k and p2 = B p1 (B = A M^-1) are orthogonalised against r_0..r_k together: one dots pass and one update pass
// over the basis serve both.  v_{k+1} comes from p1 as in the single step; p2 additionally loses its component along
// v_{k+1} (the one-column fix-up, cgs_update_jacobi_kernel), which leaves a multiple of v_{k+2}; column k+1 of H follows
// from the raw dots of p2 and the un-rotated earlier columns (pair_second_kernel).

// block-wide sums of two values with the barriers of one; same order as block_sum_256, results valid in thread 0
__device__ __forceinline__ void block_sum2_256(double& a, double& b, double* lds8) {
    a = wave_sum(a);
    b = wave_sum(b);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { lds8[w] = a; lds8[4 + w] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = (lds8[0] + lds8[1]) + (lds8[2] + lds8[3]);
        b = (lds8[4] + lds8[5]) + (lds8[6] + lds8[7]);
    }
    __syncthreads();
}

// as cgs_dots_stage1 with two vectors in registers: part[col * nrb + blk] of w1, part[(ncol + col) * nrb + blk] of w2
__global__ __launch_bounds__(BLK) void cgs_dots2_stage1(I n, I ncol, const T* __restrict__ Q, long long ldq,
                                                       const T* __restrict__ w1, const T* __restrict__ w2, T* __restrict__ part,
                                                       int nrb, int ct) {
    __shared__ double lds[8];
    const long long r0 = (long long)blockIdx.x * ROWS_PER_BLOCK;
    const int c0 = blockIdx.y * ct;
    double2 u[RPT], v[RPT];
    long long row[RPT];
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
        row[i] = r0 + 2LL * threadIdx.x + (long long)i * (2 * BLK);
        if (row[i] + 1 < n) {
            u[i] = *reinterpret_cast<const double2*>(w1 + row[i]);
            v[i] = *reinterpret_cast<const double2*>(w2 + row[i]);
        } else {
            u[i].x = (row[i] < n) ? w1[row[i]] : 0.0; u[i].y = 0.0;
            v[i].x = (row[i] < n) ? w2[row[i]] : 0.0; v[i].y = 0.0;
        }
    }
    for (int c = 0; c < ct; ++c) {
        const int col = c0 + c;
        if (col >= ncol) break;  // uniform
        const T* q = Q + (long long)col * ldq;
        double a1 = 0.0, a2 = 0.0;
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
            double2 qv;
            if (row[i] + 1 < n) qv = ld_stream(q + row[i]);
            else { qv.x = (row[i] < n) ? q[row[i]] : 0.0; qv.y = 0.0; }
            a1 += qv.x * u[i].x + qv.y * u[i].y;
            a2 += qv.x * v[i].x + qv.y * v[i].y;
        }
        block_sum2_256(a1, a2, lds);
        if (threadIdx.x == 0) {
            part[(long long)col * nrb + blockIdx.x] = a1;
            part[((long long)ncol + col) * nrb + blockIdx.x] = a2;
        }
    }
}

// grid (ncol, 2), the order of cgs_dots_raw_stage2.  y = 0: h1_j = <r_j, w1> / nu_j into column k of H and of its un-rotated
// copy, c1_j = h1_j / nu_j;  y = 1: e_j = <r_j, w2> / nu_j, c2_j = e_j / nu_j
__global__ __launch_bounds__(BLK) void cgs_dots2_stage2(int nrb, I ncol, const T* part, const T* __restrict__ nu, T* d_h1, T* d_h1_raw,
                                                       T* d_c1, T* d_e, T* d_c2) {
    __shared__ double lds[4];
    const int j = blockIdx.x;
    const T* p = part + ((long long)blockIdx.y * ncol + j) * nrb;
    double acc = 0.0;
    for (int i = threadIdx.x; i < nrb; i += BLK) acc += p[i];
    const double r = block_sum_256(acc, lds);
    if (threadIdx.x == 0) {
        const double v = nu[j], h = r / v;
        if (blockIdx.y == 0) {
            d_h1[j] = h;
            if (d_h1_raw) d_h1_raw[j] = h;
            d_c1[j] = h / v;
        } else {
            d_e[j] = h;
            d_c2[j] = h / v;
        }
    }
}

// w1 -= Q c1 and w2 -= Q c2, streamed as cgs_update_kernel<true> streams; partials of ||w1'||^2, <w1', w2'>, ||w2'||^2 at
// part[blk], part[gridDim.x + blk], part[2 gridDim.x + blk]
__global__ __launch_bounds__(BLK) void cgs_update2_kernel(I n, I ncol, const T* __restrict__ Q, long long ldq,
                                                         const T* __restrict__ d_c1, const T* __restrict__ d_c2, T* __restrict__ w1,
                                                         T* __restrict__ w2, T* __restrict__ part) {
    __shared__ double lds[8];
    __shared__ double sh1[128], sh2[128];
    for (int j = threadIdx.x; j < ncol && j < 128; j += BLK) { sh1[j] = d_c1[j]; sh2[j] = d_c2[j]; }
    __syncthreads();
    const long long blk = blockIdx.x;
    const long long r0 = blk * UROWS;
    long long row[UPT];
    double2 a[UPT], b[UPT];
#pragma unroll
    for (int i = 0; i < UPT; ++i) {
        row[i] = r0 + 2LL * threadIdx.x + (long long)i * (2 * BLK);
        if (row[i] + 1 < n) {
            a[i] = *reinterpret_cast<const double2*>(w1 + row[i]);
            b[i] = *reinterpret_cast<const double2*>(w2 + row[i]);
        } else {
            a[i].x = (row[i] < n) ? w1[row[i]] : 0.0; a[i].y = 0.0;
            b[i].x = (row[i] < n) ? w2[row[i]] : 0.0; b[i].y = 0.0;
        }
    }
#pragma unroll 4
    for (int j = 0; j < ncol; ++j) {
        const double h1 = (j < 128) ? sh1[j] : d_c1[j], h2 = (j < 128) ? sh2[j] : d_c2[j];
        const T* q = Q + (long long)j * ldq;
#pragma unroll
        for (int i = 0; i < UPT; ++i) {
            double2 qv;
            if (row[i] + 1 < n) qv = ld_stream(q + row[i]);
            else { qv.x = (row[i] < n) ? q[row[i]] : 0.0; qv.y = 0.0; }
            a[i].x -= qv.x * h1; a[i].y -= qv.y * h1;
            b[i].x -= qv.x * h2; b[i].y -= qv.y * h2;
        }
    }
    double s11 = 0.0, s12 = 0.0, s22 = 0.0;
#pragma unroll
    for (int i = 0; i < UPT; ++i) {
        if (row[i] + 1 < n) {
            *reinterpret_cast<double2*>(w1 + row[i]) = a[i];
            *reinterpret_cast<double2*>(w2 + row[i]) = b[i];
        } else if (row[i] < n) { w1[row[i]] = a[i].x; w2[row[i]] = b[i].x; }
        s11 += a[i].x * a[i].x + a[i].y * a[i].y;
        s12 += a[i].x * b[i].x + a[i].y * b[i].y;
        s22 += b[i].x * b[i].x + b[i].y * b[i].y;
    }
    block_sum2_256(s11, s12, lds);
    const double r22 = block_sum_256(s22, lds);
    if (threadIdx.x == 0) {
        part[blk] = s11;
        part[(long long)gridDim.x + blk] = s12;
        part[2LL * gridDim.x + blk] = r22;
    }
}

// The scalars of a pair after the two-vector update, one workgroup: second stage of s11, s12, s22 (fixed order), nu1 =
// sqrt(s11) = nrm[k+1], sc = [c = s12 / s11 (the fix-up coefficient), d = s12 / nu1 = <v_{k+1}, p2>, s22, nu1]; column k of H
// has h1 in rows 0..k already (cgs_dots2_stage2): nu1 goes below it, in H's un-rotated copy too, then the Givens step
__global__ __launch_bounds__(BLK) void pair_first_kernel(int npart, const T* part, I k, T* nu, T* H, T* Hraw, I ldh, T* gv, T* beta,
                                                        T* res_hist, T* sc) {
    __shared__ double lds[8];
    __shared__ double s_nrm;
    __shared__ double s_col[GIV_MAX], s_gv[2 * GIV_MAX];
    double a11 = 0.0, a12 = 0.0, a22 = 0.0;
    for (int i = threadIdx.x; i < npart; i += BLK) {
        a11 += part[i];
        a12 += part[npart + i];
        a22 += part[2 * npart + i];
    }
    block_sum2_256(a11, a12, lds);
    const double r22 = block_sum_256(a22, lds);
    if (threadIdx.x == 0) {
        const double nu1 = sqrt(a11);
        nu[k + 1] = nu1;
        sc[0] = a12 / a11;
        sc[1] = a12 / nu1;
        sc[2] = r22;
        sc[3] = nu1;
        Hraw[(long long)k * ldh + k + 1] = nu1;
        s_nrm = nu1;
    }
    __syncthreads();
    givens_step_block(k, s_nrm, H, ldh, gv, beta, res_hist, s_col, s_gv);
}

// The scalars of a pair after the fix-up, one workgroup: nu_q = ||q|| = nrm[k+2] from the fix-up's partials; *d_flag is raised
// when nu_q < 1e-4 sqrt(s22) (the relative error of q is about eps ||p2'|| / nu_q: 1e-12 at this threshold).  Column k+1
// of H from p2 = B p1 = sum_{j<=k} h1_j B v_j + nu1 B v_{k+1} and B v_j = sum_i Hraw[i,j] v_i:
//   rows i <= k: (e_i - sum_{j<k} h1_j Hraw[i,j] - h1_k h1_i) / nu1   (Hraw[i,j] = 0 for i > j + 1)
//   row k+1: (d - h1_k nu1) / nu1,   row k+2: nu_q / nu1
// into H and its un-rotated copy, then the Givens step of that column
__global__ __launch_bounds__(BLK) void pair_second_kernel(int npart, const T* part, I k, T* nu, T* H, T* Hraw, I ldh,
                                                         const T* __restrict__ d_e, const T* __restrict__ sc, T* gv, T* beta,
                                                         T* res_hist, int* d_flag) {
    __shared__ double lds[4];
    __shared__ double s_nrm;
    __shared__ double s_col[GIV_MAX], s_gv[2 * GIV_MAX];
    double acc = 0.0;
    for (int i = threadIdx.x; i < npart; i += BLK) acc += part[i];
    const double qq = block_sum_256(acc, lds);
    const double nu1 = sc[3];
    if (threadIdx.x == 0) {
        const double nuq = sqrt(qq);
        nu[k + 2] = nuq;
        if (d_flag && nuq < 1e-4 * sqrt(sc[2])) *d_flag = 1;
        s_nrm = nuq / nu1;
    }
    __syncthreads();
    const T* h1 = Hraw + (long long)k * ldh;
    T* col = H + (long long)(k + 1) * ldh;
    T* raw = Hraw + (long long)(k + 1) * ldh;
    const double h1k = h1[k];
    for (int i = threadIdx.x; i <= k; i += BLK) {
        double t = d_e[i];
        for (int j = (i > 0 ? i - 1 : 0); j < k; ++j) t -= h1[j] * Hraw[(long long)j * ldh + i];
        t -= h1k * h1[i];
        const double v = t / nu1;
        col[i] = v;
        raw[i] = v;
    }
    if (threadIdx.x == 0) {
        const double v = (sc[1] - h1k * nu1) / nu1;
        col[k + 1] = v;
        raw[k + 1] = v;
        raw[k + 2] = s_nrm;
    }
    __syncthreads();
    givens_step_block(k + 1, s_nrm, H, ldh, gv, beta, res_hist, s_col, s_gv);
}

// ---- up to four Arnoldi steps per pass over the raw basis (gmres_block, host/gmres.c) ----------------------------------
// The pair generalised to S = 3 or 4 products p_0 = B v_k, p_i = B p_{i-1}, held in S consecutive columns w + i ldw: one
// dots pass and one update pass over r_0..r_k serve all of them.  The updated p_i' = (I - V V^T) p_i span v_{k+1}..v_{k+S};
// they are orthogonalised among themselves through their Gram matrix G (block_first_kernel: q_i = sum_{l<=i} C[i,l] p_l', C
// unit lower triangular), the q_i are formed in one pass over the S columns (cgs_fixup_block_kernel), and the columns
// k+1..k+S-1 of H follow from the coordinates of the p_i in the orthonormal basis and the un-rotated earlier columns
// (block_second_kernel).  Scalars of a block, d_sc: [0,16) G, [16,32) C, [32,48) U[l,i] = C[l].G[:,i] = <q_l, p_i'> (l < i),
// each 4 x 4 row-major.
constexpr int SC_G = 0, SC_C = 16, SC_U = 32;
constexpr int CTB = 64;  // columns per workgroup of the block dots: one tile up to 64 columns, the S vectors are then read once
// double2 slots per thread of the dots (R) and of the update (U), from the compiler's resource report for gfx950 and bench runs at
// M = 119.  Dots, S = 4: R = 2 takes 74 VGPRs (6 waves per SIMD), R = 3 100 and R = 4 126 (4 waves); in
// one job that ran the variants side by side the step time was the same for R = 2, 3, 4 and 0.3 ms longer for R = 1.  Update,
// S = 4: U = 2 takes 122 VGPRs (4 waves, four columns in flight per wave), U = 1 78 (6 waves) and, likewise side by side, a
// step 0.9 ms longer; S = 3: 102 VGPRs at U = 2.
template <int S> struct BlockShape;
template <> struct BlockShape<3> { static constexpr int R = 2, U = 2; };
template <> struct BlockShape<4> { static constexpr int R = 2, U = 2; };

// block-wide sums of S values with the barriers of one; same order as block_sum_256, results valid in thread 0
template <int S>
__device__ __forceinline__ void block_sumN_256(double (&v)[S], double* lds) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < S; ++i) {
        v[i] = wave_sum(v[i]);
        if (lane == 0) lds[4 * i + w] = v[i];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < S; ++i) v[i] = (lds[4 * i] + lds[4 * i + 1]) + (lds[4 * i + 2] + lds[4 * i + 3]);
    }
    __syncthreads();
}

// Sums of four values over the wave with 7 shuffles instead of 24: the halves of the wave swap two values each (xor 32), the
// quarters one (xor 16), then four steps inside 16 lanes.  Returns, in every lane, the wave's sum of v[lane >> 4]; fixed order.
__device__ __forceinline__ double wave_sum4(const double (&v)[4], int lane) {
    const bool hi = lane & 32;
    double k0 = hi ? v[2] : v[0], k1 = hi ? v[3] : v[1];
    const double s0 = hi ? v[0] : v[2], s1 = hi ? v[1] : v[3];
    k0 += __shfl_xor(s0, 32, WAVE);
    k1 += __shfl_xor(s1, 32, WAVE);
    const bool q = lane & 16;
    double k = q ? k1 : k0;
    const double s = q ? k0 : k1;
    k += __shfl_xor(s, 16, WAVE);
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) k += __shfl_xor(k, off, WAVE);
    return k;
}

// as cgs_dots2_stage1 with S vectors in registers: part[(i ncol + col) nrb + rb] of vector i; a row block rb is 512 R rows.
// The column loop holds no barrier: every wave leaves its S sums of a column in LDS (wave_sum4) and goes on to the next column,
// so the loads of several columns are in flight; one barrier after the tile, then one thread per (column, vector) adds the four
// waves in the order of block_sum_256.  (With a block sum per column, as the pair has it, the S x 12 shuffles and the two
// barriers of every column cost more than its loads at S = 4: 0.337 ms per launch at M = 119 against 0.217 ms now.)
// A workgroup takes a tile of up to CTB = 64 columns (one thread per (column, vector) in the last step): with 8-column tiles the S
// vectors were read once per tile, 120 column-lengths per solve at M = 119 instead of 40, and those re-reads reached the HBM
// (0.262 ms per launch).
// One-dimensional grid, the column tile running fastest: beyond 64 columns the workgroups that read the same rows of the S
// vectors are dispatched together.
// GRAM: the workgroup of a row block's first column tile also leaves the partials of the Gram matrix of the S vectors themselves,
// <p_a, p_b> for a <= b in row-major order of the upper triangle, at gram[t nrb + rb] -- they are in its registers
template <int S, int R, bool GRAM>
__global__ __launch_bounds__(BLK) void cgs_dots_block_stage1(I n, I ncol, const T* __restrict__ Q, long long ldq,
                                                            const T* __restrict__ w, long long ldw, T* __restrict__ part, int nrb,
                                                            int ntile, T* __restrict__ gram) {
    __shared__ double lds[CTB * 4 * 4];  // [column of the tile][vector][wave]: 8 KB
    const int rb = blockIdx.x / ntile;
    const long long r0 = (long long)rb * (BLK * R * 2);
    const int c0 = (blockIdx.x - rb * ntile) * CTB;
    const int nc = (ncol - c0 < CTB) ? (ncol - c0) : CTB;  // columns of this tile
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double2 u[S][R];
    long long row[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
        row[i] = r0 + 2LL * threadIdx.x + (long long)i * (2 * BLK);
#pragma unroll
        for (int a = 0; a < S; ++a) {
            const T* wa = w + a * ldw;
            if (row[i] + 1 < n) u[a][i] = *reinterpret_cast<const double2*>(wa + row[i]);
            else { u[a][i].x = (row[i] < n) ? wa[row[i]] : 0.0; u[a][i].y = 0.0; }
        }
    }
    auto load = [&](int c, double2(&qv)[R]) {
        const T* q = Q + (long long)(c0 + c) * ldq;
#pragma unroll
        for (int i = 0; i < R; ++i) {
            if (row[i] + 1 < n) qv[i] = ld_stream(q + row[i]);
            else { qv[i].x = (row[i] < n) ? q[row[i]] : 0.0; qv[i].y = 0.0; }
        }
    };
    auto reduce = [&](int c, const double2(&qv)[R]) {
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < R; ++i)
#pragma unroll
            for (int a = 0; a < S; ++a) acc[a] += qv[i].x * u[a][i].x + qv[i].y * u[a][i].y;
        const double r = wave_sum4(acc, lane);
        if ((lane & 15) == 0) lds[(c * 4 + (lane >> 4)) * 4 + wv] = r;
    };
    int c = 0;
    for (; c + 1 < nc; c += 2) {  // two columns per trip: the loads of both are issued before the first is reduced
        double2 qa[R], qb[R];
        load(c, qa);
        load(c + 1, qb);
        reduce(c, qa);
        reduce(c + 1, qb);
    }
    if (c < nc) {
        double2 qa[R];
        load(c, qa);
        reduce(c, qa);
    }
    __syncthreads();
    const int tc = threadIdx.x >> 2, ta = threadIdx.x & 3;
    if (tc < nc && ta < S) {
        const double* l = lds + (tc * 4 + ta) * 4;
        part[((long long)ta * ncol + c0 + tc) * nrb + rb] = (l[0] + l[1]) + (l[2] + l[3]);
    }
    if (GRAM && c0 == 0) {  // uniform
        constexpr int NG = S * (S + 1) / 2;
        double g[NG];
#pragma unroll
        for (int t = 0; t < NG; ++t) g[t] = 0.0;
#pragma unroll
        for (int i = 0; i < R; ++i) {
            int t = 0;
#pragma unroll
            for (int a = 0; a < S; ++a)
#pragma unroll
                for (int b = a; b < S; ++b, ++t) g[t] += u[a][i].x * u[b][i].x + u[a][i].y * u[b][i].y;
        }
        __syncthreads();  // the column sums have been read out of lds
        block_sumN_256<NG>(g, lds);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int t = 0; t < NG; ++t) gram[(long long)t * nrb + rb] = g[t];
        }
    }
}

// grid (ncol, S), the order of cgs_dots_raw_stage2: e_i[j] = <r_j, p_i> / nu_j at d_e[i lde + j], c_i = e_i / nu at d_c[i lde + j];
// e_0 is also column k of H and of its un-rotated copy (d_h, d_h_raw)
__global__ __launch_bounds__(BLK) void cgs_dots_block_stage2(int nrb, I ncol, const T* part, const T* __restrict__ nu, T* d_h,
                                                            T* d_h_raw, T* d_e, T* d_c, I lde) {
    __shared__ double lds[4];
    const int j = blockIdx.x, i = blockIdx.y;
    const T* p = part + ((long long)i * ncol + j) * nrb;
    double acc = 0.0;
    for (int t = threadIdx.x; t < nrb; t += BLK) acc += p[t];
    const double r = block_sum_256(acc, lds);
    if (threadIdx.x == 0) {
        const double v = nu[j], h = r / v;
        d_e[(long long)i * lde + j] = h;
        d_c[(long long)i * lde + j] = h / v;
        if (i == 0) {
            d_h[j] = h;
            if (d_h_raw) d_h_raw[j] = h;
        }
    }
}

// p_i -= Q c_i for the S vectors in one pass, streamed as cgs_update2_kernel streams; partials of G_ab = <p_a', p_b'>, a <= b
// in row-major order of the upper triangle, at part[g gridDim.x + blk]
template <int S, int U>
__global__ __launch_bounds__(BLK) void cgs_update_block_kernel(I n, I ncol, const T* __restrict__ Q, long long ldq,
                                                              const T* __restrict__ d_c, I lde, T* __restrict__ w, long long ldw,
                                                              T* __restrict__ part) {
    constexpr int NG = S * (S + 1) / 2;
    __shared__ double lds[4 * NG];
    __shared__ double sh[S][128];
    for (int j = threadIdx.x; j < ncol && j < 128; j += BLK) {
#pragma unroll
        for (int a = 0; a < S; ++a) sh[a][j] = d_c[(long long)a * lde + j];
    }
    __syncthreads();
    const long long blk = blockIdx.x;
    const long long r0 = blk * (BLK * U * 2);
    long long row[U];
    double2 v[S][U];
#pragma unroll
    for (int i = 0; i < U; ++i) {
        row[i] = r0 + 2LL * threadIdx.x + (long long)i * (2 * BLK);
#pragma unroll
        for (int a = 0; a < S; ++a) {
            const T* wa = w + a * ldw;
            if (row[i] + 1 < n) v[a][i] = *reinterpret_cast<const double2*>(wa + row[i]);
            else { v[a][i].x = (row[i] < n) ? wa[row[i]] : 0.0; v[a][i].y = 0.0; }
        }
    }
#pragma unroll 4
    for (int j = 0; j < ncol; ++j) {
        double h[S];
#pragma unroll
        for (int a = 0; a < S; ++a) h[a] = (j < 128) ? sh[a][j] : d_c[(long long)a * lde + j];
        const T* q = Q + (long long)j * ldq;
#pragma unroll
        for (int i = 0; i < U; ++i) {
            double2 qv;
            if (row[i] + 1 < n) qv = ld_stream(q + row[i]);
            else { qv.x = (row[i] < n) ? q[row[i]] : 0.0; qv.y = 0.0; }
#pragma unroll
            for (int a = 0; a < S; ++a) { v[a][i].x -= qv.x * h[a]; v[a][i].y -= qv.y * h[a]; }
        }
    }
    double g[NG];
#pragma unroll
    for (int t = 0; t < NG; ++t) g[t] = 0.0;
#pragma unroll
    for (int i = 0; i < U; ++i) {
#pragma unroll
        for (int a = 0; a < S; ++a) {
            T* wa = w + a * ldw;
            if (row[i] + 1 < n) *reinterpret_cast<double2*>(wa + row[i]) = v[a][i];
            else if (row[i] < n) wa[row[i]] = v[a][i].x;
        }
        int t = 0;
#pragma unroll
        for (int a = 0; a < S; ++a)
#pragma unroll
            for (int b = a; b < S; ++b, ++t) g[t] += v[a][i].x * v[b][i].x + v[a][i].y * v[b][i].y;
    }
    block_sumN_256<NG>(g, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int t = 0; t < NG; ++t) part[(long long)t * gridDim.x + blk] = g[t];
    }
}

// the S x S Gram matrix, symmetric in a zeroed 4 x 4, from its upper triangle in row-major order
template <int S>
__device__ __forceinline__ void gram_unpack(const double (&g)[S * (S + 1) / 2], double (&G)[4][4]) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) G[a][b] = 0.0;
    int t = 0;
#pragma unroll
    for (int a = 0; a < S; ++a)
#pragma unroll
        for (int b = a; b < S; ++b, ++t) { G[a][b] = g[t]; G[b][a] = g[t]; }
}

// Gram-Schmidt on G, one thread: C unit lower triangular with q_i = sum_{l<=i} C[i,l] p_l' orthogonal as G has them, and
// U[l,i] = C[l].G[:,i], l < i.  Row i starts as the unit vector, then for l < i: C[i] -= (C[l].G[:,i] / C[l].G.C[l]) C[l]
template <int S>
__device__ __forceinline__ void gram_schmidt_on_G(const double (&G)[4][4], double (&Cm)[4][4], double (&Um)[4][4]) {
    double d[4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) { Cm[a][b] = (a == b) ? 1.0 : 0.0; Um[a][b] = 0.0; }
#pragma unroll
    for (int i = 0; i < S; ++i) {
#pragma unroll
        for (int l = 0; l < i; ++l) {
            double u = 0.0;
#pragma unroll
            for (int m = 0; m <= l; ++m) u += Cm[l][m] * G[m][i];
            Um[l][i] = u;
            const double f = u / d[l];
#pragma unroll
            for (int m = 0; m <= l; ++m) Cm[i][m] -= f * Cm[l][m];
        }
        double dd = 0.0;  // C[i].G.C[i] = ||q_i||^2 as G has it
#pragma unroll
        for (int a = 0; a <= i; ++a) {
            double r = 0.0;
#pragma unroll
            for (int b = 0; b <= i; ++b) r += G[a][b] * Cm[i][b];
            dd += Cm[i][a] * r;
        }
        d[i] = dd;
    }
}

// cgs_dots_block_stage2 with S (S + 1) / 2 more workgroups, which finish the raw Gram sums <p_a, p_b> (gram: their partials, t-th
// entry of the upper triangle at gram[t nrb]) in the same fixed order into graw[t]; one-dimensional grid, the first ncol S
// workgroups are those of cgs_dots_block_stage2, vector-major, and write what it writes bit for bit
__global__ __launch_bounds__(BLK) void cgs_dots_block_gram_stage2(int nrb, I ncol, int ns, const T* part, const T* __restrict__ nu,
                                                                 T* d_h, T* d_h_raw, T* d_e, T* d_c, I lde, const T* gram,
                                                                 T* graw) {
    __shared__ double lds[4];
    const int nd = ncol * ns;
    const bool dots = (int)blockIdx.x < nd;
    const int i = blockIdx.x / ncol, j = blockIdx.x - i * ncol;
    const T* p = dots ? part + ((long long)i * ncol + j) * nrb : gram + (long long)(blockIdx.x - nd) * nrb;
    double acc = 0.0;
    for (int t = threadIdx.x; t < nrb; t += BLK) acc += p[t];
    const double r = block_sum_256(acc, lds);
    if (threadIdx.x == 0) {
        if (dots) {
            const double v = nu[j], h = r / v;
            d_e[(long long)i * lde + j] = h;
            d_c[(long long)i * lde + j] = h / v;
            if (i == 0) {
                d_h[j] = h;
                if (d_h_raw) d_h_raw[j] = h;
            }
        } else graw[blockIdx.x - nd] = r;
    }
}

// After cgs_dots_block_gram_stage2, one workgroup: from the raw Gram sums (sc[SC_GR + t], t-th entry of the upper triangle) the
// Gram matrix the updated vectors WILL have -- r_j / nu_j are orthonormal, so <p_a', p_b'> = <p_a, p_b> - sum_{j<=k} e_a[j] e_b[j],
// j ascending -- and C by Gram-Schmidt on it, before the update pass runs.  sc[SC_C] = C, sc[SC_GD] = the derived G, sc[SC_GR] =
// the raw sums, each 4 x 4.  C only chooses the basis inside the block (block_fused_kernel).
constexpr int SC_GD = 48, SC_GR = 64;
template <int S>
__global__ __launch_bounds__(64) void block_gram_kernel(I ncol, const T* __restrict__ d_e, I lde, T* sc) {
    constexpr int NG = S * (S + 1) / 2;
    __shared__ double s_raw[NG], s_der[NG];
    if (threadIdx.x < NG) s_raw[threadIdx.x] = sc[SC_GR + threadIdx.x];
    __syncthreads();
    if (threadIdx.x < NG) {  // one thread per entry of the upper triangle
        int a = 0, b = threadIdx.x;
        while (b >= S - a) { b -= S - a; ++a; }
        b += a;
        const T* ea = d_e + (long long)a * lde;
        const T* eb = d_e + (long long)b * lde;
        double v = s_raw[threadIdx.x];
        for (int j = 0; j < ncol; ++j) v -= ea[j] * eb[j];
        s_der[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double gr[NG], gd[NG], Gr[4][4], G[4][4], Cm[4][4], Um[4][4];
#pragma unroll
        for (int t = 0; t < NG; ++t) { gr[t] = s_raw[t]; gd[t] = s_der[t]; }
        gram_unpack<S>(gr, Gr);
        gram_unpack<S>(gd, G);
        gram_schmidt_on_G<S>(G, Cm, Um);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                sc[SC_C + 4 * a + b] = Cm[a][b];
                sc[SC_GD + 4 * a + b] = G[a][b];
                sc[SC_GR + 4 * a + b] = Gr[a][b];
            }
    }
}

// The scalars of a block after the S-vector update, one workgroup: second stage of G (fixed order), nu[k+1] = sqrt(G_00) below
// e_0 in column k of H and of its un-rotated copy, the Givens step of that column; C by Gram-Schmidt on G: row i starts as the
// unit vector, then for l < i: C[i] -= (C[l].G[:,i] / C[l].G.C[l]) C[l]  (S = 2: C[1,0] = -s12 / s11, the pair's coefficient)
template <int S>
__global__ __launch_bounds__(BLK) void block_first_kernel(int npart, const T* part, I k, T* nu, T* H, T* Hraw, I ldh, T* gv, T* beta,
                                                         T* res_hist, T* sc) {
    constexpr int NG = S * (S + 1) / 2;
    __shared__ double lds[4 * NG];
    __shared__ double s_nrm;
    __shared__ double s_col[GIV_MAX], s_gv[2 * GIV_MAX];
    double g[NG];
#pragma unroll
    for (int t = 0; t < NG; ++t) g[t] = 0.0;
#pragma unroll 2
    for (int i = threadIdx.x; i < npart; i += BLK) {  // (the NG loads of a trip are independent: one latency per trip, not per load)
#pragma unroll
        for (int t = 0; t < NG; ++t) g[t] += part[(long long)t * npart + i];
    }
    block_sumN_256<NG>(g, lds);
    if (threadIdx.x == 0) {
        double G[4][4], Cm[4][4], Um[4][4];
        gram_unpack<S>(g, G);
        gram_schmidt_on_G<S>(G, Cm, Um);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                sc[SC_G + 4 * a + b] = G[a][b];
                sc[SC_C + 4 * a + b] = Cm[a][b];
                sc[SC_U + 4 * a + b] = Um[a][b];
            }
        const double nu1 = sqrt(G[0][0]);
        nu[k + 1] = nu1;
        Hraw[(long long)k * ldh + k + 1] = nu1;
        s_nrm = nu1;
    }
    __syncthreads();
    givens_step_block(k, s_nrm, H, ldh, gv, beta, res_hist, s_col, s_gv);
}

// q_i = sum_{l <= i} C[i,l] p_l' for i = 1..S-1, in place (p_0' = q_0 stays), one pass over the S columns: a workgroup owns 256
// nodes as in cgs_update_jacobi_kernel (same slots, same vec_ok rule); partials of ||q_i||^2 at part[(i-1) gridDim.x + blk];
// Z4: z4[node] = M^-1 q_{S-1}[node] from the registers through the LDS regroup of cgs_update_jacobi_kernel
template <int S, bool Z4>
__global__ __launch_bounds__(BLK) void cgs_fixup_block_kernel(I N, T* __restrict__ w, long long ldw, const T* __restrict__ sc,
                                                             T* __restrict__ part, const T* __restrict__ dinv33,
                                                             const T* __restrict__ dinv1, T* __restrict__ z4, int vec_ok) {
    __shared__ double lds[4 * (S - 1)];
    __shared__ double2 sm[Z4 ? BLK * UPT : 1];  // q_{S-1} of the block: [0, 768) u, [768, 1024) p
    double Cm[S][S];
#pragma unroll
    for (int a = 1; a < S; ++a)
#pragma unroll
        for (int l = 0; l < a; ++l) Cm[a][l] = sc[SC_C + 4 * a + l];
    const long long blk = blockIdx.x;
    const long long a0 = blk * BLK;
    const long long nb = (N - a0 < BLK) ? (N - a0) : BLK;  // nodes of this block
    double ss[S - 1];
#pragma unroll
    for (int a = 0; a < S - 1; ++a) ss[a] = 0.0;
#pragma unroll
    for (int i = 0; i < UPT; ++i) {
        const int slot = threadIdx.x + i * BLK;  // slots [0, 384): u rows, [384, 512): p rows
        long long row, lim;
        if (slot < 384) { row = 3 * a0 + 2LL * slot; lim = 3 * (a0 + nb); }
        else { row = 3LL * N + a0 + 2LL * (slot - 384); lim = 3LL * N + a0 + nb; }
        const bool vec = vec_ok && row + 1 < lim && !(row & 1);
        double2 p[S];
#pragma unroll
        for (int a = 0; a < S; ++a) {
            const T* wa = w + a * ldw;
            if (vec) p[a] = *reinterpret_cast<const double2*>(wa + row);
            else { p[a].x = (row < lim) ? wa[row] : 0.0; p[a].y = (row + 1 < lim) ? wa[row + 1] : 0.0; }
        }
#pragma unroll
        for (int a = S - 1; a >= 1; --a) {  // descending: q_a needs p_l', l < a, as they were
#pragma unroll
            for (int l = 0; l < a; ++l) { p[a].x += Cm[a][l] * p[l].x; p[a].y += Cm[a][l] * p[l].y; }
            T* wa = w + a * ldw;
            if (vec) *reinterpret_cast<double2*>(wa + row) = p[a];
            else {
                if (row < lim) wa[row] = p[a].x;
                if (row + 1 < lim) wa[row + 1] = p[a].y;
            }
            ss[a - 1] += p[a].x * p[a].x + p[a].y * p[a].y;
        }
        if (Z4) sm[slot] = p[S - 1];
    }
    block_sumN_256<S - 1>(ss, lds);  // (its barriers also publish sm)
    if (threadIdx.x == 0) {
#pragma unroll
        for (int a = 0; a < S - 1; ++a) part[(long long)a * gridDim.x + blk] = ss[a];
    }
    if (Z4) {
        const double* s = reinterpret_cast<const double*>(sm);
        const int t = threadIdx.x;
        if (t < nb) {
            const long long i = a0 + t;
            const T* A = dinv33 + i * 9;  // column-major image, as pc_apply_kernel (Q7)
            const double x0 = s[3 * t], x1 = s[3 * t + 1], x2 = s[3 * t + 2], xp = s[768 + t];
            const double y0 = A[0] * x0 + A[3] * x1 + A[6] * x2, y1 = A[1] * x0 + A[4] * x1 + A[7] * x2;
            const double y2 = A[2] * x0 + A[5] * x1 + A[8] * x2, yp = xp * dinv1[i];
            double2* o = reinterpret_cast<double2*>(z4 + 4 * i);
            o[0] = make_double2(y0, y1);
            o[1] = make_double2(y2, yp);
        }
    }
}

// cgs_update_block_kernel and cgs_fixup_block_kernel in one pass, C known beforehand (block_gram_kernel): a workgroup owns 256 nodes
// as the fix-up does (same slots, same vec_ok rule, which here covers Q as well), streams columns 0..ncol-1 as the update does
// (p_i -= c_i[j] r_j, j ascending, the same expressions), then from the registers: the partials of the measured G = [<p_a', p_b'>]
// at part[t gridDim.x + blk], q_a for a = S-1 down to 1 with the fix-up's expressions, the partials of ||q_i||^2 at
// part[(NG + i - 1) gridDim.x + blk]; every column is stored once (p_0' = q_0 included: nothing has stored it yet).  Given the same
// tables q_i and z4 are those of the two kernels bit for bit.  The columns leave with nontemporal stores, z4 with plain ones: the
// product that opens the next block gathers from z4 first, and the 4 c of columns stored after it no longer push it out of the
// Infinity Cache (M = 119, one trace job: this kernel 276 against 293 us, the product behind it 546 against 561 us).
template <int S, bool Z4>
__global__ __launch_bounds__(BLK) void cgs_update_fixup_block_kernel(I N, I ncol, const T* __restrict__ Q, long long ldq,
                                                                    const T* __restrict__ d_c, I lde, T* __restrict__ w,
                                                                    long long ldw, const T* __restrict__ sc, T* __restrict__ part,
                                                                    const T* __restrict__ dinv33, const T* __restrict__ dinv1,
                                                                    T* __restrict__ z4, int vec_ok) {
    constexpr int NG = S * (S + 1) / 2, NP = NG + S - 1;
    __shared__ double lds[4 * NP];
    __shared__ double sh[S][128];
    __shared__ double2 sm[Z4 ? BLK * UPT : 1];  // q_{S-1} of the block: [0, 768) u, [768, 1024) p
    for (int j = threadIdx.x; j < ncol && j < 128; j += BLK) {
#pragma unroll
        for (int a = 0; a < S; ++a) sh[a][j] = d_c[(long long)a * lde + j];
    }
    __syncthreads();
    double Cm[S][S];
#pragma unroll
    for (int a = 1; a < S; ++a)
#pragma unroll
        for (int l = 0; l < a; ++l) Cm[a][l] = sc[SC_C + 4 * a + l];
    const long long blk = blockIdx.x;
    const long long a0 = blk * BLK;
    const long long nb = (N - a0 < BLK) ? (N - a0) : BLK;  // nodes of this block
    long long row[UPT];
    int ok[UPT];  // bit 0: row is inside, bit 1: row + 1 is, bit 2: the slot is one aligned double2
    double2 v[S][UPT];
#pragma unroll
    for (int i = 0; i < UPT; ++i) {
        const int slot = threadIdx.x + i * BLK;  // slots [0, 384): u rows, [384, 512): p rows
        long long lim;
        if (slot < 384) { row[i] = 3 * a0 + 2LL * slot; lim = 3 * (a0 + nb); }
        else { row[i] = 3LL * N + a0 + 2LL * (slot - 384); lim = 3LL * N + a0 + nb; }
        ok[i] = (row[i] < lim ? 1 : 0) | (row[i] + 1 < lim ? 2 : 0) | ((vec_ok && row[i] + 1 < lim && !(row[i] & 1)) ? 4 : 0);
#pragma unroll
        for (int a = 0; a < S; ++a) {
            const T* wa = w + a * ldw;
            if (ok[i] & 4) v[a][i] = *reinterpret_cast<const double2*>(wa + row[i]);
            else { v[a][i].x = (ok[i] & 1) ? wa[row[i]] : 0.0; v[a][i].y = (ok[i] & 2) ? wa[row[i] + 1] : 0.0; }
        }
    }
#pragma unroll 4
    for (int j = 0; j < ncol; ++j) {
        double h[S];
#pragma unroll
        for (int a = 0; a < S; ++a) h[a] = (j < 128) ? sh[a][j] : d_c[(long long)a * lde + j];
        const T* q = Q + (long long)j * ldq;
#pragma unroll
        for (int i = 0; i < UPT; ++i) {
            double2 qv;
            if (ok[i] & 4) qv = ld_stream(q + row[i]);
            else { qv.x = (ok[i] & 1) ? q[row[i]] : 0.0; qv.y = (ok[i] & 2) ? q[row[i] + 1] : 0.0; }
#pragma unroll
            for (int a = 0; a < S; ++a) { v[a][i].x -= qv.x * h[a]; v[a][i].y -= qv.y * h[a]; }
        }
    }
    double g[NP];
#pragma unroll
    for (int t = 0; t < NP; ++t) g[t] = 0.0;
    auto store = [&](int a, int i, const double2& x) {
        T* wa = w + a * ldw;
        if (ok[i] & 4) {
            d2s y;
            y.x = x.x; y.y = x.y;
            __builtin_nontemporal_store(y, reinterpret_cast<d2s*>(wa + row[i]));
        } else {
            if (ok[i] & 1) wa[row[i]] = x.x;
            if (ok[i] & 2) wa[row[i] + 1] = x.y;
        }
    };
#pragma unroll
    for (int i = 0; i < UPT; ++i) {
        double2 p[S];
#pragma unroll
        for (int a = 0; a < S; ++a) p[a] = v[a][i];
        int t = 0;
#pragma unroll
        for (int a = 0; a < S; ++a)
#pragma unroll
            for (int b = a; b < S; ++b, ++t) g[t] += p[a].x * p[b].x + p[a].y * p[b].y;
#pragma unroll
        for (int a = S - 1; a >= 1; --a) {  // descending: q_a needs p_l', l < a, as they were
#pragma unroll
            for (int l = 0; l < a; ++l) { p[a].x += Cm[a][l] * p[l].x; p[a].y += Cm[a][l] * p[l].y; }
            store(a, i, p[a]);
            g[NG + a - 1] += p[a].x * p[a].x + p[a].y * p[a].y;
        }
        store(0, i, p[0]);
        if (Z4) sm[threadIdx.x + i * BLK] = p[S - 1];
    }
    block_sumN_256<NP>(g, lds);  // (its barriers also publish sm)
    if (threadIdx.x == 0) {
#pragma unroll
        for (int t = 0; t < NP; ++t) part[(long long)t * gridDim.x + blk] = g[t];
    }
    if (Z4) {
        const double* s = reinterpret_cast<const double*>(sm);
        const int t = threadIdx.x;
        if (t < nb) {
            const long long i = a0 + t;
            const T* A = dinv33 + i * 9;  // column-major image, as pc_apply_kernel (Q7)
            const double x0 = s[3 * t], x1 = s[3 * t + 1], x2 = s[3 * t + 2], xp = s[768 + t];
            const double y0 = A[0] * x0 + A[3] * x1 + A[6] * x2, y1 = A[1] * x0 + A[4] * x1 + A[7] * x2;
            const double y2 = A[2] * x0 + A[5] * x1 + A[8] * x2, yp = xp * dinv1[i];
            double2* o = reinterpret_cast<double2*>(z4 + 4 * i);
            o[0] = make_double2(y0, y1);
            o[1] = make_double2(y2, yp);
        }
    }
}

// The scalars of a block after the fix-up, one workgroup: nu[k+1+i] = ||q_i|| (i >= 1) from the fix-up's partials, measured and
// not derived from G; *d_flag is raised when one of them is below 1e-4 sqrt(G_ii).  rho_i, the coordinates of p_i in v_0..v_{k+1+i}:
// e_i in rows 0..k, U[l,i] / nu[k+1+l] in row k+1+l (l < i), nu[k+1+i] in row k+1+i.  p_i = B p_{i-1} and B v_j = Hraw[:,j] give
//   H[:, k+i] = (rho_i - sum_{j < k+i} Hraw[:,j] rho_{i-1}[j]) / nu[k+i],   j ascending, from max(row - 1, 0) (Hessenberg zeros)
// into H and its un-rotated copy, each column followed by its Givens step; S = 2 is pair_second_kernel term for term
// the columns k+1..k+S-1 of that formula with their Givens steps, by a whole workgroup; s_nu = nu[k..k+S], s_t[l][i] = U[l,i] / nu[k+1+l]
template <int S>
__device__ __forceinline__ void block_columns(I k, T* H, T* Hraw, I ldh, const T* __restrict__ d_e, I lde, const double* s_nu,
                                              const double (*s_t)[S], double* s_nrm, T* gv, T* beta, T* res_hist, double* s_col,
                                              double* s_gv) {
    for (int i = 1; i < S; ++i) {
        const I c = k + i;  // the column; rows 0..c+1
        T* col = H + (long long)c * ldh;
        T* raw = Hraw + (long long)c * ldh;
        const T* ei = d_e + (long long)i * lde;
        const T* ep = d_e + (long long)(i - 1) * lde;
        const double den = s_nu[i];  // rho_{i-1}[k+i] = nu[k+i]
        for (int r = threadIdx.x; r <= c + 1; r += BLK) {
            double t;
            if (r <= k) t = ei[r];
            else if (r - k - 1 < i) t = s_t[r - k - 1][i];
            else t = s_nu[1 + i];
            for (int j = (r > 0 ? r - 1 : 0); j < c; ++j) {
                const double rp = (j <= k) ? ep[j] : s_t[j - k - 1][i - 1];  // rho_{i-1}[j], j < k+i
                t -= rp * Hraw[(long long)j * ldh + r];
            }
            const double v = t / den;
            raw[r] = v;
            if (r <= c) col[r] = v;
            else *s_nrm = v;
        }
        __syncthreads();
        givens_step_block(c, *s_nrm, H, ldh, gv, beta, res_hist, s_col, s_gv);
        __syncthreads();
    }
}

template <int S>
__global__ __launch_bounds__(BLK) void block_second_kernel(int npart, const T* part, I k, T* nu, T* H, T* Hraw, I ldh,
                                                          const T* __restrict__ d_e, I lde, const T* __restrict__ sc, T* gv, T* beta,
                                                          T* res_hist, int* d_flag) {
    __shared__ double lds[4 * (S - 1)];
    __shared__ double s_nu[S + 1];   // nu[k .. k+S]
    __shared__ double s_t[S][S];     // s_t[l][i] = U[l,i] / nu[k+1+l]
    __shared__ double s_nrm;
    __shared__ double s_col[GIV_MAX], s_gv[2 * GIV_MAX];
    double qq[S - 1];
#pragma unroll
    for (int a = 0; a < S - 1; ++a) qq[a] = 0.0;
#pragma unroll 4
    for (int i = threadIdx.x; i < npart; i += BLK) {
#pragma unroll
        for (int a = 0; a < S - 1; ++a) qq[a] += part[(long long)a * npart + i];
    }
    block_sumN_256<S - 1>(qq, lds);
    if (threadIdx.x == 0) {
        s_nu[0] = nu[k];
        s_nu[1] = nu[k + 1];
        bool low = false;
#pragma unroll
        for (int i = 1; i < S; ++i) {
            const double v = sqrt(qq[i - 1]);
            nu[k + 1 + i] = v;
            s_nu[1 + i] = v;
            low = low || v < 1e-4 * sqrt(sc[SC_G + 5 * i]);
        }
        if (d_flag && low) *d_flag = 1;
        for (int l = 0; l < S; ++l)
            for (int i = 0; i < S; ++i) s_t[l][i] = (l < i) ? sc[SC_U + 4 * l + i] / s_nu[1 + l] : 0.0;
    }
    __syncthreads();
    block_columns<S>(k, H, Hraw, ldh, d_e, lde, s_nu, s_t, &s_nrm, gv, beta, res_hist, s_col, s_gv);
}

// The scalars of a fused block (cgs_update_fixup_block_kernel), one workgroup, in the place of block_first_kernel and
// block_second_kernel: C came from the derived Gram matrix before the pass (block_gram_kernel, sc[SC_C]); here everything that
// enters H is measured on the vectors the pass formed.  part: S (S + 1) / 2 sets of npart partials of G = [<p_a', p_b'>], then
// S - 1 sets of ||q_i||^2.  nu[k+1] = sqrt(G_00) and the Givens step of column k as block_first_kernel; U[l,i] = C[l].G[:,i], the
// measured nu[k+1+i], the cancellation flag d_flag[0] and the columns k+1..k+S-1 by the code of block_second_kernel.  d_flag[1] is
// raised when the q_a the pass formed are not orthogonal: |C[a].G.C[b]| > tau ||q_a|| ||q_b|| for some a < b.
// One thing differs from block_second_kernel: the coordinate of p_i' along v_{k+1+l} is D[i,l] nu[k+1+l], D = C^-1, not
// U[l,i] / nu[k+1+l].  The two agree when the q_i are orthogonal; with C from the derived G they are orthogonal only as far as
// r_0..r_k are, the projection U / nu is then no coordinate, while p' = C^-1 q holds for the vectors formed whatever C is: the
// relation B V = V H stays exact and a less accurate C costs orthogonality only.  (Dense "spread" operator of the numpy model,
// s = 4: history 1.1e-12 r0 from plain Arnoldi with U / nu, 7.8e-14 with C^-1.)  U is still formed and left in sc.
template <int S>
__global__ __launch_bounds__(BLK) void block_fused_kernel(int npart, const T* __restrict__ part, I k, T* nu, T* H, T* Hraw, I ldh,
                                                         const T* __restrict__ d_e, I lde, T* sc, T* gv, T* beta, T* res_hist,
                                                         int* d_flag, double tau) {
    constexpr int NG = S * (S + 1) / 2, NP = NG + S - 1;
    __shared__ double lds[4 * NP];
    __shared__ double s_nu[S + 1];
    __shared__ double s_t[S][S];
    __shared__ double s_nrm;
    __shared__ double s_col[GIV_MAX], s_gv[2 * GIV_MAX];
    double g[NP];
#pragma unroll
    for (int t = 0; t < NP; ++t) g[t] = 0.0;
#pragma unroll 2
    for (int i = threadIdx.x; i < npart; i += BLK) {  // (independent loads: one latency per trip)
#pragma unroll
        for (int t = 0; t < NP; ++t) g[t] += part[(long long)t * npart + i];
    }
    block_sumN_256<NP>(g, lds);
    if (threadIdx.x == 0) {
        double gm[NG], G[4][4], Cm[4][4], Um[4][4];
#pragma unroll
        for (int t = 0; t < NG; ++t) gm[t] = g[t];
        gram_unpack<S>(gm, G);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) { Cm[a][b] = sc[SC_C + 4 * a + b]; Um[a][b] = 0.0; }
#pragma unroll
        for (int i = 0; i < S; ++i)
#pragma unroll
            for (int l = 0; l < i; ++l) {
                double u = 0.0;
#pragma unroll
                for (int m = 0; m <= l; ++m) u += Cm[l][m] * G[m][i];
                Um[l][i] = u;
            }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                sc[SC_G + 4 * a + b] = G[a][b];
                sc[SC_U + 4 * a + b] = Um[a][b];
            }
        const double nu1 = sqrt(G[0][0]);
        nu[k + 1] = nu1;
        Hraw[(long long)k * ldh + k + 1] = nu1;
        s_nrm = nu1;
        s_nu[0] = nu[k];
        s_nu[1] = nu1;
        bool low = false;
#pragma unroll
        for (int i = 1; i < S; ++i) {
            const double v = sqrt(g[NG + i - 1]);
            nu[k + 1 + i] = v;
            s_nu[1 + i] = v;
            low = low || v < 1e-4 * sqrt(G[i][i]);
        }
        bool skew = false;  // <q_a, q_b> = C[a].G.C[b] as achieved, a < b
#pragma unroll
        for (int b = 1; b < S; ++b) {
            double Gc[4];
#pragma unroll
            for (int m = 0; m < S; ++m) {
                double r = 0.0;
#pragma unroll
                for (int l = 0; l <= b; ++l) r += G[m][l] * Cm[b][l];
                Gc[m] = r;
            }
#pragma unroll
            for (int a = 0; a < b; ++a) {
                double qq = 0.0;
#pragma unroll
                for (int m = 0; m <= a; ++m) qq += Cm[a][m] * Gc[m];
                skew = skew || !(fabs(qq) <= tau * s_nu[1 + a] * s_nu[1 + b]);
            }
        }
        if (d_flag && low) d_flag[0] = 1;
        if (d_flag && skew) d_flag[1] = 1;
        // coordinates of p_i' in q_0..q_i from the identity p' = D q, D = C^-1 (forward substitution, m ascending): D[i][l] nu[k+1+l]
        double D[4][4];
#pragma unroll
        for (int i = 0; i < S; ++i)
#pragma unroll
            for (int l = 0; l < i; ++l) {
                double v = 0.0;
#pragma unroll
                for (int m = l; m < i; ++m) v -= Cm[i][m] * (m == l ? 1.0 : D[m][l]);
                D[i][l] = v;
            }
#pragma unroll
        for (int l = 0; l < S; ++l)
#pragma unroll
            for (int i = 0; i < S; ++i) s_t[l][i] = (l < i) ? D[i][l] * s_nu[1 + l] : 0.0;
    }
    __syncthreads();
    givens_step_block(k, s_nrm, H, ldh, gv, beta, res_hist, s_col, s_gv);
    __syncthreads();
    block_columns<S>(k, H, Hraw, ldh, d_e, lde, s_nu, s_t, &s_nrm, gv, beta, res_hist, s_col, s_gv);
}

// H[0:m,0:m] y = beta by back substitution (cublasDtrsv, krylov.c:297-301), one workgroup: column-oriented so that every
// step is one coalesced column update (a single thread walking rows pays a dependent global load per entry: 85 us at m = 40)
template <bool STAGED>
__global__ __launch_bounds__(BLK) void gmres_trsv_kernel(I m, const T* __restrict__ H, I ldh, T* __restrict__ beta) {
    extern __shared__ double s_mem[];  // [m] right-hand side, then (STAGED) the m x m upper triangle, column-major
    __shared__ double s_y;
    double* s_b = s_mem;
    double* s_H = s_mem + m;
    const int t = threadIdx.x;
    for (int i = t; i < m; i += BLK) s_b[i] = beta[i];
    if (STAGED)
        for (int k = t; k < m * m; k += BLK) {
            const int c = k / m, r = k - c * m;
            s_H[k] = H[(long long)c * ldh + r];
        }
    __syncthreads();
    for (I i = m - 1; i >= 0; --i) {
        const T* col = STAGED ? s_H + (long long)i * m : H + (long long)i * ldh;  // H(r, i), r <= i: contiguous
        if (t == 0) {
            s_y = s_b[i] / col[i];
            s_b[i] = s_y;
        }
        __syncthreads();
        const double y = s_y;
        for (int r = t; r < i; r += BLK) s_b[r] -= col[r] * y;
        __syncthreads();
    }
    for (int i = t; i < m; i += BLK) beta[i] = s_b[i];
}

__global__ void sqrt_kernel(T* v) { v[0] = sqrt(v[0]); }

// one wave that stays resident for about `us` microseconds of the constant 100 MHz clock (bounded by an iteration count as
// well, so that it ends whatever the clock does): lets a host routine find out whether two streams run CONCURRENTLY
__global__ void spin_kernel(int us, int* sink) {
    const unsigned long long t0 = wall_clock64();
    const unsigned long long ticks = (unsigned long long)us * 100ull;
    int it = 0;
    while (wall_clock64() - t0 < ticks && it < (1 << 22)) {
        __builtin_amdgcn_s_sleep(32);
        ++it;
    }
    if (sink && it < 0) *sink = it;
}

__global__ void residual_update_kernel(T* beta, T* gv) {
    double b0 = beta[0];
    beta[1] = -gv[1] * b0;
    beta[0] = b0 * gv[0];
}

// halo pack / unpack: out[i] = x[idx[i]] and x[idx[i]] = in[i]
__global__ __launch_bounds__(256) void gather_idx_kernel(I n, const I* __restrict__ idx, const T* __restrict__ x,
                                                        T* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = x[idx[i]];
}
__global__ __launch_bounds__(256) void scatter_idx_kernel(I n, const I* __restrict__ idx, const T* __restrict__ in,
                                                         T* __restrict__ x) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) x[idx[i]] = in[i];
}


// ---- generalized-alpha state algebra of the Newton driver, fused (src/main.c:107-118, 242-253, 535-565) -----------------
// One thread per node.  The reference runs this as memset + 6 cublasDaxpy/Dcopy passes over 6N-vectors; the arithmetic
// per entry is kept (zero + a*x as a product, every axpy as one fused multiply-add, in the reference's order):
//   dwgalpha = f1_0 * dwgold + f1_1 * dwg           (pressure slot: dwgalpha = dwg, not alpha-interpolated)
//   wgalpha  = wgold + f2_0 * dwgold + f2_1 * dwg   (pressure slot: 0)
// nodep != NULL: the packed gather record of the node (pack_nodes_kernel layout) is written in the same pass.
__global__ __launch_bounds__(BLK) void alpha_states_kernel(I N, const T* __restrict__ wgold, const T* __restrict__ dwgold,
                                                          const T* __restrict__ dwg, T f1_0, T f1_1, T f2_0, T f2_1,
                                                          const T* __restrict__ xg, T* __restrict__ wga, T* __restrict__ dwga,
                                                          T* __restrict__ nodep, T* __restrict__ nodexu) {
    const long long i = (long long)blockIdx.x * BLK + threadIdx.x;
    if (i >= N) return;
    const long long idx[6] = {3 * i, 3 * i + 1, 3 * i + 2, 3LL * N + i, 4LL * N + i, 5LL * N + i};
    double w[6], d[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double o = wgold[idx[k]], d0 = dwgold[idx[k]], d1 = dwg[idx[k]];
        if (k == 3) { d[k] = d1; w[k] = 0.0; }
        else {
            d[k] = fma(f1_1, d1, f1_0 * d0);
            w[k] = fma(f2_1, d1, fma(f2_0, d0, o));
        }
        wga[idx[k]] = w[k];
        dwga[idx[k]] = d[k];
    }
    if (nodep) {  // x[3] u[3] phi T du[3] p(rate vector, Q9) dphi dT pad pad
        double2* o = reinterpret_cast<double2*>(nodep + i * 16);
        const double x0 = xg[3 * i], x1 = xg[3 * i + 1], x2 = xg[3 * i + 2];
        o[0] = make_double2(x0, x1);
        o[1] = make_double2(x2, w[0]);
        o[2] = make_double2(w[1], w[2]);
        o[3] = make_double2(w[4], w[5]);
        o[4] = make_double2(d[0], d[1]);
        o[5] = make_double2(d[2], d[3]);
        o[6] = make_double2(d[4], d[5]);
        o[7] = make_double2(0.0, 0.0);
        if (nodexu) {  // the compact (x, u) records of the Jacobian kernel
            double2* c = reinterpret_cast<double2*>(nodexu + i * 8);
            c[0] = make_double2(x0, x1);
            c[1] = make_double2(x2, w[0]);
            c[2] = make_double2(w[1], w[2]);
            c[3] = make_double2(0.0, 0.0);
        }
    }
}

// predictor (main.c:544-546): dwg *= fac on the velocity and phi / T slots (the pressure slot is left alone)
__global__ __launch_bounds__(BLK) void alpha_predict_kernel(I N, T fac, T* __restrict__ dwg) {
    const long long i = (long long)blockIdx.x * BLK + threadIdx.x;
    if (i >= 6LL * N) return;
    if (i >= 3LL * N && i < 4LL * N) return;
    dwg[i] *= fac;
}
// corrector (main.c:556-565): wgold += c0 * dwgold + c1 * dwg (not the pressure slot), then dwgold = dwg (all slots)
__global__ __launch_bounds__(BLK) void alpha_correct_kernel(I N, T c0, T c1, T* __restrict__ wgold, T* __restrict__ dwgold,
                                                           const T* __restrict__ dwg) {
    const long long i = (long long)blockIdx.x * BLK + threadIdx.x;
    if (i >= 6LL * N) return;
    const double d1 = dwg[i];
    if (!(i >= 3LL * N && i < 4LL * N)) wgold[i] = fma(c1, d1, fma(c0, dwgold[i], wgold[i]));
    dwgold[i] = d1;
}

// four segment sums of squares in one pass (Newton norms of u, p, phi, T; main.c:125-130): grid (blocks, 4)
__global__ __launch_bounds__(BLK) void norms4_stage1(I N, const T* __restrict__ F, T* __restrict__ part, int nblk) {
    __shared__ double lds[4];
    const int seg = blockIdx.y;
    const long long begin = seg == 0 ? 0 : (2LL + seg) * N, len = seg == 0 ? 3LL * N : N;
    double acc = 0.0;
    for (long long k = (long long)blockIdx.x * BLK + threadIdx.x; k < len; k += (long long)nblk * BLK) {
        const double v = F[begin + k];
        acc += v * v;
    }
    const double r = block_sum_256(acc, lds);
    if (threadIdx.x == 0) part[seg * nblk + blockIdx.x] = r;
}
template <bool SQRT>
__global__ __launch_bounds__(BLK) void norms4_stage2(int nblk, const T* __restrict__ part, T* __restrict__ out) {
    __shared__ double lds[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < nblk; i += BLK) acc += part[blockIdx.x * nblk + i];
    const double r = block_sum_256(acc, lds);
    if (threadIdx.x == 0) out[blockIdx.x] = SQRT ? sqrt(r) : r;
}

// host launchers of the block kernels (templates: outside extern "C")
template <int NS>
void launch_dots_block(I n, I ncol, const T* Q, int64_t ldq, const T* w, int64_t ldw, const T* d_nu, T* d_h, T* d_h_raw,
                              T* d_e, T* d_c, I lde, T* work, void* stream) {
    const int nrb = ceil_div(n, BLK * BlockShape<NS>::R * 2);
    const int ntile = ceil_div(ncol, CTB);
    if ((long long)nrb * ntile > 0x7fffffffLL) abort();
    cgs_dots_block_stage1<NS, BlockShape<NS>::R, false><<<nrb * ntile, BLK, 0, S(stream)>>>(n, ncol, Q, ldq, w, ldw, work, nrb, ntile,
                                                                                            nullptr);
    cgs_dots_block_stage2<<<dim3(ncol, NS), BLK, 0, S(stream)>>>(nrb, ncol, work, d_nu, d_h, d_h_raw, d_e, d_c, lde);
}
// ... with the Gram partials of the S vectors behind the dots partials in work, and C from the derived Gram matrix into d_sc
template <int NS>
void launch_dots_block_gram(I n, I ncol, const T* Q, int64_t ldq, const T* w, int64_t ldw, const T* d_nu, T* d_h, T* d_h_raw,
                            T* d_e, T* d_c, I lde, T* d_sc, T* work, void* stream) {
    const int nrb = ceil_div(n, BLK * BlockShape<NS>::R * 2);
    const int ntile = ceil_div(ncol, CTB);
    if ((long long)nrb * ntile > 0x7fffffffLL) abort();
    T* const gram = work + (size_t)NS * (size_t)ncol * (size_t)nrb;
    cgs_dots_block_stage1<NS, BlockShape<NS>::R, true><<<nrb * ntile, BLK, 0, S(stream)>>>(n, ncol, Q, ldq, w, ldw, work, nrb, ntile,
                                                                                           gram);
    cgs_dots_block_gram_stage2<<<ncol * NS + NS * (NS + 1) / 2, BLK, 0, S(stream)>>>(nrb, ncol, NS, work, d_nu, d_h, d_h_raw, d_e, d_c, lde,
                                                                                   gram, d_sc + SC_GR);
    block_gram_kernel<NS><<<1, 64, 0, S(stream)>>>(ncol, d_e, lde, d_sc);
}
template <int NS>
void launch_update_fixup_block(I N, I ncol, const T* Q, int64_t ldq, const T* d_c, I lde, T* w, int64_t ldw, const T* d_sc,
                               const T* dinv33, const T* dinv1, T* z4, T* work, void* stream) {
    const int g = ceil_div(N, BLK);
    const int vec_ok = aligned16(Q) && aligned16(w) && !(ldq & 1) && !(ldw & 1);
    if (z4) cgs_update_fixup_block_kernel<NS, true><<<g, BLK, 0, S(stream)>>>(N, ncol, Q, ldq, d_c, lde, w, ldw, d_sc, work, dinv33, dinv1,
                                                                              z4, vec_ok);
    else cgs_update_fixup_block_kernel<NS, false><<<g, BLK, 0, S(stream)>>>(N, ncol, Q, ldq, d_c, lde, w, ldw, d_sc, work, nullptr, nullptr,
                                                                            nullptr, vec_ok);
}
template <int NS>
void launch_fixup_block(I N, T* w, int64_t ldw, const T* d_sc, const T* dinv33, const T* dinv1, T* z4, T* work, void* stream) {
    const int g = ceil_div(N, BLK);
    const int vec_ok = aligned16(w) && !(ldw & 1);
    if (z4) cgs_fixup_block_kernel<NS, true><<<g, BLK, 0, S(stream)>>>(N, w, ldw, d_sc, work, dinv33, dinv1, z4, vec_ok);
    else cgs_fixup_block_kernel<NS, false><<<g, BLK, 0, S(stream)>>>(N, w, ldw, d_sc, work, nullptr, nullptr, nullptr, vec_ok);
}

}  // namespace

extern "C" {
void dfl_gather_idx(I n, const I* idx, const T* x, T* out, void* stream) {
    if (n <= 0) return;
    gather_idx_kernel<<<ceil_div(n, 256), 256, 0, S(stream)>>>(n, idx, x, out);
    DFL_LAUNCH_CHECK();
}
void dfl_scatter_idx(I n, const I* idx, const T* in, T* x, void* stream) {
    if (n <= 0) return;
    scatter_idx_kernel<<<ceil_div(n, 256), 256, 0, S(stream)>>>(n, idx, in, x);
    DFL_LAUNCH_CHECK();
}



void dfl_alpha_states2(I N, const T* wgold, const T* dwgold, const T* dwg, T f1_0, T f1_1, T f2_0, T f2_1, const T* xg, T* wgalpha,
                       T* dwgalpha, T* nodep, T* nodexu, void* stream) {
    if (N <= 0) return;
    alpha_states_kernel<<<ceil_div(N, BLK), BLK, 0, S(stream)>>>(N, wgold, dwgold, dwg, f1_0, f1_1, f2_0, f2_1, xg, wgalpha, dwgalpha, nodep,
                                                                 nodexu);
    DFL_LAUNCH_CHECK();
}
void dfl_alpha_states(I N, const T* wgold, const T* dwgold, const T* dwg, T f1_0, T f1_1, T f2_0, T f2_1, const T* xg, T* wgalpha,
                      T* dwgalpha, T* nodep, void* stream) {
    dfl_alpha_states2(N, wgold, dwgold, dwg, f1_0, f1_1, f2_0, f2_1, xg, wgalpha, dwgalpha, nodep, nullptr, stream);
}
void dfl_alpha_predict(I N, T fac, T* dwg, void* stream) {
    if (N <= 0) return;
    alpha_predict_kernel<<<ceil_div(6LL * N, BLK), BLK, 0, S(stream)>>>(N, fac, dwg);
    DFL_LAUNCH_CHECK();
}
void dfl_alpha_correct(I N, T c0, T c1, T* wgold, T* dwgold, const T* dwg, void* stream) {
    if (N <= 0) return;
    alpha_correct_kernel<<<ceil_div(6LL * N, BLK), BLK, 0, S(stream)>>>(N, c0, c1, wgold, dwgold, dwg);
    DFL_LAUNCH_CHECK();
}
void dfl_norms4(I N, const T* F, T* d_out4, int take_sqrt, T* work, void* stream) {
    if (N <= 0) return;
    int nblk = ceil_div(3LL * N, BLK * 8);
    if (nblk < 1) nblk = 1;
    if (nblk > MAX_PART / 4) nblk = MAX_PART / 4;
    norms4_stage1<<<dim3(nblk, 4), BLK, 0, S(stream)>>>(N, F, work, nblk);
    if (take_sqrt) norms4_stage2<true><<<4, BLK, 0, S(stream)>>>(nblk, work, d_out4);
    else norms4_stage2<false><<<4, BLK, 0, S(stream)>>>(nblk, work, d_out4);
    DFL_LAUNCH_CHECK();
}

int dfl_abi_version(void) { return 1; }
const char* dfl_last_error(void) { return g_err; }

void dfl_daxpy(I n, T alpha, const T* x, T* y, void* stream) {
    launch_map3(n, x, y, y, [alpha] __device__(double a, double b) { return alpha * a + b; }, stream);
}
void dfl_dscal(I n, T alpha, T* x, void* stream) {
    launch_map1(n, x, [alpha] __device__(double a) { return alpha * a; }, stream);
}
void dfl_dcopy(I n, const T* x, T* y, void* stream) {
    if (n > 0) DFL_GUARD(hipMemcpyAsync(y, x, (size_t)n * sizeof(T), hipMemcpyDeviceToDevice, S(stream)));
}
void dfl_dset(I n, T alpha, T* x, void* stream) {
    launch_map1(n, x, [alpha] __device__(double) { return alpha; }, stream);
}
void SetValGPU(T* val, I n, T alpha) { dfl_dset(n, alpha, val, nullptr); }
void dfl_pointwise_mult(I n, const T* x, const T* y, T* z, void* stream) {
    launch_map3(n, x, y, z, [] __device__(double a, double b) { return a * b; }, stream);
}
void dfl_pointwise_div(I n, const T* x, const T* y, T* z, void* stream) {
    launch_map3(n, x, y, z, [] __device__(double a, double b) { return a / b; }, stream);
}
void dfl_pointwise_inv(I n, T* x, void* stream) {
    launch_map1(n, x, [] __device__(double a) { return 1.0 / a; }, stream);
}

I dfl_reduce_work_size(void) { return MAX_PART; }

static int reduce_grid(I n) {
    int g = ceil_div(n, BLK * 8);
    if (g < 1) g = 1;
    if (g > MAX_PART) g = MAX_PART;
    return g;
}
void dfl_ddot(I n, const T* x, const T* y, T* d_out, T* work, void* stream) {
    int g = reduce_grid(n);
    reduce_stage1<true><<<g, BLK, 0, S(stream)>>>(n, x, y, work);
    reduce_stage2<false><<<1, BLK, 0, S(stream)>>>(g, work, d_out);
    DFL_LAUNCH_CHECK();
}
void dfl_dnrm2(I n, const T* x, T* d_out, T* work, void* stream) {
    int g = reduce_grid(n);
    reduce_stage1<false><<<g, BLK, 0, S(stream)>>>(n, x, x, work);
    reduce_stage2<true><<<1, BLK, 0, S(stream)>>>(g, work, d_out);
    DFL_LAUNCH_CHECK();
}
void dfl_dscal_inv_dev(I n, const T* d_scale, T* x, void* stream) {
    if (n <= 0) return;
    scal_inv_dev<<<ceil_div((n >> 1) + 1, BLK), BLK, 0, S(stream)>>>(n, d_scale, x);
    DFL_LAUNCH_CHECK();
}

int64_t dfl_cgs_work_size(I n, I ncol) {
    int64_t nrb = ceil_div(n, ROWS_PER_BLOCK);
    int64_t a = 2 * nrb * (int64_t)(ncol > 0 ? ncol : 1);  // two vectors per dots pass (dfl_cgs_dots2_raw)
    int64_t b = 3 * (int64_t)ceil_div(n, UROWS);           // s11, s12, s22 of dfl_cgs_update2
    for (int s = 3; s <= 4; ++s) {                         // blocks of s products: s sets of dots partials, s (s + 1) / 2 of G
        const int64_t ng = s * (s + 1) / 2;
        // (fused blocks: the Gram partials of the raw vectors behind the dots partials; G and the s - 1 norms of the one pass)
        const int64_t as = ((int64_t)s * (int64_t)(ncol > 0 ? ncol : 1) + ng) * dfl_cgs_dots_block_parts(n, s);
        int64_t bs = ng * dfl_cgs_update_block_parts(n, s);
        const int64_t fs = (ng + s - 1) * (int64_t)dfl_cgs_update_fixup_block_parts((I)ceil_div(n, 4));
        if (fs > bs) bs = fs;
        if (as > a) a = as;
        if (bs > b) b = bs;
    }
    return (a > b ? a : b) + 16;
}
void dfl_cgs_dots(I n, I ncol, const T* Q, int64_t ldq, const T* w, T* d_h, T* work, void* stream) {
    if (ncol <= 0) return;
    int nrb = ceil_div(n, ROWS_PER_BLOCK);
    // column tile of a workgroup: CT columns share one read of w per row block (tiles of 64, which read w once per 41-column
    // step, measured 0.2013-0.2017 against 0.2021-0.2026 ms per CGS kernel: the re-reads of w come out of the caches)
    dim3 grid(nrb, ceil_div(ncol, CT));
    cgs_dots_stage1<<<grid, BLK, 0, S(stream)>>>(n, ncol, Q, ldq, w, work, nrb, CT);
    cgs_dots_stage2<<<ncol, BLK, 0, S(stream)>>>(nrb, work, d_h);
    DFL_LAUNCH_CHECK();
}
void dfl_cgs_update(I n, I ncol, const T* Q, int64_t ldq, const T* d_h, T* w, T* d_nrm, int take_sqrt, T* work, void* stream) {
    int g = ceil_div(n, UROWS);
    cgs_update_kernel<true><<<g, BLK, 0, S(stream)>>>(n, ncol, Q, ldq, d_h, w, d_nrm ? work : nullptr);
    if (d_nrm) {
        if (take_sqrt) reduce_stage2<true><<<1, BLK, 0, S(stream)>>>(g, work, d_nrm);
        else reduce_stage2<false><<<1, BLK, 0, S(stream)>>>(g, work, d_nrm);
    }
    DFL_LAUNCH_CHECK();
}
void dfl_cgs_update_givens(I n, I ncol, const T* Q, int64_t ldq, const T* d_h, T* w, T* d_nrm, T* work, I iter, T* d_H, I ldh,
                           T* d_gv, T* d_beta, T* d_res_hist, void* stream) {
    int g = ceil_div(n, UROWS);
    cgs_update_kernel<true><<<g, BLK, 0, S(stream)>>>(n, ncol, Q, ldq, d_h, w, work);
    norm_givens_kernel<<<1, BLK, 0, S(stream)>>>(g, work, d_nrm, iter, d_H, ldh, d_gv, d_beta, d_res_hist, nullptr);
    DFL_LAUNCH_CHECK();
}
void dfl_cgs_dots_raw(I n, I ncol, const T* Q, int64_t ldq, const T* w, const T* d_nu, T* d_h, T* d_c, T* work, void* stream) {
    if (ncol <= 0) return;
    int nrb = ceil_div(n, ROWS_PER_BLOCK);
    dim3 grid(nrb, ceil_div(ncol, CT));
    cgs_dots_stage1<<<grid, BLK, 0, S(stream)>>>(n, ncol, Q, ldq, w, work, nrb, CT);
    cgs_dots_raw_stage2<<<ncol, BLK, 0, S(stream)>>>(nrb, work, d_nu, d_h, d_c);
    DFL_LAUNCH_CHECK();
}
static int launch_update_jacobi(I N, I ncol, const T* Q, int64_t ldq, const T* d_c, T* w, const T* dinv33, const T* dinv1, T* z4,
                                T* work, void* stream) {
    const int g = ceil_div(N, BLK);
    const int vec_ok = aligned16(Q) && aligned16(w) && !(ldq & 1);
    if (z4) cgs_update_jacobi_kernel<true><<<g, BLK, 0, S(stream)>>>(N, ncol, Q, ldq, d_c, w, work, dinv33, dinv1, z4, vec_ok);
    else cgs_update_jacobi_kernel<false><<<g, BLK, 0, S(stream)>>>(N, ncol, Q, ldq, d_c, w, work, nullptr, nullptr, nullptr, vec_ok);
    return g;
}
void dfl_cgs_update_jacobi_givens_keep(I N, I ncol, const T* Q, int64_t ldq, const T* d_c, T* w, const T* dinv33, const T* dinv1,
                                       T* z4, T* d_nrm, T* work, I iter, T* d_H, I ldh, T* d_gv, T* d_beta, T* d_res_hist,
                                       T* d_raw_col, void* stream) {
    if (N <= 0) return;
    const int g = launch_update_jacobi(N, ncol, Q, ldq, d_c, w, dinv33, dinv1, z4, work, stream);
    norm_givens_kernel<<<1, BLK, 0, S(stream)>>>(g, work, d_nrm, iter, d_H, ldh, d_gv, d_beta, d_res_hist, d_raw_col);
    DFL_LAUNCH_CHECK();
}
void dfl_cgs_update_jacobi_givens(I N, I ncol, const T* Q, int64_t ldq, const T* d_c, T* w, const T* dinv33, const T* dinv1, T* z4,
                                  T* d_nrm, T* work, I iter, T* d_H, I ldh, T* d_gv, T* d_beta, T* d_res_hist, void* stream) {
    dfl_cgs_update_jacobi_givens_keep(N, ncol, Q, ldq, d_c, w, dinv33, dinv1, z4, d_nrm, work, iter, d_H, ldh, d_gv, d_beta, d_res_hist,
                                      nullptr, stream);
}
void dfl_cgs_update_jacobi(I N, I ncol, const T* Q, int64_t ldq, const T* d_c, T* w, const T* dinv33, const T* dinv1, T* z4, T* work,
                           void* stream) {
    if (N <= 0) return;
    (void)launch_update_jacobi(N, ncol, Q, ldq, d_c, w, dinv33, dinv1, z4, work, stream);
    DFL_LAUNCH_CHECK();
}
void dfl_cgs_dots2_raw(I n, I ncol, const T* Q, int64_t ldq, const T* w1, const T* w2, const T* d_nu, T* d_h1, T* d_h1_raw, T* d_c1,
                       T* d_e, T* d_c2, T* work, void* stream) {
    if (ncol <= 0) return;
    int nrb = ceil_div(n, ROWS_PER_BLOCK);
    dim3 grid(nrb, ceil_div(ncol, CT));
    cgs_dots2_stage1<<<grid, BLK, 0, S(stream)>>>(n, ncol, Q, ldq, w1, w2, work, nrb, CT);
    cgs_dots2_stage2<<<dim3(ncol, 2), BLK, 0, S(stream)>>>(nrb, ncol, work, d_nu, d_h1, d_h1_raw, d_c1, d_e, d_c2);
    DFL_LAUNCH_CHECK();
}
void dfl_cgs_update2(I n, I ncol, const T* Q, int64_t ldq, const T* d_c1, const T* d_c2, T* w1, T* w2, T* work, void* stream) {
    if (n <= 0) return;
    cgs_update2_kernel<<<ceil_div(n, UROWS), BLK, 0, S(stream)>>>(n, ncol, Q, ldq, d_c1, d_c2, w1, w2, work);
    DFL_LAUNCH_CHECK();
}
void dfl_gmres_pair_first(int npart, const T* part, I k, T* d_nu, T* d_H, T* d_Hraw, I ldh, T* d_gv, T* d_beta, T* d_res_hist,
                          T* d_sc, void* stream) {
    pair_first_kernel<<<1, BLK, 0, S(stream)>>>(npart, part, k, d_nu, d_H, d_Hraw, ldh, d_gv, d_beta, d_res_hist, d_sc);
    DFL_LAUNCH_CHECK();
}
void dfl_gmres_pair_second(int npart, const T* part, I k, T* d_nu, T* d_H, T* d_Hraw, I ldh, const T* d_e, const T* d_sc, T* d_gv,
                           T* d_beta, T* d_res_hist, int* d_flag, void* stream) {
    pair_second_kernel<<<1, BLK, 0, S(stream)>>>(npart, part, k, d_nu, d_H, d_Hraw, ldh, d_e, d_sc, d_gv, d_beta, d_res_hist, d_flag);
    DFL_LAUNCH_CHECK();
}
int dfl_cgs_update2_parts(I n) { return ceil_div(n, UROWS); }
// blocks of s = 3 or 4 products: any other s is an error (s = 2 is the pair above, s = 1 the single step)
int dfl_cgs_dots_block_parts(I n, int s) {
    if (s == 3) return ceil_div(n, BLK * BlockShape<3>::R * 2);
    if (s == 4) return ceil_div(n, BLK * BlockShape<4>::R * 2);
    abort();
}
int dfl_cgs_update_block_parts(I n, int s) {
    if (s == 3) return ceil_div(n, BLK * BlockShape<3>::U * 2);
    if (s == 4) return ceil_div(n, BLK * BlockShape<4>::U * 2);
    abort();
}
void dfl_cgs_dots_block(I n, I ncol, int s, const T* Q, int64_t ldq, const T* w, int64_t ldw, const T* d_nu, T* d_h, T* d_h_raw,
                        T* d_e, T* d_c, I lde, T* work, void* stream) {
    if (ncol <= 0 || n <= 0) return;
    if (s == 3) launch_dots_block<3>(n, ncol, Q, ldq, w, ldw, d_nu, d_h, d_h_raw, d_e, d_c, lde, work, stream);
    else if (s == 4) launch_dots_block<4>(n, ncol, Q, ldq, w, ldw, d_nu, d_h, d_h_raw, d_e, d_c, lde, work, stream);
    else abort();
    DFL_LAUNCH_CHECK();
}
void dfl_cgs_update_block(I n, I ncol, int s, const T* Q, int64_t ldq, const T* d_c, I lde, T* w, int64_t ldw, T* work,
                          void* stream) {
    if (n <= 0) return;
    const int g = dfl_cgs_update_block_parts(n, s);
    if (s == 3) cgs_update_block_kernel<3, BlockShape<3>::U><<<g, BLK, 0, S(stream)>>>(n, ncol, Q, ldq, d_c, lde, w, ldw, work);
    else cgs_update_block_kernel<4, BlockShape<4>::U><<<g, BLK, 0, S(stream)>>>(n, ncol, Q, ldq, d_c, lde, w, ldw, work);
    DFL_LAUNCH_CHECK();
}
void dfl_gmres_block_first(int npart, const T* part, int s, I k, T* d_nu, T* d_H, T* d_Hraw, I ldh, T* d_gv, T* d_beta,
                           T* d_res_hist, T* d_sc, void* stream) {
    if (s == 3) block_first_kernel<3><<<1, BLK, 0, S(stream)>>>(npart, part, k, d_nu, d_H, d_Hraw, ldh, d_gv, d_beta, d_res_hist, d_sc);
    else if (s == 4) block_first_kernel<4><<<1, BLK, 0, S(stream)>>>(npart, part, k, d_nu, d_H, d_Hraw, ldh, d_gv, d_beta, d_res_hist, d_sc);
    else abort();
    DFL_LAUNCH_CHECK();
}
void dfl_cgs_fixup_block(I N, int s, T* w, int64_t ldw, const T* d_sc, const T* dinv33, const T* dinv1, T* z4, T* work,
                         void* stream) {
    if (N <= 0) return;
    if (s == 3) launch_fixup_block<3>(N, w, ldw, d_sc, dinv33, dinv1, z4, work, stream);
    else if (s == 4) launch_fixup_block<4>(N, w, ldw, d_sc, dinv33, dinv1, z4, work, stream);
    else abort();
    DFL_LAUNCH_CHECK();
}
void dfl_gmres_block_second(int npart, const T* part, int s, I k, T* d_nu, T* d_H, T* d_Hraw, I ldh, const T* d_e, I lde,
                            const T* d_sc, T* d_gv, T* d_beta, T* d_res_hist, int* d_flag, void* stream) {
    if (s == 3)
        block_second_kernel<3><<<1, BLK, 0, S(stream)>>>(npart, part, k, d_nu, d_H, d_Hraw, ldh, d_e, lde, d_sc, d_gv, d_beta, d_res_hist,
                                                         d_flag);
    else if (s == 4)
        block_second_kernel<4><<<1, BLK, 0, S(stream)>>>(npart, part, k, d_nu, d_H, d_Hraw, ldh, d_e, lde, d_sc, d_gv, d_beta, d_res_hist,
                                                         d_flag);
    else abort();
    DFL_LAUNCH_CHECK();
}
int dfl_cgs_update_fixup_block_parts(I N) { return ceil_div(N, BLK); }
void dfl_cgs_dots_block_gram(I n, I ncol, int s, const T* Q, int64_t ldq, const T* w, int64_t ldw, const T* d_nu, T* d_h, T* d_h_raw,
                             T* d_e, T* d_c, I lde, T* d_sc, T* work, void* stream) {
    if (ncol <= 0 || n <= 0) return;
    if (s == 3) launch_dots_block_gram<3>(n, ncol, Q, ldq, w, ldw, d_nu, d_h, d_h_raw, d_e, d_c, lde, d_sc, work, stream);
    else if (s == 4) launch_dots_block_gram<4>(n, ncol, Q, ldq, w, ldw, d_nu, d_h, d_h_raw, d_e, d_c, lde, d_sc, work, stream);
    else abort();
    DFL_LAUNCH_CHECK();
}
void dfl_cgs_update_fixup_block(I N, I ncol, int s, const T* Q, int64_t ldq, const T* d_c, I lde, T* w, int64_t ldw, const T* d_sc,
                                const T* dinv33, const T* dinv1, T* z4, T* work, void* stream) {
    if (N <= 0) return;
    if (s == 3) launch_update_fixup_block<3>(N, ncol, Q, ldq, d_c, lde, w, ldw, d_sc, dinv33, dinv1, z4, work, stream);
    else if (s == 4) launch_update_fixup_block<4>(N, ncol, Q, ldq, d_c, lde, w, ldw, d_sc, dinv33, dinv1, z4, work, stream);
    else abort();
    DFL_LAUNCH_CHECK();
}
void dfl_gmres_block_fused(int npart, const T* part, int s, I k, T* d_nu, T* d_H, T* d_Hraw, I ldh, const T* d_e, I lde, T* d_sc,
                           T* d_gv, T* d_beta, T* d_res_hist, int* d_flag, T tau, void* stream) {
    if (s == 3)
        block_fused_kernel<3><<<1, BLK, 0, S(stream)>>>(npart, part, k, d_nu, d_H, d_Hraw, ldh, d_e, lde, d_sc, d_gv, d_beta, d_res_hist,
                                                        d_flag, tau);
    else if (s == 4)
        block_fused_kernel<4><<<1, BLK, 0, S(stream)>>>(npart, part, k, d_nu, d_H, d_Hraw, ldh, d_e, lde, d_sc, d_gv, d_beta, d_res_hist,
                                                        d_flag, tau);
    else abort();
    DFL_LAUNCH_CHECK();
}
void dfl_gmres_scale_inv(I m, const T* d_nu, T* d_y, void* stream) {
    if (m <= 0) return;
    scale_inv_vec_kernel<<<ceil_div(m, BLK), BLK, 0, S(stream)>>>(m, d_nu, d_y);
    DFL_LAUNCH_CHECK();
}
void dfl_spin_us(int us, void* stream) {
    if (us <= 0) return;
    if (us > 20000) us = 20000;
    spin_kernel<<<1, 64, 0, S(stream)>>>(us, nullptr);
    DFL_LAUNCH_CHECK();
}
void dfl_dsqrt_dev(T* d_val, void* stream) {
    sqrt_kernel<<<1, 1, 0, S(stream)>>>(d_val);
    DFL_LAUNCH_CHECK();
}
void dfl_gemv_n(I n, I ncol, const T* Q, int64_t ldq, const T* d_c, T* y, void* stream) {
    int g = ceil_div(n, UROWS);
    cgs_update_kernel<false><<<g, BLK, 0, S(stream)>>>(n, ncol, Q, ldq, d_c, y, nullptr);
    DFL_LAUNCH_CHECK();
}

void dfl_gmres_givens(I iter, const T* d_nrm, T* d_H, I ldh, T* d_gv, T* d_beta, T* d_res_hist, void* stream) {
    gmres_givens_kernel<false><<<1, BLK, 0, S(stream)>>>(iter, const_cast<T*>(d_nrm), d_H, ldh, d_gv, d_beta, d_res_hist);
    DFL_LAUNCH_CHECK();
}
void dfl_gmres_givens_sq(I iter, T* d_nrm_sq, T* d_H, I ldh, T* d_gv, T* d_beta, T* d_res_hist, void* stream) {
    gmres_givens_kernel<true><<<1, BLK, 0, S(stream)>>>(iter, d_nrm_sq, d_H, ldh, d_gv, d_beta, d_res_hist);
    DFL_LAUNCH_CHECK();
}
void dfl_cgs_update_pc_givens(I nrows, I N, I ncol, const T* Q, int64_t ldq, const T* d_hraw, T* w, const T* dinv33, const T* dinv1,
                              T* z, I iter, T* d_H, I ldh, T* d_gv, T* d_beta, T* d_res_hist, T* d_nrm, int* d_flag, void* stream) {
    dfl_cgs_update_pc_givens_x4(nrows, N, ncol, Q, ldq, d_hraw, w, dinv33, dinv1, z, nullptr, iter, d_H, ldh, d_gv, d_beta, d_res_hist,
                                d_nrm, d_flag, stream);
}
void dfl_cgs_update_pc_givens_x4(I nrows, I N, I ncol, const T* Q, int64_t ldq, const T* d_hraw, T* w, const T* dinv33,
                                 const T* dinv1, T* z, T* z4, I iter, T* d_H, I ldh, T* d_gv, T* d_beta, T* d_res_hist, T* d_nrm,
                                 int* d_flag, void* stream) {
    if (ncol + 1 > GIV_MAX + 2 || nrows <= 0) abort();  // the caller falls back to the separate kernels beyond GIV_MAX columns
    cgs_update_pc_kernel<<<ceil_div(nrows, BLK), BLK, 0, S(stream)>>>(nrows, N, ncol, Q, ldq, d_hraw, w, dinv33, dinv1, z, iter, d_H, ldh,
                                                                      d_gv, d_beta, d_res_hist, d_nrm, d_flag, z4);
    DFL_LAUNCH_CHECK();
}
void dfl_gmres_givens_pythagoras(I iter, T* d_nrm, T* d_H, I ldh, T* d_gv, T* d_beta, T* d_res_hist, int* d_flag, void* stream) {
    gmres_givens_pythagoras_kernel<<<1, BLK, 0, S(stream)>>>(iter, d_nrm, d_H, ldh, d_gv, d_beta, d_res_hist, d_flag);
    DFL_LAUNCH_CHECK();
}
void dfl_gmres_trsv(I m, const T* d_H, I ldh, T* d_beta, void* stream) {
    if (m <= 0) return;
    const size_t staged = ((size_t)m * m + m) * sizeof(double);
    if (staged <= 60 * 1024) gmres_trsv_kernel<true><<<1, BLK, staged, S(stream)>>>(m, d_H, ldh, d_beta);
    else gmres_trsv_kernel<false><<<1, BLK, (size_t)m * sizeof(double), S(stream)>>>(m, d_H, ldh, d_beta);
    DFL_LAUNCH_CHECK();
}
void GMRESResidualUpdatePrivate(T* beta, T* gv) {
    residual_update_kernel<<<1, 1>>>(beta, gv);
    DFL_LAUNCH_CHECK();
}

}  // extern "C"
