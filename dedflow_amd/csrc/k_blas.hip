// BLAS-1, deterministic reductions and the driver's state algebra -- replaces the
// cuBLAS calls of src/krylov.c:114-319, src/main.c:107-130 and the elementwise
// kernels of src/vec.cu:14-76.  (Fused classical Gram-Schmidt and the GMRES small
// recurrences: k_cgs.hip, one Arnoldi step per pass; k_cgs_block.hip, two to four.)
// All of these are HBM-bound streams: 16-byte accesses per lane, grid sized to
// a few blocks per CU, two-stage (order-fixed) reductions instead of atomics so
// that Krylov residual histories are bitwise reproducible run to run.
#include "cgs_device.hpp"

static char g_err[512] = "";
void dfl_record_error(hipError_t e, const char* file, int line) {
    snprintf(g_err, sizeof g_err, "HIP error: %s at %s:%d", hipGetErrorString(e), file, line);
    fprintf(stderr, "GPUAssert: %s\n", g_err);
}

namespace {

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
    const double r = partials_sum_256(part, npart, lds);
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

}  // namespace

void dfl_reduce_partials(int npart, const T* part, T* d_out, int take_sqrt, void* stream) {
    if (take_sqrt) reduce_stage2<true><<<1, BLK, 0, S(stream)>>>(npart, part, d_out);
    else reduce_stage2<false><<<1, BLK, 0, S(stream)>>>(npart, part, d_out);
}

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
void GMRESResidualUpdatePrivate(T* beta, T* gv) {
    residual_update_kernel<<<1, 1>>>(beta, gv);
    DFL_LAUNCH_CHECK();
}

}  // extern "C"
