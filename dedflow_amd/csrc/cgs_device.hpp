// What the Krylov translation units (k_blas.hip, k_cgs.hip, k_cgs_block.hip) share: the launch constants, the nontemporal
// stream load, the block-wide sums, the Givens step, and ONE copy of every rule their kernels repeat -- the row slot, the
// Jacobi epilogue, the second stage of a reduction, the raw-basis coefficients and the launcher dispatch.  Where the tests
// demand bit-for-bit equality between paths (the fused pass against update + fix-up, the dots with Gram sums against the
// plain dots), both sides call the same helper.  Not here: the node-block slot rule (slots [0, 384) u rows, [384, 512) p
// rows) of cgs_update_jacobi_kernel, cgs_fixup_block_kernel and cgs_update_fixup_block_kernel -- every shared form of it
// that was tried compiled the three kernels to other code.
// Everything has internal linkage: every translation unit compiles its own copy into its own code object.
#pragma once
#include "dfl_common.hpp"
#include <cmath>
#include <cstdlib>
#include <type_traits>

// k_blas.hip: reduce_stage2 for the other translation units, d_out[0] = the sum of the npart partials (take_sqrt: its root)
void dfl_reduce_partials(int npart, const T* part, T* d_out, int take_sqrt, void* stream);

namespace {

constexpr int BLK = 256;

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Krylov basis columns are streamed once per pass (2.3 GB at 10M tets, m = 40): nontemporal
// loads keep them from displacing w and the partial sums in L2 / MALL.
typedef double d2s __attribute__((ext_vector_type(2)));
__device__ __forceinline__ double2 ld_stream(const T* p) {
    const d2s v = __builtin_nontemporal_load(reinterpret_cast<const d2s*>(p));
    return make_double2(v.x, v.y);
}

// ---- fused CGS: launch constants -----------------------------------------------------------------------------------------
constexpr int CT = 8;
constexpr int RPT = 4;                      // double2 slots per thread
constexpr int ROWS_PER_BLOCK = BLK * RPT * 2;  // 2048 rows
constexpr int UPT = 2;  // double2 slots per thread (1 and 4 measured: 0.2093 against 0.2028 ms per CGS kernel)
constexpr int UROWS = BLK * UPT * 2;

// ---- the n-bounded row slot ------------------------------------------------------------------------------------------------
// Rows `row`, `row + 1` of a vector of n rows: one 16-byte access if both rows are inside, else scalar with zero fill (row + 1
// is then outside).  Plain load, nontemporal load (basis columns), store.  The two-vector kernels of the pair
// (cgs_dots2_stage1, cgs_update2_kernel) keep their own copy for w1, w2: there one test guards both vectors, and two calls
// of these helpers compile to other code.
__device__ __forceinline__ double2 slot_load(const T* p, long long row, I n) {
    double2 v;
    if (row + 1 < n) v = *reinterpret_cast<const double2*>(p + row);
    else { v.x = (row < n) ? p[row] : 0.0; v.y = 0.0; }
    return v;
}
__device__ __forceinline__ double2 slot_stream(const T* q, long long row, I n) {
    double2 v;
    if (row + 1 < n) v = ld_stream(q + row);
    else { v.x = (row < n) ? q[row] : 0.0; v.y = 0.0; }
    return v;
}
__device__ __forceinline__ void slot_store(T* p, long long row, I n, const double2& v) {
    if (row + 1 < n) *reinterpret_cast<double2*>(p + row) = v;
    else if (row < n) p[row] = v.x;
}

// ---- the Jacobi application ------------------------------------------------------------------------------------------------
// y = M^-1 x of node i: A = dinv33 + 9 i, the column-major image of its inverted 3 x 3 velocity block, as pc_apply_kernel
// (Q7); dinv1[i] its inverted pressure diagonal, read last
__device__ __forceinline__ void jacobi_apply_node(const T* A, const T* dinv1, long long i, double x0, double x1, double x2,
                                                  double xp, double& y0, double& y1, double& y2, double& yp) {
    y0 = A[0] * x0 + A[3] * x1 + A[6] * x2;
    y1 = A[1] * x0 + A[4] * x1 + A[7] * x2;
    y2 = A[2] * x0 + A[5] * x1 + A[8] * x2;
    yp = xp * dinv1[i];
}
// The epilogue of a node-block kernel (a workgroup owns the nb <= 256 nodes from a0): sm holds the block's 512 double2 slots,
// doubles [0, 768) u and [768, 1024) p, published by a barrier; regrouped to one node per thread, z4[node] = M^-1 x[node],
// interleaved for dfl_bcsr_spmv_x4
__device__ __forceinline__ void jacobi_store_z4(const double2* sm, long long nb, long long a0, const T* dinv33, const T* dinv1,
                                                T* z4) {
    const double* s = reinterpret_cast<const double*>(sm);
    const int t = threadIdx.x;
    if (t < nb) {
        const long long i = a0 + t;
        const T* A = dinv33 + i * 9;
        const double x0 = s[3 * t], x1 = s[3 * t + 1], x2 = s[3 * t + 2], xp = s[768 + t];
        double y0, y1, y2, yp;
        jacobi_apply_node(A, dinv1, i, x0, x1, x2, xp, y0, y1, y2, yp);
        double2* o = reinterpret_cast<double2*>(z4 + 4 * i);
        o[0] = make_double2(y0, y1);
        o[1] = make_double2(y2, yp);
    }
}

// ---- block-wide sums -------------------------------------------------------------------------------------------------------
// second stage of a reduction, one workgroup: the n stage-1 partials in a fixed order; result valid in thread 0
__device__ __forceinline__ double partials_sum_256(const T* part, int n, double* lds4) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += BLK) acc += part[i];
    return block_sum_256(acc, lds4);
}

// the coefficients of a raw dot g = <r_j, w> (raw basis: r_j = nu q_j): (h, c), h = g / nu goes into H, c = h / nu multiplies
// r_j in the update; called by thread 0 of a dots stage 2
__device__ __forceinline__ double2 raw_coeff(double g, double nu) {
    const double h = g / nu;
    return make_double2(h, h / nu);
}

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

// ---- launcher dispatch -----------------------------------------------------------------------------------------------------
// blocks of s = 3 or 4 products: f(std::integral_constant<int, s>); any other s is an error (s = 2 is the pair, s = 1 the
// single step)
template <class F>
auto dispatch_block_size(int s, F f) -> decltype(f(std::integral_constant<int, 3>())) {
    if (s == 3) return f(std::integral_constant<int, 3>());
    if (s == 4) return f(std::integral_constant<int, 4>());
    abort();
}
// the Z4 instantiation of a kernel writes z4, the other does not: f(std::true_type) if z4, else f(std::false_type)
template <class F>
void dispatch_z4(const T* z4, F f) {
    if (z4) f(std::true_type());
    else f(std::false_type());
}

}  // namespace
