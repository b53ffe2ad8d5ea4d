// Block-CSR SpMV, block-Jacobi preconditioner, diagonal extraction, Dirichlet
// row elimination and layout conversion.
//
// Layout (see include/dedflow_kernels.h): val[k*16 + r*4 + c], one 128-byte
// line per nodal nonzero, so a node row is one contiguous run of len*128 B.
// SpMV maps 8 lanes to a node row: lane l owns block entries (2l, 2l+1), i.e.
// one 16-byte load per lane and one full 128-byte line per 8 lanes -- every
// wave instruction touches 8 whole lines, which is what the HBM roofline needs
// (algorithmic bytes 132*nnz1 + 4(N+1) + 64N).
#include "dfl_common.hpp"

namespace {

constexpr int BLK = 256;

// x index of block column c (0..3) of node `col` in the [u AoS | p] layout
__device__ __forceinline__ long long xidx(int col, int c, long long N3) { return c < 3 ? 3LL * col + c : N3 + col; }

typedef double d2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ d2v ld_val(const d2v* p) {
    // the 3.3 GB value stream is read exactly once per matvec: nontemporal keeps it from
    // evicting the gathered x (55 MB at 10M tets) out of L2 / MALL
    return __builtin_nontemporal_load(p);
}

// Matvec reading x INTERLEAVED (x4[node][4] = u0 u1 u2 p, 32 B per node): the pair of lanes of a block row fetches its two
// x entries with ONE 16-byte load each instead of two 8-byte loads from two places (u part / p part of the reference layout):
// one gather instruction and about one L2 request less per nodal nonzero.  Same products, same order: bitwise the same y.
__global__ __launch_bounds__(BLK) void interleave4_kernel(I node0, I node1, I N, const T* __restrict__ x, T* __restrict__ x4) {
    const long long i = node0 + (long long)blockIdx.x * BLK + threadIdx.x;
    if (i >= node1) return;
    double2* o = reinterpret_cast<double2*>(x4 + 4 * i);
    o[0] = make_double2(x[3 * i], x[3 * i + 1]);
    o[1] = make_double2(x[3 * i + 2], x[3LL * N + i]);
}
// The U column indices of a trip come with ONE load per row group (lane l fetches ci[k + l % U]) and are passed round with
// shuffles, instead of U broadcast loads.  DSCALE: y = tot * (1.0 / *d_nrm) instead of alpha * tot -- the raw-basis GMRES step
// folds the normalisation of the Krylov column into the matvec that consumes M^-1 of it (host/gmres.c).
// FOLD: the row group also writes z4_out[row][4] = M^-1 y_row of the block-Jacobi tree, for the product that follows in a
// block of Krylov steps: it holds the row's four components of y after the pair reduction and has streamed the row's
// diagonal block (nonzero diag_pos[row]; each lane keeps its two entries as they pass).  Same inverse (inv3) and same
// expressions as pc_setup_kernel + pc_apply_kernel; y is stored as without FOLD.  z4_out must not be x4 (rows of one launch
// gather x4 of arbitrary other rows)
__device__ __forceinline__ void inv3(const double* m, double* o);
// (FOLD: seven waves per SIMD asked for, as the plain kernel has -- left alone the compiler takes 76 VGPRs for it, six waves)
template <bool DSCALE, bool FOLD>
__global__ __launch_bounds__(BLK, FOLD ? 7 : 1) void bcsr_spmv_x4_kernel(I row0, I nrows, I N, const I* __restrict__ rp,
                                                          const I* __restrict__ ci, const T* __restrict__ val, T alpha,
                                                          const T* __restrict__ x4,
                                                          T* __restrict__ y, const T* __restrict__ d_nrm,
                                                          const I* __restrict__ diag_pos, T* __restrict__ z4_out) {
    constexpr int U = 4;  // nodal nonzeros per loop trip
    long long blk = blockIdx.x;
    const long long per = gridDim.x >> 3;  // grid is a multiple of 8
    blk = (blk & 7) * per + (blk >> 3);
    const long long gid = blk * BLK + threadIdx.x;
    const int row = row0 + (int)(gid >> 3);
    const int l = threadIdx.x & 7;
    if (row >= nrows) return;
    const long long N3 = 3LL * N;
    const int r = l >> 1;
    const int hi = l & 1;
    const int s = rp[row], e = rp[row + 1];
    const d2v* __restrict__ v2 = reinterpret_cast<const d2v*>(val) + l;
    const d2v* __restrict__ xv = reinterpret_cast<const d2v*>(x4) + hi;
    int dp = 0;
    d2v dd = {0.0, 0.0};  // FOLD: entries (2l, 2l+1) of the row's diagonal block
    if constexpr (FOLD) dp = diag_pos[row];
    double acc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) acc[u] = 0.0;
    int k = s;
    for (; k + U <= e; k += U) {
        int c[U];
        d2v a[U], xx[U];
        const int cl = ci[k + (l & (U - 1))];
#pragma unroll
        for (int u = 0; u < U; ++u) c[u] = __shfl(cl, u, 8);
#pragma unroll
        for (int u = 0; u < U; ++u) a[u] = ld_val(v2 + (long long)(k + u) * 8);
#pragma unroll
        for (int u = 0; u < U; ++u) xx[u] = xv[2LL * c[u]];
        // (without this the scheduler, with the diagonal's registers to place, waits for the first gather before it issues the
        // other three: one more trip to L2 per loop trip)
        if constexpr (FOLD) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < U; ++u) acc[u] += a[u].x * xx[u].x + a[u].y * xx[u].y;
        if constexpr (FOLD) {
#pragma unroll
            for (int u = 0; u < U; ++u) dd = (k + u == dp) ? a[u] : dd;
        }
    }
    for (; k < e; ++k) {
        const int c0 = ci[k];
        const d2v a0 = ld_val(v2 + (long long)k * 8);
        const d2v x0 = xv[2LL * c0];
        acc[0] += a0.x * x0.x + a0.y * x0.y;
        if constexpr (FOLD) dd = (k == dp) ? a0 : dd;
    }
    double tot = acc[0];
#pragma unroll
    for (int u = 1; u < U; ++u) tot += acc[u];
    tot += __shfl_xor(tot, 1, WAVE);
    if constexpr (!FOLD) {
        if (DSCALE) {
            if (!hi) y[xidx(row, r, N3)] = tot * (1.0 / d_nrm[0]);
        } else {
            if (!hi) y[xidx(row, r, N3)] = alpha * tot;
        }
    } else {
        const double yv = DSCALE ? tot * (1.0 / d_nrm[0]) : alpha * tot;  // both lanes of a pair: the fold reads it from either
        if (!hi) y[xidx(row, r, N3)] = yv;
        // lane 2r holds D[r][0], D[r][1], lane 2r+1 holds D[r][2], D[r][3]; both lanes of a pair hold y_r
        double m[9], o[9];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            m[3 * q + 0] = __shfl(dd.x, 2 * q, 8);
            m[3 * q + 1] = __shfl(dd.y, 2 * q, 8);
            m[3 * q + 2] = __shfl(dd.x, 2 * q + 1, 8);
        }
        const double x0 = __shfl(yv, 0, 8), x1 = __shfl(yv, 2, 8), x2 = __shfl(yv, 4, 8);
        inv3(m, o);  // row-major inv(D) == the column-major image A of pc_apply_kernel: A(r,c) = o[r + 3c]
        d2v* out = reinterpret_cast<d2v*>(z4_out + 4LL * row);
        if (l == 0) {
            const d2v z01 = {o[0] * x0 + o[3] * x1 + o[6] * x2, o[1] * x0 + o[4] * x1 + o[7] * x2};
            out[0] = z01;
        } else if (l == 7) {  // this lane holds D[3][3] and y_p
            const d2v z2p = {o[2] * x0 + o[5] * x1 + o[8] * x2, yv * (1.0 / dd.y)};
            out[1] = z2p;
        }
    }
}

// ---- single-precision COPY of the block values (PC_TWOLEVEL only: its smoother and its residual matvec read it; the Krylov
// solver outside is flexible and stays in double precision).  Same lane mapping as the double-precision kernel -- 8 lanes per
// node row, lane l owns entries (2l, 2l+1) of every block, now one 8-byte load -- half the bytes per matvec.
typedef float f2v __attribute__((ext_vector_type(2)));
__global__ __launch_bounds__(BLK) void values_to_f32_kernel(long long n, const T* __restrict__ val, float* __restrict__ valf) {
    const long long i = ((long long)blockIdx.x * BLK + threadIdx.x) * 4;
    if (i + 3 < n) {
        const double2 a = *reinterpret_cast<const double2*>(val + i), b = *reinterpret_cast<const double2*>(val + i + 2);
        *reinterpret_cast<float4*>(valf + i) = make_float4((float)a.x, (float)a.y, (float)b.x, (float)b.y);
    } else {
        for (long long k = i; k < n; ++k) valf[k] = (float)val[k];
    }
}
__global__ __launch_bounds__(BLK) void bcsr_spmv_f32_kernel(I nrows, I N, const I* __restrict__ rp, const I* __restrict__ ci,
                                                           const float* __restrict__ valf, const T* __restrict__ x,
                                                           T* __restrict__ y) {
    long long blk = blockIdx.x;
    const long long per = gridDim.x >> 3;  // grid is a multiple of 8: one contiguous slab of rows per XCD
    blk = (blk & 7) * per + (blk >> 3);
    const long long gid = blk * BLK + threadIdx.x;
    const int row = (int)(gid >> 3);
    const int l = threadIdx.x & 7;
    if (row >= nrows) return;  // whole 8-lane groups
    const long long N3 = 3LL * N;
    const int r = l >> 1;
    const bool hi = (l & 1);
    const int s = rp[row], e = rp[row + 1];
    const f2v* __restrict__ v2 = reinterpret_cast<const f2v*>(valf) + l;
    // eight nonzeros in flight per row group: with 8-byte value loads the bytes in flight per wave are those of the
    // double-precision kernel with four (at U = 4 this kernel took 0.55 ms against 0.59 ms for twice the bytes: latency-bound)
    constexpr int U = 8;
    double acc[U] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int k = s;
    for (; k + U <= e; k += U) {
        int c[U];
        f2v a[U];
        double xa[U], xb[U];
#pragma unroll
        for (int u = 0; u < U; ++u) c[u] = ci[k + u];
#pragma unroll
        for (int u = 0; u < U; ++u) a[u] = __builtin_nontemporal_load(v2 + (long long)(k + u) * 8);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            xa[u] = x[hi ? 3LL * c[u] + 2 : 3LL * c[u]];
            xb[u] = x[hi ? N3 + c[u] : 3LL * c[u] + 1];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) acc[u] += (double)a[u].x * xa[u] + (double)a[u].y * xb[u];
    }
    for (; k + 4 <= e; k += 4) {
        int c[4];
        f2v a[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) c[u] = ci[k + u];
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] = __builtin_nontemporal_load(v2 + (long long)(k + u) * 8);
#pragma unroll
        for (int u = 0; u < 4; ++u)
            acc[u] += (double)a[u].x * x[hi ? 3LL * c[u] + 2 : 3LL * c[u]] + (double)a[u].y * x[hi ? N3 + c[u] : 3LL * c[u] + 1];
    }
    for (; k < e; ++k) {
        const int c0 = ci[k];
        const f2v a0 = __builtin_nontemporal_load(v2 + (long long)k * 8);
        acc[0] += (double)a0.x * x[hi ? 3LL * c0 + 2 : 3LL * c0] + (double)a0.y * x[hi ? N3 + c0 : 3LL * c0 + 1];
    }
    double tot = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
    tot += __shfl_xor(tot, 1, WAVE);
    if (!hi) y[xidx(row, r, N3)] = tot;
}

// U nodal nonzeros per loop trip: all U index loads, then all U value loads, then the 2U
// gathers are issued before the first FMA -- more bytes in flight per 8-lane row group
template <bool BETA0, bool XCD>
__global__ __launch_bounds__(BLK) void bcsr_spmv_kernel(I row0, I nrows, I N, const I* __restrict__ rp, const I* __restrict__ ci,
                                                       const T* __restrict__ val, T alpha, const T* __restrict__ x, T beta,
                                                       T* __restrict__ y) {
    constexpr int U = 4;
    // XCD: workgroup b runs on XCD b % 8 (one L2 each); hand every XCD one contiguous slab of rows so that the x
    // entries shared by neighbouring rows are fetched into ONE L2 instead of up to eight
    long long blk = blockIdx.x;
    if (XCD) {
        const long long per = gridDim.x >> 3;  // grid is a multiple of 8
        blk = (blk & 7) * per + (blk >> 3);
    }
    const long long gid = blk * BLK + threadIdx.x;
    const int row = row0 + (int)(gid >> 3);
    const int l = threadIdx.x & 7;
    if (row >= nrows) return;  // whole 8-lane groups
    const long long N3 = 3LL * N;
    const int r = l >> 1;
    const bool hi = (l & 1);  // false: columns (u0,u1); true: columns (u2,p)
    const int s = rp[row], e = rp[row + 1];
    const d2v* __restrict__ v2 = reinterpret_cast<const d2v*>(val) + l;
    double acc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) acc[u] = 0.0;
    int k = s;
    for (; k + U <= e; k += U) {
        int c[U];
        d2v a[U];
        double xa[U], xb[U];
#pragma unroll
        for (int u = 0; u < U; ++u) c[u] = ci[k + u];
#pragma unroll
        for (int u = 0; u < U; ++u) a[u] = ld_val(v2 + (long long)(k + u) * 8);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long ia = hi ? 3LL * c[u] + 2 : 3LL * c[u];
            const long long ib = hi ? N3 + c[u] : 3LL * c[u] + 1;
            xa[u] = x[ia];
            xb[u] = x[ib];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) acc[u] += a[u].x * xa[u] + a[u].y * xb[u];
    }
    for (; k < e; ++k) {
        const int c0 = ci[k];
        const d2v a0 = ld_val(v2 + (long long)k * 8);
        const long long ia = hi ? 3LL * c0 + 2 : 3LL * c0;
        const long long ib = hi ? N3 + c0 : 3LL * c0 + 1;
        acc[0] += a0.x * x[ia] + a0.y * x[ib];
    }
    double tot = acc[0];
#pragma unroll
    for (int u = 1; u < U; ++u) tot += acc[u];
    tot += __shfl_xor(tot, 1, WAVE);
    if (!hi) {
        const long long yi = xidx(row, r, N3);
        y[yi] = BETA0 ? alpha * tot : alpha * tot + beta * y[yi];
    }
}

// scalar CSR, 8 lanes per row (reference-layout sub-matrices)
__global__ __launch_bounds__(BLK) void csr_spmv_kernel(I nrow, const I* __restrict__ rp, const I* __restrict__ ci,
                                                      const T* __restrict__ val, T alpha, const T* __restrict__ x, T beta,
                                                      T* __restrict__ y) {
    const long long gid = (long long)blockIdx.x * BLK + threadIdx.x;
    const long long row = gid >> 3;
    const int l = threadIdx.x & 7;
    if (row >= nrow) return;
    double acc = 0.0;
    for (int k = rp[row] + l; k < rp[row + 1]; k += 8) acc += val[k] * x[ci[k]];
    acc += __shfl_xor(acc, 1, WAVE);
    acc += __shfl_xor(acc, 2, WAVE);
    acc += __shfl_xor(acc, 4, WAVE);
    if (l == 0) y[row] = (beta == 0.0) ? alpha * acc : alpha * acc + beta * y[row];
}

__device__ __forceinline__ int find_diag(const I* __restrict__ rp, const I* __restrict__ ci, int node) {
    int lo = rp[node], hi = rp[node + 1] - 1;  // col_ind sorted ascending per row (csr.c:57-79)
    while (lo < hi) {
        int mid = (lo + hi) >> 1;
        if (ci[mid] < node) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(BLK) void diag_pos_kernel(I N, const I* __restrict__ rp, const I* __restrict__ ci, I* __restrict__ diag_pos) {
    const int node = blockIdx.x * BLK + threadIdx.x;
    if (node < N) diag_pos[node] = find_diag(rp, ci, node);
}

// closed-form inverse of a 3x3 given row-major m; returns inverse row-major
__device__ __forceinline__ void inv3(const double* m, double* o) {
    const double c00 = m[4] * m[8] - m[5] * m[7];
    const double c01 = m[5] * m[6] - m[3] * m[8];
    const double c02 = m[3] * m[7] - m[4] * m[6];
    const double det = m[0] * c00 + m[1] * c01 + m[2] * c02;
    const double id = 1.0 / det;
    o[0] = c00 * id;
    o[1] = (m[2] * m[7] - m[1] * m[8]) * id;
    o[2] = (m[1] * m[5] - m[2] * m[4]) * id;
    o[3] = c01 * id;
    o[4] = (m[0] * m[8] - m[2] * m[6]) * id;
    o[5] = (m[2] * m[3] - m[0] * m[5]) * id;
    o[6] = c02 * id;
    o[7] = (m[1] * m[6] - m[0] * m[7]) * id;
    o[8] = (m[0] * m[4] - m[1] * m[3]) * id;
}

// PCJacobiSetup (pc.c:44-85): the reference extracts D row-major, hands the 9
// numbers to column-major LAPACK (=> inverts D^T) and keeps the column-major
// result.  Memory image = inv(D^T) column-major = inv(D) row-major.
__global__ __launch_bounds__(BLK) void pc_setup_kernel(I nrows, const I* rp, const I* ci, const T* val, T* dinv33, T* dinv1) {
    const int node = blockIdx.x * BLK + threadIdx.x;
    if (node >= nrows) return;
    const int k = find_diag(rp, ci, node);
    const T* b = val + (long long)k * 16;
    double m[9], o[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) m[r * 3 + c] = b[r * 4 + c];
    inv3(m, o);
#pragma unroll
    for (int i = 0; i < 9; ++i) dinv33[(long long)node * 9 + i] = o[i];  // inv(D) row-major == inv(D^T) col-major
    dinv1[node] = 1.0 / b[15];
}

// PCDecompositionApply (pc.c:136-147): z_u = inv(D)^T r_u (Q7), z_p = r_p * dinv1, tail copied.
template <bool SCALED>
__global__ __launch_bounds__(BLK) void pc_apply_kernel(I nrows, I N, const T* __restrict__ dinv33, const T* __restrict__ dinv1,
                                                      const T* __restrict__ x, const T* __restrict__ d_nrm, T* __restrict__ q,
                                                      T* __restrict__ y, T* __restrict__ y4 = nullptr) {
    const long long i = (long long)blockIdx.x * BLK + threadIdx.x;
    const double s = SCALED ? 1.0 / d_nrm[0] : 1.0;
    if (i < nrows) {
        const T* A = dinv33 + i * 9;  // column-major image: A(r,c) = A[r + 3c]
        double x0 = x[3 * i], x1 = x[3 * i + 1], x2 = x[3 * i + 2], xp = x[3LL * N + i];
        if (SCALED) {
            x0 *= s; x1 *= s; x2 *= s; xp *= s;
            q[3 * i] = x0; q[3 * i + 1] = x1; q[3 * i + 2] = x2; q[3LL * N + i] = xp;
        }
        const double y0 = A[0] * x0 + A[3] * x1 + A[6] * x2, y1 = A[1] * x0 + A[4] * x1 + A[7] * x2;
        const double y2 = A[2] * x0 + A[5] * x1 + A[8] * x2, yp = xp * dinv1[i];
        if (y) {  // (y == NULL: the caller only wants the interleaved copy)
            y[3 * i + 0] = y0; y[3 * i + 1] = y1; y[3 * i + 2] = y2; y[3LL * N + i] = yp;
        }
        if (y4) {  // the interleaved copy the matvec gathers from (dfl_bcsr_spmv_x4): 32 B per node, written here for free
            double2* o = reinterpret_cast<double2*>(y4 + 4 * i);
            o[0] = make_double2(y0, y1);
            o[1] = make_double2(y2, yp);
        }
    }
}

// PCNone sections (phi, T): plain copy, optionally with the same normalisation
__global__ __launch_bounds__(BLK) void tail_copy_kernel(long long begin, long long n, const T* x, const T* d_nrm, T* q, T* y) {
    const long long i = begin + (long long)blockIdx.x * BLK + threadIdx.x;
    if (i >= n) return;
    double v = x[i];
    if (d_nrm) { v *= 1.0 / d_nrm[0]; q[i] = v; }
    y[i] = v;
}

__global__ __launch_bounds__(BLK) void block3_invert_kernel(I N, T* d) {
    const int node = blockIdx.x * BLK + threadIdx.x;
    if (node >= N) return;
    double m[9], o[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) m[i] = d[(long long)node * 9 + i];
    inv3(m, o);
#pragma unroll
    for (int i = 0; i < 9; ++i) d[(long long)node * 9 + i] = o[i];
}

// cublasDgemvStridedBatched(OP_N) on the column-major image (pc.c:104-112)
__global__ __launch_bounds__(BLK) void block3_apply_kernel(I N, const T* __restrict__ dinv, const T* __restrict__ x, T* __restrict__ y) {
    const long long i = (long long)blockIdx.x * BLK + threadIdx.x;
    if (i >= N) return;
    const T* A = dinv + i * 9;
    const double x0 = x[3 * i], x1 = x[3 * i + 1], x2 = x[3 * i + 2];
    y[3 * i + 0] = A[0] * x0 + A[3] * x1 + A[6] * x2;
    y[3 * i + 1] = A[1] * x0 + A[4] * x1 + A[7] * x2;
    y[3 * i + 2] = A[2] * x0 + A[5] * x1 + A[8] * x2;
}

__global__ __launch_bounds__(BLK) void get_diag_kernel(I N, const I* rp, const I* ci, const T* val, T* d33, T* dp, T* du) {
    const int node = blockIdx.x * BLK + threadIdx.x;
    if (node >= N) return;
    const int k = find_diag(rp, ci, node);
    const T* b = val + (long long)k * 16;
    if (d33)
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) d33[(long long)node * 9 + r * 3 + c] = b[r * 4 + c];
    if (dp) dp[node] = b[15];
    if (du)
        for (int r = 0; r < 3; ++r) du[(long long)node * 3 + r] = b[r * 4 + r];
}

// one thread per (nodal nonzero, entry)
template <bool EXPORT>
__global__ __launch_bounds__(BLK) void convert_kernel(I N, const I* __restrict__ rp, T* __restrict__ val, T* A00, T* A01,
                                                     T* A10, T* A11) {
    const int node = blockIdx.x;
    const int start = rp[node], len = rp[node + 1] - start;
    for (int t = threadIdx.x; t < len * 16; t += BLK) {
        const int kk = t >> 4, e = t & 15, r = e >> 2, c = e & 3;
        T* blk = val + ((long long)(start + kk)) * 16 + e;
        T* dst;
        if (r < 3 && c < 3) dst = A00 + (long long)start * 9 + (long long)r * len * 3 + kk * 3 + c;  // csr_impl.cu:24-59
        else if (r < 3) dst = A01 + (long long)start * 3 + (long long)r * len + kk;
        else if (c < 3) dst = A10 + (long long)start * 3 + kk * 3 + c;
        else dst = A11 + start + kk;
        if (EXPORT) *dst = *blk; else *blk = *dst;
    }
}

__global__ __launch_bounds__(BLK) void dirichlet_vec_kernel(T* b, I n, const I* bnode, I shape, I comp) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i >= n) return;
    b[(long long)bnode[i] * shape + comp] = 0.0;
}

// MatrixFSZeroRow on the block layout: A00 row <- diag * delta, A01 row <- 0
// (matrix.c:449-469, matrix_impl.cu:6-23).  8 lanes per boundary node.
__global__ __launch_bounds__(BLK) void zero_rows_kernel(I N, const I* rp, const I* ci, T* val, I n, const I* bnode, I comp,
                                                       T diag) {
    const long long gid = (long long)blockIdx.x * BLK + threadIdx.x;
    const int i = (int)(gid >> 3), l = threadIdx.x & 7;
    if (i >= n) return;
    const int node = bnode[i];
    if (node < 0 || node >= N) return;
    for (int k = rp[node] + l; k < rp[node + 1]; k += 8) {
        T* b = val + (long long)k * 16 + comp * 4;
        const bool isdiag = (ci[k] == node);
        b[0] = (isdiag && comp == 0) ? diag : 0.0;
        b[1] = (isdiag && comp == 1) ? diag : 0.0;
        b[2] = (isdiag && comp == 2) ? diag : 0.0;
        b[3] = 0.0;
    }
}

// ---- reference-layout launchers (same symbols as matrix_impl.h / dirichlet.c) ----
__global__ void ref_zero_row_kernel(T* matval, I num_row, const I* rp, const I* ci, I n, const I* row, I shift, T diag) {
    int i = blockDim.x * blockIdx.x + threadIdx.x;
    if (i >= n) return;
    I ir = shift + row[i];
    if (ir < 0 || ir >= num_row) return;
    for (I j = rp[ir]; j < rp[ir + 1]; ++j) matval[j] = diag * (T)(ci[j] == ir);
}
__global__ void ref_get_diag_kernel(const T* val, const I* rp, const I* ci, T* diag, I num_row) {
    int i = blockDim.x * blockIdx.x + threadIdx.x;
    if (i >= num_row) return;
    for (I j = rp[i]; j < rp[i + 1]; ++j)
        if (ci[j] == i) { diag[i] = val[j]; break; }
}
__global__ void ref_get_diag_block_kernel(const T* matval, I bs, I num_row, const I* rp, const I* ci, T* out, int lda, int stride) {
    int idx = blockDim.x * blockIdx.x + threadIdx.x;
    if (idx >= num_row) return;
    I start = rp[idx], end = rp[idx + 1], len = end - start, k;
    for (k = start; k < end; ++k) if (ci[k] == idx) break;
    const T* m = matval + (long long)start * bs * bs + (long long)(k - start) * bs;
    T* d = out + (long long)idx * stride;
    for (I i = 0; i < bs; ++i)
        for (I j = 0; j < bs; ++j) d[i * lda + j] = m[(long long)i * len * bs + j];
}
__global__ void row_from_node_kernel(I n, I* row, I shape, I init) {
    int i = blockDim.x * blockIdx.x + threadIdx.x;
    if (i < n) row[i] = row[i] * shape + init;
}
__global__ void node_from_row_kernel(I n, I* node, I shape) {
    int i = blockDim.x * blockIdx.x + threadIdx.x;
    if (i < n) node[i] = node[i] / shape;
}

// scalar-CSR point Jacobi, y_i = x_i / a_ii (pc_impl.cu:7-40; y may alias x for the in-place form).  Rows without a stored
// diagonal are left untouched, as in the reference.
__global__ __launch_bounds__(BLK) void csr_jacobi_kernel(I n, const T* __restrict__ data, const I* __restrict__ rp,
                                                        const I* __restrict__ ci, const T* x, T* y) {
    const long long i = (long long)blockIdx.x * BLK + threadIdx.x;
    if (i >= n) return;
    I lo = rp[i], hi = rp[i + 1] - 1;
    if (lo > hi) return;
    while (lo < hi) {
        const I mid = (lo + hi) >> 1;
        if (ci[mid] < (I)i) lo = mid + 1; else hi = mid;
    }
    if (ci[lo] == (I)i) y[i] = x[i] / data[lo];
}

// SetBlockValueToSubmatGPU (matrix_impl.h:59-64, kernel matrix_impl.cu:370-453): the colored scatter of the reference --
// one thread per (batch element, a, b); the (offset[i], offset[j]) sub-block of the lda-strided element block goes into
// sub-matrix (i, j)'s row-expanded value array (NULL sub-matrices are skipped), m = alpha*m + beta*b.  Row-expanded
// layout (csr_impl.cu:24-59): scalar row node*br + ii holds len*bc entries, entry (k - start)*bc + jj.
__global__ __launch_bounds__(BLK) void block_to_submat_kernel(T* const* __restrict__ matval, T alpha, I n_offset,
                                                             const I* __restrict__ offset, I nshl, I batch_size,
                                                             const I* __restrict__ batch_index_ptr, const I* __restrict__ ien,
                                                             const I* __restrict__ rp, const I* __restrict__ ci,
                                                             const T* __restrict__ val, int lda, int stride, T beta,
                                                             const I* __restrict__ mask) {
    const long long idx = (long long)blockIdx.x * BLK + threadIdx.x;
    const int n2 = nshl * nshl;
    if (idx >= (long long)batch_size * n2) return;
    const long long slot = idx / n2;
    if (mask && mask[slot] == 0) return;
    const long long iel = batch_index_ptr ? batch_index_ptr[slot] : slot;
    const int aa = (int)(idx % n2) / nshl, bb = (int)(idx % nshl);
    const I row = ien[iel * nshl + aa], col = ien[iel * nshl + bb];
    const I start = rp[row], len = rp[row + 1] - start;
    I lo = 0, hi = len - 1;  // ascending column indices inside a row
    while (lo < hi) {
        const I mid = (lo + hi) >> 1;
        if (ci[start + mid] < col) lo = mid + 1; else hi = mid;
    }
    if (len <= 0 || ci[start + lo] != col) return;
    const T* b = val + idx * stride;
    for (I i = 0; i < n_offset; ++i) {
        const I br = offset[i + 1] - offset[i];
        for (I j = 0; j < n_offset; ++j) {
            T* m = matval[i * n_offset + j];
            if (!m) continue;
            const I bc = offset[j + 1] - offset[j];
            m += (long long)start * br * bc + (long long)lo * bc;
            for (I ii = 0; ii < br; ++ii)
                for (I jj = 0; jj < bc; ++jj) {
                    T* dst = m + (long long)ii * len * bc + jj;
                    *dst = alpha * *dst + beta * b[(offset[i] + ii) * lda + (offset[j] + jj)];
                }
        }
    }
}


// (batch slot, a, b) -> element id, row node, column node and the position of (row, col) in the nodal pattern (-1: absent)
struct ElemEntry { long long iel; I row, start, len, pos; };
__device__ __forceinline__ ElemEntry elem_entry(long long idx, I nshl, const I* __restrict__ batch_index_ptr,
                                                const I* __restrict__ ien, const I* __restrict__ rp, const I* __restrict__ ci) {
    const int n2 = nshl * nshl;
    const long long slot = idx / n2;
    ElemEntry e;
    e.iel = batch_index_ptr ? batch_index_ptr[slot] : slot;
    const int aa = (int)(idx % n2) / nshl, bb = (int)(idx % nshl);
    e.row = ien[e.iel * nshl + aa];
    const I col = ien[e.iel * nshl + bb];
    e.start = rp[e.row];
    e.len = rp[e.row + 1] - e.start;
    I lo = 0, hi = e.len - 1;  // ascending column indices inside a row
    while (lo < hi) {
        const I mid = (lo + hi) >> 1;
        if (ci[e.start + mid] < col) lo = mid + 1; else hi = mid;
    }
    e.pos = (e.len > 0 && ci[e.start + lo] == col) ? lo : -1;
    return e;
}

// One scalar or row-expanded block CSR matrix over a nodal pattern (the single-matrix case of the kernel above):
// MatrixCSRAddElemValue[Blocked]BatchedGPU, matrix_impl.h:29-43.  The reference's kernels (matrix_impl.cu:88-208) take
// the (a, b) pair from the ELEMENT id instead of the thread id and mix two value layouts; this is the behaviour their
// call sites document (scatter of one br x bc block per (element, a, b) into the layout of csr_impl.cu:24-59).
__global__ __launch_bounds__(BLK) void csr_elem_blocked_kernel(T* __restrict__ matval, T alpha, I nshl, I batch_size,
                                                              const I* __restrict__ batch_index_ptr, const I* __restrict__ ien,
                                                              const I* __restrict__ rp, const I* __restrict__ ci, I br, I bc,
                                                              const T* __restrict__ val, int lda, int stride, T beta,
                                                              const I* __restrict__ mask) {
    const long long idx = (long long)blockIdx.x * BLK + threadIdx.x;
    if (idx >= (long long)batch_size * nshl * nshl) return;
    if (mask && mask[idx / (nshl * nshl)] == 0) return;
    const ElemEntry e = elem_entry(idx, nshl, batch_index_ptr, ien, rp, ci);
    if (e.pos < 0) return;
    T* m = matval + (long long)e.start * br * bc + (long long)e.pos * bc;
    const T* b = val + idx * stride;
    for (I ii = 0; ii < br; ++ii)
        for (I jj = 0; jj < bc; ++jj) {
            T* dst = m + (long long)ii * e.len * bc + jj;
            *dst = alpha * *dst + beta * b[ii * lda + jj];
        }
}

// the same scatter straight into the 4x4 block array of a block-mode (u,p) MatrixFS: rows / columns 0..3 of the
// lda-strided element block, the phi / T part dropped exactly as the reference drops it (NULL sub-matrices)
__global__ __launch_bounds__(BLK) void bcsr_elem_scatter_kernel(T* __restrict__ block_val, T alpha, I nshl, I batch_size,
                                                               const I* __restrict__ batch_index_ptr, const I* __restrict__ ien,
                                                               const I* __restrict__ rp, const I* __restrict__ ci,
                                                               const T* __restrict__ val, int lda, int stride, T beta,
                                                               const I* __restrict__ mask) {
    const long long idx = (long long)blockIdx.x * BLK + threadIdx.x;
    if (idx >= (long long)batch_size * nshl * nshl) return;
    if (mask && mask[idx / (nshl * nshl)] == 0) return;
    const ElemEntry e = elem_entry(idx, nshl, batch_index_ptr, ien, rp, ci);
    if (e.pos < 0) return;
    T* m = block_val + ((long long)e.start + e.pos) * 16;
    const T* b = val + idx * stride;
#pragma unroll
    for (int ii = 0; ii < 4; ++ii)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) m[ii * 4 + jj] = alpha * m[ii * 4 + jj] + beta * b[ii * lda + jj];
}

// MatrixZeroRow on a block-mode (u,p) MatrixFS: `row` holds scalar rows of the velocity block-row (node*3 + comp,
// dirichlet.c:54-59); rows outside [0, 3N) after the shift are skipped like the reference's pressure block-row call
// (matrix.c:449-469).  8 lanes per row.
__global__ __launch_bounds__(BLK) void bcsr_zero_scalar_rows_kernel(I N, const I* rp, const I* ci, T* val, I n, const I* row,
                                                                   I shift, T diag) {
    const long long gid = (long long)blockIdx.x * BLK + threadIdx.x;
    const int i = (int)(gid >> 3), l = threadIdx.x & 7;
    if (i >= n) return;
    const long long r = (long long)row[i] + shift;
    if (r < 0 || r >= 3LL * N) return;
    const int node = (int)(r / 3), comp = (int)(r - 3LL * node);
    for (int k = rp[node] + l; k < rp[node + 1]; k += 8) {
        T* b = val + (long long)k * 16 + comp * 4;
        const bool isdiag = (ci[k] == node);
        b[0] = (isdiag && comp == 0) ? diag : 0.0;
        b[1] = (isdiag && comp == 1) ? diag : 0.0;
        b[2] = (isdiag && comp == 2) ? diag : 0.0;
        b[3] = 0.0;
    }
}

// MatrixCSRSetValue[Blocked]BatchedGPU (matrix_impl.h:45-62): one (row, col) pair per thread
__global__ __launch_bounds__(BLK) void csr_set_blocked_kernel(T* __restrict__ matval, T alpha, const I* __restrict__ rp,
                                                             const I* __restrict__ ci, I batch_size, const I* __restrict__ brow,
                                                             const I* __restrict__ bcol, I br, I bc, const T* __restrict__ A,
                                                             T beta, int lda, int stride) {
    const long long idx = (long long)blockIdx.x * BLK + threadIdx.x;
    if (idx >= batch_size) return;
    const I row = brow[idx], col = bcol[idx];
    const I start = rp[row], len = rp[row + 1] - start;
    I pos = -1;
    for (I k = 0; k < len; ++k)
        if (ci[start + k] == col) { pos = k; break; }
    if (pos < 0) return;
    T* m = matval + (long long)start * br * bc + (long long)pos * bc;
    const T* a = A + idx * stride;
    for (I ii = 0; ii < br; ++ii)
        for (I jj = 0; jj < bc; ++jj) {
            T* dst = m + (long long)ii * len * bc + jj;
            *dst = beta * a[ii * lda + jj] + alpha * *dst;
        }
}

// MatrixCSRAddElementLHSGPU (matrix_impl.h:38-43, kernel matrix_impl.cu:209-247): scalar CSR whose rows / columns are
// node*BS + component; one thread per element adds its (NSHL*BS)^2 dense block.  One batch must be conflict-free.
__global__ __launch_bounds__(BLK) void csr_add_element_lhs_kernel(T* __restrict__ matval, I nshl, I bs, const I* __restrict__ rp,
                                                                 const I* __restrict__ ci, I batch_size,
                                                                 const I* __restrict__ batch_ptr, const I* __restrict__ ien,
                                                                 const T* __restrict__ val) {
    const long long idx = (long long)blockIdx.x * BLK + threadIdx.x;
    if (idx >= batch_size) return;
    const long long iel = batch_ptr ? batch_ptr[idx] : idx;
    const T* v = val + (long long)nshl * nshl * bs * bs * idx;
    for (I aa = 0; aa < nshl; ++aa)
        for (I ii = 0; ii < bs; ++ii) {
            const I ir = ien[iel * nshl + aa] * bs + ii;
            for (I bb = 0; bb < nshl; ++bb)
                for (I jj = 0; jj < bs; ++jj) {
                    const I ic = ien[iel * nshl + bb] * bs + jj;
                    for (I j = rp[ir]; j < rp[ir + 1]; ++j)
                        if (ci[j] == ic) { matval[j] += v[(aa * bs + ii) * bs * nshl + bb * bs + jj]; break; }
                }
        }
}

}  // namespace

extern "C" {

void dfl_bcsr_spmv_range(I row0, I row1, I N, const I* rp, const I* ci, const T* val, T alpha, const T* x, T beta, T* y,
                         void* stream) {
    if (row1 <= row0) return;
    const I nrows = row1;
    const int grid = ceil_div((long long)(row1 - row0) * 8, BLK);
    if (beta == 0.0)
        bcsr_spmv_kernel<true, true><<<(grid + 7) & ~7, BLK, 0, S(stream)>>>(row0, nrows, N, rp, ci, val, alpha, x, beta, y);
    else
        bcsr_spmv_kernel<false, false><<<grid, BLK, 0, S(stream)>>>(row0, nrows, N, rp, ci, val, alpha, x, beta, y);
    DFL_LAUNCH_CHECK();
}
void dfl_bcsr_spmv_rows(I nrows, I N, const I* rp, const I* ci, const T* val, T alpha, const T* x, T beta, T* y, void* stream) {
    dfl_bcsr_spmv_range(0, nrows, N, rp, ci, val, alpha, x, beta, y, stream);
}
void PCJacobiDevice(I n, I nnz, double* data, I* rp, I* ci, double* x, double* y) {  // pc_impl.h:6
    (void)nnz;
    if (n > 0) csr_jacobi_kernel<<<ceil_div(n, BLK), BLK>>>(n, data, rp, ci, x, y);
    DFL_LAUNCH_CHECK();
}
void PCJacobiInplaceDevice(I n, I nnz, double* data, I* rp, I* ci, double* x) {  // pc_impl.h:7
    PCJacobiDevice(n, nnz, data, rp, ci, x, x);
}
void SetBlockValueToSubmatGPU(T** matval, T alpha, I n_offset, const I* offset, I nshl, I batch_size, const I* batch_index_ptr,
                              const I* ien, I num_row, I num_col, const I* rp, const I* ci, const T* val, int lda, int stride, T beta,
                              const I* mask) {
    (void)num_row; (void)num_col;
    if (batch_size <= 0) return;
    const long long nthread = (long long)batch_size * nshl * nshl;
    block_to_submat_kernel<<<ceil_div(nthread, BLK), BLK>>>(matval, alpha, n_offset, offset, nshl, batch_size, batch_index_ptr, ien,
                                                            rp, ci, val, lda, stride, beta, mask);
    DFL_LAUNCH_CHECK();
}

void MatrixCSRAddElemValueBlockedBatchedGPU(T* matval, T alpha, I batch_size, const I* batch_index_ptr, const I* ien, I nshl,
                                            I num_row, I num_col, const I* rp, const I* ci, I block_row, I block_col, const T* val,
                                            int lda, int stride, T beta, const I* mask) {
    (void)num_row; (void)num_col;
    if (batch_size <= 0) return;
    csr_elem_blocked_kernel<<<ceil_div((long long)batch_size * nshl * nshl, BLK), BLK>>>(matval, alpha, nshl, batch_size, batch_index_ptr,
                                                                                        ien, rp, ci, block_row, block_col, val, lda,
                                                                                        stride, beta, mask);
    DFL_LAUNCH_CHECK();
}
void MatrixCSRAddElemValueBatchedGPU(T* matval, T alpha, I batch_size, const I* batch_index_ptr, const I* ien, I nshl, I num_row,
                                     I num_col, const I* rp, const I* ci, const T* val, T beta, const I* mask) {
    MatrixCSRAddElemValueBlockedBatchedGPU(matval, alpha, batch_size, batch_index_ptr, ien, nshl, num_row, num_col, rp, ci, 1, 1, val, 1,
                                           1, beta, mask);
}
void MatrixCSRSetValueBlockedBatchedGPU(T* matval, T alpha, I csr_num_row, I csr_num_col, const I* rp, const I* ci, I batch_size,
                                        const I* batch_row_ind, const I* batch_col_ind, I block_row, I block_col, const T* A, T beta,
                                        int lda, int stride) {
    (void)csr_num_row; (void)csr_num_col;
    if (batch_size <= 0) return;
    csr_set_blocked_kernel<<<ceil_div(batch_size, BLK), BLK>>>(matval, alpha, rp, ci, batch_size, batch_row_ind, batch_col_ind, block_row,
                                                               block_col, A, beta, lda, stride);
    DFL_LAUNCH_CHECK();
}
void MatrixCSRSetValueBatchedGPU(T* matval, T alpha, I csr_num_row, I csr_num_col, const I* rp, const I* ci, I batch_size,
                                 const I* batch_row_ind, const I* batch_col_ind, const T* A, T beta) {
    MatrixCSRSetValueBlockedBatchedGPU(matval, alpha, csr_num_row, csr_num_col, rp, ci, batch_size, batch_row_ind, batch_col_ind, 1, 1, A,
                                       beta, 1, 1);
}
void MatrixCSRAddElementLHSGPU(T* matval, I nshl, I bs, I num_row, const I* rp, I num_col, const I* ci, I batch_size,
                               const I* batch_ptr, const I* ien, const T* val, int lda) {
    (void)num_row; (void)num_col; (void)lda;
    if (batch_size <= 0) return;
    csr_add_element_lhs_kernel<<<ceil_div(batch_size, BLK), BLK>>>(matval, nshl, bs, rp, ci, batch_size, batch_ptr, ien, val);
    DFL_LAUNCH_CHECK();
}
void dfl_bcsr_add_elem_blocked(T* block_val, T alpha, I nshl, I batch_size, const I* batch_index_ptr, const I* ien, const I* rp,
                               const I* ci, const T* val, int lda, int stride, T beta, const I* mask, void* stream) {
    if (batch_size <= 0) return;
    bcsr_elem_scatter_kernel<<<ceil_div((long long)batch_size * nshl * nshl, BLK), BLK, 0, S(stream)>>>(
        block_val, alpha, nshl, batch_size, batch_index_ptr, ien, rp, ci, val, lda, stride, beta, mask);
    DFL_LAUNCH_CHECK();
}
void dfl_bcsr_zero_scalar_rows(I N, const I* rp, const I* ci, T* val, I n, const I* row, I shift, T diag, void* stream) {
    if (n <= 0) return;
    bcsr_zero_scalar_rows_kernel<<<ceil_div((long long)n * 8, BLK), BLK, 0, S(stream)>>>(N, rp, ci, val, n, row, shift, diag);
    DFL_LAUNCH_CHECK();
}
void dfl_interleave4(I node0, I node1, I N, const T* x, T* x4, void* stream) {
    if (node1 <= node0) return;
    interleave4_kernel<<<ceil_div(node1 - node0, BLK), BLK, 0, S(stream)>>>(node0, node1, N, x, x4);
    DFL_LAUNCH_CHECK();
}
void dfl_bcsr_spmv_x4(I row0, I row1, I N, const I* rp, const I* ci, const T* val, T alpha, const T* x4, T* y, void* stream) {
    if (row1 <= row0) return;
    const int grid = ceil_div((long long)(row1 - row0) * 8, BLK);
    const int grid8 = (grid + 7) & ~7;
    // (column indices by one cooperative load per row group and trip: 0.4990 against 0.5027 ms back to back)
    bcsr_spmv_x4_kernel<false, false><<<grid8, BLK, 0, S(stream)>>>(row0, row1, N, rp, ci, val, alpha, x4, y, nullptr, nullptr, nullptr);
    DFL_LAUNCH_CHECK();
}
void dfl_bcsr_spmv_x4_scaled(I row0, I row1, I N, const I* rp, const I* ci, const T* val, const T* d_nrm, const T* x4, T* y,
                             void* stream) {
    if (row1 <= row0) return;
    const int grid = ceil_div((long long)(row1 - row0) * 8, BLK);
    const int grid8 = (grid + 7) & ~7;
    bcsr_spmv_x4_kernel<true, false><<<grid8, BLK, 0, S(stream)>>>(row0, row1, N, rp, ci, val, 1.0, x4, y, d_nrm, nullptr, nullptr);
    DFL_LAUNCH_CHECK();
}
// the two products above over all N rows, each row group also writing z4_out[row][4] = M^-1 y_row (block-Jacobi tree; diag_pos:
// dfl_bcsr_diag_pos).  Returns 0, or -1 without a launch when z4_out is the buffer x4 is gathered from
int dfl_bcsr_spmv_x4_pc(I N, const I* rp, const I* ci, const I* diag_pos, const T* val, const T* x4, T* y, T* z4_out, void* stream) {
    if (z4_out == x4 || !z4_out || !diag_pos) return -1;
    if (N <= 0) return 0;
    const int grid8 = (ceil_div((long long)N * 8, BLK) + 7) & ~7;
    bcsr_spmv_x4_kernel<false, true><<<grid8, BLK, 0, S(stream)>>>(0, N, N, rp, ci, val, 1.0, x4, y, nullptr, diag_pos, z4_out);
    DFL_LAUNCH_CHECK();
    return 0;
}
int dfl_bcsr_spmv_x4_scaled_pc(I N, const I* rp, const I* ci, const I* diag_pos, const T* val, const T* d_nrm, const T* x4, T* y,
                               T* z4_out, void* stream) {
    if (z4_out == x4 || !z4_out || !diag_pos) return -1;
    if (N <= 0) return 0;
    const int grid8 = (ceil_div((long long)N * 8, BLK) + 7) & ~7;
    bcsr_spmv_x4_kernel<true, true><<<grid8, BLK, 0, S(stream)>>>(0, N, N, rp, ci, val, 1.0, x4, y, d_nrm, diag_pos, z4_out);
    DFL_LAUNCH_CHECK();
    return 0;
}
// diag_pos[row] = the nonzero that pc_setup_kernel inverts for this row (the stored diagonal; col_ind sorted per row)
void dfl_bcsr_diag_pos(I N, const I* rp, const I* ci, I* diag_pos, void* stream) {
    if (N <= 0) return;
    diag_pos_kernel<<<ceil_div(N, BLK), BLK, 0, S(stream)>>>(N, rp, ci, diag_pos);
    DFL_LAUNCH_CHECK();
}
void dfl_bcsr_values_to_f32(int64_t n, const T* val, float* valf, void* stream) {
    if (n <= 0) return;
    values_to_f32_kernel<<<(unsigned)((n / 4 + BLK) / BLK), BLK, 0, S(stream)>>>(n, val, valf);
    DFL_LAUNCH_CHECK();
}
void dfl_bcsr_spmv_f32(I nrows, I N, const I* rp, const I* ci, const float* valf, const T* x, T* y, void* stream) {
    if (nrows <= 0) return;
    const long long groups = ((long long)nrows * 8 + BLK - 1) / BLK;
    const unsigned grid8 = (unsigned)((groups + 7) / 8 * 8);
    bcsr_spmv_f32_kernel<<<grid8, BLK, 0, S(stream)>>>(nrows, N, rp, ci, valf, x, y);
    DFL_LAUNCH_CHECK();
}
void dfl_bcsr_spmv(I N, const I* rp, const I* ci, const T* val, T alpha, const T* x, T beta, T* y, void* stream) {
    dfl_bcsr_spmv_rows(N, N, rp, ci, val, alpha, x, beta, y, stream);
}

void dfl_csr_spmv(I nrow, const I* rp, const I* ci, const T* val, T alpha, const T* x, T beta, T* y, void* stream) {
    if (nrow <= 0) return;
    csr_spmv_kernel<<<ceil_div((long long)nrow * 8, BLK), BLK, 0, S(stream)>>>(nrow, rp, ci, val, alpha, x, beta, y);
    DFL_LAUNCH_CHECK();
}

void dfl_pc_jacobi_setup_rows(I nrows, const I* rp, const I* ci, const T* val, T* dinv33, T* dinv1, void* stream) {
    if (nrows <= 0) return;
    pc_setup_kernel<<<ceil_div(nrows, BLK), BLK, 0, S(stream)>>>(nrows, rp, ci, val, dinv33, dinv1);
    DFL_LAUNCH_CHECK();
}
void dfl_pc_jacobi_setup(I N, const I* rp, const I* ci, const T* val, T* dinv33, T* dinv1, void* stream) {
    dfl_pc_jacobi_setup_rows(N, rp, ci, val, dinv33, dinv1, stream);
}

void dfl_pc_jacobi_apply_rows(I nrows, I N, I n, const T* dinv33, const T* dinv1, const T* x, T* y, void* stream) {
    if (nrows > 0) pc_apply_kernel<false><<<ceil_div(nrows, BLK), BLK, 0, S(stream)>>>(nrows, N, dinv33, dinv1, x, nullptr, nullptr, y);
    if (n > 4 * N)
        tail_copy_kernel<<<ceil_div((long long)n - 4LL * N, BLK), BLK, 0, S(stream)>>>(4LL * N, n, x, nullptr, nullptr, y);
    DFL_LAUNCH_CHECK();
}
void dfl_pc_jacobi_apply(I N, I n, const T* dinv33, const T* dinv1, const T* x, T* y, void* stream) {
    dfl_pc_jacobi_apply_rows(N, N, n, dinv33, dinv1, x, y, stream);
}

void dfl_pc_jacobi_apply_scaled_rows(I nrows, I N, I n, const T* dinv33, const T* dinv1, const T* w, const T* d_nrm, T* q_out,
                                     T* y, void* stream) {
    if (nrows > 0) {
        pc_apply_kernel<true><<<ceil_div(nrows, BLK), BLK, 0, S(stream)>>>(nrows, N, dinv33, dinv1, w, d_nrm, q_out, y);
    }
    if (n > 4 * N)
        tail_copy_kernel<<<ceil_div((long long)n - 4LL * N, BLK), BLK, 0, S(stream)>>>(4LL * N, n, w, d_nrm, q_out, y);
    DFL_LAUNCH_CHECK();
}
void dfl_pc_jacobi_apply_scaled_rows_x4(I nrows, I N, I n, const T* dinv33, const T* dinv1, const T* w, const T* d_nrm, T* q_out,
                                        T* y, T* y4, void* stream) {
    if (nrows > 0) {
        const int g = ceil_div(nrows, BLK);
        if (d_nrm) pc_apply_kernel<true><<<g, BLK, 0, S(stream)>>>(nrows, N, dinv33, dinv1, w, d_nrm, q_out, y, y4);
        else pc_apply_kernel<false><<<g, BLK, 0, S(stream)>>>(nrows, N, dinv33, dinv1, w, nullptr, nullptr, y, y4);
    }
    if (n > 4 * N && y)
        tail_copy_kernel<<<ceil_div((long long)n - 4LL * N, BLK), BLK, 0, S(stream)>>>(4LL * N, n, w, d_nrm, q_out, y);
    DFL_LAUNCH_CHECK();
}
void dfl_pc_jacobi_apply_scaled(I N, I n, const T* dinv33, const T* dinv1, const T* w, const T* d_nrm, T* q_out, T* y,
                                void* stream) {
    dfl_pc_jacobi_apply_scaled_rows(N, N, n, dinv33, dinv1, w, d_nrm, q_out, y, stream);
}

void dfl_block3_invert(I N, T* diag33, void* stream) {
    if (N <= 0) return;
    block3_invert_kernel<<<ceil_div(N, BLK), BLK, 0, S(stream)>>>(N, diag33);
    DFL_LAUNCH_CHECK();
}
void dfl_block3_apply(I N, const T* dinv33, const T* x, T* y, void* stream) {
    if (N <= 0) return;
    block3_apply_kernel<<<ceil_div(N, BLK), BLK, 0, S(stream)>>>(N, dinv33, x, y);
    DFL_LAUNCH_CHECK();
}

void dfl_bcsr_get_diag(I N, const I* rp, const I* ci, const T* val, T* d33, T* dp, T* du, void* stream) {
    if (N <= 0) return;
    get_diag_kernel<<<ceil_div(N, BLK), BLK, 0, S(stream)>>>(N, rp, ci, val, d33, dp, du);
    DFL_LAUNCH_CHECK();
}

void dfl_block_export_fs(I N, const I* rp, const T* val, T* A00, T* A01, T* A10, T* A11, void* stream) {
    if (N <= 0) return;
    convert_kernel<true><<<N, BLK, 0, S(stream)>>>(N, rp, const_cast<T*>(val), A00, A01, A10, A11);
    DFL_LAUNCH_CHECK();
}
void dfl_block_import_fs(I N, const I* rp, T* val, const T* A00, const T* A01, const T* A10, const T* A11, void* stream) {
    if (N <= 0) return;
    convert_kernel<false><<<N, BLK, 0, S(stream)>>>(N, rp, val, const_cast<T*>(A00), const_cast<T*>(A01), const_cast<T*>(A10),
                                                   const_cast<T*>(A11));
    DFL_LAUNCH_CHECK();
}

void dfl_dirichlet_vec(T* b, I n, const I* bnode, I shape, I comp, void* stream) {
    if (n <= 0) return;
    dirichlet_vec_kernel<<<ceil_div(n, BLK), BLK, 0, S(stream)>>>(b, n, bnode, shape, comp);
    DFL_LAUNCH_CHECK();
}
void ApplyBCVecNodalGPU(T* b, I n, const I* bc_node, I shape, I init) { dfl_dirichlet_vec(b, n, bc_node, shape, init, nullptr); }

void dfl_bcsr_zero_rows(I N, const I* rp, const I* ci, T* val, I n, const I* bnode, I comp, T diag, void* stream) {
    if (n <= 0) return;
    zero_rows_kernel<<<ceil_div((long long)n * 8, BLK), BLK, 0, S(stream)>>>(N, rp, ci, val, n, bnode, comp, diag);
    DFL_LAUNCH_CHECK();
}

void MatrixCSRZeroRowGPU(T* matval, I num_row, I num_col, const I* rp, const I* ci, I n, const I* row, I shift, T diag) {
    (void)num_col;
    if (n <= 0) return;  // the reference launches with a negative n for the pressure block-row (matrix.c:464)
    ref_zero_row_kernel<<<ceil_div(n, BLK), BLK>>>(matval, num_row, rp, ci, n, row, shift, diag);
    DFL_LAUNCH_CHECK();
}
void MatrixCSRGetDiagGPU(const T* val, const I* rp, const I* ci, T* diag, I num_row) {
    if (num_row <= 0) return;
    ref_get_diag_kernel<<<ceil_div(num_row, BLK), BLK>>>(val, rp, ci, diag, num_row);
    DFL_LAUNCH_CHECK();
}
void MatrixGetDiagBlockGPU(const T* matval, I bs, I num_row, I num_col, const I* rp, const I* ci, T* out, int lda, int stride) {
    (void)num_col;
    if (num_row <= 0) return;
    ref_get_diag_block_kernel<<<ceil_div(num_row, BLK), BLK>>>(matval, bs, num_row, rp, ci, out, lda, stride);
    DFL_LAUNCH_CHECK();
}
void GetRowFromNodeGPU(I n, I* row, I shape, I init) {
    if (n <= 0) return;
    row_from_node_kernel<<<ceil_div(n, BLK), BLK>>>(n, row, shape, init);
    DFL_LAUNCH_CHECK();
}
void GetNodeFromRowGPU(I n, I* node, I shape) {
    if (n <= 0) return;
    node_from_row_kernel<<<ceil_div(n, BLK), BLK>>>(n, node, shape);
    DFL_LAUNCH_CHECK();
}

}  // extern "C"
