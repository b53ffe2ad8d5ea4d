// Two to four Arnoldi steps per pass over the raw Krylov basis: the pair kernels, the blocks of three and four, and the
// fused block pass whose update and fix-up are one kernel.  The row slot, Jacobi and reduction rules are
// those of cgs_device.hpp; one step per pass: k_cgs.hip.
#include "cgs_device.hpp"

namespace {

// ---- two Arnoldi steps per pass over the raw basis (GmresPlan.pair) -----------------------------------------------------
// p1 = B v_k and p2 = B p1 (B = A M^-1) are orthogonalised against r_0..r_k together: one dots pass and one update pass
// over the basis serve both.  v_{k+1} comes from p1 as in the single step; p2 additionally loses its component along
// v_{k+1} (the one-column fix-up, cgs_update_jacobi_kernel), which leaves a multiple of v_{k+2}; column k+1 of H follows
// from the raw dots of p2 and the un-rotated earlier columns (pair_second_kernel).

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
            const double2 qv = slot_stream(q, row[i], n);
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
    const double r = partials_sum_256(part + ((long long)blockIdx.y * ncol + j) * nrb, nrb, lds);
    if (threadIdx.x == 0) {
        const double2 hc = raw_coeff(r, nu[j]);
        if (blockIdx.y == 0) {
            d_h1[j] = hc.x;
            if (d_h1_raw) d_h1_raw[j] = hc.x;
            d_c1[j] = hc.y;
        } else {
            d_e[j] = hc.x;
            d_c2[j] = hc.y;
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
            const double2 qv = slot_stream(q, row[i], n);
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
    const double qq = partials_sum_256(part, npart, lds);
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
        for (int a = 0; a < S; ++a) u[a][i] = slot_load(w + a * ldw, row[i], n);
    }
    auto load = [&](int c, double2(&qv)[R]) {
        const T* q = Q + (long long)(c0 + c) * ldq;
#pragma unroll
        for (int i = 0; i < R; ++i) qv[i] = slot_stream(q, row[i], n);
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

// what the second stage of the block dots leaves for vector i and column j, thread 0: hc = (e_i[j], c_i[j])
__device__ __forceinline__ void store_block_coeff(const double2& hc, int i, int j, T* d_h, T* d_h_raw, T* d_e, T* d_c, I lde) {
    d_e[(long long)i * lde + j] = hc.x;
    d_c[(long long)i * lde + j] = hc.y;
    if (i == 0) {
        d_h[j] = hc.x;
        if (d_h_raw) d_h_raw[j] = hc.x;
    }
}

// grid (ncol, S), the order of cgs_dots_raw_stage2: e_i[j] = <r_j, p_i> / nu_j at d_e[i lde + j], c_i = e_i / nu at d_c[i lde + j];
// e_0 is also column k of H and of its un-rotated copy (d_h, d_h_raw)
__global__ __launch_bounds__(BLK) void cgs_dots_block_stage2(int nrb, I ncol, const T* part, const T* __restrict__ nu, T* d_h,
                                                            T* d_h_raw, T* d_e, T* d_c, I lde) {
    __shared__ double lds[4];
    const int j = blockIdx.x, i = blockIdx.y;
    const double r = partials_sum_256(part + ((long long)i * ncol + j) * nrb, nrb, lds);
    if (threadIdx.x == 0) store_block_coeff(raw_coeff(r, nu[j]), i, j, d_h, d_h_raw, d_e, d_c, lde);
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
        for (int a = 0; a < S; ++a) v[a][i] = slot_load(w + a * ldw, row[i], n);
    }
#pragma unroll 4
    for (int j = 0; j < ncol; ++j) {
        double h[S];
#pragma unroll
        for (int a = 0; a < S; ++a) h[a] = (j < 128) ? sh[a][j] : d_c[(long long)a * lde + j];
        const T* q = Q + (long long)j * ldq;
#pragma unroll
        for (int i = 0; i < U; ++i) {
            const double2 qv = slot_stream(q, row[i], n);
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
        for (int a = 0; a < S; ++a) slot_store(w + a * ldw, row[i], n, v[a][i]);
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
    const double r = partials_sum_256(p, nrb, lds);
    if (threadIdx.x == 0) {
        if (dots) store_block_coeff(raw_coeff(r, nu[j]), i, j, d_h, d_h_raw, d_e, d_c, lde);
        else graw[blockIdx.x - nd] = r;
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
    if (Z4) jacobi_store_z4(sm, nb, a0, dinv33, dinv1, z4);
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
    if (Z4) jacobi_store_z4(sm, nb, a0, dinv33, dinv1, z4);
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
    dispatch_z4(z4, [&](auto z) {
        cgs_update_fixup_block_kernel<NS, decltype(z)::value><<<g, BLK, 0, S(stream)>>>(N, ncol, Q, ldq, d_c, lde, w, ldw, d_sc, work, dinv33,
                                                                                        dinv1, z4, vec_ok);
    });
}
template <int NS>
void launch_fixup_block(I N, T* w, int64_t ldw, const T* d_sc, const T* dinv33, const T* dinv1, T* z4, T* work, void* stream) {
    const int g = ceil_div(N, BLK);
    const int vec_ok = aligned16(w) && !(ldw & 1);
    dispatch_z4(z4, [&](auto z) {
        cgs_fixup_block_kernel<NS, decltype(z)::value><<<g, BLK, 0, S(stream)>>>(N, w, ldw, d_sc, work, dinv33, dinv1, z4, vec_ok);
    });
}

}  // namespace

extern "C" {
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
// blocks of s = 3 or 4 products: any other s is an error (dispatch_block_size; s = 2 is the pair above, s = 1 the single step)
int dfl_cgs_dots_block_parts(I n, int s) {
    return dispatch_block_size(s, [&](auto ns) { return ceil_div(n, BLK * BlockShape<ns()>::R * 2); });
}
int dfl_cgs_update_block_parts(I n, int s) {
    return dispatch_block_size(s, [&](auto ns) { return ceil_div(n, BLK * BlockShape<ns()>::U * 2); });
}
void dfl_cgs_dots_block(I n, I ncol, int s, const T* Q, int64_t ldq, const T* w, int64_t ldw, const T* d_nu, T* d_h, T* d_h_raw,
                        T* d_e, T* d_c, I lde, T* work, void* stream) {
    if (ncol <= 0 || n <= 0) return;
    dispatch_block_size(s, [&](auto ns) { launch_dots_block<ns()>(n, ncol, Q, ldq, w, ldw, d_nu, d_h, d_h_raw, d_e, d_c, lde, work, stream); });
    DFL_LAUNCH_CHECK();
}
void dfl_cgs_update_block(I n, I ncol, int s, const T* Q, int64_t ldq, const T* d_c, I lde, T* w, int64_t ldw, T* work,
                          void* stream) {
    if (n <= 0) return;
    const int g = dfl_cgs_update_block_parts(n, s);
    dispatch_block_size(s, [&](auto ns) {
        cgs_update_block_kernel<ns(), BlockShape<ns()>::U><<<g, BLK, 0, S(stream)>>>(n, ncol, Q, ldq, d_c, lde, w, ldw, work);
    });
    DFL_LAUNCH_CHECK();
}
void dfl_gmres_block_first(int npart, const T* part, int s, I k, T* d_nu, T* d_H, T* d_Hraw, I ldh, T* d_gv, T* d_beta,
                           T* d_res_hist, T* d_sc, void* stream) {
    dispatch_block_size(s, [&](auto ns) {
        block_first_kernel<ns()><<<1, BLK, 0, S(stream)>>>(npart, part, k, d_nu, d_H, d_Hraw, ldh, d_gv, d_beta, d_res_hist, d_sc);
    });
    DFL_LAUNCH_CHECK();
}
void dfl_cgs_fixup_block(I N, int s, T* w, int64_t ldw, const T* d_sc, const T* dinv33, const T* dinv1, T* z4, T* work,
                         void* stream) {
    if (N <= 0) return;
    dispatch_block_size(s, [&](auto ns) { launch_fixup_block<ns()>(N, w, ldw, d_sc, dinv33, dinv1, z4, work, stream); });
    DFL_LAUNCH_CHECK();
}
void dfl_gmres_block_second(int npart, const T* part, int s, I k, T* d_nu, T* d_H, T* d_Hraw, I ldh, const T* d_e, I lde,
                            const T* d_sc, T* d_gv, T* d_beta, T* d_res_hist, int* d_flag, void* stream) {
    dispatch_block_size(s, [&](auto ns) {
        block_second_kernel<ns()><<<1, BLK, 0, S(stream)>>>(npart, part, k, d_nu, d_H, d_Hraw, ldh, d_e, lde, d_sc, d_gv, d_beta, d_res_hist,
                                                            d_flag);
    });
    DFL_LAUNCH_CHECK();
}
int dfl_cgs_update_fixup_block_parts(I N) { return ceil_div(N, BLK); }
void dfl_cgs_dots_block_gram(I n, I ncol, int s, const T* Q, int64_t ldq, const T* w, int64_t ldw, const T* d_nu, T* d_h, T* d_h_raw,
                             T* d_e, T* d_c, I lde, T* d_sc, T* work, void* stream) {
    if (ncol <= 0 || n <= 0) return;
    dispatch_block_size(s, [&](auto ns) {
        launch_dots_block_gram<ns()>(n, ncol, Q, ldq, w, ldw, d_nu, d_h, d_h_raw, d_e, d_c, lde, d_sc, work, stream);
    });
    DFL_LAUNCH_CHECK();
}
void dfl_cgs_update_fixup_block(I N, I ncol, int s, const T* Q, int64_t ldq, const T* d_c, I lde, T* w, int64_t ldw, const T* d_sc,
                                const T* dinv33, const T* dinv1, T* z4, T* work, void* stream) {
    if (N <= 0) return;
    dispatch_block_size(s, [&](auto ns) {
        launch_update_fixup_block<ns()>(N, ncol, Q, ldq, d_c, lde, w, ldw, d_sc, dinv33, dinv1, z4, work, stream);
    });
    DFL_LAUNCH_CHECK();
}
void dfl_gmres_block_fused(int npart, const T* part, int s, I k, T* d_nu, T* d_H, T* d_Hraw, I ldh, const T* d_e, I lde, T* d_sc,
                           T* d_gv, T* d_beta, T* d_res_hist, int* d_flag, T tau, void* stream) {
    dispatch_block_size(s, [&](auto ns) {
        block_fused_kernel<ns()><<<1, BLK, 0, S(stream)>>>(npart, part, k, d_nu, d_H, d_Hraw, ldh, d_e, lde, d_sc, d_gv, d_beta, d_res_hist,
                                                           d_flag, tau);
    });
    DFL_LAUNCH_CHECK();
}

}  // extern "C"
