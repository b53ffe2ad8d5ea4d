// One Arnoldi step per pass over the Krylov basis: fused classical Gram-Schmidt (dots, update, the update with the Jacobi
// application folded in), the Givens recurrence and the triangular solve of GMRES.  The row slot, Jacobi and reduction
// rules are those of cgs_device.hpp; two to four steps per pass: k_cgs_block.hip.
#include "cgs_device.hpp"

namespace {

// ---- fused CGS -------------------------------------------------------------------
// d_h[j] = Q[:,j].w : grid (row blocks, column tiles of CT); each thread owns
// RPT double2 row slots, keeps w in registers across the CT columns of its tile.
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
        wv[i] = slot_load(w, row[i], n);
    }
    for (int c = 0; c < ct; ++c) {
        const int col = c0 + c;
        if (col >= ncol) break;  // uniform
        const T* q = Q + (long long)col * ldq;
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
            const double2 qv = slot_stream(q, row[i], n);
            acc += qv.x * wv[i].x + qv.y * wv[i].y;
        }
        double r = block_sum_256(acc, lds);
        if (threadIdx.x == 0) part[(long long)col * nrb + blockIdx.x] = r;
    }
}

__global__ __launch_bounds__(BLK) void cgs_dots_stage2(int nrb, const T* part, T* d_h) {
    __shared__ double lds[4];
    const double r = partials_sum_256(part + (long long)blockIdx.x * nrb, nrb, lds);
    if (threadIdx.x == 0) d_h[blockIdx.x] = r;
}

// w -= Q h (SUB) or y = Q c (!SUB); optional partial ||w||^2 per block
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
        if (SUB) acc[i] = slot_load(w, row[i], n);
        else { acc[i].x = 0.0; acc[i].y = 0.0; }
    }
#pragma unroll 4  // (8 columns in flight: 0.212 against 0.205 ms per CGS kernel -- slower)
    for (int j = 0; j < ncol; ++j) {
        const double h = (j < 128) ? sh[j] : d_h[j];
        const T* q = Q + (long long)j * ldq;
#pragma unroll
        for (int i = 0; i < UPT; ++i) {
            const double2 qv = slot_stream(q, row[i], n);
            if (SUB) { acc[i].x -= qv.x * h; acc[i].y -= qv.y * h; }
            else { acc[i].x += qv.x * h; acc[i].y += qv.y * h; }
        }
    }
    double ss = 0.0;
#pragma unroll
    for (int i = 0; i < UPT; ++i) {
        slot_store(w, row[i], n, acc[i]);
        ss += acc[i].x * acc[i].x + acc[i].y * acc[i].y;
    }
    if (part) {
        double r = block_sum_256(ss, lds);
        if (threadIdx.x == 0 && blk < gridDim.x) part[blk] = r;  // (the bound always holds; kept: the kernel stays as measured)
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
    const double r = partials_sum_256(part, npart, lds);
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
        double z0, z1, z2, zp;
        jacobi_apply_node(dinv33 + i * 9, dinv1, i, a0, a1, a2, ap, z0, z1, z2, zp);
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
    const double r = partials_sum_256(part + (long long)blockIdx.x * nrb, nrb, lds);
    if (threadIdx.x == 0) {
        const double2 hc = raw_coeff(r, nu[blockIdx.x]);
        d_h[blockIdx.x] = hc.x;
        d_c[blockIdx.x] = hc.y;
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
    if (Z4) jacobi_store_z4(sm, nb, a, dinv33, dinv1, z4);
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

}  // namespace

extern "C" {
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
    if (d_nrm) dfl_reduce_partials(g, work, d_nrm, take_sqrt, stream);
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
    dispatch_z4(z4, [&](auto z) {
        cgs_update_jacobi_kernel<decltype(z)::value><<<g, BLK, 0, S(stream)>>>(N, ncol, Q, ldq, d_c, w, work, dinv33, dinv1, z4, vec_ok);
    });
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
void dfl_gmres_scale_inv(I m, const T* d_nu, T* d_y, void* stream) {
    if (m <= 0) return;
    scale_inv_vec_kernel<<<ceil_div(m, BLK), BLK, 0, S(stream)>>>(m, d_nu, d_y);
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

}  // extern "C"
