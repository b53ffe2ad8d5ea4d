/* dedflow_kernels.h -- thin C ABI of the hand-written gfx950 (MI355X) kernels.
 *
 * Plain pointers and sizes only (no torch / C++ types).  Every pointer is a
 * DEVICE pointer unless the name starts with h_.  `stream` is a hipStream_t
 * passed as void* (NULL = the null stream).  Launchers are asynchronous and
 * never allocate, free or synchronise unless their comment says so; the caller
 * owns every buffer (same ownership rule as the reference).
 *
 * Each entry cites the reference interface it replaces (paths relative to
 * zexxzhao/DEDFlow @ 2024-10-16).  Where the reference called a vendor library
 * from host C (cuBLAS / cuSPARSE / cuRAND / Thrust / CUB) the replacement is a
 * dfl_* launcher here.
 *
 * Native matrix layout ("block CSR"): one nodal pattern (row_ptr[N+1],
 * col_ind[nnz1], sorted ascending per row) shared by all sub-matrices and one
 * 4x4 block of f64 per nodal nonzero, val[k*16 + r*4 + c] with r,c in
 * (u0,u1,u2,p).  It replaces the reference's four row-expanded scalar CSR
 * arrays A00/A01/A10/A11 (src/main.c:385-391, src/csr_impl.cu:24-59); the
 * phi/T rows and columns are not stored, exactly as the reference drops them
 * (NULL sub-matrices, src/matrix_impl.cu:424-426).  dfl_block_export_fs /
 * dfl_block_import_fs convert to/from the reference layout.
 * Global vectors keep the reference layout [u: Nx3 AoS | p: N | phi: N | T: N]
 * (src/main.c:108-118).
 */
#ifndef DEDFLOW_KERNELS_H
#define DEDFLOW_KERNELS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t dfl_index;   /* index_type  = i32 (config/config.mk:51) */
typedef double dfl_value;    /* value_type  = f64 */

/* ---- library / device ------------------------------------------------------- */
int dfl_abi_version(void);
/* last HIP error text seen by a launcher (thread-unsafe, like the reference's CUGUARD printf) */
const char* dfl_last_error(void);

/* ---- BLAS-1 on device vectors (replaces cublasD{axpy,copy,scal,nrm2,dot},
 *      src/krylov.c:114-319, src/main.c:107-130,226,242-265,544-565; VecAXPY etc. src/vec.cu:14-76) */
void dfl_daxpy(dfl_index n, dfl_value alpha, const dfl_value* x, dfl_value* y, void* stream);
void dfl_dscal(dfl_index n, dfl_value alpha, dfl_value* x, void* stream);
void dfl_dcopy(dfl_index n, const dfl_value* x, dfl_value* y, void* stream);
void dfl_dset(dfl_index n, dfl_value alpha, dfl_value* x, void* stream);               /* SetValGPU, matrix_impl.cu:467-471 */
void dfl_pointwise_mult(dfl_index n, const dfl_value* x, const dfl_value* y, dfl_value* z, void* stream); /* VecPointwiseMult */
void dfl_pointwise_div(dfl_index n, const dfl_value* x, const dfl_value* y, dfl_value* z, void* stream);  /* VecPointwiseDiv  */
void dfl_pointwise_inv(dfl_index n, dfl_value* x, void* stream);                                          /* VecPointwiseInv  */
/* halo pack / unpack for element-partitioned runs: out[i] = x[idx[i]];  x[idx[i]] = in[i] (idx unique) */
void dfl_gather_idx(dfl_index n, const dfl_index* idx, const dfl_value* x, dfl_value* out, void* stream);
void dfl_scatter_idx(dfl_index n, const dfl_index* idx, const dfl_value* in, dfl_value* x, void* stream);
/* deterministic two-stage reductions; result written to *d_out (device).  `work`
 * holds at least dfl_reduce_work_size() doubles. */
dfl_index dfl_reduce_work_size(void);
void dfl_ddot(dfl_index n, const dfl_value* x, const dfl_value* y, dfl_value* d_out, dfl_value* work, void* stream);
void dfl_dnrm2(dfl_index n, const dfl_value* x, dfl_value* d_out, dfl_value* work, void* stream);
/* one resident wave for about `us` microseconds (<= 20000; bounded whatever the clock does): a probe for whether two streams
 * of this process run concurrently (host/comm_rccl.c picks its halo stream with it) */
void dfl_spin_us(int us, void* stream);
/* x *= 1 / *d_scale  (cublasDscal with the reciprocal of a device-resident norm, krylov.c:130-131,235-237) */
void dfl_dscal_inv_dev(dfl_index n, const dfl_value* d_scale, dfl_value* x, void* stream);

/* ---- generalized-alpha state algebra of the Newton driver, one pass each (replaces the cublasDaxpy / Dcopy / Dscal /
 *      Dnrm2 sequences of src/main.c:107-130, 242-265, 544-565; vectors are [u: Nx3 | p | phi | T]):
 *  dfl_alpha_states  : dwgalpha = f1_0 dwgold + f1_1 dwg (p slot: dwg), wgalpha = wgold + f2_0 dwgold + f2_1 dwg (p slot: 0);
 *                      nodep != NULL also writes the packed gather records of dfl_pack_nodes from these states and xg
 *  dfl_alpha_predict : dwg *= fac except the p slot;   dfl_alpha_correct: wgold += c0 dwgold + c1 dwg (except p), dwgold = dwg
 *  dfl_norms4        : d_out4[k] = ||F_u||, ||F_p||, ||F_phi||, ||F_T|| (take_sqrt = 0: sums of squares, for partitioned
 *                      runs that all-reduce first); work >= dfl_reduce_work_size() doubles */
void dfl_alpha_states(dfl_index N, const dfl_value* wgold, const dfl_value* dwgold, const dfl_value* dwg, dfl_value f1_0,
                      dfl_value f1_1, dfl_value f2_0, dfl_value f2_1, const dfl_value* xg, dfl_value* wgalpha, dfl_value* dwgalpha,
                      dfl_value* nodep, void* stream);
void dfl_alpha_states2(dfl_index N, const dfl_value* wgold, const dfl_value* dwgold, const dfl_value* dwg, dfl_value f1_0,
                       dfl_value f1_1, dfl_value f2_0, dfl_value f2_1, const dfl_value* xg, dfl_value* wgalpha, dfl_value* dwgalpha,
                       dfl_value* nodep /*or NULL*/, dfl_value* nodexu /*or NULL: compact (x, u) records*/, void* stream);
void dfl_alpha_predict(dfl_index N, dfl_value fac, dfl_value* dwg, void* stream);
void dfl_alpha_correct(dfl_index N, dfl_value c0, dfl_value c1, dfl_value* wgold, dfl_value* dwgold, const dfl_value* dwg, void* stream);
void dfl_norms4(dfl_index N, const dfl_value* F, dfl_value* d_out4, int take_sqrt, dfl_value* work, void* stream);

/* ---- fused classical Gram-Schmidt (replaces the two cublasDgemv of krylov.c:166-183
 *      and the Dnrm2 of :230).
 *   dfl_cgs_dots   : d_h[j] = Q[:,j] . w, j < ncol  (one pass over Q[:,0:ncol] and ~ncol/16 passes over w)
 *   dfl_cgs_update : w -= Q[:,0:ncol] h ; *d_nrm = ||w||_2   (one pass over Q, w read+written once)
 * Q is column-major with leading dimension ldq.  `work` >= dfl_cgs_work_size(n, ncol) doubles (it covers the two-vector
 * forms below, two sets of dots partials and three of update partials, and the blocks of three and four vectors). */
int64_t dfl_cgs_work_size(dfl_index n, dfl_index ncol);
void dfl_cgs_dots(dfl_index n, dfl_index ncol, const dfl_value* Q, int64_t ldq, const dfl_value* w, dfl_value* d_h,
                  dfl_value* work, void* stream);
void dfl_cgs_update(dfl_index n, dfl_index ncol, const dfl_value* Q, int64_t ldq, const dfl_value* d_h, dfl_value* w,
                    dfl_value* d_nrm, int take_sqrt, dfl_value* work, void* stream);
/* dfl_cgs_update (with the square root) followed by the Givens step of column `iter`; the second stage of the norm
 * and the Givens recurrence share one launch (2 launches instead of 3) */
void dfl_cgs_update_givens(dfl_index n, dfl_index ncol, const dfl_value* Q, int64_t ldq, const dfl_value* d_h, dfl_value* w,
                           dfl_value* d_nrm, dfl_value* work, dfl_index iter, dfl_value* d_H, dfl_index ldh, dfl_value* d_gv,
                           dfl_value* d_beta, dfl_value* d_res_hist, void* stream);
/* Raw (unnormalised) basis on one GPU: column j of Q holds r_j = nu_j q_j, d_nu[j] = ||r_j||.
 * dfl_cgs_dots_raw: g_j = Q[:,j].w, then d_h[j] = g_j / nu_j (the entry of H) and d_c[j] = d_h[j] / nu_j (the coefficient of
 *   the raw column in the update); same partial sums and summation order as dfl_cgs_dots.
 * dfl_cgs_update_jacobi_givens: vectors of 4N rows ([u AoS | p]); w -= Q d_c, *d_nrm = ||w||, the Givens step of column
 *   `iter` (as dfl_cgs_update_givens), and -- z4 != NULL -- z4[node][4] = M^-1 w for the block-Jacobi tree (dinv33, dinv1:
 *   dfl_pc_jacobi_setup), written from the update's registers for dfl_bcsr_spmv_x4_scaled.  work: dfl_cgs_work_size(4N, ncol).
 * dfl_gmres_scale_inv: d_y[j] /= d_nu[j], j < m (the triangular-solve result in terms of the raw columns). */
void dfl_cgs_dots_raw(dfl_index n, dfl_index ncol, const dfl_value* Q, int64_t ldq, const dfl_value* w, const dfl_value* d_nu,
                      dfl_value* d_h, dfl_value* d_c, dfl_value* work, void* stream);
void dfl_cgs_update_jacobi_givens(dfl_index N, dfl_index ncol, const dfl_value* Q, int64_t ldq, const dfl_value* d_c, dfl_value* w,
                                  const dfl_value* dinv33, const dfl_value* dinv1, dfl_value* z4, dfl_value* d_nrm, dfl_value* work,
                                  dfl_index iter, dfl_value* d_H, dfl_index ldh, dfl_value* d_gv, dfl_value* d_beta,
                                  dfl_value* d_res_hist, void* stream);
void dfl_gmres_scale_inv(dfl_index m, const dfl_value* d_nu, dfl_value* d_y, void* stream);
/* Two Arnoldi steps per pass over the raw basis: w1 = B v_k, w2 = B w1 (B = A M^-1) against columns 0..ncol-1 = r_0..r_k.
 * dfl_cgs_dots2_raw: one pass over Q for both vectors; d_h1[j] = <r_j, w1> / nu_j (column k of H; d_h1_raw, may be NULL, gets a
 *   copy), d_c1 = d_h1 / nu, d_e[j] = <r_j, w2> / nu_j, d_c2 = d_e / nu.  Fixed summation order; work: dfl_cgs_work_size.
 * dfl_cgs_update2: w1 -= Q d_c1, w2 -= Q d_c2 in one pass; work holds g = dfl_cgs_update2_parts(n) partials each of ||w1'||^2,
 *   <w1', w2'>, ||w2'||^2 at work[0], work[g], work[2g].
 * dfl_gmres_pair_first: second stage of those 3 x npart partials; d_nu[k+1] = nu1 = ||w1'||, d_sc = [<w1',w2'> / nu1^2 (the
 *   coefficient of the fix-up), <w1',w2'> / nu1, ||w2'||^2, nu1], nu1 into row k+1 of column k of d_Hraw (the un-rotated copy of
 *   H, same leading dimension), the Givens step of column k.
 * dfl_cgs_update_jacobi: the update of dfl_cgs_update_jacobi_givens without the norm's second stage and the Givens step; one
 *   partial of ||w'||^2 per block of 256 nodes in work.  With one column and d_c = d_sc it is the fix-up q = w2' - c w1'.
 * dfl_gmres_pair_second: d_nu[k+2] = nu_q = ||q|| from npart partials; column k+1 of H and of d_Hraw from d_e, d_sc and the
 *   earlier columns of d_Hraw; its Givens step; *d_flag (may be NULL) raised when nu_q < 1e-4 ||w2'||.
 * dfl_cgs_update_jacobi_givens_keep: dfl_cgs_update_jacobi_givens that also keeps the un-rotated column (h[0..iter], norm) in
 *   d_raw_col (NULL: none kept). */
int dfl_cgs_update2_parts(dfl_index n);
void dfl_cgs_dots2_raw(dfl_index n, dfl_index ncol, const dfl_value* Q, int64_t ldq, const dfl_value* w1, const dfl_value* w2,
                       const dfl_value* d_nu, dfl_value* d_h1, dfl_value* d_h1_raw, dfl_value* d_c1, dfl_value* d_e, dfl_value* d_c2,
                       dfl_value* work, void* stream);
void dfl_cgs_update2(dfl_index n, dfl_index ncol, const dfl_value* Q, int64_t ldq, const dfl_value* d_c1, const dfl_value* d_c2,
                     dfl_value* w1, dfl_value* w2, dfl_value* work, void* stream);
void dfl_gmres_pair_first(int npart, const dfl_value* part, dfl_index k, dfl_value* d_nu, dfl_value* d_H, dfl_value* d_Hraw,
                          dfl_index ldh, dfl_value* d_gv, dfl_value* d_beta, dfl_value* d_res_hist, dfl_value* d_sc, void* stream);
void dfl_cgs_update_jacobi(dfl_index N, dfl_index ncol, const dfl_value* Q, int64_t ldq, const dfl_value* d_c, dfl_value* w,
                           const dfl_value* dinv33, const dfl_value* dinv1, dfl_value* z4, dfl_value* work, void* stream);
void dfl_gmres_pair_second(int npart, const dfl_value* part, dfl_index k, dfl_value* d_nu, dfl_value* d_H, dfl_value* d_Hraw,
                           dfl_index ldh, const dfl_value* d_e, const dfl_value* d_sc, dfl_value* d_gv, dfl_value* d_beta,
                           dfl_value* d_res_hist, int* d_flag, void* stream);
void dfl_cgs_update_jacobi_givens_keep(dfl_index N, dfl_index ncol, const dfl_value* Q, int64_t ldq, const dfl_value* d_c,
                                       dfl_value* w, const dfl_value* dinv33, const dfl_value* dinv1, dfl_value* z4, dfl_value* d_nrm,
                                       dfl_value* work, dfl_index iter, dfl_value* d_H, dfl_index ldh, dfl_value* d_gv,
                                       dfl_value* d_beta, dfl_value* d_res_hist, dfl_value* d_raw_col, void* stream);
/* Blocks of s = 3 or 4 Arnoldi steps per pass over the raw basis (any other s aborts): the products p_0 = B v_k, p_i = B p_{i-1}
 * lie in s consecutive columns w + i ldw; d_e, d_c hold s vectors of lde doubles; d_sc holds 48 doubles, three 4 x 4 row-major
 * tables: G (the Gram matrix of the updated p_i'), C (unit lower triangular, q_i = sum_{l<=i} C[i,l] p_l'), U[l,i] = <q_l, p_i'>.
 * dfl_cgs_dots_block: one pass over Q; d_e[i lde + j] = <r_j, p_i> / nu_j, d_c = d_e / nu; e_0 also into d_h (column k of H) and
 *   d_h_raw (may be NULL).  work holds s x ncol x dfl_cgs_dots_block_parts(n, s) partials; fixed summation order.
 * dfl_cgs_update_block: p_i -= Q d_c[i] for all i in one pass; work holds g = dfl_cgs_update_block_parts(n, s) partials of each
 *   G_ab, a <= b, the upper triangle in row-major order, at work[t g].
 * dfl_gmres_block_first: second stage of G, d_nu[k+1] = sqrt(G_00) (also row k+1 of column k of d_Hraw), d_sc, the Givens step
 *   of column k.
 * dfl_cgs_fixup_block: q_i in place for i >= 1, vectors of 4N rows; work[(i-1) g + blk] = partials of ||q_i||^2, g = ceil(N / 256);
 *   z4 != NULL: z4 = M^-1 q_{s-1} as dfl_cgs_update_jacobi writes it.
 * dfl_gmres_block_second: d_nu[k+1+i] = ||q_i|| from those partials, columns k+1..k+s-1 of H and d_Hraw with their Givens
 *   steps; *d_flag (may be NULL) raised when some ||q_i|| < 1e-4 sqrt(G_ii). */
int dfl_cgs_dots_block_parts(dfl_index n, int s);
int dfl_cgs_update_block_parts(dfl_index n, int s);
void dfl_cgs_dots_block(dfl_index n, dfl_index ncol, int s, const dfl_value* Q, int64_t ldq, const dfl_value* w, int64_t ldw,
                        const dfl_value* d_nu, dfl_value* d_h, dfl_value* d_h_raw, dfl_value* d_e, dfl_value* d_c, dfl_index lde,
                        dfl_value* work, void* stream);
void dfl_cgs_update_block(dfl_index n, dfl_index ncol, int s, const dfl_value* Q, int64_t ldq, const dfl_value* d_c, dfl_index lde,
                          dfl_value* w, int64_t ldw, dfl_value* work, void* stream);
void dfl_gmres_block_first(int npart, const dfl_value* part, int s, dfl_index k, dfl_value* d_nu, dfl_value* d_H, dfl_value* d_Hraw,
                           dfl_index ldh, dfl_value* d_gv, dfl_value* d_beta, dfl_value* d_res_hist, dfl_value* d_sc, void* stream);
void dfl_cgs_fixup_block(dfl_index N, int s, dfl_value* w, int64_t ldw, const dfl_value* d_sc, const dfl_value* dinv33,
                         const dfl_value* dinv1, dfl_value* z4, dfl_value* work, void* stream);
void dfl_gmres_block_second(int npart, const dfl_value* part, int s, dfl_index k, dfl_value* d_nu, dfl_value* d_H, dfl_value* d_Hraw,
                            dfl_index ldh, const dfl_value* d_e, dfl_index lde, const dfl_value* d_sc, dfl_value* d_gv,
                            dfl_value* d_beta, dfl_value* d_res_hist, int* d_flag, void* stream);
/* The same blocks with the update and the fix-up in one pass (host/gmres.c, GmresPlan.fuse_fixup).  r_j / nu_j are orthonormal, so
 * the Gram matrix of the updated vectors is known before the update: G_ab = <p_a, p_b> - sum_{j<ncol} e_a[j] e_b[j]; C comes from it.
 * d_sc holds 80 doubles here: G, C, U as above, then the derived G at 48 and the raw sums <p_a, p_b> at 64.
 * dfl_cgs_dots_block_gram: dfl_cgs_dots_block (d_h, d_h_raw, d_e, d_c bit for bit) whose pass also sums <p_a, p_b>; work holds the
 *   dots partials, then s (s + 1) / 2 x dfl_cgs_dots_block_parts(n, s) Gram partials; the second stage finishes both kinds of sums
 *   in one launch, and a one-workgroup kernel then writes C, the derived G and the raw sums into d_sc (C by the Gram-Schmidt of
 *   dfl_gmres_block_first).
 * dfl_cgs_update_fixup_block: vectors of 4N rows; p_i -= Q d_c[i], then q_i = sum_{l<=i} C[i,l] p_l' from the registers, every
 *   column stored once, z4 as dfl_cgs_fixup_block; q_i and z4 are those of dfl_cgs_update_block + dfl_cgs_fixup_block bit for bit.
 *   work, g = dfl_cgs_update_fixup_block_parts(N): the partials of the measured G_ab = <p_a', p_b'>, a <= b, at work[t g], then
 *   those of ||q_i||^2 at work[(s (s + 1) / 2 + i - 1) g].
 * dfl_gmres_block_fused: in the place of dfl_gmres_block_first and dfl_gmres_block_second; reads C from d_sc, writes the measured
 *   G and U = C G there, d_nu[k+1..k+s], columns k..k+s-1 of H and d_Hraw with their Givens steps.  The columns are those of
 *   dfl_gmres_block_second with the coordinate of p_i' along v_{k+1+l} taken as (C^-1)[i,l] nu[k+1+l] -- exact for the vectors
 *   formed whatever C is -- where U[l,i] / nu[k+1+l] presumes the q_i orthogonal.  d_flag (may be NULL) points to
 *   two ints: [0] raised when some ||q_i|| < 1e-4 sqrt(G_ii), [1] when some |<q_a, q_b>| = |C[a].G.C[b]| > tau ||q_a|| ||q_b||. */
int dfl_cgs_update_fixup_block_parts(dfl_index N);
void dfl_cgs_dots_block_gram(dfl_index n, dfl_index ncol, int s, const dfl_value* Q, int64_t ldq, const dfl_value* w, int64_t ldw,
                             const dfl_value* d_nu, dfl_value* d_h, dfl_value* d_h_raw, dfl_value* d_e, dfl_value* d_c, dfl_index lde,
                             dfl_value* d_sc, dfl_value* work, void* stream);
void dfl_cgs_update_fixup_block(dfl_index N, dfl_index ncol, int s, const dfl_value* Q, int64_t ldq, const dfl_value* d_c,
                                dfl_index lde, dfl_value* w, int64_t ldw, const dfl_value* d_sc, const dfl_value* dinv33,
                                const dfl_value* dinv1, dfl_value* z4, dfl_value* work, void* stream);
void dfl_gmres_block_fused(int npart, const dfl_value* part, int s, dfl_index k, dfl_value* d_nu, dfl_value* d_H, dfl_value* d_Hraw,
                           dfl_index ldh, const dfl_value* d_e, dfl_index lde, dfl_value* d_sc, dfl_value* d_gv, dfl_value* d_beta,
                           dfl_value* d_res_hist, int* d_flag, dfl_value tau, void* stream);
void dfl_dsqrt_dev(dfl_value* d_val, void* stream); /* *d_val = sqrt(*d_val) */
/* y = Q[:,0:ncol] c  (cublasDgemv OP_N of krylov.c:304-311) */
void dfl_gemv_n(dfl_index n, dfl_index ncol, const dfl_value* Q, int64_t ldq, const dfl_value* d_c, dfl_value* y, void* stream);

/* ---- GMRES small recurrences, device resident (replaces cublasDrot x k, Drotg,
 *      cudaMemset(8B), GMRESResidualUpdatePrivate of krylov.c:256-277, krylov_util.cu:5-19).
 * Column `iter` of H (leading dimension ldh) holds h[0..iter]; *d_nrm = ||w|| becomes h[iter+1].
 * d_res_hist[iter] = |beta[iter+1]|. */
void dfl_gmres_givens(dfl_index iter, const dfl_value* d_nrm, dfl_value* d_H, dfl_index ldh, dfl_value* d_gv,
                      dfl_value* d_beta, dfl_value* d_res_hist, void* stream);
/* same, for partitioned runs: *d_nrm_sq holds the all-reduced squared norm and is replaced by its square root first */
void dfl_gmres_givens_sq(dfl_index iter, dfl_value* d_nrm_sq, dfl_value* d_H, dfl_index ldh, dfl_value* d_gv,
                         dfl_value* d_beta, dfl_value* d_res_hist, void* stream);
/* fused-norm option of partitioned runs: H[0..iter, iter] = all-reduced h, H[iter+1, iter] = all-reduced w.w from the same
 * reduction; the norm of the orthogonalised vector comes from w.w - sum h_j^2 (written to *d_nrm); *d_flag (int, may be
 * NULL) is raised when cancellation leaves less than 1e-6 of w.w */
/* partitioned runs, fused norm + Jacobi tree: w -= Q h, the Pythagorean norm and Givens step of column `iter` (d_hraw =
 * [h_0..h_iter, w.w] all-reduced, copied into H), q = w / nrm in place and z = M^-1 q for the next Arnoldi step: one launch */
void dfl_cgs_update_pc_givens(dfl_index nrows, dfl_index N, dfl_index ncol, const dfl_value* Q, int64_t ldq, const dfl_value* d_hraw,
                              dfl_value* w, const dfl_value* dinv33, const dfl_value* dinv1, dfl_value* z, dfl_index iter,
                              dfl_value* d_H, dfl_index ldh, dfl_value* d_gv, dfl_value* d_beta, dfl_value* d_res_hist,
                              dfl_value* d_nrm, int* d_flag, void* stream);
/* the same, also writing z interleaved into z4[node][4] (owned rows) for dfl_bcsr_spmv_x4; z4 == NULL: as above */
void dfl_cgs_update_pc_givens_x4(dfl_index nrows, dfl_index N, dfl_index ncol, const dfl_value* Q, int64_t ldq, const dfl_value* d_hraw,
                                 dfl_value* w, const dfl_value* dinv33, const dfl_value* dinv1, dfl_value* z, dfl_value* z4,
                                 dfl_index iter, dfl_value* d_H, dfl_index ldh, dfl_value* d_gv, dfl_value* d_beta,
                                 dfl_value* d_res_hist, dfl_value* d_nrm, int* d_flag, void* stream);
void dfl_gmres_givens_pythagoras(dfl_index iter, dfl_value* d_nrm, dfl_value* d_H, dfl_index ldh, dfl_value* d_gv,
                                 dfl_value* d_beta, dfl_value* d_res_hist, int* d_flag, void* stream);
/* back substitution H[0:m,0:m] y = beta[0:m] in place on beta (cublasDtrsv, krylov.c:297-301) */
void dfl_gmres_trsv(dfl_index m, const dfl_value* d_H, dfl_index ldh, dfl_value* d_beta, void* stream);
void GMRESResidualUpdatePrivate(dfl_value* beta, dfl_value* gv); /* same symbol as krylov_util.cu:22-24 */

/* ---- block-CSR SpMV (replaces scal + 4 x cusparseSpMV, src/matrix.c:101-165,471-497):
 *      y[0:4N] = alpha * A * x[0:4N] + beta * y[0:4N] */
void dfl_bcsr_spmv(dfl_index N, const dfl_index* row_ptr, const dfl_index* col_ind, const dfl_value* val, dfl_value alpha,
                   const dfl_value* x, dfl_value beta, dfl_value* y, void* stream);
/* element-partitioned runs: only the first `nrows` node rows (the nodes this rank owns) are
 * computed; x / y keep the local layout with N = owned + ghost nodes */
void dfl_bcsr_spmv_rows(dfl_index nrows, dfl_index N, const dfl_index* row_ptr, const dfl_index* col_ind, const dfl_value* val,
                        dfl_value alpha, const dfl_value* x, dfl_value beta, dfl_value* y, void* stream);
/* node rows [row0, row1) only (interior / boundary split that overlaps the halo exchange with the matvec) */
void dfl_bcsr_spmv_range(dfl_index row0, dfl_index row1, dfl_index N, const dfl_index* row_ptr, const dfl_index* col_ind,
                         const dfl_value* val, dfl_value alpha, const dfl_value* x, dfl_value beta, dfl_value* y, void* stream);
void dfl_pc_jacobi_setup_rows(dfl_index nrows, const dfl_index* row_ptr, const dfl_index* col_ind, const dfl_value* val,
                              dfl_value* dinv33, dfl_value* dinv1, void* stream);
void dfl_pc_jacobi_apply_rows(dfl_index nrows, dfl_index N, dfl_index n, const dfl_value* dinv33, const dfl_value* dinv1,
                              const dfl_value* x, dfl_value* y, void* stream);
void dfl_pc_jacobi_apply_scaled_rows(dfl_index nrows, dfl_index N, dfl_index n, const dfl_value* dinv33, const dfl_value* dinv1,
                                     const dfl_value* w, const dfl_value* d_nrm, dfl_value* q_out, dfl_value* y, void* stream);
/* multicolor block-DILU (csrc/k_dilu.hip): rows[0:nrows_c] = node rows of one color; color[N] u8; Einv[N][16].
 * setup: E_i^-1 of one color (all lower colors already done; columns >= nown (ghosts) are ignored).
 * sweep: one color of the forward (z = E^-1(r - L z)) or backward (z -= E^-1 U z) substitution over rows[slot0 ..
 * slot0+nrows_c); the strictly lower / upper neighbours of the row at slot s are enz / ecol [eptr[s], eptr[s+1])
 * (nodal nonzero index and column node), built once per coloring by the host */
void dfl_dilu_setup_color(dfl_index nrows_c, const dfl_index* rows, dfl_index nown, const dfl_index* row_ptr,
                          const dfl_index* col_ind, const dfl_value* val, const unsigned char* color, dfl_value* Einv, void* stream);
void dfl_dilu_sweep_color(int forward, dfl_index slot0, dfl_index nrows_c, const dfl_index* rows, dfl_index N,
                          const dfl_index* eptr, const dfl_index* enz, const dfl_index* ecol, const dfl_value* val,
                          const dfl_value* Einv, const dfl_value* r, dfl_value* z, void* stream);
void dfl_copy_range(int64_t begin, int64_t end, const dfl_value* x, dfl_value* y, void* stream); /* y[begin:end] = x[begin:end] */
/* scalar CSR SpMV for the reference-layout sub-matrices (cusparseSpMV, matrix.c:151-162) */
void dfl_csr_spmv(dfl_index nrow, const dfl_index* row_ptr, const dfl_index* col_ind, const dfl_value* val, dfl_value alpha,
                  const dfl_value* x, dfl_value beta, dfl_value* y, void* stream);

/* ---- preconditioner (src/pc.c:44-147, src/krylov.c:439-453):
 *  setup : dinv33[9N] = image of inv(D_uu)^T as the reference stores it (row-major extract,
 *          column-major inverse, Q7), dinv1[N] = 1 / A_pp diagonal
 *  apply : y[0:3N] = inv(D)^T x, y[3N:4N] = x * dinv1, y[4N:n] = x (PCNone sections) */
void dfl_pc_jacobi_setup(dfl_index N, const dfl_index* row_ptr, const dfl_index* col_ind, const dfl_value* val,
                         dfl_value* dinv33, dfl_value* dinv1, void* stream);
void dfl_pc_jacobi_apply(dfl_index N, dfl_index n, const dfl_value* dinv33, const dfl_value* dinv1, const dfl_value* x,
                         dfl_value* y, void* stream);
/* same, fused with the normalisation of the incoming Krylov vector:
 *   q = w / *d_nrm (stored to q_out), y = M^{-1} q */
void dfl_pc_jacobi_apply_scaled(dfl_index N, dfl_index n, const dfl_value* dinv33, const dfl_value* dinv1, const dfl_value* w,
                                const dfl_value* d_nrm, dfl_value* q_out, dfl_value* y, void* stream);
/* stand-alone pieces of the same preconditioner (generic PC tree):
 *  dfl_block3_invert : in place, row-major 3x3 blocks -> the reference's post-getri memory image (pc.c:75-77)
 *  dfl_block3_apply  : cublasDgemvStridedBatched(OP_N) on that image (pc.c:104-112) */
void dfl_block3_invert(dfl_index N, dfl_value* diag33, void* stream);
void dfl_block3_apply(dfl_index N, const dfl_value* dinv33, const dfl_value* x, dfl_value* y, void* stream);
/* diagonal extraction with the reference's semantics (matrix_impl.cu:25-44, 642-683) */
void dfl_bcsr_get_diag(dfl_index N, const dfl_index* row_ptr, const dfl_index* col_ind, const dfl_value* val,
                       dfl_value* diag33_rowmajor /*9N or NULL*/, dfl_value* diag_p /*N or NULL*/,
                       dfl_value* diag_u_scalar /*3N or NULL*/, void* stream);

/* ---- layout conversion block CSR <-> reference FS layout (parity tests, export) */
void dfl_block_export_fs(dfl_index N, const dfl_index* row_ptr, const dfl_value* val, dfl_value* A00, dfl_value* A01,
                         dfl_value* A10, dfl_value* A11, void* stream);
void dfl_block_import_fs(dfl_index N, const dfl_index* row_ptr, dfl_value* val, const dfl_value* A00, const dfl_value* A01,
                         const dfl_value* A10, const dfl_value* A11, void* stream);

/* ---- Dirichlet (src/dirichlet_impl.cu:15-36, src/matrix_impl.cu:6-23, src/matrix.c:449-469) */
void ApplyBCVecNodalGPU(dfl_value* b, dfl_index n_bc_node, const dfl_index* bc_node, dfl_index shape, dfl_index init);
void GetRowFromNodeGPU(dfl_index n, dfl_index* row, dfl_index shape, dfl_index init);
void GetNodeFromRowGPU(dfl_index n, dfl_index* node, dfl_index shape);
void dfl_dirichlet_vec(dfl_value* b, dfl_index n_bnode, const dfl_index* bnode, dfl_index shape, dfl_index comp, void* stream);
/* rows (node*3+comp) of the block matrix <- diag * unit row (velocity part), pressure column part <- 0 */
void dfl_bcsr_zero_rows(dfl_index N, const dfl_index* row_ptr, const dfl_index* col_ind, dfl_value* val, dfl_index n_bnode,
                        const dfl_index* bnode, dfl_index comp, dfl_value diag, void* stream);
/* reference-layout launcher, same symbol/signature as matrix_impl.h:10-12 (Q3-safe) */
void MatrixCSRZeroRowGPU(dfl_value* matval, dfl_index num_row, dfl_index num_col, const dfl_index* row_ptr,
                         const dfl_index* col_ind, dfl_index n, const dfl_index* row, dfl_index shift, dfl_value diag);
void MatrixCSRGetDiagGPU(const dfl_value* val, const dfl_index* row_ptr, const dfl_index* col_ind, dfl_value* diag,
                         dfl_index num_row);
void MatrixGetDiagBlockGPU(const dfl_value* matval, dfl_index block_size, dfl_index num_row, dfl_index num_col,
                           const dfl_index* row_ptr, const dfl_index* col_idx, dfl_value* diag_block, int lda, int stride);
void SetValGPU(dfl_value* val, dfl_index n, dfl_value alpha);

/* ---- sparsity pattern (host algorithm in the reference: src/csr.c:81-190; expansion src/csr_impl.cu:24-59) */
/* counts per-row unique neighbours into row_len[N]; *d_overflow != 0 if a row exceeds 64 (csr.c:63 ASSERT) */
void dfl_pattern_count(dfl_index N, const dfl_index* ien, const dfl_index* v2e_row, const dfl_index* v2e_col,
                       dfl_index* row_len, dfl_index* d_overflow, void* stream);
void dfl_pattern_fill(dfl_index N, const dfl_index* ien, const dfl_index* v2e_row, const dfl_index* v2e_col,
                      const dfl_index* row_ptr, dfl_index* col_ind, void* stream);
/* exclusive scan of len[n] into ptr[n+1] (thrust::inclusive_scan, color_impl.cu:35); temp from dfl_scan_temp_bytes */
int64_t dfl_scan_temp_bytes(dfl_index n);
void dfl_exclusive_scan_i32(dfl_index n, const dfl_index* len, dfl_index* ptr, void* temp, int64_t temp_bytes, void* stream);
/* ExpandCSRByBlockSize on raw arrays (csr_impl.cu:126-156), last row_ptr entry written (Q3 fix) */
void dfl_csr_expand(dfl_index N, const dfl_index* row_ptr, const dfl_index* col_ind, dfl_index br, dfl_index bc,
                    dfl_index* new_row_ptr, dfl_index* new_col_ind, void* stream);
/* (elem,a,b) -> nodal nonzero index, replaces the per-thread linear col_ind search of matrix_impl.cu:407-411 */
void dfl_elem_nzmap(dfl_index T, const dfl_index* ien_b, const dfl_index* row_ptr, const dfl_index* col_ind,
                    dfl_index* nzmap_b, void* stream);

/* ---- coloring + batching (src/color_impl.cu:17-255, src/indexing.cu:92-102, src/Mesh.c:165-206) */
void GenerateV2EMapRowTetGPU(const dfl_index* ien, dfl_index num_elem, dfl_index num_node, dfl_index* row_ptr);
void GenerateV2EMapColTetGPU(const dfl_index* ien, dfl_index num_elem, dfl_index num_node, const dfl_index* row_ptr,
                             dfl_index* col_idx);
/* prism (6 vertices) and hex (8) flavours of the same map (color_impl.h:12-16; those element types are otherwise empty
 * in the reference and out of scope here) */
void GenerateV2EMapRowPrismGPU(const dfl_index* ien, dfl_index num_elem, dfl_index num_node, dfl_index* row_ptr);
void GenerateV2EMapColPrismGPU(const dfl_index* ien, dfl_index num_elem, dfl_index num_node, const dfl_index* row_ptr, dfl_index* col_idx);
void GenerateV2EMapRowHexGPU(const dfl_index* ien, dfl_index num_elem, dfl_index num_node, dfl_index* row_ptr);
void GenerateV2EMapColHexGPU(const dfl_index* ien, dfl_index num_elem, dfl_index num_node, const dfl_index* row_ptr, dfl_index* col_idx);
void GenerateRandomColor(dfl_index* color, dfl_index num_elem, dfl_index max_color); /* XORWOW(1234), LEGACY ordering */
void ColorElementJPLTetGPU(const dfl_index* ien, const dfl_index* row_ptr, const dfl_index* col_ind, dfl_index max_color,
                           dfl_index* color, dfl_index num_elem);
void GetMaxColorGPU(const dfl_index* color, dfl_index num_elem, dfl_index* h_max_color);
dfl_index CountValueColorLegacy(const dfl_index* data, dfl_index n, dfl_index value);
void FindValueColor(const dfl_index* data, dfl_index n, dfl_index value, dfl_index* result);
dfl_index CountValueI(const dfl_index* data, dfl_index n, dfl_index value);                      /* indexing.h:9 */
void FindValueI(const dfl_index* data, dfl_index n, dfl_index value, dfl_index* result);          /* indexing.h:10 */
dfl_index CountValueColor(const dfl_index* data, dfl_index n, dfl_index value, void* buffer);     /* indexing.h:13, buffer unused */
/* positions of (row[i], col[i]) in a CSR pattern, -1 if absent (kernel behind CSRAttrGetNZIndBatchedGPU, csr_impl.h:7-9) */
void dfl_csr_find_nz(dfl_index batch_size, const dfl_index* row_ptr, const dfl_index* col_ind, const dfl_index* row,
                     const dfl_index* col, dfl_index* ind, void* stream);
/* pc_impl.h:6-7: point Jacobi on a scalar CSR matrix, y = x / diag(A) (in place: x /= diag(A)) */
void PCJacobiDevice(dfl_index n, dfl_index nnz, dfl_value* data, dfl_index* row_ptr, dfl_index* col_idx, dfl_value* x, dfl_value* y);
void PCJacobiInplaceDevice(dfl_index n, dfl_index nnz, dfl_value* data, dfl_index* row_ptr, dfl_index* col_idx, dfl_value* x);
/* matrix_impl.h:59-64: the reference's colored element-block scatter into the row-expanded sub-matrix arrays (a14).  The
 * assembly kernels of this library scatter directly into the block array and never call it; it is exported for a host that
 * keeps its own element kernels.  matval = DEVICE array of n_offset^2 device pointers (NULL = sub-matrix absent), offset =
 * DEVICE array [n_offset+1]; one batch must be conflict-free (a color), as in the reference. */
void SetBlockValueToSubmatGPU(dfl_value** matval, dfl_value alpha, dfl_index n_offset, const dfl_index* offset, dfl_index nshl,
                              dfl_index batch_size, const dfl_index* batch_index_ptr, const dfl_index* ien, dfl_index num_row,
                              dfl_index num_col, const dfl_index* row_ptr, const dfl_index* col_ind, const dfl_value* val, int lda,
                              int stride, dfl_value beta, const dfl_index* mask);
/* matrix_impl.h:29-62: the single-matrix forms of the same scatter.  (row_ptr, col_ind) is the NODAL pattern; matval is a
 * scalar CSR array (block 1x1) or a row-expanded block_row x block_col array over it (csr_impl.cu:24-59).  The reference's
 * kernels behind these names (matrix_impl.cu:88-208) derive (a, b) from the element id and mix two layouts -- dead code
 * there; implemented here as their call sites describe them.  One batch must be conflict-free. */
void MatrixCSRAddElemValueBatchedGPU(dfl_value* matval, dfl_value alpha, dfl_index batch_size, const dfl_index* batch_index_ptr,
                                     const dfl_index* ien, dfl_index nshl, dfl_index num_row, dfl_index num_col,
                                     const dfl_index* row_ptr, const dfl_index* col_ind, const dfl_value* val, dfl_value beta,
                                     const dfl_index* mask);
void MatrixCSRAddElemValueBlockedBatchedGPU(dfl_value* matval, dfl_value alpha, dfl_index batch_size, const dfl_index* batch_index_ptr,
                                            const dfl_index* ien, dfl_index nshl, dfl_index num_row, dfl_index num_col,
                                            const dfl_index* row_ptr, const dfl_index* col_ind, dfl_index block_row,
                                            dfl_index block_col, const dfl_value* val, int lda, int stride, dfl_value beta,
                                            const dfl_index* mask);
void MatrixCSRAddElementLHSGPU(dfl_value* matval, dfl_index nshl, dfl_index bs, dfl_index num_row, const dfl_index* row_ptr,
                               dfl_index num_col, const dfl_index* col_ind, dfl_index batch_size, const dfl_index* batch_ptr,
                               const dfl_index* ien, const dfl_value* val, int lda);
void MatrixCSRSetValueBatchedGPU(dfl_value* matval, dfl_value alpha, dfl_index csr_num_row, dfl_index csr_num_col,
                                 const dfl_index* csr_row_ptr, const dfl_index* csr_col_ind, dfl_index batch_size,
                                 const dfl_index* batch_row_ind, const dfl_index* batch_col_ind, const dfl_value* A, dfl_value beta);
void MatrixCSRSetValueBlockedBatchedGPU(dfl_value* matval, dfl_value alpha, dfl_index csr_num_row, dfl_index csr_num_col,
                                        const dfl_index* csr_row_ptr, const dfl_index* csr_col_ind, dfl_index batch_size,
                                        const dfl_index* batch_row_ind, const dfl_index* batch_col_ind, dfl_index block_row,
                                        dfl_index block_col, const dfl_value* A, dfl_value beta, int lda, int stride);
/* the same element-block scatter straight into the 4x4 block array (block-mode MatrixFS): rows / columns 0..3 of every
 * lda-strided (a, b) block, block = alpha * block + beta * element block */
void dfl_bcsr_add_elem_blocked(dfl_value* block_val, dfl_value alpha, dfl_index nshl, dfl_index batch_size,
                               const dfl_index* batch_index_ptr, const dfl_index* ien, const dfl_index* row_ptr,
                               const dfl_index* col_ind, const dfl_value* val, int lda, int stride, dfl_value beta,
                               const dfl_index* mask, void* stream);
/* MatrixZeroRow on the block array: row[i] + shift = scalar row node*3 + comp of the velocity block-row; others skipped */
void dfl_bcsr_zero_scalar_rows(dfl_index N, const dfl_index* row_ptr, const dfl_index* col_ind, dfl_value* val, dfl_index n,
                               const dfl_index* row, dfl_index shift, dfl_value diag, void* stream);
/* matrix_impl.h:17-26 (scalar CSR value setters; off the hot path, kept for launcher-level completeness) */
void MatrixCSRSetValuesCOOGPU(dfl_value* matval, dfl_value alpha, dfl_index num_row, dfl_index num_col, const dfl_index* row_ptr,
                              const dfl_index* col_ind, dfl_index n, const dfl_index* row, const dfl_index* col,
                              const dfl_value* val, dfl_value beta);
void MatrixCSRSetValuesIndGPU(dfl_value* matval, dfl_value alpha, dfl_index n, const dfl_index* ind, const dfl_value* val,
                              dfl_value beta);
/* all colors at once: stable counting sort of element ids by color.
 * h_batch_offset[num_color+1] (host), batch_ind[T] (device). Synchronises. */
void dfl_color_batches(const dfl_index* color, dfl_index T, dfl_index num_color, dfl_index* h_batch_offset,
                       dfl_index* batch_ind);
/* ien_b[i*4+a] = ien[batch_ind[i]*4+a] : batch-ordered connectivity for streaming reads */
void dfl_gather_ien(dfl_index T, const dfl_index* ien, const dfl_index* batch_ind, dfl_index* ien_b, void* stream);
/* number of adjacent equal-priority pairs (Q1 diagnostic); synchronises */
dfl_index dfl_count_priority_ties(const dfl_index* ien, dfl_index T, const dfl_index* v2e_row, const dfl_index* v2e_col,
                                  const dfl_index* prio);

/* ---- element assembly, one launch per color batch (src/assemble.cu:1559-1738 chain fused).
 *  ien_b / nzmap_b point at the first element of the batch (batch-ordered arrays).
 *  Node data is gathered from a packed per-node record array (one 128-byte line per node:
 *  x[3] u[3] phi T du[3] p dphi dT pad pad) written once per assembly call by dfl_pack_nodes --
 *  replaces the 8 LoadElementValueKernel launches per batch (assemble.cu:1601-1619,1663-1678).
 *  The RHS kernel accumulates into packed 64-byte residual records (F_u[3] F_p F_phi F_T pad pad);
 *  dfl_unpack_rhs adds them to F in the reference layout and clears the packed buffer. */
void dfl_pack_nodes(dfl_index N, const dfl_value* xg, const dfl_value* wgalpha, const dfl_value* dwgalpha /*or NULL*/,
                    dfl_value* nodep /*[N][16]*/, void* stream);
/* the same, and (nodexu != NULL) the compact records of the Jacobian kernel: nodexu[i][8] = x[3] u[3] pad pad, 64 B per node;
 * nodep == NULL writes the compact records only (and reads only xg and the velocity part of wgalpha) */
void dfl_pack_nodes2(dfl_index N, const dfl_value* xg, const dfl_value* wgalpha, const dfl_value* dwgalpha /*or NULL*/,
                     dfl_value* nodep, dfl_value* nodexu /*or NULL*/, void* stream);
void dfl_unpack_rhs(dfl_index N, dfl_value* Fp /*[N][8], zeroed on return*/, dfl_value* F, void* stream);
/* per-element geometry cache (static mesh): egeo[e*16 + ..] = shape gradients[12], |det J|, sum G_ij^2, 1/tr G, pad;
 * `ien_x` is the connectivity in the order the consuming kernel walks (schedule or patch order) */
void dfl_elem_geometry(dfl_index T, const dfl_index* ien_x, const dfl_value* xg, dfl_value* egeo, void* stream);
void dfl_assemble_tet_lhs(dfl_index batch_size, const dfl_index* ien_b, const dfl_index* nzmap_b, const dfl_value* egeo_b,
                          const dfl_value* nodep, dfl_value* val, void* stream);
void dfl_assemble_tet_rhs(dfl_index batch_size, const dfl_index* ien_b, const dfl_value* nodep, dfl_value* Fp, void* stream);
/* dfl_rhs_node_sum adds, for every node, the 6-component partial records of the patch form of the residual
 * (dfl_assemble_tet_rhs_lane) gidx[goff[n] .. goff[n+1]) in that order into F (reference layout).  No atomics: bitwise
 * reproducible. */
void dfl_rhs_node_sum(dfl_index N, const dfl_index* goff, const dfl_index* gidx, const dfl_value* partial, dfl_value* F,
                      void* stream);
/* slot-owner form (assembly schedule 4, default; host/slotpatch.c, csrc/k_assemble2.hip): workgroup p owns the CSR rows of
 * its node patch; hdr[p] = {tet_off, num_tet | num_node << 16, pos_off, num_pos, group_off, trips_lo, trips_hi, node_off};
 * pnode[node_off + n] = global id of the patch's n-th distinct node (ascending; every node of every tet touching the patch,
 * <= DFL_SLOT_NODES); ptet_lid[tet_off + k] = the four LOCAL node ids (one byte each) of the k-th tet touching the patch;
 * position q of the patch (lane pair q % 128 in pass q / 128) is nodal nonzero slot_nz[pos_off + q] & 0x3fffffff (bit 30 /
 * 31: first / other part of a slot cut into four adjacent positions) and sums the contributions its two lanes find in the
 * lane-major descriptor groups ldesc (layout: host/slotpatch.c), each (local tet << 4) | (a << 2) | b or 0xFFFF.
 * val = beta * val + assembled rows (beta = 0 overwrites).  max_tets = largest num_tet over the patches (sizes the
 * workgroup's LDS: dfl_lhs_slot_lds_bytes).  No atomics: bitwise reproducible. */
#ifndef DFL_SLOT_BLOCK
#define DFL_SLOT_BLOCK 256 /* threads of a slot-owner workgroup: caps a patch at this many tets and DFL_SLOT_BLOCK - 1 slot
                              positions (host/slotpatch.c builds to these caps) */
#define DFL_SLOT_NODES 64  /* distinct nodes of the tets touching a patch: their (x, u) records are staged in LDS, one lane
                              per node (3 x 16 B each, 3 KB) */
#endif
int dfl_lhs_slot_record_bytes(void);
int64_t dfl_lhs_slot_lds_bytes(dfl_index max_tets);
/* nodexu = the compact node records of dfl_pack_nodes2 ([N][8]: x[3] u[3] pad pad) */
void dfl_assemble_tet_lhs_slot(dfl_index npatch, const int32_t* hdr, const uint32_t* ptet_lid, const dfl_index* pnode,
                               const dfl_index* slot_nz, const uint32_t* ldesc, const dfl_value* nodexu, dfl_value* val,
                               dfl_value beta, dfl_index max_tets, void* stream);
/* patch form of the residual (schedule 4, host/patch.c: DflBuildRhsPatchSchedule): the padded layout -- patch p holds tet
 * slots [p*64, ..) of lien (four local node ids per tet, a byte each) and node slots [p*64, ..) of pnode / partial;
 * cnt[p] = num_tets | num_nodes << 16.  One lane per tet; every patch node gets one 6-component partial record, summed in
 * adjacency order.  grid cap > 0 (tests): at most that many workgroups (rounded up to a multiple of 8), so that a small mesh
 * walks the pipelined patch loop. */
void dfl_set_rhs_lane_grid_cap(int workgroups);
/* the adjacency as sub-lists of exactly 4 result slots (256 = zero slot),
 * sub4[p][128][4], and sub_start[p][65] (first sub-list of each patch node; entry num_nodes.. = number of sub-lists) */
void dfl_assemble_tet_rhs_lane(dfl_index npatch, const dfl_index* cnt, const dfl_index* pnode, const unsigned char* lien,
                               const unsigned short* sub4, const unsigned short* sub_start, const dfl_value* nodep,
                               dfl_value* partial, void* stream);
/* weak-BC faces of one color (src/assemble.cu:1764-1964): face list entries index f2e/forn of the group */
void dfl_assemble_face(dfl_index n_face, const dfl_index* face_list, const dfl_index* f2e, const dfl_index* forn,
                       const dfl_index* ien, dfl_index N, const dfl_value* xg, const dfl_value* wgalpha,
                       const dfl_value* dwgalpha, dfl_value* F /*or NULL*/, const dfl_index* row_ptr, const dfl_index* col_ind,
                       dfl_value* val /*or NULL*/, void* stream);
/* two-pass form of the same face terms: every face parks its contributions (pF[f][a][4], pJ[f][a*4+b][16]; NULL = part not
 * wanted), then each touched node / nodal nonzero sums its entries ent[off[k] .. off[k+1]) (= f*4+a resp. f*16+a*4+b) in
 * that order.  One launch for all faces instead of one per conflict-free class; summation order fixed by the lists. */
void dfl_assemble_face_park(dfl_index nf, const dfl_index* f2e, const dfl_index* forn, const dfl_index* ien, dfl_index N,
                            const dfl_value* xg, const dfl_value* wg, const dfl_value* dwg, dfl_value* pF, dfl_value* pJ,
                            void* stream);
void dfl_face_sum_F(dfl_index num_node_entries, const dfl_index* fnode, const dfl_index* off, const dfl_index* ent,
                    const dfl_value* pF, dfl_index N, dfl_value* F, void* stream);
void dfl_face_sum_J(dfl_index num_nz_entries, const dfl_index* fnz, const dfl_index* off, const dfl_index* ent,
                    const dfl_value* pJ, dfl_value* val, void* stream);

/* ---- two-level preconditioner (csrc/k_amg.hip, host/pc_twolevel.c; build-defined): piecewise-constant aggregation.
 *  galerkin   : coarse 4x4 blocks val_coarse[cz] = sum of val_fine[idx[off[cz] .. off[cz+1])] (list order)
 *  restrict_diff   : rc[I] = sum of r - sub over the nodes anode[aoff[I] .. aoff[I+1]) of aggregate I, layouts
 *                    [u: 3N | p: N] (the residual r - A z with sub = A z from a plain matvec)
 *  prolong_add_rows: z[i] += xc[agg[i]] for rows [0, nrows) of N (partitioned runs: the owned nodes come first) */
void dfl_amg_galerkin(dfl_index nnzc, const dfl_index* off, const dfl_index* idx, const dfl_value* val_fine, dfl_value* val_coarse,
                      void* stream);
/* The matvec with x gathered from an INTERLEAVED copy x4[node][4] = (u0 u1 u2 p): the two lanes of a block row fetch their x
 * entries with one 16-byte load each instead of two 8-byte loads from the u part and the p part of the reference layout --
 * one gather instruction and about one L2 request less per nodal nonzero: 0.50 against 0.57 ms at 10M tets (6.95 TB/s),
 * bitwise the same y.  dfl_interleave4 writes the copy for nodes [node0, node1); y rows [row0, row1) = alpha * A x. */
/* the fused Jacobi-tree application (dfl_pc_jacobi_apply[_scaled]_rows; d_nrm == NULL: unscaled, q_out unused) that ALSO
 * writes y interleaved into y4[node][4] for the owned rows -- the matvec that follows needs no interleave pass; y == NULL:
 * only the interleaved copy (n == 4N then: the phi / T tail has nowhere to go) */
void dfl_pc_jacobi_apply_scaled_rows_x4(dfl_index nrows, dfl_index N, dfl_index n, const dfl_value* dinv33, const dfl_value* dinv1,
                                        const dfl_value* w, const dfl_value* d_nrm, dfl_value* q_out, dfl_value* y, dfl_value* y4,
                                        void* stream);
void dfl_interleave4(dfl_index node0, dfl_index node1, dfl_index N, const dfl_value* x, dfl_value* x4, void* stream);
void dfl_bcsr_spmv_x4(dfl_index row0, dfl_index row1, dfl_index N, const dfl_index* row_ptr, const dfl_index* col_ind,
                      const dfl_value* val, dfl_value alpha, const dfl_value* x4, dfl_value* y, void* stream);
/* the same with the output scaled by a device scalar: y = (A x4) * (1.0 / *d_nrm) */
void dfl_bcsr_spmv_x4_scaled(dfl_index row0, dfl_index row1, dfl_index N, const dfl_index* row_ptr, const dfl_index* col_ind,
                             const dfl_value* val, const dfl_value* d_nrm, const dfl_value* x4, dfl_value* y, void* stream);
/* The two products over all N rows with the block-Jacobi tree folded into the store: the row group that forms y_row also writes
 * z4_out[row][4] = M^-1 y_row (of the scaled y in the scaled form), interleaved for the product that follows -- same inverse and
 * same expressions as dfl_pc_jacobi_setup + dfl_pc_jacobi_apply on the row's diagonal block, which the group has just streamed;
 * y as without the fold, bit for bit.  diag_pos[row]: the nonzero holding that block (dfl_bcsr_diag_pos).  z4_out must not be
 * x4: rows of one launch gather x4 of arbitrary other rows.  Return 0, or -1 without a launch (z4_out == x4, or a NULL) */
int dfl_bcsr_spmv_x4_pc(dfl_index N, const dfl_index* row_ptr, const dfl_index* col_ind, const dfl_index* diag_pos,
                        const dfl_value* val, const dfl_value* x4, dfl_value* y, dfl_value* z4_out, void* stream);
int dfl_bcsr_spmv_x4_scaled_pc(dfl_index N, const dfl_index* row_ptr, const dfl_index* col_ind, const dfl_index* diag_pos,
                               const dfl_value* val, const dfl_value* d_nrm, const dfl_value* x4, dfl_value* y, dfl_value* z4_out,
                               void* stream);
/* diag_pos[row] = the nonzero dfl_pc_jacobi_setup inverts for the row (col_ind sorted ascending per row) */
void dfl_bcsr_diag_pos(dfl_index N, const dfl_index* row_ptr, const dfl_index* col_ind, dfl_index* diag_pos, void* stream);
/* single-precision copy of block values (n = nnz1 * 16 entries) and the matvec / DILU sweeps reading it: PC_TWOLEVEL's
 * smoother and residual matvec (a preconditioner under FGMRES may be inexact; everything outside it stays double) */
void dfl_bcsr_values_to_f32(int64_t n, const dfl_value* val, float* valf, void* stream);
void dfl_bcsr_spmv_f32(dfl_index nrows, dfl_index N, const dfl_index* row_ptr, const dfl_index* col_ind, const float* valf,
                       const dfl_value* x, dfl_value* y, void* stream); /* y = A x on rows [0, nrows) */
void dfl_dilu_sweep_color_f32(int forward, dfl_index slot0, dfl_index nrows_c, const dfl_index* rows, dfl_index N,
                              const dfl_index* eptr, const dfl_index* enz, const dfl_index* ecol, const float* valf,
                              const dfl_value* Einv, const dfl_value* r, dfl_value* z, void* stream);
void dfl_amg_restrict_diff(dfl_index Nc, const dfl_index* aoff, const dfl_index* anode, dfl_index N, const dfl_value* r,
                           const dfl_value* sub, dfl_value* rc, void* stream);
void dfl_amg_prolong_add_rows(dfl_index nrows, dfl_index N, const dfl_index* agg, dfl_index Nc, const dfl_value* xc, dfl_value* z,
                              void* stream);

/* ---- PC_AMGX: scalar pairwise-aggregation AMG V-cycle (csrc/k_amgx.hip, host/pc_amgx.c).  One level of the hierarchy as
 * the kernels see it; every pointer is device memory, the structure is built on the host (PCCreateAMGX).
 *   rows[coff[c] .. coff[c+1])   the rows of colour c (greedy colouring in row order)
 *   diag[i]                      position of a_ii;  trans[k] position of a_ji for a_ij = val[k] (-1: not stored)
 *   agg[n] / aoff[nc+1], amem[n] the map to the next level (nc rows) and the members of every next-level row, ascending
 *   goff[nnz+1], gidx            this level's nonzero k = sum of the previous level's val[gidx[goff[k] .. goff[k+1])]
 *   einv                         1/E (DILU) or 1/a_ii (Jacobi); b, x, w: right-hand side, iterate, sweep scratch
 *   lu[n*n], piv[n], zpiv[n]     coarsest level only: the dense LU, its row exchanges, the pivots that count as zero */
typedef struct dfl_amgx_level {
    dfl_index n, nnz, ncolor, nc;
    const dfl_index *rp, *ci, *diag, *trans, *color, *rows, *coff;
    const dfl_index *agg, *aoff, *amem, *goff, *gidx;
    dfl_value *val, *einv, *b, *x, *w;
    dfl_value* lu;
    dfl_index *piv, *zpiv;
} dfl_amgx_level;
/* the (3,3) entry of every 4x4 block: the pressure sub-matrix A11 of the block-mode (u,p) matrix as a compact scalar array */
void dfl_amgx_gather_a11(dfl_index nnz, const dfl_value* block_val, dfl_value* val, void* stream);
/* setup on one grid level: Galerkin sums of level c from the values vf of the level above; DILU E^-1 of the rows of colour
 * `color` = rows[s0 .. s0+cnt) (colours in ascending order, one launch each); Jacobi 1/a_ii */
void dfl_amgx_galerkin(dfl_amgx_level c, const dfl_value* vf, void* stream);
void dfl_amgx_dilu_setup_color(dfl_amgx_level L, dfl_index color, dfl_index s0, dfl_index cnt, void* stream);
void dfl_amgx_jacobi_setup(dfl_amgx_level L, void* stream);
/* one smoothing step x <- x + omega S^-1 (b - A x) on one grid level.  DILU: forward colour kernels (ascending) compute
 * w = (E+L)^-1 (b - A x) with the residual in the same row walk, backward kernels (descending) w = (E+U)^-1 E w and
 * x += omega w.  Jacobi: w = x + omega D^-1 (b - A x) in one launch (the caller swaps x and w).  x_zero: x is zero, not read */
void dfl_amgx_dilu_forward(dfl_amgx_level L, dfl_index color, dfl_index s0, dfl_index cnt, int x_zero, void* stream);
void dfl_amgx_dilu_backward(dfl_amgx_level L, dfl_index color, dfl_index s0, dfl_index cnt, dfl_value omega, int x_zero,
                            void* stream);
void dfl_amgx_jacobi_sweep(dfl_amgx_level L, dfl_value omega, int x_zero, void* stream);
/* c.b = P^T (L.b - L.A L.x) (x_zero: P^T L.b);  L.x (+)= P c.x;  t = r - A z on level L */
void dfl_amgx_restrict(dfl_amgx_level L, dfl_amgx_level c, int x_zero, void* stream);
void dfl_amgx_prolong(dfl_amgx_level L, const dfl_value* xc, int x_zero, void* stream);
void dfl_amgx_residual(dfl_amgx_level L, const dfl_value* r, const dfl_value* z, dfl_value* t, void* stream);
/* the tail: levels [l0, nlev) of the device array `levels` in ONE launch of one 1024-thread workgroup, phases separated by
 * __syncthreads.  tail_setup: Galerkin sums of levels max(l0,1) .. nlev-1, their smoother data, the dense LU of the coarsest.
 * tail_cycle: the V-cycle from level l0 down and back (b0 / x0 / w0 replace level l0's b / x / w) */
void dfl_amgx_tail_setup(const dfl_amgx_level* levels, dfl_index l0, dfl_index nlev, int jacobi, void* stream);
void dfl_amgx_tail_cycle(const dfl_amgx_level* levels, dfl_index l0, dfl_index nlev, int jacobi, int presweeps, int postsweeps,
                         dfl_value omega, const dfl_value* b0, dfl_value* x0, dfl_value* w0, void* stream);

/* ---- shared pieces of the count -> scan -> emit passes and of the two-stage reductions (csrc/k_scan.hip, csrc/block_ops.hpp)
 *    dfl_scan_num_chunks       integers of chunk_sum that dfl_scan_counts needs for n entries: ceil((n + 1) / 1024)
 *    dfl_scan_counts           start[0 .. n] = exclusive scan of count[0 .. n), start[n] = the total, count zeroed; two
 *                              launches on `stream`, nothing allocated or synchronised; returns at once for n < 0
 *    dfl_tets_per_block        tets per workgroup of the one-thread-per-tet passes (redistancing, volume correction, laser
 *                              surface): their blk_count / blk_base hold ceil(T / that) and one more entries
 *    dfl_node_reduce_max_part  the most partials a two-stage node reduction writes per value: `work` of dfl_phase_stats,
 *                              dfl_redistance_node_stats and dfl_volume_node_sum holds that many times their values */
dfl_index dfl_scan_num_chunks(dfl_index n);
void dfl_scan_counts(dfl_index n, dfl_index* count, dfl_index* chunk_sum, dfl_index* start, void* stream);
dfl_index dfl_tets_per_block(void);
dfl_index dfl_node_reduce_max_part(void);

/* ---- DEM contact sweep (build-defined; the reference's Particle.c holds storage only)
 *  model: spheres, linear spring-dashpot normal contact F = (kn*overlap - gamma_n*vn) n between particles and against
 *  the six walls of the unit box or the boundary faces of a tet mesh; uniform cell list with cell edge >= 4R.  Opt-in:
 *  contact friction with rotation, per-particle radius and mass (the blocks below).  The launchers of the sweep
 *  (dfl_dem_build_cells ... dfl_walls_forces) follow the types they take: "DEM contact sweep: launchers" below.
 *    dfl_dem_integrate    v += dt*a ; x += dt*v */
void dfl_dem_integrate(dfl_index P, dfl_value dt, dfl_value* coord, dfl_value* vel, const dfl_value* acc, void* stream);

/* ---- DEM contacts with the boundary faces of a tet mesh (build-defined, csrc/k_walls.hip; model in include/dedflow.h)
 *  dfl_grid3            a uniform grid: cell (i, j, k) = floor((x - lo) * inv) per axis, n cells per axis, x fastest
 *  dfl_wall_tri         one wall triangle in one 128-byte cache line: vertices v[3][3], inward unit normal n, plane offset
 *                       off = n . v0, the mesh node ids of the vertices and the triangle id
 *  DFL_WALL_MAX_CONTACTS distinct wall contacts of one particle at most; the sweep counts the ones beyond */
#ifndef DFL_WALL_MAX_CONTACTS
#define DFL_WALL_MAX_CONTACTS 8
#endif
typedef struct dfl_grid3 {
    dfl_value lo[3], inv[3];
    dfl_index n[3];
} dfl_grid3;
typedef struct dfl_wall_tri {
    dfl_value v[9], n[3], off, pad;
    dfl_index node[3], id;
} dfl_wall_tri;

/* ---- DEM contact friction and rotation (build-defined, opt-in; csrc/dem_friction.hpp, model in include/dedflow.h)
 *  dfl_contact_hist     one history entry (32 B): the contact key and the tangential spring xi
 *  dfl_friction_law     mu, kt, gamma_t (resolved: kt > 0, gamma_t >= 0), the sweep's dt (the springs advance by it) and
 *                       the moment of inertia I = 2/5 m R^2
 *  dfl_contact_history  rows of DFL_DEM_MAX_HISTORY entries per particle id: the previous sweep's rows and live counts
 *                       (read), this sweep's (written; the two alternate between sweeps), *overflow += the contacts of a
 *                       particle that found no free entry
 *    dfl_dem_integrate_spin  v += dt (a + g) ; x += dt v ; omega += dt alpha (omega NULL: no rotation)
 *    dfl_dem_spin            omega += dt alpha */
#ifndef DFL_DEM_MAX_HISTORY
#define DFL_DEM_MAX_HISTORY 16
#endif
typedef struct dfl_contact_hist {
    uint64_t key;
    dfl_value xi[3];
} dfl_contact_hist;
typedef struct dfl_friction_law {
    dfl_value mu, kt, gamma_t, dt, inertia;
} dfl_friction_law;
typedef struct dfl_contact_history {
    const dfl_contact_hist* old_row;
    const dfl_index* old_count;
    dfl_contact_hist* new_row;
    dfl_index* new_count;
    dfl_index* overflow;
} dfl_contact_history;
void dfl_dem_integrate_spin(dfl_index P, dfl_value dt, const dfl_value* g, dfl_value* coord, dfl_value* vel,
                            const dfl_value* acc, dfl_value* omega, const dfl_value* alpha, void* stream);
void dfl_dem_spin(dfl_index P, dfl_value dt, dfl_value* omega, const dfl_value* alpha, void* stream);

/* ---- particle-fluid coupling (build-defined, csrc/k_couple.hip; model in include/dedflow.h)
 *    dfl_couple_sort_v2e      every V2E list ascending (one thread per node)
 *    dfl_couple_neighbours    nbr[4t + k] = tet across the face opposite local vertex k, -1 on the boundary
 *    dfl_couple_locate        walk of every particle from tet[i] (or the seed-grid tet when tet[i] < 0); writes tet[i]
 *                             (-1 outside, -2 walk cap hit: *lost += 1) and lambda[i][4]; `order` (may be NULL) = the
 *                             thread -> particle map.  A tet >= 0 has every lambda >= -1e-12 by comparison (no NaN); tet
 *                             < 0 has lambda 0.  A coordinate that is not finite gives -1, lambda 0 and no lost count
 *    dfl_couple_fluid_step    drag + gravity + integration of every particle; imp[i][3] += drag impulse.  With
 *                             radius_i != NULL (per-particle sizes) d = 2 r_i, rho_p = m_i / (4/3 pi r_i^3) from mass_i /
 *                             radius_i, and the scalars mass and radius are not read
 *    dfl_couple_sort_by_tet   members[tstart[t] .. tstart[t+1]) = the particles in tet t, ascending id; tcount[T] is
 *                             zero-initialised scratch that the call leaves zeroed again
 *    dfl_couple_node_load     load[3a + d] = -scale * sum_{e in V2E(a)} sum_{p in e} lambda_{p,k(a,e)} imp[p][d]
 *    dfl_couple_node_scalar   the same sum of one value per particle: out[a] = -scale * sum lambda_{p,k(a,e)} e[p] */
#define DFL_COUPLE_MAX_WALK 4096
void dfl_couple_sort_v2e(dfl_index N, const dfl_index* vrow, dfl_index* vcol, void* stream);
void dfl_couple_neighbours(dfl_index T, const dfl_index* ien, const dfl_index* vrow, const dfl_index* vcol, dfl_index* nbr,
                           void* stream);
void dfl_couple_locate(dfl_index P, const dfl_index* order, const dfl_value* coord, const dfl_value* xg, const dfl_index* ien,
                       const dfl_index* nbr, const dfl_index* seed, const dfl_value* grid_lo, const dfl_value* grid_inv_h,
                       dfl_index grid_dim, dfl_index* tet, dfl_value* lambda, dfl_index* lost, void* stream);
void dfl_couple_fluid_step(dfl_index P, const dfl_index* order, const dfl_index* tet, const dfl_value* lambda,
                           const dfl_index* ien, const dfl_value* w, dfl_value mass, dfl_value radius, const dfl_value* mass_i,
                           const dfl_value* radius_i, dfl_value rho_f, dfl_value mu_f, const dfl_value* gravity, dfl_value dt,
                           dfl_value* coord, dfl_value* vel, dfl_value* acc, dfl_value* imp, void* stream);
void dfl_couple_sort_by_tet(dfl_index P, dfl_index T, const dfl_index* tet, dfl_index* tcount, dfl_index* rank,
                            dfl_index* tstart, dfl_index* slot, dfl_index* members, void* scan_temp, int64_t scan_temp_bytes,
                            void* stream);
void dfl_couple_node_load(dfl_index N, const dfl_index* vrow, const dfl_index* vcol, const dfl_index* ien,
                          const dfl_index* tstart, const dfl_index* members, const dfl_value* lambda, const dfl_value* imp,
                          dfl_value scale, dfl_value* load, void* stream);
void dfl_couple_node_scalar(dfl_index N, const dfl_index* vrow, const dfl_index* vcol, const dfl_index* ien,
                            const dfl_index* tstart, const dfl_index* members, const dfl_value* lambda, const dfl_value* e,
                            dfl_value scale, dfl_value* out, void* stream);
/* the same sum of five values per particle (the deposits of the melt-pool capture): out[5a + d] = -scale * sum ... dep[p][d] */
void dfl_couple_node_deposit(dfl_index N, const dfl_index* vrow, const dfl_index* vcol, const dfl_index* ien,
                             const dfl_index* tstart, const dfl_index* members, const dfl_value* lambda, const dfl_value* dep,
                             dfl_value scale, dfl_value* out, void* stream);

/* ---- particle inflow and outflow (build-defined, opt-in; csrc/k_flow.hip, model in include/dedflow.h)
 *    dfl_flow_flag          keep[i] = 0 when particle i is beyond a plane (n . x > d) or, by_tet, at tet[i] == -1; else 1.
 *                           rtet (may be NULL; needs tet) = tet[i] of the removed particles, -1 for the kept ones
 *    dfl_flow_compact       stable scatter of every kept particle i to newid[i] (newid = exclusive scan of keep): every
 *                           (src, dst) pair of dfl_flow_fields and, with hrow_src != NULL, the live history entries (partner
 *                           keys remapped through newid, entries of removed partners dropped).  Destinations are distinct
 *                           from every source
 *    dfl_inflow_block       blocked[nu nv] <- 0, then 1 for every slot whose candidate lies closer than 2R to a particle;
 *                           with radius_i != NULL (per-particle sizes) closer than r_y + r_k, r_k = r_lo + (r_hi - r_lo) u_k
 *                           (include/dedflow.h), and the scalar radius is not read
 *    dfl_inflow_select      key_out / slot_out = the slots in ascending (rank key, slot): rank key H(c, k, 2) >> 1, 2^63
 *                           for a blocked slot; temp from dfl_inflow_select_temp_bytes
 *    dfl_inflow_append      the first `want` (<= nu nv) of the sorted slots that are free are appended at ids P, P+1, ...;
 *                           *count <- their number.  hist_count / tet / lambda / imp / omega / alpha may be NULL; with
 *                           radius_i != NULL also radius_i[i] = r_k and mass_i[i] = m0 ((q q) q), q = r_k / r0 */
typedef struct dfl_outflow_planes {
    dfl_value plane[8][4];
    dfl_index num;
} dfl_outflow_planes;
/* what a compaction moves: (src, dst) pairs of per-particle arrays grouped by the bytes of one particle, 4 / 8 / 24 / 32:
 * the pairs of group g are pair[first[g]] .. pair[first[g + 1] - 1]; and the friction history (hrow_src NULL: none) */
#define DFL_FLOW_MAX_FIELDS 16
typedef struct dfl_flow_fields {
    struct {
        const void* src;
        void* dst;
    } pair[DFL_FLOW_MAX_FIELDS];
    int first[5];
    const dfl_contact_hist* hrow_src;
    const dfl_index* hcount_src;
    dfl_contact_hist* hrow_dst;
    dfl_index* hcount_dst;
} dfl_flow_fields;
/* the inlet lattice: the host constants of include/dedflow.h (base, pu, pv, ou, ov), the plane frame (o, unit uhat, vhat,
 * normal) and the prefilter widths of the blocking pass */
typedef struct dfl_inlet {
    dfl_value base[3], pu[3], pv[3], ou[3], ov[3];
    dfl_value o[3], uhat[3], vhat[3], nrm[3];
    dfl_value pitch_u, pitch_v, ju, jv, plane_tol;
    dfl_value vel[3];            /* velocity of an inserted particle */
    dfl_index nu, nv;
    uint64_t seed, call;
} dfl_inlet;
void dfl_flow_flag(dfl_index P, const dfl_value* coord, dfl_outflow_planes planes, const dfl_index* tet, int by_tet,
                   dfl_index* keep, dfl_index* rtet, void* stream);
void dfl_flow_compact(dfl_index P, const dfl_index* keep, const dfl_index* newid, dfl_flow_fields f, void* stream);
void dfl_inflow_block(dfl_index P, const dfl_value* coord, dfl_inlet in, dfl_value radius, const dfl_value* radius_i,
                      dfl_value r_lo, dfl_value r_hi, dfl_index* blocked, void* stream);
int64_t dfl_inflow_select_temp_bytes(dfl_index nslot);
void dfl_inflow_select(dfl_inlet in, const dfl_index* blocked, uint64_t* key, uint64_t* key_out, dfl_index* slot,
                       dfl_index* slot_out, void* temp, int64_t temp_bytes, void* stream);
void dfl_inflow_append(dfl_index P, dfl_index want, dfl_inlet in, const uint64_t* key_sorted, const dfl_index* slot_sorted,
                       int64_t first_tag, dfl_value* coord, dfl_value* vel, dfl_value* acc,
                       int64_t* tag, dfl_value* omega, dfl_value* alpha, dfl_index* hist_count, dfl_index* tet,
                       dfl_value* lambda, dfl_value* imp, dfl_value* radius_i, dfl_value* mass_i, dfl_value r_lo,
                       dfl_value r_hi, dfl_value r0, dfl_value m0, dfl_index* count, void* stream);

/* ---- polydisperse particles (build-defined, opt-in; model in include/dedflow.h, "polydisperse particles")
 *  dfl_sizes            per-particle radius and mass (device [P], by particle id), the radii in the sweep's cell order
 *                       (sorted_r [P], written by the cell sort) and rmax >= every radius (the search range and the grids).
 *  A launcher takes the per-particle arrays as optional arguments: not NULL selects its per-particle-size variant */
typedef struct dfl_sizes {
    const dfl_value* radius;
    const dfl_value* mass;
    const dfl_value* sorted_r;
    dfl_value rmax;
} dfl_sizes;

/* ---- DEM contact sweep: launchers (csrc/k_dem.hip, csrc/k_walls.hip, csrc/dem_sweep.hpp)
 * One sweep is a cell sort and one force kernel, on the unit box (dfl_dem_*) or on a mesh's grid (dfl_walls_*), all on
 * `stream`, with no allocation and no synchronisation.  Optional arguments select the variant:
 *    friction   on when omega (cell sort) / sorted_w (forces) is not NULL; off: sorted_w, law, hist and alpha are not read
 *    sizes      per-particle when radius (cell sort) / sz.sorted_r (forces) is not NULL, and then the scalars radius and
 *               mass are not read; one size: sz is not read (a zeroed dfl_sizes) and every particle has radius, mass
 *    dfl_dem_build_cells    counting sort of the particles by cell (5 launches): cell_start[ncell^3 + 1], order[P] =
 *                           particle ids by (cell, id), and the copies in that order: sorted[P][6] = position and
 *                           velocity, sorted_w[P][3] = omega (friction), sorted_r[P] = radius (sizes).  count[ncell^3 + 1]
 *                           is zero on entry and the call leaves it zeroed again (its last entry is never touched);
 *                           chunk_sum[dfl_scan_num_chunks(ncell^3)], cell_of, rank and slot [P] are plain scratch:
 *                           written before they are read, left with whatever the call put there
 *    dfl_dem_sort_binned    the last four launches of dfl_dem_build_cells, for a bin pass of the caller's over nbin bins
 *    dfl_dem_forces         acc[i] = (sum_j F_ij + F_walls) / m_i, neighbours from the cells within the interaction range;
 *                           with friction also alpha[i] = torque / I_i and the new history rows
 *    dfl_walls_build_cells  dfl_dem_build_cells on `grid`; a particle outside it goes to the extra bin nx*ny*nz (count and
 *                           cell_start then hold nx*ny*nz + 2 entries, chunk_sum dfl_scan_num_chunks(nx*ny*nz + 1))
 *    dfl_walls_forces       dfl_dem_forces for the particles inside `grid` with the mesh's walls, 0 for the others; the
 *                           wall candidates of a particle are wall_list[wall_start[c] .. wall_start[c+1]) of the wall_grid
 *                           cell c holding its centre; *dropped += contacts over DFL_WALL_MAX_CONTACTS; plane[F] = the
 *                           plane id of every wall triangle (include/dedflow.h, contact keys), read with friction only */
void dfl_dem_sort_binned(dfl_index P, dfl_index nbin, const dfl_value* coord, const dfl_value* vel, const dfl_value* omega,
                         const dfl_value* radius, dfl_index* cell_of, dfl_index* rank, dfl_index* count, dfl_index* chunk_sum,
                         dfl_index* cell_start, dfl_index* slot, dfl_index* order, dfl_value* sorted, dfl_value* sorted_w,
                         dfl_value* sorted_r, void* stream);
void dfl_dem_build_cells(dfl_index P, const dfl_value* coord, const dfl_value* vel, const dfl_value* omega,
                         const dfl_value* radius, dfl_value cell, dfl_index ncell, dfl_index* cell_of, dfl_index* rank,
                         dfl_index* count, dfl_index* chunk_sum, dfl_index* cell_start, dfl_index* slot, dfl_index* order,
                         dfl_value* sorted, dfl_value* sorted_w, dfl_value* sorted_r, void* stream);
void dfl_dem_forces(dfl_index P, const dfl_value* sorted, const dfl_value* sorted_w, dfl_value radius, dfl_value mass,
                    dfl_sizes sz, dfl_value kn, dfl_value gamma_n, dfl_friction_law law, dfl_value cell, dfl_index ncell,
                    const dfl_index* order, const dfl_index* cell_start, dfl_contact_history hist, dfl_value* acc,
                    dfl_value* alpha, void* stream);
void dfl_walls_build_cells(dfl_index P, const dfl_value* coord, const dfl_value* vel, const dfl_value* omega,
                           const dfl_value* radius, dfl_grid3 grid, dfl_index* cell_of, dfl_index* rank, dfl_index* count,
                           dfl_index* chunk_sum, dfl_index* cell_start, dfl_index* slot, dfl_index* order, dfl_value* sorted,
                           dfl_value* sorted_w, dfl_value* sorted_r, void* stream);
void dfl_walls_forces(dfl_index P, const dfl_value* sorted, const dfl_value* sorted_w, dfl_value radius, dfl_value mass,
                      dfl_sizes sz, dfl_value kn, dfl_value gamma_n, dfl_friction_law law, dfl_grid3 grid,
                      const dfl_index* order, const dfl_index* cell_start, const dfl_wall_tri* tri, const dfl_index* plane,
                      dfl_grid3 wall_grid, const dfl_index* wall_start, const dfl_index* wall_list, dfl_value tol,
                      dfl_index* dropped, dfl_contact_history hist, dfl_value* acc, dfl_value* alpha, void* stream);

/* ---- particle heat transfer (build-defined, opt-in; csrc/k_heat.hip, model in include/dedflow.h)
 * One thermal sub-step = gather, conduction (when k_p > 0), update; all on `stream`, nothing allocated or synchronised.
 *    dfl_heat_gather           sorted_t[s] = temp[order[s]]: the temperatures in the contact sweep's cell order
 *    dfl_heat_conduction       q[i] = sum_j 2 k_p sqrt(r* delta) (T_j - T_i) over the contacts of the unit-box sweep whose
 *                              cell sort left sorted / order / cell_start (and sz.sorted_r when per-particle sizes)
 *    dfl_heat_conduction_grid  the same over the sweep on a mesh's grid (dfl_walls_build_cells); 0 for a particle outside it
 *    dfl_heat_update           the temperature update of every particle, in id order: convection with the fluid state w
 *                              ([6N], T = w[5N + node]) for a particle with tet[i] >= 0, conduction rate q (may be NULL);
 *                              w or tet NULL: conduction only.  m, r: per-particle mass and radius, or NULL for the scalars.
 *                              pr13 = Pr^(1/3).  Writes temp, rate = C (T' - T) / dt (0 when dt == 0), e += the energy the
 *                              fluid gave.  laser (may be NULL): W absorbed by every particle, added to q; NULL runs the
 *                              kernel without it, the arithmetic of a context that has no laser
 *    dfl_heat_fill             temp = t_init, rate = e = 0 for the particles [first, first + count) */
void dfl_heat_gather(dfl_index P, const dfl_index* order, const dfl_value* temp, dfl_value* sorted_t, void* stream);
void dfl_heat_conduction(dfl_index P, const dfl_value* sorted, dfl_value radius, dfl_sizes sz, dfl_value cell, dfl_index ncell,
                         const dfl_index* order, const dfl_index* cell_start, const dfl_value* sorted_t, dfl_value k_p,
                         dfl_value* q, void* stream);
void dfl_heat_conduction_grid(dfl_index P, const dfl_value* sorted, dfl_value radius, dfl_sizes sz, dfl_grid3 grid,
                              const dfl_index* order, const dfl_index* cell_start, const dfl_value* sorted_t, dfl_value k_p,
                              dfl_value* q, void* stream);
void dfl_heat_update(dfl_index P, const dfl_index* tet, const dfl_value* lambda, const dfl_index* ien, const dfl_value* w,
                     dfl_index N, dfl_value mass, dfl_value radius, const dfl_value* m, const dfl_value* r, const dfl_value* vel,
                     dfl_value cp_p, dfl_value k_f, dfl_value rho_f, dfl_value mu_f, dfl_value pr13, dfl_value dt,
                     const dfl_value* q, const dfl_value* laser, dfl_value* temp, dfl_value* rate, dfl_value* e, void* stream);
void dfl_heat_fill(dfl_index first, dfl_index count, dfl_value t_init, dfl_value* temp, dfl_value* rate, dfl_value* e,
                   void* stream);

/* ---- laser energy deposition (build-defined, opt-in; csrc/k_laser.hip, model in include/dedflow.h)
 * One laser step = hit (substrate only), bin + dfl_dem_sort_binned on the laser's own scratch, columns, deposit, tally; all
 * on `stream`, nothing allocated or synchronised, no floating-point atomics, every output written once.
 *  dfl_laser_beam        the beam of one step: origin o, frame (e1, e2, dir), column edge h, a = h h, n columns per side
 *    dfl_laser_column_cap   entries of a column run the column kernel sorts in LDS; longer runs take its fallback
 *    dfl_laser_bin          cell_of[i] = column of particle i, or n n + (i >> DFL_LASER_OUTSIDE_SHIFT) outside the grid (and
 *                           then rate[i] = 0): n n + ((P - 1) >> DFL_LASER_OUTSIDE_SHIFT) + 1 bins; rank, count as the bin
 *                           pass of dfl_walls_build_cells
 *    dfl_laser_hit          colkey[n n] <- all ones, then per column the minimum over the candidate faces tri[0, nf) whose
 *                           projection holds the column centre (edges and vertices included) of
 *                           floor((depth - s_lo) scale) << 24 | face, the depth field clamped to [0, 2^40 - 1] (nf <= 2^24).
 *                           Two faces whose depths fall into one grid step tie: the lower face index wins, also where it is
 *                           the deeper of the two; so do all depths below s_lo, and all at or beyond s_lo + 2^40 / scale
 *    dfl_laser_columns      per column the run cell_start[c] .. cell_start[c+1] of order / sorted / sorted_r (NULL: every
 *                           particle has `radius`) by (depth, id): rate[id] (+0.0, never -0.0, for a particle deeper than
 *                           the column's hit; one at the hit depth is lit), col_T[c] = transmitted power, col_face[c] = id
 *                           of the hit face's record (-1: none), part[6][n n] = column power, absorbed, scattered,
 *                           substrate, reflected, missed.  gw[2n] = the column weights gx, gy.  k_tau / k_id [P]: scratch
 *                           of runs longer than the cap.  P <= 0: no particles, cell_start is not read
 *    dfl_laser_deposit      per substrate node a in [0, ns) with faces sface[soff[a] .. soff[a+1]) = 4 face + local
 *                           vertex: power[a] = sum over the columns its faces won of eta_s col_T w_vertex;
 *                           energy[a] += dt power[a]
 *    dfl_laser_tally        tally[6] = power - sum column power, and the sums of the other five partials (fixed tree)
 *    dfl_laser_source_add   q[snode[a]] += energy[a] inv_time; energy[a] = 0 */
#define DFL_LASER_OUTSIDE_SHIFT 3
typedef struct dfl_laser_beam {
    dfl_value o[3], e1[3], e2[3], dir[3];
    dfl_value h, area;
    dfl_index n;
} dfl_laser_beam;
dfl_index dfl_laser_column_cap(void);
void dfl_laser_bin(dfl_index P, const dfl_value* coord, dfl_laser_beam b, dfl_index* cell_of, dfl_index* rank, dfl_index* count,
                   dfl_value* rate, void* stream);
void dfl_laser_hit(dfl_index nf, const dfl_wall_tri* tri, dfl_laser_beam b, dfl_value s_lo, dfl_value scale, uint64_t* colkey,
                   void* stream);
void dfl_laser_columns(dfl_index P, dfl_laser_beam b, dfl_value power, dfl_value eta_p, dfl_value eta_s, const dfl_value* gw,
                       const dfl_index* cell_start, const dfl_index* order, const dfl_value* sorted, const dfl_value* sorted_r,
                       dfl_value radius, const dfl_wall_tri* tri, const uint64_t* colkey, dfl_value* k_tau, dfl_index* k_id,
                       dfl_value* rate, dfl_value* col_T, dfl_index* col_face, dfl_value* part, void* stream);
void dfl_laser_deposit(dfl_index ns, const dfl_index* soff, const dfl_index* sface, const dfl_wall_tri* tri, dfl_laser_beam b,
                       dfl_value eta_s, dfl_value dt, const uint64_t* colkey, const dfl_value* col_T, dfl_value* power,
                       dfl_value* energy, void* stream);
void dfl_laser_tally(dfl_index ncol, dfl_value power, const dfl_value* part, dfl_value* tally, void* stream);
void dfl_laser_source_add(dfl_index ns, const dfl_index* snode, dfl_value inv_time, dfl_value* energy, dfl_value* q,
                          void* stream);

/* ---- the laser on the level-set surface (build-defined, opt-in; csrc/k_laser_surface.hip, model in include/dedflow.h)
 * Snapshot: count -> dfl_scan_counts of the workgroup counts -> emit -> nodes.  Deposit: once per laser step.  All on
 * `stream`; nothing allocated or synchronised; no floating-point atomics; no atomic decides an order.
 *    dfl_laser_surface_count       blk_count[b] = candidate facets of the tets of workgroup b (dfl_tets_per_block()
 *                                  tets each): the facets of lf_tet_facets with side (g . dir) > 0, |g| > 0 and nine finite
 *                                  coordinates.  phi = w + 4N; dir: three host doubles, the normalised beam direction
 *    dfl_laser_surface_emit        facet f = blk_base[b] + (candidates of the earlier tets of workgroup b), f < cap:
 *                                  facets[f][9], tet[f], t[f][3], ij[f] = per vertex v the edge i | j << 2 in bits
 *                                  [4 v, 4 v + 4), and cand[f] = the facet as a wall record with id = -2 - tet (the caller
 *                                  passes the candidate list offset by the boundary records in front)
 *    dfl_laser_surface_nodes       the distinct nodes of the facets' tets: unode[0 .. nu) ascending, nu = start[4 nfs], and
 *                                  fslot[4 f + a] = the index in unode of local node a of facet f's tet.  key, key_out, rec,
 *                                  rec_out, flag: [4 nfs]; start: [4 nfs + 1]; chunk_sum as dfl_scan_counts needs for
 *                                  4 nfs entries; temp: dfl_laser_surface_temp_bytes(4 nfs, .) bytes
 *    dfl_laser_surface_deposit     power[0 .. 4 nfs) <- 0; then per slot the sum, from +0.0 in ascending column id, of
 *                                  (eta_s col_T[c]) lambda_a over the columns c whose hit key names a facet (index >= nfb in
 *                                  cand, the whole candidate list): power[slot], energy[slot] += dt power[slot].  key,
 *                                  key_out, val: [4 n n]; temp: dfl_laser_surface_temp_bytes(., 4 n n) bytes
 *    dfl_laser_surface_source_add  q[unode[a]] += energy[a] inv_time, energy[a] = 0, a < min(nmax, *nu)
 *    dfl_laser_surface_power       q[0 .. N) <- 0, then q[unode[a]] = power[a]
 *    dfl_laser_surface_carry       carry[unode[a]] += energy[a], energy[a] = 0 (carry dense, [N])
 *    dfl_laser_surface_carry_add   q[n] += carry[n] inv_time, carry[n] = 0, n < N */
int64_t dfl_laser_surface_temp_bytes(dfl_index n_node_keys, dfl_index n_records);
void dfl_laser_surface_count(dfl_index T, const dfl_index* ien, const dfl_value* xg, const dfl_value* w, dfl_index N, dfl_value level,
                             dfl_index side, const dfl_value* dir, dfl_index* blk_count, void* stream);
void dfl_laser_surface_emit(dfl_index T, const dfl_index* ien, const dfl_value* xg, const dfl_value* w, dfl_index N, dfl_value level,
                            dfl_index side, const dfl_value* dir, const dfl_index* blk_base, dfl_wall_tri* cand, dfl_value* facets,
                            dfl_index* tet, dfl_index* ij, dfl_value* t, dfl_index cap, void* stream);
void dfl_laser_surface_nodes(dfl_index nfs, const dfl_index* ien, const dfl_index* tet, uint32_t* key, uint32_t* key_out,
                             dfl_index* rec, dfl_index* rec_out, dfl_index* flag, dfl_index* chunk_sum, dfl_index* start,
                             dfl_index* fslot, dfl_index* unode, void* temp, int64_t temp_bytes, void* stream);
void dfl_laser_surface_deposit(dfl_laser_beam b, const uint64_t* colkey, dfl_index nfb, dfl_index nfs, const dfl_wall_tri* cand,
                               const dfl_index* ij, const dfl_value* t, const dfl_index* fslot, dfl_value eta_s, dfl_value dt,
                               const dfl_value* col_T, uint64_t* key, uint64_t* key_out, dfl_value* val, dfl_value* power,
                               dfl_value* energy, void* temp, int64_t temp_bytes, void* stream);
void dfl_laser_surface_source_add(dfl_index nmax, const dfl_index* nu, const dfl_index* unode, dfl_value inv_time, dfl_value* energy,
                                  dfl_value* q, void* stream);
void dfl_laser_surface_power(dfl_index N, dfl_index nmax, const dfl_index* nu, const dfl_index* unode, const dfl_value* power,
                             dfl_value* q, void* stream);
void dfl_laser_surface_carry(dfl_index nmax, const dfl_index* nu, const dfl_index* unode, dfl_value* energy, dfl_value* carry,
                             void* stream);
void dfl_laser_surface_carry_add(dfl_index N, dfl_value inv_time, dfl_value* carry, dfl_value* q, void* stream);

/* ---- laser reflections (build-defined, opt-in; csrc/k_laser_reflect.hip, model in include/dedflow.h "laser reflections")
 * Reflection list R: count -> dfl_scan_counts of the workgroup counts -> emit; its node slots are dfl_laser_surface_nodes on
 * R's tets.  One laser step: trace -> deposit -> tally.  All on `stream`, no synchronisation.
 *    dfl_laser_reflect_count    blk_count[b] = facets of R in the tets of workgroup b (dfl_tets_per_block() tets each)
 *    dfl_laser_reflect_emit     facet f = blk_base[b] + (facets of the earlier tets of workgroup b), f < cap: facets [.][9],
 *                               tet [.], grad [.][3] (the tet's gradient), ij [.], t [.][3] as dfl_laser_surface_emit
 *    dfl_laser_reflect_trace    one wave per column c < n n.  colkey, nfb, nfs, cand as the surface deposit sees them, ftet
 *                               [nfs] the candidates' tets; R = (nr, facets, rtet, rgrad).  Writes, for every b <=
 *                               max_bounce (1 .. 8), hit_facet[b n n + c] (index into R, -1), hit_abs[.], hit_w[.][3];
 *                               ray_end[c] = escaped, ray_end[n n + c] = remaining; and, for a column that starts a ray,
 *                               part[3 n n + c] = its absorbed sum, part[4 n n + c] = escaped + remaining (part: the
 *                               [6][n n] tally partials of dfl_laser_columns)
 *    dfl_laser_reflect_deposit  power[0 .. 4 nr) <- 0; then per slot the sum, from +0.0 in ascending (b n n + c) 4 + a, of
 *                               hit_abs lambda_a; energy[slot] += dt power[slot] for the slots with a record.  nrec =
 *                               (max_bounce + 1) n n; key, key_out, val: [4 nrec]; temp: dfl_laser_reflect_temp_bytes(4 nrec)
 *    dfl_laser_reflect_tally    out[0 .. 9) absorbed per bounce, out[9] escaped, out[10] remaining, out[11 .. 20) rays per
 *                               bounce as doubles; one workgroup, a fixed tree */
int64_t dfl_laser_reflect_temp_bytes(dfl_index n_records);
void dfl_laser_reflect_count(dfl_index T, const dfl_index* ien, const dfl_value* xg, const dfl_value* w, dfl_index N, dfl_value level,
                             dfl_index* blk_count, void* stream);
void dfl_laser_reflect_emit(dfl_index T, const dfl_index* ien, const dfl_value* xg, const dfl_value* w, dfl_index N, dfl_value level,
                            const dfl_index* blk_base, dfl_value* facets, dfl_index* tet, dfl_value* grad, dfl_index* ij, dfl_value* t,
                            dfl_index cap, void* stream);
void dfl_laser_reflect_trace(dfl_laser_beam b, const uint64_t* colkey, dfl_index nfb, dfl_index nfs, const dfl_wall_tri* cand,
                             const dfl_index* ftet, dfl_index nr, const dfl_value* facets, const dfl_index* rtet, const dfl_value* rgrad,
                             dfl_index side, dfl_index model, dfl_index max_bounce, dfl_value eta_s, dfl_value eps,
                             const dfl_value* col_T, dfl_index* hit_facet, dfl_value* hit_abs, dfl_value* hit_w, dfl_value* ray_end,
                             dfl_value* part, void* stream);
/*    dfl_laser_reflect_cells_count / _emit   the uniform grid `grid` (dfl_grid3: lo, cells per unit length inv, n per axis) over R:
 *                               count[cell] += 1, then entry[start[cell] + arrival] = facet, for every cell that the box of
 *                               a facet's vertices overlaps (coordinates clamped into the grid).  count / cursor: [cells],
 *                               zero on entry; start: the exclusive scan of count, [cells + 1]; entry: [cap], clipped
 *    dfl_laser_reflect_trace_grid   dfl_laser_reflect_trace through the cells (cell_start NULL: over all of R); group = 16 or
 *                               64 lanes per ray; visited (or NULL): [n n] entries tested per column, all bounces.  The
 *                               result has the bits of dfl_laser_reflect_trace where the grid's box holds the hit points
 *                               (Update's is the node bounding box, which holds every facet); a facet beyond the box sits in
 *                               the boundary cells and is found only where the ray's rectangle in the last layer holds it */
void dfl_laser_reflect_cells_count(dfl_index nr, const dfl_value* facets, dfl_grid3 grid, dfl_index* count, void* stream);
void dfl_laser_reflect_cells_emit(dfl_index nr, const dfl_value* facets, dfl_grid3 grid, const dfl_index* start, dfl_index* cursor,
                                  dfl_index* entry, dfl_index cap, void* stream);
void dfl_laser_reflect_trace_grid(dfl_laser_beam b, const uint64_t* colkey, dfl_index nfb, dfl_index nfs, const dfl_wall_tri* cand,
                                  const dfl_index* ftet, dfl_index nr, const dfl_value* facets, const dfl_index* rtet,
                                  const dfl_value* rgrad, dfl_index side, dfl_index model, dfl_index max_bounce, dfl_value eta_s,
                                  dfl_value eps, const dfl_value* col_T, dfl_index* hit_facet, dfl_value* hit_abs, dfl_value* hit_w,
                                  dfl_value* ray_end, dfl_value* part, dfl_grid3 grid, const dfl_index* cell_start,
                                  const dfl_index* cell_entry, dfl_index group, dfl_value* visited, void* stream);
void dfl_laser_reflect_deposit(dfl_index nrec, const dfl_index* hit_facet, const dfl_value* hit_abs, const dfl_value* hit_w, dfl_index nr,
                               const dfl_index* ij, const dfl_value* t, const dfl_index* fslot, dfl_value dt, uint64_t* key,
                               uint64_t* key_out, dfl_value* val, dfl_value* power, dfl_value* energy, void* temp, int64_t temp_bytes,
                               void* stream);
void dfl_laser_reflect_tally(dfl_index ncol, dfl_index max_bounce, const dfl_index* hit_facet, const dfl_value* hit_abs,
                             const dfl_value* ray_end, dfl_value* out, void* stream);

/* ---- melt-pool capture (build-defined, opt-in; csrc/k_capture.hip, model in include/dedflow.h)
 *    dfl_capture_flag       one thread per particle: the decision of include/dedflow.h from tet / lambda (of a locate just
 *                           run), the node coordinates xg and the fluid state w [6N].  keep[i] = 0 when captured, else 1;
 *                           rtet[i] = the tet of a captured particle, else -1; dep[5i ..] = (V, dP0, dP1, dP2, E) of a
 *                           captured particle, zeros otherwise.  mass_i / radius_i NULL: the scalars.  temp NULL (heat
 *                           off): E = 0.  No LDS, no atomics
 *    dfl_capture_source     q_vol[a] = A[5a] / time, load[3a + d] = A[5a + 1 + d] / time, q_heat[a] = A[5a + 4] / time; any
 *                           of the three may be NULL */
void dfl_capture_flag(dfl_index P, const dfl_index* tet, const dfl_value* lambda, const dfl_index* ien, const dfl_value* xg,
                      const dfl_value* w, dfl_index N, const dfl_value* vel, const dfl_value* temp, dfl_value mass,
                      dfl_value radius, const dfl_value* mass_i, const dfl_value* radius_i, dfl_value rho_f, dfl_value cp_p,
                      dfl_value level, dfl_value side, dfl_value reach, dfl_value T_melt, dfl_index* keep, dfl_index* rtet,
                      dfl_value* dep, void* stream);
void dfl_capture_source(dfl_index N, const dfl_value* A, dfl_value time, dfl_value* q_vol, dfl_value* load, dfl_value* q_heat,
                        void* stream);

/* ---- solid-surface contact (build-defined, opt-in; csrc/k_surface_contact.hip, model in include/dedflow.h)
 *  dfl_surface_counters  step[k]: the counts of the last sub-step of parity k, in contact in the low and buried in the high 32
 *                        bits, spread over DFL_SURFACE_SLOTS slots of one cache line each (a workgroup adds to slot
 *                        blockIdx mod DFL_SURFACE_SLOTS; their sum is the count); total: the contacts of every earlier sub-step
 *    dfl_surface_grad_max   one thread per tet: *grad_max = max over the tets and k = 1, 2, 3 of |c_k| / |det| (the |grad N_k|
 *                           of the closed form of g, from the same device function the contact divides by); +inf or a NaN
 *                           when a tet is degenerate or a coordinate is not finite, which turns the early exit off.  A
 *                           memset and one launch
 *    dfl_surface_contact    one launch, one thread per particle (one workgroup when P = 0): the contact of include/dedflow.h
 *                           from tet / lambda of the locate just run, xg, the fluid state w [6N], vel and omega; acc, alpha
 *                           and the history row of a particle in contact are added to / appended to, no other particle is
 *                           written.  Variants: friction when omega is not NULL (hist = previous rows and the rows this
 *                           sub-step's sweep wrote with their counts; off: omega, law, hist and alpha are not read), sizes per
 *                           particle when sz.radius is not NULL (then the scalars are not read).  grad_max: device [1], what
 *                           dfl_surface_grad_max wrote for this mesh; it lets a particle far on the gas side leave before T and
 *                           the coordinates are gathered, and the result does not depend on it (a value that is not > 0 lets nothing leave early).  cur (0 or 1) alternates between launches: the launch adds to cnt->step[cur], and
 *                           folds step[1 - cur] into total and clears it.  No allocation, no synchronisation */
#define DFL_SURFACE_SLOTS 64
#define DFL_SURFACE_SLOT_STRIDE 16
typedef struct dfl_surface_counters {
    unsigned long long step[2][DFL_SURFACE_SLOTS * DFL_SURFACE_SLOT_STRIDE];
    long long total;
} dfl_surface_counters;
void dfl_surface_grad_max(dfl_index T, const dfl_index* ien, const dfl_value* xg, dfl_value* grad_max, void* stream);
void dfl_surface_contact(dfl_index P, const dfl_index* tet, const dfl_value* lambda, const dfl_index* ien, const dfl_value* xg,
                         const dfl_value* w, dfl_index N, const dfl_value* vel, const dfl_value* omega, dfl_value mass,
                         dfl_value radius, dfl_sizes sz, dfl_value kn, dfl_value gamma_n, dfl_friction_law law, dfl_value level,
                         dfl_value side, dfl_value T_solid, const dfl_value* grad_max, dfl_contact_history hist,
                         dfl_surface_counters* cnt, int cur, dfl_value* acc, dfl_value* alpha, void* stream);

/* ---- scalar transport (host/scalar.c, csrc/k_scalar.hip) ------------------------------------------------------------
 * dfl_assemble_scalar_jacobian: the level-set and temperature Jacobians (d R_phi / d dphi, d R_T / d dT) over the nodal
 * pattern (row_ptr / col_ind, columns ascending), one value per nonzero, overwritten (beta = 0).  vrow / vcol: the V2E map
 * of the tets with every list ascending; wgalpha: the alpha-level state (only u = wgalpha[0, 3N) is read).  Either value
 * array may be NULL.  One launch, no atomics: bitwise reproducible. */
void dfl_assemble_scalar_jacobian(dfl_index N, const dfl_index* vrow, const dfl_index* vcol, const dfl_index* ien,
                                  const dfl_value* xg, const dfl_value* wgalpha, const dfl_index* row_ptr,
                                  const dfl_index* col_ind, dfl_value* val_phi, dfl_value* val_T, void* stream);

/* ---- free-surface forces (build-defined, opt-in; host/surface.c, csrc/k_surface.hip, model in include/dedflow.h)
 *    dfl_surface_load    the node sums load [3N], q_heat [N], area [N] (any of them NULL: not written; the others overwritten
 *                        in full) of the smeared-interface terms at the state w [6N].  vrow / vcol: the V2E map of the tets
 *                        with every list ascending.  A group of 16 lanes per node walks the node's list, a lane
 *                        per tet; a lane whose tet lies outside the band leaves, the others evaluate their own node's share,
 *                        and the group adds the shares in list order through LDS.  No atomics: bitwise reproducible.
 *                        flag NULL: every lane gathers its tet's ien line, phi and coordinates for the band test;
 *                        flag [T] (dfl_surface_flag_tets just run on the same w): lanes of tets with flag 0 leave after one
 *                        byte.  Both give the same bits: the flag is the same test run by the same code.
 *    dfl_surface_flag_tets  one thread per tet: flag[e] = 1 when the tet passes the |g| > 0 and the band test, else 0 */
typedef struct dfl_surface_params {
    dfl_value level, side, eps;
    dfl_value sigma0, dsigma_dT, T_ref;
    dfl_value recoil_p0, recoil_a, T_boil;
    dfl_value h_conv, emissivity, T_amb, evap_q0;
} dfl_surface_params;
void dfl_surface_flag_tets(dfl_index T, const dfl_index* ien, const dfl_value* xg, const dfl_value* w, dfl_index N,
                           const dfl_surface_params* prm, unsigned char* flag, void* stream);
void dfl_surface_load(dfl_index N, const dfl_index* vrow, const dfl_index* vcol, const dfl_index* ien, const dfl_value* xg,
                      const dfl_value* w, const dfl_surface_params* prm, const unsigned char* flag, dfl_value* load,
                      dfl_value* q_heat, dfl_value* area, void* stream);

/* ---- phase change (build-defined, opt-in; host/phase.c, csrc/k_phase.hip, model in include/dedflow.h)
 *    dfl_phase_coefficients  the node sums D [N] (kg/s), H [N] (J/K), G [N] (m^3) at the state w [6N]; any of them NULL: not
 *                            written, the others overwritten in full.  vrow / vcol: the V2E map of the tets with every list
 *                            ascending.  A group of 16 lanes per node walks the node's list, a lane per tet; a lane whose
 *                            tet the skip rules drop leaves, the others evaluate their own node's share, and the group adds
 *                            the shares in list order through LDS.  No atomics: bitwise reproducible.  flag NULL: every lane
 *                            gathers its tet and applies the skip rules itself; flag [T] (dfl_phase_flag_tets just run on
 *                            the same w): a lane whose byte is 0 leaves after that byte.  Both give the same bits.
 *    dfl_phase_flag_tets     one thread per tet: bit 0 = the tet adds to D / H, bit 1 = it adds to G
 *    dfl_phase_apply_F       F[3a + d] += D[a] wgalpha[3a + d], F[5N + a] += H[a] dwgalpha[5N + a] (D or H NULL: that part
 *                            is left out); products rounded before the add
 *    dfl_phase_apply_J       val[16 k + 5 d] += fact2 D[a], d < 3, k the position of column a in row a of the nodal pattern
 *    dfl_phase_apply_JT      val[k] += alpham H[a] on the same diagonal of a scalar CSR matrix over the nodal pattern
 *    dfl_phase_stats         out9 = (sum G in a fixed two-stage order, T_max over metal nodes, number of molten nodes, lo[3],
 *                            hi[3] of their coordinates); work >= dfl_phase_stats_work_size() doubles
 * Every launcher returns at once for n <= 0. */
typedef struct dfl_phase_params {
    dfl_value T_solidus, T_liquidus, latent, darcy_c, darcy_b;
    dfl_value level, side, eps;
    int use_phi;
} dfl_phase_params;
void dfl_phase_flag_tets(dfl_index T, const dfl_index* ien, const dfl_value* xg, const dfl_value* w, dfl_index N,
                         const dfl_phase_params* prm, unsigned char* flag, void* stream);
void dfl_phase_coefficients(dfl_index N, const dfl_index* vrow, const dfl_index* vcol, const dfl_index* ien, const dfl_value* xg,
                            const dfl_value* w, const dfl_phase_params* prm, const unsigned char* flag, dfl_value* D,
                            dfl_value* H, dfl_value* G, void* stream);
void dfl_phase_apply_F(dfl_index N, const dfl_value* D, const dfl_value* H, const dfl_value* wgalpha, const dfl_value* dwgalpha,
                       dfl_value* F, void* stream);
void dfl_phase_apply_J(dfl_index N, const dfl_index* row_ptr, const dfl_index* col_ind, const dfl_value* D, dfl_value fact2,
                       dfl_value* val, void* stream);
void dfl_phase_apply_JT(dfl_index N, const dfl_index* row_ptr, const dfl_index* col_ind, const dfl_value* H, dfl_value alpham,
                        dfl_value* val, void* stream);
dfl_index dfl_phase_stats_work_size(void);
void dfl_phase_stats(dfl_index N, const dfl_value* xg, const dfl_value* w, const dfl_value* G, const dfl_phase_params* prm,
                     dfl_value* work, dfl_value* out9, void* stream);

/* ---- thermal material (build-defined, opt-in; host/thermal.c, csrc/k_thermal.hip, csrc/k_scalar.hip, model in include/dedflow.h)
 *    dfl_thermal_rows        the node sums r [N] (W), Kn [N] (W m / K), Cn [N] (J / K) at the states w, dw [6N] (taken as the
 *                            alpha states); any of them NULL: not written, the others overwritten in full.  vrow / vcol: the
 *                            V2E map of the tets with every list ascending.  The node gather of the phase-change pass: a lane
 *                            per (node, tet), the shares added in list order through LDS, no atomics, bitwise reproducible.
 *                            r alone: a tet whose dk_q and dc_q are all exactly 0 leaves early; its share of r is +0.0 in
 *                            either case.
 *    dfl_thermal_add_rows    the same r, added by its owner lane to FT[a] (the T rows F + 5N of an assembly): FT[a] += r[a],
 *                            r[a] summed and rounded first.  One launch, no buffer.
 *    dfl_assemble_scalar_jacobian_material   dfl_assemble_scalar_jacobian with the entries jm of the section added to every
 *                            tet's T entries before they are summed (the base entry is rounded first); val_phi gets the bits of
 *                            the plain launcher.  wgalpha: u, phi and T are read.
 * Every launcher returns at once for N <= 0. */
typedef struct dfl_thermal_params {
    dfl_value k_gas, k_solid, k_liquid, c_gas, c_metal;
    dfl_value T_solidus, T_liquidus;
    dfl_value level, side, eps;
    int use_phi;
} dfl_thermal_params;
void dfl_thermal_rows(dfl_index N, const dfl_index* vrow, const dfl_index* vcol, const dfl_index* ien, const dfl_value* xg,
                      const dfl_value* w, const dfl_value* dw, const dfl_thermal_params* prm, dfl_value* r, dfl_value* Kn,
                      dfl_value* Cn, void* stream);
void dfl_thermal_add_rows(dfl_index N, const dfl_index* vrow, const dfl_index* vcol, const dfl_index* ien, const dfl_value* xg,
                          const dfl_value* wgalpha, const dfl_value* dwgalpha, const dfl_thermal_params* prm, dfl_value* FT,
                          void* stream);
void dfl_assemble_scalar_jacobian_material(dfl_index N, const dfl_index* vrow, const dfl_index* vcol, const dfl_index* ien,
                                           const dfl_value* xg, const dfl_value* wgalpha, const dfl_index* row_ptr,
                                           const dfl_index* col_ind, const dfl_thermal_params* prm, dfl_value* val_phi,
                                           dfl_value* val_T, void* stream);

/* ---- fluid material (build-defined, opt-in; host/fluid.c, csrc/k_fluid.hip, csrc/fluid_coeff.hpp, model in include/dedflow.h)
 *    dfl_fluid_rows          the node sums r [4N] (momentum rows r[3a + d], continuity rows r[3N + a]), Rn [N] (kg), Mn [N]
 *                            (Pa s m^3) at the states w, dw [6N] (taken as the alpha states; the pressure is dw[3N + a], as
 *                            in the assembly); any of them NULL: not written, the others overwritten in full.  vrow / vcol:
 *                            the V2E map of the tets with every list ascending.  The node gather of the thermal rows: a lane
 *                            per (node, tet), the shares added in list order through LDS, no atomics, bitwise reproducible.
 *                            r alone: a tet whose rho_q, mu_q are the built-in constants and whose f_q are zero leaves
 *                            early; its share of r is +0.0 in either case.
 *    dfl_fluid_add_rows      the same r, added by its owner lanes to F[0 .. 4N): F[i] += r[i], r[i] summed and rounded
 *                            first.  One launch, no buffer.
 *    dfl_fluid_add_jacobian  val[16 nz + e] += S[e] for every nonzero nz of the nodal pattern row_ptr / col_ind (block values
 *                            of the (u,p) matrix, e = 4 i + j): S = the sum of the difference blocks jm_ab over the row's
 *                            tets that hold the column, ascending tet id, from +0.0, rounded before the one
 *                            read-modify-write by the lane that owns the nonzero.  wgalpha: u, phi (with use_phi) are read.
 * Every launcher returns at once for N <= 0. */
typedef struct dfl_fluid_params {
    dfl_value rho_gas, rho_metal, mu_gas, mu_metal;
    dfl_value gravity[3];
    dfl_value beta, T_ref;
    dfl_value level, side, eps;
    int use_phi;
} dfl_fluid_params;
void dfl_fluid_rows(dfl_index N, const dfl_index* vrow, const dfl_index* vcol, const dfl_index* ien, const dfl_value* xg,
                    const dfl_value* w, const dfl_value* dw, const dfl_fluid_params* prm, dfl_value* r, dfl_value* Rn,
                    dfl_value* Mn, void* stream);
void dfl_fluid_add_rows(dfl_index N, const dfl_index* vrow, const dfl_index* vcol, const dfl_index* ien, const dfl_value* xg,
                        const dfl_value* wgalpha, const dfl_value* dwgalpha, const dfl_fluid_params* prm, dfl_value* F,
                        void* stream);
void dfl_fluid_add_jacobian(dfl_index N, const dfl_index* vrow, const dfl_index* vcol, const dfl_index* ien, const dfl_value* xg,
                            const dfl_value* wgalpha, const dfl_index* row_ptr, const dfl_index* col_ind,
                            const dfl_fluid_params* prm, dfl_value* val, void* stream);

/* ---- level-set redistancing (build-defined, opt-in; host/redistance.c, csrc/k_redistance.hip, model in include/dedflow.h)
 * phi = w + 4N.  grid: the uniform cell grid over the mesh's bounding box; a point's cell per axis is
 * clamp(floor((x - lo) inv_h), 0, n - 1), cell id = cx + n[0] (cy + n[1] cz).
 *    dfl_redistance_cut      one thread per tet, workgroups of dfl_tets_per_block() tets.  part[2 b], part[2 b + 1]
 *                            = workgroup b's volume of {phi > level} (fixed tree) and its maximum of ||g| - 1| over the cut
 *                            tets.  With blk_count: blk_count[b] = facets of workgroup b, and cell_count[c] += 1 for every
 *                            cell c the bounding box of a facet's finite vertices overlaps (integer atomics; a vertex
 *                            with a NaN coordinate cannot win, the others still count).  blk_count NULL: the statistics alone.
 *    dfl_redistance_emit     the facets in ascending tet order, a quad's first triangle first: facet blk_base[b] + (facets of
 *                            the earlier tets of workgroup b), and its index into every cell it overlaps at
 *                            cell_start[c] + cell_fill[c]++ (cell_fill zero on entry; the order inside a cell is free).
 *                            Nothing is written at or beyond cap_facets / cap_entries.
 *    dfl_redistance_nodes    ncand[0] = 0 on entry.  Pass 1, one thread per node: the entries of the 27 cells around the node
 *                            as nine three-cell runs of cell_start; none: phi = level +- band at once (chg = -1), else
 *                            the node joins list (wave ballot, one integer atomic per wave).  Pass 2, 16 lanes per listed
 *                            node: the lanes stride the entries with a running minimum of the squared distance, four
 *                            xor-shuffles, lane 0 writes phi = level +- min(d, band) and chg = |new - old| where d < band,
 *                            else -1.  A node with hold[a] != 0 (hold NULL: none) or a NaN phi keeps its value (chg 0 in
 *                            the band).
 *    dfl_redistance_node_stats  out2 = (number of nodes with chg >= 0, their maximum chg); work >= 2 dfl_node_reduce_max_part()
 *                            doubles
 *    dfl_redistance_reduce   out2 = (sum of part[2 i] in a fixed order, max of part[2 i + 1]), i < npart */
typedef struct dfl_redistance_grid {
    dfl_value lo[3], inv_h;
    dfl_index n[3];
} dfl_redistance_grid;
void dfl_redistance_cut(dfl_index T, const dfl_index* ien, const dfl_value* xg, const dfl_value* w, dfl_index N, dfl_value level,
                        const dfl_redistance_grid* grid, dfl_index* blk_count, dfl_index* cell_count, dfl_value* part,
                        void* stream);
void dfl_redistance_emit(dfl_index T, const dfl_index* ien, const dfl_value* xg, const dfl_value* w, dfl_index N, dfl_value level,
                         const dfl_redistance_grid* grid, const dfl_index* blk_base, const dfl_index* cell_start,
                         dfl_index* cell_fill, dfl_value* facets, dfl_index cap_facets, dfl_index* entries,
                         dfl_index cap_entries, void* stream);
void dfl_redistance_nodes(dfl_index N, const dfl_value* xg, dfl_value* w, dfl_value level, dfl_value band,
                          const dfl_redistance_grid* grid, const dfl_index* cell_start, const dfl_index* entries,
                          const dfl_value* facets, dfl_index cap_facets, const unsigned char* hold, dfl_index* ncand,
                          dfl_index* list, dfl_value* chg, void* stream);
void dfl_redistance_node_stats(dfl_index N, const dfl_value* chg, dfl_value* work, dfl_value* out2, void* stream);
void dfl_redistance_reduce(dfl_index npart, const dfl_value* part, dfl_value* out2, void* stream);

/* ---- level-set volume correction (build-defined, opt-in; host/volume.c, csrc/k_volume.hip, model in include/dedflow.h)
 * phi = w + 4N, lo = level - max_shift, hi = level + max_shift.  A tet is inside when its four phi are > hi, a band tet when
 * it is not inside and has a phi > lo.  Workgroups of dfl_tets_per_block() tets.  Every sum has a fixed order.
 *    dfl_volume_classify  one thread per tet.  blk_count[b] = band tets of workgroup b; part: [workgroups][5]; out5 = (V_in: the
 *                         |det| / 6 of the inside tets, the volume of {phi > level}, {phi > lo} and {phi > hi} inside the
 *                         band tets, the mesh volume)
 *    dfl_volume_emit      the ids of the band tets in ascending order: list[blk_base[b] + (band tets among the earlier tets
 *                         of workgroup b)] = tet id.  Nothing is written at or beyond cap
 *    dfl_volume_eval      outK[k] = the volume of {phi > cand[k]} inside the nband listed tets, k < DFL_VOLUME_K; cand is on
 *                         the host and travels as a kernel argument; part: [ceil(nband / 256)][DFL_VOLUME_K]
 *    dfl_volume_shift     phi_a += delta for every node, one rounded addition; a NaN is not written
 *    dfl_volume_node_sum  out1[0] = sum of q[0 .. N); work >= dfl_node_reduce_max_part() doubles */
#define DFL_VOLUME_K 15
void dfl_volume_classify(dfl_index T, const dfl_index* ien, const dfl_value* xg, const dfl_value* w, dfl_index N, dfl_value level,
                         dfl_value lo, dfl_value hi, dfl_index* blk_count, dfl_value* part, dfl_value* out5, void* stream);
void dfl_volume_emit(dfl_index T, const dfl_index* ien, const dfl_value* w, dfl_index N, dfl_value lo, dfl_value hi,
                     const dfl_index* blk_base, dfl_index* list, dfl_index cap, void* stream);
void dfl_volume_eval(dfl_index nband, const dfl_index* list, const dfl_index* ien, const dfl_value* xg, const dfl_value* w,
                     dfl_index N, const dfl_value* cand, dfl_value* part, dfl_value* outK, void* stream);
void dfl_volume_shift(dfl_index N, dfl_value* w, dfl_value delta, void* stream);
void dfl_volume_node_sum(dfl_index N, const dfl_value* q, dfl_value* work, dfl_value* out1, void* stream);

/* ---- solidification record (build-defined, opt-in; host/solidify.c, csrc/k_solidify.hip, model in include/dedflow.h)
 * The record arrays: T_prev, T_peak, t_liquid, t_solid, cool [N], grad3 [3N], melts [N] integers, metal [N] bytes (the metal
 * flag of every node as its last update saw it).  nblk = ceil(N / dfl_tets_per_block()) workgroups of the per-node kernels.
 *    dfl_solid_reset     the initial values: T_prev NaN, T_peak -inf, t_solid NaN, everything else 0
 *    dfl_solid_prime     T_prev = T, T_peak = fmax(T_peak, T), metal, of the state w [6N]
 *    dfl_solid_count     the freeze and melt events of an update of w as two counts per workgroup, blk_count and melt_count
 *                        [nblk]; writes nothing else.  The caller scans blk_count into blk_base [nblk + 1] (dfl_scan_counts)
 *    dfl_solid_events    the same decision again and every elementwise rule of the update of length dt at the elapsed time t;
 *                        the freeze-event nodes into list [N] in ascending order, blk_base[nblk] of them
 *    dfl_solid_gradient  grad3[3a + d] of the first *count nodes of list: a group of 16 lanes per listed node walks the node's
 *                        sorted V2E list, a lane per tet, four sums per node in list order through LDS.  The grid strides
 *                        over the list and reads count on the device.  No atomics: bitwise reproducible
 *    dfl_solid_stats     out11 = (frozen, liquid, freeze events, melt events, G_min, G_max, cool_min, cool_max, R_min, R_max,
 *                        T_peak_max) in a fixed two-stage order; freeze_total: the device word that holds the list length;
 *                        work >= dfl_solid_stats_work_size() doubles
 * Every launcher returns at once for N <= 0. */
typedef struct dfl_solid_params {
    dfl_value T_front, level, side;
    int use_phi;
} dfl_solid_params;
void dfl_solid_reset(dfl_index N, dfl_value* T_prev, dfl_value* T_peak, dfl_value* t_liquid, dfl_index* melts, dfl_value* t_solid,
                     dfl_value* cool, dfl_value* grad3, unsigned char* metal, void* stream);
void dfl_solid_prime(dfl_index N, const dfl_value* w, const dfl_solid_params* prm, dfl_value* T_prev, dfl_value* T_peak,
                     unsigned char* metal, void* stream);
void dfl_solid_count(dfl_index N, const dfl_value* w, const dfl_solid_params* prm, dfl_value dt, const dfl_value* T_prev,
                     dfl_index* blk_count, dfl_index* melt_count, void* stream);
void dfl_solid_events(dfl_index N, const dfl_value* w, const dfl_solid_params* prm, dfl_value t, dfl_value dt,
                      const dfl_index* blk_base, dfl_value* T_prev, dfl_value* T_peak, dfl_value* t_liquid, dfl_index* melts,
                      dfl_value* t_solid, dfl_value* cool, dfl_value* grad3, unsigned char* metal, dfl_index* list, void* stream);
void dfl_solid_gradient(dfl_index N, const dfl_index* count, const dfl_index* list, const dfl_index* vrow, const dfl_index* vcol,
                        const dfl_index* ien, const dfl_value* xg, const dfl_value* w, const dfl_solid_params* prm,
                        dfl_value* grad3, void* stream);
dfl_index dfl_solid_stats_work_size(void);
void dfl_solid_stats(dfl_index N, dfl_value T_front, const dfl_value* T_prev, const dfl_value* T_peak, const dfl_value* t_solid,
                     const dfl_value* cool, const dfl_value* grad3, const unsigned char* metal, dfl_index nblk,
                     const dfl_index* freeze_total, const dfl_index* melt_count, dfl_value* work, dfl_value* out11, void* stream);

/* ---- track cross-sections (build-defined, opt-in; host/track.c, csrc/k_track.hip, model in include/dedflow.h)
 * prm: the frame (o, n, t, u) as the host formed it, level, side (+-1.0), T_fuse and the num_station ascending offsets c.
 * Workgroups of dfl_tets_per_block() tets, nblk of them; count [num_station nblk] and base [num_station nblk + 1] are
 * station-major: entry k nblk + b belongs to station k and workgroup b.  No atomics; every sum has a fixed order.
 *    dfl_track_count    count[k nblk + b] = pairs of station k among the tets of workgroup b.  A workgroup without a pair
 *                       writes nothing: count is zero on entry (dfl_scan_counts leaves it so)
 *    dfl_track_offsets  off65[k] = base[k nblk] for k < num_station, the total base[num_station nblk] from there on
 *    dfl_track_emit     the same decisions again: the tet ids of station k into list[off65[k] ..) in ascending order.  Nothing is
 *                       written at or beyond cap
 *    dfl_track_eval     one thread per pair, grid (max_chunk, num_station) with max_chunk >= ceil(longest segment / 256): the
 *                       DFL_TRACK_NSTAT components of every station (area_clad, area_fused, area_scale, height, depth,
 *                       y_lo_clad, y_hi_clad, y_lo_fused, y_hi_fused) through part [num_station][max_chunk][DFL_TRACK_NSTAT]
 *                       into out [num_station][DFL_TRACK_NSTAT]; T_peak NULL: every g is -inf.  A station without a pair gets
 *                       0 for the sums, +inf for the minima, -inf for the maxima */
#define DFL_TRACK_MAX_STATION 64
#define DFL_TRACK_NSTAT 9
typedef struct dfl_track_params {
    dfl_value o[3], n[3], t[3], u[3];
    dfl_value level, side, T_fuse;
    dfl_index num_station;
    dfl_value c[DFL_TRACK_MAX_STATION];
} dfl_track_params;
void dfl_track_count(dfl_index T, const dfl_index* ien, const dfl_value* xg, const dfl_value* w, dfl_index N,
                     const dfl_track_params* prm, dfl_index nblk, dfl_index* count, void* stream);
void dfl_track_offsets(dfl_index num_station, dfl_index nblk, const dfl_index* base, dfl_index* off65, void* stream);
void dfl_track_emit(dfl_index T, const dfl_index* ien, const dfl_value* xg, const dfl_value* w, dfl_index N,
                    const dfl_track_params* prm, dfl_index nblk, const dfl_index* base, dfl_index* list, dfl_index cap,
                    void* stream);
void dfl_track_eval(dfl_index max_chunk, const dfl_index* off65, const dfl_index* list, const dfl_index* ien, const dfl_value* xg,
                    const dfl_value* w, dfl_index N, const dfl_value* T_peak, const dfl_track_params* prm, dfl_value* part,
                    dfl_value* out, void* stream);

/* ---- the time step as a run-time value (include/dedflow.h, "time step") ------------------------------------------------------
 * dfl_step_consts is everything the kernels and the driver take from the step dt, formed by dfl_step_consts_from_dt alone, every
 * entry in the operation order of the compile-time expression it replaces (products only: nothing a compiler could fuse).  The
 * kernels get it by value as a kernel argument: it is wave-uniform and lives in SGPRs.  A product that the compiler used to
 * fold into ONE literal is ONE entry here, so that the fused multiply-adds formed around it stay the ones formed around the
 * literal, and the default step gives the bits of the compile-time build.
 *
 * Every launcher above that depends on the step keeps its name, arguments and behaviour (the default step) and forwards to the
 * *_dt entry point of the same argument list with `const dfl_step_consts* k` before the stream.
 *
 * Step limits (csrc/k_steplimit.hip; the formulas are in include/dedflow.h, "time step"):
 *    dfl_step_limit_partials  grid-stride over 256-tet workgroups, `grid` of them: the three maxima and their lowest tet ids
 *                             and the two counts of every workgroup into part_v [grid][3], part_i [grid][5]
 *    dfl_step_limit_finish    one workgroup: the same over the partials into out_v [3], out_i [5]
 *    dfl_step_limits          both; max_workgroups 0: the default grid.  part_v / part_i hold dfl_step_limit_grid(T, max_workgroups)
 *                             records.  out_i = tet_adv, tet_surface, tet_cap, num_cut, num_nonfinite.  No atomics: maxima are
 *                             exact in any order and "the lowest id that attains it" is order-free */
#ifndef DFL_DEFAULT_TIME_STEP
#define DFL_DEFAULT_TIME_STEP (5e-2)
#endif
typedef struct dfl_step_consts {
    dfl_value dt;
    dfl_value t0;          /* 4.0 / (dt * dt) */
    dfl_value fact2;       /* dt * kALPHAF * kGAMMA */
    dfl_value fact2_rho;   /* fact2 * kRHO */
    dfl_value fact2_rho2;  /* fact2 * kRHO * kRHO */
    dfl_value fact2_mu4;   /* 4.0 * fact2 * kMU */
    dfl_value fact2_kappa; /* fact2 * kKAPPA */
    dfl_value states_old;  /* dt * kALPHAF * (1.0 - kGAMMA): with fact2 the alpha-level state */
    dfl_value corr_old;    /* dt * (1.0 - kGAMMA): with corr_new the corrector */
    dfl_value corr_new;    /* dt * kGAMMA */
} dfl_step_consts;
void dfl_step_consts_from_dt(double dt, dfl_step_consts* k);
const dfl_step_consts* dfl_step_consts_default(void); /* those of DFL_DEFAULT_TIME_STEP */
void dfl_assemble_tet_lhs_dt(dfl_index batch_size, const dfl_index* ien_b, const dfl_index* nzmap_b, const dfl_value* egeo_b,
                             const dfl_value* nodep, dfl_value* val, const dfl_step_consts* k, void* stream);
void dfl_assemble_tet_rhs_dt(dfl_index batch_size, const dfl_index* ien_b, const dfl_value* nodep, dfl_value* Fp,
                             const dfl_step_consts* k, void* stream);
void dfl_assemble_tet_lhs_slot_dt(dfl_index npatch, const int32_t* hdr, const uint32_t* ptet_lid, const dfl_index* pnode,
                                  const dfl_index* slot_nz, const uint32_t* ldesc, const dfl_value* nodep, dfl_value* val,
                                  dfl_value beta, dfl_index max_tets, const dfl_step_consts* k, void* stream);
void dfl_assemble_tet_rhs_lane_dt(dfl_index npatch, const dfl_index* cnt, const dfl_index* pnode, const unsigned char* lien,
                                  const unsigned short* sub4, const unsigned short* sub_start, const dfl_value* nodep,
                                  dfl_value* partial, const dfl_step_consts* k, void* stream);
void dfl_assemble_face_dt(dfl_index n_face, const dfl_index* face_list, const dfl_index* f2e, const dfl_index* forn,
                          const dfl_index* ien, dfl_index N, const dfl_value* xg, const dfl_value* wg, const dfl_value* dwg,
                          dfl_value* F, const dfl_index* rp, const dfl_index* ci, dfl_value* val, const dfl_step_consts* k,
                          void* stream);
void dfl_assemble_face_park_dt(dfl_index nf, const dfl_index* f2e, const dfl_index* forn, const dfl_index* ien, dfl_index N,
                               const dfl_value* xg, const dfl_value* wg, const dfl_value* dwg, dfl_value* pF, dfl_value* pJ,
                               const dfl_step_consts* k, void* stream);
void dfl_assemble_scalar_jacobian_dt(dfl_index N, const dfl_index* vrow, const dfl_index* vcol, const dfl_index* ien,
                                     const dfl_value* xg, const dfl_value* wgalpha, const dfl_index* row_ptr,
                                     const dfl_index* col_ind, dfl_value* val_phi, dfl_value* val_T, const dfl_step_consts* k,
                                     void* stream);
void dfl_assemble_scalar_jacobian_material_dt(dfl_index N, const dfl_index* vrow, const dfl_index* vcol, const dfl_index* ien,
                                              const dfl_value* xg, const dfl_value* wgalpha, const dfl_index* row_ptr,
                                              const dfl_index* col_ind, const dfl_thermal_params* prm, dfl_value* val_phi,
                                              dfl_value* val_T, const dfl_step_consts* k, void* stream);
void dfl_fluid_rows_dt(dfl_index N, const dfl_index* vrow, const dfl_index* vcol, const dfl_index* ien, const dfl_value* xg,
                       const dfl_value* w, const dfl_value* dw, const dfl_fluid_params* prm, dfl_value* r, dfl_value* Rn,
                       dfl_value* Mn, const dfl_step_consts* k, void* stream);
void dfl_fluid_add_rows_dt(dfl_index N, const dfl_index* vrow, const dfl_index* vcol, const dfl_index* ien, const dfl_value* xg,
                           const dfl_value* wgalpha, const dfl_value* dwgalpha, const dfl_fluid_params* prm, dfl_value* F,
                           const dfl_step_consts* k, void* stream);
void dfl_fluid_add_jacobian_dt(dfl_index N, const dfl_index* vrow, const dfl_index* vcol, const dfl_index* ien,
                               const dfl_value* xg, const dfl_value* wgalpha, const dfl_index* row_ptr, const dfl_index* col_ind,
                               const dfl_fluid_params* prm, dfl_value* val, const dfl_step_consts* k, void* stream);

typedef struct dfl_step_limit_params {
    dfl_value level;
    dfl_value sigma0, dsigma_dT, T_ref; /* all 0 without surface forces: sigma_e = 0 */
} dfl_step_limit_params;
dfl_index dfl_step_limit_grid(dfl_index T, dfl_index max_workgroups);
void dfl_step_limit_partials(dfl_index T, const dfl_index* ien, const dfl_value* xg, const dfl_value* w, dfl_index N,
                             const dfl_step_limit_params* prm, dfl_index grid, dfl_value* part_v, dfl_index* part_i, void* stream);
void dfl_step_limit_finish(dfl_index grid, const dfl_value* part_v, const dfl_index* part_i, dfl_value* out_v, dfl_index* out_i,
                           void* stream);
void dfl_step_limits(dfl_index T, const dfl_index* ien, const dfl_value* xg, const dfl_value* w, dfl_index N,
                     const dfl_step_limit_params* prm, dfl_index max_workgroups, dfl_value* part_v, dfl_index* part_i,
                     dfl_value* out_v, dfl_index* out_i, void* stream);

/* ---- porosity record (build-defined, opt-in; host/porosity.c, csrc/k_porosity.hip, model in include/dedflow.h)
 * prm: level, side (+-1.0) and the rows kept.  parent / label / open / rank / pore are [N]; rows [max_pores]; tot is one device
 * record that a single copy brings back.  Every launcher returns the number of launches it made, which depends on its
 * arguments' sizes and never on the state (a sort counts as one).  No float atomics; integer atomics carry counts and extremes.
 *    dfl_porosity_label   rows and counters to their empty values; parent[a] = a (gas), -1 (metal), -2 (phi not finite, counted);
 *                         the lock-free union-find over the tets without a bad node (agent-scope atomics on parent[] only);
 *                         label[a] = the smallest node id of a's component; open[label] = 1 at the gas nodes of the nof faces
 *                         oface (indices into f2e / forn)
 *    dfl_porosity_rank    the pore roots (label[a] == a, not open) in ascending id get rank[a]; row rank gets its label;
 *                         pore[a] = the rank of a's pore or -1; nodes and the node part of the box of every row; the
 *                         components counted.  count [nblk], base [nblk + 1] with nblk = ceil(N / dfl_tets_per_block())
 *    dfl_porosity_tets    per tet without a bad node the metal volume, and the gas volume to the open or the pore total, through
 *                         part [nblk][3] into tot->volume; the bad tets counted; count / base as above over the tets: the tets of
 *                         closed components.  Then pores = node_base[nblk_node] and the closed tets into tot->count
 *    dfl_porosity_pores   the keys rank << 32 | tet of the nclosed closed tets in ascending tet id, sorted (the keys are distinct) into
 *                         key_out (temp of dfl_porosity_temp_bytes(cap) bytes); per key the gas volume and |det| / 6 into vals
 *                         [cap][2], the crossing points and the metal nodes' T into the row's extremes; the head of every run
 *                         sums its run in order and owns volume, volume_scale and tets of its row.  Rows at or beyond max_pores
 *                         are not kept */
#define DFL_POROSITY_NCOUNT 8
#define DFL_POROSITY_MAX_PORES 65536
typedef struct dfl_porosity_params {
    dfl_value level, side;
    dfl_index max_pores;
} dfl_porosity_params;
/* ext: lo[3], hi[3], T_wall_min, T_wall_max as integers of the doubles' order: bits | 2^63 for a value whose sign bit is clear,
 * ~bits otherwise */
typedef struct dfl_pore_row {
    dfl_index label, nodes, tets, pad;
    dfl_value volume, volume_scale;
    uint64_t ext[8];
} dfl_pore_row;
/* count: 0 components, 1 pores, 2 tets of closed components, 3 bad nodes, 4 bad tets; volume: metal, open, pores */
typedef struct dfl_porosity_totals {
    dfl_index count[DFL_POROSITY_NCOUNT];
    dfl_value volume[3];
} dfl_porosity_totals;
int64_t dfl_porosity_temp_bytes(dfl_index n);
int dfl_porosity_label(dfl_index N, dfl_index T, const dfl_index* ien, const dfl_value* w, const dfl_porosity_params* prm,
                       dfl_index nof, const dfl_index* oface, const dfl_index* f2e, const dfl_index* forn, dfl_index* parent,
                       dfl_index* label, dfl_index* open, dfl_pore_row* rows, dfl_porosity_totals* tot, void* stream);
int dfl_porosity_rank(dfl_index N, const dfl_value* xg, const dfl_porosity_params* prm, const dfl_index* label,
                      const dfl_index* open, dfl_index* count, dfl_index* base, dfl_index* chunk_sum, dfl_index* rank,
                      dfl_index* pore, dfl_pore_row* rows, dfl_porosity_totals* tot, void* stream);
int dfl_porosity_tets(dfl_index T, const dfl_index* ien, const dfl_value* xg, const dfl_value* w, dfl_index N,
                      const dfl_porosity_params* prm, const dfl_index* label, const dfl_index* open, dfl_index nblk_node,
                      const dfl_index* node_base, dfl_index* count, dfl_index* base, dfl_index* chunk_sum, dfl_value* part,
                      dfl_porosity_totals* tot, void* stream);
int dfl_porosity_pores(dfl_index T, const dfl_index* ien, const dfl_value* xg, const dfl_value* w, dfl_index N,
                       const dfl_porosity_params* prm, const dfl_index* label, const dfl_index* open, const dfl_index* pore,
                       const dfl_index* base, dfl_index nclosed, uint64_t* key, uint64_t* key_out, dfl_index cap, dfl_value* vals,
                       void* temp, int64_t temp_bytes, dfl_pore_row* rows, void* stream);

/* ---- surface mesh (build-defined, opt-in; host/surface_mesh.c, csrc/k_surface_mesh.hip, model in include/dedflow.h)
 * prm: level and side (+-1.0).  code is [T] bytes; count [2 nblk] and start [2 nblk + 1] with nblk = ceil(T /
 * dfl_tets_per_block()), chunk_sum for a scan of 2 nblk entries; tot is one device record that a single copy brings back.  Every
 * launcher returns the number of launches it made, which depends on its arguments' sizes and never on the state (a sort counts
 * as one).  No float atomics; integer atomics carry counts only.
 *    dfl_surface_mesh_count   zeroes tot; the bad nodes counted; code[e] = 0 for a tet that emits nothing (bad and degenerate
 *                             tets counted), else the mask of its metal nodes | 16 for a negative determinant; the triangles
 *                             and edge keys per workgroup scanned into start; tot->count[0] = triangles, [1] = edge keys
 *    dfl_surface_mesh_build   nt and nkeys are those two counts (nothing is launched when either is 0).  tri_tet [capt] at every
 *                             tet's triangle offset; the keys min << bits | max of the cut edges, bits = ceil(log2 N), sorted
 *                             into key_out (temp of dfl_surface_mesh_temp_bytes(N, nkeys) bytes at least); the heads of the
 *                             runs counted per workgroup (kcount [nkb], kbase [nkb + 1], nkb = ceil(nkeys / 256), kchunk for
 *                             that scan); per head its rank's key (into key: the unique list), edge [.][2], t, verts [.][3] and
 *                             vals [.][num_fields] (each list holds capk rows); per triangle the three ranks by binary search,
 *                             oriented by the table, into tris [capt][3], and its area through part [ceil(nt / 256)] into
 *                             tot->area; tot->count[2] = vertices.  fields: num_fields <= 8 device [N] arrays (a host array) */
#define DFL_SURFACE_MESH_NCOUNT 8
#define DFL_SURFACE_MESH_MAX_FIELDS 8
typedef struct dfl_surface_mesh_params {
    dfl_value level, side;
} dfl_surface_mesh_params;
/* count: 0 triangles, 1 edge keys (one per cut edge of every emitting tet), 2 vertices, 3 bad nodes, 4 bad tets, 5 degenerate tets */
typedef struct dfl_surface_mesh_totals {
    dfl_index count[DFL_SURFACE_MESH_NCOUNT];
    dfl_value area;
} dfl_surface_mesh_totals;
/* the largest number of keys rocprim sorts inside one workgroup (the tests size a case beyond it) */
dfl_index dfl_surface_mesh_sort_block(void);
int64_t dfl_surface_mesh_temp_bytes(dfl_index N, dfl_index n);
int dfl_surface_mesh_count(dfl_index N, dfl_index T, const dfl_index* ien, const dfl_value* xg, const dfl_value* w,
                           const dfl_surface_mesh_params* prm, unsigned char* code, dfl_index* count, dfl_index* start,
                           dfl_index* chunk_sum, dfl_surface_mesh_totals* tot, void* stream);
int dfl_surface_mesh_build(dfl_index N, dfl_index T, const dfl_index* ien, const dfl_value* xg, const dfl_value* w,
                           const dfl_surface_mesh_params* prm, const unsigned char* code, const dfl_index* start, dfl_index nt,
                           dfl_index nkeys, uint64_t* key, uint64_t* key_out, dfl_index capk, void* temp, int64_t temp_bytes,
                           dfl_index* kcount, dfl_index* kbase, dfl_index* kchunk, const dfl_value* const* fields,
                           dfl_index num_fields, dfl_value* verts, dfl_index* edge, dfl_value* t, dfl_value* vals, dfl_index* tris,
                           dfl_index* tri_tet, dfl_index capt, dfl_value* part, dfl_surface_mesh_totals* tot, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DEDFLOW_KERNELS_H */
