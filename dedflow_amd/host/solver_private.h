/* Krylov solver internals shared by host/solver.c, host/gmres.c and host/ws_placement.c. */
#ifndef DFL_SOLVER_PRIVATE_H
#define DFL_SOLVER_PRIVATE_H
#include "dedflow.h"

typedef struct KrylovExt {
    KrylovStats stats;
    index_type check_interval;
    b32 check_interval_set; /* KrylovSetCheckInterval was called: PC_TWOLEVEL leaves the interval alone */
    b32 verbose;
    DflComm comm;
    b32 has_comm;
    PCType pc_type; /* tree KrylovSolve builds: PC_DECOMPOSITION (reference) or PC_ILU0 */
    index_type restart; /* GMRES(m): basis columns per cycle; <= 0 or >= max_iter = full GMRES (the reference, krylov.c:56-334) */
    b32 flexible_user; /* KrylovSetFlexible(on): FGMRES whatever the preconditioner; otherwise PC_TWOLEVEL alone switches it on */
    b32 flexible;   /* FGMRES: keep Z[:,k] = M_k^-1 Q[:,k] (a second basis) so that the preconditioner may vary from step to step */
    const Mesh3D* mesh; /* optional: node coordinates for preconditioners that aggregate nodes (PC_TWOLEVEL) */
    index_type agg_size; /* PC_TWOLEVEL: nodes per aggregate */
    b32 fused_norm; /* partitioned runs: ||w - Qh|| from w.w - sum h^2, one all-reduce per Arnoldi step (off by default) */
    int q_pooled;   /* the basis Q came from the device pool (placement calibration may pick either kind) */
    int* d_flag;    /* device int raised by the fused-norm kernel on heavy cancellation */
    f64* hraw;      /* [ldh] raw CGS coefficients + w.w of the current column (fused update + PC + Givens kernel) */
    /* cached GMRES work space */
    index_type ws_n, ws_maxit, ws_hist;
    int ws_pooled; /* where Q and tmp of the cached work space came from */
    b32 ws_fresh;  /* the basis was (re)allocated and its placement has not been calibrated yet */
    f64 *Q, *Z, *H, *tmp, *gv, *beta, *res_hist, *nrm, *work;
    int64_t work_len;
    /* host reads of a solve without idling the GPU (GMRESSolvePrivate): probes + ||r0|| travel with the first convergence
       check, the check itself is read one iteration late */
    f64* nrm_base;      /* allocation behind nrm: [tail probe, x probe, -, -, nrm[0], ...] */
    f64* h_stat;        /* pinned host staging [16] */
    hipEvent_t ev_stat;
    b32 assume_valid, assume_tail_zero, assume_x_zero; /* what the previous solve of this solver found (verified per solve) */
    /* p(1)-pipelined GMRES (KrylovSetPipelined): auxiliary basis z_{j+1} = A M^-1 v_j, the reduction's own stream */
    b32 pipelined;
    f64* Zp;
    index_type zp_n, zp_m;
    int zp_pooled;
    hipStream_t red_stream;
    hipEvent_t ev_w, ev_h;
    b32 no_calibration; /* inner / coarse solvers of PC_TWOLEVEL: never time basis placements (DflKrylovMarkInner) */
    char* amgx_cfg;     /* KrylovSetAMGXConfig: options of PCCreateAMGX (NULL: the reference configuration) */
    int last_step;      /* GmresStep of the most recent gmres_run (DflKrylovLastGmresStep), -1 before the first */
    /* raw-basis steps of more than one iteration (GmresPlan.block): the un-rotated copy of H (same shape); pair_buf, 8 ldh + 96
       doubles: [c1 | c2 | e | scalars] of a pair (ldh doubles each), or [c_0..c_3 | e_0..e_3 | G, C, U, derived G, raw sums] of a
       block (gmres_block);
       and how many counted steps of each size the most recent gmres_run took (DflKrylovLastGmresBlocks) */
    f64 *h_unrot, *pair_buf;
    int last_blocks[5], last_pair_cancelled;
    int last_folded; /* products of the most recent gmres_run that wrote M^-1 of their own output (DflKrylovLastFoldedProducts) */
    int last_fused;  /* counted blocks of that run whose update and fix-up were one pass (DflKrylovLastFusedBlocks) */
} KrylovExt;

static inline KrylovExt* kext(const Krylov* k) { return (KrylovExt*)k->ext; }

/* columns of the basis block behind the m + 1 Krylov vectors of a cycle: the two interleaved copies the matvec gathers from
   (GmresPlan.z4, z4b) share the block, and with it the placement the calibration chose */
#define DFL_BASIS_SPARE_COLS 2

/* Everything about one GMRES solve that does not change while it runs; filled once per solve by DflGmresPlanFill. */
typedef enum { GMRES_X4_NONE, GMRES_X4_SINGLE, GMRES_X4_PARTITIONED } GmresX4; /* matvec gathers from the interleaved copy */
typedef enum {
    GMRES_STEP_REFERENCE,      /* one GPU: dots, then update + norm + Givens in one launch (dfl_cgs_update_givens) */
    GMRES_STEP_TWO_REDUCTIONS, /* partitioned: all-reduce of h, update, all-reduce of the norm, dfl_givens_sq */
    GMRES_STEP_FUSED_NORM,     /* KrylovSetFusedNorm: ||w - Qh|| from w.w - sum h^2, one reduction (dfl_gmres_givens_pythagoras) */
    GMRES_STEP_FUSED_UPDATE_PC, /* ... with update, Givens and the next M^-1 in one launch (dfl_cgs_update_pc_givens_x4) */
    GMRES_STEP_RAW_BASIS       /* one GPU, Jacobi tree, x4: unnormalised basis, raw dots (dfl_cgs_dots_raw), the next M^-1 inside
                                  the update (dfl_cgs_update_jacobi_givens), the normalisation inside the matvec */
} GmresStep;
typedef struct GmresPlan {
    index_type n, na, m, ldh, maxit; /* rows, active length, basis columns per cycle, leading dimension of H, iteration cap */
    b32 dist, split_rows;            /* communicator; interior rows run while the halo is in flight */
    index_type n_interior, owned_rows;
    hipStream_t side;          /* split rows: the exchange's stream, which the boundary rows run on; NULL: the library stream */
    GmresX4 x4;                /* x4_N: nodes of the block matrix; x4_owned: nodes whose entries the producer of z interleaves */
    index_type x4_N, x4_owned;
    b32 x4_skip_z;             /* one GPU: nothing reads z in the reference layout, the PC kernel does not store it */
    f64* z4;                   /* the interleaved copy: the spare column of the basis block; NULL without x4 */
    f64* z4b;                  /* fold_pc: the second interleaved copy, the next spare column (gmres_products) */
    b32 fold_pc;               /* GMRES_STEP_RAW_BASIS, block > 1: every product of a pair or block but the last writes M^-1 of its
                                  own output, interleaved, for the product that follows (dfl_bcsr_spmv_x4_pc) instead of a Jacobi
                                  launch between the two; DFL_GMRES_FOLD_PC=0: the separate launches */
    b32 fuse_fixup;            /* GMRES_STEP_RAW_BASIS, block >= 3: a block of three or four takes C from the Gram matrix derived in
                                  the dots pass and runs update and fix-up as one pass (dfl_cgs_update_fixup_block), 9 launches
                                  instead of 10; DFL_GMRES_FUSE_FIXUP=0: the two passes with G measured between them */
    GmresStep step;
    int block;                 /* GMRES_STEP_RAW_BASIS: the largest number of iterations one pass over the basis serves (1..4); a trip
                                  takes as many as fit into the cycle with no convergence check between them (gmres_pair: 2,
                                  gmres_block: 3, 4); DFL_GMRES_BLOCK, default 4; DFL_GMRES_TWO_STEP=0: 1; any other step: 0 */
    const f64 *d33, *d1;       /* Jacobi tree (DflPcJacobiTreeData: d33, d1, N, rows) for the fused step */
    index_type N, rows;
    f64* Zb;                   /* FGMRES: the basis of preconditioned vectors; NULL otherwise */
    b32 lazy;                  /* host reads ride behind the next iteration instead of idling the device */
} GmresPlan;

/* A fused block raises bit 1 of the flag DflKrylovLastGmresBlocks reports when some |<q_a, q_b>| > tau ||q_a|| ||q_b||, measured on
   the vectors it formed: 100 times the largest value the numpy model shows on the six Kuhn-cube systems M = 6..40
   (9.3e-8 at M = 6; tests/fused_block_model.py: table()) */
#define DFL_GMRES_ORTH_TAU 9.3e-6

#define DFL_INTERNAL __attribute__((visibility("hidden"))) /* shared between the host sources, not exported */

/* host/solver.c */
PC* DflKrylovBuildPC(Krylov* ksp, Matrix* A);            /* the (re)build step of KrylovSolve */
void DflKrylovMarkInner(Krylov* ksp);
/* the reference's tree (krylov.c:439-453) in its fused form: the two inverse-diagonal arrays, node count, owned rows */
DFL_INTERNAL b32 DflPcJacobiTreeData(PC* pc, const f64** d33, const f64** d1, index_type* N, index_type* nrows);

/* host/gmres.c */
int DflWsInPool(void);
void DflWsVecFreeAs(f64* p, int pooled);
void DflPcApplyFused(PC* pc, index_type na, f64* w, const f64* d_nrm, f64* z);
b32 DflPcApplyFusedX4(PC* pc, index_type na, f64* w, const f64* d_nrm, f64* z, f64* z4); /* TRUE: z4 written too */
b32 DflKrylovEnsureWorkspace(Krylov* ksp, Matrix* A, index_type* n, index_type* m, index_type* ldh);
DFL_INTERNAL void GMRESSolvePrivate(Matrix* A, f64* x, f64* b, void* ctx);
DFL_INTERNAL void DflWsEnsure(KrylovExt* x, index_type n, index_type maxit, index_type ldh, index_type hist);
DFL_INTERNAL void DflWsFree(KrylovExt* x);
DFL_INTERNAL void DflGmresSizes(const KrylovExt* ex, index_type max_iter, index_type* m, index_type* ldh);
DFL_INTERNAL index_type DflKrylovTailBegin(Matrix* A);
DFL_INTERNAL void DflProbeOperands(const f64* b, index_type begin, index_type n, const f64* x, f64* scratch, b32* tail_zero, b32* x_zero);
DFL_INTERNAL void DflZeroGhostRows(const KrylovExt* ex, Matrix* A, f64* v, index_type na);
DFL_INTERNAL void DflGmresPlanFill(GmresPlan* p, const KrylovExt* ex, index_type max_iter, Matrix* A, PC* pc, index_type na, b32 pipelined);
DFL_INTERNAL b32 DflKrylovConverged(const Krylov* ksp, f64 rnrm, f64 rnrm_init);
DFL_INTERNAL void DflKrylovPrintProgress(const Krylov* ksp, index_type it, f64 rnrm, f64 rnrm_init, index_type restart_cycle);

/* host/ws_placement.c: where the Krylov basis (and, in the explicit heavy form, the value array) is placed */
f64* DflWsPickBasis(KrylovExt* ex, Matrix* A, PC* pc, f64* first, index_type max_iter, index_type na);

#endif
