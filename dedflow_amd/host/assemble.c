/* AssembleSystemTet / AssembleSystemTetFace (src/assemble.h:13-14) and their caller
 * AssembleSystem (src/main.c:31-75): the color-batch loop of src/assemble.cu:1559-1738
 * with one fused launch per color, no per-call device allocation (the reference
 * mallocs+memsets+frees nine work buffers per call, :1533-1553,1746-1760). */
#include <string.h>
#include "dedflow.h"
#include "dedflow_kernels.h"
#include "host_private.h"

#define BS (6)
static b32 g_quiet = FALSE;
/* process defaults of the per-mesh assembly configuration (copied into every mesh at Mesh3DCreate):
 *   schedule 4  nodes per patch, nodal nonzeros and tets per patch (one slot offset / one tet per lane of a 256-thread
 *               workgroup: <= 255 / <= 256)
 *   face group  boundary group whose faces carry the weak-BC terms (the reference hard-codes group 4) */
static AsmConfig g_asm = {4, 4, 7, 200, 128};
const AsmConfig* DflAsmDefaults(void) { return &g_asm; }
/* the schedule numbers that exist (include/dedflow.h); anything else is reported and replaced by the default */
static int checked_schedule(int mode) {
    if (mode == 0 || mode == 1 || mode == 4) return mode;
    fprintf(stderr, "dedflow: assembly schedule %d does not exist (0, 1 or 4); using schedule 4\n", mode);
    return 4;
}
void DflSetAssemblySchedule(int mode) { g_asm.sched_mode = checked_schedule(mode); }
void DflSetSlotPatchParameters(index_type leaf_nodes, index_type slot_cap, index_type tet_cap) {
    if (leaf_nodes > 0) g_asm.slot_leaf = leaf_nodes;
    if (slot_cap > 0) g_asm.slot_cap = slot_cap > DFL_SLOT_BLOCK - 1 ? DFL_SLOT_BLOCK - 1 : slot_cap;
    if (tet_cap > 0) g_asm.slot_tets = tet_cap > DFL_SLOT_BLOCK ? DFL_SLOT_BLOCK : tet_cap;
}
void DflSetWeakBCGroup(index_type group) { g_asm.face_group = group; }
/* the same two switches for one existing mesh (the schedule before Mesh3DGenerateColorBatch) */
void DflMeshSetAssemblySchedule(Mesh3D* mesh, int mode) { ((MeshExt*)mesh->ext)->cfg.sched_mode = checked_schedule(mode); }
void DflMeshSetWeakBCGroup(Mesh3D* mesh, index_type group) { ((MeshExt*)mesh->ext)->cfg.face_group = group; }
void DflSetQuiet(b32 quiet) { g_quiet = quiet; }
void DflMeshSetExternalLoad(Mesh3D* mesh, const f64* load) { ((MeshExt*)mesh->ext)->ext_load = load; }
const f64* DflMeshExternalLoad(const Mesh3D* mesh) { return ((const MeshExt*)mesh->ext)->ext_load; }
void DflMeshSetHeatSource(Mesh3D* mesh, const f64* q) { ((MeshExt*)mesh->ext)->heat_source = q; }
const f64* DflMeshHeatSource(const Mesh3D* mesh) { return ((const MeshExt*)mesh->ext)->heat_source; }
void DflMeshSetVolumeSource(Mesh3D* mesh, const f64* q_vol) { ((MeshExt*)mesh->ext)->vol_source = q_vol; }
const f64* DflMeshVolumeSource(const Mesh3D* mesh) { return ((const MeshExt*)mesh->ext)->vol_source; }
/* node coordinates were modified (moving mesh): drop the per-element geometry cache, rebuilt at the next assembly */
void DflMeshGeometryChanged(Mesh3D* mesh) {
    MeshExt* x = (MeshExt*)mesh->ext;
    if (!x) return;
    CdamFreeDevice(x->egeo_b, 0);
    x->egeo_b = NULL;
    x->geom_epoch++; /* a coupled particle context's bound on |grad N| (host/surface_contact.c) is recomputed at its next use */
    DflRedistanceGeometryChanged(x->redistance); /* its cell grid covers the old bounding box */
    /* schedule 4 and the residual kernels recompute the geometry from the node records; the face lists hold no geometry,
       and the free-surface and phase-change states (host/surface.c, host/phase.c) hold connectivity only: their kernels read xg
       at every call */
}
b32 DflQuiet(void) { return g_quiet; }

/* the 4x4-block array the kernels write and its nodal pattern.  Block mode: the matrix's own storage.  Reference layout
 * (MatrixFSUseReferenceLayout): a scratch block array filled from the four sub-matrix arrays, written back by block_done --
 * *scratch says which.  Anything else is not the (u,p) matrix of main.c:374-391: message + trap, as the reference's guards. */
static const CSRAttr* block_pattern(Matrix* J, value_type** val, b32* scratch) {
    *val = MatrixFSBlockValues(J);
    *scratch = FALSE;
    if (!*val) {
        *val = DflMatrixFSScratchBlockBegin(J);
        *scratch = *val != NULL;
    }
    if (!*val) {
        fprintf(stderr, "AssembleSystemTet: J must be the (u,p) field-split matrix of src/main.c:374-391 after MatrixSetup\n");
        ASSERT(FALSE);
        return NULL;
    }
    return ((MatrixFS*)J->data)->spy1x1;
}
static void block_done(Matrix* J, b32 scratch) {
    if (scratch) DflMatrixFSScratchBlockEnd(J);
}

/* (elem,a,b) -> nonzero map for this pattern, batch order; built once per (mesh, pattern) */
static void ensure_nzmap(Mesh3D* mesh, const CSRAttr* spy) {
    MeshExt* x = (MeshExt*)mesh->ext;
    if (x->nzmap_b && x->nzmap_attr == spy) return;
    CdamFreeDevice(x->nzmap_b, 0);
    x->nzmap_b = (index_type*)CdamMallocDevice((ptrdiff_t)mesh->num_tet * 16 * SIZE_OF(index_type));
    dfl_elem_nzmap(mesh->num_tet, x->ien_b, spy->row_ptr, spy->col_ind, x->nzmap_b, DflStream());
    x->nzmap_attr = spy;
}

f64* DflMeshNodeRecords(Mesh3D* mesh) {
    MeshExt* x = (MeshExt*)mesh->ext;
    if (!x->nodep) {
        const index_type N = Mesh3DNumNode(mesh);
        x->nodep = (f64*)CdamMallocDevice((ptrdiff_t)N * 16 * SIZE_OF(f64));
        x->nodexu = (f64*)CdamMallocDevice((ptrdiff_t)N * 8 * SIZE_OF(f64));
        x->Fp = (f64*)CdamMallocDevice((ptrdiff_t)N * 8 * SIZE_OF(f64));
    }
    return x->nodep;
}

/* The Jacobian schedule of this mesh for this pattern (mode 4), built on first use.  A builder that refuses the mesh --
 * it has printed why: a node patch beyond the kernel's slot / tet limits, too many patch colors -- makes the mesh FALL BACK
 * to schedule 1 (compact colors, the reference-shaped scatter) for good instead of trapping.  Returns the mode in force. */
static int ensure_lhs_schedule(Mesh3D* mesh, const CSRAttr* spy) {
    MeshExt* x = (MeshExt*)mesh->ext;
    if (x->cfg.sched_mode != 4) return x->cfg.sched_mode;
    if (x->slotpatch && x->slotpatch->attr != spy) { DflFreeSlotPatchSchedule(x->slotpatch); x->slotpatch = NULL; }
    if (!x->slotpatch) x->slotpatch = DflBuildSlotPatchSchedule(mesh, spy, x->cfg.slot_leaf, x->cfg.slot_cap, x->cfg.slot_tets);
    if (!x->slotpatch) {
        fprintf(stderr, "dedflow: assembly schedule 4 is not available for this mesh; falling back to schedule 1 (compact colors)\n");
        x->cfg.sched_mode = 1;
    }
    return x->cfg.sched_mode;
}

void AssembleSystemTet(Mesh3D* mesh, f64* wgalpha_dptr, f64* dwgalpha_dptr, f64* F, Matrix* J) {
    DflAssembleSystemTetBeta(mesh, wgalpha_dptr, dwgalpha_dptr, F, J, 1.0);
}

void DflAssembleSystemTetBeta(Mesh3D* mesh, f64* wgalpha_dptr, f64* dwgalpha_dptr, f64* F, Matrix* J, f64 beta_J) {
    MeshExt* x = (MeshExt*)mesh->ext;
    const Mesh3DData* dev = Mesh3DDevice(mesh);
    const index_type N = Mesh3DNumNode(mesh);
    hipStream_t s = DflStream();
    ASSERT((F || J) && "Either F or J should be provided");
    ASSERT(x && x->ien_b && "Mesh3DGenerateColorBatch must run before assembly");
    if (!g_quiet) printf("Assemble: %s %s\n", F ? "F" : "", J ? "J" : "");
    value_type* val = NULL;
    const CSRAttr* spy = NULL;
    b32 scratch = FALSE;
    if (J) {
        spy = block_pattern(J, &val, &scratch);
        const int before = x->cfg.sched_mode;
        if (ensure_lhs_schedule(mesh, spy) != before && beta_J == 0.0) {
            /* the caller counted on an overwriting schedule; the colored scatter adds */
            HIPGUARD(hipMemsetAsync(val, 0, (size_t)spy->nnz * 16 * sizeof(value_type), s));
            beta_J = 1.0;
        }
        if (x->cfg.sched_mode != 4) ensure_nzmap(mesh, spy);
    }
    /* packed gather records (one line per node) and packed residual accumulator */
    DflMeshNodeRecords(mesh);
    /* (the compact (x, u) copy only when a Jacobian follows: the residual kernels read the full records) */
    const b32 slot_lhs = J && x->cfg.sched_mode == 4;
    const b32 patch_rhs = F && x->cfg.sched_mode == 4;
    /* Who reads which records: the slot-owner J kernel only the compact (x, u) ones, every other element kernel the full
       ones; a Jacobian-only call on the default schedule therefore packs only the compact records. */
    const b32 need_full = F || (J && !slot_lhs);
    if (!x->nodep_current)
        dfl_pack_nodes2(N, dev->xg, wgalpha_dptr, dwgalpha_dptr, need_full ? x->nodep : NULL, slot_lhs ? x->nodexu : NULL, s);
    if (J && !slot_lhs && !x->egeo_b) { /* geometry cache in schedule order (static mesh), built once; the LHS kernels read it */
        x->egeo_b = (f64*)CdamMallocDevice((ptrdiff_t)mesh->num_tet * 16 * SIZE_OF(f64));
        dfl_elem_geometry(mesh->num_tet, x->ien_b, dev->xg, x->egeo_b, s);
    }
    /* one launch per class of the execution schedule (mesh.c: the reference's color batches in
       mode 0, the compact re-coloring otherwise) */
    for (index_type b = 0; b < x->sched_num; ++b) {
        const index_type off = x->sched_offset[b];
        const index_type bsz = x->sched_offset[b + 1] - off;
        if (bsz == 0) continue;
        const index_type* ien_b = x->ien_b + (size_t)off * 4;
        if (F && !patch_rhs) DFL_TIMED(DFL_TAG_ASM_RHS, dfl_assemble_tet_rhs_dt(bsz, ien_b, x->nodep, x->Fp, &x->step, s));
        if (J && !slot_lhs)
            DFL_TIMED(DFL_TAG_ASM_LHS, dfl_assemble_tet_lhs_dt(bsz, ien_b, x->nzmap_b + (size_t)off * 16, x->egeo_b + (size_t)off * 16,
                                                               x->nodep, val, &x->step, s));
    }
    if (slot_lhs) { /* schedule 4: ONE launch, every nodal nonzero is summed in registers by its owner lanes (host/slotpatch.c) */
        const SlotPatchSched* ss = x->slotpatch;
        DFL_TIMED(DFL_TAG_ASM_LHS, dfl_assemble_tet_lhs_slot_dt(ss->num_patch, ss->d_hdr, ss->d_ptet_lid, ss->d_pnode, ss->d_slot_nz, ss->d_ldesc,
                                                                x->nodexu, val, beta_J, ss->max_tets, &x->step, s));
    }
    if (patch_rhs) { /* schedule 4: patch-staged residual, two launches, fixed summation order (host/patch.c) */
        if (!x->rhspatch) x->rhspatch = DflBuildRhsPatchSchedule(mesh);
        const RhsPatchSched* rp = x->rhspatch;
        int slot = DflProfileBegin(DFL_TAG_ASM_RHS);
        dfl_assemble_tet_rhs_lane_dt(rp->num_patch, rp->d_cnt, rp->d_pnode, rp->d_lien, rp->d_sub4, rp->d_sub_start, x->nodep,
                                     rp->d_partial, &x->step, s);
        dfl_rhs_node_sum(N, rp->d_goff, rp->d_gidx, rp->d_partial, F, s);
        DflProfileEnd(slot);
    } else if (F) {
        dfl_unpack_rhs(N, x->Fp, F, s);
    }
    if (J) block_done(J, scratch);
}

void AssembleSystemTetFace(Mesh3D* mesh, f64* wgalpha_dptr, f64* dwgalpha_dptr, f64* F, Matrix* J) {
    const index_type group = ((MeshExt*)mesh->ext)->cfg.face_group; /* 4 in the reference, hard-coded at assemble.cu:1826-1828 */
    const Mesh3DData* dev = Mesh3DDevice(mesh);
    const index_type N = Mesh3DNumNode(mesh);
    hipStream_t s = DflStream();
    if (mesh->num_bound <= group) return;
    DflMeshPrepareFaces(mesh, group);
    MeshExt* x = (MeshExt*)mesh->ext;
    value_type* val = NULL;
    const CSRAttr* spy = NULL;
    b32 scratch = FALSE;
    if (J) spy = block_pattern(J, &val, &scratch);
    const index_type* f2e = Mesh3DBoundF2E(mesh, group);
    const index_type* forn = Mesh3DBoundFORN(mesh, group);
    int slot = DflProfileBegin(DFL_TAG_FACE);
    if (spy) DflMeshPrepareFaceNonzeros(mesh, group, spy);
    /* pass 1: every face parks its terms; pass 2: ordered sums into F and the block values */
    dfl_assemble_face_park_dt(x->face_nf, f2e, forn, dev->ien, N, dev->xg, wgalpha_dptr, dwgalpha_dptr, F ? x->face_pF : NULL,
                              spy ? x->face_pJ : NULL, &x->step, s);
    if (F) dfl_face_sum_F(x->face_nn, x->face_node, x->face_node_off, x->face_node_ent, x->face_pF, N, F, s);
    if (spy) dfl_face_sum_J(x->face_nnz, x->face_nz, x->face_nz_off, x->face_nz_ent, x->face_pJ, val, s);
    DflProfileEnd(slot);
    if (J) block_done(J, scratch);
}

void AssembleSystem(Mesh3D* mesh, f64* wgalpha, f64* dwgalpha, f64* F, Matrix* J, Dirichlet** bcs, index_type nbc) {
    DflAssembleSystemPrepacked(mesh, wgalpha, dwgalpha, F, J, bcs, nbc, FALSE);
}

void DflAssembleSystemPrepacked(Mesh3D* mesh, f64* wgalpha, f64* dwgalpha, f64* F, Matrix* J, Dirichlet** bcs, index_type nbc,
                                b32 prepacked) {
    index_type num_node = Mesh3DNumNode(mesh);
    MeshExt* x = (MeshExt*)mesh->ext;
    x->nodep_current = prepacked && x->nodep != NULL;
    hipStream_t s = DflStream();
    DflRangePush(F && J ? "AssembleSystem(F,J)" : F ? "AssembleSystem(F)" : "AssembleSystem(J)");
    if (F) HIPGUARD(hipMemsetAsync(F, 0, (size_t)num_node * sizeof(f64) * BS, s));
    /* schedule 4 writes every row of J exactly once: the zero pass folds into that write */
    if (J && Mesh3DNumTet(mesh) && MatrixFSBlockValues(J) && x->cfg.sched_mode == 4)
        (void)ensure_lhs_schedule(mesh, ((MatrixFS*)J->data)->spy1x1); /* may fall back to schedule 1: decides `overwrite` */
    const b32 overwrite = J && x->cfg.sched_mode == 4 && Mesh3DNumTet(mesh) && MatrixFSBlockValues(J);
    if (J && !overwrite) MatrixZero(J);
    if (Mesh3DNumTet(mesh)) {
        DflAssembleSystemTetBeta(mesh, wgalpha, dwgalpha, F, J, overwrite ? 0.0 : 1.0);
        AssembleSystemTetFace(mesh, wgalpha, dwgalpha, F, J);
    }
    /* external force on the momentum equations (particle reaction, include/dedflow.h): R = (...) - f_ext, after the tet and
       face terms and before the Dirichlet rows */
    if (F && x->ext_load) dfl_daxpy(3 * num_node, -1.0, x->ext_load, F, s);
    /* volume source on the continuity rows (melt-pool capture, include/dedflow.h): R_p = (...) - q_V, explicit as the load */
    if (F && x->vol_source) dfl_daxpy(num_node, -1.0, x->vol_source, F + 3 * (size_t)num_node, s);
    /* heat source on the T rows (particle heat, include/dedflow.h): R_T = (...) - q, before the rows are captured */
    if (F && x->heat_source) dfl_daxpy(num_node, -1.0, x->heat_source, F + 5 * (size_t)num_node, s);
    /* phase change (include/dedflow.h): the drag D u on the momentum rows and fact2 D on J's diagonal blocks, the latent term
       H dT on the T rows, before those rows are captured and before the Dirichlet rows */
    if (x->phase) DflPhaseApplySystem(mesh, wgalpha, dwgalpha, F, J, prepacked);
    /* thermal material (include/dedflow.h): the T rows' correction to k_q and c_q, after the phase-change rows and before the
       rows are captured; launched only when the scalar transport advances T */
    if (F && x->thermal) DflThermalApplyRows(mesh, wgalpha, dwgalpha, F);
    /* fluid material (include/dedflow.h): the (u,p) rows' correction to rho_q, mu_q and the body force on F, the matching
       difference blocks on J after the phase-change diagonal; both before the Dirichlet rows */
    if (x->fluid) DflFluidApplySystem(mesh, wgalpha, dwgalpha, F, J);
    x->nodep_current = FALSE;
    if (F && x->scalar) DflScalarCaptureResidual(mesh, F); /* the phi / T rows, kept for the scalar transport (host/scalar.c) */
    if (F) HIPGUARD(hipMemsetAsync(F + 4 * (size_t)num_node, 0, (size_t)num_node * sizeof(f64) * 2, s)); /* main.c:63-66 */
    for (index_type ibc = 0; ibc < nbc; ++ibc) {
        if (F) DirichletApplyVec(bcs[ibc], F);
        if (J) DirichletApplyMat(bcs[ibc], J);
    }
    DflRangePop();
}
