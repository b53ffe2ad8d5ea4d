/* dedflow.h -- host-side object API of the MI355X implementation of DEDFlow's
 * per-timestep hot path.  One consolidated header that keeps the names,
 * argument meaning and struct prefixes of the reference's public headers so a
 * caller written against them (src/main.c) compiles against this library:
 *
 *   common.h:20-111   scalar typedefs, ASSERT/CEIL_DIV, Init/Finalize, GlobalContextGet
 *   alloc.h:19-36     Allocator vtable, CdamMalloc{Host,Device}/CdamFree{Host,Device}
 *   MeshData.h:10-36  Mesh3DData           Mesh.h:14-73   Mesh3D
 *   csr.h:14-36       CSRAttr              matrix.h:27-147 Matrix / MatrixOp / MatrixCSR / MatrixFS
 *   vec.h:7-10        Vec*                 dirichlet.h:8-33 Dirichlet
 *   pc.h:15-88        PC tree              krylov.h:12-30  Krylov
 *   assemble.h:13-14  AssembleSystemTet / AssembleSystemTetFace
 *   Array.h:11-39 / Particle.h:13-35       Array, ParticleContext
 *
 * Differences a caller can observe (all listed in INTEGRATION.md):
 *   - cudaStream_t fields are hipStream_t.
 *   - A MatrixFS holding the reference's (u,p) 2x2 layout stores ONE shared-pattern
 *     array of 4x4 blocks (include/dedflow_kernels.h); sub-matrix `val` arrays in the
 *     reference layout are materialised only by MatrixFSExportSubmatrices().
 *   - structs end with one extra `ext` pointer owned by the library.
 *   - expanded patterns have a correct last row_ptr entry (reference bug Q3).
 * No status returns, guard-and-trap error behaviour, caller-owned buffers, one
 * host thread: as in the reference.
 */
#ifndef DEDFLOW_H
#define DEDFLOW_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- scalars (common.h:20-66) ------------------------------------------------- */
typedef int8_t i8;
typedef int16_t i16;
typedef int32_t i32;
typedef int64_t i64;
typedef uint8_t u8;
typedef uint16_t u16;
typedef uint32_t u32;
typedef uint64_t u64;
typedef float f32;
typedef double f64;
typedef char byte;
typedef f64 value_type;  /* -DUSE_F64_VALUE */
typedef i32 index_type;  /* -DUSE_I32_INDEX */
typedef int32_t b32;
typedef i32 color_t;
#ifndef TRUE
#define TRUE (1 == 1)
#define FALSE (1 == 0)
#endif
#define SIZE_OF(x) ((index_type)sizeof(x))
#define CEIL_DIV(a, b) (((a) + (b)-1) / (b))
#define UNUSED(args) ((void)(args))
#if defined(NDEBUG)
#define ASSERT(expr) /* empty */
#else
#define ASSERT(expr) \
    while (!(expr)) __builtin_trap()
#endif
typedef hipMemcpyKind MemCopyKind;
#define H2D (hipMemcpyHostToDevice)
#define D2H (hipMemcpyDeviceToHost)
#define D2D (hipMemcpyDeviceToDevice)
#define H2H (hipMemcpyHostToHost)
void DflGuardPrivate(hipError_t code, const char* file, int line);
#define HIPGUARD(err) DflGuardPrivate((err), __FILE__, __LINE__)

#define UNCOLORED (0x0)
#define MAX_COLOR (1 << 8)

/* ---- runtime (common.h:103-111, alloc.h) --------------------------------------- */
void Init(int argc, char** argv);
void Finalize(void);
typedef enum GlobalContextType { GLOBAL_CONTEXT_SPARSE_HANDLE = 0, GLOBAL_CONTEXT_BLAS_HANDLE = 1 } GlobalContextType;
/* the reference returns cuSPARSE/cuBLAS handles here; this library has no vendor
 * handles -- both slots return a pointer to the hipStream_t every launcher uses. */
void* GlobalContextGet(GlobalContextType type);
hipStream_t DflStream(void);
void DflSetStream(hipStream_t s);

typedef enum DeviceType { HOST = 0, DEVICE = 1 } DeviceType;
typedef void* UserCtxPtr;
typedef struct Allocator {
    void* (*malloc)(ptrdiff_t, UserCtxPtr);
    void (*free)(void*, ptrdiff_t, UserCtxPtr);
    UserCtxPtr ctx;
} Allocator;
Allocator* GetDefaultAllocator(int device_id);
#define CdamMallocHost(count) (GetDefaultAllocator(HOST)->malloc((ptrdiff_t)(count), GetDefaultAllocator(HOST)->ctx))
#define CdamFreeHost(ptr, count) (GetDefaultAllocator(HOST)->free(ptr, (ptrdiff_t)(count), GetDefaultAllocator(HOST)->ctx))
#define CdamMallocDevice(count) (GetDefaultAllocator(DEVICE)->malloc((ptrdiff_t)(count), GetDefaultAllocator(DEVICE)->ctx))
#define CdamFreeDevice(ptr, count) (GetDefaultAllocator(DEVICE)->free(ptr, (ptrdiff_t)(count), GetDefaultAllocator(DEVICE)->ctx))
/* the two macros above as functions, for bindings that cannot expand C macros (zero-filled, pooled: host/runtime.c) */
void* DflDeviceMalloc(int64_t bytes);
void DflDeviceFree(void* ptr);

/* ---- mesh (MeshData.h, Mesh.h) --------------------------------------------------- */
typedef struct H5FileInfo H5FileInfo;
typedef struct Mesh3DData {
    b32 is_host;
    index_type num_node, num_tet, num_prism, num_hex;
    f64* xg;         /* xg[3*num_node] */
    index_type* ien; /* ien[4*num_tet + 6*num_prism + 8*num_hex] */
} Mesh3DData;
#define Mesh3DDataNumNode(data) ((data)->num_node)
#define Mesh3DDataNumTet(data) ((data)->num_tet)
#define Mesh3DDataNumPrism(data) ((data)->num_prism)
#define Mesh3DDataNumHex(data) ((data)->num_hex)
#define Mesh3DDataCoord(data) ((data)->xg)
#define Mesh3DDataIEN(data) ((data)->ien)
#define Mesh3DDataTet(data) (Mesh3DDataNumTet(data) ? (data)->ien + 0 : NULL)
Mesh3DData* Mesh3DDataCreateHost(index_type num_node, index_type num_tet, index_type num_prism, index_type num_hex);
Mesh3DData* Mesh3DDataCreateDevice(index_type num_node, index_type num_tet, index_type num_prism, index_type num_hex);
void Mesh3DDataDestroy(Mesh3DData* data);
void Mesh3DDataCopy(Mesh3DData* dst, Mesh3DData* src, MemCopyKind kind);
Mesh3DData* Mesh3DDataCreateH5(H5FileInfo* h5f, const char* group_name); /* MeshData.c:57-109; in libdedflow_h5.so */

typedef struct Mesh3D {
    index_type num_node, num_tet, num_prism, num_hex;
    Mesh3DData* host;
    Mesh3DData* device;
    index_type num_bound;
    index_type* bound_fid;
    index_type* bound_node_offset; /* host */
    index_type* bound_node;        /* device */
    index_type* bound_elem_offset; /* host */
    index_type* bound_ien;
    index_type* bound_f2e;  /* device */
    index_type* bound_forn; /* device */
    index_type num_batch;
    index_type* batch_offset; /* host */
    index_type* batch_ind;    /* device */
    color_t num_color;
    color_t* color; /* device */
    void* ext;      /* library-owned: batch-ordered ien, (elem,a,b)->nz map, face lists */
} Mesh3D;
#define Mesh3DHost(mesh) ((mesh)->host)
#define Mesh3DDevice(mesh) ((mesh)->device)
#define Mesh3DNumNode(mesh) ((mesh)->num_node)
#define Mesh3DNumTet(mesh) ((mesh)->num_tet)
#define Mesh3DNumPrism(mesh) ((mesh)->num_prism)
#define Mesh3DNumHex(mesh) ((mesh)->num_hex)
#define Mesh3DBoundNumNode(mesh, i) ((mesh)->bound_node_offset[(i) + 1] - (mesh)->bound_node_offset[(i)])
#define Mesh3DBoundNode(mesh, i) ((mesh)->bound_node + (mesh)->bound_node_offset[(i)])
#define Mesh3DBoundNumElem(mesh, i) ((mesh)->bound_elem_offset[(i) + 1] - (mesh)->bound_elem_offset[(i)])
#define Mesh3DBoundF2E(mesh, i) ((mesh)->bound_f2e + (mesh)->bound_elem_offset[(i)])
#define Mesh3DBoundFORN(mesh, i) ((mesh)->bound_forn + (mesh)->bound_elem_offset[(i)])
Mesh3D* Mesh3DCreate(index_type num_node, index_type num_tet, index_type num_prism, index_type num_hex);
Mesh3D* Mesh3DCreateH5(H5FileInfo* h5f, const char* group_name);
void Mesh3DDestroy(Mesh3D* mesh);
void Mesh3DUpdateHost(Mesh3D* mesh);
void Mesh3DUpdateDevice(Mesh3D* mesh);
void Mesh3DColor(Mesh3D* mesh);
void Mesh3DGenerateColorBatch(Mesh3D* mesh);
/* boundary groups from host arrays (the reference only fills them from HDF5, Mesh.c:12-59) */
void Mesh3DSetBound(Mesh3D* mesh, index_type num_bound, const index_type* node_offset, const index_type* node,
                    const index_type* elem_offset, const index_type* f2e, const index_type* forn);
void ColorMeshTet(const Mesh3D* mesh, index_type max_color_len, color_t* color);
color_t GetMaxColor(const color_t* color, index_type num_elem);

/* ---- HDF5 formats (h5util.h:24-58; implemented in libdedflow_h5.so, dedflow_amd/h5/h5io.c) ----- */
H5FileInfo* H5OpenFile(const char* filename, const char* mode);
void H5CloseFile(H5FileInfo* h5file);
b32 H5FileIsReadable(H5FileInfo* h5file);
b32 H5FileIsWritable(H5FileInfo* h5file);
b32 H5DatasetExist(H5FileInfo* h5file, const char* dataset_name);
void H5GetDatasetSize(H5FileInfo* h5file, const char* dataset_name, index_type* size);
void H5ReadDatasetf64(H5FileInfo* h5file, const char* dataset_name, f64* data);
void H5ReadDatasetInd(H5FileInfo* h5file, const char* dataset_name, index_type* data);
void H5WriteDatasetf64(H5FileInfo* h5file, const char* dataset_name, index_type len, const f64* data);
void H5WriteDatasetInd(H5FileInfo* h5file, const char* dataset_name, index_type len, const index_type* data);
/* mesh writer in the schema tools/mesh_convert.py:116-126 produces; solution files of main.c:521-532,571-590 */
void DflMeshWriteH5(H5FileInfo* f, const char* group, index_type N, index_type T, const f64* xg, const index_type* ien,
                    index_type nb, const index_type* node_offset, const index_type* node, const index_type* elem_offset,
                    const index_type* bien, const index_type* f2e, const index_type* forn);
void DflSolutionWriteH5(const char* filename, index_type N, const f64* d_wgold, const f64* d_dwgold);
void DflSolutionReadH5(const char* filename, index_type N, f64* d_wgold, f64* d_dwgold);

/* ---- sparsity (csr.h) ------------------------------------------------------------ */
typedef index_type csr_index_type;
typedef struct CSRAttr CSRAttr;
struct CSRAttr {
    index_type num_row, num_col, nnz;
    index_type* row_ptr; /* device */
    index_type* col_ind; /* device */
    const CSRAttr* parent;
    index_type* diag_pos; /* device, [num_row]: the stored diagonal of every row of a nodal pattern (CSRAttrCreate); NULL: not built */
};
#define CSRAttrNumRow(attr) ((attr)->num_row)
#define CSRAttrNumCol(attr) ((attr)->num_col)
#define CSRAttrNNZ(attr) ((attr)->nnz)
#define CSRAttrRowPtr(attr) ((attr)->row_ptr)
#define CSRAttrColInd(attr) ((attr)->col_ind)
CSRAttr* CSRAttrCreate(const Mesh3D* mesh);
void CSRAttrDestroy(CSRAttr* attr);
CSRAttr* CSRAttrCreateBlock(const CSRAttr* attr, csr_index_type block_row, csr_index_type block_col);
/* csr.h:32-36.  The reference reads attr->row_ptr (a device pointer) on the host in the first two; here they copy the
 * 4 / 8 bytes they need back.  CSRAttrRow returns a DEVICE pointer into col_ind. */
index_type CSRAttrLength(CSRAttr* attr, csr_index_type row);
csr_index_type* CSRAttrRow(CSRAttr* attr, csr_index_type row);
void CSRAttrGetNonzeroIndBatched(const CSRAttr* attr, csr_index_type batch_size, const index_type* row, const index_type* col,
                                 index_type* ind);
/* csr_impl.h:6-9 */
void ExpandCSRByBlockSize(const CSRAttr* attr, CSRAttr* new_attr, csr_index_type block_size[2]);
void CSRAttrGetNZIndBatchedGPU(const CSRAttr* attr, csr_index_type batch_size, const index_type* row, const index_type* col,
                               csr_index_type* ind);

/* ---- matrices (matrix.h) --------------------------------------------------------- */
typedef enum MatType { MAT_TYPE_NONE = 0, MAT_TYPE_DENSE = 1, MAT_TYPE_CSR = 2, MAT_TYPE_FS = 4, MAT_TYPE_CUSTOM = 8 } MatType;
typedef struct Matrix Matrix;
typedef struct MatrixOp {
    void (*setup)(Matrix* matrix);
    void (*zero)(Matrix* matrix);
    void (*zero_row)(Matrix* matrix, index_type, const index_type* row, index_type shift, value_type diag);
    void (*amvpby)(Matrix* A, value_type alpha, value_type* x, value_type beta, value_type* y);
    void (*amvpby_mask)(Matrix* A, value_type alpha, value_type* x, value_type beta, value_type* y, value_type* left_mask,
                        value_type* right_mask);
    void (*matvec)(Matrix* matrix, value_type* x, value_type* y);
    void (*matvec_mask)(Matrix* matrix, value_type* x, value_type* y, value_type* left_mask, value_type* right_mask);
    void (*get_diag)(Matrix* matrix, value_type* diag, index_type bs);
    void (*set_values_coo)(Matrix* matrix, value_type alpha, index_type n, const index_type* row, const index_type* col,
                           const value_type* val, value_type beta);
    void (*set_values_ind)(Matrix* matrix, value_type alpha, index_type n, const index_type* ind, const value_type* val,
                           value_type beta);
    void (*add_elem_value_batched)(Matrix* matrix, index_type nshl, index_type batch_size, const index_type* batch_ptr,
                                   const index_type* ien, const value_type* val, const index_type* mask);
    void (*add_elem_value_blocked_batched)(Matrix* matrix, index_type nshl, index_type batch_size, const index_type* batch_ptr,
                                           const index_type* ien, index_type block_row_size, index_type block_col_size,
                                           const value_type* val, int lda, int stride, const index_type* mask);
    void (*add_value_batched)(Matrix* matrix, index_type batch_size, const index_type* batch_row_ind,
                              const index_type* batch_col_ind, const value_type* A);
    void (*add_value_blocked_batched)(Matrix* matrix, index_type batch_size, const index_type* batch_row_ind,
                                      const index_type* batch_col_ind, index_type block_row, index_type block_col,
                                      const value_type* A, int lda, int stride);
    void (*destroy)(Matrix* matrix);
} MatrixOp;
struct Matrix {
    index_type size[2];
    MatType type;
    void* data;
    hipStream_t stream_ref;
    MatrixOp op[1];
};
#define MatrixNumRow(A) ((A)->size[0])
#define MatrixNumCol(A) ((A)->size[1])
#define MatrixType(A) ((A)->type)
typedef struct MatrixFS MatrixFS;
typedef struct MatrixCSR {
    b32 external_attr;
    const CSRAttr* attr;
    value_type* val; /* reference-layout values; NULL while the matrix is a view into a block-mode MatrixFS */
    void* descr;     /* unused (cusparseSpMatDescr_t in the reference) */
    index_type buffer_size;
    void* buffer;
    /* ext */
    MatrixFS* owner;       /* block-mode parent, or NULL */
    index_type owner_slot; /* i * n_offset + j inside the parent */
} MatrixCSR;
struct MatrixFS {
    index_type n_offset;
    index_type* offset;
    index_type* d_offset;
    hipStream_t* stream;
    const CSRAttr* spy1x1;
    value_type** d_matval;
    Matrix** mat;
    /* ext */
    b32 block_mode;        /* the (u,p) 2x2 layout of src/main.c:374-391 was recognised */
    value_type* block_val; /* [nnz1][16] device, 4x4 blocks over spy1x1 */
    index_type owned_rows; /* node rows this rank owns (== spy1x1->num_row on one GPU): SpMV / PC run on these only */
    b32 reference_layout;  /* MatrixFSUseReferenceLayout: keep the four row-expanded sub-matrix arrays (no block mode) */
    b32 block_val_heap;    /* block_val is a plain hipMalloc block (moved out of the allocator's pool by the Krylov placement
                              calibration, host/solver.c) -- MatrixDestroy frees it accordingly */
    value_type* x4;        /* [num_row][4] interleaved copy of the matvec's input (dfl_bcsr_spmv_x4), allocated on first use */
    b32 x4_pool;           /* x4 came from the allocator's pool (DFL_X4_POOL=1) rather than from hipMalloc */
};
Matrix* MatrixCreateTypeCSR(const CSRAttr* attr, void*);
Matrix* MatrixCreateTypeFS(index_type n_offset, const index_type* offset, void*);
void MatrixDestroy(Matrix* matrix);
void MatrixSetup(Matrix* matrix);
void MatrixZero(Matrix* matrix);
void MatrixZeroRow(Matrix* matrix, index_type n, const index_type* row, index_type shift, value_type diag);
void MatrixAMVPBY(Matrix* A, value_type alpha, value_type* x, value_type beta, value_type* y);
void MatrixAMVPBYWithMask(Matrix* A, value_type alpha, value_type* x, value_type beta, value_type* y, value_type* left_mask,
                          value_type* right_mask);
void MatrixMatVec(Matrix* matrix, value_type* x, value_type* y);
/* block-mode (u,p) MatrixFS: the interleaved scratch the matvec gathers from (allocated on first call), and y = A x with the
 * scratch already filled by the caller for all columns the rows [row0, row1) read (dfl_interleave4, or a producer that
 * writes both layouts, e.g. dfl_pc_jacobi_apply_scaled_rows_x4) */
value_type* DflMatrixFSInterleavedScratch(Matrix* matrix);
void DflMatrixFSMatVecX4Range(Matrix* matrix, const value_type* x4, value_type* y, index_type row0, index_type row1);
/* ... with the output divided by the device scalar *d_nrm: y = (A x4) * (1 / *d_nrm) */
void DflMatrixFSMatVecX4RangeScaled(Matrix* matrix, const value_type* x4, const value_type* d_nrm, value_type* y, index_type row0,
                                    index_type row1);
/* y = A x4 over all rows -- d_nrm != NULL: times 1 / *d_nrm -- and z4_out[row][4] = M^-1 y_row of the block-Jacobi tree, written by
 * the row group that forms y_row (dfl_bcsr_spmv_x4_pc); needs the pattern's diag_pos and z4_out != x4 */
void DflMatrixFSMatVecX4Pc(Matrix* matrix, const value_type* x4, const value_type* d_nrm, value_type* y, value_type* z4_out);
void MatrixMatVecWithMask(Matrix* matrix, value_type* x, value_type* y, value_type* left_mask, value_type* right_mask);
void MatrixGetDiag(Matrix* matrix, value_type* diag, index_type bs);
void MatrixSetValuesCOO(Matrix* matrix, value_type alpha, index_type n, const index_type* row, const index_type* col,
                        const value_type* val, value_type beta);
void MatrixSetValuesInd(Matrix* matrix, value_type alpha, index_type n, const index_type* ind, const value_type* val,
                        value_type beta);
void MatrixAddElemValueBatched(Matrix* matrix, index_type nshl, index_type num_batch, const index_type* batch_ptr,
                               const index_type* ien, const value_type* val, const index_type* mask);
/* the reference's live LHS scatter entry point (assemble.cu:253-271): one batch = one color; val holds one lda-strided
 * block per (batch slot, a, b), `stride` values apart.  On the (u,p) MatrixFS the rows / columns 0..3 of every block go
 * into the 4x4 block array (block mode) or through SetBlockValueToSubmatGPU into the four sub-matrices. */
void MatrixAddElemValueBlockedBatched(Matrix* matrix, index_type nshl, index_type num_batch, const index_type* batch_ptr,
                                      const index_type* ien, index_type block_row_size, index_type block_col_size,
                                      const value_type* val, int lda, int stride, const index_type* mask);
void MatrixAddValueBatched(Matrix* matrix, index_type batch_size, const index_type* batch_row_ind, const index_type* batch_col_ind,
                           const value_type* A);
void MatrixAddValueBlockedBatched(Matrix* matrix, index_type batch_size, const index_type* batch_row_ind,
                                  const index_type* batch_col_ind, index_type block_row_size, index_type block_col_size,
                                  const value_type* A, int lda, int stride);
/* matrix.h:141-147 */
MatrixCSR* MatrixCSRCreate(const CSRAttr* attr, void*);
void MatrixCSRDestroy(Matrix* matrix);
MatrixFS* MatrixFSCreate(index_type n_offset, const index_type* offset, void*);
void MatrixFSDestroy(Matrix* matrix);
/* call before MatrixSetup: keep the reference's storage (four row-expanded CSR value arrays, per-sub-matrix loops of
 * matrix.c:449-551) instead of the 4x4 block array -- for hosts that write into MatrixCSR.val themselves */
void MatrixFSUseReferenceLayout(Matrix* matrix, b32 on);
/* block-mode helpers (not in the reference) */
value_type* MatrixFSBlockValues(Matrix* matrix); /* NULL unless block mode */
/* fills the four sub-matrices' `val` arrays (reference layout) from the block storage, allocating them on first use */
void MatrixFSExportSubmatrices(Matrix* matrix);
void MatrixFSImportSubmatrices(Matrix* matrix);
/* element-partitioned runs: local nodes are numbered owned-first; rows >= n are ghost rows */
void MatrixFSSetOwnedRows(Matrix* matrix, index_type n);
/* y = A x on node rows [row0, row1) of the block-mode (u,p) system only */
void MatrixFSMatVecRange(Matrix* matrix, value_type* x, value_type* y, index_type row0, index_type row1);
index_type MatrixFSOwnedRows(Matrix* matrix);
/* recursive coordinate bisection of tet centroids into num_part parts (the reference's METIS
 * wrapper, src/partition.c:16-77, is dead code and METIS is unavailable): epart[T] on the host */
void DflPartitionRCB(index_type num_tet, const index_type* ien, const f64* xg, index_type num_part, index_type* epart);

/* ---- vectors (vec.h) --------------------------------------------------------------- */
void VecAXPY(value_type a, const value_type* x, value_type* y, index_type n);
void VecPointwiseMult(const value_type* x, const value_type* y, value_type* z, index_type n);
void VecPointwiseDiv(const value_type* x, const value_type* y, value_type* z, index_type n);
void VecPointwiseInv(value_type* x, index_type n);

/* ---- Dirichlet (dirichlet.h) --------------------------------------------------------- */
typedef enum BCType { BC_NONE = 0, BC_STRONG = 1, BC_WEAK = 2, BC_OUTFLOW = 4 } BCType;
typedef struct Dirichlet {
    const Mesh3D* mesh;
    index_type face_ind;
    index_type shape;
    size_t buffer_size;
    void* buffer;
    BCType bctype[];
} Dirichlet;
Dirichlet* DirichletCreate(const Mesh3D* mesh, index_type face_ind, index_type shape);
void DirichletDestroy(Dirichlet* dirichlet);
void DirichletApplyVec(Dirichlet* dirichlet, value_type* b);
void DirichletApplyMat(Dirichlet* dirichlet, Matrix* A);

/* ---- preconditioners (pc.h) ---------------------------------------------------------- */
typedef enum PCType { PC_NONE = 0x0, PC_JACOBI = 0x1, PC_DECOMPOSITION = 0x2, PC_AMGX = 0x3, PC_CUSTOM = 0x4, PC_ILU0 = 0x5,
                      PC_TWOLEVEL = 0x6 } PCType;
typedef struct PC PC;
typedef struct PCOps {
    void (*setup)(PC*);
    void (*destroy)(PC*);
    void (*apply)(PC*, value_type*, value_type*);
} PCOps;
struct PC {
    PCType type;
    void* mat;
    PCOps op[1];
    void* data;
    void* cublas_handle; /* kept for layout compatibility; unused */
};
typedef struct PCNone { index_type n; } PCNone;
typedef struct PCJacobi { index_type n; index_type bs; void* diag; } PCJacobi;
typedef struct PCDecomposition { index_type n_sec; index_type* offset; PC** pc; void* ext; } PCDecomposition;
PC* PCCreateNone(Matrix* mat, index_type n);
PC* PCCreateJacobi(Matrix* mat, index_type bs, void* handle);
PC* PCCreateDecomposition(Matrix* mat, index_type n, const index_type* offset, void* handle);
/* PC_AMGX (host/pc_amgx.c, csrc/k_amgx.hip): a native scalar AMG in place of the NVIDIA AMGX library the reference links
 * (pc.c:160-235, 279-295): pairwise aggregation (SIZE_2/4/8), piecewise-constant P, Galerkin P^T A P, multicolour-DILU or
 * Jacobi smoothing, dense LU on the coarsest level (zero pivots skipped: singular coarsest matrices such as the Neumann
 * pressure block are fine), V-cycles from a zero initial guess.  `mat`: a MAT_TYPE_CSR matrix with its own values, or the
 * A11 view fs->mat[n_offset+1] of a block-mode (u,p) MatrixFS on one GPU.  `options`: NULL (the reference configuration of
 * krylov.c:413-437), an inline AMGX string "config_version=2, solver:preconditioner:smoother=..., ..." or the path of a file
 * holding that string or AMGX's JSON form.  Structure is built here from the current values; PCSetup recomputes every value,
 * PCAMGXRebuild the structure.  Returns NULL (with a message on stderr) for an unsupported matrix or option value.
 * The V-cycle is a fixed linear operator: plain (non-flexible) GMRES. */
PC* PCCreateAMGX(Matrix* mat, void* options);
typedef struct DflAMGXConfig {
    f64 relaxation_factor;
    int32_t selector_passes; /* SIZE_2 / SIZE_4 / SIZE_8: 1 / 2 / 3 pairwise passes per level */
    int32_t smoother;        /* DFL_AMGX_SMOOTHER_* */
    int32_t presweeps, postsweeps, max_levels, min_coarse_rows, max_iters;
    int32_t unknown_keys;    /* keys that were listed on stderr and ignored */
} DflAMGXConfig;
enum { DFL_AMGX_SMOOTHER_DILU = 0, DFL_AMGX_SMOOTHER_JACOBI = 1 };
int DflAMGXParseConfig(const char* options, DflAMGXConfig* cfg); /* host only; 0 = accepted */
/* host only: the aggregates PCCreateAMGX forms on a host CSR matrix (columns ascending) with `passes` pairwise passes;
 * agg_out[n]; returns the number of aggregates */
index_type DflAMGXAggregateHost(index_type n, const index_type* rp, const index_type* ci, const f64* val, int passes,
                                index_type* agg_out);
void PCAMGXRebuild(PC* pc);
index_type PCAMGXNumLevels(PC* pc);
/* per level (arrays of PCAMGXNumLevels entries, any may be NULL): rows, nonzeros, colours; operator complexity; the first
 * level of the one-workgroup tail; kernel launches of the last PCApply and the last PCSetup */
void PCAMGXInfo(PC* pc, index_type* rows, index_type* nnz, index_type* colors, f64* op_complexity, index_type* tail_level,
                int64_t* launches_apply, int64_t* launches_setup);
const index_type* PCAMGXLevelAggregates(PC* pc, index_type level); /* device [n_level]: row -> next-level row; NULL on the coarsest */
const index_type* PCAMGXLevelColors(PC* pc, index_type level);     /* device [n_level] */
Matrix* PCAMGXLevelMatrix(PC* pc, index_type level); /* MAT_TYPE_CSR over the level's values (current after PCSetup); owned by the PC */
const index_type* PCAMGXCoarsePivots(PC* pc); /* device [2 n_coarsest]: the LU's row exchanges, then 1 for pivots taken as zero */
/* PC_ILU0: multicolor block-DILU on the block-mode (u,p) matrix (host/pc_dilu.c, csrc/k_dilu.hip); build-defined:
 * the reference's PCType ends at PC_CUSTOM = 0x4 (pc.h:15-21); 0x5 and 0x6 are this build's additions.  KrylovSetPCType(ksp, PC_ILU0) makes KrylovSolve build it instead
 * of the reference's Jacobi tree (PC_DECOMPOSITION = the reference default). */
PC* PCCreateDILU(Matrix* mat);
void PCDILUSetActiveLength(PC* pc, index_type n_active);
/* sweeps read the off-diagonal blocks from a caller-kept single-precision copy (NULL = the matrix's own values); host/pc_dilu.c */
void PCDILUSetF32Values(PC* pc, const float* valf);
index_type PCDILUGetColors(PC* pc, u8* color_out);
const f64* PCDILUGetInverseBlocks(PC* pc);
/* PC_TWOLEVEL (host/pc_twolevel.c, csrc/k_amg.hip; build-defined, in the spirit of the AMGX aggregation configuration the
 * reference sketches at krylov.c:409-437): block-DILU smoothing plus a coarse-grid correction on node aggregates --
 * z = S r;  z += P Ac^-1 P^T (r - A z), P = piecewise constant over spatial aggregates of ~agg_size nodes (recursive
 * coordinate bisection of the mesh nodes), Ac = P^T A P (Galerkin, 4x4 blocks over the aggregate graph, rebuilt at every
 * PCSetup), Ac^-1 by a few inner Jacobi-GMRES iterations (rtol 0.1) -- hence the outer solver runs as FGMRES.  Iteration
 * counts become (nearly) independent of the mesh size: 50M tets converge in tens of iterations instead of ~600. */
PC* PCCreateTwoLevel(Matrix* mat, const Mesh3D* mesh, index_type agg_size);
/* the same on an element-partitioned matrix (owned rows first, MatrixFSSetOwnedRows): every rank aggregates the nodes it
 * owns, the Galerkin coarse matrix is assembled from the owned rows and REPLICATED (its values all-reduced at PCSetup, the
 * restricted residual all-reduced per application: one halo exchange + one all-reduce of 4 Nc doubles per apply), every rank
 * solves the same small coarse problem, the smoother is the rank-local DILU.  `comm` (copied) must carry rank / world;
 * NULL = PCCreateTwoLevel.  Collective: every rank of the partition calls it, and PCSetup / PCApply, together. */
struct DflComm;
PC* PCCreateTwoLevelDist(Matrix* mat, const Mesh3D* mesh, index_type agg_size, const struct DflComm* comm);
void PCTwoLevelSetActiveLength(PC* pc, index_type n_active);
void PCTwoLevelSetInner(PC* pc, index_type max_iter, f64 rtol); /* inner coarse solve: default 40 iterations, rtol 0.1 */
void PCTwoLevelInfo(PC* pc, index_type* num_aggregate, index_type* coarse_nnz, int64_t* inner_iterations);
const index_type* PCTwoLevelAggregates(PC* pc); /* device [N]: aggregate of every node (tests) */
Matrix* PCTwoLevelCoarseMatrix(PC* pc);          /* the Galerkin coarse matrix, a block-mode MatrixFS (tests) */
void PCSetup(PC* pc);
void PCDestroy(PC* pc);
void PCApply(PC* pc, f64* x, f64* y);

/* ---- Krylov (krylov.h) ---------------------------------------------------------------- */
typedef void (*KSPSolveFunc)(Matrix*, value_type*, value_type*, void*);
typedef struct Krylov {
    index_type max_iter;
    f64 atol, rtol;
    void* handle;
    KSPSolveFunc ksp_solve;
    size_t ksp_ctx_size;
    void* ksp_ctx;
    void* pc;
    void* ext; /* library-owned workspace + statistics (KrylovStats) */
} Krylov;
Krylov* KrylovCreateCG(index_type, f64, f64, void*);    /* stub in the reference (krylov.c:42-51); build-defined here */
Krylov* KrylovCreateGMRES(index_type, f64, f64, void*);
void KrylovDestroy(Krylov* krylov);
/* argument order of the DEFINITION and the call site (krylov.c:386, main.c:217): (ksp, A, x, b) -- Q10 */
void KrylovSolve(Krylov* krylov, Matrix* A, f64* x, f64* b);
typedef struct KrylovStats {
    index_type iterations;
    f64 rnrm_init;
    f64 res_hist[512]; /* |beta[k+1]| after iteration k */
    b32 converged;
    b32 fused_norm_cancelled; /* KrylovSetFusedNorm: an iteration kept < 1e-6 of w.w -- history unreliable */
    /* running totals since the solver was created (a Newton loop makes several solves per step) */
    index_type total_solves, total_converged;
    int64_t total_iterations;
} KrylovStats;
const KrylovStats* KrylovGetStats(const Krylov* krylov);
/* 0: GMRES tests convergence every 20 iterations like the reference (krylov.c:281-290); k>0: every k */
void KrylovSetCheckInterval(Krylov* krylov, index_type k);
void KrylovSetVerbose(Krylov* krylov, b32 verbose);
/* PC_DECOMPOSITION (default, reference tree), PC_ILU0, PC_TWOLEVEL or PC_AMGX.  PC_AMGX: on a (u,p) MatrixFS the reference
 * tree with pc[1] = PCCreateAMGX(A11, cfg) (the commented line krylov.c:450), on a MAT_TYPE_CSR matrix PCCreateAMGX(A, cfg);
 * cfg from KrylovSetAMGXConfig.  With a communicator, or when PCCreateAMGX returns NULL, the solver says so and builds what
 * it builds without PC_AMGX. */
void KrylovSetPCType(Krylov* krylov, PCType type);
void KrylovSetAMGXConfig(Krylov* krylov, const char* options); /* copied; NULL = the reference configuration */
PC* KrylovGetPC(const Krylov* krylov);
/* off by default: the norm of the orthogonalised vector from w.w - sum h_j^2, so that a partitioned Arnoldi step needs ONE
 * all-reduce (h and w.w together) instead of two and, with the Jacobi tree on <= 500k rows, ONE launch for update + Givens
 * step + next preconditioner application (7 -> 4 launches per step; since round 3 also without a communicator -- the
 * last-level solver of PC_TWOLEVEL uses it); rounding differs from the explicit norm and heavy cancellation raises
 * KrylovStats.fused_norm_cancelled */
void KrylovSetFusedNorm(Krylov* krylov, b32 on);
/* p(1)-pipelined GMRES (host/solver.c, gmres_pipelined; build-defined, off by default): ONE reduction per Arnoldi step -- the CGS
 * coefficients and w.w together, the norm from the Pythagorean identity -- overlapped with the matvec of the NEXT step through
 * the auxiliary basis z_{j+1} = A M^-1 v_j (Ghysels et al. 2013).  Hides the all-reduce latency of partitioned runs behind the
 * matvec (own stream with the RCCL communicator); costs a second basis, a third basis pass per step and some accuracy of the
 * residual history (~1e-8 r0 instead of 1e-10; heavy cancellation raises KrylovStats.fused_norm_cancelled).  Ignored with
 * FGMRES / PC_TWOLEVEL and with restarts. */
void KrylovSetPipelined(Krylov* krylov, b32 on);
/* which Arnoldi step the most recent unpipelined GMRES solve ran (0 reference, 1 two reductions, 2 fused norm, 3 fused update +
 * preconditioner, 4 raw basis: DESIGN.md section 3); -1 before the first solve or for another solver.  For tests and A/B runs */
int DflKrylovLastGmresStep(Krylov* krylov);
/* how that solve advanced: counts[s] = counted steps that took s iterations in one pass over the basis, s = 1..4 (counts[0] is 0),
   and whether one of them raised a flag: bit 0, a new vector lost more than four digits in the orthogonalisation; bit 1, a block
   whose update and fix-up ran as one pass formed vectors less orthogonal to each other than 9.3e-6 */
void DflKrylovLastGmresBlocks(Krylov* krylov, int counts[5], int* cancelled);
/* how many matrix products of the most recent unpipelined GMRES solve wrote the Jacobi application of their own output */
int DflKrylovLastFoldedProducts(Krylov* krylov);
/* ... and how many of its counted blocks of three or four iterations ran update and fix-up as one pass (DFL_GMRES_FUSE_FIXUP=0: none) */
int DflKrylovLastFusedBlocks(Krylov* krylov);
/* the same as pairs and single steps: a counted step of s iterations adds floor(s / 2) to pairs and s mod 2 to singles */
void DflKrylovLastGmresPairs(Krylov* krylov, int* pairs, int* singles, int* cancelled);
/* A non-blocking stream (default priority) that was PROBED to run concurrently with `main_stream`: HIP maps streams onto a few
 * hardware queues round-robin, and a side stream on the main stream's own queue runs behind it instead of beside it; a
 * highest-priority stream avoids that but was seen to delay every kernel of the normal-priority stream (host/comm_rccl.c).
 * What the RCCL communicator uses for its halo exchange; a host that fills DflComm.halo_stream itself should create its stream
 * with this.  The caller destroys it with hipStreamDestroy. */
hipStream_t DflPickConcurrentStream(hipStream_t main_stream);
/* GMRES(m): restart after m basis columns (x updated, true residual recomputed); m <= 0 or m >= max_iter (default) = the
 * reference's full GMRES.  Keeps the basis at m+1 vectors for long solves (config 5: 50M tets, PC_ILU0). */
void KrylovSetRestart(Krylov* krylov, index_type m);
/* FGMRES: keep Z[:,k] = M_k^-1 Q[:,k] (doubles the basis memory) so that the preconditioner may change between iterations;
 * switched on automatically by PC_TWOLEVEL */
void KrylovSetFlexible(Krylov* krylov, b32 on);
/* node coordinates for preconditioners that aggregate nodes (PC_TWOLEVEL); SolveFlowSystem passes its mesh itself */
void KrylovSetMesh(Krylov* krylov, const Mesh3D* mesh);
void KrylovSetAggregateSize(Krylov* krylov, index_type nodes_per_aggregate); /* PC_TWOLEVEL, default 64 */
/* optional communicator for element-partitioned runs (one process per GPU); NULL = single GPU */
typedef struct DflComm {
    void (*allreduce_sum)(void* ctx, f64* d_buf, index_type n); /* in place, device buffer */
    void (*halo_exchange)(void* ctx, f64* d_x);                /* fill ghost entries of a [u|p|..] vector */
    void* ctx;
    index_type num_owned_node; /* dots / norms run over owned nodes only */
    /* optional split exchange: halo_begin starts filling the ghost entries of d_x asynchronously (the caller has
     * finished writing d_x on the library stream), halo_end makes the library stream wait for it.  With
     * num_interior_node > 0 (owned nodes [0, num_interior_node) have no ghost neighbour) the Krylov matvec runs the
     * interior rows between the two.  NULL / 0: halo_exchange before the whole matvec. */
    void (*halo_begin)(void* ctx, f64* d_x);
    void (*halo_end)(void* ctx, f64* d_x);
    index_type num_interior_node;
    /* this process's place in the partition (0 / 0 when the implementer does not say: preconditioners that need a global
     * numbering -- PC_TWOLEVEL on a partitioned matrix -- then refuse and KrylovSolve falls back to PC_ILU0) */
    int rank, world;
    /* optional: the stream the exchange started by halo_begin runs on (NULL / returns NULL: synchronous).  The Krylov matvec
     * enqueues the boundary rows there, behind the unpack, so that they overlap the interior rows on the library stream and
     * the library stream waits once (in halo_end) for both */
    hipStream_t (*halo_stream)(void* ctx);
} DflComm;
void KrylovSetComm(Krylov* krylov, const DflComm* comm);
const DflComm* KrylovGetComm(const Krylov* krylov); /* NULL on a single GPU */

/* RCCL implementation of DflComm (host/comm_rccl.c): collectives enqueued from C on the library stream.
 * Bootstrap: every rank DflRcclLoad(path to librccl.so, NULL/"" = "librccl.so.1"); rank 0 DflRcclGetUniqueId and
 * broadcasts the DflRcclUniqueIdBytes() bytes (MPI, torch.distributed, a file ...); all ranks DflRcclCommCreate
 * (collective), optionally DflRcclCommCreateHaloComm with a second broadcast id, DflRcclCommSetHalo with their halo plan, KrylovSetComm(ksp, DflRcclCommVtable(c)). */
typedef struct DflRcclComm DflRcclComm;
int DflRcclLoad(const char* path);
int DflRcclUniqueIdBytes(void);
int DflRcclGetUniqueId(char* out_bytes);
DflRcclComm* DflRcclCommCreate(const char* id_bytes, int rank, int world);
/* optional own communicator for the halo stream; 0 = created.  If it fails on ANY rank, every rank must call
 * DflRcclCommDropHaloComm (agree on the result first): mixed use pairs sends and receives of different communicators */
int DflRcclCommCreateHaloComm(DflRcclComm* c, const char* id_bytes);
void DflRcclCommDropHaloComm(DflRcclComm* c);
void DflRcclCommSetInterior(DflRcclComm* c, index_type n_interior); /* owned nodes [0, n_interior) touch no ghost */
void DflRcclCommSetHalo(DflRcclComm* c, index_type n_local, index_type n_owned, const index_type* send_count,
                        const index_type* send_idx, const index_type* recv_count, const index_type* recv_idx);
const DflComm* DflRcclCommVtable(const DflRcclComm* c);
void DflRcclCommCounters(const DflRcclComm* c, int64_t* n_allreduce, int64_t* n_halo);
void DflRcclCommDestroy(DflRcclComm* c);

/* ---- assembly (assemble.h) ------------------------------------------------------------ */
void AssembleSystemTet(Mesh3D* mesh, f64* wgalpha_dptr, f64* dwgalpha_dptr, f64* F, Matrix* J);
void AssembleSystemTetFace(Mesh3D* mesh, f64* wgalpha_dptr, f64* dwgalpha_dptr, f64* F, Matrix* J);
/* the caller of the hot path, src/main.c:31-75 (static there) */
void AssembleSystem(Mesh3D* mesh, f64* wgalpha, f64* dwgalpha, f64* F, Matrix* J, Dirichlet** bcs, index_type nbc);
/* generalized-alpha Newton solve of one time level (src/main.c:77-283, static there; `maxit` <= 0 -> 4).
 * Returns the Newton iteration count; rnorm_out / rnorm_init_out (4 each: u, p, phi, T) may be NULL. */
index_type SolveFlowSystem(Mesh3D* mesh, f64* wgold, f64* dwgold, f64* dwg, Matrix* J, f64* F, f64* dx, Krylov* ksp,
                           Dirichlet** bcs, index_type nbc, index_type maxit, f64* rnorm_out, f64* rnorm_init_out);
struct ParticleContext;
/* one pass of the time loop body (src/main.c:537-565): predictor, SolveFlowSystem, corrector; with a
 * particle context also `dem_substeps` contact sweeps + particle updates (the calls the reference has
 * commented out at main.c:547-569) */
index_type DflTimeStep(Mesh3D* mesh, f64* wgold, f64* dwgold, f64* dwg, Matrix* J, f64* F, f64* dx, Krylov* ksp, Dirichlet** bcs,
                       index_type nbc, index_type newton_maxit, struct ParticleContext* pctx, index_type dem_substeps,
                       f64* rnorm_out, f64* rnorm_init_out);
/* ---- time step: a per-mesh dt, and the step limits of a state (build-defined) ----------------------------------------------
 * The reference steps with a compile-time literal (src/main.c:24, src/assemble.cu:24).  Here every mesh carries its own step,
 * DFL_DEFAULT_TIME_STEP until DflMeshSetTimeStep accepts another, and everything that uses dt reads the mesh's value at the
 * call: the volume and weak-BC face kernels of F and J under every schedule, the scalar residual rows and Jacobians, the
 * thermal-material Jacobian entries, the fluid-material rows and blocks, the phase-change J diagonal, the alpha states, the
 * predictor / corrector of DflTimeStep, the time window of a two-way capture source and of the volume target that follows it,
 * the solidification record's in_time_step updates, and DflScalarTransportSolve.  dt enters the kernels as kernel arguments
 * formed by one host function (dfl_step_consts_from_dt, include/dedflow_kernels.h); at the default step every result has the
 * bits of the compile-time build.  The step may change between any two calls and two meshes in one process may differ;
 * nothing cached depends on it.  In a partitioned run every rank sets the step of its own mesh.  The particle context's own
 * dt (ParticleContextSetContactModel) and dem_substeps stay the caller's business.
 *
 * Step limits of a state w (level: the surface phi = level).  No fused multiply-add anywhere; dot products are
 * (a0 b0 + a1 b1) + a2 b2.  Per tet e with nodes n_a, g_a = grad N_a in the closed form of the melt-pool capture section
 * (g_1 = c23 / det, g_2 = c31 / det, g_3 = c12 / det, g_0d = -((g_1d + g_2d) + g_3d)):
 *   ubar_d = 0.25 (((u_0d + u_1d) + u_2d) + u_3d),  c_a = ubar . g_a,  r_e = max_a |c_a|   (the rate at which a material
 *               point's barycentric coordinate changes: 1 / r_e is the time the fluid takes to cross the tet's altitude)
 *   m_e = max_a (g_a . g_a)                        1 / (shortest altitude)^2
 *   f_a = phi_a - level; the tet is CUT iff not all f_a > 0 and not all f_a < 0 (phi equal to level at a vertex: cut)
 *   Tbar        the vertex mean of T, formed as ubar
 *   sigma_e = max(0, sigma0 + dsigma_dT (Tbar - T_ref)) from the mesh's DflSurfaceForces, 0 when none is set
 *   q_e = sigma_e (m_e sqrt(m_e))                  sigma / h^3
 *   a tet is NON-FINITE when any of its twelve gradient entries, ubar, Tbar or any f_a is not finite: it is counted and takes
 *               part in no maximum.  A NaN never wins a comparison.
 * rate_adv = max r_e over the finite tets, rate_adv_surface = max r_e and cap_q = max q_e over the cut ones; each with the
 * lowest tet id that attains it.  The host finishes dt_adv = 1 / rate_adv, dt_surface = 1 / rate_adv_surface and
 * dt_capillary = sqrt(rho_bar / (2 pi cap_q)), the explicit surface-tension bound of the free-surface section, with
 * rho_bar = 0.5 (rho_gas + rho_metal) of the fluid material when one is set, else the built-in density.  The implicit parts
 * (viscosity, conduction, Darcy drag) impose no bound and get none.  One pass over the tets and a one-workgroup second stage,
 * no atomics: maxima and "the lowest id" are exact in any order, two runs agree bit for bit.  The state is sized at the first
 * call on a mesh and freed with it; later calls allocate nothing.  DflTimeStep does not adapt the step itself: with the setter
 * and the limits a controller is a few lines in the caller's loop. */
#ifndef DFL_DEFAULT_TIME_STEP
#define DFL_DEFAULT_TIME_STEP (5e-2)               /* the reference's kDT */
#endif
int  DflTimeStepCheck(f64 dt, char* why, size_t why_len);   /* host only; 0 = accepted: finite and > 0 */
void DflMeshSetTimeStep(Mesh3D* mesh, f64 dt);     /* refused on stderr, mesh unchanged, when the check refuses */
f64  DflMeshTimeStep(const Mesh3D* mesh);          /* DFL_DEFAULT_TIME_STEP until set */
typedef struct DflTimeStepLimits {
    f64 rate_adv, rate_adv_surface, cap_q;     /* maxima over the tets, above; 0 when no tet qualifies */
    index_type tet_adv, tet_surface, tet_cap;  /* the lowest tet id that attains each maximum; -1 when none */
    index_type num_cut, num_nonfinite;         /* cut tets; tets left out of every maximum */
    f64 dt_adv, dt_surface, dt_capillary;      /* 1 / rate_adv, 1 / rate_adv_surface, sqrt(rho_bar / (2 pi cap_q)); HUGE_VAL when the maximum is 0 */
    f64 dt;                                    /* DflMeshTimeStep(mesh) at the call */
} DflTimeStepLimits;
void DflMeshTimeStepLimits(Mesh3D* mesh, const f64* w, f64 level, DflTimeStepLimits* out);  /* w: device 6N state; waits for the device once */
/* ---- scalar transport: level set phi and temperature T (build-defined; opt-in) -------------------------------------------
 * The residual has SUPG rows for phi (advection) and T (advection-diffusion) (src/assemble.cu:885-906), but the reference
 * zeroes them before the solve (main.c:63-66) and its matrix has no phi / T blocks, so neither field ever moves.  With a
 * transport configured on the mesh both become transported fields:
 *   Jacobians  the exact derivatives of the phi / T rows with respect to the rates dphi / dT at fixed u (alpha-level chain
 *              rule: f1 = alpha_m, f2 = dt alpha_f gamma).  Given u the rows are affine in (dphi, dT), phi and T feed neither
 *              each other nor the (u,p) rows: two independent N x N systems, volume terms only.
 *   residual   every F assembly of the mesh (AssembleSystem, SolveFlowSystem) keeps the phi / T rows it computed in a
 *              mesh-owned [2N] array (DflMeshScalarResidual) before zeroing F[4N:6N) as the reference does; F itself and
 *              the (u,p) solve are unchanged.
 *   Dirichlet  nodes of the boundary groups in dirichlet_phi / dirichlet_T (bit g = group g) get a zero residual row and a
 *              unit matrix row: their increment is 0, they keep their value (separate from Dirichlet / DirichletApplyVec).
 *   Newton     SolveFlowSystem, after each (u,p) solve, assembles both Jacobians at the same alpha states, solves them
 *              (one GMRES per field, rtol / maxit below) against the saved residual into dx[4N:5N) and dx[5N:6N), and the
 *              one update dwg -= dx applies all increments (block-Jacobi Newton: the dependence of phi / T on u is left out,
 *              as in the reference's block structure).  rnorm[2] / rnorm[3] are the norms of the saved residual, so the
 *              convergence test covers them.  With a communicator SolveFlowSystem and DflTimeStep print why and return -1.
 * A mesh that never had a transport set, or had it cleared with NULL, computes bit for bit what it computed before. */
typedef struct DflScalarTransport {
    b32 phi, T;                            /* fields to advance */
    index_type dirichlet_phi, dirichlet_T; /* bit masks of boundary groups whose nodes hold their value */
    PCType pc;                             /* PC_JACOBI (default; PC_NONE is taken as PC_JACOBI) or PC_AMGX */
    f64 rtol;                              /* inner GMRES: relative tolerance (<= 0: 1e-10) */
    index_type maxit;                      /* inner GMRES: iterations (<= 0: 200) */
} DflScalarTransport;
void DflMeshSetScalarTransport(Mesh3D* mesh, const DflScalarTransport* cfg); /* copied; NULL: off, frees everything */
b32 DflMeshScalarTransportEnabled(const Mesh3D* mesh);
/* both Jacobians at the alpha states (wgalpha: only u is read; dwgalpha unused, the Jacobians do not depend on it) into
 * MAT_TYPE_CSR matrices over the nodal pattern (CSRAttrCreate; columns ascending) that own their values, overwritten; either
 * may be NULL.  Under a configured transport the rows of its Dirichlet groups become unit rows.  One launch per pattern
 * (csrc/k_scalar.hip), bitwise reproducible, the same under every assembly schedule. */
void DflAssembleScalarJacobian(Mesh3D* mesh, f64* wgalpha, f64* dwgalpha, Matrix* Jphi, Matrix* JT);
/* device [2N]: the phi / T rows of the last F assembly, scalar Dirichlet rows zeroed (a field that is not advanced: zeros);
 * NULL without a transport */
f64* DflMeshScalarResidual(Mesh3D* mesh);
/* one scalar Newton update at the current u: alpha states, residual, both Jacobians, both solves, dwg[4N:6N) -= dx.  Lets a
 * caller prescribe u and march the scalars alone.  rnorm_out[2] (may be NULL): norms of the phi / T residual it solved
 * against.  Returns 0, or -1 (with a message) when the mesh has no transport. */
index_type DflScalarTransportSolve(Mesh3D* mesh, f64* wgold, f64* dwgold, f64* dwg, f64* rnorm_out);
/* GMRES iterations of the last phi / T solves (-1: field not solved yet) */
void DflScalarTransportIterations(const Mesh3D* mesh, index_type its[2]);

/* the assembly caches J^-1-derived element geometry per mesh (the reference recomputes it every call); after writing new
 * node coordinates into Mesh3DDevice(mesh)->xg call this once so the next assembly rebuilds the cache */
void DflMeshGeometryChanged(Mesh3D* mesh);
/* device memory pool of the default DEVICE allocator (host/runtime.c; DFL_DEVICE_POOL_GB=0 disables it) */
void DflDevicePoolStats(int64_t* reserved_bytes, int64_t* in_use_bytes);
/* The driver wipes freed device memory in the background (~36 GB/s) and streaming kernels run up to 8 % slower meanwhile;
 * hipMemGetInfo counts that memory as free at once.  DflDeviceMemoryInUse: the driver's own "VRAM in use" figure for the
 * current device in bytes (it includes memory still to be wiped), -1 when rocm_smi is unavailable.  DflWaitDeviceMemoryQuiet:
 * blocks while a wipe is in progress (that figure falling, or the SOC clock at its high level), at most max_seconds; returns
 * the seconds waited, 0 when there was nothing to wait for, -1 when unknown.  Init() and the Krylov work-space calibration
 * call it; a host program that frees tens of GB right before a timed region may want to as well (host/runtime.c). */
int64_t DflDeviceMemoryInUse(void);
/* text log of this process's most recent Krylov work-space calibration (host/solver.c: what every candidate placement
 * measured, what was chosen, how long the waits were); "" when none has run.  DFL_WS_VERBOSE=1 prints the same to stderr. */
const char* DflKrylovCalibrationLog(void);
/* Placement of the Krylov work space (host/ws_placement.c).  The first KrylovSolve that allocates a GMRES basis for a large
 * block-mode system times at most four candidate blocks and keeps the fastest: bounded (<= 16 GB or a quarter of the free
 * memory extra, < 1 s), nothing the caller can see moves (DFL_WS_CANDIDATES=1 switches even that off).  This call is the
 * explicit, heavy form: builds the solver's preconditioner and work space for A now and draws many more placements -- basis
 * blocks and heap copies of the block value array behind spacers of up to 5/8 of the free memory, waiting for the driver's
 * memory wipe around the timings (5-15 s) -- holding at most max_extra_bytes of transient device memory (<= 0: no cap).  It
 * MAY move the block value array: ask MatrixFSBlockValues(A) again afterwards (DFL_VAL_RELOCATE=0 forbids the move). */
void DflKrylovCalibratePlacement(Krylov* krylov, Matrix* A, int64_t max_extra_bytes);
double DflWaitDeviceMemoryQuiet(double max_seconds);
/* boundary group whose faces get the weak-BC terms of AssembleSystemTetFace (default 4 = the reference's hard-coded group,
 * assemble.cu:1826-1828); lists are rebuilt when the group changes */
void DflSetWeakBCGroup(index_type group);
/* DflSetWeakBCGroup, DflSetAssemblySchedule and the Dfl*Parameters setters below change the PROCESS DEFAULTS; every mesh
 * copies them at Mesh3DCreate and keeps its own configuration from then on (two meshes with different schedules or face
 * groups coexist).  The two per-mesh forms (the schedule before Mesh3DGenerateColorBatch): */
void DflMeshSetAssemblySchedule(Mesh3D* mesh, int mode);
void DflMeshSetWeakBCGroup(Mesh3D* mesh, index_type group);
void DflSetQuiet(b32 quiet); /* suppress the reference's stdout chatter ("Assemble: F J", timers) */
/* which schedule the assembly kernels execute (set BEFORE Mesh3DGenerateColorBatch):
 *   0  the reference's JPL color batches, one launch per color (reference summation order)
 *   1  compact balanced re-coloring, ~4x fewer / larger launches; mesh->color,
 *      batch_offset and batch_ind are the reference's JPL result in both modes
 *   4  (default) slot-owner node patches for J (host/slotpatch.c): one launch, every workgroup owns the CSR rows of its nodes,
 *      every nodal nonzero is summed in registers by its owner lanes and written once -- no atomics, fixed summation order
 *      (bitwise reproducible), no geometry cache; AssembleSystem skips the zero pass.  The residual is assembled by spatial
 *      patches of <= 64 tets / <= 64 nodes (host/patch.c), one lane per tet, summed per node in a fixed order.
 *      A mesh whose patches exceed the kernel's limits falls back to schedule 1 (with a message on stderr).
 * Any other value is reported on stderr and replaced by 4. */
void DflSetAssemblySchedule(int mode);
/* schedule 4: nodes per patch, cap on the nodal nonzeros of a patch and on the tets touching it */
void DflSetSlotPatchParameters(index_type leaf_nodes, index_type slot_cap, index_type tet_cap);

/* ---- arrays / particles (Array.h, Particle.h) ------------------------------------------ */
typedef struct Array {
    b32 is_host;
    index_type len;
    f64* data;
} Array;
#define ArrayLen(a) ((a)->len)
#define ArrayData(a) ((a)->data)
Array* ArrayCreateHost(index_type len);
Array* ArrayCreateDevice(index_type len);
void ArrayDestroy(Array* a);
void ArrayCopy(Array* dst, const Array* src, MemCopyKind kind);
void ArrayLoad(Array* a, H5FileInfo* h5f, const char* dataset_name);       /* Array.c:242-253; in libdedflow_h5.so */
void ArraySave(const Array* a, H5FileInfo* h5f, const char* dataset_name); /* Array.c:255-261 */
/* BLAS-1 wrappers of Array.h:24-36 (Array.c:83-238).  A device array runs the library's own kernels on the library stream and
 * returns when the result is on the host / the array is updated, like the reference's cuBLAS calls with a host result pointer;
 * a host array is walked on the host in index order, like the reference.  Both operands must live on the same side.
 * ArrayZero is ArrayScale(a, 0.0) as in the reference (Array.c:103-105: a NaN stays a NaN).  SetAt with a repeated index keeps
 * the LAST value, as the reference's sequential loop does.  The reference declares ArrayGetAt and defines ArrayAt: both names. */
void ArraySet(Array* a, f64 val);
void ArrayZero(Array* a);
void ArraySetAt(Array* a, index_type n, const index_type* idx, const f64* val);
void ArrayGetAt(const Array* a, index_type n, const index_type* idx, f64* val);
void ArrayAt(const Array* a, index_type n, const index_type* idx, f64* val);
void ArrayScale(Array* a, f64 val);
void ArrayDot(f64* result, const Array* a, const Array* b);
void ArrayNorm2(f64* result, const Array* a);
void ArrayAXPY(Array* y, f64 a, const Array* x);
void ArrayAXPBY(Array* y, f64 a, const Array* x, f64 b); /* y = a x + b y */

/* ---- nodal fields (Field.h:13-33, Field.c:15-77): a host and a device Array of num_node * num_nodal_dof values ------- */
typedef struct Field {
    index_type shape[2];
    Array* host;
    Array* device;
} Field;
#define FieldHost(f) ((f)->host)
#define FieldDevice(f) ((f)->device)
Field* FieldCreate3D(const Mesh3D* mesh, i32 num_nodal_dof);
void FieldDestroy(Field* f);
void FieldInit(Field* f, void (*func)(f64*, void* ctx), void* ctx); /* func fills the host array; then H2D */
void FieldLoad(Field* f, H5FileInfo* h5f, const char* group_name);       /* Field.c:47-51; in libdedflow_h5.so */
void FieldSave(const Field* f, H5FileInfo* h5f, const char* group_name); /* Field.c:53-57 (saves the HOST copy) */
void FieldCopy(Field* dst, const Field* src);
void FieldUpdateHost(Field* f);
void FieldUpdateDevice(Field* f);
typedef struct ParticleContext {
    index_type num_particle;
    i32 num_pointwise_dof;
    Array* h_arr[3];
    Array* d_arr[3];
    f64 buff[2];
    void* ext; /* cell list workspace of the DEM sweep */
} ParticleContext;
#define ParticleCTXNumParticle(pctx) ((pctx)->num_particle)
#define ParticleCTXHostCoord(pctx) ((pctx)->h_arr[0])
#define ParticleCTXHostVel(pctx) ((pctx)->h_arr[1])
#define ParticleCTXHostAcc(pctx) ((pctx)->h_arr[2])
#define ParticleCTXDeviceCoord(pctx) ((pctx)->d_arr[0])
#define ParticleCTXDeviceVel(pctx) ((pctx)->d_arr[1])
#define ParticleCTXDeviceAcc(pctx) ((pctx)->d_arr[2])
#define ParticleMass(pctx) (((pctx)->buff)[0])
#define ParticleRadius(pctx) (((pctx)->buff)[1])
ParticleContext* ParticleContextCreate(index_type num_particle);
void ParticleContextDestroy(ParticleContext* ctx);
void ParticleContextCopy(ParticleContext* dst, const ParticleContext* src);
/* <group_name>/{coord,vel,acc} (Particle.c:66-103); in libdedflow_h5.so */
void ParticleContextLoad(ParticleContext* ctx, H5FileInfo* h5f, const char* group_name);
void ParticleContextSave(const ParticleContext* ctx, H5FileInfo* h5f, const char* group_name);
void ParticleContextUpdateHost(ParticleContext* ctx);
void ParticleContextUpdateDevice(ParticleContext* ctx);
/* empty in the reference (Particle.c:120-130); here: inlet insertion and outflow removal once configured (below) */
void ParticleContextAdd(ParticleContext* ctx);
/* empty in the reference (Particle.c:120-130); here: contact-force sweep + explicit update (build-defined) */
void ParticleContextUpdate(ParticleContext* ctx);
void ParticleContextRemove(ParticleContext* ctx);
void ParticleContextSetContactModel(ParticleContext* ctx, f64 kn, f64 gamma_n, f64 dt);
void ParticleContextComputeForces(ParticleContext* ctx); /* acc <- contact forces / mass */

/* ---- particle-fluid coupling (build-defined: the reference has the hooks, not the physics) -------------------------
 * Opt-in; a context that is never coupled behaves exactly as without this section.
 *   location   every particle is located on the tet mesh by a walk over the tet neighbour table, starting from its tet
 *              of the previous call (or from a uniform seed grid over the mesh's bounding box when it has none).  The
 *              result is the tet (-1: outside the mesh, -2: the walk hit its cap of DFL_COUPLE_MAX_WALK steps; such a
 *              particle is counted by ParticleContextLostCount) and the barycentric coordinates lambda[4] (min >= -1e-12:
 *              a tet is accepted when each of its four lambdas compares >= -1e-12, so never with a NaN among them).
 *              A particle with a coordinate that is not finite (+-inf, NaN) is outside: tet -1, lambda 0, not counted as
 *              lost, whatever tet it came from.
 *              "Outside" means the walk stood in a tet whose only faces with lambda < -1e-12 are boundary faces: exact
 *              for CONVEX domains; in a non-convex domain a particle may be reported outside wrongly.
 *   drag       u_f = sum_a lambda_a u(node_a) (u = the first 3N entries of the 6N state), d = 2R,
 *              rho_p = m / (4/3 pi R^3), Re = rho_f |u_f - v| d / mu_f, Schiller-Naumann f = 1 + 0.15 Re^0.687 (Re <= 1000)
 *              or 0.44 Re / 24, tau = rho_p d^2 / (18 mu_f).  Implicit in v with f lagged (stable for any dt / tau):
 *                v' = (v + dt (a_contact + (1 - rho_f/rho_p) g + f u_f / tau)) / (1 + dt f / tau),  x' = x + dt v'
 *              acc <- (v' - v) / dt; the drag impulse m f (u_f - v') / tau dt is accumulated per particle.  A particle
 *              outside the mesh feels gravity only (no buoyancy, no drag).
 *   reaction   load[3a + d] = -sum_p lambda_{a,p} impulse_p[d] / (time since the last call): the force of the particles
 *              on the fluid at node a, with the particles' latest lambda (a particle outside the mesh at that moment
 *              contributes nothing).  Summed in a fixed order (no float atomics): bitwise reproducible; sum_a load =
 *              -sum_p impulse_p / dt to rounding.
 *   two-way    DflMeshSetExternalLoad registers such a force on a mesh; the assembly of F subtracts it from the momentum
 *              rows (the residual is R = (...) - f_ext: body forces enter with a minus sign, as kRHO * fb does) after the tet
 *              and face terms and before the Dirichlet rows, which therefore stay exact.  The coupling is explicit (not
 *              in J).  DflTimeStep registers the reaction load of the previous step's sub-steps for its Newton solve.
 * Defaults: rho_f = 1e3, mu_f = 10/3 (the reference's kRHO and kMU), g = 0, two_way off.  One GPU only: DflTimeStep
 * refuses a coupled context when the solver has a communicator.  Nothing is allocated or synchronised per call except
 * by ParticleContextLostCount (one 4-byte read). */
typedef struct DflFluidCoupling {
    f64 rho_f, mu_f, gravity[3];
    b32 two_way;
} DflFluidCoupling;
/* couple to `mesh` (builds the neighbour table and seed grid once per mesh, and has the mesh build its sorted V2E lists if
 * nothing did before: they belong to the mesh and stay with it when the coupling goes; resets every particle's tet
 * to "none", the impulses and the lost count); cfg NULL = defaults; mesh NULL = coupling off (frees its state) */
void ParticleContextSetFluidCoupling(ParticleContext* ctx, Mesh3D* mesh, const DflFluidCoupling* cfg);
void ParticleContextLocate(ParticleContext* ctx);
const index_type* ParticleContextTet(const ParticleContext* ctx);        /* device [P] */
const f64* ParticleContextBarycentric(const ParticleContext* ctx);       /* device [P][4] */
index_type ParticleContextLostCount(const ParticleContext* ctx);        /* walks that hit the cap since coupling was set */
/* one coupled sub-step with the fluid state w (device, 6N): contact forces, locate, drag + gravity + integration (dt of
 * ParticleContextSetContactModel) */
void ParticleContextFluidStep(ParticleContext* ctx, const f64* w);
/* load (device, 3N) <- the reaction load of the sub-steps since the last call (zero when there were none); resets them */
void ParticleContextReactionLoad(ParticleContext* ctx, f64* load);
/* device [3N] external force on the momentum equations (NULL = none); the array must outlive its registration */
void DflMeshSetExternalLoad(Mesh3D* mesh, const f64* load);

/* ---- particle walls from a mesh's boundary faces (build-defined; opt-in) ----------------------------------------------
 * A context that never calls ParticleContextSetWallMesh keeps the six walls of the unit box and its contact grid over
 * [0,1]^3, bit for bit.  With walls set, every contact sweep (ParticleContextComputeForces, hence ParticleContextUpdate,
 * ParticleContextFluidStep and the DEM sub-steps of DflTimeStep) collides the particles with the wall triangles instead:
 *   walls      the boundary faces of the groups whose bit is set in group_mask; the other groups are open (inlet, outlet):
 *              particles cross them freely.  Normal n_t of a triangle t = the unit normal towards the opposite vertex of
 *              its tet (into the fluid).
 *   law        the linear spring-dashpot law of the particle pairs, no clamping of negative f:
 *                f = kn delta - gamma_n (v . n),  F += f n
 *              for centre c, triangle t (vertex a), s = (c - a) . n_t and q = the point of t closest to c:
 *                face contact     q in the interior of t (Voronoi region of the face) and -R < s < R: delta = R - s, n = n_t
 *                                 (a centre slightly behind the plane is still pushed out, as the box law does)
 *                edge / vertex    q on an edge or vertex of t, s > 0 and |c - q| < R: delta = R - |c - q|,
 *                                 n = (c - q) / |c - q|; a q at an endpoint of an edge is that vertex's contact
 *   de-duplication (tolerance tol = 1e-12 x the diagonal of the mesh's bounding box; the candidates in ascending id):
 *              1. face contacts with the same supporting plane (normals equal to 1e-12, offsets to tol) count once;
 *              2. an edge or vertex contact whose q lies in the plane of a kept face contact is dropped;
 *              3. edge contacts count once per sorted node pair, vertex contacts once per node id;
 *              4. an edge or vertex contact is dropped unless it is a local minimum of the distance to the walls, i.e.
 *                 when a wall triangle holding that edge (both nodes) or vertex lies nearer to c than |c - q| - tol.  This keeps
 *                 one contact at a convex edge of the domain whether c faces the middle of a mesh edge or a mesh vertex,
 *                 and none from the further vertices along that edge.
 *   cap        a particle keeps at most DFL_WALL_MAX_CONTACTS distinct contacts; further ones are dropped and counted
 *              (ParticleContextWallDroppedCount).
 *   grids      the contact cell grid spans the mesh's bounding box padded by R (cell edge >= 4R per axis, about half a
 *              particle per cell, at most 2^24 cells).  A particle whose centre lies outside that box gets NO contact
 *              acceleration, from pairs or walls, and is no pair partner of the others: it has left through an open group.
 *              Wall candidates come from a static grid over the same box; forces are bitwise reproducible.
 *   setup      the wall records and grids are built at the call, and again only when ParticleRadius changes; a change of
 *              the particle count rebuilds the particle grid only (host arithmetic); a sweep allocates nothing and does not
 *              wait for the device.  The walls are a snapshot of
 *              the mesh: a moved mesh needs another call.  Point location of the coupling stays exact for convex domains
 *              only; walls do not change that. */
#ifndef DFL_WALL_MAX_CONTACTS
#define DFL_WALL_MAX_CONTACTS 8
#endif
/* particle walls = the boundary faces of `mesh` in the groups whose bit is set in group_mask (bit i = group i);
 * replaces the unit-box walls and spans the contact cell grid over the mesh's bounding box padded by R;
 * mesh NULL = back to the unit box (frees the wall state) */
void ParticleContextSetWallMesh(ParticleContext* ctx, Mesh3D* mesh, index_type group_mask);
/* wall contacts dropped since the walls were set because a particle had more than DFL_WALL_MAX_CONTACTS */
index_type ParticleContextWallDroppedCount(const ParticleContext* ctx);

/* ---- contact friction and particle rotation (build-defined; opt-in) ---------------------------------------------------
 * A context that never calls ParticleContextSetFriction with a configuration runs the frictionless kernels, bit for bit.
 * With friction on, every contact sweep (ParticleContextComputeForces, hence ParticleContextUpdate,
 * ParticleContextFluidStep and the DEM sub-steps of DflTimeStep, coupled or not) adds the Cundall-Strack tangential law
 * to the pair, unit-box and mesh-wall contacts:
 *   spheres    radius R, mass m, moment of inertia I = 2/5 m R^2 (per particle: polydisperse block); angular velocity w, angular acceleration
 *              alpha = tau / I.  The normal law is unchanged: f_n = kn delta - gamma_n v_n, not clamped.
 *   contact    unit normal n towards the particle; lever ell = distance from the centre to the contact point:
 *                pair           ell = dist / 2 (the contact point is the midpoint of the centres)
 *                wall           ell = max(R - delta, 0) (unit box, mesh face, edge or vertex; the point is q, the closest
 *                               point of the wall)
 *              contact-point velocity  pair: v_rel = (v_i - v_j) - ell (w_i + w_j) x n;  wall at rest: v_rel = v - ell w x n
 *              v_t = v_rel - (v_rel . n) n
 *   spring     xi = the contact's tangential spring from the previous sweep (0 for a new contact); it is first rotated onto
 *              the current tangent plane keeping its length, xi <- (xi - (xi.n) n) |xi| / |xi - (xi.n) n| (0 when the
 *              denominator is 0), then xi <- xi + v_t dt
 *   force      F_t = -kt xi - gamma_t v_t; when |F_t| > mu max(f_n, 0) it is scaled to that cap and
 *              xi <- -(F_t + gamma_t v_t) / kt (the spring consistent with sliding).  Load: force f_n n + F_t, torque
 *              (-ell n) x F_t.  A pair is evaluated so that particle j's computation is the exact negation of i's: the
 *              tangential forces are exactly opposite and the torques exactly equal, and an isolated pair conserves
 *              sum m x x v + I w (to rounding under the semi-implicit step).
 *   history    EVERY sweep advances the springs by the context's dt (ParticleContextSetContactModel):
 *              ParticleContextComputeForces is no longer a pure function of the state once friction is on.  History is
 *              matched by a 64-bit contact key, kind in the two high bits:
 *                0 << 62 | j                  partner particle j
 *                1 << 62 | 2 axis + side      unit-box wall (side 0: x_axis = 0, side 1: x_axis = 1)
 *                1 << 62 | plane id           mesh face contact: the smallest triangle id among the triangles whose plane
 *                                             equals this one under de-duplication rule 1 of the walls block (assigned at
 *                                             ParticleContextSetWallMesh; a sphere rolling over coplanar triangles keeps
 *                                             one history)
 *                2 << 62 | n0 << 31 | n1      mesh edge contact, node ids n0 < n1
 *                3 << 62 | node               mesh vertex contact
 *                1 << 62 | 1 << 61            the surface phi = level ("solid-surface contact"; beyond every plane id)
 *              (a context has unit-box walls or mesh walls, never both, so the two wall keys do not meet.)
 *   capacity   at most DFL_DEM_MAX_HISTORY entries per particle, pairs and walls together, taken in the sweep's visit
 *              order (pairs, then walls).  A contact that finds no free entry gets its normal force and the tangential
 *              force of a new contact (xi = 0), stores nothing and is counted (ParticleContextFrictionOverflowCount).
 *   state      turning friction on allocates w and alpha (zero) and the history; later ParticleContextSetFriction calls
 *              keep w and clear the history and the overflow count; ParticleContextSetWallMesh clears the history.
 *              cfg NULL turns friction off and frees the state.  Nothing is allocated per sweep.
 *   integration ParticleContextUpdate and ParticleContextFluidStep integrate w by semi-implicit Euler with alpha after the
 *              sweep.  The fluid exerts no torque on a particle (no rotational drag, no lift).
 *   gravity    ParticleContextSetGravity sets a body acceleration that ParticleContextUpdate (hence the uncoupled DEM
 *              sub-steps of DflTimeStep) adds in its integration step; default 0.  The coupled sub-step keeps using
 *              DflFluidCoupling.gravity.  acc stays the contact acceleration.
 *   not kept   ParticleContextCopy and ParticleContextSave / Load handle coord, vel and acc only: w and the history are
 *              neither copied nor saved. */
#ifndef DFL_DEM_MAX_HISTORY
#define DFL_DEM_MAX_HISTORY 16
#endif
typedef struct DflContactFriction {
    f64 mu, kt, gamma_t; /* kt <= 0: 2/7 kn; gamma_t < 0: gamma_n (of ParticleContextSetContactModel at this call) */
} DflContactFriction;
void ParticleContextSetFriction(ParticleContext* ctx, const DflContactFriction* cfg); /* NULL: off, frees the state */
f64* ParticleContextAngularVelocity(ParticleContext* ctx);        /* device [P][3], writable (initial spin); NULL when off */
const f64* ParticleContextAngularAcc(const ParticleContext* ctx); /* device [P][3], torque / I of the last sweep */
/* contacts that found no free history entry since friction was last set */
index_type ParticleContextFrictionOverflowCount(const ParticleContext* ctx);
void ParticleContextSetGravity(ParticleContext* ctx, const f64 g[3]); /* body acceleration of ParticleContextUpdate */
/* the history the next sweep reads: device rows [P][DFL_DEM_MAX_HISTORY] of 32-byte entries (uint64 key, f64 xi[3]) and
 * live counts [P]; both NULL when friction is off */
void ParticleContextFrictionHistory(const ParticleContext* ctx, const void** rows, const index_type** counts);

/* ---- particle inflow and outflow (build-defined; opt-in) ---------------------------------------------------------------
 * A context that never calls ParticleContextSetInflow or ParticleContextSetOutflow with a configuration keeps its particle
 * count for life: ParticleContextAdd and ParticleContextRemove are no-ops and DflTimeStep is unchanged, bit for bit.
 *   tags       the first Set call gives every particle a stable 64-bit tag 0 .. P-1; inserted particles take the next tags
 *              in insertion order.  Ids change under compaction, tags do not (ParticleContextTag).
 *   capacity   every per-particle buffer is sized to a capacity >= num_particle that grows by x1.5 only when an Add needs
 *              it.  The Arrays' len is always 3 num_particle (ParticleContextSave writes the live particles).  Add and
 *              Remove swap the Arrays' data pointers with spare storage: a pointer taken from ArrayData, or from
 *              ParticleContextTet / Barycentric / AngularVelocity / AngularAcc / Tag, is valid until the next Add or Remove.
 *   Remove     1. with outside_mesh on a coupled context: ParticleContextLocate first (tet -1 also means "not located").
 *              2. particle i is removed when n . x_i > d for any plane (n[3], d) = plane[k], computed as
 *                 (n0 x0 + n1 x1) + n2 x2 without fused multiply-add, or (outside_mesh, coupled) when tet_i == -1.  A particle
 *                 at tet -2 (walk cap hit; counted by ParticleContextLostCount) is kept.
 *              3. stable compaction: survivors keep their relative order and carry coord, vel, acc, the tag, with friction
 *                 w, alpha and the history rows the next sweep reads (partner keys 0 << 62 | j remapped to the partner's
 *                 new id, entries whose partner was removed dropped, the others in their order; wall keys unchanged),
 *                 and with coupling tet, lambda and the pending drag impulse.
 *              4. the drag impulse of the removed particles still pending (imp_time > 0) is scattered to the nodes with
 *                 their current lambda (fixed order, no float atomics) into a per-context accumulator that the next
 *                 ParticleContextReactionLoad adds and clears: that load equals, to rounding, the one without the Remove.
 *   Add        inlet rectangle o + s u + t v (s, t in [0, 1], u perpendicular to v), nu = floor(|u| / 2R), nv likewise;
 *              slot k = i + nu j (i < nu, j < nv).  No slot when nu or nv is 0.  Host constants, IEEE double, left to right:
 *                pu = u / nu, pv = v / nv, base = (o + 0.5 pu) + 0.5 pv,
 *                ju = jitter (0.5 (|u| / nu - 2R)), ou = (u / |u|) ju, and jv, ov likewise (|u| = sqrt((u0 u0 + u1 u1) + u2 u2))
 *              hash h(a) = splitmix64(a) = mix(a + 0x9E3779B97F4A7C15) with mix(z) = z ^ (z >> 30), * 0xBF58476D1CE4E5B9,
 *                ^ (z >> 27), * 0x94D049BB133111EB, ^ (z >> 31) (wrapping 64-bit);  H(c, k, a) = h(h(h(seed) ^ c) ^ (4k + a))
 *                with c = the index of this Add call since ParticleContextSetInflow (0, 1, ...), counted whether or not it
 *                inserts;  r_a = 2 ((H(c, k, a) >> 11) 2^-53) - 1 in [-1, 1)
 *              candidate centre of slot k in call c, per axis d, without fused multiply-add:
 *                x_d = (((base_d + i pu_d) + j pv_d) + r_0 ou_d) + r_1 ov_d
 *              so two candidates are never closer than 2R.  Slot k is blocked when an existing particle centre y has
 *              (y0 - x0)^2 + (y1 - x1)^2 + (y2 - x2)^2 < (2R)^2 (summed left to right).  Candidates are not tested against
 *              walls: the caller places the inlet inside the fluid domain, at least R from every wall.
 *              credit += per_call; want = floor(credit); credit -= want; want = min(want, max(max_particles - P, 0)).  The
 *              free slots in ascending (H(c, k, 2) >> 1, k) are the candidates; the first min(want, free) are appended at
 *              ids P, P+1, ... with vel = cfg.vel, acc 0, spin 0, an empty history row, tet -1, lambda 0, no impulse.
 *              want - inserted is added to `blocked` and not carried over.  Selection and positions are a pure function
 *              of (seed, c, the blocked slots).
 *   cost       Remove and Add each read 4 bytes back (the new count) and allocate nothing except when Add grows the
 *              capacity; DflTimeStep calls ParticleContextAdd after the predictor (inflow set) and ParticleContextRemove
 *              after the particle sub-steps (outflow set), as the reference's commented-out calls at main.c:548 and :569.
 *   other      the contact sweep's cell order is invalidated by a count change (the next locate runs in id order until
 *              the next sweep); mesh walls rebuild only their particle grid.  Set*flow(ctx, NULL) turns that direction
 *              off; tags and the statistics stay until the context is destroyed.  One GPU only. */
#define DFL_OUTFLOW_MAX_PLANES 8
typedef struct DflParticleOutflow {
    index_type num_planes;
    f64 plane[DFL_OUTFLOW_MAX_PLANES][4]; /* removed when n . x > d, (n[3], d) = plane[k] */
    b32 outside_mesh;                     /* coupled only: also remove the particles located outside the mesh (tet -1) */
} DflParticleOutflow;
typedef struct DflParticleInflow {
    f64 origin[3], edge_u[3], edge_v[3]; /* inlet rectangle origin + s u + t v, s, t in [0, 1]; u perpendicular to v */
    f64 vel[3];                          /* velocity of an inserted particle */
    f64 per_call;                        /* particles wanted per ParticleContextAdd (the fraction is carried as credit) */
    f64 jitter;                          /* in [0, 1]: share of each slot's slack used for the in-plane offset */
    uint64_t seed;
    index_type max_particles;            /* Add never lets num_particle exceed this */
} DflParticleInflow;
typedef struct DflParticleFlowStats {
    int64_t inserted, removed, blocked;
} DflParticleFlowStats;
void ParticleContextSetOutflow(ParticleContext* ctx, const DflParticleOutflow* cfg); /* NULL: off */
void ParticleContextSetInflow(ParticleContext* ctx, const DflParticleInflow* cfg);   /* NULL: off; resets call index and credit */
/* particles inserted, removed and inlet candidates that found their slot blocked since the first Set*flow call */
void ParticleContextFlowStats(const ParticleContext* ctx, DflParticleFlowStats* out);
const int64_t* ParticleContextTag(const ParticleContext* ctx); /* device [P]; NULL until inflow or outflow was set */

/* ---- polydisperse particles (build-defined; opt-in) ---------------------------------------------------------------------
 * A context that never calls ParticleContextSetSizes or ParticleContextSetInflowSizes is monodisperse: every kernel reads
 * ParticleRadius / ParticleMass and runs as without this section, bit for bit.  Once sizes are set:
 *   spheres    particle i has radius r_i > 0 and mass m_i > 0, I_i = 2/5 m_i r_i^2.  ParticleRadius and ParticleMass are
 *              only the reference particle of the default masses and of inflow without SetInflowSizes; no kernel reads
 *              them.  Rmax (ParticleContextMaxRadius) bounds every radius: the max of the radii passed to SetSizes and of
 *              r_hi of SetInflowSizes (and R when inflow inserts at R); Remove never lowers it; it is host state only.
 *   laws       the laws above with per-particle values, written so that with every radius R and every mass M the floating
 *              point operations are exactly the monodisperse ones:
 *                pairs   contact when d2 < (r_i + r_j)^2, delta = (r_i + r_j) - dist, f = kn delta - gamma_n v_n,
 *                        acc_i = F_i (1 / m_i)   ((R + R) == 2R and (R + R)^2 == 4 R R exactly)
 *                walls   r_i wherever R appears: the unit box, the face test -r_i < s < r_i, edge and vertex contacts
 *                        |c - q| < r_i, the wall lever max(r_i - delta, 0)
 *                friction  contact point = the middle of the overlap: levers ell_i = 0.5 (dist + (r_i - r_j)) and
 *                        ell_j = 0.5 (dist + (r_j - r_i)); v_rel = (v_i - v_j) - (ell_i w_i + ell_j w_j) x n; torque on i
 *                        (-ell_i n) x F_t.  The lever term is ell (w_i + w_j) x n with ell = 0.5 dist when r_i == r_j (as
 *                        above), else ell_a (w_a x n) + ell_b (w_b x n) with a the smaller particle id: j's evaluation stays
 *                        the exact negation of i's (xi_j == -xi_i), and sum m x x v + I w is conserved to rounding
 *                coupling  d_i = 2 r_i, rho_p,i = m_i / (4/3 pi r_i^3), the impulse with m_i; location and the reaction
 *                        load are unchanged
 *   search     particle i searches the cells within r_i + Rmax; cell edge >= 4 Rmax (unit-box grid, padded mesh-wall grid
 *              and the wall grid's R-expansion, rebuilt when Rmax changes).  Radius ratios above about 3 stay correct but
 *              slow: many small particles share one big cell (no multi-level grid).
 *   history    a big particle among small ones can exceed DFL_DEM_MAX_HISTORY contacts; the excess is counted by
 *              ParticleContextFrictionOverflowCount as before.
 *   masses     SetSizes without masses: m_i = ParticleMass ((q q) q), q = r_i / ParticleRadius (the reference particle's
 *              density; q = 1 gives ParticleMass exactly).
 *   inflow     SetInflowSizes(r_lo, r_hi), 0 < r_lo <= r_hi (a monodisperse context becomes polydisperse, every particle at
 *              ParticleRadius / ParticleMass): the slot lattice and jitter of the inflow block with R replaced by r_hi;
 *              slot k of call c gets r = r_lo + (r_hi - r_lo) u, u = (H(c, k, 3) >> 11) 2^-53 (no fused multiply-add) and
 *              the default mass; a slot is blocked when dist^2 < (r_y + r_k)^2 against an existing particle y.  Without
 *              SetInflowSizes a polydisperse context inserts at ParticleRadius.
 *   outflow    compaction carries r and m; capacity growth and the spare-buffer swaps cover them.
 *   kept       ParticleContextCopy carries the sizes (dst becomes what src is); ParticleContextSave writes <group>/radius and
 *              <group>/mass when polydisperse; ParticleContextLoad reads them when both are present (the context becomes
 *              polydisperse); files without them behave as before.
 *   cost       the sort writes a sorted copy of the radii ([P], next to the 48-byte records); the force kernels read 8 more
 *              bytes per tested neighbour and the own mass.  Nothing new allocates per sweep or reads back to the host. */
/* radius, mass: host [P]; mass NULL = the default masses; radius NULL = monodisperse again (frees the arrays).  A non-positive
 * or non-finite value is reported on stderr and leaves the context unchanged */
void ParticleContextSetSizes(ParticleContext* ctx, const f64* radius, const f64* mass);
const f64* ParticleContextRadii(const ParticleContext* ctx);  /* device [P]; NULL when monodisperse; valid until Add / Remove */
const f64* ParticleContextMasses(const ParticleContext* ctx); /* device [P]; NULL when monodisperse; valid until Add / Remove */
f64 ParticleContextMaxRadius(const ParticleContext* ctx);     /* Rmax; ParticleRadius when monodisperse */
void ParticleContextSetInflowSizes(ParticleContext* ctx, f64 r_lo, f64 r_hi);

/* ---- particle heat transfer (build-defined; opt-in) ---------------------------------------------------------------------
 * The reference has no physics here (empty particle hooks, no source in its T equation).  A context that never calls
 * ParticleContextSetHeat with a configuration, and a mesh that never gets a heat source, compute bit for bit what they
 * compute without this section, through the same launches.  One GPU only (DflTimeStep refuses a coupled context under a
 * communicator).  With r_i, m_i the particle's radius and mass (ParticleRadius / ParticleMass when monodisperse),
 * d = 2 r_i, C_i = m_i cp_p:
 *   conduction  (k_p > 0) for every particle pair in contact in the sub-step's contact sweep -- the sorted copies, the cell
 *               list and the overlap test of the force kernel, through the same pair loop, so no pair is a contact for the
 *               force and not for the heat -- with overlap delta = (r_i + r_j) - dist: contact radius a = sqrt(r* delta),
 *               r* = r_i r_j / (r_i + r_j), conductance H = 2 k_p a (Batchelor-O'Brien, equal conductivities),
 *               q_i += H (T_j - T_i) with the temperatures at the START of the sub-step (explicit).  H is evaluated with
 *               commutative operations on (r_i, r_j): both partners get exactly opposite heat.  Visit order = the pair
 *               loop's: bitwise reproducible for a given contact grid; two grids that bin the particles differently (the
 *               unit box and a wall mesh's, or another Rmax) visit a particle's partners in another order and agree to
 *               the rounding of the sum.  Walls are adiabatic (box walls and mesh walls alike).  A particle outside
 *               the contact grid of a wall mesh has no partner, as for forces.  Explicit conduction is stable for
 *               dt sum_j H_ij / C_i < 1: the caller's condition, not enforced.
 *   convection  (coupled context, fluid state given, particle located in a tet) T_f = sum_a lambda_a T(node_a) with
 *               T = w[5N + node], u_f as the drag does, Re = rho_f |u_f - v| d / mu_f with the velocity v the particle has
 *               when the heat step runs, Pr = cp_f mu_f / k_f, Ranz-Marshall Nu = 2 + 0.6 Re^(1/2) Pr^(1/3),
 *               tau_T = C_i / (Nu k_f pi d); rho_f and mu_f are the coupling's.  A particle outside the mesh (tet < 0)
 *               exchanges nothing with the fluid.
 *   update      implicit in T_i for the convective part (stable for any dt / tau_T, the thermal twin of the drag update):
 *                 T_i' = (T_i + dt (q_i / C_i + T_f / tau_T)) / (1 + dt / tau_T);   without convection T_i' = T_i + dt q_i / C_i
 *               heat_rate_i = C_i (T_i' - T_i) / dt (0 for dt = 0).  The energy the fluid gave the particle, e_i = dt C_i (T_f - T_i') / tau_T,
 *               is accumulated per particle like the drag impulse.
 *   source      q[a] = -sum_p lambda_{a,p} e_p / (time since the last call), summed in the fixed order of the reaction load
 *               (no float atomics, bitwise reproducible), with the latest lambda; a particle outside the mesh at that
 *               moment contributes nothing.  The energy pending on particles that ParticleContextRemove takes out is kept
 *               and added to the next source.  sum_a q[a] = -sum_p e_p / time to rounding.
 *   T rows      with a source registered (DflMeshSetHeatSource) every F assembly subtracts it from F[5N:6N): the residual is
 *               R_T = (...) - q, after the tet and face terms and before the phi / T rows are captured for the scalar
 *               transport, whose Dirichlet rows stay exactly zero and whose Newton solve sees it.  Explicit: not in J_T.
 *   time step   ParticleContextUpdate (uncoupled: conduction only) and ParticleContextFluidStep (coupled) run the heat step
 *               after their integration when heat is on; it never changes coord / vel / acc / omega.  Conduction thus sees
 *               the geometry of the sub-step's force sweep (positions before the integration), convection the tets and
 *               weights of that sub-step's location and the velocity after it.  With two_way, DflTimeStep registers the
 *               pending source for its Newton solve and restores the caller's registration afterwards, as it treats the
 *               reaction load; a user source already registered is an ASSERT.  A bare ParticleContextHeatStep runs the cell
 *               sort itself when no sweep is valid for the current particles (it never computes forces) and, coupled with
 *               a fluid state, locates the particles first.  A sweep stops being valid when the particle count, the sizes
 *               or the wall mesh change; particles that merely MOVED since the last sweep (its own integration, or
 *               coordinates the caller rewrote) do not invalidate it: conduction then sees that sweep's geometry, as in the
 *               sub-steps.  Call ParticleContextComputeForces first to conduct over rewritten coordinates.
 *   travel      temperature and pending energy follow the particle through ParticleContextRemove; particles inserted by
 *               ParticleContextAdd get T_init; ParticleContextCopy carries the heat state (dst becomes what src is);
 *               ParticleContextSave writes <group>/temp when heat is on, ParticleContextLoad reads it when the file has it
 *               and heat is on (the file holds no heat configuration; with heat off the dataset is skipped with a line
 *               on stderr).
 * A heat step is three small launches (one when k_p <= 0); nothing is allocated or synchronised per call: the per-node
 * buffers are sized when heat is set on a coupled context or the coupling is set on a context with heat. */
typedef struct DflParticleHeat {
    f64 cp_p;        /* particle specific heat            (> 0, required)                              */
    f64 k_p;         /* particle conductivity for contact conduction; <= 0: no contact conduction      */
    f64 cp_f, k_f;   /* fluid specific heat / conductivity; <= 0: the reference's kCP = 1, kKAPPA = 0.66 */
    f64 T_init;      /* temperature of every particle at the call, and of particles inserted later      */
    b32 two_way;     /* DflTimeStep feeds the particles' heat back into the T rows                      */
} DflParticleHeat;
/* cfg NULL: off, frees the state.  A call with a configuration sets every temperature to T_init and clears what is pending;
 * cp_p <= 0 is reported on stderr and leaves the context unchanged */
void ParticleContextSetHeat(ParticleContext* ctx, const DflParticleHeat* cfg);
f64* ParticleContextTemperature(ParticleContext* ctx);           /* device [P], writable; NULL when off; valid until Add / Remove */
const f64* ParticleContextHeatRate(const ParticleContext* ctx);  /* device [P]: W into each particle, last step; NULL when off */
void ParticleContextHeatStep(ParticleContext* ctx, const f64* w);/* one thermal sub-step; w NULL or uncoupled: conduction only */
/* q (device [N]) <- the heat given to the fluid per node and unit time since the last call (zero when no coupled sub-step
 * ran); resets it.  Needs heat on and a coupled context */
void ParticleContextHeatSource(ParticleContext* ctx, f64* q);
void DflMeshSetHeatSource(Mesh3D* mesh, const f64* q);           /* device [N], NULL = none; must outlive registration */

/* ---- laser energy deposition (build-defined; opt-in) -------------------------------------------------------------------
 * The reference has no source term in its T equation.  A context that never calls ParticleContextSetLaser with a
 * configuration computes bit for bit what it computes without this section, through the same launches.  The laser needs
 * particle heat on (ParticleContextSetHeat).  One GPU only.
 *   beam       collimated and Gaussian: a point `origin` on the axis, the direction `dir` (normalised by the library:
 *              dir / sqrt((d0 d0 + d1 d1) + d2 d2)), power P, 1/e^2 radius w: I(rho) = 2P / (pi w^2) exp(-2 rho^2 / w^2)
 *              at distance rho from the axis.  The axis translates with scan_vel: every laser step first advances the
 *              elapsed time, t += dt (t = 0 at the call that set the laser), and then uses o = origin + scan_vel t, the
 *              axis at the END of the sub-step, where the sub-step's integration has put the particles.
 *   frame      k = the coordinate axis least aligned with dir (smallest |dir_k|, the lowest k on a tie);
 *              e1 = (a_k - dir_k dir) / |a_k - dir_k dir|, e2 = dir x e1.  A point x has transverse coordinates
 *              u = (x - o) . e1, v = (x - o) . e2 and depth s = (x - o) . dir, every dot product evaluated as
 *              (d0 a0 + d1 a1) + d2 a2 in IEEE double without fused multiply-add.
 *   columns    n x n square columns of edge h centred on the axis, n = 2 ceil(r_cut / h) <= 256, h >= 2 Rmax; column
 *              (i, j), id i + n j, holds floor(u / h) = i - n/2 and floor(v / h) = j - n/2.  Its power is
 *              P_c = ((P / 4) gx[i]) gy[j], gx[i] = erf(sqrt2 x_{i+1} / w) - erf(sqrt2 x_i / w), x_i = (i - n/2) h, gy = gx,
 *              computed on the host with the C library's erf.  P - sum_c P_c falls outside the grid.
 *   shadowing  Beer-Lambert per column.  A particle belongs to the column holding the projection of its centre; outside
 *              the grid it is unlit.  Within a column the particles are ordered by depth s ascending, ties by ascending
 *              id.  With A_i = pi r_i^2, a = h^2: p_in = P_c exp(-sum_{j before i} A_j / a); particle i intercepts
 *              p_in (1 - exp(-A_i / a)), evaluated as -expm1(-A_i / a), and absorbs the fraction eta_p of it
 *              (laser_rate_i, W); the rest of what it intercepts is scattered and leaves the beam.  A particle deeper
 *              than its column's substrate hit (s > s_hit) is unlit and shadows nothing; a particle AT the hit depth is
 *              lit.  The laser_rate of an unlit particle, outside the grid or behind the hit, is +0.0.
 *   substrate  on a coupled context with substrate_groups != 0: the candidate faces are the boundary faces of the coupled
 *              mesh in those groups (bit g = group g, the records of ParticleContextSetWallMesh) whose inward normal
 *              opposes the beam, n . dir < 0.  Each column's centre ray ((i - n/2 + 1/2) h, (j - n/2 + 1/2) h) is
 *              deposited on the first candidate face whose projection holds it (edges included): the smallest depth
 *              of the hit point, depths compared on a grid of 2^-40 of the candidates' depth range, ties by the lowest
 *              face id -- so a ray through a shared edge or vertex has exactly one owner.  The column's transmitted power
 *              T_c = P_c exp(-sum A_j / a) splits into eta_s T_c absorbed and (1 - eta_s) T_c reflected; the absorbed part
 *              goes to the face's three nodes by the barycentric weights of the hit point (nodal power in W, the unit of
 *              DflMeshSetHeatSource).  A column without a hit (uncoupled context, mask 0, a ray that leaves through an
 *              open group) books T_c as missed.  The face list is a snapshot of the mesh, built once per (coupled mesh,
 *              mask, direction); at most 2^24 candidate faces.
 *   tally      DflLaserTally holds the power of the last laser step in W; its six entries sum to P up to rounding.
 *   time step  a laser step runs inside every thermal sub-step (ParticleContextUpdate, ParticleContextFluidStep, the DEM
 *              sub-steps of DflTimeStep, ParticleContextHeatStep) with the context's dt, before the heat update, which sees
 *              q_i + laser_rate_i where it sees q_i without a laser.  The substrate's nodal energy accumulates over the
 *              steps (+= dt power); ParticleContextHeatSource adds energy / (time of those steps) to the q it returns
 *              and clears it, so the two-way path of DflTimeStep puts the laser on the T rows.  ParticleContextLaserStep
 *              is the bare step (bin, attenuation, deposit, tally; no temperature update), also with zero particles.
 *   travel     ParticleContextCopy carries the configuration and the elapsed scan time (dst becomes what src is; substrate
 *              energy still pending on src is not copied: dst starts with none); laser_rate is recomputed by every step
 *              and is not carried by Remove / Add.  ParticleContextSetFluidCoupling rebuilds the substrate list for the
 *              new mesh (none when uncoupled: every column then books its power as missed) and drops pending energy.
 *   limits     h >= 2 Rmax is checked at ParticleContextSetLaser only: sizes set later (ParticleContextSetSizes,
 *              SetInflowSizes) are the caller's to keep below h / 2; a larger particle is still binned by its centre
 *              and its A / a may exceed 1.  Non-finite particle coordinates are not supported (the depth order of that
 *              particle's column is then undefined; nothing is written out of bounds).
 * Column runs longer than the column kernel's LDS cap (512 particles) take a slower path with the same result.  A step
 * allocates nothing and does not wait for the device; the state is sized at ParticleContextSetLaser and again when the
 * coupling or the particle capacity changes; only ParticleContextLaserTally copies to the host. */
typedef struct DflLaser {
    f64 origin[3], dir[3], scan_vel[3];
    f64 power, w, h, r_cut;        /* P (W), 1/e^2 radius, column edge, cut-off radius of the column grid */
    f64 eta_p, eta_s;              /* absorptivity of the powder / of the substrate, in [0, 1] */
    index_type substrate_groups;   /* boundary groups of the coupled mesh that receive the transmitted beam; 0: none */
} DflLaser;
typedef struct DflLaserTally {
    f64 outside, absorbed_particles, scattered, substrate, reflected, missed;
} DflLaserTally;
/* the configuration is copied; NULL: off, frees the state.  Reported on stderr, context unchanged: heat off, a zero dir,
 * non-finite or non-positive w, h, r_cut, a negative power, an eta outside [0, 1], n > 256, h < 2 Rmax */
void ParticleContextSetLaser(ParticleContext* ctx, const DflLaser* cfg);
void ParticleContextLaserStep(ParticleContext* ctx, f64 dt);
const f64* ParticleContextLaserRate(const ParticleContext* ctx); /* device [P] by id: W absorbed in the last step; NULL when off */
void ParticleContextLaserTally(ParticleContext* ctx, DflLaserTally* out); /* the last step's (synchronises); zeros when off */
/* device [n n], read-only: every column's transmitted power and the record id of the face it hit (-1: none; -2 - tet for
 * a hit on the level-set surface inside that tet, see "laser on the level-set surface"); returns n n (0 and NULL pointers
 * when off) */
index_type ParticleContextLaserColumns(const ParticleContext* ctx, const f64** transmitted, const index_type** face);

/* ---- laser on the level-set surface (build-defined; opt-in) -------------------------------------------------------------
 * The sections around this one place the metal surface phi = level inside the mesh, with gas above; the substrate of "laser
 * energy deposition" is boundary faces only.  With a laser surface set the transmitted beam is also deposited on the
 * surface phi = level.  A context that never sets one, or clears it with NULL, computes bit for bit what it computes
 * without this section, through the same launches.  One GPU only.  No fused multiply-add anywhere; every dot product is
 * (x0 y0 + x1 y1) + x2 y2.
 *   snapshot   ParticleContextLaserSurfaceUpdate reads phi = w[4N, 5N) of the coupled mesh.  The candidate facets are the
 *              facets of "level-set redistancing" (per cut tet one triangle, or a quad as two), in ascending tet id, a
 *              quad's first triangle first, kept only where (1) the tet's gradient g = sum_a phi_a grad N_a has
 *              side (g . dir) > 0 -- the beam enters the metal there; a NaN is not greater --, (2) all nine coordinates of
 *              the facet are finite and (3) |g| > 0.  Every facet vertex is a crossing point P_ij = x_i + t (x_j - x_i),
 *              t = f_i / (f_i - f_j), f = phi - level; its weights in the tet are 1 - t at local node i, t at j, 0
 *              elsewhere.  The list is compacted by per-workgroup counts and a scan: its order does not depend on arrival.
 *              The surface moves on the fluid's time scale: the snapshot is taken by Update (and by DflTimeStep, below),
 *              never by a laser step; before the first Update there are no facets.
 *   first hit  the boundary candidates of substrate_groups and the facets compete per column centre ray: the facets are
 *              appended to the candidate list behind the boundary records, with record id -2 - tet, and the smallest depth
 *              wins on one depth grid; a tie on the grid goes to the lower list index (boundary faces before facets, facets
 *              in list order).  With a surface set the depth grid spans x . dir over the eight corners of the coupled
 *              mesh's node bounding box (computed at Set and when the coupling changes) instead of the boundary candidates'
 *              range.  At most 2^24 records in total: beyond that the facets are dropped with a line on stderr and the
 *              step behaves as if there were no snapshot.
 *   column     unchanged: s_hit is the winner's depth, particles deeper than it are unlit and shadow nothing, T_c splits
 *              into eta_s T_c absorbed (the `substrate` entry of the tally) and (1 - eta_s) T_c reflected; `missed` gets
 *              only the columns without any hit.
 *   deposit    with w_0..2 the barycentric weights of the centre ray in the projected facet (as for a boundary face) and
 *              c_ka the weight of facet vertex k at local node a of the facet's tet, lambda_a = (w_0 c_0a + w_1 c_1a) +
 *              w_2 c_2a, and power[n] = the sum, from +0.0 over the columns c that hit a facet in ascending column id, of
 *              (eta_s T_c) lambda_a(c) for the local node a of that column's tet that is n.  No floating-point atomics;
 *              bitwise reproducible.  A step costs O(columns + candidates), nothing of the size of the mesh.  Energy
 *              accumulates as += dt power; ParticleContextHeatSource adds energy / time to q and clears it, exactly as for
 *              the boundary substrate.
 *   time step  DflTimeStep calls Update once per call when a surface is set on a context coupled to its mesh: after the
 *              redistancing of wgold if that is due and before the first particle sub-step, with the fluid state those
 *              sub-steps see.  ParticleContextFluidStep / HeatStep / LaserStep never update.  The beam axis still moves per
 *              sub-step with scan_vel; the facets stay fixed between Updates.  Energy pending when an Update replaces the
 *              node list is kept and reaches the next heat source.
 *   travel     ParticleContextCopy carries the configuration, not the snapshot or pending energy.
 *              ParticleContextSetFluidCoupling drops the snapshot and pending energy and recomputes the depth range.
 *              ParticleContextSetLaser on a context with a surface keeps the surface configuration and drops the snapshot. */
typedef struct DflLaserSurface {
    f64 level; index_type side;   /* the surface phi = level; metal where side (phi - level) > 0, side = +-1 */
} DflLaserSurface;
/* the configuration is copied; NULL: off, frees the state.  Reported on stderr, context unchanged: the laser is off, the
 * context is uncoupled, side is not +-1, level is not finite */
void ParticleContextSetLaserSurface(ParticleContext* ctx, const DflLaserSurface* cfg);
/* the snapshot at the device 6N state w: returns the number of candidate facets, -1 when off.  Waits for the device once
 * (the count); grows its lists only when the count exceeds their capacity */
index_type ParticleContextLaserSurfaceUpdate(ParticleContext* ctx, const f64* w);
/* the snapshot's device lists [nf][9] and [nf] (the tet of every facet), valid until the next Update or Set; returns nf
 * (-1 when off, 0 and NULL pointers before the first Update) */
index_type ParticleContextLaserSurfaceFacets(const ParticleContext* ctx, const f64** facets, const index_type** tet);
/* the last laser step's nodal surface power in W into the device array q[N], overwritten in full (zero where nothing was
 * deposited).  For callers and tests; no step calls it */
void ParticleContextLaserSurfacePower(ParticleContext* ctx, f64* q);

/* ---- laser reflections (build-defined; opt-in) ---------------------------------------------------------------------------
 * "laser on the level-set surface" ends at the first hit: (1 - eta_s) T_c leaves the simulation, and eta_s does not depend on
 * the angle of incidence.  With a reflection set on a context that has a laser and a laser surface, a column ray that hits a
 * facet of the snapshot is reflected specularly and followed for up to max_bounce reflections over all facets of
 * phi = level, and deposits at every hit a share given by the constant eta_s (model 0) or by a Fresnel approximation of the
 * angle of incidence (model 1).  A context that never sets one, or clears it with NULL, computes bit for bit what it computes
 * without this section, through the same launches.  One GPU only.  No fused multiply-add anywhere; every dot product is
 * (a0 b0 + a1 b1) + a2 b2, every cross product (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0).
 *   list R     with a reflection set, ParticleContextLaserSurfaceUpdate also builds the reflection list R: every facet of
 *              phi = level that satisfies conditions (2) and (3) of the snapshot -- nine finite coordinates, |g| > 0 --
 *              without the side (g . dir) > 0 filter: a reflected ray travels in any direction.  R is in ascending tet id, a
 *              quad's first triangle first, and keeps per facet the tet, its gradient g and (i, j, t) of every vertex.  The
 *              candidate list stays what it is, bit for bit; it is a subset of R; the primary hit is found by the unchanged
 *              hit and column kernels.  The node list of the surface covers the nodes of every tet in R.  R's total rides on
 *              Update's one synchronisation.  At most 2^24 facets: beyond that no ray is reflected (a line on stderr).
 *              Setting or clearing a reflection drops the snapshot (pending energy is kept): the next Update takes a new one.
 *   rays       only a column whose primary hit is a facet (record id -2 - tet) starts a ray; a column that hits a boundary
 *              face, or nothing, behaves as without a reflection.  X_0 = (w_0 V_0 + w_1 V_1) + w_2 V_2 with w the weights
 *              of the centre ray in the projected facet and V its vertices; d_0 = dir (normalised); g_0 the gradient of the
 *              facet's tet; p_0 = T_c.  At bounce b (b = 0: the primary hit):
 *                c = |d . g| / sqrt((g . g) (d . d));
 *                model 0: A = eta_s;  model 1: A(c) = 1 - ((1 + (1 - eps c)^2) / (1 + (1 + eps c)^2)
 *                                                          + (eps^2 - 2 eps c + 2 c^2) / (eps^2 + 2 eps c + 2 c^2)) / 2;
 *                absorbed_b = A p_b;  p_{b+1} = p_b - absorbed_b.
 *              Under model 1 A(c_0) replaces eta_s for primary hits on facets; boundary faces keep eta_s.
 *              After bounce b = max_bounce the power left goes to `remaining`.  Otherwise the ray is reflected,
 *              d' = d - (2 (d . g) / (g . g)) g (no square root on the ray's path), and its next hit leaving tet t0 is looked
 *              for over all facets k of R with tet_k != t0 (this drops both triangles of a quad) and side (g_k . d') > 0
 *              (the ray enters the metal there; a NaN is not greater), by Moeller-Trumbore in this order:
 *                e1 = B - A, e2 = C - A, p = d x e2, det = e1 . p; skip the facet when det == 0;
 *                s = X - A, u = (s . p) / det, q = s x e1, v = (d . q) / det, tau = (e2 . q) / det;
 *                a hit iff u >= 0, v >= 0, u + v <= 1 and tau > 0.
 *              The smallest tau wins, compared as doubles; on a tie the lowest index in R.  Then
 *              X' = ((1 - u - v) A + u B) + v C, with 1 - u - v = (1 - u) - v, and g' = g_k.  No hit: the ray's power goes
 *              to `escaped`.  This test is the definition; it is not watertight along shared edges.
 *   deposit    at a hit with facet weights (w_0, w_1, w_2) -- primary: those of the centre ray; later: (1 - u - v, u, v) --
 *              lambda_a is formed as in "laser on the level-set surface" from the facet's (i, j, t).  The record (bounce b,
 *              column c, local node a) carries absorbed_b lambda_a; nodal power is the sum, from +0.0, of a node's records
 *              in ascending (b n^2 + c) 4 + a: bounce-major, then column id.  With only bounce-0 records this is the order of
 *              the surface alone.  No floating-point atomics; bitwise reproducible.  Energy accumulates and reaches
 *              ParticleContextHeatSource exactly as for the surface.
 *   tallies    DflLaserTally: `substrate` = boundary hits + the sum over b of absorbed[b] (per column in ascending b, then
 *              the columns' tree), `reflected` = boundary reflections + escaped + remaining; the six entries still sum to P
 *              up to rounding.  One exception in the last bit: under model 0 a ray that finds no second facet leaves its
 *              column's entries as the column kernel booked them, eta_s T_c and (1 - eta_s) T_c, so that the six entries of a
 *              surface without second hits have the bits of a step without reflections.  DflLaserReflectionTally is that of the last laser step.
 *   limits     reflected rays see neither particles nor boundary faces; a ray that leaves the node bounding box has escaped;
 *              specular reflection only, one ray per column.
 *   search     the next hit is the minimum over all of R by definition.  Update enters the facets of R into a uniform grid
 *              over the coupled mesh's node bounding box (every cell that the box of a facet's vertices overlaps; n cells per
 *              axis, n = ceil(sqrt(|R| / 4)) <= 128, or DFL_LASER_REFLECT_CELLS = 1 .. 256 as read by Set), which costs one
 *              more read of four bytes in Update.  A lane group per ray (a wave; DFL_LASER_REFLECT_GROUP = 16 or 64) walks
 *              the layers of cells along the ray's dominant axis -- in each the rectangle that the ray's entry and exit
 *              points span, padded by one cell, starting one layer behind the ray's origin -- and stops one layer behind
 *              the best hit so far.  The grid changes no bit of the result for rays that decide with a margin (a facet hit
 *              only through rounding, more than a cell away from the exact ray, could be missed).
 *   travel     ParticleContextSetLaserSurface(ctx, NULL) also clears the reflection; a new surface configuration keeps it.
 *              ParticleContextSetLaser keeps the reflection configuration and drops the snapshot; ParticleContextCopy
 *              carries the configuration, not the lists; ParticleContextSetFluidCoupling drops the lists. */
typedef struct DflLaserReflection {
    index_type max_bounce;   /* 1 .. 8: reflections followed per column ray */
    index_type model;        /* 0: eta_s at every facet hit; 1: Fresnel approximation with eps */
    f64 eps;                 /* model 1: material constant, finite and > 0 (ignored by model 0) */
} DflLaserReflection;
typedef struct DflLaserReflectionTally {
    f64 absorbed[9];         /* W absorbed at bounce b (b = 0: the primary hit on a facet), last laser step */
    f64 escaped;             /* W on rays that found no facet */
    f64 remaining;           /* W still on rays after bounce max_bounce */
    index_type rays[9];      /* rays that hit a facet at bounce b */
} DflLaserReflectionTally;
/* host only; 0 = accepted, otherwise the reason in why (when not NULL): max_bounce outside 1..8, model not 0 or 1, eps not
 * finite or not > 0 under model 1 */
int DflLaserReflectionCheck(const DflLaserReflection* cfg, char* why, size_t why_len);
/* the configuration is copied; NULL: off, frees the state.  Reported on stderr, context unchanged: the laser or the laser
 * surface is off, or DflLaserReflectionCheck refuses */
void ParticleContextSetLaserReflection(ParticleContext* ctx, const DflLaserReflection* cfg);
void ParticleContextLaserReflectionTally(ParticleContext* ctx, DflLaserReflectionTally* out); /* synchronises; zeros when off */
/* device, read-only, valid until the next laser step: for (b, c), index b n n + c, the facet hit at bounce b as an index
 * into the reflection list (-1: none) and the power absorbed there; returns (max_bounce + 1) n n, 0 when off or before the
 * first step with a reflection list */
index_type ParticleContextLaserReflectionRays(const ParticleContext* ctx, const index_type** facet, const f64** absorbed);
/* the reflection list of the last Update: facets [nr][9], their tets [nr], the tets' gradients [nr][3]; -1 when off */
index_type ParticleContextLaserReflectionFacets(const ParticleContext* ctx, const f64** facets, const index_type** tet, const f64** grad);

/* ---- melt-pool capture (build-defined; opt-in) ---------------------------------------------------------------------------
 * The reference's particle hooks are empty and its continuity equation has no source.  A context that never calls
 * ParticleContextSetCapture with a configuration, and a mesh that never gets a volume source, compute bit for bit what they
 * compute without this section, through the same launches.  The context must be coupled to a mesh
 * (ParticleContextSetFluidCoupling).  One GPU only.  A particle that reaches the metal surface phi = level where the fluid
 * is molten leaves the particle set and joins the fluid as mass, momentum and heat.
 *   decision    ParticleContextCapture first runs ParticleContextLocate.  For particle i in tet t = tet_i >= 0 with nodes
 *               n_a = ien[4t + a] and weights lambda_a, I(f) = ((lambda_0 f_0 + lambda_1 f_1) + lambda_2 f_2) + lambda_3 f_3
 *               without fused multiply-add; phi_p = I(w[4N + n_a]), T_f = I(w[5N + n_a]), u_f as the drag computes it.
 *               g = sum_a phi_a grad N_a, the tet's constant gradient, from the node coordinates x_a in closed form: with
 *               e_k = x_k - x_0, c23 = e_2 x e_3, c31 = e_3 x e_1, c12 = e_1 x e_2 and det = (e_1 . c23),
 *                 g_d = (((phi_1 - phi_0) c23_d + (phi_2 - phi_0) c31_d) + (phi_3 - phi_0) c12_d) / det,
 *               |g| = sqrt((g0 g0 + g1 g1) + g2 g2).  c_i = side (phi_p - level) + (reach r_i) |g|: for a distance-like phi
 *               (|g| = 1) reach = 0 asks the centre to cross the surface and reach = 1 the sphere to touch it.  Captured
 *               iff t >= 0, c_i >= 0 and T_f >= T_melt; a NaN anywhere captures nothing; particles at tet -1 or -2 are
 *               kept (removing those is the outflow's job).
 *   deposits    of a captured particle, with m_i, r_i the particle's mass and radius (ParticleMass / ParticleRadius when
 *               monodisperse): volume V_i = m_i / rho_f (rho_f of the coupling: mass is conserved in the single-density
 *               fluid), excess momentum dP_i = m_i (v_i - u_f), excess heat E_i = (m_i cp_p)(T_i - T_f) with heat on, else
 *               0.  The latent heat of the particle is not deposited (the phase-change section below models the fluid's).
 *   nodes       one accumulator A[N][5] = (vol, mom0, mom1, mom2, heat), A[n_a] += lambda_a (V_i, dP_i, E_i), summed in
 *               the fixed order of the reaction load (particles sorted by tet, stable by id; nodes walk their sorted V2E
 *               lists) by one sort and one node pass for all five components: no float atomics, bitwise reproducible;
 *               sum_a A[a] = the sum over the captured particles to rounding.  The drag impulse and the convective energy
 *               still pending on a captured particle go where ParticleContextRemove sends them.
 *   compaction  the stable compaction of ParticleContextRemove: survivors keep their order and every carried field, friction
 *               history partners are remapped, entries whose partner was captured are dropped.  ParticleContextSetCapture
 *               creates the tags as the first Set*flow call does.  A call reads 4 bytes back (the new count), allocates
 *               nothing and does nothing further when no particle was captured.
 *   source      ParticleContextCaptureSource(ctx, time, q_vol, load, q_heat) writes A / time into q_vol [N] (m^3/s),
 *               load [3N] (N) and q_heat [N] (W) -- any of them may be NULL, which drops that part -- and clears A.  The
 *               caller gives the time window: a deposit applied as a rate over a fluid step of that length delivers
 *               exactly the deposited amount.  time <= 0 is an ASSERT.
 *   p rows      with a volume source registered (DflMeshSetVolumeSource) every F assembly subtracts it from F[3N:4N): the
 *               residual is R_p = (...) - q_V, after the tet and face terms and before the Dirichlet rows, so the converged
 *               field has int N_a div u = q_V[a]: the velocity diverges where metal arrives, the level set moves out with
 *               u, and the liquid volume grows by the deposited volume.  Explicit: not in J.
 *   time step   with two_way and something pending, DflTimeStep takes the source with time = dt (the mesh's time step), registers q_vol as the
 *               volume source (one already registered is an ASSERT, as for the load), adds the momentum rate to the load
 *               and the heat rate to the heat source it registers (in the capture's own buffers, together with the reaction
 *               load / particle heat source when those are pending too) and restores the caller's registrations after the
 *               solve.  After the particle sub-steps it calls ParticleContextCapture(pctx, wgold), then
 *               ParticleContextRemove.  That call locates the particles at their positions after the sub-steps whether or
 *               not it captures anything, as ParticleContextRemove with outside_mesh does: with capture set, a two-way
 *               reaction load or heat source taken afterwards is spread with the weights of those positions, not with
 *               those of the last sub-step's locate, so a two-way coupled run with capture set that never fires agrees
 *               with the run without capture to the change of those weights, not bit for bit.  One-way runs are
 *               bit-identical.
 *   travel      ParticleContextCopy carries the configuration (to a coupled dst), not the pending A;
 *               ParticleContextSetFluidCoupling on another mesh resizes A and drops what was pending; Save / Load are
 *               untouched: capture has no per-particle state. */
typedef struct DflParticleCapture {
    f64 level;        /* phi value of the metal surface */
    index_type side;  /* +1: metal where phi > level, -1: metal where phi < level (anything else: refused on stderr) */
    f64 reach;        /* >= 0, in particle radii: 0 = the centre must cross, 1 = the sphere touches the surface */
    f64 T_melt;       /* captured only where the fluid has T_f >= T_melt; -HUGE_VAL: anywhere */
    b32 two_way;      /* DflTimeStep puts the deposits on the p, momentum and T rows */
} DflParticleCapture;
typedef struct DflParticleCaptureStats {
    int64_t captured; /* since capture was first set on the context */
    index_type last;  /* by the last ParticleContextCapture */
} DflParticleCaptureStats;
/* the configuration is copied; NULL: off, frees the state.  Reported on stderr, context unchanged: side not +-1, reach < 0
 * or not finite, an uncoupled context */
void ParticleContextSetCapture(ParticleContext* ctx, const DflParticleCapture* cfg);
index_type ParticleContextCapture(ParticleContext* ctx, const f64* w); /* w: device 6N fluid state; returns the number captured */
void ParticleContextCaptureSource(ParticleContext* ctx, f64 time, f64* q_vol, f64* load, f64* q_heat);
void ParticleContextCaptureStats(const ParticleContext* ctx, DflParticleCaptureStats* out); /* zeros when off */
void DflMeshSetVolumeSource(Mesh3D* mesh, const f64* q_vol);     /* device [N], m^3/s; NULL = none; must outlive registration */
const f64* DflMeshVolumeSource(const Mesh3D* mesh);

/* ---- solid-surface contact (build-defined; opt-in) ----------------------------------------------------------------------
 * Particle walls are boundary faces of a mesh; the metal surface phi = level lies inside the mesh, and capture takes a
 * particle that reaches it only where the fluid is molten.  With a surface contact set, every coupled sub-step
 * (ParticleContextFluidStep, hence the coupled DEM sub-steps of DflTimeStep) also collides every particle with the implicit
 * surface phi = level wherever the fluid there counts as solid.  A context that never calls ParticleContextSetSurfaceContact
 * with a configuration, or clears it with NULL, computes bit for bit what it computes without this section, through the same
 * launches.  The context must be coupled to a mesh (ParticleContextSetFluidCoupling).  One GPU only.  ParticleContextUpdate
 * (the uncoupled step) never runs it.  No fused multiply-add anywhere; every dot product is (a0 b0 + a1 b1) + a2 b2.
 *   where       inside ParticleContextFluidStep, after the contact sweep and ParticleContextLocate and before the drag and
 *               the integration: one launch, one thread per particle.  It sees the positions, velocities and angular
 *               velocities the sweep saw, the tets and weights of this sub-step's locate and the fluid state w of the call.
 *   quantities  for particle i in tet t = tet_i >= 0: lambda_a, phi_p = I(w[4N + n_a]), T_f = I(w[5N + n_a]), the tet's
 *               gradient g and |g| exactly as "melt-pool capture" defines them (the same device functions).  Then, with
 *               r_i, m_i the particle's radius and mass (ParticleRadius / ParticleMass when monodisperse),
 *                 f = phi_p - level,  q = -(side f),  s = q / |g|,  n_d = (-(side g_d)) / |g|:
 *               s is the centre's distance from the surface, positive on the gas side, and n the unit normal towards the
 *               gas, that is, towards the particle.  side is +-1, so q and side g_d carry no rounding.
 *   decision    contact iff t >= 0, |g| > 0, -r_i < s < r_i and T_f < T_solid.  A NaN anywhere compares false: no contact.
 *               Tets -1 and -2: no contact.  s <= -r_i with the other conditions true is "buried": no force, as the walls
 *               treat a centre further than R behind a face; it is counted.  With T_solid equal to capture's T_melt exactly
 *               one of contact and capture applies to a particle that touches the surface.
 *   normal law  that of the pairs and walls, the wall at rest, not clamped:
 *                 delta = r_i - s,  v_n = (v_0 n_0 + v_1 n_1) + v_2 n_2,  f_n = kn delta - gamma_n v_n
 *               with kn, gamma_n of ParticleContextSetContactModel.
 *   friction    off: F_d = f_n n_d.  On (ParticleContextSetFriction): the law of "contact friction and particle rotation"
 *               for a wall at rest, by the sweeps' own device function, with lever ell = max(r_i - delta, 0), v = v_i,
 *               w = omega_i; F_d = f_n n_d + F_t,d and torque tau = (-ell n) x F_t.  The history key is
 *                 1 << 62 | 1 << 61             the surface phi = level
 *               which no plane id (31 bits) and no unit-box wall can equal.  The spring is looked up in the row the previous
 *               sweep left (which holds the surface entry of the previous sub-step) and the new entry is appended to the
 *               row this sub-step's sweep wrote, behind the sweep's entries; the capacity and the overflow rule are those
 *               of that section (a full row: the force of a new contact, nothing stored, counted).  The entry is dropped by
 *               the first sweep after the particle has left the surface.  ParticleContextRemove leaves the key alone, as it
 *               does the wall keys.
 *   result      acc_d <- acc_d + F_d (1 / m_i), and with friction alpha_d <- alpha_d + tau_d (1 / I_i), I_i = 2/5 m_i r_i^2
 *               as that section evaluates it, added to what the sweep wrote.  A particle without contact is not written:
 *               its acc, alpha and history row keep the sweep's bits.
 *   energy      the contact is adiabatic, as the walls are, and exerts no reaction on the fluid: the solid metal is held by
 *               the mushy-zone drag of "phase change", not by the particles.
 *   geometry    the contact is exact for a distance-like phi that is linear in the centre's tet: phi is extrapolated
 *               linearly from the centre's tet over the distance r_i, the approximation capture's `reach` already makes;
 *               "level-set redistancing" keeps it good.
 *   stats       integer counters on the device, at most one atomic per wave, read only by
 *               ParticleContextSurfaceContactStats (which waits for the device): `last` and `buried` of the last sub-step,
 *               `total` = particle-sub-steps in contact since the configuration was last set.
 *   travel      ParticleContextSetFluidCoupling with NULL frees the state; coupling to another mesh keeps the configuration
 *               and the counters; ParticleContextCopy carries the configuration to a coupled dst (not the counters).  A
 *               sub-step allocates nothing and does not wait for the device; the state is sized at Set.  The kernel lets a
 *               particle far on the gas side go before it gathers T and the coordinates, by a bound on |grad N| over the mesh
 *               that never changes a decision; one pass over the tets computes it at Set, when the coupling changes and, as
 *               a second launch, in the first sub-step after DflMeshGeometryChanged.
 *   limits      not modelled: conduction between a resting particle and the substrate; a moving solid (the wall is at rest);
 *               a reaction force on the fluid; more than one GPU; a facet-based contact for meshes much finer than the
 *               particles (a sphere larger than its tet still sees that tet's plane only). */
typedef struct DflSurfaceContact {
    f64 level;        /* phi value of the metal surface */
    index_type side;  /* +1: metal where phi > level, -1: metal where phi < level (as DflParticleCapture.side) */
    f64 T_solid;      /* contact only where the fluid has T_f < T_solid; HUGE_VAL: everywhere */
} DflSurfaceContact;
typedef struct DflSurfaceContactStats {
    index_type last, buried; /* particles in contact / buried in the last sub-step */
    int64_t total;           /* particle-sub-steps in contact since the configuration was last set */
} DflSurfaceContactStats;
/* host only; 0 when ParticleContextSetSurfaceContact accepts the configuration, else why not in `why`: side must be +1 or
 * -1, level finite, T_solid not a NaN */
int DflSurfaceContactCheck(const DflSurfaceContact* cfg, char* why, size_t why_len);
/* the configuration is copied; NULL: off, frees the state.  Reported on stderr, context unchanged: what the check refuses,
 * an uncoupled context */
void ParticleContextSetSurfaceContact(ParticleContext* ctx, const DflSurfaceContact* cfg);
void ParticleContextSurfaceContactStats(const ParticleContext* ctx, DflSurfaceContactStats* out); /* zeros when off */

/* ---- free-surface forces (build-defined; opt-in) ------------------------------------------------------------------------
 * The reference's level set carries no surface physics.  A mesh that never calls DflMeshSetSurfaceForces with a
 * configuration, or clears it with NULL, computes bit for bit what it computes without this section, through the same
 * launches.  One GPU only.  With a configuration the surface phi = level of the melt pool gets surface tension, the
 * Marangoni stress of a temperature-dependent sigma, the recoil pressure of the evaporating metal and the surface heat loss,
 * as a smeared interface with every term explicit, evaluated at the state w the caller passes.
 *   tet         with nodes n_a = ien[4e + a], coordinates x_a, phi_a = w[4N + n_a], T_a = w[5N + n_a]; grad N_a and det in
 *               the closed form of the capture section: e_k = x_k - x_0, c23 = e_2 x e_3, c31 = e_3 x e_1, c12 = e_1 x e_2,
 *               det = e_1 . c23, grad N_1 = c23 / det, grad N_2 = c31 / det, grad N_3 = c12 / det,
 *               grad N_0 = -((c23 + c31) + c12) / det.  g = sum_a phi_a grad N_a as the capture section forms it,
 *               |g| = sqrt((g0 g0 + g1 g1) + g2 g2); a tet with !(|g| > 0) contributes nothing.  n = g / |g| and
 *               d_a = (phi_a - level) / |g|, the tet's own distance: the band keeps its physical half-width eps where phi is
 *               not a distance function.  A tet with all d_a >= eps or all d_a <= -eps contributes nothing.
 *   quadrature  the four points of the assembly, N_a(q) = 0.5854101966249685 (a = q) or 0.1381966011250105, weight 1/24:
 *               d_q = sum_a N_a(q) d_a, T_q = sum_a N_a(q) T_a, t = d_q / eps,
 *               delta_q = |t| < 1 ? 15 / (16 eps) (1 - t t)^2 : 0   (the biweight kernel: a polynomial, C1, integral 1),
 *               W_q = |det| / 24 delta_q,
 *               sigma_q = max(0, sigma0 + dsigma_dT (T_q - T_ref)),
 *               E_q = exp(recoil_a (1 - T_boil / T_q)) where T_q > 0, else the recoil and evaporation terms are 0,
 *               p_q = recoil_p0 > 0 ? recoil_p0 E_q : 0,
 *               loss_q = h_conv (T_q - T_amb) + emissivity kSB (T_q^4 - T_amb^4) + evap_q0 E_q sqrt(T_boil / T_q),
 *               kSB = 5.670374419e-8, each of the three only while its coefficient is > 0.
 *   tet node    S = sum_q W_q sigma_q,
 *               f_a    = -S (grad N_a - n (n . grad N_a)) + side n sum_q W_q p_q N_a(q)   (N),
 *               heat_a = -sum_q W_q loss_q N_a(q)                                         (W, the unit of DflMeshSetHeatSource),
 *               area_a =  sum_q W_q N_a(q)                                                (nodal share of the smeared area).
 *               The first term of f_a is the Laplace-Beltrami weak form -int sigma P : grad v with P = I - n n: it needs
 *               first derivatives of phi only, and a variable sigma gives the Marangoni stress without further code.  The
 *               recoil normal side n points into the metal, where side (phi - level) > 0.
 *   nodes       load[3a + d], q_heat[a], area[a] = the sums over node a's tets in ascending tet id, starting from +0.0:
 *               a one-byte-per-tet band pass and one launch over the nodes' sorted tet lists (csrc/k_surface.hip), no float
 *               atomics, bitwise reproducible, the same under every assembly schedule.  DFL_SURFACE_FLAGS=0 (read by
 *               DflMeshSetSurfaceForces) drops the band pass: the node pass then tests the band itself, with the same bits out.
 *   time step   with in_time_step, DflTimeStep evaluates load and q_heat at wgold before the predictor into buffers the
 *               mesh owns, adds the reaction / capture load and the particle / capture heat source that are pending, registers
 *               both (DflMeshSetExternalLoad, DflMeshSetHeatSource; one the caller registered already is an ASSERT, as for
 *               the reaction load) and restores the caller's registrations after the solve.  With a communicator it prints
 *               why and returns -1.
 * Explicit surface tension is stable only below the capillary time step, dt < sqrt(rho h^3 / (2 pi sigma)) with h the tet
 * size at the surface: keeping the step (DflMeshSetTimeStep) below it is the caller's condition: DflMeshTimeStepLimits reports it as dt_capillary.  The mass the
 * evaporation carries away is not modelled: evap_q0 is a heat loss only; the latent heat of melting is the phase-change
 * section's. */
typedef struct DflSurfaceForces {
    f64 level; index_type side; f64 eps;      /* surface phi = level; metal where side (phi - level) > 0; half-width of the band (length) */
    f64 sigma0, dsigma_dT, T_ref;
    f64 recoil_p0, recoil_a, T_boil;          /* recoil_p0 <= 0: no recoil */
    f64 h_conv, emissivity, T_amb, evap_q0;   /* each <= 0: that loss is off */
    b32 in_time_step;                         /* DflTimeStep applies load and heat loss itself */
} DflSurfaceForces;
/* the configuration is copied; NULL: off, frees everything of its own.  Reported on stderr, mesh unchanged: side not +-1, eps not
 * finite or not positive, any non-finite parameter, T_boil <= 0 while recoil or evaporation is on.  Has the mesh build the
 * sorted tet lists of the nodes if nothing did before (one copy per mesh, shared with the other features and freed with the
 * mesh) and builds every buffer here (synchronises): DflMeshSurfaceLoad allocates nothing and does not wait for the device */
void DflMeshSetSurfaceForces(Mesh3D* mesh, const DflSurfaceForces* cfg);
b32  DflMeshSurfaceForcesEnabled(const Mesh3D* mesh);
/* w: device 6N state; load [3N], q_heat [N], area [N] on the device, any of them NULL, every other one overwritten in full.
 * Without a configuration: a line on stderr, nothing written */
void DflMeshSurfaceLoad(Mesh3D* mesh, const f64* w, f64* load, f64* q_heat, f64* area);

/* ---- phase change: latent heat and mushy-zone drag (build-defined; opt-in) ----------------------------------------------
 * The reference's fluid has one phase.  A mesh that never calls DflMeshSetPhaseChange with a configuration, or clears it
 * with NULL, computes bit for bit what it computes without this section, through the same launches.  One GPU only.  With
 * a configuration the metal melts and freezes between T_solidus and T_liquidus: crossing the range costs the latent heat,
 * and the solid and the mushy zone resist the flow with a Darcy (Carman-Kozeny) drag.
 *   liquid      s = min(1, max(0, (T - T_solidus) / (T_liquidus - T_solidus))), fl = s s (3 - 2 s),
 *   fraction    fl' = 6 s (1 - s) / (T_liquidus - T_solidus), which is 0 where s is clamped;
 *               C(fl) = darcy_c (1 - fl)^2 / (fl^3 + darcy_b).  A NaN T gives fl = fl' = 0 and C = 0: a NaN freezes
 *               nothing and costs nothing.
 *   metal       with use_phi, per tet g, |g| and d_a = (phi_a - level) / |g| exactly as the free-surface section forms
 *   fraction    them (the same closed form, without fused multiply-add); d_q = sum_a N_a(q) d_a, m_q = Hs(side d_q / eps),
 *               Hs(t) = 0 for t <= -1, 1 for t >= 1, else 0.5 + 15/16 (t - 2/3 t^3 + 1/5 t^5): the integral of the
 *               biweight kernel of delta_q; a NaN t gives 0.  A tet with !(|g| > 0) has m_q = 1 if
 *               side (mean phi_a - level) > 0, mean = ((phi_0 + phi_1) + (phi_2 + phi_3)) / 4, else 0.  Without use_phi
 *               m_q = 1.
 *   tet to      the four quadrature points and W = |det| / 24 of the assembly, T_q = sum_a N_a(q) T_a:
 *   node          D_a += W N_a(q) m_q C(fl(T_q))          drag coefficient, kg/s
 *                 H_a += W N_a(q) m_q latent fl'(T_q)     latent heat capacity, J/K
 *                 G_a += W N_a(q) m_q fl(T_q)             the node's share of the liquid metal volume, m^3
 *   skip rules  part of the model, so that the flag pass and the node pass decide alike: a tet adds nothing to D, H and G
 *               if use_phi and all side d_a <= -eps (a tet with !(|g| > 0): if its m_q = 0); nothing to D and H if all
 *               T_a >= T_liquidus; nothing to G if all T_a <= T_solidus.
 *   nodes       D[a], H[a], G[a] = the sums over node a's tets in ascending tet id, starting from +0.0; a switched-off
 *               part (latent <= 0, darcy_c <= 0) gives exact +0.0.  One launch over the nodes' sorted tet lists (csrc/k_phase.hip)
 *               that applies the skip rules itself, no float atomics, bitwise reproducible, the same under every assembly
 *               schedule.  DFL_PHASE_FLAGS=1 (read by DflMeshSetPhaseChange) puts a one-byte-per-tet flag pass in front
 *               (bit 0: adds to D / H, bit 1: adds to G), DFL_PHASE_FLAGS=0 drops it again, with the same bits out
 *               either way; it is off by default because most tets stay (the whole substrate is solid) and the pass
 *               measures slower in front than left out.
 *   rows        implicit in the rates and lumped per node, with the coefficient evaluated inside the tets so that a mushy
 *               band thinner than an element is still seen.  Every F assembly adds, after the tet and face terms and the
 *               sources and before the T rows are saved for the scalar transport and the Dirichlet rows are applied,
 *                 R[3a + d] += D_a u_a[d]     (u from wgalpha),       R[5N + a] += H_a dT_a     (dT from dwgalpha),
 *               with D and H evaluated at (wgalpha, dwgalpha).  Every J assembly adds fact2 D_a, fact2 = dt kALPHAF kGAMMA,
 *               to the entries (d, d), d < 3, of node a's diagonal 4x4 block: D depends on T only, so this is the exact
 *               derivative with respect to the velocity rates.  J must have the block layout: drag with a
 *               reference-layout FS matrix is an ASSERT.  DflAssembleScalarJacobian adds kALPHAM H_a to the diagonal of
 *               the T Jacobian before its Dirichlet unit rows.  Products are rounded before the add (no fused
 *               multiply-add).  H is frozen over the Newton iteration: this is the apparent-heat-capacity Picard form.
 *               The exact term fact2 latent fl'' dT changes sign under cooling and can make the diagonal negative for
 *               realistic L / (cp dT); the frozen form keeps it positive and converges to the same residual.  The SUPG /
 *               PSPG parameters do not see C: where C is large, u is approximately 0 and the stabilisation is idle.
 *   stats       liquid volume = sum_a G_a (a fixed two-stage order), T_max over the metal nodes (a NaN is passed over),
 *               number and bounding box of the molten nodes: fl(T_a) >= 0.5 and metal (!use_phi or
 *               side (phi_a - level) > 0).  An empty set gives count 0, lo = +inf, hi = -inf (and T_max = -inf).
 * Limits: one GPU (SolveFlowSystem and DflTimeStep with a communicator print why and return -1); H frozen per Newton
 * iteration; C not in the stabilisation; no volume change on freezing (one density). */
typedef struct DflPhaseChange {
    f64 T_solidus, T_liquidus;      /* T_liquidus > T_solidus */
    f64 latent;                     /* rho L, J/m^3; <= 0: no latent heat */
    f64 darcy_c, darcy_b;           /* C(fl) = darcy_c (1-fl)^2 / (fl^3 + darcy_b), kg/(m^3 s); darcy_c <= 0: no drag; darcy_b > 0 */
    b32 use_phi; f64 level; index_type side; f64 eps;   /* metal where side (phi - level) > 0, smeared over eps; use_phi 0: metal everywhere */
} DflPhaseChange;
typedef struct DflPhaseChangeStats {
    f64 liquid_volume;  /* sum_a G_a */
    f64 T_max;          /* over the metal nodes */
    int64_t molten;     /* nodes with fl >= 0.5 that are metal */
    f64 lo[3], hi[3];   /* their bounding box */
} DflPhaseChangeStats;
/* the configuration is copied; NULL: off, frees everything of its own.  Reported on stderr, mesh unchanged: any non-finite
 * parameter, T_liquidus <= T_solidus, darcy_b <= 0 while drag is on, use_phi with side not +-1 or eps <= 0.  Has the mesh
 * build the sorted tet lists of the nodes if nothing did before (shared, freed with the mesh) and builds every buffer here
 * (synchronises): the later calls allocate nothing and, but for the stats, do not
 * wait for the device */
void DflMeshSetPhaseChange(Mesh3D* mesh, const DflPhaseChange* cfg);
b32  DflMeshPhaseChangeEnabled(const Mesh3D* mesh);
/* host only: 0 when DflMeshSetPhaseChange accepts the configuration, else why not in `why` */
int  DflPhaseChangeCheck(const DflPhaseChange* cfg, char* why, size_t why_len);
/* w: device 6N state; D, H, G [N] on the device, any of them NULL, every other one overwritten in full.  Without a
 * configuration: a line on stderr, nothing written */
void DflMeshPhaseCoefficients(Mesh3D* mesh, const f64* w, f64* D, f64* H, f64* G);
/* the statistics at the state w (synchronises, reads 72 bytes back); without a configuration: a line on stderr, the
 * empty-set values */
void DflMeshPhaseChangeStats(Mesh3D* mesh, const f64* w, DflPhaseChangeStats* out);

/* ---- thermal material: conductivity and heat capacity follow phi (build-defined; opt-in) --------------------------------
 * The reference's heat equation has one material: the T rows use kKAPPA = 0.66 and kRHO kCP = 1000 everywhere, so the
 * shielding gas conducts and stores heat as the metal does.  A mesh that never calls DflMeshSetThermalMaterial with a
 * configuration, or clears it with NULL, computes bit for bit what it computes without this section, through the same
 * launches.  One GPU only.  With a configuration the Galerkin part of the T rows becomes the one with the conductivity k_q
 * and the capacity c_q below, by a correction with the differences to the built-in constants.
 *   per tet     grad N_a, det, g, |g|, d_a, d_q, m_q = Hs(side d_q / eps) and the rule for a tet with !(|g| > 0) exactly as
 *               the phase-change section forms them (the same closed form, without fused multiply-add); without use_phi
 *               m_q = 1.  T_q = sum_a N_a(q) T_a, fl_q = fl(T_q), the smoothstep of the phase-change section between
 *               T_solidus and T_liquidus; a NaN T_q gives 0, and fl_q = 0 when k_liquid == k_solid (the two temperatures are
 *               then not read).
 *                 k_q = k_gas + m_q ((k_solid + fl_q (k_liquid - k_solid)) - k_gas)      dk_q = k_q - kKAPPA
 *                 c_q = c_gas + m_q (c_metal - c_gas)                                    dc_q = c_q - kRHO kCP
 *               W = |det| / 24 and the four quadrature points of the assembly.
 *   rows        at the alpha states (T, u from wgalpha, dT from dwgalpha), gT = sum_b T_b grad N_b, u_q and dT_q interpolated
 *               as the assembly does: the contribution of tet e to node a is
 *                 r_a(e) = sum_q W [ dc_q N_a(q) (dT_q + u_q . gT) + dk_q (grad N_a . gT) ],
 *               with the sign of the base terms btc shl + kKAPPA grad . shg of the element residual, so that base + correction
 *               is the Galerkin T row with c_q and k_q.  r[a] = the sum over a's tets in ascending tet id, from +0.0; a tet
 *               whose eight dk_q, dc_q are all exactly 0 adds +0.0.  One launch over the nodes' sorted tet lists
 *               (csrc/k_thermal.hip), no float atomics, bitwise reproducible, the same under every assembly schedule.  Every F
 *               assembly adds r[a] to R[5N + a] after the phase-change rows and before the T rows are saved for the scalar
 *               transport; only when that transport advances T (otherwise the rows are zeroed anyway and nothing is launched).
 *               The capacity correction is the consistent one on purpose: the base term is the consistent mass with
 *               kRHO kCP, and a lumped correction would leave c0 M_c + (c - c0) M_l, which is indefinite for c < 0.8 c0
 *               (the smallest eigenvalue of M_l^-1 M_c on linear tets is 1/5) -- the gas.  With the consistent form the total
 *               is sum_q W c_q N_a N_b, positive definite whenever c_q > 0.
 *   Jacobian    DflAssembleScalarJacobian adds to every tet's entries of the T Jacobian, coefficients frozen at the alpha states,
 *                 jm_ab(e) = sum_q W [ dc_q N_a(q) (f1 N_b(q) + f2 u_q . grad N_b) + f2 dk_q grad N_a . grad N_b ],
 *               f1 = kALPHAM, f2 = dt kALPHAF kGAMMA: the tet's entry is base + jm (the base rounded first), summed over the
 *               row's tets in ascending tet id as without the section, in the same single launch, before the phase-change
 *               diagonal and the Dirichlet unit rows.  This is Picard in fl, as H is in the phase-change section; with
 *               k_liquid == k_solid it is the exact derivative.  The phi Jacobian is untouched.
 *   inspection  Kn[a] = sum W N_a(q) k_q and Cn[a] = sum W N_a(q) c_q (totals, not differences): divided by the nodal volume
 *               they are the node's mean conductivity and capacity.
 * Limits: one GPU (SolveFlowSystem and DflTimeStep with a communicator print why and return -1); the SUPG part of the T row
 * keeps kRHO kCP and kKAPPA (tau3 and its test-function factor): it stays a positive streamline-diffusion term, mis-scaled
 * by c_q / (kRHO kCP); no density change in the momentum rows from this section (density, viscosity and weight there are the
 * section "fluid material" below); k does not depend on T other than through fl.  A 1000 : 1
 * conductivity jump costs the Jacobi-preconditioned T solve iterations: PC_AMGX (DflScalarTransport.pc) is the remedy. */
typedef struct DflThermalMaterial {
    f64 k_gas, k_solid, k_liquid;     /* W/(m K), each > 0 */
    f64 c_gas, c_metal;               /* rho cp, J/(m^3 K), each > 0 */
    f64 T_solidus, T_liquidus;        /* read only when k_liquid != k_solid; then T_liquidus > T_solidus */
    b32 use_phi; f64 level; index_type side; f64 eps;   /* as DflPhaseChange; use_phi 0: metal everywhere */
} DflThermalMaterial;
/* host only: 0 when DflMeshSetThermalMaterial accepts the configuration, else why not in `why`.  Refused: any non-finite
 * value, any of the five coefficients <= 0, k_liquid != k_solid with T_liquidus <= T_solidus, use_phi with side not +-1 or
 * eps <= 0 */
int  DflThermalMaterialCheck(const DflThermalMaterial* cfg, char* why, size_t why_len);
/* the configuration is copied; NULL: off.  A refused configuration is reported on stderr and leaves the mesh unchanged.  Has
 * the mesh build the sorted tet lists of the nodes if nothing did before (shared, freed with the mesh) and synchronises: the
 * later calls allocate nothing and do not wait for the device */
void DflMeshSetThermalMaterial(Mesh3D* mesh, const DflThermalMaterial* cfg);
b32  DflMeshThermalMaterialEnabled(const Mesh3D* mesh);
/* w, dw: device 6N, taken as the alpha states; r, Kn, Cn [N] on the device, any of them NULL, every other one overwritten in
 * full.  Without a configuration: a line on stderr, nothing written */
void DflMeshThermalRows(Mesh3D* mesh, const f64* w, const f64* dw, f64* r, f64* Kn, f64* Cn);

/* ---- fluid material: density, viscosity and buoyancy of the (u,p) rows follow phi (build-defined; opt-in) ----------------
 * The reference's momentum and continuity rows belong to one fluid without weight: kRHO = 1000, kMU = 10/3 and a zero body
 * force everywhere, so the shielding gas is as heavy and as viscous as the metal and a hot pool has no natural convection.
 * A mesh that never calls DflMeshSetFluidMaterial with a configuration, or clears it with NULL, computes bit for bit what it
 * computes without this section, through the same launches.  One GPU only.  With a configuration the (u,p) rows and the
 * (u,p) Jacobian become those with rho_q, mu_q and the body force f_q below at every quadrature point, by a correction that
 * is added to what the untouched assembly kernels give.
 *   per tet     grad N_a, det, g, |g|, d_a, d_q, m_q = Hs(side d_q / eps) and the rule for a tet with !(|g| > 0) exactly as
 *               the phase-change and thermal-material sections form them (the same closed form, without fused
 *               multiply-add); without use_phi m_q = 1.  T_q = sum_a N_a(q) T_a.
 *                 rho_q  = rho_gas + m_q (rho_metal - rho_gas)
 *                 mu_q   = mu_gas  + m_q (mu_metal  - mu_gas)
 *                 f_q[i] = gravity[i] (1 - m_q beta (T_q - T_ref))          a NaN T_q gives the factor 1
 *               Only the weight sees beta; the inertia keeps rho_q (Boussinesq).  T is read only when beta != 0.
 *               W = |det| / 24 and the four quadrature points of the assembly.
 *   rows        E_a[0..3](rho[4], mu[4], f[4][3]) is the contribution of a tet to the three momentum rows and the continuity
 *               row of its node a: the terms of the element residual of the assembly (rLi, tmp0, tmp1, tau[0], tau[1] and the
 *               two weak forms) at the alpha states (u from wgalpha; du and the pressure from dwgalpha, as the assembly takes
 *               them), with rho_q for kRHO, mu_q for kMU and f_q for the body force at quadrature point q wherever they occur.
 *               Stabilisation: nu_q = mu_q / rho_q, y_q = t1_q + 3 nu_q^2 sum G_ij^2, tau0_q = (1 / sqrt(4 / dt^2 + y_q)) / rho_q,
 *               tau1_q = sqrt(y_q) / tr G, where t1_q is the velocity term of the kernel that the correction belongs to: u.G.u
 *               as the residual forms it in the rows, |J^-1 u_q|^2 = sum_{b=1..3} (u_q . grad N_b)^2 as the element Jacobian
 *               forms it in the blocks.  The correction of a tet is
 *                 r_a(e) = E_a(rho_q, mu_q, f_q) - E_a(kRHO, kMU, 0),
 *               both evaluations through the same function without fused multiply-add, so a tet whose coefficients are the
 *               built-in ones and whose f_q are zero gives exactly +0.0.  r[3a + d] and r[3N + a] are the sums over a's tets in
 *               ascending tet id, from +0.0.  One launch over the nodes' sorted tet lists (csrc/k_fluid.hip), no float atomics,
 *               bitwise reproducible, the same under every assembly schedule.  Every F assembly adds r to R[0 .. 4N) after the
 *               thermal-material rows and before the Dirichlet rows.
 *   Jacobian    B_ab(rho[4], mu[4]) is the 4 x 4 block of the element Jacobian with the coefficients inside the quadrature
 *               sums (s_a = N_a(q), c_a = u_q . grad N_a, eK = grad N_a . grad N_b, f1 = kALPHAM, f2 = dt kALPHAF kGAMMA,
 *               w = W):
 *                 diag = w sum_q [ f1 rho_q s_a s_b + f1 rho_q^2 tau0_q c_a s_b + f2 rho_q s_a c_b + f2 rho_q^2 tau0_q c_a c_b
 *                                  + f2 mu_q eK ]
 *                 B[i][j] = cK gradN_a[j] gradN_b[i] + cT gradN_a[i] gradN_b[j] (+ diag for i == j),
 *                           cK = f2 w sum_q mu_q, cT = f2 w sum_q rho_q tau1_q
 *                 B[i][3] = cP1 gradN_b[i] - cP0 gradN_a[i],  cP0 = w sum_q s_b, cP1 = w sum_q rho_q tau0_q c_a
 *                 B[3][i] = cU0 gradN_a[i] + cU1 gradN_b[i],  cU0 = w sum_q rho_q tau0_q (f1 s_b + f2 c_b), cU1 = w f2 sum_q s_a
 *                 B[3][3] = w eK sum_q tau0_q
 *               The body force does not enter (the base Jacobian does not differentiate rLi either), and the coefficients are
 *               frozen at the alpha states: Picard in phi and T, as in the two sections before.
 *                 jm_ab(e) = B_ab(rho_q, mu_q) - B_ab(kRHO, kMU).
 *               For every nonzero (a, b) of the nodal pattern S = the sum of jm_ab(e) over a's tets that hold b, in ascending
 *               tet id from +0.0, and val[16 nz + e] = fl(val[16 nz + e] + S[e]): every J assembly, after the tet and face
 *               terms AND after the phase-change diagonal, before the Dirichlet unit rows.  J needs the block layout of the
 *               (u,p) matrix (with MatrixFSUseReferenceLayout: an ASSERT with a message, as for the phase-change drag).
 *   inspection  Rn[a] = sum W N_a(q) rho_q and Mn[a] = sum W N_a(q) mu_q (totals, not differences): divided by the nodal volume
 *               they are the node's mean density and viscosity.
 * Limits: one GPU (SolveFlowSystem and DflTimeStep with a communicator print why and return -1); the weak-boundary-condition
 * face terms keep kRHO and kMU; the SUPG part of the T row and the DEM drag keep their own constants; the mixing is arithmetic
 * in m_q; no volume change on melting (the continuity row stays div u). */
typedef struct DflFluidMaterial {
    f64 rho_gas, rho_metal;   /* kg/m^3, each > 0 */
    f64 mu_gas,  mu_metal;    /* Pa s,   each > 0 */
    f64 gravity[3];           /* m/s^2; all zero: no weight */
    f64 beta, T_ref;          /* thermal expansion of the metal, 1/K (Boussinesq); beta = 0: none */
    b32 use_phi; f64 level; index_type side; f64 eps;   /* as DflPhaseChange; use_phi 0: metal everywhere */
} DflFluidMaterial;
/* host only: 0 when DflMeshSetFluidMaterial accepts the configuration, else why not in `why`.  Refused: any non-finite
 * value, a density or viscosity <= 0, use_phi with side not +-1 or eps <= 0 */
int  DflFluidMaterialCheck(const DflFluidMaterial* cfg, char* why, size_t why_len);
/* the configuration is copied; NULL: off.  A refused configuration is reported on stderr and leaves the mesh unchanged.  Has
 * the mesh build the sorted tet lists of the nodes if nothing did before (shared, freed with the mesh) and synchronises: the
 * later calls allocate nothing and do not wait for the device */
void DflMeshSetFluidMaterial(Mesh3D* mesh, const DflFluidMaterial* cfg);
b32  DflMeshFluidMaterialEnabled(const Mesh3D* mesh);
/* w, dw: device 6N, taken as the alpha states; r [4N], Rn, Mn [N] on the device, any of them NULL, every other one
 * overwritten in full.  Without a configuration: a line on stderr, nothing written */
void DflMeshFluidRows(Mesh3D* mesh, const f64* w, const f64* dw, f64* r, f64* Rn, f64* Mn);

/* ---- level-set redistancing: the exact band distance to the surface phi = level (build-defined; opt-in) -----------------
 * The reference advects phi and never restores |grad phi| = 1.  A mesh that never calls DflMeshSetRedistance with a
 * configuration, or clears it with NULL, computes bit for bit what it computes without this section, through the same
 * launches.  One GPU only.  With a configuration DflMeshRedistance replaces phi, inside a band around the surface
 * phi = level, by the signed distance to the piecewise-linear surface itself: the minimum over its triangles of the
 * point-triangle distance.  A minimum needs no order, no iteration and no causality, so the result is bitwise reproducible.
 * No operation below is fused (no multiply-add), and every dot product is associated (x0 y0 + x1 y1) + x2 y2.
 *   inputs      w (device, 6N), phi_a = w[4N + a], f_a = phi_a - level.  Node a is positive iff f_a > 0: a NaN is not.
 *   facets      the tets in ascending tet id, nodes n_k = ien[4e + k], k the local index.  A tet with 0 or 4 positive nodes
 *               has no facet.  The crossing point of edge (i positive, j not) is P_ij = x_i + t (x_j - x_i),
 *               t = f_i / (f_i - f_j), per component.
 *                 1 positive node i:   the triangle (P_ij), j over the three others in local order;
 *                 3 positive nodes:    the triangle (P_ij), i over the positives in local order, j the fourth;
 *                 2 positive a < b, the others c < d: the quad P_ac, P_ad, P_bd, P_bc (planar: phi is linear in the tet) as
 *                                      the triangles (0, 1, 2) and (0, 2, 3).
 *               The facet list is [nf][9] f64 (A, B, C), ascending tet id, a quad's first triangle first.
 *   distance    of a point p to a facet (A, B, C), squared: the minimum of seven candidates, started from +inf and replaced
 *               only where candidate < minimum, so a NaN never wins:
 *                 the vertices   |p - V|^2, V = A, B, C;
 *                 the segments   (U, V) = (A, B), (B, C), (C, A): e = V - U, only where e . e > 0:
 *                                t = ((p - U) . e) / (e . e), t < 0 -> 0, t > 1 -> 1, |p - (U + t e)|^2;
 *                 the plane      n = (B - A) x (C - A), only where n . n > 0 and the projection is inside:
 *                                b1 = ((p - A) x (C - A)) . n >= 0, b2 = ((B - A) x (p - A)) . n >= 0, b1 + b2 <= n . n:
 *                                ((p - A) . n)^2 / (n . n).
 *               a x b = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0).  Degenerate facets (nodes exactly on the surface)
 *               need no special case: their vertices and edges still count.
 *   result      d_a = sqrt(min over all facets), +inf without a facet; phi_a <- level + s_a min(d_a, band), s_a = +1 for a
 *               positive node, else -1.  A node whose phi is NaN keeps its NaN; a node of a boundary group in hold_groups
 *               (bit g = group g, g < 31) keeps its value; the rate dphi and every other slot of w are not touched.
 *   search      a uniform grid over the bounding box of the nodes (made by the Set call and again by the first call after
 *               DflMeshGeometryChanged), cell edge band x DFL_REDISTANCE_CELL (read by the Set call, default 1, a value below
 *               1 is refused), enlarged by steps of 1.25 while the grid would have more than 2^24 cells.  Every facet is
 *               entered into every cell the bounding box of its finite vertices overlaps (a NaN vertex never wins), so the closest point of a node with d_a < band lies in
 *               one of the 27 cells around the node's own and its facet is listed there; whatever the search finds beyond
 *               band is clamped to band.  The result therefore does not depend on the cell size.
 *   statistics  of the last call: facets; band_nodes = the nodes with d_a < band (held and NaN nodes included); max_change =
 *               max over them of |new phi_a - old phi_a| (0 for a node that kept its value); grad_dev_before / _after =
 *               max of ||g| - 1| over the cut tets (those with a facet) of the old / new field, g and |g| as the free-surface
 *               section forms them, a NaN passed over, 0 without a cut tet; volume_before / _after = the volume of
 *               {phi > level}: the sum over the tets, in a fixed two-stage order, of
 *                 0 positive nodes: 0;   4: |det| / 6, det = e_1 . (e_2 x e_3) of the free-surface section;
 *                 1 (i):  |det4(x_i, P_ij1, P_ij2, P_ij3)| / 6, det4(q0, q1, q2, q3) = (q1 - q0) . ((q2 - q0) x (q3 - q0));
 *                 3 (j not positive):  |det| / 6 - |det4(x_j, P_i1j, P_i2j, P_i3j)| / 6;
 *                 2:  the wedge u = (x_a, P_ac, P_ad), v = (x_b, P_bc, P_bd) as the tets (u0 u1 u2 v0), (u1 u2 v0 v1),
 *                     (u2 v0 v1 v2): ((|det4| + |det4|) + |det4|) / 6;
 *               a tet whose value is NaN (a NaN phi at a node of a cut tet) adds 0.
 *   time step   with every > 0, DflTimeStep redistances phi of wgold on every every-th call since the Set call, before the
 *               surface load and anything else is evaluated.  With a communicator it prints why and returns -1.
 * Limits: the surface ends at the mesh boundary, so the distance is to the part of the surface inside the mesh.  Beyond band
 * the field is flat at level +- band; there |g| = 0, which the free-surface and phase-change sections treat as "contributes
 * nothing" / "mean sign", so band >= eps + 2 h (h the tet size) is the caller's condition.  One GPU only.  The call
 * itself does not correct the volume: the zero set of the new interpolant moves by O(h^2), volume_before / volume_after say
 * by how much, and the "level-set volume correction" section below restores it.  Fewer than 2^31 facets and cell entries. */
typedef struct DflRedistance {
    f64 level, band;          /* the surface phi = level; half-width of the band (length), > 0 */
    index_type hold_groups;   /* bit g: the nodes of boundary group g keep their phi */
    index_type every;         /* > 0: DflTimeStep redistances wgold on every every-th call; 0: only DflMeshRedistance does */
} DflRedistance;
typedef struct DflRedistanceStats {
    int64_t facets, band_nodes;
    f64 max_change, grad_dev_before, grad_dev_after, volume_before, volume_after;
} DflRedistanceStats;
/* host only: 0 when DflMeshSetRedistance accepts the configuration, else why not in `why`: level or band not finite,
 * band <= 0, every < 0 */
int  DflRedistanceCheck(const DflRedistance* cfg, char* why, size_t why_len);
/* the configuration is copied; NULL: off, frees everything of its own.  A refused configuration (or DFL_REDISTANCE_CELL) is
 * reported on stderr and leaves the mesh as it was.  Builds the grid, the hold mask and every buffer but the two lists
 * below (synchronises), and restarts the count of time steps */
void DflMeshSetRedistance(Mesh3D* mesh, const DflRedistance* cfg);
b32  DflMeshRedistanceEnabled(const Mesh3D* mesh);
/* in place on w[4N:5N), w on the device; returns the number of facets, -1 when not set.  Every call waits for the device
 * once, to read the facet and cell-entry totals back (the first is its return value), and grows the facet and entry lists
 * when a total exceeds their capacity; it allocates nothing otherwise */
index_type DflMeshRedistance(Mesh3D* mesh, f64* w);
/* the facet list of the last call, device [nf][9] (NULL with nf <= 0), valid until the next call or Set; returns nf, -1
 * when not set or never called */
index_type DflMeshRedistanceFacets(const Mesh3D* mesh, const f64** facets);
/* the statistics of the last call (synchronises, reads 48 bytes back); zeros when not set (with a line on stderr) or never
 * called */
void DflMeshRedistanceStats(Mesh3D* mesh, DflRedistanceStats* out);
/* the volume of {phi > level} at the state w (device 6N) as the statistics form it; needs no configuration.  Allocates and
 * frees its own scratch and synchronises */
f64  DflMeshLevelSetVolume(Mesh3D* mesh, const f64* w, f64 level);

/* ---- level-set volume correction: a global shift of phi that restores the metal volume (build-defined; opt-in) -----------
 * Level-set advection does not conserve volume and every redistancing moves the zero set by O(h^2); the reference does
 * nothing about either.  A mesh that never calls DflMeshSetVolumeCorrection with a configuration, or clears it with NULL,
 * computes bit for bit what it computes without this section, through the same launches.  One GPU only.
 *   volume      V(c) = the volume of {phi > c}, summed over the tets exactly as volume_before / _after of the redistancing
 *               section form it (a NaN tet adds 0), in a fixed order.  V is continuous, non-increasing in c and piecewise
 *               cubic.  V_mesh = the sum of |det| / 6 over all tets.
 *   correction  finds c* in [level - max_shift, level + max_shift] with |V(c*) - target| <= tol V_mesh and writes
 *               phi_a <- phi_a + delta, delta = level - c*, for every node, as one rounded addition.  A NaN stays a NaN (it is
 *               not written); no other slot of w is touched.
 *   status      0 corrected: a c* within the tolerance was found, the shift is applied;
 *               1 already within tolerance: |V(level) - target| <= tol V_mesh, tested first: delta = 0, no node written, no
 *                 search pass.  Also the answer of the call that records an unset target (below);
 *               2 not bracketed: target > V(level - max_shift) or target < V(level + max_shift) (no surface, or a drift
 *                 larger than the caller allows): nothing written;
 *               3 pass limit reached before the tolerance: the evaluated c with the smallest |V(c) - target| is applied.
 *   search      lo = level - max_shift, hi = level + max_shift.  One pass over all tets: a tet whose four phi are > hi is
 *               inside for every candidate and its |det| / 6 goes into V_in; a tet with no phi > lo adds nothing; every
 *               other tet is a band tet, and the ids of the band tets are compacted in ascending order into a list.  The
 *               same pass gives V at level, lo and hi, and V_mesh.  The bracket [a, b], V(a) >= target >= V(b), starts as
 *               [lo, level] or [level, hi].  A K-section pass (K = 15) evaluates V = V_in + V_band at K candidates in one read
 *               of the band list: the K - 1 points a + k ((b - a) / K) and the trial c, the linear interpolant of V between
 *               a and b at the target (the midpoint where V(a) = V(b)), inserted in ascending order.  The host reads the K
 *               sums back, stops when the best evaluated c meets the tolerance, and else keeps the first sub-interval
 *               whose right end has V <= target.  The pass limit is 12; DFL_VOLUME_PASSES (an integer >= 1, read by the Set
 *               call; anything else is refused) replaces it.
 *   target      the volume of {phi > level} to restore.  NaN in the configuration: the first correction call (direct or
 *               from DflTimeStep) records V(level) of the state it sees and returns 1 without writing anything.
 *               SetTarget / AddTarget change it between calls.
 *   time step   with every > 0, DflTimeStep corrects phi of wgold on every every-th call since the Set call, after the
 *               redistancing of that call, if any, and before the surface load and anything else is evaluated.  With a
 *               communicator it prints why and returns -1.  With track_capture, a step that took a pending two-way capture
 *               source (ParticleContextSetCapture) adds side dt sum_a q_vol[a], the volume the captured particles brought,
 *               to the target after its Newton solve (summed on the device in a fixed two-stage order; reads 8 bytes back).
 *   statistics  of the last call: status, passes, band_tets, shift = delta (0 unless the status is 0 or 3), target,
 *               volume_before = V(level) as the call found it, volume_after = V(c*) (= volume_before unless shifted: the
 *               volume of {phi > level} of the new field up to the rounding of the addition), volume_mesh.
 * Limits: one shift for the whole mesh, so the volume is restored but not where it was lost; the surface moves by delta / |grad
 * phi| everywhere, and after a redistancing |grad phi| = 1 inside its band.  side only orients what track_capture adds: the
 * target is the volume of {phi > level} either way, so with side = -1 the metal volume is V_mesh - target.  One GPU only. */
typedef struct DflVolumeCorrection {
    f64 level;            /* the surface phi = level */
    index_type side;      /* +1: metal where phi > level, -1: metal where phi < level (as DflParticleCapture.side) */
    f64 max_shift;        /* > 0: the largest |delta| the call may apply */
    f64 tol;              /* >= 0, relative to the mesh volume */
    f64 target;           /* volume of {phi > level} to restore; NaN: taken from the state the first call sees */
    index_type every;     /* > 0: DflTimeStep corrects wgold on every every-th call; 0: only DflMeshVolumeCorrect does */
    b32 track_capture;    /* DflTimeStep adds what a two-way capture deposited to the target */
} DflVolumeCorrection;
typedef struct DflVolumeCorrectionStats {
    index_type status, passes;
    int64_t band_tets;
    f64 shift, target, volume_before, volume_after, volume_mesh;
} DflVolumeCorrectionStats;
/* host only: 0 when DflMeshSetVolumeCorrection accepts the configuration, else why not in `why`: level, max_shift or tol not
 * finite, max_shift <= 0, tol < 0, side not +-1, every < 0, target infinite */
int  DflVolumeCorrectionCheck(const DflVolumeCorrection* cfg, char* why, size_t why_len);
/* the configuration is copied; NULL: off, frees everything of its own.  A refused configuration (or DFL_VOLUME_PASSES) is
 * reported on stderr and leaves the mesh as it was.  Allocates every buffer but the band list (synchronises), takes the
 * target from the configuration and restarts the count of time steps */
void DflMeshSetVolumeCorrection(Mesh3D* mesh, const DflVolumeCorrection* cfg);
b32  DflMeshVolumeCorrectionEnabled(const Mesh3D* mesh);
/* in place on w[4N:5N), w on the device; returns the status, -1 when not set.  Waits for the device once after the pass over
 * all tets and once per K-section pass.  The band list grows when the band-tet count exceeds its capacity; the call
 * allocates nothing otherwise.  The geometry is read on every call: DflMeshGeometryChanged needs no rebuild here */
index_type DflMeshVolumeCorrect(Mesh3D* mesh, f64* w);
/* the statistics of the last call; zeros, status -1, when not set (with a line on stderr) or never called */
void DflMeshVolumeCorrectionStats(Mesh3D* mesh, DflVolumeCorrectionStats* out);
/* the target: NaN when not set, or not recorded yet */
f64  DflMeshVolumeCorrectionTarget(const Mesh3D* mesh);
/* NaN: the next call records it again; an infinite volume, a dV that is not finite, or a mesh without a configuration: a line
 * on stderr, nothing changed.  A dV added to a target not recorded yet is lost: the recording call sees the state with it */
void DflMeshVolumeCorrectionSetTarget(Mesh3D* mesh, f64 volume);
void DflMeshVolumeCorrectionAddTarget(Mesh3D* mesh, f64 dV); /* dV of {phi > level} */

/* ---- solidification record: gradient, cooling rate and front speed per node (build-defined; opt-in) ----------------------
 * The phase-change statistics are a snapshot of the pool; nothing there survives the step in which a node crosses the
 * freezing isotherm.  This section keeps, per node, how the node froze the last time: when, how fast it cooled and the thermal
 * gradient G at that moment (the front speed R = cooling rate / |G|; G / R and G R say what grains to expect), and besides
 * the peak temperature, the time spent liquid and the number of remelts.  It is passive: it reads the state and never writes
 * it, so a mesh computes bit for bit the same flow with it on, and a mesh that never calls DflMeshSetSolidification with a
 * configuration, or clears it with NULL, runs the launches it runs without this section.  One GPU only.
 *   record      per node a: T_prev (NaN until primed), T_peak (-inf), t_liquid (0), melts (0, index_type), t_solid (NaN: no
 *               record), cool (0), grad3[3a + d] (0); the metal flag of the node as its last update saw it; on the host the
 *               elapsed time t (0) and the number of updates.  DflMeshSetSolidification and DflMeshSolidificationReset set
 *               these initial values.
 *   priming     the first Update after Set or Reset sets T_prev = T and T_peak = fmax(T_peak, T) for every node, leaves t as
 *               it is, books no event (the event list is empty) and ignores dt, which must still be finite and positive.
 *   update      every later one, with Tp = T_prev[a], Tn = w[5N + a], metal = !use_phi || side (w[4N + a] - level) > 0,
 *               above_p = Tp >= T_front, above_n = Tn >= T_front:
 *                 a NaN Tn leaves every entry of the node as it was, T_prev included;
 *                 T_peak[a] = fmax(T_peak[a], Tn), metal or not;
 *                 where metal: above at both ends adds dt to t_liquid; a freezing crossing (above_p && !above_n) adds
 *                 theta dt, theta = (Tp - T_front) / (Tp - Tn); a melting crossing (!above_p && above_n) adds
 *                 (1 - (T_front - Tp) / (Tn - Tp)) dt.  Every product is rounded before the add (no fused multiply-add);
 *                 freeze event (metal && above_p && !above_n): t_solid = t + theta dt, cool = (Tp - Tn) / dt, grad3 = the
 *                 recovered gradient below at w; the node enters the event list;
 *                 melt event (metal && !above_p && above_n): melts += 1, t_solid = NaN, cool = 0, grad3 = 0: a remelted
 *                 node has no record until it freezes again;
 *                 T_prev[a] = Tn.
 *               After the launches t += dt on the host.  A node primed with a NaN has a NaN T_prev: it compares as below
 *               the isotherm, and a melt event from it makes t_liquid NaN.
 *   gradient    of node a, over the tets e of its sorted list (ascending tet id): det and the cross products of the edge
 *               vectors in the closed form the free-surface and phase-change sections use (without fused multiply-add),
 *               gN_1 = c23 / det, gN_2 = c31 / det, gN_3 = c12 / det, gN_0 = -((gN_1 + gN_2) + gN_3), each component
 *               divided on its own; g_e[d] = ((T_0 gN_0[d] + T_1 gN_1[d]) + T_2 gN_2[d]) + T_3 gN_3[d].  A tet adds nothing
 *               if !(|det| > 0), or with use_phi if side (mean phi - level) > 0 is false, mean = ((phi_0 + phi_1) +
 *               (phi_2 + phi_3)) * 0.25.  S_d = sum |det_e| g_e[d] and V = sum |det_e|, each in ascending tet id from +0.0;
 *               grad3[3a + d] = V > 0 ? S_d / V : 0: the volume-weighted mean of the tet gradients, exact for a linear T.
 *   front speed not stored: R = |G| > 0 ? cool / |G| : 0, |G| = sqrt((g0 g0 + g1 g1) + g2 g2).
 *   statistics  time = t, updates = accepted Update calls since Set or Reset (the priming one included), frozen = nodes with
 *               a record (t_solid not NaN), liquid = nodes with the metal flag and T_prev >= T_front, the event counts of the
 *               last update, minimum and maximum of |G|, cool and R over the records (a NaN is passed over), T_peak_max over
 *               the nodes with the metal flag (a NaN is passed over); in a fixed two-stage order.  An empty set gives count 0,
 *               minimum +inf, maximum -inf.
 *   time step   with in_time_step, DflTimeStep calls DflMeshSolidificationUpdate(mesh, wgold, DflMeshTimeStep(mesh)) once the step has
 *               written wgold.  The first DflTimeStep after Set or Reset first primes the record at its incoming wgold, so
 *               that its own step is already booked.  With a communicator DflTimeStep prints why and returns -1.
 * Every sum has a fixed order and no float atomic is used: two runs agree bit for bit, under every assembly schedule.  An
 * Update is five launches and one 4-byte copy to pinned host memory; it allocates nothing and does not wait for the device.
 * The geometry is read on every call: DflMeshGeometryChanged needs nothing here. */
typedef struct DflSolidification {
    f64 T_front;                                /* the freezing isotherm (typically T_solidus or T_liquidus) */
    b32 use_phi; f64 level; index_type side;    /* metal where side (phi - level) > 0; use_phi 0: metal everywhere */
    b32 in_time_step;                           /* DflTimeStep updates the record itself */
} DflSolidification;
typedef struct DflSolidificationStats {
    f64 time;                                   /* elapsed time t */
    int64_t updates;                            /* accepted Update calls since Set or Reset */
    int64_t frozen, liquid;                     /* nodes with a record; metal nodes with T_prev >= T_front */
    int64_t freeze_events_last, melt_events_last;
    f64 G_min, G_max, cool_min, cool_max, R_min, R_max; /* over the records */
    f64 T_peak_max;                             /* over the metal nodes */
} DflSolidificationStats;
/* host only: 0 when DflMeshSetSolidification accepts the configuration, else why not in `why`: T_front or level not finite,
 * use_phi with side not +-1 */
int  DflSolidificationCheck(const DflSolidification* cfg, char* why, size_t why_len);
/* the configuration is copied; NULL: off, frees everything of its own (the sorted tet lists of the nodes are the mesh's and
 * stay).  A refused configuration is reported on stderr and leaves the mesh and the record as they were.  Has the mesh build
 * the sorted tet lists if nothing did before, builds every buffer and sets the record to its initial values (synchronises) */
void DflMeshSetSolidification(Mesh3D* mesh, const DflSolidification* cfg);
b32  DflMeshSolidificationEnabled(const Mesh3D* mesh);
/* w: device 6N state at the END of a step of length dt.  Without a configuration, or with a dt that is not finite or not
 * positive: a line on stderr, nothing changed */
void DflMeshSolidificationUpdate(Mesh3D* mesh, const f64* w, f64 dt);
/* records to their initial values, time 0, unprimed */
void DflMeshSolidificationReset(Mesh3D* mesh);
/* borrowed device arrays, valid until the feature is cleared or the mesh destroyed: t_solid, cool, T_peak, t_liquid [N],
 * grad3 [3N], melts [N]; any out pointer NULL.  Without a configuration every pointer asked for comes back NULL */
void DflMeshSolidificationFields(const Mesh3D* mesh, const f64** t_solid, const f64** grad3, const f64** cool,
                                 const f64** T_peak, const f64** t_liquid, const index_type** melts);
/* device list of the nodes frozen by the last update, ascending; returns its length (synchronises); 0 and NULL when not set */
index_type DflMeshSolidificationEvents(const Mesh3D* mesh, const index_type** nodes);
/* synchronises, reads 88 bytes back; without a configuration: a line on stderr, the empty-set values */
void DflMeshSolidificationStats(Mesh3D* mesh, DflSolidificationStats* out);

/* ---- track cross-sections: bead height, width, depth and dilution per station (build-defined; opt-in) -------------------------
 * What a DED experiment measures on a cut and polished sample: the bead above the original substrate surface, the fused zone
 * below it, their areas and the ratio of the two, the dilution.  The phase-change statistics are a box around what is molten
 * now and the solidification statistics are extrema over nodes; neither is geometry.  This section cuts the mesh on the device
 * by up to 64 parallel planes.  It is passive: it reads the state and never writes it, so a mesh computes bit for bit the same
 * flow with it on, and a mesh that never calls DflMeshSetTrackSections with a configuration, or clears it with NULL, runs the
 * launches it runs without this section.  One GPU only.
 *   frame       n = normal / sqrt((n0 n0 + n1 n1) + n2 n2), the scan direction; u = up - (up . n) n, divided by its own length
 *               formed the same way, the build direction; t = u x n (t0 = u1 n2 - u2 n1, cyclic).  Every dot product is
 *               (a0 b0 + a1 b1) + a2 b2 and every product is rounded before it is added (no fused multiply-add), as in the
 *               laser section.  Station k is the plane (x - origin) . n = c_k, c = station, strictly ascending.
 *   nodes       with d = x_a - origin formed first: s_a = d . n, y_a = d . t, h_a = d . u; f_a = phi_a - level, negated for
 *               side = -1: metal where f > 0; g_a = Tpk_a - T_fuse: fused where g >= 0.  h = 0 is the original substrate
 *               surface: origin lies on it.
 *   pairs       tet e and station k form a pair when the mask of sigma_a = s_a - c_k > 0 over the tet's four nodes is neither
 *               0 nor 15 (a NaN is not positive) and at least one f_a > 0.  So a station that lies exactly on a plane of nodes
 *               sees the tets on its positive side, once, and a station on the far boundary of the mesh sees nothing.  The
 *               pair list is ordered by station, then by tet id.
 *   cut         of one pair: the facets of the surface sigma = 0 in the tet as the redistancing section makes them (one
 *               positive node i: P_ij, j over the three others in local order; three: P_ij, i over the positives in local
 *               order; two, a < b, the others c < d: the quad P_ac, P_ad, P_bd, P_bc as (0, 1, 2) and (0, 2, 3)).  Vertex P_ij
 *               has tt = sigma_i / (sigma_i - sigma_j) and carries q_i + tt (q_j - q_i) for each q of (y, h, f, g); (y, h) are
 *               its coordinates in the station's plane.
 *   clip        Sutherland-Hodgman on a polygon of carried vertices against inside(q): walking the edges U -> V in order (the
 *               last V is vertex 0), U goes out when it is inside, then, when exactly one of U, V is inside, the crossing
 *               A + tau (B - A) from the inside vertex A towards the outside B, tau = q_A / (q_A - q_B), for all four
 *               quantities.  metal = the triangle clipped by f > 0 (at most 4 vertices); clad = metal clipped by h > 0 (at
 *               most 5); fused = metal clipped by !(h > 0) (5) and then by g >= 0 (6).  More vertices than that cannot come
 *               out in exact arithmetic; where rounding makes one, it is dropped.
 *   polygon     with at least 3 vertices: its area = the sum from +0.0, in fan order, of 0.5 |(y_k - y_0)(h_k+1 - h_0) -
 *               (y_k+1 - y_0)(h_k - h_0)|, k = 1 .. n - 2, counted as 0 when it is a NaN; and the minima and maxima of its
 *               vertices' y and h, where a NaN never wins a comparison.
 *   result      per station: area_clad, area_fused = the sums of the polygon areas, area_scale = the sum of the uncut facets'
 *               areas (the same fan); a pair adds its facets in their order from the pair's partial sum, and the pairs are
 *               summed in a fixed tree over chunks of 256 consecutive pairs of the list (the xor tree inside every wave of
 *               64, then waves 1, 2, 3 into wave 0), the chunks then by one workgroup (thread t takes chunks t, t + 256, ...;
 *               then the same tree).  height = max h over the clad vertices, depth = max of -h over the fused vertices,
 *               y_lo / y_hi of both.  An empty set gives +inf for a minimum and -inf for a maximum; a zero extent is +0.0.
 *               pairs = the station's pairs; dilution = area_fused / (area_clad + area_fused) where that sum is > 0, else 0,
 *               formed on the host.
 *   T_peak      a device [N] array; NULL: the T_peak of the solidification record when one is set on the mesh; without one
 *               every g is -inf and nothing is fused.
 *   time step   with every > 0, DflTimeStep evaluates on every every-th call since the Set call, at the wgold it has just
 *               written and after the solidification record's update of that step.  With a communicator it prints why and
 *               returns -1.
 * No atomics, on floats or on integers; the list order does not depend on arrival: two evaluations agree bit for bit.  Limits:
 * one normal for all stations; a NaN in a tet's numbers costs the station that tet's share of the areas, nothing else; the
 * pairs of all stations together must stay below 2^31. */
typedef struct DflTrackSections {
    f64 origin[3], normal[3], up[3];            /* a point of the substrate surface, the scan direction, the build direction */
    index_type num_station;                     /* 1 .. 64 */
    f64 station[64];                            /* the offsets c_k along n, strictly ascending */
    f64 level; index_type side;                 /* metal where side (phi - level) > 0 */
    f64 T_fuse;                                 /* fused where T_peak >= T_fuse */
    index_type every;                           /* > 0: DflTimeStep evaluates on every every-th call; 0: never */
} DflTrackSections;
typedef struct DflTrackSection {
    f64 area_clad, area_fused;                  /* metal above / fused metal at or below h = 0 */
    f64 area_scale;                             /* the station's whole cut through its pairs' tets: the parity scale */
    f64 height, depth;                          /* max h of the clad, max -h of the fused */
    f64 y_lo_clad, y_hi_clad, y_lo_fused, y_hi_fused;
    int64_t pairs;
    f64 dilution;
} DflTrackSection;
/* host only: 0 when DflMeshSetTrackSections accepts the configuration, else why not in `why`: an entry of origin, normal or up
 * that is not finite, a normal without length, an up parallel to the normal, num_station outside 1 .. 64, a station that is not
 * finite or does not ascend strictly, a level or T_fuse that is not finite, side not +-1, every < 0 */
int  DflTrackSectionsCheck(const DflTrackSections* cfg, char* why, size_t why_len);
/* the configuration is copied; NULL: off, frees everything of its own.  A refused configuration is reported on stderr and
 * leaves the mesh as it was.  Builds every buffer but the lists, forgets the last evaluation and restarts the count of time
 * steps (synchronises) */
void DflMeshSetTrackSections(Mesh3D* mesh, const DflTrackSections* cfg);
b32  DflMeshTrackSectionsEnabled(const Mesh3D* mesh);
index_type DflMeshTrackSectionsStations(const Mesh3D* mesh); /* num_station of the configuration; 0 when not set */
/* w: the device 6N state; T_peak: device [N] or NULL (above).  Waits for the device once, for the pair counts; the pair list
 * and the reduction records grow when a count exceeds their capacity and the call allocates nothing otherwise.  The geometry
 * is read on every call: DflMeshGeometryChanged needs nothing here.  Without a configuration: a line on stderr */
void DflMeshTrackSections(Mesh3D* mesh, const f64* w, const f64* T_peak);
/* synchronises and writes the num_station results of the last evaluation; before the first one every station has no pairs
 * and the empty-set values.  Without a configuration: a line on stderr, out untouched */
void DflMeshTrackSectionsResult(Mesh3D* mesh, DflTrackSection* out);

/* ---- porosity record: closed gas pores by connected components of phi (build-defined; opt-in) -----------------------------
 * Gas trapped in the metal: a bubble in the pool, a void frozen under the bead, a gap between a particle-fed bead and the
 * substrate.  Whether a gas pocket is closed is a question of connectivity, which no box, no single volume and no cutting plane
 * answers.  This section labels the connected components of the gas region on the device and lists the closed ones.  It is
 * passive: it reads the state and never writes it, so a mesh computes bit for bit the same flow with it on, and a mesh that
 * never calls DflMeshSetPorosity with a configuration, or clears it with NULL, runs the launches it runs without this section.
 * One GPU only.
 *   sign        f_a = phi_a - level, negated for side = -1.  A node whose phi is not finite is bad: neither metal nor gas, and
 *               counted.  Every other node is metal where f_a > 0 and gas otherwise (also where the difference of two finite
 *               numbers overflowed to -inf).  A tet with a bad node joins nothing and adds no volume; such tets are counted.
 *   graph       two gas nodes are joined when they share a tet that has no bad node.  For a piecewise-linear phi this is the
 *               connectivity of the gas region itself: inside a tet the gas part is convex and contains the tet's gas nodes,
 *               and across a face it contains that face's gas nodes.  A component is a connected set of gas nodes; its label is
 *               the smallest node id in it, which no order of evaluation changes.  Every tet with at least one gas node and no
 *               bad node belongs to exactly one component, that of its gas nodes.
 *   open        a component is open when it holds a node of a boundary face of a group in open_groups (bit g: group g, as in
 *               ParticleContextSetWallMesh and the laser's substrate_groups; the faces are those of bound_elem_offset /
 *               bound_f2e / bound_forn).  Every other component is a pore.  With open_groups = 0 every component is closed
 *               and the atmosphere itself is listed as a pore.
 *   pore        pores are listed by ascending label; row k is the pore of rank k.  label; nodes = its gas nodes; tets = its
 *               tets; volume = the sum over its tets in ascending tet id, from +0.0, of the tet's gas volume |det| / 6 - V+,
 *               V+ the volume of {f > 0} in the tet exactly as the redistancing section decomposes it (a NaN adds 0);
 *               volume_scale = the same sum of |det| / 6, the parity scale; lo, hi = the box of the pore's gas nodes and of
 *               the crossing points P_ij = x_i + t (x_j - x_i), t = f_i / (f_i - f_j), on every edge from a gas node i to a
 *               metal node j of its tets, formed as in the redistancing section without fused multiply-add; T_wall_min,
 *               T_wall_max = the extremes of T over the metal nodes of its tets.  A NaN never wins a comparison; an empty
 *               set gives +inf for a minimum and -inf for a maximum; a zero is +0.0.  "Frozen in" is T_wall_max < T_solidus:
 *               the caller's decision, not the library's.
 *   totals      components, pores, listed = min(pores, max_pores); bad_nodes, bad_tets; volume_metal = the sum of V+ over the
 *               tets without a bad node, volume_open and volume_pores = the gas volumes of the tets of open and of closed
 *               components (all pores, listed or not), each summed in a fixed tree over workgroups of 256 consecutive tets
 *               (the xor tree inside every wave of 64, then waves 1, 2, 3 into wave 0), the workgroups then by one workgroup
 *               (thread t takes workgroups t, t + 256, ...; then the same tree); porosity = volume_pores / (volume_metal +
 *               volume_pores) where that sum is > 0, else 0, formed on the host.
 *   time step   with every > 0, DflTimeStep evaluates on every every-th call since the Set call, at the wgold it has just
 *               written, after the solidification record's update and the track cross-sections of that step.  With a
 *               communicator it prints why and returns -1.
 * No atomics on floats: every sum has a fixed order.  Counts and extremes use integer atomics, whose result no order changes:
 * two evaluations of one state agree bit for bit, lists included.  The number of launches and the one wait of an evaluation do
 * not depend on the state.  Limits: node and tet counts below 2^31. */
typedef struct DflPorosity {
    f64 level; index_type side;                 /* metal where side (phi - level) > 0 */
    index_type open_groups;                     /* boundary groups that are the atmosphere, bit g: group g */
    index_type max_pores;                       /* 1 .. 65536 rows kept, lowest labels first */
    index_type every;                           /* > 0: DflTimeStep evaluates on every every-th call; 0: never */
} DflPorosity;
typedef struct DflPore {
    index_type label, nodes, tets;
    f64 volume, volume_scale, lo[3], hi[3], T_wall_min, T_wall_max;
} DflPore;
typedef struct DflPorosityStats {
    int64_t components, pores, listed, bad_nodes, bad_tets;
    f64 volume_metal, volume_open, volume_pores, porosity;
} DflPorosityStats;
/* host only: 0 when DflMeshSetPorosity accepts the configuration, else why not in `why`: a level that is not finite, side not
 * +-1, a negative open_groups, max_pores outside 1 .. 65536, every < 0 */
int  DflPorosityCheck(const DflPorosity* cfg, char* why, size_t why_len);
/* the configuration is copied; NULL: off, frees everything of its own.  A refused configuration is reported on stderr and
 * leaves the mesh as it was.  Builds every buffer whose size follows from the mesh, forgets the last evaluation and restarts
 * the count of time steps (synchronises) */
void DflMeshSetPorosity(Mesh3D* mesh, const DflPorosity* cfg);
b32  DflMeshPorosityEnabled(const Mesh3D* mesh);
/* w: the device 6N state.  Returns the number of pores; waits for the device once, for the pore and closed-tet counts; the key
 * lists grow when the closed tets exceed their capacity and the call allocates nothing otherwise.  The geometry is read on
 * every call: DflMeshGeometryChanged needs nothing here.  Without a configuration: a line on stderr, returns -1 */
index_type DflMeshPorosity(Mesh3D* mesh, const f64* w);
/* synchronises; the totals of the last evaluation (all zero before the first).  Without a configuration: a line on stderr */
void DflMeshPorosityStats(Mesh3D* mesh, DflPorosityStats* out);
/* copies min(listed, cap) rows of the last evaluation, returns listed (synchronises); -1 without a configuration */
index_type DflMeshPorosityResult(Mesh3D* mesh, DflPore* out, index_type cap);
/* two device [N] arrays that stay valid until the next evaluation or Set call: label[a] = the label of a's component, -1 for
 * metal, -2 for bad; pore[a] = the rank of a's pore in the list, -1 for metal, bad or open (a rank at or above listed is a pore
 * that the list did not keep).  Returns N, 0 without a configuration (both NULL then) */
index_type DflMeshPorosityLabels(const Mesh3D* mesh, const index_type** label, const index_type** pore);

/* ---- surface mesh: welded, oriented triangles of phi = level with vertex fields (build-defined; opt-in) --------------------
 * The bead as a geometric object: the surface phi = level as one indexed triangle mesh with connectivity, a consistent
 * orientation and nodal fields interpolated to its vertices, to view, to compare with a scan, to measure roughness on, to colour
 * by temperature or cooling rate, or to hand on as the next layer's substrate (dedflow_amd/surface_io.py writes PLY and STL).
 * It is passive: it reads the state and never writes it, and a mesh that never calls DflMeshSetSurfaceMesh with a
 * configuration, or clears it with NULL, runs the launches it runs without this section.  One GPU only.
 *   sign        f_a = phi_a - level, negated for side = -1.  A node whose phi is not finite is bad and counted in bad_nodes; a
 *               tet with a bad node emits nothing and is counted in bad_tets.  Every other node is metal where f_a > 0 and gas
 *               otherwise: the porosity record's convention.  A tet is cut when it has no bad node and one, two or three
 *               metal nodes.  A cut tet whose determinant (tet_cross) is zero or not finite emits nothing and is counted in
 *               degenerate_tets; every other cut tet emits.
 *   vertices    one per cut mesh edge: an unordered node pair {i, j} of at least one emitting tet, i metal and j not.  The
 *               vertex is P = x_i + t (x_j - x_i), t = f_i / (f_i - f_j), formed exactly as the redistancing section forms its
 *               crossing points, metal node first and without fused multiply-add, so every tet around the edge would compute
 *               the same bits and every coordinate is bit for bit a coordinate of that section's unwelded facets.  Vertex ids
 *               are the ranks of the keys min(i, j) << 32 | max(i, j) in ascending order.  Welding is by edge, never by
 *               coordinates: where phi == level exactly at a gas node, several vertices coincide with that node and stay
 *               distinct.
 *   triangles   emitting tets in ascending tet id; inside a tet the facets of the redistancing section in its order (one
 *               metal node i: P_ij over the three others in local order; three: P_ij, i over the metal nodes in local order;
 *               two, a < b, the others c < d: the quad P_ac, P_ad, P_bd, P_bc as (0, 1, 2) and (0, 2, 3)).  Each triangle is
 *               an index triple into the vertex list; tri_tet[k] is the tet it came from.
 *   orientation the normal (B - A) x (C - A) points out of the metal: in exact arithmetic ((B - A) x (C - A)) . g < 0 with
 *               g = sum_a f_a grad N_a.  Where the facet as listed fails that, its second and third index are swapped.  The
 *               decision is combinatorial, a table over the 14 masks of metal nodes times the sign of the tet's determinant,
 *               and never looks at the rounded crossing points; a zero-area triangle gets the table's answer like any other.
 *               Inside one mask and one sign the answer cannot change, because the triangle does not degenerate while the
 *               signs of f are strict.
 *   per vertex  edge[v] = (i, j), metal node first; t[v]; and for each of the K <= 8 nodal fields q the caller passes,
 *               val[v][k] = q_i + t (q_j - q_i), without fused multiply-add.
 *   totals      vertices, triangles, bad_nodes, bad_tets, degenerate_tets, and area = the sum over the triangles in list
 *               order of 0.5 |(B - A) x (C - A)| of the oriented triple (differences, cross product, (n0 n0 + n1 n1) + n2 n2,
 *               square root), summed in the fixed tree of the porosity totals over workgroups of 256 consecutive triangles;
 *               +0.0 for no triangle.
 *   properties  every triangle edge lies on a tet face or is a quad's diagonal.  An interior tet face that the surface cuts
 *               holds exactly one segment, and both its tets emit it (unless one of them is bad or degenerate), so the mesh is
 *               edge-manifold: every edge that is not on a boundary face of the tet mesh is used by exactly two triangles, in
 *               opposite directions.  A metal region that does not touch the boundary gives a closed, consistently oriented
 *               surface, and the volume (1 / 6) sum A . (B x C) it encloses is the volume of {f > 0} that
 *               DflMeshLevelSetVolume sums tet by tet.
 *   time step   with every > 0, DflTimeStep evaluates on every every-th call since the Set call, at the wgold it has just
 *               written, after the porosity record, with the one field T.  With a communicator it prints why and returns -1.
 * No atomics on floats; counts use integer atomics, whose result no order changes: two evaluations of one state agree bit for
 * bit, lists included.  An evaluation is 5 launches, one wait for the counts and, where there is a triangle, 9 more launches.
 * Limits: node, tet, triangle and key counts below 2^31. */
typedef struct DflSurfaceMesh {
    f64 level; index_type side;                 /* metal where side (phi - level) > 0 */
    index_type every;                           /* > 0: DflTimeStep evaluates on every every-th call; 0: never */
} DflSurfaceMesh;
typedef struct DflSurfaceMeshStats {
    int64_t vertices, triangles, bad_nodes, bad_tets, degenerate_tets;
    int64_t fields;                             /* K of the last evaluation: the row length of vals */
    f64 area;
} DflSurfaceMeshStats;
#define DFL_SURFACE_MESH_FIELDS 8
/* host only: 0 when DflMeshSetSurfaceMesh accepts the configuration, else why not in `why`: a level that is not finite, side not
 * +-1, every < 0 */
int  DflSurfaceMeshCheck(const DflSurfaceMesh* cfg, char* why, size_t why_len);
/* the configuration is copied; NULL: off, frees everything of its own.  A refused configuration is reported on stderr and
 * leaves the mesh as it was.  Builds every buffer whose size follows from the mesh, forgets the last evaluation and restarts
 * the count of time steps (synchronises) */
void DflMeshSetSurfaceMesh(Mesh3D* mesh, const DflSurfaceMesh* cfg);
b32  DflMeshSurfaceMeshEnabled(const Mesh3D* mesh);
/* w: the device 6N state; fields: num_fields device [N] arrays (a host array of pointers; NULL with 0).  Returns the number of
 * triangles.  Waits for the device once, for the triangle and key counts; the lists grow by x 1.5 when a count exceeds their
 * capacity (the vertex lists are sized by the key count, which bounds the vertices; the field values by keys x num_fields)
 * and the call allocates nothing otherwise.  The geometry is read on every call: DflMeshGeometryChanged needs nothing here.
 * Without a configuration, or with num_fields outside 0 .. 8: a line on stderr, returns -1, the last evaluation stays */
index_type DflMeshSurfaceMesh(Mesh3D* mesh, const f64* w, const f64* const* fields, index_type num_fields);
/* synchronises; the totals of the last evaluation (all zero before the first).  Without a configuration: a line on stderr */
void DflMeshSurfaceMeshStats(Mesh3D* mesh, DflSurfaceMeshStats* out);
/* synchronises; device pointers that stay valid until the next evaluation or Set call: verts [nv][3], edge [nv][2], t [nv],
 * vals [nv][K] (K of the last evaluation; NULL for 0), tris [nt][3], tri_tet [nt]; any of them may be NULL.  Returns nt and
 * writes nv; 0 and NULL pointers without a configuration */
index_type DflMeshSurfaceMeshArrays(Mesh3D* mesh, const f64** verts, const index_type** edge, const f64** t, const f64** vals,
                                    const index_type** tris, const index_type** tri_tet, index_type* nv);
/* copies the last evaluation to host buffers verts [nv][3], vals [nv][K], tris [nt][3]; any of them may be NULL; synchronises */
void DflMeshSurfaceMeshCopy(Mesh3D* mesh, f64* verts, f64* vals, index_type* tris);

#ifdef __cplusplus
}
#endif
#endif /* DEDFLOW_H */
