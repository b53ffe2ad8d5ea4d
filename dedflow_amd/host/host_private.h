/* Library-private declarations shared by the host C files. */
#ifndef DFL_HOST_PRIVATE_H
#define DFL_HOST_PRIVATE_H
#include "dedflow.h"
#include "dedflow_kernels.h"

/* RHS patch schedule (host/patch.c): spatial patches of <= 64 tets / <= 64 nodes in a fixed-stride layout (patch p at tet
 * slot p*64, node slot p*64); partial residual records per (patch, node) + a node -> partials list for the ordered second
 * pass. */
typedef struct RhsPatchSched {
    index_type num_patch, total_nodes;
    index_type* d_pnode;     /* device [total_nodes] global node of each patch node, -1 = unused slot */
    u8* d_lien;              /* device [P*64][4] local (patch) node index of each tet vertex */
    index_type* d_goff;      /* device [N+1] node -> range of gidx */
    index_type* d_gidx;      /* device [total_nodes] partial record ids of each node, ascending patch */
    f64* d_partial;          /* device [total_nodes][6] */
    index_type* d_cnt;       /* device [P] num_tets | num_nodes << 16 */
    /* the adjacency of a patch node (its (tet, vertex) results, ascending tet) cut into sub-lists of <= 4 entries */
    uint16_t* d_sub4;        /* device [P][128][4] result slots (local tet * 4 + a) of each sub-list, 256 = the zero slot */
    uint16_t* d_sub_start;   /* device [P][65] first sub-list of each patch node; entry nn = number of sub-lists */
} RhsPatchSched;
RhsPatchSched* DflBuildRhsPatchSchedule(Mesh3D* mesh);
void DflFreeRhsPatchSchedule(RhsPatchSched* ps);

/* Slot-owner patch schedule (host/slotpatch.c): node patches; every nodal nonzero is summed by one lane pair. */
typedef struct SlotPatchSched {
    const CSRAttr* attr;
    index_type num_patch, max_tets, max_slots, max_contrib;
    int64_t total_tets;
    int32_t* d_hdr;          /* device [num_patch][8]: tet_off, num_tet | num_node << 16, pos_off, num_pos, group_off, trips_lo, trips_hi, node_off */
    uint32_t* d_ptet_lid;    /* device [total_tets]: the four patch-local node ids (a byte each) of every (patch, tet) pair */
    index_type* d_pnode;     /* device [total_nodes]: global ids of every patch's distinct nodes, ascending inside a patch */
    index_type max_nodes;
    int64_t total_nodes;
    index_type* d_slot_nz;   /* device [positions] nodal nonzero of each slot position (+ split flags) */
    uint32_t* d_ldesc;       /* device lane-major descriptor groups: [group][64 lanes] x 2 x ((local tet << 4) | (a << 2) | b) */
} SlotPatchSched;
SlotPatchSched* DflBuildSlotPatchSchedule(Mesh3D* mesh, const CSRAttr* spy, index_type leaf, index_type slot_cap, index_type tet_cap);
void DflFreeSlotPatchSchedule(SlotPatchSched* ps);

/* Assembly configuration of ONE mesh: a copy of the process defaults (the DflSet* setters of include/dedflow.h) taken
 * at Mesh3DCreate, so that two meshes with different schedules / face groups / patch shapes coexist in one process. */
typedef struct AsmConfig {
    int sched_mode;              /* 0 reference colors, 1 compact colors, 4 slot-owner patches (default) */
    index_type face_group;       /* boundary group of the weak-BC faces (4 in the reference, assemble.cu:1826-1828) */
    index_type slot_leaf, slot_cap, slot_tets;  /* schedule 4: nodes per patch, nodal nonzeros, tets touching the patch */
} AsmConfig;
const AsmConfig* DflAsmDefaults(void);
struct FlowWork;
void DflFreeFlowWork(struct FlowWork* fw);

typedef struct MeshExt {
    AsmConfig cfg;                 /* assembly configuration of this mesh */
    struct FlowWork* flow;         /* alpha-level state vectors + norm scratch of SolveFlowSystem (host/driver.c) */
    b32 nodep_current;             /* the packed node records already hold the states the next AssembleSystem is given */
    index_type* ien_b;             /* device [T][4], elements in execution-schedule order */
    index_type sched_num;          /* number of conflict-free launches of the execution schedule */
    index_type* sched_offset;      /* host [sched_num+1] */
    index_type* nzmap_b;           /* device [T][16], (elem,a,b) -> nodal nonzero, batch order */
    const CSRAttr* nzmap_attr;     /* pattern the map was built for */
    index_type face_group;         /* boundary group the face lists below belong to (-1: none) */
    index_type face_nf;            /* faces of that group */
    index_type face_nn;            /* nodes touched by their parent tets */
    index_type *face_node, *face_node_off, *face_node_ent; /* device: node, CSR offsets, entries f*4+a (ascending f) */
    const CSRAttr* face_attr;      /* pattern the nonzero lists below were built for */
    index_type face_nnz;           /* nodal nonzeros touched by the faces' 4x4 node blocks */
    index_type *face_nz, *face_nz_off, *face_nz_ent;       /* device: nonzero, CSR offsets, entries f*16+a*4+b */
    f64 *face_pF, *face_pJ;        /* device parking buffers [nf][16] and [nf][256] */
    index_type* h_f2e;             /* host copy of bound_f2e */
    f64* egeo_b;                   /* device [T][16] element geometry cache in schedule order (LHS kernel) */
    f64* nodep;                    /* device [N][16] packed gather records (x,u,phi,T,du,p,dphi,dT) */
    f64* nodexu;                   /* device [N][8] compact (x,u) records: all the slot-owner Jacobian kernel reads of a node */
    f64* Fp;                       /* device [N][8] packed residual accumulator, zero between calls */
    RhsPatchSched* rhspatch;       /* RHS patch schedule (mode 4), built on first use */
    SlotPatchSched* slotpatch;     /* LHS slot-owner schedule (mode 4, default), built on first use */
    const f64* ext_load;           /* device [3N] external load on the momentum rows (DflMeshSetExternalLoad), NULL: none */
    struct ScalarState* scalar;    /* phi / T transport (host/scalar.c, DflMeshSetScalarTransport), NULL: off */
    const f64* heat_source;        /* device [N] heat source of the T rows (DflMeshSetHeatSource), NULL: none */
    const f64* vol_source;         /* device [N] volume source of the p rows (DflMeshSetVolumeSource), NULL: none */
    struct SurfaceState* surface;  /* free-surface forces (host/surface.c, DflMeshSetSurfaceForces), NULL: off */
    struct PhaseState* phase;      /* phase change (host/phase.c, DflMeshSetPhaseChange), NULL: off */
    b32 phase_current;             /* its D and H already hold the alpha states the next driver assembly is given */
    struct ThermalState* thermal;  /* thermal material (host/thermal.c, DflMeshSetThermalMaterial), NULL: off */
    struct FluidState* fluid;      /* fluid material (host/fluid.c, DflMeshSetFluidMaterial), NULL: off */
    struct RedistanceState* redistance; /* level-set redistancing (host/redistance.c, DflMeshSetRedistance), NULL: off */
    struct VolumeState* volume;    /* level-set volume correction (host/volume.c, DflMeshSetVolumeCorrection), NULL: off */
    struct SolidifyState* solidify; /* solidification record (host/solidify.c, DflMeshSetSolidification), NULL: off */
    struct TrackState* track;      /* track cross-sections (host/track.c, DflMeshSetTrackSections), NULL: off */
    struct PorosityState* porosity; /* porosity record (host/porosity.c, DflMeshSetPorosity), NULL: off */
    struct SurfaceMeshState* surface_mesh; /* surface mesh (host/surface_mesh.c, DflMeshSetSurfaceMesh), NULL: off */
    index_type *v2e_row, *v2e_col; /* device [N+1], [4T]: the sorted V2E map (DflMeshSortedV2E), NULL until first asked for */
    dfl_step_consts step;          /* the time step of this mesh and everything derived from it (host/timestep.c): DflMeshStepConsts */
    struct StepLimitState* steplimit; /* DflMeshTimeStepLimits: partials and results, sized at the first call (host/timestep.c) */
    uint64_t geom_epoch;           /* counts DflMeshGeometryChanged: what a particle context derived from the coordinates is stale */
} MeshExt;

/* the generalized-alpha constants of the time integration (src/assemble.cu:23-27), textually those of csrc/asm_device.hpp */
#define kRHOC (0.5)
#define kALPHAM ((3.0 - kRHOC) / (1.0 + kRHOC))
#define kALPHAF (1.0 / (1.0 + kRHOC))
#define kGAMMA (0.5 + kALPHAM - kALPHAF)

/* the time step of a mesh (include/dedflow.h, "time step"; host/timestep.c): what the kernels and the driver take from it, derived
 * by dfl_step_consts_from_dt alone when the mesh is made and whenever DflMeshSetTimeStep accepts a step.  Read it at the call */
static inline const dfl_step_consts* DflMeshStepConsts(const Mesh3D* mesh) { return &((const MeshExt*)mesh->ext)->step; }
struct StepLimitState;
void DflStepLimitFree(struct StepLimitState* st);
/* the configurations the step limits read (host/surface.c, host/fluid.c): NULL while the feature is off */
const DflSurfaceForces* DflSurfaceConfig(const Mesh3D* mesh);
const DflFluidMaterial* DflFluidConfig(const Mesh3D* mesh);

/* the sorted V2E map of a mesh: per node its tets in ascending tet id, device [N + 1] and [4T].  One per mesh, shared by every
 * pass that sums over a node's tets in that order (scalar Jacobians, free-surface forces, phase change, the particle
 * coupling's node scatter and neighbour table).  The pointers are borrowed: the mesh builds the map at the first call
 * (allocates and synchronises, then never again) and Mesh3DDestroy alone frees it, so clearing one feature cannot take it
 * from another.  It depends on the connectivity only: DflMeshGeometryChanged leaves it alone. */
void DflMeshSortedV2E(Mesh3D* mesh, const index_type** vrow, const index_type** vcol);
/* the [T] bytes of a per-tet flag pass, allocated or freed (after a synchronisation) to match `on` */
void DflTetFlagsMatch(u8** flag, index_type T, b32 on);

/* the host side of a "count per workgroup -> scan -> emit in ascending tet order" pass (redistancing, volume correction, the
 * laser surface): the counts of the one-thread-per-tet kernels, their exclusive scan and the scan's scratch.  chunk_sum may
 * serve other scans of the same owner (the redistancing cells, the laser surface's node heads) */
typedef struct DflBlockScan {
    index_type nblk;                  /* workgroups of the tet passes: ceil(T / dfl_tets_per_block()) */
    index_type *count, *base;         /* device [nblk], [nblk + 1] */
    index_type *chunk_sum, cap_chunk; /* device [cap_chunk] */
} DflBlockScan;
/* other_n: the largest other count that will be scanned through chunk_sum (0: none) */
void DflBlockScanAlloc(DflBlockScan* bs, index_type T, index_type other_n);
/* chunk_sum grows to serve a scan of n entries; the caller has synchronised */
void DflBlockScanReserve(DflBlockScan* bs, index_type n);
void DflBlockScanFree(DflBlockScan* bs);
/* enqueues the scan of count into base and the copy of the total base[nblk] to *total; does not synchronise */
void DflBlockScanEnqueue(const DflBlockScan* bs, index_type* total, hipStream_t s);
/* the capacity a list grows to when it must hold n entries: n + n / 2, n itself where that overflows */
index_type DflGrowCap(index_type n);
/* the bounding box of N > 0 nodes from host coordinates xg [N][3] (a NaN coordinate is passed over), and that of the nodes
 * the device holds (copies them to the host: the caller has synchronised) */
void DflNodeBounds(const f64* xg, index_type N, f64 lo[3], f64 hi[3]);
void DflMeshNodeBounds(Mesh3D* mesh, f64 lo[3], f64 hi[3]);

void DflMeshPrepareFaces(Mesh3D* mesh, index_type group);
void DflMeshPrepareFaceNonzeros(Mesh3D* mesh, index_type group, const CSRAttr* spy);
void DflMeshFreeFaceLists(struct MeshExt* x);
/* AssembleSystemTet with J = beta_J * J + contributions (beta_J = 0 only takes effect in schedule 4) */
void DflAssembleSystemTetBeta(Mesh3D* mesh, f64* wgalpha, f64* dwgalpha, f64* F, Matrix* J, f64 beta_J);
b32 DflQuiet(void);

/* workspace of a ParticleContext (ctx->ext): the contact sweep (host/particle.c) and the fluid coupling (host/couple.c) */
typedef struct ParticleExt {
    f64 kn, gamma_n, dt;
    f64 cell;
    index_type ncell;
    /* persistent workspace of the sweep (device): nothing is allocated, freed or synchronised per sweep */
    index_type *cell_of, *rank, *slot, *order;  /* [P] */
    index_type *count, *cell_start, *chunk_sum; /* [ncell^3 + 1], [ncell^3 + 1], [chunks] */
    f64* sorted;                                /* [P][6] position + velocity in (cell, id) order */
    index_type cap_particle, cap_cell;
    struct CoupleState* couple;                 /* particle-fluid coupling (host/couple.c), NULL when off */
    struct WallState* walls;                    /* mesh walls (host/walls.c), NULL: the unit box */
    /* contact friction and rotation (ParticleContextSetFriction); friction is on when omega != NULL */
    dfl_friction_law law;                       /* mu, resolved kt / gamma_t; dt and inertia are set per sweep */
    f64 *omega, *alpha, *sorted_w;              /* device [P][3] */
    dfl_contact_hist* hist[2];                  /* device [P][DFL_DEM_MAX_HISTORY] rows, ping-pong */
    index_type* hist_count[2];                  /* device [P] live entries of every row */
    index_type* overflow;                       /* device [1] */
    int hist_cur;                               /* the rows the next sweep reads */
    f64 gravity[3];                             /* body acceleration of ParticleContextUpdate */
    index_type cap;                             /* capacity of every per-particle buffer (>= num_particle; host/flow.c) */
    b32 order_valid;                            /* `order` is the last sweep's, for the current particles */
    b32 sort_valid;                             /* ... and its cell list and sorted copies are those of the current grid and
                                                   sizes (cleared by SetSizes / SetInflowSizes / SetWallMesh too): what a
                                                   bare heat step needs before it reuses the sweep */
    struct FlowState* flow;                     /* particle inflow / outflow (host/flow.c), NULL when never set */
    /* polydisperse particles (ParticleContextSetSizes); monodisperse when radius == NULL */
    f64 *radius, *mass;                         /* device [cap], by particle id */
    f64* sorted_r;                              /* device [cap] radii in the sweep's cell order */
    f64 rmax;                                   /* upper bound on every radius (host only, never lowered by Remove) */
    b32 in_sizes;                               /* ParticleContextSetInflowSizes was called: inserted radii in [in_r_lo, in_r_hi) */
    f64 in_r_lo, in_r_hi;
    struct HeatState* heat;                     /* particle heat transfer (host/heat.c), NULL when off */
    struct LaserState* laser;                   /* laser energy deposition (host/laser.c), NULL when off; needs heat */
    struct CaptureState* capture;               /* melt-pool capture (host/capture.c), NULL when off; needs the coupling */
    struct SurfaceContactState* surface_contact; /* solid-surface contact (host/surface_contact.c), NULL when off; needs the coupling */
} ParticleExt;
/* the per-particle sizes of the kernels (all NULL, rmax 0 while x->radius == NULL: one size) */
dfl_sizes DflSizes(const ParticleExt* x);
/* the radius range of the particles the next ParticleContextAdd inserts: (r_lo, r_hi) of SetInflowSizes, else (R, R) */
void DflInflowRadii(const ParticleContext* ctx, f64* r_lo, f64* r_hi);
/* the history of the next sweep (flips the ping-pong: call once per sweep); friction off: all NULL */
dfl_contact_history DflFrictionHistory(ParticleExt* x);
/* after a sweep, without flipping: the rows that sweep read as the previous ones, and the rows it wrote (with their counts) as
 * the current ones, for a contact that appends to them (host/surface_contact.c); friction off: all NULL */
dfl_contact_history DflFrictionHistoryCurrent(const ParticleExt* x);
dfl_friction_law DflFrictionLaw(const ParticleContext* ctx);
void DflFrictionClearHistory(ParticleContext* ctx); /* no-op when friction is off */
/* the sweep's device workspace for P particles over nbin cell-list bins (count / cell_start [nbin + 1]); grows only */
void DflDemReserve(ParticleExt* x, index_type P, index_type nbin);
/* the cell sort of the contact sweep alone (unit box or mesh-wall grid): order / cell_start / sorted copies, order_valid */
void DflDemBuildCells(ParticleContext* ctx);
/* the per-particle device arrays of a context, one table for all features (host/pfields.c).  A row: the owning pointer,
 * the bytes of one particle and a kind -- carried (the first num_particle entries follow the particle), scratch (sized by
 * the capacity, contents never carried) or the friction history (carried by grow; a compaction remaps its keys itself).
 * `extra`: entries beyond the capacity. */
enum { DFL_PF_CARRIED, DFL_PF_SCRATCH, DFL_PF_HISTORY };
enum { DFL_PF_BASE = 1, DFL_PF_FRICTION = 2, DFL_PF_SIZES = 4, DFL_PF_HEAT = 8, DFL_PF_COUPLE = 16, DFL_PF_LASER = 32, DFL_PF_FLOW = 64,
       DFL_PF_CAPTURE = 128 };
#define DFL_PF_MAX_ROWS 48
typedef struct DflPField {
    void** ptr;
    int bytes, kind, extra;
} DflPField;
unsigned DflParticleLiveFeatures(const ParticleContext* ctx);     /* coord / vel / acc and every feature that is on */
int DflParticleFields(ParticleContext* ctx, unsigned features, DflPField* rows); /* rows [DFL_PF_MAX_ROWS]; returns their number */
void* DflParticleFieldAlloc(const DflPField* row, index_type cap);  /* a buffer of the row for capacity cap */
/* every array of one feature at the context's capacity x->cap (its state struct is attached), and freed and NULLed again */
void DflParticleFieldsAlloc(ParticleContext* ctx, unsigned feature);
void DflParticleFieldsFree(ParticleContext* ctx, unsigned feature);
index_type DflReadDeviceIndex(const index_type* d);               /* one device counter copied back (synchronises) */
/* particle-fluid coupling state (host/couple.c) */
typedef struct CoupleState {
    Mesh3D* mesh;
    index_type N, T, P;
    DflFluidCoupling cfg;
    b32 use_order;                   /* locate in the contact sweep's cell order (DFL_COUPLE_CELL_ORDER=0: id order) */
    index_type* nbr;                 /* device [T][4] */
    index_type* seed;                /* device [gdim^3] */
    index_type gdim;
    f64 lo[3], inv_h[3];
    index_type *tet, *lost;          /* device [cap], [1] */
    f64 *lambda, *imp;               /* device [cap][4], [cap][3] */
    index_type *tcount, *tstart;     /* device [T], [T+1] */
    index_type *rank, *slot, *members; /* device [cap] */
    void* scan_tmp;
    int64_t scan_bytes;
    f64* load;                       /* device [3N]: the reaction load DflTimeStep registers */
    f64 imp_time;                    /* time the impulses were accumulated over */
    f64 *rem_load, *rem_tmp;         /* device [3N]: -(impulse of removed particles) scattered to the nodes, and scratch */
    b32 rem_pending;                 /* rem_load holds something the next reaction load adds */
} CoupleState;
void DflCoupleFree(ParticleContext* ctx);
/* the node scatter of the coupled mesh: out[ncomp a + d] = -scale * sum over the particles p of the tets e around node a of
 * lambda_{p,k(a,e)} val[ncomp p + d], `tet` (c->tet, or the removed particles' rtet) saying which tet holds p; ncomp 1 or 3.
 * The sort by tet, then the node pass */
void DflCoupleNodeScatter(ParticleContext* ctx, const index_type* tet, const f64* val, int ncomp, f64 scale, f64* out);
/* scatter the pending impulse of the particles with rtet[i] >= 0 (removed, located) into rem_load (host/couple.c) */
void DflCoupleAccumulateRemoved(ParticleContext* ctx, const index_type* rtet);
/* particle heat transfer (host/heat.c): every per-particle buffer has the context's capacity */
typedef struct HeatState {
    DflParticleHeat cfg;
    f64 cp_f, k_f;                   /* resolved fluid constants */
    f64 *temp, *e, *rate;            /* device [cap] by particle id: temperature, pending energy from the fluid, last heat rate */
    f64 *q, *sorted_t;               /* device [cap]: conduction rate by id, temperatures in the sweep's cell order */
    f64 time;                        /* time the pending energy was accumulated over */
    index_type N;                    /* nodes the two buffers below are sized for (0: none yet) */
    f64 *source, *rem_q;             /* device [N]: the source DflTimeStep registers; -(energy of removed particles) per node */
    b32 rem_pending;
} HeatState;
void DflHeatFree(ParticleContext* ctx);
/* one thermal sub-step after the integration of ParticleContextUpdate (w NULL) / ParticleContextFluidStep */
void DflHeatStep(ParticleContext* ctx, const f64* w);
void DflHeatCopy(ParticleContext* dst, const ParticleContext* src);
void DflHeatCouplingChanged(ParticleContext* ctx); /* SetFluidCoupling: pending energy and time start from zero */
/* scatter the pending energy of the particles with rtet[i] >= 0 (removed, located) into rem_q, as the impulse above */
void DflHeatAccumulateRemoved(ParticleContext* ctx, const index_type* rtet);
b32 DflHeatPending(const ParticleContext* ctx);    /* heat on, coupled, and a coupled heat step ran since the last source */
const f64* DflParticlePendingEnergy(const ParticleContext* ctx); /* device [P]: e_i since the last source (tests, probes) */
const f64* DflParticleConductionRate(const ParticleContext* ctx); /* device [P]: q_i of the last heat step with k_p > 0 (tests) */
b32 DflParticleHeatTwoWay(const ParticleContext* ctx);
f64* DflParticlePendingHeatSource(ParticleContext* ctx); /* the pending source in the context's own [N] buffer, or NULL */
const f64* DflMeshHeatSource(const Mesh3D* mesh);
/* laser energy deposition (host/laser.c); every call below is a no-op on a context without a laser */
typedef struct LaserState {
    DflLaser cfg;                    /* as the caller gave it */
    f64 dir[3], e1[3], e2[3];        /* the frame of include/dedflow.h */
    f64 t;                           /* elapsed scan time */
    index_type n, ncol;
    f64* gw;                         /* device [2n]: gx, gy */
    index_type nbin;                 /* bins of the column sort: the columns + one per 8 particle ids for those outside */
    index_type *count, *cell_start, *chunk_sum; /* device [nbin + 1], [nbin + 1], [chunks], sized with the capacity */
    uint64_t* colkey;                /* device [ncol] */
    f64 *col_T, *part, *tally;       /* device [ncol], [6][ncol], [6] */
    index_type* col_face;            /* device [ncol] */
    f64 *rate, *sorted, *sorted_r, *k_tau;         /* device [cap], [cap][6], [cap], [cap] */
    index_type *cell_of, *rank, *slot, *order, *k_id; /* device [cap] */
    /* substrate */
    index_type nf, ns;               /* candidate faces, their distinct nodes */
    dfl_wall_tri* tri;               /* device [nf], ascending record id */
    index_type *snode, *soff, *sface; /* device [ns], [ns + 1], [3 nf]: node id, its faces as 4 face + local vertex */
    f64 *power, *energy;             /* device [ns] */
    f64 vdmin, vdmax;                /* range of v . dir over the candidates' vertices */
    f64 time;                        /* time the energy was accumulated over */
    struct LaserSurface* surf;       /* the level-set surface as a target (host/laser_surface.c), NULL when off */
} LaserState;
/* the laser on the level-set surface (host/laser_surface.c): configuration, the depth range of the coupled mesh's bounding
 * box, the snapshot of the last Update and the compact nodal power / energy keyed by its node list */
typedef struct LaserSurface {
    DflLaserSurface cfg;
    Mesh3D* mesh;                    /* the coupled mesh the buffers are sized for */
    index_type N, T;
    f64 vdmin, vdmax;                /* range of x . dir over the corners of the node bounding box */
    DflBlockScan scan;               /* the facet counts of the tet passes; its chunk_sum also serves the 4 cap node heads */
    index_type nf;                   /* candidate facets of the snapshot, -1: no Update yet */
    index_type nn;                   /* facets whose tets the node list covers: nf, or the reflection list's nr */
    index_type nfb;                  /* boundary records in front of them in cand */
    index_type cap, cap_cand;        /* facets the lists hold; records cand holds */
    dfl_wall_tri* cand;              /* device [cap_cand]: the boundary candidates, then the facets */
    f64 *facets, *ft;                /* device [cap][9], [cap][3] */
    index_type *ftet, *fij;          /* device [cap] */
    uint32_t *nkey, *nkey_out;       /* device [4 cap]: the node sort */
    index_type *nrec, *nrec_out, *nflag, *nstart, *fslot, *unode; /* device [4 cap] ([4 cap + 1]: nstart) */
    f64 *power, *energy;             /* device [4 cap], keyed by unode */
    uint64_t *rkey, *rkey_out;       /* device [4 ncol]: the deposit records */
    f64* rval;                       /* device [4 ncol] */
    void* temp;                      /* radix sort scratch */
    int64_t temp_bytes;
    f64* carry;                      /* device [N] or NULL: energy pending when a new snapshot replaced the node list */
    b32 carry_on;                    /* carry holds energy */
    b32 dirty;                       /* a step deposited into energy since it was last cleared */
    struct LaserReflect* refl;       /* reflections on the surface (host/laser_reflect.c), NULL when off */
} LaserSurface;
/* the laser's reflections (host/laser_reflect.c): configuration, the reflection list R of the last Update and the per
 * (bounce, column) output of the last step.  With it set the surface's node list covers the tets of R and fslot is indexed
 * by R, and the step deposits through DflLaserReflectDeposit instead of DflLaserSurfaceDeposit */
typedef struct LaserReflect {
    DflLaserReflection cfg;
    DflBlockScan scan;               /* R's counts of the tet passes */
    index_type nr, cap;              /* facets of R (0: none), facets its lists hold */
    f64 *facets, *grad, *ft;         /* device [cap][9], [cap][3], [cap][3] */
    index_type *tet, *fij;           /* device [cap] */
    index_type nhit;                 /* (max_bounce + 1) ncol */
    index_type* hit_facet;           /* device [nhit] */
    f64 *hit_abs, *hit_w, *ray_end;  /* device [nhit], [nhit][3], [2][ncol] */
    uint64_t *rkey, *rkey_out;       /* device [4 nhit]: the deposit records */
    f64* rval;                       /* device [4 nhit] */
    void* temp;                      /* radix sort scratch of the records */
    int64_t temp_bytes;
    f64* tally;                      /* device [20] */
    b32 stepped;                     /* hit_* hold a step's output */
    /* the cell grid over the coupled mesh's node bounding box: R's facets entered into every cell their boxes overlap */
    f64 lo[3], hi[3];                /* the node bounding box */
    index_type cells_env, group;     /* DFL_LASER_REFLECT_CELLS (0: sized from nr), DFL_LASER_REFLECT_GROUP (lanes per ray) */
    dfl_grid3 grid;
    index_type ncell, cap_cell;      /* cells of the grid of the last Update (0: no grid), cells the arrays hold */
    index_type *cell_count, *cell_start, *cell_chunk; /* device [cap_cell], [cap_cell + 1], [chunks] */
    index_type nentry, cap_entry;
    index_type* cell_entry;          /* device [cap_entry] */
    f64* visited;                    /* device [ncol]: entries tested per column in the last step */
} LaserReflect;
/* for probes: facets in cells and cells of the last Update, mean and max entries tested per ray of the last step (synchronises) */
void DflLaserReflectionGridStats(ParticleContext* ctx, index_type* entries, index_type* cells, f64* mean_visited, f64* max_visited);
void DflLaserReflectFree(LaserSurface* s);           /* frees s->refl */
void DflLaserReflectInstall(LaserState* l, const DflLaserReflection* cfg); /* a checked configuration on a state with a surface */
void DflLaserReflectDropLists(LaserSurface* s);      /* no R, no step output; the capacity stays */
void DflLaserReflectMeshChanged(LaserSurface* s);    /* after bind_mesh: no R, the scan sized for the new mesh */
/* Update: enqueue R's count at the state w with the copy of its total to *nr (rides on Update's one synchronisation); then,
 * with that total, grow R's lists when they must and emit R */
void DflLaserReflectCount(LaserState* l, const f64* w, index_type* nr);
void DflLaserReflectEmit(LaserState* l, const f64* w, index_type nr);
void DflLaserReflectDeposit(LaserState* l, dfl_laser_beam b, f64 dt); /* the step's trace, records, sum and tally */
void DflLaserReflectIdle(LaserState* l);             /* a step without facets: no ray, a zero tally */
void DflLaserSurfaceInstall(ParticleContext* ctx, const DflLaserSurface* cfg); /* a checked configuration on a context with a laser */
void DflLaserSurfaceFree(LaserState* l);             /* frees l->surf */
void DflLaserSurfaceDropSnapshot(LaserState* l, index_type nf); /* pending energy to the dense array, no facets, no keys */
void DflLaserSurfaceCouplingChanged(ParticleContext* ctx); /* drops the snapshot and pending energy, the new depth range */
void DflLaserSurfaceDeposit(LaserState* l, dfl_laser_beam b, f64 dt); /* after the columns of a step with facets */
void DflLaserSurfaceAddSource(LaserState* l, f64* q); /* q += surface energy / l->time; clears it */
void DflLaserSurfaceTimeStep(ParticleContext* ctx, const f64* w); /* DflTimeStep: Update when a surface is set */
void DflLaserFree(ParticleContext* ctx);            /* off: frees the state */
void DflLaserStep(ParticleContext* ctx, f64 dt);    /* one laser step (the laser must be on) */
void DflLaserCouplingChanged(ParticleContext* ctx); /* SetFluidCoupling: the substrate list of the new mesh, nothing pending */
void DflLaserCapacityChanged(ParticleContext* ctx); /* after the table's buffers grew: the bins of the new capacity, rate zero */
void DflLaserCopy(ParticleContext* dst, const ParticleContext* src);
b32 DflLaserPending(const ParticleContext* ctx);    /* substrate energy accumulated since the last heat source */
void DflLaserAddSource(ParticleContext* ctx, f64* q); /* q[N] += that energy / its time; clears it */
/* the boundary faces of the masked groups as wall records in group order (host/walls.c; synchronises; free() both) */
dfl_wall_tri* DflMeshBoundaryTris(Mesh3D* mesh, index_type group_mask, index_type* nf_out, f64 lo[3], f64 hi[3], f64** edges_out);
/* particle inflow / outflow (host/flow.c) */
typedef struct FlowState {
    b32 in_on, out_on;
    DflParticleInflow in;
    DflParticleOutflow out;
    dfl_inlet inlet;                 /* lattice of the current radius */
    f64 inlet_R;                     /* radius the lattice was built for */
    index_type nslot;
    uint64_t call;                   /* Add calls since ParticleContextSetInflow */
    f64 credit;
    int64_t next_tag;
    DflParticleFlowStats stats;
    int64_t* tag;                    /* device [cap] */
    index_type *keep, *newid, *rtet; /* device [cap], [cap + 1], [cap] */
    /* what a compaction writes: buffers of the capacity, one per carried field of the features that are on; after it they
       hold the fields' old buffers.  spare_bytes: bytes per particle of each, which is all that tells them apart */
    void* spare[DFL_FLOW_MAX_FIELDS];
    int spare_bytes[DFL_FLOW_MAX_FIELDS];
    void* scan_tmp;
    int64_t scan_bytes;
    index_type *blocked, *slot, *slot_out; /* device [nslot] */
    uint64_t *key, *key_out;               /* device [nslot] */
    void* sort_tmp;
    int64_t sort_bytes;
    index_type* count;               /* device [1] */
} FlowState;
void DflFlowFree(ParticleContext* ctx);
/* what ParticleContextRemove and ParticleContextCapture share (host/flow.c): the flow state of a context, created with the
 * tags 0 .. P-1 at the first call; the spares the next compaction writes, for the features that are on now; and the
 * compaction itself: with keep [P] and its exclusive scan newid [P + 1] in the flow state and new_count = newid[P] <
 * num_particle, every carried field and the friction history move to the survivors' new ids and the count is set */
FlowState* DflFlowState(ParticleContext* ctx);
void DflFlowEnsureSpares(ParticleContext* ctx);
void DflFlowCompact(ParticleContext* ctx, index_type new_count);
/* melt-pool capture (host/capture.c) */
typedef struct CaptureState {
    DflParticleCapture cfg;
    DflParticleCaptureStats stats;
    f64* dep;                        /* device [cap][5]: the deposits of the last capture call, by particle id (scratch) */
    index_type N;                    /* nodes the buffers below are sized for */
    f64 *A, *A_tmp;                  /* device [N][5]: the accumulator, and one call's node sums */
    f64 *q_vol, *load, *q_heat;      /* device [N], [3N], [N]: what DflTimeStep registers */
    b32 pending, heat_pending;       /* A holds something; ... that was captured with heat on */
} CaptureState;
void DflCaptureFree(ParticleContext* ctx);
void DflCaptureCopy(ParticleContext* dst, const ParticleContext* src);
void DflCaptureCouplingChanged(ParticleContext* ctx); /* SetFluidCoupling: A sized for the new mesh, nothing pending */
b32 DflParticleCaptureOn(const ParticleContext* ctx);
/* two_way and something pending: the source over `time` into the context's own buffers (heat NULL when nothing was captured
 * with heat on); FALSE and nothing done otherwise */
b32 DflCaptureTakePending(ParticleContext* ctx, f64 time, f64** q_vol, f64** load, f64** q_heat);
/* solid-surface contact (host/surface_contact.c) */
typedef struct SurfaceContactState {
    DflSurfaceContact cfg;
    dfl_surface_counters* cnt;       /* device [1] */
    dfl_surface_counters* host;      /* host [1]: where the Stats call copies them */
    int cur;                         /* the parity the last launch counted into */
    f64* grad_max;                   /* device [1]: >= |grad N_k| over the coupled mesh (dfl_surface_grad_max) */
    uint64_t geom_epoch;             /* the mesh's geometry epoch grad_max was computed at */
} SurfaceContactState;
void DflSurfaceContactFree(ParticleContext* ctx);
void DflSurfaceContactCopy(ParticleContext* dst, const ParticleContext* src);
void DflSurfaceContactCouplingChanged(ParticleContext* ctx); /* SetFluidCoupling: uncoupled frees the state; a mesh keeps it */
b32 DflParticleSurfaceContactOn(const ParticleContext* ctx);
/* the contact alone, as ParticleContextFluidStep runs it between the locate and the drag (tests, probes call it by hand
 * after ParticleContextComputeForces and ParticleContextLocate); a no-op when off */
void DflSurfaceContactApply(ParticleContext* ctx, const f64* w);
/* probes only: zeroes the bound, so that every located particle gathers T and the coordinates until the bound is next
 * recomputed (a coupling or geometry change); results are the same */
void DflSurfaceContactTestNoEarlyExit(ParticleContext* ctx);
struct WallState;
void DflWallsFree(struct WallState* w);
/* the contact sweep against the mesh walls (ParticleContextComputeForces when walls are set) */
void DflWallsComputeForces(ParticleContext* ctx);
void DflWallsBuildCells(ParticleContext* ctx);                   /* its cell sort alone */
const dfl_grid3* DflWallsParticleGrid(const ParticleContext* ctx); /* the particle grid of that sort */
/* the mesh a particle context is coupled to (NULL: uncoupled), its two-way switch, and the reaction load of the sub-steps
 * since the last ParticleContextReactionLoad into the context's own [3N] buffer (NULL when there were none) */
Mesh3D* DflParticleCoupledMesh(const ParticleContext* ctx);
b32 DflParticleTwoWay(const ParticleContext* ctx);
f64* DflParticlePendingLoad(ParticleContext* ctx);
const f64* DflMeshExternalLoad(const Mesh3D* mesh);

/* profiling tags (runtime.c) */
enum { DFL_TAG_SPMV = 0, DFL_TAG_CGS_DOTS = 1, DFL_TAG_CGS_UPDATE = 2, DFL_TAG_PC = 3, DFL_TAG_ASM_LHS = 4,
       DFL_TAG_ASM_RHS = 5, DFL_TAG_FACE = 6, DFL_TAG_DIRICHLET = 7, DFL_TAG_SMALL = 8 };
void DflProfileEnable(int on);
int DflProfileBegin(int tag);
void DflProfileEnd(int slot);
int DflProfileCollect(int tag, double* total_ms, double* min_ms);
int DflProfileDurations(int tag, double* out_ms, int max_out);
#define DFL_TIMED(tag, call) do { int _s = DflProfileBegin(tag); call; DflProfileEnd(_s); } while (0)

/* AssembleSystem for the Newton driver: `prepacked` = the packed node records were just written from these very states
 * by the fused alpha-state kernel (host/driver.c), so the pack launch is skipped */
void DflAssembleSystemPrepacked(Mesh3D* mesh, f64* wgalpha, f64* dwgalpha, f64* F, Matrix* J, Dirichlet** bcs, index_type nbc,
                                b32 prepacked);
f64* DflMeshNodeRecords(Mesh3D* mesh); /* [N][16] packed gather records, allocated on first use */
void DflKrylovWorkspaceInPool(int on);
void* DflVectorArenaAlloc(size_t bytes);
int DflVectorArenaFree(void* p);
/* driver.c */
index_type SolveFlowSystem(Mesh3D* mesh, f64* wgold, f64* dwgold, f64* dwg, Matrix* J, f64* F, f64* dx, Krylov* ksp,
                           Dirichlet** bcs, index_type nbc, index_type maxit, f64* rnorm_out, f64* rnorm_init_out);
void DflKrylovSolvePrepared(Krylov* ksp, Matrix* A, f64* x, f64* b); /* KrylovSolve without PC (re)build and PCSetup */

/* host/scalar.c: the phi / T transport of a mesh (all of them no-ops or unused while it is off) */
struct ScalarState;
void DflScalarFree(struct ScalarState* st);
void DflScalarCaptureResidual(Mesh3D* mesh, const f64* F);        /* F[4N:6N) -> the mesh's [2N] residual, Dirichlet rows zeroed */
void DflScalarSolveIncrements(Mesh3D* mesh, f64* wgalpha, f64* dwgalpha, f64* dx2); /* Jacobians + both solves -> dx2 [2N] */
void DflScalarNorms(Mesh3D* mesh, f64* out2);                      /* ||R_phi||, ||R_T|| of that residual (synchronises) */
void DflScalarWork(Mesh3D* mesh, f64** F, f64** dx2);              /* scratch [6N], [2N] of DflScalarTransportSolve */
b32 DflScalarAdvancesT(const Mesh3D* mesh);                        /* a transport is set and advances T */

/* host/surface.c: the free-surface forces of a mesh */
struct SurfaceState;
void DflSurfaceFree(struct SurfaceState* st);
/* 0 when DflMeshSetSurfaceForces accepts the configuration, else why not in `why` */
int DflSurfaceForcesCheck(const DflSurfaceForces* cfg, char* why, size_t why_len);
b32 DflSurfaceInTimeStep(const Mesh3D* mesh); /* a configuration with in_time_step is set */
/* in_time_step is set: load [3N] and q_heat [N] at the state w into the mesh's own buffers; FALSE and nothing done otherwise */
b32 DflSurfaceTakeLoad(Mesh3D* mesh, const f64* w, f64** load, f64** q_heat);

/* host/phase.c: the phase change of a mesh (no-ops while it is off) */
struct PhaseState;
void DflPhaseFree(struct PhaseState* st);
/* the drag and latent terms of one assembly: F += D u, H dT and J += fact2 D on the diagonal blocks, D and H evaluated at
 * wgalpha.  reuse: the caller is the Newton driver, which assembles F, J and JT at the same alpha states and clears
 * MeshExt.phase_current whenever it forms new ones; any other caller passes FALSE and the coefficients are recomputed */
void DflPhaseApplySystem(Mesh3D* mesh, const f64* wgalpha, const f64* dwgalpha, f64* F, Matrix* J, b32 reuse);
/* kALPHAM H on the diagonal of the T Jacobian values val_T over the nodal pattern attr */
void DflPhaseApplyScalarJacobian(Mesh3D* mesh, const f64* wgalpha, const CSRAttr* attr, f64* val_T, b32 reuse);

/* host/thermal.c: the thermal material of a mesh (no-ops while it is off) */
struct ThermalState;
void DflThermalFree(struct ThermalState* st);
/* F[5N + a] += r[a] at the alpha states, one launch; nothing unless the mesh's scalar transport advances T (the rows are
 * zeroed otherwise) */
void DflThermalApplyRows(Mesh3D* mesh, const f64* wgalpha, const f64* dwgalpha, f64* F);
/* the configuration as the kernels take it (the T Jacobian's MATERIAL launch, host/scalar.c), NULL: off */
const dfl_thermal_params* DflThermalParams(const Mesh3D* mesh);

/* host/fluid.c: the fluid material of a mesh (no-ops while it is off) */
struct FluidState;
void DflFluidFree(struct FluidState* st);
/* F[0 .. 4N) += r at the alpha states (one launch) and, with J, the block values += S (one launch; J must keep the block
 * layout) */
void DflFluidApplySystem(Mesh3D* mesh, const f64* wgalpha, const f64* dwgalpha, f64* F, Matrix* J);

/* host/redistance.c: the level-set redistancing of a mesh (no-ops while it is off) */
struct RedistanceState;
void DflRedistanceFree(struct RedistanceState* st);
void DflRedistanceGeometryChanged(struct RedistanceState* st); /* the nodes moved: the next call makes the cell grid again */
b32 DflRedistanceInTimeStep(const Mesh3D* mesh);                /* a configuration with every > 0 is set */
/* counts one DflTimeStep; on every every-th since the Set call redistances wgold (DflMeshRedistance) and returns TRUE */
b32 DflRedistanceTimeStep(Mesh3D* mesh, f64* wgold);
/* host/volume.c: the level-set volume correction of a mesh (no-ops while it is off) */
struct VolumeState;
void DflVolumeCorrectionFree(struct VolumeState* st);
b32 DflVolumeCorrectionInTimeStep(const Mesh3D* mesh);         /* a configuration with every > 0 is set */
/* counts one DflTimeStep; on every every-th since the Set call corrects wgold (DflMeshVolumeCorrect) */
void DflVolumeCorrectionTimeStep(Mesh3D* mesh, f64* wgold);
/* with track_capture: the target grows by side * time * sum q_vol (device [N]); sums on the device and waits for it */
void DflVolumeCorrectionCaptured(Mesh3D* mesh, const f64* q_vol, f64 time);
/* host/solidify.c: the solidification record of a mesh (no-ops while it is off) */
struct SolidifyState;
void DflSolidificationFree(struct SolidifyState* st);
b32 DflSolidificationInTimeStep(const Mesh3D* mesh);            /* a configuration with in_time_step is set */
/* DflTimeStep, on entry: with in_time_step and a record not primed yet, the priming update at the incoming wgold */
void DflSolidificationTimeStepPrime(Mesh3D* mesh, const f64* wgold);
/* DflTimeStep, once the step has written wgold: with in_time_step, DflMeshSolidificationUpdate(mesh, wgold, DflMeshTimeStep(mesh)) */
void DflSolidificationTimeStep(Mesh3D* mesh, const f64* wgold);
/* T_prev [N] and the metal flags [N] of the record on the device (tests, probes); NULL when not set */
void DflSolidificationTestFields(const Mesh3D* mesh, const f64** T_prev, const u8** metal);
/* host/track.c: the track cross-sections of a mesh (no-ops while they are off) */
struct TrackState;
void DflTrackSectionsFree(struct TrackState* st);
b32 DflTrackSectionsInTimeStep(const Mesh3D* mesh);             /* a configuration with every > 0 is set */
/* DflTimeStep, once the step has written wgold: counts the call; on every every-th since the Set call
 * DflMeshTrackSections(mesh, wgold, NULL) */
void DflTrackSectionsTimeStep(Mesh3D* mesh, const f64* wgold);
/* the pair list of the last evaluation on the device (tet ids, by station, then ascending) and its 65 segment offsets:
 * station k owns [off65[k], off65[k + 1]), every entry from num_station on is the total, which is returned (synchronises;
 * tests, probes) */
index_type DflTrackSectionsTestPairs(const Mesh3D* mesh, const index_type** list, index_type* off65);
void DflTrackSectionsTestCapacity(const Mesh3D* mesh, index_type* cap_list, index_type* cap_part);
/* host/porosity.c: the porosity record of a mesh (no-ops while it is off) */
struct PorosityState;
void DflPorosityFree(struct PorosityState* st);
b32 DflPorosityInTimeStep(const Mesh3D* mesh);                  /* a configuration with every > 0 is set */
/* DflTimeStep, once the step has written wgold: counts the call; on every every-th since the Set call DflMeshPorosity(mesh, wgold) */
void DflPorosityTimeStep(Mesh3D* mesh, const f64* wgold);
/* launches of the last evaluation (a sort counts as one; 0 before the first): it depends on the mesh and the configuration,
 * never on the state (tests, probes) */
index_type DflPorosityTestLaunches(const Mesh3D* mesh);
/* the capacity of the key lists (tests: they grow only when the closed tets exceed it); cap > 0 sets a smaller one first */
index_type DflPorosityTestCapacity(Mesh3D* mesh, index_type cap);

/* host/surface_mesh.c: the surface mesh of a mesh (no-ops while it is off) */
struct SurfaceMeshState;
void DflSurfaceMeshFree(struct SurfaceMeshState* st);
b32 DflSurfaceMeshInTimeStep(const Mesh3D* mesh);               /* a configuration with every > 0 is set */
/* DflTimeStep, once the step has written wgold: counts the call; on every every-th since the Set call
 * DflMeshSurfaceMesh(mesh, wgold, {T}, 1) */
void DflSurfaceMeshTimeStep(Mesh3D* mesh, const f64* wgold);
/* test hooks (exported, not in dedflow.h): the launches of the last evaluation; the evaluations that allocated so far, with the
 * capacities of the key and triangle lists */
index_type DflSurfaceMeshTestLaunches(const Mesh3D* mesh);
index_type DflSurfaceMeshTestGrows(const Mesh3D* mesh, index_type* cap_key, index_type* cap_tri);

/* named ranges for rocprofv3 --marker-trace (DFL_ROCTX=1); no-ops otherwise */
void DflRangePush(const char* name);
void DflRangePop(void);

int DflDevicePoolEnabled(void); /* the default DEVICE allocator carves large requests out of its pool */
void* DflDevicePoolAllocNoGrow(size_t bytes); /* from the chunks already reserved, or NULL */

void DflMatrixFSRelocateBlockValues(Matrix* m, value_type* new_val); /* host/matrix.c */
value_type* DflMatrixFSScratchBlockBegin(Matrix* m); /* reference-layout (u,p) FS matrix -> scratch block array (host/matrix.c) */
void DflMatrixFSScratchBlockEnd(Matrix* m);
/* host/slotpatch.c */
int DflSlotPatchLimitCheck(int64_t num_positions, int64_t num_tets, int64_t num_nodes, int64_t max_contributions_of_a_position, char* why,
                           size_t why_len);
void DflSlotPatchSetTestLimits(int positions, int tets);

#endif
