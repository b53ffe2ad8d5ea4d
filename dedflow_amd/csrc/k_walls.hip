// DEM contact sweep against the boundary faces of a tet mesh (build-defined, opt-in: ParticleContextSetWallMesh; the
// contact model and the de-duplication rule are stated in include/dedflow.h).
//
// The sweep is the unit-box sweep of k_dem.hip on a general grid:
//   particle grid  origin lo, nx * ny * nz cells (edge >= 4R per axis) over the mesh's bounding box padded by R.  A particle
//                  whose centre lies outside goes to one extra bin, cell nx*ny*nz, sorted behind all others: no neighbour
//                  loop visits that bin, and its own acceleration is zero
//   wall grid      a static uniform grid over the same box (host-built at setup, host/walls.c): cell k lists, ascending,
//                  every wall triangle whose R-expanded bounding box overlaps it.  A particle reads the one cell that holds
//                  its centre: fixed order => bitwise reproducible forces
// The bin kernel is the only new launch of the cell sort (chunk / scan / place / sort are k_dem.hip's); the force kernel
// runs the shared pair loop (dem_sweep.hpp) and then the wall contacts, with the same POLY and FRICTION variants as the
// unit box.  Threads run in the sorted (cell, id) order, so the lanes of a wave share
// one or two wall cells: the "wall cell empty" branch is wave-uniform in the interior, and the 128-byte records (one cache
// line each) of a shared cell are read once per wave from L1 / L2.
#include "dfl_common.hpp"
#include "dem_sweep.hpp"

namespace {

constexpr int BLK = 256;
constexpr int MAXC = DFL_WALL_MAX_CONTACTS;

using dfl_dem::grid_coord;

__device__ __forceinline__ bool in_grid(double x, double lo, double inv, int n) {
    const double c = floor((x - lo) * inv);
    return c >= 0.0 && c < (double)n;
}

__global__ __launch_bounds__(BLK) void wall_bin_kernel(I P, const T* __restrict__ coord, dfl_grid3 g, I* __restrict__ cell_of,
                                                      I* __restrict__ rank, I* __restrict__ count) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i >= P) return;
    const double x = coord[3 * i], y = coord[3 * i + 1], z = coord[3 * i + 2];
    int c = g.n[0] * g.n[1] * g.n[2];  // outside the padded box: the extra bin behind every cell
    if (in_grid(x, g.lo[0], g.inv[0], g.n[0]) && in_grid(y, g.lo[1], g.inv[1], g.n[1]) && in_grid(z, g.lo[2], g.inv[2], g.n[2]))
        c = (int)floor((x - g.lo[0]) * g.inv[0]) + g.n[0] * ((int)floor((y - g.lo[1]) * g.inv[1]) +
                                                             g.n[1] * (int)floor((z - g.lo[2]) * g.inv[2]));
    cell_of[i] = c;
    rank[i] = atomicAdd(&count[c], 1);
}

// closest point q of triangle (a, b, c) to p, by the feature whose Voronoi region holds p (Ericson, Real-Time Collision
// Detection, 5.1.5).  Returns 0 face, 1 edge (local vertices e0 < e1), 2 vertex (local vertex e0)
__device__ __forceinline__ int closest_feature(const double* a, const double* b, const double* c, const double* p, double* q,
                                               int& e0, int& e1) {
    double ab[3], ac[3], ap[3], bp[3], cp[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        ab[d] = b[d] - a[d]; ac[d] = c[d] - a[d];
        ap[d] = p[d] - a[d]; bp[d] = p[d] - b[d]; cp[d] = p[d] - c[d];
    }
    const double d1 = ab[0] * ap[0] + ab[1] * ap[1] + ab[2] * ap[2];
    const double d2 = ac[0] * ap[0] + ac[1] * ap[1] + ac[2] * ap[2];
    e1 = -1;
    if (d1 <= 0.0 && d2 <= 0.0) {
        e0 = 0;
        for (int d = 0; d < 3; ++d) q[d] = a[d];
        return 2;
    }
    const double d3 = ab[0] * bp[0] + ab[1] * bp[1] + ab[2] * bp[2];
    const double d4 = ac[0] * bp[0] + ac[1] * bp[1] + ac[2] * bp[2];
    if (d3 >= 0.0 && d4 <= d3) {
        e0 = 1;
        for (int d = 0; d < 3; ++d) q[d] = b[d];
        return 2;
    }
    const double vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        const double t = d1 / (d1 - d3);
        e0 = 0; e1 = 1;
        for (int d = 0; d < 3; ++d) q[d] = a[d] + t * ab[d];
        return 1;
    }
    const double d5 = ab[0] * cp[0] + ab[1] * cp[1] + ab[2] * cp[2];
    const double d6 = ac[0] * cp[0] + ac[1] * cp[1] + ac[2] * cp[2];
    if (d6 >= 0.0 && d5 <= d6) {
        e0 = 2;
        for (int d = 0; d < 3; ++d) q[d] = c[d];
        return 2;
    }
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
        const double t = d2 / (d2 - d6);
        e0 = 0; e1 = 2;
        for (int d = 0; d < 3; ++d) q[d] = a[d] + t * ac[d];
        return 1;
    }
    const double va = d3 * d6 - d5 * d4;
    if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {
        const double t = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        e0 = 1; e1 = 2;
        for (int d = 0; d < 3; ++d) q[d] = b[d] + t * (c[d] - b[d]);
        return 1;
    }
    const double den = 1.0 / (va + vb + vc);
    const double v = vb * den, w = vc * den;
    for (int d = 0; d < 3; ++d) q[d] = a[d] + ab[d] * v + ac[d] * w;
    return 0;
}

struct Feature {
    int kind;      // 0 face, 1 edge, 2 vertex
    int k0, k1;    // node ids: edge = sorted pair, vertex = (id, -1)
    double q[3];
    double d2;     // |p - q|^2
    double s;      // (p - a) . n
};

__device__ __forceinline__ double plane_distance(const dfl_wall_tri* __restrict__ t, const double* p) {
    return (p[0] - t->v[0]) * t->n[0] + (p[1] - t->v[1]) * t->n[1] + (p[2] - t->v[2]) * t->n[2];
}

__device__ __forceinline__ Feature feature_of(const dfl_wall_tri* __restrict__ t, const double* p) {
    Feature f;
    int e0, e1;
    f.kind = closest_feature(t->v, t->v + 3, t->v + 6, p, f.q, e0, e1);
    f.k0 = f.k1 = -1;
    if (f.kind == 1) {
        const int n0 = t->node[e0], n1 = t->node[e1];
        f.k0 = n0 < n1 ? n0 : n1;
        f.k1 = n0 < n1 ? n1 : n0;
    } else if (f.kind == 2) {
        f.k0 = t->node[e0];
    }
    const double dx = p[0] - f.q[0], dy = p[1] - f.q[1], dz = p[2] - f.q[2];
    f.d2 = dx * dx + dy * dy + dz * dz;
    f.s = plane_distance(t, p);
    return f;
}

__device__ __forceinline__ bool holds(const dfl_wall_tri* __restrict__ t, int k0, int k1) {
    const bool h0 = t->node[0] == k0 || t->node[1] == k0 || t->node[2] == k0;
    if (k1 < 0) return h0;
    return h0 && (t->node[0] == k1 || t->node[1] == k1 || t->node[2] == k1);
}

// wall contacts of particle a over the candidate triangles list[lo, hi) (ascending id), each kept contact handed to the
// sink with its normal, overlap delta and normal force kn delta - gn v.n; returns the number of distinct contacts dropped
// by the cap.  History keys (FRICTION only): a face by the plane id of its triangle, an edge by its sorted node pair, a
// vertex by its node id
template <bool FRICTION, class SinkT>
__device__ __forceinline__ int wall_contacts(const dfl_dem::Particle& a, double kn, double gn, double tol,
                                             const dfl_wall_tri* __restrict__ tri, const I* __restrict__ plane_id,
                                             const I* __restrict__ list, int lo, int hi, SinkT& sink) {
    const double* p = a.p;
    const double* v = a.v;
    const double R = a.r;
    double plane[MAXC][4];   // kept face contacts: normal, offset
    int key[MAXC][2];        // kept edge / vertex contacts: node ids
    int nf = 0, ne = 0, dropped = 0;
    // pass 1: face contacts, one per supporting plane
    for (int k = lo; k < hi; ++k) {
        const dfl_wall_tri* t = tri + list[k];
        const double s = plane_distance(t, p);
        if (!(s > -R && s < R)) continue;  // no contact of any kind: |c - q| >= |s|
        const Feature ft = feature_of(t, p);
        if (ft.kind != 0) continue;
        bool dup = false;
        for (int j = 0; j < nf; ++j)
            dup |= fabs(plane[j][0] - t->n[0]) <= 1e-12 && fabs(plane[j][1] - t->n[1]) <= 1e-12 &&
                   fabs(plane[j][2] - t->n[2]) <= 1e-12 && fabs(plane[j][3] - t->off) <= tol;
        if (dup) continue;
        if (nf + ne >= MAXC) { ++dropped; continue; }
        plane[nf][0] = t->n[0]; plane[nf][1] = t->n[1]; plane[nf][2] = t->n[2]; plane[nf][3] = t->off;
        ++nf;
        const double n[3] = {t->n[0], t->n[1], t->n[2]};
        const double vn = v[0] * n[0] + v[1] * n[1] + v[2] * n[2];
        const double delta = R - ft.s;
        const uint64_t hk = FRICTION ? dfl_friction::KEY_WALL | (uint64_t)plane_id[list[k]] : 0;
        sink.wall(a, hk, n, delta, kn * delta - gn * vn);
    }
    // pass 2: edge and vertex contacts that are local minima of the distance to the wall and off every kept face plane
    const double R2 = R * R;
    for (int k = lo; k < hi; ++k) {
        const dfl_wall_tri* t = tri + list[k];
        const double s = plane_distance(t, p);
        if (!(s > 0.0 && s < R)) continue;
        const Feature ft = feature_of(t, p);
        if (ft.kind == 0 || !(ft.d2 < R2)) continue;
        bool skip = false;
        for (int j = 0; j < nf; ++j)
            skip |= fabs(ft.q[0] * plane[j][0] + ft.q[1] * plane[j][1] + ft.q[2] * plane[j][2] - plane[j][3]) <= tol;
        for (int j = 0; j < ne; ++j) skip |= key[j][0] == ft.k0 && key[j][1] == ft.k1;
        if (skip) continue;
        const double dist = sqrt(ft.d2);
        for (int m = lo; m < hi && !skip; ++m) {
            if (m == k) continue;
            const dfl_wall_tri* u = tri + list[m];
            if (!holds(u, ft.k0, ft.k1)) continue;
            const Feature fu = feature_of(u, p);
            skip = sqrt(fu.d2) < dist - tol;
        }
        if (skip) continue;
        if (nf + ne >= MAXC) { ++dropped; continue; }
        key[ne][0] = ft.k0; key[ne][1] = ft.k1;
        ++ne;
        const double inv = 1.0 / dist;
        const double n[3] = {(p[0] - ft.q[0]) * inv, (p[1] - ft.q[1]) * inv, (p[2] - ft.q[2]) * inv};
        const double vn = v[0] * n[0] + v[1] * n[1] + v[2] * n[2];
        const double delta = R - dist;
        const uint64_t hk = ft.k1 >= 0 ? dfl_friction::edge_key(ft.k0, ft.k1) : (dfl_friction::KEY_VERTEX | (uint64_t)ft.k0);
        sink.wall(a, hk, n, delta, kn * delta - gn * vn);
    }
    return dropped;
}

// The force kernel over a mesh: pairs (the order of the unit box), then the wall contacts of the wall-grid cell that holds
// the centre: faces, then edges and vertices.  A particle outside the padded box (the extra bin) gets zero acc and, with
// FRICTION, zero alpha and an empty history row.  Arguments as dem_force_kernel (k_dem.hip)
template <bool POLY, bool FRICTION>
__global__ __launch_bounds__(BLK) void wall_force_kernel(I P, const T* __restrict__ sorted, const T* __restrict__ sorted_w, T R,
                                                        T mass, dfl_sizes sz, T kn, T gn, dfl_friction_law law, dfl_grid3 g,
                                                        const I* __restrict__ order, const I* __restrict__ cell_start,
                                                        const dfl_wall_tri* __restrict__ tri, const I* __restrict__ plane_id,
                                                        dfl_grid3 wg, const I* __restrict__ wstart, const I* __restrict__ wlist,
                                                        T tol, I* __restrict__ dropped, dfl_contact_history hist,
                                                        T* __restrict__ acc, T* __restrict__ alpha) {
    dfl_dem::Particle a;
    a.s = blockIdx.x * BLK + threadIdx.x;
    if (a.s >= P) return;
    a.i = order[a.s];
    a.r = POLY ? sz.sorted_r[a.s] : R;
    dfl_dem::Sink<POLY, FRICTION> sink(a, law, hist, sorted_w, order);
    if (a.s >= cell_start[g.n[0] * g.n[1] * g.n[2]]) {
        sink.finish(a, mass, sz, acc, alpha);  // no contact: 0 / m
        return;
    }
    dfl_dem::load_state<FRICTION>(a, sorted, sorted_w);
    dfl_dem::pair_contacts<POLY>(a, dfl_dem::MeshGrid{g}, sorted, cell_start, kn, gn, sz, sink);
    const int wc = grid_coord(a.p[0], wg.lo[0], wg.inv[0], wg.n[0]) +
                   wg.n[0] * (grid_coord(a.p[1], wg.lo[1], wg.inv[1], wg.n[1]) + wg.n[1] * grid_coord(a.p[2], wg.lo[2], wg.inv[2], wg.n[2]));
    const int wlo = wstart[wc], whi = wstart[wc + 1];
    if (wlo < whi) {
        const int nd = wall_contacts<FRICTION>(a, kn, gn, tol, tri, plane_id, wlist, wlo, whi, sink);
        if (nd) atomicAdd(dropped, nd);
    }
    sink.finish(a, mass, sz, acc, alpha);
}

}  // namespace

extern "C" {

void dfl_walls_build_cells(I P, const T* coord, const T* vel, const T* omega, const T* radius, dfl_grid3 grid, I* cell_of, I* rank,
                           I* count, I* chunk_sum, I* cell_start, I* slot, I* order, T* sorted, T* sorted_w, T* sorted_r,
                           void* stream) {
    if (P <= 0) return;
    wall_bin_kernel<<<ceil_div(P, BLK), BLK, 0, S(stream)>>>(P, coord, grid, cell_of, rank, count);
    DFL_LAUNCH_CHECK();
    const I nbin = grid.n[0] * grid.n[1] * grid.n[2] + 1;
    dfl_dem_sort_binned(P, nbin, coord, vel, omega, radius, cell_of, rank, count, chunk_sum, cell_start, slot, order, sorted,
                        sorted_w, sorted_r, stream);
}

void dfl_walls_forces(I P, const T* sorted, const T* sorted_w, T radius, T mass, dfl_sizes sz, T kn, T gamma_n, dfl_friction_law law,
                      dfl_grid3 grid, const I* order, const I* cell_start, const dfl_wall_tri* tri, const I* plane,
                      dfl_grid3 wall_grid, const I* wall_start, const I* wall_list, T tol, I* dropped, dfl_contact_history hist,
                      T* acc, T* alpha, void* stream) {
    if (P <= 0) return;
    const auto kernel = sz.sorted_r ? (sorted_w ? wall_force_kernel<true, true> : wall_force_kernel<true, false>)
                                    : (sorted_w ? wall_force_kernel<false, true> : wall_force_kernel<false, false>);
    kernel<<<ceil_div(P, BLK), BLK, 0, S(stream)>>>(P, sorted, sorted_w, radius, mass, sz, kn, gamma_n, law, grid, order, cell_start,
                                                  tri, plane, wall_grid, wall_start, wall_list, tol, dropped, hist, acc, alpha);
    DFL_LAUNCH_CHECK();
}

}  // extern "C"
