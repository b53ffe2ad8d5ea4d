"""Surface mesh at bench size (kuhn_cube(119, jitter=0.2), 10M tets) for three surfaces -- the plane z = 0.5, a sphere of radius
0.3 about the centre, the wavy surface z = 0.5 + 0.1 sin(2 pi x) cos(2 pi y) -- with K = 0, 1 and 8 nodal fields.  Device
events on the library stream, warm, the median of --reps batches of --batch calls:

  evaluation_ms        one DflMeshSurfaceMesh: every launch and the one wait for the counts inside it (per K)
  level_set_volume_ms  one DflMeshLevelSetVolume on the same state in the same process: the project's plain one-pass read of
                       every tet
  facet_pass_ms        the redistancing section's facet pass on the same state with buffers of the probe's own: dfl_redistance_cut
                       with the workgroup and cell counts, both scans, dfl_redistance_emit (the triangle soup and its cell
                       lists; band = 4 cells), the cell counts zeroed between calls
  count_ms, build_ms   the two launchers of an evaluation called by hand on buffers of the probe's own, no wait between them:
                       dfl_surface_mesh_count (bad nodes, classify, the scan's two, counts) and dfl_surface_mesh_build (emit,
                       sort, run heads, the scan's two, vertices, triangles, area, vertex count), with K = 8

The split per kernel comes from running this probe under a kernel trace (profiles/README.md).  One JSON record on stdout and
into --out.

    python tools/probe_surface_mesh.py --M 119 --out profiles/surface_mesh_M119.json
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dedflow_amd import api  # noqa: E402
from dedflow_amd.meshgen import kuhn_cube  # noqa: E402


class Grid(C.Structure):
    _fields_ = [("lo", C.c_double * 3), ("inv_h", C.c_double), ("n", C.c_int32 * 3)]


def scenes(m):
    x = m.xg.reshape(-1, 3)
    yield "plane", 0.5 - x[:, 2]
    yield "sphere", 0.3 - np.linalg.norm(x - 0.5, axis=1)
    yield "wavy", 0.5 + 0.1 * np.sin(2 * np.pi * x[:, 0]) * np.cos(2 * np.pi * x[:, 1]) - x[:, 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=119)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--jitter", type=float, default=0.2)
    ap.add_argument("--fields", default="0,1,8")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = api.lib()
    m = kuhn_cube(a.M, jitter=a.jitter)
    N, T = m.num_node, m.num_tet
    P = api.Problem(m)
    dev = P.mesh.contents.device.contents
    tm = api.Timer()
    rec = {"what": "surface_mesh", "M": a.M, "N": N, "T": T, "reps": a.reps, "batch": a.batch, "warmup": a.warmup, "scenes": {}}

    def median_ms(fn):
        for _ in range(a.warmup):
            fn()
        api.sync()
        t = []
        for _ in range(a.reps):
            tm.start()
            for _ in range(a.batch):
                fn()
            tm.stop()
            t.append(tm.ms() / a.batch)
        return {"median": float(np.median(t)), "min": min(t), "max": max(t)}

    vp, i32, f64, I32 = C.c_void_p, C.c_int32, C.c_double, np.int32
    for name, args in (("dfl_redistance_cut", [i32, vp, vp, vp, i32, f64, C.POINTER(Grid), vp, vp, vp, vp]),
                       ("dfl_scan_counts", [i32, vp, vp, vp, vp]),
                       ("dfl_redistance_emit", [i32, vp, vp, vp, i32, f64, C.POINTER(Grid), vp, vp, vp, vp, i32, vp, i32, vp])):
        getattr(L, name).restype, getattr(L, name).argtypes = None, args
    per = int(L.dfl_tets_per_block())
    nblk = (T + per - 1) // per
    s = L.DflStream()
    prm = api.dfl_surface_mesh_params(0.0, 1.0)
    # the redistancing facet pass: its grid over the mesh with cells of 4 mesh cells
    band = 4.0 / a.M
    x = m.xg.reshape(-1, 3)
    lo, hi = x.min(axis=0), x.max(axis=0)
    n = [int(np.floor((hi[d] - lo[d]) / band)) + 1 for d in range(3)]
    grid = Grid((C.c_double * 3)(*lo), 1.0 / band, (C.c_int32 * 3)(*n))
    ncell = n[0] * n[1] * n[2]
    blk_count, blk_base = api.DeviceArray(nblk, I32), api.DeviceArray(nblk + 1, I32)
    cell_count, cell_start = api.DeviceArray(ncell, I32), api.DeviceArray(ncell + 1, I32)
    r_chunk = api.DeviceArray(int(L.dfl_scan_num_chunks(max(ncell, nblk))), I32)
    r_part = api.DeviceArray(2 * nblk + 2)
    # the surface mesh launchers by hand
    code = api.DeviceArray(T, np.uint8)
    count, start = api.DeviceArray(2 * nblk, I32), api.DeviceArray(2 * nblk + 1, I32)
    chunk = api.DeviceArray(int(L.dfl_scan_num_chunks(2 * nblk)), I32)
    tot = api.DeviceArray(5)
    fields = [api.DeviceArray.from_numpy(1500.0 / (k + 1) + 400.0 * m.xg[k % 3::3]) for k in range(8)]
    fptr = (vp * 8)(*[q.ptr for q in fields])

    for name, phi in scenes(m):
        w = np.zeros(6 * N)
        w[4 * N:5 * N] = phi
        w[5 * N:] = 1500.0 + 400.0 * m.xg[0::3]
        w_d = api.DeviceArray.from_numpy(w)
        P.set_surface_mesh(level=0.0)
        r = {"evaluation_ms": {}}
        for K in (int(v) for v in a.fields.split(",")):
            r["evaluation_ms"][str(K)] = median_ms(lambda: L.DflMeshSurfaceMesh(P.mesh, w_d.ptr, fptr, K))
        res = P.surface_mesh()
        r.update({k: res[k] for k in ("vertices", "triangles", "bad_nodes", "bad_tets", "degenerate_tets", "area")})
        r["launches"] = int(L.DflSurfaceMeshTestLaunches(P.mesh))
        r["level_set_volume_ms"] = median_ms(lambda: L.DflMeshLevelSetVolume(P.mesh, w_d.ptr, 0.0))

        def facet_count():
            cell_count.zero()
            L.dfl_redistance_cut(T, dev.ien, dev.xg, w_d.ptr, N, 0.0, C.byref(grid), blk_count.ptr, cell_count.ptr, r_part.ptr, s)
            L.dfl_scan_counts(nblk, blk_count.ptr, r_chunk.ptr, blk_base.ptr, s)
            L.dfl_scan_counts(ncell, cell_count.ptr, r_chunk.ptr, cell_start.ptr, s)

        facet_count()
        api.sync()
        nf, ne = int(blk_base.numpy()[-1]), int(cell_start.numpy()[-1])
        facets, entries = api.DeviceArray(max(nf, 1) * 9), api.DeviceArray(max(ne, 1), I32)

        def facet_pass():
            facet_count()
            L.dfl_redistance_emit(T, dev.ien, dev.xg, w_d.ptr, N, 0.0, C.byref(grid), blk_base.ptr, cell_start.ptr, cell_count.ptr,
                                  facets.ptr, nf, entries.ptr, ne, s)

        r["facet_pass_ms"] = median_ms(facet_pass)
        r["facets"] = nf
        assert nf == res["triangles"]

        def g_count():
            L.dfl_surface_mesh_count(N, T, dev.ien, dev.xg, w_d.ptr, C.byref(prm), code.ptr, count.ptr, start.ptr, chunk.ptr, tot.ptr, s)

        g_count()
        api.sync()
        nt, nkeys = (int(v) for v in tot.numpy().view(I32)[:2])
        assert nt == res["triangles"]
        r["keys"] = nkeys
        nkb, ntb = (nkeys + per - 1) // per, (nt + per - 1) // per
        key, key_out = api.DeviceArray(nkeys, np.uint64), api.DeviceArray(nkeys, np.uint64)
        tbytes = int(L.dfl_surface_mesh_temp_bytes(N, nkeys))
        temp = api.DeviceArray(tbytes // 8 + 1)
        kcount, kbase = api.DeviceArray(nkb, I32), api.DeviceArray(nkb + 1, I32)
        kchunk = api.DeviceArray(int(L.dfl_scan_num_chunks(nkb)), I32)
        verts, edge, tv, vals = api.DeviceArray(3 * nkeys), api.DeviceArray(2 * nkeys, I32), api.DeviceArray(nkeys), api.DeviceArray(8 * nkeys)
        tris, tri_tet, part = api.DeviceArray(3 * nt, I32), api.DeviceArray(nt, I32), api.DeviceArray(ntb)

        def g_build():
            L.dfl_surface_mesh_build(N, T, dev.ien, dev.xg, w_d.ptr, C.byref(prm), code.ptr, start.ptr, nt, nkeys, key.ptr, key_out.ptr,
                                     nkeys, temp.ptr, tbytes, kcount.ptr, kbase.ptr, kchunk.ptr, fptr, 8, verts.ptr, edge.ptr, tv.ptr,
                                     vals.ptr, tris.ptr, tri_tet.ptr, nt, part.ptr, tot.ptr, s)

        r["count_ms"] = median_ms(g_count)
        g_count()
        r["build_ms"] = median_ms(g_build)
        api.sync()
        assert np.array_equal(tris.numpy().reshape(-1, 3), res["tris"]) and int(tot.numpy().view(I32)[2]) == res["vertices"]
        rec["scenes"][name] = r
        print(json.dumps({name: r}), flush=True)
        for d in (w_d, facets, entries, key, key_out, temp, kcount, kbase, kchunk, verts, edge, tv, vals, tris, tri_tet, part):
            d.free()
    P.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
