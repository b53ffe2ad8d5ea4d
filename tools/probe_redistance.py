"""Level-set redistancing at bench size: the time of one DflMeshRedistance on the M = 119 cube for a tilted plane and a sphere at
band = 4 h, as the median of --reps calls after --warmup, timed with device events.

Three figures per field.  first_call_ms: the call on a fresh configuration, which reads the totals back and grows the facet
and entry lists.  call_ms: the later calls, whose lists are large enough already (they still read the two totals back: the
return value is one of them).  kernels: the same launches issued from here through the library's launchers into buffers of
this script's own, each timed alone and with nothing read back, and their sum -- the cost without the host round trip.  The
script checks that its own sequence gives the bits of the library call.  With the candidate-node count and the mean number of
cell entries per candidate node.  --step-json: a bench.py result line of the same session, copied beside the figures.

    python tools/probe_redistance.py --M 119 --out profiles/redistance_M119.json
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

TILT = np.array([0.2, -0.3, 1.0]) / np.sqrt(1.13)


class Grid(C.Structure):
    _fields_ = [("lo", C.c_double * 3), ("inv_h", C.c_double), ("n", C.c_int32 * 3)]


def median(v):
    return float(np.median(v))


def kernel_path(L, P, m, phi0, level, band, reps, warmup):
    """the launch sequence of host/redistance.c with buffers of this script, every launcher timed alone"""
    N, T = m.num_node, m.num_tet
    x = m.xg.reshape(-1, 3)
    lo, hi = x.min(axis=0), x.max(axis=0)
    n = [int(np.floor((hi[d] - lo[d]) / band)) + 1 for d in range(3)]
    grid = Grid((C.c_double * 3)(*lo), 1.0 / band, (C.c_int32 * 3)(*n))
    ncell = n[0] * n[1] * n[2]
    per = int(L.dfl_tets_per_block())
    nblk = (T + per - 1) // per
    I, F = np.int32, np.float64
    dev = P.mesh.contents.device.contents
    w0 = np.zeros(6 * N)
    w0[4 * N:5 * N] = phi0
    w_src, w = api.DeviceArray.from_numpy(w0), api.DeviceArray(6 * N)
    blk_count, blk_base = api.DeviceArray(nblk, I), api.DeviceArray(nblk + 1, I)
    cell_count, cell_start = api.DeviceArray(ncell, I), api.DeviceArray(ncell + 1, I)
    chunk = api.DeviceArray(int(L.dfl_scan_num_chunks(max(ncell, nblk))), I)
    part, out = api.DeviceArray(2 * max(nblk, int(L.dfl_node_reduce_max_part()))), api.DeviceArray(6)
    ncand, lst, chg = api.DeviceArray(1, I), api.DeviceArray(N, I), api.DeviceArray(N)
    s = L.DflStream()
    vp, i32, f64 = C.c_void_p, C.c_int32, C.c_double
    for name, args in (("dfl_redistance_cut", [i32, vp, vp, vp, i32, f64, C.POINTER(Grid), vp, vp, vp, vp]),
                       ("dfl_scan_counts", [i32, vp, vp, vp, vp]),
                       ("dfl_redistance_emit", [i32, vp, vp, vp, i32, f64, C.POINTER(Grid), vp, vp, vp, vp, i32, vp, i32, vp]),
                       ("dfl_redistance_nodes", [i32, vp, vp, f64, f64, C.POINTER(Grid), vp, vp, vp, i32, vp, vp, vp, vp, vp]),
                       ("dfl_redistance_node_stats", [i32, vp, vp, vp, vp]), ("dfl_redistance_reduce", [i32, vp, vp, vp])):
        getattr(L, name).restype, getattr(L, name).argtypes = None, args

    def count():
        L.dfl_redistance_cut(T, dev.ien, dev.xg, w.ptr, N, level, C.byref(grid), blk_count.ptr, cell_count.ptr, part.ptr, s)
        L.dfl_redistance_reduce(nblk, part.ptr, out.ptr, s)

    def scans():
        L.dfl_scan_counts(nblk, blk_count.ptr, chunk.ptr, blk_base.ptr, s)
        L.dfl_scan_counts(ncell, cell_count.ptr, chunk.ptr, cell_start.ptr, s)

    def reset():
        api._chk(api.hip().hipMemcpy(w.ptr, w_src.ptr, w.nbytes, 3))
        cell_count.upload(np.zeros(ncell, I))
        ncand.upload(np.zeros(1, I))

    reset(); count(); scans(); api.sync()
    nf, ne = int(blk_base.numpy()[-1]), int(cell_start.numpy()[-1])
    facets, entries = api.DeviceArray(max(nf, 1) * 9), api.DeviceArray(max(ne, 1), I)

    def emit():
        L.dfl_redistance_emit(T, dev.ien, dev.xg, w.ptr, N, level, C.byref(grid), blk_base.ptr, cell_start.ptr, cell_count.ptr,
                              facets.ptr, nf, entries.ptr, ne, s)

    def nodes():
        L.dfl_redistance_nodes(N, dev.xg, w.ptr, level, band, C.byref(grid), cell_start.ptr, entries.ptr, facets.ptr, nf, None,
                               ncand.ptr, lst.ptr, chg.ptr, s)

    def after():
        L.dfl_redistance_cut(T, dev.ien, dev.xg, w.ptr, N, level, None, None, None, part.ptr, s)
        L.dfl_redistance_reduce(nblk, part.ptr, C.c_void_p(out.ptr + 16), s)
        L.dfl_redistance_node_stats(N, chg.ptr, part.ptr, C.c_void_p(out.ptr + 32), s)

    steps = (("cut_count", count), ("scans", scans), ("emit_fill", emit), ("node_passes", nodes), ("after_stats", after))
    t = {k: [] for k, _ in steps}
    tm = api.Timer()
    for r in range(warmup + reps):
        reset(); api.sync()
        for k, fn in steps:
            tm.start(); fn(); tm.stop()
            if r >= warmup:
                t[k].append(tm.ms())
    api.sync()
    nc = int(ncand.numpy()[0])
    cs = cell_start.numpy().astype(np.int64)
    # entries of the 27 cells around every candidate node
    cx = [np.clip(np.floor((x[:, d] - lo[d]) / band).astype(np.int64), 0, n[d] - 1) for d in range(3)]
    cnt = np.diff(cs).reshape(n[2], n[1], n[0])
    pad = np.pad(cnt, 1)
    box = sum(pad[1 + dz + cx[2], 1 + dy + cx[1], 1 + dx + cx[0]] for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    rec = {k + "_ms": median(v) for k, v in t.items()}
    rec["sum_ms"] = float(sum(rec.values()))
    rec.update(facets=nf, cell_entries=ne, cells=ncell, candidate_nodes=nc, candidate_nodes_by_host_count=int((box > 0).sum()),
               mean_entries_per_candidate=float(box[box > 0].mean()) if (box > 0).any() else 0.0,
               max_entries_per_candidate=int(box.max()))
    return rec, w.numpy()[4 * N:5 * N]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=119)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--jitter", type=float, default=0.2)
    ap.add_argument("--step-json", default=None, help="a file whose last line is a bench.py result of the same session")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = api.lib()
    m = kuhn_cube(a.M, jitter=a.jitter)
    N, T = m.num_node, m.num_tet
    x = m.xg.reshape(-1, 3)
    band = 4.0 / a.M
    fields = {"plane": (x - 0.5) @ TILT, "sphere": np.sqrt(((x - np.array([0.55, 0.52, 0.46])) ** 2).sum(axis=1)) - 0.3}
    rec = {"what": "redistance", "M": a.M, "N": N, "T": T, "band": band, "reps": a.reps, "warmup": a.warmup, "fields": {}}
    P = api.Problem(m)
    tm = api.Timer()
    ok = True
    for name, phi in fields.items():
        w0 = np.zeros(6 * N)
        w0[4 * N:5 * N] = phi
        w_src, w = api.DeviceArray.from_numpy(w0), api.DeviceArray(6 * N)

        def call():
            api._chk(api.hip().hipMemcpy(w.ptr, w_src.ptr, w.nbytes, 3))
            api.sync()
            tm.start(); nf = P.redistance(w); tm.stop()
            return nf, tm.ms()

        P.set_redistance()                                          # a fresh state: the lists at their first size
        P.set_redistance(0.0, band)
        nf, first = call()
        t = [call()[1] for _ in range(a.warmup + a.reps)][a.warmup:]
        got = w.numpy()[4 * N:5 * N]
        st = P.redistance_stats()
        frec = {"first_call_ms": first, "call_ms": median(t), "call_ms_min": min(t), "call_ms_max": max(t), "stats": st}
        frec["kernels"], own = kernel_path(L, P, m, phi, 0.0, band, a.reps, a.warmup)
        frec["kernel_path_same_bits"] = bool(np.array_equal(own.view(np.uint64), got.view(np.uint64)))
        frec["facets_agree"] = frec["kernels"]["facets"] == nf
        ok = ok and frec["kernel_path_same_bits"] and frec["facets_agree"]
        rec["fields"][name] = frec
    P.close()
    if a.step_json:
        with open(a.step_json) as f:
            lines = [ln for ln in f.read().splitlines() if ln.startswith("{")]
        rec["parent_step"] = json.loads(lines[-1])
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not ok:
        sys.exit("the probe's own launch sequence and the library call disagree")


if __name__ == "__main__":
    main()
