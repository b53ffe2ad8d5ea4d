"""Porosity record at bench size (kuhn_cube(119, jitter=0.2), 10M tets): a plane substrate surface z = 0.8 with gas above, open
through the group z+, and 0 / 8 / 512 spherical pores of a few tets' diameter below it.  Device events on the library stream,
warm, the median of --reps batches of --batch calls:

  evaluation_ms        one DflMeshPorosity: every launch and the one wait for the counts inside it
  level_set_volume_ms  one DflMeshLevelSetVolume on the same state in the same process: the project's plain one-pass read of
                       every tet (dfl_volume_classify), the yardstick of the volume correction and the track sections
  label_ms .. pores_ms the four launchers of an evaluation called by hand on buffers of the probe's own, no wait between them:
                       dfl_porosity_label (init, classify, hook, flatten, mark open), dfl_porosity_rank, dfl_porosity_tets,
                       dfl_porosity_pores
  label_no_tets_ms     dfl_porosity_label with T = 0: the same launches without the hook's work and with an identity flatten;
                       label_ms - label_no_tets_ms is the hook pass with the walks it leaves to the flatten pass

One JSON record on stdout and into --out.

    python tools/probe_porosity.py --M 119 --out profiles/porosity_M119.json
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

Z_PLUS = 1 << 5


def scene(m, npores, z0=0.8):
    """phi: metal below z0, gas above and inside npores balls of radius 2.5 cells on a cubic grid below the surface"""
    x = m.xg.reshape(-1, 3)
    phi = z0 - x[:, 2]
    k = round(npores ** (1.0 / 3.0)) if npores else 0
    r = 2.5 / m.M
    for c in np.ndindex(k, k, k):
        ctr = np.array([0.1 + 0.8 * (c[0] + 0.5) / k, 0.1 + 0.8 * (c[1] + 0.5) / k, 0.1 + 0.6 * (c[2] + 0.5) / k])
        near = np.flatnonzero(np.all(np.abs(x - ctr) <= r, axis=1))
        phi[near] = np.minimum(phi[near], np.linalg.norm(x[near] - ctr, axis=1) - r)
    return phi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=119)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--jitter", type=float, default=0.2)
    ap.add_argument("--pores", default="0,8,512")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = api.lib()
    m = kuhn_cube(a.M, jitter=a.jitter)
    N, T = m.num_node, m.num_tet
    P = api.Problem(m)
    dev = P.mesh.contents.device.contents
    tm = api.Timer()
    rec = {"what": "porosity", "M": a.M, "N": N, "T": T, "reps": a.reps, "batch": a.batch, "warmup": a.warmup, "scenes": {}}

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

    # the probe's own buffers for the launchers called by hand
    per = int(L.dfl_tets_per_block())
    nbn, nbt = (N + per - 1) // per, (T + per - 1) // per
    prm = api.dfl_porosity_params(0.0, 1.0, 1024)
    I32 = np.int32
    parent, label, opened, rank, pore = (api.DeviceArray(N, I32) for _ in range(5))
    ncount, nbase, tcount, tbase = (api.DeviceArray(n, I32) for n in (nbn, nbn + 1, nbt, nbt + 1))
    chunk = api.DeviceArray(int(L.dfl_scan_num_chunks(max(nbn, nbt))), I32)
    part, tot, rows = api.DeviceArray(3 * nbt), api.DeviceArray(7), api.DeviceArray(12 * 1024)
    off = m.bound_elem_offset
    oface = api.DeviceArray.from_numpy(np.arange(off[5], off[6], dtype=I32))
    f2e, forn = P.mesh.contents.bound_f2e, P.mesh.contents.bound_forn
    s = L.DflStream()                                                      # the library's stream

    for npores in (int(v) for v in a.pores.split(",")):
        w = np.zeros(6 * N)
        w[4 * N:5 * N] = scene(m, npores)
        w[5 * N:] = 1500.0 + 400.0 * m.xg[0::3]
        w_d = api.DeviceArray.from_numpy(w)
        P.set_porosity(level=0.0, open_groups=Z_PLUS, max_pores=1024)
        r = {"evaluation_ms": median_ms(lambda: L.DflMeshPorosity(P.mesh, w_d.ptr)),
             "level_set_volume_ms": median_ms(lambda: L.DflMeshLevelSetVolume(P.mesh, w_d.ptr, 0.0))}
        res = P.porosity()
        r.update({k: res[k] for k in ("components", "pores", "listed", "volume_metal", "volume_open", "volume_pores", "porosity")})
        r["launches"] = int(L.DflPorosityTestLaunches(P.mesh))
        closed = int(sum(p["tets"] for p in res["list"]))
        r["closed_tets"] = closed
        cap = max(closed, 1024)
        key, key_out, vals = api.DeviceArray(cap), api.DeviceArray(cap), api.DeviceArray(2 * cap)
        tbytes = int(L.dfl_porosity_temp_bytes(cap))
        temp = api.DeviceArray(tbytes // 8 + 1)

        def g_label(nt=T):
            L.dfl_porosity_label(N, nt, dev.ien, w_d.ptr, C.byref(prm), oface.n, oface.ptr, f2e, forn, parent.ptr, label.ptr,
                                 opened.ptr, rows.ptr, tot.ptr, s)

        def g_rank():
            L.dfl_porosity_rank(N, dev.xg, C.byref(prm), label.ptr, opened.ptr, ncount.ptr, nbase.ptr, chunk.ptr, rank.ptr, pore.ptr,
                                rows.ptr, tot.ptr, s)

        def g_tets():
            L.dfl_porosity_tets(T, dev.ien, dev.xg, w_d.ptr, N, C.byref(prm), label.ptr, opened.ptr, nbn, nbase.ptr, tcount.ptr,
                                tbase.ptr, chunk.ptr, part.ptr, tot.ptr, s)

        def g_pores():
            L.dfl_porosity_pores(T, dev.ien, dev.xg, w_d.ptr, N, C.byref(prm), label.ptr, opened.ptr, pore.ptr, tbase.ptr, closed,
                                 key.ptr, key_out.ptr, cap, vals.ptr, temp.ptr, tbytes, rows.ptr, s)

        r["label_no_tets_ms"] = median_ms(lambda: g_label(0))
        r["label_ms"] = median_ms(g_label)
        r["rank_ms"] = median_ms(g_rank)
        r["tets_ms"] = median_ms(g_tets)
        r["pores_ms"] = median_ms(g_pores)
        api.sync()
        assert np.array_equal(label.numpy(), res["label"]) and np.array_equal(pore.numpy(), res["pore"])
        rec["scenes"][str(npores)] = r
        print(json.dumps({str(npores): r}), flush=True)
        for d in (w_d, key, key_out, vals, temp):
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
