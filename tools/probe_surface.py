"""Free-surface forces at bench size: the time of one DflMeshSurfaceLoad (all terms on, planar surface z = 0.5, eps = 2h on
the bench mesh) against one AssembleSystem(F) of the same problem, the two alternated call by call in one job and timed
with device events; with the one-byte-per-tet band pass in front (the default) and the node pass alone (DFL_SURFACE_FLAGS=0),
whose outputs must be the same bits.  One JSON record on stdout and into --out.

    python tools/probe_surface.py --M 119 --out profiles/surface_forces_M119.json
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/probe_surface.py --M 119 --trace-only   (kernel means, own run)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dedflow_amd import api  # noqa: E402
from dedflow_amd.meshgen import kuhn_cube, synthetic_fields  # noqa: E402

CFG = dict(level=0.0, side=-1, sigma0=1.8, dsigma_dT=-4e-4, T_ref=1900.0, recoil_p0=1.0e5, recoil_a=11.0, T_boil=3100.0,
           h_conv=80.0, emissivity=0.4, T_amb=300.0, evap_q0=2.0e9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=119)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--jitter", type=float, default=0.2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-only", action="store_true", help="no timing: warm-up + reps calls of each kind for a kernel trace")
    a = ap.parse_args()
    L = api.lib()
    m = kuhn_cube(a.M, jitter=a.jitter)
    N, T = m.num_node, m.num_tet
    x = m.xg.reshape(-1, 3)
    wg, dwg = synthetic_fields(m)
    wg[4 * N:5 * N] = x[:, 2] - 0.5
    wg[5 * N:] = 2500.0 + 1000.0 * np.sin(3.0 * x[:, 0] + 2.0 * x[:, 1] + 0.3)
    P = api.Problem(m)
    wg_d, dwg_d, F_d = api.DeviceArray.from_numpy(wg), api.DeviceArray.from_numpy(dwg), api.DeviceArray(6 * N)
    out = [api.DeviceArray(3 * N), api.DeviceArray(N), api.DeviceArray(N)]

    def surface():
        L.DflMeshSurfaceLoad(P.mesh, wg_d.ptr, out[0].ptr, out[1].ptr, out[2].ptr)

    def assemble():
        P.assemble_system(wg_d, dwg_d, F_d)

    rec = {"what": "surface_forces", "M": a.M, "N": N, "T": T, "node_tet_pairs": 4 * T, "eps_over_h": 2.0, "reps": a.reps}
    tm = api.Timer()
    results = {}
    for mode in ("node_pass", "flag_pass"):
        os.environ["DFL_SURFACE_FLAGS"] = "1" if mode == "flag_pass" else "0"
        P.set_surface_forces(eps=2.0 / a.M, **CFG)
        for _ in range(a.warmup):
            surface()
            assemble()
        api.sync()
        ts, ta = [], []
        for _ in range(a.reps):
            if a.trace_only:
                surface()
                assemble()
                continue
            tm.start(); surface(); tm.stop(); ts.append(tm.ms())
            tm.start(); assemble(); tm.stop(); ta.append(tm.ms())
        api.sync()
        results[mode] = [o.numpy() for o in out]
        if not a.trace_only:
            rec[mode] = {"surface_load_ms_mean": float(np.mean(ts)), "surface_load_ms_min": min(ts), "surface_load_ms_max": max(ts),
                         "assemble_F_ms_mean": float(np.mean(ta)), "assemble_F_ms_min": min(ta), "assemble_F_ms_max": max(ta)}
    same = all(np.array_equal(p.view(np.uint64), q.view(np.uint64)) for p, q in zip(results["node_pass"], results["flag_pass"]))
    area = results["node_pass"][2]
    rec.update({"flag_pass_same_bits": bool(same), "area": float(area.sum()), "band_nodes": int((area != 0).sum()),
                "finite": bool(all(np.isfinite(r).all() for r in results["node_pass"]))})
    # bytes from HBM at the least: V2E (4 B x (N + 1 + 4T)), the outputs (40 B x N); ien (16 B x T), phi and coordinates (32 B x N)
    # once each when L2 serves the repeats; the flag pass adds T bytes written and read back
    rec["hbm_floor_bytes"] = 4 * (N + 1 + 4 * T) + 40 * N + 16 * T + 32 * N
    P.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not same:
        sys.exit("the flag pass changed the results")


if __name__ == "__main__":
    main()
