"""Times the step-limit kernels (dfl_step_limits: csrc/k_steplimit.hip) and, in the same process, one plain volume evaluation
(dfl_volume_classify, the classify pass of the level-set volume correction: a comparable read over ien with node gathers) on a
Kuhn cube, with hipEvents over `reps` launches after a warm-up.  Prints one JSON line.

    python tools/bench_steplimit.py [--M 119] [--reps 20]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=119, help="cells per cube edge (119 -> 10.1M tets)")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    from dedflow_amd import api
    from dedflow_amd.meshgen import kuhn_cube
    L = api.lib()
    m = kuhn_cube(args.M, jitter=0.2)
    N, T = m.num_node, m.num_tet
    x = m.xg.reshape(-1, 3)
    rng = np.random.default_rng(1)
    w = np.zeros(6 * N)
    w[:3 * N] = rng.standard_normal(3 * N)
    w[4 * N:5 * N] = (x - 0.5) @ np.array([0.3, 0.1, -1.0]) / np.sqrt(1.1)
    w[5 * N:] = 1650.0 + 120.0 * ((x - 0.5) @ np.array([0.2, -0.3, 1.0]))
    P = api.Problem(m, color=False)
    dev = P.mesh.contents.device.contents
    ien, xg = C.cast(dev.ien, C.c_void_p), C.cast(dev.xg, C.c_void_p)
    w_d = api.DeviceArray.from_numpy(w)
    vp, i32, f64 = C.c_void_p, C.c_int32, C.c_double
    L.dfl_tets_per_block.restype, L.dfl_tets_per_block.argtypes = i32, []
    L.dfl_volume_classify.restype = None
    L.dfl_volume_classify.argtypes = [i32, vp, vp, vp, i32, f64, f64, f64, vp, vp, vp, vp]
    grid = L.dfl_step_limit_grid(T, 0)
    pv, pi = api.DeviceArray(3 * grid + 3), api.DeviceArray(5 * grid + 5, np.int32)
    ov, oi = api.DeviceArray(3), api.DeviceArray(5, np.int32)
    prm = api.dfl_step_limit_params(0.0, 1.8, -4.0e-4, 1650.0)
    nblk = (T + L.dfl_tets_per_block() - 1) // L.dfl_tets_per_block()
    cnt, part, out5 = api.DeviceArray(nblk, np.int32), api.DeviceArray(5 * nblk), api.DeviceArray(5)
    s = L.DflStream()
    calls = {"step_limits": lambda: L.dfl_step_limits(T, ien, xg, w_d.ptr, N, prm, 0, pv.ptr, pi.ptr, ov.ptr, oi.ptr, s),
             "volume_classify": lambda: L.dfl_volume_classify(T, ien, xg, w_d.ptr, N, 0.0, -0.05, 0.05, cnt.ptr, part.ptr, out5.ptr, s)}
    out = {"M": args.M, "nodes": int(N), "tets": int(T), "reps": args.reps, "step_limit_grid": int(grid)}
    tm = api.Timer()
    for rnd in range(2):                       # two rounds, alternating, so that neither call always runs first
        for name, fn in calls.items():
            for _ in range(3):
                fn()
            tm.start()
            for _ in range(args.reps):
                fn()
            tm.stop()
            out.setdefault(name + "_ms", []).append(round(tm.ms() / args.reps, 5))
    api.sync()
    out["limits"] = P.time_step_limits(w_d)
    out["ratio"] = round(min(out["step_limits_ms"]) / min(out["volume_classify_ms"]), 3)
    P.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
