"""Cost of the melt-pool capture at 1M tets (kuhn_cube(55, jitter=0.2)) and 100k particles (dem_particles(100000, 0.004)),
between two device events.  Two kinds of record, one JSON line each (appended to --out):

  substep   the coupled sub-step plus ParticleContextRemove (an outflow plane that removes nothing), mean of --reps after
            --warmup: what a context pays per sub-step.  With --capture-set the context also has capture set (it is not
            called by the sub-step: the cost must not change).  Runs on the parent commit too (--root, without --capture-set).
  call      ONE ParticleContextRemove or ParticleContextCapture that takes out none, about 5 % or all of the particles (the
            particles below a z quantile: the plane z < z_q for Remove, phi = z - 0.5 < level for capture, hot everywhere),
            on a fresh context after three coupled sub-steps (impulses pending), mean and min of --calls contexts.  Remove
            is the yardstick: a capture is a Remove plus one gather kernel, one sort and one node pass.

Run it under `rocprofv3 --kernel-trace --stats` for the per-kernel times; --kernel-stats turns the CSV of such a run into
records of the same file.  --root imports the package of another checkout, --label names the side in the records.

  python tools/probe_capture.py [--reps 50] [--warmup 5] [--calls 5] [--kinds substep,remove,capture] [--capture-set]
                                [--root DIR] [--label this] [--out profiles/capture_M55.jsonl]
  python tools/probe_capture.py --kernel-stats DIR/..._kernel_stats.csv --label this_rocprofv3 --out profiles/capture_M55.jsonl
"""
import argparse
import json
import os
import re
import sys

import numpy as np

FRACTIONS = {"none": 0.0, "5pct": 0.05, "all": 1.0}


def kernel_stats(path, label, out):
    """the particle kernels of a rocprofv3 --kernel-trace --stats CSV as one record each"""
    import csv
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row["Name"]
            if not any(k in name for k in ("dem_", "couple_", "heat_", "wall_", "flow_", "capture_", "scan")):
                continue
            short = re.sub(r"\(anonymous namespace\)::|^void ", "", name)
            short = short[:short.index(">(") + 1] if ">(" in short else short.split("(")[0]
            rec = {"label": label, "kernel": short, "calls": int(row["Calls"]),
                   "mean_us": float(row["AverageNs"]) / 1e3, "min_us": float(row["MinNs"]) / 1e3,
                   "max_us": float(row["MaxNs"]) / 1e3}
            emit(rec, out)


def emit(rec, out):
    print(json.dumps(rec))
    if out:
        with open(out, "a") as g:
            g.write(json.dumps(rec) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=55)
    ap.add_argument("--particles", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--kinds", default="substep,remove,capture")
    ap.add_argument("--capture-set", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="this")
    ap.add_argument("--kernel-stats", default="")
    a = ap.parse_args()
    if a.kernel_stats:
        kernel_stats(a.kernel_stats, a.label, a.out)
        return
    sys.path.insert(0, a.root)
    from dedflow_amd import api
    from dedflow_amd.meshgen import dem_particles, kuhn_cube, synthetic_fields
    m = kuhn_cube(a.M, jitter=0.2)
    N = m.num_node
    wg, _ = synthetic_fields(m)
    wg[4 * N:5 * N] = m.xg.reshape(-1, 3)[:, 2] - 0.5
    wg[5 * N:] = 2000.0
    x, v, R = dem_particles(a.particles, 0.004)
    z = np.sort(x.reshape(-1, 3)[:, 2])
    P = api.Problem(m)
    w_d = api.DeviceArray.from_numpy(wg)
    base = {"label": a.label, "M": a.M, "tets": m.num_tet}
    kinds = a.kinds.split(",")
    if "substep" in kinds:
        pc = api.Particles(x, v, R, dt=1e-5)
        pc.couple(P)
        pc.set_outflow(planes=[(0.0, 0.0, 1.0, 10.0)])
        if a.capture_set:
            pc.set_capture(level=0.0, side=-1, reach=0.0, T_melt=np.inf)
        for _ in range(a.warmup):
            pc.fluid_step(w_d)
            pc.remove()
        api.sync()
        t = api.Timer()
        t.start()
        for _ in range(a.reps):
            pc.fluid_step(w_d)
            pc.remove()
        t.stop()
        emit(dict(base, kind="substep", capture_set=bool(a.capture_set), particles=pc.P, reps=a.reps,
                  substep_remove_us=1e3 * t.ms() / a.reps), a.out)
        pc.close()
    for kind in ("remove", "capture"):
        if kind not in kinds:
            continue
        for name, frac in FRACTIONS.items():
            zq = -1.0 if frac == 0.0 else (2.0 if frac == 1.0 else float(z[int(frac * len(z))]))
            times, taken = [], 0
            for _ in range(a.calls):
                pc = api.Particles(x, v, R, dt=1e-5)
                pc.couple(P)
                if kind == "remove":
                    pc.set_outflow(planes=[(0.0, 0.0, -1.0, -zq)])
                else:
                    pc.set_capture(level=zq - 0.5, side=-1, reach=0.0, T_melt=-np.inf)
                for _ in range(3):
                    pc.fluid_step(w_d)
                api.sync()
                n0 = pc.P
                t = api.Timer()
                t.start()
                if kind == "remove":
                    pc.remove()
                else:
                    pc.capture(w_d)
                t.stop()
                times.append(1e3 * t.ms())
                taken = n0 - pc.P
                pc.close()
            emit(dict(base, kind="call", call=kind, fraction=name, particles=n0, taken=taken, calls=a.calls,
                      mean_us=float(np.mean(times)), min_us=float(np.min(times)), max_us=float(np.max(times))), a.out)
    P.close()


if __name__ == "__main__":
    main()
