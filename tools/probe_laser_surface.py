"""Cost of the laser on the level-set surface at bench size (kuhn_cube(119, jitter=0.2), 10M tets) with 100k particles
(dem_particles(100000, 0.004)) under a 26 x 26 column beam along -z, the z- boundary group as substrate, the tilted plane
phi = (x - 1/2) . (0.2, -0.3, 1) / sqrt(1.13) at level 0.03 as the surface.  Device events on the library stream, warm runs:

  update_first_ms / update_ms    ParticleContextLaserSurfaceUpdate on fresh lists (it grows them) and afterwards (median);
                                 both read the facet count back
  laser_step_us per case         the bare ParticleContextLaserStep as the mean of --batch steps, median / min / max over --reps
                                 batches:  no_surface (the launches of the parent commit), surface_no_snapshot (a surface set,
                                 no Update yet), surface (138 k-facet snapshot; the beam hits it)

--root imports the package of another checkout (the parent commit: --cases no_surface), --label names the side.  One JSON
line per run, appended to --out.

    python tools/probe_laser_surface.py --out profiles/laser_surface_M119.json
    python tools/probe_laser_surface.py --root PARENT --label parent --cases no_surface --out profiles/laser_surface_M119.json
"""
import argparse
import json
import os
import sys

import numpy as np

CASES = ("no_surface", "surface_no_snapshot", "surface")
TILT = np.array([0.2, -0.3, 1.0]) / np.sqrt(1.13)
LEVEL, SIDE = 0.03, -1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=119)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    from dedflow_amd import api
    from dedflow_amd.meshgen import dem_particles, kuhn_cube
    m = kuhn_cube(a.M, jitter=0.2)
    N = m.num_node
    x, v, R = dem_particles(100000, 0.004)
    P = api.Problem(m)
    w = np.zeros(6 * N)
    w[4 * N:5 * N] = (m.xg.reshape(-1, 3) - 0.5) @ TILT
    w_d = api.DeviceArray.from_numpy(w)
    tm = api.Timer()
    rec = {"what": "laser_surface", "label": a.label, "M": a.M, "N": N, "T": m.num_tet,
           "reps": a.reps, "batch": a.batch, "warmup": a.warmup, "laser_step_us": {}}
    for case in a.cases.split(","):
        pc = api.Particles(x, v, R, dt=1e-5)
        rec["particles"] = pc.P
        pc.couple(P)
        pc.set_heat(cp_p=500.0, T_init=1500.0)
        pc.set_laser((0.5, 0.5, 2.0), (0.0, 0.0, -1.0), power=400.0, w=0.05, h=2.0 * R, r_cut=0.1, eta_p=0.35, eta_s=0.45,
                     substrate_groups=(4,))
        if case != "no_surface":
            pc.set_laser_surface(LEVEL, SIDE)
        if case == "surface":
            api.sync()
            tm.start(); nf = pc.laser_surface_update(w_d); tm.stop()
            rec["update_first_ms"], rec["facets"] = tm.ms(), nf
            t = []
            for _ in range(a.warmup + a.reps):
                tm.start(); pc.laser_surface_update(w_d); tm.stop()
                t.append(tm.ms())
            t = t[a.warmup:]
            rec.update(update_ms=float(np.median(t)), update_ms_min=min(t), update_ms_max=max(t))
        for _ in range(a.warmup):
            pc.laser_step(1e-5)
        api.sync()
        t = []
        for _ in range(a.reps):
            tm.start()
            for _ in range(a.batch):
                pc.laser_step(1e-5)
            tm.stop()
            t.append(1e3 * tm.ms() / a.batch)
        rec["columns"] = len(pc.laser_columns()[0])
        rec["laser_step_us"][case] = {"median": float(np.median(t)), "min": min(t), "max": max(t), "tally": pc.laser_tally(),
                                      "surface_columns": int((pc.laser_columns()[1] <= -2).sum())}
        pc.close()
    P.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
