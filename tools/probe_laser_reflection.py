"""Cost of the laser's reflections at bench size (kuhn_cube(119, jitter=0.2), 10M tets) with 100k particles
(dem_particles(100000, 0.004)) under a 26 x 26 column beam along -z: the set-up of tools/probe_laser_surface.py.  Fields: the
tilted plane of that probe (no ray finds a second facet) and a groove under the beam, phi = z - min(0.8, 0.2 + 6 |x - 1/2|)
at level 0 (the beam's cut-off radius 0.1 spans its walls).  Device events on the library stream, warm runs:

  update_ms per case            ParticleContextLaserSurfaceUpdate without and with the reflection list R (median of --reps)
  laser_step_us per case        the bare ParticleContextLaserStep as the mean of --batch steps, median / min / max over --reps
                                batches: surface (a snapshot, no reflection set: the launches of the parent commit) and
                                reflect_1 / reflect_4 / reflect_8 (max_bounce, model 1, eps 0.25)
  reflect_8_g16 / _g64          the same with 16 / 64 lanes per ray (DFL_LASER_REFLECT_GROUP); reflect_1_onecell: a grid of one
                                cell (DFL_LASER_REFLECT_CELLS=1), every ray against all of R
  facets, R, rays               candidate facets, facets of R, rays per bounce and the reflection tally of the last step;
                                cells and cell entries of the grid, mean / max entries tested per ray over all its bounces

--root imports the package of another checkout (the parent commit: --cases surface), --label names the side.  One JSON line
per run, appended to --out.

    python tools/probe_laser_reflection.py --out profiles/laser_reflection_M119.json
    python tools/probe_laser_reflection.py --root PARENT --label parent --cases surface --out profiles/laser_reflection_M119.json
"""
import argparse
import json
import os
import sys

import numpy as np

CASES = ("surface", "reflect_1", "reflect_4", "reflect_8", "reflect_8_g64", "reflect_8_g16", "reflect_1_onecell")
TILT = np.array([0.2, -0.3, 1.0]) / np.sqrt(1.13)
FIELDS = {
    "plane": (lambda x: (x - 0.5) @ TILT, 0.03),
    "groove": (lambda x: x[:, 2] - np.minimum(0.8, 0.2 + 6.0 * np.abs(x[:, 0] - 0.5)), 0.0),
}
SIDE = -1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=119)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--fields", default=",".join(FIELDS))
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
    tm = api.Timer()
    rec = {"what": "laser_reflection", "label": a.label, "M": a.M, "N": N, "T": m.num_tet, "reps": a.reps, "batch": a.batch,
           "warmup": a.warmup, "fields": {}}
    for field in a.fields.split(","):
        phi, level = FIELDS[field]
        w = np.zeros(6 * N)
        w[4 * N:5 * N] = phi(m.xg.reshape(-1, 3))
        w_d = api.DeviceArray.from_numpy(w)
        out = rec["fields"][field] = {"laser_step_us": {}, "update_ms": {}}
        for case in a.cases.split(","):
            pc = api.Particles(x, v, R, dt=1e-5)
            pc.couple(P)
            pc.set_heat(cp_p=500.0, T_init=1500.0)
            pc.set_laser((0.5, 0.5, 2.0), (0.0, 0.0, -1.0), power=400.0, w=0.05, h=2.0 * R, r_cut=0.1, eta_p=0.35, eta_s=0.45,
                         substrate_groups=(4,))
            pc.set_laser_surface(level, SIDE)
            if case != "surface":
                # _g16 / _g64: lanes per ray (DFL_LASER_REFLECT_GROUP); _onecell: a grid of one cell, every ray tests all of R
                for k in ("DFL_LASER_REFLECT_GROUP", "DFL_LASER_REFLECT_CELLS"):
                    os.environ.pop(k, None)
                if "_g" in case:
                    os.environ["DFL_LASER_REFLECT_GROUP"] = case.split("_g")[1]
                if case.endswith("_onecell"):
                    os.environ["DFL_LASER_REFLECT_CELLS"] = "1"
                pc.set_laser_reflection(int(case.split("_")[1]), 1, 0.25)
            t = []
            for _ in range(a.warmup + a.reps):
                tm.start(); nf = pc.laser_surface_update(w_d); tm.stop()
                t.append(tm.ms())
            t = t[a.warmup:]
            out["update_ms"][case] = {"median": float(np.median(t)), "min": min(t), "max": max(t)}
            out["facets"] = nf
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
            r = {"median": float(np.median(t)), "min": min(t), "max": max(t), "tally": pc.laser_tally(),
                 "surface_columns": int((pc.laser_columns()[1] <= -2).sum())}
            if case != "surface":
                rt = pc.laser_reflection_tally()
                out["R"] = int(pc.laser_reflection_facets()[1].size)
                r.update(rays=rt["rays"].tolist(), absorbed=rt["absorbed"].tolist(), escaped=rt["escaped"], remaining=rt["remaining"],
                         )
                import ctypes as C
                ent, cells, mean, mx = C.c_int32(0), C.c_int32(0), C.c_double(0), C.c_double(0)
                api.lib().DflLaserReflectionGridStats(pc.ctx, C.byref(ent), C.byref(cells), C.byref(mean), C.byref(mx))
                r.update(cell_entries=ent.value, cells=cells.value, entries_tested_per_ray_mean=mean.value,
                         entries_tested_per_ray_max=mx.value)
            out["laser_step_us"][case] = r
            rec["columns"] = len(pc.laser_columns()[0])
            pc.close()
    P.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
