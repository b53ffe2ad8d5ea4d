"""Contact friction at 100k particles: the friction force kernels against the frictionless ones, on the unit box and with
the boundary faces of config 4's mesh (kuhn_cube(55, jitter=0.2)) as walls.  --state dilute: dem_particles(100000, 0.004)
(BASELINE config 4's particles, about 0.1 contacts per particle); --state dense: a simple-cubic lattice at spacing 1.9 R
(R = 0.0114, 97,336 particles, 6 pair contacts per interior particle) with random velocities and spins.  Each variant runs
--reps contact sweeps after --warmup, timed per force launch with device events (DflProfile tag of host/particle.c and
host/walls.c); the kernel names of a rocprofv3 --kernel-trace run separate box / walls and frictionless / friction.
Prints one JSON line (and writes it to --out).

  python tools/probe_friction.py --state dense [--reps 50] [--warmup 5] [--out profiles/probe_friction_dense.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dedflow_amd import api  # noqa: E402
from dedflow_amd.meshgen import dem_lattice, dem_particles, kuhn_cube  # noqa: E402

TAG_DEM_FORCE = 9   # DFL_TAG_SMALL + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--state", choices=("dilute", "dense"), default="dense")
    ap.add_argument("--M", type=int, default=55)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L = api.lib()
    rng = np.random.default_rng(3)
    if a.state == "dilute":
        x, v, R = dem_particles(100000, 0.004)
        x, v = x.reshape(-1, 3), v.reshape(-1, 3)
    else:
        R = 0.0114
        x = dem_lattice((0, 0, 0), (1, 1, 1), R, jitter=0.05)
        v = rng.normal(scale=0.1, size=x.shape)
    w = rng.normal(scale=5.0, size=x.shape)
    P = api.Problem(kuhn_cube(a.M, jitter=0.2))
    out = {"state": a.state, "particles": len(x), "R": R, "M": a.M}
    for walls in (False, True):
        for friction in (False, True):
            pc = api.Particles(x.reshape(-1), v.reshape(-1), R)
            if walls:
                pc.set_walls(P)
            if friction:
                pc.set_friction(0.5)
                pc.set_omega(w)
            for _ in range(a.warmup):
                pc.compute_forces()
            api.sync()
            L.DflProfileEnable(1)
            for _ in range(a.reps):
                pc.compute_forces()
            api.sync()
            tot, mn = C.c_double(0), C.c_double(0)
            n = L.DflProfileCollect(TAG_DEM_FORCE, C.byref(tot), C.byref(mn))
            L.DflProfileEnable(0)
            key = ("walls" if walls else "box") + ("_friction" if friction else "")
            out[key] = {"force_mean_us": 1e3 * tot.value / max(n, 1), "force_min_us": 1e3 * mn.value, "n": n,
                        "overflow": pc.friction_overflow_count(), "dropped": pc.wall_dropped_count()}
            pc.close()
    P.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
