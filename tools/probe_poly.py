"""Polydisperse particles at 100k: the POLY force kernels against the monodisperse ones, on the unit box and with the
boundary faces of config 4's mesh (kuhn_cube(55, jitter=0.2)) as walls, friction off and on, for three variants:
  mono   the monodisperse context (radius R = 0.004, dem_particles(100000, R): BASELINE config 4's particles)
  equal  the same context after set_sizes(full(P, R)): the POLY kernels on equal radii (bitwise the same results)
  half   radii uniform in [R/2, R] (default masses)
Each case runs --reps contact sweeps after --warmup.  force_us = the force launch (device events, the DflProfile tag of
host/particle.c and host/walls.c); sweep_us = the whole ParticleContextComputeForces (bin, scan, place, sort, force) between
two events.  Run it under `rocprofv3 --kernel-trace --stats` for per-kernel times: the template argument in the kernel
names separates <false> (monodisperse) from <true> (POLY).  Prints one JSON line (and writes it to --out).

  python tools/probe_poly.py [--reps 50] [--warmup 5] [--out profiles/r09_probe_poly.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dedflow_amd import api  # noqa: E402
from dedflow_amd.meshgen import dem_particles, kuhn_cube  # noqa: E402

TAG_DEM_FORCE = 9   # DFL_TAG_SMALL + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=55)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L = api.lib()
    x, v, R = dem_particles(100000, 0.004)
    rng = np.random.default_rng(3)
    w = rng.normal(scale=5.0, size=x.size)
    half = rng.uniform(0.5 * R, R, size=x.size // 3)
    P = api.Problem(kuhn_cube(a.M, jitter=0.2))
    out = {"particles": x.size // 3, "R": R, "M": a.M, "reps": a.reps}
    for walls in (False, True):
        for friction in (False, True):
            for variant in ("mono", "equal", "half"):
                pc = api.Particles(x, v, R)
                if variant == "equal":
                    pc.set_sizes(np.full(pc.P, R))
                elif variant == "half":
                    pc.set_sizes(half)
                if walls:
                    pc.set_walls(P)
                if friction:
                    pc.set_friction(0.5)
                    pc.set_omega(w)
                for _ in range(a.warmup):
                    pc.compute_forces()
                api.sync()
                L.DflProfileEnable(1)
                t = api.Timer()
                t.start()
                for _ in range(a.reps):
                    pc.compute_forces()
                t.stop()
                sweep_ms = t.ms()
                tot, mn = C.c_double(0), C.c_double(0)
                n = L.DflProfileCollect(TAG_DEM_FORCE, C.byref(tot), C.byref(mn))
                L.DflProfileEnable(0)
                key = ("walls" if walls else "box") + ("_friction" if friction else "") + "_" + variant
                out[key] = {"force_mean_us": 1e3 * tot.value / max(n, 1), "force_min_us": 1e3 * mn.value,
                            "sweep_mean_us": 1e3 * sweep_ms / a.reps, "n": n,
                            "overflow": pc.friction_overflow_count(), "dropped": pc.wall_dropped_count()}
                pc.close()
            for what in ("force_mean_us", "sweep_mean_us"):
                k = ("walls" if walls else "box") + ("_friction" if friction else "")
                out[k + "_ratio_equal_" + what.split("_")[0]] = out[k + "_equal"][what] / out[k + "_mono"][what]
    P.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
