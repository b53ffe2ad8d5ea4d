"""Cost of the solid-surface contact at the coupling probe's size: kuhn_cube(55, jitter=0.2) (998,250 tets) with 100k
particles of R = 0.004, a tenth of them in one layer within R of the solid plane z = 1/2 (phi = z - 1/2, metal below, cold
everywhere), the rest on a lattice in the gas above.  kn = 1, gamma_n = 0 and dt = 1e-9 keep the particles where they are,
so every sub-step of every variant does the same work.

Times ParticleContextFluidStep (device events around `reps` sub-steps, `rounds` times, the variants alternating inside a
round) with the contact never set, set, and set with the bound behind the kernel's early exit zeroed (every located
particle then gathers T and the coordinates; DflSurfaceContactTestNoEarlyExit, a hook for this probe), then, in a pass of
its own with the library's profile tags on, the contact, locate and drag kernels.  Run
from a checkout without the feature (the parent commit) it times the first variant only: that is the parent's figure, and
repeated runs of it give the run-to-run spread.  Prints one JSON line (and writes it to --out).

  python tools/probe_surface_contact.py [--reps 200] [--rounds 5] [--out profiles/surface_contact_M55.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dedflow_amd import api  # noqa: E402
from dedflow_amd.meshgen import kuhn_cube  # noqa: E402

TAG_LOCATE, TAG_DRAG, TAG_CONTACT = 10, 11, 14   # DFL_TAG_SMALL + 2, + 3, + 6


def collect(L, tag):
    tot, mn = C.c_double(0), C.c_double(0)
    n = L.DflProfileCollect(tag, C.byref(tot), C.byref(mn))
    return {"n": n, "mean_us": 1e3 * tot.value / max(n, 1), "min_us": 1e3 * mn.value}


def powder(P, R, seed=4):
    """P / 10 particles in one layer within R of z = 1/2, the others on a lattice above it; no two overlap"""
    rng = np.random.default_rng(seed)
    n_layer = P // 10
    side = int(np.ceil(np.sqrt(n_layer)))
    g = (np.arange(side) + 0.5) / side
    xy = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)[:n_layer]
    layer = np.c_[xy, 0.5 + rng.uniform(-0.9 * R, 0.9 * R, n_layer)]
    rest = P - n_layer
    nz = int(np.ceil(rest / (side * side)))
    z = 0.5 + 3 * R + (0.5 - 4 * R) * (np.arange(nz) + 0.5) / nz
    lat = np.stack(np.meshgrid(g, g, z, indexing="ij"), axis=-1).reshape(-1, 3)[:rest]
    x = np.vstack([layer, lat])
    assert 1.0 / side > 2 * R and (0.5 - 4 * R) / nz > 2 * R
    return np.ascontiguousarray(x[rng.permutation(P)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=55)
    ap.add_argument("--particles", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L = api.lib()
    m = kuhn_cube(a.M, jitter=0.2)
    N = m.num_node
    R = 0.004
    x = powder(a.particles, R)
    w = np.zeros(6 * N)
    w[4 * N:5 * N] = m.xg.reshape(-1, 3)[:, 2] - 0.5
    w[5 * N:] = 300.0
    P = api.Problem(m, maxit=120, atol=1e-12, rtol=1e-4)
    w_d = api.DeviceArray.from_numpy(w)
    have = hasattr(api.Particles, "set_surface_contact")
    out = {"M": a.M, "tets": m.num_tet, "particles": a.particles, "R": R, "reps": a.reps, "feature": have,
           "within_R": int((np.abs(x[:, 2] - 0.5) < R).sum())}
    variants = ["off"] + (["on", "on_no_early_exit"] if have else [])
    ctx = {}
    for key in variants:
        pc = api.Particles(x.reshape(-1), np.zeros(3 * a.particles), R, mass=2000.0 * 4.0 / 3.0 * np.pi * R ** 3, kn=1.0, gamma_n=0.0,
                           dt=1e-9)
        pc.couple(P)
        if key != "off":
            pc.set_surface_contact(level=0.0, side=-1, T_solid=1500.0)
            if key == "on_no_early_exit":
                pc._surface_contact_no_early_exit()
        for _ in range(5):                       # warm-up of every launch shape
            pc.fluid_step(w_d)
        ctx[key] = pc
        out[key] = {"fluid_substep_us": []}
    api.sync()
    t = api.Timer()
    for _ in range(a.rounds):
        for key in variants:
            t.start()
            for _ in range(a.reps):
                ctx[key].fluid_step(w_d)
            t.stop()
            out[key]["fluid_substep_us"].append(1e3 * t.ms() / a.reps)
    for key in variants:
        pc = ctx[key]
        L.DflProfileEnable(1)
        for _ in range(a.reps):
            pc.fluid_step(w_d)
        out[key].update(locate=collect(L, TAG_LOCATE), drag=collect(L, TAG_DRAG))
        if key != "off":
            out[key].update(contact=collect(L, TAG_CONTACT), stats=pc.surface_contact_stats())
        L.DflProfileEnable(0)
        out[key]["outside"] = int((pc.tet() == -1).sum())
        pc.close()
    P.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
