"""Particle-fluid coupling at BASELINE config-4 size: kuhn_cube(55, jitter=0.2) (998,250 tets) with 100k particles of
R = 0.004.  Times, per sub-step, with device events (DflProfile tags of host/couple.c and host/particle.c):
  locate from history and from cold (every tet reset to "none"), the drag kernel, the whole fluid sub-step (contact sweep +
  locate + drag), the reaction load (counting sort by tet + node scatter) after 10 sub-steps;
the walk with the particles in the contact sweep's cell order against particle-id order
(DFL_COUPLE_CELL_ORDER=0: the walk; the drag kernel always runs in id order); and DflTimeStep (two-level PC, 2 Newton
iterations, 10 sub-steps) coupled one-way and two-way against the uncoupled contact sweep.  With --walls every particle
context takes its walls from all six boundary groups of the mesh (ParticleContextSetWallMesh) instead of the unit box;
"sweep" then also times the contact sweep alone.  With --friction every particle context turns on the contact friction
(ParticleContextSetFriction, mu = 0.5, default kt and gamma_t).  Prints one JSON line (and writes it to --out).

  python tools/probe_coupling.py [--reps 50] [--steps 3] [--walls] [--friction] [--out profiles/probe_coupling.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dedflow_amd import api  # noqa: E402
from dedflow_amd.meshgen import dem_particles, kuhn_cube, synthetic_fields  # noqa: E402

TAG_DEM_FORCE, TAG_LOCATE, TAG_DRAG, TAG_REACTION = 9, 10, 11, 12   # DFL_TAG_SMALL + 1 .. + 4


def collect(L, tag):
    tot, mn = C.c_double(0), C.c_double(0)
    n = L.DflProfileCollect(tag, C.byref(tot), C.byref(mn))
    return {"n": n, "mean_us": 1e3 * tot.value / max(n, 1), "min_us": 1e3 * mn.value}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=55)
    ap.add_argument("--particles", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--walls", action="store_true")
    ap.add_argument("--friction", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L = api.lib()
    m = kuhn_cube(a.M, jitter=0.2)
    N = m.num_node
    wg, dw0 = synthetic_fields(m)
    wg[3 * N:4 * N] = 0.0
    R = 0.004
    mass = 2000.0 * 4.0 / 3.0 * np.pi * R ** 3
    x, v, _ = dem_particles(a.particles, R)
    P = api.Problem(m, maxit=120, atol=1e-12, rtol=1e-4)
    L.KrylovSetPCType(P.ksp, api.PC_TWOLEVEL)
    w_d = api.DeviceArray.from_numpy(wg)
    out = {"M": a.M, "tets": m.num_tet, "particles": a.particles, "R": R, "walls": a.walls, "friction": a.friction}

    def particles(order=True):
        if not order:
            os.environ["DFL_COUPLE_CELL_ORDER"] = "0"
        try:
            pc = api.Particles(x, v, R, mass=mass, dt=1e-4)
            t0 = time.perf_counter()
            if a.walls:
                pc.set_walls(P)
            if a.friction:
                pc.set_friction(0.5)
            pc.couple(P, two_way=True)
            api.sync()
            return pc, time.perf_counter() - t0
        finally:
            os.environ.pop("DFL_COUPLE_CELL_ORDER", None)

    for order in (True, False):
        pc, setup_s = particles(order)
        key = "cell_order" if order else "id_order"
        for _ in range(3):                       # warm-up of every launch shape
            pc.fluid_step(w_d)
        pc.reaction_load()
        api.sync()
        # cold: every particle starts from the seed grid (couple() on the same mesh only resets the per-particle state)
        L.DflProfileEnable(1)
        for _ in range(a.reps):
            pc.couple(P, two_way=True)
            pc.locate()
        cold = collect(L, TAG_LOCATE)
        L.DflProfileEnable(1)
        for _ in range(a.reps):
            pc.locate()
        hist = collect(L, TAG_LOCATE)
        L.DflProfileEnable(1)
        t = api.Timer()
        t.start()
        for _ in range(a.reps):
            pc.fluid_step(w_d)
        t.stop()
        sub_ms = t.ms() / a.reps
        drag = collect(L, TAG_DRAG)
        force = collect(L, TAG_DEM_FORCE)
        loc_sub = collect(L, TAG_LOCATE)
        L.DflProfileEnable(1)
        load = api.DeviceArray(3 * N)
        for _ in range(a.reps):
            for _ in range(10):
                pc.fluid_step(w_d)
            pc.reaction_load(load)
        react = collect(L, TAG_REACTION)
        L.DflProfileEnable(0)
        t = api.Timer()
        t.start()
        for _ in range(a.reps):
            pc.compute_forces()
        t.stop()
        sweep_us = 1e3 * t.ms() / a.reps
        out[key] = {"setup_s": setup_s, "sweep_us": sweep_us, "locate_cold": cold, "locate_history": hist, "locate_in_substep": loc_sub, "drag": drag,
                    "dem_force": force, "fluid_substep_us": 1e3 * sub_ms, "reaction_load": react,
                    "lost": pc.lost_count(), "outside": int((pc.tet() == -1).sum())}
        pc.close()

    # DflTimeStep: uncoupled contact sweep vs one-way and two-way coupling, 10 sub-steps each, same states.  The two-way
    # leg changes the flow problem itself (the reaction of 1e-3 s of particle time enters a 0.05 s fluid step), so its
    # GMRES iteration counts are reported beside the times
    stats = L.KrylovGetStats(P.ksp).contents
    for key in ("uncoupled", "one_way", "two_way"):
        pc = api.Particles(x, v, R, mass=mass, dt=1e-4)
        if a.walls:
            pc.set_walls(P)
        if a.friction:
            pc.set_friction(0.5)
        if key != "uncoupled":
            pc.couple(P, two_way=key == "two_way")
        st = [api.DeviceArray.from_numpy(q) for q in (wg, 0.1 * dw0, 0.1 * dw0)]
        F_d, dx_d = api.DeviceArray(6 * N), api.DeviceArray(6 * N)
        times, its, gmres = [], [], []
        for k in range(a.steps + 1):
            api.sync()
            g0 = int(stats.total_iterations)
            t0 = time.perf_counter()
            it, rn, ri = P.time_step(st[0], st[1], st[2], F_d, dx_d, newton_maxit=2, particles=pc, dem_substeps=10)
            api.sync()
            if k:                                 # the first step builds schedules / calibrates
                times.append(1e3 * (time.perf_counter() - t0))
                its.append(it)
                gmres.append(int(stats.total_iterations) - g0)
        out["timestep_" + key] = {"ms": times, "newton_its": its, "gmres_its": gmres}
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
