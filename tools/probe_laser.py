"""Cost of the laser step at 1M tets (kuhn_cube(55, jitter=0.2)) and 100k particles (dem_particles(100000, 0.004), BASELINE
config 4's particles): the coupled sub-step (ParticleContextFluidStep: contact sweep, locate, drag, heat step) with heat on
(conduction + convection) and the laser off, and with the laser on (beam along -z through the middle of the box, the z-
boundary group as substrate), between two device events, mean of --reps after --warmup.  Run it under
`rocprofv3 --kernel-trace --stats` for per-kernel times (laser_*_kernel and the dem_* launches of the column sort next to
heat_*_kernel, dem_force_kernel and couple_fluid_kernel); --kernel-stats turns the CSV of such a run into records of the
same file.  Prints one JSON line per case (appended to --out).  --root imports the package of another checkout (the parent
commit, which has no laser: --cases laser_off), --label names the side in the records.

  python tools/probe_laser.py [--reps 50] [--warmup 5] [--cases laser_off,laser_on] [--root DIR] [--label this]
                              [--out profiles/laser_M55.jsonl]
  python tools/probe_laser.py --kernel-stats DIR/..._kernel_stats.csv --label this_rocprofv3 --out profiles/laser_M55.jsonl
"""
import argparse
import json
import os
import re
import sys

CASES = ("laser_off", "laser_on")


def kernel_stats(path, label, out):
    """the DEM / coupling / heat / laser kernels of a rocprofv3 --kernel-trace --stats CSV as one record each"""
    import csv
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row["Name"]
            if not any(k in name for k in ("dem_", "couple_", "heat_", "wall_", "laser_")):
                continue
            short = re.sub(r"\(anonymous namespace\)::|^void ", "", name)
            short = short[:short.index(">(") + 1] if ">(" in short else short.split("(")[0]
            rec = {"label": label, "kernel": short, "calls": int(row["Calls"]),
                   "mean_us": float(row["AverageNs"]) / 1e3, "min_us": float(row["MinNs"]) / 1e3,
                   "max_us": float(row["MaxNs"]) / 1e3}
            print(json.dumps(rec))
            if out:
                with open(out, "a") as g:
                    g.write(json.dumps(rec) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=55)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--cases", default=",".join(CASES))
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
    wg, _ = synthetic_fields(m)
    x, v, R = dem_particles(100000, 0.004)
    P = api.Problem(m)
    w_d = api.DeviceArray.from_numpy(wg)
    for case in a.cases.split(","):
        pc = api.Particles(x, v, R, dt=1e-5)
        pc.couple(P)
        pc.set_heat(cp_p=500.0, k_p=40.0, T_init=1500.0)
        if case == "laser_on":   # a 0.2-wide beam: 25 x 25 columns of edge 2R hold about 6% of the particles
            pc.set_laser((0.5, 0.5, 2.0), (0.0, 0.0, -1.0), power=400.0, w=0.05, h=2.0 * R, r_cut=0.1, eta_p=0.35, eta_s=0.45,
                         substrate_groups=(4,))
        for _ in range(a.warmup):
            pc.fluid_step(w_d)
        api.sync()
        t = api.Timer()
        t.start()
        for _ in range(a.reps):
            pc.fluid_step(w_d)
        t.stop()
        rec = {"label": a.label, "case": case, "M": a.M, "tets": m.num_tet, "particles": pc.P, "reps": a.reps,
               "fluid_step_us": 1e3 * t.ms() / a.reps}
        if case == "laser_on":
            rec["tally"] = pc.laser_tally()
        print(json.dumps(rec))
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(rec) + "\n")
        pc.close()
    P.close()


if __name__ == "__main__":
    main()
