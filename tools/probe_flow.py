"""Particle inflow and outflow cost: ParticleContextRemove removing 10 % of the particles and ParticleContextAdd inserting
1000, at 100k and 1M particles, with friction and coupling off and on.  Every call is timed with a device-event pair on the
library stream around it (it ends with its own 4-byte read back, so the pair spans the whole call) and by the host clock.
Remove runs on a fresh context per repetition (it is destructive), after contact sweeps (live friction history) and, when
coupled, fluid sub-steps (pending impulse: the removed particles' impulse is scattered too).  Add runs after one warm-up
call (which grows the capacity) with the inlet moved between calls so that every call finds 1000 free slots.  The frictionless
contact sweep of the same state is timed for comparison.  Prints one JSON line (and writes it to --out).

  python tools/probe_flow.py [--sizes 100000,1000000] [--reps 5] [--M 40] [--out profiles/flow_probe.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dedflow_amd import api  # noqa: E402
from dedflow_amd.meshgen import dem_particles, kuhn_cube, synthetic_fields  # noqa: E402


def _timed(fn):
    t = api.Timer()
    h0 = time.perf_counter()
    t.start()
    fn()
    t.stop()
    ms = t.ms()
    return 1e3 * ms, 1e6 * (time.perf_counter() - h0)


def _context(x, v, R, problem, w_d, friction, coupled):
    pc = api.Particles(x, v, R, mass=1.0, dt=1e-5)
    if friction:
        pc.set_friction(0.5)
    if coupled:
        pc.couple(problem)
    for _ in range(2):
        if coupled:
            pc.fluid_step(w_d)
        else:
            pc.update()
    api.sync()
    return pc


def _bytes_remove(P, removed, friction, coupled, hist_live):
    """byte model: flag (24 read + 4 write [+ 4 tet]), scan (4 read + 4 write), compaction (keep 4 + newid 4 read, then per
    survivor: 3 x 24 B coord/vel/acc + 8 B tag read and written, [+ 2 x 24 B w/alpha + 4 B count + 32 B per live history
    entry], [+ 4 + 32 + 24 B tet/lambda/imp])"""
    S = P - removed
    rec = 3 * 24 + 8 + (48 + 4 + 0) * friction + (4 + 32 + 24) * coupled
    b = P * (24 + 4 + 4 * coupled) + 8 * P + 8 * P + 2 * S * rec + 2 * 32 * hist_live * friction
    return int(b)


def _bytes_add(P_near, n, nslot, friction, coupled):
    """byte model: block pass reads 24 B of every particle (P_near of them test slots), keys 8 + 4 B per slot, radix sort
    ~ 8 passes x 2 x 12 B per slot, append writes 3 x 24 + 8 B [+ 48 + 4] [+ 4 + 32 + 24] per inserted particle"""
    return None if P_near is None else int(P_near + 12 * nslot + 8 * 2 * 12 * nslot
                                           + n * (80 + 52 * friction + 60 * coupled))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--M", type=int, default=40)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L = api.lib()
    m = kuhn_cube(a.M, jitter=0.2)
    problem = api.Problem(m)
    wg, _ = synthetic_fields(m)
    w_d = api.DeviceArray.from_numpy(wg)
    out = {"M": a.M, "tets": m.num_tet, "reps": a.reps, "runs": []}
    for P in (int(s) for s in a.sizes.split(",")):
        R = 0.004 * (100000 / P) ** (1.0 / 3.0)
        x, v, _ = dem_particles(P, R)
        for friction in (False, True):
            for coupled in (False, True):
                row = {"P": P, "R": R, "friction": friction, "coupled": coupled}
                rem_ev, rem_host, removed, hist_live = [], [], 0, 0
                for _ in range(a.reps):
                    pc = _context(x, v, R, problem, w_d, friction, coupled)
                    if friction:
                        hist_live = int(pc.friction_history()[2].sum())
                    pc.set_outflow([(1.0, 0.0, 0.0, 0.9)])
                    ev, host = _timed(pc.remove)
                    rem_ev.append(ev)
                    rem_host.append(host)
                    removed = pc.flow_stats()["removed"]
                    pc.close()
                row["remove"] = {"removed": removed, "event_us": rem_ev, "host_us": rem_host,
                                 "min_event_us": min(rem_ev), "bytes_model": _bytes_remove(P, removed, friction, coupled, hist_live)}
                pc = _context(x, v, R, problem, w_d, friction, coupled)
                side = 50 * 2 * R * 1.02
                add_ev, add_host, ins = [], [], []
                for k in range(a.reps + 1):
                    pc.set_inflow((0.3, 0.3, 0.2 + 0.05 * k), (side, 0.0, 0.0), (0.0, side, 0.0), per_call=1000, seed=k)
                    before = pc.flow_stats()["inserted"]
                    ev, host = _timed(pc.add)
                    if k > 0:   # the first call grows the capacity
                        add_ev.append(ev)
                        add_host.append(host)
                        ins.append(pc.flow_stats()["inserted"] - before)
                row["add"] = {"inserted": ins, "event_us": add_ev, "host_us": add_host, "min_event_us": min(add_ev),
                              "bytes_model": _bytes_add(24 * pc.P, 1000, 2500, friction, coupled)}
                if not friction and not coupled:
                    pc.close()
                    pc = api.Particles(x, v, R)
                    for _ in range(3):
                        pc.compute_forces()
                    sw = [_timed(pc.compute_forces)[0] for _ in range(10)]
                    row["sweep_event_us"] = min(sw)
                pc.close()
                out["runs"].append(row)
                print(json.dumps({k: row[k] for k in ("P", "friction", "coupled")}), "remove",
                      round(row["remove"]["min_event_us"], 1), "add", round(row["add"]["min_event_us"], 1), flush=True)
    problem.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
