"""Track cross-sections at bench size: the time of one DflMeshTrackSections at 1, 8 and 64 stations across a bead, beside
DflMeshLevelSetVolume on the same state (the project's plain one-pass read of every tet: the yardstick of the count pass) and
beside the same evaluation made the obvious way, one configuration of one station and one full evaluation per station (only the
evaluations are timed, not the Set calls between them).  Call by call in one job, warm, device events around every call; an
evaluation waits for the device once inside, and that wait is inside its time.  One JSON record on stdout and into --out.

    python tools/probe_track_sections.py --M 119 --out profiles/track_sections_M119.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dedflow_amd import api  # noqa: E402
from dedflow_amd.meshgen import kuhn_cube, synthetic_fields  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=119)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--jitter", type=float, default=0.2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = api.lib()
    m = kuhn_cube(a.M, jitter=a.jitter)
    N, T = m.num_node, m.num_tet
    x = m.xg.reshape(-1, 3)
    wg, _ = synthetic_fields(m)
    wg[4 * N:5 * N] = 0.7 - x[:, 2] - 0.8 * np.abs(x[:, 1] - 0.5)          # the bead of the tests: substrate below z = 0.5
    w_d = api.DeviceArray.from_numpy(wg)
    Tp_d = api.DeviceArray.from_numpy(1700.0 + 1000.0 * (x[:, 2] - 0.4))
    base = dict(origin=(0.0, 0.5, 0.5), normal=(1.0, 0.0, 0.0), up=(0.0, 0.0, 1.0), level=0.0, side=1, T_fuse=1700.0)
    P = api.Problem(m)
    tm = api.Timer()
    rec = {"what": "track_sections", "M": a.M, "N": N, "T": T, "reps": a.reps, "stations": {}}

    def timed(fn):
        tm.start(); fn(); tm.stop()
        return tm.ms()

    def volume():
        L.DflMeshLevelSetVolume(P.mesh, w_d.ptr, 0.0)

    def evaluate():
        L.DflMeshTrackSections(P.mesh, w_d.ptr, Tp_d.ptr)

    for ns in (1, 8, 64):
        stations = [0.1 + 0.8 * (k + 0.5) / ns for k in range(ns)]
        P.set_track_sections(stations, **base)
        for _ in range(a.warmup):
            evaluate(); volume()
        api.sync()
        t_eval, t_vol = [], []
        for _ in range(a.reps):
            t_eval.append(timed(evaluate))
            t_vol.append(timed(volume))
        res = P.track_sections_result()
        t_each = []
        for _ in range(max(1, a.reps // 4)):
            total = 0.0
            for c in stations:
                P.set_track_sections([c], **base)
                total += timed(evaluate)
            t_each.append(total)
        rec["stations"][str(ns)] = {
            "evaluation_ms_mean": float(np.mean(t_eval)), "evaluation_ms_min": min(t_eval), "evaluation_ms_max": max(t_eval),
            "level_set_volume_ms_mean": float(np.mean(t_vol)), "level_set_volume_ms_min": min(t_vol),
            "one_evaluation_per_station_ms_mean": float(np.mean(t_each)), "one_evaluation_per_station_ms_min": min(t_each),
            "pairs": int(sum(r["pairs"] for r in res)),
            "area_clad_max_error": float(max(abs(r["area_clad"] - 0.05) for r in res)),
            "area_fused_max_error": float(max(abs(r["area_fused"] - 0.0625) for r in res)),
            "dilution_first": res[0]["dilution"]}
    P.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
