"""Level-set volume correction at bench size, timed with device events, calls alternating in one job, for a planar and a
spherical surface whose volume drifted by a fraction of the tet size h = 1 / M:

  - one DflMeshLevelSetVolume (one full evaluation of V: the yardstick, and what a naive search pays per candidate);
  - one whole DflMeshVolumeCorrect (the pass over all tets, the band list, the K-section passes, the node pass), with its
    status, passes and band-tet fraction;
  - the same call with the pass limit forced to 1 and to 2 (DFL_VOLUME_PASSES): the difference is one K-section pass with
    its read-back (where the search needs a second pass at all: on a plane V is linear and the first trial is the root).

Every call starts from the same uploaded state.  One JSON record on stdout and into --out.

    python tools/probe_volume_correction.py --M 119 --out profiles/volume_correction_M119.json
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

K = 15


def stats(t):
    return {"ms_mean": float(np.mean(t)), "ms_min": float(min(t)), "ms_max": float(max(t))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=119)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--jitter", type=float, default=0.2)
    ap.add_argument("--drift", type=float, default=0.3, help="drift of the surface, in units of h")
    ap.add_argument("--max-shift", type=float, default=2.0, help="max_shift, in units of h")
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    m = kuhn_cube(a.M, jitter=a.jitter)
    N, T = m.num_node, m.num_tet
    h = 1.0 / a.M
    x = m.xg.reshape(-1, 3)
    wg, _ = synthetic_fields(m)
    fields = {"plane": x[:, 2] - 0.5, "sphere": np.sqrt(((x - np.array([0.55, 0.52, 0.46])) ** 2).sum(axis=1)) - 0.3}
    P = api.Problem(m)
    w_d = api.DeviceArray(6 * N)
    rec = {"what": "volume_correction", "M": a.M, "N": N, "T": T, "K": K, "h": h, "drift_over_h": a.drift,
           "max_shift_over_h": a.max_shift, "tol": a.tol, "reps": a.reps, "warmup": a.warmup, "fields": {}}
    tm = api.Timer()

    def timed(fn):
        tm.start(); fn(); tm.stop()
        return tm.ms()

    for name, phi in fields.items():
        wg[4 * N:5 * N] = phi
        w_d.upload(wg)
        api.sync()
        target = P.level_set_volume(w_d, -a.drift * h)
        variants = {"volume": None, "correct": "", "correct_1_pass": "1", "correct_2_passes": "2"}
        t = {k: [] for k in variants}
        seen = {}
        for rep in range(a.warmup + a.reps):
            for k, limit in variants.items():
                if k == "volume":
                    ms = timed(lambda: P.level_set_volume(w_d, 0.0))
                else:
                    os.environ["DFL_VOLUME_PASSES"] = limit      # (empty: the default)
                    P.set_volume_correction(0.0, a.max_shift * h, a.tol, target)
                    if rep == 0:
                        P.volume_correct(w_d)                    # (the first call grows the band list)
                    w_d.upload(wg)
                    api.sync()
                    ms = timed(lambda: P.volume_correct(w_d))
                    seen[k] = P.volume_correction_stats()
                if rep >= a.warmup:
                    t[k].append(ms)
        os.environ.pop("DFL_VOLUME_PASSES", None)
        st = seen["correct"]
        w_d.upload(wg)
        P.set_volume_correction(0.0, a.max_shift * h, a.tol, target)
        P.volume_correct(w_d)
        after = P.level_set_volume(w_d, 0.0)
        r = {k: stats(v) for k, v in t.items()}
        r["stats"] = st
        r["band_tet_fraction"] = st["band_tets"] / T
        r["band_list_bytes"] = st["band_tets"] * 4
        r["volume_of_new_field_minus_target_over_mesh"] = (after - target) / st["volume_mesh"]
        r["per_pass_ms"] = r["correct_2_passes"]["ms_mean"] - r["correct_1_pass"]["ms_mean"]
        r["naive_search_ms"] = (1 + st["passes"] * K) * r["volume"]["ms_mean"]
        r["speedup_over_naive"] = r["naive_search_ms"] / r["correct"]["ms_mean"]
        rec["fields"][name] = r
    P.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
