"""Phase change at bench size: the time of one DflMeshPhaseCoefficients (D, H and G, latent heat and drag on) in three states --
all solid (the worst case: every tet adds to D and H), a realistic pool (a hot spot on a cold block under a planar surface,
use_phi) and all liquid -- with the one-byte-per-tet flag pass in front and the node pass alone (DFL_PHASE_FLAGS=0), whose
outputs must be the same bits; beside them, call by call in the same job and timed with device events, DflMeshSurfaceLoad
without its flags (the same gathers) and AssembleSystem(F) with the phase terms in it (coefficient pass + F update), and first
of all AssembleSystem(F) before the feature is set.  One JSON record on stdout and into --out.

    python tools/probe_phase.py --M 119 --out profiles/phase_change_M119.json
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

PHASE = dict(T_solidus=1600.0, T_liquidus=1700.0, latent=2.0e9, darcy_c=1.0e6, darcy_b=1e-3)
SURFACE = dict(level=0.0, side=-1, sigma0=1.8, dsigma_dT=-4e-4, T_ref=1900.0, recoil_p0=1.0e5, recoil_a=11.0, T_boil=3100.0,
               h_conv=80.0, emissivity=0.4, T_amb=300.0, evap_q0=2.0e9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=119)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--jitter", type=float, default=0.2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = api.lib()
    m = kuhn_cube(a.M, jitter=a.jitter)
    N, T = m.num_node, m.num_tet
    x = m.xg.reshape(-1, 3)
    wg, dwg = synthetic_fields(m)
    wg[4 * N:5 * N] = x[:, 2] - 0.75                              # metal below z = 0.75
    r2 = (x[:, 0] - 0.5) ** 2 + (x[:, 1] - 0.5) ** 2 + (x[:, 2] - 0.75) ** 2
    fields = {"all_solid": (np.full(N, 300.0), {}),
              "pool": (300.0 + 2200.0 * np.exp(-r2 / 0.15 ** 2), dict(use_phi=True, level=0.0, side=-1, eps=2.0 / a.M)),
              "all_liquid": (np.full(N, 2500.0), {})}
    os.environ["DFL_SURFACE_FLAGS"] = "0"
    P = api.Problem(m)
    P.set_surface_forces(eps=2.0 / a.M, **SURFACE)
    wg_d, dwg_d, F_d = api.DeviceArray.from_numpy(wg), api.DeviceArray.from_numpy(dwg), api.DeviceArray(6 * N)
    out = [api.DeviceArray(N) for _ in range(3)]
    sout = [api.DeviceArray(3 * N), api.DeviceArray(N), api.DeviceArray(N)]

    def phase():
        L.DflMeshPhaseCoefficients(P.mesh, wg_d.ptr, out[0].ptr, out[1].ptr, out[2].ptr)

    def surface():
        L.DflMeshSurfaceLoad(P.mesh, wg_d.ptr, sout[0].ptr, sout[1].ptr, sout[2].ptr)

    def assemble():
        P.assemble_system(wg_d, dwg_d, F_d)

    rec = {"what": "phase_change", "M": a.M, "N": N, "T": T, "node_tet_pairs": 4 * T, "reps": a.reps, "states": {}}
    tm = api.Timer()
    for _ in range(a.warmup):
        assemble()
    api.sync()
    t0 = []
    for _ in range(a.reps):                                       # before the feature is set: the residual as it was
        tm.start(); assemble(); tm.stop(); t0.append(tm.ms())
    rec["assemble_F_off_ms_mean"], rec["assemble_F_off_ms_min"] = float(np.mean(t0)), min(t0)
    all_same = True
    for name, (Tf, extra) in fields.items():
        wg[5 * N:] = Tf
        wg_d.upload(wg)
        srec, results = {}, {}
        for mode in ("node_pass", "flag_pass"):
            os.environ["DFL_PHASE_FLAGS"] = "1" if mode == "flag_pass" else "0"
            P.set_phase_change(**dict(PHASE, **extra))
            for _ in range(a.warmup):
                phase(); surface(); assemble()
            api.sync()
            t = {"phase": [], "surface": [], "assemble": []}
            for _ in range(a.reps):
                for key, fn in (("phase", phase), ("surface", surface), ("assemble", assemble)):
                    tm.start(); fn(); tm.stop(); t[key].append(tm.ms())
            api.sync()
            results[mode] = [o.numpy() for o in out]
            srec[mode] = {"coefficients_ms_mean": float(np.mean(t["phase"])), "coefficients_ms_min": min(t["phase"]),
                          "coefficients_ms_max": max(t["phase"]),
                          "surface_load_noflags_ms_mean": float(np.mean(t["surface"])), "surface_load_noflags_ms_min": min(t["surface"]),
                          "assemble_F_with_phase_ms_mean": float(np.mean(t["assemble"])),
                          "assemble_F_with_phase_ms_min": min(t["assemble"])}
        same = all(np.array_equal(p.view(np.uint64), q.view(np.uint64)) for p, q in zip(results["node_pass"], results["flag_pass"]))
        all_same = all_same and same
        D, H, G = results["node_pass"]
        srec.update({"flag_pass_same_bits": bool(same), "sum_D": float(D.sum()), "sum_H": float(H.sum()), "liquid_volume": float(G.sum()),
                     "nodes_with_drag": int((D != 0).sum()), "finite": bool(all(np.isfinite(r).all() for r in results["node_pass"]))})
        st = P.phase_stats(wg_d)
        srec["stats"] = {"liquid_volume": st["liquid_volume"], "T_max": st["T_max"], "molten": st["molten"]}
        rec["states"][name] = srec
    # bytes from HBM at the least: V2E (4 B x (N + 1 + 4T)), the outputs (24 B x N); ien (16 B x T), T, phi and coordinates
    # (40 B x N) once each when L2 serves the repeats; the flag pass adds T bytes written and read back
    rec["hbm_floor_bytes"] = 4 * (N + 1 + 4 * T) + 24 * N + 16 * T + 40 * N
    P.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not all_same:
        sys.exit("the flag pass changed the results")


if __name__ == "__main__":
    main()
