"""Thermal material at bench size, timed with device events, call by call in one job:

  - DflMeshThermalRows with r alone (thermal_rows_kernel<1>, the launch every F assembly adds) beside the phase-change
    coefficient pass (the same node gather, its yardstick) and with all three outputs (thermal_rows_kernel<3>);
  - DflAssembleScalarJacobian without and with a material (scalar_jac_row_kernel<false> / <true>; no transport and no phase
    change are set, so the call is that one launch), alternating;
  - one DflScalarTransportSolve (T alone, Jacobi) without and with the material, a 1000 : 1 conductivity jump across
    phi = 0, with the GMRES iterations of the T solve.

One JSON record on stdout and into --out.

    python tools/probe_thermal.py --M 119 --out profiles/thermal_material_M119.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dedflow_amd import api  # noqa: E402
from dedflow_amd.meshgen import kuhn_cube, synthetic_fields  # noqa: E402

PHASE = dict(T_solidus=1600.0, T_liquidus=1700.0, latent=2.0e9, darcy_c=1.0e6, darcy_b=1e-3)


def stats(t):
    return {"ms_mean": float(np.mean(t)), "ms_min": float(min(t)), "ms_max": float(max(t))}


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
    wg[5 * N:] = 300.0 + 2200.0 * np.exp(-r2 / 0.15 ** 2)         # a hot spot on a cold block
    mat = dict(k_gas=0.03, k_solid=30.0, k_liquid=45.0, c_gas=1.0e3, c_metal=4.0e6, T_solidus=1600.0, T_liquidus=1700.0,
               use_phi=True, level=0.0, side=-1, eps=2.0 / a.M)
    P = api.Problem(m)
    wg_d, dwg_d = api.DeviceArray.from_numpy(wg), api.DeviceArray.from_numpy(dwg)
    out = [api.DeviceArray(N) for _ in range(3)]
    rec = {"what": "thermal_material", "M": a.M, "N": N, "T": T, "node_tet_pairs": 4 * T, "nnz": int(P.nnz1), "reps": a.reps}
    tm = api.Timer()

    def timed(fn):
        tm.start(); fn(); tm.stop()
        return tm.ms()

    # ---- the row pass beside the phase-change coefficient pass ----------------------------------------------------------
    P.set_phase_change(use_phi=True, level=0.0, side=-1, eps=2.0 / a.M, **PHASE)
    P.set_thermal_material(**mat)
    calls = {"thermal_rows_r": lambda: L.DflMeshThermalRows(P.mesh, wg_d.ptr, dwg_d.ptr, out[0].ptr, None, None),
             "phase_coefficients": lambda: L.DflMeshPhaseCoefficients(P.mesh, wg_d.ptr, out[0].ptr, out[1].ptr, out[2].ptr),
             "thermal_rows_r_Kn_Cn": lambda: L.DflMeshThermalRows(P.mesh, wg_d.ptr, dwg_d.ptr, out[0].ptr, out[1].ptr, out[2].ptr)}
    for _ in range(a.warmup):
        for fn in calls.values():
            fn()
    api.sync()
    t = {k: [] for k in calls}
    for _ in range(a.reps):
        for k, fn in calls.items():
            t[k].append(timed(fn))
    api.sync()
    rec["rows"] = {k: stats(v) for k, v in t.items()}
    r = out[0].numpy()
    rec["rows"]["finite"] = bool(np.isfinite(r).all())
    P.set_phase_change()
    # ---- the scalar Jacobians, alternating ------------------------------------------------------------------------------
    t = {"jacobian_off": [], "jacobian_on": []}
    for rep in range(a.warmup + a.reps):
        for k in t:
            P.set_thermal_material(**mat) if k == "jacobian_on" else P.set_thermal_material()
            L.DflAssembleScalarJacobian(P.mesh, wg_d.ptr, dwg_d.ptr, *_scalar_matrices(P, L))   # (the first call allocates)
            api.sync()
            ms = timed(lambda: L.DflAssembleScalarJacobian(P.mesh, wg_d.ptr, dwg_d.ptr, *_scalar_matrices(P, L)))
            if rep >= a.warmup:
                t[k].append(ms)
    rec["jacobian"] = {k: stats(v) for k, v in t.items()}
    # ---- one T solve each way ---------------------------------------------------------------------------------------------
    rec["solve"] = {}
    for k, cfg in (("off", None), ("on", mat)):
        P.set_scalar_transport(phi=False, T=True, rtol=1e-8, maxit=200)
        P.set_thermal_material(**cfg) if cfg else P.set_thermal_material()
        st = [api.DeviceArray.from_numpy(v) for v in (wg, 0.1 * dwg, 0.1 * dwg)]
        P.solve_scalar(st[0], st[1], st[2])                        # builds the solver
        api.sync()
        st[2].upload(0.1 * dwg)
        api.sync()
        t0 = time.perf_counter()
        rn, its = P.solve_scalar(st[0], st[1], st[2])              # (reads the norms back: synchronised)
        api.sync()
        rec["solve"][k] = {"ms": 1e3 * (time.perf_counter() - t0), "gmres_iterations_T": int(its[1]), "residual_T": float(rn[1]),
                           "finite": bool(np.isfinite(st[2].numpy()).all())}
        P.clear_scalar_transport()
    # bytes from HBM at the least, row pass: V2E (4 B x (N + 1 + 4T)), r (8 B x N), ien (16 B x T), x, u, phi, T, dT (72 B x N)
    # once each when L2 serves the repeats
    rec["rows_hbm_floor_bytes"] = 4 * (N + 1 + 4 * T) + 8 * N + 16 * T + 72 * N
    P.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


def _scalar_matrices(P, L):
    if getattr(P, "_sj", None) is None:
        P._sj = (L.MatrixCreateTypeCSR(P.spy1x1, None), L.MatrixCreateTypeCSR(P.spy1x1, None))
    return P._sj


if __name__ == "__main__":
    main()
