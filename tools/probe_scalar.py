"""phi / T transport at bench size: time of the scalar Jacobian kernel (with its byte model), of one scalar Newton update
(DflScalarTransportSolve: residual, both Jacobians, both GMRES solves) for Jacobi and AMG, the GMRES iterations per
solve, and one DflTimeStep with the transport on and off.  One JSON line per measurement on stdout and into --out.

    python tools/probe_scalar.py --M 119 --out profiles/scalar_M119.jsonl
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dedflow_amd import api  # noqa: E402
from dedflow_amd.meshgen import kuhn_cube, synthetic_fields  # noqa: E402


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=119)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-steps", action="store_true")
    a = ap.parse_args()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    L = api.lib()
    m = kuhn_cube(a.M)
    N, T = m.num_node, m.num_tet
    wgold, dwgold = synthetic_fields(m)
    P = api.Problem(m)
    nnz1 = P.nnz1
    d = [api.DeviceArray.from_numpy(x) for x in (wgold, dwgold, 0.5 * dwgold)]

    # ---- the kernel alone: two CSR matrices over the nodal pattern, transport set (V2E built once, as in the driver)
    P.set_scalar_transport()
    Jp, Jt = L.MatrixCreateTypeCSR(P.spy1x1, None), L.MatrixCreateTypeCSR(P.spy1x1, None)
    L.DflAssembleScalarJacobian(P.mesh, d[0].ptr, d[1].ptr, Jp, Jt)  # warm-up (allocates values, builds V2E)
    api.sync()
    tm = api.Timer()
    times = []
    for _ in range(a.reps):
        tm.start()
        L.DflAssembleScalarJacobian(P.mesh, d[0].ptr, d[1].ptr, Jp, Jt)
        tm.stop()
        times.append(tm.ms())
    # bytes: values written (2 x 8 B x nnz1), row_ptr + col_ind (4 B x (N + 1 + nnz1)), V2E (4 B x (N + 1 + 4T)), and per
    # (row, tet) pair one ien line (16 B) + 4 nodes x 48 B of coordinates and velocities (L2 hits mostly; counted once per
    # node as the HBM floor: 48 B x N)
    floor = 16 * nnz1 + 4 * (N + 1 + nnz1) + 4 * (N + 1 + 4 * T) + 16 * T + 48 * N
    emit(a.out, {"what": "scalar_jacobian_kernel", "M": a.M, "N": N, "T": T, "nnz1": nnz1, "ms_min": min(times),
                 "ms_median": float(np.median(times)), "hbm_floor_bytes": floor,
                 "floor_GBps_at_min": floor / (min(times) * 1e-3) / 1e9, "row_tet_pairs": 4 * T})
    L.MatrixDestroy(Jp)
    L.MatrixDestroy(Jt)

    # ---- one scalar Newton update, Jacobi and AMG
    for pc in ("jacobi", "amgx"):
        P.set_scalar_transport(pc=pc)
        dd = [api.DeviceArray.from_numpy(x) for x in (wgold, dwgold, 0.5 * dwgold)]
        P.solve_scalar(*dd)  # warm-up: state, PC structure, GMRES bases
        api.sync()
        ts = []
        for _ in range(3):
            dd[2].upload(0.5 * dwgold)
            api.sync()
            t0 = time.perf_counter()
            rn, its = P.solve_scalar(*dd)
            api.sync()
            ts.append((time.perf_counter() - t0) * 1e3)
        emit(a.out, {"what": "scalar_newton_update", "pc": pc, "M": a.M, "ms_min": min(ts), "ms_all": ts,
                     "gmres_its_phi": its[0], "gmres_its_T": its[1], "rnorm": rn.tolist()})
    P.clear_scalar_transport()

    # ---- one DflTimeStep, transport on and off (each after a warm-up step of its own)
    if not a.skip_steps:
        for on in (False, True):
            if on:
                P.set_scalar_transport()
            F_d, dx_d = api.DeviceArray(6 * N), api.DeviceArray(6 * N)
            rec = {"what": "time_step", "transport": on, "M": a.M}
            for k in range(2):
                dd = [api.DeviceArray.from_numpy(x) for x in (wgold, dwgold, dwgold)]
                api.sync()
                t0 = time.perf_counter()
                it, rn, r0 = P.time_step(dd[0], dd[1], dd[2], F_d, dx_d)
                api.sync()
                ms = (time.perf_counter() - t0) * 1e3
                rec["warmup_ms" if k == 0 else "ms"] = ms
            its = (C.c_int32 * 2)()
            L.DflScalarTransportIterations(P.mesh, its)
            rec.update({"newton_its": it, "rnorm": rn.tolist(), "rnorm_init": r0.tolist(),
                        "gmres_its_last_scalar": [int(its[0]), int(its[1])] if on else None})
            emit(a.out, rec)
            for x in (F_d, dx_d):
                x.free()
        P.clear_scalar_transport()
    P.close()


if __name__ == "__main__":
    main()
