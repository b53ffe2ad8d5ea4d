"""Fluid material at bench size, timed with device events, alternating call by call in one job: a planar surface with metal
below, a hot spot on it.

  - DflMeshFluidRows with r alone (fluid_rows_kernel<4>, the launch every F assembly adds) and with all three outputs (<6>);
  - the Jacobian correction alone (fluid_jac_row_kernel through its launcher, onto the block values of the (u,p) matrix);
  - beside them the kernels with the same skeletons: DflMeshThermalRows (r alone) and DflAssembleScalarJacobian with a
    thermal material;
  - the F assembly and the J assembly of the (u,p) system with the fluid material off: the launches of the parent commit.

One JSON record on stdout and into --out, with the ratios of the two new kernels to those four yardsticks.

    python tools/probe_fluid.py --M 119 --out profiles/fluid_material_M119.json
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dedflow_amd import api  # noqa: E402
from dedflow_amd.meshgen import kuhn_cube, synthetic_fields  # noqa: E402


class FluidParams(C.Structure):                                   # dfl_fluid_params of include/dedflow_kernels.h
    _fields_ = [("rho_gas", C.c_double), ("rho_metal", C.c_double), ("mu_gas", C.c_double), ("mu_metal", C.c_double),
                ("gravity", C.c_double * 3), ("beta", C.c_double), ("T_ref", C.c_double), ("level", C.c_double),
                ("side", C.c_double), ("eps", C.c_double), ("use_phi", C.c_int)]


def stats(t):
    return {"ms_mean": float(np.mean(t)), "ms_min": float(min(t)), "ms_max": float(max(t))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=119)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
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
    eps = 2.0 / a.M
    fluid = dict(rho_gas=1.2, rho_metal=7000.0, mu_gas=2.0e-5, mu_metal=5.0e-3, gravity=(0.0, 0.0, -9.81), beta=1.0e-4, T_ref=1700.0,
                 use_phi=True, level=0.0, side=-1, eps=eps)
    thermal = dict(k_gas=0.03, k_solid=30.0, k_liquid=45.0, c_gas=1.0e3, c_metal=4.0e6, T_solidus=1600.0, T_liquidus=1700.0,
                   use_phi=True, level=0.0, side=-1, eps=eps)
    P = api.Problem(m)
    wg_d, dwg_d = api.DeviceArray.from_numpy(wg), api.DeviceArray.from_numpy(dwg)
    r4, rn, mn, F = api.DeviceArray(4 * N), api.DeviceArray(N), api.DeviceArray(N), api.DeviceArray(6 * N)
    rec = {"what": "fluid_material", "M": a.M, "N": N, "T": T, "node_tet_pairs": 4 * T, "nnz": int(P.nnz1), "reps": a.reps}
    tm = api.Timer()

    def timed(fn):
        tm.start(); fn(); tm.stop()
        return tm.ms()

    P.set_thermal_material(**thermal)
    sj = (L.MatrixCreateTypeCSR(P.spy1x1, None), L.MatrixCreateTypeCSR(P.spy1x1, None))
    P.set_fluid_material(**fluid)
    vrow, vcol = C.c_void_p(), C.c_void_p()
    L.DflMeshSortedV2E.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.DflMeshSortedV2E.restype = None
    L.DflMeshSortedV2E(P.mesh, C.byref(vrow), C.byref(vcol))
    L.dfl_fluid_add_jacobian.argtypes = [C.c_int32] + [C.c_void_p] * 10
    L.dfl_fluid_add_jacobian.restype = None
    prm = FluidParams(fluid["rho_gas"], fluid["rho_metal"], fluid["mu_gas"], fluid["mu_metal"], (C.c_double * 3)(*fluid["gravity"]),
                      fluid["beta"], fluid["T_ref"], fluid["level"], float(fluid["side"]), fluid["eps"], 1)
    dev, spy = P.mesh.contents.device.contents, P.spy1x1.contents
    P.set_fluid_material()
    P.assemble_system(wg_d, dwg_d, F, want_J=True)                # allocates what the assemblies allocate once
    api.sync()
    val = L.MatrixFSBlockValues(P.J)

    def jac_correction():
        L.dfl_fluid_add_jacobian(N, vrow, vcol, C.cast(dev.ien, C.c_void_p), C.cast(dev.xg, C.c_void_p), wg_d.ptr,
                                 C.cast(spy.row_ptr, C.c_void_p), C.cast(spy.col_ind, C.c_void_p), C.byref(prm), val, L.DflStream())

    on = {"fluid_rows_r": lambda: L.DflMeshFluidRows(P.mesh, wg_d.ptr, dwg_d.ptr, r4.ptr, None, None),
          "fluid_rows_r_Rn_Mn": lambda: L.DflMeshFluidRows(P.mesh, wg_d.ptr, dwg_d.ptr, r4.ptr, rn.ptr, mn.ptr),
          "fluid_jacobian_correction": jac_correction,
          "thermal_rows_r": lambda: L.DflMeshThermalRows(P.mesh, wg_d.ptr, dwg_d.ptr, rn.ptr, None, None),
          "scalar_jacobian_material": lambda: L.DflAssembleScalarJacobian(P.mesh, wg_d.ptr, dwg_d.ptr, *sj)}
    off = {"assemble_F_off": lambda: P.assemble_system(wg_d, dwg_d, F, want_J=False),
           "assemble_J_off": lambda: P.assemble_system(wg_d, dwg_d, None, want_J=True)}
    t = {k: [] for k in list(on) + list(off)}
    for rep in range(a.warmup + a.reps):
        P.set_fluid_material(**fluid)                             # (synchronises: outside the timed calls)
        for k, fn in on.items():
            ms = timed(fn)
            if rep >= a.warmup:
                t[k].append(ms)
        P.set_fluid_material()
        for k, fn in off.items():
            ms = timed(fn)
            if rep >= a.warmup:
                t[k].append(ms)
    api.sync()
    rec["calls"] = {k: stats(v) for k, v in t.items()}
    c = {k: v["ms_mean"] for k, v in rec["calls"].items()}
    rec["ratios"] = {"rows_over_thermal_rows": c["fluid_rows_r"] / c["thermal_rows_r"],
                     "rows_over_assemble_F": c["fluid_rows_r"] / c["assemble_F_off"],
                     "jacobian_over_scalar_jacobian": c["fluid_jacobian_correction"] / c["scalar_jacobian_material"],
                     "jacobian_over_assemble_J": c["fluid_jacobian_correction"] / c["assemble_J_off"]}
    P.set_fluid_material(**fluid)
    L.DflMeshFluidRows(P.mesh, wg_d.ptr, dwg_d.ptr, r4.ptr, rn.ptr, mn.ptr)
    api.sync()
    rec["finite"] = bool(np.isfinite(r4.numpy()).all() and np.isfinite(rn.numpy()).all())
    rec["mean_density"] = float(rn.numpy().sum())                 # the cube has volume 1
    P.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
