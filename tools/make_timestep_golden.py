"""Writes tests/golden/timestep_default_bits.json: the sha256 of what the assembly kernels and the driver compute at the
default time step on a Kuhn cube of M = 4, with the `hipcc --version` string of the build.  It uses only the interface that
existed before the time step became a run-time value, so it can be run on the commit before that change; the test
tests/test_gpu_timestep.py::test_bits_of_the_parent recomputes the same hashes (it imports `collect` from here).

    python tools/make_timestep_golden.py [out.json]
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

THERMAL = dict(k_gas=0.02, k_solid=30.0, k_liquid=45.0, c_gas=1.2e3, c_metal=4.0e6, T_solidus=1600.0, T_liquidus=1700.0,
               use_phi=True, level=0.05, side=1, eps=0.3)
FLUID = dict(rho_gas=1.2, rho_metal=7.8e3, mu_gas=2e-5, mu_metal=6e-3, gravity=(0.0, 0.0, -9.81), beta=1e-4, T_ref=1650.0,
             use_phi=True, level=0.05, side=1, eps=0.3)
PHASE = dict(T_solidus=1600.0, T_liquidus=1700.0, latent=2.0e9, darcy_c=1.0e6)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def compiler_string():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    try:
        return subprocess.run([hipcc, "--version"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return "unknown"


def fields(m):
    """alpha-level states with a velocity field, phi through the mesh and T through the melting range"""
    from dedflow_amd.meshgen import synthetic_fields
    N = m.num_node
    wg, dwg = synthetic_fields(m)
    x = m.xg.reshape(-1, 3)
    wg[4 * N:5 * N] = (x - 0.5) @ np.array([0.3, 0.1, -1.0]) / np.sqrt(1.1)
    wg[5 * N:] = 1650.0 + 120.0 * ((x - 0.5) @ np.array([0.2, -0.3, 1.0]))
    return wg, dwg


def _system(api, P, wg, dwg):
    """F and the block values of J of one AssembleSystem"""
    wg_d, dwg_d = api.DeviceArray.from_numpy(wg), api.DeviceArray.from_numpy(dwg)
    F_d = api.DeviceArray(6 * P.N)
    P.assemble_system(wg_d, dwg_d, F_d, want_J=True)
    api.sync()
    return F_d.numpy(), P.block_values().numpy()


def collect(api, configure=None):
    """name -> sha256.  configure(P) is applied to every Problem right after it is made (the test passes the time-step setter)"""
    from dedflow_amd.meshgen import kuhn_cube, synthetic_fields
    configure = configure or (lambda P: None)
    m = kuhn_cube(4, jitter=0.2)
    N = m.num_node
    wg, dwg = fields(m)
    out = {}
    for sched in (0, 1, 4):
        P = api.Problem(m, schedule=sched)
        configure(P)
        F, J = _system(api, P, wg, dwg)
        out[f"F_s{sched}"], out[f"J_s{sched}"] = sha(F), sha(J)
        if sched == 4:
            vp, vt = P.assemble_scalar_jacobian(api.DeviceArray.from_numpy(wg), api.DeviceArray.from_numpy(dwg))
            out["Jphi"], out["JT"] = sha(vp), sha(vt)
        P.close()
    for name, setter, cfg in (("fluid", "set_fluid_material", FLUID), ("thermal", "set_thermal_material", THERMAL),
                              ("phase", "set_phase_change", PHASE)):
        P = api.Problem(m)
        configure(P)
        getattr(P, setter)(**cfg)
        F, J = _system(api, P, wg, dwg)
        out[f"F_{name}"], out[f"J_{name}"] = sha(F), sha(J)
        if name == "thermal":
            _, vt = P.assemble_scalar_jacobian(api.DeviceArray.from_numpy(wg), api.DeviceArray.from_numpy(dwg))
            out["JT_thermal"] = sha(vt)
        P.close()
    # two steps of the driver with scalar transport on
    wgold, dwgold = synthetic_fields(m)
    P = api.Problem(m)
    configure(P)
    P.set_scalar_transport()
    d = [api.DeviceArray.from_numpy(a) for a in (wgold, dwgold, dwgold.copy())]
    F_d, dx_d = api.DeviceArray(6 * N), api.DeviceArray(6 * N)
    for _ in range(2):
        P.time_step(d[0], d[1], d[2], F_d, dx_d, newton_maxit=2)
    api.sync()
    out["wgold_2steps"], out["dwgold_2steps"] = sha(d[0].numpy()), sha(d[1].numpy())
    P.close()
    return out


def main():
    from dedflow_amd import api
    api.lib()
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "timestep_default_bits.json")
    doc = {"mesh": "kuhn_cube(4, jitter=0.2)", "hipcc_version": compiler_string(), "sha256": collect(api)}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
