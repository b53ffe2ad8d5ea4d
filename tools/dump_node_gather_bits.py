"""Inputs and raw outputs of every pass that sums over the sorted V2E map or uses the level-set tet geometry, on two small
meshes: kuhn_cube(6, jitter=0.2) and fan_mesh (76 tets on one node).  Public Python API only, so the same file runs on any
commit that has these features; run on one commit it writes the fixtures another commit is compared with bit for bit
(tests/test_gpu_node_gather_bits.py, fixtures under tests/golden/node_gather/).

    python tools/dump_node_gather_bits.py --out tests/golden/node_gather --commit $(git rev-parse HEAD)

Per mesh one <name>.npz: the mesh, the state w / dw, the particle case and the configurations (`in_*`, `mesh_*`), and
    out_surface_load / _heat / _area        DflMeshSurfaceLoad, sphere field, all terms on
    out_phase_{D,H,G}, out_phase_phi_{D,H,G}  DflMeshPhaseCoefficients without and with use_phi
    out_scalar_phi / _T                     DflAssembleScalarJacobian (no transport set) under the synthetic velocity
    out_capture_tags / _rtet / _q_vol / _load / _q_heat
                                            the capture decision of 300 particles: the surviving tags (keep), the tet of every
                                            captured particle (-1: kept) and the deposits through their node sums
The *_FLAGS switches are read from the environment when a feature is set; the caller picks them."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SURFACE = dict(level=0.0, side=-1, sigma0=1.8, dsigma_dT=-4e-4, T_ref=1900.0, recoil_p0=1.0e5, recoil_a=11.0, T_boil=3100.0,
               h_conv=80.0, emissivity=0.4, T_amb=300.0, evap_q0=2.0e9)
PHASE = dict(T_solidus=1600.0, T_liquidus=1700.0, latent=2.0e9, darcy_c=1.0e6, darcy_b=1e-3)
CAPTURE = dict(level=0.0, side=-1, reach=1.0, T_melt=1650.0)
NPART, RADIUS, MASS, RHO_F, CP_P = 300, 0.01, 2.0e-3, 1.0e3, 450.0
MESH_FIELDS = ("M", "xg", "ien", "bound_node_offset", "bound_node", "bound_elem_offset", "bound_ien", "bound_f2e", "bound_forn")


def make_inputs(name):
    """mesh_* and in_* arrays of one case"""
    from dedflow_amd.meshgen import fan_mesh, kuhn_cube, synthetic_fields
    m = {"cube6": lambda: kuhn_cube(6, jitter=0.2), "cube4": lambda: kuhn_cube(4, jitter=0.2), "fan": fan_mesh}[name]()
    N = m.num_node
    x = m.xg.reshape(-1, 3)
    lo, hi = x.min(axis=0), x.max(axis=0)
    c, ext = 0.5 * (lo + hi) + np.array([0.03, -0.02, 0.05]) * (hi - lo), (hi - lo).max()
    w, dw = synthetic_fields(m)
    r = np.linalg.norm(x - c, axis=1)
    w[4 * N:5 * N] = r - 0.3 * ext                                # a sphere: metal (side -1) inside it
    # liquid centre, a wide mushy shell (on fan_mesh every surface node lies in it) and a solid rim
    w[5 * N:] = 1650.0 + 300.0 * np.tanh((0.45 * ext - r) / (0.25 * ext))
    rng = np.random.default_rng(31)
    pts = lo + (0.02 + 0.96 * rng.uniform(size=(NPART, 3))) * (hi - lo)
    vel = rng.normal(0.0, 0.3, size=(NPART, 3))
    temp = rng.uniform(300.0, 2500.0, size=NPART)
    inp = {"mesh_" + k: np.asarray(getattr(m, k)) for k in MESH_FIELDS}
    inp.update(in_w=w, in_dw=dw, in_eps=np.float64(0.25 * ext), in_pts=pts, in_vel=vel, in_temp=temp)
    return inp


def mesh_of(inp):
    from dedflow_amd.meshgen import TetMesh
    return TetMesh(**{k: (int(inp["mesh_M"]) if k == "M" else np.ascontiguousarray(inp["mesh_" + k])) for k in MESH_FIELDS})


def run(api, inp):
    """every out_* array of one case, on a Problem and a particle context of its own"""
    m = mesh_of(inp)
    eps = float(inp["in_eps"])
    out = {}
    P = api.Problem(m)
    try:
        w_d, dw_d = api.DeviceArray.from_numpy(inp["in_w"]), api.DeviceArray.from_numpy(inp["in_dw"])
        P.set_surface_forces(eps=eps, **SURFACE)
        for k, a in P.surface_load(w_d).items():
            api.sync()
            out["out_surface_" + k] = a.numpy()
        for tag, extra in (("phase_", {}), ("phase_phi_", dict(use_phi=True, level=0.0, side=-1, eps=eps))):
            P.set_phase_change(**dict(PHASE, **extra))
            for k, a in P.phase_coefficients(w_d).items():
                api.sync()
                out["out_" + tag + k] = a.numpy()
        P.set_phase_change()
        P.set_surface_forces()
        out["out_scalar_phi"], out["out_scalar_T"] = P.assemble_scalar_jacobian(w_d, dw_d)
        pc = api.Particles(inp["in_pts"].reshape(-1), inp["in_vel"].reshape(-1), RADIUS, mass=MASS)
        try:
            pc.couple(P, rho_f=RHO_F, mu_f=1.0e-2)
            pc.set_heat(cp_p=CP_P, T_init=0.0)
            pc.set_temperature(inp["in_temp"])
            pc.set_capture(**CAPTURE)
            pc.locate()
            api.sync()
            tet = pc.tet()
            pc.capture(w_d)
            api.sync()
            tags = pc.tags()
            rtet = tet.copy()
            rtet[tags] = -1
            q = pc.capture_source(0.05)
            api.sync()
            out.update(out_capture_tags=tags, out_capture_rtet=rtet, out_capture_q_vol=q[0].numpy(), out_capture_load=q[1].numpy(),
                       out_capture_q_heat=q[2].numpy())
        finally:
            pc.close()
    finally:
        P.close()
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--commit", required=True, help="hash of the commit the library was built from; stored in every file")
    ap.add_argument("--cases", nargs="+", default=["cube6", "fan"])
    a = ap.parse_args()
    from dedflow_amd import api
    api.lib()
    os.makedirs(a.out, exist_ok=True)
    for name in a.cases:
        inp = make_inputs(name)
        out = run(api, inp)
        for k, v in out.items():
            assert v.dtype.kind != "f" or np.isfinite(v).all(), k
        nz = {k: int(np.count_nonzero(v)) for k, v in out.items()}
        path = os.path.join(a.out, name + ".npz")
        np.savez_compressed(path, commit=np.array(a.commit), **inp, **out)
        print(f"{path}: {os.path.getsize(path)} B, nonzeros {nz}", flush=True)


if __name__ == "__main__":
    main()
