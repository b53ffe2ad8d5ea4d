"""Inputs and raw outputs of every pass built from "count per workgroup -> scan -> emit in ascending order" or from the
fixed-tree workgroup reductions, on two small meshes: kuhn_cube(6, jitter=0.2) (1296 tets: five full workgroups and one of
16 tets) and fan_mesh (76 tets on one node).  Public Python API only, so the same file runs on any commit that has these
features; run on one commit it writes the fixtures another commit is compared with bit for bit
(tests/test_gpu_compaction_bits.py, fixtures under tests/golden/compaction/).

    python tools/dump_compaction_bits.py --out tests/golden/compaction --commit $(git rev-parse HEAD)

Per mesh one <name>.npz: the mesh, the state w and the particles (`mesh_*`, `in_*`; the sphere phi and the tanh temperature
of tools/dump_node_gather_bits.py), and
    out_redistance_phi / _facets / _stats   DflMeshRedistance: phi afterwards, the facet list, DflRedistanceStats in field order
    out_level_set_volume                    DflMeshLevelSetVolume at level 0
    out_volume_correct / _phi               DflMeshVolumeCorrect of phi + drift towards the volume of phi:
                                            DflVolumeCorrectionStats in field order (status, passes, band_tets, shift, target,
                                            the three volumes) and phi afterwards
    out_phase_stats                         DflMeshPhaseChangeStats: liquid_volume, T_max, molten, lo [3], hi [3]
    out_laser_surface_facets / _tets        the snapshot of ParticleContextLaserSurfaceUpdate
    out_laser_surface_power / _source / _rate / _tally
                                            after one laser step: the nodal surface power, the heat source (the substrate faces
                                            and the surface), the particles' rates and the six tally entries
cube6 only:
    out_dem_acc                             the accelerations of ParticleContextComputeForces for 2000 particles of R = 0.02 in
                                            the unit box: a 12^3-cell grid, 1729 scan entries, two scan chunks.  The cell order
                                            has no public accessor; the accelerations sum every particle's contacts in that
                                            order, so they carry it"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PHASE = dict(T_solidus=1600.0, T_liquidus=1700.0, latent=2.0e9, darcy_c=1.0e6, darcy_b=1e-3)
LEVEL, SIDE = 0.0, -1                                             # metal inside the sphere
NPART, MASS, CP_P = 300, 2.0e-3, 450.0
DEM_P, DEM_R = 2000, 0.02
LASER_DT = 1e-3
TALLY = ("outside", "absorbed_particles", "scattered", "substrate", "reflected", "missed")
MESH_FIELDS = ("M", "xg", "ien", "bound_node_offset", "bound_node", "bound_elem_offset", "bound_ien", "bound_f2e", "bound_forn")
SUBSTRATE = {"cube6": (4,), "fan": (0,)}                          # the z- faces of the cube; the fan's whole surface


def make_inputs(name):
    """mesh_* and in_* arrays of one case"""
    from dedflow_amd.meshgen import fan_mesh, kuhn_cube, synthetic_fields
    m = {"cube6": lambda: kuhn_cube(6, jitter=0.2), "fan": fan_mesh}[name]()
    N = m.num_node
    x = m.xg.reshape(-1, 3)
    lo, hi = x.min(axis=0), x.max(axis=0)
    c, ext = 0.5 * (lo + hi) + np.array([0.03, -0.02, 0.05]) * (hi - lo), (hi - lo).max()
    w, _ = synthetic_fields(m)
    r = np.linalg.norm(x - c, axis=1)
    w[4 * N:5 * N] = r - 0.3 * ext
    w[5 * N:] = 1650.0 + 300.0 * np.tanh((0.45 * ext - r) / (0.25 * ext))
    rng = np.random.default_rng(47)
    pts = lo + (0.02 + 0.96 * rng.uniform(size=(NPART, 3))) * (hi - lo)
    inp = {"mesh_" + k: np.asarray(getattr(m, k)) for k in MESH_FIELDS}
    inp.update(in_w=w, in_ext=np.float64(ext), in_pts=pts, in_substrate=np.array(SUBSTRATE[name], np.int32),
               in_laser_origin=np.array([c[0] + 0.013 * ext, c[1] - 0.007 * ext, hi[2] + 0.3 * ext]))
    if name == "cube6":
        inp.update(in_dem_x=rng.uniform(0.0, 1.0, size=(DEM_P, 3)), in_dem_v=rng.normal(0.0, 0.1, size=(DEM_P, 3)))
    return inp


def mesh_of(inp):
    from dedflow_amd.meshgen import TetMesh
    return TetMesh(**{k: (int(inp["mesh_M"]) if k == "M" else np.ascontiguousarray(inp["mesh_" + k])) for k in MESH_FIELDS})


def _fields(s):
    return np.array([float(v) for v in s.values()])


def run(api, inp):
    """every out_* array of one case, on a Problem and particle contexts of its own"""
    m = mesh_of(inp)
    N = m.num_node
    ext, w = float(inp["in_ext"]), inp["in_w"]
    out = {}
    P = api.Problem(m)
    try:
        w_d = api.DeviceArray.from_numpy(w)
        P.set_redistance(level=LEVEL, band=0.25 * ext)
        P.redistance(w_d)
        out["out_redistance_facets"] = P.redistance_facets()
        out["out_redistance_stats"] = _fields(P.redistance_stats())
        out["out_redistance_phi"] = w_d.numpy()[4 * N:5 * N]
        P.set_redistance()

        w_d = api.DeviceArray.from_numpy(w)
        V0 = P.level_set_volume(w_d, LEVEL)
        out["out_level_set_volume"] = np.array([V0])
        drift = w.copy()
        drift[4 * N:5 * N] += 0.01 * ext
        w_d = api.DeviceArray.from_numpy(drift)
        P.set_volume_correction(level=LEVEL, max_shift=0.03 * ext, tol=1e-10, target=V0)
        P.volume_correct(w_d)
        out["out_volume_correct"] = _fields(P.volume_correction_stats())
        out["out_volume_correct_phi"] = w_d.numpy()[4 * N:5 * N]
        P.set_volume_correction()

        w_d = api.DeviceArray.from_numpy(w)
        P.set_phase_change(**PHASE)
        s = P.phase_stats(w_d)
        out["out_phase_stats"] = np.concatenate([[s["liquid_volume"], s["T_max"], float(s["molten"])], s["lo"], s["hi"]])
        P.set_phase_change()

        pts = inp["in_pts"]
        pc = api.Particles(pts.reshape(-1), np.zeros(pts.size), 0.01 * ext, mass=MASS, dt=LASER_DT)
        try:
            pc.set_heat(cp_p=CP_P, T_init=300.0)
            pc.couple(P)
            pc.set_laser(inp["in_laser_origin"], (0.15, -0.1, -1.0), power=400.0, w=0.2 * ext, h=0.05 * ext, r_cut=0.4 * ext,
                         eta_p=0.35, eta_s=0.7, substrate_groups=[int(g) for g in inp["in_substrate"]])
            pc.set_laser_surface(LEVEL, SIDE)
            pc.laser_surface_update(w_d)
            out["out_laser_surface_facets"], out["out_laser_surface_tets"] = pc.laser_surface_facets()
            pc.laser_step(LASER_DT)
            out["out_laser_surface_power"] = pc.laser_surface_power().numpy()
            out["out_laser_surface_rate"] = pc.laser_rate()
            t = pc.laser_tally()
            out["out_laser_surface_tally"] = np.array([t[k] for k in TALLY])
            out["out_laser_surface_source"] = pc.heat_source().numpy()
        finally:
            pc.close()
    finally:
        P.close()
    if "in_dem_x" in inp:
        pc = api.Particles(inp["in_dem_x"].reshape(-1), inp["in_dem_v"].reshape(-1), DEM_R)
        try:
            pc.compute_forces()
            api.sync()
            out["out_dem_acc"] = pc.arrays()[2]
        finally:
            pc.close()
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
        again = run(api, inp)
        for k, v in out.items():
            assert same_bits(v, again[k]), k                      # a fixture must not hold what one commit cannot repeat
        nz = {k: (v.shape, int(np.count_nonzero(v))) for k, v in out.items()}
        path = os.path.join(a.out, name + ".npz")
        np.savez_compressed(path, commit=np.array(a.commit), **inp, **out)
        print(f"{path}: {os.path.getsize(path)} B, (shape, nonzeros) {nz}", flush=True)
        for k in ("out_redistance_stats", "out_level_set_volume", "out_volume_correct", "out_phase_stats", "out_laser_surface_tally"):
            print(" ", k, out[k].tolist(), flush=True)


if __name__ == "__main__":
    main()
