"""CPU checks of the particle-fluid coupling model (tests/coupling_model.py) and of the library's coupling entry points
being exported (no compute calls: there is no GPU here)."""
import ctypes
import os
import subprocess

import numpy as np

import coupling_model as cm
from dedflow_amd.meshgen import fan_mesh, kuhn_cube

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_inside(m, n, seed):
    """n points inside random tets of m, with the tets and the barycentric coordinates used to place them"""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, m.num_tet, n)
    lam = rng.dirichlet(np.ones(4), n)
    x = m.xg.reshape(-1, 3)[m.ien.reshape(-1, 4)[t]]
    return np.einsum("na,nad->nd", lam, x), t, lam


def test_barycentric_sum_to_one_and_recover_placement():
    for m in (kuhn_cube(4, jitter=0.2), fan_mesh()):
        p, t, lam = _random_inside(m, 500, 3)
        got = cm.barycentric(m.xg, m.ien, t, p)
        assert np.abs(got.sum(axis=1) - 1.0).max() < 1e-14
        assert np.abs(got - lam).max() < 1e-12
        assert cm.contains(m.xg, m.ien, t, p).all()


def test_brute_force_location():
    m = kuhn_cube(3, jitter=0.2)
    p, t, _ = _random_inside(m, 200, 4)
    found = cm.locate_brute(m.xg, m.ien, p)
    assert (found >= 0).all() and cm.contains(m.xg, m.ien, found, p).all()
    out = np.array([[1.5, 0.5, 0.5], [-0.1, 0.2, 0.3], [0.5, 0.5, 1.0 + 1e-9]])
    assert (cm.locate_brute(m.xg, m.ien, out) == -1).all()


def test_affine_fields_are_reproduced():
    m = kuhn_cube(4, jitter=0.2)
    rng = np.random.default_rng(5)
    a, B = rng.normal(size=3), rng.normal(size=(3, 3))
    x = m.xg.reshape(-1, 3)
    w = np.zeros(6 * m.num_node)
    w[: 3 * m.num_node] = (a[None, :] + x @ B.T).reshape(-1)
    p, t, _ = _random_inside(m, 300, 6)
    lam = cm.barycentric(m.xg, m.ien, t, p)
    uf = cm.interpolate(w, m.ien, t, lam)
    assert np.abs(uf - (a[None, :] + p @ B.T)).max() < 1e-13


def test_implicit_drag_is_bounded_and_settles_at_the_fixed_point():
    mass, R = 0.05, 0.01
    g = np.array([0.0, 0.0, -9.81])
    tau = cm.response_time(mass, R)
    # dt >> tau: the implicit update lands on u_f without overshoot
    uf = np.array([[1.0, -2.0, 0.5]])
    x, v = np.zeros((1, 3)), np.array([[-3.0, 4.0, 0.0]])
    for _ in range(30):
        x, v, _, _ = cm.drag_step(x, v, np.zeros((1, 3)), uf, [True], mass, R, 1e3 * tau)
    assert np.abs(v - uf).max() < 1e-10
    # settling in a fluid at rest
    vt = cm.terminal_velocity(mass, R, g)
    rho_p = cm.particle_density(mass, R)
    re_t = cm.RHO_F * np.linalg.norm(vt) * 2 * R / cm.MU_F
    assert np.allclose(vt, (1 - cm.RHO_F / rho_p) * g * tau / cm.schiller_naumann(re_t), rtol=1e-14, atol=0)
    v = np.zeros((1, 3))
    for _ in range(400):
        x, v, _, _ = cm.drag_step(x, v, np.zeros((1, 3)), np.zeros((1, 3)), [True], mass, R, 0.2 * tau, gravity=g)
    assert np.abs(v[0] - vt).max() <= 1e-10 * np.abs(vt).max()


def test_scatter_conserves_momentum():
    m = kuhn_cube(4, jitter=0.2)
    p, t, _ = _random_inside(m, 400, 7)
    lam = cm.barycentric(m.xg, m.ien, t, p)
    imp = np.random.default_rng(8).normal(size=(400, 3))
    load = cm.node_scatter(m.num_node, m.ien, t, lam, imp, 0.25).reshape(-1, 3)
    assert np.allclose(load.sum(axis=0), -imp.sum(axis=0) / 0.25, rtol=1e-12, atol=1e-12)


def test_library_exports_the_coupling_entry_points():
    subprocess.check_call(["make", "-s", "-j8", "-C", ROOT])
    lib = ctypes.CDLL(os.path.join(ROOT, "dedflow_amd", "libdedflow.so"))
    for name in ("ParticleContextSetFluidCoupling", "ParticleContextLocate", "ParticleContextTet", "ParticleContextBarycentric",
                 "ParticleContextLostCount", "ParticleContextFluidStep", "ParticleContextReactionLoad", "DflMeshSetExternalLoad",
                 "dfl_couple_locate", "dfl_couple_fluid_step", "dfl_couple_node_load"):
        assert hasattr(lib, name), name
