"""CPU checks of the DEM contact friction and rotation: the numpy model (tests/friction_model.py) against closed forms of a
sphere on the unit-box floor and the conservation laws of an isolated pair, meshgen.dem_lattice, and the library's friction
entry points being exported (no compute calls: no GPU here)."""
import os
import subprocess

import numpy as np

import friction_model as fm
import walls_model as wm
from dedflow_amd.meshgen import dem_lattice, kuhn_cube

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 9.81
# a stiff floor (overlap ~1e-5 R: the lever R - delta is R to 1e-4) and damped springs (the transients die in ~0.05 s)
R, KN, GN, GT, DT = 0.05, 1.0e6, 200.0, 50.0, 1.0e-4


def _roll(theta, mu, steps, v0=(0.0, 0.0, 0.0), x0=0.2):
    """one sphere on the floor z = 0 under gravity tilted by theta about the y axis; returns t, v, w per step"""
    g = G * np.array([np.sin(theta), 0.0, -np.cos(theta)])
    z0 = R - G * np.cos(theta) / KN              # the equilibrium overlap
    m = fm.Model([[x0, 0.5, z0]], [v0], R, kn=KN, gn=GN, mu=mu, gamma_t=GT, dt=DT, gravity=g)
    t, v, w = [], [], []
    for k in range(steps):
        m.step()
        t.append((k + 1) * DT)
        v.append(m.v[0].copy())
        w.append(m.w[0].copy())
    return np.array(t), np.array(v), np.array(w), m


def _fit_acc(t, vx, t0):
    sel = t >= t0
    return np.polyfit(t[sel], vx[sel], 1)[0]


def test_rolling_down_an_incline():
    theta = np.radians(20.0)
    mu = 0.5                                     # >= 2/7 tan(theta) = 0.104: rolls
    t, v, w, m = _roll(theta, mu, 3000)
    a = _fit_acc(t, v[:, 0], 0.1)
    want = 5.0 / 7.0 * G * np.sin(theta)
    assert abs(a - want) <= 0.01 * want, (a, want)
    slip = v[-1] + np.cross(w[-1], [0.0, 0.0, -R])     # velocity of the contact point
    assert np.linalg.norm(slip) <= 0.01 * np.linalg.norm(v[-1]), (slip, v[-1])
    assert abs(v[-1, 1]) < 1e-12 and abs(w[-1, 0]) < 1e-12 and abs(w[-1, 2]) < 1e-12


def test_sliding_down_an_incline():
    theta = np.radians(20.0)
    mu = 0.05                                    # < 2/7 tan(theta): slides
    t, v, w, m = _roll(theta, mu, 3000)
    a = _fit_acc(t, v[:, 0], 0.1)
    want = G * (np.sin(theta) - mu * np.cos(theta))
    assert abs(a - want) <= 0.01 * want, (a, want)
    # still slipping, spinning up at the Coulomb torque
    assert v[-1, 0] - R * w[-1, 1] > 0.1 * v[-1, 0]


def test_launched_sphere_ends_rolling_at_five_sevenths():
    v0 = 1.0
    t, v, w, m = _roll(0.0, 0.3, 5000, v0=(v0, 0.0, 0.0))
    want = 5.0 / 7.0 * v0
    assert abs(v[-1, 0] - want) <= 0.01 * want, v[-1]
    assert abs(w[-1, 1] * R - want) <= 0.01 * want, w[-1]


def test_isolated_pair_conserves_momentum_and_angular_momentum():
    Rp = 0.06
    x = np.array([[0.45, 0.5, 0.5], [0.56, 0.53, 0.49]])
    v = np.array([[1.0, 0.2, 0.0], [-0.5, 0.0, 0.1]])
    w = np.array([[3.0, -1.0, 20.0], [0.0, 5.0, -2.0]])
    for mu in (0.5, 0.05):                       # sticking and sliding
        m = fm.Model(x, v, Rp, mass=2.0, kn=1.0e4, gn=1.0, mu=mu, dt=1.0e-4, w=w)
        p0, L0 = (m.mass * m.v).sum(axis=0), m.angular_momentum()
        spun = 0.0
        for _ in range(300):
            acc, alpha = m.step()
            spun = max(spun, np.abs(alpha).max())
        p1, L1 = (m.mass * m.v).sum(axis=0), m.angular_momentum()
        assert spun > 0.0 and np.abs(m.w - w).max() > 1e-3
        assert np.abs(p1 - p0).max() <= 1e-12 * np.abs(m.mass * v).sum()
        assert np.abs(L1 - L0).max() <= 1e-12 * np.abs(L0).max(), (L0, L1)


def test_pair_forces_are_opposite_and_torques_equal():
    Rp = 0.06
    x = np.array([[0.45, 0.5, 0.5], [0.55, 0.52, 0.49]])
    m = fm.Model(x, [[0.3, -1.0, 0.2], [0.0, 0.4, -0.1]], Rp, mu=0.3, w=[[1.0, 2.0, 3.0], [-4.0, 0.5, 0.0]])
    for _ in range(3):
        acc, alpha = m.step()
        assert np.array_equal(acc[0], -acc[1]) and np.array_equal(alpha[0], alpha[1])
        assert np.abs(alpha[0]).max() > 0.0


def test_mesh_floor_keeps_one_history_across_triangles():
    """on the floor of kuhn_cube(8), a face contact is keyed by its plane: the key stays the same over every triangle"""
    W = wm.Walls(kuhn_cube(8))
    keys = set()
    for px in np.linspace(0.1, 0.9, 23):
        m = fm.Model([[px, 0.37, 0.04]], [[0.0, 0.0, 0.0]], 0.05, W=W)
        m.forces()
        keys.update(m.hist[0].keys())
    assert len(keys) == 1
    (k,) = keys
    assert k >> 62 == 1 and np.allclose(W.n[k & ((1 << 62) - 1)], [0.0, 0.0, 1.0])


def test_dem_lattice():
    Rl = 0.05
    x = dem_lattice((0, 0, 0), (1, 1, 1), Rl)
    assert (x >= Rl - 1e-12).all() and (x <= 1 - Rl + 1e-12).all()
    d = np.linalg.norm(x[1] - x[0])
    assert abs(d - 1.9 * Rl) < 1e-12
    xf = dem_lattice((0, 0, 0), (1, 1, 1), Rl, kind="fcc", max_particles=100, jitter=0.01)
    assert xf.shape == (100, 3)


def test_library_exports_the_friction_entry_points():
    subprocess.check_call(["make", "-s", "-j8", "-C", ROOT])
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "dedflow_amd", "libdedflow.so")], text=True)
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in ("ParticleContextSetFriction", "ParticleContextAngularVelocity", "ParticleContextAngularAcc",
                 "ParticleContextFrictionOverflowCount", "ParticleContextSetGravity", "dfl_dem_build_cells",
                 "dfl_walls_build_cells", "dfl_dem_forces", "dfl_walls_forces",
                 "dfl_dem_integrate_spin", "dfl_dem_spin"):
        assert name in names, name
