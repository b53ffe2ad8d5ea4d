"""CPU checks of the solid-surface contact: the properties of the case generators of tests/surface_contact_model.py that the
GPU tests rely on, the model against the closed-form plane-wall law of tests/walls_model.py, and DflSurfaceContactCheck
(host only: no GPU is touched)."""
import numpy as np
import pytest

import capture_model as cm
import surface_contact_model as sm
from dedflow_amd.meshgen import kuhn_cube

KN, GN = 1.0e4, 3.0


def _decide(m, case, w, poly, side, T_solid=sm.T_SOLID):
    tet, lam = cm.brute_locate(m.xg, m.ien, case["pts"])
    return sm.decide(m.xg, m.ien, w, tet, lam, case["r"] if poly else case["R"], sm.LEVEL, side, T_solid), tet


@pytest.mark.parametrize("poly", [False, True], ids=["mono", "poly"])
@pytest.mark.parametrize("side", [1, -1], ids=["above", "below"])
@pytest.mark.parametrize("P", [63, 65, 257, 300])
def test_plane_cases_have_margins_and_every_class(P, side, poly):
    m = kuhn_cube(3)
    case = sm.plane_case(P, poly)
    dec, tet = _decide(m, case, sm.plane_fields(m.xg, side), poly, side)
    assert sm.margins_ok(dec, sm.T_SOLID)
    cls = sm.classify(dec, sm.T_SOLID)
    want = np.arange(P) % 6
    want[want == 5] = 0
    want[5] = 5
    assert np.array_equal(cls, want)                                   # every particle in the class it was placed in
    assert set(cls) == set(range(6)) and tet[5] == -1
    # the plane's gradient is arbitrary, not 1, and s is the geometric distance to the plane all the same
    loc = dec["located"]
    assert np.allclose(dec["gn"][loc].astype(float), sm.PLANE_G, rtol=1e-12)
    dist = (case["pts"] - 0.5) @ sm.PLANE_DIR
    assert np.abs(dec["s"][loc].astype(float) - dist[loc]).max() < 1e-13


def test_a_single_particle_is_a_contact():
    m = kuhn_cube(3)
    case = sm.plane_case(1, False)
    dec, _ = _decide(m, case, sm.plane_fields(m.xg, 1), False, 1)
    assert sm.margins_ok(dec, sm.T_SOLID) and dec["contact"].all()


@pytest.mark.parametrize("side", [1, -1], ids=["above", "below"])
def test_sphere_case_has_margins_and_every_class(side):
    m = kuhn_cube(4)
    case = sm.sphere_case(300, True, R=0.04)
    w = sm.sphere_fields(m.xg, side)
    dec, _ = _decide(m, case, w, True, side)
    assert sm.margins_ok(dec, sm.T_SOLID)
    cls = sm.classify(dec, sm.T_SOLID)
    assert set(cls) == set(range(6)) and min(np.bincount(cls)[:5]) >= 8
    # not linear: the gradient differs from tet to tet, and is no unit vector
    gn = dec["gn"][dec["located"]].astype(float)
    assert gn.max() - gn.min() > 0.05


@pytest.mark.parametrize("side", [1, -1], ids=["above", "below"])
def test_plane_force_is_the_plane_wall_law(side):
    """for a plane the model's frictionless force is the face contact of walls_model with the same plane, delta and normal,
    to the rounding of the double-precision wall model"""
    m = kuhn_cube(3)
    case = sm.plane_case(300, True)
    dec, _ = _decide(m, case, sm.plane_fields(m.xg, side), True, side)
    F, tau, xi, fn = sm.forces(dec, case["vel"], case["m"], KN, GN)
    assert not tau.any() and all(x is None for x in xi)
    hit = 0
    for i in range(300):
        f, contacts = sm.plane_wall_force(case["pts"][i], case["vel"][i], case["r"][i], KN, GN)
        touching = len(contacts) == 1
        # the wall model has no temperature and no mesh: it touches wherever -r < s < r
        assert touching == bool(dec["contact"][i] or (sm.classify(dec, sm.T_SOLID)[i] in (4, 5) and abs((case["pts"][i] - 0.5) @ sm.PLANE_DIR) < case["r"][i]))
        if dec["contact"][i]:
            # s comes from coordinates and nodal phi of size O(1) held in doubles: its rounding is eps O(1), not eps r
            scale = KN * (1.0 + 2 * case["r"][i]) + GN * np.linalg.norm(case["vel"][i])
            assert np.abs(F[i].astype(float) - f).max() <= 64 * sm.EPS * scale
            assert abs(contacts[0][2] - float(dec["delta"][i])) <= 64 * sm.EPS
            hit += 1
        else:
            assert not F[i].any()
    assert hit > 60


def test_friction_adds_a_tangential_force_and_a_torque():
    m = kuhn_cube(3)
    case = sm.plane_case(65, False)
    dec, _ = _decide(m, case, sm.plane_fields(m.xg, 1), False, 1)
    law = dict(mu=0.4, kt=2.0 / 7.0 * KN, gamma_t=GN, dt=1e-5)
    F0, _, _, fn = sm.forces(dec, case["vel"], case["mass"], KN, GN)
    F, tau, xi, _ = sm.forces(dec, case["vel"], case["mass"], KN, GN, friction=law, omega=case["omega"])
    for i in np.nonzero(dec["contact"])[0]:
        Ft = (F[i] - F0[i]).astype(float)
        n = dec["n"][i].astype(float)
        assert abs(Ft @ n) <= 1e-9 * np.linalg.norm(Ft) and np.linalg.norm(Ft) <= 0.4 * max(float(fn[i]), 0.0) * (1 + 1e-12) + 1e-300
        assert abs(tau[i].astype(float) @ n) <= 1e-9 * (np.linalg.norm(tau[i].astype(float)) + 1e-300) and xi[i] is not None
    assert not F[~dec["contact"]].any() and not tau[~dec["contact"]].any()


def test_what_is_no_contact():
    """tets -1 and -2, a NaN anywhere, a constant phi, T_solid = -inf; T_solid = +inf collides the hot class too"""
    m = kuhn_cube(3)
    N = m.num_node
    case = sm.plane_case(300, False)
    w = sm.plane_fields(m.xg, 1)
    tet, lam = cm.brute_locate(m.xg, m.ien, case["pts"])
    base = sm.decide(m.xg, m.ien, w, tet, lam, case["R"], sm.LEVEL, 1, sm.T_SOLID)
    for bad in (-1, -2):
        t2 = tet.copy()
        t2[base["contact"]] = bad
        d = sm.decide(m.xg, m.ien, w, t2, lam, case["R"], sm.LEVEL, 1, sm.T_SOLID)
        assert not d["contact"].any() and not d["buried"][base["contact"]].any()
    d = sm.decide(m.xg, m.ien, w, tet, lam, case["R"], sm.LEVEL, 1, -np.inf)
    assert not d["contact"].any() and not d["buried"].any()
    d = sm.decide(m.xg, m.ien, w, tet, lam, case["R"], sm.LEVEL, 1, np.inf)
    hot = sm.classify(base, sm.T_SOLID) == 4
    assert d["contact"][hot].any() and np.array_equal(d["contact"][~hot], base["contact"][~hot])
    ien4 = m.ien.reshape(-1, 4)
    for field in (4, 5):
        node = int(ien4[tet[np.nonzero(base["contact"])[0][0]], 0])
        w2 = w.copy()
        w2[field * N + node] = np.nan
        d = sm.decide(m.xg, m.ien, w2, tet, lam, case["R"], sm.LEVEL, 1, sm.T_SOLID)
        touched = (ien4[np.where(tet >= 0, tet, 0)] == node).any(axis=1) & (tet >= 0)
        assert touched.any() and not d["contact"][touched].any() and not d["buried"][touched].any()
        assert np.array_equal(d["contact"][~touched], base["contact"][~touched])
    w2 = w.copy()
    w2[4 * N:5 * N] = sm.LEVEL - 0.001
    d = sm.decide(m.xg, m.ien, w2, tet, lam, case["R"], sm.LEVEL, 1, sm.T_SOLID)
    assert not (d["gn"][d["located"]] > 0).any() and not d["contact"].any() and not d["buried"].any()


def test_check_accepts_and_refuses_what_the_header_says():
    from dedflow_amd import api
    ok = api.surface_contact_check
    assert ok(0.0, 1, np.inf) is None and ok(-3.5, -1, 1700.0) is None and ok(0.0, 1, -np.inf) is None
    for side in (0, 2, -2):
        assert "side" in ok(0.0, side, 1.0)
    for level in (np.nan, np.inf, -np.inf):
        assert "level" in ok(level, 1, 1.0)
    assert "T_solid" in ok(0.0, -1, np.nan)
    assert sm.KEY_SURFACE == (1 << 62) | (1 << 61) and sm.KEY_SURFACE >> 62 == 1 and sm.KEY_SURFACE & ((1 << 31) - 1) == 0
