"""The numpy model of the level-set redistancing (tests/redistance_model.py) against analysis; no GPU.

Planes are reproduced to rounding where the foot point lies inside the mesh (the surface ends at the mesh boundary), the
volume of a half space clipped by the unit cube has a closed form, a sphere converges at second order in h (the surface is
the piecewise-linear interpolant's zero set: its distance from the sphere is O(h^2 / R)), and the result depends on the zero
set of phi alone, not on its slope."""
import numpy as np
import pytest

import redistance_model as rm
from dedflow_amd.meshgen import kuhn_cube

LD = np.longdouble
TILT = np.array([0.2, -0.3, 1.0]) / np.sqrt(1.13)
CENTRE, R = np.array([0.55, 0.52, 0.46]), 0.3


def test_plane_is_reproduced_and_its_volume_is_exact():
    m = kuhn_cube(4, jitter=0.2)
    x = m.xg.reshape(-1, 3)
    band = 0.6
    for level in (0.0, 0.13):
        phi = (x - 0.5) @ TILT
        res = rm.redistance(m, phi, level, band)
        assert len(res["facets"]) > 0 and np.isfinite(res["phi"]).all()
        foot = x - (phi - level)[:, None] * TILT
        inside = ((foot >= 0.0) & (foot <= 1.0)).all(axis=1) & (np.abs(phi - level) < band)
        assert inside.sum() > 40
        err = np.abs(res["phi"] - phi)[inside].max()
        print(f"plane level {level}: {inside.sum()} nodes, max deviation {err:.2e}")
        assert err <= 1e-14
        # nodes whose foot point is outside see the surface's edge: farther, never nearer
        assert (np.abs(res["phi"] - level) >= np.abs(phi - level) - 1e-14)[np.abs(phi - level) < band].all()
        want = rm.clipped_cube_volume(TILT, level + 0.5 * TILT.sum())
        got = float(rm.volume(m.xg, m.ien, phi, level))
        print(f"  volume {got:.15f}, analytic {want:.15f}")
        assert abs(got - want) <= 1e-12
        if level == 0.0:
            assert abs(want - 0.5) <= 1e-15
        # the positive and the negative part make up every tet
        vp, full = rm.tet_volumes(m.xg, m.ien, phi, level)
        vn, _ = rm.tet_volumes(m.xg, m.ien, -phi, -level)
        assert np.abs(vp + vn - full).max() <= 1e-15
        assert abs(float(full.astype(LD).sum()) - 1.0) <= 1e-13


def _sphere(M):
    m = kuhn_cube(M, jitter=0.2)
    x = m.xg.reshape(-1, 3)
    return m, x, np.sqrt(((x - CENTRE) ** 2).sum(axis=1)) - R


_sphere_cache = {}


def sphere_errors(M):
    """node errors of the redistanced exact and deformed fields against the exact distance, over |exact| < band - h"""
    if M not in _sphere_cache:
        m, x, d = _sphere(M)
        h = 1.0 / M
        band = 3 * h
        near = np.abs(d) < band - h
        out = {}
        for name, phi in (("exact", d), ("deformed", d + 2 * d ** 3 / R ** 2 + 1.5 * d * (x[:, 0] - 0.5)), ("scaled", 3 * d)):
            res = rm.redistance(m, phi, 0.0, band)
            out[name] = dict(err=float(np.abs(res["phi"] - d)[near].max()), res=res, phi=phi)
        out["mesh"], out["d"], out["band"], out["near"] = m, d, band, near
        _sphere_cache[M] = out
    return _sphere_cache[M]


@pytest.mark.parametrize("field,measured", [("exact", 3.5), ("deformed", 3.2)])
def test_sphere_converges_at_second_order(field, measured):
    e6, e12 = sphere_errors(6)[field]["err"], sphere_errors(12)[field]["err"]
    assert sphere_errors(12)["near"].sum() > 500
    print(f"sphere {field}: error {e6:.4f} at M = 6, {e12:.4f} at M = 12, ratio {e6 / e12:.2f} (first order would give 2)")
    assert e6 / e12 >= 2.5


def test_result_does_not_depend_on_the_slope():
    s = sphere_errors(12)
    dev = np.abs(s["scaled"]["res"]["phi"] - s["exact"]["res"]["phi"]).max()
    print(f"3 d against d: {dev:.2e}")
    assert dev <= 1e-13
    assert len(s["scaled"]["res"]["facets"]) == len(s["exact"]["res"]["facets"])


def test_gradient_is_as_good_as_the_interpolated_distance():
    s = sphere_errors(12)
    m = s["mesh"]
    exact = rm.grad_dev(m.xg, m.ien, s["d"], 0.0)
    st = rm.stats(m, s["deformed"]["phi"], s["deformed"]["res"], 0.0)
    print(f"grad_dev: {st['grad_dev_before']:.3f} before, {st['grad_dev_after']:.3f} after, {exact:.3f} for the interpolated distance")
    assert st["grad_dev_after"] <= exact + 0.05
    assert st["grad_dev_before"] > st["grad_dev_after"]
    ball = 4.0 / 3.0 * np.pi * R ** 3
    assert abs((1.0 - st["volume_before"]) - ball) < 0.05 * ball and abs(st["volume_after"] - st["volume_before"]) < 0.02 * ball
    assert st["band_nodes"] > 0 and st["max_change"] > 0.0 and st["facets"] > 0


def test_node_layer_exactly_at_the_level():
    m = kuhn_cube(4)
    phi = m.xg.reshape(-1, 3)[:, 2] - 0.5
    band = 0.3
    res = rm.redistance(m, phi, 0.0, band)
    assert not np.isnan(res["phi"]).any()
    assert np.array_equal(res["phi"], np.clip(phi, -band, band))
    F = res["facets"]
    assert len(F) == 128 and not np.isnan(F).any()
    n = rm.cross(F[:, 3:6] - F[:, 0:3], F[:, 6:9] - F[:, 0:3])
    assert (rm.dot(n, n) > 0).sum() == 32                            # the 32 faces in the layer; the other 96 are edges and points
    assert np.abs(F[:, 2::3] - 0.5).max() == 0.0
    assert abs(float(rm.volume(m.xg, m.ien, phi, 0.0)) - 0.5) <= 1e-15   # (192 tets of 1/384 each, every one rounded once)


def test_level_nowhere_reached():
    m = kuhn_cube(3, jitter=0.2)
    phi = (m.xg.reshape(-1, 3) - 0.5) @ TILT
    res = rm.redistance(m, phi, 5.0, 0.25)
    assert len(res["facets"]) == 0 and np.array_equal(res["phi"], np.full(m.num_node, 4.75))
    st = rm.stats(m, phi, res, 5.0)
    assert all(v == 0 for v in st.values()), st
    up = rm.redistance(m, phi, -5.0, 0.25)
    assert np.array_equal(up["phi"], np.full(m.num_node, -4.75))


def test_a_nan_node_stays_and_spoils_nothing_else():
    m = kuhn_cube(4, jitter=0.2)
    phi = (m.xg.reshape(-1, 3) - 0.5) @ TILT
    clean = rm.redistance(m, phi, 0.0, 0.6)
    k = int(np.argmin(np.abs(phi)))                                  # a node next to the surface
    bad = phi.copy()
    bad[k] = np.nan
    res = rm.redistance(m, bad, 0.0, 0.6)
    assert np.isnan(res["phi"][k]) and np.isfinite(np.delete(res["phi"], k)).all()
    assert np.isnan(res["facets"]).any()                             # the facets of its tets hold NaN and never win
    far = np.abs(m.xg.reshape(-1, 3) - m.xg.reshape(-1, 3)[k]).max(axis=1) > 0.6
    assert far.any() and np.abs(res["phi"] - clean["phi"])[far].max() <= 1e-14
    st = rm.stats(m, bad, res, 0.0)
    assert all(np.isfinite(v) for v in st.values()), st


def test_refusals():
    assert rm.refusal(0.0, 0.1) is None
    assert rm.refusal(np.nan, 0.1) == "level" and rm.refusal(0.0, np.inf) == "band" and rm.refusal(0.0, 0.0) == "band"
    assert rm.refusal(0.0, 0.1, every=-1) == "every"


def test_longdouble_variant_agrees():
    s = sphere_errors(6)
    m = s["mesh"]
    ld = rm.redistance(m, s["deformed"]["phi"], 0.0, s["band"], dtype=LD)
    dev = float(np.abs(ld["phi"] - s["deformed"]["res"]["phi"].astype(LD)).max())
    print(f"float64 model against longdouble: {dev:.2e}")
    assert ld["phi"].dtype == LD and dev <= 1e-12
