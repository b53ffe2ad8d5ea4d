"""CPU tests of the track cross-sections (include/dedflow.h, "track cross-sections"): the symbols, the library's host-only
configuration check, and the numpy model (tests/track_sections_model.py) against closed forms: the bead of a piecewise-linear
phi, and the area rule (everything metal and fused: the two areas add up to the area of the plane inside the cube)."""
import ctypes as C
import os

import numpy as np
import pytest

import track_sections_model as tm
from dedflow_amd.meshgen import kuhn_cube, single_tet

_cache = {}


def _cube(M):
    if M not in _cache:
        _cache[M] = kuhn_cube(M)
    return _cache[M]


def test_symbols_declared_and_exported():
    from dedflow_amd import api
    lib = api.lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pub = open(os.path.join(root, "include", "dedflow.h")).read()
    ker = open(os.path.join(root, "include", "dedflow_kernels.h")).read()
    for n in ("DflTrackSectionsCheck", "DflMeshSetTrackSections", "DflMeshTrackSectionsEnabled", "DflMeshTrackSectionsStations",
              "DflMeshTrackSections", "DflMeshTrackSectionsResult"):
        assert n in pub and hasattr(lib, n), n
    for n in ("dfl_track_count", "dfl_track_offsets", "dfl_track_emit", "dfl_track_eval"):
        assert n in ker and hasattr(lib, n), n
    assert hasattr(lib, "DflTrackSectionsTestPairs")
    for n in ("set_track_sections", "track_sections_on", "track_sections", "track_sections_result"):
        assert hasattr(api.Problem, n), n
    assert C.sizeof(api.DflTrackSections) == 9 * 8 + 8 + 64 * 8 + 8 + 8 + 8 + 8 and C.sizeof(api.DflTrackSection) == 11 * 8


def test_configuration_check():
    from dedflow_amd import api
    L = api.lib()
    why = C.create_string_buffer(200)

    def library(stations=(0.1, 0.2), **kw):
        cfg = api.track_sections_config(stations, **kw)
        return L.DflTrackSectionsCheck(C.byref(cfg), why, 200), why.value.decode()

    for good in (dict(), dict(stations=[0.5]), dict(stations=np.arange(64) / 64.0), dict(side=-1), dict(every=3),
                 dict(normal=(0, 0, 5.0), up=(1.0, 0, 2.0)), dict(T_fuse=-1e300), dict(stations=(-3.0, 0.0, 1e9))):
        assert library(**good)[0] == 0, good
    nan, inf = np.nan, np.inf
    for reason, bad in (("origin", dict(origin=(0, nan, 0))), ("normal", dict(normal=(inf, 0, 0))), ("up", dict(up=(0, 0, nan))),
                        ("normal", dict(normal=(0, 0, 0))), ("up", dict(up=(0, 0, 0))), ("up", dict(up=(2.0, 0, 0))),
                        ("up", dict(normal=(0, -4.0, 0), up=(0, 0.5, 0))),
                        ("num_station", dict(stations=())), ("num_station", dict(num_station=65)),
                        ("num_station", dict(num_station=-1)), ("station", dict(stations=(0.1, nan))),
                        ("station", dict(stations=(0.1, inf))), ("ascend", dict(stations=(0.2, 0.2))),
                        ("ascend", dict(stations=(0.1, 0.3, 0.2))), ("level", dict(level=nan)), ("side", dict(side=0)),
                        ("side", dict(side=2)), ("T_fuse", dict(T_fuse=nan)), ("T_fuse", dict(T_fuse=-inf)),
                        ("every", dict(every=-1))):
        rc, text = library(**bad)
        assert rc != 0 and reason in text, (reason, bad, text)


def test_frame():
    n, u, t = tm.frame(tm.config([0.0], normal=(1.0, 1.0, 0.0), up=(0.3, 0.0, 2.0)))
    for a in (n, u, t):
        assert abs(np.dot(a, a) - 1.0) <= 4e-16
    assert abs(np.dot(n, u)) <= 4e-16 and abs(np.dot(n, t)) <= 4e-16 and abs(np.dot(u, t)) <= 4e-16
    assert np.allclose(np.cross(u, n), t, atol=1e-16) and u[2] > 0
    n, u, t = tm.frame(tm.config([0.0]))
    assert (n == (1, 0, 0)).all() and (u == (0, 0, 1)).all() and (t == (0, 1, 0)).all()


@pytest.mark.parametrize("M", [4, 6, 10])
def test_bead_closed_forms(M):
    """1e-12 relative, of the closed form itself"""
    m = _cube(M)
    cfg, w, T_peak = tm.bead(m)
    res, lst, off = tm.evaluate(m, w, T_peak, cfg)
    assert len(res) == 4 and off[4] == lst.size and off[64] == lst.size
    for c, r in zip(cfg["stations"], res):
        assert r["pairs"] > 0
        for key, want in tm.BEAD.items():
            assert abs(r[key] - want) <= 1e-12 * abs(want), (M, c, key, r[key], want)
        for key in tm.AREAS:
            assert abs(float(r["ld"][key]) - r[key]) <= 1e-12 * r["area_scale"], (M, c, key)


def test_bead_without_a_peak_temperature_fuses_nothing():
    m = _cube(4)
    cfg, w, _ = tm.bead(m)
    for r in tm.evaluate(m, w, None, cfg)[0]:
        assert r["area_fused"] == 0.0 and r["depth"] == -np.inf and r["y_lo_fused"] == np.inf and r["dilution"] == 0.0
        assert abs(r["area_clad"] - 0.05) <= 1e-12 * 0.05


def test_side_minus_one_is_the_other_phase():
    """the complement of the bead in the plane: the areas of both sides add up to the upper and lower half of the square"""
    m = _cube(6)
    cfg, w, T_peak = tm.bead(m, stations=(0.3,))
    a = tm.evaluate(m, w, T_peak * 0.0 + 1e4, cfg)[0][0]
    b = tm.evaluate(m, w, T_peak * 0.0 + 1e4, dict(cfg, side=-1))[0][0]
    assert abs(a["area_clad"] + b["area_clad"] - 0.5) <= 1e-12 and abs(a["area_fused"] + b["area_fused"] - 0.5) <= 1e-12
    assert abs(b["height"] - 0.5) <= 1e-15 and abs(b["depth"] - 0.2) <= 1e-15   # the gas reaches h = 0.2 - 0.8 / 2 at the walls


@pytest.mark.parametrize("M", [4, 6])
def test_area_rule_axis_normal(M):
    m = _cube(M)
    stations = (0.0, 0.25, 0.3, 0.5, 0.75, 1.0) if M == 4 else (0.0, 1.0 / 6.0, 0.41, 0.5, 1.0)
    cfg, w, T_peak = tm.all_metal(m, stations)
    res, lst, off = tm.evaluate(m, w, T_peak, cfg)
    for c, r in zip(stations, res):
        want = 0.0 if c == 1.0 else 1.0
        assert abs(r["area_clad"] + r["area_fused"] - want) <= 1e-12, (c, r)
        assert abs(r["area_scale"] - want) <= 1e-12 and abs(r["area_clad"] - 0.5 * want) <= 1e-12
        if c == 1.0:
            assert r["pairs"] == 0 and r["height"] == -np.inf     # the far boundary sees nothing
        else:
            assert r["pairs"] > 0 and abs(r["height"] - 0.5) <= 1e-15 and abs(r["depth"] - 0.5) <= 1e-15
            assert r["y_lo_clad"] == 0.0 and r["y_hi_clad"] == 1.0 and r["y_lo_fused"] == 0.0 and r["y_hi_fused"] == 1.0
    # a station on a node plane sees the tets on its positive side, once
    k = stations.index(0.5)
    x = m.xg.reshape(-1, 3)[np.asarray(m.ien).reshape(-1, 4)[lst[off[k]:off[k + 1]]]][:, :, 0]
    assert (x >= 0.5).all() and (x > 0.5).any(axis=1).all()


def test_area_rule_oblique_normal():
    m = _cube(4)
    r2 = np.sqrt(2.0)
    cfg, w, T_peak = tm.all_metal(m, (0.0, 0.3, 0.5 / r2), normal=(1.0, 1.0, 0.0), origin=(0.5, 0.5, 0.5))
    res = tm.evaluate(m, w, T_peak, cfg)[0]
    for c, r in zip(cfg["stations"], res):
        want = r2 - 2.0 * c                         # the chord of the unit square at distance c from its diagonal, times 1
        assert abs(r["area_clad"] + r["area_fused"] - want) <= 1e-12 * r2, (c, r)
        assert abs(r["area_scale"] - want) <= 1e-12 * r2 and r["pairs"] > 0


def test_single_tet_vertex_edge_face():
    m = single_tet()
    w, T_peak = tm.state(4, 1.0), np.zeros(4)
    # n = e_x: c = 0 is the face x = 0 (the tet lies on its positive side: one pair, the cut is that face, area 1 / 2); c = 1 the
    # vertex (1, 0, 0) (nothing positive: no pair)
    cfg = tm.config((0.0, 0.5, 1.0), origin=(0, 0, 0.25), level=0.0, T_fuse=tm.ALL_FUSED)
    res = tm.evaluate(m, w, T_peak, cfg)[0]
    assert [r["pairs"] for r in res] == [1, 1, 0]
    assert abs(res[0]["area_scale"] - 0.5) <= 1e-15 and abs(res[1]["area_scale"] - 0.125) <= 1e-15
    assert abs(res[0]["area_clad"] + res[0]["area_fused"] - 0.5) <= 1e-15
    # n = (1, 1, 0) / sqrt 2 through the edge x = y = 0: the tet is on the positive side, the cut degenerates to that edge
    cfg = tm.config((0.0,), normal=(1.0, 1.0, 0.0), level=0.0, T_fuse=tm.ALL_FUSED)
    r = tm.evaluate(m, w, T_peak, cfg)[0][0]
    assert r["pairs"] == 1 and r["area_scale"] == 0.0 and r["area_clad"] == 0.0 and r["area_fused"] == 0.0


def test_nan_inputs_cost_only_their_share():
    m = _cube(4)
    cfg, w, T_peak = tm.bead(m, stations=(0.3,))
    clean = tm.evaluate(m, w, T_peak, cfg)[0][0]
    bad = w.copy()
    bad[4 * m.num_node + 62] = np.nan
    r = tm.evaluate(m, bad, T_peak, cfg)[0][0]
    for key in tm.AREAS + tm.EXTENTS:
        assert np.isfinite(r[key]), key
    assert r["area_clad"] <= clean["area_clad"] and r["area_scale"] <= clean["area_scale"]
