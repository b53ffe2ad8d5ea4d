"""The model of the laser on the level-set surface (tests/laser_surface_model.py) against analysis on a plane, the exported
symbols, and the condition the GPU tests put on their inputs -- all without a GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import laser_model as lm
import laser_surface_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS, LD = sm.EPS, sm.LD
NONE = np.zeros((0, 3))


@pytest.fixture(scope="module")
def m():
    return sm.mesh()


def _plane(m, name, scale=1.0):
    """the tilted plane of the GPU tests; scale != 1: phi - level scaled (exactly, by a power of two) about level 0"""
    kw = sm.beam_args(name)
    b = lm.Beam(**kw)
    phi, level = sm.plane_phi(m.xg), sm.PLANE_LEVEL
    if scale != 1.0:
        phi, level = scale * (phi - level), 0.0
    cand = sm.Candidates(m.xg, m.ien, phi, level, sm.SIDE, b.dir)
    return b, cand, sm.step(b, NONE, 0.0, cand=cand)


@pytest.mark.parametrize("name", sorted(sm.DIRECTIONS))
def test_plane_every_ray_that_meets_the_plane_inside_the_mesh_hits(m, name):
    b, cand, o = _plane(m, name)
    assert len(cand.tet) == 138                                     # every facet of the plane faces the beam
    o0 = b.at(0.0)
    cu, cv = b.centres()
    # the centre ray o + cu e1 + cv e2 + s dir meets n . (x - 1/2) = level at s
    base = o0[None, :] + cu[:, None] * b.e1[None, :] + cv[:, None] * b.e2[None, :]
    s = (sm.PLANE_LEVEL - (base - 0.5) @ sm.PLANE_N) / (b.dir @ sm.PLANE_N)
    x = base + s[:, None] * b.dir[None, :]
    margin = np.minimum(x, 1.0 - x).min(axis=1)                     # > 0: inside the unit cube (its boundary is not jittered)
    assert np.abs(margin).min() > 1e-9                              # no ray meets the plane on the mesh's boundary
    assert np.array_equal(o["surf"], margin > 0.0)
    assert o["surf"].sum() == {"vertical": 256, "oblique": 240}[name]
    depth = o["hit"][2]
    assert np.abs(depth[o["surf"]].astype(float) - s[o["surf"]]).max() < 1e-13
    assert (o["face"][o["surf"]] == -2 - cand.tet[o["facet"][o["surf"]]]).all() and (o["face"][~o["surf"]] == -1).all()


@pytest.mark.parametrize("name", sorted(sm.DIRECTIONS))
def test_plane_weights_sum_to_one_and_the_nodes_get_the_substrate_tally(m, name):
    b, cand, o = _plane(m, name)
    lam = o["lam"][o["surf"]]
    assert (lam >= -8 * EPS).all() and np.abs(lam.sum(axis=1) - 1).max() < 8 * EPS
    total = sum(o["power"].values())
    assert abs(total - o["tally"]["substrate"]) <= 8 * b.ncol * EPS * b.power
    assert abs(lm.tally_sum(o["tally"]) - b.power) <= 8 * b.ncol * EPS * b.power
    assert o["tally"]["missed"] > 0 if name == "oblique" else o["tally"]["missed"] == 0
    # the hit point is sum_a lambda_a x_a: it lies on the centre ray
    cu, cv = b.centres()
    for c in np.nonzero(o["surf"])[0][::17]:
        p = (o["lam"][c][:, None] * m.xg.reshape(-1, 3)[cand.nodes[o["facet"][c]]].astype(LD)).sum(axis=0)
        u, v, _ = b.project(p.astype(float), b.at(0.0))
        assert abs(u[0] - cu[c]) < 1e-12 and abs(v[0] - cv[c]) < 1e-12


@pytest.mark.parametrize("name", sorted(sm.DIRECTIONS))
def test_scaling_phi_minus_level_by_four_changes_no_bit(m, name):
    b, c1, o1 = _plane(m, name, scale=1.0)
    _, c4, o4 = _plane(m, name, scale=4.0)                          # f = phi - level is the same float64, times 4 exactly
    for k in ("F", "tet", "i", "j", "t"):
        assert np.array_equal(getattr(c1, k), getattr(c4, k))
    assert np.array_equal(o1["face"], o4["face"]) and np.array_equal(o1["lam"], o4["lam"])
    assert o1["power"] == o4["power"] and o1["tally"] == o4["tally"]


def test_gradient_filter_and_nan(m):
    b = lm.Beam(**sm.beam_args("vertical"))
    phi = sm.plane_phi(m.xg)
    assert len(sm.Candidates(m.xg, m.ien, phi, sm.PLANE_LEVEL, +1, b.dir).tet) == 0      # the beam leaves the metal everywhere
    full = sm.Candidates(m.xg, m.ien, phi, sm.PLANE_LEVEL, sm.SIDE, b.dir)
    bad = phi.copy()
    node = int(full.nodes[0, 0])
    bad[node] = np.nan
    cut = sm.Candidates(m.xg, m.ien, bad, sm.PLANE_LEVEL, sm.SIDE, b.dir)
    touched = (np.asarray(m.ien).reshape(-1, 4) == node).any(axis=1)
    assert not touched[cut.tet].any() and np.isfinite(cut.F).all() and np.isfinite(cut.t).all()
    assert np.array_equal(cut.tet, full.tet[~touched[full.tet]])
    two = sm.Candidates(m.xg, m.ien, sm.two_layer_phi(m.xg), 0.0, sm.SIDE, b.dir)
    import redistance_model as rm
    every = rm.facets(m.xg, m.ien, sm.two_layer_phi(m.xg), 0.0)[1]
    assert 0 < len(two.tet) < len(every) and np.isin(two.tet, every).all()                 # the slab's underside is not entered
    assert sm.refusal(True, True, 0.0, 2) == "side" and sm.refusal(True, True, np.inf, 1) == "level"
    assert sm.refusal(False, True, 0.0, 1) == "laser" and sm.refusal(True, False, 0.0, 1) == "coupling"
    assert sm.refusal(True, True, 0.0, -1) is None


@pytest.mark.parametrize("name", sorted(sm.DIRECTIONS))
def test_the_gpu_tests_inputs_keep_every_centre_off_the_edges(m, name):
    """the condition of test_gpu_laser_surface.py: every hit column's centre lies more than 1e-9 from every projected
    candidate edge (so no decision hangs on a rounding), and on the two-layer field at least two entering candidates lie
    under every hit column"""
    b = lm.Beam(**sm.beam_args(name))
    sub = lm.Substrate(m, [4], b)
    for phi, level, hits in ((sm.plane_phi(m.xg), sm.PLANE_LEVEL, {"vertical": 256, "oblique": 240}[name]),
                             (sm.two_layer_phi(m.xg), 0.0, 256)):
        cand = sm.Candidates(m.xg, m.ien, phi, level, sm.SIDE, b.dir)
        for s in (None, sub):
            o = sm.step(b, NONE, 0.0, sub=s, cand=cand)
            has = o["hit"][0] >= 0
            assert o["surf"].sum() == hits and o["hit"][4][has].min() > 1e-9
    under = sm.entering_under(cand, None, b, b.at(0.0))
    # vertical: two under every column.  Oblique: the rays of the last row (j = 15) enter the slab's top and leave the mesh
    # through y = 0 above the lower metal surface: one candidate there, two under the other 240 columns
    one = np.zeros(b.ncol, bool) if name == "vertical" else np.arange(b.ncol) // b.n == b.n - 1
    assert (under[o["surf"] & ~one] >= 2).all() and (under[one] == 1).all()
    top = cand.F.reshape(-1, 3, 3)[o["facet"][o["surf"]]][:, :, 2]
    assert (np.abs(top - 0.8) < 1e-12).all()                        # the winner is the slab's top


def test_new_symbols_are_exported():
    subprocess.check_call(["make", "-s", "-j8", "-C", ROOT])
    lib = ctypes.CDLL(os.path.join(ROOT, "dedflow_amd", "libdedflow.so"))
    for name in ("ParticleContextSetLaserSurface", "ParticleContextLaserSurfaceUpdate", "ParticleContextLaserSurfaceFacets",
                 "ParticleContextLaserSurfacePower", "dfl_laser_surface_count", "dfl_laser_surface_emit", "dfl_laser_surface_nodes",
                 "dfl_laser_surface_deposit", "dfl_laser_surface_source_add", "dfl_laser_surface_power"):
        assert hasattr(lib, name), name
