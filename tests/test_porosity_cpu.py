"""CPU tests of the porosity record (include/dedflow.h, "porosity record"): the symbols, the library's host-only configuration
check, the numpy model (tests/porosity_model.py) against a plain flood fill, and what every scene of test_gpu_porosity.py
promises: how many pores it makes, which components are open, the snake's diameter."""
import ctypes as C
import os

import numpy as np
import pytest

import porosity_model as pm
from dedflow_amd.meshgen import fan_mesh, kuhn_cube, single_tet

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
    for n in ("DflPorosityCheck", "DflMeshSetPorosity", "DflMeshPorosityEnabled", "DflMeshPorosity", "DflMeshPorosityStats",
              "DflMeshPorosityResult", "DflMeshPorosityLabels"):
        assert n in pub and hasattr(lib, n), n
    for n in ("dfl_porosity_label", "dfl_porosity_rank", "dfl_porosity_tets", "dfl_porosity_pores", "dfl_porosity_temp_bytes"):
        assert n in ker and hasattr(lib, n), n
    assert hasattr(lib, "DflPorosityTestLaunches")
    for n in ("set_porosity", "porosity_on", "porosity"):
        assert hasattr(api.Problem, n), n
    assert C.sizeof(api.DflPorosity) == 24 and C.sizeof(api.DflPore) == 16 + 10 * 8 and C.sizeof(api.DflPorosityStats) == 9 * 8


def test_configuration_check():
    from dedflow_amd import api
    L = api.lib()
    why = C.create_string_buffer(200)

    def library(**kw):
        cfg = api.porosity_config(**kw)
        return L.DflPorosityCheck(C.byref(cfg), why, 200), why.value.decode()

    for good in (dict(), dict(level=-3.5), dict(side=-1), dict(open_groups=63), dict(open_groups=0), dict(max_pores=1),
                 dict(max_pores=65536), dict(every=7)):
        assert library(**good)[0] == 0 and pm.refusal(pm.config(**good)) is None, good
    for reason, bad in (("level", dict(level=np.nan)), ("level", dict(level=np.inf)), ("level", dict(level=-np.inf)),
                        ("side", dict(side=0)), ("side", dict(side=2)), ("side", dict(side=-3)),
                        ("open_groups", dict(open_groups=-1)), ("max_pores", dict(max_pores=0)),
                        ("max_pores", dict(max_pores=-5)), ("max_pores", dict(max_pores=65537)), ("every", dict(every=-1))):
        rc, text = library(**bad)
        assert rc != 0 and reason in text and pm.refusal(pm.config(**bad)) == reason, (reason, bad, text)


def _scenes(M):
    m = _cube(M)
    yield "plane", pm.plane(m)
    yield "plane/closed", pm.plane(m, open_groups=0)
    yield "one", pm.spheres(m, pm.ONE_BUBBLE)
    yield "two", pm.spheres(m, pm.TWO_BUBBLES, side=-1)
    yield "wall", pm.spheres(m, pm.WALL_BUBBLE)


@pytest.mark.parametrize("M", [4, 6])
def test_model_labels_against_a_flood_fill(M):
    m = _cube(M)
    N = m.num_node
    for what, (cfg, w) in _scenes(M):
        want = pm.flood_fill_labels(m, w[4 * N:5 * N], cfg["level"], cfg["side"])
        assert np.array_equal(pm.labels(m, w[4 * N:5 * N], cfg["level"], cfg["side"]), want), what
    rng = np.random.default_rng(5)
    phi = rng.normal(size=N)                       # a random sign per node: many small components
    phi[rng.integers(0, N, 3)] = np.nan
    for side in (1, -1):
        assert np.array_equal(pm.labels(m, phi, 0.1, side), pm.flood_fill_labels(m, phi, 0.1, side))
    f = fan_mesh()
    phi = rng.normal(size=f.num_node)
    assert np.array_equal(pm.labels(f, phi, 0.0, 1), pm.flood_fill_labels(f, phi, 0.0, 1))


def test_single_tet_masks():
    m = single_tet()
    for mask in range(16):
        for side in (1, -1):
            cfg, w = pm.single_tet_masks(m, mask, side)
            r = pm.evaluate(m, w, cfg)
            gas = [a for a in range(4) if (mask >> a) & 1]
            assert r["components"] == r["pores"] == (1 if gas else 0)
            assert [p["label"] for p in r["list"]] == gas[:1] and all(p["nodes"] == len(gas) and p["tets"] == 1 for p in r["list"])
            assert abs(float(r["volume_metal"] + r["volume_pores"]) - 1.0 / 6.0) <= 1e-15
            if mask == 15:
                assert r["list"][0]["volume"] == r["list"][0]["volume_scale"] and r["list"][0]["T_wall_min"] == np.inf
            opened = pm.evaluate(m, w, dict(cfg, open_groups=15))
            assert opened["pores"] == 0 and opened["components"] == r["components"]
            assert abs(float(opened["volume_open"] - r["volume_pores"])) <= 1e-18


@pytest.mark.parametrize("M", [6, 13])
@pytest.mark.parametrize("side", [1, -1])
def test_plane_and_bubble_promises(M, side):
    m = _cube(M)
    r = pm.evaluate(m, *pm.plane(m, side=side)[::-1])
    assert (r["components"], r["pores"]) == (1, 0) and (r["pore"] == -1).all()
    assert abs(float(r["volume_metal"]) - 0.55) <= 1e-12 and abs(float(r["volume_open"]) - 0.45) <= 1e-12
    cfg, w = pm.plane(m, side=side, open_groups=0)
    r = pm.evaluate(m, w, cfg)
    assert (r["components"], r["pores"], r["listed"]) == (1, 1, 1) and abs(r["list"][0]["volume"] - 0.45) <= 1e-12
    assert r["list"][0]["lo"][2] == 0.55 or abs(r["list"][0]["lo"][2] - 0.55) <= 1e-15
    assert r["list"][0]["hi"] == (1.0, 1.0, 1.0) and abs(r["porosity"] - 0.45) <= 1e-12
    x = np.asarray(m.xg).reshape(-1, 3)
    for phi in (np.ones(m.num_node), -np.ones(m.num_node)):                # all metal, all gas
        r = pm.evaluate(m, pm.state(m, phi, side=side), cfg)
        assert r["components"] == r["pores"] == (1 if phi[0] < 0 else 0)
        assert abs(float(r["volume_metal"] + r["volume_pores"]) - 1.0) <= 1e-12
    one = pm.evaluate(m, *pm.spheres(m, pm.ONE_BUBBLE, side=side)[::-1])
    assert (one["components"], one["pores"]) == (2, 1) and one["list"][0]["nodes"] >= 1
    assert one["list"][0]["T_wall_min"] < one["list"][0]["T_wall_max"] < np.inf
    lo, hi = np.array(one["list"][0]["lo"]), np.array(one["list"][0]["hi"])
    assert (lo >= np.array([0.3, 0.3, 0.2]) - 1.0 / M).all() and (hi <= np.array([0.7, 0.7, 0.6]) + 1.0 / M).all() and (hi > lo).all()
    two = pm.evaluate(m, *pm.spheres(m, pm.TWO_BUBBLES, side=side)[::-1])
    assert (two["components"], two["pores"]) == (3, 2) and two["list"][0]["label"] < two["list"][1]["label"]
    cfg, w = pm.spheres(m, pm.WALL_BUBBLE, side=side)
    assert pm.evaluate(m, w, cfg)["pores"] == 1                            # x- is not open: a pore
    both = pm.evaluate(m, w, dict(cfg, open_groups=pm.Z_PLUS | 1))
    assert (both["components"], both["pores"]) == (2, 0)                   # x- open: no pore
    assert abs(float(both["volume_open"]) - float(pm.evaluate(m, w, cfg)["volume_open"] + pm.evaluate(m, w, cfg)["volume_pores"])) <= 1e-15


def test_touching_and_separated_blocks():
    m = _cube(13)
    N = m.num_node
    for blocks, pores in ((pm.TOUCHING, 1), (pm.SEPARATED, 2)):
        cfg, w = pm.boxes(m, blocks, z_gas=12)
        r = pm.evaluate(m, w, cfg)
        assert (r["components"], r["pores"]) == (pores + 1, pores), blocks
        ijk = pm.lattice(m)
        inside = [np.all([(ijk[:, d] >= b[d][0]) & (ijk[:, d] <= b[d][1]) for d in range(3)], axis=0) for b in blocks]
        assert (inside[0] & inside[1]).sum() == (1 if pores == 1 else 0)
        assert sum(p["nodes"] for p in r["list"]) == (inside[0] | inside[1]).sum()


def test_snake_promises():
    m = _cube(13)
    cfg, w = pm.snake(m)
    r = pm.evaluate(m, w, cfg)
    nodes = pm.snake_nodes(m)
    assert (r["components"], r["pores"]) == (1, 1) and r["list"][0]["label"] == nodes.min() and r["list"][0]["nodes"] == nodes.size
    assert pm.graph_diameter(m, w, cfg, nodes.min()) >= 64
    ien = np.asarray(m.ien).reshape(-1, 4)
    tets = np.flatnonzero(np.isin(ien, nodes).any(axis=1))
    assert np.unique(tets // 256).size > 1 and r["list"][0]["tets"] == tets.size
    ijk = pm.lattice(m)[nodes]
    assert ijk.min() >= 1 and ijk.max() <= 12                              # closed in metal: no boundary node


def test_many_pores_promises():
    m = _cube(13)
    cfg, w = pm.many_pores(m, max_pores=16)
    r = pm.evaluate(m, w, cfg)
    assert r["components"] == r["pores"] == 343 and r["listed"] == 16 and len(r["list"]) == 16
    assert [p["label"] for p in r["list"]] == sorted(np.flatnonzero(r["label"] >= 0))[:16]
    assert all(p["nodes"] == 1 for p in r["list"]) and (r["pore"] >= 16).sum() == 343 - 16
    full = pm.evaluate(m, w, dict(cfg, max_pores=1024))
    assert full["listed"] == 343 and abs(float(sum(p["ld_volume"] for p in full["list"]) - full["volume_pores"])) <= 1e-15


def test_bad_values_split_and_count():
    m = _cube(6)
    N = m.num_node
    cfg, w = pm.spheres(m, pm.ONE_BUBBLE)
    clean = pm.evaluate(m, w, cfg)
    centre = int(np.argmin(np.linalg.norm(np.asarray(m.xg).reshape(-1, 3) - np.array([0.5, 0.5, 0.4]), axis=1)))
    assert clean["pore"][centre] == 0
    for value in (np.nan, np.inf, -np.inf):
        bad = w.copy()
        bad[4 * N + centre] = value
        r = pm.evaluate(m, bad, cfg)
        assert r["bad_nodes"] == 1 and r["bad_tets"] == 24 and r["label"][centre] == -2 and r["pore"][centre] == -1
        assert float(r["volume_metal"]) < float(clean["volume_metal"]) and r["pores"] >= 1
    far = w.copy()
    far[4 * N + 0] = np.nan                                                # a metal corner: one node, its tets, nothing else
    r = pm.evaluate(m, far, cfg)
    assert r["bad_nodes"] == 1 and r["pores"] == clean["pores"] and np.array_equal(r["pore"], clean["pore"])
    hot = w.copy()
    hot[5 * N:] = np.nan
    r = pm.evaluate(m, hot, cfg)
    assert r["list"][0]["T_wall_min"] == np.inf and r["list"][0]["T_wall_max"] == -np.inf
    assert r["list"][0]["volume"] == clean["list"][0]["volume"]


def test_permutation_keeps_everything_but_the_labels():
    m = _cube(13)
    cfg, w = pm.spheres(m, pm.TWO_BUBBLES)
    base = pm.evaluate(m, w, cfg)
    for perm in (np.random.default_rng(11).permutation(m.num_node), np.arange(m.num_node)[::-1].copy()):
        m2, w2 = pm.permuted(m, w, perm)
        r = pm.evaluate(m2, w2, cfg)
        assert r["pores"] == base["pores"] and r["components"] == base["components"]
        assert np.array_equal(r["label"] >= 0, (base["label"] >= 0)[np.argsort(perm)])
        key = lambda p: (p["nodes"], p["tets"], p["volume"], p["lo"], p["hi"], p["T_wall_min"], p["T_wall_max"])
        assert sorted(map(key, r["list"])) == sorted(map(key, base["list"]))
        for p in r["list"]:
            assert p["label"] == np.flatnonzero(r["pore"] == r["list"].index(p)).min()
