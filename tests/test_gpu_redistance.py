"""GPU tests of the level-set redistancing (include/dedflow.h "level-set redistancing"; host/redistance.c,
csrc/k_redistance.hip, csrc/level_facets.hpp) against tests/redistance_model.py: the facet list, the new phi at every node, the
statistics and the volume, bit-for-bit reproducibility (run to run, under another cell size, with facets that span many
cells, after the buffers grew), memory safety, the hold groups, DflTimeStep and the refusals.

Bounds.  L = the largest extent of the mesh.  Facets and nodes: deviation from the float64 model <= 1e-12 L, no node excluded;
the model performs the kernel's operations in the kernel's association, so zero is expected.  Against the np.longdouble model
the bound is four times the float64 model's own deviation from it on the same case, measured here on the CPU (the projection
onto a sliver facet is ill-conditioned, so that is not 1e-12).  Statistics: integers equal, floats to 1e-12 (relative to
max(1, |value|); the values are volumes of the unit scale and gradient deviations of order one).  With DFL_PARITY_OUT set, the
observed ratios go to that file (profiles/redistance_parity.jsonl is such a run)."""
import ctypes as C

import numpy as np
import pytest

import redistance_model as rm
from dedflow_amd.meshgen import fan_mesh, kuhn_cube, single_tet, synthetic_fields
from guarded_buffers import Pool, Recorder, assert_bits, raw

pytestmark = pytest.mark.gpu
LD = np.longdouble
BOUND = 1e-12
record = Recorder("a")
TILT = np.array([0.2, -0.3, 1.0]) / np.sqrt(1.13)
MESHES = {"single": single_tet, "fan": fan_mesh, "cube4": lambda: kuhn_cube(4, jitter=0.2), "cube12": lambda: kuhn_cube(12, jitter=0.2)}
BAND = {"single": 0.5, "fan": 0.45, "cube4": 0.3, "cube12": 1.5 / 12}     # (cube12: a 9^3 grid, so most cells are interior)
FIELDS = ["plane", "sphere", "sphere3", "unreached", "layer", "const5", "nan"]
CASES = [(mn, f) for mn in MESHES for f in FIELDS]


@pytest.fixture(scope="module")
def api():
    from dedflow_amd import api as A
    A.lib()
    return A


@pytest.fixture(scope="module", autouse=True)
def _parity_records():
    yield
    record.write()


@pytest.fixture
def pool(api):
    p = Pool(api)
    yield p
    p.free()


_mesh_cache, _model_cache = {}, {}


def _mesh(name):
    if name not in _mesh_cache:
        _mesh_cache[name] = MESHES[name]()
    return _mesh_cache[name]


def _problem(api, mesh_name, **kw):
    m = _mesh(mesh_name)
    return api.Problem(m, bcs=[], **kw) if mesh_name == "single" else api.Problem(m, **kw)   # (the tet has four groups)


def extent(m):
    x = m.xg.reshape(-1, 3)
    return float((x.max(axis=0) - x.min(axis=0)).max())


def case(mesh_name, field):
    """(mesh, phi [N], level, band)"""
    m = _mesh(mesh_name)
    x = m.xg.reshape(-1, 3)
    c = 0.5 * (x.min(axis=0) + x.max(axis=0))
    L = extent(m)
    plane = (x - c) @ TILT
    level = 0.25 * L                      # passes 0.015 from the corner (0, 1, 1) of the cubes: a band node in a corner cell
    phi = plane
    if field in ("sphere", "sphere3"):
        phi = np.sqrt(((x - (c + L * np.array([0.05, 0.02, -0.04]))) ** 2).sum(axis=1)) - 0.3 * L
        phi, level = (3.0 * phi if field == "sphere3" else phi), 0.0
    elif field == "unreached":
        level = 10.0 * L
    elif field == "layer":                # every node near the surface is put exactly on it
        phi = np.where(np.abs(plane - level) < 0.08 * L, level, plane)
    elif field == "const5":               # every fifth tet is flat
        phi = plane.copy()
        ien = m.ien.reshape(-1, 4)
        for e in range(0, m.num_tet, 5):
            phi[ien[e]] = phi[ien[e, 0]]
    elif field == "nan":
        phi = plane.copy()
        phi[1 if m.num_node < 10 else int(np.argsort(np.abs(plane - level))[2])] = np.nan
    return m, np.ascontiguousarray(phi, np.float64), float(level), BAND[mesh_name]


def model(mesh_name, field, hold_groups=0, band=None):
    """the float64 model, its statistics, and the longdouble model on the nodes that can be inside the band"""
    key = (mesh_name, field, hold_groups, band)
    if key not in _model_cache:
        m, phi, level, b = case(mesh_name, field)
        b = band or b
        res = rm.redistance(m, phi, level, b, hold_groups)
        near = res["d"] < 1.25 * b
        ld = rm.redistance(m, phi, level, b, hold_groups, dtype=LD, nodes=near)
        res["stats"] = rm.stats(m, phi, res, level)
        res["ld"] = ld["phi"]
        _model_cache[key] = res
    return _model_cache[key]


def state(m, phi, seed=3):
    """w [6N] with phi in its slot and recognisable numbers everywhere else"""
    N = m.num_node
    w = np.random.default_rng(seed).uniform(-2.0, 2.0, 6 * N)
    w[4 * N:5 * N] = phi
    return w


def _run(api, pool, P, m, phi, level, band, **cfg):
    """set, redistance a guarded state in place; returns (nf, new phi, slot) after the bands and every other slot were checked"""
    N = m.num_node
    P.set_redistance(level, band, **cfg)
    assert P.redistance_on
    ws = pool.slot(state(m, phi))
    nf = P.redistance(ws.ptr)
    api.sync()
    written = np.zeros(6 * N, bool)
    written[4 * N:5 * N] = True
    out = ws.check("w: bands, u, p, dphi-side slots and T", written=written)
    return nf, out[4 * N:5 * N].copy(), ws


def _dev(got, ref):
    """max |got - ref| in longdouble; the NaNs must sit in the same places"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaNs in other places"
    ok = ~np.isnan(ref)
    return float(np.abs(got[ok].astype(LD) - ref[ok].astype(LD)).max()) if ok.any() else 0.0


def _close(got, want):
    return abs(got - want) <= 1e-12 * max(1.0, abs(want))


@pytest.mark.parametrize("mesh_name,field", CASES)
def test_parity_with_the_model(api, pool, mesh_name, field):
    m, phi, level, band = case(mesh_name, field)
    ref = model(mesh_name, field)
    L = extent(m)
    P = _problem(api, mesh_name)
    try:
        nf, new, ws = _run(api, pool, P, m, phi, level, band)
        # facets: count, order, values
        F = P.redistance_facets()
        assert nf == len(ref["facets"]) == len(F)
        fdev = _dev(F, ref["facets"]) / L
        # nodes: every one of them
        ndev = _dev(new, ref["phi"]) / L
        own = _dev(ref["phi"], ref["ld"])                      # the float64 model against the longdouble one
        ldev = _dev(new, ref["ld"])
        print(f"redistance {mesh_name}/{field}: {nf} facets, {int(ref['band'].sum())} band nodes; deviation / L facets {fdev:.2e}, "
              f"nodes {ndev:.2e}; from longdouble {ldev:.2e} (the model's own {own:.2e})")
        record("redistance_facets", f"{mesh_name}/{field}", fdev / BOUND, facets=int(nf))
        record("redistance_nodes", f"{mesh_name}/{field}", ndev / BOUND, band_nodes=int(ref["band"].sum()),
               from_longdouble=ldev, model_from_longdouble=own)
        assert fdev <= BOUND and ndev <= BOUND
        assert ldev <= 4.0 * own
        if field == "unreached":
            assert nf == 0 and np.all(new == level - band)
        if field == "nan":
            assert np.isnan(new).sum() == 1 and np.isnan(F).any()
        if field == "layer":
            n = rm.cross(F[:, 3:6] - F[:, 0:3], F[:, 6:9] - F[:, 0:3])
            assert mesh_name == "single" or (rm.dot(n, n) < 1e-24 * L ** 4).any()   # degenerate (to rounding) facets are in the list
        # statistics and volume
        st, want = P.redistance_stats(), ref["stats"]
        assert st["facets"] == want["facets"] and st["band_nodes"] == want["band_nodes"], (st, want)
        for k in ("max_change", "grad_dev_before", "grad_dev_after", "volume_before", "volume_after"):
            assert _close(st[k], want[k]), (k, st[k], want[k])
        vol = P.level_set_volume(ws.ptr, level)
        assert _close(vol, want["volume_after"]) and vol == st["volume_after"]
        # a second call on the same input: the same bits, the same list
        nf2, new2, _ = _run(api, pool, P, m, phi, level, band)
        assert nf2 == nf
        assert_bits(new2, new, "phi of a second run")
        assert_bits(P.redistance_facets(), F, "facets of a second run")
    finally:
        P.close()


def test_plane_volume_is_analytic(api):
    """DflMeshLevelSetVolume of a tilted plane through the unit cube against the closed form (test_redistance_cpu.py)"""
    m, phi, level, _ = case("cube4", "plane")
    P = _problem(api, "cube4")
    try:
        w = api.DeviceArray.from_numpy(state(m, phi))
        got = P.level_set_volume(w, level)                      # (no configuration is set)
        want = rm.clipped_cube_volume(TILT, level + 0.5 * TILT.sum())
        print(f"clipped cube: {got:.15f} against {want:.15f}")
        assert abs(got - want) <= 1e-12
        assert abs(got + P.level_set_volume(api.DeviceArray.from_numpy(state(m, -phi)), -level) - 1.0) <= 1e-12
    finally:
        P.close()


def test_edge_shapes_are_covered():
    """what the cases above are there for: N no multiple of 16, band nodes in corner cells, nodes with more than 16 and more
    than 64 candidate entries (a facet whose box meets [p - band, p + band] sits in one of the 27 cells around p)"""
    assert all(_mesh(k).num_node % 16 for k in MESHES)
    most = {}
    for mesh_name in ("cube4", "cube12"):
        m, phi, level, band = case(mesh_name, "plane")
        ref = model(mesh_name, "plane")
        x = m.xg.reshape(-1, 3)
        corner = np.isin(x, (0.0, 1.0)).all(axis=1)
        assert corner.sum() == 8 and (ref["band"] & corner).any()
        F = ref["facets"].reshape(-1, 3, 3)
        lo, hi = F.min(axis=1), F.max(axis=1)
        meets = ((lo[None] <= x[:, None] + band) & (hi[None] >= x[:, None] - band)).all(axis=2)
        most[mesh_name] = int(meets.sum(axis=1).max())
    print("largest candidate lists (lower bounds):", most)
    assert most["cube4"] > 16 and most["cube12"] > 64


def test_cell_size_does_not_matter(api, pool, monkeypatch):
    m, phi, level, band = case("cube12", "sphere")
    P = _problem(api, "cube12")
    try:
        out = {}
        for cell in ("1", "2.5"):
            monkeypatch.setenv("DFL_REDISTANCE_CELL", cell)
            nf, new, _ = _run(api, pool, P, m, phi, level, band)
            out[cell] = (nf, new, P.redistance_facets(), P.redistance_stats())
        assert out["1"][0] == out["2.5"][0] > 0
        assert_bits(out["2.5"][1], out["1"][1], "phi under DFL_REDISTANCE_CELL=2.5")
        assert_bits(out["2.5"][2], out["1"][2], "facets under DFL_REDISTANCE_CELL=2.5")
        assert out["1"][3] == out["2.5"][3]
        assert_bits(out["1"][1], model("cube12", "sphere")["phi"], "phi against the model")
    finally:
        P.close()


def test_band_below_the_mesh_size(api, pool):
    """band = 0.02 against h = 0.25: a 51^3 grid, every facet spans many cells"""
    m, phi, level, _ = case("cube4", "plane")
    ref = model("cube4", "plane", band=0.02)
    assert 0 < ref["band"].sum() < m.num_node
    P = _problem(api, "cube4")
    try:
        nf, new, _ = _run(api, pool, P, m, phi, level, 0.02)
        assert nf == len(ref["facets"])
        assert_bits(new, ref["phi"], "phi with band < h")
        assert P.redistance_stats()["band_nodes"] == int(ref["band"].sum())
    finally:
        P.close()


def test_same_bits_after_the_buffers_grew(api, pool):
    m, phi, level, band = case("cube12", "plane")
    fresh = _problem(api, "cube12")
    try:
        nf, want, _ = _run(api, pool, fresh, m, phi, level, band)
        assert nf > 1024                                        # more than the lists hold at first: this call grew them
    finally:
        fresh.close()
    P = _problem(api, "cube12")
    try:
        for f in ("unreached", "sphere"):                       # nothing, then a smaller surface: the lists grow in two steps
            _run(api, pool, P, *case("cube12", f))
        nf2, got, _ = _run(api, pool, P, m, phi, level, band)
        assert nf2 == nf
        assert_bits(got, want, "phi after unrelated calls")
    finally:
        P.close()


@pytest.mark.parametrize("mesh_name,groups", [("cube4", 0b000101), ("fan", 0b1), ("cube4", 1 << 30)])
def test_hold_groups_keep_their_bits(api, pool, mesh_name, groups):
    m, phi, level, band = case(mesh_name, "plane")
    ref = model(mesh_name, "plane", hold_groups=groups)
    held = rm.hold_mask(m, groups)
    assert held.any() == (groups < (1 << 30))
    P = _problem(api, mesh_name)
    try:
        nf, new, _ = _run(api, pool, P, m, phi, level, band, hold_groups=groups)
        assert_bits(new[held], phi[held], "held nodes")
        assert_bits(new, ref["phi"], "phi with hold groups")
        if held.any():
            assert (raw(new[~held]) != raw(phi[~held])).any() and (ref["band"] & held).any()
        st = P.redistance_stats()
        assert st["band_nodes"] == ref["stats"]["band_nodes"] and st["max_change"] == ref["stats"]["max_change"]
    finally:
        P.close()


# ---- DflTimeStep -------------------------------------------------------------------------------------------------------------
def _steps(api, m, mode, nstep=2):
    """nstep time steps of a steep phi; mode: "never", "every0", "every2", or "by hand" (DflMeshRedistance before the second)"""
    N = m.num_node
    wg, dwg = synthetic_fields(m)
    x = m.xg.reshape(-1, 3)
    wg[4 * N:5 * N] = 3.0 * ((x - 0.5) @ TILT)
    wg[5 * N:] = 1650.0 + 120.0 * ((x - 0.5) @ TILT)
    P = api.Problem(m, maxit=120, atol=1e-14, rtol=1e-6)
    try:
        P.set_scalar_transport(phi=True, T=True)
        if mode != "never":
            P.set_redistance(0.0, 0.3, every=2 if mode == "every2" else 0)
        st = [api.DeviceArray.from_numpy(a) for a in (wg, 0.1 * dwg, 0.1 * dwg)]
        F_d, dx_d = api.DeviceArray(6 * N), api.DeviceArray(6 * N)
        its = []
        for k in range(nstep):
            if mode == "by hand" and k == 1:
                assert P.redistance(st[0]) > 0
            its.append(P.time_step(st[0], st[1], st[2], F_d, dx_d, newton_maxit=2)[0])
        api.sync()
        return dict(it=its, w=st[0].numpy(), dw=st[2].numpy())
    finally:
        P.close()


def test_time_step_redistances_every_other_step(api):
    m = _mesh("cube4")
    run = {mode: _steps(api, m, mode) for mode in ("never", "every0", "every2", "by hand")}
    for k in ("w", "dw"):
        assert np.isfinite(run["never"][k]).all()
        assert_bits(run["every0"][k], run["never"][k], f"{k} with every = 0")
        assert_bits(run["every2"][k], run["by hand"][k], f"{k} with every = 2")
    assert run["every0"]["it"] == run["never"]["it"] and run["every2"]["it"] == run["by hand"]["it"]
    assert (raw(run["every2"]["w"]) != raw(run["never"]["w"])).any()
    one = {mode: _steps(api, m, mode, nstep=1) for mode in ("never", "every2")}   # the first step is not an every-th one
    assert_bits(one["every2"]["w"], one["never"]["w"], "w after one step")


def test_refusals(api, capfd, monkeypatch):
    m = _mesh("cube4")
    N = m.num_node
    why = C.create_string_buffer(160)
    for cfg, reason in [((np.nan, 0.1, 0, 0), "level is not finite"), ((0.0, np.inf, 0, 0), "band is not finite"),
                        ((0.0, 0.0, 0, 0), "band must be positive"), ((0.0, -1.0, 0, 0), "band must be positive"),
                        ((0.0, 0.1, 0, -1), "every must not be negative")]:
        assert api.lib().DflRedistanceCheck(C.byref(api.DflRedistance(*cfg)), why, 160) != 0
        assert reason in why.value.decode(), (cfg, why.value)
    assert api.lib().DflRedistanceCheck(C.byref(api.DflRedistance(0.0, 0.1, 5, 3)), why, 160) == 0
    P = api.Problem(m)
    try:
        capfd.readouterr()
        P.set_redistance(0.0, -0.1)
        assert not P.redistance_on and "band must be positive" in capfd.readouterr().err
        w = api.DeviceArray.from_numpy(state(m, (m.xg.reshape(-1, 3) - 0.5) @ TILT))
        before = w.numpy()
        assert api.lib().DflMeshRedistance(P.mesh, w.ptr) == -1
        assert "no redistancing is set" in capfd.readouterr().err
        assert api.lib().DflMeshRedistanceFacets(P.mesh, None) == -1
        assert_bits(w.numpy(), before, "nothing written")
        P.set_redistance(0.0, 0.3, every=1)
        assert P.redistance_on and capfd.readouterr().err == ""
        assert all(v == 0 for v in P.redistance_stats().values())       # no call yet
        P.set_redistance(np.inf, 0.3)                                  # refused: the earlier configuration stays
        assert P.redistance_on and "level is not finite" in capfd.readouterr().err
        monkeypatch.setenv("DFL_REDISTANCE_CELL", "0.5")                # refused as well
        P.set_redistance(0.0, 0.2)
        assert "DFL_REDISTANCE_CELL" in capfd.readouterr().err
        monkeypatch.delenv("DFL_REDISTANCE_CELL")
        # a solver with a communicator: refused before anything is computed
        comm = api.DflComm()
        api.lib().KrylovSetComm(P.ksp, C.byref(comm))
        st = [api.DeviceArray.from_numpy(np.zeros(6 * N)) for _ in range(3)]
        F_d, dx_d = api.DeviceArray(6 * N), api.DeviceArray(6 * N)
        assert P.time_step(st[0], st[1], st[2], F_d, dx_d)[0] == -1
        assert "redistancing is single-GPU only" in capfd.readouterr().err
        api.lib().KrylovSetComm(P.ksp, None)
        P.set_redistance()
        assert not P.redistance_on
    finally:
        P.close()
