"""GPU tests of the track cross-sections (include/dedflow.h "track cross-sections"; host/track.c, csrc/k_track.hip) against
tests/track_sections_model.py: the pair list, its 65 offsets and the six extents bit for bit, the three areas within the bound
below, the bead's closed forms, the area rule, 64 stations in one cell layer, stations through a vertex, an edge and a face,
outside the mesh, NaN inputs, side = -1, the sources of T_peak, reproducibility, list reuse, the passive DflTimeStep hook and
the refusals.  The state and T_peak sit in guarded buffers and must come back untouched.

Bound of the areas.  |dev - model| <= 1e-12 x area_scale against np.longdouble, the project's standing bound for fixed-order
sums; area_scale is the model's.  With DFL_PARITY_OUT set, the observed err / bound of every case goes to that file
(profiles/track_sections_parity.jsonl is such a run)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import track_sections_model as tm
from dedflow_amd.meshgen import fan_mesh, kuhn_cube, single_tet, synthetic_fields
from guarded_buffers import Pool, Recorder, assert_bits

pytestmark = pytest.mark.gpu
BOUND = 1e-12
record = Recorder("a")
MESHES = {"single": single_tet, "fan": fan_mesh, "cube4": lambda: kuhn_cube(4), "cube6": lambda: kuhn_cube(6),
          "cube13": lambda: kuhn_cube(13)}
EMPTY = dict(area_clad=0.0, area_fused=0.0, area_scale=0.0, height=-np.inf, depth=-np.inf, y_lo_clad=np.inf, y_hi_clad=-np.inf,
             y_lo_fused=np.inf, y_hi_fused=-np.inf, pairs=0, dilution=0.0)


@pytest.fixture(scope="module")
def api():
    from dedflow_amd import api as A
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


def _problem(api, name, mesh=None, **kw):
    m = mesh if mesh is not None else _mesh(name)
    return api.Problem(m, bcs=[], **kw) if name == "single" else api.Problem(m, **kw)   # (the tet has four groups)


def _model(key, mesh, w, T_peak, cfg):
    """the model's answer, computed once per case"""
    if key not in _model_cache:
        _model_cache[key] = tm.evaluate(mesh, w, T_peak, cfg)
    return _model_cache[key]


def _pairs(api, P):
    p, off = C.c_void_p(), (C.c_int32 * 65)()
    total = int(api.lib().DflTrackSectionsTestPairs(P.mesh, C.byref(p), off))
    return (api.d2h(p.value, total, np.int32) if total > 0 else np.zeros(0, np.int32)), np.array(off[:], np.int32)


def _set(P, cfg):
    P.set_track_sections(**cfg)
    assert P.track_sections_on


def _compare(api, P, got, want, what, kernel="ts_eval_kernel"):
    """device results `got` against the model's (results, list, offsets) `want`; returns the worst err / bound"""
    res, lst, off = want
    dlst, doff = _pairs(api, P)
    assert np.array_equal(doff, off), (what, doff, off)
    assert dlst.dtype == np.int32 and np.array_equal(dlst, lst), what
    assert len(got) == len(res), what
    worst = 0.0
    for k, (g, r) in enumerate(zip(got, res)):
        assert g["pairs"] == r["pairs"], (what, k)
        for key in tm.EXTENTS:
            assert_bits(np.array([g[key]]), np.array([r[key]]), f"{what}: station {k} {key}")
        scale = r["ld"]["area_scale"]
        for key in tm.AREAS:
            err, bound = abs(tm.LD(g[key]) - r["ld"][key]), BOUND * scale
            ratio = float(err / bound) if bound > 0 else (0.0 if err == 0 else np.inf)
            print(f"track sections parity {what}: station {k} {key} = {g[key]!r}, err {float(err):.3e}, err / bound {ratio:.3e}")
            assert err <= bound, (what, k, key, g[key], float(r["ld"][key]), ratio)
            worst = max(worst, ratio)
        both = g["area_clad"] + g["area_fused"]
        assert g["dilution"] == (g["area_fused"] / both if both > 0.0 else 0.0), (what, k)
    record(kernel, what, worst, stations=len(res), pairs=int(lst.size), nodes=int(P.N), tets=int(P.T))
    return worst


def _evaluate(api, pool, P, cfg, w, T_peak, what, off=0):
    """Set, one evaluation from guarded buffers, which must come back untouched; returns the device results"""
    _set(P, cfg)
    ws = pool.slot(w, off=off)
    ts = pool.slot(T_peak, off=1 - off) if T_peak is not None else None
    got = P.track_sections(ws.ptr, ts.ptr if ts is not None else None)
    ws.check(what + ": w")
    if ts is not None:
        ts.check(what + ": T_peak")
    return got


@pytest.mark.parametrize("side", [1, -1])
@pytest.mark.parametrize("name", list(MESHES))
def test_parity_and_memory_safety(api, pool, name, side):
    m = _mesh(name)
    cfg, w, T_peak = tm.wavy(m, num_station=5, side=side)
    what = f"{name}/wavy/side{side:+d}"
    P = _problem(api, name)
    try:
        xg0 = api.d2h(P.mesh.contents.device.contents.xg, 3 * P.N, np.float64)
        got = _evaluate(api, pool, P, cfg, w, T_peak, what, off=(side + 1) // 2)
        want = _model(what, m, w, T_peak, cfg)
        _compare(api, P, got, want, what)
        assert sum(r["pairs"] for r in got) > 0, what
        if name.startswith("cube"):
            assert all(r["area_clad"] > 0 and r["pairs"] > 0 for r in got) and sum(r["area_fused"] > 0 for r in got) >= 3, what
            assert any(0.0 < r["dilution"] < 1.0 for r in got)
        api.sync()
        assert_bits(api.d2h(P.mesh.contents.device.contents.xg, 3 * P.N, np.float64), xg0, "xg")
    finally:
        P.close()


def test_side_minus_one_mirrors_side_plus_one(api, pool):
    """phi -> -phi, level -> -level, side -> -side is the same metal: the same pairs and the same numbers"""
    m = _mesh("cube6")
    out = []
    for side in (1, -1):
        cfg, w, T_peak = tm.wavy(m, num_station=5, side=side)
        P = _problem(api, "cube6")
        try:
            out.append((_evaluate(api, pool, P, cfg, w, T_peak, f"mirror{side:+d}"), _pairs(api, P)))
        finally:
            P.close()
    assert out[0][0] == out[1][0] and np.array_equal(out[0][1][0], out[1][1][0]) and np.array_equal(out[0][1][1], out[1][1][1])


@pytest.mark.parametrize("M", [4, 6])
def test_bead_closed_forms(api, pool, M):
    """the bead of a piecewise-linear phi: the closed forms within 1e-12 relative, at a node plane and off it"""
    name = f"cube{M}"
    m = _mesh(name)
    cfg, w, T_peak = tm.bead(m)
    P = _problem(api, name)
    try:
        got = _evaluate(api, pool, P, cfg, w, T_peak, f"{name}/bead")
        _compare(api, P, got, _model(f"{name}/bead", m, w, T_peak, cfg), f"{name}/bead")
        for c, r in zip(cfg["stations"], got):
            for key, want in tm.BEAD.items():
                assert abs(r[key] - want) <= 1e-12 * abs(want), (M, c, key, r[key], want)
    finally:
        P.close()


@pytest.mark.parametrize("case", ["axis", "oblique"])
def test_area_rule(api, pool, case):
    """everything metal and fused: area_clad + area_fused = area_scale = the area of the plane inside the unit cube; a station
    on a node plane counts once, one on the far boundary sees nothing"""
    m = _mesh("cube4")
    r2 = np.sqrt(2.0)
    if case == "axis":
        stations = (0.0, 0.25, 0.3, 0.5, 1.0)
        cfg, w, T_peak = tm.all_metal(m, stations)
        areas = [1.0, 1.0, 1.0, 1.0, 0.0]
    else:
        stations = (0.0, 0.3, 0.5 / r2)
        cfg, w, T_peak = tm.all_metal(m, stations, normal=(1.0, 1.0, 0.0), origin=(0.5, 0.5, 0.5))
        areas = [r2 - 2.0 * c for c in stations]
    P = _problem(api, "cube4")
    try:
        got = _evaluate(api, pool, P, cfg, w, T_peak, f"area/{case}")
        _compare(api, P, got, _model(f"area/{case}", m, w, T_peak, cfg), f"area/{case}")
        for c, r, want in zip(stations, got, areas):
            assert abs(r["area_clad"] + r["area_fused"] - want) <= 1e-12 * r2, (c, r)
            assert abs(r["area_scale"] - want) <= 1e-12 * r2, (c, r)
            assert (r["pairs"] == 0) == (want == 0.0)
        if case == "axis":
            assert got[-1] == EMPTY
    finally:
        P.close()


def test_64_stations_in_one_cell_layer(api, pool):
    """64 stations 1 / 256 apart inside one layer of cells of cube4: every tet of the layer pairs with all of them, one
    workgroup meets all 64 bits and every lane of it sets several"""
    m = _mesh("cube4")
    stations = [0.25 + (k + 0.5) / 256.0 for k in range(64)]
    cfg, w, T_peak = tm.bead(m, stations)
    P = _problem(api, "cube4")
    try:
        got = _evaluate(api, pool, P, cfg, w, T_peak, "cube4/64")
        want = _model("cube4/64", m, w, T_peak, cfg)
        _compare(api, P, got, want, "cube4/64")
        assert len(got) == 64 and min(r["pairs"] for r in got) >= 32
        lst, off = want[1], want[2]
        assert np.array_equal(lst[off[0]:off[1]], lst[off[63]:off[64]])       # the same tets pair with the first and the last
        for r in got:
            assert abs(r["area_clad"] - 0.05) <= 1e-12 * 0.05 and abs(r["dilution"] - 5.0 / 9.0) <= 1e-12
    finally:
        P.close()


def test_one_station_reuses_the_lists_of_a_larger_evaluation(api, pool):
    m = _mesh("cube6")
    cfg64, w, T_peak = tm.bead(m, [0.02 + k / 70.0 for k in range(64)])
    cfg1 = dict(cfg64, stations=[0.41])
    P = _problem(api, "cube6")
    try:
        def cap():
            a, b = C.c_int32(), C.c_int32()
            api.lib().DflTrackSectionsTestCapacity(P.mesh, C.byref(a), C.byref(b))
            return a.value, b.value

        _set(P, cfg1)
        small = cap()
        big = _evaluate(api, pool, P, cfg64, w, T_peak, "cube6/64")
        _compare(api, P, big, _model("cube6/64", m, w, T_peak, cfg64), "cube6/64")
        grown = cap()
        assert grown[0] > small[0] and grown[0] >= sum(r["pairs"] for r in big)
        got = _evaluate(api, pool, P, cfg1, w, T_peak, "cube6/1")
        assert cap() == grown                                              # nothing was allocated for the smaller one
        assert len(got) == 1
        _compare(api, P, got, _model("cube6/1", m, w, T_peak, cfg1), "cube6/1")
        assert abs(got[0]["area_fused"] - 0.0625) <= 1e-12 * 0.0625
    finally:
        P.close()


def test_single_tet_vertex_edge_face_and_outside(api, pool):
    m = _mesh("single")
    w, T_peak = tm.state(4, 1.0), np.zeros(4)
    P = _problem(api, "single")
    try:
        # n = e_x: the face x = 0 (the tet is on its positive side: one pair, the cut is the face), the middle, the vertex
        # (1, 0, 0) (nothing beyond it: no pair) and a plane outside the mesh
        cfg = tm.config((0.0, 0.5, 1.0, 5.0), origin=(0, 0, 0.25), level=0.0, T_fuse=tm.ALL_FUSED)
        got = _evaluate(api, pool, P, cfg, w, T_peak, "single/face-vertex")
        _compare(api, P, got, _model("single/face-vertex", m, w, T_peak, cfg), "single/face-vertex")
        assert [r["pairs"] for r in got] == [1, 1, 0, 0] and got[2] == EMPTY and got[3] == EMPTY
        assert abs(got[0]["area_scale"] - 0.5) <= 1e-15 and abs(got[1]["area_scale"] - 0.125) <= 1e-15
        assert abs(got[0]["area_clad"] + got[0]["area_fused"] - 0.5) <= 1e-15
        # n = (1, 1, 0) / sqrt 2 through the edge x = y = 0: one pair whose cut degenerates to the edge
        cfg = tm.config((0.0,), normal=(1.0, 1.0, 0.0), level=0.0, T_fuse=tm.ALL_FUSED)
        got = _evaluate(api, pool, P, cfg, w, T_peak, "single/edge")
        _compare(api, P, got, _model("single/edge", m, w, T_peak, cfg), "single/edge")
        assert got[0]["pairs"] == 1 and got[0]["area_scale"] == 0.0 and got[0]["area_clad"] == 0.0
    finally:
        P.close()


def test_result_before_the_first_evaluation_and_outside_the_mesh(api, pool):
    m = _mesh("cube4")
    cfg, w, T_peak = tm.bead(m, (-2.0, 7.0))
    P = _problem(api, "cube4")
    try:
        _set(P, cfg)
        assert P.track_sections_result() == [EMPTY, EMPTY]                 # nothing evaluated yet
        got = _evaluate(api, pool, P, cfg, w, T_peak, "cube4/outside")
        assert got == [EMPTY, EMPTY]
        lst, off = _pairs(api, P)
        assert lst.size == 0 and (off == 0).all()
        inside = _evaluate(api, pool, P, dict(cfg, stations=[0.3]), w, T_peak, "cube4/inside")
        assert inside[0]["pairs"] > 0
        _set(P, cfg)                                                       # a new configuration forgets the last evaluation
        assert P.track_sections_result() == [EMPTY, EMPTY]
    finally:
        P.close()


@pytest.mark.parametrize("what", ["phi", "coordinate"])
def test_a_nan_costs_only_its_tets(api, pool, what):
    m = _mesh("cube4")
    cfg, w, T_peak = tm.bead(m, (0.3, 0.41))
    node = 62                                                              # the centre of the cube
    if what == "phi":
        w = w.copy()
        w[4 * m.num_node + node] = np.nan
    else:
        xg = m.xg.copy()
        xg[3 * node + 1] = np.nan
        m = dataclasses.replace(m, xg=xg)
    P = _problem(api, "cube4", mesh=m)
    try:
        got = _evaluate(api, pool, P, cfg, w, T_peak, f"cube4/nan-{what}")
        _compare(api, P, got, _model(f"cube4/nan-{what}", m, w, T_peak, cfg), f"cube4/nan-{what}")
        for r in got:
            assert all(np.isfinite(r[k]) for k in tm.AREAS + tm.EXTENTS) and r["pairs"] > 0
            assert 0.0 <= r["area_clad"] <= 0.05 * (1 + 1e-12) and r["area_scale"] > 0.0
    finally:
        P.close()


def test_sources_of_the_peak_temperature(api, pool):
    """T_peak NULL: the solidification record's when one is set, else nothing is fused"""
    m = _mesh("cube6")
    N = m.num_node
    cfg, w, T_peak = tm.bead(m)
    w = w.copy()
    w[5 * N:] = T_peak                                                     # the record primes T_peak with T of the state
    P = _problem(api, "cube6")
    try:
        got = _evaluate(api, pool, P, cfg, w, None, "cube6/no-T_peak")
        _compare(api, P, got, _model("cube6/no-T_peak", m, w, None, cfg), "cube6/no-T_peak")
        assert all(r["area_fused"] == 0.0 and r["depth"] == -np.inf and r["area_clad"] > 0 for r in got)
        P.set_solidification(T_front=1650.0)
        ws = pool.slot(w)
        P.solidification_update(ws.ptr, 0.1)
        got = P.track_sections(ws.ptr)
        _compare(api, P, got, _model("cube6/record", m, w, T_peak, cfg), "cube6/record")
        assert all(abs(r["area_fused"] - 0.0625) <= 1e-12 * 0.0625 for r in got)
        explicit = P.track_sections(ws.ptr, pool.slot(T_peak + 50.0, off=1).ptr)   # an explicit array wins over the record
        assert all(a["area_fused"] > b["area_fused"] for a, b in zip(explicit, got))
        P.set_solidification()
        assert all(r["area_fused"] == 0.0 for r in P.track_sections(ws.ptr))
    finally:
        P.close()


def test_two_evaluations_agree_bit_for_bit(api, pool):
    m = _mesh("cube13")
    cfg, w, T_peak = tm.wavy(m, num_station=5)
    runs = []
    for _ in range(2):
        P = _problem(api, "cube13")
        try:
            a = _evaluate(api, pool, P, cfg, w, T_peak, "cube13/repeat")
            la = _pairs(api, P)
            b = P.track_sections(pool.slot(w, off=1).ptr, pool.slot(T_peak).ptr)
            lb = _pairs(api, P)
            assert a == b and np.array_equal(la[0], lb[0]) and np.array_equal(la[1], lb[1])
            runs.append((a, la))
        finally:
            P.close()
    assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1][0], runs[1][1][0])
    for r in runs[0][0]:
        for k in tm.AREAS + ("height", "y_lo_clad", "y_hi_clad"):         # (the last station fuses nothing: an empty set)
            assert np.isfinite(r[k])


# ---- DflTimeStep ----------------------------------------------------------------------------------------------------------------
def _two_steps(api, on):
    m = _mesh("cube4")
    N = m.num_node
    wg, dwg = synthetic_fields(m)
    x = m.xg.reshape(-1, 3)
    wg[4 * N:5 * N] = 0.7 - x[:, 2] - 0.8 * np.abs(x[:, 1] - 0.5)
    wg[5 * N:] = 1700.0 + 1000.0 * (x[:, 2] - 0.4)
    P = api.Problem(m, maxit=120, atol=1e-14, rtol=1e-6)
    try:
        P.set_scalar_transport(phi=True, T=True)
        if on:
            P.set_solidification(T_front=1650.0, in_time_step=True)
            P.set_track_sections(**dict(tm.bead(m, (0.3, 0.5))[0], every=1))
            assert P.track_sections_on
        st = [api.DeviceArray.from_numpy(a) for a in (wg, 0.1 * dwg, 0.1 * dwg)]
        F_d, dx_d = api.DeviceArray(6 * N), api.DeviceArray(6 * N)
        o = dict(w=[], it=[], res=[])
        for _ in range(2):
            it, rn, r0 = P.time_step(st[0], st[1], st[2], F_d, dx_d, newton_maxit=2)
            api.sync()
            o["it"].append(it)
            o["w"].append(st[0].numpy())
            if on:
                o["res"].append(P.track_sections_result())
        o["dw"], o["F"] = st[2].numpy(), F_d.numpy()
        if on:
            o["manual"] = P.track_sections(st[0])                          # the same state, T_peak of the record
        return o
    finally:
        P.close()


def test_time_step_is_passive_and_fills_the_result(api):
    base, on = _two_steps(api, False), _two_steps(api, True)
    assert base["it"] == on["it"] and min(base["it"]) >= 0
    for k in range(2):
        assert np.isfinite(base["w"][k]).all()
        assert_bits(on["w"][k], base["w"][k], f"wgold after step {k}")
    for k in ("dw", "F"):
        assert_bits(on[k], base[k], k)
    assert on["res"][1] == on["manual"]
    for res in on["res"]:
        assert len(res) == 2 and all(r["pairs"] > 0 and r["area_clad"] > 0 and r["area_fused"] > 0 for r in res)


def test_refusals(api, capfd):
    m = _mesh("cube4")
    N = m.num_node
    cfg, w, T_peak = tm.bead(m)
    P = api.Problem(m)
    L = api.lib()
    try:
        wd = api.DeviceArray.from_numpy(w)
        capfd.readouterr()
        L.DflMeshTrackSections(P.mesh, wd.ptr, None)                        # without a configuration
        assert "no track sections" in capfd.readouterr().err
        out = (api.DflTrackSection * 64)()
        L.DflMeshTrackSectionsResult(P.mesh, out)
        assert "no track sections" in capfd.readouterr().err
        for reason, bad in (("normal", dict(normal=(0.0, 0.0, 0.0))), ("up", dict(up=(3.0, 0.0, 0.0))), ("ascend", dict(stations=(0.3, 0.3))),
                            ("T_fuse", dict(T_fuse=np.nan)), ("side", dict(side=0)), ("num_station", dict(stations=()))):
            P.set_track_sections(**dict(cfg, **bad))
            assert not P.track_sections_on and reason in capfd.readouterr().err
        _set(P, cfg)
        assert capfd.readouterr().err == ""
        before = P.track_sections(wd, api.DeviceArray.from_numpy(T_peak))
        P.set_track_sections(**dict(cfg, level=np.nan))                    # refused: configuration and result stay
        assert P.track_sections_on and "level" in capfd.readouterr().err
        assert P.track_sections_result() == before and len(before) == 4
        # a solver with a communicator: refused before anything is computed, but only with every > 0
        P.set_track_sections(**dict(cfg, every=1))
        comm = api.DflComm()
        L.KrylovSetComm(P.ksp, C.byref(comm))
        arr = [api.DeviceArray.from_numpy(np.zeros(6 * N)) for _ in range(3)]
        F_d, dx_d = api.DeviceArray(6 * N), api.DeviceArray(6 * N)
        capfd.readouterr()
        assert P.time_step(arr[0], arr[1], arr[2], F_d, dx_d)[0] == -1
        assert "track cross-sections are single-GPU only" in capfd.readouterr().err
        assert all(r == EMPTY for r in P.track_sections_result())          # nothing was evaluated
        L.KrylovSetComm(P.ksp, None)
        P.set_track_sections()
        assert not P.track_sections_on
    finally:
        P.close()
