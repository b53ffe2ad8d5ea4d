"""GPU tests of the porosity record (include/dedflow.h "porosity record"; host/porosity.c, csrc/k_porosity.hip) against
tests/porosity_model.py: label[], pore[], the pore list's labels / nodes / tets, every count, the boxes and the T extremes bit for
bit; the volumes within the bound below.  Scenes: the single tet's 16 masks, the plane, bubbles, the snake, renumbered meshes,
hundreds of one-node pores, bad values, the state after an evaluation, the passive DflTimeStep hook and the refusals.  The state
sits in a guarded buffer and must come back untouched.

Bound of the volumes.  |dev - model| <= 1e-12 x volume_scale against np.longdouble sums, the project's standing bound for
fixed-order sums; the scale is the model's.  The three totals: the same bound against the mesh volume.  With DFL_PARITY_OUT set,
the observed err / bound of every case goes to that file (profiles/porosity_parity.jsonl is such a run)."""
import ctypes as C

import numpy as np
import pytest

import porosity_model as pm
from dedflow_amd.meshgen import fan_mesh, kuhn_cube, single_tet, synthetic_fields
from guarded_buffers import Pool, Recorder, assert_bits

pytestmark = pytest.mark.gpu
BOUND = 1e-12
LD = pm.LD
record = Recorder("a")
MESHES = {"single": single_tet, "fan": fan_mesh, "cube4": lambda: kuhn_cube(4), "cube6": lambda: kuhn_cube(6),
          "cube13": lambda: kuhn_cube(13)}


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


def _problem(api, name, mesh=None):
    m = mesh if mesh is not None else _mesh(name)
    return api.Problem(m, bcs=[]) if name == "single" else api.Problem(m)   # (the tet has four groups)


def _model(key, mesh, w, cfg):
    """the model's answer, computed once per case"""
    if key not in _model_cache:
        _model_cache[key] = pm.evaluate(mesh, w, cfg)
    return _model_cache[key]


def _launches(api, P):
    return int(api.lib().DflPorosityTestLaunches(P.mesh))


def _evaluate(api, pool, P, cfg, w, what, off=0):
    """Set, one evaluation from a guarded buffer, which must come back untouched; returns the device result"""
    P.set_porosity(**cfg)
    assert P.porosity_on
    ws = pool.slot(w, off=off)
    got = P.porosity(ws.ptr)
    ws.check(what + ": w")
    return got


def _ratio(err, bound):
    return float(err / bound) if bound > 0 else (0.0 if err == 0 else np.inf)


def _compare(got, want, what, P=None):
    """the device result against the model's; returns the worst err / bound of the volumes"""
    assert got["label"].dtype == np.int32 and np.array_equal(got["label"], want["label"]), what
    assert np.array_equal(got["pore"], want["pore"]), what
    for k in pm.COUNTS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert len(got["list"]) == len(want["list"]) == want["listed"], what
    worst = 0.0
    for k, (g, r) in enumerate(zip(got["list"], want["list"])):
        for key in ("label", "nodes", "tets"):
            assert g[key] == r[key], (what, k, key, g[key], r[key])
        for key in ("lo", "hi", "T_wall_min", "T_wall_max"):
            assert_bits(np.array(g[key]), np.array(r[key]), f"{what}: pore {k} {key}")
        scale = r["ld_scale"]
        for key, ld in (("volume", r["ld_volume"]), ("volume_scale", scale)):
            err, bound = abs(LD(g[key]) - ld), BOUND * scale
            ratio = _ratio(err, bound)
            print(f"porosity parity {what}: pore {k} {key} = {g[key]!r}, err {float(err):.3e}, err / bound {ratio:.3e}")
            assert err <= bound, (what, k, key, g[key], float(ld), ratio)
            worst = max(worst, ratio)
    for key in pm.TOTALS:
        err, bound = abs(LD(got[key]) - want[key]), BOUND * want["mesh_volume"]
        ratio = _ratio(err, bound)
        print(f"porosity parity {what}: {key} = {got[key]!r}, err {float(err):.3e}, err / bound {ratio:.3e}")
        assert err <= bound, (what, key, got[key], float(want[key]), ratio)
        worst = max(worst, ratio)
    both = got["volume_metal"] + got["volume_pores"]
    assert got["porosity"] == (got["volume_pores"] / both if both > 0.0 else 0.0), what
    record("porosity", what, worst, pores=want["pores"], listed=want["listed"], components=want["components"],
           closed_tets=want["closed_tets"], nodes=int(want["label"].size))
    return worst


def _case(api, pool, name, cfg, w, what, mesh=None, off=0):
    """one Problem, one evaluation, compared with the model; returns (device result, launches)"""
    m = mesh if mesh is not None else _mesh(name)
    P = _problem(api, name, mesh)
    try:
        got = _evaluate(api, pool, P, cfg, w, what, off)
        _compare(got, _model(what, m, w, cfg), what)
        return got, _launches(api, P)
    finally:
        P.close()


# ---- single tet, plane ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [1, -1])
def test_single_tet_all_masks(api, pool, side):
    m = _mesh("single")
    P = _problem(api, "single")
    try:
        for mask in range(16):
            for groups in (0, 15):
                cfg, w = pm.single_tet_masks(m, mask, side, groups)
                what = f"single/mask{mask}/side{side:+d}/open{groups}"
                got = _evaluate(api, pool, P, cfg, w, what, off=mask & 1)
                _compare(got, _model(what, m, w, cfg), what)
                assert got["pores"] == (1 if mask and not groups else 0), what
    finally:
        P.close()


@pytest.mark.parametrize("side", [1, -1])
@pytest.mark.parametrize("name", ["fan", "cube6", "cube13"])
def test_plane_surface(api, pool, name, side):
    m = _mesh(name)
    N = m.num_node
    if name == "fan":                                                      # group 0 is the whole surface
        cfg, w = pm.plane(m, z0=0.1, side=side, open_groups=1)
    else:
        cfg, w = pm.plane(m, side=side)
    P = _problem(api, name)
    try:
        xg0 = api.d2h(P.mesh.contents.device.contents.xg, 3 * N, np.float64)
        what = f"{name}/plane/side{side:+d}"
        got = _evaluate(api, pool, P, cfg, w, what)
        _compare(got, _model(what, m, w, cfg), what)
        assert (got["components"], got["pores"]) == (1, 0) and (got["pore"] == -1).all() and got["porosity"] == 0.0
        closed = dict(cfg, open_groups=0)                                  # the atmosphere itself is listed
        got = _evaluate(api, pool, P, closed, w, what + "/closed", off=1)
        _compare(got, _model(what + "/closed", m, w, closed), what + "/closed")
        assert (got["components"], got["pores"], got["listed"]) == (1, 1, 1) and got["list"][0]["nodes"] == (got["label"] >= 0).sum()
        for tag, phi in (("metal", np.ones(N)), ("gas", -np.ones(N))):
            w1 = pm.state(m, phi, side=side)
            got = _evaluate(api, pool, P, cfg, w1, f"{what}/all-{tag}")
            _compare(got, _model(f"{what}/all-{tag}", m, w1, cfg), f"{what}/all-{tag}")
            assert got["components"] == (tag == "gas") and got["pores"] == 0
        api.sync()
        assert_bits(api.d2h(P.mesh.contents.device.contents.xg, 3 * N, np.float64), xg0, "xg")
    finally:
        P.close()


# ---- bubbles -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [1, -1])
@pytest.mark.parametrize("name", ["cube6", "cube13"])
def test_spherical_bubbles(api, pool, name, side):
    m = _mesh(name)
    P = _problem(api, name)
    try:
        for tag, balls, groups, pores in (("one", pm.ONE_BUBBLE, pm.Z_PLUS, 1), ("two", pm.TWO_BUBBLES, pm.Z_PLUS, 2),
                                          ("wall-closed", pm.WALL_BUBBLE, pm.Z_PLUS, 1),
                                          ("wall-open", pm.WALL_BUBBLE, pm.Z_PLUS | 1, 0)):
            cfg, w = pm.spheres(m, balls, side=side, open_groups=groups)
            what = f"{name}/{tag}/side{side:+d}"
            got = _evaluate(api, pool, P, cfg, w, what, off=(side + 1) // 2)
            _compare(got, _model(what, m, w, cfg), what)
            assert (got["components"], got["pores"]) == (1 + max(pores, 1), pores), what
            for p in got["list"]:
                assert 0.0 < p["volume"] < p["volume_scale"] and p["T_wall_min"] < p["T_wall_max"], what
            assert (got["porosity"] > 0.0) == (pores > 0)
    finally:
        P.close()


@pytest.mark.parametrize("side", [1, -1])
def test_touching_and_separated_bubbles(api, pool, side):
    """two blocks of gas nodes that share exactly one node are one pore; one layer of metal nodes between them makes two"""
    for tag, blocks, pores in (("touching", pm.TOUCHING, 1), ("separated", pm.SEPARATED, 2)):
        cfg, w = pm.boxes(_mesh("cube13"), blocks, side=side, z_gas=12)
        got, _ = _case(api, pool, "cube13", cfg, w, f"cube13/{tag}/side{side:+d}")
        assert (got["components"], got["pores"]) == (pores + 1, pores)
        assert got["list"][0]["nodes"] == (53 if pores == 1 else 27)


# ---- the snake --------------------------------------------------------------------------------------------------------------------
def test_snake_is_one_pore_in_the_launches_of_the_plane(api, pool):
    m = _mesh("cube13")
    cfg, w = pm.snake(m)
    got, launches = _case(api, pool, "cube13", cfg, w, "cube13/snake")
    nodes = pm.snake_nodes(m)
    assert (got["components"], got["pores"]) == (1, 1)
    assert got["list"][0]["label"] == nodes.min() and got["list"][0]["nodes"] == nodes.size
    assert np.array_equal(np.flatnonzero(got["pore"] == 0), np.sort(nodes))
    _, plane_launches = _case(api, pool, "cube13", *pm.plane(m), "cube13/plane-launches")
    assert launches == plane_launches and launches > 0


# ---- renumbered meshes ------------------------------------------------------------------------------------------------------------
def _row_key(p):
    return (p["nodes"], p["tets"], p["volume"], p["volume_scale"], p["lo"], p["hi"], p["T_wall_min"], p["T_wall_max"])


@pytest.mark.parametrize("order", ["random", "reversed"])
@pytest.mark.parametrize("scene", ["bubbles", "snake"])
def test_renumbered_mesh(api, pool, scene, order):
    m = _mesh("cube13")
    N = m.num_node
    cfg, w = pm.spheres(m, pm.TWO_BUBBLES) if scene == "bubbles" else pm.snake(m)
    perm = np.random.default_rng(11).permutation(N) if order == "random" else np.arange(N)[::-1].copy()
    base, _ = _case(api, pool, "cube13", cfg, w, f"cube13/{'two' if scene == 'bubbles' else 'snake'}/unpermuted")
    m2, w2 = pm.permuted(m, w, perm)
    got, _ = _case(api, pool, "cube13", cfg, w2, f"cube13/{scene}/{order}", mesh=m2)
    # everything but the labels is the unpermuted result mapped through the permutation, to the last bit
    for k in pm.COUNTS + pm.TOTALS:
        assert got[k] == base[k], k
    assert sorted(map(_row_key, got["list"])) == sorted(map(_row_key, base["list"]))
    assert np.array_equal(got["label"][perm] >= 0, base["label"] >= 0)
    new_rank = {}
    for a in np.flatnonzero(base["pore"] >= 0):
        assert new_rank.setdefault(int(base["pore"][a]), int(got["pore"][perm[a]])) == got["pore"][perm[a]]
    assert len(set(new_rank.values())) == len(new_rank) == base["pores"]
    for old, new in new_rank.items():
        assert _row_key(got["list"][new]) == _row_key(base["list"][old])
        assert got["list"][new]["label"] == perm[base["label"] == base["list"][old]["label"]].min()


# ---- many pores -------------------------------------------------------------------------------------------------------------------
def test_many_one_node_pores(api, pool):
    m = _mesh("cube13")
    cfg, w = pm.many_pores(m, max_pores=16)
    got, _ = _case(api, pool, "cube13", cfg, w, "cube13/many/16")
    assert (got["pores"], got["listed"], len(got["list"])) == (343, 16, 16)
    assert [p["label"] for p in got["list"]] == list(np.flatnonzero(got["label"] >= 0)[:16])
    assert (got["pore"] >= 16).sum() == 343 - 16 and got["pore"].max() == 342
    cfg_all = dict(cfg, max_pores=4096)
    full, _ = _case(api, pool, "cube13", cfg_all, w, "cube13/many/all")
    assert (full["pores"], full["listed"]) == (343, 343) and full["volume_pores"] == got["volume_pores"]
    assert full["list"][:16] == got["list"] and all(p["nodes"] == 1 and p["tets"] > 0 for p in full["list"])
    assert abs(sum(p["volume"] for p in full["list"]) - full["volume_pores"]) <= 1e-12


# ---- bad values -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_bad_phi_inside_on_the_wall_and_far_away(api, pool, value):
    m = _mesh("cube6")
    N = m.num_node
    x = np.asarray(m.xg).reshape(-1, 3)
    cfg, w = pm.spheres(m, pm.ONE_BUBBLE)
    clean = _model("cube6/one/side+1", m, w, cfg)
    centre = int(np.argmin(np.linalg.norm(x - np.array([0.5, 0.5, 0.4]), axis=1)))
    inside = np.flatnonzero(clean["pore"] == 0)
    ien = np.asarray(m.ien).reshape(-1, 4)
    wall = int(np.setdiff1d(ien[np.isin(ien, inside).any(axis=1)].ravel(), inside)[0])
    P = _problem(api, "cube6")
    try:
        for tag, node in (("inside", centre), ("wall", wall), ("far", 0)):
            bad = w.copy()
            bad[4 * N + node] = value
            what = f"cube6/bad-{tag}/{value}"
            got = _evaluate(api, pool, P, cfg, bad, what)
            _compare(got, _model(what, m, bad, cfg), what)
            assert got["bad_nodes"] == 1 and got["bad_tets"] == np.isin(ien, node).any(axis=1).sum()
            assert got["label"][node] == -2 and got["pore"][node] == -1
            if tag == "far":
                assert np.array_equal(np.delete(got["pore"], node), np.delete(clean["pore"], node))
                assert got["list"][0]["volume"] == clean["list"][0]["volume"]
    finally:
        P.close()


def test_nan_temperature_never_wins(api, pool):
    m = _mesh("cube6")
    N = m.num_node
    cfg, w = pm.spheres(m, pm.ONE_BUBBLE)
    some, every = w.copy(), w.copy()
    some[5 * N::3] = np.nan
    every[5 * N:] = np.nan
    got, _ = _case(api, pool, "cube6", cfg, some, "cube6/T-some-nan")
    assert np.isfinite(got["list"][0]["T_wall_min"]) and np.isfinite(got["list"][0]["T_wall_max"])
    got, _ = _case(api, pool, "cube6", cfg, every, "cube6/T-all-nan")
    assert got["list"][0]["T_wall_min"] == np.inf and got["list"][0]["T_wall_max"] == -np.inf


# ---- the state after an evaluation ----------------------------------------------------------------------------------------------------
def _same(a, b):
    return (all(a[k] == b[k] for k in pm.COUNTS + pm.TOTALS + ("porosity", "list")) and np.array_equal(a["label"], b["label"])
            and np.array_equal(a["pore"], b["pore"]))


def test_labels_are_roots_and_evaluations_repeat_bit_for_bit(api, pool):
    m = _mesh("cube13")
    rng = np.random.default_rng(3)
    x = np.asarray(m.xg).reshape(-1, 3)
    cfg = pm.config(level=0.05, open_groups=pm.Z_PLUS, max_pores=4096)
    w = pm.state(m, 0.3 * rng.normal(size=m.num_node) + 0.4 - x[:, 2])   # many components of every size
    other = pm.many_pores(m)[1]
    P = _problem(api, "cube13")
    try:
        a = _evaluate(api, pool, P, cfg, w, "cube13/noise")
        _compare(a, _model("cube13/noise", m, w, cfg), "cube13/noise")
        gas = np.flatnonzero(a["label"] >= 0)
        assert a["pores"] > 10 and (a["label"][gas] <= gas).all() and np.array_equal(a["label"][a["label"][gas]], a["label"][gas])
        b = P.porosity(pool.slot(w, off=1).ptr)
        assert _same(a, b)
        # a tiny capacity: the next evaluation grows the key lists; then a different state; then the first one again
        assert int(api.lib().DflPorosityTestCapacity(P.mesh, 4)) == 4
        c = P.porosity(pool.slot(w).ptr)
        grown = int(api.lib().DflPorosityTestCapacity(P.mesh, 0))
        assert _same(a, c) and grown >= _model("cube13/noise", m, w, cfg)["closed_tets"] > 4
        mid = P.porosity(pool.slot(other).ptr)
        assert mid["pores"] == 0 or not _same(a, mid)
        d = P.porosity(pool.slot(w, off=1).ptr)
        assert _same(a, d) and int(api.lib().DflPorosityTestCapacity(P.mesh, 0)) >= grown
    finally:
        P.close()
    P = _problem(api, "cube13")                                            # and in a fresh mesh
    try:
        assert _same(a, _evaluate(api, pool, P, cfg, w, "cube13/noise/again"))
    finally:
        P.close()


# ---- DflTimeStep ----------------------------------------------------------------------------------------------------------------------
def _two_steps(api, every):
    m = _mesh("cube4")
    N = m.num_node
    wg, dwg = synthetic_fields(m)
    x = m.xg.reshape(-1, 3)
    wg[4 * N:5 * N] = np.minimum(0.75 - x[:, 2] - 0.8 * np.abs(x[:, 1] - 0.5), np.linalg.norm(x - 0.25, axis=1) - 0.2)
    wg[5 * N:] = 1700.0 + 1000.0 * (x[:, 2] - 0.4)
    P = api.Problem(m, maxit=120, atol=1e-14, rtol=1e-6)
    try:
        P.set_scalar_transport(phi=True, T=True)
        if every:
            P.set_porosity(level=0.0, open_groups=pm.Z_PLUS, every=every)
            assert P.porosity_on
        st = [api.DeviceArray.from_numpy(a) for a in (wg, 0.1 * dwg, 0.1 * dwg)]
        F_d, dx_d = api.DeviceArray(6 * N), api.DeviceArray(6 * N)
        o = dict(w=[], it=[], res=[], launches=[])
        for _ in range(2):
            it, rn, r0 = P.time_step(st[0], st[1], st[2], F_d, dx_d, newton_maxit=2)
            api.sync()
            o["it"].append(it)
            o["w"].append(st[0].numpy())
            if every:
                o["launches"].append(_launches(api, P))
                o["res"].append(P.porosity())
        o["dw"], o["F"] = st[2].numpy(), F_d.numpy()
        if every:
            o["manual"] = P.porosity(st[0])                                # the same state, evaluated directly
            o["model"] = pm.evaluate(m, o["w"][1], pm.config(level=0.0, open_groups=pm.Z_PLUS))
        return o
    finally:
        P.close()


def test_time_step_is_passive_and_fills_the_result(api):
    base, on, second = _two_steps(api, 0), _two_steps(api, 1), _two_steps(api, 2)
    for run in (on, second):
        assert base["it"] == run["it"] and min(base["it"]) >= 0
        for k in range(2):
            assert np.isfinite(base["w"][k]).all()
            assert_bits(run["w"][k], base["w"][k], f"wgold after step {k}")
        for k in ("dw", "F"):
            assert_bits(run[k], base[k], k)
        assert _same(run["res"][1], run["manual"])
        _compare(run["manual"], run["model"], "cube4/time-step")
    assert on["launches"][0] > 0 and on["launches"][0] == on["launches"][1] and on["res"][0]["components"] >= 1
    assert second["launches"] == [0, on["launches"][1]]                   # every = 2: the first step evaluates nothing
    assert second["res"][0]["components"] == 0 and (second["res"][0]["label"] == -1).all()


def test_refusals_and_off(api, capfd):
    m = _mesh("cube6")
    N = m.num_node
    cfg, w = pm.spheres(m, pm.ONE_BUBBLE)
    P = api.Problem(m)
    L = api.lib()
    try:
        wd = api.DeviceArray.from_numpy(w)
        capfd.readouterr()
        assert L.DflMeshPorosity(P.mesh, wd.ptr) == -1                     # without a configuration
        assert "no porosity record" in capfd.readouterr().err
        assert L.DflMeshPorosityResult(P.mesh, None, 0) == -1 and "no porosity record" in capfd.readouterr().err
        lab, por = C.c_void_p(1), C.c_void_p(1)
        assert L.DflMeshPorosityLabels(P.mesh, C.byref(lab), C.byref(por)) == 0 and lab.value is None and por.value is None
        for reason, bad in (("level", dict(level=np.nan)), ("side", dict(side=0)), ("open_groups", dict(open_groups=-2)),
                            ("max_pores", dict(max_pores=0)), ("max_pores", dict(max_pores=65537)), ("every", dict(every=-1))):
            P.set_porosity(**dict(cfg, **bad))
            assert not P.porosity_on and reason in capfd.readouterr().err
        P.set_porosity(**cfg)
        assert P.porosity_on and capfd.readouterr().err == ""
        before = P.porosity(wd)
        assert before["pores"] == 1
        for reason, bad in (("level", dict(level=np.inf)), ("side", dict(side=3)), ("open_groups", dict(open_groups=-1)),
                            ("max_pores", dict(max_pores=-1)), ("every", dict(every=-4))):
            P.set_porosity(**dict(cfg, **bad))                             # refused: configuration and result stay
            assert P.porosity_on and reason in capfd.readouterr().err
            assert _same(P.porosity(), before)
        assert _same(P.porosity(wd), before)                               # ... and it still evaluates as configured
        # a solver with a communicator: refused before anything is computed, but only with every > 0
        P.set_porosity(**dict(cfg, every=1))
        comm = api.DflComm()
        L.KrylovSetComm(P.ksp, C.byref(comm))
        arr = [api.DeviceArray.from_numpy(np.zeros(6 * N)) for _ in range(3)]
        F_d, dx_d = api.DeviceArray(6 * N), api.DeviceArray(6 * N)
        capfd.readouterr()
        assert P.time_step(arr[0], arr[1], arr[2], F_d, dx_d)[0] == -1
        assert "porosity record is single-GPU only" in capfd.readouterr().err
        assert _launches(api, P) == 0 and P.porosity()["components"] == 0  # nothing was evaluated
        L.KrylovSetComm(P.ksp, None)
        P.set_porosity()                                                   # NULL frees
        assert not P.porosity_on
        assert L.DflMeshPorosity(P.mesh, wd.ptr) == -1 and "no porosity record" in capfd.readouterr().err
        with pytest.raises(RuntimeError):
            P.porosity(wd)
    finally:
        P.close()
