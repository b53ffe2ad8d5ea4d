"""GPU tests of the laser on the level-set surface (host/laser_surface.c, csrc/k_laser_surface.hip; model in include/dedflow.h
"laser on the level-set surface").  Decisions -- which facets are candidates, which tet a column hits, which columns are
lit -- are compared exactly with tests/laser_surface_model.py; weights and powers within the model's a-priori bounds
(laser_surface_model.step: 8 eps kappa per barycentric weight, T_rel on T_c, 6 roundings of lambda, (terms + 4) eps for the
sequential sum), the tally within (n^2 + P) eps P as in test_gpu_laser.py.  There is no fitted tolerance.

Inputs: kuhn_cube(4, jitter=0.2), 16 x 16 columns, a vertical and an oblique beam.  test_laser_surface_cpu.py checks in the
model alone that every hit column's centre lies more than 1e-9 from every projected candidate edge; the tests assert it again
where they use the model's hits."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import guarded_buffers as gb
import laser_model as lm
import laser_surface_model as sm

pytestmark = pytest.mark.gpu
EPS, LD = sm.EPS, sm.LD
KEYS = ("outside", "absorbed_particles", "scattered", "substrate", "reflected", "missed")
NAMES = sorted(sm.DIRECTIONS)
DT = 1e-3
NONE = np.zeros((0, 3))
R = 0.004


@pytest.fixture(scope="module")
def api():
    from dedflow_amd import api as A
    A.lib()
    return A


@pytest.fixture(scope="module")
def m():
    return sm.mesh()


def _mass(r, rho_p=7800.0):
    return rho_p * 4.0 / 3.0 * np.pi * np.asarray(r) ** 3


def _state(api, m, phi):
    w = np.zeros(6 * m.num_node)
    w[4 * m.num_node:5 * m.num_node] = phi
    return api.DeviceArray.from_numpy(w)


@contextlib.contextmanager
def _context(api, m, kw, x=NONE, groups=(), dt=DT):
    """a coupled context with heat and the laser on; yields (particles, problem)"""
    x = np.asarray(x, np.float64).reshape(-1, 3)
    P = api.Problem(m)
    pc = api.Particles(x.reshape(-1), np.zeros(x.size), R, mass=float(_mass(R)), dt=dt)
    try:
        pc.set_heat(cp_p=500.0, T_init=300.0)
        pc.couple(P)
        pc.set_laser(kw["origin"], kw["direction"], kw["power"], kw["w"], kw["h"], kw["r_cut"], kw["eta_p"], kw["eta_s"],
                     kw.get("scan_vel", (0.0, 0.0, 0.0)), groups)
        assert pc.laser_on
        yield pc, P
    finally:
        pc.close()
        P.close()


def _outputs(api, pc, P=0):
    out = dict(power=pc.laser_surface_power().numpy() if pc.laser_surface_on else None, tally=pc.laser_tally(),
               cols=pc.laser_columns(), rate=pc.laser_rate() if P else np.zeros(0))
    api.sync()
    return out


def _run(api, m, kw, phi, level, side=sm.SIDE, x=NONE, groups=(), surface=True, update=True, source=False):
    """one laser step on a fresh context; surface False: no surface is ever set"""
    with _context(api, m, kw, x, groups) as (pc, _):
        nf = None
        if surface:
            pc.set_laser_surface(level, side)
            assert pc.laser_surface_on
            if update:
                nf = pc.laser_surface_update(_state(api, m, phi))
        pc.laser_step(DT)
        out = _outputs(api, pc, len(x))
        out["nf"] = nf
        if surface:
            out["facets"], out["tet"] = pc.laser_surface_facets()
        if source:
            out["q"] = pc.heat_source().numpy()
        return out


def _within(name, got, ref, bound):
    d = np.abs(np.asarray(got, LD) - np.asarray(ref, LD))
    bound = np.broadcast_to(np.asarray(bound, np.float64), d.shape)
    if d.size:
        k = int(np.argmax(d / np.maximum(bound, 1e-300)))
        print(f"laser surface {name}: error {float(d.flat[k]):.3e} bound {float(bound.flat[k]):.3e}")
        assert (d <= bound).all(), (name, float(d.flat[k]), float(bound.flat[k]))


def _check_power(name, power, mdl, N):
    nodes = np.array(sorted(mdl["power"]), np.int64)
    rest = np.setdiff1d(np.arange(N), nodes)
    assert (power[rest] == 0.0).all() and np.isfinite(power).all()
    if nodes.size:
        _within(f"{name}_power", power[nodes], [mdl["power"][k] for k in nodes], [mdl["power_bound"][k] for k in nodes])
    return nodes


def _check_tally(name, got, mdl, b, count=0):
    extra = float(mdl["rate_bound"].sum()) / b.eta_p
    total = sum(LD(got[k]) for k in KEYS)
    _within(f"{name}_identity", total, b.power, (b.ncol + count) * EPS * b.power)
    for k in KEYS:
        _within(f"{name}_tally_{k}", got[k], mdl["tally"][k], extra + (b.ncol + count) * EPS * b.power)


def _check_against_model(name, o, mdl, cand, b, N, count=0):
    has = mdl["hit"][0] >= 0
    assert mdl["hit"][4][has].min() > 1e-9                          # the condition on the input
    assert np.array_equal(o["cols"][1], mdl["face"])                # -2 - tet on every column that hits the surface
    _within(f"{name}_transmitted", o["cols"][0], mdl["T"], mdl["T_rel"] * mdl["T"].astype(float))
    nodes = _check_power(name, o["power"], mdl, N)
    _check_tally(name, o["tally"], mdl, b, count)
    # sum of Power against the substrate tally of the surface columns: |sum_a lambda_a - 1| <= 12 eps per column (3: the
    # normalised weights, 6: lambda's roundings, 3: its four-term sum), the nodal sums 4 n^2 terms, the tally's tree n^2
    surf_sub = LD(b.eta_s) * mdl["T"][mdl["surf"]].sum()
    _within(f"{name}_sum_power", o["power"].astype(LD).sum(), surf_sub, (5 * b.ncol + 20) * EPS * b.power)
    return nodes


@pytest.mark.parametrize("name", NAMES)
def test_tilted_plane(api, m, name):
    kw = sm.beam_args(name)
    b = lm.Beam(**kw)
    phi = sm.plane_phi(m.xg)
    cand = sm.Candidates(m.xg, m.ien, phi, sm.PLANE_LEVEL, sm.SIDE, b.dir)
    mdl = sm.step(b, NONE, 0.0, t=DT, cand=cand)
    o = _run(api, m, kw, phi, sm.PLANE_LEVEL)
    assert o["nf"] == 138 == len(cand.tet)
    gb.assert_bits(o["facets"], cand.F, "facets")
    assert np.array_equal(o["tet"], cand.tet)
    assert mdl["surf"].sum() == {"vertical": 256, "oblique": 240}[name]
    nodes = _check_against_model(f"plane_{name}", o, mdl, cand, b, m.num_node)
    assert nodes.size and (o["power"][nodes] > 0.0).any()
    if name == "vertical":
        assert o["tally"]["missed"] == 0.0
        _within("plane_sum_power_is_substrate", o["power"].astype(LD).sum(), o["tally"]["substrate"], (5 * b.ncol + 20) * EPS * b.power)
    # phi - level scaled by 4 about level 0: an exact scaling
    o4 = _run(api, m, kw, 4.0 * (phi - sm.PLANE_LEVEL), 0.0)
    gb.assert_bits(o4["facets"], o["facets"], "scaled facets")
    assert np.array_equal(o4["tet"], o["tet"]) and np.array_equal(o4["cols"][1], o["cols"][1])
    gb.assert_bits(o4["power"], o["power"], "scaled power")
    gb.assert_bits(o4["cols"][0], o["cols"][0], "scaled transmitted")
    assert o4["tally"] == o["tally"]


@pytest.mark.parametrize("name", NAMES)
def test_first_hit_is_the_top_of_the_floating_slab(api, m, name):
    kw = sm.beam_args(name)
    b = lm.Beam(**kw)
    phi = sm.two_layer_phi(m.xg)
    cand = sm.Candidates(m.xg, m.ien, phi, 0.0, sm.SIDE, b.dir)
    mdl = sm.step(b, NONE, 0.0, t=DT, cand=cand)
    under = sm.entering_under(cand, None, b, b.at(DT))
    one = np.zeros(b.ncol, bool) if name == "vertical" else np.arange(b.ncol) // b.n == b.n - 1   # see test_laser_surface_cpu.py
    assert mdl["surf"].all() and (under[~one] >= 2).all() and (under[one] == 1).all()
    o = _run(api, m, kw, phi, 0.0)
    assert o["nf"] == len(cand.tet)
    gb.assert_bits(o["facets"], cand.F, "facets")
    nodes = _check_against_model(f"slab_{name}", o, mdl, cand, b, m.num_node)
    won = -2 - o["cols"][1]                                         # the tet of every column
    assert (won >= 0).all()
    z = o["facets"].reshape(-1, 3, 3)[:, :, 2]
    top = np.unique(o["tet"][(np.abs(z - 0.8) < 1e-12).all(axis=1)])
    assert np.isin(won, top).all()                                  # the winner is the slab's top
    top_nodes = np.unique(np.asarray(m.ien).reshape(-1, 4)[top])
    assert np.isin(np.flatnonzero(o["power"] != 0.0), top_nodes).all()


def test_shadowing(api, m):
    kw = sm.beam_args("vertical")
    b = lm.Beam(**kw)
    phi = sm.plane_phi(m.xg)
    cand = sm.Candidates(m.xg, m.ien, phi, sm.PLANE_LEVEL, sm.SIDE, b.dir)
    o0 = np.array(kw["origin"])
    col = lambda i, j, z, du=0.3, dv=0.6: o0 + (i - b.n // 2 + du) * b.h * b.e1 + (j - b.n // 2 + dv) * b.h * b.e2 + (z - o0[2]) * np.array([0, 0, 1.0])
    x = np.array([col(8, 8, 0.9), col(8, 8, 0.2, 0.6, 0.3), col(3, 11, 0.95), col(12, 4, 0.1), col(5, 5, 0.7), col(30, 2, 0.5)])
    mdl = sm.step(b, x, R, t=DT, cand=cand)
    c = int(mdl["col"][0])
    assert mdl["col"][1] == c and mdl["col"][5] == b.ncol
    depth = mdl["hit"][2]
    assert mdl["s"][0] < depth[c] < mdl["s"][1] and mdl["s"][3] > depth[mdl["col"][3]]    # above, below; another one below
    o = _run(api, m, kw, phi, sm.PLANE_LEVEL, x=x)
    assert o["rate"][1] == 0.0 and o["rate"][3] == 0.0 and o["rate"][5] == 0.0
    assert (o["rate"][[0, 2, 4]] > 0.0).all()
    _within("shadow_rate", o["rate"], mdl["rate"], mdl["rate_bound"])
    _check_against_model("shadow", o, mdl, cand, b, m.num_node, count=len(x))
    assert o["cols"][0][c] < b.column_power()[c] and mdl["T"][c] < b.column_power()[c]    # the one above lowers T_c
    empty = sm.step(b, NONE, 0.0, t=DT, cand=cand)
    assert float(empty["T"][c]) == b.column_power()[c]
    perm = np.array([4, 2, 5, 0, 3, 1])
    op = _run(api, m, kw, phi, sm.PLANE_LEVEL, x=x[perm])
    gb.assert_bits(op["power"], o["power"], "permuted power")
    assert np.array_equal(op["rate"], o["rate"][perm]) and op["tally"] == o["tally"]


@pytest.mark.parametrize("name", NAMES)
def test_competition_with_boundary_faces(api, m, name):
    kw = sm.beam_args(name)
    b = lm.Beam(**kw)
    phi = sm.plane_phi(m.xg)
    sub = lm.Substrate(m, [4], b)
    cand = sm.Candidates(m.xg, m.ien, phi, sm.PLANE_LEVEL, sm.SIDE, b.dir)
    mdl = sm.step(b, NONE, 0.0, t=DT, sub=sub, cand=cand)
    alone = sm.step(b, NONE, 0.0, t=DT, cand=cand)
    assert np.array_equal(mdl["surf"], alone["surf"])               # surface hits win wherever the plane is met
    o = _run(api, m, kw, phi, sm.PLANE_LEVEL, groups=[4], source=True)
    _check_against_model(f"compete_{name}", o, mdl, cand, b, m.num_node)
    face = o["cols"][1]
    assert (face[mdl["surf"]] <= -2).all() and (face[~mdl["surf"]] >= -1).all()
    # the heat source of one step: boundary nodes get q, surface nodes power (dt power / dt: two more roundings)
    ref, bound = np.zeros(m.num_node, LD), np.zeros(m.num_node)
    for src, bd in ((mdl["q"], mdl["q_bound"]), (mdl["power"], mdl["power_bound"])):
        for k in src:
            ref[k] += src[k]
            bound[k] += bd[k] + 4 * EPS * float(src[k])
    _within(f"compete_{name}_heat_source", o["q"], ref, bound)
    # a hole in the surface (a NaN phi drops the facets around one node): the boundary faces win under it
    bad = phi.copy()
    bad[int(cand.nodes[40, 1])] = np.nan
    holed = sm.Candidates(m.xg, m.ien, bad, sm.PLANE_LEVEL, sm.SIDE, b.dir)
    mdl = sm.step(b, NONE, 0.0, t=DT, sub=sub, cand=holed)
    assert len(mdl["q"]) and len(mdl["power"]) and ((mdl["hit"][0] >= 0) & ~mdl["surf"]).any()
    o = _run(api, m, kw, bad, sm.PLANE_LEVEL, groups=[4], source=True)
    _check_against_model(f"hole_{name}", o, mdl, holed, b, m.num_node)
    ref, bound = np.zeros(m.num_node, LD), np.zeros(m.num_node)
    for src, bd in ((mdl["q"], mdl["q_bound"]), (mdl["power"], mdl["power_bound"])):
        for k in src:
            ref[k] += src[k]
            bound[k] += bd[k] + 4 * EPS * float(src[k])
    _within(f"hole_{name}_heat_source", o["q"], ref, bound)
    assert (o["q"][sorted(mdl["q"])] > 0.0).all()
    # no entering facet (side +1), or no cut tet: bit for bit the run without a surface
    base = _run(api, m, kw, phi, sm.PLANE_LEVEL, groups=[4], surface=False, source=True)
    for args in (dict(phi=phi, level=sm.PLANE_LEVEL, side=+1), dict(phi=np.ones(m.num_node), level=0.0)):
        p = _run(api, m, kw, groups=[4], source=True, **args)
        assert p["nf"] == 0 and len(p["tet"]) == 0 and (p["power"] == 0.0).all()
        assert np.array_equal(p["cols"][1], base["cols"][1])
        gb.assert_bits(p["cols"][0], base["cols"][0], "transmitted")
        gb.assert_bits(p["q"], base["q"], "nodal power of the boundary faces")
        assert p["tally"] == base["tally"]


def test_snapshot_semantics(api, m):
    vel = (0.31, -0.17, 0.0)
    kw = sm.beam_args("oblique", scan_vel=vel)
    b = lm.Beam(**kw)
    phi = sm.plane_phi(m.xg)
    sub = lm.Substrate(m, [4], b)
    with _context(api, m, kw, groups=[4]) as (ref, _):
        ref.laser_step(DT)
        base = _outputs(api, ref)
    pool = gb.Pool(api)
    with _context(api, m, kw, groups=[4]) as (pc, _):
        try:
            pc.set_laser_surface(sm.PLANE_LEVEL, sm.SIDE)
            assert pc.laser_surface_facets()[0].shape == (0, 9)
            pc.laser_step(DT)                                       # before the first Update: no facets
            o = _outputs(api, pc)
            assert o["tally"] == base["tally"] and np.array_equal(o["cols"][1], base["cols"][1]) and (o["power"] == 0.0).all()
            gb.assert_bits(o["cols"][0], base["cols"][0], "transmitted before the first Update")
            t = DT
            assert pc.laser_surface_update(_state(api, m, phi)) == 138
            cand = sm.Candidates(m.xg, m.ien, phi, sm.PLANE_LEVEL, sm.SIDE, b.dir)
            faces = []
            for _ in range(3):                                      # the beam moves over fixed facets
                pc.laser_step(20 * DT)
                t += 20 * DT
                mdl = sm.step(b, NONE, 0.0, t=t, sub=sub, cand=cand)
                o = _outputs(api, pc)
                _check_against_model(f"moving_t{t:.3f}", o, mdl, cand, b, m.num_node)
                faces.append(o["cols"][1])
            assert not np.array_equal(faces[0], faces[2])
            # a shifted level moves the hits
            pc.set_laser_surface(0.1, sm.SIDE)
            assert pc.laser_surface_facets()[0].shape == (0, 9)     # Set drops the snapshot
            high = sm.Candidates(m.xg, m.ien, phi, 0.1, sm.SIDE, b.dir)
            assert pc.laser_surface_update(_state(api, m, phi)) == len(high.tet)
            pc.laser_step(0.0)
            o = _outputs(api, pc)
            mdl = sm.step(b, NONE, 0.0, t=t, sub=sub, cand=high)    # (the laser's clock is not the surface's to reset)
            _check_against_model("shifted", o, mdl, high, b, m.num_node)
            assert not np.array_equal(o["cols"][1], faces[2])
            # more facets than the lists hold: the plane, then the two-layer field; Power into a guarded buffer
            pc.set_laser_surface(0.0, sm.SIDE)                      # (a Set starts from the first capacity again)
            two = sm.Candidates(m.xg, m.ien, sm.two_layer_phi(m.xg), 0.0, sm.SIDE, b.dir)
            flat = sm.Candidates(m.xg, m.ien, phi - sm.PLANE_LEVEL, 0.0, sm.SIDE, b.dir)
            assert len(two.tet) > len(flat.tet) + len(flat.tet) // 2   # beyond the growth of the first Update
            for cnd, field in ((flat, phi - sm.PLANE_LEVEL), (two, sm.two_layer_phi(m.xg))):
                assert pc.laser_surface_update(_state(api, m, field)) == len(cnd.tet)
                F, tet = pc.laser_surface_facets()
                gb.assert_bits(F, cnd.F, "facets")
                assert np.array_equal(tet, cnd.tet)
                pc.laser_step(0.0)
                slot = pool.slot(gb.sent(m.num_node))
                api.lib().ParticleContextLaserSurfacePower(pc.ctx, slot.ptr)
                api.sync()
                power = slot.check("Power", gb.ALL).copy()
                mdl = sm.step(b, NONE, 0.0, t=t, sub=sub, cand=cnd)
                o = _outputs(api, pc)
                gb.assert_bits(power, o["power"], "Power in the guarded buffer")
                _check_against_model(f"grown_{len(cnd.tet)}", o, mdl, cnd, b, m.num_node)
        finally:
            pool.free()


def test_robustness_and_edge_shapes(api, m):
    kw = sm.beam_args("vertical")
    b = lm.Beam(**kw)
    phi = sm.plane_phi(m.xg)
    full = sm.Candidates(m.xg, m.ien, phi, sm.PLANE_LEVEL, sm.SIDE, b.dir)
    bad = phi.copy()
    bad[int(full.nodes[40, 1])] = np.nan                            # a node of a cut tet
    cand = sm.Candidates(m.xg, m.ien, bad, sm.PLANE_LEVEL, sm.SIDE, b.dir)
    assert 0 < len(cand.tet) < len(full.tet)
    o = _run(api, m, kw, bad, sm.PLANE_LEVEL)                       # (zero particles, as most cases here)
    assert o["nf"] == len(cand.tet) and np.array_equal(o["tet"], cand.tet)
    gb.assert_bits(o["facets"], cand.F, "facets")
    assert np.isfinite(o["power"]).all() and all(np.isfinite(o["tally"][k]) for k in KEYS)
    _check_against_model("nan", o, sm.step(b, NONE, 0.0, t=DT, cand=cand), cand, b, m.num_node)
    base = _run(api, m, kw, phi, sm.PLANE_LEVEL, surface=False, source=True)
    L = api.lib()

    def pool_bytes():
        r, u = C.c_int64(0), C.c_int64(0)
        L.DflDevicePoolStats(C.byref(r), C.byref(u))
        return u.value

    with _context(api, m, kw) as (pc, _):
        api.sync()
        before = pool_bytes()
        pc.set_laser_surface(sm.PLANE_LEVEL, sm.SIDE)
        assert pc.laser_surface_update(_state(api, m, phi)) == 138
        pc.laser_step(DT)
        assert pc.laser_tally()["substrate"] > 0.0
        pc.set_laser_surface(None)                                  # off: frees, and the pending energy goes with it
        api.sync()
        assert not pc.laser_surface_on and pool_bytes() == before and pc.laser_surface_update(_state(api, m, phi)) == -1
        pc.set_laser(kw["origin"], kw["direction"], kw["power"], kw["w"], kw["h"], kw["r_cut"], kw["eta_p"], kw["eta_s"])
        pc.laser_step(DT)
        o = _outputs(api, pc)
        q = pc.heat_source().numpy()
        assert o["tally"] == base["tally"] and np.array_equal(o["cols"][1], base["cols"][1])
        gb.assert_bits(o["cols"][0], base["cols"][0], "transmitted after Set(NULL)")
        gb.assert_bits(q, base["q"], "heat source after Set(NULL)")
        # refusals leave the context unchanged
        pc.set_laser_surface(sm.PLANE_LEVEL, sm.SIDE)
        assert pc.laser_surface_update(_state(api, m, phi)) == 138
        for level, side in ((0.5, 0), (0.5, 2), (np.inf, 1), (np.nan, -1)):
            assert sm.refusal(True, True, level, side) is not None
            pc.set_laser_surface(level, side)
            assert pc.laser_surface_on and pc.laser_surface_facets()[1].size == 138      # configuration and snapshot stay
        pc.couple(None)                                             # uncoupled: the snapshot goes, the configuration stays
        assert pc.laser_surface_on and pc.laser_surface_facets()[1].size == 0
        pc.set_laser_surface(None)
        pc.set_laser_surface(sm.PLANE_LEVEL, sm.SIDE)
        assert not pc.laser_surface_on and sm.refusal(True, False, sm.PLANE_LEVEL, sm.SIDE) == "coupling"
        pc.set_laser(None)
        pc.set_laser_surface(sm.PLANE_LEVEL, sm.SIDE)
        assert not pc.laser_surface_on and sm.refusal(False, False, sm.PLANE_LEVEL, sm.SIDE) == "laser"


def test_two_fresh_contexts_agree_bit_for_bit(api, m):
    kw = sm.beam_args("oblique")
    phi = sm.two_layer_phi(m.xg)
    rng = np.random.default_rng(3)
    x = np.column_stack([rng.uniform(0.2, 0.8, 300), rng.uniform(0.2, 0.8, 300), rng.uniform(0.05, 1.2, 300)])
    a = _run(api, m, kw, phi, 0.0, x=x, groups=[4], source=True)
    c = _run(api, m, kw, phi, 0.0, x=x, groups=[4], source=True)
    gb.assert_bits(a["power"], c["power"], "power")
    gb.assert_bits(a["q"], c["q"], "heat source")
    gb.assert_bits(a["cols"][0], c["cols"][0], "transmitted")
    assert a["tally"] == c["tally"] and np.array_equal(a["cols"][1], c["cols"][1]) and np.array_equal(a["rate"], c["rate"])
    assert (a["power"] > 0.0).any()


def test_heat_source_after_k_steps(api, m):
    kw = sm.beam_args("vertical", scan_vel=(0.4, 0.25, 0.0))
    b = lm.Beam(**kw)
    phi = sm.plane_phi(m.xg)
    cand = sm.Candidates(m.xg, m.ien, phi, sm.PLANE_LEVEL, sm.SIDE, b.dir)
    k, dt = 4, 15 * DT
    with _context(api, m, kw) as (pc, _):
        pc.set_laser_surface(sm.PLANE_LEVEL, sm.SIDE)
        pc.laser_surface_update(_state(api, m, phi))
        for step in range(k):
            if step == 2:                                           # a new snapshot (of the same surface) replaces the node list
                assert pc.laser_surface_update(_state(api, m, phi)) == 138     # while energy is pending: it is kept
            pc.laser_step(dt)
        q = pc.heat_source().numpy()
        again = pc.heat_source().numpy()                            # cleared
    ref, bound = np.zeros(m.num_node, LD), np.zeros(m.num_node)
    for s in range(1, k + 1):
        mdl = sm.step(b, NONE, 0.0, t=s * dt, cand=cand)
        assert mdl["hit"][4][mdl["surf"]].min() > 1e-9
        for nd in mdl["power"]:
            ref[nd] += LD(dt) * mdl["power"][nd]
            bound[nd] += dt * mdl["power_bound"][nd]
    ref, bound = ref / (k * LD(dt)), bound / (k * dt)
    # energy += dt power: two roundings a step; the time k additions; 1 / time and the product; the energy of before and
    # after the second Update reaches q in two additions of two roundings each: (3 k + 8) eps q
    _within("heat_source", q, ref, bound + (3 * k + 8) * EPS * ref.astype(float))
    assert (q[ref == 0] == 0.0).all() and (q > 0.0).any() and (again == 0.0).all()


def test_time_step_takes_the_snapshot(api, m):
    from dedflow_amd.meshgen import synthetic_fields
    kw = sm.beam_args("vertical")
    b = lm.Beam(**kw)
    N = m.num_node
    wg, dw = synthetic_fields(m)
    phi = sm.plane_phi(m.xg)
    with _context(api, m, kw) as (pc, P):
        pc.set_laser_surface(sm.PLANE_LEVEL, sm.SIDE)
        assert pc.laser_surface_update(_state(api, m, phi)) == 138
        wg[4 * N:5 * N] = sm.two_layer_phi(m.xg) + sm.PLANE_LEVEL   # a changed phi in wgold
        st = [api.DeviceArray.from_numpy(a) for a in (wg, 0.1 * dw, 0.1 * dw)]
        F_d, dx_d = api.DeviceArray(6 * N), api.DeviceArray(6 * N)
        P.time_step(st[0], st[1], st[2], F_d, dx_d, newton_maxit=1, particles=pc, dem_substeps=1)
        api.sync()
        after = st[0].numpy()[4 * N:5 * N]                          # the state the sub-steps saw
        cand = sm.Candidates(m.xg, m.ien, after, sm.PLANE_LEVEL, sm.SIDE, b.dir)
        F, tet = pc.laser_surface_facets()
        assert len(tet) == len(cand.tet) != 138 and np.array_equal(tet, cand.tet)
        gb.assert_bits(F, cand.F, "facets of the time step's snapshot")
        assert (pc.laser_columns()[1] <= -2).any()                 # the sub-step's laser step used it


def test_travel(api, m):
    """Copy carries the configuration, not the snapshot; SetLaser keeps the configuration and drops the snapshot; the
    surface goes with the laser"""
    kw = sm.beam_args("vertical")
    phi = sm.plane_phi(m.xg)
    laser = (kw["origin"], kw["direction"], kw["power"], kw["w"], kw["h"], kw["r_cut"], kw["eta_p"], kw["eta_s"])
    with _context(api, m, kw) as (src, _), _context(api, m, kw) as (dst, _):
        w = _state(api, m, phi)
        src.set_laser_surface(sm.PLANE_LEVEL, sm.SIDE)
        assert src.laser_surface_update(w) == 138 and not dst.laser_surface_on
        api.lib().ParticleContextCopy(dst.ctx, src.ctx)
        assert dst.laser_surface_on and dst.laser_surface_facets()[1].size == 0
        assert dst.laser_surface_update(w) == 138                   # level and side came along
        src.laser_step(DT)
        dst.laser_step(DT)
        gb.assert_bits(dst.laser_surface_power().numpy(), src.laser_surface_power().numpy(), "power of the copy")
        src.set_laser(*laser)
        assert src.laser_surface_on and src.laser_surface_facets()[1].size == 0
        assert src.laser_surface_update(w) == 138
        src.set_laser(None)
        assert not src.laser_surface_on
        api.lib().ParticleContextCopy(dst.ctx, src.ctx)             # dst becomes what src is
        assert not dst.laser_on and not dst.laser_surface_on
