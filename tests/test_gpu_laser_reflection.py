"""GPU tests of the laser's reflections (host/laser_reflect.c, csrc/k_laser_reflect.hip; model in include/dedflow.h "laser
reflections").  Decisions -- which facets are in the reflection list, which facet a ray hits at every bounce -- are compared
exactly with tests/laser_reflection_model.py; absorbed powers, nodal power, both tallies and the heat source within the
model's a-priori bounds (its docstring derives them; there is no fitted tolerance).

Inputs: kuhn_cube(6, jitter=0.2), 16 x 16 columns, a vertical and an oblique beam, a groove, a cone and a tilted plane,
eps = 0.25, max_bounce = 6.  test_laser_reflection_cpu.py checks in the model alone that every ray of these inputs decides
with a margin of more than 1e-9.  With DFL_PARITY_OUT set, the observed error and bound of every check go to that file
(profiles/laser_reflection_parity.jsonl is such a run)."""
import contextlib
import json
import os

import numpy as np
import pytest

import guarded_buffers as gb
import laser_reflection_model as rf
import laser_surface_model as sm

pytestmark = pytest.mark.gpu
EPS, LD = rf.EPS, rf.LD
KEYS = ("outside", "absorbed_particles", "scattered", "substrate", "reflected", "missed")
DT = 1e-3
NONE = np.zeros((0, 3))
R_P = 0.004
CASES = [(f, d) for f in sorted(rf.FIELDS) for d in sorted(rf.DIRECTIONS)]


@pytest.fixture(scope="module")
def api():
    from dedflow_amd import api as A
    A.lib()
    return A


@pytest.fixture(scope="module")
def m():
    return rf.mesh()


@pytest.fixture(scope="module")
def models(m):
    """the model's step of every shared input, computed once"""
    cache = {}

    def get(field, direction, model=1, max_bounce=rf.MAX_BOUNCE):
        key = (field, direction, model, max_bounce)
        if key not in cache:
            cache[key] = rf.case(m, field, direction, model=model, max_bounce=max_bounce)
        return cache[key]
    return get


def _mass(r, rho_p=7800.0):
    return rho_p * 4.0 / 3.0 * np.pi * np.asarray(r) ** 3


def _state(api, m, phi):
    w = np.zeros(6 * m.num_node)
    w[4 * m.num_node:5 * m.num_node] = phi
    return api.DeviceArray.from_numpy(w)


@contextlib.contextmanager
def _context(api, m, kw, x=NONE):
    x = np.asarray(x, np.float64).reshape(-1, 3)
    P = api.Problem(m)
    pc = api.Particles(x.reshape(-1), np.zeros(x.size), R_P, mass=float(_mass(R_P)), dt=DT)
    try:
        pc.set_heat(cp_p=500.0, T_init=300.0)
        pc.couple(P)
        pc.set_laser(kw["origin"], kw["direction"], kw["power"], kw["w"], kw["h"], kw["r_cut"], kw["eta_p"], kw["eta_s"],
                     kw.get("scan_vel", (0.0, 0.0, 0.0)), ())
        assert pc.laser_on
        pc.set_laser_surface(rf.LEVEL, rf.SIDE)
        assert pc.laser_surface_on
        yield pc, P
    finally:
        pc.close()
        P.close()


def _outputs(api, pc, P=0, source=False):
    out = dict(power=pc.laser_surface_power().numpy(), tally=pc.laser_tally(), cols=pc.laser_columns(),
               rate=pc.laser_rate() if P else np.zeros(0), surf=pc.laser_surface_facets())
    if pc.laser_reflection_on:
        out.update(rtally=pc.laser_reflection_tally(), rays=pc.laser_reflection_rays(), R=pc.laser_reflection_facets())
    if source:
        out["q"] = pc.heat_source().numpy()
    api.sync()
    return out


def _run(api, m, direction, field, reflection=(rf.MAX_BOUNCE, 1, rf.EPS_MAT), x=NONE, source=False, clear=False):
    """one laser step on a fresh context; reflection None: never set; clear: set, then cleared with NULL before the Update"""
    kw = sm.beam_args(direction)
    with _context(api, m, kw, x) as (pc, _):
        if reflection is not None:
            pc.set_laser_reflection(*reflection)
            assert pc.laser_reflection_on
            if clear:
                pc.set_laser_reflection(None)
                assert not pc.laser_reflection_on
        nf = pc.laser_surface_update(_state(api, m, rf.FIELDS[field](m.xg)))
        pc.laser_step(DT)
        out = _outputs(api, pc, len(x), source)
        out["nf"] = nf
        return out


def _within(name, got, ref, bound):
    d = np.abs(np.asarray(got, LD) - np.asarray(ref, LD))
    bound = np.broadcast_to(np.asarray(bound, np.float64), d.shape)
    if d.size:
        k = int(np.argmax(d / np.maximum(bound, 1e-300)))
        print(f"laser reflection {name}: error {float(d.flat[k]):.3e} bound {float(bound.flat[k]):.3e}")
        if os.environ.get("DFL_PARITY_OUT"):
            with open(os.environ["DFL_PARITY_OUT"], "a") as f:
                f.write(json.dumps(dict(name=name, err=float(d.flat[k]), bound=float(bound.flat[k]))) + "\n")
        assert (d <= bound).all(), (name, float(d.flat[k]), float(bound.flat[k]))


def _same_bits(a, b, what):
    """every output of a surface step, bit for bit"""
    gb.assert_bits(a["power"], b["power"], f"{what}: power")
    gb.assert_bits(a["cols"][0], b["cols"][0], f"{what}: transmitted")
    gb.assert_bits(a["surf"][0], b["surf"][0], f"{what}: facets")
    assert np.array_equal(a["cols"][1], b["cols"][1]) and np.array_equal(a["surf"][1], b["surf"][1]), what
    assert a["tally"] == b["tally"], (what, a["tally"], b["tally"])
    assert np.array_equal(a["rate"], b["rate"]), what
    if "q" in a and "q" in b:
        gb.assert_bits(a["q"], b["q"], f"{what}: heat source")


def _check(name, o, b, cand, R, mdl, N, count=0):
    # the lists
    assert o["nf"] == len(cand.tet) and np.array_equal(o["surf"][1], cand.tet)
    gb.assert_bits(o["surf"][0], cand.F, "candidate facets with a reflection set")
    F, tet, g = o["R"]
    assert np.array_equal(tet, R.tet)
    gb.assert_bits(F, R.F, "R facets")
    gb.assert_bits(g, R.g, "R gradients")
    # decisions
    facet, absorbed = o["rays"]
    assert np.array_equal(o["cols"][1], mdl["face"])
    assert np.array_equal(facet, mdl["facet_r"])
    # values
    _within(f"{name}_absorbed", absorbed, mdl["absorbed"], mdl["absorbed_bound"])
    assert (absorbed[mdl["facet_r"] < 0] == 0.0).all()
    nodes = np.array(sorted(mdl["power"]), np.int64)
    rest = np.setdiff1d(np.arange(N), nodes)
    assert (o["power"][rest] == 0.0).all() and np.isfinite(o["power"]).all()
    _within(f"{name}_power", o["power"][nodes], [mdl["power"][k] for k in nodes], [mdl["power_bound"][k] for k in nodes])
    rt, mt, mb = o["rtally"], mdl["rtally"], mdl["rtally_bound"]
    assert np.array_equal(rt["rays"], mt["rays"])
    _within(f"{name}_rtally_absorbed", rt["absorbed"], mt["absorbed"], mb["absorbed"])
    _within(f"{name}_rtally_escaped", rt["escaped"], mt["escaped"], mb["escaped"])
    _within(f"{name}_rtally_remaining", rt["remaining"], mt["remaining"], mb["remaining"])
    extra = float(mdl["rate_bound"].sum()) / b.eta_p
    total = sum(LD(o["tally"][k]) for k in KEYS)
    _within(f"{name}_identity", total, b.power, (b.ncol + count) * EPS * b.power + mdl["tally_extra"]["substrate"]
            + mdl["tally_extra"]["reflected"])
    for k in KEYS:
        _within(f"{name}_tally_{k}", o["tally"][k], mdl["tally"][k],
                extra + (b.ncol + count) * EPS * b.power + mdl["tally_extra"].get(k, 0.0))
    if "q" in o:
        # one step: energy = dt power, q = energy / dt: 3 roundings
        _within(f"{name}_heat_source", o["q"][nodes], [mdl["power"][k] for k in nodes],
                [mdl["power_bound"][k] + 3 * EPS * float(mdl["power"][k]) for k in nodes])
        assert (o["q"][rest] == 0.0).all()


@pytest.mark.parametrize("field,direction", CASES)
def test_against_the_model(api, m, models, field, direction):
    b, cand, R, mdl = models(field, direction)
    o = _run(api, m, direction, field, source=True)
    _check(f"{field}_{direction}", o, b, cand, R, mdl, m.num_node)
    if field == "plane":
        assert o["rtally"]["rays"][1:].sum() == 0                   # no ray finds a second facet: no self-hit
    if field == "groove":
        assert o["rtally"]["rays"][1] > 0 and (o["rtally"]["remaining"] > 0.0) == (direction == "oblique")


@pytest.mark.parametrize("direction", sorted(rf.DIRECTIONS))
def test_model_0_against_the_model(api, m, models, direction):
    b, cand, R, mdl = models("groove", direction, model=0, max_bounce=3)
    o = _run(api, m, direction, "groove", reflection=(3, 0, 0.0), source=True)
    _check(f"groove_{direction}_model0", o, b, cand, R, mdl, m.num_node)


@pytest.mark.parametrize("direction", sorted(rf.DIRECTIONS))
def test_model_0_on_the_plane_has_the_bits_of_the_surface_alone(api, m, direction):
    a = _run(api, m, direction, "plane", reflection=(4, 0, 0.0), source=True)
    c = _run(api, m, direction, "plane", reflection=None, source=True)
    _same_bits(a, c, "model 0 on the plane")
    assert a["rtally"]["rays"][0] > 0 and a["rtally"]["rays"][1:].sum() == 0


@pytest.mark.parametrize("field", ["groove", "plane"])
def test_cleared_is_never_set(api, m, field):
    """set and cleared with NULL: every output of the surface step has the bits of a context that never set a reflection"""
    a = _run(api, m, "oblique", field, clear=True, source=True)
    c = _run(api, m, "oblique", field, reflection=None, source=True)
    _same_bits(a, c, "cleared")
    assert "rtally" not in a


def test_run_to_run_and_after_the_lists_grew(api, m):
    kw = sm.beam_args("oblique")
    a = _run(api, m, "oblique", "groove", source=True)
    c = _run(api, m, "oblique", "groove", source=True)
    with _context(api, m, kw) as (pc, _):
        pc.set_laser_reflection(rf.MAX_BOUNCE, 1, rf.EPS_MAT)
        pc.laser_surface_update(_state(api, m, rf.plane_phi(m.xg)))  # 320 facets: the lists grow from their first capacity
        pc.laser_step(DT)
        pc.heat_source()                                            # (clears the plane's energy)
        pc.set_laser(kw["origin"], kw["direction"], kw["power"], kw["w"], kw["h"], kw["r_cut"], kw["eta_p"], kw["eta_s"])
        assert pc.laser_reflection_on and pc.laser_reflection_facets()[1].size == 0    # SetLaser: configuration kept, lists dropped
        pc.laser_surface_update(_state(api, m, rf.groove_phi(m.xg)))                    # 496: they grow again
        pc.laser_step(DT)
        g = _outputs(api, pc, source=True)
    for other, what in ((c, "run to run"), (g, "after the lists grew")):
        _same_bits(a, other, what)
        assert np.array_equal(a["rays"][0], other["rays"][0])
        gb.assert_bits(a["rays"][1], other["rays"][1], f"{what}: absorbed")
        gb.assert_bits(a["R"][0], other["R"][0], f"{what}: R")
        assert np.array_equal(a["rtally"]["rays"], other["rtally"]["rays"])
        gb.assert_bits(a["rtally"]["absorbed"], other["rtally"]["absorbed"], f"{what}: tally")
        assert a["rtally"]["escaped"] == other["rtally"]["escaped"] and a["rtally"]["remaining"] == other["rtally"]["remaining"]


@pytest.mark.parametrize("cells,group", [("1", "64"), ("3", "16"), ("7", "64"), ("40", "16"), ("256", "64")])
def test_the_grid_changes_no_bit(api, m, monkeypatch, cells, group):
    """the cell grid at other resolutions (DFL_LASER_REFLECT_CELLS cells per axis, read by Set) and with the other lane-group
    size (DFL_LASER_REFLECT_GROUP): the bits of the default"""
    a = _run(api, m, "oblique", "groove", source=True)
    monkeypatch.setenv("DFL_LASER_REFLECT_CELLS", cells)
    monkeypatch.setenv("DFL_LASER_REFLECT_GROUP", group)
    for field, ref in (("groove", a), ("cone", None)):
        o = _run(api, m, "oblique", field, source=True)
        if ref is None:
            monkeypatch.delenv("DFL_LASER_REFLECT_CELLS")
            monkeypatch.delenv("DFL_LASER_REFLECT_GROUP")
            ref = _run(api, m, "oblique", field, source=True)
        _same_bits(ref, o, f"{cells} cells per axis, {group} lanes")
        assert np.array_equal(ref["rays"][0], o["rays"][0])
        gb.assert_bits(ref["rays"][1], o["rays"][1], "absorbed")
        gb.assert_bits(ref["rtally"]["absorbed"], o["rtally"]["absorbed"], "tally")
        assert ref["rtally"]["escaped"] == o["rtally"]["escaped"] and ref["rtally"]["remaining"] == o["rtally"]["remaining"]


def test_particles_in_the_beam(api, m):
    """shadowing is unchanged by the reflections, and the rays start from the attenuated T_c"""
    rng = np.random.default_rng(7)
    x = np.column_stack([rng.uniform(0.3, 0.7, 200), rng.uniform(0.3, 0.7, 200), rng.uniform(0.85, 1.2, 200)])
    b, cand, R, mdl = rf.case(m, "groove", "vertical", x=x, r=R_P)
    o = _run(api, m, "vertical", "groove", x=x, source=True)
    base = _run(api, m, "vertical", "groove", reflection=None, x=x)
    assert np.array_equal(o["rate"], base["rate"]) and (o["rate"] > 0.0).any()
    gb.assert_bits(o["cols"][0], base["cols"][0], "transmitted with particles")
    assert np.array_equal(o["cols"][1], base["cols"][1])
    assert (mdl["T"] < b.column_power() * (1 - 1e-6)).any()         # some columns are attenuated
    _check("groove_vertical_particles", o, b, cand, R, mdl, m.num_node, count=len(x))


def test_refusals_and_travel(api, m):
    kw = sm.beam_args("vertical")
    laser = (kw["origin"], kw["direction"], kw["power"], kw["w"], kw["h"], kw["r_cut"], kw["eta_p"], kw["eta_s"])
    w = _state(api, m, rf.groove_phi(m.xg))
    with _context(api, m, kw) as (src, P), _context(api, m, kw) as (dst, _):
        for cfg in ((0, 1, 0.25), (9, 1, 0.25), (4, 2, 0.25), (4, -1, 0.25), (4, 1, 0.0), (4, 1, -1.0), (4, 1, np.nan), (4, 1, np.inf)):
            assert rf.refusal(True, True, *cfg) is not None
            src.set_laser_reflection(*cfg)
            assert not src.laser_reflection_on
        src.set_laser_reflection(8, 0, np.nan)                      # model 0 ignores eps
        assert src.laser_reflection_on and rf.refusal(True, True, 8, 0, np.nan) is None
        src.set_laser_reflection(5, 1, 0.3)
        src.set_laser_reflection(0, 1, 0.3)                         # refused: the configuration stays
        assert src.laser_reflection_on
        assert src.laser_surface_update(w) == 493 and src.laser_reflection_facets()[1].size == 496
        src.laser_step(DT)
        assert src.laser_reflection_rays()[0].shape == (6, 256)
        # Copy: the configuration, not the lists
        api.lib().ParticleContextCopy(dst.ctx, src.ctx)
        assert dst.laser_reflection_on and dst.laser_reflection_facets()[1].size == 0 and dst.laser_reflection_rays()[0] is None
        assert dst.laser_surface_update(w) == 493
        dst.laser_step(DT)
        assert dst.laser_reflection_rays()[0].shape == (6, 256)     # max_bounce came along
        gb.assert_bits(dst.laser_surface_power().numpy(), src.laser_surface_power().numpy(), "power of the copy")
        # SetLaser keeps the configuration and drops the snapshot
        src.set_laser(*laser)
        assert src.laser_reflection_on and src.laser_reflection_facets()[1].size == 0
        assert src.laser_surface_update(w) == 493 and src.laser_reflection_facets()[1].size == 496
        # the coupling drops the lists
        src.couple(None)
        assert src.laser_reflection_on and src.laser_reflection_facets()[1].size == 0
        src.couple(P)
        assert src.laser_reflection_on and src.laser_reflection_facets()[1].size == 0
        assert src.laser_surface_update(w) == 493 and src.laser_reflection_facets()[1].size == 496
        # SetLaserSurface(NULL) clears the reflection; without a surface, or a laser, it is refused
        src.set_laser_surface(None)
        assert not src.laser_reflection_on
        t = src.laser_reflection_tally()
        assert t["escaped"] == 0.0 and not t["absorbed"].any() and not t["rays"].any()
        src.set_laser_reflection(4, 1, 0.25)
        assert not src.laser_reflection_on and rf.refusal(True, False, 4, 1, 0.25) == "surface"
        src.set_laser(None)
        src.set_laser_reflection(4, 1, 0.25)
        assert not src.laser_reflection_on and rf.refusal(False, False, 4, 1, 0.25) == "laser"
        api.lib().ParticleContextCopy(dst.ctx, src.ctx)             # dst becomes what src is
        assert not dst.laser_on and not dst.laser_reflection_on
