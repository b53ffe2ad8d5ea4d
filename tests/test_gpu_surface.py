"""GPU tests of the free-surface forces (include/dedflow.h "free-surface forces"; host/surface.c, csrc/k_surface.hip): the
node sums against tests/surface_model.py (np.longdouble), exact zeros, guard bands, reproducibility, the side switch,
DflTimeStep's wiring against the same step registered by hand, the off path and the state after the nodes moved.

Parity bound.  max|dev - model| / max|model| < 1e-12 per output, the bound of test_gpu_scalar.py for the same kind of kernel
(a fixed-order sum of a few dozen O(50)-operation fp64 terms against longdouble).  The band decision needs no exclusion: a tet
at the edge of the band has delta = 0 at every quadrature point (the kernel is C1), so taking it or leaving it changes nothing
beyond rounding.  With DFL_PARITY_OUT set, the observed ratio of every case goes to that file
(profiles/surface_forces_parity.jsonl is such a run)."""
import ctypes as C

import numpy as np
import pytest

import surface_model as sm
from dedflow_amd.meshgen import fan_mesh, kuhn_cube, single_tet
from guarded_buffers import Pool, Recorder, assert_bits, raw, sent

pytestmark = pytest.mark.gpu
LD = np.longdouble
BOUND = 1e-12
record = Recorder("a")
TILT = np.array([0.2, -0.3, 1.0]) / np.sqrt(1.13)
ALL_ON = dict(sigma0=1.8, dsigma_dT=-4e-4, T_ref=1900.0, recoil_p0=1.0e5, recoil_a=11.0, T_boil=3100.0, h_conv=80.0,
              emissivity=0.4, T_amb=300.0, evap_q0=2.0e9)
MESHES = {"single": single_tet, "cube4": lambda: kuhn_cube(4, jitter=0.2), "cube12": lambda: kuhn_cube(12, jitter=0.2),
          "fan": fan_mesh}
EPS = {"single": 0.5, "cube4": 0.3, "cube12": 2.0 / 12, "fan": 0.5, "cube4flat": 0.25}   # two tet sizes
FIELDS = ["plane", "sphere", "unreached", "wide", "constant"]
CASES = [(mn, f) for mn in MESHES for f in FIELDS] + [("cube4flat", "edge")]


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


_mesh_cache = {}


def _mesh(name):
    if name not in _mesh_cache:
        _mesh_cache[name] = kuhn_cube(4) if name == "cube4flat" else MESHES[name]()
    return _mesh_cache[name]


def case(mesh_name, field):
    """(mesh, w [6N], configuration): T in 1500 .. 3500 everywhere, all terms on"""
    m = _mesh(mesh_name)
    x = m.xg.reshape(-1, 3)
    N = m.num_node
    c = 0.5 * (x.min(axis=0) + x.max(axis=0))
    L = float((x.max(axis=0) - x.min(axis=0)).max())
    level, eps = 0.0, EPS[mesh_name]
    phi = (x - c) @ TILT
    if field == "sphere":
        phi = np.sqrt(((x - c - L * np.array([0.1, 0.05, -0.07])) ** 2).sum(axis=1)) - 0.4 * L
    elif field == "unreached":
        level = 10.0 * L
    elif field == "wide":
        eps = 4.0 * L
    elif field == "constant":                     # every fifth tet holds one value of phi on its four nodes: |g| = 0 exactly
        ien = m.ien.reshape(-1, 4)
        phi = phi.copy()
        phi[ien[::5].reshape(-1)] = 0.0625
    elif field == "edge":                         # vertices at exactly level +- eps |g|
        phi = x[:, 2] - 0.5
    T = 2500.0 + 1000.0 * np.sin(3.0 * x[:, 0] + 2.0 * x[:, 1] + x[:, 2] + 0.3)
    assert T.min() >= 1500.0 and T.max() <= 3500.0
    return m, sm.state(N, phi, T), sm.config(level=level, eps=eps, **ALL_ON)


_model_cache = {}


def model(mesh_name, field):
    """the model's node sums of a case, computed once"""
    if (mesh_name, field) not in _model_cache:
        m, w, cfg = case(mesh_name, field)
        _model_cache[mesh_name, field] = sm.surface_load(m.xg, m.ien, w, cfg)
    return _model_cache[mesh_name, field]


def _device_run(api, pool, P, w, outputs=("load", "heat", "area")):
    """DflMeshSurfaceLoad into guarded NaN-filled outputs; returns the outputs, after the bands and the input were checked"""
    N = P.N
    ws = pool.slot(w)
    size = {"load": 3 * N, "heat": N, "area": N}
    slots = {k: pool.slot(sent(size[k]), off=1) for k in outputs}
    ptr = [slots[k].ptr if k in slots else None for k in ("load", "heat", "area")]
    api.lib().DflMeshSurfaceLoad(P.mesh, ws.ptr, *ptr)
    api.sync()
    ws.check("w")
    return {k: s.check(k, written=True).copy() for k, s in slots.items()}


def _parity(name, got, ref):
    ref = np.asarray(ref, LD).reshape(-1)
    scale = np.abs(ref).max()
    if scale == 0:
        assert not got.any(), name
        return 0.0
    assert np.isfinite(got).all(), name
    ratio = float(np.abs(got.astype(LD) - ref).max() / scale)
    print(f"surface parity {name}: {ratio:.3e}")
    return ratio


@pytest.mark.parametrize("mesh_name,field", CASES)
def test_parity_zeros_and_memory_safety(api, pool, monkeypatch, mesh_name, field):
    m, w, cfg = case(mesh_name, field)
    load, heat, area, active, t = model(mesh_name, field)
    K, T = t["e"].size, m.num_tet
    if field in ("plane", "edge") or (field == "sphere" and mesh_name != "single"):   # (the one tet lies outside that band)
        assert K > 0
    if field == "unreached":
        assert K == 0
    if field == "wide":
        assert K == T
    if field == "constant":
        assert K < T
    if field == "edge":                           # the planes z = 0.25 and z = 0.75 sit exactly on the band's edge
        d = (w[4 * m.num_node:5 * m.num_node] - cfg["level"]) / cfg["eps"]
        assert np.isin(d, [-2.0, -1.0, 0.0, 1.0, 2.0]).all() and K == T // 2
    P = api.Problem(m, bcs=[]) if mesh_name == "single" else api.Problem(m)   # (the single tet has four boundary groups)
    try:
        xg0 = api.d2h(P.mesh.contents.device.contents.xg, 3 * P.N, np.float64)
        ien0 = api.d2h(P.mesh.contents.device.contents.ien, 4 * P.T, np.int32)
        monkeypatch.delenv("DFL_SURFACE_FLAGS", raising=False)
        P.set_surface_forces(**cfg)
        assert P.surface_forces_on
        out = _device_run(api, pool, P, w)
        ref = {"load": load, "heat": heat, "area": area}
        for k in ("load", "heat", "area"):
            ratio = _parity(f"{mesh_name}/{field}/{k}", out[k], ref[k])
            record("surface_node_kernel", f"{mesh_name}/{field}/{k}", ratio / BOUND, active_tets=int(K), tets=int(T))
            assert ratio < BOUND, (k, ratio)
        # nodes none of whose tets lies inside the band are exactly zero
        idle = ~active
        assert not out["load"].reshape(-1, 3)[idle].any() and not out["heat"][idle].any() and not out["area"][idle].any()
        if K == 0:
            assert not any(a.any() for a in out.values())
        else:
            assert out["area"][active].min() >= 0.0 and out["area"].max() > 0.0
        # a NULL output in each position, and a second run: the same bits
        for drop in ("load", "heat", "area"):
            part = _device_run(api, pool, P, w, outputs=[k for k in ("load", "heat", "area") if k != drop])
            for k, a in part.items():
                assert_bits(a, out[k], f"{k} without {drop}")
        # without the one-byte-per-tet band pass in front: the same bits
        monkeypatch.setenv("DFL_SURFACE_FLAGS", "0")
        P.set_surface_forces(**cfg)
        direct = _device_run(api, pool, P, w)
        for k in out:
            assert_bits(direct[k], out[k], f"{k} without the flag pass")
        api.sync()
        assert_bits(api.d2h(P.mesh.contents.device.contents.xg, 3 * P.N, np.float64), xg0, "xg")
        assert np.array_equal(api.d2h(P.mesh.contents.device.contents.ien, 4 * P.T, np.int32), ien0)
    finally:
        P.close()


def _plain_run(api, m, w, cfg, schedule=4):
    P = api.Problem(m, schedule=schedule)
    try:
        P.set_surface_forces(**cfg)
        assert P.surface_forces_on
        out = P.surface_load(api.DeviceArray.from_numpy(w))
        api.sync()
        return {k: a.numpy() for k, a in out.items()}
    finally:
        P.close()


@pytest.mark.parametrize("mesh_name", ["cube12", "fan"])
def test_bitwise_equal_under_both_assembly_schedules(api, mesh_name):
    m, w, cfg = case(mesh_name, "sphere")
    a, b = _plain_run(api, m, w, cfg, 4), _plain_run(api, m, w, cfg, 1)
    for k in a:
        assert_bits(a[k], b[k], k)
        assert np.abs(a[k]).max() > 0.0


def test_side(api):
    m, w, cfg = case("cube12", "sphere")
    off = dict(cfg, recoil_p0=0.0)
    a, b = _plain_run(api, m, w, dict(off, side=1)), _plain_run(api, m, w, dict(off, side=-1))
    for k in a:
        assert_bits(a[k], b[k], k + ", recoil off")
    only = dict(cfg, sigma0=0.0, dsigma_dT=0.0)
    a, b = _plain_run(api, m, w, dict(only, side=1)), _plain_run(api, m, w, dict(only, side=-1))
    assert np.abs(a["load"]).max() > 0.0
    assert np.isfinite(a["load"]).all() and np.array_equal(b["load"], -a["load"])   # (a zero stays +0.0 under both signs)
    assert_bits(a["heat"], b["heat"], "heat")
    assert_bits(a["area"], b["area"], "area")


def test_refusals_and_the_call_without_a_configuration(api, capfd):
    m = _mesh("cube4")
    P = api.Problem(m)
    try:
        good = dict(eps=0.5, **ALL_ON)
        for reason, change in [("side", dict(side=0)), ("eps", dict(eps=0.0)), ("eps", dict(eps=np.inf)),
                               ("sigma0", dict(sigma0=np.nan)), ("T_boil", dict(T_boil=0.0)), ("T_amb", dict(T_amb=np.inf))]:
            P.set_surface_forces(**dict(good, **change))
            assert not P.surface_forces_on and reason in capfd.readouterr().err
        out = api.DeviceArray.from_numpy(sent(3 * P.N))
        api.lib().DflMeshSurfaceLoad(P.mesh, api.DeviceArray(6 * P.N).ptr, out.ptr, None, None)
        api.sync()
        assert "no free-surface forces" in capfd.readouterr().err
        assert_bits(out.numpy(), sent(3 * P.N), "nothing written")
        P.set_surface_forces(**good)
        assert P.surface_forces_on and capfd.readouterr().err == ""
        P.set_surface_forces(**dict(good, side=3))                 # refused: the earlier configuration stays
        assert P.surface_forces_on
        P.set_surface_forces(eps=None)
        assert not P.surface_forces_on
    finally:
        P.close()


def test_after_geometry_changed_the_new_coordinates_are_used(api):
    m, w, cfg = case("cube4", "plane")
    x1 = m.xg.reshape(-1, 3).copy()
    inner = (np.minimum(x1, 1.0 - x1).min(axis=1) > 0.0)
    x1[inner] += np.random.default_rng(9).uniform(-0.03, 0.03, (int(inner.sum()), 3))
    P = api.Problem(m)
    try:
        P.set_surface_forces(**cfg)
        w_d = api.DeviceArray.from_numpy(w)
        before = {k: a.numpy() for k, a in P.surface_load(w_d).items()}
        api.sync()
        api.DeviceArray(3 * P.N, ptr=P.mesh.contents.device.contents.xg).upload(x1.reshape(-1))
        api.lib().DflMeshGeometryChanged(P.mesh)
        after = {k: a.numpy() for k, a in P.surface_load(w_d).items()}
        api.sync()
    finally:
        P.close()
    load, heat, area, _, _ = sm.surface_load(x1.reshape(-1), m.ien, w, cfg)
    for k, ref in (("load", load), ("heat", heat), ("area", area)):
        assert _parity(f"moved/{k}", after[k], ref) < BOUND
        assert _parity(f"moved/{k} against the old coordinates", before[k], ref) > 1e-6


# ---- DflTimeStep ------------------------------------------------------------------------------------------------------------
STEP_CFG = dict(level=0.0, side=-1, eps=2.0 / 6, sigma0=1.8, dsigma_dT=-4e-4, T_ref=1900.0, recoil_p0=40.0, recoil_a=11.0,
                T_boil=3100.0, h_conv=80.0, emissivity=0.4, T_amb=300.0, evap_q0=2.0e3)
STEP_R = 0.01
STEP_MASS = 7800.0 * 4.0 / 3.0 * np.pi * STEP_R ** 3


def _step_state(m):
    """fluid at rest, phi = z - 0.5 (metal below), T in 1500 .. 3500"""
    N = m.num_node
    x = m.xg.reshape(-1, 3)
    return sm.state(N, x[:, 2] - 0.5, 2500.0 + 1000.0 * np.sin(3.0 * x[:, 0] + 2.0 * x[:, 1] + 0.3))


def _registrations(api, P):
    L = api.lib()
    for f in (L.DflMeshExternalLoad, L.DflMeshHeatSource):
        f.restype, f.argtypes = C.c_void_p, [C.POINTER(api.Mesh3D)]
    return L.DflMeshExternalLoad(P.mesh), L.DflMeshHeatSource(P.mesh)


def _step(api, mode, particles=False):
    """one DflTimeStep of kuhn_cube(6) with phi and T transported (after a first step that leaves a reaction load pending when
    `particles`).  mode: "in_step" (in_time_step set), "by_hand" (surface_load at wgold, registered by the caller, and with
    particles a one-way context whose reaction load the caller adds), "cleared" (set, then cleared with NULL), "never" """
    m = kuhn_cube(6)
    N = m.num_node
    P = api.Problem(m, maxit=120, atol=1e-14, rtol=1e-6)
    pc = None
    try:
        P.set_scalar_transport(phi=True, T=True)
        st = [api.DeviceArray.from_numpy(a) for a in (_step_state(m), np.zeros(6 * N), np.zeros(6 * N))]
        F_d, dx_d = api.DeviceArray(6 * N), api.DeviceArray(6 * N)
        o = {}
        if particles:
            xy = np.array([[0.3, 0.3], [0.5, 0.3], [0.7, 0.3], [0.3, 0.6], [0.5, 0.6], [0.7, 0.62]]) + 0.013
            pts = np.c_[xy, np.full(6, 0.62)]
            pc = api.Particles(pts.reshape(-1), np.tile([0.3, 0.0, -1.0], 6), STEP_R, mass=STEP_MASS, dt=1e-3)
            pc.couple(P, rho_f=1.0e3, mu_f=1.0e-3, two_way=(mode == "in_step"))
            P.time_step(st[0], st[1], st[2], F_d, dx_d, newton_maxit=2, particles=pc, dem_substeps=20)
            api.sync()
            o["w1"] = st[0].numpy()
        if mode == "in_step":
            P.set_surface_forces(in_time_step=True, **STEP_CFG)
        elif mode == "by_hand":
            P.set_surface_forces(in_time_step=False, **STEP_CFG)
            q = P.surface_load(st[0], want=("load", "heat"))
            api.sync()
            o["load"], o["heat"] = q["load"].numpy(), q["heat"].numpy()
            if particles:
                o["reaction"] = pc.reaction_load().numpy()
                q["load"] = api.DeviceArray.from_numpy(o["load"] + o["reaction"])
            P.set_external_load(q["load"])
            P.set_heat_source(q["heat"])
        elif mode == "cleared":
            P.set_surface_forces(in_time_step=True, **STEP_CFG)
            P.set_surface_forces(eps=None)
            assert not P.surface_forces_on
        it, rn, r0 = P.time_step(st[0], st[1], st[2], F_d, dx_d, newton_maxit=2, particles=pc, dem_substeps=20 if pc else 0)
        api.sync()
        if mode == "by_hand":
            P.set_external_load(None)
            P.set_heat_source(None)
        o.update(it=it, rn=rn, r0=r0, regs=_registrations(api, P), w=st[0].numpy(), dw=st[2].numpy())
        if pc:
            o["x"] = pc.arrays()[0]
        return o
    finally:
        if pc:
            pc.close()
        P.close()


def _same_step(a, b, keys=("rn", "r0", "w", "dw")):
    assert a["it"] == b["it"]
    for k in keys:
        assert np.isfinite(a[k]).all(), k
        assert_bits(a[k], b[k], k)


def test_time_step_applies_load_and_heat_loss_itself(api):
    a, b, c = _step(api, "in_step"), _step(api, "by_hand"), _step(api, "never")
    assert np.abs(b["load"]).max() > 0.0 and np.abs(b["heat"]).max() > 0.0
    _same_step(a, b)
    assert a["regs"] == (None, None)                                     # restored after the solve
    assert a["r0"][0] > c["r0"][0] and a["r0"][3] != c["r0"][3]          # the terms reached the momentum and the T rows
    assert (raw(a["w"]) != raw(c["w"])).any()


def test_time_step_merges_a_pending_reaction_load(api):
    a, b = _step(api, "in_step", particles=True), _step(api, "by_hand", particles=True)
    assert_bits(a["w1"], b["w1"], "the state after the first step")
    assert np.abs(b["reaction"]).max() > 0.0 and np.abs(b["load"]).max() > 0.0
    _same_step(a, b, keys=("rn", "r0", "w", "dw", "x"))
    assert a["regs"] == (None, None)


def test_cleared_steps_like_never_set(api):
    _same_step(_step(api, "cleared"), _step(api, "never"))
