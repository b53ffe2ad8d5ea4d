"""GPU tests of the phase change (include/dedflow.h "phase change"; host/phase.c, csrc/k_phase.hip): the node sums D, H, G
against tests/phase_model.py (np.longdouble), exact zeros, guard bands, reproducibility, the row updates of F, J and JT bit for
bit from the device's own D and H, the off path, a solid that holds still, latent heat that slows heating, the statistics and
the refusals.

Parity bound.  max|dev - model| / max|model| <= 1e-12 per output, the bound of test_gpu_surface.py for the same kind of kernel
(a fixed-order sum of a few dozen O(50)-operation fp64 terms against longdouble; observed there at the 1e-15 scale, so about
1000x margin).  darcy_b = 1e-3, where C's relative condition in fl is about 10.  The skip rules need no exclusion: fl, fl', C
and Hs are continuous where the rules switch, so a tet at the edge adds nothing beyond rounding whether it is taken or left.
With DFL_PARITY_OUT set, the observed ratio of every case goes to that file (profiles/phase_change_parity.jsonl is such a
run)."""
import ctypes as C

import numpy as np
import pytest

import phase_model as pm
from dedflow_amd.meshgen import fan_mesh, kuhn_cube, single_tet
from guarded_buffers import Pool, Recorder, assert_bits, raw, sent

pytestmark = pytest.mark.gpu
LD = np.longdouble
BOUND = 1e-12
record = Recorder("a")
TILT = np.array([0.2, -0.3, 1.0]) / np.sqrt(1.13)
BASE = dict(T_solidus=1600.0, T_liquidus=1700.0, latent=2.0e9, darcy_c=1.0e6, darcy_b=1e-3)
MESHES = {"single": single_tet, "cube2": lambda: kuhn_cube(2), "cube6": lambda: kuhn_cube(6, jitter=0.2), "fan": fan_mesh}
EPS = {"single": 0.5, "cube2": 0.4, "cube6": 0.3, "fan": 0.5}
FIELDS = ["solid", "liquid", "gas", "linear", "linear_phi", "random"]
CASES = [(mn, f) for mn in MESHES for f in FIELDS]
OUT = ("D", "H", "G")


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
        _mesh_cache[name] = MESHES[name]()
    return _mesh_cache[name]


def _problem(api, mesh_name, **kw):
    m = _mesh(mesh_name)
    return api.Problem(m, bcs=[], **kw) if mesh_name == "single" else api.Problem(m, **kw)   # (the tet has four groups)


def case(mesh_name, field):
    """(mesh, w [6N], configuration)"""
    m = _mesh(mesh_name)
    x = m.xg.reshape(-1, 3)
    N = m.num_node
    c = 0.5 * (x.min(axis=0) + x.max(axis=0))
    L = float((x.max(axis=0) - x.min(axis=0)).max())
    s = (x - c) @ TILT / L                                  # about -0.6 .. 0.6
    phi = (x - c) @ np.array([0.3, 0.1, -1.0]) / np.sqrt(1.1)
    cfg = dict(BASE)
    T = 1650.0 + 250.0 * s                                  # through the whole range
    if field == "solid":
        T = 1500.0 + 90.0 * s
    elif field == "liquid":
        T = 1800.0 + 90.0 * s
    elif field == "gas":
        cfg.update(use_phi=True, side=1, level=10.0 * L, eps=EPS[mesh_name])
    elif field == "linear_phi":
        cfg.update(use_phi=True, side=1, level=0.05 * L, eps=EPS[mesh_name])
    elif field == "random":
        T = np.random.default_rng(17).uniform(1550.0, 1750.0, N)
        T[1:: max(3, N // 4)] = np.nan                      # (not node 0: every tet of the fan holds it)
    return m, pm.state(N, phi, T), pm.config(**cfg)


_model_cache = {}


def model(mesh_name, field):
    if (mesh_name, field) not in _model_cache:
        m, w, cfg = case(mesh_name, field)
        _model_cache[mesh_name, field] = pm.coefficients(m.xg, m.ien, w, cfg)
    return _model_cache[mesh_name, field]


def _device_run(api, pool, P, w, outputs=OUT):
    """DflMeshPhaseCoefficients into guarded NaN-filled outputs; returns them, after the bands and the input were checked"""
    ws = pool.slot(w)
    slots = {k: pool.slot(sent(P.N), off=1) for k in outputs}
    api.lib().DflMeshPhaseCoefficients(P.mesh, ws.ptr, *[slots[k].ptr if k in slots else None for k in OUT])
    api.sync()
    ws.check("w")
    return {k: s.check(k, written=True).copy() for k, s in slots.items()}


def _parity(name, got, ref):
    ref = np.asarray(ref, LD).reshape(-1)
    scale = np.abs(ref).max()
    if scale == 0:
        assert_bits(got, np.zeros(got.size), name)
        return 0.0
    assert np.isfinite(got).all(), name
    ratio = float(np.abs(got.astype(LD) - ref).max() / scale)
    print(f"phase parity {name}: {ratio:.3e}")
    return ratio


@pytest.mark.parametrize("mesh_name,field", CASES)
def test_parity_zeros_memory_safety_and_stats(api, pool, monkeypatch, mesh_name, field):
    m, w, cfg = case(mesh_name, field)
    ref = model(mesh_name, field)
    nc, nv, T = int(ref["tets"]["coeff"].sum()), int(ref["tets"]["vol"].sum()), m.num_tet
    if field == "solid":
        assert nc == T and nv == 0
    if field == "liquid":
        assert nc == 0 and nv == T
    if field == "gas":
        assert nc == 0 and nv == 0
    if field in ("linear", "linear_phi", "random") and mesh_name == "cube6":   # (the coarser meshes have no tet to skip)
        assert 0 < nc < T and 0 < nv < T
    P = _problem(api, mesh_name)
    try:
        xg0 = api.d2h(P.mesh.contents.device.contents.xg, 3 * P.N, np.float64)
        ien0 = api.d2h(P.mesh.contents.device.contents.ien, 4 * P.T, np.int32)
        monkeypatch.setenv("DFL_PHASE_FLAGS", "1")              # with the one-byte-per-tet flag pass in front
        P.set_phase_change(**cfg)
        assert P.phase_change_on
        out = _device_run(api, pool, P, w)
        for k in OUT:
            ratio = _parity(f"{mesh_name}/{field}/{k}", out[k], ref[k])
            record("phase_node_kernel", f"{mesh_name}/{field}/{k}", ratio / BOUND, coeff_tets=nc, volume_tets=nv, tets=int(T))
            assert ratio <= BOUND, (k, ratio)
        # nodes none of whose tets adds to a sum hold exactly +0.0 there
        zero = np.zeros(P.N)
        assert_bits(out["D"][~ref["touched_c"]], zero[~ref["touched_c"]], "D of untouched nodes")
        assert_bits(out["H"][~ref["touched_c"]], zero[~ref["touched_c"]], "H of untouched nodes")
        assert_bits(out["G"][~ref["touched_v"]], zero[~ref["touched_v"]], "G of untouched nodes")
        assert min(a.min() for a in out.values()) >= 0.0
        # a NULL output in each position, and so a second and third run: the same bits
        for drop in OUT:
            part = _device_run(api, pool, P, w, outputs=[k for k in OUT if k != drop])
            for k, a in part.items():
                assert_bits(a, out[k], f"{k} without {drop}")
        # the statistics at the same state
        st = P.phase_stats(api.DeviceArray.from_numpy(w))
        want = pm.stats(m.xg, w, cfg, out["G"])
        assert abs(LD(st["liquid_volume"]) - want["liquid_volume"]) <= 1e-13 * float(np.abs(out["G"]).sum())
        assert st["molten"] == want["molten"] and st["T_max"] == want["T_max"]
        assert np.array_equal(st["lo"], want["lo"]) and np.array_equal(st["hi"], want["hi"])
        if field in ("solid", "gas"):                          # the empty set
            assert st["molten"] == 0 and np.all(st["lo"] == np.inf) and np.all(st["hi"] == -np.inf)
            assert st["liquid_volume"] == 0.0
        if field == "gas":
            assert st["T_max"] == -np.inf
        if field == "liquid":
            assert st["molten"] == P.N
        # a switched-off part is exactly +0.0 and leaves the other part's bits alone
        P.set_phase_change(**dict(cfg, latent=0.0))
        part = _device_run(api, pool, P, w)
        assert_bits(part["H"], zero, "H with latent = 0")
        assert_bits(part["D"], out["D"], "D with latent = 0")
        assert_bits(part["G"], out["G"], "G with latent = 0")
        P.set_phase_change(**dict(cfg, darcy_c=0.0))
        part = _device_run(api, pool, P, w)
        assert_bits(part["D"], zero, "D with darcy_c = 0")
        assert_bits(part["H"], out["H"], "H with darcy_c = 0")
        # without the one-byte-per-tet flag pass in front: the same bits
        monkeypatch.setenv("DFL_PHASE_FLAGS", "0")
        P.set_phase_change(**cfg)
        direct = _device_run(api, pool, P, w)
        for k in OUT:
            assert_bits(direct[k], out[k], f"{k} without the flag pass")
        monkeypatch.delenv("DFL_PHASE_FLAGS")                   # and the default
        P.set_phase_change(**cfg)
        direct = _device_run(api, pool, P, w)
        for k in OUT:
            assert_bits(direct[k], out[k], f"{k} by default")
        api.sync()
        assert_bits(api.d2h(P.mesh.contents.device.contents.xg, 3 * P.N, np.float64), xg0, "xg")
        assert np.array_equal(api.d2h(P.mesh.contents.device.contents.ien, 4 * P.T, np.int32), ien0)
    finally:
        P.close()


@pytest.mark.parametrize("mesh_name", ["cube6", "fan"])
def test_bitwise_equal_under_both_assembly_schedules(api, mesh_name):
    m, w, cfg = case(mesh_name, "linear_phi")
    res = []
    for schedule in (4, 1):
        P = _problem(api, mesh_name, schedule=schedule)
        try:
            P.set_phase_change(**cfg)
            out = P.phase_coefficients(api.DeviceArray.from_numpy(w))
            api.sync()
            res.append({k: a.numpy() for k, a in out.items()})
        finally:
            P.close()
    for k in OUT:
        assert_bits(res[0][k], res[1][k], k)
        assert np.abs(res[0][k]).max() > 0.0


# ---- the assemblies ---------------------------------------------------------------------------------------------------------
def _alpha_fields(m):
    """alpha-level states with a velocity field, rates on every slot and T through the melting range"""
    from dedflow_amd.meshgen import synthetic_fields
    N = m.num_node
    wg, dwg = synthetic_fields(m)
    x = m.xg.reshape(-1, 3)
    wg[5 * N:] = 1650.0 + 120.0 * ((x - 0.5) @ TILT)
    dwg[5 * N:] *= 40.0
    return wg, dwg


def _assemblies(api, m, mode, schedule=4, cfg=None):
    """F, the saved phi / T rows, J's block values and JT of one mesh at _alpha_fields; mode "never", "cleared" or "on" """
    N = m.num_node
    wg, dwg = _alpha_fields(m)
    P = api.Problem(m, schedule=schedule)
    try:
        P.set_scalar_transport(phi=True, T=True, dirichlet_T=(0,))
        o = {}
        if mode in ("on", "cleared"):
            P.set_phase_change(**(cfg or BASE))
        if mode == "cleared":
            P.set_phase_change()
            assert not P.phase_change_on
        wd, dd, F = api.DeviceArray.from_numpy(wg), api.DeviceArray.from_numpy(dwg), api.DeviceArray(6 * N)
        if mode == "on":
            c = P.phase_coefficients(wd, want=("D", "H"))
            api.sync()
            o["D"], o["H"] = c["D"].numpy(), c["H"].numpy()
        P.assemble_system(wd, dd, F, want_J=False)
        api.sync()
        o["F"], o["res"] = F.numpy(), P.scalar_residual()
        P.assemble_system(wd, dd, None, want_J=True)
        api.sync()
        o["J"] = P.block_values().numpy()
        P.assemble_system(wd, dd, F, want_J=True)             # both in one call: the same
        api.sync()
        o["F2"], o["J2"] = F.numpy(), P.block_values().numpy()
        o["JT"] = P.assemble_scalar_jacobian(wd, dd)[1]
        o["pattern"] = P.pattern()
        o["wg"], o["dwg"] = wg, dwg
        return o
    finally:
        P.close()


def _dirichlet_rows(m, bcs):
    """boolean [N, 3]: the momentum rows a strong condition holds"""
    held = np.zeros((m.num_node, 3), bool)
    for g, comp in bcs:
        nodes = m.bound_node[m.bound_node_offset[g]:m.bound_node_offset[g + 1]]
        for d in range(3):
            if comp[d]:
                held[nodes, d] = True
    return held


@pytest.mark.parametrize("schedule", [4, 1])
def test_row_updates_bit_for_bit(api, schedule):
    from dedflow_amd.api import REFERENCE_BCS
    m = _mesh("cube6")
    N = m.num_node
    off, on = _assemblies(api, m, "never", schedule), _assemblies(api, m, "on", schedule)
    D, H = on["D"], on["H"]
    assert D.max() > 0.0 and H.max() > 0.0 and (D == 0.0).any()
    held = _dirichlet_rows(m, REFERENCE_BCS)
    assert held.any() and not held.all()
    heldT = np.zeros(N, bool)
    heldT[m.bound_node[m.bound_node_offset[0]:m.bound_node_offset[1]]] = True
    # F: momentum rows
    want = pm.update_F(off["F"], D, None, on["wg"], on["dwg"])
    free = ~held.reshape(-1)
    assert_bits(on["F"][:3 * N][free], want[:3 * N][free], "momentum rows")
    assert_bits(on["F"][:3 * N][~free], off["F"][:3 * N][~free], "Dirichlet rows of F")
    assert (raw(on["F"][:3 * N]) != raw(off["F"][:3 * N])).any()
    assert_bits(on["F"][3 * N:], off["F"][3 * N:], "p, phi and T rows of F")
    assert_bits(on["F2"], on["F"], "F of the (F, J) call")
    # the saved T rows
    wantT = off["res"][N:] + H * on["dwg"][5 * N:]
    assert_bits(on["res"][N:][~heldT], wantT[~heldT], "saved T rows")
    assert_bits(on["res"][N:][heldT], off["res"][N:][heldT], "held T rows")
    assert_bits(on["res"][:N], off["res"][:N], "saved phi rows")
    assert (raw(on["res"][N:]) != raw(off["res"][N:])).any()
    # J: the (d, d) entries of the diagonal blocks of rows that are not held, nothing else
    rp, ci = on["pattern"]
    k = pm.diagonal_positions(rp, ci)
    wantJ = pm.update_J(off["J"], D, rp, ci).reshape(-1, 16)
    offJ = off["J"].reshape(-1, 16)
    for d in range(3):
        wantJ[k[held[:, d]], 5 * d] = offJ[k[held[:, d]], 5 * d]
    assert_bits(on["J"], wantJ.reshape(-1), "J")
    assert (raw(on["J"]) != raw(off["J"])).any()
    assert_bits(on["J2"], on["J"], "J of the (F, J) call")
    # JT
    wantJT = pm.update_JT(off["JT"], H, rp, ci)
    wantJT[k[heldT]] = off["JT"][k[heldT]]
    assert_bits(on["JT"], wantJT, "JT")
    assert (raw(on["JT"]) != raw(off["JT"])).any()


def _step(api, m, mode, cfg=None, newton_maxit=2):
    N = m.num_node
    wg, dwg = _alpha_fields(m)
    P = api.Problem(m, maxit=120, atol=1e-14, rtol=1e-6)
    try:
        P.set_scalar_transport(phi=True, T=True)
        if mode in ("on", "cleared"):
            P.set_phase_change(**(cfg or BASE))
        if mode == "cleared":
            P.set_phase_change()
        st = [api.DeviceArray.from_numpy(a) for a in (wg, 0.1 * dwg, 0.1 * dwg)]
        F_d, dx_d = api.DeviceArray(6 * N), api.DeviceArray(6 * N)
        it, rn, r0 = P.time_step(st[0], st[1], st[2], F_d, dx_d, newton_maxit=newton_maxit)
        api.sync()
        return dict(it=it, rn=rn, r0=r0, w=st[0].numpy(), dw=st[2].numpy())
    finally:
        P.close()


def test_off_is_off(api):
    m = _mesh("cube6")
    a, b = _assemblies(api, m, "never"), _assemblies(api, m, "cleared")
    for k in ("F", "res", "J", "F2", "J2", "JT"):
        assert_bits(a[k], b[k], k)
    s, t = _step(api, m, "never"), _step(api, m, "cleared")
    assert s["it"] == t["it"]
    for k in ("rn", "r0", "w", "dw"):
        assert np.isfinite(s[k]).all(), k
        assert_bits(s[k], t[k], k)
    u = _step(api, m, "on")                                    # and on is on
    assert (raw(u["w"]) != raw(s["w"])).any() and np.isfinite(u["w"]).all()


def test_driver_reuse_gives_the_same_jacobian(api):
    """SolveFlowSystem assembles J with the D its F assembly left behind; a caller's own AssembleSystem at the same alpha states
    recomputes D: the same bits.  From rest rates the alpha states are the state itself (p slot 0)."""
    m = _mesh("cube6")
    N = m.num_node
    wg, _ = _alpha_fields(m)
    wg[3 * N:4 * N] = 0.0
    P = api.Problem(m, maxit=20)
    try:
        P.set_phase_change(**BASE)
        st = [api.DeviceArray.from_numpy(a) for a in (wg, np.zeros(6 * N), np.zeros(6 * N))]
        F_d, dx_d = api.DeviceArray(6 * N), api.DeviceArray(6 * N)
        assert P.solve_flow_system(st[0], st[1], st[2], F_d, dx_d, maxit=1)[0] == 1
        api.sync()
        driven = P.block_values().numpy()
        P.assemble_system(api.DeviceArray.from_numpy(wg), api.DeviceArray.from_numpy(np.zeros(6 * N)), None, want_J=True)
        api.sync()
        assert_bits(P.block_values().numpy(), driven, "J")
        P.set_phase_change()
        P.assemble_system(api.DeviceArray.from_numpy(wg), api.DeviceArray.from_numpy(np.zeros(6 * N)), None, want_J=True)
        api.sync()
        assert (raw(P.block_values().numpy()) != raw(driven)).any()
    finally:
        P.close()


def _spin_up(api, cfg):
    """one DflTimeStep of kuhn_cube(8) from rest under a rotational load, no-slip walls, the lower half solid; returns
    max speed one layer inside the solid / max speed in the liquid"""
    m = kuhn_cube(8)
    N = m.num_node
    x = m.xg.reshape(-1, 3)
    V = pm.nodal_volume(m.xg, m.ien).astype(np.float64)
    load = 1.0e3 * np.c_[-(x[:, 1] - 0.5), x[:, 0] - 0.5, np.zeros(N)] * V[:, None]
    w0 = pm.state(N, 0.0, np.where(x[:, 2] <= 0.5 + 1e-9, 1500.0, 1800.0))
    P = api.Problem(m, maxit=200, atol=1e-14, rtol=1e-8, bcs=[(g, (1, 1, 1)) for g in range(6)])
    try:
        if cfg:
            P.set_phase_change(**cfg)
        P.set_external_load(api.DeviceArray.from_numpy(load.reshape(-1)))
        st = [api.DeviceArray.from_numpy(a) for a in (w0, np.zeros(6 * N), np.zeros(6 * N))]
        F_d, dx_d = api.DeviceArray(6 * N), api.DeviceArray(6 * N)
        it, rn, r0 = P.time_step(st[0], st[1], st[2], F_d, dx_d, newton_maxit=4)
        api.sync()
        P.set_external_load(None)
        speed = np.sqrt((st[0].numpy()[:3 * N].reshape(-1, 3) ** 2).sum(axis=1))
    finally:
        P.close()
    assert np.isfinite(speed).all() and it > 0
    solid, liquid = x[:, 2] <= 0.375 + 1e-9, x[:, 2] >= 0.625 - 1e-9
    assert solid.sum() > 100 and liquid.sum() > 100 and speed[liquid].max() > 0.0
    return float(speed[solid].max() / speed[liquid].max())


def test_solid_holds_still(api):
    """C(0) = 1e9 against rho / dt = 2e4: the model scale of the ratio is 2e-5; the condition is 1e-2, about 500x above it.
    Without the feature the solid half spins like the liquid one."""
    on = _spin_up(api, dict(T_solidus=1600.0, T_liquidus=1700.0, darcy_c=1.0e6, darcy_b=1e-3))
    off = _spin_up(api, None)
    print(f"solid / liquid speed: {on:.3e} with the drag, {off:.3e} without")
    record("solid_holds_still", "drag on", on / 1e-2, measured=on)
    record("solid_holds_still", "drag off", 0.1 / off, measured=off)
    assert on < 1e-2
    assert off > 0.1


def _heating_rate(api, latent, T0, q0):
    m = kuhn_cube(4)
    N = m.num_node
    V = pm.nodal_volume(m.xg, m.ien).astype(np.float64)
    P = api.Problem(m, maxit=200, atol=1e-30, rtol=1e-6, bcs=[])
    try:
        P.set_scalar_transport(phi=False, T=True, rtol=1e-13)
        P.set_phase_change(T_solidus=1600.0, T_liquidus=1700.0, latent=latent)
        P.set_heat_source(api.DeviceArray.from_numpy(q0 * V))
        st = [api.DeviceArray.from_numpy(a) for a in (pm.state(N, 0.0, T0), np.zeros(6 * N), np.zeros(6 * N))]
        F_d, dx_d = api.DeviceArray(6 * N), api.DeviceArray(6 * N)
        it, rn, r0 = P.time_step(st[0], st[1], st[2], F_d, dx_d, newton_maxit=4)
        api.sync()
        P.set_heat_source(None)
        return st[2].numpy()[5 * N:], rn[3] / r0[3], it
    finally:
        P.close()


def test_latent_heat_slows_heating(api):
    """u = 0, uniform T0 inside the range, q_a = q0 V_a: the field stays uniform and the converged rate x = dT solves
    kALPHAM (rho cp + latent fl'(T0 + fact2 x)) x = q0 (generalized alpha from rest: dT_alpha_m = kALPHAM x,
    T_alpha = T0 + fact2 x).  T0 lies in the lower half of the range and heats, so fl'' > 0 and g(x) = lhs has x g'(x) >= g(x):
    a relative residual rho of the T rows bounds the relative error of x by rho.  That is the tolerance, plus fp64 rounding
    of the uniform field (64 ulp).  Observed on one MI355X: error 4.88e-4 under a reported residual of 4.98e-4 after two
    Newton iterations (x g'(x) / g(x) = 1.013 here), the rate 197 times below the one without latent heat."""
    import scalar_model as sm
    latent, T0, q0 = 2.0e7, 1620.0, 4.0e6
    cfg = pm.config(T_solidus=1600.0, T_liquidus=1700.0, latent=latent)
    rc = LD(sm.kRHO) * LD(sm.kCP)

    def g(x):
        return LD(sm.kALPHAM) * (rc + LD(latent) * pm.liquid_fraction(cfg, LD(T0) + LD(pm.FACT2) * x)[1]) * x

    lo = LD(0)
    hi = top = LD(q0) / (LD(sm.kALPHAM) * rc)                  # the rate without latent heat; g is increasing here: bisection
    for _ in range(200):
        mid = (lo + hi) / 2
        lo, hi = (mid, hi) if g(mid) < q0 else (lo, mid)
    x = (lo + hi) / 2
    dT, rho, it = _heating_rate(api, latent, T0, q0)
    dT0, rho0, _ = _heating_rate(api, 0.0, T0, q0)
    err = float(np.abs(dT.astype(LD) - x).max() / x)
    err0 = float(np.abs(dT0.astype(LD) - top).max() / top)
    print(f"latent heating: rate {float(x):.6e} K/s, relative error {err:.3e}, reported residual {rho:.3e} after {it} iterations; "
          f"without latent heat {float(dT0.mean()):.6e} K/s, error {err0:.3e}, residual {rho0:.3e}")
    record("latent_heating", "rate", err / max(rho, 1e-300), error=err, residual=float(rho), iterations=it)
    ulp = 64 * np.finfo(np.float64).eps
    assert err <= rho + ulp
    assert dT.max() < dT0.min() and dT.min() > 0.0
    assert T0 + pm.FACT2 * float(x) < 1650.0                    # the alpha-level T stays in the lower half: fl'' > 0


def test_refusals(api, capfd):
    m = _mesh("cube2")
    N = m.num_node
    P = api.Problem(m)
    try:
        for reason, change in [("T_liquidus", dict(T_liquidus=1600.0)), ("darcy_b", dict(darcy_b=0.0)), ("latent", dict(latent=np.nan)),
                               ("side", dict(use_phi=True, side=0)), ("eps", dict(use_phi=True, eps=0.0))]:
            P.set_phase_change(**dict(BASE, **change))
            assert not P.phase_change_on and reason in capfd.readouterr().err
        out = api.DeviceArray.from_numpy(sent(N))
        api.lib().DflMeshPhaseCoefficients(P.mesh, api.DeviceArray(6 * N).ptr, out.ptr, None, None)
        api.sync()
        assert "no phase change" in capfd.readouterr().err
        assert_bits(out.numpy(), sent(N), "nothing written")
        P.set_phase_change(**BASE)
        assert P.phase_change_on and capfd.readouterr().err == ""
        w = api.DeviceArray.from_numpy(pm.state(N, 0.0, 1650.0))
        before = P.phase_coefficients(w)["D"].numpy()
        P.set_phase_change(**dict(BASE, darcy_b=-1.0))              # refused: the earlier configuration stays
        assert P.phase_change_on and "darcy_b" in capfd.readouterr().err
        assert_bits(P.phase_coefficients(w)["D"].numpy(), before, "D after a refused configuration")
        # a solver with a communicator: refused before anything is computed
        comm = api.DflComm()
        api.lib().KrylovSetComm(P.ksp, C.byref(comm))
        st = [api.DeviceArray.from_numpy(np.zeros(6 * N)) for _ in range(3)]
        F_d, dx_d = api.DeviceArray(6 * N), api.DeviceArray(6 * N)
        assert P.time_step(st[0], st[1], st[2], F_d, dx_d)[0] == -1
        assert "phase change is single-GPU only" in capfd.readouterr().err
        assert P.solve_flow_system(st[0], st[1], st[2], F_d, dx_d)[0] == -1
        assert "phase change is single-GPU only" in capfd.readouterr().err
        api.lib().KrylovSetComm(P.ksp, None)
        P.set_phase_change()
        assert not P.phase_change_on
    finally:
        P.close()
