"""GPU tests of the fluid material (include/dedflow.h "fluid material"; host/fluid.c, csrc/k_fluid.hip): the (u,p)-row
correction r and the nodal totals Rn, Mn against tests/fluid_model.py (np.longdouble), the Jacobian correction S as the
difference of two assemblies against the model, the neutral configuration and the off path bit for bit, the similarity
rho, mu, p -> s rho, s mu, s p against the untouched base kernels, hydrostatic rest, guard bands, reproducibility, the hook
order, and DflTimeStep: similarity, buoyancy, the refusal with a communicator.

Parity bound.  |dev - model| <= 1e-12 max(abs-sum) per output, the bound test_gpu_thermal.py uses for the same kind of
fixed-order sum of a few dozen O(100)-operation fp64 terms against longdouble, scaled by the sums of the absolute values of
the terms (fluid_model.py) because the rows cancel.  The momentum rows and the continuity rows of r are two outputs: their
scales differ by the density.  With DFL_PARITY_OUT set, the observed ratio of every case goes to that file
(profiles/fluid_material_parity.jsonl is such a run)."""
import ctypes as C

import numpy as np
import pytest

import fluid_model as fm
import phase_model as pm
from dedflow_amd.meshgen import fan_mesh, kuhn_cube, single_tet, synthetic_fields
from guarded_buffers import Pool, Recorder, assert_bits, raw, sent

pytestmark = pytest.mark.gpu
LD = np.longdouble
BOUND = 1e-12
record = Recorder("a")
TILT = np.array([0.2, -0.3, 1.0]) / np.sqrt(1.13)
BASE = dict(rho_gas=1.2, rho_metal=7000.0, mu_gas=2.0e-5, mu_metal=5.0e-3, gravity=(0.3, -0.2, -9.81), beta=1.0e-4, T_ref=1650.0)
MESHES = {"single": single_tet, "cube2": lambda: kuhn_cube(2), "cube6": lambda: kuhn_cube(6, jitter=0.2), "fan": fan_mesh}
EPS = {"single": 0.5, "cube2": 0.4, "cube6": 0.3, "fan": 0.5}
FIELDS = ["gas", "metal", "interface", "random", "flow"]
CASES = [(mn, f) for mn in MESHES for f in FIELDS]
OUT = ("r", "Rn", "Mn")
CLOSED_BOX = [(g, (1, 1, 1)) for g in range(6)]


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
        _mesh_cache[name] = MESHES[name]() if name in MESHES else kuhn_cube(int(name[5:]))
    return _mesh_cache[name]


def _problem(api, mesh_name, **kw):
    m = _mesh(mesh_name)
    if mesh_name == "single":                                # (the tet has four groups)
        kw.setdefault("bcs", [])
    return api.Problem(m, **kw)


def case(mesh_name, field):
    """(mesh, w [6N], dw [6N], configuration)"""
    m = _mesh(mesh_name)
    x = m.xg.reshape(-1, 3)
    N = m.num_node
    c = 0.5 * (x.min(axis=0) + x.max(axis=0))
    L = float((x.max(axis=0) - x.min(axis=0)).max())
    s = (x - c) @ TILT / L                                  # about -0.6 .. 0.6
    phi = (x - c) @ np.array([0.3, 0.1, -1.0]) / np.sqrt(1.1)
    rng = np.random.default_rng(31)
    cfg = dict(BASE)
    T = 1650.0 + 250.0 * s
    u, du = np.zeros((N, 3)), np.zeros((N, 3))
    p = 7000.0 * ((x - c) @ np.array(BASE["gravity"]))      # about the metal's hydrostatic pressure
    if field == "gas":
        cfg.update(use_phi=True, side=1, level=10.0 * L, eps=EPS[mesh_name])
    elif field in ("interface", "flow", "random"):
        cfg.update(use_phi=True, side=1, level=0.05 * L, eps=EPS[mesh_name])
    if field in ("flow", "random"):
        u, du = rng.standard_normal((N, 3)), 20.0 * rng.standard_normal((N, 3))
        p = p + 1.0e3 * rng.standard_normal(N)
    if field == "random":
        T = rng.uniform(1550.0, 1750.0, N)
        T[1:: max(3, N // 4)] = np.nan                      # (a NaN T_q: the factor 1, no NaN in r)
        if N > 8:
            p[N - 2] = np.nan                               # (a NaN pressure reaches the rows of the node's neighbours)
    return m, fm.state(N, phi, T, u=u), fm.rates(N, du=du, p=p), fm.config(**cfg)


_model_cache = {}


def model(mesh_name, field):
    if (mesh_name, field) not in _model_cache:
        m, w, dw, cfg = case(mesh_name, field)
        _model_cache[mesh_name, field] = fm.rows(m.xg, m.ien, w, dw, cfg)
    return _model_cache[mesh_name, field]


def _device_rows(api, pool, P, w, dw, outputs=OUT):
    """DflMeshFluidRows into guarded NaN-filled outputs; returns them, after the bands and the inputs were checked"""
    ws, ds = pool.slot(w), pool.slot(dw, off=1)
    slots = {k: pool.slot(sent(4 * P.N if k == "r" else P.N), off=1) for k in outputs}
    api.lib().DflMeshFluidRows(P.mesh, ws.ptr, ds.ptr, *[slots[k].ptr if k in slots else None for k in OUT])
    api.sync()
    ws.check("w")
    ds.check("dw")
    return {k: s.check(k, written=True).copy() for k, s in slots.items()}


def _ratio(name, got, ref, ref_abs):
    """max |got - ref| / max(abs-sum) over the entries the model has a number for; the others must be NaN on the device too"""
    got = np.asarray(got).reshape(-1)
    ref, ref_abs = np.asarray(ref, LD).reshape(-1), np.asarray(ref_abs, LD).reshape(-1)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), name
    if nan.all():
        return 0.0
    scale = ref_abs[~nan].max()
    if scale == 0:
        assert_bits(got[~nan], np.zeros(int((~nan).sum())), name)
        return 0.0
    ratio = float(np.abs(got[~nan].astype(LD) - ref[~nan]).max() / scale)
    print(f"fluid parity {name}: {ratio:.3e} of the abs-sum ({ratio / BOUND:.3e} of the bound)")
    return ratio


def _split(r, N):
    return {"r_u": r[:3 * N], "r_p": r[3 * N:]}


@pytest.mark.parametrize("mesh_name,field", CASES)
def test_rows_parity_and_memory_safety(api, pool, mesh_name, field):
    m, w, dw, cfg = case(mesh_name, field)
    ref = model(mesh_name, field)
    N = m.num_node
    if field == "random" and N > 8:
        assert np.isnan(ref["r"]).any() and not np.isnan(ref["r"]).all()
    P = _problem(api, mesh_name)
    try:
        xg0 = api.d2h(P.mesh.contents.device.contents.xg, 3 * P.N, np.float64)
        ien0 = api.d2h(P.mesh.contents.device.contents.ien, 4 * P.T, np.int32)
        P.set_fluid_material(**cfg)
        assert P.fluid_material_on
        out = _device_rows(api, pool, P, w, dw)
        parts = dict(_split(out["r"], N), Rn=out["Rn"], Mn=out["Mn"])
        refs = dict(_split(ref["r"], N), Rn=ref["Rn"], Mn=ref["Mn"])
        abss = dict(_split(ref["r_abs"], N), Rn=ref["Rn_abs"], Mn=ref["Mn_abs"])
        for k in parts:
            ratio = _ratio(f"{mesh_name}/{field}/{k}", parts[k], refs[k], abss[k])
            record("fluid_rows_kernel", f"{mesh_name}/{field}/{k}", ratio / BOUND, nodes=int(P.N), tets=int(P.T))
            assert ratio <= BOUND, (k, ratio)
        assert out["Rn"].min() > 0.0 and out["Mn"].min() > 0.0
        # a NULL output in each position (r alone is the kernel of the assembly path): the same bits, a second and third time
        for keep in (("r",), ("Rn", "Mn"), ("r", "Mn"), ("Rn",)):
            part = _device_rows(api, pool, P, w, dw, outputs=keep)
            for k, a in part.items():
                assert_bits(a, out[k], f"{k} of {keep}")
        api.sync()
        assert_bits(api.d2h(P.mesh.contents.device.contents.xg, 3 * P.N, np.float64), xg0, "xg")
        assert np.array_equal(api.d2h(P.mesh.contents.device.contents.ien, 4 * P.T, np.int32), ien0)
    finally:
        P.close()


def _block_values(api, P, w, dw, F=None):
    """the block values [nnz, 16] of one J assembly (and F, when given a DeviceArray)"""
    P.assemble_system(api.DeviceArray.from_numpy(w), api.DeviceArray.from_numpy(dw), F, want_J=True)
    api.sync()
    return P.block_values().numpy().reshape(-1, 16).copy()


def _unit_rows(val, rp, ci):
    """mask [nnz, 16] of the entries that lie in a Dirichlet unit row of the block values val: row i of node a's blocks is
    a unit row when it is 1 on the diagonal entry and 0 everywhere else"""
    N = rp.size - 1
    rows_of = np.repeat(np.arange(N), np.diff(rp))
    v = val.reshape(-1, 4, 4)
    want = np.zeros_like(v)
    want[rows_of == ci] = np.eye(4)
    bad = np.zeros((N, 4), np.int64)
    np.add.at(bad, rows_of, (v != want).any(axis=2).astype(np.int64))
    unit = bad == 0                                          # [N, i]
    return np.repeat(unit[rows_of][:, :, None], 4, axis=2).reshape(-1, 16)


@pytest.mark.parametrize("mesh_name,field", [(mn, f) for mn in MESHES for f in ("gas", "interface", "random", "flow")])
def test_jacobian_parity(api, mesh_name, field):
    """block values assembled with the feature minus block values assembled without (same w, dw, in longdouble) against the
    model's S, every entry of every block; the scale is the abs-sum of the total (both B's), which the half-ulp of the base
    the difference carries is far inside.  The Dirichlet rows are unit rows either way"""
    m, w, dw, cfg = case(mesh_name, field)
    N = m.num_node
    dw = np.where(np.isnan(dw), 0.0, dw)                     # (J does not read the pressure; the base F is not asked for)
    jm, jm_abs = fm.element_jm(m.xg, m.ien, w, cfg)
    P = _problem(api, mesh_name)
    try:
        rp, ci = P.pattern()
        v0 = _block_values(api, P, w, dw)
        P.set_fluid_material(**cfg)
        v1 = _block_values(api, P, w, dw)
    finally:
        P.close()
    S, S_abs = fm.on_pattern(m.ien, N, rp, ci, jm), fm.on_pattern(m.ien, N, rp, ci, jm_abs)
    unit = _unit_rows(v0, rp, ci)
    assert mesh_name == "single" or unit.any()
    assert_bits(v1[unit], v0[unit], "unit rows")
    assert np.isfinite(v1).all() and (raw(v1[~unit]) != raw(v0[~unit])).any()
    diff = v1.astype(LD) - v0.astype(LD)
    for name, sel in (("uu", [0, 1, 2, 4, 5, 6, 8, 9, 10]), ("up", [3, 7, 11]), ("pu", [12, 13, 14]), ("pp", [15])):
        keep = ~unit[:, sel]
        scale = float(S_abs[:, sel].max())
        ratio = float(np.abs((diff[:, sel] - S[:, sel])[keep]).max() / scale)
        print(f"fluid parity {mesh_name}/{field}/J {name}: {ratio:.3e} of the abs-sum")
        record("fluid_jac_row_kernel", f"{mesh_name}/{field}/J_{name}", ratio / BOUND, nodes=int(N), tets=int(m.num_tet))
        assert ratio <= BOUND, (name, ratio)


# ---- the assemblies ---------------------------------------------------------------------------------------------------------
def _alpha_fields(m):
    """alpha-level states with a velocity field, rates on every slot, phi through the mesh and T about T_ref"""
    N = m.num_node
    wg, dwg = synthetic_fields(m)
    x = m.xg.reshape(-1, 3)
    c = 0.5 * (x.min(axis=0) + x.max(axis=0))
    wg[4 * N:5 * N] = (x - c) @ np.array([0.3, 0.1, -1.0]) / np.sqrt(1.1)
    wg[5 * N:] = 1650.0 + 120.0 * ((x - c) @ TILT)
    return wg, dwg


INTERFACE = dict(BASE, use_phi=True, side=1, level=0.03, eps=0.3)
NEUTRAL = dict(fm.NEUTRAL, beta=1.0e-4, T_ref=1650.0, use_phi=True, side=1, level=0.03, eps=0.3)


def _assemblies(api, m, cfg, schedule=4, extras=False, clear=False, bcs=None, fields=None):
    """F and the block values of one (F, J) assembly at _alpha_fields, with the device's own r; cfg None: no fluid material;
    extras: an external load, the phase-change drag and a thermal material set as well; clear: set and cleared again first"""
    N = m.num_node
    wg, dwg = fields if fields is not None else _alpha_fields(m)
    P = api.Problem(m, schedule=schedule) if bcs is None else api.Problem(m, schedule=schedule, bcs=bcs)
    try:
        load = None
        if extras:
            P.set_scalar_transport(phi=True, T=True)
            P.set_phase_change(T_solidus=1600.0, T_liquidus=1700.0, latent=2.0e9, darcy_c=1.0e6)
            P.set_thermal_material(k_gas=0.02, k_solid=30.0, c_gas=1.2e3, c_metal=4.0e6, use_phi=True, side=1, level=0.03, eps=0.3)
            load = api.DeviceArray.from_numpy(1.0e3 * np.repeat(pm.nodal_volume(m.xg, m.ien).astype(np.float64), 3))
            P.set_external_load(load)
        if cfg is not None:
            P.set_fluid_material(**cfg)
        if clear:
            P.set_fluid_material()
            assert not P.fluid_material_on
        wd, dd, F = api.DeviceArray.from_numpy(wg), api.DeviceArray.from_numpy(dwg), api.DeviceArray(6 * N)
        o = dict(wg=wg, dwg=dwg)
        if P.fluid_material_on:
            o["r"] = P.fluid_rows(wd, dd, want=("r",))["r"].numpy()
        P.assemble_system(wd, dd, F, want_J=True)
        api.sync()
        o["F"], o["J"] = F.numpy(), P.block_values().numpy().reshape(-1, 16).copy()
        o["pattern"] = P.pattern()
        if extras:
            P.set_external_load(None)
        return o
    finally:
        P.close()


def test_neutral_configuration_and_off_are_the_one_fluid_bits(api, pool):
    """rho_* = kRHO, mu_* = kMU, g = 0: r is exactly +0.0 and F and J are those of a mesh never configured, bit for bit; the
    same after the material was set and cleared.  Rn / V = 1000 and Mn / V = kMU to 1e-11"""
    m = _mesh("cube6")
    N = m.num_node
    for schedule in (4, 1):
        off = _assemblies(api, m, None, schedule)
        for name, o in (("neutral", _assemblies(api, m, NEUTRAL, schedule)), ("cleared", _assemblies(api, m, INTERFACE, schedule, clear=True))):
            if name == "neutral":
                assert_bits(o["r"], np.zeros(4 * N), "r of the neutral configuration")
            for k in ("F", "J"):
                assert np.isfinite(off[k]).all()
                assert_bits(o[k], off[k], f"{name}: {k}")
        on = _assemblies(api, m, INTERFACE, schedule)             # and on is on
        assert (raw(on["F"]) != raw(off["F"])).any() and (raw(on["J"]) != raw(off["J"])).any()
    P = api.Problem(m)
    try:
        P.set_fluid_material(**NEUTRAL)
        out = _device_rows(api, pool, P, off["wg"], off["dwg"])
        assert_bits(out["r"], np.zeros(4 * N), "r beside Rn and Mn")
        V = pm.nodal_volume(m.xg, m.ien)
        assert np.abs(out["Rn"] / V - LD(1000.0)).max() <= 1e-11 and np.abs(out["Mn"] / V - LD(fm.kMU)).max() <= 1e-11
    finally:
        P.close()


def test_nothing_written_without_a_configuration(api, pool, capfd):
    m = _mesh("cube2")
    N = m.num_node
    P = api.Problem(m)
    try:
        slots = [pool.slot(sent(4 * N if k == 0 else N), off=1) for k in range(3)]
        w = pool.slot(np.zeros(6 * N))
        api.lib().DflMeshFluidRows(P.mesh, w.ptr, w.ptr, *[s.ptr for s in slots])
        api.sync()
        assert "no fluid material" in capfd.readouterr().err
        for s in slots:
            s.check("nothing written")
        with pytest.raises(RuntimeError):
            P.fluid_rows(w.dev, w.dev)
    finally:
        P.close()


@pytest.mark.parametrize("s", [2.0, 0.5])
def test_similarity_against_the_base_kernels(api, s):
    """the fan (its weak-BC group 4 is empty), no Dirichlet rows: F and J assembled with rho = s kRHO, mu = s kMU, g = 0 and
    the pressure s p against the base kernels' F and J at the same state, entry by entry: momentum rows s x base, continuity
    rows equal, J[i][j] = s J0, J[i][3] and J[3][i] equal, J[3][3] = J0 / s.  The scale is the abs-sum of what was added:
    the base's and both sides of the correction"""
    m = _mesh("fan")
    N = m.num_node
    wg, dwg = synthetic_fields(m)
    ds = dwg.copy()
    ds[3 * N:4 * N] *= s
    cfg = fm.config(rho_metal=s * fm.kRHO, mu_metal=s * fm.kMU)
    base = _assemblies(api, m, None, bcs=[], fields=(wg, dwg))
    on = _assemblies(api, m, cfg, bcs=[], fields=(wg, ds))
    rp, ci = base["pattern"]
    g = fm.tet_coefficients(m.xg, m.ien, wg, cfg)
    u, du, p = fm.fields(N, g["ien"], wg, ds)
    rho0, mu0, f0 = fm.base_coefficients(len(g["ien"]))
    E_abs = fm._node_sum(N, g["ien"], fm.element_E(g, u, du, p, g["rho"], g["mu"], g["f"], True)
                         + 2 * fm.element_E(g, u, du, p, rho0, mu0, f0, True))
    B_abs = fm.on_pattern(m.ien, N, rp, ci, fm.element_B(g, u, g["rho"], g["mu"], True) + 2 * fm.element_B(g, u, rho0, mu0, True))
    F0, F1 = base["F"].astype(LD), on["F"].astype(LD)
    J0, J1 = base["J"].astype(LD), on["J"].astype(LD)
    uu, up, pu = [0, 1, 2, 4, 5, 6, 8, 9, 10], [3, 7, 11], [12, 13, 14]
    checks = [("F momentum", F1[:3 * N], s * F0[:3 * N], E_abs[:, :3].max()), ("F continuity", F1[3 * N:4 * N], F0[3 * N:4 * N], E_abs[:, 3].max()),
              ("J uu", J1[:, uu], s * J0[:, uu], B_abs[:, uu].max()), ("J up", J1[:, up], J0[:, up], B_abs[:, up].max()),
              ("J pu", J1[:, pu], J0[:, pu], B_abs[:, pu].max()), ("J pp", J1[:, 15], J0[:, 15] / s, B_abs[:, 15].max())]
    for name, got, want, scale in checks:
        ratio = float(np.abs(got - want).max() / scale)
        print(f"fluid similarity s = {s}, {name}: {ratio:.3e} of the abs-sum")
        record("fluid_similarity", f"s={s}/{name}", ratio / BOUND)
        assert np.abs(want).max() > 0 and ratio <= BOUND, (name, ratio)
    assert_bits(on["F"][4 * N:], base["F"][4 * N:], "phi / T rows")


def _hydrostatic(m, rho, gravity):
    N = m.num_node
    x = m.xg.reshape(-1, 3)
    return fm.state(N, np.zeros(N), np.zeros(N)), fm.rates(N, p=rho * ((x - x[0]) @ np.asarray(gravity)))


def test_hydrostatic_rest(api):
    """kuhn_cube(6), no Dirichlet rows, metal everywhere, rho = 7000, g = (0, 0, -9.81), u = 0, p = rho g . (x - x0): the
    assembled momentum rows of the interior nodes and all continuity rows are <= 1e-12 of the rows' abs-sum scale (base and
    both sides of the correction); with the feature off the same state does not pass: the weight is missing"""
    m = _mesh("kuhn:6")
    N = m.num_node
    gravity = (0.0, 0.0, -9.81)
    cfg = fm.config(rho_metal=7000.0, mu_metal=5.0e-3, gravity=gravity)
    w, dw = _hydrostatic(m, 7000.0, gravity)
    on, off = _assemblies(api, m, cfg, bcs=[], fields=(w, dw)), _assemblies(api, m, None, bcs=[], fields=(w, dw))
    g = fm.tet_coefficients(m.xg, m.ien, w, cfg)
    u, du, p = fm.fields(N, g["ien"], w, dw)
    rho0, mu0, f0 = fm.base_coefficients(len(g["ien"]))
    E_abs = fm._node_sum(N, g["ien"], fm.element_E(g, u, du, p, g["rho"], g["mu"], g["f"], True)
                         + 2 * fm.element_E(g, u, du, p, rho0, mu0, f0, True))
    x = m.xg.reshape(-1, 3)
    interior = ((x > 1e-9) & (x < 1 - 1e-9)).all(axis=1)
    assert interior.sum() == 125
    scale_u, scale_p = float(E_abs[:, :3].max()), float(E_abs[:, 3].max())
    res = {}
    for name, o in (("on", on), ("off", off)):
        Fu, Fp = o["F"][:3 * N].reshape(-1, 3), o["F"][3 * N:4 * N]
        res[name] = (float(np.abs(Fu[interior]).max() / scale_u), float(np.abs(Fp).max() / scale_p))
        print(f"hydrostatic rest, feature {name}: momentum {res[name][0]:.3e}, continuity {res[name][1]:.3e} of the abs-sum")
        record("fluid_hydrostatic", name, max(res[name]) / BOUND, momentum=res[name][0], continuity=res[name][1])
    assert res["on"][0] <= BOUND and res["on"][1] <= BOUND
    assert res["off"][0] > 1e-3 or res["off"][1] > 1e-3


@pytest.mark.parametrize("mesh_name", ["cube6", "fan"])
def test_reproducible_and_the_same_under_every_assembly_schedule(api, mesh_name):
    """two runs of schedule 4 and one of schedule 1: r, Rn, Mn the same bits throughout; F and J the same bits between the two
    runs, and between the schedules wherever the feature-off assemblies of the two schedules agree bit for bit (the correction
    is one rounded sum added once: it cannot add a difference of its own)"""
    m, w, dw, cfg = case(mesh_name, "flow")
    res = []
    for schedule in (4, 4, 1):
        P = _problem(api, mesh_name, schedule=schedule)
        try:
            wd, dd, F = api.DeviceArray.from_numpy(w), api.DeviceArray.from_numpy(dw), api.DeviceArray(6 * P.N)
            o = {"J0": _block_values(api, P, w, dw, F), "F0": F.numpy()}
            P.set_fluid_material(**cfg)
            o.update({k: a.numpy() for k, a in P.fluid_rows(wd, dd).items()})
            o["J"] = _block_values(api, P, w, dw, F)
            o["F"] = F.numpy()
            for k, a in P.fluid_rows(wd, dd).items():
                assert_bits(a.numpy(), o[k], f"{k} again")
            assert_bits(_block_values(api, P, w, dw, F), o["J"], "J again")
            assert_bits(F.numpy(), o["F"], "F again")
            res.append(o)
        finally:
            P.close()
    for o in res[1:]:
        for k in OUT:
            assert_bits(o[k], res[0][k], k)
            assert np.abs(o[k]).max() > 0.0
    for k in ("F", "J"):
        assert_bits(res[1][k], res[0][k], f"{k}, schedule 4 twice")
        same = raw(res[2][k + "0"]) == raw(res[0][k + "0"])
        print(f"{mesh_name}: schedules 1 and 4 agree on {same.mean():.3f} of the feature-off {k}")
        assert same.any()
        assert_bits(res[2][k][same], res[0][k][same], f"{k} where the feature-off schedules 1 and 4 agree")


class _FluidParams(C.Structure):
    _fields_ = [("rho_gas", C.c_double), ("rho_metal", C.c_double), ("mu_gas", C.c_double), ("mu_metal", C.c_double),
                ("gravity", C.c_double * 3), ("beta", C.c_double), ("T_ref", C.c_double), ("level", C.c_double),
                ("side", C.c_double), ("eps", C.c_double), ("use_phi", C.c_int)]


def _device_S(api, P, cfg, wg):
    """the kernel's own S [nnz, 16]: dfl_fluid_add_jacobian on zeroed block values (0 + S is S)"""
    L = api.lib()
    vrow, vcol = C.c_void_p(), C.c_void_p()
    L.DflMeshSortedV2E.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.DflMeshSortedV2E.restype = None
    L.DflMeshSortedV2E(P.mesh, C.byref(vrow), C.byref(vcol))
    prm = _FluidParams(cfg["rho_gas"], cfg["rho_metal"], cfg["mu_gas"], cfg["mu_metal"], (C.c_double * 3)(*cfg["gravity"]),
                       cfg["beta"], cfg["T_ref"], cfg["level"], float(cfg["side"]), cfg["eps"], 1 if cfg["use_phi"] else 0)
    val = api.DeviceArray.from_numpy(np.zeros(P.nnz1 * 16))
    wd = api.DeviceArray.from_numpy(wg)
    dev, spy = P.mesh.contents.device.contents, P.spy1x1.contents
    L.dfl_fluid_add_jacobian.argtypes = [C.c_int32] + [C.c_void_p] * 10
    L.dfl_fluid_add_jacobian.restype = None
    L.dfl_fluid_add_jacobian(P.N, vrow, vcol, C.cast(dev.ien, C.c_void_p), C.cast(dev.xg, C.c_void_p), wd.ptr,
                             C.cast(spy.row_ptr, C.c_void_p), C.cast(spy.col_ind, C.c_void_p), C.byref(prm), val.ptr, None)
    api.sync()
    return val.numpy().reshape(-1, 16)


def _dirichlet_dofs(m, bcs):
    held = np.zeros((m.num_node, 3), bool)
    for group, flags in bcs:
        nodes = m.bound_node[m.bound_node_offset[group]:m.bound_node_offset[group + 1]]
        for d in range(3):
            if flags[d]:
                held[nodes, d] = True
    return held


@pytest.mark.parametrize("schedule", [4, 1])
def test_hook_order(api, schedule):
    """an external load, the phase-change drag and a thermal material set: F is fl(F without the fluid material + r), r as
    DflMeshFluidRows gives it at the same states, with the Dirichlet rows zero; J is fl(J without + S) with the kernel's own S
    (the documented order: after the phase-change diagonal), with the Dirichlet rows unit rows"""
    m = _mesh("cube6")
    N = m.num_node
    cfg = fm.config(**INTERFACE)
    off, on = _assemblies(api, m, None, schedule, extras=True), _assemblies(api, m, INTERFACE, schedule, extras=True)
    held = _dirichlet_dofs(m, api.REFERENCE_BCS)
    assert held.any() and not held.all() and np.abs(on["r"]).max() > 0.0
    want = off["F"][:4 * N] + on["r"]
    want[:3 * N][held.reshape(-1)] = 0.0
    assert_bits(on["F"][:4 * N], want, "F[0 .. 4N)")
    assert_bits(on["F"][4 * N:], off["F"][4 * N:], "phi / T rows")
    assert (raw(on["F"]) != raw(off["F"])).any()
    P = api.Problem(m, schedule=schedule)
    try:
        S = _device_S(api, P, cfg, on["wg"])
    finally:
        P.close()
    rp, ci = on["pattern"]
    unit = _unit_rows(off["J"], rp, ci)
    rows_of = np.repeat(np.arange(N), np.diff(rp))
    assert np.array_equal(unit.reshape(-1, 4, 4)[:, :3, 0], held[rows_of])
    want_J = np.where(unit, off["J"], off["J"] + S)
    assert_bits(on["J"], want_J, "J")
    assert np.abs(S).max() > 0.0


# ---- through DflTimeStep ------------------------------------------------------------------------------------------------
def _step(api, m, cfg, load, rtol, w0=None, weak_bc=True, maxit=600, newton_maxit=4, check_every=0):
    """one DflTimeStep from rest in the closed no-slip box (GMRES with the library's default preconditioner, block Jacobi);
    returns u [N, 3], p [N], the Newton iterations"""
    N = m.num_node
    P = api.Problem(m, maxit=maxit, atol=1e-30, rtol=rtol, bcs=CLOSED_BOX)
    try:
        if not weak_bc:
            api.lib().DflMeshSetWeakBCGroup(P.mesh, 6)           # an empty group: no face terms
        api.lib().KrylovSetCheckInterval(P.ksp, check_every)     # (0: every 20 iterations, as the reference)
        if cfg is not None:
            P.set_fluid_material(**cfg)
        ld = None
        if load is not None:
            ld = api.DeviceArray.from_numpy(load)
            P.set_external_load(ld)
        w = np.zeros(6 * N) if w0 is None else w0
        st = [api.DeviceArray.from_numpy(a) for a in (w, np.zeros(6 * N), np.zeros(6 * N))]
        F_d, dx_d = api.DeviceArray(6 * N), api.DeviceArray(6 * N)
        it, rn, r0 = P.time_step(st[0], st[1], st[2], F_d, dx_d, newton_maxit=newton_maxit)
        api.sync()
        if load is not None:
            P.set_external_load(None)
        wn, dn = st[0].numpy(), st[2].numpy()
        assert it >= 0 and np.isfinite(wn[:4 * N]).all() and np.isfinite(dn[:4 * N]).all()
        return wn[:3 * N].reshape(-1, 3), dn[3 * N:4 * N], it
    finally:
        P.close()


def test_time_step_similarity(api):
    """s = 8 (rho = 8 kRHO, mu = 8 kMU) with the external load scaled by 8 reproduces the base run's u and 8 x its p (p up to
    its constant).  Measured against the base run's own sensitivity: the difference between two feature-off runs at rtol 1e-10
    and 1e-11; the margin over that is x 100, because the similar system is solved in a different residual norm.  For rtol to
    be what the state carries, every run makes one Newton iteration and GMRES tests convergence at every iteration
    (KrylovSetCheckInterval 1): with the default test every 20 iterations the two feature-off runs stop at the same iteration
    and are the same bits (measured: sensitivity exactly 0 beside 1.1e-12 in u and 5.2e-9 in p of the similar run; with four
    Newton iterations as well every run converges to rounding, 1.7e-17 and 1.6e-14).  The weak-BC group is empty in all three
    runs (its face terms keep kRHO and kMU)"""
    m = _mesh("kuhn:6")
    x = m.xg.reshape(-1, 3)
    V = pm.nodal_volume(m.xg, m.ien).astype(np.float64)
    body = np.stack([-(x[:, 1] - 0.5), x[:, 0] - 0.5, 0.3 * np.sin(np.pi * x[:, 0])], axis=1)
    load = (1.0e3 * V[:, None] * body).reshape(-1)
    ua, pa, _ = _step(api, m, None, load, 1e-10, weak_bc=False, newton_maxit=1, check_every=1)
    ub, pb, _ = _step(api, m, None, load, 1e-11, weak_bc=False, newton_maxit=1, check_every=1)
    us, ps, _ = _step(api, m, fm.config(rho_metal=8 * fm.kRHO, mu_metal=8 * fm.kMU), 8.0 * load, 1e-10, weak_bc=False, newton_maxit=1, check_every=1)
    c = lambda p: p - p.mean()
    sens_u, sens_p = float(np.abs(ua - ub).max()), float(np.abs(c(pa) - c(pb)).max())
    err_u, err_p = float(np.abs(us - ua).max()), float(np.abs(c(ps) / 8.0 - c(pa)).max())
    print(f"time-step similarity: |u_s - u| {err_u:.3e} (sensitivity {sens_u:.3e}), |p_s / 8 - p| {err_p:.3e} (sensitivity {sens_p:.3e}); "
          f"max |u| {np.abs(ua).max():.3e}, max |p| {np.abs(c(pa)).max():.3e}")
    over = max(err_u / (100 * sens_u), err_p / (100 * sens_p)) if sens_u > 0 and sens_p > 0 else float("inf")
    record("fluid_time_step", "similarity s=8", over, err_u=err_u, sens_u=sens_u,
           err_p=err_p, sens_p=sens_p, max_u=float(np.abs(ua).max()), max_p=float(np.abs(c(pa)).max()))
    assert np.abs(ua).max() > 0 and err_u <= 100 * sens_u and err_p <= 100 * sens_p


def test_rest_stays_at_rest_and_heat_rises(api):
    """uniform metal with g = (0, 0, -9.81) and a hot blob in the middle: with beta > 0 the vertical velocity at the blob's
    centre is positive after one step; with beta = 0 (the control) the fluid stays at rest: max |u| below 1e-3 of the heated
    run's"""
    m = _mesh("kuhn:6")
    N = m.num_node
    x = m.xg.reshape(-1, 3)
    T = 1700.0 + 200.0 * np.exp(-((x - 0.5) ** 2).sum(axis=1) / 0.03)
    w0 = fm.state(N, np.zeros(N), T)
    cfg = dict(rho_metal=2000.0, mu_metal=1.0, gravity=(0.0, 0.0, -9.81), T_ref=1700.0)
    uh, _, _ = _step(api, m, fm.config(beta=1.0e-3, **cfg), None, 1e-10, w0=w0)
    uc, _, _ = _step(api, m, fm.config(beta=0.0, **cfg), None, 1e-10, w0=w0)
    centre = int(np.argmin(((x - 0.5) ** 2).sum(axis=1)))
    hot, cold = float(np.abs(uh).max()), float(np.abs(uc).max())
    print(f"buoyancy: w at the blob's centre {uh[centre, 2]:.3e}, max |u| heated {hot:.3e}, control {cold:.3e}")
    record("fluid_time_step", "buoyancy", cold / (1e-3 * hot), w_centre=float(uh[centre, 2]), max_u_heated=hot, max_u_control=cold)
    assert np.allclose(x[centre], 0.5) and uh[centre, 2] > 0.0
    assert cold < 1e-3 * hot


def test_refusals(api, capfd):
    m = _mesh("cube2")
    N = m.num_node
    P = api.Problem(m)
    try:
        for reason, change in [("rho_gas", dict(rho_gas=0.0)), ("mu_metal", dict(mu_metal=np.nan)), ("gravity", dict(gravity=(0.0, np.inf, 0.0))),
                               ("side", dict(use_phi=True, side=0)), ("eps", dict(use_phi=True, eps=0.0))]:
            P.set_fluid_material(**dict(BASE, **change))
            assert not P.fluid_material_on and reason in capfd.readouterr().err
        P.set_fluid_material(**BASE)
        assert P.fluid_material_on and capfd.readouterr().err == ""
        wg, dwg = _alpha_fields(m)
        wd, dd = api.DeviceArray.from_numpy(wg), api.DeviceArray.from_numpy(dwg)
        before = P.fluid_rows(wd, dd)["r"].numpy()
        P.set_fluid_material(**dict(BASE, rho_metal=-1.0))             # refused: the earlier configuration stays
        assert P.fluid_material_on and "rho_metal" in capfd.readouterr().err
        assert_bits(P.fluid_rows(wd, dd)["r"].numpy(), before, "r after a refused configuration")
        # a solver with a communicator (world 1): refused before anything is computed
        comm = api.DflComm()
        api.lib().KrylovSetComm(P.ksp, C.byref(comm))
        st = [api.DeviceArray.from_numpy(np.zeros(6 * N)) for _ in range(3)]
        F_d, dx_d = api.DeviceArray(6 * N), api.DeviceArray(6 * N)
        assert P.time_step(st[0], st[1], st[2], F_d, dx_d)[0] == -1
        assert "fluid material is single-GPU only" in capfd.readouterr().err
        assert P.solve_flow_system(st[0], st[1], st[2], F_d, dx_d)[0] == -1
        assert "fluid material is single-GPU only" in capfd.readouterr().err
        api.lib().KrylovSetComm(P.ksp, None)
        P.set_fluid_material()
        assert not P.fluid_material_on
    finally:
        P.close()
