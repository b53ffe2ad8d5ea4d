"""GPU tests of the run-time time step (include/dedflow.h, "time step"): every kernel that takes dt against the private model
copies of tests/timestep_model.py away from the default step, the default step against a problem that never set one and against
the recorded bits of the build before the step became a run-time value (tests/golden/timestep_default_bits.json, written by
tools/make_timestep_golden.py), the driver's factors, a step that changes mid-run, two meshes with two steps, the refusals.

Bounds.  F and J of the (u,p,phi,T) system: per entry 8 c u K a (+ 2.2e-14 t under schedule 4), c from the float64
restatement of the model against its longdouble evaluation on the same mesh, as tests/test_gpu_assembly_kernels.py does; the
scalar Jacobians: 1e-12 of the largest entry (tests/test_gpu_scalar.py); the fluid rows and blocks, the thermal Jacobian:
1e-12 of the largest abs-sum (tests/test_gpu_fluid.py, tests/test_gpu_thermal.py); the phase-change diagonal: bit for bit
(tests/test_gpu_phase.py).  Nothing is fitted to the kernels."""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest

import timestep_model as ts
from dedflow_amd.meshgen import kuhn_cube, synthetic_fields
from krylov_model import EXTENDED_REASON, HAVE_EXTENDED

pytestmark = pytest.mark.gpu
needs_ld = pytest.mark.skipif(not HAVE_EXTENDED, reason=EXTENDED_REASON)
LD, F64 = np.longdouble, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTS = [1e-3, 2.0]          # at M = 4 one makes t0 = 4 / dt^2 dominate tau, the other makes it negligible
BOUND = 1e-12


def _tool():
    spec = importlib.util.spec_from_file_location("_make_timestep_golden", os.path.join(ROOT, "tools", "make_timestep_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _tool()
FLUID, THERMAL, PHASE = G.FLUID, G.THERMAL, G.PHASE


@pytest.fixture(scope="module")
def api():
    from dedflow_amd import api as A
    A.lib()
    return A


@pytest.fixture(scope="module")
def mesh():
    m = kuhn_cube(4, jitter=0.2)
    wg, dwg = G.fields(m)
    return m, wg, dwg


def raw(a):
    return np.ascontiguousarray(np.asarray(a, F64)).view(np.uint64)


def same(a, b, what):
    assert np.array_equal(raw(a), raw(b)), what


def _dev(api, *arrs):
    return [api.DeviceArray.from_numpy(np.ascontiguousarray(a, F64)) for a in arrs]


def _problem(api, m, dt, **kw):
    P = api.Problem(m, **kw)
    if dt is not None:
        P.set_time_step(dt)
        assert P.time_step_size() == dt
    return P


def _tet_and_face(api, P, wg, dwg):
    """F [6N] and the block values [nnz, 16] of AssembleSystemTet + AssembleSystemTetFace from zero"""
    wg_d, dwg_d = _dev(api, wg, dwg)
    F_d = api.DeviceArray(6 * P.N)
    F_d.zero()
    P.block_values().zero()
    P.assemble_tet(wg_d, dwg_d, F_d, want_J=True)
    P.assemble_face(wg_d, dwg_d, F_d, want_J=True)
    api.sync()
    return F_d.numpy(), P.block_values().numpy().reshape(-1, 16).copy()


def _system(api, P, wg, dwg):
    wg_d, dwg_d = _dev(api, wg, dwg)
    F_d = api.DeviceArray(6 * P.N)
    P.assemble_system(wg_d, dwg_d, F_d, want_J=True)
    api.sync()
    return F_d.numpy(), P.block_values().numpy().reshape(-1, 16).copy()


def quantities(api, m, wg, dwg, dt):
    """every dt-dependent quantity of test 1 at the step dt (None: never set), name -> array"""
    out = {}
    for sched in (0, 1, 4):
        P = _problem(api, m, dt, schedule=sched, bcs=[])
        out["F s%d" % sched], out["J s%d" % sched] = _tet_and_face(api, P, wg, dwg)
        if sched == 4:
            out["pattern"] = P.pattern()
            out["Jphi"], out["JT"] = P.assemble_scalar_jacobian(*_dev(api, wg, dwg))
        P.close()
    P = _problem(api, m, dt, bcs=[])
    out["F off"], out["J off"] = _system(api, P, wg, dwg)
    P.set_fluid_material(**FLUID)
    rows = P.fluid_rows(*_dev(api, wg, dwg), want=("r",))
    api.sync()
    out["fluid r"] = rows["r"].numpy()
    out["F fluid"], out["J fluid"] = _system(api, P, wg, dwg)
    P.set_fluid_material()
    P.set_thermal_material(**THERMAL)
    out["JT thermal"] = P.assemble_scalar_jacobian(*_dev(api, wg, dwg))[1]
    P.set_thermal_material()
    P.set_phase_change(**PHASE)
    out["F phase"], out["J phase"] = _system(api, P, wg, dwg)
    out["D"] = P.phase_coefficients(_dev(api, wg)[0], want=("D",))["D"].numpy()
    P.close()
    return out


_Q = {}


def q_at(api, mesh, dt):
    if dt not in _Q:
        _Q[dt] = quantities(api, *mesh, dt)
    return _Q[dt]


# ---- 1. kernel parity away from the default ----------------------------------------------------------------------------------
@needs_ld
@pytest.mark.parametrize("dt", DTS)
def test_assembly_parity(api, mesh, dt):
    """F and J of the volume and weak-BC face kernels under schedules 0, 1 and 4 against the private assembly_model"""
    m, wg, dwg = mesh
    A = ts.private("assembly_model", dt)
    N = m.num_node
    got = q_at(api, mesh, dt)
    rp, ci = got["pattern"]
    g = 4
    f2e = m.bound_f2e[m.bound_elem_offset[g]:m.bound_elem_offset[g + 1]]
    forn = m.bound_forn[m.bound_elem_offset[g]:m.bound_elem_offset[g + 1]]
    assert f2e.size > 0

    def model(dtype):
        Ft, Jt = A.assemble_tet(m.xg, m.ien, N, wg, dwg, rp, ci, dtype)
        Ff, Jf = A.assemble_face(m.xg, m.ien, N, f2e, forn, wg, dwg, rp, ci, dtype)
        return Ft + Ff, Jt + Jf
    F, J = model(LD)
    Fr, Jr = model(F64)
    cF, cJ = A.ratio_c(A.restatement_error(F, Fr), F.a), A.ratio_c(A.restatement_error(J, Jr), J.a)
    for sched in (0, 1, 4):
        for name, dev, mod, c in (("F", got["F s%d" % sched], F, cF), ("J", got["J s%d" % sched], J, cJ)):
            assert np.isfinite(dev).all()
            b = A.bound(mod, c, 1.0, sched == 4)
            err = np.abs(dev.astype(LD) - mod.v).astype(F64)
            zero = np.asarray(mod.a == 0)
            assert np.all(dev[zero] == 0.0)
            ratio = float((err[~zero] / b[~zero]).max())
            print("dt %g schedule %d %s: err / bound = %.3g (c = %.3g)" % (dt, sched, name, ratio, c))
            assert ratio <= 1.0, (dt, sched, name, ratio)
    # the step reaches the kernels: nothing equals the default's bits
    ref = q_at(api, mesh, None)
    for k in ("F s0", "J s0", "F s1", "J s1", "F s4", "J s4"):
        assert not np.array_equal(raw(got[k]), raw(ref[k])), k


@pytest.mark.parametrize("dt", DTS)
def test_scalar_jacobian_parity(api, mesh, dt):
    m, wg, dwg = mesh
    S = ts.private("scalar_model", dt)
    got = q_at(api, mesh, dt)
    rp, ci = got["pattern"]
    Jp, Jt = S.jacobians(m.xg, m.ien, wg)
    for name, dev, mod in (("Jphi", got["Jphi"], S.on_pattern(Jp, rp, ci)), ("JT", got["JT"], S.on_pattern(Jt, rp, ci))):
        ratio = float(np.abs(dev - mod).max() / np.abs(mod).max())
        print("dt %g %s: %.3e of the largest entry" % (dt, name, ratio))
        assert ratio < BOUND, (name, ratio)
        assert not np.array_equal(raw(dev), raw(q_at(api, mesh, None)[name]))


@needs_ld
@pytest.mark.parametrize("dt", DTS)
def test_fluid_parity(api, mesh, dt):
    m, wg, dwg = mesh
    Fm = ts.private("fluid_model", dt)
    N = m.num_node
    got = q_at(api, mesh, dt)
    rp, ci = got["pattern"]
    cfg = Fm.config(**FLUID)
    ref = Fm.rows(m.xg, m.ien, wg, dwg, cfg)
    for name, sl in (("r_u", slice(0, 3 * N)), ("r_p", slice(3 * N, 4 * N))):
        ratio = float(np.abs(got["fluid r"][sl].astype(LD) - ref["r"][sl]).max() / ref["r_abs"][sl].max())
        print("dt %g fluid %s: %.3e of the abs-sum" % (dt, name, ratio))
        assert ratio <= BOUND, (name, ratio)
    jm, jm_abs = Fm.element_jm(m.xg, m.ien, wg, cfg)
    S, S_abs = Fm.on_pattern(m.ien, N, rp, ci, jm), Fm.on_pattern(m.ien, N, rp, ci, jm_abs)
    diff = got["J fluid"].astype(LD) - got["J off"].astype(LD)
    for name, sel in (("uu", [0, 1, 2, 4, 5, 6, 8, 9, 10]), ("up", [3, 7, 11]), ("pu", [12, 13, 14]), ("pp", [15])):
        ratio = float(np.abs(diff[:, sel] - S[:, sel]).max() / float(S_abs[:, sel].max()))
        print("dt %g fluid J %s: %.3e of the abs-sum" % (dt, name, ratio))
        assert ratio <= BOUND, (name, ratio)
    d0 = q_at(api, mesh, None)
    assert not np.array_equal(raw(got["fluid r"]), raw(d0["fluid r"]))
    assert not np.array_equal(raw(got["J fluid"] - got["J off"]), raw(d0["J fluid"] - d0["J off"]))


@needs_ld
@pytest.mark.parametrize("dt", DTS)
def test_thermal_jacobian_parity(api, mesh, dt):
    m, wg, dwg = mesh
    Tm, S = ts.private("thermal_model", dt), ts.private("scalar_model", dt)
    got = q_at(api, mesh, dt)
    rp, ci = got["pattern"]
    A, A_abs = Tm.jacobian_T(m.xg, m.ien, wg, Tm.config(**THERMAL))
    want, scale = S.on_pattern(A, rp, ci), float(np.abs(S.on_pattern(A_abs, rp, ci)).max())
    ratio = float(np.abs(got["JT thermal"] - want).max() / scale)
    print("dt %g thermal JT: %.3e of the abs-sum" % (dt, ratio))
    assert ratio <= BOUND
    assert not np.array_equal(raw(got["JT thermal"]), raw(got["JT"]))
    assert not np.array_equal(raw(got["JT thermal"]), raw(q_at(api, mesh, None)["JT thermal"]))


@pytest.mark.parametrize("dt", DTS)
def test_phase_diagonal(api, mesh, dt):
    Pm = ts.private("phase_model", dt)
    got = q_at(api, mesh, dt)
    rp, ci = got["pattern"]
    assert got["D"].max() > 0.0
    same(got["J phase"].reshape(-1), Pm.update_J(got["J off"], got["D"], rp, ci), "J with the phase change")
    assert not np.array_equal(raw(got["J phase"]), raw(got["J off"]))


# ---- 2. the default is the default ----------------------------------------------------------------------------------------------
def test_default_step_set_equals_never_set(api, mesh):
    a, b = q_at(api, mesh, None), quantities(api, *mesh, ts.DEFAULT_DT)
    for k in a:
        if k != "pattern":
            same(a[k], b[k], k)


# ---- 3. the bits of the build before the change -------------------------------------------------------------------------------
def test_bits_of_the_parent(api):
    doc = json.load(open(os.path.join(ROOT, "tests", "golden", "timestep_default_bits.json")))
    here = G.compiler_string()
    if here != doc["hipcc_version"]:
        print("compiler here:\n%s\nrecorded:\n%s" % (here, doc["hipcc_version"]))
        pytest.skip("the golden bits were recorded with another compiler: " + doc["hipcc_version"].splitlines()[0])
    got = G.collect(api)
    bad = [k for k in doc["sha256"] if got.get(k) != doc["sha256"][k]]
    assert not bad, bad


# ---- 4. driver wiring -------------------------------------------------------------------------------------------------------------
def _state(api, m):
    wgold, dwgold = synthetic_fields(m)
    return _dev(api, wgold, dwgold, dwgold.copy())


def _work(api, N):
    return api.DeviceArray(6 * N), api.DeviceArray(6 * N)


def _steps(api, m, dts, transport=False, start=None):
    """one time_step per entry of dts on a fresh Problem; returns (wgold, dwgold, dwg) as numpy"""
    P = api.Problem(m)
    if transport:
        P.set_scalar_transport()
    d = _dev(api, *start) if start is not None else _state(api, m)
    F_d, dx_d = _work(api, m.num_node)
    for dt in dts:
        if dt is not None:
            P.set_time_step(dt)
        P.time_step(d[0], d[1], d[2], F_d, dx_d, newton_maxit=2)
    api.sync()
    out = [a.numpy() for a in d]
    P.close()
    return out


def test_time_step_by_hand(api, mesh):
    m = mesh[0]
    N = m.num_node
    dt = 1e-3
    L = api.lib()
    L.dfl_alpha_predict.restype, L.dfl_alpha_predict.argtypes = None, [C.c_int32, C.c_double, C.c_void_p, C.c_void_p]
    L.dfl_alpha_correct.restype = None
    L.dfl_alpha_correct.argtypes = [C.c_int32, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    import scalar_model as sm
    a = _steps(api, m, [dt])
    P = api.Problem(m)
    P.set_time_step(dt)
    d = _state(api, m)
    F_d, dx_d = _work(api, N)
    L.dfl_alpha_predict(N, (sm.kGAMMA - 1.0) / sm.kGAMMA, d[2].ptr, L.DflStream())
    P.solve_flow_system(d[0], d[1], d[2], F_d, dx_d, maxit=2)
    L.dfl_alpha_correct(N, dt * (1.0 - sm.kGAMMA), dt * sm.kGAMMA, d[0].ptr, d[1].ptr, d[2].ptr, L.DflStream())
    api.sync()
    for x, y, name in zip(a, [v.numpy() for v in d], ("wgold", "dwgold", "dwg")):
        same(x, y, name)
    P.close()
    b = _steps(api, m, [None])
    assert not np.array_equal(raw(a[0]), raw(b[0]))


def test_scalar_transport_follows_the_step(api, mesh):
    m = mesh[0]
    N = m.num_node
    a, b = _steps(api, m, [1e-3, None], transport=True), _steps(api, m, [None, None], transport=True)
    assert np.isfinite(a[0]).all()
    assert not np.array_equal(raw(a[0][5 * N:]), raw(b[0][5 * N:]))
    assert not np.array_equal(raw(a[0][4 * N:5 * N]), raw(b[0][4 * N:5 * N]))


def test_solidification_record_books_the_step(api, mesh):
    m = mesh[0]
    N = m.num_node
    dt, k = 1e-3, 3
    P = api.Problem(m)
    P.set_time_step(dt)
    P.set_solidification(T_front=0.5, in_time_step=True)
    d = _state(api, m)
    F_d, dx_d = _work(api, N)
    for _ in range(k):
        P.time_step(d[0], d[1], d[2], F_d, dx_d, newton_maxit=1)
    t = P.solidification_stats()["time"]
    P.close()
    assert abs(t - k * dt) <= 4 * k * np.finfo(float).eps * k * dt, t


def test_capture_source_is_taken_over_the_step(api):
    """step 1 captures; step 2 of the two-way context equals the one-way context whose caller took the source with time = dt
    and registered it by hand, and differs from one who took it with the default step"""
    m = kuhn_cube(4)
    N = m.num_node
    dt = 1e-2
    r = 0.01
    mass = 7800.0 * 4.0 / 3.0 * np.pi * r ** 3
    runs = {}
    for mode in ("two_way", "by_hand", "by_hand_default"):
        w0 = np.zeros(6 * N)
        w0[4 * N:5 * N] = m.xg.reshape(-1, 3)[:, 2] - 0.5
        w0[5 * N:] = 2000.0
        xy = np.array([[0.3, 0.3], [0.5, 0.3], [0.7, 0.3], [0.3, 0.6], [0.5, 0.6], [0.7, 0.62]]) + 0.013
        pts = np.concatenate([np.c_[xy, np.full(6, 0.508)], np.c_[xy, np.full(6, 0.62)]])
        vel = np.tile([0.0, 0.0, -1.0], (12, 1))
        P = api.Problem(m, maxit=120, atol=1e-14, rtol=1e-6)
        P.set_time_step(dt)
        pc = api.Particles(pts.reshape(-1), vel.reshape(-1), r, mass=mass, dt=1e-3)
        try:
            pc.couple(P, rho_f=1.0e3, mu_f=1.0e-3)
            pc.set_capture(level=0.0, side=-1, reach=0.0, T_melt=1500.0, two_way=(mode == "two_way"))
            st = _dev(api, w0, np.zeros(6 * N), np.zeros(6 * N))
            F_d, dx_d = _work(api, N)
            P.time_step(st[0], st[1], st[2], F_d, dx_d, newton_maxit=2, particles=pc, dem_substeps=20)
            api.sync()
            assert pc.capture_stats()["captured"] == 6
            if mode != "two_way":
                q = pc.capture_source(dt if mode == "by_hand" else ts.DEFAULT_DT)
                P.set_volume_source(q[0])
                P.set_external_load(q[1])
            it, rn, r0 = P.time_step(st[0], st[1], st[2], F_d, dx_d, newton_maxit=2, particles=pc, dem_substeps=20)
            api.sync()
            runs[mode] = (r0, rn, st[0].numpy())
            if mode != "two_way":
                P.set_volume_source(None)
                P.set_external_load(None)
        finally:
            pc.close()
            P.close()
    a, b, c = runs["two_way"], runs["by_hand"], runs["by_hand_default"]
    assert a[0][1] > 0.0
    for x, y in zip(a, b):
        same(x, y, "two-way against by hand with time = dt")
    assert not np.array_equal(raw(a[0]), raw(c[0]))


# ---- 5. the step changes mid-run ------------------------------------------------------------------------------------------------
def test_step_changes_mid_run(api, mesh):
    m = mesh[0]
    dt1, dt2 = 2e-2, 1e-3
    mid = _steps(api, m, [dt1, None], transport=True)                  # (None: the step stays dt1)
    a = _steps(api, m, [dt1, None, dt2], transport=True)
    b = _steps(api, m, [dt2], transport=True, start=mid)
    for x, y, name in zip(a, b, ("wgold", "dwgold", "dwg")):
        same(x, y, name)
    c = _steps(api, m, [dt1], transport=True, start=mid)
    assert not np.array_equal(raw(a[0]), raw(c[0]))


# ---- 6. two meshes, two steps -------------------------------------------------------------------------------------------------------
def test_two_problems_two_steps(api, mesh):
    m = mesh[0]
    m2 = kuhn_cube(5, jitter=0.2)
    dta, dtb = 1e-3, 2e-1
    alone = _steps(api, m, [dta, None]), _steps(api, m2, [dtb, None])
    Pa, Pb = api.Problem(m), api.Problem(m2)
    Pa.set_time_step(dta)
    Pb.set_time_step(dtb)
    da, db = _state(api, m), _state(api, m2)
    wa, wb = _work(api, m.num_node), _work(api, m2.num_node)
    for _ in range(2):                                                   # interleaved
        Pa.time_step(da[0], da[1], da[2], wa[0], wa[1], newton_maxit=2)
        Pb.time_step(db[0], db[1], db[2], wb[0], wb[1], newton_maxit=2)
    api.sync()
    assert Pa.time_step_size() == dta and Pb.time_step_size() == dtb
    for got, ref in ((da, alone[0]), (db, alone[1])):
        for x, y, name in zip(got, ref, ("wgold", "dwgold", "dwg")):
            same(x.numpy(), y, name)
    Pa.close()
    Pb.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("inf")])
def test_refusals(api, mesh, bad, capfd):
    P = api.Problem(mesh[0])
    try:
        assert P.time_step_size() == ts.DEFAULT_DT
        P.set_time_step(2.5e-4)
        capfd.readouterr()
        P.set_time_step(bad)
        err = capfd.readouterr().err
        assert "DflMeshSetTimeStep" in err and "unchanged" in err, err
        assert P.time_step_size() == 2.5e-4
    finally:
        P.close()
