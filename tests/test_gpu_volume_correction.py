"""GPU tests of the level-set volume correction (include/dedflow.h "level-set volume correction"; host/volume.c,
csrc/k_volume.hip) against tests/volume_correction_model.py on the meshes and fields of test_gpu_redistance.py: conservation,
the shift, the bits of the new phi and of everything around it, the evaluator, the four statuses, the target calls,
DflTimeStep and the refusals.

Setup.  L = the largest extent of the mesh, max_shift = 0.1 L, tol = 1e-10.  The drifts +0.03 L and -0.0437 L are off the
candidate grid (a drift of +-0.05 L would land on a candidate and test nothing); the target is the float64 model's
V(level - drift).

Bounds.
  conservation  the float64 model's volume of the device's new phi at level is within (tol + 1e-12) V_mesh of the target: tol
                is what the search stops at, 1e-12 covers the rounding of the volume sums and of phi + delta (test_volume_
                correction_cpu.py).  Path independent.
  shift         |delta_dev - delta_model| <= 2 tol V_mesh / A + 1e-12 L, A = the model's |dV/dc| at its root by a central
                difference with eta = 1e-4 L: both searches stop within tol V_mesh of the target, so their roots differ by at
                most 2 tol V_mesh / A.  A is an area, of order one here (0.03 on the single tet, 0.3 .. 3.2 on the
                other meshes: the surface area of the plane or sphere inside the mesh times 1 / |grad phi|); the observed ratio
                goes to the Recorder (profiles/volume_correction_parity.jsonl is such a run).
  evaluator     volume_before, volume_after and volume_mesh to 1e-12 relative to max(1, |value|); band_tets exactly.
  bits          new phi = fl(phi + shift) with the reported shift at every node, a NaN keeps its bits, every other slot of w
                and the guard bands are untouched; two runs and a run after the band list grew give the same bits."""
import ctypes as C

import numpy as np
import pytest

import redistance_model as rm
import volume_correction_model as vm
from dedflow_amd.meshgen import kuhn_cube, synthetic_fields
from guarded_buffers import Pool, Recorder, assert_bits, raw
from test_gpu_redistance import FIELDS, MESHES, TILT, _mesh, _problem, case, extent, state

pytestmark = pytest.mark.gpu
TOL = 1e-10
DRIFTS = [0.03, -0.0437]
MUST_CORRECT = {(mn, f) for mn in ("fan", "cube4", "cube12") for f in ("plane", "sphere", "sphere3")}
record = Recorder("a")


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


_setup_cache, _model_cache = {}, {}


def setup(mesh_name, field, drift):
    """(mesh, phi, level, max_shift, target)"""
    key = (mesh_name, field, drift)
    if key not in _setup_cache:
        m, phi, level, _ = case(mesh_name, field)
        L = extent(m)
        target = float(rm.volume(m.xg, m.ien, phi, level - drift * L))
        if field == "unreached":                                 # V = 0 on the whole bracket: any volume is out of reach
            target = 0.01 * vm.mesh_volume(m)
        _setup_cache[key] = (m, phi, level, 0.1 * L, target)
    return _setup_cache[key]


def model(mesh_name, field, drift, passes=vm.PASSES):
    key = (mesh_name, field, drift, passes)
    if key not in _model_cache:
        m, phi, level, ms, target = setup(mesh_name, field, drift)
        _model_cache[key] = vm.correct(m, phi, level, ms, TOL, target, passes=passes)
    return _model_cache[key]


def _close(got, want):
    return abs(got - want) <= 1e-12 * max(1.0, abs(want))


def _run(api, pool, P, m, phi, level, ms, target, **cfg):
    """set, correct a guarded state in place; returns (status, new phi, stats) after the bands, every other slot of w and the
    bits of the new phi were checked"""
    N = m.num_node
    P.set_volume_correction(level, ms, TOL, target, **cfg)
    assert P.volume_correction_on
    ws = pool.slot(state(m, phi))
    status = P.volume_correct(ws.ptr)
    api.sync()
    st = P.volume_correction_stats()
    assert st["status"] == status
    written = np.zeros(6 * N, bool)
    written[4 * N:5 * N] = status in (0, 3)
    new = ws.check("w: bands, u, p, dphi-side slots and T", written=written)[4 * N:5 * N].copy()
    with np.errstate(invalid="ignore"):
        assert_bits(new, np.where(np.isnan(phi), phi, phi + st["shift"]), "phi + shift")
    if status in (1, 2):
        assert st["shift"] == 0.0 and st["volume_after"] == st["volume_before"]
    return status, new, st


@pytest.mark.parametrize("drift", DRIFTS)
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("mesh_name", list(MESHES))
def test_against_the_model(api, pool, mesh_name, field, drift):
    m, phi, level, ms, target = setup(mesh_name, field, drift)
    ref = model(mesh_name, field, drift)
    L = extent(m)
    P = _problem(api, mesh_name)
    try:
        status, new, st = _run(api, pool, P, m, phi, level, ms, target)
        V_new = float(rm.volume(m.xg, m.ien, new, level))
        miss = abs(V_new - target) / ref["volume_mesh"]
        print(f"volume correction {mesh_name}/{field}/{drift:+}: status {status} (model {ref['status']}), {st['passes']} passes "
              f"(model {ref['passes']}), {st['band_tets']} band tets, shift / L {st['shift'] / L:+.9f}, "
              f"|V - target| / V_mesh {miss:.2e}")
        # statuses: the cases the model corrects must be corrected
        if (mesh_name, field) in MUST_CORRECT:
            assert ref["status"] == 0
        assert status == ref["status"]
        # conservation, path independent
        if status == 0:
            record("volume_conservation", f"{mesh_name}/{field}/{drift:+}", miss / (TOL + 1e-12), passes=st["passes"])
            assert miss <= TOL + 1e-12
            assert abs(st["shift"]) <= ms
        # the shift against the model's
        if status == 0:
            A = vm.slope(m, phi, level - ref["shift"], 1e-4 * L)
            assert A > 0.0
            bound = 2.0 * TOL * ref["volume_mesh"] / A + 1e-12 * L
            dev = abs(st["shift"] - ref["shift"])
            print(f"    A = {A:.3f}, |delta_dev - delta_model| = {dev:.2e} against {bound:.2e}")
            record("volume_shift", f"{mesh_name}/{field}/{drift:+}", dev / bound, A=A)
            assert dev <= bound
        # the evaluator
        assert st["band_tets"] == ref["band_tets"]
        assert _close(st["volume_mesh"], vm.mesh_volume(m)) and _close(st["volume_mesh"], ref["volume_mesh"])
        assert _close(st["volume_before"], float(rm.volume(m.xg, m.ien, phi, level)))
        assert _close(st["volume_after"], V_new)
        assert st["target"] == target
        assert _close(P.level_set_volume(pool.slot(state(m, new)).ptr, level), st["volume_after"])
        if field == "nan":
            assert np.isnan(new).sum() == 1
        if field == "unreached":
            assert status == 2 and st["band_tets"] == 0 and st["volume_before"] == 0.0
        # a second call on the same input: the same bits, the same statistics
        status2, new2, st2 = _run(api, pool, P, m, phi, level, ms, target)
        assert status2 == status and st2 == st
        assert_bits(new2, new, "phi of a second run")
    finally:
        P.close()


def test_cases_cover_the_paths():
    """what the cases are there for: a band list beyond its first capacity and several workgroups, tets of all three classes,
    all four cut shapes among the band tets, a NaN tet"""
    for field in ("plane", "sphere"):
        m, phi, level, ms, _ = setup("cube12", field, DRIFTS[0])
        inside, band = vm.classify(m, phi, level, ms)
        assert band.sum() > 1024 and inside.any() and (~inside & ~band).any() and m.num_tet > 40 * 256
        npos = (phi[m.ien.reshape(-1, 4)][band] > level).sum(axis=1)
        assert set(npos) == {0, 1, 2, 3, 4}
    assert all(_mesh(k).num_tet % 256 for k in MESHES)


def test_same_bits_after_the_band_list_grew(api, pool):
    args = setup("cube12", "plane", DRIFTS[1])
    fresh = _problem(api, "cube12")
    try:
        status, want, st = _run(api, pool, fresh, *args)
        assert status == 0 and st["band_tets"] > 1024            # more than the list holds at first: this call grew it
    finally:
        fresh.close()
    P = _problem(api, "cube12")
    try:
        for f in ("unreached", "sphere3"):                       # nothing, then a smaller band: the list grows in two steps
            _run(api, pool, P, *setup("cube12", f, DRIFTS[1]))
        status2, got, st2 = _run(api, pool, P, *args)
        assert status2 == 0 and st2 == st
        assert_bits(got, want, "phi after unrelated calls")
    finally:
        P.close()


def test_statuses_and_target(api, pool, monkeypatch, capfd):
    m, phi, level, ms, target = setup("cube12", "sphere", DRIFTS[0])
    V0 = float(rm.volume(m.xg, m.ien, phi, level))
    P = _problem(api, "cube12")
    try:
        # 1: zero drift, nothing written, no pass
        status, new, st = _run(api, pool, P, m, phi, level, ms, V0)
        assert status == 1 and st["passes"] == 0
        assert_bits(new, phi, "phi at zero drift")
        # 2: a target outside the bracket, on either side
        for d in (0.15, -0.15):
            far = float(rm.volume(m.xg, m.ien, phi, level - d * extent(m)))
            status, new, st = _run(api, pool, P, m, phi, level, ms, far)
            assert status == 2 and st["passes"] == 0
            assert_bits(new, phi, "phi with an unreachable target")
        # 3: the pass limit forced to 1; the best candidate so far is applied
        monkeypatch.setenv("DFL_VOLUME_PASSES", "1")
        status, new, st = _run(api, pool, P, m, phi, level, ms, target)
        ref = model("cube12", "sphere", DRIFTS[0], passes=1)
        assert status == 3 == ref["status"] and st["passes"] == 1
        assert abs(st["shift"] - ref["shift"]) <= 1e-12 * extent(m) and st["shift"] != 0.0
        assert TOL * st["volume_mesh"] < abs(st["volume_after"] - target) < abs(st["volume_before"] - target)
        assert _close(st["volume_after"], float(rm.volume(m.xg, m.ien, new, level)))
        for bad in ("0", "x", "2.5"):
            monkeypatch.setenv("DFL_VOLUME_PASSES", bad)
            capfd.readouterr()
            P.set_volume_correction(level, ms, TOL, 0.123)
            assert "DFL_VOLUME_PASSES" in capfd.readouterr().err and P.volume_target == target    # unchanged
        monkeypatch.delenv("DFL_VOLUME_PASSES")
        # an unset target: the first call records V(level) and returns 1; the next one has nothing to do
        P.set_volume_correction(level, ms, TOL)
        assert np.isnan(P.volume_target) and P.volume_correction_stats()["status"] == -1
        ws = pool.slot(state(m, phi))
        assert P.volume_correct(ws.ptr) == 1
        assert_bits(ws.check("w of the recording call"), ws.host(), "nothing written")
        assert _close(P.volume_target, V0) and P.volume_target == P.volume_correction_stats()["volume_before"]
        assert P.volume_correct(ws.ptr) == 1
        # SetTarget / AddTarget
        P.volume_target = target
        assert P.volume_target == target
        P.add_volume_target(0.125)
        assert P.volume_target == target + 0.125
        P.add_volume_target(-0.125)
        assert P.volume_correct(ws.ptr) == 0
        api.sync()
        N = m.num_node
        assert abs(float(rm.volume(m.xg, m.ien, ws.get()[4 * N:5 * N], level)) - target) <= (TOL + 1e-12) * st["volume_mesh"]
    finally:
        P.close()


# ---- DflTimeStep -------------------------------------------------------------------------------------------------------------
def _steps(api, m, mode, nstep):
    """nstep time steps of a steep phi.  mode: "never"; "cleared" (set, then NULL); "every0"; "every2"; "by hand"
    (DflMeshVolumeCorrect before steps 2 and 4); "both2" (redistancing and correction with every = 2); "both by hand"
    (redistance, then correct, before steps 2 and 4); "both swapped" (correct, then redistance)"""
    N = m.num_node
    wg, dwg = synthetic_fields(m)
    x = m.xg.reshape(-1, 3)
    wg[4 * N:5 * N] = 3.0 * ((x - 0.5) @ TILT)
    wg[5 * N:] = 1650.0 + 120.0 * ((x - 0.5) @ TILT)
    target = float(rm.volume(m.xg, m.ien, wg[4 * N:5 * N], -0.06))
    P = api.Problem(m, maxit=120, atol=1e-14, rtol=1e-6)
    try:
        P.set_scalar_transport(phi=True, T=True)
        if mode != "never":
            P.set_volume_correction(0.0, 0.2, TOL, target, every=2 if mode in ("every2", "both2") else 0)
        if mode.startswith("both"):
            P.set_redistance(0.0, 0.3, every=2 if mode == "both2" else 0)
        if mode == "cleared":
            P.set_volume_correction()
            assert not P.volume_correction_on
        st = [api.DeviceArray.from_numpy(a) for a in (wg, 0.1 * dwg, 0.1 * dwg)]
        F_d, dx_d = api.DeviceArray(6 * N), api.DeviceArray(6 * N)
        its, seen = [], []
        for k in range(nstep):
            if k % 2 == 1:
                if mode == "by hand":
                    assert P.volume_correct(st[0]) == 0
                elif mode == "both by hand":
                    assert P.redistance(st[0]) > 0
                    assert P.volume_correct(st[0]) == 0
                elif mode == "both swapped":
                    assert P.volume_correct(st[0]) == 0
                    assert P.redistance(st[0]) > 0
            its.append(P.time_step(st[0], st[1], st[2], F_d, dx_d, newton_maxit=2)[0])
            if mode == "every2":
                seen.append(P.volume_correction_stats())
        api.sync()
        return dict(it=its, w=st[0].numpy(), dw=st[2].numpy(), seen=seen)
    finally:
        P.close()


def test_time_step_corrects_every_other_step(api):
    m = _mesh("cube4")
    run = {mode: _steps(api, m, mode, 4 if mode in ("every2", "by hand") else 2)
           for mode in ("never", "cleared", "every0", "every2", "by hand", "both2", "both by hand", "both swapped")}
    for k in ("w", "dw"):
        assert np.isfinite(run["never"][k]).all()
        assert_bits(run["cleared"][k], run["never"][k], f"{k} with the feature cleared")
        assert_bits(run["every0"][k], run["never"][k], f"{k} with every = 0")
        assert_bits(run["every2"][k], run["by hand"][k], f"{k} with every = 2")
        assert_bits(run["both2"][k], run["both by hand"][k], f"{k} with redistancing and correction, every = 2")
    assert run["every0"]["it"] == run["never"]["it"] and run["every2"]["it"] == run["by hand"]["it"]
    assert (raw(run["both swapped"]["w"]) != raw(run["both by hand"]["w"])).any()      # the order matters, so it is tested
    seen = run["every2"]["seen"]                                                        # calls 2 and 4 only
    assert seen[0]["status"] == -1 and seen[1]["status"] == 0 and seen[2] == seen[1] and seen[3]["status"] == 0
    assert seen[3] != seen[1] and seen[1]["shift"] != 0.0
    one = {mode: _steps(api, m, mode, 1) for mode in ("never", "every2")}               # the first step is not an every-th one
    assert_bits(one["every2"]["w"], one["never"]["w"], "w after one step")


def test_time_step_adds_the_captured_volume_to_the_target(api):
    """the steps of test_gpu_capture.py: step 1 captures six particles, step 2 takes their source.  The capture deposits a
    particle's mass at the fluid density, so the volume is 6 m / rho_f; with side = -1 the metal is {phi < level} and the
    target, the volume of {phi > level}, shrinks by it.  The target starts at 0 so that the sum is not rounded into it"""
    from test_gpu_capture import STEP_MASS, _step_setup
    m = kuhn_cube(4)
    total = 6 * STEP_MASS / 1.0e3
    got = {}
    for track in (True, False):
        P, pc, st, F_d, dx_d = _step_setup(api, m)
        try:
            pc.set_capture(level=0.0, side=-1, reach=0.0, T_melt=1500.0, two_way=True)
            P.set_volume_correction(0.0, 0.05, TOL, 0.0, side=-1, track_capture=track)
            P.time_step(st[0], st[1], st[2], F_d, dx_d, newton_maxit=2, particles=pc, dem_substeps=20)
            api.sync()
            assert pc.capture_stats()["captured"] == 6 and P.volume_target == 0.0      # nothing was pending in step 1
            P.time_step(st[0], st[1], st[2], F_d, dx_d, newton_maxit=2, particles=pc, dem_substeps=20)
            got[track] = P.volume_target
            P.time_step(st[0], st[1], st[2], F_d, dx_d, newton_maxit=2, particles=pc, dem_substeps=20)
            assert P.volume_target == got[track]                                         # nothing new was captured
        finally:
            pc.close()
            P.close()
    print(f"captured volume: target {got[True]:.17e} against {-total:.17e}")
    assert got[False] == 0.0
    assert abs(got[True] + total) <= 1e-12 * total


def test_refusals(api, capfd):
    m = _mesh("cube4")
    N = m.num_node
    P = api.Problem(m)
    try:
        capfd.readouterr()
        for kw, reason in [(dict(level=np.nan), "level is not finite"), (dict(max_shift=np.inf), "max_shift is not finite"),
                           (dict(max_shift=0.0), "max_shift must be positive"), (dict(tol=np.nan), "tol is not finite"),
                           (dict(tol=-1.0), "tol must not be negative"), (dict(side=0), "side must be +1 or -1"),
                           (dict(every=-1), "every must not be negative"), (dict(target=np.inf), "target is infinite")]:
            P.set_volume_correction(**dict(dict(level=0.0, max_shift=0.1), **kw))
            err = capfd.readouterr().err
            assert not P.volume_correction_on and reason in err and vm.refusal(**dict(dict(level=0.0), **kw)) == reason, (kw, err)
        w = api.DeviceArray.from_numpy(state(m, (m.xg.reshape(-1, 3) - 0.5) @ TILT))
        before = w.numpy()
        assert api.lib().DflMeshVolumeCorrect(P.mesh, w.ptr) == -1
        assert "no volume correction is set" in capfd.readouterr().err
        assert np.isnan(api.lib().DflMeshVolumeCorrectionTarget(P.mesh))
        s = api.DflVolumeCorrectionStats()
        api.lib().DflMeshVolumeCorrectionStats(P.mesh, C.byref(s))
        assert s.status == -1 and "no volume correction is set" in capfd.readouterr().err
        assert_bits(w.numpy(), before, "nothing written")
        P.set_volume_correction(0.0, 0.1, every=1)
        assert P.volume_correction_on and capfd.readouterr().err == ""
        assert P.volume_correction_stats()["status"] == -1                # no call yet
        P.set_volume_correction(0.0, -0.1, target=0.25)                   # refused: the earlier configuration stays
        assert P.volume_correction_on and np.isnan(P.volume_target) and "max_shift must be positive" in capfd.readouterr().err
        P.volume_target = np.inf
        assert np.isnan(P.volume_target) and "target is infinite" in capfd.readouterr().err
        # a solver with a communicator: refused before anything is computed
        comm = api.DflComm()
        api.lib().KrylovSetComm(P.ksp, C.byref(comm))
        st = [api.DeviceArray.from_numpy(np.zeros(6 * N)) for _ in range(3)]
        F_d, dx_d = api.DeviceArray(6 * N), api.DeviceArray(6 * N)
        assert P.time_step(st[0], st[1], st[2], F_d, dx_d)[0] == -1
        assert "volume correction is single-GPU only" in capfd.readouterr().err
        api.lib().KrylovSetComm(P.ksp, None)
        P.set_volume_correction()
        assert not P.volume_correction_on
    finally:
        P.close()
