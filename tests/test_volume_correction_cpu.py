"""CPU tests of the level-set volume correction (include/dedflow.h, "level-set volume correction"): the refusals of
DflVolumeCorrectionCheck (host only, no GPU), and the numpy model of tests/volume_correction_model.py against an np.longdouble
evaluation of V on the cases of test_gpu_volume_correction.py.

Bound.  The model stops at |V(c*) - target| <= tol V_mesh in float64; the longdouble volume of the shifted field differs from
that by the rounding of the float64 volume (a few 1e-16 of a volume of order one) and of the addition phi + delta (1e-16 L
times |dV/dc|, of order one): (tol + 1e-12) V_mesh covers both with room."""
import ctypes as C

import numpy as np
import pytest

import redistance_model as rm
import volume_correction_model as vm
from test_gpu_redistance import _mesh, case, extent

LD = np.longdouble
TOL = 1e-10
DRIFTS = [0.03, -0.0437]                   # times L; off the candidate grid of the first pass (multiples of max_shift / 15)
MESHES = ["fan", "cube4", "cube12"]
FIELDS = ["plane", "sphere", "sphere3"]


def setup(mesh_name, field, drift):
    """(mesh, phi, level, max_shift, target): the target is the float64 model's V(level - drift L)"""
    m, phi, level, _ = case(mesh_name, field)
    L = extent(m)
    target = float(rm.volume(m.xg, m.ien, phi, level - drift * L))
    return m, phi, level, 0.1 * L, target


@pytest.mark.parametrize("drift", DRIFTS)
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("mesh_name", MESHES)
def test_model_meets_the_tolerance(mesh_name, field, drift):
    m, phi, level, ms, target = setup(mesh_name, field, drift)
    L = extent(m)
    res = vm.correct(m, phi, level, ms, TOL, target)
    V_new = rm.volume(m.xg, m.ien, res["phi"], level, dtype=LD)
    miss = float(abs(V_new - LD(target))) / res["volume_mesh"]
    print(f"model {mesh_name}/{field}/{drift:+}: status {res['status']}, {res['passes']} passes, {res['band_tets']} of "
          f"{m.num_tet} tets in the band, shift / L {res['shift'] / L:+.6f}, |V - target| / V_mesh {miss:.2e}")
    assert res["status"] == 0 and 1 <= res["passes"] <= 4
    assert miss <= TOL + 1e-12
    assert abs(res["shift"] - drift * L) <= 1e-6 * L          # the shift undoes the drift
    assert abs(res["shift"]) <= ms
    ok = ~np.isnan(phi)
    assert np.array_equal(res["phi"][ok], phi[ok] + res["shift"])


def test_candidates_are_ascending_and_inside():
    for a, b, Va, Vb, t in [(0.0, 1.0, 1.0, 0.0, 0.3), (-2.0, -1.0, 5.0, 5.0, 5.0), (0.0, 1.0, 1.0, 0.0, 1.0), (0.0, 1.0, 1.0, 0.0, 0.0),
                            (0.25, 0.25 + 1e-15, 0.7, 0.6, 0.65)]:
        c = vm.candidates(a, b, Va, Vb, t)
        assert len(c) == vm.K and all(a <= v <= b for v in c) and all(x <= y for x, y in zip(c, c[1:]))


def test_model_statuses():
    m, phi, level, _ = case("cube4", "plane")
    L = extent(m)
    V0 = float(rm.volume(m.xg, m.ien, phi, level))
    same = vm.correct(m, phi, level, 0.1 * L, TOL, V0)                       # zero drift
    assert same["status"] == 1 and same["passes"] == 0 and same["shift"] == 0.0 and np.array_equal(same["phi"], phi)
    unset = vm.correct(m, phi, level, 0.1 * L, TOL)                           # NaN target: recorded
    assert unset["status"] == 1 and abs(unset["target"] - V0) <= 1e-15   # (V_in + V_band against one sum)
    far = vm.correct(m, phi, level, 0.1 * L, TOL, float(rm.volume(m.xg, m.ien, phi, level - 0.15 * L)))
    assert far["status"] == 2 and far["shift"] == 0.0 and np.array_equal(far["phi"], phi)
    one = vm.correct(m, phi, level, 0.1 * L, TOL, float(rm.volume(m.xg, m.ien, phi, level - 0.03 * L)), passes=1)
    assert one["status"] == 3 and one["passes"] == 1 and abs(one["shift"] - 0.03 * L) < 0.1 * L / vm.K
    for mesh_name in ("single", "fan", "cube4", "cube12"):                    # level = 10 L: no surface within max_shift
        m, phi, level, _ = case(mesh_name, "unreached")
        res = vm.correct(m, phi, level, 0.1 * extent(m), TOL, 0.01)
        assert res["status"] == 2 and res["band_tets"] == 0 and res["volume_before"] == 0.0


def test_check_refuses_what_the_header_lists():
    from dedflow_amd import api
    L = api.lib()
    why = C.create_string_buffer(160)
    good = dict(level=0.0, side=1, max_shift=0.1, tol=1e-10, target=np.nan, every=0, track_capture=0)

    def check(**kw):
        c = dict(good, **kw)
        cfg = api.DflVolumeCorrection(c["level"], c["side"], c["max_shift"], c["tol"], c["target"], c["every"], c["track_capture"])
        code = L.DflVolumeCorrectionCheck(C.byref(cfg), why, 160)
        want = vm.refusal(c["level"], c["side"], c["max_shift"], c["tol"], c["target"], c["every"])
        return code, why.value.decode(), want

    refused = [dict(level=np.nan), dict(level=np.inf), dict(max_shift=np.nan), dict(max_shift=-np.inf), dict(max_shift=0.0),
               dict(max_shift=-0.1), dict(tol=np.nan), dict(tol=np.inf), dict(tol=-1e-300), dict(side=0), dict(side=2), dict(side=-2),
               dict(every=-1), dict(target=np.inf), dict(target=-np.inf)]
    codes = set()
    for kw in refused:
        code, text, want = check(**kw)
        assert code != 0 and want is not None and text.startswith(want), (kw, code, text, want)
        codes.add(code)
    assert codes == set(range(1, 9))
    accepted = [dict(), dict(tol=0.0), dict(side=-1), dict(every=7), dict(target=0.25), dict(target=-1.0), dict(track_capture=1),
                dict(level=-3.5, max_shift=1e-300), dict(max_shift=1e300)]
    for kw in accepted:
        code, text, want = check(**kw)
        assert code == 0 and want is None, (kw, code, text)
