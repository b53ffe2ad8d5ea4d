"""CPU checks of the melt-pool capture: the public and kernel symbols exist, and tests/capture_model.py (the reference of
test_gpu_capture.py) reproduces the closed forms of the model in include/dedflow.h "melt-pool capture" on linear fields.
The coordinates the GPU tests use are checked here for their decision margins."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import capture_model as cm
from dedflow_amd.meshgen import kuhn_cube

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUBLIC = ["ParticleContextSetCapture", "ParticleContextCapture", "ParticleContextCaptureSource", "ParticleContextCaptureStats",
          "DflMeshSetVolumeSource", "DflMeshVolumeSource"]
KERNELS = ["dfl_capture_flag", "dfl_capture_source", "dfl_couple_node_deposit"]


def _header(name):
    txt = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_capture_symbols_declared_and_exported():
    subprocess.check_call(["make", "-s", "-j8", "-C", ROOT])
    lib = ctypes.CDLL(os.path.join(ROOT, "dedflow_amd", "libdedflow.so"))
    pub, ker = _header("dedflow.h"), _header("dedflow_kernels.h")
    assert "DflParticleCapture" in pub and "DflParticleCaptureStats" in pub
    for n in PUBLIC:
        assert re.search(r"\b%s\s*\(" % n, pub), n
        assert hasattr(lib, n), n
    for n in KERNELS:
        assert re.search(r"\b%s\s*\(" % n, ker), n
        assert hasattr(lib, n), n
    from dedflow_amd import api
    assert ctypes.sizeof(api.DflParticleCapture) == 40 and ctypes.sizeof(api.DflParticleCaptureStats) == 16
    for n in ("set_capture", "capture", "capture_source", "capture_stats", "capture_on"):
        assert hasattr(api.Particles, n), n
    assert hasattr(api.Problem, "set_volume_source")


def _case(M=3, P=300):
    m = kuhn_cube(M)
    case = cm.decision_case(m, P)
    tet, lam = cm.brute_locate(m.xg, m.ien, case["pts"])
    return m, case, cm.linear_fields(m.xg), tet, lam


def test_linear_fields_give_the_closed_forms():
    """P1 tets interpolate the linear fields exactly: phi_p = z_p - 0.5, T_f = 1000 + 1000 x_p, u_f = U_0 + U_GRAD x_p, |g| = 1"""
    m, case, w, tet, lam = _case()
    x = case["pts"]
    d = cm.decide(m.xg, m.ien, w, tet, lam, case["R"], cm.LEVEL, -1, 0.0, cm.T_MELT)
    loc = d["located"]
    assert tet[0] == -1 and loc.sum() == len(x) - 1
    assert np.abs(lam[1]).max() == 1.0 or abs(np.abs(lam[1]).max() - 1.0) < 1e-12       # the particle on a node
    assert tet[2] == tet[3] == tet[4]
    assert np.abs(d["phi_p"][loc] - (x[loc, 2] - 0.5)).max() < 1e-14
    assert np.abs(d["T_f"][loc] - (1000.0 + 1000.0 * x[loc, 0])).max() < 1e-11
    assert np.abs(d["u_f"][loc] - (cm.U_0 + x[loc] @ cm.U_GRAD.T)).max() < 1e-14
    assert np.abs(d["gn"][loc] - 1.0).max() < 1e-13
    # the captured set in closed form: below the surface z < 0.5 + level, in the hot half x >= 0.5
    closed = loc & (x[:, 2] < 0.5 + cm.LEVEL) & (1000.0 + 1000.0 * x[:, 0] >= cm.T_MELT)
    assert np.array_equal(d["captured"], closed) and 20 < closed.sum() < 150
    assert not d["captured"][0] and d["captured"][1] and d["captured"][2:5].all()
    assert not d["captured"][x[:, 0] < 0.5].any()                                       # the cold region


@pytest.mark.parametrize("side", [1, -1])
def test_reach_scales_with_the_radius(side):
    """c(reach) - c(0) = reach r_i |g| with |g| = 1: reach = 1 captures exactly the spheres that touch the surface"""
    m, case, w, tet, lam = _case()
    x, r = case["pts"], case["r"]
    d0 = cm.decide(m.xg, m.ien, w, tet, lam, r, cm.LEVEL, side, 0.0, -np.inf)
    d1 = cm.decide(m.xg, m.ien, w, tet, lam, r, cm.LEVEL, side, 1.0, -np.inf)
    loc = d0["located"]
    assert np.abs((d1["c"] - d0["c"])[loc] - r[loc]).max() < 1e-14
    dist = side * (x[:, 2] - 0.5 - cm.LEVEL)                 # signed distance into the metal
    assert np.array_equal(d1["captured"], loc & (dist + r >= 0.0))
    assert np.array_equal(d0["captured"], loc & (dist >= 0.0))
    assert d1["captured"].sum() > d0["captured"].sum() > 0


@pytest.mark.parametrize("M,P", [(3, 300), (3, 1), (4, 12)])
def test_gpu_cases_keep_their_margins(M, P):
    """what every GPU decision test asserts again with the library's tets and weights: rounding cannot flip a decision"""
    m, case, w, tet, lam = _case(M, P)
    for side in (1, -1):
        for reach in (0.0, 1.0):
            for radius in (case["R"], case["r"]):
                for T_melt in (cm.T_MELT, -np.inf):
                    assert cm.margins_ok(cm.decide(m.xg, m.ien, w, tet, lam, radius, cm.LEVEL, side, reach, T_melt), T_melt)


def test_nan_captures_nothing():
    m, case, w, tet, lam = _case()
    w = w.copy()
    w[4 * m.num_node:5 * m.num_node] = np.nan
    assert not cm.decide(m.xg, m.ien, w, tet, lam, case["R"], cm.LEVEL, -1, 0.0, -np.inf)["captured"].any()


def test_node_sums_conserve_the_deposits():
    """sum_a lambda_a = 1: sum_a A[a] = the sum over the captured particles of (V, dP, E)"""
    m, case, w, tet, lam = _case()
    d = cm.decide(m.xg, m.ien, w, tet, lam, case["r"], cm.LEVEL, -1, 1.0, cm.T_MELT)
    dep = cm.deposits(d, case["m"], case["vel"], case["rho_f"], case["cp_p"], case["temp"])
    cap = d["captured"]
    assert np.all(dep[~cap] == 0) and np.all(dep[cap, 0] > 0)
    assert np.all(np.abs(dep[cap, 0] * case["rho_f"] - case["m"][cap]) <= 2 * cm.EPS * case["m"][cap])     # mass is conserved
    A, Aa, cnt = cm.node_accumulate(m.num_node, m.ien, tet, lam, dep, cap)
    assert cnt.sum() == 4 * cap.sum()
    total = dep.sum(axis=0)
    assert np.all(np.abs(A.sum(axis=0) - total) <= 8 * cm.EPS * np.abs(dep).sum(axis=0))
    # heat off: no excess heat anywhere
    assert np.all(cm.deposits(d, case["m"], case["vel"], case["rho_f"])[:, 4] == 0)
