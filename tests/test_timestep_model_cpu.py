"""CPU tests of the run-time time step (include/dedflow.h, "time step"): tests/timestep_model.py's private model copies at the
default step against the shared modules bit for bit and away from it, the step-limit restatement against a closed form, the
library's host-only check of a step, and the exported symbols."""
import ctypes as C
import os

import numpy as np
import pytest

import assembly_model as am
import fluid_model as fm
import phase_model as pm
import scalar_model as sm
import thermal_model as tm
import timestep_model as ts
from dedflow_amd.meshgen import kuhn_cube, synthetic_fields

F64 = np.float64
FLUID = dict(rho_gas=1.2, rho_metal=7.8e3, mu_gas=2e-5, mu_metal=6e-3, gravity=(0.0, 0.0, -9.81), beta=1e-4, T_ref=1650.0,
             use_phi=True, level=0.05, side=1, eps=0.3)
THERMAL = dict(k_gas=0.02, k_solid=30.0, k_liquid=45.0, c_gas=1.2e3, c_metal=4.0e6, T_solidus=1600.0, T_liquidus=1700.0,
               use_phi=True, level=0.05, side=1, eps=0.3)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F64)).view(np.uint64)


@pytest.fixture(scope="module")
def case():
    m = kuhn_cube(2, jitter=0.2)
    N = m.num_node
    wg, dwg = synthetic_fields(m)
    x = m.xg.reshape(-1, 3)
    wg[4 * N:5 * N] = (x - 0.5) @ np.array([0.3, 0.1, -1.0]) / np.sqrt(1.1)
    wg[5 * N:] = 1650.0 + 120.0 * ((x - 0.5) @ np.array([0.2, -0.3, 1.0]))
    rp, ci = am.nodal_pattern(m.ien, N)
    g = 4
    nf = int(m.bound_elem_offset[g + 1] - m.bound_elem_offset[g])
    f2e = m.bound_f2e[m.bound_elem_offset[g]:m.bound_elem_offset[g + 1]]
    forn = m.bound_forn[m.bound_elem_offset[g]:m.bound_elem_offset[g + 1]]
    assert nf > 0
    return m, N, wg, dwg, rp, ci, f2e, forn


def outputs(mods, case):
    """name -> float64 array of every dt-dependent output of the five models, mods = (am, sm, pm, tm, fm) or their copies"""
    A, S, Pm, Tm, Fm = mods
    m, N, wg, dwg, rp, ci, f2e, forn = case
    out = {}
    F, blk = A.assemble_tet(m.xg, m.ien, N, wg, dwg, rp, ci, F64)
    out["assembly F"], out["assembly J"] = F.v, blk.v
    _, fblk = A.assemble_face(m.xg, m.ien, N, f2e, forn, wg, dwg, rp, ci, F64)
    out["assembly face J"] = fblk.v
    Jp, Jt = S.jacobians(m.xg, m.ien, wg)
    out["scalar Jphi"], out["scalar JT"] = Jp.toarray(), Jt.toarray()
    wga, _ = S.alpha_states(N, wg, dwg, 0.5 * dwg)
    out["scalar alpha states"] = wga
    D = np.linspace(1.0, 2.0, N)
    out["phase J"] = Pm.update_J(np.zeros(ci.size * 16), D, rp, ci)
    At, _ = Tm.jacobian_T(m.xg, m.ien, wg, Tm.config(**THERMAL))
    out["thermal JT"] = At.toarray()
    cfg = Fm.config(**FLUID)
    out["fluid rows"] = np.asarray(Fm.rows(m.xg, m.ien, wg, dwg, cfg)["r"], F64)
    out["fluid blocks"] = np.asarray(Fm.element_jm(m.xg, m.ien, wg, cfg)[0], F64)
    return out


def _copies(dt):
    return tuple(ts.private(n, dt) for n in ("assembly_model", "scalar_model", "phase_model", "thermal_model", "fluid_model"))


def test_private_copies_are_private():
    for name, shared in zip(ts.MODULES, (am, sm, pm, tm, fm)):
        mod = ts.private(name, 1e-3)
        assert mod is not shared and mod.__name__ != shared.__name__
    assert am.DT == 5e-2 and sm.kDT == 5e-2 and pm.kDT == 5e-2          # the shared modules are as they were
    assert ts.private("fluid_model", 1e-3).sm is ts.private("scalar_model", 1e-3)
    assert fm.sm is sm and tm.sm is sm


def test_default_step_reproduces_the_shared_modules(case):
    ref, got = outputs((am, sm, pm, tm, fm), case), outputs(_copies(ts.DEFAULT_DT), case)
    for k in ref:
        assert np.array_equal(_bits(got[k]), _bits(ref[k])), k


@pytest.mark.parametrize("dt", [1e-3, 2.0])
def test_every_output_depends_on_the_step(case, dt):
    ref, got = outputs((am, sm, pm, tm, fm), case), outputs(_copies(dt), case)
    for k in ref:
        assert np.all(np.isfinite(got[k]))
        assert not np.array_equal(_bits(got[k]), _bits(ref[k])), k + ": a derived name was missed"
    assert sm.kDT == 5e-2 and am.FACT2 == 5e-2 * am.ALPHAF * am.GAMMA


def test_step_consts_match_the_library():
    from dedflow_amd import api
    L = api.lib()
    for dt in (5e-2, 1e-3, 2.0, 3.7e-6):
        k = api.dfl_step_consts()
        L.dfl_step_consts_from_dt(dt, C.byref(k))
        want = ts.step_consts(dt)
        for name in want:
            assert np.float64(getattr(k, name)).view(np.uint64) == np.float64(want[name]).view(np.uint64), (dt, name)


def test_limits_of_one_regular_tet():
    """a regular tet with a uniform velocity along an altitude: 1 / r_e = altitude / |u|"""
    x = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]])     # edge 2 sqrt 2
    alt = np.sqrt(2.0 / 3.0) * 2.0 * np.sqrt(2.0)
    d = x[0] - x[1:].mean(axis=0)
    d /= np.linalg.norm(d)                                               # along the altitude through vertex 0
    speed = 3.0
    w = np.zeros(24)
    w[:12] = np.tile(speed * d, 4)
    w[16:20] = [1.0, -1.0, -1.0, -1.0]                                   # cut by phi = 0
    w[20:24] = 1700.0
    out = ts.step_limits(x.reshape(-1), np.arange(4), w, 4, sigma0=1.8, dsigma_dT=-4e-4, T_ref=1650.0, rho_bar=4000.0)
    assert abs(out["dt_adv"] - alt / speed) <= 8 * np.finfo(float).eps * alt / speed
    assert out["dt_surface"] == out["dt_adv"] and out["tet_adv"] == out["tet_surface"] == out["tet_cap"] == 0
    assert out["num_cut"] == 1 and out["num_nonfinite"] == 0
    sigma = 1.8 - 4e-4 * 50.0
    want = np.sqrt(4000.0 * alt ** 3 / (2.0 * np.pi * sigma))
    assert abs(out["dt_capillary"] - want) <= 1e-14 * want
    hot = ts.step_limits(x.reshape(-1), np.arange(4), np.where(np.arange(24) >= 20, 1e4, w), 4, sigma0=1.8, dsigma_dT=-4e-4)
    assert hot["cap_q"] == 0.0 and hot["dt_capillary"] == np.inf and hot["tet_cap"] == 0   # sigma clamps at 0


def test_time_step_check_refusals():
    from dedflow_amd import api
    L = api.lib()
    why = C.create_string_buffer(160)
    for dt in (5e-2, 1e-6, 1e300, 5e-324):
        assert L.DflTimeStepCheck(dt, why, 160) == 0, dt
    for dt in (0.0, -0.0, -1.0, float("nan"), float("inf"), float("-inf")):
        assert L.DflTimeStepCheck(dt, why, 160) != 0 and b"dt" in why.value, dt


def test_symbols_declared_and_exported():
    from dedflow_amd import api
    lib = api.lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pub = open(os.path.join(root, "include", "dedflow.h")).read()
    ker = open(os.path.join(root, "include", "dedflow_kernels.h")).read()
    for n in ("DflTimeStepCheck", "DflMeshSetTimeStep", "DflMeshTimeStep", "DflMeshTimeStepLimits", "DFL_DEFAULT_TIME_STEP",
              "DflTimeStepLimits"):
        assert n in pub, n
    for n in ("DflTimeStepCheck", "DflMeshSetTimeStep", "DflMeshTimeStep", "DflMeshTimeStepLimits"):
        assert hasattr(lib, n), n
    for n in ("dfl_step_consts_from_dt", "dfl_step_consts_default", "dfl_assemble_tet_lhs_dt", "dfl_assemble_tet_rhs_dt",
              "dfl_assemble_tet_lhs_slot_dt", "dfl_assemble_tet_rhs_lane_dt", "dfl_assemble_face_dt", "dfl_assemble_face_park_dt",
              "dfl_assemble_scalar_jacobian_dt", "dfl_assemble_scalar_jacobian_material_dt", "dfl_fluid_rows_dt",
              "dfl_fluid_add_rows_dt", "dfl_fluid_add_jacobian_dt", "dfl_step_limits", "dfl_step_limit_partials",
              "dfl_step_limit_finish", "dfl_step_limit_grid"):
        assert n in ker and hasattr(lib, n), n
    for n in ("set_time_step", "time_step_size", "time_step_limits"):
        assert hasattr(api.Problem, n), n
    assert "nothing here checks it" not in pub


def test_the_step_is_named_once_in_the_product():
    """the compile-time step is gone from the product code: one line names the default"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hits = []
    for dp, _, fs in os.walk(os.path.join(root, "dedflow_amd")):
        for f in fs:
            if f.endswith((".py", ".c", ".h", ".hpp", ".hip")):
                for i, line in enumerate(open(os.path.join(dp, f), errors="replace")):
                    if "kDT" in line:
                        hits.append((f, i + 1))
    assert len(hits) == 1, hits
