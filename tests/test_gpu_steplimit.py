"""GPU tests of the step limits (include/dedflow.h, "time step"; csrc/k_steplimit.hip, host/timestep.c): the launcher alone on
synthetic decks against the float64 restatement of tests/timestep_model.py, every f64 and every id bit for bit (maxima are
exact in any order and the per-tet formulas are fixed operation by operation), between NaN guard bands; then
Problem.time_step_limits on a Kuhn cube with and without surface forces and a fluid material."""
import numpy as np
import pytest

import assembly_model as am
import timestep_model as ts
from dedflow_amd.meshgen import kuhn_cube, synthetic_fields
from guarded_buffers import I32, Pool, assert_bits, sent

pytestmark = pytest.mark.gpu
SIGMA = dict(sigma0=1.8, dsigma_dT=-4.0e-4, T_ref=1650.0)
KEYS_V = ("rate_adv", "rate_adv_surface", "cap_q")
KEYS_I = ("tet_adv", "tet_surface", "tet_cap", "num_cut", "num_nonfinite")


@pytest.fixture(scope="module")
def api():
    from dedflow_amd import api as A
    A.lib()
    return A


@pytest.fixture
def pool(api):
    p = Pool(api)
    yield p
    p.free()


def deck(T, seed=5, cut=True):
    """T disjoint tets with random velocities, phi through 0 (cut) or all positive, T through the range where sigma varies"""
    xg, ien = am.tet_soup(T, "unit", seed=seed)
    N = 4 * T
    rng = np.random.default_rng(seed)
    w = np.zeros(6 * N)
    w[:3 * N] = rng.standard_normal(3 * N)
    w[4 * N:5 * N] = rng.standard_normal(N) if cut else rng.uniform(0.5, 1.5, N)
    w[5 * N:] = rng.uniform(1500.0, 1900.0, N)
    return np.ascontiguousarray(xg, np.float64).reshape(-1), np.ascontiguousarray(ien, np.int32).reshape(-1), w, N


def launch(api, pool, xg, ien, w, N, level=0.0, max_workgroups=0, **sig):
    """dfl_step_limits between guard bands; returns the dict of the three maxima, three ids and two counts"""
    L = api.lib()
    T = ien.size // 4
    grid = L.dfl_step_limit_grid(T, max_workgroups)
    assert 1 <= grid <= max(1, (T + 255) // 256) and (max_workgroups == 0 or grid <= max_workgroups)
    xs, ws, es = pool.slot(xg), pool.slot(w, off=1), pool.slot(ien, 0, I32)
    pv, pi = pool.slot(sent(3 * grid)), pool.slot(sent(5 * grid, I32), 0, I32)
    ov, oi = pool.slot(sent(3), off=1), pool.slot(sent(5, I32), 0, I32)
    prm = api.dfl_step_limit_params(level, sig.get("sigma0", 0.0), sig.get("dsigma_dT", 0.0), sig.get("T_ref", 0.0))
    L.dfl_step_limits(T, es.ptr, xs.ptr, ws.ptr, N, prm, max_workgroups, pv.ptr, pi.ptr, ov.ptr, oi.ptr, None)
    api.sync()
    for s, name in ((xs, "xg"), (ws, "w"), (es, "ien")):
        s.check(name + ": an input changed")
    pv.check("partials", written=True)
    pi.check("partial ids", written=True)
    v, i = ov.check("out_v", written=True), oi.check("out_i", written=True)
    out = dict(zip(KEYS_V, (float(a) for a in v)))
    out.update(zip(KEYS_I, (int(a) for a in i)))
    return out


def agree(got, ref, what):
    for k in KEYS_V:
        assert_bits(np.array([got[k]]), np.array([ref[k]]), "%s: %s" % (what, k))
    for k in KEYS_I:
        assert got[k] == ref[k], (what, k, got[k], ref[k])


@pytest.mark.parametrize("T", [1, 255, 256, 257])
def test_launcher_sizes(api, pool, T):
    xg, ien, w, N = deck(T)
    ref = ts.step_limits(xg, ien, w, N, **SIGMA)
    got = launch(api, pool, xg, ien, w, N, **SIGMA)
    agree(got, ref, "T = %d" % T)
    assert got["rate_adv"] > 0.0 and got["tet_adv"] >= 0 and got["num_nonfinite"] == 0
    if T > 1:
        assert 0 < got["num_cut"] < T and got["cap_q"] > 0.0


def test_grid_stride_loop_wraps(api, pool):
    xg, ien, w, N = deck(2000, seed=9)
    ref = ts.step_limits(xg, ien, w, N, level=0.1, **SIGMA)
    a = launch(api, pool, xg, ien, w, N, level=0.1, max_workgroups=3, **SIGMA)
    agree(a, ref, "2000 tets on 3 workgroups")
    for wg in (0, 1, 5):
        agree(launch(api, pool, xg, ien, w, N, level=0.1, max_workgroups=wg, **SIGMA), ref, "2000 tets on %d workgroups" % wg)


def test_tie_takes_the_lower_id(api, pool):
    """two congruent tets with the same fields attain every maximum; the copy is placed at ids on both sides of a workgroup
    boundary and of the wrap of a small grid"""
    T = 700
    xg, ien, w, N = deck(T, seed=11)
    x, u = xg.reshape(-1, 3), w[:3 * N].reshape(-1, 3)
    lo, hi = 130, 613
    src, dst = ien.reshape(-1, 4)[lo], ien.reshape(-1, 4)[hi]
    u[src] = 50.0 * u[src]                                                # far above every other tet
    w[4 * N + src[0]], w[4 * N + src[1]] = -1.0, 1.0                      # cut
    w[5 * N + src] = 1500.0
    x[dst], u[dst] = x[src], u[src]                                       # the copy: the same numbers, bit for bit
    w[4 * N + dst], w[5 * N + dst] = w[4 * N + src], w[5 * N + src]
    ref = ts.step_limits(xg, ien, w, N, **SIGMA)
    assert ref["tet_adv"] == lo and ref["tet_surface"] == lo
    for wg in (0, 2):
        got = launch(api, pool, xg, ien, w, N, max_workgroups=wg, **SIGMA)
        agree(got, ref, "tie on %d workgroups" % wg)
    # the same maximum attained by the later tet alone once the earlier one is slowed down
    u[src] = u[src] / 100.0
    ref2 = ts.step_limits(xg, ien, w, N, **SIGMA)
    assert ref2["tet_adv"] == hi
    agree(launch(api, pool, xg, ien, w, N, **SIGMA), ref2, "the later tet alone")


def test_no_cut_tet(api, pool):
    xg, ien, w, N = deck(300, cut=False)
    got = launch(api, pool, xg, ien, w, N, **SIGMA)
    agree(got, ts.step_limits(xg, ien, w, N, **SIGMA), "no cut tet")
    assert got["num_cut"] == 0 and got["tet_surface"] == -1 and got["tet_cap"] == -1
    assert got["rate_adv_surface"] == 0.0 and got["cap_q"] == 0.0 and got["tet_adv"] >= 0
    ref = ts.step_limits(xg, ien, w, N, **SIGMA)
    assert ref["dt_surface"] == np.inf and ref["dt_capillary"] == np.inf and np.isfinite(ref["dt_adv"])


def test_degenerate_and_nan_tets_are_left_out(api, pool):
    xg, ien, w, N = deck(300, seed=13)
    x = xg.reshape(-1, 3)
    e4 = ien.reshape(-1, 4)
    x[e4[40][3]] = x[e4[40][0]]                      # det = 0: gradients are not finite
    w[3 * e4[170][2] + 1] = np.nan                   # a NaN velocity
    w[:3 * N].reshape(-1, 3)[e4[40]] *= 1e6          # (they would win every maximum if they took part)
    ref = ts.step_limits(xg, ien, w, N, **SIGMA)
    assert ref["num_nonfinite"] == 2 and ref["tet_adv"] not in (40, 170)
    got = launch(api, pool, xg, ien, w, N, **SIGMA)
    agree(got, ref, "two non-finite tets")
    clean = deck(300, seed=13)
    keep = np.setdiff1d(np.arange(300), [40, 170])
    sub = ts.step_limits(clean[0], clean[1].reshape(-1, 4)[keep].reshape(-1), clean[2], N, **SIGMA)
    for k in KEYS_V:
        assert got[k] == sub[k], k                   # the maxima come from the others


def test_phi_equal_to_level_counts_as_cut(api, pool):
    xg, ien, w, N = deck(3, cut=False)
    level = 0.25
    w[4 * N:5 * N] = level + np.abs(w[4 * N:5 * N])  # all above the level
    w[4 * N + ien[4 + 2]] = level                    # one vertex of tet 1 exactly on it
    got = launch(api, pool, xg, ien, w, N, level=level, **SIGMA)
    agree(got, ts.step_limits(xg, ien, w, N, level=level, **SIGMA), "phi == level")
    assert got["num_cut"] == 1 and got["tet_surface"] == 1 and got["tet_cap"] == 1


def test_sigma_clamps_at_zero(api, pool):
    xg, ien, w, N = deck(64)
    w[5 * N:] = 1.0e4                                # sigma0 + dsigma_dT (T - T_ref) < 0 everywhere
    got = launch(api, pool, xg, ien, w, N, **SIGMA)
    agree(got, ts.step_limits(xg, ien, w, N, **SIGMA), "hot")
    assert got["num_cut"] > 0 and got["cap_q"] == 0.0 and got["tet_cap"] >= 0 and got["rate_adv_surface"] > 0.0
    w[5 * N + ien[4 * 7: 4 * 8]] = 1600.0            # one cold tet: it alone has a surface tension
    w[4 * N + ien[4 * 7]], w[4 * N + ien[4 * 7 + 1]] = -1.0, 1.0
    got = launch(api, pool, xg, ien, w, N, **SIGMA)
    agree(got, ts.step_limits(xg, ien, w, N, **SIGMA), "one cold tet")
    assert got["tet_cap"] == 7 and got["cap_q"] > 0.0


# ---- through the Problem ---------------------------------------------------------------------------------------------------------
def test_problem_limits(api):
    m = kuhn_cube(5, jitter=0.2)
    N = m.num_node
    wg, _ = synthetic_fields(m)
    x = m.xg.reshape(-1, 3)
    wg[4 * N:5 * N] = (x - 0.5) @ np.array([0.3, 0.1, -1.0]) / np.sqrt(1.1)
    wg[5 * N:] = 1650.0 + 120.0 * ((x - 0.5) @ np.array([0.2, -0.3, 1.0]))
    surf = dict(level=0.05, side=1, eps=0.3, **SIGMA)
    fluid = dict(rho_gas=1.2, rho_metal=7.8e3, mu_gas=2e-5, mu_metal=6e-3, use_phi=True, level=0.05, side=1, eps=0.3)
    P = api.Problem(m)
    try:
        w_d = api.DeviceArray.from_numpy(wg)
        for dt, with_surf, with_fluid in ((None, False, False), (2e-5, True, False), (2e-5, True, True), (1e-4, False, True)):
            if dt is not None:
                P.set_time_step(dt)
            P.set_surface_forces(**surf) if with_surf else P.set_surface_forces()
            P.set_fluid_material(**fluid) if with_fluid else P.set_fluid_material()
            ref = ts.step_limits(m.xg, m.ien, wg, N, level=0.05, rho_bar=0.5 * (1.2 + 7.8e3) if with_fluid else 1.0e3,
                                 dt=P.time_step_size(), **(SIGMA if with_surf else {}))
            got = P.time_step_limits(w_d, level=0.05)
            again = P.time_step_limits(w_d, level=0.05)
            assert got == again                       # run to run
            assert set(got) == set(ref)
            for k in ref:
                if isinstance(ref[k], int):
                    assert got[k] == ref[k], k
                else:
                    assert_bits(np.array([got[k]]), np.array([ref[k]]), k)
            assert got["dt"] == (ts.DEFAULT_DT if dt is None else dt)
            assert got["num_cut"] > 0 and got["num_nonfinite"] == 0 and np.isfinite(got["dt_adv"]) and np.isfinite(got["dt_surface"])
            assert (got["cap_q"] > 0.0 and np.isfinite(got["dt_capillary"])) if with_surf else got["dt_capillary"] == np.inf
        assert np.array_equal(w_d.numpy().view(np.uint64), wg.view(np.uint64))
    finally:
        P.close()
