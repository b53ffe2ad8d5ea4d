"""GPU tests of the phi / T transport (include/dedflow.h "scalar transport"; host/scalar.c, csrc/k_scalar.hip): Jacobian
values against tests/scalar_model.py, the oracle's phi / T rows after a solve, a closed form, conservation, Dirichlet
nodes, the coupled Newton step, and the off path bit for bit."""
import numpy as np
import pytest

import scalar_model as sm
from dedflow_amd.meshgen import fan_mesh, kuhn_cube, synthetic_fields

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from dedflow_amd import api as A
    A.lib()
    return A


def _close(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _dev(api, *arrs):
    return [api.DeviceArray.from_numpy(np.ascontiguousarray(a, np.float64)) for a in arrs]


MESHES = {"cube4": lambda: kuhn_cube(4, jitter=0.2), "cube12": lambda: kuhn_cube(12, jitter=0.2), "fan": lambda: fan_mesh()}


@pytest.mark.parametrize("schedule", [4, 1])
@pytest.mark.parametrize("name", list(MESHES))
def test_jacobian_matches_model(api, name, schedule):
    m = MESHES[name]()
    wg, dwg = synthetic_fields(m)
    P = api.Problem(m, schedule=schedule)
    wg_d, dwg_d = _dev(api, wg, dwg)
    vp, vt = P.assemble_scalar_jacobian(wg_d, dwg_d)
    rp, ci = P.pattern()
    Jp, Jt = sm.jacobians(m.xg, m.ien, wg)
    assert _close(vp, sm.on_pattern(Jp, rp, ci)) < 1e-12
    assert _close(vt, sm.on_pattern(Jt, rp, ci)) < 1e-12
    vp2, vt2 = P.assemble_scalar_jacobian(wg_d, dwg_d)
    assert np.array_equal(vp, vp2) and np.array_equal(vt, vt2)  # bitwise reproducible
    P.close()


def _oracle_scalar_rows(S, N, wgold, dwgold, dwg, held_phi=(), held_T=()):
    wga, dwga = sm.alpha_states(N, wgold, dwgold, dwg)
    F = np.zeros(6 * N)
    S.assemble_tet(wga, dwga, F)
    r = F[4 * N:].copy()
    for g in held_phi:
        r[S.bnodes(g)] = 0.0
    for g in held_T:
        r[N + S.bnodes(g)] = 0.0
    return r


@pytest.mark.parametrize("pc", ["jacobi", "amgx"])
@pytest.mark.parametrize("held_T", [(), (0, 1)])
def test_solve_drives_the_oracle_rows_to_zero(api, oracle_lib, pc, held_T):
    m = kuhn_cube(6, jitter=0.2)
    S = oracle_lib.System(m)
    N = S.N
    wgold, dwgold = synthetic_fields(m)
    dwg = 0.5 * dwgold
    r0 = _oracle_scalar_rows(S, N, wgold, dwgold, dwg, held_T=held_T)
    P = api.Problem(m)
    P.set_scalar_transport(pc=pc, dirichlet_T=held_T, rtol=1e-10)
    d = _dev(api, wgold, dwgold, dwg)
    rn, its = P.solve_scalar(*d)
    out = d[2].numpy()
    assert np.array_equal(out[:4 * N], dwg[:4 * N])  # only the scalar rates move
    # the device residual the solve started from is the oracle's, rows held zero
    assert abs(rn[0] - np.linalg.norm(r0[:N])) <= 1e-10 * np.linalg.norm(r0[:N])
    assert abs(rn[1] - np.linalg.norm(r0[N:])) <= 1e-10 * np.linalg.norm(r0[N:])
    r1 = _oracle_scalar_rows(S, N, wgold, dwgold, out, held_T=held_T)
    assert np.linalg.norm(r1[:N]) <= 1e-8 * np.linalg.norm(r0[:N]), its
    assert np.linalg.norm(r1[N:]) <= 1e-8 * np.linalg.norm(r0[N:]), its
    assert all(0 < k <= 200 for k in its)
    P.close()


@pytest.mark.parametrize("name", ["cube4", "fan"])
def test_uniform_advection_closed_form(api, name):
    m = MESHES[name]()
    N = m.num_node
    x = m.xg.reshape(-1, 3)
    wgold = np.zeros(6 * N)
    wgold[0:3 * N:3] = 1.0          # u = e_x
    wgold[4 * N:5 * N] = x[:, 0]    # phi = x
    dwgold = np.zeros(6 * N)
    dwg = np.zeros(6 * N)
    P = api.Problem(m)
    P.set_scalar_transport(phi=True, T=False)
    d = _dev(api, wgold, dwgold, dwg)
    P.solve_scalar(*d)
    dphi = d[2].numpy()[4 * N:5 * N]
    assert np.abs(dphi + 1.0 / sm.kALPHAM).max() < 1e-9
    assert np.all(d[2].numpy()[5 * N:] == 0.0)  # T is not advanced
    P.close()


def test_conservation_without_flow(api):
    m = kuhn_cube(5, jitter=0.2)
    N = m.num_node
    rng = np.random.default_rng(3)
    wgold = np.zeros(6 * N)
    wgold[5 * N:] = rng.uniform(0.0, 1.0, N)
    dwgold = np.zeros(6 * N)
    P = api.Problem(m)
    P.set_scalar_transport(phi=False, T=True)
    fac_pred = (sm.kGAMMA - 1.0) / sm.kGAMMA
    dwg = dwgold * fac_pred            # predictor
    d = _dev(api, wgold, dwgold, dwg)
    P.solve_scalar(*d)
    dwg = d[2].numpy()
    wnew = wgold + sm.kDT * (1.0 - sm.kGAMMA) * dwgold + sm.kDT * sm.kGAMMA * dwg   # corrector
    M = sm.mass_matrix(m.xg, m.ien)
    before, after = (M @ wgold[5 * N:]).sum(), (M @ wnew[5 * N:]).sum()
    assert abs(after - before) <= 1e-10 * abs(before)
    assert np.abs(wnew[5 * N:] - wgold[5 * N:]).max() > 1e-6   # diffusion moved T
    P.close()


def test_dirichlet_nodes_hold(api):
    m = kuhn_cube(6, jitter=0.2)
    N = m.num_node
    wgold, dwgold = synthetic_fields(m)
    wgold[5 * N:] = np.random.default_rng(4).uniform(-1.0, 1.0, N)
    dwg = 0.5 * dwgold
    P = api.Problem(m)
    for pc in ("jacobi", "amgx"):
        P.set_scalar_transport(dirichlet_T=(0, 1), dirichlet_phi=(2,), pc=pc)
        d = _dev(api, wgold, dwgold, dwg)
        P.solve_scalar(*d)
        out = d[2].numpy()
        held_T = np.unique(np.concatenate([m.bound_node[m.bound_node_offset[g]:m.bound_node_offset[g + 1]] for g in (0, 1)]))
        held_p = m.bound_node[m.bound_node_offset[2]:m.bound_node_offset[3]]
        assert np.array_equal(out[5 * N + held_T], dwg[5 * N + held_T])
        assert np.array_equal(out[4 * N + held_p], dwg[4 * N + held_p])
        assert np.array_equal(d[0].numpy(), wgold)
        free = np.setdiff1d(np.arange(N), held_T)
        assert np.abs(out[5 * N + free] - dwg[5 * N + free]).max() > 0.0
        res = P.scalar_residual()
        assert np.all(res[N + held_T] == 0.0) and np.all(res[held_p] == 0.0)
    P.close()


def _step(api, m, transport, newton_maxit):
    N = m.num_node
    wgold, dwgold = synthetic_fields(m)
    P = api.Problem(m)
    if transport:
        P.set_scalar_transport()
    d = _dev(api, wgold, dwgold, dwgold)
    F_d, dx_d = api.DeviceArray(6 * N), api.DeviceArray(6 * N)
    it, rn, r0 = P.time_step(d[0], d[1], d[2], F_d, dx_d, newton_maxit=newton_maxit)
    out = [a.numpy() for a in d]
    P.close()
    return it, rn, r0, out, wgold


def test_coupled_time_step(api):
    m = kuhn_cube(8)
    N = m.num_node
    it, rn, r0, (w, dwo, dw), wgold = _step(api, m, True, 4)
    assert 0 < it <= 4
    assert np.all(r0[2:] > 0.0)
    assert np.all(rn[2:] <= 5e-4 * r0[2:]), (rn, r0)
    assert np.abs(w[4 * N:5 * N] - wgold[4 * N:5 * N]).max() > 1e-6
    assert np.abs(w[5 * N:] - wgold[5 * N:]).max() > 1e-6
    # one Newton iteration each: phi / T feed nothing into the (u, p) rows
    _, _, _, (w1, _, dw1), _ = _step(api, m, True, 1)
    _, _, _, (w0, _, dw0), _ = _step(api, m, False, 1)
    assert np.array_equal(w1[:4 * N], w0[:4 * N]) and np.array_equal(dw1[:4 * N], dw0[:4 * N])
    assert not np.array_equal(w1[4 * N:], w0[4 * N:])


def test_cleared_transport_is_the_off_path(api):
    m = kuhn_cube(6, jitter=0.2)
    N = m.num_node
    wgold, dwgold = synthetic_fields(m)
    res = []
    for touched in (False, True):
        P = api.Problem(m)
        if touched:
            P.set_scalar_transport(dirichlet_T=(0,))
            d = _dev(api, wgold, dwgold, dwgold)
            P.solve_scalar(*d)   # builds every piece of the state
            P.clear_scalar_transport()
            assert P.scalar_residual() is None
        d = _dev(api, wgold, dwgold, dwgold)
        F_d, dx_d = api.DeviceArray(6 * N), api.DeviceArray(6 * N)
        it, rn, r0 = P.solve_flow_system(d[0], d[1], d[2], F_d, dx_d)
        res.append((it, rn, r0, F_d.numpy(), d[2].numpy(), dx_d.numpy()))
        P.close()
    a, b = res
    assert a[0] == b[0]
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x, y)
    assert np.all(a[1][2:] == 0.0)  # off: the phi / T norms stay zero as in the reference
