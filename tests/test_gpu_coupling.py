"""GPU tests of the particle-fluid coupling (host/couple.c, csrc/k_couple.hip): point location, interpolation, the
implicit drag update, the reaction load and its registration on the residual, and the coupled DflTimeStep.  Build-defined
(the reference has no coupling physics): correctness is pinned to tests/coupling_model.py and to closed-form physics."""
import ctypes as C

import numpy as np
import pytest

import coupling_model as cm
from dedflow_amd.meshgen import fan_mesh, kuhn_cube, synthetic_fields

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from dedflow_amd import api as A
    A.lib()
    return A


def _inside(m, n, seed):
    rng = np.random.default_rng(seed)
    t = rng.integers(0, m.num_tet, n)
    lam = rng.dirichlet(np.ones(4), n)
    return np.einsum("na,nad->nd", lam, m.xg.reshape(-1, 3)[m.ien.reshape(-1, 4)[t]])


def _lattice(k, lo, hi, jitter=0.0, seed=1):
    g = np.linspace(lo, hi, k)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    return p + np.random.default_rng(seed).uniform(-jitter, jitter, p.shape)


def _mass(R, rho_p):
    return rho_p * 4.0 / 3.0 * np.pi * R ** 3


def _set_coord(api, pc, x):
    api.DeviceArray(3 * pc.P, ptr=pc.ctx.contents.d_arr[0].contents.data).upload(np.ascontiguousarray(x).reshape(-1))


def _state(u, N):
    w = np.zeros(6 * N)
    w[: 3 * N] = np.asarray(u).reshape(-1)
    return w


def _pool(L):
    r, u = C.c_int64(0), C.c_int64(0)
    L.DflDevicePoolStats(C.byref(r), C.byref(u))
    return r.value, u.value


def _location_points(m, cube):
    ien4, x = m.ien.reshape(-1, 4), m.xg.reshape(-1, 3)
    rng = np.random.default_rng(21)
    inside = _inside(m, 600, 22)
    if cube:
        out = rng.uniform(-0.5, 1.5, size=(400, 3))
        out = out[np.any((out < 0.0) | (out > 1.0), axis=1)][:150]
    else:
        d = rng.normal(size=(150, 3))
        out = d / np.linalg.norm(d, axis=1)[:, None] * rng.uniform(1.05, 1.5, size=(150, 1))
    t = rng.integers(0, m.num_tet, 150)
    verts = x[ien4[t, 0]]
    edges = 0.5 * (x[ien4[t, 1]] + x[ien4[t, 2]])
    faces = (x[ien4[t, 0]] + x[ien4[t, 2]] + x[ien4[t, 3]]) / 3.0
    return inside, out, np.vstack([verts, edges, faces])


@pytest.mark.parametrize("which", ["cube4", "cube12_jitter", "fan"])
def test_locate_matches_the_model(api, which):
    m = {"cube4": lambda: kuhn_cube(4), "cube12_jitter": lambda: kuhn_cube(12, jitter=0.2), "fan": fan_mesh}[which]()
    inside, out, shared = _location_points(m, which != "fan")
    pts = np.vstack([inside, out, shared])
    n_in, n_out = len(inside), len(out)
    P = api.Problem(m)
    pc = api.Particles(pts.reshape(-1), np.zeros(pts.size), 1e-4)
    try:
        pc.couple(P)
        pc.locate()
        api.sync()
        tet, lam = pc.tet(), pc.barycentric()
        assert pc.lost_count() == 0
        brute = cm.locate_brute(m.xg, m.ien, pts)
        located = np.r_[np.arange(n_in), np.arange(n_in + n_out, len(pts))]
        assert (brute[located] >= 0).all() and (brute[n_in:n_in + n_out] == -1).all()
        assert (tet[located] >= 0).all()
        assert cm.contains(m.xg, m.ien, tet[located], pts[located]).all()
        assert np.abs(lam[located] - cm.barycentric(m.xg, m.ien, tet[located], pts[located])).max() <= 1e-13
        assert (tet[n_in:n_in + n_out] == -1).all()
        # walk from history: small moves, then location from the previous tets against a fresh location
        rng = np.random.default_rng(23)
        moved = inside + rng.normal(scale=0.02 if which != "fan" else 0.05, size=inside.shape)
        moved = np.vstack([moved, out, shared])
        _set_coord(api, pc, moved)
        pc.locate()
        fresh = api.Particles(moved.reshape(-1), np.zeros(moved.size), 1e-4)
        try:
            fresh.couple(P)
            fresh.locate()
            api.sync()
            th, tf = pc.tet(), fresh.tet()
            assert pc.lost_count() == 0 and fresh.lost_count() == 0
            assert np.array_equal(th >= 0, tf >= 0)
            assert np.array_equal(th >= 0, cm.locate_brute(m.xg, m.ien, moved) >= 0)
            ok = th >= 0
            assert cm.contains(m.xg, m.ien, th[ok], moved[ok]).all() and cm.contains(m.xg, m.ien, tf[ok], moved[ok]).all()
        finally:
            fresh.close()
    finally:
        pc.close()
        P.close()


def test_interpolation_reproduces_an_affine_field(api):
    """u = a + B x at the nodes; with dt * f / tau ~ 1e15 one sub-step lands v' on u_f to 1e-15 relative"""
    m = kuhn_cube(6, jitter=0.2)
    N = m.num_node
    rng = np.random.default_rng(31)
    a, B = rng.normal(size=3), rng.normal(size=(3, 3))
    w = _state(a[None, :] + m.xg.reshape(-1, 3) @ B.T, N)
    pts = _lattice(7, 0.05, 0.95, jitter=0.02)
    R = 1e-4
    P = api.Problem(m)
    pc = api.Particles(pts.reshape(-1), np.zeros(pts.size), R, mass=_mass(R, 1000.0), dt=1e10)
    try:
        pc.couple(P)
        w_d = api.DeviceArray.from_numpy(w)
        pc.fluid_step(w_d)
        api.sync()
        _, v, _ = pc.arrays()
        exact = a[None, :] + pts @ B.T
        assert np.abs(v.reshape(-1, 3) - exact).max() <= 1e-13 * np.abs(exact).max()
    finally:
        pc.close()
        P.close()


def _drag_setup(api, m, R=0.005, rho_p=2000.0, dt=2e-4, gravity=(0.0, 0.0, 0.0), two_way=False, k=6, seed=41):
    pts = _lattice(k, 0.25, 0.75, jitter=0.01, seed=seed)
    v0 = np.random.default_rng(seed + 1).normal(scale=0.1, size=pts.shape)
    P = api.Problem(m)
    pc = api.Particles(pts.reshape(-1), v0.reshape(-1), R, mass=_mass(R, rho_p), dt=dt)
    pc.couple(P, gravity=gravity, two_way=two_way)
    return P, pc, pts, v0


def test_drag_matches_the_model_and_is_stable_for_large_steps(api):
    m = kuhn_cube(6, jitter=0.2)
    N = m.num_node
    U = np.array([0.3, -0.2, 0.1])
    R, dt = 0.005, 2e-4
    P, pc, x, v = _drag_setup(api, m, R=R, dt=dt)
    mass = _mass(R, 2000.0)
    try:
        w_d = api.DeviceArray.from_numpy(_state(np.tile(U, (N, 1)), N))
        for _ in range(20):
            pc.fluid_step(w_d)
            x, v, _, _ = cm.drag_step(x, v, np.zeros_like(x), np.tile(U, (len(x), 1)), np.ones(len(x), bool), mass, R, dt)
        api.sync()
        xd, vd, _ = pc.arrays()
        assert pc.lost_count() == 0 and (pc.tet() >= 0).all()
        assert np.abs(vd.reshape(-1, 3) - v).max() <= 1e-12 * np.abs(v).max()
        assert np.abs(xd.reshape(-1, 3) - x).max() <= 1e-12 * np.abs(x).max()
    finally:
        pc.close()
        P.close()
    # dt >> tau: bounded, and v' lands on u_f
    tau = cm.response_time(mass, R)
    P, pc, x, v = _drag_setup(api, m, R=R, dt=1e6 * tau)
    try:
        pc.fluid_step(api.DeviceArray.from_numpy(_state(np.tile(U, (N, 1)), N)))
        api.sync()
        vd = pc.arrays()[1].reshape(-1, 3)
        assert np.all(np.isfinite(vd))
        assert np.abs(vd - U[None, :]).max() <= 1e-5 * np.abs(U).max()
    finally:
        pc.close()
        P.close()


def test_settling_reaches_the_terminal_velocity(api):
    m = kuhn_cube(6, jitter=0.2)
    N = m.num_node
    R, rho_p = 0.005, 2000.0
    mass = _mass(R, rho_p)
    g = (0.0, 0.0, -9.81)
    tau = cm.response_time(mass, R)
    P, pc, _, _ = _drag_setup(api, m, R=R, rho_p=rho_p, dt=tau, gravity=g, k=3)
    try:
        w_d = api.DeviceArray(6 * N)
        for _ in range(80):
            pc.fluid_step(w_d)
        api.sync()
        vt = cm.terminal_velocity(mass, R, g)
        assert cm.RHO_F * np.linalg.norm(vt) * 2 * R / cm.MU_F < 1.0      # small Re
        assert (pc.tet() >= 0).all()
        v = pc.arrays()[1].reshape(-1, 3)
        assert np.abs(v - vt[None, :]).max() <= 1e-10 * np.abs(vt).max()
    finally:
        pc.close()
        P.close()


def _reaction_run(api, m, w, K, R, dt):
    P, pc, x, v = _drag_setup(api, m, R=R, dt=dt, seed=51)
    try:
        w_d = api.DeviceArray.from_numpy(w)
        for _ in range(K):
            pc.fluid_step(w_d)
        tet, lam = pc.tet(), pc.barycentric()
        load = pc.reaction_load().numpy()
        api.sync()
        vK = pc.arrays()[1].reshape(-1, 3)
        return load, tet, lam, x, v, vK
    finally:
        pc.close()
        P.close()


def test_reaction_load(api):
    m = kuhn_cube(6, jitter=0.2)
    N = m.num_node
    wg, _ = synthetic_fields(m)
    K, R, dt = 5, 0.005, 2e-4
    mass = _mass(R, 2000.0)
    load, tet, lam, x, v, vK = _reaction_run(api, m, wg, K, R, dt)
    v0 = v.copy()
    # the model: brute-force location, drag, impulses, scatter with the last lambda
    imp = np.zeros_like(x)
    for _ in range(K):
        t = cm.locate_brute(m.xg, m.ien, x)
        lm = cm.barycentric(m.xg, m.ien, t, x)
        x, v, _, di = cm.drag_step(x, v, np.zeros_like(x), cm.interpolate(wg, m.ien, t, lm), t >= 0, mass, R, dt)
        imp += di
    assert np.array_equal(t, tet)
    ref = cm.node_scatter(N, m.ien, t, lm, imp, K * dt)
    assert np.abs(load - ref).max() <= 1e-13 * np.abs(ref).max()
    # momentum: sum_a load = -sum_p impulse / dt (no contacts, no gravity: the impulse is the particles' momentum change)
    total = -mass * (vK - v0).sum(axis=0) / (K * dt)
    assert np.abs(load.reshape(-1, 3).sum(axis=0) - total).max() <= 1e-12 * np.abs(total).max()
    # bitwise reproducible
    load2 = _reaction_run(api, m, wg, K, R, dt)[0]
    assert np.array_equal(load, load2)
    # registered on the mesh: F(with) - F(without) = -load on the free momentum rows, 0 on the Dirichlet rows
    P = api.Problem(m)
    try:
        wg_d, dwg_d = api.DeviceArray.from_numpy(wg), api.DeviceArray.from_numpy(0.1 * synthetic_fields(m)[1])
        F0, F1 = api.DeviceArray(6 * N), api.DeviceArray(6 * N)
        P.assemble_system(wg_d, dwg_d, F0)
        P.set_external_load(api.DeviceArray.from_numpy(load))
        P.assemble_system(wg_d, dwg_d, F1)
        P.set_external_load(None)
        F2 = api.DeviceArray(6 * N)
        P.assemble_system(wg_d, dwg_d, F2)
        api.sync()
        f0, f1, f2 = F0.numpy(), F1.numpy(), F2.numpy()
        assert np.array_equal(f0, f2)
        dirichlet = np.zeros(3 * N, bool)
        for group, bctype in api.REFERENCE_BCS:
            nodes = m.bound_node[m.bound_node_offset[group]:m.bound_node_offset[group + 1]]
            for c, t in enumerate(bctype):
                if t == api.BC_STRONG:
                    dirichlet[3 * nodes + c] = True
        diff = f1[:3 * N] - f0[:3 * N]
        assert np.array_equal(diff[dirichlet], np.zeros(dirichlet.sum()))
        free = ~dirichlet
        assert np.abs(load[free]).max() > 0.0
        assert np.abs(diff[free] + load[free]).max() <= 1e-12 * max(np.abs(f0).max(), np.abs(load).max())
        assert np.array_equal(f1[3 * N:], f0[3 * N:])
    finally:
        P.close()


def _time_steps(api, m, wg, dwg, pts, v, R, steps, substeps=10, dt=1e-3, couple=True, two_way=True, clear=False, maxit=2):
    N = m.num_node
    L = api.lib()
    P = api.Problem(m, maxit=120, atol=1e-12, rtol=1e-4)
    pc = api.Particles(pts.reshape(-1), v.reshape(-1), R, mass=_mass(R, 2000.0), dt=dt)
    out = {"slip": [], "pool": [], "its": []}
    try:
        if couple:
            pc.couple(P, two_way=two_way)
        if clear:
            pc.locate()
            pc.couple(None)
        st = [api.DeviceArray.from_numpy(a) for a in (wg, dwg, dwg)]
        F_d, dx_d = api.DeviceArray(6 * N), api.DeviceArray(6 * N)
        for _ in range(steps):
            it, rn, ri = P.time_step(st[0], st[1], st[2], F_d, dx_d, newton_maxit=maxit, particles=pc, dem_substeps=substeps)
            api.sync()
            out["its"].append(it)
            out["pool"].append(_pool(L))
            if couple and not clear:
                w = st[0].numpy()
                tet, lam = pc.tet(), pc.barycentric()
                assert (tet >= 0).all()
                uf = cm.interpolate(w, m.ien, tet, lam)
                out["slip"].append(np.linalg.norm(uf - pc.arrays()[1].reshape(-1, 3), axis=1).mean())
        stats = L.KrylovGetStats(P.ksp).contents
        out["solves"], out["converged"] = int(stats.total_solves), int(stats.total_converged)
        out["w"] = st[0].numpy()
        out["particles"] = pc.arrays()
        out["lost"] = pc.lost_count()
        return out
    finally:
        pc.close()
        P.close()


def test_two_way_coupling_pushes_the_fluid_along(api):
    """fluid at rest, a cloud moving in +x: with two_way the fluid over the cloud gains +x velocity (relative to the
    one-way run, whose fluid feels nothing) and the particles slow down"""
    m = kuhn_cube(8, jitter=0.2)
    N = m.num_node
    wg, _ = synthetic_fields(m)
    wg[:4 * N] = 0.0                                    # u = 0, p = 0; phi, T as in synthetic_fields
    dwg = np.zeros(6 * N)
    pts = _lattice(5, 0.4, 0.6)
    v = np.tile([1.0, 0.0, 0.0], (len(pts), 1))
    R = 0.01
    two = _time_steps(api, m, wg, dwg, pts, v, R, steps=2, two_way=True)
    one = _time_steps(api, m, wg, dwg, pts, v, R, steps=2, two_way=False)
    # the nodes of the tets the cloud occupies
    t = cm.locate_brute(m.xg, m.ien, two["particles"][0].reshape(-1, 3))
    nodes = np.unique(m.ien.reshape(-1, 4)[t[t >= 0]])
    ux_two, ux_one = two["w"][3 * nodes].mean(), one["w"][3 * nodes].mean()
    assert ux_two > 0.0 and ux_two > ux_one + 1e-6, (ux_two, ux_one)
    assert two["particles"][1].reshape(-1, 3)[:, 0].mean() < 1.0
    assert two["converged"] == two["solves"]


def test_coupled_time_step(api):
    """M=12, synthetic flow, particles at rest: every Newton solve converges, the particles' mean slip falls step over step,
    the device pool stays flat, two runs are bitwise equal"""
    m = kuhn_cube(12, jitter=0.2)
    N = m.num_node
    wg, dw0 = synthetic_fields(m)
    wg[3 * N:4 * N] = 0.0
    pts = _lattice(4, 0.3, 0.7, jitter=0.01)
    v = np.zeros_like(pts)
    R = 0.01
    a = _time_steps(api, m, wg, 0.1 * dw0, pts, v, R, steps=3)
    assert a["solves"] == a["converged"] == sum(a["its"])
    assert a["lost"] == 0
    assert a["slip"][0] > a["slip"][1] > a["slip"][2], a["slip"]
    assert a["pool"][0] == a["pool"][-1]
    b = _time_steps(api, m, wg, 0.1 * dw0, pts, v, R, steps=3)
    assert np.array_equal(a["w"], b["w"])
    for x, y in zip(a["particles"], b["particles"]):
        assert np.array_equal(x, y)


def test_coupling_off_means_off(api):
    m = kuhn_cube(6, jitter=0.2)
    N = m.num_node
    wg, dw0 = synthetic_fields(m)
    wg[3 * N:4 * N] = 0.0
    pts = _lattice(4, 0.3, 0.7, jitter=0.01)
    v = np.random.default_rng(61).normal(scale=0.1, size=pts.shape)
    cleared = _time_steps(api, m, wg, 0.1 * dw0, pts, v, 0.01, steps=2, substeps=3, clear=True)
    never = _time_steps(api, m, wg, 0.1 * dw0, pts, v, 0.01, steps=2, substeps=3, couple=False)
    assert np.array_equal(cleared["w"], never["w"])
    for x, y in zip(cleared["particles"], never["particles"]):
        assert np.array_equal(x, y)
    assert np.abs(never["particles"][0] - pts.reshape(-1)).max() > 0.0
