"""GPU tests of the particle heat transfer (host/heat.c, csrc/k_heat.hip; model in include/dedflow.h "particle heat
transfer").  Build-defined: every comparison is against tests/heat_model.py (np.longdouble) or a closed form, except where
bit-identity between two library paths is the claim.

Bounds.  Interpolation, convection and the per-particle part of the source are a handful of fp64 operations per output:
1e-13 relative to the array's max magnitude, the coupling tests' bound.  Device sqrt is correctly rounded and Pr^(1/3) is
evaluated once on the host, so no allowance for pow is needed (the logged ratios show it).  Sums over contacts or particles
get the a-priori bound (n_terms + c) eps sum|terms|; a conduction term adds the conditioning of its overlap
delta = (r_i + r_j) - dist, which cancels: eps |term| (r_i + r_j + dist) / delta (the distance is one rounding away from
the model's).  The conduction rate q_i is read directly (a library-private accessor) and held to that bound; the heat
rate read back after the step is a second check and adds the rounding of T' - T, 4 eps C max|T| / dt.  With DFL_HEAT_PARITY_LOG set, every comparison appends observed error and bound to that
file (profiles/heat_parity.jsonl is such a log)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import heat_model as hm
import ref_driver as rd
import scalar_model as sm
from dedflow_amd.meshgen import kuhn_box, kuhn_cube

pytestmark = pytest.mark.gpu
EPS = hm.EPS
RHO_F, MU_F = 1.0e3, 1.0e-2      # Re = 1e5 |u_f - v| d


@pytest.fixture(scope="module")
def api():
    from dedflow_amd import api as A
    A.lib()
    return A


def _log(name, err, bound):
    err, bound = float(err), float(bound)
    path = os.environ.get("DFL_HEAT_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"check": name, "error": err, "bound": bound, "ratio": err / bound if bound > 0 else None}) + "\n")
    print(f"heat parity {name}: error {err:.3e} bound {bound:.3e}")
    return err, bound


def _check(name, got, ref, bound):
    """max |got - ref| against a scalar bound, or the worst ratio to a per-entry bound"""
    d = np.abs(np.asarray(got, np.longdouble) - np.asarray(ref, np.longdouble))
    if np.ndim(bound) == 0:
        err, b = _log(name, d.max(), bound)
    else:
        k = int(np.argmax(d / np.maximum(bound, 1e-300)))
        err, b = _log(name, d[k], np.asarray(bound)[k])
    assert err <= b, (name, err, b)


def _mass(r, rho_p=2000.0):
    return rho_p * 4.0 / 3.0 * np.pi * np.asarray(r) ** 3


def _pool(L):
    r, u = C.c_int64(0), C.c_int64(0)
    L.DflDevicePoolStats(C.byref(r), C.byref(u))
    return r.value, u.value


def _inside(m, n, seed):
    rng = np.random.default_rng(seed)
    t = rng.integers(0, m.num_tet, n)
    lam = rng.dirichlet(np.ones(4), n)
    return np.einsum("na,nad->nd", lam, m.xg.reshape(-1, 3)[m.ien.reshape(-1, 4)[t]])


def test_interpolation_reproduces_an_affine_field(api):
    """nodal T = a + b.x, dt / tau_T ~ 1e15: one heat step lands T_i' on a + b.x_i"""
    m = kuhn_cube(6, jitter=0.2)
    N = m.num_node
    rng = np.random.default_rng(31)
    a, b = rng.normal(), rng.normal(size=3)
    w = np.zeros(6 * N)
    w[5 * N:] = a + m.xg.reshape(-1, 3) @ b
    g = np.linspace(0.05, 0.95, 7)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) + rng.uniform(-0.02, 0.02, (343, 3))
    R = 1e-4
    P = api.Problem(m)
    pc = api.Particles(pts.reshape(-1), np.zeros(pts.size), R, mass=float(_mass(R, 1000.0)), dt=1e10)
    try:
        pc.couple(P)
        pc.set_heat(cp_p=1.0, T_init=5.0)
        tau = hm.tau_T(_mass(R, 1000.0), 2.0, hm.K_F, 2 * R)
        assert 1e14 < 1e10 / tau < 1e17
        pc.heat_step(api.DeviceArray.from_numpy(w))
        api.sync()
        assert (pc.tet() >= 0).all()
        exact = a + pts @ b
        _check("interpolation", pc.temperature(), exact, 1e-13 * np.abs(exact).max())
    finally:
        pc.close()
        P.close()


def _convection_case(api, poly, seed=41):
    m = kuhn_cube(6, jitter=0.2)
    N = m.num_node
    rng = np.random.default_rng(seed)
    xn = m.xg.reshape(-1, 3)
    w = np.zeros(6 * N)
    u = rng.normal(scale=0.5, size=(N, 3))
    u[xn[:, 0] < 0.45] = 0.0                      # a region of fluid at rest: Re = 0 exactly for particles at rest in it
    w[:3 * N] = u.reshape(-1)
    w[5 * N:] = rng.uniform(300.0, 1500.0, N)
    inside = _inside(m, 900, seed + 1)
    outside = rng.uniform(1.05, 1.4, size=(60, 3))
    pts = np.vstack([inside, outside])
    v = rng.normal(size=pts.shape) * rng.uniform(0.0, 1.5, size=(len(pts), 1))
    v[pts[:, 0] < 0.2] = 0.0
    R = 0.005
    r = rng.uniform(0.5 * R, R, len(pts)) if poly else np.full(len(pts), R)
    mass = _mass(r)
    T0 = rng.uniform(300.0, 1500.0, len(pts))
    cp_p, dt = 1.0, 0.01
    P = api.Problem(m)
    pc = api.Particles(pts.reshape(-1), v.reshape(-1), R, mass=float(_mass(R)), dt=dt)
    try:
        if poly:
            pc.set_sizes(r, mass)
        pc.couple(P, rho_f=RHO_F, mu_f=MU_F)
        pc.set_heat(cp_p=cp_p, T_init=0.0)
        pc.set_temperature(T0)
        before = pc.arrays()
        pc.heat_step(api.DeviceArray.from_numpy(w))
        api.sync()
        out = dict(T=pc.temperature(), rate=pc.heat_rate(), e=pc._pending_energy(), tet=pc.tet(), lam=pc.barycentric(),
                   after=pc.arrays(), before=before)
    finally:
        pc.close()
        P.close()
    Tf, re, nu, tau, located = hm.convection(w, N, m.ien, out["tet"], out["lam"], v, mass, r, cp_p, dt, RHO_F, MU_F)
    out.update(model=hm.update(T0, None, mass * cp_p, dt, Tf=Tf, tau=tau, located=located), re=re, located=located, T0=T0,
               dt_over_tau=dt / tau)
    return out


@pytest.mark.parametrize("poly", [False, True], ids=["mono", "poly"])
def test_convection_matches_the_model(api, poly):
    o = _convection_case(api, poly)
    loc = o["located"]
    assert loc.sum() >= 850 and (~loc).sum() == 60
    re = o["re"][loc]
    assert re.min() == 0.0 and re.max() > 1.0e3 and (re > 0).sum() > 500
    assert 0.05 < float(o["dt_over_tau"][loc].min()) and float(o["dt_over_tau"][loc].max()) < 50.0
    Tn, rate, e = o["model"]
    tag = "poly" if poly else "mono"
    _check(f"convection_T_{tag}", o["T"], Tn, 1e-13 * np.abs(Tn).max())
    _check(f"convection_rate_{tag}", o["rate"], rate, 1e-13 * float(np.abs(rate).max()))
    _check(f"convection_energy_{tag}", o["e"], e, 1e-13 * float(np.abs(e).max()))
    assert np.array_equal(o["T"][~loc], o["T0"][~loc])            # outside the mesh: exactly unchanged
    assert np.all(o["rate"][~loc] == 0.0) and np.all(o["e"][~loc] == 0.0)
    for x, y in zip(o["before"], o["after"]):                      # the heat step moves nothing
        assert np.array_equal(x, y)
    again = _convection_case(api, poly)
    for k in ("T", "rate", "e"):
        assert np.array_equal(o[k], again[k])


R_L = 0.04


def _conduction_lattice():
    rng = np.random.default_rng(7)
    g = 0.06 + 1.9 * R_L * np.arange(12)
    x = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) + rng.uniform(-0.05 * R_L, 0.05 * R_L, (1728, 3))
    r = rng.uniform(0.9 * R_L, R_L, 1728)
    T = rng.uniform(300.0, 1500.0, 1728)
    return x, r, T


K_P, CP_P, RHO_P = 40.0, 500.0, 7800.0     # steel-like


def _conduction_run(api, x, r, T, dt, wall_mesh=None, path="bare"):
    pc = api.Particles(x.reshape(-1), np.zeros(x.size), R_L, mass=float(_mass(R_L, RHO_P)), dt=dt)
    P = api.Problem(wall_mesh) if wall_mesh is not None else None
    try:
        pc.set_sizes(r, _mass(r, RHO_P))
        if P is not None:
            pc.set_walls(P)
        pc.set_heat(cp_p=CP_P, k_p=K_P, T_init=0.0)
        pc.set_temperature(T)
        if path == "bare":
            pc.heat_step()
        else:
            pc.update()
        api.sync()
        return pc.heat_rate(), pc.temperature(), pc._conduction_rate()
    finally:
        pc.close()
        if P is not None:
            P.close()


def test_conduction_matches_the_all_pairs_model(api):
    """a 12^3 lattice of spacing 1.9 R, jitter 0.05 R, radii in [0.9 R, R].  The box grid and a mesh-wall grid that bins the
    particles alike (walls at [R, 1 - R]^3: its padded box is the unit box) give bit-identical q; a wall mesh whose grid
    bins differently visits a particle's partners in another order, so its q agrees to the bound of the sum instead."""
    x, r, T = _conduction_lattice()
    Cp = _mass(r, RHO_P) * CP_P
    q, qa, cnt, hs, qc = hm.conduction(x, r, T, K_P)
    assert cnt.sum() // 2 >= 2000 and cnt.max() == 6 and (cnt == 0).sum() > 0
    dt = 0.5 / float((hs / Cp).max())            # the explicit stability condition with a margin of 2
    rate, Tn, qd = _conduction_run(api, x, r, T, dt)
    qbound = (cnt + 4) * EPS * qa.astype(float) + EPS * qc          # the sum's bound and the overlap's conditioning
    _check("conduction_q_box", qd, q, qbound + 1e-300)
    assert np.all(qd[cnt == 0] == 0.0)
    # sum_i q_i: every pair's two terms are exact negations, so what is left is the rounding of the per-particle sums
    err, b = _log("conduction_sum_q", abs(float(qd.astype(np.longdouble).sum())), float((cnt * EPS * qa.astype(float)).sum()))
    assert err <= b
    bound = qbound + 4 * EPS * Cp * np.maximum(np.abs(T), np.abs(Tn)) / dt   # + the round trip through T' - T
    _check("conduction_rate_box", rate, q, bound)
    assert np.all(rate[cnt == 0] == 0.0) and np.array_equal(Tn[cnt == 0], T[cnt == 0])
    Tm = hm.update(T, q, Cp, dt)[0]
    _check("conduction_T", Tn, Tm, bound * dt / Cp + 4 * EPS * np.abs(T))
    same_bins = kuhn_box(4, (R_L,) * 3, (1.0 - R_L,) * 3)
    rate_w, Tn_w, qd_w = _conduction_run(api, x, r, T, dt, wall_mesh=same_bins)
    assert np.array_equal(qd_w, qd) and np.array_equal(rate_w, rate) and np.array_equal(Tn_w, Tn)
    _, _, qd_o = _conduction_run(api, x, r, T, dt, wall_mesh=kuhn_cube(4))
    _check("conduction_q_other_grid", qd_o, q, qbound + 1e-300)
    rate_u, Tn_u, qd_u = _conduction_run(api, x, r, T, dt, path="update")     # ParticleContextUpdate: the sweep's contacts
    assert np.array_equal(qd_u, qd) and np.array_equal(rate_u, rate) and np.array_equal(Tn_u, Tn)
    rate2, Tn2, qd2 = _conduction_run(api, x, r, T, dt)
    assert np.array_equal(qd2, qd) and np.array_equal(rate2, rate) and np.array_equal(Tn2, Tn)


@pytest.mark.parametrize("change", ["sizes", "walls_on", "walls_off"])
def test_bare_heat_step_resorts_after_sizes_or_walls_change(api, change):
    """a sweep, then set_sizes / set_walls, then a bare heat step: the sweep's cell list and sorted copies are no longer
    those of the context, so the heat step sorts again and gives what a fresh context gives, bit for bit"""
    x, r, T = _conduction_lattice()
    dt = 1.0
    mesh = kuhn_cube(4)

    def run(stale):
        pc = api.Particles(x.reshape(-1), np.zeros(x.size), R_L, mass=float(_mass(R_L, RHO_P)), kn=0.0, gamma_n=0.0, dt=dt)
        P = api.Problem(mesh) if change != "sizes" else None
        try:
            if change != "sizes":
                pc.set_sizes(r, _mass(r, RHO_P))
            if change == "walls_off":
                pc.set_walls(P)
            if stale:
                pc.compute_forces()             # the sweep of the state before the change
            if change == "sizes":
                pc.set_sizes(r, _mass(r, RHO_P))
            elif change == "walls_on":
                pc.set_walls(P)
            else:
                pc.set_walls(None)
            pc.set_heat(cp_p=CP_P, k_p=K_P, T_init=0.0)
            pc.set_temperature(T)
            pc.heat_step()
            api.sync()
            return pc._conduction_rate(), pc.temperature()
        finally:
            pc.close()
            if P is not None:
                P.close()

    q_stale, T_stale = run(True)
    q_fresh, T_fresh = run(False)
    q, qa, cnt, _, qc = hm.conduction(x, r, T, K_P)
    _check(f"conduction_q_after_{change}", q_fresh, q, (cnt + 4) * EPS * qa.astype(float) + EPS * qc + 1e-300)
    assert np.abs(q_fresh).max() > 0.0
    assert np.array_equal(q_stale, q_fresh) and np.array_equal(T_stale, T_fresh)


def _source_case(api, remove=False, K=4, seed=61):
    m = kuhn_cube(6, jitter=0.2)
    N = m.num_node
    rng = np.random.default_rng(seed)
    w = np.zeros(6 * N)
    w[:3 * N] = rng.normal(scale=0.05, size=3 * N)
    w[5 * N:] = rng.uniform(300.0, 1500.0, N)
    g = np.linspace(0.1, 0.9, 9)               # a jittered lattice: no contacts, every particle stays inside
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) + rng.uniform(-0.02, 0.02, (729, 3))
    v = rng.normal(scale=0.05, size=pts.shape)
    R, dt, cp_p = 0.005, 0.01, 1.0
    P = api.Problem(m)
    pc = api.Particles(pts.reshape(-1), v.reshape(-1), R, mass=float(_mass(R)), dt=dt)
    try:
        pc.couple(P, rho_f=RHO_F, mu_f=MU_F)
        pc.set_heat(cp_p=cp_p, T_init=900.0)
        w_d = api.DeviceArray.from_numpy(w)
        zero = pc.heat_source().numpy()                      # no sub-step ran
        for _ in range(K):
            pc.fluid_step(w_d)
        api.sync()
        e, tet, lam = pc._pending_energy(), pc.tet(), pc.barycentric()
        if remove:
            pc.set_outflow(planes=[(1.0, 0.0, 0.0, 0.5)])
            pc.remove()
            assert 0 < pc.P < 729
        q = pc.heat_source().numpy()
        second = pc.heat_source().numpy()
        api.sync()
        return dict(N=N, ien=m.ien, zero=zero, e=e, tet=tet, lam=lam, q=q, second=second, time=K * dt, P=pc.P)
    finally:
        pc.close()
        P.close()


def test_heat_source(api):
    o = _source_case(api)
    assert np.all(o["zero"] == 0.0) and np.all(o["second"] == 0.0)
    assert (o["tet"] >= 0).all() and np.abs(o["e"]).min() > 0.0
    ref, refa, cnt = hm.node_scatter(o["N"], o["ien"], o["tet"], o["lam"], o["e"], o["time"])
    _check("source_q", o["q"], ref, (cnt + 4) * EPS * refa.astype(float) + 1e-300)
    esum = o["e"].astype(np.longdouble).sum()
    total = (o["q"].astype(np.longdouble) * o["time"]).sum()
    err, b = _log("source_total", abs(float(total + esum)), (4 * len(o["e"]) + 8) * EPS * float(np.abs(o["e"]).sum()))
    assert err <= b
    again = _source_case(api)
    assert np.array_equal(o["q"], again["q"]) and np.array_equal(o["e"], again["e"])
    # ParticleContextRemove between the sub-steps and the call: the removed particles' energy is kept
    r = _source_case(api, remove=True)
    assert np.array_equal(r["e"], o["e"])
    total_r = (r["q"].astype(np.longdouble) * r["time"]).sum()
    err, b = _log("source_total_after_remove", abs(float(total_r + esum)),
                  (4 * len(o["e"]) + 16) * EPS * float(np.abs(o["e"]).sum()))
    assert err <= b
    _check("source_q_after_remove", r["q"], ref, (cnt + 8) * EPS * refa.astype(float) + 1e-300)


def test_heat_source_enters_the_T_rows(api):
    from dedflow_amd.meshgen import synthetic_fields
    m = kuhn_cube(6, jitter=0.2)
    N = m.num_node
    wg, dwg = synthetic_fields(m)
    q = np.random.default_rng(71).normal(scale=np.abs(wg[5 * N:]).max(), size=N)
    P = api.Problem(m)
    try:
        P.set_scalar_transport(dirichlet_T=(0, 1))
        held = np.unique(np.concatenate([m.bound_node[m.bound_node_offset[g]:m.bound_node_offset[g + 1]] for g in (0, 1)]))
        free = np.setdiff1d(np.arange(N), held)
        wg_d, dwg_d = api.DeviceArray.from_numpy(wg), api.DeviceArray.from_numpy(0.1 * dwg)
        F = [api.DeviceArray(6 * N) for _ in range(3)]
        P.assemble_system(wg_d, dwg_d, F[0])
        r0 = P.scalar_residual()
        P.set_heat_source(api.DeviceArray.from_numpy(q))
        P.assemble_system(wg_d, dwg_d, F[1])
        r1 = P.scalar_residual()
        P.set_heat_source(None)
        P.assemble_system(wg_d, dwg_d, F[2])
        r2 = P.scalar_residual()
        api.sync()
        f = [a.numpy() for a in F]
        assert np.array_equal(f[0], f[1]) and np.array_equal(f[0], f[2])   # F[0:4N) untouched, F[4N:6N) zeroed as before
        assert np.array_equal(r0, r2)
        assert np.array_equal(r1[:N], r0[:N])
        assert np.all(r1[N + held] == 0.0)
        assert np.array_equal(r1[N + free], r0[N + free] - q[free])          # one correctly rounded subtraction
        ulp = EPS * np.maximum(np.abs(r0[N + free]), np.abs(q[free]))
        _check("T_rows", r1[N + free] - r0[N + free], -q[free], ulp)
        assert np.abs(q[free]).max() > 0
    finally:
        P.close()


def _mechanics_run(api, heat, steps=3, substeps=4):
    from dedflow_amd.meshgen import synthetic_fields
    m = kuhn_cube(6, jitter=0.2)
    N = m.num_node
    wg, dw0 = synthetic_fields(m)
    wg[3 * N:4 * N] = 0.0
    rng = np.random.default_rng(81)
    g = np.linspace(0.3, 0.7, 6)
    R = 0.04
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) + rng.uniform(-0.004, 0.004, (216, 3))
    v = rng.normal(scale=0.3, size=pts.shape)
    r = rng.uniform(0.85 * R, R, len(pts))
    P = api.Problem(m, maxit=120, atol=1e-12, rtol=1e-4)
    pc = api.Particles(pts.reshape(-1), v.reshape(-1), R, mass=float(_mass(R)), dt=1e-3)
    try:
        pc.set_sizes(r, _mass(r))
        pc.set_friction(0.4)
        pc.couple(P, two_way=True)
        if heat:
            pc.set_heat(cp_p=500.0, k_p=40.0, T_init=1200.0, two_way=False)
        st = [api.DeviceArray.from_numpy(a) for a in (wg, 0.1 * dw0, 0.1 * dw0)]
        F_d, dx_d = api.DeviceArray(6 * N), api.DeviceArray(6 * N)
        for _ in range(steps):
            P.time_step(st[0], st[1], st[2], F_d, dx_d, newton_maxit=2, particles=pc, dem_substeps=substeps)
        api.sync()
        T = pc.temperature() if heat else None
        return pc.arrays() + (pc.omega().reshape(-1),), st[0].numpy(), T
    finally:
        pc.close()
        P.close()


def test_mechanics_are_untouched(api):
    on, w_on, T = _mechanics_run(api, True)
    off, w_off, _ = _mechanics_run(api, False)
    for a, b in zip(on, off):
        assert np.array_equal(a, b)
    assert np.array_equal(w_on, w_off)
    assert np.abs(on[3]).max() > 0.0 and np.abs(T - 1200.0).max() > 0.0       # contacts happened, heat moved


def test_heat_steps_allocate_nothing(api):
    m = kuhn_cube(6, jitter=0.2)
    N = m.num_node
    x, r, T = _conduction_lattice()
    w = np.zeros(6 * N)
    w[5 * N:] = 400.0
    P = api.Problem(m)
    pc = api.Particles(x.reshape(-1), np.zeros(x.size), R_L, mass=float(_mass(R_L, RHO_P)), dt=1e-3)
    try:
        pc.set_sizes(r, _mass(r, RHO_P))
        pc.couple(P)
        pc.set_heat(cp_p=CP_P, k_p=K_P, T_init=900.0)
        w_d = api.DeviceArray.from_numpy(w)
        src = api.DeviceArray(N)
        pc.heat_step(w_d)
        pc.heat_source(src)
        api.sync()
        before = _pool(api.lib())
        for k in range(100):
            pc.heat_step(w_d)
            if k % 10 == 9:
                pc.heat_source(src)
        api.sync()
        assert _pool(api.lib()) == before
    finally:
        pc.close()
        P.close()


def test_temperature_travels_with_the_particle(api, tmp_path):
    rng = np.random.default_rng(91)
    pts = rng.uniform(0.1, 0.9, size=(300, 3))
    R = 0.005
    pc = api.Particles(pts.reshape(-1), np.zeros(pts.size), R, dt=1e-3)
    other = api.Particles(pts.reshape(-1), np.zeros(pts.size), R, dt=1e-3)
    try:
        pc.set_heat(cp_p=2.0, T_init=700.0)
        assert np.all(pc.temperature() == 700.0)
        T = rng.uniform(300.0, 1500.0, 300)
        pc.set_temperature(T)
        pc.set_outflow(planes=[(0.0, 0.0, 1.0, 0.5)])
        tags0 = pc.tags()
        pc.remove()
        api.sync()
        tags = pc.tags()
        assert 0 < pc.P < 300 and np.array_equal(tags, tags0[pts[:, 2] <= 0.5])
        assert np.array_equal(pc.temperature(), T[tags])
        n0 = pc.P
        pc.set_inflow(origin=(0.2, 0.2, 0.9), edge_u=(0.6, 0.0, 0.0), edge_v=(0.0, 0.6, 0.0), vel=(0.0, 0.0, -1.0), per_call=40)
        pc.add()
        api.sync()
        assert pc.P == n0 + 40
        Tn = pc.temperature()
        assert np.array_equal(Tn[:n0], T[tags]) and np.all(Tn[n0:] == 700.0)
        assert np.all(pc.heat_rate()[n0:] == 0.0) and np.all(pc._pending_energy()[n0:] == 0.0)
        # Copy carries the heat state
        small = api.Particles(np.zeros(3 * pc.P), np.zeros(3 * pc.P), R)
        try:
            api.lib().ParticleContextCopy(small.ctx, pc.ctx)
            api.sync()
            assert np.array_equal(small.temperature(), Tn)
        finally:
            small.close()
        if os.path.exists(os.path.join(os.path.dirname(api.lib_path()), "libdedflow_h5.so")):
            from dedflow_amd import h5 as H
            other.set_heat(cp_p=2.0, T_init=0.0)
            other.set_temperature(T)
            path = str(tmp_path / "p.h5")
            H.save_particles(path, other)
            assert np.array_equal(H.read_dataset(path, "particles/temp", np.float64), T)
            other.set_temperature(np.zeros(300))
            H.load_particles(path, other)
            api.sync()
            assert np.array_equal(other.temperature(), T)
    finally:
        pc.close()
        other.close()


def test_coupled_thermal_time_step(api):
    """kuhn_cube(8), fluid at rest at T0, T transported with no Dirichlet group, hot particles at rest, two_way.  The heat of
    K sub-steps is pending when DflTimeStep runs.  With u = 0 and uniform T the T rows are linear in the rate:
    R_T(dT) = J_T dT - q with J_T of scalar_model at u = 0, so the numpy driver is dT = J_T^-1 q, T' = T0 + kDT kGAMMA dT
    (ref_driver's corrector).  The inner GMRES stops at a relative residual of rtol = 1e-10 from the start dT = 0, so the
    forward error is bounded by cond(J_T) rtol max|dT| with the condition number of the model's own matrix."""
    import scipy.sparse.linalg as spl
    m = kuhn_cube(8)
    N = m.num_node
    T0, Tp, K, dt, R, cp_p, rtol = 300.0, 1500.0, 5, 2e-3, 0.01, 1.0, 1e-10
    w0 = np.zeros(6 * N)
    w0[5 * N:] = T0
    # a cloud that covers the mesh: next to an isolated point source the consistent mass matrix of linear tets undershoots
    # (the model's own J_T^-1 q goes negative there); this layout's source has a positive response at every node, which
    # the test asserts on the model before it looks at the device
    g = np.linspace(0.03, 0.97, 16)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) + 0.003
    mass = float(_mass(R))
    P = api.Problem(m, maxit=120, atol=1e-14, rtol=1e-4)
    pc = api.Particles(pts.reshape(-1), np.zeros(pts.size), R, mass=mass, dt=dt)
    try:
        P.set_scalar_transport(phi=False, T=True, rtol=rtol)
        pc.couple(P)
        pc.set_heat(cp_p=cp_p, T_init=Tp, two_way=True)
        st = [api.DeviceArray.from_numpy(a) for a in (w0, np.zeros(6 * N), np.zeros(6 * N))]
        F_d, dx_d = api.DeviceArray(6 * N), api.DeviceArray(6 * N)
        Ts = [pc.temperature()]
        for _ in range(K):
            pc.fluid_step(st[0])
            Ts.append(pc.temperature())
        api.sync()
        tet, lam, e = pc.tet(), pc.barycentric(), pc._pending_energy()
        assert (tet >= 0).all() and np.all(e < 0.0)
        # the particle model: Nu = 2 in a fluid at rest, K implicit steps towards T0
        tau = float(hm.tau_T(mass * cp_p, 2.0, hm.K_F, 2 * R))
        Tm = np.full(len(pts), Tp, np.longdouble)
        em = np.zeros(len(pts), np.longdouble)
        for _ in range(K):
            Tm, _, de = hm.update(Tm, None, mass * cp_p, dt, Tf=np.full(len(pts), T0), tau=np.full(len(pts), tau))
            em += de
        _check("step_particle_T", Ts[-1], Tm, 1e-13 * Tp)
        _check("step_particle_e", e, em, 1e-13 * float(np.abs(em).max()) * K)
        for a, b in zip(Ts[:-1], Ts[1:]):                                   # cooling monotonically towards the fluid
            assert np.all(b < a) and np.all(b > T0)
        it, rn, r0 = P.time_step(st[0], st[1], st[2], F_d, dx_d, newton_maxit=4, particles=pc, dem_substeps=K)
        api.sync()
        assert 0 < it <= 4 and r0[3] > 0.0
        assert rn[3] < 0.5e-3 * r0[3], (rn, r0)                             # the driver's tolerance
        w1, dw1 = st[0].numpy(), st[2].numpy()
        q, _, _ = hm.node_scatter(N, m.ien, tet, lam, em, K * dt)
        q = q.astype(float)
        assert np.all(q >= 0.0) and q.sum() > 0.0
        JT = sm.jacobians(m.xg, m.ien, np.zeros(6 * N))[1]
        dT = spl.spsolve(JT.tocsc(), q)
        assert dT.min() > 0.0
        hot = np.unique(m.ien.reshape(-1, 4)[tet])
        assert np.all(dw1[5 * N + hot] > 0.0)                                # the fluid warms where the particles are
        tol = np.linalg.cond(JT.toarray()) * rtol * np.abs(dT).max()
        _check("step_fluid_dT", dw1[5 * N:], dT, tol)
        Tnew = T0 + rd.kDT * rd.kGAMMA * dT
        _check("step_fluid_T", w1[5 * N:], Tnew, rd.kDT * rd.kGAMMA * tol + 4 * EPS * T0)
        assert w1[5 * N:].min() >= T0 - rd.kDT * rd.kGAMMA * tol - 4 * EPS * T0   # no node falls below its initial value
        assert np.all(w1[:4 * N] == 0.0)                                     # the fluid stays at rest
        assert np.all(pc.temperature() < Ts[-1])                             # the step's own sub-steps cool further
        assert P.scalar_residual() is not None
    finally:
        pc.close()
        P.close()
