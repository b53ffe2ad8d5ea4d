"""GPU tests of the solid-surface contact (host/surface_contact.c, csrc/k_surface_contact.hip; model in include/dedflow.h
"solid-surface contact").  Build-defined: decisions and forces are compared with tests/surface_contact_model.py
(np.longdouble) on the library's own tets and weights, with the mesh-wall sweep as an independent path, and bit for bit where
two library paths must do the same thing.

Bounds.  A decision cannot be flipped by rounding: every test first asserts the model's margins (no |s -+ r| < 1e-9, no
|s| < 1e-9, no |T_f - T_solid| < 1e-6; capture's margins).  The contact's share of acc is F (1 / m).  Counting the fp64
operations of the header's order from the nodal values on: the interpolation I(phi) and the subtraction of level (4 products, 3
sums, 1), q / |g| and r - s (2), the normal's division (1), v . n (5), kn delta - gamma_n v_n (3), f_n n_d (1), 1 / m and the
product with it (2): K = 22, on S = |kn| (r + |s|) + |gamma_n| |v|.  The bound of a component of acc is

    (22 eps S + C) / m + eps |acc|,      C = |kn| ds + 2 (|gamma_n| |v| + |f_n|) rel_g,
    rel_g = 8 eps |G| / |g|,             ds = |s| rel_g

with the model's own condition term for g: G = the sum of the absolute terms of the closed form of g over |det| (per
component; its norm is used; 8 = the roundings on the path of a term), and eps |acc| for the addition to the sweep's value.
With friction the tangential force is (kt dt + gamma_t) v_t for a new contact, capped at mu f_n, plus kt times the rotated old
spring; its bound is T = mu dfn + 3 (kt dt + gamma_t) (3 Vc dn + |w| ds + 20 eps Vc) + kt |xi_old| (4 dn + 10 eps) + 4 eps mu |f_n|
with Vc = |v| + ell |w|, dn = 2 rel_g + 2 eps the normal's perturbation and dfn the bound of f_n above; the torque's is
ell T + |F_t| (ds + ell dn) + 6 eps ell |F_t| over I; the stored spring's is (T + gamma_t dvt) / kt + dt dvt + |xi_old| (4 dn +
10 eps), dvt = 3 Vc dn + |w| ds + 20 eps Vc.  With DFL_SURFACE_CONTACT_PARITY_LOG set, every comparison appends observed error and
bound to that file (profiles/surface_contact_parity.jsonl is such a log).  Meshes are kuhn_cube(3) or (4), at most 300
particles."""
import json
import os

import numpy as np
import pytest

import surface_contact_model as sm
from dedflow_amd.meshgen import kuhn_cube

pytestmark = pytest.mark.gpu
EPS, LD = sm.EPS, sm.LD
KN, GN, MU = 1.0e4, 3.0, 0.4
KT = 2.0 / 7.0 * KN
GAS = dict(rho_f=1.0e-3, mu_f=1.0e-6)      # a fluid that hardly brakes: the drag is not what these tests are about


@pytest.fixture(scope="module")
def api():
    from dedflow_amd import api as A
    A.lib()
    return A


def _log(name, err, bound):
    err, bound = float(err), float(bound)
    path = os.environ.get("DFL_SURFACE_CONTACT_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"check": name, "error": err, "bound": bound, "ratio": err / bound if bound > 0 else None}) + "\n")
    print(f"surface contact parity {name}: error {err:.3e} bound {bound:.3e}")
    return err, bound


def _check(name, got, ref, bound):
    d = np.abs(np.asarray(got, LD) - np.asarray(ref, LD)).reshape(-1)
    bound = np.broadcast_to(np.asarray(bound, float), np.shape(got)).reshape(-1)
    if d.size == 0:
        return
    k = int(np.argmax(d / np.maximum(bound, 1e-300)))
    err, b = _log(name, d[k], bound[k])
    assert err <= b, (name, err, b)


def _upload(api, pc, k, a):
    """overwrite coord (k = 0), vel (1) or acc (2) on the device"""
    api.sync()
    api.DeviceArray(3 * pc.P, ptr=pc.ctx.contents.d_arr[k].contents.data).upload(np.asarray(a, float).reshape(-1))


def _context(api, m, case, poly, friction, dt=1e-5, gravity=(0.0, 0.0, 0.0), gamma_n=GN):
    Pb = api.Problem(m)
    pc = api.Particles(case["pts"].reshape(-1), case["vel"].reshape(-1), case["R"], mass=float(case["mass"]), kn=KN, gamma_n=gamma_n,
                       dt=dt)
    if poly and pc.P:
        pc.set_sizes(case["r"], case["m"])
    if friction:
        pc.set_friction(MU)
        if pc.P:
            pc.set_omega(case["omega"])
    pc.couple(Pb, gravity=gravity, **GAS)
    return Pb, pc


def _state(api, pc, friction):
    api.sync()
    o = dict(arrays=pc.arrays())
    if friction:
        keys, xi, cnt = pc.friction_history()
        o.update(omega=pc.omega(), alpha=pc.alpha(), keys=keys, xi=xi, cnt=cnt, overflow=pc.friction_overflow_count())
    return o


def _same_bits(a, b, friction):
    """coord, vel, acc and, with friction, omega, alpha and the live history entries, bit for bit"""
    for x, y in zip(a["arrays"], b["arrays"]):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
    if friction:
        assert np.array_equal(a["cnt"], b["cnt"])
        live = np.arange(16)[None, :] < a["cnt"][:, None]
        assert np.array_equal(a["keys"][live], b["keys"][live])
        assert np.array_equal(a["xi"][live].view(np.uint64), b["xi"][live].view(np.uint64))
        for k in ("omega", "alpha"):
            assert np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64))


def _bounds(dec, case, poly, vel, friction, omega=None, xi_old=None, fn=None, Ft=None, dt=1e-5, gamma_n=GN):
    """the a-priori bounds of the module docstring per particle: acc, alpha, xi"""
    P = len(dec["s"])
    r = dec["r"].astype(float)
    m = np.broadcast_to(np.asarray(case["m"] if poly else case["mass"], float), (P,))
    with np.errstate(invalid="ignore", divide="ignore"):
        s, gn = np.abs(dec["s"].astype(float)), dec["gn"].astype(float)
        v = np.linalg.norm(np.asarray(vel, float).reshape(-1, 3), axis=1)
        S = KN * (r + s) + gamma_n * v
        rel_g = 8 * EPS * np.linalg.norm(dec["g_cond"].astype(float), axis=1) / gn
        ds = s * rel_g
        afn = np.abs(np.asarray(fn, float))
        C = KN * ds + 2 * (gamma_n * v + afn) * rel_g
        dF = 22 * EPS * S + C
        out = dict(S=S, dF=dF, m=m)
        if friction:
            w = np.linalg.norm(np.asarray(omega, float).reshape(-1, 3), axis=1)
            ell = np.maximum(r - dec["delta"].astype(float), 0.0)
            Vc = v + ell * w
            dn = 2 * rel_g + 2 * EPS
            xo = np.array([0.0 if (xi_old is None or xi_old[i] is None) else float(np.linalg.norm(np.asarray(xi_old[i], float)))
                           for i in range(P)])
            dvt = 3 * Vc * dn + w * ds + 20 * EPS * Vc
            T = MU * dF + 3 * (KT * dt + gamma_n) * dvt + KT * xo * (4 * dn + 10 * EPS) + 4 * EPS * MU * afn
            aFt = np.linalg.norm(np.asarray(Ft, float), axis=1)
            out.update(dF=dF + T, dtau=ell * T + aFt * (ds + ell * dn) + 6 * EPS * ell * aFt, I=0.4 * m * r * r,
                       dxi=(T + gamma_n * dvt) / KT + dt * dvt + xo * (4 * dn + 10 * EPS))
    return out


def _apply_and_compare(api, tag, pc, m, case, w, w_d, poly, friction, side, T_solid, xi_from_history=False, dt=1e-5):
    """one sweep, one locate, the contact alone; decisions, acc, alpha, the history row and the stats against the model"""
    pc.compute_forces()
    pc.locate()
    before = _state(api, pc, friction)
    tet, lam = pc.tet(), pc.barycentric()
    pc._surface_contact_apply(w_d)
    after = _state(api, pc, friction)
    stats = pc.surface_contact_stats()
    P = pc.P
    radius, mass = (case["r"], case["m"]) if poly else (case["R"], case["mass"])
    dec = sm.decide(m.xg, m.ien, w, tet, lam, radius, sm.LEVEL, side, T_solid)
    assert sm.margins_ok(dec, T_solid)
    vel = before["arrays"][1].reshape(-1, 3)
    law = dict(mu=MU, kt=KT, gamma_t=GN, dt=dt) if friction else None
    # the surface springs the previous sub-step stored: the sweep just read those rows, so the caller hands them over
    xi_old = xi_from_history if friction and xi_from_history else None
    F, tau, xi, fn = sm.forces(dec, vel, mass, KN, GN, friction=law, omega=before.get("omega"), xi_old=xi_old)
    a_ref, al_ref = sm.accelerations(F, tau, mass, radius)
    con = np.asarray(dec["contact"])
    Fn = fn[:, None] * np.where(con[:, None], dec["n"], 0)
    b = _bounds(dec, case, poly, vel, friction, omega=before.get("omega"), xi_old=xi_old, fn=fn, Ft=(F - Fn), dt=dt)
    acc0, acc1 = before["arrays"][2].reshape(-1, 3), after["arrays"][2].reshape(-1, 3)
    # decisions: exactly the particles in contact were written, and the counters say so
    changed = (acc0.view(np.uint64) != acc1.view(np.uint64)).any(axis=1)
    assert not changed[~con].any()
    assert stats["last"] == int(con.sum()) and stats["buried"] == int(dec["buried"].sum())
    for k in (0, 1):
        assert np.array_equal(before["arrays"][k].view(np.uint64), after["arrays"][k].view(np.uint64))
    if con.any():
        bound = (b["dF"] / b["m"])[:, None] + EPS * np.abs(acc1)
        _check(f"acc_{tag}", (acc1.astype(LD) - acc0)[con], a_ref[con], bound[con])
        assert np.abs(acc1 - acc0)[con].max() > 0.0
    out = dict(dec=dec, stats=stats, xi=None, after=after)
    if friction:
        al0, al1 = before["alpha"], after["alpha"]
        assert np.array_equal(al0[~con].view(np.uint64), al1[~con].view(np.uint64))
        assert np.array_equal(before["omega"].view(np.uint64), after["omega"].view(np.uint64))
        c0, c1 = before["cnt"], after["cnt"]
        stored = con & (c0 < 16)                                  # a full row: the force of a new contact, nothing stored, counted
        assert np.array_equal(c1, c0 + stored) and (c1 <= 16).all()
        assert after["overflow"] - before["overflow"] == int((con & ~stored).sum())
        assert xi_old is None or not (con & ~stored).any()
        live = np.arange(16)[None, :] < c0[:, None]               # the sweep's entries stay in front, untouched
        assert np.array_equal(before["keys"][live], after["keys"][live])
        assert np.array_equal(before["xi"][live].view(np.uint64), after["xi"][live].view(np.uint64))
        if con.any():
            idx = np.nonzero(stored)[0]
            assert (after["keys"][idx, c0[idx]] == np.uint64(sm.KEY_SURFACE)).all()
            bound = (b["dtau"] / b["I"])[:, None] + EPS * np.abs(al1)
            _check(f"alpha_{tag}", (al1.astype(LD) - al0)[con], al_ref[con], bound[con])
            got = after["xi"][idx, c0[idx]]
            _check(f"xi_{tag}", got, np.array([xi[i] for i in idx], LD), b["dxi"][idx, None] + EPS * np.abs(got))
            assert np.abs(al1 - al0)[con].max() > 0.0
        out["xi"] = [after["xi"][i, c0[i]].copy() if stored[i] else None for i in range(P)]   # what the library stored
    return out


@pytest.mark.parametrize("friction", [False, True], ids=["smooth", "friction"])
@pytest.mark.parametrize("poly", [False, True], ids=["mono", "poly"])
@pytest.mark.parametrize("side", [1, -1], ids=["above", "below"])
@pytest.mark.parametrize("P", [1, 63, 65, 257, 300])
def test_decisions_and_forces_match_the_model(api, P, side, poly, friction):
    """a plane with |g| = 1.7 on kuhn_cube(3): every class of surface_contact_model.CLASSES (P > 5), one partial wave (1, 63),
    a wave and one lane (65), a workgroup and one lane (257), two workgroups (300); two sub-steps, the second with the spring
    the first one stored"""
    m = kuhn_cube(3)
    case = sm.plane_case(P, poly)
    w = sm.plane_fields(m.xg, side)
    Pb, pc = _context(api, m, case, poly, friction)
    try:
        w_d = api.DeviceArray.from_numpy(w)
        pc.set_surface_contact(level=sm.LEVEL, side=side, T_solid=sm.T_SOLID)
        assert pc.surface_contact_on and pc.surface_contact_stats() == {"last": 0, "buried": 0, "total": 0}
        tag = f"P{P}_{'above' if side == 1 else 'below'}_{'poly' if poly else 'mono'}_{'friction' if friction else 'smooth'}"
        o = _apply_and_compare(api, tag + "_1", pc, m, case, w, w_d, poly, friction, side, sm.T_SOLID)
        cls = sm.classify(o["dec"], sm.T_SOLID)
        if P > 5:
            assert set(cls) == set(range(6))
        n1 = o["stats"]["last"]
        assert o["stats"]["total"] == n1 and n1 == int((cls <= 1).sum()) > 0
        o2 = _apply_and_compare(api, tag + "_2", pc, m, case, w, w_d, poly, friction, side, sm.T_SOLID, xi_from_history=o["xi"])
        assert o2["stats"] == {"last": n1, "buried": o["stats"]["buried"], "total": 2 * n1}
        if friction:
            assert pc.friction_overflow_count() == 0
    finally:
        pc.close()
        Pb.close()


@pytest.mark.parametrize("friction", [False, True], ids=["smooth", "friction"])
def test_a_field_that_is_not_linear(api, friction):
    """the distance to a sphere sampled at the nodes of kuhn_cube(4): the gradient changes from tet to tet"""
    m = kuhn_cube(4)
    case = sm.sphere_case(300, True, R=0.04)
    w = sm.sphere_fields(m.xg, -1)
    Pb, pc = _context(api, m, case, True, friction)
    try:
        w_d = api.DeviceArray.from_numpy(w)
        pc.set_surface_contact(level=sm.LEVEL, side=-1, T_solid=sm.T_SOLID)
        o = _apply_and_compare(api, f"sphere_{'friction' if friction else 'smooth'}", pc, m, case, w, w_d, True, friction, -1, sm.T_SOLID)
        assert set(sm.classify(o["dec"], sm.T_SOLID)) == set(range(6))
    finally:
        pc.close()
        Pb.close()


def test_after_geometry_changed_the_bound_follows_the_mesh(api):
    """the early exit rests on a bound over the mesh's |grad N|: the mesh is squeezed to 0.3 of its height about z = 1/2 (the
    gradients grow), DflMeshGeometryChanged is called, and the next sub-step must decide with the new coordinates.  The
    bound of the old mesh would have dropped particles that touch, which the test first shows from the model"""
    import copy
    m = kuhn_cube(3)
    case = sm.plane_case(300, True)
    w = sm.plane_fields(m.xg, 1)

    def squeeze(x):
        x = np.array(x, float).reshape(-1, 3)
        x[:, 2] = 0.5 + 0.3 * (x[:, 2] - 0.5)
        return x

    def grad_max(xg):
        x4 = np.asarray(xg, float).reshape(-1, 3)[m.ien.reshape(-1, 4)]
        e1, e2, e3 = x4[:, 1] - x4[:, 0], x4[:, 2] - x4[:, 0], x4[:, 3] - x4[:, 0]
        c = [np.cross(e2, e3), np.cross(e3, e1), np.cross(e1, e2)]
        return max((np.linalg.norm(ck, axis=1) / np.abs((e1 * c[0]).sum(axis=1))).max() for ck in c)

    m2 = copy.copy(m)
    m2.xg = squeeze(m.xg).reshape(-1)
    case2 = dict(case, pts=squeeze(case["pts"]))
    Pb, pc = _context(api, m, case, True, False)
    try:
        w_d = api.DeviceArray.from_numpy(w)
        pc.set_surface_contact(level=sm.LEVEL, side=1, T_solid=sm.T_SOLID)
        _apply_and_compare(api, "moved_before", pc, m, case, w, w_d, True, False, 1, sm.T_SOLID)
        api.sync()
        api.DeviceArray(3 * Pb.N, ptr=Pb.mesh.contents.device.contents.xg).upload(m2.xg)
        api.lib().DflMeshGeometryChanged(Pb.mesh)
        _upload(api, pc, 0, case2["pts"])
        o = _apply_and_compare(api, "moved_after", pc, m2, case2, w, w_d, True, False, 1, sm.T_SOLID)
        dec = o["dec"]
        N = m.num_node
        phi = w[4 * N:5 * N][m.ien.reshape(-1, 4)[np.where(dec["located"], pc.tet(), 0)]]
        spread = np.abs(phi[:, 1:] - phi[:, :1]).sum(axis=1)
        q = -dec["f"].astype(float)
        assert (dec["contact"] & (q > case["r"] * spread * grad_max(m.xg) * (1 + 1e-6))).sum() > 0     # the stale bound fails
        assert not (dec["contact"] & (q > case["r"] * spread * grad_max(m2.xg) * (1 + 1e-6))).any()   # the new one holds
    finally:
        pc.close()
        Pb.close()


def _off_run(api, mode, friction, K=5):
    m = kuhn_cube(3)
    case = sm.plane_case(300, True)
    w = sm.plane_fields(m.xg, 1)
    Pb, pc = _context(api, m, case, True, friction, dt=1e-4)
    try:
        w_d = api.DeviceArray.from_numpy(w)
        if mode == "cleared":
            pc.set_surface_contact(level=sm.LEVEL, side=1, T_solid=sm.T_SOLID)
            assert pc.surface_contact_on
            pc.set_surface_contact(level=None)
            assert not pc.surface_contact_on
        elif mode == "nowhere":
            pc.set_surface_contact(level=sm.LEVEL, side=1, T_solid=-np.inf)
        elif mode == "on":
            pc.set_surface_contact(level=sm.LEVEL, side=1, T_solid=sm.T_SOLID)
        for _ in range(K):
            pc.fluid_step(w_d)
        return _state(api, pc, friction), pc.surface_contact_stats()
    finally:
        pc.close()
        Pb.close()


@pytest.mark.parametrize("friction", [False, True], ids=["smooth", "friction"])
def test_off_is_off(api, friction):
    """five coupled sub-steps: never set, set and cleared, and set with T_solid = -inf leave coord, vel, acc, omega and the
    history rows bit for bit; the same contact with a melting point changes them"""
    ref, st = _off_run(api, "never", friction)
    assert st == {"last": 0, "buried": 0, "total": 0}
    for mode in ("cleared", "nowhere"):
        o, st = _off_run(api, mode, friction)
        _same_bits(ref, o, friction)
        assert st == {"last": 0, "buried": 0, "total": 0}
    o, st = _off_run(api, "on", friction)
    assert st["total"] > 0 and not np.array_equal(ref["arrays"][1], o["arrays"][1])


def _floor_case(P=48, R=0.035, seed=3):
    """particles resting in the bottom face z = 0 of the unit cube, further than R from the five other walls and from each
    other: the first half at a tiny overlap and a large tangential velocity (they slide), the rest deeper and slow (they stick)"""
    rng = np.random.default_rng(seed)
    g = 0.15 + 0.1 * np.arange(7)
    xy = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)[:P] + rng.uniform(-0.01, 0.01, (P, 2))
    slide = np.arange(P) < P // 2
    z = np.where(slide, rng.uniform(0.990, 0.999, P), rng.uniform(0.3, 0.9, P)) * R
    vel = np.where(slide[:, None], rng.normal(scale=1.0, size=(P, 3)), rng.normal(scale=1e-4, size=(P, 3)))
    vel[:, 2] = rng.uniform(-0.01, 0.01, P)
    case = sm._particles(np.c_[xy, z], rng, R)
    case.update(vel=vel, omega=rng.normal(scale=2.0, size=(P, 3)), slide=slide)
    return case


def test_against_the_mesh_walls(api):
    """phi = z, level 0, side -1 on the unit Kuhn cube, everything solid: the surface is the bottom face.  Context A collides
    with the wall mesh of the bottom group, context B with the surface (its wall mesh is the top group, out of reach).  Over
    20 sub-steps acc, alpha and the springs agree within the bound of the parity test; after every sub-step B takes A's coord, vel and omega, so that only the springs travel on their own"""
    m = kuhn_cube(3)
    N = m.num_node
    case = _floor_case()
    P = len(case["pts"])
    w = np.zeros(6 * N)
    w[4 * N:5 * N] = m.xg.reshape(-1, 3)[:, 2]
    dt = 1e-4
    ctx = []
    try:
        for which in "AB":
            Pb, pc = _context(api, m, case, False, True, dt=dt)
            ctx.append((Pb, pc))
            pc.set_walls(Pb, groups=[4] if which == "A" else [5])
            if which == "B":
                pc.set_surface_contact(level=0.0, side=-1)
        (_, A), (_, B) = ctx
        w_d = api.DeviceArray.from_numpy(w)
        seen_slide = seen_stick = 0
        xi_prev = [None] * P
        for step in range(20):
            for pc in (A, B):
                pc.compute_forces()
                pc.locate()
            B._surface_contact_apply(w_d)
            a, b = _state(api, A, True), _state(api, B, True)
            dec = sm.decide(m.xg, m.ien, w, B.tet(), B.barycentric(), case["R"], 0.0, -1, np.inf)
            assert sm.margins_ok(dec, np.inf) and dec["contact"].all()
            vel, om = b["arrays"][1].reshape(-1, 3), b["omega"]
            accA, accB = a["arrays"][2].reshape(-1, 3), b["arrays"][2].reshape(-1, 3)
            fn = case["mass"] * accB[:, 2]
            Ft = case["mass"] * accB.copy()
            Ft[:, 2] = 0.0
            bd = _bounds(dec, case, False, vel, True, omega=om, xi_old=xi_prev, fn=fn, Ft=Ft, dt=dt)
            _check(f"walls_acc_{step}", accB, accA, ((bd["dF"] / bd["m"])[:, None] + EPS * np.abs(accA)))
            _check(f"walls_alpha_{step}", b["alpha"], a["alpha"], ((bd["dtau"] / bd["I"])[:, None] + EPS * np.abs(a["alpha"])))
            assert (a["cnt"] == 1).all() and (b["cnt"] == 1).all()
            assert (b["keys"][:, 0] == np.uint64(sm.KEY_SURFACE)).all()
            assert ((a["keys"][:, 0] >> np.uint64(62)) == 1).all() and ((a["keys"][:, 0] & np.uint64((1 << 62) - 1)) < 2 ** 31).all()
            _check(f"walls_xi_{step}", b["xi"][:, 0], a["xi"][:, 0], (bd["dxi"][:, None] + EPS * np.abs(a["xi"][:, 0])))
            sliding = np.linalg.norm(Ft, axis=1) >= MU * np.maximum(fn, 0.0) * (1 - 1e-9)
            seen_slide += int(sliding.sum())
            seen_stick += int((~sliding).sum())
            xi_prev = [b["xi"][i, 0] for i in range(P)]
            A.fluid_step(w_d)
            B.fluid_step(w_d)
            api.sync()
            for k in (0, 1):
                _upload(api, B, k, A.arrays()[k])
            B.set_omega(A.omega())
            assert (A.arrays()[0].reshape(-1, 3)[:, 2] < case["R"]).all() and (A.arrays()[0].reshape(-1, 3)[:, 2] > 0).all()
        assert seen_slide > 20 and seen_stick > 20
        assert A.friction_overflow_count() == 0 and B.friction_overflow_count() == 0 and A.wall_dropped_count() == 0
    finally:
        for Pb, pc in ctx:
            pc.close()
            Pb.close()


def test_history_order_survival_and_overflow(api):
    m = kuhn_cube(3)
    N = m.num_node
    w = np.zeros(6 * N)
    w[4 * N:5 * N] = m.xg.reshape(-1, 3)[:, 2] - 0.5                       # the surface z = 1/2, metal below
    R = 0.05
    rng = np.random.default_rng(5)
    # 0 and 1 touch each other and the surface; 2 touches the surface alone; 3 is far away (removed later)
    pts = np.array([[0.3, 0.3, 0.5 + 0.6 * R], [0.3 + 1.8 * R, 0.3, 0.5 + 0.7 * R], [0.7, 0.7, 0.5 + 0.5 * R], [0.5, 0.2, 0.9]])
    case = sm._particles(pts, rng, R)
    case["vel"] = rng.normal(scale=0.2, size=pts.shape)
    Pb, pc = _context(api, m, case, False, True, dt=1e-4)
    try:
        w_d = api.DeviceArray.from_numpy(w)
        pc.set_surface_contact(level=0.0, side=-1)
        pc.set_outflow(planes=[(0.0, 0.0, 1.0, 0.85)])
        pc.fluid_step(w_d)
        s1 = _state(api, pc, True)
        KS = np.uint64(sm.KEY_SURFACE)
        assert list(s1["cnt"]) == [2, 2, 1, 0]
        assert s1["keys"][0, 0] == 1 and s1["keys"][1, 0] == 0            # the sweep's pair entries in front
        assert s1["keys"][0, 1] == KS and s1["keys"][1, 1] == KS and s1["keys"][2, 0] == KS
        assert pc.surface_contact_stats() == {"last": 3, "buried": 0, "total": 3}
        pc.fluid_step(w_d)
        s2 = _state(api, pc, True)
        assert np.abs(s2["xi"][2, 0]).max() > np.abs(s1["xi"][2, 0]).max() > 0.0   # the spring was found and advanced
        pc.remove()                                                       # particle 3 leaves: ids and the surface key stay
        assert pc.P == 3
        s3 = _state(api, pc, True)
        assert list(s3["cnt"]) == [2, 2, 1] and s3["keys"][2, 0] == KS and s3["keys"][0, 1] == KS
        assert np.array_equal(s3["xi"][:3].view(np.uint64)[np.arange(16)[None, :] < s3["cnt"][:, None]],
                              s2["xi"][:3].view(np.uint64)[np.arange(16)[None, :] < s2["cnt"][:3, None]])
        x = pc.arrays()[0].reshape(-1, 3).copy()
        x[2, 2] = 0.5 + 3 * R                                             # particle 2 leaves the surface
        _upload(api, pc, 0, x)
        pc.fluid_step(w_d)
        s4 = _state(api, pc, True)
        assert list(s4["cnt"]) == [2, 2, 0] and pc.surface_contact_stats()["last"] == 2
        assert pc.friction_overflow_count() == 0
    finally:
        pc.close()
        Pb.close()
    # a full row: the crowded configuration of test_gpu_friction.py (20 neighbours around one particle), on the surface
    k = np.arange(20) + 0.5
    th, ph = np.arccos(1 - 2 * k / 20), np.pi * (1 + 5 ** 0.5) * k
    d = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], axis=1)
    pts = np.vstack([[0.5, 0.5, 0.5 + 0.3 * R], np.array([0.5, 0.5, 0.5 + 0.3 * R]) + 1.5 * R * d])
    case = sm._particles(pts, rng, R)
    out = []
    for on in (False, True):
        Pb, pc = _context(api, m, case, False, True, dt=1e-4)
        try:
            w_d = api.DeviceArray.from_numpy(w)
            if on:
                pc.set_surface_contact(level=0.0, side=-1)
            pc.compute_forces()
            pc.locate()
            pc._surface_contact_apply(w_d)
            st = _state(api, pc, True)
            out.append((pc.friction_overflow_count(), st, pc.surface_contact_stats(), pc.tet(), pc.barycentric()))
        finally:
            pc.close()
            Pb.close()
    (n0, s0, _, _, _), (n1, s1, stats, tet, lam) = out
    dec = sm.decide(m.xg, m.ien, w, tet, lam, R, 0.0, -1, np.inf)
    assert sm.margins_ok(dec, np.inf) and dec["contact"][0] and s0["cnt"][0] == 16 and n0 >= 4
    full = dec["contact"] & (s0["cnt"] == 16)
    assert n1 == n0 + int(full.sum()) and stats["last"] == int(dec["contact"].sum())
    assert s1["cnt"][0] == 16 and np.array_equal(s1["keys"][0], s0["keys"][0])    # nothing stored, the row untouched
    assert np.array_equal(s1["xi"][0].view(np.uint64), s0["xi"][0].view(np.uint64))
    assert np.abs(s1["arrays"][2].reshape(-1, 3)[0] - s0["arrays"][2].reshape(-1, 3)[0]).max() > 0.0   # the force still acts


def _leak_run(api, m, case, w, tets=None, friction=True, early_exit=True):
    Pb, pc = _context(api, m, case, True, friction)
    try:
        w_d = api.DeviceArray.from_numpy(w)
        pc.set_surface_contact(level=sm.LEVEL, side=1, T_solid=sm.T_SOLID)
        if not early_exit:
            pc._surface_contact_no_early_exit()
        pc.compute_forces()
        pc.locate()
        api.sync()
        if tets is not None:                                              # overwrite the located tets (library-private array)
            t = tets(pc.tet())
            api.DeviceArray(pc.P, dtype=np.int32, ptr=api.lib().ParticleContextTet(pc.ctx)).upload(t)
        before = _state(api, pc, friction)
        tet, lam = pc.tet(), pc.barycentric()
        pc._surface_contact_apply(w_d)
        return before, _state(api, pc, friction), pc.surface_contact_stats(), tet, lam
    finally:
        pc.close()
        Pb.close()


def test_nothing_leaks(api):
    m = kuhn_cube(3)
    N = m.num_node
    ien4 = m.ien.reshape(-1, 4)
    case = sm.plane_case(300, True)
    w = sm.plane_fields(m.xg, 1)
    zero = {"last": 0, "buried": 0, "total": 0}
    # P = 0
    empty = dict(case, pts=np.zeros((0, 3)), vel=np.zeros((0, 3)))
    b, a, st, _, _ = _leak_run(api, m, empty, w, friction=False)
    assert st == zero
    # every particle at tet -1, then one at tet -2
    b, a, st, _, _ = _leak_run(api, m, case, w, tets=lambda t: np.full_like(t, -1))
    _same_bits(b, a, True)
    assert st == zero
    base_b, base_a, base_st, tet0, lam0 = _leak_run(api, m, case, w)
    dec0 = sm.decide(m.xg, m.ien, w, tet0, lam0, case["r"], sm.LEVEL, 1, sm.T_SOLID)
    first = int(np.nonzero(dec0["contact"])[0][0])

    def lose(t):
        t = t.copy()
        t[first] = -2
        return t
    b, a, st, _, _ = _leak_run(api, m, case, w, tets=lose)
    assert st["last"] == base_st["last"] - 1
    assert np.array_equal(a["arrays"][2].reshape(-1, 3)[first].view(np.uint64), b["arrays"][2].reshape(-1, 3)[first].view(np.uint64))
    assert a["cnt"][first] == b["cnt"][first]
    # a NaN phi or T at one node: only the particles in the tets of that node lose their contact
    node = int(ien4[tet0[first], 0])
    touched = (ien4[np.where(tet0 >= 0, tet0, 0)] == node).any(axis=1) & (tet0 >= 0)
    acc_base = base_a["arrays"][2].reshape(-1, 3)
    for field in (4, 5):
        w2 = w.copy()
        w2[field * N + node] = np.nan
        b, a, st, tet, _ = _leak_run(api, m, case, w2)
        assert np.array_equal(tet, tet0)
        acc_b, acc_a = b["arrays"][2].reshape(-1, 3), a["arrays"][2].reshape(-1, 3)
        assert np.array_equal(acc_a[touched].view(np.uint64), acc_b[touched].view(np.uint64))
        assert np.array_equal(acc_a[~touched].view(np.uint64), acc_base[~touched].view(np.uint64))
        assert np.array_equal(a["cnt"][touched], b["cnt"][touched]) and np.array_equal(a["cnt"][~touched], base_a["cnt"][~touched])
        assert st["last"] == int((dec0["contact"] & ~touched).sum()) and st["buried"] == int((dec0["buried"] & ~touched).sum())
        assert np.isfinite(acc_a).all()
    # a constant phi: |g| = 0 in every tet
    w2 = w.copy()
    w2[4 * N:5 * N] = sm.LEVEL - 0.001
    b, a, st, _, _ = _leak_run(api, m, case, w2)
    _same_bits(b, a, True)
    assert st == zero
    # two runs are bitwise equal
    again_b, again_a, again_st, _, _ = _leak_run(api, m, case, w)
    _same_bits(base_a, again_a, True)
    assert again_st == base_st and base_st["last"] > 0
    # the early exit for particles far on the gas side only skips work: without it, the same bits and counts
    _, full_a, full_st, _, _ = _leak_run(api, m, case, w, early_exit=False)
    _same_bits(base_a, full_a, True)
    assert full_st == base_st


def _bounce_run(api, with_contact, steps=1700):
    """kuhn_cube(4), the surface z = 1/2 (metal below), gravity, gamma_n = 0; cold metal with one hot disc in the corner
    x, y > 3/4; six particles dropped from rest over cold metal, three over the disc"""
    m = kuhn_cube(4)
    N = m.num_node
    x = m.xg.reshape(-1, 3)
    w = np.zeros(6 * N)
    w[4 * N:5 * N] = x[:, 2] - 0.5
    w[5 * N:] = np.where((x[:, 0] > 0.7) & (x[:, 1] > 0.7), 2000.0, 300.0)
    R, dt, g, drop = 0.02, 1e-4, 9.81, 0.02
    cold = np.array([[0.1, 0.1], [0.3, 0.12], [0.12, 0.33], [0.31, 0.35], [0.2, 0.45], [0.45, 0.2]])
    hot = np.array([[0.8, 0.8], [0.9, 0.82], [0.82, 0.92]])
    pts = np.c_[np.vstack([cold, hot]), np.full(9, 0.5 + R + drop)]
    case = sm._particles(pts, np.random.default_rng(1), R)
    case["vel"] = np.zeros_like(pts)
    Pb, pc = _context(api, m, case, False, False, dt=dt, gravity=(0.0, 0.0, -g), gamma_n=0.0)
    try:
        w_d = api.DeviceArray.from_numpy(w)
        pc.set_capture(level=0.0, side=-1, reach=1.0, T_melt=1500.0)
        if with_contact:
            pc.set_surface_contact(level=0.0, side=-1, T_solid=1500.0)
        zmin = np.full(9, np.inf)
        apex = np.full(9, -np.inf)
        turned = np.zeros(9, bool)
        touched = 0
        for k in range(steps // 10):
            for _ in range(10):
                pc.fluid_step(w_d)
            touched += pc.surface_contact_stats()["last"]
            pc.capture(w_d)
            api.sync()
            tags = pc.tags()
            xs, vs, _ = (a.reshape(-1, 3) for a in pc.arrays())
            zmin[tags] = np.minimum(zmin[tags], xs[:, 2])
            turned[tags] |= vs[:, 2] > 0.0
            up = tags[turned[tags]]
            apex[up] = np.maximum(apex[up], xs[turned[tags], 2])
        return dict(tags=tags, zmin=zmin, apex=apex, captured=pc.capture_stats()["captured"], P=pc.P, R=R, dt=dt,
                    v_imp=np.sqrt(2 * g * drop), z0=0.5 + R + drop, touched=touched, z=xs[:, 2])
    finally:
        pc.close()
        Pb.close()


def test_powder_bounces_off_cold_metal_and_is_captured_by_the_pool(api):
    """the test that fails without the feature: particles over cold metal must not sink below the surface; they come back to
    their drop height to O(dt) (no dashpot, a gas that hardly brakes; the semi-implicit Euler step keeps a modified energy
    that differs from the true one by dt v a / 2, that is, by a height of at most dt v_impact; 5 dt v_impact is asserted, plus
    the 10-step sampling of the apex, g (10 dt)^2 / 2).  Particles over the hot disc (T >= T_solid = T_melt) never collide
    and are captured when they touch (reach = 1).  captured + remaining = P"""
    o = _bounce_run(api, True)
    assert o["captured"] == 3 and o["P"] == 6 and o["captured"] + o["P"] == 9
    assert np.array_equal(o["tags"], np.arange(6))
    cold = np.arange(6)
    assert (o["zmin"][cold] - 0.5 > -o["R"]).all() and (o["zmin"][cold] - 0.5 < o["R"]).all()     # s > -r, and they did touch
    assert o["touched"] > 0
    tol = 5 * o["dt"] * o["v_imp"] + 0.5 * 9.81 * (10 * o["dt"]) ** 2
    print("bounce: apex - drop height", o["apex"][cold] - o["z0"], "tolerance", tol)
    assert np.abs(o["apex"][cold] - o["z0"]).max() <= tol
    # without the contact the cold particles fall through the metal
    off = _bounce_run(api, False, steps=1300)
    assert off["captured"] == 3 and (off["z"] - 0.5 < -off["R"]).all()


def test_time_step_copy_and_recoupling(api):
    """DflTimeStep with the contact set equals the same calls made by hand, bit for bit; ParticleContextCopy carries the
    configuration to a coupled dst and not to an uncoupled one; re-coupling keeps it, uncoupling frees it; refusals leave
    the context as it was"""
    import ctypes as C
    m = kuhn_cube(4)
    N = m.num_node
    x = m.xg.reshape(-1, 3)
    w0 = np.zeros(6 * N)
    w0[4 * N:5 * N] = x[:, 2] - 0.5
    w0[5 * N:] = 300.0
    R = 0.02
    rng = np.random.default_rng(8)
    xy = np.stack(np.meshgrid(0.2 + 0.15 * np.arange(4), 0.2 + 0.15 * np.arange(4), indexing="ij"), axis=-1).reshape(-1, 2)
    pts = np.c_[xy, 0.5 + rng.uniform(0.3, 1.5, 16) * R]
    case = sm._particles(pts, rng, R)
    K = 6
    runs = {}
    for mode in ("time_step", "by_hand"):
        P = api.Problem(m, maxit=120, atol=1e-14, rtol=1e-6)
        pc = api.Particles(pts.reshape(-1), case["vel"].reshape(-1), R, mass=float(case["mass"]), kn=KN, gamma_n=GN, dt=1e-4)
        try:
            pc.set_friction(MU)
            pc.couple(P, gravity=(0.0, 0.0, -9.81), **GAS)
            pc.set_surface_contact(level=0.0, side=-1, T_solid=1500.0)
            st = [api.DeviceArray.from_numpy(a) for a in (w0, np.zeros(6 * N), np.zeros(6 * N))]
            F_d, dx_d = api.DeviceArray(6 * N), api.DeviceArray(6 * N)
            for _ in range(2):
                if mode == "time_step":
                    P.time_step(st[0], st[1], st[2], F_d, dx_d, newton_maxit=2, particles=pc, dem_substeps=K)
                else:
                    P.time_step(st[0], st[1], st[2], F_d, dx_d, newton_maxit=2)
                    for _ in range(K):
                        pc.fluid_step(st[0])
            stats = pc.surface_contact_stats()
            runs[mode] = (_state(api, pc, True), stats, st[0].numpy())
        finally:
            pc.close()
            P.close()
    (sa, ta, wa), (sb, tb, wb) = runs["time_step"], runs["by_hand"]
    _same_bits(sa, sb, True)
    assert ta == tb and ta["total"] > 0 and np.array_equal(wa, wb)
    # travel and refusals
    P, P2 = api.Problem(m), api.Problem(kuhn_cube(3))
    mk = lambda: api.Particles(pts.reshape(-1), case["vel"].reshape(-1), R, mass=float(case["mass"]))
    src, dst, lone = mk(), mk(), mk()
    try:
        L = api.lib()
        L.ParticleContextCopy.argtypes = [C.POINTER(api.ParticleContext), C.POINTER(api.ParticleContext)]
        L.ParticleContextCopy.restype = None
        src.set_surface_contact(level=0.0, side=-1)                       # not coupled: refused
        assert not src.surface_contact_on
        src.couple(P, **GAS)
        dst.couple(P, **GAS)
        for bad in (dict(level=0.0, side=0), dict(level=np.inf, side=1), dict(level=0.0, side=1, T_solid=np.nan)):
            src.set_surface_contact(**bad)
            assert not src.surface_contact_on
        src.set_surface_contact(level=0.0, side=-1, T_solid=1500.0)
        src.set_surface_contact(level=0.0, side=3)                        # refused: the earlier configuration stays
        assert src.surface_contact_on
        L.ParticleContextCopy(dst.ctx, src.ctx)
        L.ParticleContextCopy(lone.ctx, src.ctx)
        assert dst.surface_contact_on and not lone.surface_contact_on
        w_d = api.DeviceArray.from_numpy(w0)
        for pc in (src, dst):
            pc.fluid_step(w_d)
        assert dst.surface_contact_stats() == src.surface_contact_stats() and src.surface_contact_stats()["last"] > 0
        assert np.array_equal(src.arrays()[1], dst.arrays()[1])
        src.couple(P2, **GAS)                                             # another mesh: the configuration stays
        assert src.surface_contact_on
        x3 = kuhn_cube(3).xg.reshape(-1, 3)
        w3 = np.zeros(6 * len(x3))
        w3[4 * len(x3):5 * len(x3)] = x3[:, 2] - 0.5
        w3[5 * len(x3):] = 300.0
        before = src.surface_contact_stats()["total"]
        src.fluid_step(api.DeviceArray.from_numpy(w3))
        assert src.surface_contact_stats()["total"] > before
        src.couple(None)                                                  # uncoupling frees the state
        assert not src.surface_contact_on and src.surface_contact_stats() == {"last": 0, "buried": 0, "total": 0}
        L.ParticleContextCopy(dst.ctx, src.ctx)                           # src is off now: dst is switched off too
        assert not dst.surface_contact_on
    finally:
        for pc in (src, dst, lone):
            pc.close()
        P.close()
        P2.close()
