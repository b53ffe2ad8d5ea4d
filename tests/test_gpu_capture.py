"""GPU tests of the melt-pool capture (host/capture.c, csrc/k_capture.hip, the <5> node pass of csrc/k_couple.hip; model in
include/dedflow.h "melt-pool capture").  Build-defined: decisions and deposits are compared with tests/capture_model.py
(np.longdouble) on the library's own tets and weights; the compaction, the pending impulse / energy and DflTimeStep's
wiring are compared bit for bit with a second library path that must do the same thing.

Bounds.  A decision cannot be flipped by rounding: every test first asserts in the model that no particle has |c_i| < 1e-9
or |T_f - T_melt| < 1e-6 (c_i and T_f are O(1) and O(1e3), computed in a dozen fp64 operations).  A node's deposit is a sum
of n terms lambda_a x_i; each term carries the roundings of x_i (the interpolation of u_f or T_f, a difference that the
test's velocities and temperatures keep from cancelling, two products), of the product with lambda_a and of the division
by the time window: under 12 eps |term|, plus the n - 1 additions of the fixed-order sum: (n + 12) eps sum |terms|, the form
of test_gpu_heat.py's source bound.  Totals over the N nodes and the P particles: (N + P) eps sum |.|.  With
DFL_CAPTURE_PARITY_LOG set, every comparison appends observed error and bound to that file (profiles/capture_parity.jsonl
is such a log).  All meshes are kuhn_cube(3) or (4), at most 300 particles."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import capture_model as cm
import ref_driver as rd
from dedflow_amd.meshgen import kuhn_cube

pytestmark = pytest.mark.gpu
EPS = cm.EPS
MU_F = 1.0e-2
TIME = 0.05


@pytest.fixture(scope="module")
def api():
    from dedflow_amd import api as A
    A.lib()
    return A


def _log(name, err, bound):
    err, bound = float(err), float(bound)
    path = os.environ.get("DFL_CAPTURE_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"check": name, "error": err, "bound": bound, "ratio": err / bound if bound > 0 else None}) + "\n")
    print(f"capture parity {name}: error {err:.3e} bound {bound:.3e}")
    return err, bound


def _check(name, got, ref, bound):
    """the worst ratio of |got - ref| to a per-entry bound"""
    d = np.abs(np.asarray(got, np.longdouble) - np.asarray(ref, np.longdouble)).reshape(-1)
    bound = np.broadcast_to(np.asarray(bound, float), np.shape(got)).reshape(-1)
    k = int(np.argmax(d / np.maximum(bound, 1e-300)))
    err, b = _log(name, d[k], bound[k])
    assert err <= b, (name, err, b)


def _coord_ptr(pc):
    return pc.ctx.contents.d_arr[0].contents.data


def _set_coord(api, pc, x):
    api.sync()
    api.DeviceArray(3 * pc.P, ptr=_coord_ptr(pc)).upload(np.asarray(x, float).reshape(-1))


def _context(api, m, case, poly, heat=True, dt=1e-4):
    P = api.Problem(m)
    pc = api.Particles(case["pts"].reshape(-1), case["vel"].reshape(-1), case["R"], mass=float(case["mass"]), dt=dt)
    if poly and pc.P:
        pc.set_sizes(case["r"], case["m"])
    pc.couple(P, rho_f=case["rho_f"], mu_f=MU_F)
    if heat:
        pc.set_heat(cp_p=case["cp_p"], T_init=0.0)
        if pc.P:
            pc.set_temperature(case["temp"])
    return P, pc


def _sizes(case, poly):
    return (case["r"], case["m"]) if poly else (case["R"], case["mass"])


def _decision_run(api, poly, side, reach, T_melt, M=3, P=300, heat=True, level=cm.LEVEL, case=None):
    m = kuhn_cube(M)
    case = case or cm.decision_case(m, P)
    w = cm.linear_fields(m.xg)
    Pb, pc = _context(api, m, case, poly, heat)
    try:
        w_d = api.DeviceArray.from_numpy(w)
        pc.set_capture(level=level, side=side, reach=reach, T_melt=T_melt)
        assert pc.capture_on
        tags0 = pc.tags()
        assert np.array_equal(tags0, np.arange(pc.P))
        pc.locate()
        api.sync()
        tet, lam = pc.tet(), pc.barycentric()
        n = pc.capture(w_d)
        api.sync()
        stats = pc.capture_stats()
        out = dict(m=m, case=case, w=w, tet=tet, lam=lam, n=n, stats=stats, tags=pc.tags(), P=pc.P, arrays=pc.arrays(),
                   tet_after=pc.tet())
        q = pc.capture_source(TIME)
        second = pc.capture_source(TIME)
        api.sync()
        out["q"] = [a.numpy() for a in q]
        out["second"] = [a.numpy() for a in second]
        return out
    finally:
        pc.close()
        Pb.close()


def _model(o, poly, side, reach, T_melt, heat=True, level=cm.LEVEL):
    m, case = o["m"], o["case"]
    radius, mass = _sizes(case, poly)
    dec = cm.decide(m.xg, m.ien, o["w"], o["tet"], o["lam"], radius, level, side, reach, T_melt)
    dep = cm.deposits(dec, mass, case["vel"], case["rho_f"], case["cp_p"] if heat else None, case["temp"] if heat else None)
    return dec, dep


def _check_deposits(tag, o, dec, dep):
    m = o["m"]
    N, P = m.num_node, len(dec["c"])
    cap = dec["captured"]
    A, Aa, cnt = cm.node_accumulate(N, m.ien, o["tet"], o["lam"], dep, cap)
    bound = (cnt[:, None] + 12) * EPS * (Aa / TIME).astype(float) + 1e-300
    got = np.concatenate([o["q"][0][:, None], o["q"][1].reshape(-1, 3), o["q"][2][:, None]], axis=1)
    _check(f"deposit_nodes_{tag}", got, A / TIME, bound)
    assert np.all(got[cnt == 0] == 0.0)
    total = dep.sum(axis=0)
    tot_abs = np.abs(dep).sum(axis=0).astype(float)
    names = ["vol", "mom0", "mom1", "mom2", "heat"]
    for d in range(5):
        s = (got[:, d].astype(np.longdouble) * TIME).sum()
        err, b = _log(f"deposit_total_{names[d]}_{tag}", abs(float(s - total[d])), (N + P) * EPS * tot_abs[d] + 1e-300)
        assert err <= b
    for a in o["second"]:
        assert not a.any()


@pytest.mark.parametrize("poly", [False, True], ids=["mono", "poly"])
@pytest.mark.parametrize("side", [1, -1], ids=["above", "below"])
@pytest.mark.parametrize("reach", [0.0, 1.0], ids=["centre", "touch"])
def test_decisions_and_deposits_match_the_model(api, poly, side, reach):
    """P = 300 (two 256-thread workgroups, the last one partial) on kuhn_cube(3): particle 0 outside the mesh (kept),
    particle 1 on a mesh node, particles 2-4 in one tet, a cold half x < 0.5 where nothing is captured"""
    o = _decision_run(api, poly, side, reach, cm.T_MELT)
    dec, dep = _model(o, poly, side, reach, cm.T_MELT)
    assert cm.margins_ok(dec, cm.T_MELT)
    cap = dec["captured"]
    x = o["case"]["pts"]
    assert o["tet"][0] == -1 and (o["tet"][1:] >= 0).all() and o["tet"][2] == o["tet"][3] == o["tet"][4]
    assert 10 < cap.sum() < 200 and not cap[x[:, 0] < 0.5].any() and (~cap[x[:, 0] > 0.5]).any()
    if side == -1:
        assert cap[1] and cap[2:5].all()
    assert o["n"] == cap.sum() and o["P"] == 300 - cap.sum()
    assert o["stats"] == {"captured": int(cap.sum()), "last": int(cap.sum())}
    assert np.array_equal(o["tags"], np.arange(300)[~cap])                      # the captured set, the survivors' order
    assert o["tags"][0] == 0                                                    # outside the mesh: kept
    keep3 = np.repeat(~cap, 3)
    assert np.array_equal(o["arrays"][0], x.reshape(-1)[keep3])
    assert np.array_equal(o["arrays"][1], o["case"]["vel"].reshape(-1)[keep3])
    assert np.array_equal(o["tet_after"], o["tet"][~cap])
    _check_deposits(f"{'poly' if poly else 'mono'}_{'above' if side == 1 else 'below'}_{'touch' if reach else 'centre'}", o, dec, dep)


def test_no_melting_point_and_heat_off(api):
    """T_melt = -inf captures in the cold half too; with heat off the excess heat is exactly zero"""
    o = _decision_run(api, True, -1, 1.0, -np.inf, heat=False)
    dec, dep = _model(o, True, -1, 1.0, -np.inf, heat=False)
    assert cm.margins_ok(dec, -np.inf)
    cap = dec["captured"]
    assert cap[o["case"]["pts"][:, 0] < 0.5].any() and not cap[0]
    assert o["n"] == cap.sum() and np.array_equal(o["tags"], np.arange(300)[~cap])
    assert not o["q"][2].any()
    _check_deposits("anywhere_heat_off", o, dec, dep)


def test_two_runs_are_bit_identical(api):
    a = _decision_run(api, True, -1, 1.0, cm.T_MELT)
    b = _decision_run(api, True, -1, 1.0, cm.T_MELT)
    assert a["n"] == b["n"] > 0
    for x, y in zip(a["q"], b["q"]):
        assert np.array_equal(x, y) and np.abs(x).max() > 0.0
    for x in a["second"]:
        assert not x.any()


def test_edge_counts(api):
    """P = 0, P = 1 (kept, then captured) and every particle captured (new count 0)"""
    m = kuhn_cube(3)
    empty = dict(cm.decision_case(m, 1), pts=np.zeros((0, 3)), vel=np.zeros((0, 3)))
    o = _decision_run(api, False, -1, 0.0, -np.inf, case=empty)
    assert o["n"] == 0 and o["P"] == 0 and o["stats"] == {"captured": 0, "last": 0}
    assert not any(a.any() for a in o["q"])
    one = cm.decision_case(m, 1)
    for side in (1, -1):
        o = _decision_run(api, False, side, 0.0, -np.inf, case=one)
        dec, dep = _model(o, False, side, 0.0, -np.inf)
        assert cm.margins_ok(dec, -np.inf) and o["tet"][0] >= 0
        assert o["n"] == int(dec["captured"][0]) and o["P"] == 1 - o["n"]
        _check_deposits(f"one_particle_side{side}", o, dec, dep)
    case = cm.decision_case(m, 300)
    case["pts"][0] = (0.5, 0.5, 0.5)                                            # nobody outside the mesh
    o = _decision_run(api, True, -1, 0.0, -np.inf, level=10.0, case=case)       # phi < 10 everywhere
    dec, dep = _model(o, True, -1, 0.0, -np.inf, level=10.0)
    assert cm.margins_ok(dec, -np.inf) and dec["captured"].all()
    assert o["n"] == 300 and o["P"] == 0 and len(o["tags"]) == 0
    _check_deposits("all_captured", o, dec, dep)


def _history(pc):
    keys, xi, cnt = pc.friction_history()
    return [(keys[i, :cnt[i]].copy(), xi[i, :cnt[i]].copy()) for i in range(pc.P)], cnt


def _survivor_state(api, pc):
    api.sync()
    hist, cnt = _history(pc)
    return dict(tags=pc.tags(), arrays=pc.arrays(), omega=pc.omega(), T=pc.temperature(), e=pc._pending_energy(),
                r=pc.radii(), mass=pc.masses(), hist=hist, cnt=cnt, tet=pc.tet(), lam=pc.barycentric())


def _survivor_run(api, capture):
    """a polydisperse lattice with friction and heat, three coupled sub-steps (history, pending impulse and energy), then
    either capture() or, in the twin, the same particles moved beyond an outflow plane and remove()"""
    m = kuhn_cube(3)
    rng = np.random.default_rng(17)
    R = 0.03
    g = 0.56 - 1.9 * R * np.arange(3)                      # z = 0.56 (above the surface, kept), 0.503, 0.446 (captured)
    gx = 0.55 + 1.9 * R * np.arange(6)
    gy = 0.2 + 1.9 * R * np.arange(6)
    pts = np.stack(np.meshgrid(gx, gy, g, indexing="ij"), axis=-1).reshape(-1, 3) + rng.uniform(-0.02 * R, 0.02 * R, (108, 3))
    case = dict(cm.decision_case(m, 108), pts=pts, vel=rng.normal(scale=0.2, size=pts.shape), R=R)
    case["r"] = rng.uniform(0.95 * R, R, 108)
    case["m"] = 7800.0 * 4.0 / 3.0 * np.pi * case["r"] ** 3
    case["mass"] = 7800.0 * 4.0 / 3.0 * np.pi * R ** 3
    w = cm.linear_fields(m.xg)
    Pb, pc = _context(api, m, case, True, dt=1e-5)
    try:
        pc.set_friction(0.4)
        w_d = api.DeviceArray.from_numpy(w)
        if capture:
            pc.set_capture(level=cm.LEVEL, side=-1, reach=0.0, T_melt=cm.T_MELT)
        else:
            pc.set_outflow(planes=[(0.0, 0.0, 1.0, 5.0)])
        for _ in range(3):
            pc.fluid_step(w_d)
        pc.locate()
        before = _survivor_state(api, pc)
        dec = cm.decide(m.xg, m.ien, w, before["tet"], before["lam"], case["r"], cm.LEVEL, -1, 0.0, cm.T_MELT)
        assert cm.margins_ok(dec, cm.T_MELT)
        cap = dec["captured"]
        if capture:
            n = pc.capture(w_d)
        else:
            x = before["arrays"][0].reshape(-1, 3).copy()
            x[cap, 2] += 10.0
            _set_coord(api, pc, x)
            pc.remove()
            n = 108 - pc.P
        after = _survivor_state(api, pc)
        load = pc.reaction_load().numpy()
        src = pc.heat_source().numpy()
        api.sync()
        return dict(before=before, after=after, cap=cap, n=n, load=load, src=src)
    finally:
        pc.close()
        Pb.close()


def test_survivors_and_pending_equal_a_remove_of_the_same_particles(api):
    a = _survivor_run(api, True)
    b = _survivor_run(api, False)
    cap = a["cap"]
    assert np.array_equal(cap, b["cap"]) and 0 < cap.sum() < 108 and a["n"] == b["n"] == cap.sum()
    # the state before is the same in both, with something pending and a history pair whose partner gets captured
    assert np.abs(a["before"]["e"][cap]).min() > 0.0
    partners = [(i, int(k)) for i in np.nonzero(~cap)[0] for k in a["before"]["hist"][i][0] if (int(k) >> 62) == 0]
    assert any(cap[j] for _, j in partners) and any(not cap[j] for _, j in partners)
    sa, sb = a["after"], b["after"]
    assert np.array_equal(sa["tags"], a["before"]["tags"][~cap])
    for k in ("tags", "omega", "T", "e", "r", "mass", "cnt", "tet", "lam"):
        assert np.array_equal(sa[k], sb[k]), k
    for x, y in zip(sa["arrays"], sb["arrays"]):
        assert np.array_equal(x, y)
    for k in ("T", "e", "r", "mass"):
        assert np.array_equal(sa[k], a["before"][k][~cap]), k
    newid = np.cumsum(~cap) - 1
    for j, i in enumerate(np.nonzero(~cap)[0]):
        ka, xa = sa["hist"][j]
        kb, xb = sb["hist"][j]
        assert np.array_equal(ka, kb) and np.array_equal(xa, xb)
        k0, x0 = a["before"]["hist"][i]
        live = np.array([(int(k) >> 62) != 0 or not cap[int(k)] for k in k0], bool)
        want = np.array([int(k) if (int(k) >> 62) else newid[int(k)] for k in k0[live]], np.uint64)
        assert np.array_equal(ka, want) and np.array_equal(xa, x0[live])
    # what was pending on the captured particles goes where Remove sends it: the next load and source, bit for bit
    assert np.array_equal(a["load"], b["load"]) and np.abs(a["load"]).max() > 0.0
    assert np.array_equal(a["src"], b["src"]) and np.abs(a["src"]).max() > 0.0


def test_volume_source_enters_the_p_rows(api):
    from dedflow_amd.meshgen import synthetic_fields
    m = kuhn_cube(4, jitter=0.2)
    N = m.num_node
    wg, dwg = synthetic_fields(m)
    P = api.Problem(m)
    try:
        wg_d, dwg_d = api.DeviceArray.from_numpy(wg), api.DeviceArray.from_numpy(0.1 * dwg)
        F = [api.DeviceArray(6 * N) for _ in range(3)]
        P.assemble_system(wg_d, dwg_d, F[0])
        api.sync()
        f0 = F[0].numpy()
        q = np.random.default_rng(3).normal(scale=np.abs(f0[3 * N:4 * N]).max(), size=N)
        assert P.volume_source() is None
        P.set_volume_source(api.DeviceArray.from_numpy(q))
        assert np.array_equal(P.volume_source(), q)
        P.assemble_system(wg_d, dwg_d, F[1])
        P.set_volume_source(None)
        assert P.volume_source() is None
        P.assemble_system(wg_d, dwg_d, F[2])
        api.sync()
        f1, f2 = F[1].numpy(), F[2].numpy()
        assert np.array_equal(f0, f2)
        assert np.array_equal(f1[3 * N:4 * N], f0[3 * N:4 * N] - q) and np.abs(q).max() > 0.0
        assert np.array_equal(f1[:3 * N], f0[:3 * N]) and np.array_equal(f1[4 * N:], f0[4 * N:])
        held = 0
        for group, types in api.REFERENCE_BCS:                 # the strong rows stay exactly zero
            nodes = m.bound_node[m.bound_node_offset[group]:m.bound_node_offset[group + 1]]
            for d, t in enumerate(types):
                if t == api.BC_STRONG:
                    assert not f0[3 * nodes + d].any() and not f1[3 * nodes + d].any()
                    held += len(nodes)
        assert held > 0
    finally:
        P.close()


STEP_R = 0.01
STEP_MASS = 7800.0 * 4.0 / 3.0 * np.pi * STEP_R ** 3


def _step_setup(api, m, two_way_coupling=False, heat=None):
    """fluid at rest and hot everywhere, phi = z - 0.5; six particles that cross z = 0.5 within one step's sub-steps, six
    that do not"""
    N = m.num_node
    w0 = np.zeros(6 * N)
    w0[4 * N:5 * N] = m.xg.reshape(-1, 3)[:, 2] - 0.5
    w0[5 * N:] = 2000.0
    xy = np.array([[0.3, 0.3], [0.5, 0.3], [0.7, 0.3], [0.3, 0.6], [0.5, 0.6], [0.7, 0.62]]) + 0.013
    pts = np.concatenate([np.c_[xy, np.full(6, 0.508)], np.c_[xy, np.full(6, 0.62)]])
    vel = np.tile([0.0, 0.0, -1.0], (12, 1))
    P = api.Problem(m, maxit=120, atol=1e-14, rtol=1e-6)
    pc = api.Particles(pts.reshape(-1), vel.reshape(-1), STEP_R, mass=STEP_MASS, dt=1e-3)
    pc.couple(P, rho_f=1.0e3, mu_f=1.0e-3, two_way=two_way_coupling)
    if heat is not None:                                        # heat: the two_way flag of the particle heat
        P.set_scalar_transport(phi=False, T=True)
        pc.set_heat(cp_p=500.0, T_init=3000.0, two_way=heat)
    st = [api.DeviceArray.from_numpy(a) for a in (w0, np.zeros(6 * N), np.zeros(6 * N))]
    return P, pc, st, api.DeviceArray(6 * N), api.DeviceArray(6 * N)


def _registrations(api, P):
    L = api.lib()
    L.DflMeshExternalLoad.restype = C.c_void_p
    L.DflMeshExternalLoad.argtypes = [C.POINTER(api.Mesh3D)]
    L.DflMeshHeatSource.restype = C.c_void_p
    L.DflMeshHeatSource.argtypes = [C.POINTER(api.Mesh3D)]
    return L.DflMeshExternalLoad(P.mesh), L.DflMeshHeatSource(P.mesh), L.DflMeshVolumeSource(P.mesh)


def test_time_step_puts_the_deposits_on_the_rows(api):
    """step 1 captures; step 2 of the two-way context must see exactly what a one-way context sees when the caller takes
    the source with time = kDT and registers it by hand; a context that registers nothing sees a zero residual"""
    m = kuhn_cube(4)
    N = m.num_node
    K = 20
    runs = {}
    for mode in ("two_way", "by_hand", "nothing", "never_set"):
        P, pc, st, F_d, dx_d = _step_setup(api, m)
        try:
            if mode != "never_set":
                pc.set_capture(level=0.0, side=-1, reach=0.0, T_melt=1500.0, two_way=(mode == "two_way"))
            P.time_step(st[0], st[1], st[2], F_d, dx_d, newton_maxit=2, particles=pc, dem_substeps=K)
            api.sync()
            o = dict(P1=pc.P, stats=pc.capture_stats(), tags=pc.tags(), w1=st[0].numpy())
            if mode == "never_set":                              # the state the capture of step 1 saw, and the model's count
                pc.locate()
                api.sync()
                dec = cm.decide(m.xg, m.ien, o["w1"], pc.tet(), pc.barycentric(), STEP_R, 0.0, -1, 0.0, 1500.0)
                assert cm.margins_ok(dec, 1500.0)
                o.update(dec=dec, vel=pc.arrays()[1].reshape(-1, 3), tet=pc.tet(), lam=pc.barycentric())
            else:
                if mode == "by_hand":
                    q = pc.capture_source(rd.kDT)
                    P.set_volume_source(q[0])
                    P.set_external_load(q[1])
                    o["q"] = [a.numpy() for a in q]
                it, rn, r0 = P.time_step(st[0], st[1], st[2], F_d, dx_d, newton_maxit=2, particles=pc, dem_substeps=K)
                api.sync()
                if mode == "by_hand":
                    P.set_volume_source(None)
                    P.set_external_load(None)
                o.update(r0=r0, rn=rn, regs=_registrations(api, P), w2=st[0].numpy(), x2=pc.arrays()[0], P2=pc.P)
            runs[mode] = o
        finally:
            pc.close()
            P.close()
    ref = runs["never_set"]
    cap = ref["dec"]["captured"]
    assert cap.sum() == 6 and np.array_equal(cap, np.arange(12) < 6)
    assert not ref["w1"][:4 * N].any()                                            # the fluid was at rest through step 1
    for mode in ("two_way", "by_hand", "nothing"):
        o = runs[mode]
        assert o["stats"]["captured"] == 6 and o["P1"] == 6 and np.array_equal(o["tags"], np.arange(12)[~cap])
        assert np.array_equal(o["w1"], ref["w1"])
        assert o["regs"] == (None, None, None), mode                               # restored after the solve
    a, b, c = runs["two_way"], runs["by_hand"], runs["nothing"]
    assert np.array_equal(a["r0"], b["r0"]) and np.array_equal(a["rn"], b["rn"]) and np.array_equal(a["w2"], b["w2"])
    assert np.array_equal(a["x2"], b["x2"]) and a["P2"] == b["P2"]
    assert c["r0"][0] == 0.0 and c["r0"][1] == 0.0 and a["r0"][1] > 0.0 and a["r0"][0] > 0.0
    # the p rows of the first F assembly of step 2 carry A / kDT: the model's volume rate, node by node and in norm
    dep = cm.deposits(ref["dec"], STEP_MASS, ref["vel"], 1.0e3)
    A, Aa, cnt = cm.node_accumulate(N, m.ien, ref["tet"], ref["lam"], dep, cap)
    _check("step_q_vol", b["q"][0], A[:, 0] / rd.kDT, (cnt + 12) * EPS * (Aa[:, 0] / rd.kDT).astype(float) + 1e-300)
    _check("step_load", b["q"][1].reshape(-1, 3), A[:, 1:4] / rd.kDT,
           (cnt[:, None] + 12) * EPS * (Aa[:, 1:4] / rd.kDT).astype(float) + 1e-300)
    norm = float(np.sqrt((b["q"][0].astype(np.longdouble) ** 2).sum()))
    err, bd = _log("step_rnorm_p", abs(a["r0"][1] - norm), (N + 8) * EPS * norm)
    assert err <= bd
    total = float((b["q"][0].astype(np.longdouble) * rd.kDT).sum())
    err, bd = _log("step_volume", abs(total - 6 * STEP_MASS / 1.0e3), (N + 12) * EPS * 6 * STEP_MASS / 1.0e3)
    assert err <= bd


def test_time_step_merges_a_pending_reaction_load_and_heat_source(api):
    """two-way coupling, two-way particle heat and two-way capture, T transported: in step 2 the reaction load and the
    particle heat source of step 1's sub-steps are pending next to the deposits.  DflTimeStep must register capture + reaction
    and capture + heat; a context with all three one-way, whose caller takes the three sources, adds them and registers the
    sums, must see the same step bit for bit"""
    m = kuhn_cube(4)
    N = m.num_node
    K = 20
    runs = {}
    for mode in ("two_way", "by_hand"):
        on = mode == "two_way"
        P, pc, st, F_d, dx_d = _step_setup(api, m, two_way_coupling=on, heat=on)
        try:
            pc.set_capture(level=0.0, side=-1, reach=0.0, T_melt=1500.0, two_way=on)
            P.time_step(st[0], st[1], st[2], F_d, dx_d, newton_maxit=2, particles=pc, dem_substeps=K)
            api.sync()
            o = dict(P1=pc.P, w1=st[0].numpy())
            if not on:
                q = [a.numpy() for a in pc.capture_source(rd.kDT)]
                load, src = pc.reaction_load().numpy(), pc.heat_source().numpy()
                assert np.abs(load).max() > 0.0 and np.abs(src).max() > 0.0 and np.abs(q[1]).max() > 0.0 and np.abs(q[2]).max() > 0.0
                P.set_volume_source(api.DeviceArray.from_numpy(q[0]))
                P.set_external_load(api.DeviceArray.from_numpy(q[1] + load))
                P.set_heat_source(api.DeviceArray.from_numpy(q[2] + src))
                o.update(q=q, load=load, src=src)
            it, rn, r0 = P.time_step(st[0], st[1], st[2], F_d, dx_d, newton_maxit=2, particles=pc, dem_substeps=K)
            api.sync()
            if not on:
                P.set_volume_source(None)
                P.set_external_load(None)
                P.set_heat_source(None)
            o.update(r0=r0, rn=rn, regs=_registrations(api, P), w2=st[0].numpy(), dw2=st[2].numpy(), x2=pc.arrays()[0],
                     T2=pc.temperature(), P2=pc.P)
            runs[mode] = o
        finally:
            pc.close()
            P.close()
    a, b = runs["two_way"], runs["by_hand"]
    assert a["P1"] == b["P1"] == 6 and np.array_equal(a["w1"], b["w1"])
    assert a["regs"] == (None, None, None)                                         # all three restored after the solve
    for k in ("r0", "rn", "w2", "dw2", "x2", "T2"):
        assert np.array_equal(a[k], b[k]), k
    assert a["P2"] == b["P2"] and a["r0"][0] > 0.0 and a["r0"][1] > 0.0 and a["r0"][3] > 0.0
    # the T rows carry capture + particle heat: the norm of the by-hand sum (no Dirichlet group holds T here)
    norm = float(np.sqrt(((b["q"][2] + b["src"]).astype(np.longdouble) ** 2).sum()))
    err, bd = _log("step_rnorm_T_merged", abs(a["r0"][3] - norm), (N + 8) * EPS * norm)
    assert err <= bd


def test_capture_that_never_fires_changes_nothing(api):
    """capture set with T_melt = +inf against capture never set: three DflTimeSteps, friction, sizes and heat on, one-way"""
    from dedflow_amd.meshgen import synthetic_fields
    m = kuhn_cube(4, jitter=0.2)
    N = m.num_node
    wg, dw0 = synthetic_fields(m)
    wg[3 * N:4 * N] = 0.0
    rng = np.random.default_rng(81)
    g = np.linspace(0.3, 0.7, 5)
    R = 0.05
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) + rng.uniform(-0.004, 0.004, (125, 3))
    v = rng.normal(scale=0.3, size=pts.shape)
    r = rng.uniform(0.85 * R, R, len(pts))
    mass = lambda a: 2000.0 * 4.0 / 3.0 * np.pi * np.asarray(a) ** 3
    out = []
    for on in (True, False):
        P = api.Problem(m, maxit=120, atol=1e-12, rtol=1e-4)
        pc = api.Particles(pts.reshape(-1), v.reshape(-1), R, mass=float(mass(R)), dt=1e-3)
        try:
            pc.set_sizes(r, mass(r))
            pc.set_friction(0.4)
            pc.couple(P)
            pc.set_heat(cp_p=500.0, k_p=40.0, T_init=1200.0)
            if on:
                pc.set_capture(level=0.0, side=1, reach=1.0, T_melt=np.inf, two_way=True)
                assert pc.capture_on
            st = [api.DeviceArray.from_numpy(a) for a in (wg, 0.1 * dw0, 0.1 * dw0)]
            F_d, dx_d = api.DeviceArray(6 * N), api.DeviceArray(6 * N)
            norms = []
            for _ in range(3):
                norms.append(P.time_step(st[0], st[1], st[2], F_d, dx_d, newton_maxit=2, particles=pc, dem_substeps=4))
            api.sync()
            if on:
                assert pc.capture_stats() == {"captured": 0, "last": 0} and pc.P == 125
            out.append((pc.arrays() + (pc.omega().reshape(-1), pc.temperature(), pc._pending_energy()),
                        [s.numpy() for s in st], norms))
        finally:
            pc.close()
            P.close()
    (pa, fa, na), (pb, fb, nb) = out
    for x, y in zip(pa, pb):
        assert np.array_equal(x, y)
    for x, y in zip(fa, fb):
        assert np.array_equal(x, y)
    for (ia, ra, r0a), (ib, rb, r0b) in zip(na, nb):
        assert ia == ib and np.array_equal(ra, rb) and np.array_equal(r0a, r0b)
    assert np.abs(pa[3]).max() > 0.0                                              # contacts happened


def test_refused_configurations_leave_the_context_unchanged(api, capfd):
    m = kuhn_cube(3)
    case = cm.decision_case(m, 12)
    P = api.Problem(m)
    pc = api.Particles(case["pts"].reshape(-1), case["vel"].reshape(-1), case["R"], mass=float(case["mass"]))
    try:
        pc.set_capture(level=0.0, side=1)                                         # not coupled
        assert not pc.capture_on and "not coupled" in capfd.readouterr().err
        pc.couple(P)
        pc.set_capture(level=0.0, side=0)
        assert not pc.capture_on and "side" in capfd.readouterr().err
        pc.set_capture(level=0.0, side=1, reach=-0.5)
        assert not pc.capture_on and "reach" in capfd.readouterr().err
        assert pc.tags() is None and pc.capture_stats() == {"captured": 0, "last": 0}
        pc.set_capture(level=0.0, side=1, reach=0.5)
        assert pc.capture_on and capfd.readouterr().err == ""
        pc.set_capture(level=0.0, side=2)                                         # refused: the earlier configuration stays
        assert pc.capture_on
        pc.set_capture(level=None)
        assert not pc.capture_on
    finally:
        pc.close()
        P.close()
