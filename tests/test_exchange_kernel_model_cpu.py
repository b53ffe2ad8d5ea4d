"""CPU checks of tests/exchange_kernel_model.py, the model behind test_gpu_exchange_kernels.py: its restatements pinned to the
models the suite already has (coupling_model, heat_model, capture_model, surface_contact_model), the constants c (float64
restatement against np.longdouble relative to u A: measured here, never on a kernel), the walk's acceptance rule on a
coordinate that is not finite, and the margins and BFS distances the GPU cases rely on.  No GPU."""
import json
import os

import numpy as np
import pytest

import capture_model as cm
import coupling_model as cpm
import exchange_kernel_model as X
import heat_model as hm
import surface_contact_model as scm

F64, LD, I64 = np.float64, np.longdouble, np.int64
needs_ld = pytest.mark.skipif(not X.HAVE_EXTENDED, reason=X.EXTENDED_REASON)


def _write_c(name, c):
    out = os.environ.get("DFL_PARITY_OUT")
    if out:
        with open(out, "a") as fh:
            fh.write(json.dumps({"kernel": "restatement", "case": name, "c": np.atleast_1d(c).tolist()}) + "\n")


def _pin(name, c):
    c = np.atleast_1d(np.asarray(c, float))
    print(name, "c =", c)
    assert np.all(np.isfinite(c)) and np.all(c > 0), (name, c)
    assert np.all(c <= 16), "%s: c = %s: the abs-sum A is missing a term" % (name, c)
    _write_c(name, c)


# ---- integers --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,jitter", X.CUBES)
def test_v2e_and_neighbours_on_cubes(M, jitter):
    m = X.kuhn(M, jitter)
    vrow, vcol = m.v2e()
    for a in range(m.N):
        assert vcol[vrow[a]:vrow[a + 1]].tolist() == sorted(t for t in range(m.T) if a in m.ien[t])
    s = X.scramble(vrow, vcol)
    assert not np.array_equal(s, vcol)
    assert all(sorted(s[vrow[a]:vrow[a + 1]]) == vcol[vrow[a]:vrow[a + 1]].tolist() for a in range(m.N))
    nbr = m.nbr()
    assert (nbr < 0).sum() == 12 * M * M                      # two boundary triangles per cell face
    t, k = np.nonzero(nbr >= 0)
    assert all(t[i] in nbr[nbr[t[i], k[i]]] for i in range(len(t))), "not symmetric on a conforming mesh"
    for i in range(0, len(t), 7):                             # the neighbour shares exactly the face
        assert len(set(m.ien[t[i]]) & set(m.ien[nbr[t[i], k[i]]])) == 3 and m.ien[t[i], k[i]] not in m.ien[nbr[t[i], k[i]]]
    assert X.bfs(nbr).min() == 0 and X.bfs(nbr).max() > 0


def test_fan_lowest_id_wins():
    m = X.fan()
    nbr = m.nbr()
    assert nbr[0].tolist() == [-1, -1, -1, 1] and nbr[1].tolist() == [-1, -1, -1, 0] and nbr[2].tolist() == [-1, -1, -1, 0]
    x4 = m.x[m.ien]
    vol = np.einsum("nd,nd->n", np.cross(x4[:, 1] - x4[:, 0], x4[:, 2] - x4[:, 0]), x4[:, 3] - x4[:, 0])
    assert np.all(vol > 0)


def test_sort_by_tet():
    tet = np.array([3, -1, 0, 3, -2, 3, 0])
    start, members = X.sort_by_tet(tet, 5)
    assert start.tolist() == [0, 2, 2, 2, 5, 5] and members.tolist() == [2, 6, 0, 3, 5]


def test_mix32():
    # the two multipliers of the 32-bit mixer are odd: the map is a bijection, so 0 is its only fixed zero
    assert X.mix32([0])[0] == 0 and len(set(X.mix32(np.arange(4096)).tolist())) == 4096
    assert X.mix32([1])[0] == ((((1 * 0x7FEB352D) & 0xFFFFFFFF) ^ (((1 * 0x7FEB352D) & 0xFFFFFFFF) >> 15)) * 0x846CA68B & 0xFFFFFFFF) ^ \
        ((((((1 * 0x7FEB352D) & 0xFFFFFFFF) ^ (((1 * 0x7FEB352D) & 0xFFFFFFFF) >> 15)) * 0x846CA68B) & 0xFFFFFFFF) >> 16)


def test_grid_coord():
    got = X.grid_coord([-np.inf, -0.1, 0.0, 0.49, 0.5, 0.99, 1.0, 7.0, np.inf, np.nan], 0.0, 2.0, 2)
    assert got.tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 1, 0]


# ---- point location --------------------------------------------------------------------------------------------------
@needs_ld
def test_barycentric_is_the_coupling_model():
    m = X.kuhn(3, 0.2)
    pts, t = X.interior_points(m, 300, 1)
    lam, A = X.barycentric(m.x[m.ien[t]], pts, F64)
    ref = cpm.barycentric(m.x, m.ien, t, pts)
    assert np.all(np.abs(lam - ref) <= 8 * X.U * A.astype(F64))
    assert np.all(lam.min(axis=1) >= -1e-12) and np.all(np.abs(lam.sum(axis=1) - 1) < 1e-14)
    _pin("couple_locate:lambda", X.c_lambda())


@pytest.mark.parametrize("M,jitter", X.CUBES)
def test_walk_finds_what_brute_force_finds(M, jitter):
    m = X.kuhn(M, jitter)
    pts = np.vstack([X.interior_points(m, 257, 2, clear=1e-6)[0], X.outside_points(60, 3)])
    seed, lo, inv_h = X.seed_grid(m, 2)
    ref = X.brute(m, pts)[0]
    far = np.full(len(pts), m.T - 1)
    for start in (X.seed_start(pts, np.full(len(pts), -1), seed, lo, inv_h, 2), np.where(ref >= 0, ref, 0), far):
        w = X.walk(m, pts, start)
        assert np.array_equal(w.tet, ref) and w.margin.min() >= 1e-9 and w.steps.max() < 8 * M
        assert np.all(w.lam[ref < 0] == 0) and np.all(w.lam[ref >= 0].min(axis=1) >= -1e-12)
    assert (ref < 0).sum() == 60


@pytest.mark.parametrize("M,jitter", X.CUBES)
def test_location_families_have_the_margins_the_gpu_test_relies_on(M, jitter):
    """every particle with a unique tet is decided with a margin of 1e-9 on every step of the walk from every start, so
    rounding and contraction cannot change its tet; the walks agree with brute force; the shared points are located too"""
    m = X.kuhn(M, jitter)
    pts, unique, clear_t = X.locate_points(m)
    assert len(pts) == 513
    ref = X.brute(m, pts)[0]
    assert np.array_equal(ref[150:300], clear_t) and np.all(ref[400:460] == -1) and np.all(ref[460:] == m.T // 2)
    assert np.all(ref[:400] >= 0)
    seed, lo, inv_h = X.seed_grid(m, 2)
    for start in (X.seed_start(pts, np.full(513, -1), seed, lo, inv_h, 2), np.full(513, m.T - 1), np.zeros(513, I64)):
        w = X.walk(m, pts, start)
        assert np.array_equal(w.tet[unique], ref[unique]) and w.margin[unique].min() >= 1e-9
        assert np.all(w.tet[~unique] >= 0) and np.all(w.tet >= -1)


def test_fmin_accepts_a_point_at_infinity_and_the_fixed_rule_does_not():
    """the defect the acceptance rule had: on an axis-aligned tet a coordinate at +inf gives lambda = [nan, inf, nan, nan]
    (inf * 0), fmin drops the NaNs, and the tet is accepted.  Each lambda compared on its own refuses it"""
    m = X.kuhn(2)
    pts = np.array([[np.inf, 0.3, 0.2], [0.3, 0.3, 0.2], [0.3, -np.inf, 0.2], [0.1, 0.2, np.nan], [np.inf, np.nan, 0.5], [-np.inf, np.inf, 0.5]])
    start = np.zeros(len(pts), I64)
    old, new = X.walk(m, pts, start, rule="fmin"), X.walk(m, pts, start, rule="each")
    assert old.tet[0] >= 0 and np.isnan(old.lam[0]).sum() == 3 and np.isinf(old.lam[0]).sum() == 1, (old.tet, old.lam[0])
    assert new.tet.tolist() == [-1, old.tet[1], -1, -1, -1, -1] and old.tet[1] >= 0
    assert np.all(new.lam[[0, 2, 3, 4, 5]] == 0) and np.array_equal(new.lam[1], old.lam[1])
    assert np.all(new.steps[[0, 2, 3, 4, 5]] == 1)            # refused in the first tet: no walk on inf or NaN lambdas
    for M, j in X.CUBES:                                      # finite points: the two rules decide and write the same
        mm = X.kuhn(M, j)
        p = np.vstack([X.interior_points(mm, 200, 5)[0], X.shared_points(mm, 100, 6), X.outside_points(60, 7)])
        a, b = X.walk(mm, p, np.zeros(len(p), I64), rule="fmin"), X.walk(mm, p, np.zeros(len(p), I64), rule="each")
        assert np.array_equal(a.tet, b.tet) and np.array_equal(a.lam.view(np.uint64), b.lam.view(np.uint64))


def test_strip_bfs_and_walk():
    """what the cap cases rely on: the BFS distance from tet 0 grows by 3 per cube and reaches 4498; the walk from tet 0
    takes the BFS distance + 1 evaluations, with wide margins"""
    m = X.strip()
    assert m.T == 9000
    d = X.bfs(m.nbr())
    assert d.max() == 4498 and d.min() == 0
    cube_min = d.reshape(-1, 6).min(axis=1)
    assert np.all(np.diff(cube_min)[1:] == 3)      # (1 for the first cube, whose tet 0 is the start)
    pts, tet, must_find, must_lose = X.strip_particles()
    w = X.walk(m, pts, np.zeros(len(pts), I64))
    found = w.tet >= 0
    assert np.array_equal(w.tet[found], tet[found]) and np.all(w.tet[~found] == -2)
    assert np.array_equal(w.steps[found], d[tet[found]] + 1) and w.margin.min() >= 1e-3
    assert must_find.sum() >= 50 and must_lose.sum() >= 50 and (~must_find & ~must_lose).sum() >= 10
    assert np.all(found[must_find]) and not found[must_lose].any()
    assert np.all(w.steps[must_find] <= X.MAX_WALK - 64) and np.all(d[tet[must_lose]] >= X.MAX_WALK)


# ---- the float laws against the models the suite has --------------------------------------------------------------------
@needs_ld
def test_fluid_step_is_the_coupling_model():
    for name in X.FLUID_CASES:
        k = X.fluid_case(name)
        got = X.fluid_run(k, F64, False)
        inside = k.tet >= 0
        uf = cpm.interpolate(k.w, k.mesh.ien, np.maximum(k.tet, 0), k.lam)
        x, v, a, imp = cpm.drag_step(k.coord, k.vel, k.acc, uf, inside, k.M, k.R, k.dt, k.rho_f, k.mu_f, k.g)
        for g, r, A in ((got.vel, v, got.A_vel), (got.coord, x, got.A_coord), (got.acc, a, got.A_acc), (got.imp - k.imp, imp, got.A_imp)):
            assert np.all(np.abs(g - r) <= 64 * X.U * A.astype(F64)), name
        ld = X.fluid_run(k, LD, False)
        if name == "re0":
            assert np.all(ld.re[inside] == 0) and np.all(got.re[inside] == 0)
        if name in ("low", "high"):
            for poly in (False, True):
                re = X.fluid_run(k, LD, poly).re[inside]
                assert np.all(np.abs(re - 1000.0) >= 1e-6 * 1000.0)
        if name == "high":
            re = X.fluid_run(k, LD, True).re[inside]
            assert (re > 1000).any() and (re < 1000).any()
    assert np.isclose(X.fluid_case("stiff").dt / cpm.response_time(X.fluid_case("stiff").M, X.FLUID["R"], X.FLUID["mu_f"]), 1e6)
    assert np.isclose(X.fluid_case("slack").dt / cpm.response_time(X.fluid_case("slack").M, X.FLUID["R"], X.FLUID["mu_f"]), 1e-6)
    c = X.c_fluid()
    for k, name in enumerate(("vel", "coord", "acc", "imp")):
        _pin("couple_fluid_step:" + name, c[k])
    cp = X.c_pow()
    _pin("couple_fluid_step:pow", cp)
    assert cp <= 2.0


@needs_ld
def test_poly_with_equal_sizes_is_mono():
    k = X.fluid_case("low")
    a, b = X.fluid_run(k, LD, False), X.fluid_run(k, LD, True, same_size=True)
    assert all(np.array_equal(a[q], b[q]) for q in ("vel", "coord", "acc", "imp"))


@needs_ld
def test_heat_update_is_the_heat_model():
    k = X.heat_case()
    for poly in (False, True):
        got = X.heat_run(k, LD, poly, False)
        m, r = (k.m, k.r) if poly else (k.M, k.R)
        Tf, re, nu, tau, loc = hm.convection(k.w, k.mesh.N, k.mesh.ien, k.tet, np.where((k.tet >= 0)[:, None], k.lam, 0), k.vel, m, r,
                                             X.HEAT["cp_p"], k.dt, X.HEAT["rho_f"], X.HEAT["mu_f"], X.HEAT["k_f"], 1.0)
        Tn, rate, e = hm.update(k.temp, k.q, np.asarray(m, LD) * X.HEAT["cp_p"], k.dt, Tf, tau, loc)
        assert np.allclose(got.temp.astype(float), Tn.astype(float), rtol=1e-13, atol=0)
        assert np.allclose(got.rate.astype(float), rate.astype(float), rtol=1e-9, atol=1e-12 * np.abs(rate).max())
        assert np.allclose((got.e - k.e0).astype(float), e.astype(float), rtol=1e-9, atol=1e-12 * np.abs(e).max())
    zero = X.heat_run(k, F64, False, True, dt=0.0)
    assert np.array_equal(zero.temp, k.temp) and np.all(zero.rate == 0) and np.array_equal(zero.e, k.e0)
    unc = X.heat_run(k, LD, False, False, coupled=False)
    assert np.array_equal(unc.e, k.e0)
    c = X.c_heat()
    for j, name in enumerate(("temp", "rate", "e")):
        _pin("heat_update:" + name, c[j])


@needs_ld
def test_conduction_is_the_heat_model():
    for poly in (False, True):
        k = X.conduction_case(poly)
        pairs = hm.contacts_all_pairs(k.x, k.r)
        q, A, delta = X.conduction(LD, k.x, k.r, k.T, k.k_p, pairs)
        ref = hm.conduction(k.x, k.r, k.T, k.k_p, pairs)
        assert np.all(np.abs(q - ref[0]) <= 64 * X.U * A)
        cnt = ref[2]
        assert (cnt == 1).sum() >= 20 and (cnt >= 2).sum() >= 10 and (cnt == 0).sum() >= 20
        assert delta.min() >= 1e-9 * k.R                       # no contact about to open
        cells = hm.contacts_cell_list(k.x, k.r, 1.0 / k.ncell)
        assert np.array_equal(cells[0], pairs[0]) and np.array_equal(cells[1], pairs[1])
    _pin("heat_conduction", X.c_conduction())


@needs_ld
def test_capture_flag_is_the_capture_model():
    for poly in (False, True):
        k = X.capture_case(poly)
        m, r = (k.m, k.r) if poly else (k.M, k.R)
        dec = cm.decide(k.mesh.x, k.mesh.ien, k.w, k.tet, k.lam, r, cm.LEVEL, 1.0, 2.0, cm.T_MELT)
        assert cm.margins_ok(dec, cm.T_MELT)
        dep = cm.deposits(dec, m, k.vel, k.rho_f, k.cp_p, k.temp)
        for dt in (LD, F64):
            got = X.capture_flag(dt, k.mesh, k.w, k.tet, k.lam, k.vel, k.temp, m, r, k.rho_f, k.cp_p, cm.LEVEL, 1.0, 2.0, cm.T_MELT)
            assert np.array_equal(got.captured, dec["captured"])
            assert np.allclose(got.dep.astype(float), dep.astype(float), rtol=1e-12, atol=1e-18)
        assert 20 <= dec["captured"].sum() <= k.P - 20 and (k.tet < 0).sum() >= 1
    _pin("capture_flag:dep", X.c_capture(X.capture_case))


@needs_ld
@pytest.mark.parametrize("kind", ["plane", "sphere"])
def test_surface_contact_is_the_surface_contact_model(kind):
    for poly in (False, True):
        k = X.surface_case(kind, poly)
        m, r = (k.m, k.r) if poly else (k.M, k.R)
        dec = scm.decide(k.mesh.x, k.mesh.ien, k.w, k.tet, k.lam, r, scm.LEVEL, k.side, scm.T_SOLID)
        assert scm.margins_ok(dec, scm.T_SOLID)
        for friction in (False, True):
            law = dict(mu=X.LAW[0], kt=X.LAW[1], gamma_t=X.LAW[2], dt=X.LAW[3]) if friction else None
            F, tau, xi, fn = scm.forces(dec, k.vel, m, X.KN, X.GN, friction=law, omega=k.omega, xi_old=k.old)
            a, al = scm.accelerations(F, tau, m, r)
            got = X.surface_run(k, LD, poly, friction, old=True)
            assert np.array_equal(got.contact, dec["contact"]) and np.array_equal(got.buried, dec["buried"])
            assert np.allclose(got.d_acc.astype(float), a.astype(float), rtol=1e-11, atol=1e-12)
            if friction:
                assert np.allclose(got.d_alpha.astype(float), al.astype(float), rtol=1e-11, atol=1e-9)
            f64 = X.surface_run(k, F64, poly, friction, old=True)
            assert np.array_equal(f64.contact, dec["contact"]) and np.array_equal(f64.buried, dec["buried"])
        cls = scm.classify(dec, scm.T_SOLID)
        assert set(cls.tolist()) == set(range(6))
    if kind == "sphere":
        c = X.c_surface()
        for j, name in enumerate(("acc", "alpha", "xi")):
            _pin("surface_contact<friction>:" + name, c[j])


def test_grad_max_bounds_every_gradient():
    for M, j in X.CUBES:
        m = X.kuhn(M, j)
        gm = X.grad_max(m)
        c23, c31, c12, det = X.tet_cross(m.x[m.ien])
        assert np.isfinite(gm) and gm >= (np.linalg.norm(c23, axis=1) / np.abs(det)).max() * (1 - 1e-12)
    flat = X.Mesh("flat", [[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0, 0, 1]], [[0, 1, 2, 4], [0, 1, 2, 3]])
    assert X.grad_max(flat) == np.inf


def test_node_sum_on_dyadic_data_is_exact():
    m = X.kuhn(2, 0.2)
    tet, lam, val = X.dyadic_particles(m, 257, 1)
    start, members = X.sort_by_tet(tet, m.T)
    for C, scale in ((1, 0.5), (3, 4.0), (5, 1.0)):
        got = X.node_sum(m, start, members, lam, val[:, :C], scale, C)
        ref = np.zeros((m.N, C), LD)
        ok = tet >= 0
        np.add.at(ref, m.ien[tet[ok]].ravel(), (lam[ok][:, :, None] * val[ok][:, None, :C]).reshape(-1, C).astype(LD))
        assert np.array_equal(got.astype(LD), -scale * ref)
    # a node without a particle: -scale * 0.0
    empty = X.node_sum(m, np.zeros(m.T + 1, I64), np.zeros(0, I64), lam, val[:, :1], 2.0, 1)
    assert np.all(empty == 0) and np.all(np.signbit(empty))
