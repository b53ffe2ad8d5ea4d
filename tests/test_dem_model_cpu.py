"""CPU checks of tests/dem_model.py, the model behind test_gpu_dem_kernels.py: the float64 restatement pinned to the models the
suite already has (oracle.dem_forces, walls_model, friction_model, poly_model, at those modules' tolerances), closed forms,
the constant c of every variant (measured on the restatement, never on a kernel), the margin condition of every random
family and the exactness of the dyadic lattice.  No GPU."""
import json
import os

import numpy as np
import pytest

import dem_model as D
import friction_model as fm
import poly_model as pm
import walls_model as wm

F64, LD = D.F64, D.LD
needs_ld = pytest.mark.skipif(not D.HAVE_EXTENDED, reason=D.EXTENDED_REASON)


# ---- integer passes --------------------------------------------------------------------------------------------------
def test_scan_and_order():
    count = np.array([0, 3, 0, 1, 2])
    assert D.exclusive_scan(count).tolist() == [0, 0, 3, 3, 4, 6]
    assert D.exclusive_scan([]).tolist() == [0]
    cell_of = np.array([4, 1, 3, 1, 4, 1])
    cnt, start, order = D.cell_order(cell_of, 5)
    assert cnt.tolist() == count.tolist() and start.tolist() == [0, 0, 3, 3, 4, 6] and order.tolist() == [1, 3, 5, 2, 0, 4]
    assert D.slots(order)[order].tolist() == list(range(6))
    assert [D.scan_num_chunks(n) for n in (0, 1023, 1024, 257 * 1024)] == [1, 1, 2, 258]


def test_cell_of_a_coordinate():
    # inside, on a boundary (the upper cell), at and beyond the box (clamped)
    assert D.cell_coord([0.0, 0.2499, 0.25, 0.999, 1.0, -0.3, 1.7], 0.25, 4).tolist() == [0, 0, 1, 3, 3, 0, 3]
    # fl(1 / fl(1 / 49)) = 49.00000000000001: 2 / 49 and 4 / 49 land one cell above the exact quotient's, 1 / 49 does not
    inv = F64(1.0) / (F64(1.0) / F64(49))
    assert inv > 49.0
    k = np.arange(50)
    got = D.cell_coord(k / 49.0, 1.0 / 49, 49)
    assert np.array_equal(got, np.clip(np.floor((k / 49.0) * inv), 0, 48).astype(int))
    assert got[0] == 0 and got[49] == 48 and np.all((got[:49] - k[:49] >= 0) & (got[:49] - k[:49] <= 1))
    g = D.Grid3((-1.0, 2.0, 0.5), (3.0, 5.0, 2.0), (3, 5, 2))
    x = np.array([[-1.0, 2.0, 0.5], [-0.01, 2.99, 1.49], [0.0, 2.5, 1.0], [-1.01, 2.5, 1.0], [-0.5, 3.0, 1.0], [-0.5, 2.5, 0.49]])
    assert D.grid_bins(x, g).tolist() == [0, 2 + 3 * (4 + 5 * 1), 30, 30, 30, 30]


# ---- pins ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,R", [(3000, 0.03), (300, 0.2)])
def test_pin_oracle(P, R):
    from dedflow_amd.meshgen import dem_particles
    from oracle import orc
    x, v, _ = dem_particles(P, R)
    s = D.sweep(x, v, np.full(P, R), np.full(P, 1.5), 1.0e4, 1.0, F64)
    for brute in (False, True):
        ref, _ = orc.dem_forces(x, v, R, mass=1.5, kn=1.0e4, gn=1.0, brute=brute)
        assert np.abs(s.acc.ravel() - ref).max() <= 1e-10 * np.abs(ref).max()


def _records(W, x, R):
    plane = np.array([fm.plane_id(W, W.n[t], W.off[t]) for t in range(len(W.v))])
    cand = [list(range(len(W.v))) if ok else [] for ok in wm.padded_inside(W, x, R)]
    return D.MeshWalls(W.v, W.n, W.off, W.node, plane, W.tol, cand)


def wall_cloud(W, R, n_in, n_wall, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(W.lo - 2 * R, W.hi + 2 * R, size=(n_in, 3))
    t = rng.integers(0, len(W.v), n_wall)
    lam = rng.dirichlet(np.ones(3), n_wall)
    x = np.vstack([x, np.einsum("na,nad->nd", lam, W.v[t]) + W.n[t] * rng.uniform(-0.5 * R, R, (n_wall, 1))])
    return x, rng.normal(size=x.shape), rng.normal(0.0, 3.0, size=x.shape)


def test_pin_walls_model():
    from dedflow_amd.meshgen import fan_mesh, kuhn_cube
    for mesh, R in ((kuhn_cube(3), 0.04), (fan_mesh(), 0.1)):
        W = wm.Walls(mesh)
        x, v, _ = wall_cloud(W, R, 60, 60, 3)
        act = wm.padded_inside(W, x, R)
        s = D.sweep(x, v, np.full(len(x), R), np.ones(len(x)), 1.0e4, 1.0, F64, box=False, mesh=_records(W, x, R), active=act)
        ref, dref = wm.forces(W, x, v, R)
        assert np.count_nonzero(np.abs(ref).sum(axis=1)) > 30 and s.dropped == dref
        assert np.abs(s.acc - ref).max() <= 1e-12 * np.abs(ref).max()
    bx = np.random.default_rng(4).uniform(0, 1, (200, 3))
    bv = np.random.default_rng(5).normal(size=bx.shape)
    s = D.sweep(bx, bv, np.full(200, 0.1), np.ones(200), 1.0e4, 1.0, F64)
    ref = wm.pair_forces(bx, bv, 0.1, 1.0e4, 1.0, np.ones(200, bool)) + wm.unit_box_wall_forces(bx, bv, 0.1, 1.0e4, 1.0)
    assert np.abs(s.acc - ref).max() <= 1e-12 * np.abs(ref).max()


def _as_history(rows, P):
    h = D.History(P)
    for i, row in enumerate(rows):
        for e, (k, xi) in enumerate(row.items()):
            h.key[i, e], h.xi[i, e] = k, xi
        h.count[i] = len(row)
    return h


def test_pin_friction_and_poly_models():
    """two sweeps with the history carried over, one size (friction_model) and per-particle sizes with unequal-radii levers
    (poly_model), on clouds without overflow"""
    rng = np.random.default_rng(8)
    P, R = 250, 0.05
    x, v, w = rng.uniform(0, 1, (P, 3)), rng.normal(0, 0.1, (P, 3)), rng.normal(0, 3, (P, 3))
    r = rng.uniform(0.5 * R, R, P)
    m = pm.default_mass(r, R, 1.5)
    law = D.Law(0.5, 2.0 / 7.0 * 1.0e4, 1.0, 1.0e-4)
    for poly in (False, True):
        ref = (pm.Model(x, v, r, m, mu=0.5, w=w) if poly else fm.Model(x, v, R, mass=1.5, mu=0.5, w=w))
        old = D.History(P)
        for sweep in range(2):
            s = D.sweep(x, v, r if poly else np.full(P, R), m if poly else np.full(P, 1.5), 1.0e4, 1.0, F64, w=w, law=law, old=old)
            acc, alpha = ref.forces()
            assert s.over == 0 and s.in_contact.sum() > 100
            assert np.abs(s.acc - acc).max() <= 1e-12 * np.abs(acc).max()
            assert np.abs(s.alpha - alpha).max() <= 1e-12 * np.abs(alpha).max()
            for i in range(P):
                assert sorted(s.keys[i]) == sorted(ref.hist[i])
                for e, k in enumerate(s.keys[i]):
                    assert np.abs(s.xi[i, e] - ref.hist[i][k]).max() <= 1e-12 * max(np.abs(ref.hist[i][k]).max(), 1e-300)
            old = D.History(P, s.count, s.key, s.xi)
    # without friction the per-particle-size normal law
    s = D.sweep(x, v, r, m, 1.0e4, 1.0, F64)
    acc, _ = pm.Model(x, v, r, m).forces()
    assert np.abs(s.acc - acc).max() <= 1e-13 * np.abs(acc).max()


# ---- closed forms ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, LD])
def test_two_spheres(dtype):
    x, v = [[0.4, 0.5, 0.5], [0.4 + 0.09, 0.5, 0.5]], [[0.3, 0.1, 0.0], [-0.2, 0.0, 0.0]]
    s = D.sweep(x, v, [0.05, 0.05], [2.0, 4.0], 1.0e4, 3.0, dtype)
    fn = 1.0e4 * 0.01 - 3.0 * (0.5 * -1.0)    # n of particle 0 is -e_x: vn = dv . n = -0.5
    assert np.allclose(np.asarray(s.acc, F64), [[-fn / 2.0, 0, 0], [fn / 4.0, 0, 0]], rtol=1e-12, atol=1e-12)
    assert s.keys == [[1], [0]] and np.allclose(s.margin, 0.01)
    assert np.allclose(np.asarray(s.A_acc, F64), 1.0e4 * 0.19 + 3.0 * 0.6)


def test_sphere_on_each_wall():
    R, d = 0.05, 0.01
    for ax in range(3):
        for side in range(2):
            x = np.full(3, 0.5)
            x[ax] = R - d if side == 0 else 1.0 - R + d
            v = np.array([0.1, -0.2, 0.3])
            s = D.sweep([x], [v], [R], [2.0], 1.0e4, 3.0, F64)
            want = np.zeros(3)
            want[ax] = (1.0e4 * d - 3.0 * v[ax] * (1 if side == 0 else -1)) * (1 if side == 0 else -1) / 2.0
            assert np.allclose(s.acc[0], want, rtol=1e-11, atol=1e-11)
            assert s.keys[0] == [D.KEY_WALL | (2 * ax + side)] and abs(s.margin[0] - d) < 1e-12
            assert np.isclose(s.A_acc[0], 1.0e4 * (R + x[ax] + side) + 3.0 * abs(v[ax]))


def test_launched_sphere_ends_rolling_at_five_sevenths():
    R, kn, gn, gt, dt, g = 0.05, 1.0e6, 200.0, 50.0, 2.0e-4, np.array([0.0, 0.0, -9.81])
    law = D.Law(0.3, 2.0 / 7.0 * kn, gt, dt)
    x, v, w = np.array([[0.2, 0.5, R - 9.81 / kn]]), np.array([[1.0, 0.0, 0.0]]), np.zeros((1, 3))
    old = D.History(1)
    for _ in range(2500):
        s = D.sweep(x, v, [R], [1.0], kn, gn, F64, w=w, law=law, old=old)
        old = D.History(1, s.count, s.key, s.xi)
        x, v = D.integrate(dt, x, v, s.acc, F64, g)
        w = D.spin(dt, w, s.alpha, F64)
    assert abs(v[0, 0] - 5.0 / 7.0) <= 0.01 * 5.0 / 7.0 and abs(w[0, 1] * R - 5.0 / 7.0) <= 0.01 * 5.0 / 7.0


def test_integrators():
    x, v = D.integrate(0.5, [[1.0, 2.0, 3.0]], [[0.5, 0.0, -1.0]], [[2.0, 4.0, 0.0]], F64, (0.0, 0.0, -2.0))
    assert v.tolist() == [[1.5, 2.0, -2.0]] and x.tolist() == [[1.75, 3.0, 2.0]]
    assert D.spin(0.25, [[1.0, 0.0, 0.0]], [[4.0, 8.0, -4.0]], F64).tolist() == [[2.0, 2.0, -1.0]]


# ---- the constant c, the margins, the lattice -------------------------------------------------------------------------------
@needs_ld
@pytest.mark.parametrize("poly,fric", [(False, False), (True, False), (False, True), (True, True)])
def test_constant_c(poly, fric):
    c = D.constant(poly, fric)
    live = c[:3 if fric else 1]
    assert np.all(np.isfinite(live)) and np.all(live > 0), c
    assert np.all(c <= 16), "c = %s: the abs-sum A_i is missing a term" % c
    _write_c("dem_forces%s%s" % ("-sizes" if poly else "", "-friction" if fric else ""), c)


def _write_c(variant, c):
    out = os.environ.get("DFL_PARITY_OUT")
    if out:
        with open(out, "a") as fh:
            fh.write(json.dumps({"kernel": "restatement", "case": variant, "c_acc": c[0], "c_alpha": c[1], "c_xi": c[2]}) + "\n")


@needs_ld
@pytest.mark.parametrize("name", D.RANDOM_ONE + D.RANDOM_POLY + D.CRAFTED)
def test_margins(name):
    """every particle of every family is at least 1e-9 rmax from every contact's opening: nothing has to be left out.  The
    longdouble and the float64 sweep then find the same contacts"""
    fam = D.family(name)
    poly = fam.R is None
    a, b = D.variant_sweep(fam, poly, False, LD), D.variant_sweep(fam, poly, False, F64)
    assert a.margin.min() >= 1e-9 * fam.rmax, (name, a.margin.min() / fam.rmax)
    assert a.keys == b.keys and a.in_contact.any()
    if name.startswith("straddle"):
        assert all(len(k) == 1 for k in a.keys)
        cell = D.box_bins(fam.x, 1.0 / fam.ncell, fam.ncell)
        assert np.all(cell[0::2] != cell[1::2])
    if name == "reach":
        assert all(len(k) == 1 for k in a.keys)
        lo = D.cell_coord(fam.x[0::2] + 2 * fam.r[0::2, None], 0.25, 4), D.cell_coord(fam.x[0::2] - 2 * fam.r[0::2, None], 0.25, 4)
        big = D.cell_coord(fam.x[1::2], 0.25, 4)
        assert np.all(np.any((big > lo[0]) | (big < lo[1]), axis=1)), "a partner is inside the small particle's own range"


@needs_ld
def test_mesh_wall_constant_and_margin():
    from dedflow_amd.meshgen import fan_mesh, kuhn_cube
    law = D.Law(0.5, 2.0 / 7.0 * 1.0e4, 1.0, 1.0e-4)
    for name, mesh, R in (("kuhn_cube3", kuhn_cube(3), 0.04), ("fan", fan_mesh(), 0.1)):
        W = wm.Walls(mesh)
        x, v, w = wall_cloud(W, R, 60, 90, 3)
        act = wm.padded_inside(W, x, R)
        args = (x, v, np.full(len(x), R), np.ones(len(x)), 1.0e4, 1.0)
        kw = dict(box=False, mesh=_records(W, x, R), active=act, w=w, law=law, old=D.History(len(x)))
        a, b = D.sweep(*args, LD, **kw), D.sweep(*args, F64, **kw)
        assert a.margin.min() >= 1e-9 * R and a.keys == b.keys
        c = D.sweep_c(a, b)
        assert np.all(np.isfinite(c)) and np.all(c > 0) and np.all(c <= 16), c
        _write_c("walls_forces-friction-" + name, c)


@needs_ld
def test_lattice_is_exact():
    """on the dyadic lattice every intermediate of the float64 restatement is exact: it equals the longdouble model bit for
    bit; touching second neighbours, the coincident pair and the wall overlap of exactly 0 contribute nothing"""
    x, v = D.dyadic_lattice()
    P, R = len(x), D.LATTICE_R
    a = D.sweep(x, v, np.full(P, R), np.full(P, D.LATTICE_M), D.LATTICE_KN, D.LATTICE_GN, LD)
    b = D.sweep(x, v, np.full(P, R), np.full(P, D.LATTICE_M), D.LATTICE_KN, D.LATTICE_GN, F64)
    assert np.array_equal(a.acc.astype(F64).view(np.uint64), b.acc.view(np.uint64))
    assert np.array_equal(a.acc, b.acc.astype(LD))
    assert a.margin.min() == 0.0 and (~a.in_contact).sum() >= 1
    assert np.all(b.acc[~b.in_contact].view(np.uint64) == 0)
    d = np.linalg.norm(x[:, None] - x[None], axis=2)
    assert (d == 0).sum() == P + 2 and (d == 2 * R).sum() > 50
    for i in range(P):   # a chain neighbour at exactly R and nothing else
        assert all(d[i, k] == R for k in a.keys[i] if k < D.KEY_WALL)
    at_wall = [i for i in range(P) if any(k >= D.KEY_WALL for k in a.keys[i])]
    assert sorted(x[at_wall].min(axis=1).tolist() + x[at_wall].max(axis=1).tolist())[0] == 0.0
    assert all((x[i] == 0).any() or (x[i] == 1).any() for i in at_wall) and len(at_wall) == 8
