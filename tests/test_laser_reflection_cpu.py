"""The model of the laser's reflections (tests/laser_reflection_model.py) against analysis -- an exact V-groove of two planes,
A(0) and A(1), energy conservation --, DflLaserReflectionCheck through the library, and the condition the GPU tests put on
their inputs: every ray decides with a margin.  All without a GPU."""
import ctypes

import numpy as np
import pytest

import laser_model as lm
import laser_reflection_model as rf

EPS, LD = rf.EPS, rf.LD


@pytest.fixture(scope="module")
def m():
    return rf.mesh()


class _Soup:
    """a hand-made reflection list: triangles with a tet id and a gradient each"""

    def __init__(self, tris, tets, grads):
        self.F = np.asarray(tris, np.float64).reshape(-1, 9)
        self.tet = np.asarray(tets, np.int64)
        self.g = np.asarray(grads, np.float64).reshape(-1, 3)


def _v_groove(half_angle, depth=1.0, length=4.0):
    """two planes through the line x = z = 0, each `half_angle` from the vertical, metal below (side = -1: phi = signed
    height above the walls, g points out of the metal).  Each wall is one large triangle pair; every triangle its own tet"""
    t = np.tan(half_angle)
    tris, grads = [], []
    for sgn in (-1.0, 1.0):
        a, b = np.array([0.0, -length, 0.0]), np.array([0.0, length, 0.0])
        c, d = np.array([sgn * depth * t, -length, depth]), np.array([sgn * depth * t, length, depth])
        tris += [np.concatenate([a, b, d]), np.concatenate([a, d, c])]
        n = np.array([-sgn * np.cos(half_angle), 0.0, np.sin(half_angle)])      # out of the metal, into the groove
        grads += [n, n]
    return _Soup(tris, [0, 1, 2, 3], grads)


@pytest.mark.parametrize("half_deg,x0", [(30.0, 0.11), (22.5, 0.07), (15.0, 0.05), (40.0, 0.3)])
def test_v_groove_follows_the_unfolded_path(half_deg, x0):
    """a vertical ray in a V-groove of half angle a.  Unfolding the wedge: after k reflections the ray makes the angle 2 k a
    with the downward vertical, on alternating sides, and it meets the opposite wall while that angle is below pi - a, the
    direction of the wall itself.  So a ray that misses the apex is reflected ceil((pi - a) / (2 a)) times; the hit points
    lie at the radius x0 / sin((2 k + 1) a) <= x0 / sin a from the apex, inside the finite walls for the x0 used"""
    a = np.radians(half_deg)
    R = _v_groove(a)
    X = np.array([x0, 0.013, x0 / np.tan(a)])                       # on the right wall
    d = np.array([0.0, 0.0, -1.0])
    hits, dirs = 1, []
    cur = 2                                                         # the right wall's first triangle holds X
    tet = R.tet[cur]
    g = R.g[cur]
    while True:
        d = d - ((2.0 * rf.dot(d, g)) / rf.dot(g, g)) * g
        dirs.append(d.copy())
        nxt, u, v, tau = rf.next_hit(R, -1, X, d, tet)
        if nxt < 0:
            break
        F = R.F[nxt]
        X = (((1.0 - u) - v) * F[0:3] + u * F[3:6]) + v * F[6:9]
        assert abs(abs(X[0]) - X[2] * np.tan(a)) < 1e-12 and X[2] > 0      # on a wall
        g, tet = R.g[nxt], R.tet[nxt]
        hits += 1
    expect = int(np.ceil((np.pi - a) / (2 * a) - 1e-12))
    assert hits == expect, (hits, expect)
    for k, dk in enumerate(dirs, start=1):
        ang = 2 * k * a
        ref = np.array([(-1.0) ** k * np.sin(ang), 0.0, -np.cos(ang)])
        assert np.abs(dk - ref).max() < 1e-13 and abs(np.linalg.norm(dk) - 1) < 1e-13


def test_self_hit_and_back_faces_are_left_out():
    R = _v_groove(np.radians(30.0))
    X, d = np.array([0.1, 0.0, 0.1 / np.tan(np.radians(30.0))]), np.array([0.0, 0.0, 1.0])
    assert rf.next_hit(R, -1, X, d, 2)[0] == -1                     # upwards out of the groove: nothing
    d = np.array([-1.0, 0.0, 0.0])
    assert rf.next_hit(R, -1, X, d, 2)[0] in (0, 1)                 # across: the left wall
    assert rf.next_hit(R, 1, X, d, 2)[0] == -1                      # from inside the metal the left wall is a back face


def test_absorptivity_at_normal_and_grazing_incidence():
    for eps in (0.05, 0.25, 1.0):
        e = LD(eps)
        a1 = rf.absorptivity(1, 0.0, eps, np.asarray(LD(1)))
        ref = 1 - ((1 + (1 - e) ** 2) / (1 + (1 + e) ** 2) + (e * e - 2 * e + 2) / (e * e + 2 * e + 2)) / 2
        assert abs(a1 - ref) < 4 * EPS and 0 < a1 < 1
        assert rf.absorptivity(1, 0.0, eps, np.asarray(LD(0))) == 0   # grazing: everything is reflected
        assert rf.absorptivity(1, 0.0, eps, np.asarray(0.0)) == 0.0
        c = np.linspace(0.0, 1.0, 1001)
        A = rf.absorptivity(1, 0.0, eps, c)
        assert (A >= 0).all() and (A <= 1).all()
        assert rf.lipschitz(1, eps) >= np.abs(np.diff(A) / np.diff(c)).max()
    assert (rf.absorptivity(0, 0.7, 0.0, np.linspace(0.0, 1.0, 5)) == 0.7).all() and rf.lipschitz(0, 0.25) == 0.0


CASES = [(f, d) for f in sorted(rf.FIELDS) for d in sorted(rf.DIRECTIONS)]
PROTOTYPE_RAYS = {("groove", "vertical"): [256, 157, 113, 73, 21, 3, 0]}


@pytest.fixture(scope="module")
def stepped(m):
    out = {}
    for field, direction in CASES:
        mg = {}
        out[field, direction] = rf.case(m, field, direction, margins=mg) + (mg,)
    return out


@pytest.mark.parametrize("field,direction", CASES)
def test_energy_is_conserved(stepped, field, direction):
    b, cand, R, o, _ = stepped[field, direction]
    rt = o["rtally"]
    p0 = o["T"][o["surf"]].sum()
    total = rt["absorbed"].sum() + rt["escaped"] + rt["remaining"]
    bound = float(o["absorbed_bound"].sum() + o["end_bound"].sum()) + 4 * b.ncol * EPS * float(p0)
    assert abs(total - p0) <= bound
    assert abs(lm.tally_sum(o["tally"]) - b.power) <= 8 * b.ncol * EPS * b.power
    per_ray = o["absorbed"].sum(axis=0) + o["escaped"] + o["remaining"]
    assert np.abs(per_ray - np.where(o["surf"], o["T"], 0)).max() <= 16 * EPS * b.power
    # nodal power carries what the rays absorbed
    assert abs(sum(o["power"].values()) - rt["absorbed"].sum()) <= 16 * (rf.MAX_BOUNCE + 1) * b.ncol * EPS * b.power


@pytest.mark.parametrize("field,direction", CASES)
def test_inputs_decide_with_a_margin(stepped, field, direction):
    """all rays, no exclusions: the barycentric coordinates of every facet ahead of a ray that it enters (the hit's among
    them) lie more than 1e-9 from 0, and the two smallest tau differ by more than 1e-9"""
    b, cand, R, o, mg = stepped[field, direction]
    rays = o["rtally"]["rays"]
    print(f"{field} {direction}: R {len(R.tet)} candidates {len(cand.tet)} rays {rays.tolist()} margins {mg}")
    assert len(cand.tet) <= len(R.tet)
    if field == "plane":
        assert rays[1:].sum() == 0 and rays[0] == int(o["surf"].sum()) > 0
        return
    assert mg["bary"] > 1e-9 and mg["tau_gap"] > 1e-9
    assert rays[1] > 0 and rays[3] > 0                              # multi-bounce paths exist
    has = o["hit"][0] >= 0
    assert o["hit"][4][has].min() > 1e-9                            # the primary hits, as the surface tests ask
    if (field, direction) in PROTOTYPE_RAYS:
        assert rays[:7].tolist() == PROTOTYPE_RAYS[field, direction] and len(R.tet) == 496 and len(cand.tet) == 493
    if (field, direction) == ("groove", "oblique"):
        assert rays[rf.MAX_BOUNCE] == 1 and o["rtally"]["remaining"] > 0


def test_model_0_on_the_plane_is_the_surface_alone(m):
    import laser_surface_model as sm
    b, cand, R, o = rf.case(m, "plane", "oblique", model=0, max_bounce=4)
    base = sm.step(b, np.zeros((0, 3)), 0.0, cand=cand)
    assert set(o["power"]) == set(base["power"]) and all(o["power"][k] == base["power"][k] for k in base["power"])
    assert all(o["tally"][k] == base["tally"][k] for k in base["tally"])


def test_check_refuses_through_the_library():
    from dedflow_amd import api
    L = api.lib()
    buf = ctypes.create_string_buffer(128)
    for mb, model, eps in ((0, 1, 0.25), (9, 0, 0.25), (-1, 0, 0.25), (4, 2, 0.25), (4, -1, 0.25), (4, 1, 0.0), (4, 1, -0.5), (4, 1, float("nan")),
                           (4, 1, float("inf")), (1, 0, float("nan")), (8, 1, 1e-300), (1, 1, 0.25), (8, 0, -1.0)):
        cfg = api.DflLaserReflection(mb, model, eps)
        rc = L.DflLaserReflectionCheck(ctypes.byref(cfg), buf, len(buf))
        why = rf.refusal(True, True, mb, model, eps)
        assert (rc != 0) == (why is not None), (mb, model, eps, buf.value)
        assert (buf.value == b"") == (rc == 0) and (rc == 0 or why.encode() in buf.value)
    assert L.DflLaserReflectionCheck(None, None, 0) != 0
    for name in ("ParticleContextSetLaserReflection", "ParticleContextLaserReflectionTally", "ParticleContextLaserReflectionRays",
                 "ParticleContextLaserReflectionFacets", "dfl_laser_reflect_count", "dfl_laser_reflect_emit", "dfl_laser_reflect_trace",
                 "dfl_laser_reflect_deposit", "dfl_laser_reflect_tally", "dfl_laser_reflect_temp_bytes"):
        assert hasattr(L, name), name
