"""The sorted V2E map belongs to the mesh (DflMeshSortedV2E, host/mesh.c): the features that sum over it share one copy, and
clearing one of them cannot take it from another.

Memory.  DflDevicePoolStats sees only what the device pool serves, requests of 16 MiB and more (POOL_MIN_REQUEST,
host/runtime.c).  One map is 4(N+1) + 16T bytes: 412,872 B on kuhn_cube(16), where neither array reaches the pool and in-use
does not move whatever the code does.  The growth bounds therefore run on kuhn_cube(56), the smallest Kuhn cube whose [4T]
column array the pool serves (T = 1,053,696: 16T = 16,859,136 B, one map 17,599,912 B, the pooled block 9 x 2 MiB =
18,874,368 B); every other buffer of the two features stays below 16 MiB there (phase: 3 x 8N = 4.4 MB and the statistics
scratch; surface: T flag bytes), so a second enable moves in-use only if it builds a second map.  The lifetime sequence and
its return to the starting in-use run on kuhn_cube(16)."""
import ctypes as C

import numpy as np
import pytest

from dedflow_amd.meshgen import kuhn_cube, synthetic_fields

pytestmark = pytest.mark.gpu
SURFACE = dict(level=0.0, side=-1, sigma0=1.8, dsigma_dT=-4e-4, T_ref=1900.0, recoil_p0=1.0e5, recoil_a=11.0, T_boil=3100.0,
               h_conv=80.0, emissivity=0.4, T_amb=300.0, evap_q0=2.0e9)
PHASE = dict(T_solidus=1600.0, T_liquidus=1700.0, latent=2.0e9, darcy_c=1.0e6, darcy_b=1e-3)


@pytest.fixture(scope="module")
def api():
    from dedflow_amd import api as A
    A.lib()
    return A


def _in_use(api):
    r, u = C.c_int64(0), C.c_int64(0)
    api.lib().DflDevicePoolStats(C.byref(r), C.byref(u))
    return u.value


def _enable(P, which, eps):
    if which == "surface":
        P.set_surface_forces(eps=eps, **SURFACE)
    else:
        P.set_phase_change(use_phi=True, level=0.0, side=-1, eps=eps, **PHASE)


@pytest.mark.parametrize("first", ["surface", "phase"])
def test_the_second_feature_shares_the_map_of_the_first(api, first):
    M = 56
    m = kuhn_cube(M)
    one_map = 4 * (m.num_node + 1) + 16 * m.num_tet
    assert 16 * m.num_tet >= 16 << 20 and 8 * 3 * m.num_node < 16 << 20
    start = _in_use(api)
    P = api.Problem(m)
    try:
        u0 = _in_use(api)
        _enable(P, first, 2.0 / M)
        u1 = _in_use(api)
        _enable(P, "phase" if first == "surface" else "surface", 2.0 / M)
        u2 = _in_use(api)
        print(f"in-use: +{u1 - u0} B for {first}, +{u2 - u1} B for the second feature, one map {one_map} B")
        assert u1 - u0 >= one_map
        assert 0 <= u2 - u1 < one_map
    finally:
        P.close()
    assert _in_use(api) == start


def _fields(m):
    N = m.num_node
    x = m.xg.reshape(-1, 3)
    w, dw = synthetic_fields(m)
    r = np.linalg.norm(x - np.array([0.53, 0.48, 0.55]), axis=1)
    w[4 * N:5 * N] = r - 0.3
    w[5 * N:] = 300.0 + 3200.0 * np.exp(-(r / 0.35) ** 2)
    return w, dw


ALL = ("surface", "phase", "scalar", "couple")


def _sequence(api, m, order, features=ALL):
    """`features` on, then those of `order` cleared one at a time; after each step the raw outputs of every feature still on
    (and of DflAssembleScalarJacobian at every step: without a transport state it needs nothing but the mesh's map)"""
    w, dw = _fields(m)
    rng = np.random.default_rng(3)
    pts, vel = rng.uniform(0.05, 0.95, size=(200, 3)), rng.normal(0.0, 0.3, size=(200, 3))
    P = api.Problem(m)
    pc = api.Particles(pts.reshape(-1), vel.reshape(-1), 0.01, mass=2.0e-3)
    steps = []
    try:
        w_d, dw_d = api.DeviceArray.from_numpy(w), api.DeviceArray.from_numpy(dw)
        if "surface" in features:
            _enable(P, "surface", 2.0 / 16)
        if "phase" in features:
            _enable(P, "phase", 2.0 / 16)
        if "scalar" in features:
            P.set_scalar_transport()
        if "couple" in features:
            pc.couple(P, mu_f=1.0e-2)
        on = set(features)
        for clear in (None,) + tuple(order):
            if clear == "surface":
                P.set_surface_forces()
            elif clear == "phase":
                P.set_phase_change()
            elif clear == "scalar":
                P.clear_scalar_transport()
            elif clear == "couple":
                pc.couple(None)
            on.discard(clear)
            out = {}
            if "surface" in on:
                out.update({"surface_" + k: a for k, a in P.surface_load(w_d).items()})
            if "phase" in on:
                out.update({"phase_" + k: a for k, a in P.phase_coefficients(w_d).items()})
            if "couple" in on:
                pc.fluid_step(w_d)
                out["couple_load"] = pc.reaction_load()
            api.sync()
            out = {k: a.numpy() for k, a in out.items()}
            out["scalar_phi"], out["scalar_T"] = P.assemble_scalar_jacobian(w_d, dw_d)
            steps.append(out)
    finally:
        pc.close()
        P.close()
    return steps


def test_clearing_one_feature_leaves_the_others_their_bits(api):
    m = kuhn_cube(16)
    start = _in_use(api)
    base = _sequence(api, m, ())[0]
    assert sorted(base) == ["couple_load", "phase_D", "phase_G", "phase_H", "scalar_T", "scalar_phi", "surface_area", "surface_heat",
                            "surface_load"]
    for k, v in base.items():
        assert np.isfinite(v).all() and np.count_nonzero(v), k
    # the particles move between the steps, so the reaction load of step k is compared with step k of a run that clears
    # nothing but takes the same sub-steps: a context coupled throughout
    never = _sequence(api, m, ("none", "none", "none", "none"))
    # the phase change puts its latent heat on the diagonal of the T Jacobian: once it is cleared, the T values are those of
    # a mesh that never had it
    plain = _sequence(api, m, (), features=())[0]
    assert sorted(plain) == ["scalar_T", "scalar_phi"] and plain["scalar_phi"].tobytes() == base["scalar_phi"].tobytes()
    assert plain["scalar_T"].tobytes() != base["scalar_T"].tobytes()
    for order in (("surface", "couple", "phase", "scalar"), ("scalar", "phase", "couple", "surface")):
        steps = _sequence(api, m, order)
        assert len(steps) == 5 and sorted(steps[0]) == sorted(base)
        for k, out in enumerate(steps):
            assert len(out) == len(base) - sum({"surface": 3, "phase": 3, "scalar": 0, "couple": 1}[c] for c in order[:k])
            for name, v in out.items():
                ref = plain if name == "scalar_T" and "phase" in order[:k] else never[k]
                assert v.tobytes() == ref[name].tobytes(), (order, k, name)
    assert _in_use(api) == start
