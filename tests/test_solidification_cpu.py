"""CPU tests of the solidification record (include/dedflow.h, "solidification record"): the symbols, the library's host-only
configuration check, the numpy model's recovered gradient on a linear field, and what the state sequences of the GPU parity
test (tests/solidification_model.py, sequence) promise."""
import ctypes as C
import os

import numpy as np
import pytest

import solidification_model as sm
from dedflow_amd.meshgen import fan_mesh, kuhn_cube, single_tet

LD = np.longdouble
MESHES = {"single": single_tet, "fan": fan_mesh, "cube4": lambda: kuhn_cube(4), "cube6": lambda: kuhn_cube(6),
          "cube13": lambda: kuhn_cube(13)}
_cache = {}


def _mesh(name):
    if name not in _cache:
        _cache[name] = MESHES[name]()
    return _cache[name]


def test_symbols_declared_and_exported():
    from dedflow_amd import api
    lib = api.lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pub = open(os.path.join(root, "include", "dedflow.h")).read()
    ker = open(os.path.join(root, "include", "dedflow_kernels.h")).read()
    for n in ("DflSolidificationCheck", "DflMeshSetSolidification", "DflMeshSolidificationEnabled", "DflMeshSolidificationUpdate",
              "DflMeshSolidificationReset", "DflMeshSolidificationFields", "DflMeshSolidificationEvents",
              "DflMeshSolidificationStats"):
        assert n in pub and hasattr(lib, n), n
    for n in ("dfl_solid_reset", "dfl_solid_prime", "dfl_solid_count", "dfl_solid_events", "dfl_solid_gradient", "dfl_solid_stats",
              "dfl_solid_stats_work_size"):
        assert n in ker and hasattr(lib, n), n
    for n in ("set_solidification", "solidification_on", "solidification_update", "solidification_reset", "solidification_fields",
              "solidification_events", "solidification_stats"):
        assert hasattr(api.Problem, n), n


def test_configuration_check():
    from dedflow_amd import api
    L = api.lib()
    why = C.create_string_buffer(200)

    def library(**kw):
        c = sm.config(**dict(dict(T_front=1650.0), **kw))
        s = api.DflSolidification(c["T_front"], 1 if c["use_phi"] else 0, c["level"], c["side"], 1 if c["in_time_step"] else 0)
        return L.DflSolidificationCheck(C.byref(s), why, 200), why.value.decode()

    for good in (dict(), dict(use_phi=True, side=-1, level=0.3), dict(side=0), dict(in_time_step=True), dict(T_front=-5.0)):
        assert library(**good)[0] == 0, good                             # side counts only with use_phi
    for reason, bad in (("T_front", dict(T_front=np.nan)), ("T_front", dict(T_front=np.inf)), ("level", dict(level=np.nan)),
                        ("level", dict(level=-np.inf, use_phi=True)), ("side", dict(use_phi=True, side=0)),
                        ("side", dict(use_phi=True, side=2))):
        rc, text = library(**bad)
        assert rc != 0 and reason in text, (reason, bad, text)


@pytest.mark.parametrize("name", list(MESHES))
@pytest.mark.parametrize("use_phi", [False, True])
def test_recovered_gradient_of_a_linear_field(name, use_phi):
    """every tet gradient of a linear field is the field's gradient, and so is their weighted mean wherever a tet counts; a
    node none of whose tets counts gets 0.  longdouble: 1e-15 of max|T| / h with h the shortest edge is some 100 ulp"""
    m = _mesh(name)
    x = m.xg.reshape(-1, 3)
    g = np.array([30.0, -45.0, 12.5])
    cfg = sm.config(1650.0, use_phi=use_phi, level=0.1)
    w = sm.state(m.num_node, x @ np.array([0.3, 0.1, -1.0]) + 0.4, 1600.0 + x @ g)
    grad, scale, V = sm.recovered_gradient(m.xg, m.ien, w, cfg)
    tets = m.ien.reshape(-1, 4)
    h = min(np.linalg.norm(x[tets[:, a]] - x[tets[:, b]], axis=1).min() for a in range(4) for b in range(a))
    has = V > 0
    assert has.any()
    if not use_phi:
        assert has.all()
    else:
        counts = sm.tet_counts(m.xg, m.ien, w, cfg)
        touched = np.zeros(m.num_node, bool)
        touched[tets[counts]] = True
        assert np.array_equal(has, touched)
    assert float(np.abs(grad[has] - g.astype(LD)).max()) <= 1e-15 * np.abs(w[5 * m.num_node:]).max() / h
    assert (grad[~has] == 0).all()


@pytest.mark.parametrize("name", list(MESHES))
@pytest.mark.parametrize("use_phi", [False, True])
def test_sequence_promises(name, use_phi):
    m = _mesh(name)
    N = m.num_node
    cfg, states, dts = sm.sequence(m, use_phi)
    assert len(states) == 5 and len(dts) == 4 and len(set(dts)) == 4
    hub, p0, p1, p2, p3 = sm.planted_nodes(m)
    assert len({p0, p1, p2, p3}) == 4
    Tf = cfg["T_front"]
    T = [w[5 * N:] for w in states]
    assert T[0][p1] == Tf and T[2][p1] == Tf and T[1][p1] < Tf              # Tp == T_front and Tn == T_front exactly
    assert T[0][p2] == T[1][p2] and T[2][p2] == T[3][p2]                    # Tp == Tn on both sides
    assert sum(int(np.isnan(t).sum()) for t in T) == 1 and np.isnan(T[2][p3])
    rec, events = sm.run_model(m, cfg, states, dts)
    froze = np.zeros(N, np.int64)
    remelted = np.zeros(N, bool)
    for f, mm in events:
        remelted[mm] |= froze[mm] > 0
        froze[f] += 1
    assert (froze > 0).sum() >= 0.1 * N                                      # at least 10 % of the nodes freeze
    assert remelted.any()                                                    # one melts again after freezing
    assert (froze >= 2).any()                                                # one freezes twice
    assert froze[p0] == 2 and remelted[p0] and rec.melts[p0] == 1
    assert rec.updates == 5 and rec.t == ((dts[0] + dts[1]) + dts[2]) + dts[3]   # the prime adds no time
    if use_phi:
        phi = states[0][4 * N:5 * N]
        tets = m.ien.reshape(-1, 4)
        mean = ((phi[tets[:, 0]] + phi[tets[:, 1]]) + (phi[tets[:, 2]] + phi[tets[:, 3]])) * 0.25
        assert phi[p1] == cfg["level"] and not sm.node_metal(states[0], cfg)[p1]   # a node exactly on the level
        assert (mean == cfg["level"]).any()                                   # a tet with the mean exactly the level
        counts = sm.tet_counts(m.xg, m.ien, states[0], cfg)
        assert sm.node_metal(states[0], cfg)[p0] and not counts[(tets == p0).any(axis=1)].any()   # a metal node without a tet
        assert froze[p1] == 0
        if N > 4:
            assert counts.any() and sm.node_metal(states[0], cfg)[hub]
    else:
        assert froze[p1] == 2 and froze[p2] == 1
