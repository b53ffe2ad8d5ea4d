"""CPU checks of particle inflow and outflow: the numpy model (tests/flow_model.py) of the inlet lattice, the hash, blocking,
selection, the credit and cap arithmetic and the compaction with its history remap, and the library's entry points being
exported (no compute calls: no GPU here)."""
import os
import subprocess

import numpy as np
import pytest

import flow_model as fl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_splitmix64_reference_values():
    # the first outputs of the splitmix64 generator seeded with 0 (state += golden gamma, then the finalizer)
    assert fl.splitmix64(0) == 0xE220A8397B1DCDAF
    assert fl.splitmix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4


def test_unit_pm1_range():
    assert fl.unit_pm1(0) == -1.0
    assert fl.unit_pm1(fl.M64) < 1.0 and fl.unit_pm1(fl.M64) == 1.0 - 2.0 ** -52


@pytest.mark.parametrize("jitter", [0.0, 0.5, 1.0])
def test_lattice_fits_and_candidates_never_overlap(jitter):
    R = 0.05
    inlet = fl.Inlet((0.1, 0.2, 0.9), (0.73, 0.0, 0.0), (0.0, 0.52, 0.0), R, jitter=jitter, seed=7)
    assert (inlet.nu, inlet.nv) == (7, 5)
    for call in range(3):
        c = inlet.centres(call)
        assert np.allclose(c[:, 2], 0.9)
        # inside the rectangle, at least R from its edges along the lattice
        assert (c[:, 0] >= 0.1 + R - 1e-12).all() and (c[:, 0] <= 0.83 - R + 1e-12).all()
        assert (c[:, 1] >= 0.2 + R - 1e-12).all() and (c[:, 1] <= 0.72 - R + 1e-12).all()
        d = np.linalg.norm(c[:, None] - c[None], axis=2) + np.eye(len(c)) * 1e9
        assert d.min() >= 2 * R * (1 - 1e-12)
        if jitter == 0.0:
            assert np.array_equal(c, inlet.centres(call + 1))
        else:
            assert not np.array_equal(c, inlet.centres(call + 1))


def test_tilted_inlet_lattice():
    R = 0.02
    u, v = np.array([0.3, 0.3, 0.0]), np.array([0.0, 0.0, 0.25])
    inlet = fl.Inlet((0.2, 0.1, 0.3), u, v, R, jitter=0.8, seed=3)
    assert inlet.nu == int(np.floor(np.linalg.norm(u) / (2 * R))) and inlet.nv == 6
    c = inlet.centres(0)
    n = np.cross(u, v) / np.linalg.norm(np.cross(u, v))
    assert np.abs((c - [0.2, 0.1, 0.3]) @ n).max() < 1e-14
    d = np.linalg.norm(c[:, None] - c[None], axis=2) + np.eye(len(c)) * 1e9
    assert d.min() >= 2 * R * (1 - 1e-12)


def test_blocking_marks_exactly_the_reached_slots():
    R = 0.04   # 12 x 12 slots of pitch 1/12 > 2R: a centre on one slot blocks none of its neighbours
    inlet = fl.Inlet((0.0, 0.0, 0.5), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), R, jitter=0.0, seed=11)
    c = inlet.centres(4)
    # a particle on slot 12, one 1.9R above slot 30, one 2.1R above slot 31, one far away
    y = np.array([c[12], c[30] + [0, 0, 1.9 * R], c[31] + [0, 0, 2.1 * R], [5.0, 5.0, 5.0]])
    b = inlet.blocked(4, y)
    assert set(np.flatnonzero(b)) == {12, 30}


def test_selection_is_a_pure_function_and_skips_blocked_slots():
    inlet = fl.Inlet((0.0, 0.0, 0.0), (0.8, 0.0, 0.0), (0.0, 0.8, 0.0), 0.05, seed=5)
    free = np.zeros(inlet.nslot, bool)
    r0 = inlet.ranked_free(2, free)
    assert sorted(r0) == list(range(inlet.nslot)) and r0 == inlet.ranked_free(2, free)
    assert r0 != inlet.ranked_free(3, free)
    blk = free.copy()
    blk[r0[:5]] = True
    r1 = inlet.ranked_free(2, blk)
    assert r1 == r0[5:]


def test_credit_cap_and_no_overlap_over_many_calls():
    R = 0.05
    inlet = fl.Inlet((0.05, 0.05, 0.9), (0.9, 0.0, 0.0), (0.0, 0.9, 0.0), R, jitter=0.7, seed=99)
    m = fl.InflowModel(inlet, per_call=2.5, max_particles=40)
    coord, vel, tags = np.empty((0, 3)), np.empty((0, 3)), np.empty(0, np.int64)
    inserted, expect_credit = [], 0.0
    for k in range(30):
        P = len(coord)
        coord, vel, tags, n = m.add(coord, vel, tags, P)
        inserted.append(n)
        expect_credit += 2.5
        want = int(np.floor(expect_credit))
        expect_credit -= want
        assert n == min(want, 40 - P)      # the inlet (81 slots) is never full: only the cap limits
        assert m.credit == expect_credit
        # particles stay where they were put: later candidates find the earlier ones and are blocked
        d = np.linalg.norm(coord[:, None] - coord[None], axis=2) + np.eye(len(coord)) * 1e9
        assert len(coord) < 2 or d.min() >= 2 * R * (1 - 1e-12)
    assert len(coord) == 40 and np.array_equal(tags, np.arange(40))
    assert sum(inserted[:3]) == 2 + 3 + 2


def test_full_inlet_counts_blocked():
    R = 0.05
    inlet = fl.Inlet((0.0, 0.0, 0.5), (0.4, 0.0, 0.0), (0.0, 0.2, 0.0), R)   # 4 x 2 slots
    m = fl.InflowModel(inlet, per_call=5, max_particles=1000)
    coord, vel, tags = np.empty((0, 3)), np.empty((0, 3)), np.empty(0, np.int64)
    coord, vel, tags, n0 = m.add(coord, vel, tags, 0)
    coord, vel, tags, n1 = m.add(coord, vel, tags, n0)    # 3 free slots left, no jitter: the same centres
    coord, vel, tags, n2 = m.add(coord, vel, tags, n0 + n1)
    assert (n0, n1, n2) == (5, 3, 0)
    assert m.blocked_total == 0 + 2 + 5


def test_outflow_keep_and_history_remap():
    rng = np.random.default_rng(4)
    P = 50
    x = rng.uniform(0, 1, (P, 3))
    keep = fl.outflow_keep(x, [(1.0, 0.0, 0.0, 0.7), (0.0, 0.0, -1.0, -0.1)])
    assert np.array_equal(keep, ~((x[:, 0] > 0.7) | (-x[:, 2] > -0.1)))
    tet = rng.integers(-2, 5, P)
    keep2 = fl.outflow_keep(x, [], tet, outside_mesh=True)
    assert np.array_equal(keep2, tet != -1)
    counts = rng.integers(0, fl.MAX_HISTORY + 1, P)
    keys = np.zeros((P, fl.MAX_HISTORY), np.uint64)
    xi = rng.normal(size=(P, fl.MAX_HISTORY, 3))
    for i in range(P):
        for e in range(counts[i]):
            keys[i, e] = rng.integers(0, P) if rng.random() < 0.7 else (1 << 62) | int(rng.integers(0, 6))
    nk, nx, nc = fl.remap_history(keys, xi, counts, keep)
    newid = np.cumsum(keep) - keep
    old_of = np.flatnonzero(keep)
    assert len(nc) == keep.sum()
    for j, i in enumerate(old_of):
        live = [(int(keys[i, e]), xi[i, e]) for e in range(counts[i])
                if int(keys[i, e]) >> 62 or keep[int(keys[i, e])]]
        assert nc[j] == len(live)
        for m, (k, v) in enumerate(live):
            assert int(nk[j, m]) == (k if k >> 62 else int(newid[k]))
            assert np.array_equal(nx[j, m], v)


def test_library_exports_the_flow_entry_points():
    subprocess.check_call(["make", "-s", "-j8", "-C", ROOT])
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "dedflow_amd", "libdedflow.so")], text=True)
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in ("ParticleContextSetOutflow", "ParticleContextSetInflow", "ParticleContextFlowStats", "ParticleContextTag",
                 "ParticleContextAdd", "ParticleContextRemove", "dfl_flow_flag", "dfl_flow_compact", "dfl_inflow_block",
                 "dfl_inflow_select", "dfl_inflow_select_temp_bytes", "dfl_inflow_append"):
        assert name in names, name
