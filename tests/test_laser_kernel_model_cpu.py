"""tests/laser_kernel_model.py without a GPU: the per-launcher model pinned to laser_model.step and laser_surface_model.step on
the cases of those files' own CPU tests, and, for every named case of test_gpu_laser_kernels.py, the property the case is
named for -- asserted on the model alone, so that a GPU test that passes has tested what its name says."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import laser_kernel_model as K
import laser_model as lm
import laser_surface_model as sm
from krylov_model import EXTENDED_REASON, HAVE_EXTENDED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64, LD, I64, U64 = np.float64, np.longdouble, np.int64, np.uint64
EPS = K.EPS
needs_ld = pytest.mark.skipif(not HAVE_EXTENDED, reason=EXTENDED_REASON)


def test_struct_sizes_match_the_header():
    txt = open(os.path.join(ROOT, "include", "dedflow_kernels.h")).read()
    sizes = {}
    for name in ("dfl_laser_beam", "dfl_wall_tri"):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, re.S).group(1)
        nbytes = 0
        for typ, fields in re.findall(r"(dfl_value|dfl_index)\s+([^;]+);", body):
            for f in fields.split(","):
                dim = re.search(r"\[(\d+)\]", f)
                nbytes += (8 if typ == "dfl_value" else 4) * (int(dim.group(1)) if dim else 1)
        sizes[name] = -(-nbytes // 8) * 8                            # aligned as its doubles
    assert C.sizeof(K.CWallTri) == 128 == sizes["dfl_wall_tri"]
    assert C.sizeof(K.CBeam) == sizes["dfl_laser_beam"] == 120
    rec = K.wall_records(np.arange(18.0).reshape(2, 9), [7, -43])
    t = C.cast(rec.ctypes.data, C.POINTER(K.CWallTri))
    assert list(t[1].v) == list(range(9, 18)) and t[1].id == -43 and list(t[0].node) == [-1, -1, -1] and t[0].off == 0.0


# ---- the model against laser_model.step and laser_surface_model.step -----------------------------------------------------------
def _frame_of(beam, o):
    f = K.Frame.__new__(K.Frame)
    f.beam, f.o, f.e1, f.e2, f.dir = beam, np.asarray(o, F64), beam.e1, beam.e2, beam.dir
    f.h, f.area, f.n, f.ncol = beam.h, beam.h * beam.h, beam.n, beam.ncol
    return f


def _through_the_launchers(beam, x, r, sub, t=0.0):
    """one laser step as the host strings the launchers together: bin -> sort by (column, id) -> hit -> columns -> deposit"""
    x = np.asarray(x, F64).reshape(-1, 3)
    P = len(x)
    b = _frame_of(beam, beam.at(t))
    cell, count, outside = K.laser_bin(x, b)
    order = np.lexsort((np.arange(P), cell))
    cell_start = np.r_[0, np.cumsum(count)]
    rr = np.broadcast_to(np.asarray(r, F64), (P,))
    tri_v = None if sub is None or len(sub.id) == 0 else np.asarray(sub.v, F64).reshape(-1, 3, 3)
    key = np.full(b.ncol, K.NO_HIT, U64)
    if tri_v is not None:
        _, _, s = K.project(tri_v, b)
        lo, hi = s.min(), s.max()
        pad = 1e-6 * ((hi - lo) + abs(lo) + abs(hi))
        key = K.laser_hit(tri_v, b, lo - pad, 2.0 ** 40 / ((hi - lo) + 2 * pad))
    sorted6 = np.concatenate([x[order], np.zeros((P, 3))], 1)
    gw = np.r_[beam.g, beam.g]
    out = K.laser_columns(P, b, beam.power, beam.eta_p, beam.eta_s, gw, cell_start, order, sorted6, rr[order], 0.0, tri_v,
                          None if tri_v is None else np.asarray(sub.id), key)
    return b, cell, outside, key, out


def _pin(beam, x, r, sub=None, step=None):
    ref = step if step is not None else lm.step(beam, x, r, sub=sub)
    b, cell, outside, key, out = _through_the_launchers(beam, x, r, sub)
    assert np.array_equal(np.minimum(cell, beam.ncol), ref["col"])           # the same columns (every outside bin is `ncol`)
    face, _ = K.key_face(key)
    assert np.array_equal(face, ref["hit"][0])                               # the same faces
    assert np.array_equal(out["col_face"], ref["face"])
    lit = ~outside
    err = np.abs(out["rate"][lit] - ref["rate"][lit]).astype(F64)
    assert np.all(err <= ref["rate_bound"][lit]) and np.all(ref["rate"][outside] == 0)
    assert np.all(np.abs(out["T"] - ref["T"]).astype(F64) <= ref["T_rel"] * ref["T"].astype(F64))
    tally = [LD(beam.power) - out["part"][0].astype(LD).sum()] + [out["part"][k].sum() for k in range(1, 6)]
    for got, k in zip(tally, ("outside", "absorbed_particles", "scattered", "substrate", "reflected", "missed")):
        assert abs(got - ref["tally"][k]) <= 8 * beam.ncol * EPS * beam.power, k
    return b, key, out, ref


@needs_ld
def test_model_is_laser_model_step_on_its_own_cpu_cases():
    import test_laser_cpu as T
    b = T._beam()
    _pin(b, np.zeros((0, 3)), np.zeros(0))
    _pin(b, np.array([[0.5 + 0.3 * b.h, 0.5 - 0.4 * b.h, 0.7]]), 0.004)
    _pin(b, np.array([[0.5 + 0.5 * b.h, 0.5 - 0.5 * b.h, 0.9 - 0.05 * j] for j in range(9)]), 0.003)
    _pin(b, np.array([[0.5 + 0.2 * b.h, 0.5 - 0.2 * b.h, 0.75], [0.5 + 0.7 * b.h, 0.5 - 0.6 * b.h, 0.75],
                      [0.5 + 3 * b.r_edge, 0.5, 0.7]]), 0.004)
    from dedflow_amd.meshgen import kuhn_cube
    m = kuhn_cube(4, jitter=0.0)
    b = T._beam(origin=(0.5037, 0.4961, 1.0), h=0.0213, r_cut=0.1)
    sub = lm.Substrate(m, [4], b)
    rng = np.random.default_rng(5)
    x = np.stack([rng.uniform(0.42, 0.58, 300), rng.uniform(0.42, 0.58, 300), rng.uniform(-0.2, 0.6, 300)], 1)
    fr, key, out, ref = _pin(b, x, rng.uniform(0.001, 0.004, 300), sub)
    assert out["rate_exact0"].any()                                          # particles below the z- face are dark
    # the deposit: the same nodal powers as the model's q, within its bound
    nodes = np.unique(sub.node)
    pairs = sorted((int(np.searchsorted(nodes, sub.node[f, k])), 4 * f + k) for f in range(len(sub.id)) for k in range(3))
    soff = np.searchsorted([p[0] for p in pairs], np.arange(len(nodes) + 1))
    power, _ = K.laser_deposit(len(nodes), soff, [p[1] for p in pairs], sub.v, fr, b.eta_s, 0.0, key, out["T"].astype(F64),
                               np.zeros(len(nodes)))
    for a, nd in enumerate(nodes):
        want = ref["q"].get(int(nd), LD(0))
        assert abs(power[a] - want) <= ref["q_bound"].get(int(nd), 0.0), nd


@needs_ld
@pytest.mark.parametrize("name", sorted(sm.DIRECTIONS))
def test_model_is_laser_surface_model_step_on_its_own_cpu_cases(name):
    m = sm.mesh()
    beam = lm.Beam(**sm.beam_args(name))
    sub = lm.Substrate(m, [4], beam)
    for phi, level in ((sm.plane_phi(m.xg), sm.PLANE_LEVEL), (sm.two_layer_phi(m.xg), 0.0)):
        snap = K.Snapshot(m.xg, m.ien, phi, level, sm.SIDE, beam.dir, len(np.asarray(m.ien).reshape(-1, 4)))
        cand = snap.cand
        for i in range(snap.nf):                                             # the same candidate list, packed
            for v in range(3):
                assert (snap.ij[i] >> (4 * v)) & 3 == cand.i[i, v] and (snap.ij[i] >> (4 * v + 2)) & 3 == cand.j[i, v]
        for s in (None, sub):
            ref = sm.step(beam, np.zeros((0, 3)), 0.0, sub=s, cand=cand)
            mg = ref["merged"]
            b, key, out, _ = _pin(beam, np.zeros((0, 3)), np.zeros(0), sub=mg, step=ref)
            unode, fslot = K.surface_nodes(m.ien, cand.tet)
            assert np.array_equal(unode[fslot].reshape(-1, 4), cand.nodes)
            power, _, _, summed = K.surface_deposit(b, key, mg.nb, snap.nf, mg.v, snap.ij, snap.t, fslot, beam.eta_s, 0.0,
                                                    out["T"].astype(F64), np.zeros(4 * snap.nf))
            assert np.array_equal((K.key_face(key)[0] >= mg.nb), ref["surf"])
            for slot in np.nonzero(summed)[0]:
                nd = int(unode[slot])
                assert abs(power[slot] - ref["power"][nd]) <= ref["power_bound"][nd], nd
            assert {int(unode[s_]) for s_ in np.nonzero(summed)[0]} == set(ref["power"])


# ---- the preconditions of the GPU cases ----------------------------------------------------------------------------------------
def test_bin_cases_hold_what_they_are_named_for():
    for n in K.BIN_N:
        for P in K.BIN_P:
            b, coord, special = K.bin_case(n, P)
            cell, count, outside = K.laser_bin(coord, b)
            assert len(count) == n * n + ((P - 1) >> 3) + 1 and count.sum() == P
            assert cell.max() < len(count) and np.array_equal(cell[outside], n * n + (np.flatnonzero(outside) >> 3))
            u, v, _ = K.project(coord, b)
            by = {name: i for i, name in special.items()}
            assert not outside[by["minus_half"]] and cell[by["minus_half"]] == 0
            if P == 1:
                continue
            assert len(by) == 8 and outside.any() and (~outside).any()
            for k in ("plus_half_u", "plus_half_v", "far", "nan"):
                assert outside[by[k]], k
            assert np.isnan(coord[by["nan"]]).all() and u[by["plus_half_u"]] == n // 2 * K.H == -u[by["minus_half"]]
            for k, w in (("edge_u", u), ("edge_v", v), ("corner", u), ("corner", v)):    # exactly on an interior column edge
                q = w[by[k]] / K.H
                assert q == np.floor(q) and -n // 2 <= q < n // 2 and not outside[by[k]], k
    b, coord, _ = K.bin_case(16, 1000, "oblique")
    assert abs(b.e1 @ b.dir) < 4 * EPS and not np.array_equal(b.e1, [1.0, 0.0, 0.0])


def test_hit_cases_hold_what_they_are_named_for():
    b, tri_v, names, uvs = K.hit_case(257)
    assert set(names) == set(K.hit_specials()[0])
    u, v, s = K.project(tri_v, b)
    ok = ~np.isnan(uvs).any(axis=(1, 2)) & (np.arange(257) < len(names))     # the named faces are dyadic: projected exactly
    assert np.array_equal(u[ok], uvs[ok][:, :, 0]) and np.array_equal(v[ok], uvs[ok][:, :, 1]) and np.array_equal(s[ok], uvs[ok][:, :, 2])
    key = K.laser_hit(tri_v, b, K.HIT_S_LO, K.HIT_SCALE)
    face, field = K.key_face(key)
    per = [K.face_columns(tri_v[f], b) for f in range(257)]
    cols = lambda k: set(per[names[k]][0][per[names[k]][1]].tolist())        # noqa: E731  (the columns whose centre the face holds)
    true_depth = lambda k: uvs[names[k]][0, 2]                                # noqa: E731  (flat faces)
    q = lambda k: set(K.depth_field(per[names[k]][3][per[names[k]][1]], K.HIT_S_LO, K.HIT_SCALE).tolist())   # noqa: E731
    # shared edge and shared vertices: centres with an edge function exactly 0 in both faces, the shallower face wins them
    both = cols("diag_deep") & cols("diag_shallow")
    assert len(both) == 4
    cu, cv = b.beam.centres()
    for k in ("diag_deep", "diag_shallow"):
        f = names[k]
        w = np.stack(K.edge_functions(u[f], v[f], cu[sorted(both)], cv[sorted(both)]), 1)
        assert ((w == 0).sum(axis=1) >= 1).all() and ((w == 0).sum(axis=1) == 2).sum() == 2    # two of them on a vertex
    assert all(face[c] == names["diag_shallow"] for c in both)
    assert (face == names["diag_deep"]).any()
    # identical depth: the lower index; the second copy is the same triangle with the other orientation
    assert cols("coplanar_first") == cols("coplanar_second") and len(cols("coplanar_first")) >= 6
    assert all(face[c] == names["coplanar_first"] for c in cols("coplanar_first"))
    w = np.stack(K.edge_functions(u[names["coplanar_second"]], v[names["coplanar_second"]], cu, cv), 1)
    assert (w <= 0).all(axis=1).any() and not (w > 0).all(axis=1).any()       # back-facing
    # one grid step: equal quantised depth, different true depth, the deeper one first in the list wins
    assert true_depth("tie_deeper_first") > true_depth("tie_shallower_second") and names["tie_deeper_first"] < names["tie_shallower_second"]
    assert q("tie_deeper_first") == q("tie_shallower_second") and len(q("tie_deeper_first")) == 1
    assert all(face[c] == names["tie_deeper_first"] for c in cols("tie_deeper_first")) and len(cols("tie_deeper_first")) >= 6
    # two steps or more: the shallower one wins although it is second
    qa, qb = q("separated_deeper_first"), q("separated_shallower_second")
    assert len(qa) == len(qb) == 1 and min(qa) - max(qb) >= 2
    assert all(face[c] == names["separated_shallower_second"] for c in cols("separated_shallower_second"))
    # the clamps
    top = K.HIT_S_LO + 2.0 ** 40 / K.HIT_SCALE
    for k in ("below_first", "below_second"):
        assert true_depth(k) < K.HIT_S_LO and q(k) == {0}
    for k in ("top_exact", "top_beyond"):
        assert true_depth(k) >= top and q(k) == {2 ** 40 - 1}
    assert all(face[c] == names["below_first"] and field[c] == 0 for c in cols("below_first"))
    assert all(face[c] == names["top_exact"] and field[c] == 2 ** 40 - 1 for c in cols("top_exact"))
    # faces that win nothing
    for k in ("zero_area", "nan_vertex", "outside"):
        assert not cols(k) and not (face == names[k]).any(), k
    i0, i1, j0, j1 = K.column_range(u[names["outside"]], v[names["outside"]], b)
    assert i1 < i0                                                            # an empty column range
    i0, i1, j0, j1 = K.column_range(u[names["zero_area"]], v[names["zero_area"]], b)
    assert i0 <= i1 and j0 <= j1                                              # (its box holds centres: tri_hit refuses)
    assert cols("under_both") and all(face[c] == names["under_both"] for c in cols("under_both"))
    un, vn = u[names["straddle"]], v[names["straddle"]]
    assert un.max() > 8 * K.H and vn.max() > 8 * K.H and cols("straddle") and all(face[c] == names["straddle"] for c in cols("straddle"))
    assert (face == 256).any() and (face >= len(K.hit_specials()[0])).sum() > 50   # the last face and the fillers win columns
    assert (face < 0).any()
    # every key fits its bit field
    live = key != U64(K.NO_HIT)
    assert (field[live] < 2 ** 40).all() and (face[live] < 257).all()
    for nf in K.HIT_NF:
        for d in ("vertical", "oblique"):
            bb, tv, _, _ = K.hit_case(nf, d)
            kk = K.laser_hit(tv, bb, K.HIT_S_LO, K.HIT_SCALE)
            ff, fd = K.key_face(kk)
            assert (ff >= 0).any() and ff.max() < nf and (fd[ff >= 0] < 2 ** 40).all() and bb.n % 2 == 0


@needs_ld
def test_column_cases_hold_what_they_are_named_for():
    assert set((0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1100)) <= set(K.RUNS_N4)
    assert len(K.RUNS_N4) == 16 and len(K.runs_n6()) == 36 and -(-1100 // K.CAP) == 3 and -(-36 // 4) == 9
    for n, lengths in ((4, K.RUNS_N4), (6, K.runs_n6())):
        for poly in (False, True):
            c = K.column_case(n, lengths, poly)
            assert np.array_equal(np.diff(c["cell_start"]), lengths)          # every listed run length is produced
            assert np.array_equal(np.sort(c["order"]), np.arange(c["P"]))
            P0 = c["cell_start"][-1]
            assert c["P"] == P0 + K.EXTRA
            o = K.run_columns(c)
            assert o["S_max"] < 30.0 and (n != 4 or o["S_max"] > 15.0)       # nothing underflows; the bound stays meaningful
            x = c["sorted6"].reshape(-1, 6)[:, :3]
            s = K.project(x, c["b"])[2]
            assert np.isfinite(s).all()                                       # no particle depth is non-finite
            assert np.array_equal(o["written"], np.isin(np.arange(c["P"]), c["order"][:P0]))
            if poly:
                r = c["sorted_r"]
                assert r.max() / r.min() > 3.9 and r.max() / r.min() <= 4.0
            scr = np.corrcoef(c["order"][:P0], np.arange(P0))[0, 1]
            assert abs(scr) < 0.1                                             # ids scrambled against position
            ties = long_block = at_hit = behind = 0
            for col, ln in enumerate(lengths):
                lo = c["cell_start"][col]
                _, cnt = np.unique(s[lo:lo + ln], return_counts=True)
                ties += (cnt > 1).sum()
                long_block += (cnt > K.WAVE).sum()
                if o["has"][col]:
                    at_hit += (s[lo:lo + ln] == o["s_hit"][col]).sum()
                    behind += (s[lo:lo + ln] == np.nextafter(o["s_hit"][col], 1.0)).sum()
                    assert o["lit"][lo:lo + ln][s[lo:lo + ln] == o["s_hit"][col]].all()
            assert ties > 10 and at_hit >= 1 and behind >= 1 and (n != 4 or long_block >= 3)
            assert o["rate_exact0"].sum() > 10 and (o["rate"][o["rate_exact0"]] == 0).all()
            assert set(o["col_face"]) == {-1, 7, -43}                         # a boundary id, a facet id -2 - tet, none
            lp = o["k_id"] >= 0
            assert lp.sum() == sum(ln for ln in lengths if ln > K.CAP) and lp.any()
            # permuting positions changes nothing in the model either
            o2 = K.run_columns(K.permuted(c))
            assert np.array_equal(o["rate"], o2["rate"]) and np.array_equal(o["k_id"], o2["k_id"]) and np.array_equal(o["T"], o2["T"])
    c = K.column_case(4, K.RUNS_N4, True)
    hit_long = [ln for col, ln in enumerate(K.RUNS_N4) if K.run_columns(c)["has"][col]]
    assert max(hit_long) > K.CAP and min(hit_long) <= 3                       # s > s_hit decides in both sort paths


def test_deposit_tally_and_list_models():
    for ns in K.LIST_SIZES:
        d = K.deposit_case(ns)
        power, energy = K.laser_deposit(ns, d["soff"], d["sface"], d["tri_v"], d["b"], d["eta_s"], d["dt"], d["colkey"], d["col_T"],
                                        d["energy"])
        assert np.array_equal(energy, d["energy"] + d["dt"] * power) and (power >= 0).all() and (power > 0).any()
        assert ((d["sface"] >> 2) < 257).all() and set((d["sface"] & 3).tolist()) == {0, 1, 2}
        face, _ = K.key_face(d["colkey"])
        won = np.isin(np.arange(257), face)
        assert not won[d["names"]["tie_shallower_second"]] and not won[d["names"]["separated_deeper_first"]]
        assert not won[d["names"]["coplanar_second"]]                         # its columns were won by another face
        if ns > 1:
            assert d["soff"][ns] == d["soff"][ns - 1] and power[ns - 1] == 0 and not np.signbit(power[ns - 1])   # no faces
            assert d["soff"][1] - d["soff"][0] == 3 and power[0] == 0         # node 0: its face won no column
        total = sum((d["eta_s"] * d["col_T"][c]) for c in np.nonzero(face >= 0)[0])
        if ns > 1:                                                            # every vertex of every face is some node's
            assert abs(power.sum() - total) <= 1e-12 * total
    for ncol in K.TALLY_NCOL:
        part = np.random.default_rng(ncol).uniform(0.0, 1.0, 6 * ncol)
        out = K.laser_tally(ncol, 10.0, part)
        ref = part.reshape(6, ncol).astype(LD).sum(axis=1)
        assert abs(out[0] - (10.0 - float(ref[0]))) <= ncol * EPS * float(ref[0]) + 16 * EPS
        assert np.all(np.abs(out[1:] - ref[1:].astype(F64)) <= 12 * EPS * ref[1:].astype(F64))
    part = np.zeros(6 * 257)
    part[256], part[0], part[1] = 1.0, 2.0 ** -53, 2.0 ** -53               # thread 0: (2^-53 + 1) -> 1; the tree adds 2^-53 again
    assert K.laser_tally(257, 0.0, part)[0] == -1.0
    e, q = K.list_source_add(2, [3, 0, 1], 0.5, [2.0, 4.0, 8.0], [1.0, 1.0, 1.0, 1.0])
    assert e.tolist() == [0.0, 0.0, 8.0] and q.tolist() == [3.0, 1.0, 1.0, 2.0]
    assert K.surface_power(4, 2, [3, 0, 1], [5.0, 6.0, 7.0]).tolist() == [6.0, 0.0, 0.0, 5.0]
    e, c = K.surface_carry(1, [2, 0], [5.0, 6.0], [1.0, 1.0, 1.0])
    assert e.tolist() == [0.0, 6.0] and c.tolist() == [1.0, 1.0, 6.0]


def test_snapshot_cases_hold_what_they_are_named_for():
    from dedflow_amd.meshgen import kuhn_cube
    for mask in range(16):
        n = []
        for side in (1, -1):
            for direction in ((0.0, 0.0, -1.0), (0.6, 0.0, 0.8), (-0.28, 0.96, 0.0)):
                xg, ien, phi, level = K.single_tet(mask)
                n.append(K.Snapshot(xg, ien, phi, level, side, direction, 1).nf)
        want = 0 if mask in (0, 15) else (2 if bin(mask).count("1") == 2 else 1)
        assert set(n) == ({0, want})                                          # every mask: 0, 1 or 2 facets, for one of the sides
        xg, ien, phi, level = K.single_tet(mask, at_level=0)
        assert phi[0] == level                                                # a node exactly at the level is not positive
    m = kuhn_cube(5, jitter=0.2)
    ien = np.asarray(m.ien).reshape(-1, 4)
    assert len(ien) == 750 == K.SNAP_NT[-1]
    fields = K.snapshot_fields(m)
    count = {}
    for name, (xg, phi, level, direction) in fields.items():
        for side in (1, -1):
            s = K.Snapshot(xg, ien, phi, level, side, direction, 750)
            count[name, side] = s.nf
            assert s.blk_count.sum() == s.nf and len(s.blk_count) == 3 and (s.ij < 2 ** 12).all()
            assert np.isfinite(s.F).all() and np.isfinite(s.t).all()
            for v in range(3):
                i, j = (s.ij >> (4 * v)) & 3, (s.ij >> (4 * v + 2)) & 3
                assert (i != j).all()
    assert count["plane_vertical", -1] > 150 and count["plane_vertical", 1] == 0
    assert count["sphere", 1] > 20 and count["sphere", -1] > 20               # g . dir has both signs over the sphere
    assert 0 < count["perpendicular", 1] and 0 < count["perpendicular", -1]   # ... and in rounding noise around 0
    assert count["in_plane", 1] == 0 == count["in_plane", -1]
    xg, phi, level, direction = fields["in_plane"]
    cut = np.unique(K.rm.facets(xg, ien, phi, level)[1])
    assert len(cut) > 50
    x, ph = xg[ien[cut]], phi[ien[cut]]
    e1, e2, e3 = x[:, 1] - x[:, 0], x[:, 2] - x[:, 0], x[:, 3] - x[:, 0]
    gz = ((ph[:, 1] - ph[:, 0]) * K.rm.cross(e2, e3)[:, 2] + (ph[:, 2] - ph[:, 0]) * K.rm.cross(e3, e1)[:, 2]) \
        + (ph[:, 3] - ph[:, 0]) * K.rm.cross(e1, e2)[:, 2]
    assert (gz == 0).all()                                                    # g . dir == 0 exactly
    xg, phi, level, direction = fields["constant_tets"]
    assert all(len(set(phi[ien[e]])) == 1 for e in range(0, 50, 5))
    s = K.Snapshot(xg, ien, phi, level, -1, direction, 750)
    assert s.nf > 0 and (s.per_tet[0:50:5] == 0).all()                        # a tet with constant phi has no facet, its neighbours do
    # one NaN phi and one inf coordinate cost only their own tets
    xg, phi, level, direction = fields["nan_and_inf"]
    bad_nodes = np.r_[np.flatnonzero(np.isnan(phi)), np.flatnonzero(~np.isfinite(xg).all(axis=1))]
    assert len(bad_nodes) == 2
    touched = np.isin(ien, bad_nodes).any(axis=1)
    full = K.Snapshot(fields["plane_vertical"][0], ien, fields["plane_vertical"][1], level, -1, direction, 750)
    cut_ = K.Snapshot(xg, ien, phi, level, -1, direction, 750)
    assert np.array_equal(cut_.tet, full.tet[~touched[full.tet]]) and 0 < touched[full.tet].sum() < 60
    assert (full.per_tet == 2).any() and (full.per_tet[256:] == 2).any()


def test_nodes_and_surface_deposit_cases():
    for nfs in K.NODES_NFS:
        ien, tet = K.nodes_case(nfs)
        assert ien.dtype == np.int32 and ien.min() == 0 and ien.max() == 2 ** 31 - 1 and tet.max() < len(ien) and len(tet) == nfs
        assert nfs == 1 or tet[0] == tet[1]                                   # two facets of one tet share slots
        unode, fslot = K.surface_nodes(ien, tet)
        assert unode[0] == 0 and unode[-1] == 2 ** 31 - 1 and (np.diff(unode) > 0).all()
        assert np.array_equal(unode[fslot], ien[tet].reshape(-1)) and (nfs == 1 or len(unode) < 4 * nfs)
        assert all(len(set(r)) == 4 for r in ien.tolist())
    seen = set()
    for n, kind, nfb in ((2, "one", 0), (2, "many", 5), (16, "many", 0), (16, "many", 5), (16, "one", 5), (64, "one", 0),
                         (64, "many", 5), (256, "many", 5)):
        d = K.surface_deposit_case(n, kind, nfb)
        face, field = K.key_face(d["colkey"])
        assert 4 * d["b"].ncol <= 2 ** K.REC_BITS and d["fslot"].max() < 4 * d["nfs"] and (field[face >= 0] < 2 ** 40).all()
        assert all(len(set(r)) == 4 for r in d["fslot"].reshape(-1, 4).tolist())
        power, energy, val, summed = K.surface_deposit(d["b"], d["colkey"], nfb, d["nfs"], d["cand_v"], d["ij"], d["t"], d["fslot"],
                                                       d["eta_s"], d["dt"], d["col_T"], d["energy"])
        assert summed.any() and np.array_equal(energy[~summed], d["energy"][~summed]) and (power[~summed] == 0).all()
        if kind == "one":
            assert (face[face >= nfb] == nfb).all() and d["nfs"] == 1
            if nfb == 0:
                assert (face == 0).all()                                      # one facet over the whole grid: runs of n n terms
        elif n >= 16:
            assert (face < 0).any()                                           # columns that hit nothing
        if nfb and n >= 16:
            assert ((face >= 0) & (face < nfb)).any()                         # columns that hit a boundary record
        seen.add((n, nfb))
    assert {n for n, _ in seen} == set(K.SURF_N) and {f for _, f in seen} == {0, 5}
