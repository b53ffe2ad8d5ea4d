"""PC_AMGX host pieces without a GPU: the AMGX option parser (NULL = the reference configuration of krylov.c:413-437, the
inline string and AMGX's JSON form, rejected and ignored keys) and the pairwise aggregation against the numpy model."""
import ctypes as C

import numpy as np
import pytest

from dedflow_amd.meshgen import kuhn_cube
from tests import amgx_model as am


@pytest.fixture(scope="module")
def api():
    from dedflow_amd import api as A
    A.lib()
    return A


def _parse(api, opts):
    cfg = api.DflAMGXConfig()
    rc = api.lib().DflAMGXParseConfig(None if opts is None else opts.encode(), C.byref(cfg))
    return rc, cfg


def _fields(cfg):
    return {f: getattr(cfg, f) for f, _ in cfg._fields_ if f != "unknown_keys"}


REFERENCE = dict(relaxation_factor=0.75, selector_passes=1, smoother=0, presweeps=0, postsweeps=3, max_levels=100,
                 min_coarse_rows=32, max_iters=1)


def test_null_is_the_reference_configuration(api):
    rc, cfg = _parse(api, None)
    assert rc == 0 and _fields(cfg) == REFERENCE


def test_inline_and_json_file_agree(api, tmp_path):
    rc, a = _parse(api, am.REFERENCE_INLINE)
    assert rc == 0 and _fields(a) == REFERENCE and a.unknown_keys == 0
    f = tmp_path / "AMGX.json"
    f.write_text(am.REFERENCE_JSON)
    rc, b = _parse(api, str(f))
    assert rc == 0 and _fields(b) == REFERENCE
    g = tmp_path / "amgx.cfg"            # the inline form in a file, spread over lines
    g.write_text(am.REFERENCE_INLINE.replace(",", ",\n"))
    rc, c = _parse(api, str(g))
    assert rc == 0 and _fields(c) == REFERENCE


def test_values_and_scopes(api):
    rc, c = _parse(api, "config_version=2, solver:preconditioner:smoother=BLOCK_JACOBI, solver:preconditioner:selector=SIZE_8,"
                        "solver:preconditioner:presweeps=2, solver:preconditioner:max_iters=2, solver:max_iters=100,"
                        "solver:preconditioner:relaxation_factor=0.5")
    assert rc == 0 and c.smoother == api.AMGX_SMOOTHER_JACOBI and c.selector_passes == 3 and c.presweeps == 2
    assert c.max_iters == 2 and c.relaxation_factor == 0.5   # solver:max_iters belongs to the outer solver
    # no preconditioner scope: the top-level solver scope carries the AMG parameters (solver=AMG on the whole matrix)
    rc, c = _parse(api, "config_version=2, solver=AMG, algorithm=AGGREGATION, selector=SIZE_4, max_iters=3, postsweeps=1")
    assert rc == 0 and c.selector_passes == 2 and c.max_iters == 3 and c.postsweeps == 1
    # named scopes: solver(main)=FGMRES, main:preconditioner(amg)=AMG, amg:key=value
    rc, c = _parse(api, "config_version=2, solver(main)=FGMRES, main:max_iters=50, main:preconditioner(amg)=AMG,"
                        "amg:smoother=BLOCK_JACOBI, amg:max_iters=2")
    assert rc == 0 and c.smoother == api.AMGX_SMOOTHER_JACOBI and c.max_iters == 2


@pytest.mark.parametrize("bad", ["solver:preconditioner:cycle=W", "solver:preconditioner:algorithm=CLASSICAL",
                                 "solver:preconditioner:smoother=GS", "solver:preconditioner:selector=SIZE_3",
                                 "solver:preconditioner:coarse_solver=NOSOLVER", "solver:preconditioner:presweeps=-1",
                                 "no equals sign here"])
def test_rejected_values(api, bad):
    rc, _ = _parse(api, "config_version=2, " + bad)
    assert rc != 0


def test_unknown_keys_are_ignored(api, capfd):
    rc, c = _parse(api, "config_version=2, solver:preconditioner:postsweeps=2, solver:preconditioner:frobnicate=7, banana=1")
    assert rc == 0 and c.postsweeps == 2 and c.unknown_keys == 2
    err = capfd.readouterr().err
    assert "frobnicate" in err and "banana" in err and err.count("unknown") == 1


def _stiffness(M):
    m = kuhn_cube(M, jitter=0.2)
    return am.p1_stiffness(m), m


@pytest.mark.parametrize("passes", [1, 2, 3])
def test_host_aggregation_matches_model(api, passes):
    A, m = _stiffness(5)
    n = A.shape[0]
    rp, ci, val = A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)
    agg = np.zeros(n, np.int32)
    nc = api.lib().DflAMGXAggregateHost(n, rp.ctypes.data, ci.ctypes.data, val.ctypes.data, passes, agg.ctypes.data)
    ref, nref = am.aggregate(A, passes)
    assert nc == nref and np.array_equal(agg, ref)
    # aggregates numbered by their smallest member; pairwise sizes
    first = np.array([np.nonzero(agg == c)[0][0] for c in range(nc)])
    assert np.all(np.diff(first) > 0)
    assert 1.5 ** passes < n / nc <= 2.0 ** passes + 1


def test_host_aggregation_with_dirichlet_rows(api):
    A, m = _stiffness(5)
    bn = np.unique(m.bound_node)
    A = am.dirichlet_identity(A, bn)
    n = A.shape[0]
    rp, ci, val = A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)
    agg = np.zeros(n, np.int32)
    nc = api.lib().DflAMGXAggregateHost(n, rp.ctypes.data, ci.ctypes.data, val.ctypes.data, 1, agg.ctypes.data)
    ref, nref = am.aggregate(A, 1)
    assert nc == nref and np.array_equal(agg, ref)
    # identity rows have no strong neighbour: they stay singletons
    counts = np.bincount(agg, minlength=nc)
    assert np.all(counts[agg[bn]] == 1)
