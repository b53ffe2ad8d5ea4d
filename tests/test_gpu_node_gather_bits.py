"""Bit parity of the node-gather passes and the level-set tet geometry with the commit before they were put on one skeleton
(csrc/node_gather.hpp, csrc/tet_levelset.hpp) and one V2E map per mesh.

The fixtures tests/golden/node_gather/{cube6,fan}.npz were written by tools/dump_node_gather_bits.py on that parent commit
(its hash is the `commit` entry of each file) and hold the inputs as well as the raw outputs: the tests rebuild the mesh, the
state and the particles from the file, run the same calls through the tool's own `run` and compare every output byte for
byte -- DflMeshSurfaceLoad (load, heat, area), DflMeshPhaseCoefficients (D, H, G, without and with use_phi),
DflAssembleScalarJacobian (both value arrays) and the capture decision (surviving tags, captured tets, the deposits' node
sums) -- with the flag passes of the surface and the phase change both off and both on.  cube6 is kuhn_cube(6, jitter=0.2)
(343 nodes: 22 workgroups, the last one partial; interior nodes take two trips); fan is fan_mesh (76 tets on node 0: five
trips while the other three groups of its wave idle)."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "node_gather")
PARENT = "9d013df"


@pytest.fixture(scope="module")
def api():
    from dedflow_amd import api as A
    A.lib()
    return A


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("dump_node_gather_bits", os.path.join(ROOT, "tools", "dump_node_gather_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module", params=["cube6", "fan"])
def golden(request):
    with np.load(os.path.join(GOLDEN, request.param + ".npz")) as f:
        return request.param, {k: f[k] for k in f.files}


def test_fixture_comes_from_the_parent_commit(golden, tool):
    """and holds every input and sixteen non-trivial outputs"""
    name, g = golden
    assert str(g["commit"]).startswith(PARENT)
    outs = [k for k in g if k.startswith("out_")]
    assert len(outs) == 16
    for k in outs:                                                # nothing compares empty or all-zero arrays
        assert g[k].size and np.count_nonzero(g[k]), k
    assert sorted(k for k in g if not k.startswith("out_") and k != "commit") == sorted(
        ["mesh_" + k for k in tool.MESH_FIELDS] + ["in_w", "in_dw", "in_eps", "in_pts", "in_vel", "in_temp"])


@pytest.mark.parametrize("flags", ["0", "1"], ids=["flag_passes_off", "flag_passes_on"])
def test_every_output_has_the_parents_bits(api, tool, golden, flags, monkeypatch):
    name, g = golden
    monkeypatch.setenv("DFL_SURFACE_FLAGS", flags)
    monkeypatch.setenv("DFL_PHASE_FLAGS", flags)
    got = tool.run(api, g)
    want = {k: v for k, v in g.items() if k.startswith("out_")}
    assert sorted(got) == sorted(want)
    differ = [k for k in want if not tool.same_bits(got[k], want[k])]
    assert not differ, (name, differ)
