"""Bit parity of the "count per workgroup -> scan -> emit in ascending order" passes and of the fixed-tree reductions with the
commit before they were put on one copy of each idiom (csrc/block_ops.hpp, csrc/k_scan.hip, lf_gather_tet / lf_levels of
csrc/level_facets.hpp).

The fixtures tests/golden/compaction/{cube6,fan}.npz were written by tools/dump_compaction_bits.py on that parent commit (its
hash is the `commit` entry of each file) and hold the inputs as well as the raw outputs: the tests rebuild the mesh, the state
and the particles from the file, run the same calls through the tool's own `run` and compare every output byte for byte --
DflMeshRedistance (phi, facets, statistics), DflMeshLevelSetVolume, DflMeshVolumeCorrect towards a drifted target (statistics,
phi), DflMeshPhaseChangeStats, the laser-surface snapshot (facets, tets) and one laser step on it (surface power, heat source,
particle rates -- with +0.0 where the parent wrote -0.0 for a particle behind the hit --, tally) and, on cube6, the accelerations of a DEM sweep whose cell scan has two chunks.  cube6 is
kuhn_cube(6, jitter=0.2) (1296 tets: five full workgroups and one of 16 tets); fan is fan_mesh (76 tets, one workgroup)."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "compaction")
PARENT = "2a46803"
MESH_OUTPUTS = 13


@pytest.fixture(scope="module")
def api():
    from dedflow_amd import api as A
    A.lib()
    return A


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("dump_compaction_bits", os.path.join(ROOT, "tools", "dump_compaction_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module", params=["cube6", "fan"])
def golden(request):
    with np.load(os.path.join(GOLDEN, request.param + ".npz")) as f:
        return request.param, {k: f[k] for k in f.files}


def test_fixture_comes_from_the_parent_commit(golden, tool):
    """and holds every input and thirteen (cube6: fourteen, with the DEM sweep) non-trivial outputs"""
    name, g = golden
    assert str(g["commit"]).startswith(PARENT)
    outs = [k for k in g if k.startswith("out_")]
    assert len(outs) == MESH_OUTPUTS + (name == "cube6") and ("out_dem_acc" in outs) == (name == "cube6")
    for k in outs:                                                # nothing compares empty or all-zero arrays
        assert g[k].size and np.count_nonzero(g[k]), k
    dem = ["in_dem_x", "in_dem_v"] if name == "cube6" else []
    assert sorted(k for k in g if not k.startswith("out_") and k != "commit") == sorted(
        ["mesh_" + k for k in tool.MESH_FIELDS] + ["in_w", "in_ext", "in_pts", "in_substrate", "in_laser_origin"] + dem)
    assert g["out_redistance_facets"].shape[0] == g["out_redistance_stats"][0] > 0     # facets were emitted
    assert g["out_volume_correct"][0] == 0 and g["out_volume_correct"][2] > 0          # corrected, through a band list
    assert len(g["out_laser_surface_tets"]) > 0 and np.count_nonzero(g["out_laser_surface_power"]) > 0
    if name == "cube6":
        assert len(g["mesh_ien"]) // 4 == 5 * 256 + 16 and len(g["in_dem_x"]) == tool.DEM_P


def test_every_output_has_the_parents_bits(api, tool, golden):
    name, g = golden
    got = tool.run(api, g)
    want = {k: v for k, v in g.items() if k.startswith("out_")}
    # the parent wrote -0.0 as the laser_rate of a particle behind its column's hit; the header now fixes +0.0 there
    # (test_gpu_laser_kernels.py).  Every other bit, and every other zero, is the parent's
    r = want["out_laser_surface_rate"]
    behind = (r == 0.0) & np.signbit(r)
    assert behind.any() and ((r == 0.0) & ~np.signbit(r)).any()
    want["out_laser_surface_rate"] = np.where(behind, 0.0, r)
    assert sorted(got) == sorted(want)
    differ = [k for k in want if not tool.same_bits(got[k], want[k])]
    assert not differ, (name, differ)
