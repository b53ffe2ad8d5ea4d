"""bench.py on a small mesh: a plain run prints the headline line and nothing that takes a leg of its own; --full adds the
per-kernel, roofline, CPU-baseline, solve-to-rtol, DEM and coupled-step figures on top of the same headline keys."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEADLINE = {"metric": str, "value": float, "unit": str, "higher_is_better": bool, "dtype": str, "ms_per_step": float}
FULL_ONLY = ("kernels", "roofline", "spmv_GBps", "spmv_back_to_back_ms", "assemble_J_ms", "assemble_F_ms", "solve_to_rtol",
             "cpu_baseline", "dem_sweep", "coupled_step")


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--M", "14", "--steps", "3", "--warmup", "1", *args],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _check_headline(d):
    for key, kind in HEADLINE.items():
        assert isinstance(d[key], kind), (key, d[key])
    assert d["unit"] == "DOF/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["value"] == pytest.approx(4.0 * 15 ** 3 / (d["ms_per_step"] * 1e-3), rel=1e-12)


def test_plain_run_is_the_headline_only(tmp_path):
    d = _bench("--dump-outputs", str(tmp_path))
    _check_headline(d)
    assert not [k for k in FULL_ONLY if k in d]
    assert d["gmres_residual_drop"] < 1.0
    stats = np.load(tmp_path / "solve_stats.npy")
    assert stats[0] == 40 and np.isfinite(np.load(tmp_path / "x.npy")).all()


def test_full_run_adds_the_other_legs():
    d = _bench("--full", "--cpu-M", "8", "--cpu-single-M", "6", "--coupled-M", "8", "--dem-particles", "2000")
    _check_headline(d)
    missing = [k for k in FULL_ONLY if k not in d]
    assert not missing, missing
    assert d["kernels"]["spmv"]["launches"] > 0 and d["roofline"]["achieved"] > 0
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["single_thread"]["value"] > 0
    assert d["solve_to_rtol"]["converged"] and d["dem_sweep"]["particles"] == 2000
    assert d["coupled_step"]["ms_per_coupled_step"] > 0
