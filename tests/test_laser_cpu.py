"""CPU checks of the laser energy deposition: tests/laser_model.py against closed forms, and the drop-in boundary (the
header declares the entry points of the section and the built library exports them).  No GPU."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np

import laser_model as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUBLIC = ["ParticleContextSetLaser", "ParticleContextLaserStep", "ParticleContextLaserRate", "ParticleContextLaserTally",
          "ParticleContextLaserColumns"]
KERNELS = ["dfl_laser_column_cap", "dfl_laser_bin", "dfl_laser_hit", "dfl_laser_columns", "dfl_laser_deposit",
           "dfl_laser_tally", "dfl_laser_source_add"]
EPS = lm.EPS


def _header(name):
    txt = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_declares_and_library_exports_the_laser():
    pub, ker = _header("dedflow.h"), _header("dedflow_kernels.h")
    for n in PUBLIC:
        assert re.search(r"\b%s\s*\(" % n, pub), n
    for n in KERNELS:
        assert re.search(r"\b%s\s*\(" % n, ker), n
    for field in ("origin", "dir", "scan_vel", "power", "r_cut", "eta_p", "eta_s", "substrate_groups"):
        assert re.search(r"\b%s\b" % field, pub[pub.index("typedef struct DflLaser"):]), field
    assert re.search(r"const\s+dfl_value\s*\*\s*laser", ker[ker.index("void dfl_heat_update"):])   # the nullable pointer
    subprocess.check_call(["make", "-s", "-j8", "-C", ROOT])
    lib = ctypes.CDLL(os.path.join(ROOT, "dedflow_amd", "libdedflow.so"))
    missing = [n for n in PUBLIC + KERNELS if not hasattr(lib, n)]
    assert not missing, missing
    lib.dfl_laser_column_cap.restype = ctypes.c_int32
    assert lib.dfl_laser_column_cap() >= 64


def _beam(**kw):
    a = dict(origin=(0.5, 0.5, 1.0), direction=(0.0, 0.0, -2.0), power=200.0, w=0.05, h=0.01, r_cut=0.08, eta_p=0.4, eta_s=0.3)
    a.update(kw)
    return lm.Beam(**a)


def test_frame_is_orthonormal_and_fixed():
    b = _beam()
    assert np.array_equal(b.dir, [0.0, 0.0, -1.0]) and np.array_equal(b.e1, [1.0, 0.0, 0.0]) and np.array_equal(b.e2, [0.0, -1.0, 0.0])
    b = _beam(direction=(0.3, -0.2, -0.9))
    M = np.stack([b.e1, b.e2, b.dir])
    assert np.abs(M @ M.T - np.eye(3)).max() < 4 * EPS and np.linalg.det(M) > 0
    assert b.n == 16 and b.ncol == 256


def test_no_particles_tally_is_the_closed_form():
    b = _beam()
    o = lm.step(b, np.zeros((0, 3)), np.zeros(0))
    t = o["tally"]
    outside = b.power * (1.0 - math.erf(math.sqrt(2.0) * b.r_edge / b.w) ** 2)
    bound = (b.ncol + 8) * EPS * b.power
    assert abs(float(t["outside"]) - outside) <= bound
    assert abs(float(t["missed"]) - (b.power - outside)) <= bound
    assert t["absorbed_particles"] == 0 and t["scattered"] == 0 and t["substrate"] == 0 and t["reflected"] == 0
    assert abs(float(lm.tally_sum(t)) - b.power) <= bound


def test_one_particle_on_the_axis():
    b = _beam()
    r = 0.004
    x = np.array([[0.5 + 0.3 * b.h, 0.5 - 0.4 * b.h, 0.7]])     # column (n/2, n/2 - 1): e2 = -y
    o = lm.step(b, x, r)
    c = b.n // 2 + b.n * (b.n // 2)
    assert o["col"][0] == c
    A, a = math.pi * r * r, b.h * b.h
    exact = b.eta_p * b.column_power()[c] * (1.0 - math.exp(-A / a))
    assert abs(float(o["rate"][0]) - exact) <= 8 * EPS * exact
    assert abs(float(o["T"][c]) - b.column_power()[c] * math.exp(-A / a)) <= 8 * EPS * b.power
    assert abs(float(lm.tally_sum(o["tally"])) - b.power) <= (b.ncol + 1) * EPS * b.power


def test_stack_transmits_exp_minus_k_tau():
    b = _beam()
    r, k = 0.003, 9
    x = np.array([[0.5 + 0.5 * b.h, 0.5 - 0.5 * b.h, 0.9 - 0.05 * j] for j in range(k)])
    o = lm.step(b, x, r)
    c = int(o["col"][0])
    assert (o["col"] == c).all()
    tau = math.pi * r * r / (b.h * b.h)
    pc = b.column_power()[c]
    assert abs(float(o["T"][c]) - pc * math.exp(-k * tau)) <= 16 * EPS * pc
    for j in range(k):                                             # deeper particles are shadowed by the j before them
        exact = b.eta_p * pc * math.exp(-j * tau) * (1.0 - math.exp(-tau))
        assert abs(float(o["rate"][j]) - exact) <= 16 * EPS * exact
    t = o["tally"]
    assert abs(float(t["absorbed_particles"] + t["scattered"]) - pc * (1.0 - math.exp(-k * tau))) <= 32 * EPS * pc
    assert abs(float(lm.tally_sum(t)) - b.power) <= (b.ncol + k) * EPS * b.power


def test_depth_ties_resolve_by_id():
    b = _beam()
    r = 0.004
    x = np.array([[0.5 + 0.2 * b.h, 0.5 - 0.2 * b.h, 0.75], [0.5 + 0.7 * b.h, 0.5 - 0.6 * b.h, 0.75]])
    o = lm.step(b, x, r)
    assert o["col"][0] == o["col"][1] and o["s"][0] == o["s"][1]
    tau = math.pi * r * r / (b.h * b.h)
    assert o["rate"][0] > o["rate"][1]                             # the lower id is lit first
    assert abs(float(o["rate"][1] / o["rate"][0]) - math.exp(-tau)) <= 8 * EPS
    far = lm.step(b, np.array([[0.5 + 3 * b.r_edge, 0.5, 0.7]]), r)  # outside the grid: unlit
    assert far["col"][0] == b.ncol and far["rate"][0] == 0


def test_substrate_model_on_a_flat_face():
    from dedflow_amd.meshgen import kuhn_cube
    m = kuhn_cube(4, jitter=0.0)
    b = _beam(origin=(0.5037, 0.4961, 1.0), h=0.0213, r_cut=0.1)
    sub = lm.Substrate(m, [4], b)
    assert len(sub.id) == 32                                       # the z- face: 4 x 4 x 2 triangles, all facing the beam
    o = lm.step(b, np.zeros((0, 3)), np.zeros(0), sub=sub)
    assert (o["face"] >= 0).all() and o["hit"][4].min() > 1e-9
    t = o["tally"]
    assert abs(float(sum(o["q"].values()) - t["substrate"])) <= (3 * b.ncol) * EPS * b.power
    assert t["missed"] == 0 and abs(float(t["reflected"] / t["substrate"]) - 0.7 / 0.3) <= 1e-13
    z = m.xg.reshape(-1, 3)[:, 2]
    assert all(z[nd] == 0.0 for nd in o["q"])
    assert abs(float(lm.tally_sum(t)) - b.power) <= b.ncol * EPS * b.power
