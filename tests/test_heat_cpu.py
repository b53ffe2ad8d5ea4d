"""CPU checks of the particle heat transfer: the public and kernel symbols exist, and tests/heat_model.py (the reference of
test_gpu_heat.py) reproduces the closed forms of the model in include/dedflow.h "particle heat transfer"."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import heat_model as hm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUBLIC = ["ParticleContextSetHeat", "ParticleContextTemperature", "ParticleContextHeatRate", "ParticleContextHeatStep",
          "ParticleContextHeatSource", "DflMeshSetHeatSource"]
KERNELS = ["dfl_heat_gather", "dfl_heat_conduction", "dfl_heat_conduction_grid", "dfl_heat_update", "dfl_heat_fill",
           "dfl_couple_node_scalar"]


def _header(name):
    txt = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_heat_symbols_declared_and_exported():
    subprocess.check_call(["make", "-s", "-j8", "-C", ROOT])
    lib = ctypes.CDLL(os.path.join(ROOT, "dedflow_amd", "libdedflow.so"))
    pub, ker = _header("dedflow.h"), _header("dedflow_kernels.h")
    assert "DflParticleHeat" in pub
    for n in PUBLIC:
        assert re.search(r"\b%s\s*\(" % n, pub), n
        assert hasattr(lib, n), n
    for n in KERNELS:
        assert re.search(r"\b%s\s*\(" % n, ker), n
        assert hasattr(lib, n), n
    from dedflow_amd import api
    assert ctypes.sizeof(api.DflParticleHeat) == 48
    for n in ("set_heat", "temperature", "heat_rate", "heat_step", "heat_source"):
        assert hasattr(api.Particles, n), n
    assert hasattr(api.Problem, "set_heat_source")


def test_one_particle_in_a_fluid_at_rest_follows_the_closed_form():
    """Nu = 2: T_n = T_f + (T_0 - T_f) / (1 + dt / tau_T)^n to rounding, and -> exp(-t / tau_T) at first order in dt"""
    R, m, cp_p, k_f = 0.005, 1.0e-3, 2.0, 0.66
    C = m * cp_p
    assert hm.nusselt(0.0, 5.0) == 2.0
    tau = float(hm.tau_T(C, 2.0, k_f, 2 * R))
    T0, Tf = 900.0, 300.0
    errs = []
    for n in (50, 100, 200):
        dt = tau / n * 2.0      # to t = 2 tau
        T = np.array([T0], np.longdouble)
        for k in range(n):
            T, rate, e = hm.update(T, None, C, dt, Tf=np.array([Tf]), tau=np.array([tau]))
        closed = Tf + (T0 - Tf) / (1.0 + np.longdouble(dt) / tau) ** n
        assert abs(float(T[0] - closed)) <= 4 * n * hm.EPS * T0
        errs.append(abs(float(T[0]) - (Tf + (T0 - Tf) * np.exp(-2.0))))
        # without conduction the energy from the fluid is the whole heat of the step
        assert abs(float(e[0] - rate[0] * dt)) <= 1e-12 * abs(float(e[0]))
    assert 1.8 < errs[0] / errs[1] < 2.2 and 1.8 < errs[1] / errs[2] < 2.2, errs


def test_two_touching_particles_conserve_energy_and_relax():
    k_p, cp_p, dt = 40.0, 500.0, 0.5
    r = np.array([0.010, 0.008])
    m = 7800.0 * 4.0 / 3.0 * np.pi * r ** 3
    C = m * cp_p
    x = np.array([[0.5, 0.5, 0.5], [0.5 + 0.0175, 0.5, 0.5]])
    T = np.array([1200.0, 400.0], np.longdouble)
    i, j, dist = hm.contacts_all_pairs(x, r)
    assert sorted(zip(i, j)) == [(0, 1), (1, 0)]
    H = hm.conductance(r[0], r[1], dist[0], k_p)
    assert H == hm.conductance(r[1], r[0], dist[1], k_p) and H > 0.0
    factor = 1.0 - dt * H * (1.0 / C[0] + 1.0 / C[1])
    assert 0.0 < factor < 1.0
    E0 = (C * T).sum()
    for _ in range(40):
        q, _, cnt, _, _ = hm.conduction(x, r, T, k_p)
        assert q[0] == -q[1] and list(cnt) == [1, 1]
        Tn, rate, e = hm.update(T, q, C, dt)
        assert abs(float((Tn[0] - Tn[1]) - factor * (T[0] - T[1]))) <= 8 * hm.EPS * 1200.0
        assert abs(float((C * Tn).sum() - E0)) <= 8 * hm.EPS * float(E0)
        assert np.all(e == 0.0)
        T = Tn
    assert abs(float(T[0] - T[1])) < 800.0 * factor ** 39


def test_all_pairs_and_cell_list_conduction_agree():
    rng = np.random.default_rng(5)
    R = 0.03
    g = 0.1 + 1.9 * R * np.arange(8)
    x = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) + rng.uniform(-0.05 * R, 0.05 * R, (512, 3))
    r = rng.uniform(0.9 * R, R, 512)
    T = rng.uniform(300.0, 1500.0, 512)
    a = hm.contacts_all_pairs(x, r)
    b = hm.contacts_cell_list(x, r, 2.0 * R)
    assert len(a[0]) > 500
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    qa = hm.conduction(x, r, T, 40.0, a)[0]
    qb = hm.conduction(x, r, T, 40.0, b)[0]
    assert np.array_equal(qa, qb)
    assert abs(float(qa.sum())) <= 16 * hm.EPS * float(np.abs(qa).sum())
