"""CPU checks of the free-surface model (tests/surface_model.py; include/dedflow.h "free-surface forces") against closed
forms: what the kernel is compared with in test_gpu_surface.py has to be the physics first.  No GPU; the last test also runs
the library's own configuration check, which is host arithmetic."""
import ctypes as C

import numpy as np
import pytest

import surface_model as sm
from dedflow_amd.meshgen import kuhn_cube

LD = np.longdouble
TILT = np.array([0.2, -0.3, 1.0]) / np.sqrt(1.13)


def _x(m):
    return m.xg.reshape(-1, 3)


def _plane(m, n=TILT):
    return (_x(m) - 0.5) @ n


def _run(m, phi, T, **cfg):
    cfg = sm.config(**cfg)
    load, heat, area, active, t = sm.surface_load(m.xg, m.ien, sm.state(m.num_node, phi, T), cfg)
    return dict(load=load, heat=heat, area=area, active=active, t=t, A=area.sum())


_cache = {}


def _mesh(M, jitter=0.2):
    if (M, jitter) not in _cache:
        _cache[M, jitter] = kuhn_cube(M, jitter=jitter)
    return _cache[M, jitter]


@pytest.mark.parametrize("M", [4, 12, 24])
def test_momentum_and_virial(M):
    """recoil off: sum_a f_a = 0 and sum_a x_a . f_a = -2 S in every tet (sum_a grad N_a = 0, sum_a x_a (x) grad N_a = I), with
    a temperature field that makes sigma vary (Marangoni on)"""
    m = _mesh(M)
    T = 2000.0 + 800.0 * _x(m)[:, 0]
    o = _run(m, _plane(m), T, eps=2.0 / M, sigma0=1.8, dsigma_dT=-4e-4, T_ref=1900.0)
    tot = np.abs(o["load"].sum(axis=0)).max()
    print(f"M={M} |sum load| / (sigma0 A) = {float(tot / (1.8 * o['A'])):.2e}")
    assert tot <= 1e-12 * 1.8 * o["A"]
    virial = (o["load"] * _x(m).astype(LD)).sum()
    want = -2 * o["t"]["S"].sum()
    print(f"M={M} virial relative error {float(abs(virial - want) / abs(want)):.2e}")
    assert abs(virial - want) <= 1e-12 * abs(want)


@pytest.mark.parametrize("M", [12, 24])
@pytest.mark.parametrize("width", [1.5, 2.5])
def test_area_of_a_tilted_plane(M, width):
    m = _mesh(M)
    o = _run(m, _plane(m), 0.0, eps=width / M, sigma0=1.0)
    want = 1.0 / TILT[2]
    print(f"M={M} eps={width}h area {float(o['A']):.5f} (1 / n_z = {want:.5f})")
    assert abs(float(o["A"]) - want) <= 0.01 * want


@pytest.mark.parametrize("width", [1.5, 2.5])
def test_sphere_area_and_laplace_pressure(width):
    M, R, sigma0 = 12, 0.3, 1.7
    m = _mesh(M)
    r = _x(m) - 0.5
    rn = np.sqrt((r * r).sum(axis=1))
    o = _run(m, rn - R, 0.0, eps=width / M, sigma0=sigma0)
    area = float(o["A"]) / (4 * np.pi * R * R)
    radial = float((o["load"] * (r / rn[:, None])).sum())      # (jittered mesh: no node sits on the centre)
    force = radial / (-2 * sigma0 / R * 4 * np.pi * R * R)
    print(f"sphere eps={width}h area ratio {area:.4f} force ratio {force:.4f}")
    assert 0.95 <= area <= 1.06
    assert 0.95 <= force <= 1.05


@pytest.mark.parametrize("M", [16, 32])
def test_marangoni_force_of_a_linear_temperature(M):
    """plane z = 0.5, sigma = 1 + 0.7 (x - 0.5): tested with the pyramid psi of half-width 0.3 about the axis x = y = 0.5 the
    tangential force is int psi dsigma/dx dA = 0.7 * 0.36 / 3"""
    m = _mesh(M, 0.0)
    x = _x(m)
    o = _run(m, x[:, 2] - 0.5, x[:, 0] - 0.5, eps=2.0 / M, sigma0=1.0, dsigma_dT=0.7)
    psi = np.maximum(0.0, 1.0 - np.maximum(np.abs(x[:, 0] - 0.5), np.abs(x[:, 1] - 0.5)) / 0.3).astype(LD)
    fx, fz = float((psi * o["load"][:, 0]).sum()), float((psi * o["load"][:, 2]).sum())
    print(f"M={M} Marangoni force {fx:.5f} (0.084), z component {fz:.2e}")
    assert abs(fx - 0.084) <= 0.01 * 0.084
    assert abs(fz) < 1e-15


def test_flat_surface_at_rest():
    """constant sigma on a plane: the interior of the surface is in equilibrium"""
    M, sigma0 = 12, 1.8
    m = _mesh(M)
    o = _run(m, _plane(m), 0.0, eps=2.0 / M, sigma0=sigma0)
    x = _x(m)
    inner = (np.minimum(x, 1.0 - x).min(axis=1) > 3.0 / M) & o["active"]
    assert inner.sum() > 50
    worst = float(np.sqrt((o["load"][inner] ** 2).sum(axis=1)).max())
    print(f"flat surface: max interior |load| / (sigma0 h) = {worst / (sigma0 / M):.2e} over {inner.sum()} nodes")
    assert worst <= 2e-3 * sigma0 / M


@pytest.mark.parametrize("side", [1, -1])
def test_recoil_on_the_flat_surface(side):
    """uniform T: the recoil pressure p pushes on the area A along side n, into the metal (side (phi - level) > 0); the
    surface tension next to it sums to zero"""
    M = 12
    m = _mesh(M)
    cfg = dict(eps=2.0 / M, sigma0=1.8, recoil_p0=1.0e5, recoil_a=11.0, T_boil=3100.0)
    o = _run(m, _plane(m), 3300.0, side=side, **cfg)
    p = float(sm.recoil(sm.config(**cfg), 3300.0))
    assert p > 1.0e5
    want = side * p * TILT * float(o["A"])
    tot = o["load"].sum(axis=0).astype(float)
    print(f"recoil side={side}: sum load / (p A) = {tot / (p * float(o['A']))} (side n = {side * TILT})")
    assert np.abs(tot - want).max() <= 0.01 * p * float(o["A"])
    # side = -1 flips exactly the recoil part
    both = {s: _run(m, _plane(m), 3300.0, side=s, **cfg)["load"] for s in (1, -1)}
    none = _run(m, _plane(m), 3300.0, side=1, **dict(cfg, recoil_p0=0.0))["load"]
    assert np.abs((both[1] - none) + (both[-1] - none)).max() <= 1e-17 * p / M ** 2
    assert np.abs(both[1] - none).max() > 0.0


@pytest.mark.parametrize("which", ["h_conv", "emissivity", "evap_q0"])
def test_heat_loss_on_the_flat_surface(which):
    M, T = 12, 3200.0
    m = _mesh(M)
    cfg = dict(eps=2.0 / M, sigma0=1.8, T_amb=300.0, recoil_a=11.0, T_boil=3100.0)
    cfg[which] = {"h_conv": 80.0, "emissivity": 0.4, "evap_q0": 2.0e9}[which]
    o = _run(m, _plane(m), T, **cfg)
    want = -sm.loss(sm.config(**cfg), T) * o["A"]
    assert want < -1.0
    print(f"{which}: sum q_heat {float(o['heat'].sum()):.6e}, -loss A {float(want):.6e}")
    assert abs(o["heat"].sum() - want) <= 1e-12 * abs(want)
    others = _run(m, _plane(m), T, **dict(cfg, **{which: 0.0}))
    assert not others["heat"].any()


BAD = [("side", dict(side=0)), ("side", dict(side=2)), ("eps", dict(eps=0.0)), ("eps", dict(eps=-0.1)), ("eps", dict(eps=np.inf)),
       ("eps", dict(eps=np.nan)), ("sigma0", dict(sigma0=np.nan)), ("dsigma_dT", dict(dsigma_dT=np.inf)),
       ("T_ref", dict(T_ref=-np.inf)), ("level", dict(level=np.nan)), ("recoil_a", dict(recoil_a=np.nan)),
       ("h_conv", dict(h_conv=np.inf)), ("emissivity", dict(emissivity=np.nan)), ("T_amb", dict(T_amb=np.nan)),
       ("evap_q0", dict(evap_q0=np.inf)), ("recoil_p0", dict(recoil_p0=np.nan)),
       ("T_boil", dict(recoil_p0=1.0, T_boil=0.0)), ("T_boil", dict(evap_q0=1.0, T_boil=-5.0)), ("T_boil", dict(T_boil=np.nan))]


def test_refusals():
    """every bad configuration is refused by the model and, for the same reason, by the library's own check"""
    from dedflow_amd import api
    L = api.lib()
    why = C.create_string_buffer(160)

    def library(cfg):
        c = api.DflSurfaceForces(*[float(cfg[k]) if k not in ("side", "in_time_step") else int(cfg[k]) for k in sm.DEFAULTS])
        return L.DflSurfaceForcesCheck(C.byref(c), why, 160), why.value.decode()

    good = dict(eps=0.1, sigma0=1.8, dsigma_dT=-4e-4, T_ref=1900.0, recoil_p0=1e5, recoil_a=11.0, T_boil=3100.0, h_conv=80.0,
                emissivity=0.4, T_amb=300.0, evap_q0=2e9)
    assert sm.refusal(sm.config(**good)) is None and library(sm.config(**good))[0] == 0
    assert sm.refusal(sm.config(eps=0.1, T_boil=0.0)) is None and library(sm.config(eps=0.1, T_boil=0.0))[0] == 0
    for reason, change in BAD:
        cfg = sm.config(**dict(good, **change))
        assert sm.refusal(cfg) == reason, (reason, change)
        rc, text = library(cfg)
        assert rc != 0 and reason in text, (reason, change, text)
