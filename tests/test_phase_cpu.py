"""CPU checks of the phase-change model (tests/phase_model.py; include/dedflow.h "phase change") against closed forms: what
the kernels are compared with in test_gpu_phase.py has to be the physics first.  No GPU; the last tests run the library's own
configuration check, which is host arithmetic, and look for the exported symbols."""
import ctypes as C

import numpy as np
import pytest

import phase_model as pm
import surface_model as sm
from dedflow_amd.meshgen import kuhn_box, kuhn_cube

LD = np.longdouble
CFG = dict(T_solidus=1600.0, T_liquidus=1700.0, latent=2.0e9, darcy_c=1.0e6, darcy_b=1e-3)

_cache = {}


def _mesh(M, jitter=0.2):
    if (M, jitter) not in _cache:
        _cache[M, jitter] = kuhn_cube(M, jitter=jitter)
    return _cache[M, jitter]


def _coef(m, T, phi=0.0, **cfg):
    return pm.coefficients(m.xg, m.ien, pm.state(m.num_node, phi, T), pm.config(**cfg))


def test_smooth_step():
    t = np.linspace(-1.5, 1.5, 601).astype(LD)
    H = pm.smooth_step(t)
    assert np.abs(H + pm.smooth_step(-t) - 1).max() <= 4 * np.finfo(LD).eps
    assert pm.smooth_step(LD(1)) == 1 and pm.smooth_step(LD(-1)) == 0 and pm.smooth_step(LD(0)) == LD("0.5")
    assert pm.smooth_step(LD(7)) == 1 and pm.smooth_step(LD(-7)) == 0 and pm.smooth_step(LD(np.nan)) == 0
    assert (np.diff(H) >= 0).all()
    # its derivative is the biweight kernel of the free-surface section: delta(d) = d/dd Hs(d / eps)
    eps, h = LD("0.3"), LD("1e-6")
    d = np.linspace(-0.4, 0.4, 161).astype(LD)
    fd = (pm.smooth_step((d + h) / eps) - pm.smooth_step((d - h) / eps)) / (2 * h)
    tt = d / eps
    delta = np.where(np.abs(tt) < 1, LD(15) / (16 * eps) * (1 - tt * tt) ** 2, LD(0))
    assert sm.SHA == pm.SHA                                       # (the same quadrature as the surface model)
    assert np.abs(fd - delta).max() <= 1e-9 * float(delta.max())


def test_liquid_fraction_and_drag():
    cfg = pm.config(**CFG)
    T = np.linspace(1550.0, 1750.0, 2001).astype(LD)
    fl, dfl, Cd = pm.liquid_fraction(cfg, T)
    assert (np.diff(fl) >= 0).all() and fl[0] == 0 and fl[-1] == 1
    assert (dfl[T <= 1600] == 0).all() and (dfl[T >= 1700] == 0).all() and dfl.max() > 0
    h = LD("1e-5")
    fd = (pm.liquid_fraction(cfg, T + h)[0] - pm.liquid_fraction(cfg, T - h)[0]) / (2 * h)
    inner = (T > 1600.001) & (T < 1699.999)
    assert np.abs(fd - dfl)[inner].max() <= 1e-8 * float(dfl.max())
    assert pm.liquid_fraction(cfg, 1500.0)[2] == LD(1.0e6) / LD(1e-3)          # C(0) = darcy_c / darcy_b
    assert pm.liquid_fraction(cfg, 1800.0)[2] == 0                             # C(1) = 0
    assert (np.diff(Cd) <= 0).all()
    assert [float(v) for v in pm.liquid_fraction(cfg, np.nan)] == [0.0, 0.0, 0.0]
    assert abs(dfl.sum() * (T[1] - T[0]) - 1) < 2e-6     # int fl' dT = 1 (the sum's own error: (step / range)^2 = 1e-6)


@pytest.mark.parametrize("M", [2, 5])
def test_uniform_solid_liquid_and_mushy(M):
    m = _mesh(M)
    V = pm.nodal_volume(m.xg, m.ien)
    vol = V.sum()
    assert abs(vol - 1) <= 1e-12
    C0 = LD(1.0e6) / LD(1e-3)
    for T in (1600.0, 1200.0):                                     # solid, T <= T_solidus
        o = _coef(m, T, **CFG)
        assert np.abs(o["D"] - C0 * V).max() <= 1e-15 * float(C0 * V.max())
        assert abs(o["D"].sum() - C0 * vol) <= 1e-14 * float(C0 * vol)
        assert not o["H"].any() and not o["G"].any()
    for T in (1700.0, 2500.0):                                     # liquid, T >= T_liquidus
        o = _coef(m, T, **CFG)
        assert not o["D"].any() and not o["H"].any()
        assert abs(o["G"].sum() - vol) <= 1e-14
    T = 1637.0                                                     # mushy
    o = _coef(m, T, **CFG)
    fl, dfl, Cd = pm.liquid_fraction(pm.config(**CFG), T)
    assert abs(o["H"].sum() - LD(2.0e9) * dfl * vol) <= 1e-13 * float(LD(2.0e9) * dfl * vol)
    assert abs(o["G"].sum() - fl * vol) <= 1e-13 and abs(o["D"].sum() - Cd * vol) <= 1e-13 * float(Cd * vol)
    # switched-off parts are exact zeros
    o = _coef(m, T, **dict(CFG, latent=0.0))
    assert not o["H"].any() and o["D"].any()
    o = _coef(m, T, **dict(CFG, darcy_c=0.0))
    assert not o["D"].any() and o["H"].any()


def test_latent_heat_of_a_thin_mushy_band():
    """T linear in z across the range: sum H = latent int fl'(T) dV -> latent * area / |grad T| (int fl' dT = 1), however thin
    the band against the element; the quadrature error falls under refinement"""
    grad, area, latent = 100.0, 0.5, 2.0e9
    cfg = dict(CFG, T_solidus=68.3, T_liquidus=121.7, latent=latent)
    want = latent * area / grad
    err = []
    for M in ((2, 1, 4), (4, 2, 8), (8, 4, 16)):
        m = kuhn_box(M, (0.0, 0.0, 0.0), (1.0, 0.5, 2.0))
        o = _coef(m, grad * m.xg.reshape(-1, 3)[:, 2], **cfg)
        err.append(abs(float(o["H"].sum()) - want) / want)
        print(f"mushy band, {M} cells: sum H = {float(o['H'].sum()):.6e} (latent area / |grad T| = {want:.6e}), error {err[-1]:.2e}")
    assert err[2] < err[1] < err[0] and err[2] < 0.01


def test_liquid_volume_below_a_planar_surface():
    """use_phi, T above the liquidus: sum G = the metal volume, to the quadrature error of Hs on the tets of the band.  The
    half-width eps = 0.15 is held while the mesh is refined, so the four points resolve Hs better and better: observed
    9.1e-4, 4.6e-5, 1.3e-6 at M = 4, 8, 16"""
    err = []
    for M in (4, 8, 16):
        m = _mesh(M)
        x = m.xg.reshape(-1, 3)
        phi = x[:, 2] - 0.37 - 0.2 * (x[:, 0] - 0.5)               # metal below: the volume is 0.37
        o = _coef(m, 2000.0, phi=phi, use_phi=True, side=-1, eps=0.15, **CFG)
        err.append(abs(float(o["G"].sum()) - 0.37) / 0.37)
        print(f"planar surface, M = {M}: sum G = {float(o['G'].sum()):.8f} (0.37), error {err[-1]:.2e}")
        assert not o["D"].any() and not o["H"].any()
        gas = phi > 0.15 * 1.02 + 2.0 / M                          # every tet of the node lies beyond the band (|g| = 1.02)
        assert gas.any() and not o["G"][gas].any()
    assert err[2] < err[1] < err[0]


BAD = [("T_solidus", dict(T_solidus=np.nan)), ("T_liquidus", dict(T_liquidus=np.inf)), ("latent", dict(latent=np.nan)),
       ("darcy_c", dict(darcy_c=np.inf)), ("darcy_b", dict(darcy_b=np.nan)), ("level", dict(level=np.nan)),
       ("eps", dict(eps=np.inf)), ("T_liquidus", dict(T_liquidus=1600.0)), ("T_liquidus", dict(T_liquidus=1500.0)),
       ("darcy_b", dict(darcy_b=0.0)), ("darcy_b", dict(darcy_b=-1.0)), ("side", dict(use_phi=True, side=0)),
       ("side", dict(use_phi=True, side=2)), ("eps", dict(use_phi=True, eps=0.0)), ("eps", dict(use_phi=True, eps=-0.5))]


def test_refusals():
    """every bad configuration is refused by the model and, for the same reason, by the library's own check"""
    from dedflow_amd import api
    L = api.lib()
    why = C.create_string_buffer(160)

    def library(cfg):
        c = api.DflPhaseChange(cfg["T_solidus"], cfg["T_liquidus"], cfg["latent"], cfg["darcy_c"], cfg["darcy_b"],
                               1 if cfg["use_phi"] else 0, cfg["level"], int(cfg["side"]), cfg["eps"])
        return L.DflPhaseChangeCheck(C.byref(c), why, 160), why.value.decode()

    good = pm.config(**CFG)
    assert pm.refusal(good) is None and library(good)[0] == 0
    for ok in (dict(darcy_c=0.0, darcy_b=0.0), dict(side=0), dict(eps=0.0), dict(use_phi=True, side=-1, eps=0.1)):
        cfg = pm.config(**dict(CFG, **ok))                           # side and eps count only with use_phi, darcy_b with drag
        assert pm.refusal(cfg) is None and library(cfg)[0] == 0, ok
    for reason, change in BAD:
        cfg = pm.config(**dict(CFG, **change))
        assert pm.refusal(cfg) == reason, (reason, change)
        rc, text = library(cfg)
        assert rc != 0 and reason in text, (reason, change, text)


def test_symbols_declared_and_exported():
    import os
    from dedflow_amd import api
    lib = api.lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pub = open(os.path.join(root, "include", "dedflow.h")).read()
    ker = open(os.path.join(root, "include", "dedflow_kernels.h")).read()
    for n in ("DflMeshSetPhaseChange", "DflMeshPhaseChangeEnabled", "DflPhaseChangeCheck", "DflMeshPhaseCoefficients",
              "DflMeshPhaseChangeStats"):
        assert n in pub and hasattr(lib, n), n
    for n in ("dfl_phase_flag_tets", "dfl_phase_coefficients", "dfl_phase_apply_F", "dfl_phase_apply_J", "dfl_phase_apply_JT",
              "dfl_phase_stats", "dfl_phase_stats_work_size"):
        assert n in ker and hasattr(lib, n), n
    for n in ("set_phase_change", "phase_coefficients", "phase_stats", "phase_change_on"):
        assert hasattr(api.Problem, n), n
    assert "latent heat is not modelled" not in pub.lower()
