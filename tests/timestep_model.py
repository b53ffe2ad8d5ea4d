"""Models at a time step other than the default, and the float64 restatement of the step limits (include/dedflow.h, "time
step").  Test infrastructure only.

private(name, dt) loads a PRIVATE COPY of one of the model modules (assembly_model, scalar_model, phase_model, thermal_model,
fluid_model) under another module name and rebinds its time-step names: DT / kDT, FACT2 / F2, T0, and the private copies of the
modules it imports (sm, pm, tm).  The shared modules are never modified: other tests import them.  Every rebound name is
recomputed with the expression of the module's own source, so the copy at the default step reproduces the shared module bit for
bit (tests/test_timestep_model_cpu.py).

step_limits(...) restates csrc/k_steplimit.hip operation by operation in float64 numpy (no fused multiply-add: numpy has
none), so the launcher is compared with it bit for bit."""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_DT = 5e-2
MODULES = ("assembly_model", "scalar_model", "phase_model", "thermal_model", "fluid_model")
_cache = {}


def private(name, dt):
    """the private copy of tests/<name>.py at the step dt (cached per (name, dt); never one of the shared modules)"""
    assert name in MODULES, name
    dt = float(dt)
    key = (name, dt)
    if key in _cache:
        return _cache[key]
    spec = importlib.util.spec_from_file_location("_timestep_%s_%s" % (name, repr(dt).replace(".", "_").replace("-", "m")),
                                                  os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)          # (not entered into sys.modules: nobody else can import it)
    g = vars(mod)
    if name == "assembly_model":
        g["DT"] = dt
        g["FACT2"] = g["DT"] * g["ALPHAF"] * g["GAMMA"]
    elif name == "scalar_model":
        g["kDT"] = dt
        g["F2"] = g["kDT"] * g["kALPHAF"] * g["kGAMMA"]
    elif name == "phase_model":
        g["kDT"] = dt
        g["FACT2"] = g["kDT"] * g["kALPHAF"] * g["kGAMMA"]
    elif name == "thermal_model":
        g["sm"], g["pm"] = private("scalar_model", dt), private("phase_model", dt)
        g["F2"] = g["LD"](g["sm"].F2)
    elif name == "fluid_model":
        g["sm"], g["pm"], g["tm"] = private("scalar_model", dt), private("phase_model", dt), private("thermal_model", dt)
        LD = g["LD"]
        g["F2"] = LD(g["sm"].F2)
        g["T0"] = LD(4.0) / (LD(g["sm"].kDT) * LD(g["sm"].kDT))
    _cache[key] = mod
    return mod


def step_consts(dt, sm=None):
    """dfl_step_consts_from_dt in float64: every entry in the operation order of the C source"""
    import scalar_model
    sm = sm or scalar_model
    kMU = 10.0 / 3.0
    dt = float(dt)
    fact2 = dt * sm.kALPHAF * sm.kGAMMA
    return dict(dt=dt, t0=4.0 / (dt * dt), fact2=fact2, fact2_rho=fact2 * sm.kRHO, fact2_rho2=fact2 * sm.kRHO * sm.kRHO,
                fact2_mu4=4.0 * fact2 * kMU, fact2_kappa=fact2 * sm.kKAPPA, states_old=dt * sm.kALPHAF * (1.0 - sm.kGAMMA),
                corr_old=dt * (1.0 - sm.kGAMMA), corr_new=dt * sm.kGAMMA)


# ---- the step limits ---------------------------------------------------------------------------------------------------------
def tet_gradients(xg, ien):
    """g [T,4,3] = grad N_a and det [T] in the closed form of csrc/tet_levelset.hpp (tet_cross), operation by operation"""
    x = np.asarray(xg, np.float64).reshape(-1, 3)[np.asarray(ien).reshape(-1, 4)]
    e1, e2, e3 = x[:, 1] - x[:, 0], x[:, 2] - x[:, 0], x[:, 3] - x[:, 0]

    def cross(a, b):
        return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                         a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)
    c23, c31, c12 = cross(e2, e3), cross(e3, e1), cross(e1, e2)
    det = (e1[:, 0] * c23[:, 0] + e1[:, 1] * c23[:, 1]) + e1[:, 2] * c23[:, 2]
    g = np.empty((len(x), 4, 3))
    g[:, 1], g[:, 2], g[:, 3] = c23 / det[:, None], c31 / det[:, None], c12 / det[:, None]
    g[:, 0] = -((g[:, 1] + g[:, 2]) + g[:, 3])
    return g, det


def _max_lowest(v, mask):
    """(maximum of v over mask, the lowest index that attains it); (0.0, -1) when the mask is empty"""
    idx = np.flatnonzero(mask)
    if idx.size == 0:
        return 0.0, -1
    m = v[idx].max()
    return float(m), int(idx[v[idx] == m][0])


def step_limits(xg, ien, w, N, level=0.0, sigma0=0.0, dsigma_dT=0.0, T_ref=0.0, rho_bar=1.0e3, dt=DEFAULT_DT):
    """DflTimeStepLimits as a dict, from host arrays: xg [3N], ien [4T], w [6N]"""
    w = np.asarray(w, np.float64)
    ien4 = np.asarray(ien).reshape(-1, 4)
    with np.errstate(all="ignore"):
        g, _ = tet_gradients(xg, ien)
        u = w[:3 * N].reshape(-1, 3)[ien4]                                     # [T,4,3]
        phi, Tn = w[4 * N:5 * N][ien4], w[5 * N:6 * N][ien4]
        ubar = 0.25 * (((u[:, 0] + u[:, 1]) + u[:, 2]) + u[:, 3])               # [T,3]
        Tbar = 0.25 * (((Tn[:, 0] + Tn[:, 1]) + Tn[:, 2]) + Tn[:, 3])
        f = phi - level
        finite = (np.isfinite(g).all(axis=(1, 2)) & np.isfinite(ubar).all(axis=1) & np.isfinite(Tbar) & np.isfinite(f).all(axis=1))
        c = np.abs((ubar[:, None, 0] * g[:, :, 0] + ubar[:, None, 1] * g[:, :, 1]) + ubar[:, None, 2] * g[:, :, 2])   # [T,4]
        gg = (g[:, :, 0] * g[:, :, 0] + g[:, :, 1] * g[:, :, 1]) + g[:, :, 2] * g[:, :, 2]
        r, m = np.zeros(len(ien4)), np.zeros(len(ien4))
        for a in range(4):                                                     # (max as the kernel forms it: from 0, ascending a)
            r = np.where(c[:, a] > r, c[:, a], r)
            m = np.where(gg[:, a] > m, gg[:, a], m)
        cut = finite & ~(f > 0.0).all(axis=1) & ~(f < 0.0).all(axis=1)
        s = sigma0 + dsigma_dT * (Tbar - T_ref)
        sigma = np.where(s > 0.0, s, 0.0)
        q = sigma * (m * np.sqrt(m))
        out = {}
        out["rate_adv"], out["tet_adv"] = _max_lowest(r, finite)
        out["rate_adv_surface"], out["tet_surface"] = _max_lowest(r, cut)
        out["cap_q"], out["tet_cap"] = _max_lowest(q, cut & (q >= 0.0))
        out["num_cut"], out["num_nonfinite"] = int(cut.sum()), int((~finite).sum())
        out["dt_adv"] = 1.0 / out["rate_adv"] if out["rate_adv"] > 0.0 else np.inf
        out["dt_surface"] = 1.0 / out["rate_adv_surface"] if out["rate_adv_surface"] > 0.0 else np.inf
        out["dt_capillary"] = float(np.sqrt(rho_bar / (2.0 * np.pi * out["cap_q"]))) if out["cap_q"] > 0.0 else np.inf
        out["dt"] = float(dt)
    return out
