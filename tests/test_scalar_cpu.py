"""CPU check of the phi / T transport model (tests/scalar_model.py) against the oracle: the Jacobians are the exact
derivatives of the residual's phi / T rows with respect to the rates, and they couple to nothing else."""
import numpy as np
import pytest

import scalar_model as sm
from dedflow_amd.meshgen import kuhn_cube, synthetic_fields


def _residual(S, wga, dwga):
    F = np.zeros(6 * S.N)
    S.assemble_tet(wga, dwga, F)
    return F


@pytest.mark.parametrize("M", [2, 3])
def test_model_is_the_finite_difference_jacobian(oracle_lib, M):
    m = kuhn_cube(M, jitter=0.2)
    S = oracle_lib.System(m)
    N = S.N
    wgold, dwgold = synthetic_fields(m)
    dwg = 0.5 * dwgold + 0.01
    wga, dwga = sm.alpha_states(N, wgold, dwgold, dwg)
    F0 = _residual(S, wga, dwga)
    h = 1.0
    D = np.empty((6 * N, 2 * N))
    for j in range(2 * N):  # one column per rate dphi_j / dT_j: affine rows, so any step is exact to rounding
        wp, dp = wga.copy(), dwga.copy()
        wp[4 * N + j] += sm.F2 * h
        dp[4 * N + j] += sm.F1 * h
        D[:, j] = (_residual(S, wp, dp) - F0) / h
    Jp, Jt = sm.jacobians(m.xg, m.ien, wga)
    Jp, Jt = Jp.toarray(), Jt.toarray()
    scale = max(np.abs(Jp).max(), np.abs(Jt).max())
    assert np.abs(D[4 * N:5 * N, :N] - Jp).max() <= 1e-10 * np.abs(Jp).max()
    assert np.abs(D[5 * N:, N:] - Jt).max() <= 1e-10 * np.abs(Jt).max()
    # no cross blocks: phi <-> T, and the scalar rates into the (u, p) rows
    assert np.abs(D[4 * N:5 * N, N:]).max() <= 1e-10 * scale
    assert np.abs(D[5 * N:, :N]).max() <= 1e-10 * scale
    assert np.abs(D[:4 * N]).max() <= 1e-10 * np.abs(F0[:4 * N]).max()
    # the T matrix carries the diffusion term, the phi matrix does not: they differ by more than a scale
    assert not np.allclose(Jt / np.abs(Jt).max(), Jp / np.abs(Jp).max())


def test_consistent_mass_sums_to_the_volume():
    m = kuhn_cube(3, jitter=0.2)
    M = sm.mass_matrix(m.xg, m.ien)
    assert abs(M.sum() - 1.0) < 1e-13
