"""The blocked Arnoldi recurrences whose blocks of three and four take C from the DERIVED Gram matrix (tests/fused_block_model.py)
against plain classical Gram-Schmidt Arnoldi: the three dense operators of test_block_step_model.py with the bounds that file
applies to the scheme with two passes; an operator whose products are nearly parallel raises both flag bits; on the oracle's
Kuhn-cube systems M = 6 and 8 the history stays ten times inside the bar the solver tests apply.  No GPU."""
import numpy as np
import pytest

from fused_block_model import TAU, gmres_blocked_fused, table_row
from test_block_step_model import H_BOUND, HIST_BOUND, N, NAMES, operators
from two_step_model import gmres_reference


@pytest.mark.parametrize("m", [12, 13])
@pytest.mark.parametrize("s", [3, 4])
@pytest.mark.parametrize("name", NAMES)
def test_fused_blocks_reproduce_the_reference(name, s, m):
    """The hard case is "spread" with s = 4: the basis has lost orthogonality to 1e-9, the derived G inherits that, and where q_3
    keeps 0.006 of p_3' the q_i of the second block come out 6e-9 from orthogonal.  With the coordinates of p_i' taken from the
    projections U[l,i] / nu, which are coordinates only in an orthogonal basis, the history was 1.13e-12 ||r0|| from plain Arnoldi;
    from the identity p' = C^-1 q (fused_block_model.block_fused) it is 7.8e-14 (the scheme with two passes: 5.9e-15)."""
    ops, r0 = operators()
    Href, hist_ref = gmres_reference(ops[name], r0, m)
    H, hist, flags, ratio, skew = gmres_blocked_fused(ops[name], r0, m, s)
    dh = np.abs(H - Href).max() / np.abs(Href).max()
    dr = np.abs(hist - hist_ref).max() / np.linalg.norm(r0)
    print("%s s=%d m=%d: H %.3g relative, history %.3g r0, smallest ||q||/||p'|| %.3g, largest |<q_a,q_b>| / (||q_a|| ||q_b||) %.3g"
          % (name, s, m, dh, dr, ratio, skew))
    assert flags == 0
    assert dr <= HIST_BOUND
    if name != "spread":
        assert dh <= H_BOUND


@pytest.mark.parametrize("s", [3, 4])
def test_nearly_parallel_products_raise_both_flags(s):
    """B = I + 1e-6 K (test_block_step_model.py): p_1' keeps 1e-6 of its length at best, bit 0; the derived Gram matrix is the
    difference of numbers 1e12 times its size, C from it leaves the q_i far from orthogonal, bit 1"""
    rng = np.random.default_rng(5)
    B = np.eye(N) + 1e-6 * rng.normal(size=(N, N)) / np.sqrt(N)
    _, _, flags, ratio, skew = gmres_blocked_fused(B, rng.normal(size=N), s, s)
    print("s=%d: ||q||/||p'|| %.3g, skew %.3g (tau %.3g), flags %d" % (s, ratio, skew, TAU, flags))
    assert ratio < 1e-4 and flags == 3


@pytest.mark.parametrize("M", [6, 8])
def test_history_on_the_oracle_systems(M, oracle_lib):
    _, two, one, flags, ratio, skew = table_row(oracle_lib, M)
    print("M=%d: worst err/bar, two passes %.3g, one pass %.3g; smallest ||q||/||p'|| %.3g, skew %.3g" % (M, two, one, ratio, skew))
    assert flags == 0
    assert one < 0.1
