"""The blocked Arnoldi recurrences (tests/block_step_model.py: s = 1..4 iterations per pass over the basis) against plain classical
Gram-Schmidt Arnoldi on dense operators: the same Hessenberg matrix and the same residual history, with and without a short
last block; s = 2 against the paired model; an operator whose second product is nearly parallel to the first raises the
cancellation flag.  H is compared on the two operators whose Krylov vectors stay well conditioned ("orthogonal", "gauss"); on
"spread" only the history is compared and the deviation of H is printed: there classical Gram-Schmidt loses orthogonality in
plain Arnoldi too, block 1 (the unchanged single step) is already 1e-11 away from it in H, so no bound on H tells the schemes
apart (tests/test_two_step_model.py treats its "spread" operator the same way).  No GPU."""
import numpy as np
import pytest

from block_step_model import block_sizes, gmres_blocked
from two_step_model import gmres_paired, gmres_reference

N = 60
H_BOUND = 1e-11     # relative to the largest entry of H
HIST_BOUND = 1e-12  # of ||r0||


def operators():
    rng = np.random.default_rng(11)
    orth = np.linalg.qr(rng.normal(size=(N, N)))[0]  # Krylov vectors stay well conditioned: H itself is comparable
    gauss = rng.normal(size=(N, N)) / np.sqrt(N)     # likewise: eigenvalues all over the unit disc
    # eigenvalues on one side of the origin, as the project's systems have them: successive products turn towards each other
    # and classical Gram-Schmidt loses orthogonality, in plain Arnoldi as well (block 1, the unchanged single step, is 1e-11
    # away in H): H drifts, each scheme in its own way, the history does not -- as in test_two_step_model.py
    spread = np.diag(np.linspace(1.0, 3.0, N)) + 0.5 * rng.normal(size=(N, N)) / np.sqrt(N)
    return {"orthogonal": orth, "gauss": gauss, "spread": spread}, rng.normal(size=N)


NAMES = ["orthogonal", "gauss", "spread"]


def test_block_sizes_follow_the_driver_rule():
    assert block_sizes(12, 4) == [4, 4, 4] and block_sizes(13, 4) == [4, 4, 4, 1]
    assert block_sizes(13, 3) == [3, 3, 3, 3, 1] and block_sizes(14, 4) == [4, 4, 4, 2] and block_sizes(3, 4) == [3]


@pytest.mark.parametrize("m", [12, 13])
@pytest.mark.parametrize("s", [1, 2, 3, 4])
@pytest.mark.parametrize("name", NAMES)
def test_blocked_arnoldi_reproduces_the_reference(name, s, m):
    ops, r0 = operators()
    Href, hist_ref = gmres_reference(ops[name], r0, m)
    H, hist, flags, ratio = gmres_blocked(ops[name], r0, m, s)
    dh = np.abs(H - Href).max() / np.abs(Href).max()
    dr = np.abs(hist - hist_ref).max() / np.linalg.norm(r0)
    print("%s s=%d m=%d: H %.3g relative, history %.3g r0, smallest ||q||/||p'|| %.3g" % (name, s, m, dh, dr, ratio))
    assert flags == 0
    assert dr <= HIST_BOUND
    if name != "spread":
        assert dh <= H_BOUND


@pytest.mark.parametrize("m", [12, 13])
@pytest.mark.parametrize("name", NAMES)
def test_blocks_of_two_are_the_paired_model(name, m):
    ops, r0 = operators()
    Hp, hist_p, flags_p = gmres_paired(ops[name], r0, m)
    H, hist, flags, _ = gmres_blocked(ops[name], r0, m, 2)
    assert flags == flags_p == 0
    assert np.abs(hist - hist_p).max() <= 1e-13 * np.linalg.norm(r0)
    if name != "spread":
        assert np.abs(H - Hp).max() <= 1e-13 * np.abs(Hp).max()


@pytest.mark.parametrize("s", [2, 3, 4])
def test_nearly_parallel_products_raise_the_flag(s):
    """B = I + 1e-6 K: B^2 v - 2 B v + v = 1e-12 K^2 v, so p_1' keeps 1e-6 of its length at best after losing its part along p_0'"""
    rng = np.random.default_rng(5)
    B = np.eye(N) + 1e-6 * rng.normal(size=(N, N)) / np.sqrt(N)
    _, _, flags, ratio = gmres_blocked(B, rng.normal(size=N), s, s)
    assert ratio < 1e-4 and flags == 1
