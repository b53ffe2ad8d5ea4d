"""The paired Arnoldi recurrences (tests/two_step_model.py) against plain classical Gram-Schmidt Arnoldi on dense operators:
the same Hessenberg matrix and the same residual history, for even and odd numbers of iterations.  No GPU."""
import numpy as np
import pytest

from two_step_model import gmres_paired, gmres_reference

N = 60
BOUND = 1e-13  # m n u = 10 * 60 * 1.1e-16 = 7e-14: every entry is a sum of at most m n rounded products of O(1) numbers


def operators():
    rng = np.random.default_rng(11)
    orth = np.linalg.qr(rng.normal(size=(N, N)))[0]  # Krylov vectors stay well conditioned: H itself is comparable
    spread = np.diag(np.linspace(1.0, 3.0, N)) + 0.5 * rng.normal(size=(N, N)) / np.sqrt(N)
    return {"orthogonal": orth, "spread": spread}, rng.normal(size=N)


@pytest.mark.parametrize("m", [1, 2, 9, 10])
@pytest.mark.parametrize("name", ["orthogonal", "spread"])
def test_paired_arnoldi_reproduces_the_reference(name, m):
    ops, r0 = operators()
    Href, hist_ref = gmres_reference(ops[name], r0, m)
    H, hist, flags = gmres_paired(ops[name], r0, m)
    assert flags == 0
    assert np.abs(hist - hist_ref).max() <= BOUND * np.linalg.norm(r0)
    if name == "orthogonal":  # (with the spread spectrum both lose orthogonality, each in its own way: H drifts, the history not)
        assert np.abs(H - Href).max() <= BOUND * np.abs(Href).max()
