"""Child process of tests/test_gpu_raw_basis.py: Jacobi-GMRES solves on jittered Kuhn cubes with the environment the parent
chose (DFL_SPMV_X4_MIN is read once, when the first solve of a process runs), everything a solve left behind written to one
.npz.  Test infrastructure only.

  python raw_basis_worker.py OUT.npz M [M ...]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAXIT = 40


def operands(N, F):
    """the right-hand sides and the initial guess of the cases, shared with the parent (which gives them to the oracle)"""
    b = F.copy()
    b[4 * N:] = 0.0
    rng = np.random.default_rng(7)
    x0 = np.zeros(6 * N)
    x0[:4 * N] = 1e-3 * rng.normal(size=4 * N)
    b_tail = b.copy()
    b_tail[4 * N:] = 1e-3 * np.abs(b[:4 * N]).max() * rng.normal(size=2 * N)
    return b, x0, b_tail


def run(M, res):
    from dedflow_amd import api
    from dedflow_amd.meshgen import kuhn_cube, synthetic_fields
    L = api.lib()
    mesh = kuhn_cube(M, jitter=0.2)
    wg, dwg = synthetic_fields(mesh)
    P = api.Problem(mesh, maxit=MAXIT, atol=0.0, rtol=0.0)
    N = P.N
    wg_d, dwg_d = api.DeviceArray.from_numpy(wg), api.DeviceArray.from_numpy(dwg)
    F_d, x_d = api.DeviceArray(6 * N), api.DeviceArray(6 * N)
    P.assemble_system(wg_d, dwg_d, F_d, want_J=False)
    P.assemble_system(wg_d, dwg_d, None, want_J=True)
    api.sync()
    b, x0, b_tail = operands(N, F_d.numpy())

    def solve(key, rhs, start=None, repeat=1, restart=0):
        L.KrylovDestroy(P.ksp)
        P.ksp = L.KrylovCreateGMRES(MAXIT, 0.0, 0.0, None)
        L.KrylovSetVerbose(P.ksp, 0)
        if restart:
            L.KrylovSetRestart(P.ksp, restart)
        rhs_d = api.DeviceArray.from_numpy(rhs)
        for k in range(repeat):
            x_d.upload(start) if start is not None else x_d.zero()
            it, r0, hist, _ = P.solve(x_d, rhs_d)
            api.sync()
            pre = "M%d/%s/%d/" % (M, key, k)
            res[pre + "x"], res[pre + "hist"] = x_d.numpy(), hist
            res[pre + "scalars"] = np.array([it, r0, L.DflKrylovLastGmresStep(P.ksp)], dtype=np.float64)

    solve("default", b, repeat=2)
    solve("restart15", b, restart=15)
    solve("x0", b, start=x0)
    solve("tail", b_tail)
    P.close()


if __name__ == "__main__":
    out = {}
    for size in sys.argv[2:]:
        run(int(size), out)
    np.savez(sys.argv[1], **out)
