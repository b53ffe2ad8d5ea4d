"""Child process of tests/test_gpu_pc_fold_solver.py: Jacobi-GMRES solves on jittered Kuhn cubes with DFL_SPMV_X4_MIN=1 set by
the parent (read once per process); DFL_GMRES_BLOCK and DFL_GMRES_FOLD_PC are read per solve and set here, case by case.
Everything a solve left behind goes into one .npz.  Test infrastructure only.

  python pc_fold_worker.py OUT.npz M [M ...]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from raw_basis_worker import operands  # noqa: E402  (the right-hand sides of the raw-basis cases)

MAXIT = 40


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
    b, _, b_tail = operands(N, F_d.numpy())

    def solve(key, rhs, block, fold, restart=0, pc_type=None):
        os.environ["DFL_GMRES_BLOCK"] = str(block)
        os.environ["DFL_GMRES_FOLD_PC"] = "1" if fold else "0"
        L.KrylovDestroy(P.ksp)
        P.ksp = L.KrylovCreateGMRES(MAXIT, 0.0, 0.0, None)
        L.KrylovSetVerbose(P.ksp, 0)
        if restart:
            L.KrylovSetRestart(P.ksp, restart)
        if pc_type is not None:
            L.KrylovSetPCType(P.ksp, pc_type)
        rhs_d = api.DeviceArray.from_numpy(rhs)
        for k in range(2):  # every case twice on the same Krylov object
            x_d.zero()
            it, r0, hist, _ = P.solve(x_d, rhs_d)
            api.sync()
            pre = "M%d/%s/%d/" % (M, key, k)
            res[pre + "x"], res[pre + "hist"] = x_d.numpy(), hist
            res[pre + "scalars"] = np.array([it, r0, L.DflKrylovLastGmresStep(P.ksp), L.DflKrylovLastFoldedProducts(P.ksp)], np.float64)

    for fold in (1, 0):
        for block in (4, 3, 2):
            solve("b%d/fold%d" % (block, fold), b, block, fold)
        solve("tail/fold%d" % fold, b_tail, 4, fold)
        solve("restart10/fold%d" % fold, b, 4, fold, restart=10)
    solve("b1/fold1", b, 1, 1)
    solve("ilu0/fold1", b, 4, 1, pc_type=api.PC_ILU0)
    P.close()


if __name__ == "__main__":
    out = {}
    for size in sys.argv[2:]:
        run(int(size), out)
    np.savez(sys.argv[1], **out)
