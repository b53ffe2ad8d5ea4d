"""Child process of tests/test_gpu_fused_block.py: the solves of tests/block_step_worker.py (same systems, same cases, each twice on
one Krylov object) with the environment the parent chose -- DFL_GMRES_FUSE_FIXUP and DFL_GMRES_BLOCK are read per solve -- and, per
solve, how many blocks ran update and fix-up as one pass and the flag bits.  Test infrastructure only.

  python fused_block_worker.py OUT.npz M [M ...]
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from raw_basis_worker import operands  # noqa: E402

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
    b, x0, b_tail = operands(N, F_d.numpy())

    def solve(key, rhs, start=None, restart=0, maxit=MAXIT, check=0, rtol=0.0):
        L.KrylovDestroy(P.ksp)
        P.ksp = L.KrylovCreateGMRES(maxit, 0.0, rtol, None)
        L.KrylovSetVerbose(P.ksp, 0)
        if restart:
            L.KrylovSetRestart(P.ksp, restart)
        if check:
            L.KrylovSetCheckInterval(P.ksp, check)
        rhs_d = api.DeviceArray.from_numpy(rhs)
        for k in range(2):
            x_d.upload(start) if start is not None else x_d.zero()
            it, r0, hist, conv = P.solve(x_d, rhs_d)
            api.sync()
            counts, flags = (C.c_int * 5)(*([-1] * 5)), C.c_int(-1)
            L.DflKrylovLastGmresBlocks(P.ksp, C.byref(counts), C.byref(flags))
            pre = "M%d/%s/%d/" % (M, key, k)
            res[pre + "x"], res[pre + "hist"] = x_d.numpy(), hist
            res[pre + "scalars"] = np.array([it, r0, L.DflKrylovLastGmresStep(P.ksp), flags.value, int(conv), rtol,
                                             L.DflKrylovLastFusedBlocks(P.ksp)], dtype=np.float64)
            res[pre + "counts"] = np.array(list(counts), dtype=np.int64)
        return hist, r0

    hist, r0 = solve("it40", b)
    solve("it41", b, maxit=41)
    solve("it42", b, maxit=42)
    solve("it43", b, maxit=43)
    solve("restart15", b, restart=15)
    solve("check5", b, check=5)
    solve("check3", b, check=3)
    solve("x0", b, start=x0)
    solve("tail", b_tail)
    solve("conv", b, rtol=1.5 * hist[19] / r0)  # converges at the first check (iteration 20), as in block_step_worker.py
    P.close()


if __name__ == "__main__":
    out = {}
    for size in sys.argv[2:]:
        run(int(size), out)
    np.savez(sys.argv[1], **out)
