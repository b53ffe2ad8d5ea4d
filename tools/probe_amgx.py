"""PC_AMGX measurements on one GPU (DESIGN.md "PC_AMGX"): the hierarchy of the pressure block A11 of the assembled (u,p)
system at kuhn_cube(M), setup / apply device time, launches, the tail_rows comparison, iterations and time to rtol 1e-4
of the coupled solve for several preconditioners, and A11 alone (consistent right-hand side).

  python tools/probe_amgx.py --M 119 --what hier,tail,solve,a11
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dedflow_amd import api  # noqa: E402
from dedflow_amd.meshgen import kuhn_cube, synthetic_fields  # noqa: E402


def problem(M, maxit=600, rtol=1e-4):
    m = kuhn_cube(M, jitter=0.2)
    wg, dwg = synthetic_fields(m)
    N = m.num_node
    wg[3 * N:4 * N] = 0.0
    P = api.Problem(m, maxit=maxit, atol=0.0, rtol=rtol)
    wg_d, dwg_d = api.DeviceArray.from_numpy(wg), api.DeviceArray.from_numpy(0.1 * dwg)
    F_d = api.DeviceArray(6 * N)
    P.assemble_system(wg_d, dwg_d, F_d, want_J=False)
    P.assemble_system(wg_d, dwg_d, None, want_J=True)
    api.sync()
    return P, F_d


def timed(fn, reps):
    t = api.Timer()
    t.start()
    for _ in range(reps):
        fn()
    t.stop()
    return t.ms() / reps


def amg_stats(pc, label):
    L = api.lib()
    nl = L.PCAMGXNumLevels(pc)
    rows, nnz, cols = (C.c_int32 * nl)(), (C.c_int32 * nl)(), (C.c_int32 * nl)()
    oc, tail, la, ls = C.c_double(), C.c_int32(), C.c_int64(), C.c_int64()
    L.PCAMGXInfo(pc, rows, nnz, cols, C.byref(oc), C.byref(tail), C.byref(la), C.byref(ls))
    print(f"{label}: levels {nl}, operator complexity {oc.value:.3f}, tail from level {tail.value}, "
          f"launches per apply {la.value}, per setup {ls.value}")
    for l in range(nl):
        print(f"  level {l:2d}: rows {rows[l]:9d}  nnz {nnz[l]:10d}  colours {cols[l]:3d}")


def amg_times(P, cfg=None, reps=20):
    L = api.lib()
    pc = L.PCCreateAMGX(P.fs.mat[5], cfg)
    assert pc
    r = api.DeviceArray.from_numpy(np.random.default_rng(1).normal(size=P.N))
    z = api.DeviceArray(P.N)
    for _ in range(3):
        L.PCSetup(pc)
        L.PCApply(pc, r.ptr, z.ptr)
    api.sync()
    ts = timed(lambda: L.PCSetup(pc), reps)
    ta = timed(lambda: L.PCApply(pc, r.ptr, z.ptr), reps)
    return pc, ts, ta


def do_hier(P):
    t0 = time.time()
    pc, ts, ta = amg_times(P)
    print(f"A11 AMG (reference configuration): create+warm-up {time.time() - t0:.1f} s wall, setup {ts:.3f} ms, "
          f"apply {ta:.3f} ms (device events)")
    amg_stats(pc, "A11 hierarchy")
    api.lib().PCDestroy(pc)


def do_tail(P, values, rounds=3):
    res = {v: [] for v in values}
    for _ in range(rounds):
        for v in values:  # alternating
            os.environ["DFL_AMGX_TAIL_ROWS"] = str(v)
            pc, ts, ta = amg_times(P)
            la = C.c_int64()
            api.lib().PCAMGXInfo(pc, None, None, None, None, None, C.byref(la), None)
            res[v].append((ts, ta, la.value))
            api.lib().PCDestroy(pc)
    os.environ.pop("DFL_AMGX_TAIL_ROWS", None)
    for v in values:
        a = np.array(res[v])
        print(f"tail_rows {v:6d}: setup {np.median(a[:, 0]):.3f} ms  apply {np.median(a[:, 1]):.3f} ms "
              f"(min {a[:, 1].min():.3f})  launches/apply {int(a[0, 2])}")


def do_solve(P, F_d):
    L = api.lib()
    N = P.N
    runs = [("default tree (Jacobi on A11)", api.PC_DECOMPOSITION, None),
            ("tree, AMG on A11 (MULTICOLOR_DILU)", api.PC_AMGX, None),
            ("tree, AMG on A11 (BLOCK_JACOBI)", api.PC_AMGX, b"config_version=2, solver:preconditioner:smoother=BLOCK_JACOBI"),
            ("PC_ILU0", api.PC_ILU0, None),
            ("PC_TWOLEVEL", api.PC_TWOLEVEL, None)]
    for label, t, cfg in runs:
        L.KrylovSetPCType(P.ksp, t)
        L.KrylovSetAMGXConfig(P.ksp, cfg)
        x = api.DeviceArray(6 * N)
        P.solve(x, F_d)  # builds the PC, warm-up
        times = []
        for _ in range(2):
            x.zero()
            api.sync()
            t0 = time.perf_counter()
            it, r0, hist, conv = P.solve(x, F_d)
            api.sync()
            times.append(time.perf_counter() - t0)
        print(f"{label:40s}: {it:4d} iterations, converged {conv}, {1e3 * min(times):9.2f} ms per solve (incl. PCSetup)")
    L.KrylovSetPCType(P.ksp, api.PC_DECOMPOSITION)


def do_a11(P):
    """A11 alone with a consistent right-hand side: GMRES with AMG, and GMRES on D^-1/2 A11 D^-1/2 (= Jacobi)."""
    import scipy.sparse as sp
    L = api.lib()
    rp, ci = P.pattern()
    v = P.export_values()[3]
    N = P.N
    A = sp.csr_matrix((v, ci, rp), shape=(N, N))
    d = 1.0 / np.sqrt(np.abs(A.diagonal()))
    As = (sp.diags(d) @ A @ sp.diags(d)).tocsr()
    b = A @ np.random.default_rng(2).normal(size=N)
    for label, mat, rhs, t in (("A11, AMG (reference configuration)", A, b, api.PC_AMGX),
                               ("A11, Jacobi (symmetric scaling)", As, d * b, api.PC_DECOMPOSITION)):
        M = L.MatrixCreateTypeCSR(P.spy1x1, None)
        L.MatrixZero(M)
        csr = C.cast(M.contents.data, C.POINTER(api.MatrixCSR)).contents
        api.DeviceArray(ci.size, np.float64, ptr=csr.val).upload(mat.data)
        ksp = L.KrylovCreateGMRES(1000, 0.0, 1e-8, None)
        L.KrylovSetVerbose(ksp, 0)
        L.KrylovSetCheckInterval(ksp, 1)
        L.KrylovSetRestart(ksp, 200)
        L.KrylovSetPCType(ksp, t)
        b_d, x_d = api.DeviceArray.from_numpy(rhs), api.DeviceArray(N)
        L.KrylovSolve(ksp, M, x_d.ptr, b_d.ptr)
        api.sync()
        st = L.KrylovGetStats(ksp).contents
        print(f"{label:40s}: GMRES(200) to 1e-8: {st.iterations} iterations, converged {bool(st.converged)}")
        L.KrylovDestroy(ksp)
        L.MatrixDestroy(M)


def do_tree_history(M=10):
    """Relative residual histories of the coupled solve at rtol 1e-10: default tree against AMG on A11."""
    P, F_d = problem(M, maxit=400, rtol=1e-10)
    L = api.lib()
    L.KrylovSetCheckInterval(P.ksp, 1)
    for label, t in (("default tree", api.PC_DECOMPOSITION), ("AMG on A11", api.PC_AMGX)):
        L.KrylovSetPCType(P.ksp, t)
        x = api.DeviceArray(6 * P.N)
        it, r0, hist, conv = P.solve(x, F_d)
        rel = hist / r0
        marks = {k: int(np.argmax(rel <= k)) + 1 if (rel <= k).any() else None for k in (1e-4, 1e-6, 1e-8, 1e-10)}
        print(f"kuhn_cube({M}) {label:14s}: {it} iterations, final rel {rel[-1]:.2e}, first iteration below 1e-4/6/8/10: {marks}")
    P.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=60)
    ap.add_argument("--what", default="hier,tail,solve,a11")
    ap.add_argument("--tail-rows", default="2048,8192,32768")
    a = ap.parse_args()
    if a.what == "tree10":
        do_tree_history(10)
        return
    P, F_d = problem(a.M)
    print(f"kuhn_cube({a.M}): {P.N} nodes, {P.T} tets")
    w = a.what.split(",")
    if "hier" in w:
        do_hier(P)
    if "tail" in w:
        do_tail(P, [int(v) for v in a.tail_rows.split(",")])
    if "solve" in w:
        do_solve(P, F_d)
    if "a11" in w:
        do_a11(P)
    P.close()


if __name__ == "__main__":
    main()
