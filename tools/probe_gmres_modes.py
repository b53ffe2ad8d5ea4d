"""Probe: every solve mode of the Krylov drivers (host/gmres.c, CG in host/solver.c) on jittered Kuhn cubes, with what each
solve left behind -- x, res_hist, iterations, rnrm_init, converged, fused_norm_cancelled and, for the verbose mode, the
progress lines -- written to one .npz.  Two such files (two builds of the library, DFL_LIB chooses) are compared bit for bit.

  python tools/probe_gmres_modes.py run OUT.npz [M ...]        all modes at M = 8 and 16 (default), or at the sizes given
  python tools/probe_gmres_modes.py one OUT.npz M MODE         one mode in this process (what rocprofv3 is wrapped around)
  python tools/probe_gmres_modes.py compare A.npz B.npz        JSON summary; exit status 1 unless every array is identical

Modes that depend on an environment switch run as fresh child processes (some switches are cached per process); the rest
share one process per mesh size.  Every child runs under its own time limit and the first failure ends the run."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAXIT = 60
# mode -> environment of its child process (None: shares the per-size process)
MODES = {
    "default_twice": None, "x0_nonzero_twice": None, "verbose": None, "zero_rhs": None, "short_maxit": None,
    "tail_nonzero": None, "restart15": None, "flexible": None, "ilu0": None, "twolevel": None, "fused_norm": None,
    "pipelined": None, "cg_spd": None,
    "eager_sync": {"DFL_KRYLOV_EAGER_SYNC": "1"},
    "fused_norm_no_fused_update_pc": {"DFL_NO_FUSED_UPDATE_PC": "1"},
    "x4_off": {"DFL_SPMV_X4": "0"},
    "x4_min1": {"DFL_SPMV_X4_MIN": "1"},
}


def modes_for(M):
    return [m for m in MODES if m != "x4_min1" or M == 8]


class Captured:
    """stdout of the C library (file descriptor 1) while a solve runs"""

    def __enter__(self):
        import tempfile
        sys.stdout.flush()
        self.tmp = tempfile.TemporaryFile()
        self.saved = os.dup(1)
        os.dup2(self.tmp.fileno(), 1)
        return self

    def __exit__(self, *exc):
        C.CDLL(None).fflush(None)
        os.dup2(self.saved, 1)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read()
        self.tmp.close()


def run_modes(M, modes, out):
    from dedflow_amd import api
    from dedflow_amd.meshgen import kuhn_cube, synthetic_fields
    L = api.lib()
    mesh = kuhn_cube(M, jitter=0.2)
    wg, dwg = synthetic_fields(mesh)
    P = api.Problem(mesh)
    N = P.N
    wg_d, dwg_d = api.DeviceArray.from_numpy(wg), api.DeviceArray.from_numpy(dwg)
    F_d, x_d = api.DeviceArray(6 * N), api.DeviceArray(6 * N)
    P.assemble_system(wg_d, dwg_d, F_d, want_J=False)
    P.assemble_system(wg_d, dwg_d, None, want_J=True)
    api.sync()
    b = F_d.numpy()
    b[4 * N:] = 0.0                      # the driver path: zero phi / T tail, Krylov vectors of 4N
    rng = np.random.default_rng(7)
    x0 = np.zeros(6 * N)
    x0[:4 * N] = 1e-3 * rng.normal(size=4 * N)
    b_tail = b.copy()
    b_tail[4 * N:] = 1e-3 * rng.normal(size=2 * N)
    res = {}

    def new_solver(maxit=MAXIT, verbose=0):
        L.KrylovDestroy(P.ksp)
        P.ksp = L.KrylovCreateGMRES(maxit, 1e-12, 1e-4, None)
        L.KrylovSetVerbose(P.ksp, verbose)
        L.KrylovSetMesh(P.ksp, P.mesh)
        return P.ksp

    def record(key, ksp, x):
        api.sync()
        st = L.KrylovGetStats(ksp).contents
        res[key + "/x"] = x.numpy()
        res[key + "/res_hist"] = np.array(st.res_hist[:])
        res[key + "/iterations"] = np.array([st.iterations], dtype=np.int64)
        res[key + "/rnrm_init"] = np.array([st.rnrm_init])
        res[key + "/converged"] = np.array([st.converged], dtype=np.int64)
        res[key + "/fused_norm_cancelled"] = np.array([st.fused_norm_cancelled], dtype=np.int64)

    def solve(key, rhs=b, start=None, repeat=1):
        rhs_d = api.DeviceArray.from_numpy(rhs)
        for k in range(repeat):
            x_d.upload(start) if start is not None else x_d.zero()
            L.KrylovSolve(P.ksp, P.J, x_d.ptr, rhs_d.ptr)
            record("M%d/%s/%d" % (M, key, k), P.ksp, x_d)

    for mode in modes:
        ksp = new_solver()
        if mode in ("default_twice", "eager_sync", "x4_off", "x4_min1"):
            solve(mode, repeat=2)        # the second solve runs on the assumptions the first one left
        elif mode == "x0_nonzero_twice":
            solve(mode, start=x0, repeat=2)
        elif mode == "verbose":
            new_solver(verbose=1)
            with Captured() as cap:
                solve(mode)
            res["M%d/verbose/0/stdout" % M] = np.frombuffer(cap.text, dtype=np.uint8).copy()
        elif mode == "zero_rhs":
            solve(mode, rhs=np.zeros(6 * N))
        elif mode == "short_maxit":
            new_solver(maxit=10)         # shorter than the check interval of 20: nothing is read before the end
            solve(mode)
        elif mode == "tail_nonzero":
            solve(mode, rhs=b_tail)      # na = 6N
        elif mode == "restart15":
            L.KrylovSetRestart(ksp, 15)
            solve(mode)
        elif mode == "flexible":
            L.KrylovSetFlexible(ksp, 1)
            solve(mode)
        elif mode == "ilu0":
            L.KrylovSetPCType(ksp, api.PC_ILU0)
            solve(mode)
        elif mode == "twolevel":
            L.KrylovSetAggregateSize(ksp, 27)
            L.KrylovSetPCType(ksp, api.PC_TWOLEVEL)
            solve(mode)
        elif mode in ("fused_norm", "fused_norm_no_fused_update_pc"):
            L.KrylovSetFusedNorm(ksp, 1)
            solve(mode, repeat=2)
        elif mode == "pipelined":
            L.KrylovSetPipelined(ksp, 1)
            solve(mode)
        elif mode == "cg_spd":           # the SPD matrix of tests/test_gpu_full_size.py::test_cg_on_spd_csr_matrix
            rp, ci = P.pattern()
            val = -np.ones(ci.size)
            val[np.repeat(np.arange(N), np.diff(rp)) == ci] = (np.diff(rp) - 1.0) + 1.0
            A = L.MatrixCreateTypeCSR(P.spy1x1, None)
            L.MatrixZero(A)
            csr = C.cast(A.contents.data, C.POINTER(api.MatrixCSR)).contents
            api.DeviceArray(ci.size, np.float64, ptr=csr.val).upload(val)
            bc_d, xc_d = api.DeviceArray.from_numpy(np.random.default_rng(1).normal(size=N)), api.DeviceArray(N)
            cg = L.KrylovCreateCG(200, 0.0, 1e-12, None)
            L.KrylovSetVerbose(cg, 1)
            with Captured() as cap:
                L.KrylovSolve(cg, A, xc_d.ptr, bc_d.ptr)
            record("M%d/cg_spd/0" % M, cg, xc_d)
            res["M%d/cg_spd/0/stdout" % M] = np.frombuffer(cap.text, dtype=np.uint8).copy()
            L.KrylovDestroy(cg)
            L.MatrixDestroy(A)
        else:
            raise SystemExit("unknown mode " + mode)
    P.close()
    np.savez(out, **res)


def run_all(out, sizes):
    merged = {}
    for M in sizes:
        shared = [m for m in modes_for(M) if MODES[m] is None]
        jobs = [(shared, {})] + [([m], MODES[m]) for m in modes_for(M) if MODES[m] is not None]
        for k, (modes, extra) in enumerate(jobs):
            part = "%s.part_M%d_%d.npz" % (out, M, k)
            env = dict(os.environ)
            env.update(extra)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", part, str(M)] + modes, env=env, timeout=300)
            if r.returncode != 0:
                raise SystemExit("M=%d modes %s: exit status %d -- stopping here" % (M, modes, r.returncode))
            with np.load(part) as z:
                merged.update({key: z[key] for key in z.files})
            os.remove(part)
    np.savez(out, **merged)
    print("wrote %s: %d arrays of %d solves" % (out, len(merged), sum(key.endswith("/x") for key in merged)))


def compare(a, b):
    with np.load(a) as za, np.load(b) as zb:
        keys = sorted(set(za.files) | set(zb.files))
        differ = [k for k in keys if k not in za.files or k not in zb.files or za[k].dtype != zb[k].dtype
                  or za[k].shape != zb[k].shape or not np.array_equal(za[k].view(np.uint8), zb[k].view(np.uint8))]
        solves = sorted(k[:-2] for k in keys if k.endswith("/x"))
        its = {k: int(za[k + "/iterations"][0]) for k in solves if k + "/iterations" in za.files}
    print(json.dumps({"arrays": len(keys), "solves": len(solves), "identical": len(keys) - len(differ), "differ": differ,
                      "iterations": its}))
    return 1 if differ else 0


if __name__ == "__main__":
    cmd = sys.argv[1]
    if cmd == "run":
        run_all(sys.argv[2], [int(v) for v in sys.argv[3:]] or [8, 16])
    elif cmd == "child":
        run_modes(int(sys.argv[3]), sys.argv[4:], sys.argv[2])
    elif cmd == "one":
        run_modes(int(sys.argv[3]), [sys.argv[4]], sys.argv[2])
    elif cmd == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        raise SystemExit(__doc__)
