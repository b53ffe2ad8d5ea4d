#!/usr/bin/env python3
"""bench.py -- DEDFlow hot path on MI355X.

One "step" = one Newton linearisation of the reference driver (src/main.c:157-279)
on a synthetic Kuhn-cube tet mesh, inputs resident in HBM:
    AssembleSystem(F)  colored RHS assembly + weak-BC faces + Dirichlet      (src/main.c:124)
    AssembleSystem(J)  zero + colored LHS assembly + faces + Dirichlet rows  (src/main.c:160)
    KrylovSolve        PC setup + `--gmres-its` right-preconditioned GMRES iterations
                       (block-Jacobi PC tree of krylov.c:439-453; tolerances 0 so the
                       iteration count is fixed and the work per step is constant)
value = (4N active u,p DOFs) / (seconds per step)  -- whole-job DOFs assembled and solved per second.
Per-kernel launch durations are measured live with hipEvents on the library stream
(DflProfile*, dedflow_amd/host/runtime.c); roofline.achieved uses the ALGORITHMIC
bytes of SURVEY.md 8(d) / BASELINE.md 3.

N=1 workload: the 10M-tet cube (M=119) BASELINE.json's metric is quoted on.
N>1: the same mesh, element-partitioned over N ranks (strong scaling), halo exchange +
all-reduce on RCCL (bootstrap through torch.distributed, backend nccl).  `python bench.py --gpus N`
starts the N ranks itself (torch.distributed.run, 127.0.0.1) when it was not launched by it.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6.3 TB/s achievable

TAGS = {"spmv": 0, "cgs_dots": 1, "cgs_update": 2, "pc_apply": 3, "asm_lhs": 4, "asm_rhs": 5, "face": 6}


def algorithmic_bytes(N, T, nnz1, its):
    """bytes per launch (per unit) of each kernel class."""
    n4 = 4 * N
    return {
        "spmv": 132.0 * nnz1 + 4.0 * (N + 1) + 64.0 * N,                      # per matvec
        # per J assembly: SURVEY 8(d)'s COMPULSORY FLOOR (every block line written once, connectivity once, node fields
        # once) -- the slot-owner kernel moves more than this (slot map, contribution descriptors, per-patch connectivity;
        # DESIGN.md section 3), so the fraction is conservative.  The reference-shaped colored scatter (4116*T + 120*N:
        # every block line read+written once per tet) is reported next to it.
        "asm_lhs": 128.0 * nnz1 + 16.0 * T + 120.0 * N,
        "asm_lhs_colored": T * (16.0 + 4.0 + 4096.0) + 120.0 * N,
        "asm_rhs": T * (20.0 + 384.0) + 120.0 * N,                           # per F assembly
        "pc_apply": (9 + 1) * 8.0 * N + 2 * 8.0 * n4,                        # per apply (w read, z written -- interleaved, for the matvec)
        "cgs": [2 * 8.0 * n4 * (k + 1) + 24.0 * n4 for k in range(its)],     # dots+update of step k
    }


DUMP_SEED = 20241016      # --dump-outputs: the sample positions depend on this seed and the array lengths only
DUMP_VALUES = 1 << 19     # sampled entries of each length-6N vector (x, F)
DUMP_BLOCKS = 1 << 16     # sampled 4x4 blocks of J


def _sample(n, k):
    """Sorted positions of a fixed, seeded sample of k of n items (all of them when n <= k)."""
    if n <= k:
        return np.arange(n)
    return np.sort(np.random.default_rng(DUMP_SEED).choice(n, size=k, replace=False))


def _gather(ptr, n, width, idx, chunk_values=1 << 23):
    """Rows idx (sorted) of the float64 device array [n][width] at ptr, read in chunks so the whole array never sits on the host."""
    from dedflow_amd import api
    rows = max(1, chunk_values // width)
    out = np.empty((len(idx), width))
    for s in range(0, n, rows):
        e = min(n, s + rows)
        lo, hi = np.searchsorted(idx, [s, e])
        if lo < hi:
            part = api.DeviceArray((e - s) * width, np.float64, ptr=ptr + s * width * 8).numpy().reshape(-1, width)
            out[lo:hi] = part[idx[lo:hi] - s]
    return out


def dump_outputs(out_dir, P, x_d, F_d, its, r0, hist):
    """What one step hands its caller -- solution x, residual F, matrix J (4x4 blocks over the 1x1 pattern, include/dedflow.h)
    and the GMRES statistics -- as float64 .npy files.  x, F and J are fixed seeded samples (positions in *_index, J_row,
    J_col), about 25 MB in all at any mesh size."""
    from dedflow_amd import api
    os.makedirs(out_dir, exist_ok=True)
    save = lambda name, a: np.save(os.path.join(out_dir, name + ".npy"), np.asarray(a, dtype=np.float64))
    for name, d in (("x", x_d), ("F", F_d)):
        idx = _sample(d.n, DUMP_VALUES)
        save(name, _gather(d.ptr, d.n, 1, idx)[:, 0])
        save(name + "_index", idx)
    bv = api.lib().MatrixFSBlockValues(P.J)   # asked again: the placement calibration may have moved the array
    if not bv:
        raise RuntimeError("--dump-outputs: J holds no 4x4 block array")
    row_ptr, col_ind = P.pattern()
    k = _sample(P.nnz1, DUMP_BLOCKS)
    save("J_blocks", _gather(bv, P.nnz1, 16, k))
    save("J_row", np.searchsorted(row_ptr, k, side="right") - 1)
    save("J_col", col_ind[k])
    save("residual_history", hist)
    save("solve_stats", [its, r0])


def calibration_cap_gb(N, nnz1, its):
    """Default transient-memory cap of the explicit work-space calibration (--placement-cap-gb -1): room for what its first
    round holds at once -- five more Krylov bases of 6N x (its + 2) doubles and six copies of the 4x4 block values -- and
    40 % more for the spacers in front of its far blocks.  Every draw is still made and timed; the cap shortens the time spent
    allocating and releasing spacers of up to 5/8 of the free memory (10M-tet mesh: 48 GB, calibration 12 s instead of
    30-35 s, winning blocks as fast in the loop)."""
    held = 5 * 6.0 * N * (its + 2) * 8 + 6 * 128.0 * nnz1
    return 1.4 * held / 2 ** 30


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return None


def cpu_baseline(M_full, M_single, its):
    """The CPU oracle (oracle/liboracle.so, kind "port") timed on this box's host cores, two legs:
      * all host threads of this rank's share (<= 16) on the SAME mesh as the GPU line (M_full; about 10-30 s of CPU work),
      * one thread on a smaller mesh of the same family (M_single), with a scipy.sparse CSR matvec on that matrix as an
        independent SpMV yardstick.
    Test infrastructure used as the reported baseline only -- never on the product path."""
    from dedflow_amd.meshgen import kuhn_cube, synthetic_fields
    from oracle import orc

    def leg(S, wg, dwg, threads, reps_spmv=3):
        orc.set_threads(threads)
        spmv_bytes = 132.0 * S.nnz1 + 4.0 * (S.N + 1) + 64.0 * S.N
        x = np.random.default_rng(0).normal(size=6 * S.N)
        t0 = time.perf_counter()
        F, _ = S.assemble_system(wg, dwg, True, False)
        tF = time.perf_counter() - t0
        t0 = time.perf_counter()
        _, vals = S.assemble_system(wg, dwg, False, True)
        tJ = time.perf_counter() - t0
        S.matvec(vals, x)
        t0 = time.perf_counter()
        for _ in range(reps_spmv):
            S.matvec(vals, x)
        tS = (time.perf_counter() - t0) / reps_spmv
        t0 = time.perf_counter()
        S.gmres(vals, F, maxit=its, atol=0.0, rtol=0.0)
        tG = time.perf_counter() - t0
        step = tF + tJ + tG
        return ({"value": 4.0 * S.N / step, "cores": threads, "assemble_J_s": tJ, "assemble_F_s": tF, "gmres_s": tG, "spmv_s": tS,
                 "assemble_J_dofs_per_s": 4.0 * S.N / tJ, "spmv_GBps": spmv_bytes / tS / 1e9}, vals, x)

    ncores = max(1, min(orc.num_procs(), 16))
    t_set = time.perf_counter()
    m = kuhn_cube(M_full, jitter=0.2)
    wg, dwg = synthetic_fields(m)
    orc.set_threads(ncores)
    S = orc.System(m, sorted_coloring=True)   # one-pass form of the JPL coloring: same colors (tests/test_oracle_cpu.py)
    t_set = time.perf_counter() - t_set
    multi, vals, x = leg(S, wg, dwg, ncores)
    out = dict(multi)
    out.update({
        "unit": "DOF/s", "kind": "port", "cpu_model": cpu_model(), "host_threads_available": orc.num_procs(),
        "sample": f"the GPU line's own mesh: Kuhn cube M={M_full} ({S.T} tets, {S.N} nodes), same step (F + J assembly, {its} GMRES "
                  f"its), oracle/liboracle.so with OpenMP on {ncores} host threads (set-up {t_set:.0f} s, not in `value`)",
    })
    del S, vals, x, m, wg, dwg
    single = None
    if M_single > 0:
        m1 = kuhn_cube(M_single, jitter=0.2)
        w1, d1 = synthetic_fields(m1)
        S1 = orc.System(m1, sorted_coloring=True)
        single, vals1, x1 = leg(S1, w1, d1, 1)
        single["sample"] = f"SMALLER mesh: Kuhn cube M={M_single} ({S1.T} tets, {S1.N} nodes), one thread"
        try:   # independent SpMV yardstick: scipy.sparse CSR (one thread) on the same 4N x 4N matrix
            A = S1.to_scipy(vals1)
            xs = x1[:4 * S1.N].copy()
            A @ xs
            t0 = time.perf_counter()
            for _ in range(3):
                A @ xs
            ts = (time.perf_counter() - t0) / 3
            single["scipy_csr_spmv_s"] = ts
            single["scipy_csr_spmv_GBps"] = (132.0 * S1.nnz1 + 4.0 * (S1.N + 1) + 64.0 * S1.N) / ts / 1e9
            single["scipy_csr_bytes_actually_streamed"] = 12.0 * A.nnz + 4.0 * (4 * S1.N + 1) + 64.0 * S1.N
        except Exception as exc:  # noqa: BLE001
            single["scipy_csr_spmv_s"] = None
            single["scipy_error"] = repr(exc)
    orc.set_threads(1)
    out["single_thread"] = single
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--M", type=int, default=119, help="cells per cube edge (119 -> 10.1M tets)")
    ap.add_argument("--gmres-its", type=int, default=40)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure everything beyond the headline figure: per-kernel durations and the "
                         "roofline (a profiled pass of their own), the SpMV back to back, whole AssembleSystem calls, the solves to "
                         "rtol 1e-4, the CPU baseline, the DEM sweep and the coupled step.  Without it a run sets up, warms up, "
                         "times the steps, writes --dump-outputs and prints the result line")
    ap.add_argument("--cpu-M", type=int, default=-1, help="--full: cube size of the multi-thread CPU-baseline leg (-1 = the GPU line's M, 0 = skip)")
    ap.add_argument("--cpu-single-M", type=int, default=64, help="--full: cube size of the single-thread CPU leg + scipy yardstick (0 = skip)")
    ap.add_argument("--placement", choices=["calibrate", "default", "off"], default="calibrate",
                    help="Krylov work-space placement: explicit heavy DflKrylovCalibratePlacement before the warm-up (calibrate), the "
                         "library's bounded default, or none")
    ap.add_argument("--placement-cap-gb", type=float, default=-1.0,
                    help="transient device memory the explicit calibration may hold (-1 = room for its draws + 40 %%, 0 = no cap)")
    ap.add_argument("--jitter", type=float, default=0.2)
    ap.add_argument("--solve-to-rtol", type=int, default=1, help="--full: also time one PC_ILU0 solve to rtol 1e-4 after the timed steps (0 = skip)")
    ap.add_argument("--coupled-M", type=int, default=55, help="--full: fluid mesh of the coupled fluid + DEM step leg (0 = skip)")
    ap.add_argument("--dem-particles", type=int, default=100000, help="--full: DEM contact sweep leg after the timed step (0 = skip)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps, write what the last one computed (x, F, samples "
                                                          "of J, GMRES history) as DIR/<name>.npy")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.dump_outputs and (args.gpus > 1 or os.environ.get("DFL_FORCE_DIST") == "1"):
        ap.error("--dump-outputs is only written by the single-rank run (--gpus 1)")

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: start the N ranks ourselves (one process per GPU, torch.distributed.run with the
        # loopback rendezvous) as a CHILD process -- nothing in this process has touched the GPU yet -- and relay its output
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr",
               "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.call(cmd))
    if world > 1 and args.gpus != world:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: launch with --nproc-per-node {args.gpus}", file=sys.stderr)
        sys.exit(2)
    # stdout carries the ONE JSON line and nothing else: whatever a library prints there meanwhile (the RCCL version banner,
    # gloo's connection notes) is sent to stderr; the line itself goes to the saved descriptor at the end
    sys.stdout.flush()
    args._stdout_fd = os.dup(1)
    os.dup2(2, 1)
    if world > 1 or os.environ.get("DFL_FORCE_DIST") == "1":  # DFL_FORCE_DIST: rehearse the N>1 leg on one rank
        from dedflow_amd import dist_bench
        if not args.full:
            args.solve_to_rtol = 0    # its leg after the timed steps is one of --full's
        args.placement_cap_gb = max(args.placement_cap_gb, 0.0)   # per-rank calibrations: no cap unless one is given
        return dist_bench.run(args, rank, world, local_rank)

    from dedflow_amd import api
    from dedflow_amd.meshgen import kuhn_cube, synthetic_fields
    L = api.lib()
    api.hip().hipSetDevice(local_rank)

    t_setup = time.perf_counter()
    mesh = kuhn_cube(args.M, jitter=args.jitter)
    wg, dwg = synthetic_fields(mesh)
    its = args.gmres_its
    P = api.Problem(mesh, maxit=its, atol=0.0, rtol=0.0, quiet=True)
    N, T, nnz1 = P.N, P.T, P.nnz1
    wg_d, dwg_d = api.DeviceArray.from_numpy(wg), api.DeviceArray.from_numpy(dwg)
    F_d, x_d = api.DeviceArray(6 * N), api.DeviceArray(6 * N)
    api.sync()
    t_setup = time.perf_counter() - t_setup

    solve_timer = api.Timer()
    solve_ms = []
    quiet_waits = []

    def quiet():
        """Before a timed leg: wait while the driver is still wiping device memory that the set-up of that leg freed (DESIGN.md
        section 3, 'SpMV placement': streaming kernels run up to 8 % slower in episodes meanwhile).  Returns at once when there is
        nothing to wait for or rocm_smi is unavailable; the waits are reported in the JSON line."""
        w = L.DflWaitDeviceMemoryQuiet(15.0)
        if w > 0.0:
            quiet_waits.append(round(w, 2))

    def step():
        P.assemble_system(wg_d, dwg_d, F_d, want_J=False)
        P.assemble_system(wg_d, dwg_d, None, want_J=True)
        x_d.zero()
        solve_timer.start()           # one event pair around the whole Krylov solve (no per-kernel instrumentation)
        out = P.solve(x_d, F_d)
        solve_timer.stop()
        solve_ms.append(solve_timer.ms())
        return out

    # Krylov work-space placement: the library's default is a bounded pick among <= 4 basis blocks inside
    # the first solve; the heavy lottery (spacers, value-array copies, waits for the driver's wipe) is this explicit call,
    # made BEFORE the warm-up and named in `config.placement`
    L.DflKrylovCalibratePlacement.argtypes = [C.c_void_p, C.POINTER(api.Matrix), C.c_int64]
    L.DflKrylovCalibratePlacement.restype = None
    t_cal = 0.0
    cap_gb = calibration_cap_gb(N, nnz1, its) if args.placement_cap_gb < 0 else args.placement_cap_gb
    if args.placement == "off":
        os.environ["DFL_WS_CANDIDATES"] = "1"
    elif args.placement == "calibrate":
        P.assemble_system(wg_d, dwg_d, None, want_J=True)
        api.sync()
        t_cal = time.perf_counter()
        L.DflKrylovCalibratePlacement(P.ksp, P.J, int(cap_gb * 2 ** 30))
        api.sync()
        t_cal = time.perf_counter() - t_cal
    for _ in range(args.warmup):
        step()
    api.sync()
    quiet()   # (a no-op after the calibration's own waits; see quiet())
    # timed region: EXACTLY --steps steps, no instrumentation inside (the in-library hipEvent profiler puts two
    # event packets around every kernel, which costs bubbles and stops consecutive kernels from overlapping)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        it, r0, hist, _ = step()
    api.sync()
    t_total = time.perf_counter() - t0
    ms_per_step = 1e3 * t_total / args.steps
    solve_ms_timed = float(np.mean(solve_ms[-args.steps:]))
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, P, x_d, F_d, it, r0, hist)
    # what the Krylov work-space calibration measured and chose in the first warm-up solve ("SpMV placement":
    # the in-loop SpMV time is a property of where the value array and the basis landed; this is the record of that draw)
    placement_log = (L.DflKrylovCalibrationLog() or b"").decode(errors="replace").strip().split("\n")
    ab = algorithmic_bytes(N, T, nnz1, its)
    out = {
        "metric": "assembled DOFs/s + Krylov-SpMV GB/s (%HBM peak), 10M-tet mesh",
        "value": 4.0 * N / (ms_per_step * 1e-3), "unit": "DOF/s",
        "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_per_step,
        "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": {"workload": f"Kuhn cube M={args.M}: {T} tets, {N} nodes, nnz1={nnz1}; step = AssembleSystem(F) + "
                               f"AssembleSystem(J) + Jacobi-PC GMRES x{its} iterations",
                   "colors": P.num_color, "gmres_its": its, "parallelism": "1 GPU",
                   "placement": {"calibrate": f"explicit DflKrylovCalibratePlacement before the warm-up ({t_cal:.1f} s, cap "
                                              f"{f'{cap_gb:.1f}' if cap_gb > 0 else 'none'} GB): basis blocks + value-array copies behind spacers",
                                 "default": "library default: bounded pick among <= 4 basis blocks in the first solve",
                                 "off": "none (DFL_WS_CANDIDATES=1)"}[args.placement]},
        "spmv_placement_calibration": placement_log, "waits_for_driver_memory_wipe_s": quiet_waits,
        # the whole Krylov solve against the HBM roofline: algorithmic bytes of its `its` matvecs (x0 = 0: r0 = b needs none),
        # its CGS steps, its+1 preconditioner applications and the final basis combination over the un-instrumented solve time
        "krylov_solve": (lambda b: {"ms": solve_ms_timed, "algorithmic_GB": b / 1e9, "GBps": b / (solve_ms_timed * 1e-3) / 1e9,
                                    "frac_of_8TBps": b / (solve_ms_timed * 1e-3) / 1e9 / HBM_PEAK_GBS})(
            its * ab["spmv"] + sum(ab["cgs"]) + (its + 1) * ab["pc_apply"] + 8.0 * 4 * N * (its + 2)),
        "setup_s": t_setup, "gmres_residual_drop": float(hist[-1] / r0) if len(hist) else None,
    }
    if args.full:
        out.update(full_legs(args, L, P, step, quiet, wg_d, dwg_d, F_d, x_d))
    sys.stdout.flush()
    os.write(args._stdout_fd, (json.dumps(out) + "\n").encode())
    P.close()


def full_legs(args, L, P, step, quiet, wg_d, dwg_d, F_d, x_d):
    """What `--full` measures after the timed steps, on the same problem and device arrays: per-kernel durations and the
    roofline (a separate profiled pass), the SpMV back to back, whole AssembleSystem calls, the solves to the reference's
    tolerance, the CPU baseline, the DEM sweep and the coupled fluid + DEM step.  Returns the keys it adds to the JSON line."""
    from dedflow_amd import api
    from dedflow_amd.meshgen import kuhn_cube, synthetic_fields
    N, T, nnz1, its = P.N, P.T, P.nnz1, args.gmres_its
    L.DflProfileEnable.argtypes = [C.c_int]
    L.DflProfileCollect.argtypes = [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.DflProfileCollect.restype = C.c_int

    # separate, untimed pass with the profiler on: per-kernel durations for the roofline figures
    L.DflProfileEnable(1)
    n_prof_steps = min(args.steps, 20)   # the profiler holds 8192 intervals (~165 per step)
    for _ in range(n_prof_steps):
        step()
    api.sync()

    # the same SpMV outside the Krylov loop, 10 launches between one pair of events (no per-kernel instrumentation)
    tmr = api.Timer()
    y_d = api.DeviceArray(6 * N)
    P.matvec(F_d, y_d)
    tmr.start()
    for _ in range(10):
        P.matvec(F_d, y_d)
    tmr.stop()
    spmv_grouped_ms = tmr.ms() / 10

    prof = {}
    for name, tag in TAGS.items():
        tot, mn = C.c_double(0), C.c_double(0)
        cnt = L.DflProfileCollect(tag, C.byref(tot), C.byref(mn))
        prof[name] = (cnt, tot.value, mn.value)
    L.DflProfileEnable(0)

    ab = algorithmic_bytes(N, T, nnz1, its)
    K = n_prof_steps  # steps behind the per-kernel figures (the timed region above ran args.steps)
    kernels = {}

    def entry(name, total_bytes, cnt, tot_ms, unit_desc):
        if cnt == 0 or tot_ms <= 0:
            return
        gbps = total_bytes / (tot_ms * 1e-3) / 1e9
        kernels[name] = {"launches": cnt, "avg_ms": tot_ms / cnt, "total_ms_per_step": tot_ms / K, "GBps": gbps,
                         "frac_of_8TBps": gbps / HBM_PEAK_GBS, "bytes": unit_desc}

    c, t, _ = prof["spmv"]; entry("spmv", ab["spmv"] * c, c, t, "132*nnz1+4(N+1)+64N per launch")
    c, t, _ = prof["asm_lhs"]; entry("asm_lhs", ab["asm_lhs"] * K, c, t, "128*nnz1+16*T+120N per J assembly = SURVEY 8(d) compulsory floor "
                                                                      "(slot-owner node patches, ONE launch, no atomics; the "
                                                                      "colored scatter of SURVEY 8(d) would move 4116*T+120N)")
    if "asm_lhs" in kernels:  # what the reference-shaped colored scatter would move, for orientation only
        kernels["asm_lhs"]["colored_scatter_bytes_per_assembly"] = ab["asm_lhs_colored"]
    c, t, _ = prof["asm_rhs"]; entry("asm_rhs", ab["asm_rhs"] * K, c, t, "404*T+120N per F assembly = the colored-scatter byte model (lane-per-tet persistent wave kernel + ordered node sum: 2 launches; PMC traffic: roofline.traffic / profiles/pmc_traffic_M119.json)")
    c, t, _ = prof["pc_apply"]; entry("pc_apply", ab["pc_apply"] * c, c, t, "80N+64N per apply (z is written interleaved for the matvec that gathers from it)")
    cd, td, _ = prof["cgs_dots"]; cu, tu, _ = prof["cgs_update"]
    entry("cgs", sum(ab["cgs"]) * K, cd + cu, td + tu, "2*8*4N*(k+1)+24*4N per Arnoldi step k")
    dominant = max(kernels, key=lambda k: kernels[k]["total_ms_per_step"])
    kd = kernels[dominant]
    per_launch_bytes = {"spmv": ab["spmv"], "asm_lhs": ab["asm_lhs"] * K / max(kd["launches"], 1),
                        "asm_rhs": ab["asm_rhs"] * K / max(kd["launches"], 1), "pc_apply": ab["pc_apply"],
                        "cgs": sum(ab["cgs"]) * K / max(kd["launches"], 1)}[dominant]
    # HBM traffic per launch from the PMC passes committed under profiles/ (rocprofv3 --pmc FETCH_SIZE and
    # --pmc WRITE_SIZE in separate runs, gfx950 x2 read correction as MI355X_MICROARCH.md prescribes).  It is a
    # property of kernel + input, so it is only reported for the configuration it was collected on.
    traffic = None
    try:
        if args.M == 119:
            pmc = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic_M119.json")))
            if dominant in pmc:
                traffic = pmc[dominant]["hbm_bytes_per_launch"]
            # every kernel with a committed PMC figure also gets its rate against the bytes it really moved
            for name, kk in kernels.items():
                names = {"asm_rhs": ["asm_rhs", "rhs_node_sum"]}.get(name, [name])
                if all(nm in pmc for nm in names) and kk["launches"]:
                    tb = sum(pmc[nm]["hbm_bytes_per_launch"] for nm in names)
                    per_unit_ms = kk["total_ms_per_step"] if name in ("asm_lhs", "asm_rhs") else kk["avg_ms"]
                    kk["pmc_traffic_bytes"] = tb
                    kk["GBps_vs_pmc_traffic"] = tb / (per_unit_ms * 1e-3) / 1e9
                    kk["frac_of_8TBps_vs_pmc_traffic"] = kk["GBps_vs_pmc_traffic"] / HBM_PEAK_GBS
    except Exception:
        traffic = None
    roofline = {"kernel": dominant, "bound": "hbm", "achieved": kd["GBps"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": kd["GBps"] / HBM_PEAK_GBS, "traffic": traffic,
                "algorithmic_bytes_per_launch": per_launch_bytes, "avg_launch_ms": kd["avg_ms"]}

    # ---- AssembleSystem end to end (pack, element kernels, weak-BC faces, Dirichlet rows / entries), one event pair per call
    asm_t = api.Timer()
    asm_ms = {"F": [], "J": []}
    for _ in range(5):
        asm_t.start(); P.assemble_system(wg_d, dwg_d, F_d, want_J=False); asm_t.stop(); asm_ms["F"].append(asm_t.ms())
        asm_t.start(); P.assemble_system(wg_d, dwg_d, None, want_J=True); asm_t.stop(); asm_ms["J"].append(asm_t.ms())
    asm_F_ms, asm_J_ms = float(np.median(asm_ms["F"])), float(np.median(asm_ms["J"]))

    # ---- time to the reference's tolerance (rtol 1e-4, main.c:406) on the same system: full GMRES, PC_ILU0 (multicolor
    # block-DILU; the Jacobi tree does not reach 1e-4 within 300 iterations at this size) -- outside the timed steps
    to_rtol = None
    if args.solve_to_rtol:
        L.KrylovSetPCType.argtypes = [C.c_void_p, C.c_int]
        ksp_i = C.cast(P.ksp, C.POINTER(C.c_int32))
        ksp_f = C.cast(P.ksp, C.POINTER(C.c_double))
        ksp_i[0] = 300                    # Krylov.max_iter
        ksp_f[1], ksp_f[2] = 1e-12, 1e-4  # Krylov.atol, rtol
        L.KrylovSetPCType(P.ksp, api.PC_ILU0)
        res = []
        for rep in range(2):              # the first solve builds the DILU coloring and grows the basis
            x_d.zero()
            api.sync(); quiet(); tw = time.perf_counter()
            it2, r02, hist2, conv2 = P.solve(x_d, F_d)
            api.sync(); res.append(time.perf_counter() - tw)
        to_rtol = {"pc": "PC_ILU0 (multicolor block-DILU)", "rtol": 1e-4, "iterations": it2, "converged": bool(conv2),
                   "ms": 1e3 * res[-1], "relative_residual": float(hist2[-1] / r02) if len(hist2) else None,
                   "dofs_per_s": 4.0 * N / res[-1]}
        # the same solve with PC_TWOLEVEL (DILU smoothing + aggregation coarse level, FGMRES; build-defined)
        ksp_i[0] = 100
        L.KrylovSetPCType(P.ksp, api.PC_TWOLEVEL)
        res = []
        for rep in range(2):              # the first solve builds the aggregates and the coarse matrix
            x_d.zero()
            api.sync(); quiet(); tw = time.perf_counter()
            it3, r03, hist3, conv3 = P.solve(x_d, F_d)
            api.sync(); res.append(time.perf_counter() - tw)
        to_rtol["twolevel"] = {"pc": "PC_TWOLEVEL (block-DILU smoother + aggregation coarse level, FGMRES)", "iterations": it3,
                               "converged": bool(conv3), "ms": 1e3 * res[-1], "first_solve_incl_hierarchy_build_ms": 1e3 * res[0],
                               "relative_residual": float(hist3[-1] / r03) if len(hist3) else None, "dofs_per_s": 4.0 * N / res[-1]}
        L.KrylovSetPCType(P.ksp, api.PC_DECOMPOSITION)
        ksp_i[0] = its
        ksp_f[1], ksp_f[2] = 0.0, 0.0

    cpu_M = args.M if args.cpu_M < 0 else args.cpu_M
    cpu = cpu_baseline(cpu_M, args.cpu_single_M, its) if cpu_M > 0 else None

    # ---- DEM contact sweep (BASELINE config 4 inputs: P = 100k, R = 0.004), outside the timed step ------------
    dem = None
    if args.dem_particles > 0:
        from dedflow_amd.meshgen import dem_particles
        xp, vp_, R = dem_particles(args.dem_particles, 0.004)
        pc = api.Particles(xp, vp_, R)
        pc.compute_forces()
        api.sync()
        quiet()
        nrep = 50
        tw = time.perf_counter()          # un-instrumented: the in-library profiler puts two event packets around the force
        for _ in range(nrep):             # kernel, which is a visible share of a 50 us sweep
            pc.compute_forces()
        api.sync()
        tw = (time.perf_counter() - tw) / nrep
        L.DflProfileEnable(1)             # separate pass for the force kernel's own duration
        for _ in range(20):
            pc.compute_forces()
        api.sync()
        tot, mn = C.c_double(0), C.c_double(0)
        cnt = L.DflProfileCollect(9, C.byref(tot), C.byref(mn))
        L.DflProfileEnable(0)
        kbar = None
        if cpu_M > 0:  # mean neighbours actually tested, from the CPU oracle's cell list (same inputs)
            from oracle import orc
            _, tested = orc.dem_forces(xp, vp_, R)
            kbar = tested / float(args.dem_particles)
        P_ = float(args.dem_particles)
        dbytes = (48.0 + 24.0) * P_ + 24.0 * P_ * (kbar if kbar is not None else 0.0)
        dem = {"particles": args.dem_particles, "radius": R, "sweep_ms_incl_cell_sort": 1e3 * tw,
               "force_kernel_avg_ms": tot.value / max(cnt, 1), "mean_tested_neighbours": kbar,
               "force_kernel_GBps": dbytes / (tot.value / max(cnt, 1) * 1e-3) / 1e9 if cnt else None,
               "particles_per_s": P_ / tw}
        pc.close()

    # ---- coupled step of BASELINE config 4 (1M-tet fluid mesh + 100k DEM particles), outside the timed region ----------
    coupled = None
    if args.coupled_M > 0 and args.dem_particles > 0:
        from dedflow_amd.meshgen import dem_particles
        m4 = kuhn_cube(args.coupled_M, jitter=args.jitter)
        w4, dw4 = synthetic_fields(m4)
        N4 = m4.num_node
        w4[3 * N4:4 * N4] = 0.0
        P4 = api.Problem(m4, maxit=120, atol=1e-12, rtol=1e-4, quiet=True)
        xp, vp_, R = dem_particles(args.dem_particles, 0.004)
        pc4 = api.Particles(xp, vp_, R, dt=1e-4)
        st = [api.DeviceArray.from_numpy(a) for a in (w4, 0.1 * dw4, 0.1 * dw4)]
        F4, dx4 = api.DeviceArray(6 * N4), api.DeviceArray(6 * N4)
        substeps, newton = 10, 2
        P4.time_step(st[0], st[1], st[2], F4, dx4, newton_maxit=newton, particles=pc4, dem_substeps=substeps)
        api.sync()
        quiet()
        tw = time.perf_counter()
        nrep = 3
        its4 = 0
        for _ in range(nrep):
            it4, _, _ = P4.time_step(st[0], st[1], st[2], F4, dx4, newton_maxit=newton, particles=pc4, dem_substeps=substeps)
            its4 += it4
        api.sync()
        tw = (time.perf_counter() - tw) / nrep
        coupled = {"workload": f"Kuhn cube M={args.coupled_M} ({m4.num_tet} tets) + {args.dem_particles} particles: DflTimeStep = predictor, "
                               f"<= {newton} Newton iterations (F, J assembly + Jacobi-GMRES to rtol 1e-4, <= 120 its), corrector, "
                               f"{substeps} DEM contact sweeps + particle updates",
                   "ms_per_coupled_step": 1e3 * tw, "newton_iterations_per_step": its4 / nrep}
        pc4.close()
        P4.close()

    tJ = kernels.get("asm_lhs", {}).get("total_ms_per_step", 0.0)
    tF = kernels.get("asm_rhs", {}).get("total_ms_per_step", 0.0)
    return {
        "spmv_GBps": kernels.get("spmv", {}).get("GBps"), "spmv_frac_of_hbm_peak": kernels.get("spmv", {}).get("frac_of_8TBps"),
        # whole AssembleSystem calls (pack + element kernels + faces + Dirichlet), event-timed; the element kernels alone
        # are in `kernels` (asm_lhs / asm_rhs)
        "assemble_J_dofs_per_s": 4.0 * N / (asm_J_ms * 1e-3), "assemble_F_dofs_per_s": 6.0 * N / (asm_F_ms * 1e-3),
        "assemble_J_ms": asm_J_ms, "assemble_F_ms": asm_F_ms,
        "assemble_J_kernel_dofs_per_s": (4.0 * N / (tJ * 1e-3)) if tJ else None,
        "assemble_F_kernel_dofs_per_s": (6.0 * N / (tF * 1e-3)) if tF else None,
        "solve_to_rtol": to_rtol,
        "roofline": roofline, "kernels": kernels, "cpu_baseline": cpu, "dem_sweep": dem,
        "spmv_back_to_back_ms": spmv_grouped_ms, "coupled_step": coupled,
    }


if __name__ == "__main__":
    main()
