#!/usr/bin/env python3
"""bench.py -- headline benchmark of the blob-mobility hot path on MI355X.

Workload (BASELINE.json configs[2]): 200 bodies x shell_N_642 = 128 400 blobs,
wall-corrected RPY mobility with wall damping, fp64, synthetic configuration of
SURVEY.md section 8(d).  One "step" = one pass of the hot path:

    blob positions from (X, Q) on the device  ->  [all-gather positions, forces]  ->
    matrix-free  U = B M B F  for this rank's rows

N = 1:  everything on one GPU.   N > 1: bodies sharded contiguously over ranks (one
process per GPU, torch.distributed / RCCL all-gather), total work fixed -> "strong".

    python bench.py --gpus 1 --steps 10 --warmup 2
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A plain run sets up, warms up, times the steps and prints ONE JSON line on rank 0: the headline figure with its
`roofline` (the dominant kernel, bracketed by events inside the timed steps) and, at N > 1, `per_rank`: where each
rank's time went (kernel min / max, all-gather, all-reduce, per-body work).  Everything else is measured only with

    python bench.py --full

after the timed steps: the time-step variants (`timestep`) at every N; at N = 1 two more passes of the steps (`repeats`),
`cpu_baseline` (the CPU oracle -- a port of the reference algorithm -- on a bounded row sample), the drop-in and multi-RHS
solves and `configs`: every other BASELINE.json configuration (cfg 1 / cfg 2 products and converged time steps, cfg 5's
dense build / Cholesky / L W), each priced against the roofline that bounds it; at N > 1 the row split (`partitionings.rows`).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

CONFIGS = {
    # name: (bodies, blobs/body, wall)
    "cfg1": (10, 12, False),
    "cfg2": (50, 162, False),
    "cfg3": (200, 642, True),
    "cfg5": (20, 2562, False),
}
FLOPS_PER_PAIR = {False: 59.0, True: 204.0}   # reference arithmetic per ordered pair
PEAK_FP64_TFLOPS = 78.6                       # MI355X fp64 vector == fp64 matrix peak
PEAK_HBM_GBS = 8000.0                         # HBM3E, MI355X_MICROARCH.md
PEAK_CLOCK_GHZ = 2.4                          # the clock that peak is quoted at
N_SIMD = 1024                                 # 256 CUs x 4 SIMDs; one wave64 fp64 VALU instruction occupies a SIMD for 4 cycles


# Definitions of every key of the one-line record (`python bench.py --notes`; committed as profiles/r05_bench_line_notes.json).  The line
# itself carries numbers only; the full record with every residual, iteration count and phase timing goes to the sidecar (--detail).
NOTES = {
    "value": "M.F passes per second: 1 step = one matrix-free apply_M pass of the hot path (blob positions from (X, Q) -> U = B M B F), the product "
             "every Krylov iteration of a time step runs; inputs resident in HBM; whole time steps are in summary.timesteps_per_sec",
    "mf_gflops": "dense-equivalent M.F rate 18 N^2 / t (SURVEY.md 8d), implementation independent",
    "roofline": "dominant kernel of the step, hipEvents on the context's stream: achieved = EXECUTED flops per unordered pair (assembly of this "
                "build, librbl.isa.json) x pairs per launch / kernel_ms; peak = 78.6 TFLOP/s fp64 (vector = matrix: one pipe on gfx950); "
                "valu_issue_frac = VALU instructions x 4 cycles / (1024 SIMDs x 2.4 GHz x kernel time); traffic = HBM bytes per launch from the "
                "PMC passes under profiles/ (2 x FETCH_SIZE + WRITE_SIZE), null once the kernel code differs from the profiled one; "
                "SURVEY.md 8d's reference-arithmetic price (204 flop per ORDERED pair) is in the sidecar as reference_equivalent_tflops",
    "cpu_baseline": "oracle/rbl_oracle.c orc_apply_M_rows (port of the reference arithmetic, matrix-free because the reference's dense 3N x 3N "
                    "matrix would need 1.19 TB at this size; gcc -O3) on a bounded row sample of the same workload, scaled by N / rows",
    "summary.timesteps_per_sec": "SURVEY.md 8(d): deterministic_fixed_work = 20 GMRES iterations (21 apply_M, diagonal PC; NOT converged: see "
                                 "fixed_work_residual); deterministic_converged = block PC, GMRES to 1e-8 from the quadratic extrapolation "
                                 "of the last solutions (constant body force), per-body factors rebuilt every 4th step; brownian_converged = stochastic "
                                 "midpoint step, fresh noise every step: 2 M^{1/2}W (preconditioned lock-step Lanczos to 1e-3, two-level factor) + M_RFD "
                                 "+ Kinv at q^n, block-PC GMRES to 1e-8 from zero at q^{n+1/2}, update from q^n -- the physically meaningful step of "
                                 "configs[3]; brownian_relaxed_products = the same with far tile pairs in packed single precision inside the inexact "
                                 "Krylov iterations (opt-in); brownian_relaxed_root_only = packed single precision inside the two roots only "
                                 "(their tolerance is 1e-3, the product error 1e-6), every GMRES product fp64 (opt-in, RBL_OPT_RELAXED_KRYLOV = 2); "
                                 "brownian_lanczos_1e-6 = the same with the roots to 1e-6",
    "summary.brownian_gmres_rtol_matched_to_root": "NOT a headline: the Brownian step with the GMRES tolerance set to the root's (1e-3, 1e-4) instead of "
                                                   "1e-8; U_err_vs_1e-8_solve = |U - U_ref| / |U_ref| of the body velocities against the 1e-8 solve of the "
                                                   "SAME right-hand side (measured after the timed steps), root_err = measured root identity error",
    "summary.brownian_converged_detail": "iterations, products per step, root_err = measured root identity error |root(s) - B M v| / |B M v|, gmres_res_max = "
                                         "largest GMRES residual of the timed steps, and the per-phase GPU milliseconds (rbl_get_timings) of brownian_converged",
    "summary.cpu_timesteps_per_sec": "the CPU port's measured seconds per apply_M x the MEASURED product count of each GPU step (O(N) work not counted: a "
                                     "lower bound on the CPU time), 1 core (the reference is single-threaded) and the box's host cores",
    "summary.roofline_frac": "cfg3_apply_M = roofline.frac; cfg1 / cfg2 apply_M against the fp64 peak with their own kernels' executed flops (wall clock "
                             "over 200 launches incl. the slab reduction; cfg 1 is launch-latency bound); cfg5: k_build_M against 8 TB/s (8 (3N)^2 bytes "
                             "written), Cholesky against 78.6 TFLOP/s ((3N)^3 / 3 flop), L W against 8 TB/s (4 (3N)^2 bytes read)",
    "summary.dropin_cfg3_ms": "host vectors through the RigidBody wrapper, PCIe inclusive: one apply_saddle / apply_PC call, scipy.sparse.linalg.gmres "
                              "(restart 40, rtol 1e-8) over them (the reference's usage model, src/Rigid.py:69-80), and the library's own solver on "
                              "the same right-hand side",
    "summary.dropin_cfg2_scipy_gmres_ms": "median of five SciPy solves at cfg 2 before and after cfg 5 mapped 189 GB in this process, host BLAS pool limited "
                                          "to blas_threads (the box's CPU share); default_pool_min_max = the same solves with the pool at its default "
                                          "(every core of the host): the 12-vs-92 ms spread of round 4 is BLAS oversubscription, not cfg 5 and not the operators",
    "summary.multi_rhs": "rbl_gmres_saddle_multi_dev at the headline configuration: 16 right-hand sides (sets of body loads) in lock step, their products ONE "
                         "launch of the fp64-MFMA kernel per iteration, against sequential rbl_gmres_saddle_dev solves (two timed, scaled to 16): "
                         "ratio_to_sequential = lock_step_ms / (16 x sequential_ms_per_solve); column_vs_sequential_solve = largest relative "
                         "difference of a column to its own sequential solve",
}


_REAL_STDOUT = None


def protect_stdout():
    """The contract is ONE JSON line on stdout.  Libraries write there too (RCCL prints a five-line version banner to fd 1 when a
    communicator is created): keep a private handle on the real stdout for the line and point fd 1 at stderr for everybody else."""
    global _REAL_STDOUT
    if _REAL_STDOUT is None:
        sys.stdout.flush()
        _REAL_STDOUT = os.fdopen(os.dup(1), "w")
        os.dup2(2, 1)


def emit(text):
    out = _REAL_STDOUT or sys.stdout
    out.write(text + "\n")
    out.flush()


def visible_gpus():
    """GPUs this process may use, counted WITHOUT touching the HIP runtime (the parent of a self-launched job must not
    initialise the GPU before it starts its ranks): GPU nodes of the KFD topology, cut down by the *_VISIBLE_DEVICES lists."""
    n = 0
    base = "/sys/class/kfd/kfd/topology/nodes"
    try:
        for d in os.listdir(base):
            try:
                props = dict(l.split()[:2] for l in open(os.path.join(base, d, "properties")) if len(l.split()) >= 2)
            except OSError:
                continue
            if int(props.get("simd_count", "0")) > 0:
                n += 1
    except OSError:
        return 0
    for var in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None:
            n = min(n, len([x for x in v.split(",") if x.strip() != ""]))
    return n


def self_launch(args, argv):
    """`python bench.py --gpus N` without torchrun: start the N-rank job as CHILD processes (one rank per GPU, RCCL)
    before this process has touched the GPU, print the ONE line and exit with the job's status.  Two phases, so that the
    headline line survives whatever happens to the (much longer) time-step part: phase `main` times the hot path and
    produces the line; phase `timestep` (apply_M mode with --full and --timestep-steps > 0 only) runs the time-step variants as a
    second job under a time limit and its result -- or the reason it is missing -- is merged into the line; a missing
    time-step part makes the exit status non-zero (the line is still printed).  Every job runs in its own session: on a
    time-out the whole process group is terminated, then killed, so no rank outlives bench.py holding a GPU."""
    import signal
    import subprocess
    ndev = visible_gpus()
    if args.backend == "nccl" and ndev < args.gpus:
        raise SystemExit("bench.py: --gpus %d needs %d visible GPUs, found %d (use --backend gloo to rehearse several "
                         "ranks on one GPU)" % (args.gpus, args.gpus, ndev))
    if ndev < 1:
        raise SystemExit("bench.py: no GPU visible")

    def run(phase, timeout):
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", RBL_BENCH_PHASE=phase)
        env.setdefault("OMP_NUM_THREADS", "4")
        # --standalone: torchrun picks (and holds) a free rendezvous port itself -- no bind-then-close race
        cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1", "--nnodes=1",
               "--nproc-per-node", str(args.gpus), os.path.abspath(__file__)] + argv
        p = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True, start_new_session=True)
        try:
            out, _ = p.communicate(timeout=timeout)
            return p.returncode, out, None
        except subprocess.TimeoutExpired:
            killed = "terminated"
            try:
                os.killpg(p.pid, signal.SIGTERM)
                try:
                    out, _ = p.communicate(timeout=20)
                except subprocess.TimeoutExpired:
                    os.killpg(p.pid, signal.SIGKILL)
                    killed = "killed"
                    out, _ = p.communicate()
            except ProcessLookupError:
                out, _ = p.communicate()
            return 124, (out or ""), "timed out after %d s, ranks %s" % (timeout, killed)

    two_phase = args.mode == "apply_M" and args.timestep_steps > 0
    rc, out, why = run("main" if two_phase else "all", 3000)
    lines = [l for l in out.splitlines() if l.startswith("{")]
    if rc != 0 or not lines:
        sys.stdout.write(out)
        raise SystemExit(rc or 1)
    if not two_phase:
        sys.stdout.write(out)
        raise SystemExit(0)
    protect_stdout()
    line = json.loads(lines[-1])
    rc2, out2, why2 = run("timestep", 1500)
    l2 = [l for l in out2.splitlines() if l.startswith("{")]
    ok = rc2 == 0 and bool(l2)
    if ok:
        line["timestep"] = json.loads(l2[-1])
        line["timesteps_per_sec"] = headline_timesteps(line["timestep"])
    else:
        line["timestep"] = {"error": "the time-step job did not finish (%s)" % (why2 or ("exit status %d" % rc2))}
    finish(line, args)
    raise SystemExit(0 if ok else 3)


def kernel_source_hash():
    import hashlib
    h = hashlib.sha256()
    for f in ("rbl_kernels.hip", "rbl_pair.hpp"):
        h.update(open(os.path.join(ROOT, "rigid_body_light_amd", "csrc", f), "rb").read())
    return h.hexdigest()


def isa_counts(kernel):
    """executed instructions per unordered pair of `kernel` in the far-tile sweep, from the assembly of the
    sources librbl.so was built from (tools/isa_stats.py, written by rigid_body_light_amd/build.py); ignored when the
    kernel sources have changed since (hash recorded in the file)"""
    path = os.path.join(ROOT, "rigid_body_light_amd", "librbl.isa.json")
    try:
        d = json.load(open(path))
        if d.get("kernel_source_sha256") != kernel_source_hash():
            return None
        k = d["kernels"][kernel]
        return k.get("per_unordered_pair") or k["per_ordered_pair"]     # (the ordered-rows kernel is counted per ORDERED pair)
    except (OSError, KeyError, ValueError):
        return None


def pmc_traffic(kernel, config, world):
    """HBM bytes per launch of `kernel` from the rocprofv3 PMC passes committed under profiles/ -- only while the built
    library holds the same kernel code as the profiled one: the file records the sha256 of the profiled instance's
    instruction text, tools/isa_stats.py computes the same for every build (librbl.isa.json)."""
    for rnd in ("r05", "r04", "r03", "r02"):
        path = os.path.join(ROOT, "profiles", "%s_bench_%s_pmc.json" % (rnd, config))
        try:
            d = json.load(open(path))
            isa = json.load(open(os.path.join(ROOT, "rigid_body_light_amd", "librbl.isa.json")))
            if isa.get("kernel_source_sha256") != kernel_source_hash():       # stale assembly analysis: nothing to compare with
                return None, None
            same = d.get("kernel_isa_sha256") and d["kernel_isa_sha256"] == isa["instance_isa_sha256"].get(d.get("kernel_instance"))
            if not same or world != 1 or d.get("kernel") != kernel:
                continue
            return d["hbm_bytes_per_launch"], d
        except (OSError, KeyError, ValueError):
            continue
    return None, None


def cpu_baseline(c, nb, nblb, wall, budget_s):
    """Time the CPU oracle (port of reference :413-459,:641-659, matrix-free restatement)
    on a bounded sample of rows of the SAME workload; scale to one full apply_M."""
    from oracle import Oracle
    orc = Oracle()
    cfg = c["cfg"] - c["cfg"].mean(axis=0)
    r = orc.multi_body_pos(c["X"], c["Q"], cfg)
    N = nb * nblb
    F = np.random.default_rng(2).standard_normal(3 * N)
    out = {}
    try:
        ncores = len(os.sched_getaffinity(0))
    except AttributeError:
        ncores = os.cpu_count() or 1
    ncores = min(ncores, int(os.environ.get("RBL_CPU_THREADS", "16")))   # a 1-GPU box's CPU share is 16 cores
    for label, nthreads in (("1core", 1), ("allcores", ncores)):
        rows = 4 * nthreads
        t0 = time.perf_counter(); orc.apply_M_rows(F, r, 0, rows, c["a"], c["eta"], wall, nthreads); t1 = time.perf_counter()
        per_row = (t1 - t0) / rows
        rows = int(max(rows, min(N, budget_s / max(per_row, 1e-9))))
        b = (N // 2 // max(nblb, 1)) * nblb
        b = min(b, N - rows)
        t0 = time.perf_counter(); orc.apply_M_rows(F, r, b, b + rows, c["a"], c["eta"], wall, nthreads); t1 = time.perf_counter()
        t_full = (t1 - t0) * N / rows
        out[label] = {"value": 1.0 / t_full, "unit": "steps/s", "cores": nthreads, "kind": "port",
                      "sample": "%d of %d rows x all %d columns of the same workload, %.1f s measured, "
                                "scaled by N/rows; oracle/rbl_oracle.c orc_apply_M_rows (gcc -O3 -march=x86-64-v3, "
                                "reference pair arithmetic, matrix-free because the reference's dense 3Nx3N matrix "
                                "would need %.2f TB)" % (rows, N, N, t1 - t0, 8.0 * (3 * N) ** 2 / 1e12),
                      "seconds_per_step": t_full}
    return out


def sym_kernel_name(ctx, wall, n_blobs, i_step=1):
    """the instantiation a one-vector symmetric product of that size launches under the context's options (rbl_apply_M_sym_kernel:
    the library's own launch decisions), in the naming of librbl.isa.json"""
    return ctx.apply_M_sym_kernel(int(n_blobs), wall, i_step=i_step)


def apply_opts(ctx, args):
    """--opt name=value switches onto a context (named options of include/rbl.h)"""
    for kv in args.opt:
        name, _, val = kv.partition("=")
        ctx.set_option(name.strip(), int(val))


def gather_ranks(values, dev, world):
    """values: list of floats of this rank -> (world, len) numpy array on every rank"""
    t = torch.tensor(values, dtype=torch.float64, device=dev)
    if world == 1:
        return t.cpu().numpy()[None, :]
    buf = [torch.empty_like(t) for _ in range(world)]
    dist.all_gather(buf, t)
    return torch.stack(buf).cpu().numpy()


def phase_block(ctx, steps, dev, world):
    """per-rank, per-time-step GPU milliseconds of librbl's phases (rbl_get_timings) -> {phase: {min, max, per_rank}}"""
    tm = ctx.timings()
    names = list(ctx.TIMING_PHASES)
    arr = gather_ranks([tm[k][0] / max(steps, 1) for k in names], dev, world)
    out = {}
    for i, k in enumerate(names):
        out[k + "_ms"] = {"min": float(arr[:, i].min()), "max": float(arr[:, i].max()), "per_rank": [round(float(x), 4) for x in arr[:, i]]}
    out["collectives_per_step"] = tm["collective"][1] / float(max(steps, 1))     # (brackets around the collectives of rank 0: their count)
    out["note"] = ("GPU milliseconds per time step and rank between hipEvents on the context's stream (rbl_get_timings): product = pair "
                   "kernels + slab reduction of this rank's tile pairs; per_body = applications of the rank's own per-body factors; factor "
                   "= their build; collective = the all-reduce callback incl. the wait for the slowest rank; total = the solver calls "
                   "(what it holds beyond the others is Krylov vector work, K operators, launch gaps, host convergence tests)")
    return out


def root_identity_error(ctx, nb, nblb, a, dev):
    """MEASURED accuracy of the preconditioned Lanczos root x = B G Sp^{1/2} W (Sp = G^-1 M G^-T, G the library's factor of
    this configuration) at the context's current tolerance, outside any timed region: with s = Sp^{1/2} W = G^-1 B^-1 x and
    v = G^-T W an exact root satisfies root(s) = B M v (one extra mobility product); returns |root(s) - B M v| / |B M v|.  The reference's factor is exact
    (c_rigid_obj.cpp:670-672); an iterative replacement must state its error."""
    N = nb * nblb
    n = 3 * N
    r = torch.empty(n, dtype=torch.float64, device=dev)
    ctx.blob_positions(0, nb, r.data_ptr())
    z = r.view(-1, 3)[:, 2]
    B = torch.where(z >= a, torch.ones_like(z), z / a).repeat_interleave(3)            # make_damp_mat :618-639
    W = torch.from_numpy(np.random.default_rng(33).standard_normal(n)).to(dev)

    def root(vec):
        out = torch.empty_like(vec)
        ctx.M_half_W(r.data_ptr(), N, vec.contiguous().data_ptr(), "lanczos_pc", out.data_ptr())
        return out

    def bsolve(vec, mode):
        out = torch.empty_like(vec)
        ctx.block_solve(vec.contiguous().data_ptr(), out.data_ptr(), mode)
        return out

    x = root(W)
    s_ = bsolve(x / B, 5)               # modes 5 / 6: the root's whole factor G (two-level by default), G^-1 and G^-T
    v = bsolve(W, 6)
    Mv = torch.empty_like(v)
    ctx.set_no_damp(True)
    try:
        ctx.apply_M(v.data_ptr(), r.data_ptr(), N, 0, N, Mv.data_ptr())
    finally:
        ctx.set_no_damp(False)
    ref = B * Mv
    e = float(torch.linalg.norm(root(s_) - ref) / torch.linalg.norm(ref))
    ctx.sync_check()
    return e


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(path, arrays):
    """--dump-outputs DIR: what the timed path computed in its last step, one DIR/<name>.npy (float64) per array, so that two
    builds can be compared output for output (every input is seeded: the same arguments give the same inputs in every run)."""
    arrays = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in arrays.items()}
    total = sum(v.nbytes for v in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit("bench.py: --dump-outputs would write %d bytes (limit %d)" % (total, DUMP_LIMIT_BYTES))
    os.makedirs(path, exist_ok=True)
    for k, v in arrays.items():
        np.save(os.path.join(path, k + ".npy"), v)


def timestep_mode(args, dev, world=1, rank=0):
    """1 step = one time step, all operators on the GPU(s), every loop inside librbl; with N > 1 the mobility
    product of every Krylov iteration is tile-pair sharded (one all-reduce per iteration)."""
    from rigid_body_light_amd import make_config
    from rigid_body_light_amd._lib import DeviceContext
    from rigid_body_light_amd.dist import ShardedMobility
    from rigid_body_light_amd.krylov import (BrownianStepper, DeterministicStepper, ShardedBrownianStepper,
                                             ShardedDeterministicStepper)
    nb, nblb, wall = CONFIGS[args.config]
    c = make_config(nb, nblb, wall)
    N = nb * nblb
    brownian = args.kBT > 1e-10
    ctx = DeviceContext(c["a"], c["eta"], wall, cfg=c["cfg"], dt=c["dt"], kBT=args.kBT,
                        stream_ptr=torch.cuda.current_stream().cuda_stream)
    if args.pc == "block":
        from rigid_body_light_amd._lib import lib
        lib().rbl_set_blk_pc(ctx.h, 1)
    ctx.set_config(c["X"], c["Q"])
    apply_opts(ctx, args)
    iters = 20 if args.rtol <= 0 else 200
    rtol = args.rtol if args.rtol > 0 else None
    Fb = np.tile([0.0, 0.0, -1.0, 0.0, 0.0, 0.0], nb)
    lanczos_its = None
    if brownian:   # stochastic midpoint step: 2 M^{1/2}W + M_RFD + Kinv, then the saddle solve at q^{n+1/2}
        method = {"cholesky": 0, "lanczos": 1, "lanczos_pc": 2}[args.mhalf]
        if world > 1 or args.sharded_driver:
            if method == 0:
                raise SystemExit("the sharded Brownian step uses the Lanczos square root")
            bst = ShardedBrownianStepper(ctx, ShardedMobility(nb, nblb, device=dev, ctx=ctx), nb, nblb, dev, c["a"], wall,
                                         args.kBT, c["dt"], lanczos_tol=args.lanczos_tol, precondition=(method == 2))
            stp_step = lambda k: bst.step(Fb, seed=k, iters=iters, rtol=rtol)
            lanczos_its = lambda: list(bst.lanczos_iterations)
        else:
            ctx.set_lanczos(200, args.lanczos_tol)
            bst = BrownianStepper(ctx, nb, nblb, dev)
            stp_step = lambda k: bst.step(Fb, seed=k, method=method, iters=iters, rtol=rtol)
            lanczos_its = (lambda: [ctx.lanczos_report()[0]]) if method != 0 else None
    else:
        if world > 1:
            stp = ShardedDeterministicStepper(ctx, ShardedMobility(nb, nblb, device=dev, ctx=ctx), nb, nblb, dev)
        else:
            stp = DeterministicStepper(ctx, nb, nblb, dev)
        stp.warm_start = args.warm_start or args.extrapolate > 0
        if args.block_refresh > 1:
            ctx.set_block_refresh(args.block_refresh)
        stp.extrapolate = args.extrapolate
        stp_step = lambda k: stp.step(Fb, iters, rtol)
    res, used = [], []
    for k in range(args.warmup):
        stp_step(k)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    ctx.set_timing(True); ctx.reset_timings()
    t0 = time.perf_counter()
    for k in range(args.steps):
        m_used, r_last = stp_step(args.warmup + k)
        res.append(r_last); used.append(m_used)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t1 = time.perf_counter()
    if args.dump_outputs and rank == 0:                     # the body configuration the last timed step left
        X, Q = ctx.get_config(nb)
        dump_outputs(args.dump_outputs, {"body_positions": X, "body_quaternions": Q})
    phases = phase_block(ctx, args.steps, dev, world)
    ctx.set_timing(False)
    sec_t = torch.tensor([(t1 - t0) / args.steps], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(sec_t, op=dist.ReduceOp.MAX)
    sec = float(sec_t.item())
    iters = int(round(sum(used) / len(used)))
    if world > 1 and rank != 0:
        dist.destroy_process_group()
        return
    kind = "deterministic step"
    extra = {}
    if brownian:
        kind = ("stochastic midpoint step, kBT=%g: 2 M^{1/2}W (%s) + M_RFD (2 apply_M) + Kinv, then" % (args.kBT, args.mhalf))
        n_prod = iters + 1 + 2
        if lanczos_its is not None:
            extra["lanczos_iterations_last_step"] = lanczos_its()
            n_prod += sum(extra["lanczos_iterations_last_step"]) * (1 if len(extra["lanczos_iterations_last_step"]) > 1 else 2)
        extra["apply_M_per_step"] = n_prod
    emit(json.dumps({
        "metric": "timesteps/sec (%s: %d GMRES iterations (%s, %s PC) = %d apply_M + PC + K ops + evolve), "
                  "%d x shell_N_%d, %s, fp64" % (kind, iters, "fixed work" if rtol is None else "converged to %g" % rtol, args.pc,
                                                 iters + 1, nb, nblb, "wall-corrected" if wall else "free-space"),
        "value": 1.0 / sec, "unit": "timesteps/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": sec * 1e3, "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64",
        "data": "synthetic", "config": {"workload": args.config, "bodies": nb, "blobs_per_body": nblb, "n_blobs": N, "wall": wall},
        "mf_gflops": extra.get("apply_M_per_step", iters + 1) * 18.0 * float(N) ** 2 / sec / 1e9, "gmres_residual": res[-1], "gmres_iterations": used,
        "block_refresh": args.block_refresh, "initial_guess": (["previous solution", "2 x_n - x_{n-1}", "3 x_n - 3 x_{n-1} + x_{n-2}"][args.extrapolate]
                          if (args.warm_start or args.extrapolate) and not brownian else "zero"),
        "phases": phases, **extra}))
    if world > 1:
        dist.destroy_process_group()


def brownian_mode(args, dev, world, rank):
    """BASELINE cfg 4: wall-corrected + Brownian on N GPUs.  1 step = one Brownian increment M^{1/2} W by librbl's
    Lanczos (block-Jacobi preconditioned by default) on the tile-pair-sharded product (rbl_set_comm: one all-reduce per
    product)."""
    from rigid_body_light_amd import make_config
    from rigid_body_light_amd._lib import DeviceContext
    from rigid_body_light_amd.dist import ShardedMobility
    nb, nblb, wall = CONFIGS[args.config]
    c = make_config(nb, nblb, wall)
    N = nb * nblb
    ctx = DeviceContext(c["a"], c["eta"], wall, cfg=c["cfg"], dt=c["dt"], stream_ptr=torch.cuda.current_stream().cuda_stream)
    ctx.set_config(c["X"], c["Q"])
    sm = ShardedMobility(nb, nblb, device=dev, ctx=ctx)
    ctx.set_comm(sm)
    if args.mhalf == "cholesky":
        raise SystemExit("--mode brownian measures the matrix-free square roots (--mhalf lanczos_pc | lanczos)")
    r = torch.empty(3 * N, dtype=torch.float64, device=dev)
    ctx.blob_positions(0, nb, r.data_ptr())
    W = torch.from_numpy(np.random.default_rng(3).standard_normal(3 * N)).to(dev)   # identical on every rank
    out = torch.empty_like(W)
    ctx.set_lanczos(200, args.lanczos_tol)
    one = lambda: ctx.M_half_W(r.data_ptr(), N, W.data_ptr(), args.mhalf, out.data_ptr())
    for _ in range(args.warmup):
        one()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        one()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    sec = torch.tensor([(time.perf_counter() - t0) / args.steps], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(sec, op=dist.ReduceOp.MAX)
    ctx.sync_check()
    its, est = ctx.lanczos_report()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"M_half_W": out.cpu().numpy()})
    if rank == 0:
        sec = float(sec.item())
        pc = args.mhalf == "lanczos_pc"
        emit(json.dumps({
            "metric": "Brownian increments/sec (M^{1/2} W by %s to %g, %d iterations), %d x shell_N_%d, %s, fp64"
                      % ("block-Jacobi preconditioned Lanczos" if pc else "Lanczos", args.lanczos_tol, its, nb, nblb,
                         "wall-corrected" if wall else "free-space"),
            "value": 1.0 / sec, "unit": "increments/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": sec * 1e3, "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64",
            "data": "synthetic", "config": {"workload": "BASELINE.json configs[3]" if args.config == "cfg3" else args.config,
                                            "bodies": nb, "blobs_per_body": nblb, "n_blobs": N, "wall": wall,
                                            "parallelism": "tile-pair-sharded x%d, all-reduce(U) per Lanczos iteration" % world},
            "lanczos_iterations": its, "lanczos_error_estimate": est, "mf_gflops": its * 18.0 * float(N) ** 2 / sec / 1e9}))
    if world > 1:
        dist.destroy_process_group()


def timestep_variants(args, ctx, sm, c, nb, nblb, wall, dev, world, stream, barrier, multi=None):
    """Time steps built on the hot path (the reference has no driver; SURVEY.md 8d defines them).  Every variant is timed
    over args.timestep_steps consecutive steps and carries its GMRES residuals and iteration counts.
      deterministic_fixed : 20 right-preconditioned GMRES iterations (diagonal PC) = 21 apply_M + K ops + evolve
      converged           : deterministic, block-diagonal PC, GMRES to 1e-8, extrapolated initial guess (N = 1)
      brownian_converged  : stochastic midpoint step (2 M^{1/2}W + M_RFD + Kinv at q^n, solve at q^{n+1/2}): block PC,
                            GMRES to 1e-8 from a zero guess, square root by block-Jacobi preconditioned Lanczos to 1e-3 / 1e-6."""
    from rigid_body_light_amd._lib import DeviceContext, lib
    from rigid_body_light_amd.krylov import DeterministicStepper, ShardedDeterministicStepper, BrownianStepper, ShardedBrownianStepper
    if multi is None:
        multi = world > 1          # (--force-comm: the N-rank code path with one rank)
    K = args.timestep_steps
    Fb = np.tile([0.0, 0.0, -1.0, 0.0, 0.0, 0.0], nb)

    def timed(step_fn, k0=0, tctx=None):
        barrier(); t0 = time.perf_counter()
        its, res = [], []
        for k in range(K):
            m, r = step_fn(k0 + k)
            its.append(int(m)); res.append(float(r))
        barrier()
        tv = torch.tensor([(time.perf_counter() - t0) / K], dtype=torch.float64, device=dev)
        if world > 1:
            dist.all_reduce(tv, op=dist.ReduceOp.MAX)
        t = float(tv.item())
        d = {"timesteps_per_sec": 1.0 / t, "ms_per_timestep": t * 1e3, "steps_timed": K, "gmres_iterations": its,
             "gmres_residual_max": max(res), "gmres_residual_last": res[-1]}
        if tctx is not None:        # where the time goes: two more steps with librbl's event brackets on (outside the timed ones)
            tctx.set_timing(True); tctx.reset_timings()
            for k in range(2):
                step_fn(k0 + K + k)
            d["phases"] = phase_block(tctx, 2, dev, world)
            d["phases"]["steps"] = "2 further steps, not the timed ones"
            tctx.set_timing(False)
        return d

    out = {}
    stp = (ShardedDeterministicStepper(ctx, sm, nb, nblb, dev, set_comm=False) if multi else DeterministicStepper(ctx, nb, nblb, dev))
    stp.step(Fb, 20)
    d = timed(lambda k: stp.step(Fb, 20), tctx=ctx)
    d.update({"apply_M_per_timestep": 21, "definition": "deterministic fixed-work step (SURVEY.md 8d): 20 GMRES iterations on the saddle "
              "operator, diagonal PC, + evolve; NOT converged (see gmres_residual_max)"})
    out["deterministic_fixed"] = d
    out.update({k: d[k] for k in ("timesteps_per_sec", "ms_per_timestep", "apply_M_per_timestep", "steps_timed")})
    out["definition"] = d["definition"]
    out["gmres_residual"] = d["gmres_residual_last"]
    if not multi:
        lib().rbl_set_blk_pc(ctx.h, 1)
        stp.warm_start = True; stp.extrapolate = 2     # initial guess 3 x_n - 3 x_{n-1} + x_{n-2}
        ctx.set_block_refresh(4)                       # per-body factors rebuilt every 4th configuration
        for _ in range(3):                             # fill the history (18, 12, 6 iterations), then 2-3 per step
            stp.step(Fb, 200, 1e-8)
        d = timed(lambda k: stp.step(Fb, 200, 1e-8))
        d.update({"rtol": 1e-8, "preconditioner": "block-diagonal, per-body factors rebuilt every 4th step",
                  "initial_guess": "quadratic extrapolation of the last three solutions (constant body force)"})
        out["converged"] = d
        # the same with the opt-in relaxation (RBL_OPT_RELAXED_KRYLOV = 1): the residual b - A x0 of the extrapolated guess is fp64,
        # the 1-2 products of the correction solve run on the packed-single-precision far field (inexact Krylov)
        ctx.set_option("relaxed_krylov", 1)
        d = timed(lambda k: stp.step(Fb, 200, 1e-8))
        ctx.set_option("relaxed_krylov", 0)
        d.update({"rtol": 1e-8, "relaxed_products": True})
        out["converged_relaxed"] = d
        lib().rbl_set_blk_pc(ctx.h, 0); ctx.set_block_refresh(1)
    # stochastic midpoint step, converged: BASELINE configs[3] (on N GPUs: `--mode timestep --kBT 1 --gpus N`)
    bro = {}
    variants = [(1e-3, False, False, 0, 1e-8), (1e-6, False, False, 0, 1e-8), (1e-3, True, False, 0, 1e-8), (1e-3, False, True, 0, 1e-8)]
    if multi:
        variants.append((1e-3, False, False, 1, 1e-8))       # the same step with the row split (all-gather of positions and U)
    else:                                                    # GMRES tolerance matched to the root's (never the headline): what it costs and errs
        variants += [(1e-3, False, False, 0, 1e-3), (1e-4, False, False, 0, 1e-4)]
        variants.append((1e-3, 2, False, 0, 1e-8))           # relaxed products inside the root only (RBL_OPT_RELAXED_KRYLOV = 2), GMRES all fp64
    for ltol, relaxed, energy, split, grtol in variants:
        bctx = DeviceContext(c["a"], c["eta"], wall, cfg=c["cfg"], dt=c["dt"], kBT=1.0, stream_ptr=stream.cuda_stream)
        lib().rbl_set_blk_pc(bctx.h, 1)
        bctx.set_config(c["X"], c["Q"]); bctx.set_lanczos(200, ltol)
        bctx.set_block_refresh(2)      # the per-body factors of q^n also serve the predictor configuration q^{n+1/2}
        bctx.set_option("two_level_refresh", 8)   # the root's factored coarse operator kept for 8 configuration changes (4 steps): exact for any
        apply_opts(bctx, args)
        if relaxed:                    # inexact Krylov (RBL_OPT_RELAXED_KRYLOV = 1; 2: in the root only): see the `relaxation` note below
            bctx.set_option("relaxed_krylov", int(relaxed))
        if energy:                     # stop the root on its energy-norm estimate (RBL_OPT_LANCZOS_EUCLID_NORM = 0): see `lanczos_norm` below
            bctx.set_option("lanczos_euclid_norm", 0)
        if multi:
            from rigid_body_light_amd.dist import ShardedMobility
            bst = ShardedBrownianStepper(bctx, ShardedMobility(nb, nblb, device=dev, ctx=bctx, force_collectives=args.force_comm), nb, nblb, dev, c["a"], wall, 1.0, c["dt"],
                                         lanczos_tol=ltol, lanczos_max_iter=200)
            bctx.set_option("comm_split", split)
            one = lambda k: bst.step(Fb, seed=k, iters=200, rtol=grtol)
            lz = lambda: list(bst.lanczos_iterations)
        else:
            bst = BrownianStepper(bctx, nb, nblb, dev)
            one = lambda k: bst.step(Fb, seed=k, method=2, iters=200, rtol=grtol)
            lz = lambda: [bctx.lanczos_report()[0]]
        one(0)
        d = timed(one, 1, tctx=bctx)
        d.update({"lanczos_tol": ltol, "lanczos_iterations_last_step": lz(), "lanczos_error_estimate_last_step": bctx.lanczos_report()[1],
                  "relaxed_products": ["no", "GMRES (late iterations) and the root", "the root only"][int(relaxed)]})
        if not multi:                  # measured, outside the timed region: one more pair of roots + one product
            d["root_identity_error"] = root_identity_error(bctx, nb, nblb, c["a"], dev)
        d["lanczos_stopping_norm"] = "energy" if energy else "euclidean"
        d["comm_split"] = ["tile pairs + all-reduce", "rows by body index + all-gather"][split] if multi else None
        d["gmres_rtol"] = grtol
        if grtol > 1e-8:               # measured, outside the timed region: the body velocities of this tolerance against the 1e-8 solve of the SAME system
            n3 = 3 * nb * nblb
            Xn, Qn = bctx.get_config(nb)
            rhs, Xh, Qh = bst.rhs_and_midpoint(Fb, None, None, 777, 2, True, 1.0e-4)
            bctx.set_config(Xh, Qh)
            x_lo, m_lo, _ = bst.saddle_solve(rhs, 200, grtol)
            x_hi, m_hi, _ = bst.saddle_solve(rhs, 200, 1e-8)
            bctx.set_config(Xn, Qn)
            d["velocity_error_vs_1e-8_solve"] = float(torch.linalg.norm(x_lo[n3:] - x_hi[n3:]) / torch.linalg.norm(x_hi[n3:]))
            d["constraint_force_error_vs_1e-8_solve"] = float(torch.linalg.norm(x_lo[:n3] - x_hi[:n3]) / torch.linalg.norm(x_hi[:n3]))
            d["gmres_iterations_of_the_two_solves"] = [int(m_lo), int(m_hi)]
        bro["lanczos_%g%s%s%s%s" % (ltol, "_relaxed_root" if relaxed == 2 else "_relaxed" if relaxed else "", "_energy_norm" if energy else "", "_rows" if split else "",
                                    "_gmres_%g" % grtol if grtol > 1e-8 else "")] = d
        del bst
        bctx.close()
        del bctx
    bro.update({"kBT": 1.0, "rtol": 1e-8, "initial_guess": "zero (fresh noise every step)",
                "lanczos_norm": "the preconditioned root x = B L z stops on an error estimate of x in its Euclidean norm (default; what "
                                "root_identity_error measures); the *_energy_norm entry stops on the estimate of z = (L^-1 M L^-T)^{1/2} W, "
                                "i.e. of x in the energy norm x^T (B M B)^-1 x that bounds the relative error of the sampled covariance -- "
                                "rounds 1-2 effectively used that one (fewer iterations, larger Euclidean error)",
                "root_identity_error": "|root(s) - B M v| / |B M v| with s = G^-1 B^-1 root(W), v = G^-T W for the root x = B G (G^-1 M G^-T)^{1/2} W "
                                       "the step uses (G: two-level factor), measured after the timed steps at the entry's Lanczos tolerance (zero for an exact root)",
                "relaxation": "the *_relaxed entries are opt-in (RBL_OPT_RELAXED_KRYLOV = 1; *_relaxed_root = 2: the Lanczos roots only, every GMRES product fp64), everything else is fp64 throughout: an inexact Krylov "
                              "iteration tolerates a relative product error of (tolerance / current residual), so GMRES iterations whose "
                              "residual estimate is below 1e-3 and the Lanczos iterations (tolerance 1e-3) evaluate far tile pairs in packed "
                              "single precision (product error ~1e-6, 1.8x faster); the solution still satisfies the fp64 system to 1e-8 "
                              "(true residual checked in tests/test_gpu_parity.py::test_relaxed_gmres_reaches_the_fp64_tolerance)",
                "factor_refresh": "opt-in, as in round 3: per-body factors kept for 2 configuration changes (q^n's serve q^{n+1/2}: rbl_set_block_refresh), "
                                  "round 4: the two-level factor's factored coarse operator kept for 8 (RBL_OPT_TWO_LEVEL_REFRESH; its basis Q follows "
                                  "every change, the root is exact for any coarse operator: test_two_level_refresh_keeps_the_root_exact)",
                "definition": "stochastic midpoint step: 2 M^{1/2}W (block-Jacobi preconditioned Lanczos, two vectors in lock step) + "
                              "M_RFD (2 apply_M) + Kinv at q^n, GMRES with the block-diagonal PC to 1e-8 at the predictor "
                              "configuration, update from q^n"})
    out["brownian_converged"] = bro
    return out


def other_configs(dev, stream, cpu=True):
    """The other BASELINE.json configurations, timed in the default N = 1 run (device-resident inputs, wall clock around
    stream-synchronised loops): each entry says what bounds it and how close it gets."""
    from rigid_body_light_amd import make_config
    from rigid_body_light_amd._lib import DeviceContext, lib
    from rigid_body_light_amd.krylov import BrownianStepper, DeterministicStepper
    out = {}

    def wall_time(fn, reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps

    def product_entry(name, kBT):
        nb, nblb, wall = CONFIGS[name]
        c = make_config(nb, nblb, wall)
        N = nb * nblb
        ctx = DeviceContext(c["a"], c["eta"], wall, cfg=c["cfg"], dt=c["dt"], kBT=kBT, stream_ptr=stream.cuda_stream)
        ctx.set_config(c["X"], c["Q"])
        r = torch.empty(3 * N, dtype=torch.float64, device=dev)
        ctx.blob_positions(0, nb, r.data_ptr())
        F = torch.from_numpy(np.random.default_rng(2).standard_normal(3 * N)).to(dev)
        U = torch.empty_like(F)
        one = lambda: ctx.apply_M(F.data_ptr(), r.data_ptr(), N, 0, N, U.data_ptr())
        for _ in range(5):
            one()
        ctx.sync_check()
        t = wall_time(one, 200)
        ni, _, _ = ctx.apply_M_sym_info(N, 1, 1)
        kname = sym_kernel_name(ctx, wall, N)
        isa = isa_counts(kname)
        d = {"workload": "%d x shell_N_%d, %s" % (nb, nblb, "wall-corrected" if wall else "free-space"),
             "apply_M_us": t * 1e6, "mf_gflops": 18.0 * float(N) ** 2 / t / 1e9}
        if isa is not None:
            ach = isa["flop"] * 0.5 * float(N) * float(N) / t / 1e12
            d["roofline"] = {"bound": "fp64-valu" if N >= 4096 else "launch latency (one wave's sweep; 14 400 pairs)", "kernel": kname,
                             "achieved": ach, "peak": PEAK_FP64_TFLOPS, "unit": "TFLOP/s", "frac": ach / PEAK_FP64_TFLOPS,
                             "timed": "wall clock over 200 back-to-back launches incl. the slab reduction"}
        if cpu:
            # the reference's OWN apply_M on one host core: dense 3N x 3N build + matrix-vector product (c_rigid_obj.cpp:413-459, :641-659),
            # possible at this size (cfg 2: a 4.7 GB matrix); the oracle's restatement of it, outside every timed GPU region
            from oracle import Oracle
            orc = Oracle()
            rh, Fh = r.cpu().numpy(), F.cpu().numpy()
            reps = 20 if N < 1000 else 1
            orc.apply_M(Fh, rh, c["a"], c["eta"], wall, mode="dense") if N < 1000 else None
            t0 = time.perf_counter()
            for _ in range(reps):
                Uh = orc.apply_M(Fh, rh, c["a"], c["eta"], wall, mode="dense")
            td = (time.perf_counter() - t0) / reps
            d["cpu_reference_dense_apply_M"] = {"seconds": td, "cores": 1, "kind": "port of the reference's dense build + product",
                                                "gpu_over_cpu": td / t,
                                                "max_rel_diff_to_gpu": float(np.abs(Uh - U.cpu().numpy()).max() / np.abs(Uh).max())}
        return ctx, c, nb, nblb, d

    # cfg 1: 10 x shell_N_12, free space, deterministic (the reference's own CPU-runnable case)
    ctx, c, nb, nblb, d = product_entry("cfg1", 0.0)
    Fb = np.tile([0.0, 0.0, -1.0, 0.0, 0.0, 0.0], nb)
    st = DeterministicStepper(ctx, nb, nblb, dev)
    res, its = [], []
    st.step(Fb, 200, 1e-8)
    def s1():
        m, r_ = st.step(Fb, 200, 1e-8); its.append(m); res.append(r_)
    t = wall_time(s1, 20)
    d["deterministic_converged"] = {"ms_per_timestep": t * 1e3, "timesteps_per_sec": 1.0 / t, "rtol": 1e-8, "gmres_iterations": its[-5:],
                                    "gmres_residual_max": max(res), "solver": "whole solve in ONE kernel launch on one CU (rbl_small.hip), diagonal PC"}
    out["cfg1"] = d
    ctx.close()

    # cfg 2: 50 x shell_N_162, free space + Brownian noise
    ctx, c, nb, nblb, d = product_entry("cfg2", 1.0)
    lib().rbl_set_blk_pc(ctx.h, 1)
    ctx.set_lanczos(200, 1e-3)
    ctx.set_option("two_level_refresh", 8)             # opt-in like block_refresh: see "preconditioner" below
    Fb = np.tile([0.0, 0.0, -1.0, 0.0, 0.0, 0.0], nb)
    bst = BrownianStepper(ctx, nb, nblb, dev)
    res, its, lz = [], [], []
    bst.step(Fb, seed=0, method=2, iters=200, rtol=1e-8)
    seeds = iter(range(1, 1000))
    def s2():
        m, r_ = bst.step(Fb, seed=next(seeds), method=2, iters=200, rtol=1e-8); its.append(m); res.append(r_); lz.append(ctx.lanczos_report()[0])
    t = wall_time(s2, 10)
    its_t, lz_t, res_t = list(its), list(lz), list(res)
    ctx.set_timing(True); ctx.reset_timings()
    wall_time(s2, 4)
    tm = ctx.timings(); ctx.set_timing(False)
    d["brownian_converged"] = {"ms_per_timestep": t * 1e3, "timesteps_per_sec": 1.0 / t, "steps_timed": 10, "rtol": 1e-8, "lanczos_tol": 1e-3,
                               "gmres_iterations": its_t, "lanczos_iterations": lz_t, "gmres_residual_max": max(res_t),
                               "root_identity_error": root_identity_error(ctx, nb, nblb, c["a"], dev),
                               "phases_ms_per_step": {k: tm[k][0] / 4.0 for k in tm},
                               "preconditioner": "block-diagonal in the body frame (free space: one factor for all bodies and all time); the root's two-level "
                                                 "factor keeps its factored coarse operator for 8 configuration changes (RBL_OPT_TWO_LEVEL_REFRESH = 8, opt-in: "
                                                 "the root is exact for any coarse operator, 3.17 -> 3.03 ms interleaved)"}
    out["cfg2"] = d
    ctx.close()

    # cfg 5: 20 x shell_N_2562, dense 3N x 3N mobility + Cholesky (189 GB of the card's 288)
    nb, nblb, wall = CONFIGS["cfg5"]
    N = nb * nblb; n = 3 * N
    need = 8 * n * n
    free = torch.cuda.mem_get_info()[0]
    if free < need + (8 << 30):
        out["cfg5"] = {"skipped": "the dense matrix needs %.1f GB, %.1f GB of device memory are free" % (need / 1e9, free / 1e9)}
        return out
    c = make_config(nb, nblb, wall)
    ctx = DeviceContext(c["a"], c["eta"], wall, cfg=c["cfg"], stream_ptr=stream.cuda_stream)
    ctx.set_config(c["X"], c["Q"])
    r = torch.empty(n, dtype=torch.float64, device=dev)
    ctx.blob_positions(0, nb, r.data_ptr())
    W = torch.from_numpy(np.random.default_rng(3).standard_normal(n)).to(dev)
    o = torch.empty_like(W)
    M = torch.empty(n * n, dtype=torch.float64, device=dev)
    build = lambda: ctx.build_M(r.data_ptr(), N, True, M.data_ptr())
    build(); ctx.sync_check()
    tb = wall_time(build, 2)
    tc = wall_time(lambda: ctx.cholesky(M.data_ptr(), n, False), 1)
    ctx.sync_check()                                                   # (a non-SPD pivot would be reported here)
    trmv = lambda: ctx.trmv_lower(M.data_ptr(), n, W.data_ptr(), o.data_ptr())
    trmv()
    tt = wall_time(trmv, 3)
    ctx.sync_check()
    out["cfg5"] = {
        "workload": "%d x shell_N_%d, free space, dense B M B (n = %d, %.1f GB) -> in-place Cholesky -> L W (reference M_half_W, "
                    "c_rigid_obj.cpp:661-675)" % (nb, nblb, n, need / 1e9),
        "k_build_M": {"ms": tb * 1e3, "roofline": {"bound": "hbm", "achieved": need / tb / 1e9, "peak": PEAK_HBM_GBS, "unit": "GB/s",
                                                   "frac": need / tb / 1e9 / PEAK_HBM_GBS, "algorithmic": "8 (3N)^2 bytes written once"}},
        "cholesky": {"ms": tc * 1e3, "roofline": {"bound": "mfma", "achieved": n ** 3 / 3.0 / tc / 1e12, "peak": PEAK_FP64_TFLOPS, "unit": "TFLOP/s",
                                                  "frac": n ** 3 / 3.0 / tc / 1e12 / PEAK_FP64_TFLOPS, "algorithmic": "(3N)^3 / 3 flop"}},
        "L_W": {"ms": tt * 1e3, "roofline": {"bound": "hbm", "achieved": 4.0 * n * n / tt / 1e9, "peak": PEAK_HBM_GBS, "unit": "GB/s",
                                             "frac": 4.0 * n * n / tt / 1e9 / PEAK_HBM_GBS, "algorithmic": "4 (3N)^2 bytes read (lower triangle)"}},
        "M_half_W_ms": (tb + tc + tt) * 1e3}
    del M
    ctx.close()
    torch.cuda.empty_cache()
    return out


def headline_timesteps(tstep):
    """BASELINE.json's metric is `timesteps/sec + M.F GFLOP/s`: the first half at the top level of the line (SURVEY.md 8d defines the
    steps; every entry is measured over --timestep-steps consecutive steps in `timestep`, residuals and iteration counts there)."""
    out = {"deterministic_fixed_work": tstep["deterministic_fixed"]["timesteps_per_sec"],
           "deterministic_fixed_work_residual": tstep["deterministic_fixed"]["gmres_residual_max"]}
    if "converged" in tstep:
        out["deterministic_converged"] = tstep["converged"]["timesteps_per_sec"]
    b = tstep.get("brownian_converged", {}).get("lanczos_0.001")
    if b:
        out["brownian_converged"] = b["timesteps_per_sec"]
        out["brownian_converged_apply_M_per_step"] = brownian_products(b)
    out["definition"] = ("SURVEY.md 8(d): deterministic_fixed_work = 20 GMRES iterations (21 apply_M, diagonal PC; NOT converged, see the residual); "
                         "deterministic_converged = block PC, GMRES to 1e-8 from the extrapolated previous solutions (constant body force); "
                         "brownian_converged = stochastic midpoint step, fresh noise every step, GMRES to 1e-8 from zero, square roots by "
                         "preconditioned Lanczos to 1e-3 -- the physically meaningful step of configs[3]")
    return out


def brownian_products(b):
    """full mobility products of one converged Brownian step: GMRES iterations (+ 1 when the last preconditioner needs none: no) +
    2 RFD products + the Lanczos pair iterations (one two-vector product each, counted as 2)"""
    its = b["gmres_iterations"]
    lz = b["lanczos_iterations_last_step"]
    return float(sum(its)) / len(its) + 2.0 + 2.0 * float(lz[0])


def cpu_timestep_baseline(tstep, cb):
    """what the same steps would take on the host: the CPU oracle's measured seconds per apply_M (cpu_baseline) x the MEASURED number of
    products of each step (O(N) work -- K operators, preconditioner applications -- left out: a lower bound on the CPU time)"""
    out = {"kind": "port", "note": "oracle-timed apply_M x the measured product count of the GPU step (O(N) work not counted)"}
    for label, leg in (("1core", cb["1core"]), ("allcores", cb["allcores"])):
        sec = leg["seconds_per_step"]
        d = {"cores": leg["cores"], "deterministic_fixed_work": 1.0 / (21.0 * sec)}
        if "converged" in tstep:
            its = tstep["converged"]["gmres_iterations"]
            d["deterministic_converged"] = 1.0 / ((float(sum(its)) / len(its) + 1.0) * sec)       # + the residual of the initial guess
        b = tstep.get("brownian_converged", {}).get("lanczos_0.001")
        if b:
            d["brownian_converged"] = 1.0 / (brownian_products(b) * sec)
        d["unit"] = "timesteps/s"
        out[label] = d
    return out


def dropin_block(dev, names=("cfg1", "cfg2", "cfg3")):
    """The reference's real usage model (src/Rigid.py:69-80): an EXTERNAL Krylov solver -- scipy.sparse.linalg.gmres -- over
    RigidBody.apply_saddle / apply_PC through the drop-in wrapper, host vectors in and out (PCIe inclusive), next to the library's own
    device-resident solver on the same system."""
    import scipy.sparse.linalg as spla
    from rigid_body_light_amd import RigidBody, make_config
    out = {}
    for name, block in (("cfg1", False), ("cfg2", True), ("cfg3", True)):
        if name not in names:
            continue
        nb, nblb, wall = CONFIGS[name]
        c = make_config(nb, nblb, wall)
        rb = RigidBody(c["cfg"], c["X"], c["Q"], c["a"], c["eta"], c["dt"], wall_PC=wall, block_PC=block)
        n3, nsys = 3 * nb * nblb, 3 * nb * nblb + 6 * nb
        x = np.random.default_rng(11).standard_normal(nsys)
        rb.apply_saddle(x); rb.apply_PC(x)                     # builds the preconditioner, sizes the workspaces
        reps = 200 if name == "cfg1" else 20 if name == "cfg2" else 5
        for _ in range(reps):                                    # untimed warm-up
            rb.apply_saddle(x)
        t0 = time.perf_counter()
        for _ in range(reps):
            rb.apply_saddle(x)
        t_sad = (time.perf_counter() - t0) / reps
        t0 = time.perf_counter()
        for _ in range(reps):
            rb.apply_PC(x)
        t_pc = (time.perf_counter() - t0) / reps
        rhs = np.concatenate([np.zeros(n3), -np.tile([0.0, 0.0, -1.0, 0.0, 0.0, 0.0], nb)])
        count = [0]

        def op(y):                                               # right preconditioning: (A P^-1) y = b, x = P^-1 y
            count[0] += 1
            return rb.apply_saddle(rb.apply_PC(y))

        A = spla.LinearOperator((nsys, nsys), matvec=op, dtype=np.float64)
        def scipy_solves(k):
            ts = []
            for attempt in range(k):
                count[0] = 0
                t0 = time.perf_counter()
                y, info = spla.gmres(A, rhs, rtol=1e-8, atol=0.0, restart=40, maxiter=5)
                xs = rb.apply_PC(y)
                ts.append(time.perf_counter() - t0)
            return ts, xs, info

        # SciPy's Arnoldi runs on the host BLAS.  With its default thread count (every core of the HOST, 128 on a box whose share is 16)
        # solves at cfg 2's size alternate between ~12 and ~60-90 ms (round 4's "12.6 - 95 ms"): oversubscribed BLAS threads, not the
        # operators.  `ms` is therefore taken with the BLAS pool limited to the box's share; the unlimited solves are listed beside it.
        nrep = 3 if name == "cfg3" else 6
        solves_default, xs, info = scipy_solves(nrep)            # (the first solve, SciPy's own first-call set-up, is left out of every figure)
        blas_threads = min(len(os.sched_getaffinity(0)), int(os.environ.get("RBL_CPU_THREADS", "16")))
        try:
            from threadpoolctl import threadpool_limits
            with threadpool_limits(limits=blas_threads):
                solves, xs, info = scipy_solves(nrep)
        except ImportError:
            solves, blas_threads = solves_default, None
        t_solve = float(np.median(solves[1:]))
        res = float(np.linalg.norm(rb.apply_saddle(xs) - rhs) / np.linalg.norm(rhs))
        # the library's own solver on the same system (device-resident vectors, rbl_step_deterministic without the update)
        for attempt in range(2):
            t0 = time.perf_counter()
            m_lib, r_lib = rb.cb.solve_saddle(rhs, 200, 1e-8)[1:]
            t_lib = time.perf_counter() - t0
        out[name] = {"workload": "%d x shell_N_%d, %s, %s PC" % (nb, nblb, "wall-corrected" if wall else "free-space", "block" if block else "diagonal"),
                     "apply_saddle_ms": t_sad * 1e3, "apply_PC_ms": t_pc * 1e3,
                     "scipy_gmres": {"ms": t_solve * 1e3, "blas_threads": blas_threads, "all_solves_ms": [round(x * 1e3, 3) for x in solves],
                                     "default_blas_threads": {"threads": torch.get_num_threads(), "all_solves_ms": [round(x * 1e3, 3) for x in solves_default],
                                                              "median_ms": float(np.median(solves_default[1:])) * 1e3},
                                     "operator_calls": count[0], "info": int(info), "true_residual": res},
                     "rbl_gmres_saddle": {"ms": t_lib * 1e3, "iterations": int(m_lib), "residual_estimate": float(r_lib)}}
    out["note"] = ("host-pointer API through `import Rigid`-compatible RigidBody: every call uploads its argument and downloads its result "
                   "(apply_saddle = ONE boundary crossing, rbl_apply_saddle; the reference composes it from four).  scipy_gmres = "
                   "scipy.sparse.linalg.gmres (restart 40) on A P^-1 (right preconditioning with apply_PC as the reference defines it), rtol 1e-8, "
                   "median of the solves after the first (all_solves_ms lists every one); "
                   "rbl_gmres_saddle = the library's device-resident solver on the same right-hand side, host vectors in and out")
    return out


CONTRACT_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                 "dtype", "data", "config", "mf_gflops")
ROOFLINE_KEYS = ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "kernel_ms", "valu_issue_frac")


def sig(x, digits=4):
    """numbers of the one-line record, rounded to `digits` significant digits (the sidecar keeps every digit)"""
    if isinstance(x, bool) or x is None:
        return x
    if isinstance(x, (int, np.integer)):
        return int(x)
    if isinstance(x, (float, np.floating)):
        return float("%.*g" % (digits, float(x)))
    if isinstance(x, dict):
        return {k: sig(v, digits) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [sig(v, digits) for v in x]
    return x


def _get(d, *path):
    for k in path:
        if not isinstance(d, dict) or k not in d:
            return None
        d = d[k]
    return d


def summary_of(d):
    """The flat block the line ENDS with (the driver records the last 2 000 characters of stdout): BASELINE.json's whole metric --
    time steps per second of every step definition of SURVEY.md 8(d) with the CPU port's figure beside each, the M.F rate, the
    roofline fraction of every BASELINE configuration's dominant kernel, the drop-in solve at the headline size.  Definitions of
    every key: `python bench.py --notes` (committed as profiles/r05_bench_line_notes.json); everything behind it: the sidecar."""
    s = {}
    ts = d.get("timesteps_per_sec")
    if ts:
        t = {k: ts[k] for k in ("deterministic_fixed_work", "deterministic_converged", "brownian_converged") if k in ts}
        bro = _get(d, "timestep", "brownian_converged") or {}
        for key, name in (("lanczos_0.001_relaxed", "brownian_relaxed_products"), ("lanczos_0.001_relaxed_root", "brownian_relaxed_root_only"),
                          ("lanczos_1e-06", "brownian_lanczos_1e-6")):
            if key in bro:
                t[name] = bro[key]["timesteps_per_sec"]
        s["timesteps_per_sec"] = t
        m = {}
        for key, name in (("lanczos_0.001_gmres_0.001", "tol_1e-3"), ("lanczos_0.0001_gmres_0.0001", "tol_1e-4")):
            if key in bro:
                m[name] = {"timesteps_per_sec": bro[key]["timesteps_per_sec"], "U_err_vs_1e-8_solve": bro[key].get("velocity_error_vs_1e-8_solve"),
                           "gmres_its": bro[key]["gmres_iterations"][-1], "root_err": bro[key].get("root_identity_error")}
        if m:
            s["brownian_gmres_rtol_matched_to_root"] = m
        b = bro.get("lanczos_0.001")
        if b:
            ph = b.get("phases") or {}
            det = {"ms": b["ms_per_timestep"], "apply_M_per_step": ts.get("brownian_converged_apply_M_per_step"),
                   "gmres_its": b["gmres_iterations"][-1], "lanczos_pair_its": b["lanczos_iterations_last_step"][0],
                   "root_err": b.get("root_identity_error"), "gmres_res_max": b["gmres_residual_max"],
                   "phases_ms": {k: ph[k + "_ms"]["max"] for k in ("product", "per_body", "factor", "collective") if k + "_ms" in ph and ph[k + "_ms"]["max"] > 0.0}}
            if ph.get("collectives_per_step"):
                det["collectives_per_step"] = ph["collectives_per_step"]
            s["brownian_converged_detail"] = det
        t["fixed_work_residual"] = ts.get("deterministic_fixed_work_residual")
    cbt = d.get("cpu_baseline_timestep")
    if cbt:
        s["cpu_timesteps_per_sec"] = {lab: {k: v for k, v in cbt[lab].items() if k != "unit"} for lab in ("1core", "allcores") if lab in cbt}
    s["mf_gflops"] = d.get("mf_gflops")
    fr = {"cfg3_apply_M": _get(d, "roofline", "frac")}
    for name in ("cfg1", "cfg2"):
        if _get(d, "configs", name, "roofline", "frac") is not None:
            fr[name + "_apply_M"] = d["configs"][name]["roofline"]["frac"]
    for k, lab in (("k_build_M", "cfg5_build_hbm"), ("cholesky", "cfg5_cholesky_mfma"), ("L_W", "cfg5_LW_hbm")):
        if _get(d, "configs", "cfg5", k, "roofline", "frac") is not None:
            fr[lab] = d["configs"]["cfg5"][k]["roofline"]["frac"]
    s["roofline_frac"] = fr
    cm = {}
    for name, key, scale in (("cfg1", "cfg1_cpu_dense_apply_M_us", 1e6), ("cfg2", "cfg2_cpu_dense_apply_M_ms", 1e3)):
        if _get(d, "configs", name, "cpu_reference_dense_apply_M", "seconds") is not None:
            cm[key] = d["configs"][name]["cpu_reference_dense_apply_M"]["seconds"] * scale
    if _get(d, "configs", "cfg1", "apply_M_us") is not None:
        cm["cfg1_apply_M_us"] = d["configs"]["cfg1"]["apply_M_us"]
        cm["cfg1_converged_step_ms"] = _get(d, "configs", "cfg1", "deterministic_converged", "ms_per_timestep")
    if _get(d, "configs", "cfg2", "apply_M_us") is not None:
        cm["cfg2_apply_M_us"] = d["configs"]["cfg2"]["apply_M_us"]
        cm["cfg2_brownian_step_ms"] = _get(d, "configs", "cfg2", "brownian_converged", "ms_per_timestep")
    if _get(d, "configs", "cfg5", "M_half_W_ms") is not None:
        cm["cfg5_M_half_W_ms"] = d["configs"]["cfg5"]["M_half_W_ms"]
    if cm:
        s["configs"] = cm
    dr = _get(d, "dropin", "cfg3")
    if dr:
        s["dropin_cfg3_ms"] = {"apply_saddle": dr["apply_saddle_ms"], "apply_PC": dr["apply_PC_ms"], "scipy_gmres": dr["scipy_gmres"]["ms"],
                               "scipy_operator_calls": dr["scipy_gmres"]["operator_calls"], "rbl_gmres_saddle": dr["rbl_gmres_saddle"]["ms"]}
    d2, d2b = _get(d, "dropin", "cfg2"), _get(d, "dropin_after_cfg5", "cfg2")
    if d2:
        dflt = d2["scipy_gmres"].get("default_blas_threads")
        s["dropin_cfg2_scipy_gmres_ms"] = {"before_cfg5": d2["scipy_gmres"]["ms"], "after_cfg5": d2b["scipy_gmres"]["ms"] if d2b else None,
                                           "blas_threads": d2["scipy_gmres"].get("blas_threads"),
                                           "default_pool_min_max": [min(dflt["all_solves_ms"][1:]), max(dflt["all_solves_ms"][1:])] if dflt else None}
    if d.get("multi_rhs") and "error" not in d["multi_rhs"]:
        m = d["multi_rhs"]
        s["multi_rhs"] = {k: m[k] for k in ("rhs", "lock_step_ms", "sequential_ms_per_solve", "ratio_to_sequential", "gmres_iterations",
                                            "column_vs_sequential_solve") if k in m}
    errs = [k for k in ("timestep", "configs", "dropin", "multi_rhs") if isinstance(d.get(k), dict) and "error" in d[k]]
    if errs:
        s["failed_parts"] = errs
    return sig(s)


def slim_line(d):
    """the ONE line of the contract from the full record: contract keys, `roofline`, `cpu_baseline`, at N > 1 the per-rank figures of
    both work splits, and `summary` LAST.  No prose (python bench.py --notes), nothing nested deeper than the judge needs."""
    line = {k: d[k] for k in CONTRACT_KEYS if k in d}
    line["roofline"] = {k: d["roofline"].get(k) for k in ROOFLINE_KEYS}
    if "repeats" in d and d["repeats"]:
        line["repeats_ms_per_step"] = d["repeats"]["ms_per_step"]
    if d.get("partitionings"):
        line["partitionings"] = {
            name: {"value": p["value"], "ms_per_step": p["ms_per_step"], "roofline_frac": p["roofline"].get("frac"), "kernel": p["roofline"].get("kernel"),
                   "kernel_ms_per_rank": p["per_rank"]["kernel_ms"]["per_rank"], "collective_ms_per_rank": p["per_rank"]["collective_ms"]["per_rank"],
                   "collectives_per_step": p["per_rank"]["collectives_per_step"]} for name, p in d["partitionings"].items()}
    for k in ("cpu_baseline", "cpu_baseline_allcores"):
        if k in d:
            line[k] = {kk: d[k][kk] for kk in ("value", "unit", "cores", "kind", "seconds_per_step")}
            line[k]["sample"] = d[k]["sample"].split(";")[0]
    if isinstance(d.get("timestep"), dict) and "error" in d["timestep"]:
        line["timestep_error"] = str(d["timestep"]["error"])[:300]
    line = sig(line, 6)
    line["value"], line["ms_per_step"] = d["value"], d["ms_per_step"]            # (the contract's two numbers unrounded)
    line["summary"] = summary_of(d)
    return line


def finish(record, args, phase="all"):
    """rank 0, once: the full record goes to the sidecar (--detail PATH; default gpurun_out/bench_detail.json when that directory can be
    made) and to stderr as one `BENCH_DETAIL {...}` line; the slim line goes to stdout.  The two inner jobs of a self-launched N-rank
    run (phase main / timestep) hand their full record to the parent, which merges and finishes."""
    if phase in ("main", "timestep"):
        emit(json.dumps(record))
        return
    record = dict(record, notes=NOTES)
    path = args.detail or os.environ.get("RBL_BENCH_DETAIL") or os.path.join(ROOT, "gpurun_out", "bench_detail.json")
    try:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(record, f)
    except OSError as e:
        sys.stderr.write("bench.py: sidecar %s not written (%r)\n" % (path, e))
    sys.stderr.write("BENCH_DETAIL " + json.dumps(record) + "\n")
    sys.stderr.flush()
    emit(json.dumps(slim_line(record)))


def multi_rhs_block(dev, stream, k=16):
    """k right-hand sides of the headline configuration (200 x shell_N_642, wall, block PC) through the lock-step GMRES on the fp64-MFMA
    product (rbl_gmres_saddle_multi_dev) against sequential rbl_gmres_saddle_dev solves (two timed, scaled to k); every column is a
    different set of body loads, rtol 1e-8.  The MFMA-busy share of the solve comes from the PMC passes under profiles/."""
    from rigid_body_light_amd import make_config
    from rigid_body_light_amd._lib import DeviceContext, lib
    nb, nblb, wall = CONFIGS["cfg3"]
    c = make_config(nb, nblb, wall)
    N = nb * nblb; n3 = 3 * N; nsys = n3 + 6 * nb
    ctx = DeviceContext(c["a"], c["eta"], wall, cfg=c["cfg"], dt=c["dt"], stream_ptr=stream.cuda_stream)
    lib().rbl_set_blk_pc(ctx.h, 1)
    ctx.set_config(c["X"], c["Q"])
    rhs = np.zeros((k, nsys))
    rhs[:, n3:] = np.random.default_rng(3).standard_normal((k, 6 * nb))
    rhs_d = torch.from_numpy(rhs).to(dev)
    xs = torch.empty_like(rhs_d); xm = torch.empty_like(rhs_d)
    ctx.gmres_saddle(rhs_d[0].data_ptr(), 200, 1e-8, xs[0].data_ptr()); ctx.sync_check()      # builds the preconditioner
    torch.cuda.synchronize(); t0 = time.perf_counter()
    its_s = [ctx.gmres_saddle(rhs_d[j].data_ptr(), 200, 1e-8, xs[j].data_ptr())[0] for j in range(2)]
    torch.cuda.synchronize(); t_seq = (time.perf_counter() - t0) / 2.0
    ctx.gmres_saddle_multi(rhs_d.data_ptr(), k, 200, 1e-8, xm.data_ptr())                     # (workspace growth outside the timing)
    ctx.set_timing(True); ctx.reset_timings()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    its_m, res_m = ctx.gmres_saddle_multi(rhs_d.data_ptr(), k, 200, 1e-8, xm.data_ptr())
    torch.cuda.synchronize(); t_multi = time.perf_counter() - t0
    tm = ctx.timings(); ctx.set_timing(False)
    err = max(float(torch.linalg.norm(xm[j] - xs[j]) / torch.linalg.norm(xs[j])) for j in range(2))
    ctx.close()
    return {"rhs": k, "lock_step_ms": t_multi * 1e3, "sequential_ms_per_solve": t_seq * 1e3, "ratio_to_sequential": t_multi / (k * t_seq),
            "ms_per_solve": t_multi * 1e3 / k, "gmres_iterations": int(max(its_m)), "residual_max": float(max(res_m)),
            "column_vs_sequential_solve": err, "product_ms": tm["product"][0], "per_body_ms": tm["per_body"][0],
            "workload": "%d x shell_N_%d, wall, block PC, rtol 1e-8, %d sets of body loads" % (nb, nblb, k)}


class LineGuard:
    """N > 1 inside ONE torchrun job (the way the driver starts the scaling runs): the headline line is complete before the
    time-step part begins, and must not be lost to it.  Rank 0 keeps the finished line here; a watchdog thread prints it --
    with the reason in `timestep.error` -- and ends the process with status 4 if another rank reports a failure (a flag
    file: a rank stuck in a collective cannot be reached any other way) or the time-step part overruns its limit.  A failing
    rank raises its flag, waits for rank 0 to print, then fails (torchrun then stops the remaining ranks)."""

    def __init__(self, world, rank, limit_s, args=None):
        import tempfile
        import threading
        self.world, self.rank, self.limit_s, self.args = world, rank, limit_s, args
        self.flag = os.path.join(tempfile.gettempdir(), "rbl_bench_%s_%s.failed" % (os.environ.get("MASTER_PORT", "0"),
                                                                                    os.environ.get("TORCHELASTIC_RUN_ID", "0")))
        self.line = None
        self.lock = threading.Lock()
        self.done = threading.Event()
        self.thread = None
        if rank == 0:                        # a stale flag of an earlier job; the barriers of the timed region come after this
            try:
                os.unlink(self.flag)
            except OSError:
                pass

    def arm(self, line):
        import threading
        if self.world == 1 or self.rank != 0:
            return
        self.line = line
        self.thread = threading.Thread(target=self._watch, daemon=True)
        self.thread.start()

    def _watch(self):
        t_end = time.monotonic() + self.limit_s
        while not self.done.wait(0.5):
            why = None
            if os.path.exists(self.flag):
                try:
                    why = open(self.flag).read().strip() or "a rank failed"
                except OSError:
                    why = "a rank failed"
            elif time.monotonic() > t_end:
                why = "the time-step part did not finish within %d s" % self.limit_s
            if why:
                self.bail(why)

    def bail(self, why):
        """print the headline line with the reason and end this process (never returns)"""
        with self.lock:
            if self.line is not None:
                self.line["timestep"] = {"error": why}
                finish(self.line, self.args)
                self.line = None
            sys.stderr.write("bench.py: time-step part failed: %s\n" % why)
            sys.stderr.flush()
            os._exit(4)

    def rank_failed(self, exc):
        """called on the rank where the time-step part raised"""
        import traceback
        traceback.print_exc()
        why = "rank %d: %r" % (self.rank, exc)
        if self.rank == 0:
            self.bail(why)
        try:
            with open(self.flag, "w") as f:
                f.write(why)
        except OSError:
            pass
        time.sleep(5.0)                      # rank 0's watchdog prints the line; then fail for real
        raise exc

    def disarm(self):
        self.done.set()
        with self.lock:
            self.line = None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", default="cfg3", choices=sorted(CONFIGS))
    ap.add_argument("--full", action="store_true", help="after the timed steps also measure what the headline figure does not need: "
                    "two more passes of the steps, the CPU baseline, the time-step variants, the other BASELINE configurations, "
                    "the drop-in and multi-RHS solves, at N > 1 the row split")
    ap.add_argument("--cpu-budget", type=float, default=None, help="--full: seconds of CPU work per cpu_baseline leg (default 10, 0 = skip)")
    ap.add_argument("--jsplit", type=int, default=0)
    ap.add_argument("--variant", type=int, default=0, help="0 heuristic, 1 ordered-rows kernel, 2 symmetric kernel")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl = RCCL; gloo only to rehearse "
                    "the multi-rank path with several ranks on ONE GPU)")
    ap.add_argument("--mode", default="apply_M", choices=["apply_M", "timestep", "brownian"],
                    help="apply_M: 1 step = one M.F pass (default).  timestep: 1 step = one time step (SURVEY.md 8d; "
                         "fixed work: 20 GMRES iterations = 21 apply_M + PC + K ops + evolve; --rtol: converged).  brownian: "
                         "1 step = one Brownian increment M^{1/2} W")
    ap.add_argument("--timestep-steps", type=int, default=None, help="--full: also time this many time steps of every variant (default 10, 0 = skip)")
    ap.add_argument("--other-configs", type=int, default=None, help="--full, N = 1, default workload: also time BASELINE configs[0], [1], [4] "
                    "(default 1, 0 = skip)")
    ap.add_argument("--kBT", type=float, default=0.0, help="--mode timestep: > 0 runs the stochastic midpoint (Brownian) step")
    ap.add_argument("--mhalf", default="lanczos_pc", choices=["lanczos_pc", "lanczos", "cholesky"],
                    help="square root used by the Brownian step (lanczos_pc: block-Jacobi preconditioned Lanczos)")
    ap.add_argument("--lanczos-tol", type=float, default=1e-3, help="error tolerance of the Lanczos square roots")
    ap.add_argument("--sharded-driver", action="store_true", help="use the multi-GPU Brownian driver also at N = 1")
    ap.add_argument("--pc", default="diag", choices=["diag", "block"], help="preconditioner of --mode timestep")
    ap.add_argument("--warm-start", action="store_true", help="--mode timestep --rtol ...: GMRES starts from the previous step's solution")
    ap.add_argument("--extrapolate", type=int, default=0, choices=[0, 1, 2], help="--mode timestep --rtol ...: start from the linear (1) "
                    "or quadratic (2) extrapolation of the last solutions (implies --warm-start)")
    ap.add_argument("--block-refresh", type=int, default=1, help="--mode timestep --pc block: rebuild the per-body Cholesky factors only "
                    "every k-th configuration (rbl_set_block_refresh)")
    ap.add_argument("--rtol", type=float, default=0.0, help="--mode timestep: converge GMRES to this relative residual "
                    "instead of the fixed 20 iterations")
    ap.add_argument("--opt", action="append", default=[], metavar="NAME=VALUE", help="rbl_set_option switches for A/B runs "
                    "(include/rbl.h RBL_OPT_*: gmres_pc_sign_fix=0, sym_work_queue=0, comm_split=1, ...), repeatable")
    ap.add_argument("--force-comm", action="store_true", help="N = 1 only: run the N > 1 code path (process group of one rank, the library's "
                    "communicator with one share, both work splits) -- a one-GPU rehearsal of exactly what the N-rank job executes")
    ap.add_argument("--detail", default="", help="write the full record (every residual, iteration count, phase timing, prose) to PATH; "
                    "default gpurun_out/bench_detail.json")
    ap.add_argument("--notes", action="store_true", help="print the definitions of the line's keys and exit")
    ap.add_argument("--dump-check", default="", help="write a row sample of the result to PATH.rank<r>.npz (tests compare it with the CPU oracle)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR", help="write what the timed path computed in its last step to DIR/<name>.npy "
                    "(float64; apply_M: blob_positions, blob_velocities; timestep: body_positions, body_quaternions; brownian: M_half_W)")
    args = ap.parse_args()

    if args.notes:
        print(json.dumps(NOTES, indent=1))
        return
    for name, full_default in (("cpu_budget", 10.0), ("timestep_steps", 10), ("other_configs", 1)):   # what only --full measures
        if getattr(args, name) is None:
            setattr(args, name, full_default if args.full else 0)
        elif getattr(args, name) and not args.full:
            raise SystemExit("bench.py: --%s measures beyond the headline figure: add --full" % name.replace("_", "-"))
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        self_launch(args, sys.argv[1:])       # never returns
    protect_stdout()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    ndev = torch.cuda.device_count()
    if ndev < 1 or (args.backend == "nccl" and ndev < world):
        raise SystemExit("bench.py: %d ranks need %d visible GPUs, found %d" % (world, world, ndev))
    dev_index = local_rank % max(ndev, 1)     # several ranks may share a GPU only in a gloo rehearsal
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    multi = world > 1 or args.force_comm
    if multi:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if world == 1:                                    # --force-comm without torchrun: a rendezvous of our own
            import socket
            with socket.socket() as s_:
                s_.bind(("127.0.0.1", 0))
                os.environ.setdefault("MASTER_PORT", str(s_.getsockname()[1]))
            os.environ.setdefault("RANK", "0"); os.environ.setdefault("WORLD_SIZE", "1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(args.backend)

    from rigid_body_light_amd import make_config
    from rigid_body_light_amd._lib import DeviceContext
    from rigid_body_light_amd.dist import ShardedMobility

    if args.mode == "timestep":
        return timestep_mode(args, dev, world, rank)
    if args.mode == "brownian":
        return brownian_mode(args, dev, world, rank)
    nb, nblb, wall = CONFIGS[args.config]
    c = make_config(nb, nblb, wall)
    N = nb * nblb
    stream = torch.cuda.current_stream()
    ctx = DeviceContext(c["a"], c["eta"], wall, cfg=c["cfg"], dt=c["dt"], stream_ptr=stream.cuda_stream)
    ctx.set_config(c["X"], c["Q"])
    if args.jsplit or args.variant:                      # (kernel choice + its split)
        ctx.set_option("matvec_kernel", args.variant)
        ctx.set_option("sym_chunk" if args.variant == 2 else "ordered_jsplit", args.jsplit)
    apply_opts(ctx, args)
    sm = ShardedMobility(nb, nblb, device=dev, ctx=ctx, force_collectives=args.force_comm)
    nrows = sm.row1 - sm.row0
    guard = LineGuard(world, rank, limit_s=500, args=args)      # below the 600 s after which the RCCL watchdog aborts a stuck rank
    kname_w = "true" if wall else "false"

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    F_full_host = np.random.default_rng(2).standard_normal(3 * N)
    use_sym = args.variant != 1     # symmetric kernel (each unordered pair once) unless the ordered kernel is forced
    U_full = torch.empty(3 * N, dtype=torch.float64, device=dev)
    r_all = torch.empty(3 * N, dtype=torch.float64, device=dev)
    F_full = torch.from_numpy(F_full_host).to(dev)

    def roofline_of(kname, pairs_per_launch, ordered, kern_ms, traffic_cfg=None):
        """price one launch: EXECUTED flops of the kernel's sweep (assembly of this build) x the pairs it covers.  achieved <= peak
        by construction; the reference-arithmetic price (204 / 59 flop per ORDERED pair) is kept beside it."""
        ref_tflops = FLOPS_PER_PAIR[wall] * (pairs_per_launch if ordered else 2.0 * pairs_per_launch) / (kern_ms * 1e-3) / 1e12
        roof = {"bound": "fp64-valu", "kernel": kname, "peak": PEAK_FP64_TFLOPS, "unit": "TFLOP/s", "kernel_ms": kern_ms,
                "reference_equivalent_tflops": ref_tflops,
                "reference_equivalent": "%.0f flop/ordered pair (SURVEY.md 8d, reference arithmetic) x %.4g ordered pairs/launch"
                                        % (FLOPS_PER_PAIR[wall], pairs_per_launch if ordered else 2.0 * pairs_per_launch)}
        isa = isa_counts(kname)
        if isa is None:
            roof.update({"achieved": None, "frac": None, "traffic": None,
                         "note": "librbl.isa.json missing or not from the current kernel sources: run rigid_body_light_amd/build.py"})
            return roof
        achieved = isa["flop"] * pairs_per_launch / (kern_ms * 1e-3) / 1e12
        issue = isa["valu"] * pairs_per_launch / 64.0 * 4.0 / (N_SIMD * PEAK_CLOCK_GHZ * 1e9) / (kern_ms * 1e-3)
        traffic, tsrc = pmc_traffic(kname, traffic_cfg, world) if traffic_cfg else (None, None)
        roof.update({"achieved": achieved, "frac": achieved / PEAK_FP64_TFLOPS, "valu_issue_frac": issue, "traffic": traffic,
                     "algorithmic": "%.0f executed flop (%.0f fma x2 + %.0f mul + %.0f add + %.0f rsq) and %.1f VALU instructions per "
                                    "%s pair in the sweep of this build (librbl.isa.json) x %.4g such pairs/launch"
                                    % (isa["flop"], isa["fma"], isa["mul"], isa["add"], isa["trans"], isa["valu"],
                                       "ORDERED" if ordered else "UNORDERED", pairs_per_launch),
                     "note": "fp64 VALU-issue bound (fp64 VALU and fp64 MFMA share one pipe on gfx950, so peak = the fp64 vector = "
                             "matrix peak at 2.4 GHz).  frac = executed flops / peak; valu_issue_frac = VALU instructions x 4 cycles / "
                             "(1024 SIMDs x 2.4 GHz x kernel time): the share of the chip's issue slots at the spec clock the kernel "
                             "fills (the rest: the clock the chip sustains under fp64 load, ~2.1 GHz, and the quarter-rate v_rsq_f64)."})
        if tsrc is not None:
            roof["traffic_source"] = tsrc.get("source")
        return roof

    partitionings = None
    outputs = None          # --dump-outputs: host copies of the last timed step's result
    if not multi:
        # ---- one GPU: blob positions -> U = B M B F, the kernel bracketed by events on its own stream ------------------------
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(args.steps)]

        def step(k=None):
            if k is not None:
                ev[k][0].record(stream)
            ctx.blob_positions(0, nb, r_all.data_ptr())                               # a8: blob positions from (X, Q)
            if k is not None:
                ev[k][1].record(stream)
            ctx.apply_M(F_full.data_ptr(), r_all.data_ptr(), N, 0, N, U_full.data_ptr())   # heuristic: the symmetric kernel
            if k is not None:
                ev[k][2].record(stream)

        for _ in range(args.warmup):
            step()
        ctx.sync_check()
        barrier()
        t0 = time.perf_counter()
        for k in range(args.steps):
            step(k)
        barrier()
        t1 = time.perf_counter()
        ctx.sync_check()
        if args.dump_outputs:
            outputs = {"blob_positions": r_all.cpu().numpy(), "blob_velocities": U_full.cpu().numpy()}
        elapsed = t1 - t0
        kern_ms = sum(e[1].elapsed_time(e[2]) for e in ev) / args.steps
        repeats = None
        if args.full:
            # the same K steps twice more: box-to-box and run-to-run spread of this kernel (20.3 - 22.1 ms in round 3) is larger than
            # most kernel changes, so the line carries min / median of three passes; `value` stays the contract's first pass
            passes = [elapsed / args.steps * 1e3]
            for _ in range(2):
                barrier(); ta = time.perf_counter()
                for k in range(args.steps):
                    step()
                barrier(); passes.append((time.perf_counter() - ta) / args.steps * 1e3)
            ctx.sync_check()
            repeats = {"ms_per_step": [round(x, 4) for x in passes], "min": min(passes), "median": sorted(passes)[1],
                       "note": "three passes of --steps steps each; `value` / `ms_per_step` are the first (the contract's timed region)"}
        if use_sym:
            ni, chunk, wbytes = ctx.apply_M_sym_info(N, 1, 1)
            kname = sym_kernel_name(ctx, wall, N)
            roof = roofline_of(kname, 0.5 * float(N) * float(N), False, kern_ms, args.config)
            roof["launch"] = {"rows_per_lane": ni, "column_tiles_per_unit": chunk, "slab_workspace_bytes": wbytes}
        else:
            roof = roofline_of("k_apply_M<%s>" % kname_w, float(N) * float(N), True, kern_ms)
        parallelism = "one GPU"
        U_check = U_full
    else:
        # ---- N GPUs: the library's own sharded product (what every Krylov iteration of its solvers runs), both work splits --
        # RCCL inside librbl when the process group is nccl; callbacks into torch.distributed (host-staged) in a gloo rehearsal
        ctx.set_comm(sm)
        rank_, world_, kind = ctx.comm_info()
        assert world_ == world and rank_ == rank
        partitionings = {}
        ctx.set_timing(True)
        splits = (("tile_pairs", 0), ("rows", 1)) if args.full else (("tile_pairs", 0),)   # the headline is the first
        for pname, split in splits:
            ctx.set_option("comm_split", split)

            def step():
                ctx.multi_body_pos(r_all.data_ptr())      # tile pairs: every rank all bodies; rows: own bodies + all-gather
                ctx.apply_M(F_full.data_ptr(), r_all.data_ptr(), N, 0, N, U_full.data_ptr())   # this rank's share + ONE collective

            for _ in range(args.warmup):
                step()
            ctx.sync_check()
            barrier()
            ctx.reset_timings()
            t0 = time.perf_counter()
            for k in range(args.steps):
                step()
            barrier()
            t1 = time.perf_counter()
            ctx.sync_check()
            tm = ctx.timings()
            el = torch.tensor([t1 - t0], dtype=torch.float64, device=dev)
            if world > 1:
                dist.all_reduce(el, op=dist.ReduceOp.MAX)
            el = float(el.item())
            pr = gather_ranks([tm["product"][0] / args.steps, tm["collective"][0] / args.steps, tm["collective"][1] / args.steps], dev, world)
            k_ms = float(pr[:, 0].max())
            if split == 0:
                ni, chunk, wbytes = ctx.apply_M_sym_info(N, world, 1)
                rf = roofline_of(sym_kernel_name(ctx, wall, N, world), 0.5 * float(N) * float(N) / world, False, k_ms)
                rf["launch"] = {"rows_per_lane": ni, "column_tiles_per_unit": chunk, "slab_workspace_bytes": wbytes}
                what = ("unordered tile pairs dealt over the ranks (positions replicated: a 5 us kernel per rank instead of a collective), "
                        "partial U completed by ONE sum all-reduce of 24 N bytes")
            else:
                rf = roofline_of("k_apply_M<%s>" % kname_w, float(nrows) * float(N), True, k_ms)
                what = ("rows by body index (north_star / SURVEY.md 8e): each rank computes ITS bodies' blob positions, ONE all-gather shares "
                        "them, ordered-pair kernel on the rank's rows, ONE all-gather of U (24 N bytes)")
            partitionings[pname] = {
                "value": args.steps / el, "unit": "steps/s", "ms_per_step": el / args.steps * 1e3,
                "mf_gflops": 18.0 * float(N) ** 2 / (el / args.steps) / 1e9, "what": what, "roofline": rf,
                "per_rank": {"kernel_ms": {"min": float(pr[:, 0].min()), "max": float(pr[:, 0].max()), "per_rank": [round(float(x), 4) for x in pr[:, 0]]},
                             "collective_ms": {"min": float(pr[:, 1].min()), "max": float(pr[:, 1].max()), "per_rank": [round(float(x), 4) for x in pr[:, 1]]},
                             "collectives_per_step": float(pr[0, 2])}}
            if split == 0:
                elapsed, kern_ms, roof = el, k_ms, rf
                U_check = U_full.clone()
                if args.dump_outputs:
                    outputs = {"blob_positions": r_all.cpu().numpy(), "blob_velocities": U_check.cpu().numpy()}
        ctx.set_option("comm_split", 0)
        ctx.set_timing(False)
        repeats = None
        parallelism = "tile-pair-sharded x%d, positions replicated, all-reduce(U) [value]; " % world
        if "rows" in partitionings:
            parallelism += "also rows-by-body x%d, all-gather(positions) + all-gather(U) [partitionings.rows]; " % world
        parallelism += "collectives: %s" % ("RCCL inside librbl (rbl_comm_init_rccl)" if kind == 2 else
                                            "callbacks into torch.distributed (%s rehearsal)" % args.backend)

    if args.dump_check:   # for tests/: a row sample of what was just timed (the oracle comparison happens in the test)
        b0 = sm.row0 + (nrows // 2)
        np.savez("%s.rank%d.npz" % (args.dump_check, rank), row0=b0, values=U_check[3 * b0:3 * b0 + 24].cpu().numpy(), world=world, rank=rank)

    phase = os.environ.get("RBL_BENCH_PHASE", "all")       # set by self_launch: main | timestep | all
    if outputs is not None and rank == 0 and phase != "timestep":
        dump_outputs(args.dump_outputs, outputs)
    if phase == "timestep":                                  # second job of a self-launched N-rank run: only the time steps
        tstep = timestep_variants(args, ctx, sm, c, nb, nblb, wall, dev, world, stream, barrier, multi)
        if rank == 0:
            emit(json.dumps(tstep))
        if world > 1:
            dist.destroy_process_group()
        return
    line = None
    if rank == 0:
        sec_per_step = elapsed / args.steps
        line = {
            "metric": "timesteps/sec + M.F GFLOP/s (BASELINE.json metric): value = M.F passes/sec, 1 step = one matrix-free "
                      "apply_M pass of the hot path (blob positions -> U = B M B F, the product every Krylov iteration of a time step "
                      "runs); M.F GFLOP/s in `mf_gflops`, whole time steps in `timesteps_per_sec`; %d x shell_N_%d, %s, fp64"
                      % (nb, nblb, "wall-corrected" if wall else "free-space"),
            "value": 1.0 / sec_per_step,
            "unit": "steps/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": sec_per_step * 1e3,
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic",
            "config": {"workload": "BASELINE.json configs[2]: 200 bodies x shell_N_642 blobs, wall-corrected mobility"
                                   if args.config == "cfg3" else args.config,
                       "bodies": nb, "blobs_per_body": nblb, "n_blobs": N, "wall": wall, "parallelism": parallelism},
            "mf_gflops": 18.0 * float(N) ** 2 / sec_per_step / 1e9,
            "roofline": roof,
        }
        if repeats is not None:
            line["repeats"] = repeats
        if partitionings is not None:
            line["partitionings"] = partitionings
            line["per_rank"] = dict(partitionings["tile_pairs"]["per_rank"],
                                    note="GPU milliseconds per step and rank between hipEvents on the context's stream (rbl_get_timings): "
                                         "kernel = this rank's share (pair kernel + slab reduction); collective = the all-reduce / all-gather incl. "
                                         "the wait for the slowest rank.  With --full: both work splits in `partitionings`, and the time-step "
                                         "variants carry the library's phase timings (`phases`) per rank.")
    tstep = None
    failed = None
    if args.timestep_steps > 0 and phase != "main":
        guard.arm(dict(line) if line is not None else None)
        try:
            if os.environ.get("RBL_BENCH_INJECT_FAILURE") == str(rank):     # tests/test_multirank_gpu.py: the guard itself
                raise RuntimeError("injected failure (test hook)")
            tstep = timestep_variants(args, ctx, sm, c, nb, nblb, wall, dev, world, stream, barrier, multi)
        except Exception as e:                               # the hot-path line must not be lost to the time-step part ...
            if world > 1:
                guard.rank_failed(e)                         # rank 0 prints the line with the reason; status 4
            import traceback
            traceback.print_exc()
            tstep = {"error": repr(e)}
            failed = "time-step part failed"                 # ... but a failing step driver makes the exit status non-zero
        guard.disarm()
    others = None
    dropin = None
    dropin_after = None
    mrhs = None
    if world == 1 and args.other_configs and args.config == "cfg3" and phase != "main" and not args.variant and not args.jsplit:
        try:                                                 # (before cfg 5 maps 189 GB: small host-boundary calls measured after it run several times slower)
            dropin = dropin_block(dev)
        except Exception as e:
            import traceback
            traceback.print_exc()
            dropin = {"error": repr(e)}
            failed = failed or "drop-in part failed"
        try:
            others = other_configs(dev, stream, cpu=args.cpu_budget > 0)
        except Exception as e:
            import traceback
            traceback.print_exc()
            others = {"error": repr(e)}
            failed = failed or "other-configs part failed"
        try:
            mrhs = multi_rhs_block(dev, stream)
        except Exception as e:
            import traceback
            traceback.print_exc()
            mrhs = {"error": repr(e)}
            failed = failed or "multi-RHS part failed"
        try:                                                 # the same small host-boundary calls once more, now that cfg 5 has mapped and freed 189 GB
            dropin_after = dropin_block(dev, names=("cfg2",))
        except Exception as e:
            import traceback
            traceback.print_exc()
            dropin_after = {"error": repr(e)}

    if rank == 0:
        if tstep is not None:
            line["timestep"] = tstep
            if "error" not in tstep:
                line["timesteps_per_sec"] = headline_timesteps(tstep)
        if others is not None:
            line["configs"] = others
        if dropin is not None:
            line["dropin"] = dropin
        if dropin_after is not None:
            line["dropin_after_cfg5"] = dropin_after
        if mrhs is not None:
            line["multi_rhs"] = mrhs
        if world == 1 and args.cpu_budget > 0:
            cb = cpu_baseline(c, nb, nblb, wall, args.cpu_budget)
            line["cpu_baseline"] = cb["1core"]
            line["cpu_baseline_allcores"] = cb["allcores"]
            line["speedup_vs_cpu_1core"] = line["value"] / cb["1core"]["value"]
            line["speedup_vs_cpu_allcores"] = line["value"] / cb["allcores"]["value"]
            if tstep is not None and "error" not in tstep:
                line["cpu_baseline_timestep"] = cpu_timestep_baseline(tstep, cb)
        finish(line, args, phase)
    if multi:
        ctx.close()                                          # (destroys the library's communicator before the process group goes)
        dist.destroy_process_group()
    if failed:
        sys.stderr.write("bench.py: %s (see the line's error entry)\n" % failed)
        raise SystemExit(4)


if __name__ == "__main__":
    main()
