#!/usr/bin/env python3
"""Headline benchmark: EKF update-steps/sec at N landmarks and HBM GB/s of the (I - K H) P downdate.

Workload (BASELINE.json configs[2] / configs[3]; SURVEY.md section 8d "Config 3/4"): N = 10 000 landmarks,
known correspondence, F64.  The state is bulk-loaded (x from the seeded world, P = D + U U' with
D = diag(U(0.01,0.1)), U = n x 8 N(0,0.01^2)); one step = 1 predict + 1 correction (EKF_SLAM.m:40-51 and
:124-145) on a cycling landmark index, with range/bearing taken from the world's true pose.  Inputs are
resident in HBM before the timed region; the only per-step host->device traffic is kernel arguments.

A plain run measures the headline alone: set-up, W warm-up steps, exactly K timed steps (one block), the result line.
Everything else below is measured only with --full (every leg carries its own algorithmic bytes per step, so
bytes/step / ms/step <= HBM peak can be checked on each):
  * HEADLINE (`value`, `ms_per_step`, `roofline`): the update-step AS WRITTEN -- cfg.batch = 1, every correction rewrites
    P at once (EKF_SLAM.m:145 once per update-step): B_alg = w n (n+1) bytes per step, one k_downdate_w
    launch per step, purely HBM-bound; this is the number to hold against the >= 60 % roofline target.  With --full a timed
    region under MIN_REGION_S is repeated and the median block quoted; a sharded run (N > 1, --force-sharded) adds one more
    instrumented block, `breakdown_us_per_step`.
  * `deferred`: the engine's deferred mode, cfg.batch = --batch: corrections are kept as pending rank-2
    pairs (every row a later correction reads is patched on the fly) and applied to P in ONE pass per `batch`
    update-steps -- bit-identical results, B_alg / batch + O(n) bytes per step.  The timed region ends with a flush, so
    every correction has been applied to every entry of P inside it.
  * N > 1 only, `deferred_lookahead`: the same with the next batch's landmarks announced (ekf_prefetch_rows): one
    all-gather per batch instead of one per update-step.
  * N = 1 only, `cpu_baseline` / `cpu_baselines` (--no-cpu-baseline skips them): the structured C restatement and the literal-dense
    one, timed on the host's cores.
  * N = 1 only, `other_configs` (after the legs above, each in a child process; --no-other-configs skips it): BASELINE.json's other
    single-GPU configurations -- configs[1] (1 000 landmarks, unknown correspondence, the device-resident measure loop) and the whole
    configs[4] workload on one GPU (40 000 -> 50 000 landmarks, float tiles, the pass in F32 arithmetic): their own JSON lines, verbatim.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--landmarks 10000] [--tile 128] [--full] [--dump-outputs DIR]

--dump-outputs DIR: after the timed steps, the headline leg's state after its last step goes to DIR/<name>.npy, all float64:
x.npy (3+2N), P_digest.npy (trace, sum and sum of squares of P's lower triangle), and on one GPU P_diag_blocks.npy ((N+1) x 2 x 2,
P(1:2,1:2) and every landmark's block) and P_rows.npy (the robot's three rows of P and a fixed, seeded sample of the others,
dump_rows(n); under 64 MB in all).  The inputs are seeded: the same arguments give the same inputs in every run.

N > 1: one process per GPU.  Started by an external launcher (RANK / WORLD_SIZE in the environment, e.g.
`python -m torch.distributed.run --nproc-per-node N bench.py --gpus N ...`) this process is one rank; started plainly as
`python bench.py --gpus N` it spawns that launcher as a CHILD process before touching HIP or torch, relays rank 0's JSON
line and exits non-zero if any rank failed.  P is split over the ranks (tile (I,J) on rank (I+J) mod N) and each
update-step carries one RCCL all-gather of the 2 x 2N landmark row-panel on the library's own communicator
(`config.transport` = "rccl-native"; a failed attach is an error, there is no second transport behind it).
EKF_BENCH_BACKEND=gloo rehearses the multi-rank flow on ONE GPU (host-staged exchange, all ranks on device 0).

Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # B/s, MI355X_MICROARCH.md chip table
F32_MATRIX_PEAK = 157.3e12  # FLOP/s, dense v_mfma_f32_*_f32 (256 FLOPs/cycle/CU x 256 CUs x 2.4 GHz), same table
F64_MATRIX_PEAK = 78.6e12   # FLOP/s, dense v_mfma_f64_*
BF16_MATRIX_PEAK = 2.5e15   # FLOP/s, dense v_mfma_f32_*_bf16 (never the 2:1-sparsity figure), same table
MIN_REGION_S = 0.2          # --full: a timed region shorter than this is repeated (run_leg) and the median quoted
MAX_REPEATS = 9
DUMP_ROWS = 128             # --dump-outputs: rows of P written (fewer where they would pass DUMP_ROWS_BYTES)
DUMP_ROWS_BYTES = 48 << 20


def make_state(N, seed):
    """SURVEY.md 8d config 3 state: world landmarks as the map, P = D + U U' (SPD, dense)."""
    from ekf_slam_amd.world import World
    w = World(N, seed)
    rng = np.random.default_rng(seed + 1)
    n = 3 + 2 * N
    x = np.concatenate([[0.0, 0.0, 0.0], w.landmarks.reshape(-1)])
    d = rng.uniform(0.01, 0.1, size=n)
    U = rng.normal(0.0, 0.01, size=(n, 8))
    s = np.arange(1, N + 1, dtype=np.float64)
    return w, x, s, d, U


def dump_rows(n):
    """Rows of P that --dump-outputs writes: the robot's three, then a fixed, seeded sample of the landmark rows, ascending."""
    m = max(3, min(DUMP_ROWS, n, DUMP_ROWS_BYTES // (8 * n)))
    rest = np.random.default_rng(20260101).choice(np.arange(3, n), size=m - 3, replace=False)
    return np.concatenate([[0, 1, 2], np.sort(rest)]).astype(np.int64)


def make_steps(w, N, count, Rc):
    """(u, z, R, idx0) per step: noisy odometry, observation of a cycling landmark from the true pose."""
    steps = []
    for t in range(count):
        u = w.step()
        k = (t * 37) % N
        (_, r, b), = w.observe([k])
        steps.append((u, np.array([r, b]), np.diag([r * Rc[0], b * Rc[1]]), k))
    return steps


def cpu_baseline(N, x, s, d, U, steps, budget_s=20.0):
    """The structured C restatement (oracle/, kind "port") timed on this host's cores on a bounded sample."""
    from oracle.ekf_structured import StructuredEKF, available_cores
    o = StructuredEKF(N, "known")
    n = 3 + 2 * N
    P = o.raw_P()
    blk = 2048
    for r0 in range(0, n, blk):                       # build D + U U' in row blocks, in place
        r1 = min(n, r0 + blk)
        P[r0:r1, :n] = U[r0:r1] @ U.T
    P[np.arange(n), np.arange(n)] += d
    o._x[:n] = x
    o._s[:N] = s
    o.L.oekf_set_num_landmarks(o.h, N)
    done, t0 = 0, time.perf_counter()
    for (u, z, R, k) in steps:
        o.predict(u)
        o.correct(z, R, k + 1)
        done += 1
        if time.perf_counter() - t0 > budget_s:
            break
    dt = time.perf_counter() - t0
    return {"value": done / dt, "unit": "update-steps/s", "cores": available_cores(), "kind": "port",
            "sample": "%d steps (1 predict + 1 correct) of the same %d-landmark workload, structured O(n^2) C "
                      "restatement with OpenMP (oracle/ekf_structured.c), full n x n P" % (done, N)}


def cpu_baseline_dense(N_target, seed, Rc, n_small=1000, steps=2):
    """the LITERAL-DENSE restatement (oracle/ekf_dense.py: every eye(n), zeros(n), 5 x n selector and n x n x n
    product of EKF_SLAM.m executed as written -- what the reference's MATLAB / MKL executes) timed at n_small landmarks on this
    host's cores and extrapolated to N_target by n^3 (the step is dominated by the two n x n x n products of EKF_SLAM.m:47 and
    the one of :145).  A reported figure beside the primary, structured baseline -- not a target."""
    from oracle import ekf_dense as D
    from oracle.ekf_structured import available_cores
    w, x, s, d, U = make_state(n_small, seed)
    n = 3 + 2 * n_small
    e = D.EKF_SLAM()
    e.x, e.P, e.s = x.copy(), np.diag(d) + U @ U.T, list(s)
    st = make_steps(w, n_small, steps + 1, Rc)
    e.predict(st[0][0]); e._correct(st[0][1], st[0][2], st[0][3] + 1)          # untimed: BLAS threads start, pages are touched
    t0 = time.perf_counter()
    for (u, z, R, k) in st[1:]:
        e.predict(u)
        e._correct(z, R, k + 1)
    dt = (time.perf_counter() - t0) / steps
    nt = 3 + 2 * N_target
    scale = (nt / n) ** 3
    return {"value": 1.0 / (dt * scale), "unit": "update-steps/s", "cores": available_cores(),
            "kind": "literal-dense, extrapolated n^3",
            "sample": "%d steps (1 predict + 1 correct) at %d landmarks through oracle/ekf_dense.py (NumPy/OpenBLAS, O(n^3) as the "
                      "reference is written): %.3f s per step, x (%d/%d)^3 = %.0f for %d landmarks"
                      % (steps, n_small, dt, nt, n, scale, N_target)}


def git_blob_hash(path):
    """`git hash-object` of a file, so that the committed summary a figure was taken from can be told from a stale copy."""
    import hashlib
    with open(path, "rb") as fh:
        data = fh.read()
    return hashlib.sha1(b"blob %d\0" % len(data) + data).hexdigest()


def load_committed_pmc(N, tile, pairs):
    """HBM bytes per downdate launch from the newest committed PMC summary (profiles/round*_downdate_pmc.json: separate
    rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command) for exactly this launch shape, else None."""
    import glob
    import re
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "round*_downdate_pmc.json")),
                   key=lambda f: int(re.search(r"round(\d+)_", os.path.basename(f)).group(1)))
    for path in reversed(files):
        try:
            with open(path) as fh:
                rec = json.load(fh)
        except (OSError, ValueError):
            continue
        for leg in rec.get("legs", []):
            if leg.get("landmarks") == N and leg.get("tile") == tile and leg.get("batch") == pairs:
                return {"file": os.path.relpath(path, ROOT), "git_blob": git_blob_hash(path), "pairs_per_launch": pairs,
                        "landmarks": N, "tile": tile,
                        "kernel": leg.get("kernel"), "hbm_bytes_per_launch": leg.get("hbm_bytes_per_launch"),
                        "matrix_pipe_busy": leg.get("matrix_pipe_busy")}
    return None


def other_configs(timeout_s=300):
    """BASELINE.json's other single-GPU configurations, measured in the same invocation (each in a fresh child process, after the headline
    legs; a failure there is reported in its own entry and never touches the headline): configs[1] -- 1 000 landmarks, unknown
    correspondence, the device-resident measure loop (scripts/bench_config2.py) -- and configs[4]'s whole workload on ONE GPU -- 40 000
    landmarks bulk-loaded, predict + append + correction per step until 50 000, float tiles, the pass in F32 arithmetic at batch 64 and
    again in split arithmetic (scripts/bench_config5.py).  Parity of both is the test suite's business (tests/test_config2_uc_gpu.py, tests/test_full_size_gpu.py)."""
    import subprocess
    root = os.path.dirname(os.path.abspath(__file__))
    runs = (("configs[1]", ["scripts/bench_config2.py", "--batch", "8"]),
            ("configs[4] on one GPU", ["scripts/bench_config5.py", "--storage", "f32_mixed", "--batch", "64", "--landmarks", "40000",
                                       "--steps", "9936", "--warmup", "64"]),
            # the same workload with the pass in split arithmetic (cfg.pass_arith = EKF_ARITH_SPLIT3: three bf16 pieces per float operand,
            # six exact partial products, float accumulation -- the fmaf chain's error class, not its bits; flush32_split.h)
            ("configs[4] on one GPU, split arithmetic", ["scripts/bench_config5.py", "--storage", "f32_split", "--batch", "64", "--landmarks", "40000",
                                                         "--steps", "9936", "--warmup", "64"]),
            # both again with cfg.async_flush: the pass on a second, CU-masked stream beside the next batch's appends and corrections (twice the
            # tile memory; with float tiles not the synchronous engine's bits -- tests/test_f32_mixed_gpu.py, tests/test_f32_split_gpu.py)
            ("configs[4] on one GPU, asynchronous pass", ["scripts/bench_config5.py", "--storage", "f32_mixed", "--batch", "64", "--landmarks", "40000",
                                                          "--steps", "9936", "--warmup", "64", "--async-flush"]),
            ("configs[4] on one GPU, split arithmetic, asynchronous pass", ["scripts/bench_config5.py", "--storage", "f32_split", "--batch", "64",
                                                                            "--landmarks", "40000", "--steps", "9936", "--warmup", "64", "--async-flush"]))
    out = {}
    for key, cmd in runs:
        try:
            r = subprocess.run([sys.executable] + cmd, capture_output=True, text=True, timeout=timeout_s, cwd=root)
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            if r.returncode == 0 and lines:
                out[key] = json.loads(lines[-1])
            else:
                out[key] = {"error": "exit code %d: %s" % (r.returncode, r.stderr.strip().splitlines()[-1][:200] if r.stderr.strip() else "")}
        except Exception as exc:                               # a leg beside the headline: report, never raise
            out[key] = {"error": repr(exc)[:200]}
    return out


def spawn_ranks(args, argv):
    """`python bench.py --gpus N` without a launcher: start one rank per GPU as CHILD processes.  Nothing in this
    process has touched HIP or torch (never re-exec a process that initialised the GPU)."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + argv
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, env=env, text=True)
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
    for ln in proc.stdout.splitlines():
        if not ln.startswith("{"):
            print(ln, file=sys.stderr)
    if proc.returncode != 0 or not lines:
        print("bench.py: the %d-rank run failed (launcher exit code %d)" % (args.gpus, proc.returncode), file=sys.stderr)
        sys.exit(proc.returncode or 1)
    print(lines[-1], flush=True)
    sys.exit(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=1280)
    ap.add_argument("--warmup", type=int, default=128)
    ap.add_argument("--landmarks", type=int, default=10000)
    ap.add_argument("--tile", type=int, default=128)
    ap.add_argument("--batch", type=int, default=20,
                    help="corrections per pass over P in the `deferred` leg (0 / 1: skip that leg).  20: the pass stays above 0.70 of the "
                         "HBM roofline with margin (0.554 ms, 0.72; 24 pairs: 0.57 ms, 0.69-0.70 depending on the box); from 28 pairs on it "
                         "is co-limited by the f64 pipe (32: 0.63 ms, 0.64) for ~20 %% more update-steps/s -- DESIGN.md 3b")
    ap.add_argument("--batch2", type=int, default=32,
                    help="a second `deferred` leg at this batch (entry `deferred_b<batch2>`; 0: none): 32 pairs is the faster whole-step "
                         "rate, 20 the higher roofline fraction of the pass -- both are reported")
    ap.add_argument("--deferred-steps", type=int, default=0,
                    help="timed steps of the deferred legs (default: 40 batches; always whole batches)")
    ap.add_argument("--async-flush", action="store_true",
                    help="every leg: run each pass over P on a second stream into a second tile store, beside the next gather / "
                         "exchange (cfg.async_flush; measured on one GPU: slower at every size, 5-40 %%: profiles/round2_tuning.md sweeps 21, 22)")
    ap.add_argument("--force-sharded", action="store_true",
                    help="--gpus 1 only: run the SHARDED code path (row-panel extraction, RCCL all-gather on the library's own 1-rank "
                         "communicator, sharded gather; cfg.force_sharded) -- the per-step fixed cost of a shard, measurable on one GPU")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baselines")
    ap.add_argument("--no-deferred", action="store_true", help="--full: skip the deferred legs")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="--full: skip the `other_configs` entry (configs[1] and configs[4]'s workload on one GPU, each run in a child process)")
    ap.add_argument("--full", action="store_true",
                    help="beside the headline, every other measurement: the deferred legs, the CPU baselines, other_configs, the sharded "
                         "breakdown, and a short timed region repeated (median quoted).  Without it only the headline leg runs, once")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the headline leg's state after its last timed step to DIR/<name>.npy (float64; module docstring)")
    args = ap.parse_args()

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        spawn_ranks(args, sys.argv[1:])
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        sys.exit("bench.py: --gpus %d but the launcher started %d rank(s)" % (args.gpus, world))

    # stdout carries ONE line, the JSON: libraries that write to file descriptor 1 themselves (RCCL prints a version banner there
    # when a communicator is created) are sent to stderr for the rest of the run
    sys.stdout.flush()
    json_out = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)

    import torch
    from ekf_slam_amd import Engine
    from ekf_slam_amd import _lib as L

    dist = None
    backend = os.environ.get("EKF_BENCH_BACKEND", "nccl")      # "gloo": rehearsal of the multi-rank flow on one GPU
    ndev = torch.cuda.device_count()
    if backend == "nccl" and world > ndev:
        sys.exit("bench.py: %d ranks but %d GPU(s) visible (one process per GPU; EKF_BENCH_BACKEND=gloo rehearses on one)"
                 % (world, ndev))
    device = local_rank % max(ndev, 1)
    if world > 1:
        import torch.distributed as dist
        torch.cuda.set_device(device)
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", device))
        else:
            dist.init_process_group(backend=backend)

    N = args.landmarks
    n = 3 + 2 * N
    seed = 20260101 + 3
    w, x, s, d, U = make_state(N, seed)
    Rc = [.01, 5.0]                                           # EKF_SLAM.m:13
    batch = args.batch if args.full and args.batch > 1 and not args.no_deferred else 0
    d_steps = 0
    if batch:
        d_steps = args.deferred_steps if args.deferred_steps > 0 else 40 * batch
        d_steps = max(batch, (d_steps // batch) * batch)       # whole batches: every launch applies `batch` pairs
    d_warm = 4 * batch
    batch2 = args.batch2 if batch and args.batch2 > 1 and args.batch2 != batch else 0
    d2_steps = max(batch2, ((args.deferred_steps if args.deferred_steps > 0 else 40 * batch2) // max(batch2, 1)) * batch2)
    total = max(args.warmup + args.steps, d_warm + d_steps, 4 * batch2 + d2_steps)
    steps = make_steps(w, N, total, Rc)
    b_alg = 8 * n * (n + 1)                                   # every unique entry read + written once
    b_alg_rank = b_alg / world
    # lower-order bytes of one update-step (9 n w for the 5 gathered rows, G and K), and what a deferred step
    # adds: its (K, G) pair is written once by the gather and read once by the flush (2 x 32 n bytes)
    b_small = 9 * n * 8
    b_pair = 2 * 32 * n

    def barrier(e):
        e.sync()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    conditioning = {"steps": 0}

    forced = bool(args.force_sharded) and world == 1
    sharded = world > 1 or forced

    def run_leg(batch, nsteps, nwarm, lookahead=False, dump=False):
        e = Engine(mode="known", capacity=N, tile=args.tile, device=device, rank=rank, world=world, batch=batch,
                   async_flush=args.async_flush, force_sharded=1 if forced else 0)
        e.load_lowrank_state(x, s, d, U)
        transport = "none"
        if forced:
            import ctypes
            raw = ctypes.create_string_buffer(L.EKF_COMM_ID_BYTES)
            if L.lib().ekf_comm_unique_id(raw) != 0:
                sys.exit("bench.py: --force-sharded needs librccl (ekf_comm_unique_id failed)")
            e.comm_init(raw.raw)                                  # ncclCommInitRank with one rank: no second transport behind it
            transport = "rccl-native"
        if world > 1:
            from ekf_slam_amd.sharding import attach_communicator
            # nccl: the library's own RCCL communicator or an error (no silent second transport); gloo: the rehearsal path
            transport = attach_communicator(e, dist, torch, transport="rccl" if backend == "nccl" else "torch")

        def run(chunk):
            # `chunk` is a marshalled run (Engine.marshal_steps): per step the host only passes addresses -- the per-call
            # numpy / ctypes conversions of the plain methods cost more than a shard's GPU time per step at 8 GPUs
            m = chunk["m"]
            if lookahead and sharded and batch > 1:
                # a host that knows which landmarks the next `batch` corrections touch fetches their base row-panels
                # in ONE all-gather (ekf_prefetch_rows); the corrections then need no exchange of their own.  With the
                # library's own communicator the batch AFTER is announced as well (ekf_prefetch_next): its row-panels are
                # extracted in front of this batch's pass as that pass will leave them, and exchanged beside it
                announce = e._host_exchange is None
                for b0 in range(0, m, batch):
                    b1 = min(m, b0 + batch)
                    if b0 == 0 or not announce:
                        e.prefetch_rows(sorted(set(chunk["k"][b0:b1])))
                    if announce and b1 < m:
                        e.prefetch_next(sorted(set(chunk["k"][b1:min(m, b1 + batch)])))
                    for i in range(b0, b1):
                        e.step_raw(chunk, i)
            else:
                for i in range(m):
                    e.step_raw(chunk, i)
            e.flush()

        # Device conditioning, outside the contract's W warm-up steps and reported as `conditioning_steps`: the first
        # sustained burst of launches in a process sees a one-off 35-70 ms device stall (scripts/probe_queue.py; it does
        # not depend on the queue depth).  Burn it once, then restore the initial state so that W + K steps are the
        # stated workload.
        if not conditioning["steps"]:
            ncond = 448 if batch > 1 else 64
            run(e.marshal_steps((steps * (1 + ncond // max(len(steps), 1)))[:ncond]))
            barrier(e)
            e.load_lowrank_state(x, s, d, U)
            conditioning["steps"] = ncond
        warm_run, timed_run = e.marshal_steps(steps[:nwarm]), e.marshal_steps(steps[nwarm:nwarm + nsteps])

        def reduce_max(v):
            if dist is None:
                return v
            t = torch.tensor([v], dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            return float(t.item())

        def timed_block(fresh):
            """W untimed warm-up steps, then exactly K timed steps between barrier + synchronize pairs; max over ranks."""
            if not fresh:
                e.load_lowrank_state(x, s, d, U)                 # every block runs the same W + K steps from the same state
            run(warm_run)
            barrier(e)
            e.timing_read(L.EKF_KERNEL_DOWNDATE)                 # (drops the warm-up's launches)
            t0 = time.perf_counter()
            run(timed_run)
            barrier(e)
            dt_block = reduce_max(time.perf_counter() - t0)
            cnt, ms = e.timing_read(L.EKF_KERNEL_DOWNDATE)
            pass_stats[0] += cnt
            pass_stats[1] += ms
            return dt_block

        pass_stats = [0, 0.0]                                    # launches of the pass over P inside the timed regions, their device time
        e.timing_enable(L.EKF_KERNEL_DOWNDATE, True, launches=max(nwarm, nsteps) + 8)
        dts = [timed_block(True)]
        # a timed region under 0.2 s is at the mercy of one scheduling hiccup (round 3: 0.01 s regions moved by 7 % between two runs of
        # the same build): with --full, repeat the whole block -- the count follows from the FIRST block's max-over-ranks time, so every
        # rank takes the same number -- and quote the median.  A plain run times exactly its K steps, once
        if args.full and dts[0] < MIN_REGION_S:
            want = int(np.ceil(3 * MIN_REGION_S / max(dts[0], 1e-6)))
            want = min(MAX_REPEATS, max(3, want)) | 1
            while len(dts) < want:
                dts.append(timed_block(False))
        dt = float(np.median(dts))
        launches, kernel_ms = pass_stats
        kernel, kpairs = e.downdate_kernel_name()                # what the launcher actually chose for the last launch
        e.timing_enable(L.EKF_KERNEL_DOWNDATE, False)
        outputs = None
        if dump:
            # what a caller receives after the last timed step (every block ends in the same state); all-reduced digest below
            outputs = {"x": e.get_x()}
            if world == 1:
                outputs["P_diag_blocks"] = e.get_P_diag_blocks()
                outputs["P_rows"] = np.stack([e.get_P_block(int(r), 0, 1, n)[0] for r in dump_rows(n)])
        breakdown = None
        if sharded and args.full:
            # where a sharded update-step's time goes, from one more block with HIP events around every launch of every family (the
            # events cost launches of their own: this block is never the one quoted)
            kinds = (("extraction", L.EKF_KERNEL_ROWPANEL), ("all_gather", L.EKF_KERNEL_EXCHANGE), ("gather", L.EKF_KERNEL_GATHER),
                     ("predict", L.EKF_KERNEL_PREDICT), ("pass", L.EKF_KERNEL_DOWNDATE))
            for _, kid in kinds:
                e.timing_enable(kid, True, launches=nwarm + nsteps + 8)
            e.load_lowrank_state(x, s, d, U)
            run(warm_run)
            barrier(e)
            for _, kid in kinds:
                e.timing_read(kid)                               # (reading resets the sums: the warm-up's launches are dropped)
            t0 = time.perf_counter()
            run(timed_run)
            barrier(e)
            dt_i = reduce_max(time.perf_counter() - t0)
            breakdown = {"unit": "us per update-step, device time between HIP events on this rank's stream (rank 0)",
                         "ms_per_step_instrumented": dt_i / nsteps * 1e3}
            acc = 0.0
            for name, kid in kinds:
                cnt, ms = e.timing_read(kid)
                breakdown[name] = ms * 1e3 / nsteps
                breakdown[name + "_launches"] = cnt
                acc += ms * 1e3 / nsteps
                e.timing_enable(kid, False)
            breakdown["other"] = dt_i / nsteps * 1e6 - acc       # host issue, launch gaps, the step's small copies
        x_end = e.get_x()
        finite = bool(np.isfinite(x_end).all())
        digest = e.digest()                      # this rank's tiles (+ the replicated robot rows on rank 0)
        if dist is not None:
            tdig = torch.tensor(digest, dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
            dist.all_reduce(tdig, op=dist.ReduceOp.SUM)
            digest = tdig.cpu().numpy()
        e.close()
        if outputs is not None:
            outputs["P_digest"] = np.asarray(digest, dtype=np.float64)
        avg_ms = kernel_ms / max(launches, 1)
        achieved = b_alg_rank / (avg_ms * 1e-3)
        per_launch = nsteps * len(dts) / max(launches, 1)
        pmc = load_committed_pmc(N, args.tile, kpairs) if world == 1 else None
        if pmc is not None and pmc.get("kernel") and pmc["kernel"] not in kernel:
            pmc = None                                           # measured on another kernel: does not describe this launch
        roof = {"bound": "hbm", "achieved": achieved / 1e9, "peak": HBM_PEAK / 1e9, "unit": "GB/s",
                "frac": achieved / HBM_PEAK,
                # HBM bytes per launch from PMC counters: they need their own rocprofv3 passes (MI355X_MICROARCH.md), so the
                # figure comes from the committed summary of exactly this launch shape -- null when none matches this run
                "traffic": pmc["hbm_bytes_per_launch"] if pmc else None,
                "from_committed_profile": pmc,
                "kernel": kernel, "pairs_per_launch": kpairs, "launches": launches,
                "avg_launch_ms": avg_ms, "algorithmic_bytes_per_launch": b_alg_rank,
                "update_steps_per_launch": per_launch}
        # algorithmic bytes one update-step moves on this rank: the pass over (this rank's share of) P divided by the steps
        # it serves, + the gathered rows / G / K (replicated on every rank), + the pending pair's write and read when deferred
        b_step = b_alg_rank / max(per_launch, 1e-9) + b_small + (b_pair if batch > 1 else 0)
        ms_step = dt / nsteps * 1e3
        return {"value": nsteps / dt, "ms_per_step": ms_step, "steps": nsteps, "warmup": nwarm, "deferred_batch": batch,
                "repeats": len(dts), "ms_per_step_min": min(dts) / nsteps * 1e3, "ms_per_step_max": max(dts) / nsteps * 1e3,
                "algorithmic_bytes_per_step": b_step, "effective_GBps": b_step / (ms_step * 1e-3) / 1e9,
                "roofline": roof, "transport": transport, "state_finite": finite, "x_end": x_end, "digest": digest,
                "breakdown_us_per_step": breakdown, "outputs": outputs}

    def public(leg, note):
        out = {k: leg[k] for k in ("value", "ms_per_step", "steps", "warmup", "repeats", "ms_per_step_min", "ms_per_step_max",
                                   "deferred_batch", "algorithmic_bytes_per_step", "effective_GBps", "roofline", "state_finite")}
        if leg["breakdown_us_per_step"] is not None:
            out["breakdown_us_per_step"] = leg["breakdown_us_per_step"]
        out["note"] = note
        out["state_digest"] = [float(v) for v in leg["digest"]]
        if leg["steps"] + leg["warmup"] == head["steps"] + head["warmup"]:
            # the same update-steps as the as-written leg: the digest kernel adds in a fixed order, so on one GPU equal
            # states give bit-equal digests (several GPUs: the cross-rank sum is the all-reduce's, equal to rounding)
            out["digest_equals_as_written_leg"] = bool(np.array_equal(leg["digest"], head["digest"]))
            out["x_equals_as_written_leg"] = bool(np.array_equal(leg["x_end"], head["x_end"]))
        return out

    head = run_leg(1, args.steps, args.warmup, dump=args.dump_outputs is not None)
    dfr = dfr2 = look = None
    if batch:
        dfr = run_leg(batch, d_steps, d_warm)
        if batch2:
            dfr2 = run_leg(batch2, d2_steps, 4 * batch2)
        if sharded:
            try:
                look = run_leg(batch, d_steps, d_warm, lookahead=True)
            except Exception as ex:  # noqa: BLE001 -- an argument / state error is raised identically on every rank: report, go on
                print("[rank %d] lookahead leg failed: %s" % (rank, ex), file=sys.stderr, flush=True)
                look = None

    if rank == 0:
        out = {
            "metric": "EKF update-steps/sec at N landmarks; HBM GB/s on (I\u2212KH)P vs roofline",
            "value": head["value"],
            "unit": "update-steps/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": head["ms_per_step"],
            # the timed block (W warm-up + exactly K timed steps) ran `repeats` times; value / ms_per_step are the MEDIAN block's
            "repeats": head["repeats"], "ms_per_step_min": head["ms_per_step_min"], "ms_per_step_max": head["ms_per_step_max"],
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic",
            "config": {"workload": "configs[2]: %d landmarks, known correspondence (EKF_SLAM.m), F64; step = 1 predict"
                                   " + 1 correction on a cycling landmark, P rewritten by every correction as written "
                                   "(EKF_SLAM.m:145); P split over %d GPU(s)" % (N, world),
                       "landmarks": N, "state_dim": n, "tile": args.tile, "storage": "f64",
                       "deferred_batch": 1,
                       "shard": "tile (I,J) on rank (I+J) mod %d" % world, "transport": head["transport"],
                       "exchange": "none" if not sharded else "one all-gather of the 2 x 2N row-panel per update-step",
                       "backend": backend if sharded else "none", "force_sharded": forced,
                       "conditioning_steps": conditioning["steps"], "async_flush": bool(args.async_flush),
                       "state_finite": head["state_finite"],
                       # trace / sum / sum of squares of the final P (lower triangle): the same workload gives the same
                       # digest on 1, 2, 4 or 8 GPUs (to summation order)
                       "state_digest": [float(v) for v in head["digest"]]},
            "algorithmic_bytes_per_step": head["algorithmic_bytes_per_step"],
            "effective_GBps": head["effective_GBps"],
            # SURVEY.md 8d's second unit: a SLAM iteration = 1 predict + m update-steps; here m = 1
            "slam_iterations_per_s": head["value"], "update_steps_per_iteration": 1,
            "roofline": head["roofline"],
        }
        if dfr is not None:
            out["deferred"] = public(dfr, "SURVEY.md 8f-1: the same workload with cfg.batch = %d -- corrections kept as pending rank-2 "
                                          "pairs, ONE pass over P per %d update-steps (k_flush_mfma), bit-identical results; the "
                                          "timed region ends with a flush.  Its own steps / warm-up / bytes per step are stated "
                                          "here; `roofline` describes the flush launch%s"
                                     % (batch, batch, "; one all-gather per update-step" if world > 1 else ""))
        if dfr2 is not None:
            out["deferred_b%d" % batch2] = public(dfr2, "as `deferred`, at cfg.batch = %d" % batch2)
        if look is not None:
            out["deferred_lookahead"] = public(look, "as `deferred`, with the landmarks of the next %d corrections announced: one "
                                                     "all-gather per batch%s" % (batch, " (ekf_prefetch_rows)" if look["transport"] != "rccl-native" else
                                                     ", issued in front of the previous batch's pass and run beside it (ekf_prefetch_next)"))
        if world == 1 and args.full and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(N, x, s, d, U, steps[args.warmup:])
            # SURVEY.md 8d asks for both restatements beside the GPU figure: [0] the primary above, [1] the literal-dense one
            out["cpu_baselines"] = [out["cpu_baseline"], cpu_baseline_dense(N, seed, Rc)]
        if world == 1 and args.full and not args.no_other_configs and not forced:
            out["other_configs"] = other_configs()
        if head["breakdown_us_per_step"] is not None:
            out["breakdown_us_per_step"] = head["breakdown_us_per_step"]
        timed_s = head["ms_per_step"] * 1e-3 * args.steps
        if head["repeats"] > 1 and timed_s < MIN_REGION_S:
            out["config"]["note"] = ("--steps %d: one timed region of the headline leg is %.3f s (< %.1f s): the block was run %d times, "
                                     "`value` is the median block's" % (args.steps, timed_s, MIN_REGION_S, head["repeats"]))
        if args.dump_outputs is not None:
            os.makedirs(args.dump_outputs, exist_ok=True)
            for name, arr in head["outputs"].items():
                np.save(os.path.join(args.dump_outputs, name + ".npy"), np.ascontiguousarray(arr, dtype=np.float64))
        print(json.dumps(out), file=json_out, flush=True)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
