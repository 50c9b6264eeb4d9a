#!/usr/bin/env python3
"""ekf_append_model measured on the two states of profiles/linear_obs.json: configs[2]'s (10 000 landmarks, F64 tiles of edge 128,
low-rank load) and configs[4]'s starting state (40 000 landmarks, float tiles of edge 256, the pass in F32 arithmetic).  One process per
state; every figure is a median over repeated measurements, with the spread (max - min) / median between the repeats beside it.

Per state and per scan size m in {1, 8, 32}:
  call_us    the whole no-wait call, host clock from the call to a stream synchronise behind it: one ekf_append_model of m entries
  launch_us  device time of its launch under the EKF_KERNEL_APPEND timer: k_append_model
The yardstick, in the same process and on the same state: m ekf_append calls (m k_append launches), measured the same way.  Every repeat
starts from the same map: the landmarks a repeat appended are removed again (ekf_remove_landmarks, outside the timed region).

The expectations (stated, not asserted): a scan of one costs about one k_append launch; a scan of m costs clearly less than m appends.

    python scripts/bench_append_model.py --state 10k|40k [--reps K] --out FILE
    python scripts/bench_append_model.py --combine A.json B.json --out profiles/append_model.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATES = {"10k": ("configs[2]", 10000, "f64", 128, 20260104), "40k": ("configs[4] start", 40000, "f32_mixed", 256, 20260106)}
R_FIX = np.array([[0.02, 0.005], [0.005, 0.03]])
R_RB = np.array([[0.02, 0.01], [0.01, 1.2]])
SCANS = (1, 8, 32)


def median(v):
    return float(sorted(v)[len(v) // 2])


def spread(v):
    return float((max(v) - min(v)) / median(v))


def figure(v):
    return {"median": median(v), "spread": spread(v), "all": v}


def measure_state(key, reps):
    import bench
    from ekf_slam_amd import Engine, _lib
    name, N, storage, tile, seed = STATES[key]
    world, x, s, d, U = bench.make_state(N, seed)
    rng = np.random.default_rng(5)
    e = Engine(capacity=N + max(SCANS), tile=tile, storage=storage, batch=1)
    e.load_lowrank_state(x, s, d, U)
    e.sync()
    out = {"state": name, "landmarks": N, "storage": storage, "tile": tile, "reps": reps, "scans": {}}
    u = np.array([0.1, 1.0])
    for m in SCANS:
        entries = [(1, [rng.uniform(2.0, 25.0), rng.uniform(0.0, 360.0)], R_RB, 1e6 + b) if b % 2 == 0 else
                   (4, rng.uniform(-15.0, 15.0, 2), R_FIX, 1e6 + b) for b in range(m)]
        spots = rng.uniform(-20.0, 20.0, (m, 2))

        def scan():
            e.append_model(entries)

        def singles():
            for b in range(m):
                e.append(u, R_RB, spots[b], 1e6 + b)

        def restore():
            e.remove_landmarks(list(range(N, N + m)))
            e.sync()
            assert e.N == N

        rec = {}
        for leg, fn in (("append_model", scan), ("append_x_m", singles)):
            fn(); restore()                                   # warm-up: every kernel the timed calls launch
            call, launch = [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                fn()
                e.sync()
                call.append((time.perf_counter() - t0) * 1e6)
                restore()
            for _ in range(reps):                             # the launches' device time, one reading per repeat
                e.timing_enable(_lib.EKF_KERNEL_APPEND, True, 2 * m)
                e.timing_read(_lib.EKF_KERNEL_APPEND)
                fn()
                launches, ms = e.timing_read(_lib.EKF_KERNEL_APPEND)
                e.timing_enable(_lib.EKF_KERNEL_APPEND, False)
                assert launches == (1 if leg == "append_model" else m)
                launch.append(1e3 * ms)
                restore()
            rec[leg] = {"call_us": figure(call), "launch_us": figure(launch), "launches": 1 if leg == "append_model" else m}
        a, y = rec["append_model"], rec["append_x_m"]
        rec["ratios"] = {"call_over_m_appends": a["call_us"]["median"] / y["call_us"]["median"],
                         "launch_over_m_appends": a["launch_us"]["median"] / y["launch_us"]["median"],
                         "launch_over_one_append": a["launch_us"]["median"] / (y["launch_us"]["median"] / m)}
        out["scans"][str(m)] = rec
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--state", choices=sorted(STATES))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--combine", nargs="+", help="per-state outputs to join into one record")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    if args.combine:
        rec = {"metric": "ekf_append_model of m entries against m ekf_append calls (host clock from the call to a stream synchronise; device time of "
               "the launches under EKF_KERNEL_APPEND), medians of the repeats", "data": "synthetic",
               "expectation": "a scan of one costs about one k_append launch; a scan of m clearly less than m appends (expectations, not assertions)",
               "states": [json.load(open(p)) for p in args.combine]}
    else:
        sys.path.insert(0, ROOT)
        rec = measure_state(args.state, args.reps)
    line = json.dumps(rec)
    print(line, flush=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
