#!/usr/bin/env python3
"""ekf_predict_model measured on the two states of profiles/linear_obs.json: configs[2]'s (10 000 landmarks, F64 tiles of edge 128,
low-rank load) and configs[4]'s starting state (40 000 landmarks, float tiles of edge 256, the pass in F32 arithmetic).  One process per
state and library; every figure is a median over repeated measurements, with the spread (max - min) / median between the repeats beside it.

Per state and per chain length m in {1, 8, 32}:
  call_us    the whole no-wait call, host clock from the call to a stream synchronise behind it: one ekf_predict_model of m steps
  launch_us  device time of its launch under the EKF_KERNEL_PREDICT timer: k_predict_model
The yardstick, in the same process and on the same state: m ekf_predict calls and the synchronise behind them -- each call carries out the
one recorded before it and the synchronise the last, m k_predict / k_predict_mfma launches -- measured the same way.  The same yardstick
from another library (the parent commit's): --legs baseline --lib PATH, which runs nothing that library does not have.

The expectations (stated, not asserted): a chain of one costs about one ekf_predict launch; a chain of 32 clearly less than 32 of them,
since the strip is read and written once.

    python scripts/bench_predict_model.py --state 10k|40k [--legs new|baseline] [--lib PATH] [--reps K] --out FILE
    python scripts/bench_predict_model.py --combine A.json B.json ... --out profiles/predict_model.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATES = {"10k": ("configs[2]", 10000, "f64", 128, 20260104), "40k": ("configs[4] start", 40000, "f32_mixed", 256, 20260106)}
M2 = np.array([[1e-4, 2e-5], [2e-5, 4e-4]])
M3 = np.array([[1e-4, 2e-5, 0.0], [2e-5, 1e-4, 1e-5], [0.0, 1e-5, 4e-4]])
CHAINS = (1, 8, 32)


def median(v):
    return float(sorted(v)[len(v) // 2])


def figure(v):
    return {"median": median(v), "spread": float((max(v) - min(v)) / median(v)), "all": v}


def measure_state(key, reps, legs):
    import bench
    from ekf_slam_amd import Engine, _lib
    name, N, storage, tile, seed = STATES[key]
    world, x, s, d, U = bench.make_state(N, seed)
    e = Engine(capacity=N, tile=tile, storage=storage, batch=1)
    e.load_lowrank_state(x, s, d, U)
    e.sync()
    out = {"state": name, "landmarks": N, "storage": storage, "tile": tile, "reps": reps, "legs": legs, "library": os.path.basename(_lib.LIB_PATH),
           "chains": {}}
    u = np.array([0.01, 0.5])
    for m in CHAINS:
        steps = [((1, [0.01, 0.5], M2), (2, [0.01, 0.5], M2), (3, [0.01, 0.0, 0.5], M3))[b % 3] for b in range(m)]

        def chain():
            e.predict_model(steps)

        def singles():
            for _ in range(m):
                e.predict(u)

        rec = {}
        for leg, fn in ((("predict_model", chain),) if legs == "new" else ()) + (("predict_x_m", singles),):
            fn(); e.sync()                                    # warm-up: every kernel the timed calls launch
            call, launch = [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                fn()
                e.sync()
                call.append((time.perf_counter() - t0) * 1e6)
            for _ in range(reps):                             # the launches' device time, one reading per repeat
                e.timing_enable(_lib.EKF_KERNEL_PREDICT, True, 2 * m)
                e.timing_read(_lib.EKF_KERNEL_PREDICT)
                fn()
                e.sync()
                launches, ms = e.timing_read(_lib.EKF_KERNEL_PREDICT)
                e.timing_enable(_lib.EKF_KERNEL_PREDICT, False)
                assert launches == (1 if leg == "predict_model" else m), (leg, launches)
                launch.append(1e3 * ms)
            rec[leg] = {"call_us": figure(call), "launch_us": figure(launch), "launches": 1 if leg == "predict_model" else m}
        if legs == "new":
            a, y = rec["predict_model"], rec["predict_x_m"]
            rec["ratios"] = {"call_over_m_predicts": a["call_us"]["median"] / y["call_us"]["median"],
                             "launch_over_m_predicts": a["launch_us"]["median"] / y["launch_us"]["median"],
                             "launch_over_one_predict": a["launch_us"]["median"] / (y["launch_us"]["median"] / m)}
        out["chains"][str(m)] = rec
    assert np.all(np.isfinite(e.get_x()[:3]))
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--state", choices=sorted(STATES))
    ap.add_argument("--legs", choices=("new", "baseline"), default="new")
    ap.add_argument("--lib", help="the library to load instead of the tree's own (the parent commit's, with --legs baseline)")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--combine", nargs="+", help="per-state outputs to join into one record")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    if args.combine:
        rec = {"metric": "ekf_predict_model of m steps against m ekf_predict launches (host clock from the call to a stream synchronise; device time of "
               "the launches under EKF_KERNEL_PREDICT), medians of the repeats", "data": "synthetic",
               "expectation": "a chain of one costs about one ekf_predict launch; a chain of 32 clearly less than 32 of them (expectations, not assertions)",
               "runs": [json.load(open(p)) for p in args.combine]}
    else:
        if args.lib:
            os.environ["EKF_LIB_PATH"] = os.path.abspath(args.lib)        # (read when ekf_slam_amd._lib is imported)
        sys.path.insert(0, ROOT)
        if args.legs == "baseline":                                       # a library from before this entry point: bind what it has
            import ctypes
            from ekf_slam_amd import _lib
            raw = ctypes.CDLL(_lib.LIB_PATH)
            for n in ("ekf_predict_model", "ekf_motion_evaluate"):
                assert not hasattr(raw, n), "--legs baseline wants a library WITHOUT the new entry points"
                _lib.SIGNATURES.pop(n)
        rec = measure_state(args.state, args.reps, args.legs)
    line = json.dumps(rec)
    print(line, flush=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
