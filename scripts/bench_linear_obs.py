#!/usr/bin/env python3
"""Linear observations as update-steps (ekf_observe_linear, ekf_linear_innovation) measured on the two benchmark states: configs[2]'s
(10 000 landmarks, F64 tiles of edge 128, low-rank load) and configs[4]'s starting state (40 000 landmarks, float tiles of edge 256,
the pass in F32 arithmetic).  One process per state; every figure is a median over repeated measurements.

Per state and per cfg.batch in {1, 32}:
  step_ms       one update-step, host clock over cfg.batch consecutive no-wait steps up to a stream synchronise, divided by cfg.batch
                (the batch's pass over P included: at batch 1 every step carries one) -- for ekf_correct (the yardstick) and for a
                position fix, a landmark fix and a two-landmark H
  waited_ms     host clock around ONE ekf_observe_linear call that asks for its result (it waits for the launch's record itself)
  gather_us     device time of the launch under the EKF_KERNEL_GATHER timer: k_gather for a correction, k_gather_linear for each kind
  innovation_ms host clock around one ekf_linear_innovation call

The yardstick is one ekf_correct step and its k_gather, which the change does not touch: measured in the same process, and from the
PARENT commit's library with `--legs baseline --lib <its libekfslam.so> --commit <its hash>` (binds nothing but what the parent
exports, refuses a library that has the new symbols); hand that output to the run of the new legs with --baseline-json.  The ratios
are step_ms of each kind over the correction's step_ms at the same batch; the expectation (stated, not asserted) is <= 1.25.

    python scripts/bench_linear_obs.py --state 10k|40k [--legs new|baseline] [--lib FILE] [--commit LABEL] [--baseline-json FILE]
                                       [--reps K] --out FILE
    python scripts/bench_linear_obs.py --combine A.json B.json --out profiles/linear_obs.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ekf_observe_linear", "ekf_linear_innovation", "ekf_linear_rejections")
STATES = {"10k": ("configs[2]", 10000, "f64", 128, 20260104), "40k": ("configs[4] start", 40000, "f32_mixed", 256, 20260106)}
R_FIX = np.array([[0.02, 0.005], [0.005, 0.03]])
BATCHES = (1, 32)


def median(v):
    return float(sorted(v)[len(v) // 2])


def measure_state(key, legs, reps):
    import bench
    from ekf_slam_amd import Engine, _lib
    name, N, storage, tile, seed = STATES[key]
    world, x, s, d, U = bench.make_state(N, seed)
    steps = bench.make_steps(world, N, 64, [.01, 5.0])
    rng = np.random.default_rng(seed + 7)
    at = lambda k: x[3 + 2 * k:5 + 2 * k]
    i, j = N // 3, N - 5
    kinds = {"position_fix": dict(z=x[:2] + [0.03, -0.02], R=R_FIX, Hr=[[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], landmarks=(), Hl=()),
             "landmark_fix": dict(z=at(i) + [0.05, -0.03], R=R_FIX, Hr=None, landmarks=(i,), Hl=(np.eye(2),)),
             "two_landmark_H": dict(z=(at(i) - at(j)) + [0.05, -0.03], R=R_FIX, Hr=rng.standard_normal((2, 3)) * [0.1, 0.1, 0.001],
                                    landmarks=(i, j), Hl=(np.eye(2), -np.eye(2)))}
    out = {"state": name, "landmarks": N, "storage": storage, "tile": tile, "reps": reps, "batches": {}}
    for batch in BATCHES:
        e = Engine(capacity=N, tile=tile, storage=storage, batch=batch)
        e.load_lowrank_state(x, s, d, U)
        e.sync()

        def correct_step(t):
            u, z, R, k = steps[t % len(steps)]
            e.predict(u); e.correct(z, R, k)

        def runner(kind):
            if kind == "correct":
                return correct_step
            o = kinds[kind]
            return lambda t: (e.predict(steps[t % len(steps)][0]), e.observe_linear(o["z"], o["R"], o["Hr"], o["landmarks"], o["Hl"]))

        rec = {}
        for kind in ["correct"] + (sorted(kinds) if legs == "new" else []):
            step = runner(kind)
            for t in range(batch):                            # warm-up: every kernel the timed steps launch, one whole batch
                step(t)
            e.sync()
            per_step = []
            for r in range(reps):
                t0 = time.perf_counter()
                for t in range(batch):
                    step(r * batch + t)
                e.sync()
                per_step.append((time.perf_counter() - t0) * 1e3 / batch)
            assert e.pending() == 0
            e.timing_enable(_lib.EKF_KERNEL_GATHER, True, 2 * batch * reps)
            e.timing_read(_lib.EKF_KERNEL_GATHER)
            for t in range(batch * reps):
                step(t)
            launches, ms = e.timing_read(_lib.EKF_KERNEL_GATHER)
            e.timing_enable(_lib.EKF_KERNEL_GATHER, False)
            rec[kind] = {"step_ms": {"median": median(per_step), "all": per_step}, "gather_us": 1e3 * ms / max(launches, 1), "gather_launches": launches}
            if kind != "correct":
                o = kinds[kind]
                w, q = [], []
                for r in range(reps):
                    e.predict(steps[r][0]); e.sync()
                    t0 = time.perf_counter()
                    e.linear_innovation(o["z"], o["R"], o["Hr"], o["landmarks"], o["Hl"])
                    q.append((time.perf_counter() - t0) * 1e3)
                    t0 = time.perf_counter()
                    e.observe_linear(o["z"], o["R"], o["Hr"], o["landmarks"], o["Hl"], wait=True)
                    w.append((time.perf_counter() - t0) * 1e3)
                    e.sync()
                e.flush(); e.sync()
                rec[kind]["waited_ms"] = {"median": median(w), "all": w}
                rec[kind]["innovation_ms"] = {"median": median(q), "all": q}
        rec["pass_kernel"] = e.downdate_kernel_name()[0]
        out["batches"][str(batch)] = rec
        e.close()
    return out


def with_ratios(new, base):
    """step_ms of each kind over the correction's, same batch: against the correction of the same process and against the parent's."""
    r = {"expectation": "every ratio <= 1.25 (an expectation, not an assertion)", "over_own_correct": {}, "over_parent_correct": {}}
    for b, rec in new["batches"].items():
        own = rec["correct"]["step_ms"]["median"]
        par = base["batches"][b]["correct"]["step_ms"]["median"] if base else None
        r["over_own_correct"][b] = {k: v["step_ms"]["median"] / own for k, v in rec.items() if isinstance(v, dict) and k != "correct"}
        if par:
            r["over_parent_correct"][b] = {k: v["step_ms"]["median"] / par for k, v in rec.items() if isinstance(v, dict) and k != "correct"}
            r["over_parent_correct"][b]["correct"] = own / par
    worst = [v for grp in ("over_own_correct", "over_parent_correct") for d in r[grp].values() for k, v in d.items() if k != "correct"]
    r["met"] = bool(worst) and max(worst) <= 1.25
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--state", choices=sorted(STATES))
    ap.add_argument("--legs", choices=["new", "baseline"], default="new")
    ap.add_argument("--lib", help="the libekfslam.so to measure (default: the tree's)")
    ap.add_argument("--commit", default="working tree", help="label of the code the library was built from")
    ap.add_argument("--baseline-json", help="output of a --legs baseline run of the same state on the parent commit")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--combine", nargs="+", help="per-state outputs to join into one record")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    if args.combine:
        rec = {"metric": "ekf_observe_linear / ekf_linear_innovation against one ekf_correct step (host clock over cfg.batch no-wait steps to a "
               "stream synchronise, per step; device time of the gather launch), medians", "data": "synthetic",
               "states": [json.load(open(p)) for p in args.combine]}
    else:
        if args.lib:
            os.environ["EKF_LIB_PATH"] = os.path.abspath(args.lib)
        sys.path.insert(0, ROOT)
        from ekf_slam_amd import _lib
        if args.legs == "baseline":
            import ctypes
            raw = ctypes.CDLL(_lib.LIB_PATH)
            assert not any(hasattr(raw, n) for n in NEW_SYMBOLS), "--legs baseline wants a library WITHOUT the new entry points"
            for n in NEW_SYMBOLS:
                _lib.SIGNATURES.pop(n)
        res = measure_state(args.state, args.legs, args.reps)
        rec = {"commit": args.commit, "library": os.path.basename(_lib.LIB_PATH), "legs": args.legs, **res}
        base = json.load(open(args.baseline_json)) if args.baseline_json else None
        if base:
            assert base["landmarks"] == res["landmarks"] and base["storage"] == res["storage"]
        if args.legs == "new":
            rec = {"state": res["state"], "landmarks": res["landmarks"], "storage": res["storage"], "tile": res["tile"], "parent": base,
                   "this_change": rec, "ratios": with_ratios(res, base)}
    line = json.dumps(rec)
    print(line, flush=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
