#!/usr/bin/env python3
"""The relinearised model observation (ekf_observe_model_iterated) measured on the two states of scripts/bench_model_obs.py: 10 000
landmarks on F64 tiles of edge 128 and 40 000 landmarks on float tiles of edge 256 (the pass in F32 arithmetic), low-rank loads.  One
process per state; every figure is a median over repeated measurements.

Per state, per cfg.batch in {1, 32}, for a range-and-bearing observation of one landmark and a landmark range between two:
  step_ms    one update-step, host clock over cfg.batch consecutive no-wait steps up to a stream synchronise, divided by cfg.batch
             (the batch's pass over P included: at batch 1 every step carries one)
  gather_us  device time of the launch under the EKF_KERNEL_GATHER timer: k_gather_model / k_gather_model_iter
for ekf_observe_model (the yardstick, in the same process) and for ekf_observe_model_iterated asked for 1, 3 and 8 linearisations with
tol = 0.  `used` is how many of them ran, as ekf_model_innovation_iterated reports it on the loaded state: under tol = 0 the loop ends
early only at a step of exactly 0, which the tight priors of these states do reach (the landmark range within three).

The expectation (stated, not asserted): a few microseconds per extra linearisation on a launch of 8-17, invisible beside the pass.
per_linearisation_us is (gather_us at 8 - gather_us at 1) / (used at 8 - used at 1); the spread of a quantity is (max - min) / median
over its repeats.

    python scripts/bench_model_obs_iterated.py --state 10k|40k [--reps K] --out FILE
    python scripts/bench_model_obs_iterated.py --combine A.json B.json --out profiles/model_obs_iterated.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATES = {"10k": ("10 000 landmarks, F64", 10000, "f64", 128, 20260104), "40k": ("40 000 landmarks, float tiles", 40000, "f32_mixed", 256, 20260106)}
R_FIX = np.array([[0.02, 0.005], [0.005, 0.03]])
BATCHES = (1, 32)
ITERATIONS = (1, 3, 8)


def median(v):
    return float(sorted(v)[len(v) // 2])


def spread(v):
    return float((max(v) - min(v)) / median(v))


def measure_state(key, reps):
    import bench
    from ekf_slam_amd import Engine, _lib
    name, N, storage, tile, seed = STATES[key]
    world, x, s, d, U = bench.make_state(N, seed)
    steps = bench.make_steps(world, N, 64, [.01, 5.0])
    at = lambda k: x[3 + 2 * k:5 + 2 * k]
    i, j = N // 3, N - 5
    out = {"state": name, "landmarks": N, "storage": storage, "tile": tile, "reps": reps, "batches": {}}
    for batch in BATCHES:
        e = Engine(capacity=N, tile=tile, storage=storage, batch=batch)
        e.load_lowrank_state(x, s, d, U)
        e.sync()
        obs = {}
        for kind, model, lms in (("range_bearing", 1, (i,)), ("landmark_range", 5, (i, j))):
            hx, _ = Engine.model_evaluate(model, x[:3], at(lms[0]), at(lms[1]) if model == 5 else None, lib=e.lib)
            rows = 2 if model == 1 else 1
            obs[kind] = dict(model=model, z=hx[:rows] + 0.05, R=R_FIX if rows == 2 else np.array([[0.05, 0.0], [0.0, 0.0]]), landmarks=lms)

        def runner(kind, n):
            o = obs[kind]
            if n == 0:
                return lambda t: (e.predict(steps[t % len(steps)][0]), e.observe_model(o["model"], o["z"], o["R"], o["landmarks"]))
            return lambda t: (e.predict(steps[t % len(steps)][0]),
                              e.observe_model_iterated(o["model"], o["z"], o["R"], o["landmarks"], iterations=n, tol=0.0))

        def measure(kind, n):
            step = runner(kind, n)
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
            gather = []
            for r in range(reps):                             # the launch's device time, one reading per repeat: its spread is measured too
                e.timing_enable(_lib.EKF_KERNEL_GATHER, True, 2 * batch)
                e.timing_read(_lib.EKF_KERNEL_GATHER)
                for t in range(batch):
                    step(r * batch + t)
                launches, ms = e.timing_read(_lib.EKF_KERNEL_GATHER)
                e.timing_enable(_lib.EKF_KERNEL_GATHER, False)
                assert launches == batch
                gather.append(1e3 * ms / launches)
            e.flush(); e.sync()
            return {"step_ms": {"median": median(per_step), "spread": spread(per_step), "all": per_step},
                    "gather_us": {"median": median(gather), "spread": spread(gather), "all": gather}}

        rec = {}
        for kind in sorted(obs):
            legs = {"observe_model": measure(kind, 0)}
            o = obs[kind]
            for n in ITERATIONS:
                used = e.model_innovation_iterated(o["model"], o["z"], o["R"], o["landmarks"], iterations=n, tol=0.0)["iterated"]["used"]
                legs["iterated_%d" % n] = dict(measure(kind, n), used=used)
            g = {k: v["gather_us"]["median"] for k, v in legs.items()}
            st = {k: v["step_ms"]["median"] for k, v in legs.items()}
            extra = legs["iterated_8"]["used"] - legs["iterated_1"]["used"]
            legs["summary"] = {"per_linearisation_us": (g["iterated_8"] - g["iterated_1"]) / extra if extra else None,
                               "gather_iterated_1_over_observe_model": g["iterated_1"] / g["observe_model"],
                               "step_over_observe_model": {k: st[k] / st["observe_model"] for k in st if k != "observe_model"}}
            rec[kind] = legs
        irregular, gated = e.linear_rejections()
        assert (irregular, gated) == (0, 0), "a timed observation did not apply"
        rec["pass_kernel"] = e.downdate_kernel_name()[0]
        out["batches"][str(batch)] = rec
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
        rec = {"metric": "ekf_observe_model_iterated with 1, 3 and 8 linearisations against ekf_observe_model in the same process (host clock over "
               "cfg.batch no-wait steps to a stream synchronise, per step; device time of the gather launch), medians of the repeats",
               "data": "synthetic", "states": [json.load(open(p)) for p in args.combine]}
    else:
        sys.path.insert(0, ROOT)
        rec = measure_state(args.state, args.reps)
    line = json.dumps(rec)
    print(line, flush=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
