#!/usr/bin/env python3
"""ekf_joint_innovation measured on configs[2]'s state of profiles/linear_obs.json: 10 000 landmarks, F64 tiles of edge 128, low-rank
load.  One process; every figure is a median over repeated measurements, with the spread (max - min) / median between the repeats.

Per scan size m in {8, 32}, hypothesis count nh in {1, 64, 256} and 0 / 31 pending pairs (cfg.batch = 32, 31 update-steps behind the load):
  call_us     the whole call, host clock around one ekf_joint_innovation with the prefixes asked for (it returns with the results: the
              upload of the hypotheses, one launch, one readback, one wait)
  launch_us   device time of k_joint_innovation under the EKF_KERNEL_ASSOCIATE timer
Every hypothesis pairs ALL m observations (models 1 and 4 alternating: the 2m x 2m system), each with a landmark of its own: the most a
hypothesis can cost.  With pending pairs every one of the m (m - 1) / 2 cross blocks walks the 31-pair chain four times.
Beside them, in the same process and on the same state, as yardsticks:
  model_innovation    one ekf_model_innovation (one pairing, one launch, one wait)
  associate_model     one ekf_associate_model of the same m observations against all N landmarks
No figure is a pass/fail bar.

    python scripts/bench_joint.py [--reps K] --out profiles/joint_innovation.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, STORAGE, TILE, SEED = 10000, "f64", 128, 20260104
R_FIX = np.array([[0.02, 0.005], [0.005, 0.03]])
R_RB = np.array([[0.02, 0.01], [0.01, 1.2]])
SCANS, HYPS, PENDING = (8, 32), (1, 64, 256), (0, 31)


def median(v):
    return float(sorted(v)[len(v) // 2])


def figure(v):
    return {"median": median(v), "spread": float((max(v) - min(v)) / median(v)), "all": v}


def sighting(xe, lm, model):
    """h(x) of a range-and-bearing (1) or relative-position (4) sighting of landmark lm at the state xe."""
    dx, dy = xe[3 + 2 * lm] - xe[0], xe[4 + 2 * lm] - xe[1]
    if model == 1:
        return [float(np.hypot(dx, dy)), float(np.degrees(np.arctan2(dy, dx)) - xe[2])]
    c, sn = np.cos(np.radians(xe[2])), np.sin(np.radians(xe[2]))
    return [float(c * dx + sn * dy), float(-sn * dx + c * dy)]


def timed(e, fn, reps, brackets):
    """(call_us, launch_us) of fn: the host clock around it, then the device time of its launches under EKF_KERNEL_ASSOCIATE."""
    from ekf_slam_amd import _lib
    fn()                                                      # warm-up
    call, launch = [], []
    for _ in range(reps):
        e.sync()
        t0 = time.perf_counter()
        fn()
        call.append((time.perf_counter() - t0) * 1e6)
    for _ in range(reps):
        e.timing_enable(_lib.EKF_KERNEL_ASSOCIATE, True, 4)
        e.timing_read(_lib.EKF_KERNEL_ASSOCIATE)
        fn()
        launches, ms = e.timing_read(_lib.EKF_KERNEL_ASSOCIATE)
        e.timing_enable(_lib.EKF_KERNEL_ASSOCIATE, False)
        assert launches == brackets
        launch.append(1e3 * ms)
    return figure(call), figure(launch)


def measure(reps):
    import bench
    from ekf_slam_amd import Engine
    world, x, s, d, U = bench.make_state(N, SEED)
    rng = np.random.default_rng(5)
    out = {"state": "configs[2]", "landmarks": N, "storage": STORAGE, "tile": TILE, "reps": reps, "legs": []}
    for pending in PENDING:
        e = Engine(capacity=N, tile=TILE, storage=STORAGE, batch=32)
        e.load_lowrank_state(x, s, d, U)
        for q in range(pending):                              # update-steps that stay pending: sightings of landmarks spread over the map
            k = (q * 313) % N
            e.observe_model(4, np.array(sighting(x, k, 4)) + 0.01, R_FIX, [k])
        e.sync()
        assert e.pending() == pending
        for m in SCANS:
            lms = rng.choice(N, m, replace=False)
            xe = e.get_x()
            # sightings of the landmarks themselves: the first hypothesis is the true one
            entries = [dict(model=1 if b % 2 == 0 else 4, z=sighting(xe, int(lm), 1 if b % 2 == 0 else 4), R=R_RB if b % 2 == 0 else R_FIX, gate=9.21)
                       for b, lm in enumerate(lms)]
            yard = {}
            ent = entries[0]
            probe = []
            for _ in range(reps):
                e.sync()
                t0 = time.perf_counter()
                e.model_innovation(ent["model"], ent["z"], ent["R"], [int(lms[0])])
                probe.append((time.perf_counter() - t0) * 1e6)
            yard["model_innovation"] = {"call_us": figure(probe)}
            call, launch = timed(e, lambda: e.associate_model(entries), reps, 1)
            yard["associate_model"] = {"call_us": call, "launch_us": launch}
            for nh in HYPS:
                hyps = np.array([np.roll(lms, i % m) if i % 2 == 0 else rng.permutation(lms) for i in range(nh)], dtype=np.int64)
                res = e.joint_innovation(entries, hyps)
                assert np.all(res["pairings"] == m) and res["outcome"][0] == 1 and np.isfinite(res["d2"][0])
                call, launch = timed(e, lambda: e.joint_innovation(entries, hyps), reps, 1)
                out["legs"].append({"m": m, "nh": nh, "pending": pending, "call_us": call, "launch_us": launch,
                                    "launch_share_of_call": launch["median"] / call["median"],
                                    "call_over_model_innovation": call["median"] / yard["model_innovation"]["call_us"]["median"],
                                    "call_over_associate_model": call["median"] / yard["associate_model"]["call_us"]["median"],
                                    "regular_hypotheses": int(np.sum(res["outcome"] == 1)), "yardsticks": yard})
            assert e.pending() == pending
        e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    rec = {"metric": "ekf_joint_innovation of nh hypotheses that pair all m observations (host clock around the waited call; device time of "
           "k_joint_innovation under EKF_KERNEL_ASSOCIATE), with ekf_model_innovation and ekf_associate_model in the same process as yardsticks; "
           "medians of the repeats", "data": "synthetic", "expectation": "none: the cost of this probe is measured, not tuned"}
    rec.update(measure(args.reps))
    line = json.dumps(rec)
    print(line, flush=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
