#!/usr/bin/env python3
"""The joint update (ekf_observe_model_joint) measured against the sequential route on the two states of scripts/bench_model_obs.py:
10 000 landmarks on F64 tiles of edge 128 and 40 000 landmarks on float tiles of edge 256, low-rank loads.  One process per state; every
figure is a median over repeats, each repeat from a RELOADED state (an update shrinks P: repeats on the state it leaves would not measure
the same thing), with the spread (max - min) / median between the repeats.

Per state and per np in {1, 4, 8, 32} pairings (models 1 and 4 alternating, each on a landmark of its own, spread over the map):
  joint            one ekf_observe_model_joint, host clock from the call to a stream synchronise behind it: the factor launch, its
                   readback and wait, the gather launch, the np-pair pass.  Beside it the device time of its launches under the
                   EKF_KERNEL_ASSOCIATE (k_joint_factor), _GATHER (k_gather_joint) and _DOWNDATE (the pass) timers.
  sequential_b1    np ekf_observe_model steps on a handle with cfg.batch = 1 (np gathers, np one-pair passes), to a synchronise
  sequential_b32   the same on a handle with cfg.batch = 32, then ekf_flush (np gathers, ONE np-pair pass), to a synchronise
  one_pair_pass    device time of the pass of ONE ekf_observe_model step at cfg.batch = 1, under EKF_KERNEL_DOWNDATE
all in the same process.  The expectations (stated, not asserted): the joint call is about one np-pair pass plus 0.1 ms, far below np
steps at batch 1, and possibly slower than the sequential route at batch 32 for small np.

    python scripts/bench_observe_joint.py --state 10k|40k [--reps K] --out FILE
    python scripts/bench_observe_joint.py --all [--reps K] [--limit SECONDS] --out profiles/observe_joint.json
--all runs each state as a child process of its own under a time limit (--limit, through `timeout`), one after the other, stops at the
first that fails, and joins their records.  --state alone sets no limit: start it under `timeout` yourself.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATES = {"10k": ("10 000 landmarks, F64", 10000, "f64", 128, 20260104), "40k": ("40 000 landmarks, float tiles", 40000, "f32_mixed", 256, 20260106)}
R_FIX = np.array([[0.02, 0.005], [0.005, 0.03]])
R_RB = np.array([[0.02, 0.01], [0.01, 1.2]])
PAIRINGS = (1, 4, 8, 32)


def median(v):
    return float(sorted(v)[len(v) // 2])


def figure(v):
    return {"median": median(v), "spread": float((max(v) - min(v)) / median(v)), "all": v}


def sighting(xe, lm, model):
    """h(x) of a range-and-bearing (1) or relative-position (4) sighting of landmark lm at the state xe, a little beside it."""
    dx, dy = xe[3 + 2 * lm] - xe[0], xe[4 + 2 * lm] - xe[1]
    if model == 1:
        return [float(np.hypot(dx, dy)) + 0.01, float(np.degrees(np.arctan2(dy, dx)) - xe[2]) + 0.05]
    c, sn = np.cos(np.radians(xe[2])), np.sin(np.radians(xe[2]))
    return [float(c * dx + sn * dy) + 0.01, float(-sn * dx + c * dy) - 0.01]


def measure_state(key, reps):
    import bench
    from ekf_slam_amd import Engine, _lib
    name, N, storage, tile, seed = STATES[key]
    world, x, s, d, U = bench.make_state(N, seed)
    out = {"state": name, "landmarks": N, "storage": storage, "tile": tile, "reps": reps, "legs": []}
    scans = {}
    for npair in PAIRINGS:
        lms = [(q * 313 + 7) % N for q in range(npair)]
        scans[npair] = ([dict(model=1 if q % 2 == 0 else 4, z=sighting(x, lm, 1 if q % 2 == 0 else 4), R=R_RB if q % 2 == 0 else R_FIX)
                         for q, lm in enumerate(lms)], lms)
    timers = {"factor_us": _lib.EKF_KERNEL_ASSOCIATE, "gather_us": _lib.EKF_KERNEL_GATHER, "pass_us": _lib.EKF_KERNEL_DOWNDATE}
    results = {npair: {} for npair in PAIRINGS}
    for batch in (32, 1):
        e = Engine(capacity=N, tile=tile, storage=storage, batch=batch)

        def reload():
            e.load_lowrank_state(x, s, d, U)
            e.sync()

        def clocked(fn):
            reload(); fn(); e.sync()                          # warm-up: every kernel the timed call launches
            v = []
            for _ in range(reps):
                reload()
                t0 = time.perf_counter()
                fn()
                e.sync()
                v.append((time.perf_counter() - t0) * 1e3)
            return figure(v)

        def device(fn, which, launches_expected):
            v = []
            for _ in range(reps):
                reload()
                e.timing_enable(which, True, 2 * launches_expected + 2)
                e.timing_read(which)
                fn()
                launches, ms = e.timing_read(which)
                e.timing_enable(which, False)
                assert launches == launches_expected, (launches, launches_expected)
                v.append(1e3 * ms)
            return figure(v)

        for npair in PAIRINGS:
            ents, lms = scans[npair]

            def sequential(flush):
                for ent, lm in zip(ents, lms):
                    e.observe_model(ent["model"], ent["z"], ent["R"], [lm])
                if flush:
                    e.flush()

            if batch == 32:
                def joint():
                    res = e.observe_model_joint(ents, lms)
                    assert res["outcome"] == 1 and res["pairings"] == npair
                rec = {"call_ms": clocked(joint)}
                for label, which in timers.items():
                    rec[label] = device(joint, which, 1)
                rec["pass_kernel"], pairs = e.downdate_kernel_name()
                assert pairs == npair and e.pending() == 0
                results[npair]["joint"] = rec
                results[npair]["sequential_b32"] = {"call_ms": clocked(lambda: sequential(True)), "pass_us": device(lambda: sequential(True), timers["pass_us"], 1),
                                                    "pass_kernel": e.downdate_kernel_name()[0]}
            else:
                results[npair]["sequential_b1"] = {"call_ms": clocked(lambda: sequential(False)), "pass_kernel": e.downdate_kernel_name()[0]}
                if npair == 1:
                    out["one_pair_pass_us"] = device(lambda: sequential(False), timers["pass_us"], 1)
        assert e.linear_rejections() == (0, 0), "a timed observation did not apply"
        e.close()
    for npair in PAIRINGS:
        r = results[npair]
        j, b1, b32 = r["joint"]["call_ms"]["median"], r["sequential_b1"]["call_ms"]["median"], r["sequential_b32"]["call_ms"]["median"]
        out["legs"].append(dict(r, pairings=npair, joint_over_sequential_b1=j / b1, joint_over_sequential_b32=j / b32,
                                joint_call_minus_its_pass_ms=j - r["joint"]["pass_us"]["median"] * 1e-3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--state", choices=sorted(STATES))
    ap.add_argument("--all", action="store_true", help="each state as a child process under --limit seconds, then the joined record")
    ap.add_argument("--limit", type=int, default=420)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    if args.all:
        parts = []
        with tempfile.TemporaryDirectory() as tmp:
            for key in sorted(STATES):
                part = os.path.join(tmp, key + ".json")
                cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--state", key, "--reps", str(args.reps), "--out", part]
                rc = subprocess.run(cmd, stdout=subprocess.DEVNULL).returncode
                if rc != 0:
                    print("state %s ended with status %d: nothing after it is started" % (key, rc), file=sys.stderr)
                    return rc
                parts.append(json.load(open(part)))
        rec = {"metric": "ekf_observe_model_joint of np pairings against np ekf_observe_model steps at cfg.batch = 1 and at cfg.batch = 32 (then a "
               "flush) in the same process: host clock from the call to a stream synchronise, every repeat from a reloaded state; device time "
               "of the joint call's three launches; medians of the repeats", "data": "synthetic",
               "expectation": "stated, not asserted: about one np-pair pass plus 0.1 ms; far below np steps at batch 1; possibly slower than batch 32 "
               "for small np", "states": parts}
    else:
        sys.path.insert(0, ROOT)
        rec = measure_state(args.state, args.reps)
    line = json.dumps(rec)
    print(line, flush=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
