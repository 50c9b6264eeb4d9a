#!/usr/bin/env python3
"""A scan assigned and applied by the device alone (ekf_observe_model_assigned) measured against today's route -- ekf_assign_model, the host
reads the landmarks, m ekf_observe_model steps with res = NULL -- on the two states of scripts/bench_observe_joint.py: 10 000 landmarks
on F64 tiles of edge 128 and 40 000 landmarks on float tiles of edge 256, low-rank loads.  One process per state; every figure is a median
over repeats, each repeat from a RELOADED state (an update shrinks P: repeats on the state it leaves would not measure the same thing),
with the spread (max - min) / median between the repeats.

Per state, per cfg.batch in {1, 32} and per scan of m in {1, 4, 8, 32} sightings (models 1 and 4 alternating, each aimed a little beside a
landmark of its own, spread over the map, gate 9.21), in the same process:
  assigned   one ekf_observe_model_assigned:  returns_ms  host clock until the call returns (nothing is waited for)
                                              drained_ms  ... until a stream synchronise behind it has returned
  today      ekf_assign_model, then m ekf_observe_model at the landmarks it returned: the same two clocks (returns_ms: the last call's return)
  gather_us  device time per launch of the m update-steps under EKF_KERNEL_GATHER (ekf_kernel_timing_read), k_gather_model_assigned beside
             k_gather_model
No ratio is expected in advance: what the removed round trip is worth beside the assignment's own launches is what this measures, and a
point where the new route is slower is reported as it is.

    python scripts/bench_observe_assigned.py --state 10k|40k [--reps K] --out FILE
    python scripts/bench_observe_assigned.py --all [--reps K] [--limit SECONDS] --out profiles/observe_assigned.json
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
SCANS = (1, 4, 8, 32)
GATE = 9.21


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
    out = {"state": name, "landmarks": N, "storage": storage, "tile": tile, "reps": reps, "gate": GATE, "legs": []}
    scans = {}
    for m in SCANS:
        lms = [(q * 313 + 7) % N for q in range(m)]
        scans[m] = [dict(model=1 if q % 2 == 0 else 4, z=sighting(x, lm, 1 if q % 2 == 0 else 4), R=R_RB if q % 2 == 0 else R_FIX, gate=GATE)
                    for q, lm in enumerate(lms)]
    for batch in (1, 32):
        e = Engine(capacity=N, tile=tile, storage=storage, batch=batch)

        def reload():
            e.load_lowrank_state(x, s, d, U)
            e.sync()

        def clocked(fn):
            """(until fn returns, until the streams have drained), ms"""
            reload(); fn(); e.sync()                          # warm-up: every kernel the timed calls launch
            ret, drained = [], []
            for _ in range(reps):
                reload()
                t0 = time.perf_counter()
                fn()
                t1 = time.perf_counter()
                e.sync()
                t2 = time.perf_counter()
                ret.append((t1 - t0) * 1e3); drained.append((t2 - t0) * 1e3)
            return {"returns_ms": figure(ret), "drained_ms": figure(drained)}

        def gather_us(fn, launches_expected):
            v = []
            for _ in range(reps):
                reload()
                e.timing_enable(_lib.EKF_KERNEL_GATHER, True, 2 * launches_expected + 2)
                e.timing_read(_lib.EKF_KERNEL_GATHER)
                fn()
                launches, ms = e.timing_read(_lib.EKF_KERNEL_GATHER)
                e.timing_enable(_lib.EKF_KERNEL_GATHER, False)
                assert launches == launches_expected, (launches, launches_expected)
                v.append(1e3 * ms / launches)
            return figure(v)

        for m in SCANS:
            ents = scans[m]

            def assigned():
                e.observe_model_assigned(ents)

            def today():
                res = e.assign_model(ents)
                for ent, lm in zip(ents, res["landmark"]):
                    e.observe_model(ent["model"], ent["z"], ent["R"], [int(lm)], gate=GATE)

            # what the timed scan does, once, outside the clocks: every sighting finds its landmark and applies, on both routes
            reload(); assigned()
            got = e.assigned_scan_result()
            assert np.all(got["landmark"] >= 0) and np.all(got["outcome"] == _lib.EKF_LINEAR_APPLIED), (got["landmark"], got["outcome"])
            reload()
            assert e.assign_model(ents)["landmark"].tolist() == got["landmark"].tolist()
            leg = {"batch": batch, "scan": m, "assigned": clocked(assigned), "today": clocked(today)}
            leg["assigned"]["gather_us"] = gather_us(assigned, m)
            leg["today"]["gather_us"] = gather_us(today, m)
            for clock in ("returns_ms", "drained_ms"):
                leg["assigned_over_today_" + clock[:-3]] = leg["assigned"][clock]["median"] / leg["today"][clock]["median"]
            out["legs"].append(leg)
        assert e.linear_rejections() == (0, 0), "a timed observation did not apply"
        e.close()
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
        rec = {"metric": "one ekf_observe_model_assigned of a scan of m sightings against ekf_assign_model plus m ekf_observe_model steps in the same "
               "process, at cfg.batch = 1 and 32: host clock until the call(s) return and until a stream synchronise behind them, every repeat from "
               "a reloaded state; device time per update-step launch of either route under EKF_KERNEL_GATHER; medians of the repeats",
               "data": "synthetic", "expectation": "none stated: no ratio is fixed in advance", "states": parts}
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
