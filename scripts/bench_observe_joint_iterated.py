#!/usr/bin/env python3
"""The relinearised joint update (ekf_observe_model_joint_iterated) measured against ekf_observe_model_joint in the same process, on the
states and by the protocol of scripts/bench_observe_joint.py: 10 000 landmarks on F64 tiles of edge 128 and 40 000 landmarks on float
tiles of edge 256, low-rank loads, np in {1, 4, 8, 32} pairings, every figure a median over repeats, each repeat from a RELOADED state,
with the spread (max - min) / median between the repeats.

Per state and np:
  joint            one ekf_observe_model_joint: host clock from the call to a stream synchronise behind it, and the device time of its factor
                   launch (k_joint_factor) under EKF_KERNEL_ASSOCIATE
  iterated_1       ekf_observe_model_joint_iterated with iterations = 1: the same two figures (k_joint_factor_iter with one linearisation)
  iterated_4       ... with iterations = 4, tol = 0, and the linearisations it used
and from them  factor_iter_over_factor = iterated_1 / joint (device time of the factor launch)  and  per_further_linearisation_us =
(iterated_4 - iterated_1) / (used - 1).  The expectation (stated, not asserted): one linearisation costs about k_joint_factor plus the
move, each further one about one k_joint_factor -- invisible beside the pass up to np = 8, visible at 32.

    python scripts/bench_observe_joint_iterated.py --state 10k|40k [--reps K] --out FILE
    python scripts/bench_observe_joint_iterated.py --all [--reps K] [--limit SECONDS] --out profiles/observe_joint_iterated.json
--all runs each state as a child process of its own under a time limit (--limit, through `timeout`), one after the other, stops at the
first that fails, and joins their records.  --state alone sets no limit: start it under `timeout` yourself.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_observe_joint import PAIRINGS, R_FIX, R_RB, STATES, figure, sighting  # noqa: E402


def measure_state(key, reps):
    import bench
    from ekf_slam_amd import Engine, _lib, marshal
    name, N, storage, tile, seed = STATES[key]
    world, x, s, d, U = bench.make_state(N, seed)
    out = {"state": name, "landmarks": N, "storage": storage, "tile": tile, "reps": reps, "legs": []}
    e = Engine(capacity=N, tile=tile, storage=storage, batch=32)
    factor = _lib.EKF_KERNEL_ASSOCIATE

    def reload():
        e.load_lowrank_state(x, s, d, U)
        e.sync()

    def clocked(fn):
        reload(); fn(); e.sync()                              # warm-up: every kernel the timed call launches
        v = []
        for _ in range(reps):
            reload()
            t0 = time.perf_counter()
            fn()
            e.sync()
            v.append((time.perf_counter() - t0) * 1e3)
        return figure(v)

    def device(fn):
        v = []
        for _ in range(reps):
            reload()
            e.timing_enable(factor, True, 4)
            e.timing_read(factor)
            fn()
            launches, ms = e.timing_read(factor)
            e.timing_enable(factor, False)
            assert launches == 1, launches
            v.append(1e3 * ms)
        return figure(v)

    for npair in PAIRINGS:
        lms = [(q * 313 + 7) % N for q in range(npair)]
        ents = [dict(model=1 if q % 2 == 0 else 4, z=sighting(x, lm, 1 if q % 2 == 0 else 4), R=R_RB if q % 2 == 0 else R_FIX)
                for q, lm in enumerate(lms)]
        arr, m = marshal.scan_obs(ents)
        idx, _ = marshal.index_array([float(k) for k in lms])
        used = {}

        def joint():
            res = e.observe_model_joint(ents, lms)
            assert res["outcome"] == 1 and res["pairings"] == npair

        def iterated(n):
            res, it = _lib.EkfJointResult(), _lib.EkfJointIterResult()
            e._check(e.lib.ekf_observe_model_joint_iterated(e.h, arr, m, idx, float("inf"), n, 0.0, ctypes.byref(res), ctypes.byref(it), None, None))
            assert res.outcome == 1 and res.pairings == npair and it.irregular_at == -1
            used[n] = int(it.used)

        leg = {"pairings": npair}
        for label, fn in (("joint", joint), ("iterated_1", lambda: iterated(1)), ("iterated_4", lambda: iterated(4))):
            leg[label] = {"call_ms": clocked(fn), "factor_us": device(fn)}
        leg["iterated_4"]["used"] = used[4]
        f0, f1, f4 = (leg[k]["factor_us"]["median"] for k in ("joint", "iterated_1", "iterated_4"))
        leg["factor_iter_over_factor"] = f1 / f0
        leg["per_further_linearisation_us"] = (f4 - f1) / (used[4] - 1) if used[4] > 1 else None
        leg["iterated_4_call_over_joint_call"] = leg["iterated_4"]["call_ms"]["median"] / leg["joint"]["call_ms"]["median"]
        out["legs"].append(leg)
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--state", choices=sorted(STATES))
    ap.add_argument("--all", action="store_true", help="each state as a child process under --limit seconds, then the joined record")
    ap.add_argument("--limit", type=int, default=300)
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
        rec = {"metric": "ekf_observe_model_joint_iterated with 1 and with 4 linearisations against ekf_observe_model_joint in the same process: host "
               "clock from the call to a stream synchronise, every repeat from a reloaded state; device time of the factor launch; medians of "
               "the repeats", "data": "synthetic",
               "expectation": "stated, not asserted: each further linearisation costs about one k_joint_factor", "states": parts}
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
