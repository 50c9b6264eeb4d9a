#!/usr/bin/env python3
"""The linear observation with a dense H (ekf_observe_dense) measured on the two states of scripts/bench_observe_joint.py: 10 000
landmarks on F64 tiles of edge 128 and 40 000 landmarks on float tiles of edge 256, low-rank loads.  One process per state; every figure
is a median over repeats, each repeat from a RELOADED state (an update shrinks P), with the spread (max - min) / median between them.

Per state and per k in {1, 2, 8, 16} dense Gaussian rows (R a hundredth of the mean diagonal of H P H', z = H x + 0.1):
  dense            one ekf_observe_dense, host clock from the call to a stream synchronise behind it.  Beside it the device time of its
                   launches by timing family: EKF_KERNEL_ASSOCIATE (the tile pass of the product, k_dense_gram and k_dense_factor: three
                   launches), _COMPACT (the product's sums), _GATHER (k_gather_dense), _DOWNDATE (the pass).  The family timers cannot
                   separate k_dense_gram and k_dense_factor from the tile pass: `gram_factor_us` is the family's time less the tile
                   pass of ekf_multiply_map measured beside it.
  multiply_map     one ekf_multiply_map of the same k rows to a synchronise, and the device time of its tile pass: with the one-pair pass
                   below, the floor this design sets itself
  joint            one ekf_observe_model_joint of ceil(k / 2) pairings, to a synchronise
  one_pair_pass    device time of the pass of ONE ekf_observe_model step at cfg.batch = 1
  host_route       (10 000 landmarks only, 3 repeats) get_P, the NumPy update, set_P
all in the same process.  No figure is asserted.

    python scripts/bench_observe_dense.py --state 10k|40k [--reps K] --out FILE
    python scripts/bench_observe_dense.py --all [--reps K] [--limit SECONDS] --out profiles/observe_dense.json
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_observe_joint import R_FIX, R_RB, STATES, figure, sighting  # noqa: E402

ROWS = (1, 2, 8, 16)


def measure_state(key, reps):
    import bench
    from ekf_slam_amd import Engine, _lib
    name, N, storage, tile, seed = STATES[key]
    world, x, s, d, U = bench.make_state(N, seed)
    n = 3 + 2 * N
    out = {"state": name, "landmarks": N, "storage": storage, "tile": tile, "reps": reps, "legs": []}
    e = Engine(capacity=N, tile=tile, storage=storage, batch=1)

    def reload():
        e.load_lowrank_state(x, s, d, U)
        e.sync()

    def clocked(fn, count=reps):
        reload(); fn(); e.sync()                              # warm-up: every kernel and every allocation of the timed call
        v = []
        for _ in range(count):
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

    # the scale of H P H' from one product (the low-rank state's P is not formed on the host)
    reload()
    rng = np.random.default_rng(7)
    Hall = rng.standard_normal((max(ROWS), n))
    rho = 0.01 * float(np.mean(np.sum(Hall * e.multiply_map(Hall), axis=1)))
    ent1 = dict(model=1, z=sighting(x, 7, 1), R=R_RB)
    out["one_pair_pass_us"] = device(lambda: e.observe_model(ent1["model"], ent1["z"], ent1["R"], [7]), _lib.EKF_KERNEL_DOWNDATE, 1)
    for k in ROWS:
        H = np.ascontiguousarray(Hall[:k])
        z, R = H @ x + 0.1, rho * np.eye(k)

        def dense():
            res = e.observe_dense(H, z, R)
            assert res["outcome"] == 1 and res["rows"] == k

        rec = {"rows": k, "dense": {"call_ms": clocked(dense)}}
        for label, which, launches in (("associate_us", _lib.EKF_KERNEL_ASSOCIATE, 3), ("sums_us", _lib.EKF_KERNEL_COMPACT, 1),
                                       ("gather_us", _lib.EKF_KERNEL_GATHER, 1), ("pass_us", _lib.EKF_KERNEL_DOWNDATE, 1)):
            rec["dense"][label] = device(dense, which, launches)
        rec["dense"]["pass_kernel"], pairs = e.downdate_kernel_name()
        assert pairs == (k + 1) // 2 and e.pending() == 0
        rec["multiply_map"] = {"call_ms": clocked(lambda: e.multiply_map(H)),
                               "tile_pass_us": device(lambda: e.multiply_map(H), _lib.EKF_KERNEL_ASSOCIATE, 1)}
        rec["dense"]["gram_factor_us"] = rec["dense"]["associate_us"]["median"] - rec["multiply_map"]["tile_pass_us"]["median"]
        npair = (k + 1) // 2
        lms = [(q * 313 + 7) % N for q in range(npair)]
        ents = [dict(model=1 if q % 2 == 0 else 4, z=sighting(x, lm, 1 if q % 2 == 0 else 4), R=R_RB if q % 2 == 0 else R_FIX) for q, lm in enumerate(lms)]
        rec["joint"] = {"pairings": npair, "call_ms": clocked(lambda: e.observe_model_joint(ents, lms))}
        floor = rec["multiply_map"]["call_ms"]["median"] + out["one_pair_pass_us"]["median"] * 1e-3
        rec["dense_over_floor"] = rec["dense"]["call_ms"]["median"] / floor
        rec["dense_over_joint"] = rec["dense"]["call_ms"]["median"] / rec["joint"]["call_ms"]["median"]
        if key == "10k":
            def host_route():
                P, xe = e.get_P(), e.get_x()
                G = P @ H.T
                S = H @ G + R
                W = np.linalg.solve(np.linalg.cholesky(S), G.T)
                e.set_x(xe + W.T @ np.linalg.solve(np.linalg.cholesky(S), z - H @ xe))
                P -= W.T @ W
                e.set_P(P)
            if k in (1, 16):
                rec["host_route"] = {"call_ms": clocked(host_route, 3)}
                rec["host_over_dense"] = rec["host_route"]["call_ms"]["median"] / rec["dense"]["call_ms"]["median"]
        out["legs"].append(rec)
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
        rec = {"metric": "ekf_observe_dense of k dense rows: host clock from the call to a stream synchronise, every repeat from a reloaded state; "
               "device time of its launches by timing family; beside it ekf_multiply_map of the same rows, the one-pair pass, "
               "ekf_observe_model_joint at ceil(k / 2) pairings and (10 000 landmarks) get_P + NumPy + set_P; medians of the repeats",
               "data": "synthetic", "expectation": "stated, not asserted: one multiply chunk plus one pass plus small launches", "states": parts}
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
