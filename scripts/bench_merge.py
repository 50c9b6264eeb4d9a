#!/usr/bin/env python3
"""Landmark fusion on the device (ekf_constrain_landmarks, ekf_merge_landmarks, ekf_landmark_distance) measured on the two benchmark
states: configs[2]'s (10 000 landmarks, F64 tiles of edge 128, low-rank load) and configs[4]'s starting state (40 000 landmarks,
float tiles of edge 256).  One process per state; every figure is the host clock around one call that ends in a stream
synchronise, the median over repeated calls, each from a reloaded state.

Legs of the new entry points (--legs new): the whole ekf_constrain_landmarks call; the whole ekf_merge_landmarks call for a `drop`
near the front, in the middle and near the end; ekf_landmark_distance; and, at 10 000 landmarks, the only route a caller had before
(ekf_get_P -> NumPy -> ekf_set_x / ekf_set_s / ekf_set_P).

Baseline legs (both modes): one ekf_correct at batch = 1, whole call; one ekf_remove_landmarks of the same `drop`, whole call.  The
yardstick is the PARENT commit: run `--legs baseline --lib <the parent's libekfslam.so> --commit <its hash>` once -- that mode binds
nothing but what the parent exports and refuses a library that has the new symbols -- and hand its output to the run of the new
legs with --baseline-json; both sets of figures go into the JSON, labelled by commit, with the ratios

    constrain / parent's correct            merge / (parent's correct + parent's removal of the same drop)

    python scripts/bench_merge.py --state 10k|40k [--legs new|baseline] [--lib FILE] [--commit LABEL] [--baseline-json FILE]
                                  [--skip-round-trip] [--reps K] [--out FILE]
    python scripts/bench_merge.py --combine A.json B.json ... --out profiles/merge_landmarks.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ekf_constrain_landmarks", "ekf_merge_landmarks", "ekf_landmark_distance")
STATES = {"10k": ("configs[2]", 10000, "f64", 128, 20260104), "40k": ("configs[4] start", 40000, "f32", 256, 20260106)}
R_MERGE = np.array([[0.02, 0.005], [0.005, 0.03]])
KEEP = 40


def median(v):
    return float(sorted(v)[len(v) // 2])


def timed(e, fn):
    e.sync()
    t0 = time.perf_counter()
    fn()
    e.sync()
    return (time.perf_counter() - t0) * 1e3


def measure_state(key, legs, reps, round_trip):
    import bench
    from ekf_slam_amd import Engine
    name, N, storage, tile, seed = STATES[key]
    world, x, s, d, U = bench.make_state(N, seed)
    steps = bench.make_steps(world, N, 4, [.01, 5.0])
    drops = {"near_front": 3, "middle": N // 2, "near_end": N - 4}
    e = Engine(capacity=N, tile=tile, storage=storage, batch=1)

    def load(drop=None):
        xx = np.array(x)
        if drop is not None:                       # a duplicate as a SLAM run produces it: `drop` within 0.1 of `keep`
            xx[3 + 2 * drop:5 + 2 * drop] = xx[3 + 2 * KEEP:5 + 2 * KEEP] + np.array([0.05, -0.03])
        e.load_lowrank_state(xx, s, d, U)
        e.sync()

    load()
    first_removal_ms = timed(e, lambda: e.remove_landmarks([N - 1]))      # allocates the second tile store: timed apart
    n = 3 + 2 * N
    w_bytes = 8 if storage == "f64" else 4
    out = {"state": name, "landmarks": N, "storage": storage, "tile": int(e.cfg.tile), "reps": reps,
           "one_pass_algorithmic_bytes": w_bytes * n * (n + 1), "first_removal_ms_with_store_allocation": first_removal_ms}
    # ---- baseline legs: a correction at batch 1, a removal of each drop
    u, z, R, k = steps[0]
    load(); e.predict(u); e.correct(z, R, k); e.sync()                   # warm-up of every kernel the timed calls launch
    t = []
    for _ in range(reps):
        load()
        t.append(timed(e, lambda: e.correct(z, R, k)))
    out["correct_batch1_ms"] = {"median": median(t), "all": t, "pass_kernel": e.downdate_kernel_name()[0]}
    out["remove_ms"] = {}
    for cname, drop in drops.items():
        t = []
        for _ in range(reps):
            load(drop)
            t.append(timed(e, lambda: e.remove_landmarks([drop])))
        out["remove_ms"][cname] = {"drop": drop, "median": median(t), "all": t}
    if legs == "baseline":
        e.close()
        return out
    # ---- the new entry points
    ci, cj = KEEP, N // 2
    delta = (x[3 + 2 * ci:5 + 2 * ci] - x[3 + 2 * cj:5 + 2 * cj]) + np.array([0.05, -0.03])
    load(); e.constrain_landmarks(ci, cj, delta, R_MERGE); e.sync()       # warm-up
    t = []
    for _ in range(reps):
        load()
        t.append(timed(e, lambda: e.constrain_landmarks(ci, cj, delta, R_MERGE)))
    out["constrain_ms"] = {"pair": [ci, cj], "median": median(t), "all": t, "pass_kernel": e.downdate_kernel_name()[0]}
    out["merge_ms"] = {}
    for cname, drop in drops.items():
        t = []
        for _ in range(reps):
            load(drop)
            t.append(timed(e, lambda: e.merge_landmarks(KEEP, drop, R_MERGE)))
            assert e.N == N - 1
        out["merge_ms"][cname] = {"keep": KEEP, "drop": drop, "median": median(t), "all": t}
    t = []
    for _ in range(reps):
        load(drops["middle"])
        t.append(timed(e, lambda: e.landmark_distance(KEEP, drops["middle"], None, R_MERGE)))
    out["distance_ms"] = {"median": median(t), "all": t}
    if round_trip:
        # what a caller could do before, on the same state: the whole covariance over PCIe, the update in NumPy, and back
        drop = drops["middle"]
        load(drop)
        dev_ms = out["merge_ms"]["middle"]["median"]
        t0 = time.perf_counter()
        xs, ss, P = e.get_x(), e.get_s(), e.get_P()
        t_get = time.perf_counter() - t0
        ai, aj = 3 + 2 * KEEP, 3 + 2 * drop
        G = P[ai:ai + 2, :] - P[aj:aj + 2, :]
        S = G[:, ai:ai + 2] - G[:, aj:aj + 2] + R_MERGE
        K = G.T @ np.linalg.inv(S)
        xs = xs + K @ (-(xs[ai:ai + 2] - xs[aj:aj + 2]))
        P -= K @ G
        ent = [aj, aj + 1]
        x2, s2, P2 = np.delete(xs, ent), np.delete(ss, drop), np.delete(np.delete(P, ent, axis=0), ent, axis=1)
        t_np = time.perf_counter() - t0 - t_get
        e.set_state(x2, P2, s2)
        e.sync()
        total = time.perf_counter() - t0
        out["host_round_trip"] = {"get_s": t_get, "numpy_s": t_np, "set_s": total - t_get - t_np, "total_s": total,
                                  "pcie_bytes": 2 * 8 * n * n, "device_merge_ms": dev_ms, "round_trip_over_device_merge": total * 1e3 / dev_ms}
    e.close()
    return out


def with_ratios(new, base):
    """The issue's expectation, stated as ratios against the PARENT's figures: constrain <= 1.25 x correction, merge <= 1.25 x
    (correction + removal of the same drop), whole calls."""
    corr = base["correct_batch1_ms"]["median"]
    r = {"constrain_over_parent_correct": new["constrain_ms"]["median"] / corr, "merge_over_parent_correct_plus_remove": {}}
    for cname, m in new["merge_ms"].items():
        r["merge_over_parent_correct_plus_remove"][cname] = m["median"] / (corr + base["remove_ms"][cname]["median"])
    r["expectation"] = "both <= 1.25 (an expectation, not an assertion)"
    r["met"] = r["constrain_over_parent_correct"] <= 1.25 and all(v <= 1.25 for v in r["merge_over_parent_correct_plus_remove"].values())
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--state", choices=sorted(STATES))
    ap.add_argument("--legs", choices=["new", "baseline"], default="new")
    ap.add_argument("--lib", help="the libekfslam.so to measure (default: the tree's)")
    ap.add_argument("--commit", default="working tree", help="label of the code the library was built from")
    ap.add_argument("--baseline-json", help="output of a --legs baseline run of the same state on the parent commit")
    ap.add_argument("--skip-round-trip", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--combine", nargs="+", help="per-state outputs to join into one record")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    if args.combine:
        rec = {"metric": "ekf_constrain_landmarks / ekf_merge_landmarks / ekf_landmark_distance: whole calls (host clock to stream "
               "synchronise, median of repeated calls from a reloaded state) against the parent commit's correction and removal",
               "data": "synthetic", "states": [json.load(open(p)) for p in args.combine]}
    else:
        if args.lib:
            os.environ["EKF_LIB_PATH"] = os.path.abspath(args.lib)
        sys.path.insert(0, ROOT)
        from ekf_slam_amd import _lib
        if args.legs == "baseline":
            # the parent's library exports none of the new entry points: bind what it has, and make sure it IS such a library
            import ctypes
            raw = ctypes.CDLL(_lib.LIB_PATH)
            assert not any(hasattr(raw, n) for n in NEW_SYMBOLS), "--legs baseline wants a library WITHOUT the new entry points"
            for n in NEW_SYMBOLS:
                _lib.SIGNATURES.pop(n)
        res = measure_state(args.state, args.legs, args.reps, args.state == "10k" and not args.skip_round_trip)
        rec = {"commit": args.commit, "library": os.path.basename(_lib.LIB_PATH), "legs": args.legs, **res}
        if args.baseline_json:
            base = json.load(open(args.baseline_json))
            assert base["landmarks"] == res["landmarks"] and base["storage"] == res["storage"]
            rec = {"state": res["state"], "landmarks": res["landmarks"], "storage": res["storage"], "tile": res["tile"],
                   "parent": base, "this_change": rec, "ratios": with_ratios(res, base)}
    line = json.dumps(rec)
    print(line, flush=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
