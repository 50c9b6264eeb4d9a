#!/usr/bin/env python3
"""A batch of landmark fusions in one call (ekf_merge_landmarks_batch) measured on the two benchmark states: configs[2]'s (10 000
landmarks, F64 tiles of edge 128, low-rank load) and configs[4]'s starting state (40 000 landmarks, float tiles of edge 256).  One
process per state; whole calls are the host clock around one call that ends in a stream synchronise, kernel legs come from the
library's own event timers; every figure is the median over repeated calls, each from a reloaded state.  The first batch call (which
allocates the private pair ring, the snapshot and the second tile store) is timed apart.

Legs of this change (--legs new), for m in {1, 4, 16, 32} planted duplicates:
    the whole ekf_merge_landmarks_batch call; the fused pass alone (EKF_KERNEL_DOWNDATE); the chain of m gathers (EKF_KERNEL_GATHER);
    in the same process: m sequential ekf_merge_landmarks calls, the one-pair pass of ekf_constrain_landmarks (EKF_KERNEL_DOWNDATE)
    and k_compact_tiles for the same drops (EKF_KERNEL_COMPACT of one ekf_remove_landmarks).
Baseline (--legs baseline --lib <the PARENT commit's libekfslam.so> --commit <its hash>): m sequential ekf_merge_landmarks; that mode
binds nothing the parent lacks and refuses a library that has the new symbol.  Hand its output to the run of the new legs with
--baseline-json: both sets go into the JSON, labelled by commit, with the ratios.  Expectations are REPORTED, not asserted.

    python scripts/bench_merge_batch.py --state 10k|40k [--legs new|baseline] [--lib FILE] [--commit LABEL] [--baseline-json FILE]
                                        [--reps K] [--out FILE]
    python scripts/bench_merge_batch.py --combine A.json B.json ... --out profiles/merge_batch.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOL = "ekf_merge_landmarks_batch"
STATES = {"10k": ("configs[2]", 10000, "f64", 128, 20260104), "40k": ("configs[4] start", 40000, "f32", 256, 20260106)}
R_MERGE = np.array([[0.02, 0.005], [0.005, 0.03]])
MS = (1, 4, 16, 32)


def median(v):
    return float(sorted(v)[len(v) // 2])


def timed(e, fn):
    e.sync()
    t0 = time.perf_counter()
    fn()
    e.sync()
    return (time.perf_counter() - t0) * 1e3


def pairs_for(N, m):
    """m (keep, drop): keeps in the front third, drops spread over the back half (distinct; no keep is dropped)"""
    return [(40 + 101 * k, N // 2 + 1 + (N // 2 - 8) // 32 * k) for k in range(m)]


def measure_state(key, legs, reps):
    import bench
    from ekf_slam_amd import Engine
    from ekf_slam_amd import _lib as L
    name, N, storage, tile, seed = STATES[key]
    world, x, s, d, U = bench.make_state(N, seed)
    e = Engine(capacity=N, tile=tile, storage=storage, batch=1)
    allp = pairs_for(N, max(MS))
    xx = np.array(x)
    for k, (kp, dr) in enumerate(allp):            # duplicates as a SLAM run produces them: each drop within 0.1 of its keep
        xx[3 + 2 * dr:5 + 2 * dr] = xx[3 + 2 * kp:5 + 2 * kp] + np.array([0.05, -0.03]) * (1.0 + 0.02 * k)

    def load():
        e.load_lowrank_state(xx, s, d, U)
        e.sync()

    def sequential(pairs):
        gone = []
        for kp, dr in pairs:                       # each merge renumbers: the indices as they are when the merge is made
            e.merge_landmarks(kp - sum(g < kp for g in gone), dr - sum(g < dr for g in gone), R_MERGE)
            gone.append(dr)

    n = 3 + 2 * N
    w_bytes = 8 if storage == "f64" else 4
    out = {"state": name, "landmarks": N, "storage": storage, "tile": int(e.cfg.tile), "reps": reps,
           "one_pass_algorithmic_bytes": w_bytes * n * (n + 1)}
    load()
    out["first_merge_ms_with_allocations"] = timed(e, lambda: sequential(allp[:1]))
    out["sequential_merges_ms"] = {}
    for m in MS:
        t = []
        for _ in range(reps):
            load()
            t.append(timed(e, lambda: sequential(allp[:m])))
            assert e.N == N - m
        out["sequential_merges_ms"][str(m)] = {"median": median(t), "all": t}
    if legs == "baseline":
        e.close()
        return out
    load()
    out["first_batch_ms_with_allocations"] = timed(e, lambda: e.merge_landmarks_batch(allp[:1], R_MERGE))
    out["batch_ms"], out["fused_pass_ms"], out["chain_ms"] = {}, {}, {}
    for m in MS:
        t = []
        for _ in range(reps):
            load()
            t.append(timed(e, lambda: e.merge_landmarks_batch(allp[:m], R_MERGE)))
            assert e.N == N - m
        out["batch_ms"][str(m)] = {"median": median(t), "all": t, "over_sequential_same_library": median(t) / out["sequential_merges_ms"][str(m)]["median"]}
        tp, tc = [], []
        for which in (L.EKF_KERNEL_DOWNDATE, L.EKF_KERNEL_GATHER):
            e.timing_enable(which, True, 64)
        for _ in range(reps):
            load()
            e.timing_read(L.EKF_KERNEL_DOWNDATE); e.timing_read(L.EKF_KERNEL_GATHER)
            e.merge_landmarks_batch(allp[:m], R_MERGE)
            np_, ms_p = e.timing_read(L.EKF_KERNEL_DOWNDATE)
            ng, ms_g = e.timing_read(L.EKF_KERNEL_GATHER)
            assert (np_, ng) == (1, m)
            tp.append(ms_p); tc.append(ms_g)
        for which in (L.EKF_KERNEL_DOWNDATE, L.EKF_KERNEL_GATHER):
            e.timing_enable(which, False)
        out["fused_pass_ms"][str(m)] = {"median": median(tp), "all": tp, "kernel": e.downdate_kernel_name()[0],
                                        "algorithmic_TB_per_s": out["one_pass_algorithmic_bytes"] / (median(tp) * 1e-3) / 1e12}
        out["chain_ms"][str(m)] = {"median": median(tc), "all": tc, "per_gather": median(tc) / m}
    # beside them, in the same process: the one-pair pass and the compaction of the same drops
    t1, tk = [], {str(m): [] for m in MS}
    e.timing_enable(L.EKF_KERNEL_DOWNDATE, True, 64)
    e.timing_enable(L.EKF_KERNEL_COMPACT, True, 64)
    for _ in range(reps):
        load()
        e.timing_read(L.EKF_KERNEL_DOWNDATE)
        e.constrain_landmarks(allp[0][0], allp[0][1], None, R_MERGE)
        t1.append(e.timing_read(L.EKF_KERNEL_DOWNDATE)[1])
        for m in MS:
            load()
            e.timing_read(L.EKF_KERNEL_COMPACT)
            e.remove_landmarks([dr for _, dr in allp[:m]])
            tk[str(m)].append(e.timing_read(L.EKF_KERNEL_COMPACT)[1])
    e.timing_enable(L.EKF_KERNEL_DOWNDATE, False)
    e.timing_enable(L.EKF_KERNEL_COMPACT, False)
    out["one_pair_pass_ms"] = {"median": median(t1), "all": t1}
    out["compact_tiles_ms"] = {m: {"median": median(v), "all": v, "note": "the rows above the first drop are not compacted (copied, or left in place)"}
                               for m, v in tk.items()}
    out["fused_pass_m1_over_pass_plus_compaction"] = out["fused_pass_ms"]["1"]["median"] / (median(t1) + median(tk["1"]))
    e.close()
    return out


def with_ratios(new, base):
    r = {"batch_over_parent_sequential": {m: new["batch_ms"][m]["median"] / base["sequential_merges_ms"][m]["median"] for m in new["batch_ms"]},
         "fused_pass_growth_m32_over_m1": new["fused_pass_ms"]["32"]["median"] / new["fused_pass_ms"]["1"]["median"],
         "fused_pass_m1_over_pass_plus_compaction": new["fused_pass_m1_over_pass_plus_compaction"],
         "expectations": "fused pass at m = 1 <= one-pair pass + compaction; its time grows slowly with m; the whole call at m = 16 far below "
                         "16 of the parent's merges (reported, not asserted)"}
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--state", choices=sorted(STATES))
    ap.add_argument("--legs", choices=["new", "baseline"], default="new")
    ap.add_argument("--lib", help="the libekfslam.so to measure (default: the tree's)")
    ap.add_argument("--commit", default="working tree", help="label of the code the library was built from")
    ap.add_argument("--baseline-json", help="output of a --legs baseline run of the same state on the parent commit")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--combine", nargs="+", help="per-state outputs to join into one record")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    if args.combine:
        rec = {"metric": "ekf_merge_landmarks_batch: whole calls (host clock to stream synchronise) and kernel legs (event timers), medians of "
               "repeated calls from a reloaded state, against m sequential ekf_merge_landmarks of the parent commit",
               "data": "synthetic", "states": [json.load(open(p)) for p in args.combine]}
    else:
        if args.lib:
            os.environ["EKF_LIB_PATH"] = os.path.abspath(args.lib)
        sys.path.insert(0, ROOT)
        from ekf_slam_amd import _lib
        if args.legs == "baseline":
            import ctypes
            raw = ctypes.CDLL(_lib.LIB_PATH)
            assert not hasattr(raw, NEW_SYMBOL), "--legs baseline wants a library WITHOUT " + NEW_SYMBOL
            _lib.SIGNATURES.pop(NEW_SYMBOL)
        res = measure_state(args.state, args.legs, args.reps)
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
