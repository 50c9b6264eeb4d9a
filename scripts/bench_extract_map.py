#!/usr/bin/env python3
"""ekf_extract_map measured on the state of profiles/linear_obs.json's configs[2] (10 000 landmarks, F64 tiles of edge 128, low-rank load):
m = 100 and m = 1 000 landmarks taken out into an F64 handle of tile edge 128, in both frames, with the index list as an ascending run and
shuffled.  Every figure is a median of the repeats, each from a RELOADED source state, with the spread (max - min) / median between the
repeats beside it.  Reported, not asserted.

Per (m, frame, list):
  call_us      the whole call, host clock, its waits included (the call synchronises both handles)
  launches_us  device time of its two launches under the source's EKF_KERNEL_COMPACT timer: k_extract_state and k_extract_rows
  rows_us      launches_us - state_us, k_extract_rows' share, where state_us is the same timer for m = 0 (k_extract_state alone, one
               workgroup; at m = 1 000 it runs eight, so the subtraction flatters k_extract_rows by well under a microsecond)
  bytes        what k_extract_rows writes (every tile of the destination's active tile rows, diagonal tiles whole) plus the m (2 m + 1)
               entries it reads, against rows_us
The yardsticks, in the same process on the same state:
  host_route   (m = 100, map frame, ascending run) ekf_get_x / _s / _P, the selection in NumPy, ekf_set_x / _s / _P on the destination
  join_rows    k_join_rows for a local map of the same M joined into the 10 000: 8 (2M 2N + M (2M + 1)) bytes of an almost pure write
               stream (scripts/bench_join_map.py's figure, measured here again), as the per-byte comparison

    python scripts/bench_extract_map.py [--reps 7] [--landmarks 10000] --out profiles/extract_map.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (100, 1000)
TILE = 128
HBM_BYTES_PER_S = 8.0e12


def median(v):
    return float(sorted(v)[len(v) // 2])


def figure(v):
    return {"median": median(v), "spread": float((max(v) - min(v)) / median(v)) if median(v) else 0.0, "all": v}


def index_lists(N, m):
    """an ascending run in the middle of the map, and the same count of landmarks drawn from the whole map in random order"""
    a = (N - m) // 2
    return {"run": list(range(a, a + m)), "shuffled": [int(i) for i in np.random.default_rng(m).permutation(N)[:m]]}


def rows_bytes(m):
    nt = (2 * m + TILE - 1) // TILE
    written = 8 * TILE * TILE * nt * (nt + 1) // 2
    return written, 8 * m * (2 * m + 1)


def measure(N, reps):
    import bench
    from ekf_slam_amd import Engine, _lib
    world, x, s, d, U = bench.make_state(N, 20260104)
    g = Engine(capacity=N + max(SIZES), tile=TILE, storage="f64", batch=1)
    dst = Engine(capacity=max(SIZES), tile=TILE, storage="f64")
    out = {"state": "configs[2]", "landmarks": N, "storage": "f64", "tile": TILE, "reps": reps, "hbm_bytes_per_s": HBM_BYTES_PER_S, "extract": {}}

    def reload():
        g.load_lowrank_state(x, s, d, U)
        g.sync()

    def timed(which, fn, want):
        g.timing_enable(which, True, 64)
        g.timing_read(which)
        fn()
        launches, ms = g.timing_read(which)
        g.timing_enable(which, False)
        assert launches == want, (launches, want)
        return 1e3 * ms

    def leg(fn, which, launches, check):
        reload(); fn()                                        # warm-up: every kernel the timed calls launch
        call, dev = [], []
        for _ in range(reps):
            reload()
            t0 = time.perf_counter()
            fn()
            call.append((time.perf_counter() - t0) * 1e6)
            check()
        rec = {"call_us": figure(call)}
        if launches is not None:
            for _ in range(reps):
                reload()
                dev.append(timed(which, fn, launches))
            rec.update(launches_us=figure(dev), launches=launches)
        return rec

    out["state_us"] = leg(lambda: g.extract_map([], "map", into=dst), _lib.EKF_KERNEL_COMPACT, 1, lambda: None)["launches_us"]
    empty = Engine(capacity=1, storage="f64")
    empty.set_x([0.0, 0.0, 0.0]); empty.set_P(np.zeros((3, 3)))
    out["join_state_us"] = leg(lambda: g.join_map(empty), _lib.EKF_KERNEL_APPEND, 1, lambda: None)["launches_us"]
    for m in SIZES:
        written, read = rows_bytes(m)
        rec = {"bytes_rows_written": written, "bytes_rows_read": read}
        for name, idx in index_lists(N, m).items():
            for frame in ("map", "robot"):
                def check():
                    assert dst.N == m and g.N == N
                r = leg(lambda: g.extract_map(idx, frame, into=dst), _lib.EKF_KERNEL_COMPACT, 2, check)
                rows_us = r["launches_us"]["median"] - out["state_us"]["median"]
                r["rows_us"] = rows_us
                r["rows_bytes_per_s"] = (written + read) / (rows_us * 1e-6) if rows_us > 0 else None
                r["rows_over_floor"] = rows_us / (1e6 * (written + read) / HBM_BYTES_PER_S)
                rec["%s_%s" % (frame, name)] = r
        # the yardsticks
        run = index_lists(N, m)["run"]
        if m == 100:
            sel = np.concatenate([[0, 1, 2]] + [[3 + 2 * l, 4 + 2 * l] for l in run]).astype(int)

            def host_route():
                xs, ss, Ps = g.get_x(), g.get_s(), g.get_P()
                dst.set_x(xs[sel]); dst.set_s(ss[run]); dst.set_P(Ps[np.ix_(sel, sel)])
            rec["host_route"] = leg(host_route, None, None, lambda: None)
            rec["call_over_host_route"] = rec["map_run"]["call_us"]["median"] / rec["host_route"]["call_us"]["median"]
        g.extract_map(run, "robot", into=dst)                 # a local map of the same M for the join: q = 0, PL_qq = 0, PL(q, .) = 0
        jr = leg(lambda: g.join_map(dst), _lib.EKF_KERNEL_APPEND, 2, lambda: None)
        join_bytes = 8 * (2 * m * 2 * N + m * (2 * m + 1))
        jrows = jr["launches_us"]["median"] - out["join_state_us"]["median"]
        jr.update(rows_us=jrows, bytes_rows_written=join_bytes, rows_bytes_per_s=join_bytes / (jrows * 1e-6) if jrows > 0 else None)
        rec["join_rows"] = jr
        out["extract"][str(m)] = rec
    out["dst_device_bytes"] = dst.device_bytes()
    empty.close()
    dst.close()
    g.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--landmarks", type=int, default=10000)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    rec = {"metric": "ekf_extract_map of m landmarks out of 10 000 into an F64 handle (host clock of the whole synchronising call; device time of its "
           "two launches under EKF_KERNEL_COMPACT), medians of the repeats, each from a reloaded state", "data": "synthetic",
           "expectation": "tens of microseconds whatever N is; a shuffled list reads 32-byte pieces and sits well below the ascending run per byte "
           "(an expectation, not an assertion)"}
    rec.update(measure(args.landmarks, args.reps))
    line = json.dumps(rec)
    print(line, flush=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
