#!/usr/bin/env python3
"""ekf_transform_map measured on low-rank loaded states: 10 000 landmarks on F64 tiles of edge 128 and 40 000 landmarks on float tiles of
edge 256.  Every figure is a median of the repeats, each from a RELOADED state, with the spread (max - min) / median between the repeats
beside it.  Reported, not asserted.

Per state and form (exact rigid, uncertain rigid, robot frame):
  call_us      the whole call, host clock, its waits included (the call synchronises)
  launches_us  device time of its two launches under EKF_KERNEL_COMPACT: k_transform_state (one lane per column) and k_transform_tiles
  bytes        every tile of the active tile rows read once and written once; bytes_per_s = bytes / launches_us, so k_transform_state's
               few microseconds count against k_transform_tiles
The yardsticks, in the same process on the same state:
  one_pair_pass  the handle's pass over P for one pending pair (EKF_KERNEL_DOWNDATE, cfg.batch = 1): it streams the same bytes
  join_route     today's rigid route: ekf_join_map of the map into an EMPTY second handle that sits at the transform (EKF_KERNEL_APPEND)
  extract_route  today's robocentric route: ekf_extract_map of all N landmarks in EKF_FRAME_ROBOT into a second handle (EKF_KERNEL_COMPACT)

    python scripts/bench_transform_map.py [--reps 7] --out profiles/transform_map.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATES = ((10000, 128, "f64", 8), (40000, 256, "f32", 4))
T_RIGID = [3.5, -2.25, 37.0]
SIGMA = np.array([[0.04, 0.01, 0.02], [0.01, 0.09, -0.03], [0.02, -0.03, 0.5]])
FORMS = {"exact": ("map", T_RIGID, None), "uncertain": ("map", T_RIGID, SIGMA), "robot": ("robot", None, None)}


def median(v):
    return float(sorted(v)[len(v) // 2])


def figure(v):
    return {"median": median(v), "spread": float((max(v) - min(v)) / median(v)) if median(v) else 0.0, "all": v}


def measure(N, tile, storage, elt, reps):
    import bench
    from ekf_slam_amd import Engine, _lib
    world, x, s, d, U = bench.make_state(N, 20260104)
    g = Engine(capacity=N, tile=tile, storage=storage, batch=1)
    other = Engine(capacity=N, tile=tile, storage=storage)
    nt = (2 * N + tile - 1) // tile
    store = elt * tile * tile * nt * (nt + 1) // 2
    out = {"landmarks": N, "storage": storage, "tile": tile, "store_bytes": store, "bytes": 2 * store}

    def reload():
        g.load_lowrank_state(x, s, d, U)
        g.sync()

    def leg(fn, on, which, launches, before=lambda: None):
        reload(); before(); fn()                              # warm-up: every kernel the timed calls launch
        call, dev = [], []
        for _ in range(reps):
            reload(); before()
            t0 = time.perf_counter()
            fn()
            call.append((time.perf_counter() - t0) * 1e6)
        for _ in range(reps):
            reload(); before()
            on.timing_enable(which, True, 64)
            on.timing_read(which)
            fn()
            n, ms = on.timing_read(which)
            on.timing_enable(which, False)
            assert n == launches, (n, launches)
            dev.append(1e3 * ms)
        rec = {"call_us": figure(call), "launches_us": figure(dev), "launches": launches}
        rec["bytes_per_s"] = 2 * store / (rec["launches_us"]["median"] * 1e-6)
        return rec

    for name, args in FORMS.items():
        out[name] = leg(lambda: g.transform_map(*args), g, _lib.EKF_KERNEL_COMPACT, 2)
    dxy = x[3 + 2 * 7:5 + 2 * 7] - x[0:2]
    z = [float(np.hypot(*dxy)), float(np.degrees(np.arctan2(dxy[1], dxy[0])) - x[2])]
    u, R = [0.1, 1.0], np.diag([0.1, 0.2])

    def one_pair():
        g.predict(u); g.correct(z, R, 7); g.flush(); g.sync()
    out["one_pair_pass"] = leg(one_pair, g, _lib.EKF_KERNEL_DOWNDATE, 1)

    def at_transform():
        other.set_x(T_RIGID); other.set_P(SIGMA)
    out["join_route"] = leg(lambda: other.join_map(g), other, _lib.EKF_KERNEL_APPEND, 2, at_transform)
    every = list(range(N))
    out["extract_route"] = leg(lambda: g.extract_map(every, "robot", into=other), g, _lib.EKF_KERNEL_COMPACT, 2)
    for name in FORMS:
        out[name]["over_one_pair_pass"] = out[name]["launches_us"]["median"] / out["one_pair_pass"]["launches_us"]["median"]
    out["uncertain"]["over_join_route"] = out["uncertain"]["launches_us"]["median"] / out["join_route"]["launches_us"]["median"]
    out["robot"]["over_extract_route"] = out["robot"]["launches_us"]["median"] / out["extract_route"]["launches_us"]["median"]
    other.close()
    g.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    rec = {"metric": "ekf_transform_map of the whole map, in place (host clock of the whole synchronising call; device time of its two launches "
           "under EKF_KERNEL_COMPACT), medians of the repeats, each from a reloaded state", "data": "synthetic", "reps": args.reps,
           "expectation": "HBM-bound like the one-pair pass beside it, which streams the same bytes (an expectation, not an assertion)",
           "states": []}
    for N, tile, storage, elt in STATES:
        rec["states"].append(measure(N, tile, storage, elt, args.reps))
        print(json.dumps(rec["states"][-1]), flush=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
