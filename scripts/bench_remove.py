#!/usr/bin/env python3
"""Landmark removal on the device (ekf_remove_landmarks) measured on the two benchmark states: configs[2]'s (10 000 landmarks, F64
tiles of edge 128, low-rank load) and configs[4]'s starting state (40 000 landmarks, float tiles of edge 256).

Per state three removals, each from the freshly loaded state: 1 landmark near the front, 16 spread over the map, 1 near the end.
Per case: the time of k_compact_tiles by HIP events on the engine's stream (EKF_KERNEL_COMPACT), the bytes it moves and the bytes the
device-to-device copy beside it moves, GB/s, and the host time of the whole call up to a stream synchronise.  Held against, in the
same process on the same state: (1) the one-pair pass over P, which moves the same bytes as a compaction from the front, (2) at
10 000 landmarks the only way a caller had before: ekf_get_P -> numpy.delete -> ekf_set_x / ekf_set_s / ekf_set_P.

Prints one JSON line and writes it to --out (default profiles/remove_landmarks.json).

    python scripts/bench_remove.py [--skip-40k] [--skip-round-trip] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def traffic(N, T, w, first):
    """(bytes k_compact_tiles reads + writes, bytes the copy beside it reads + writes) for a removal whose lowest index is `first`:
    the kernel rewrites every tile from the first removed landmark's tile row on; the smaller of the untouched prefix and that
    suffix is copied device to device (ekf_slam_amd/csrc/host/edits.h: ekf_remove_landmarks)."""
    nt = (2 * N + T - 1) // T
    I0 = (2 * first) // T
    prefix = I0 * (I0 + 1) // 2
    suffix = nt * (nt + 1) // 2 - prefix
    tile = T * T * w
    return 2 * suffix * tile, 2 * min(prefix, suffix) * tile


def measure_state(name, N, storage, tile, seed, round_trip):
    from ekf_slam_amd import Engine, _lib as L
    w_bytes = 8 if storage == "f64" else 4
    world, x, s, d, U = bench.make_state(N, seed)
    steps = bench.make_steps(world, N, 8, [.01, 5.0])
    e = Engine(capacity=N, tile=tile, storage=storage, batch=1)

    def load():
        e.load_lowrank_state(x, s, d, U)
        e.sync()

    load()
    t0 = time.perf_counter()
    e.remove_landmarks([N - 1])            # the first removal of a handle allocates the second tile store: timed apart
    e.sync()
    first_call_ms = (time.perf_counter() - t0) * 1e3
    load()
    # (1) the one-pair pass on this state
    e.timing_enable(L.EKF_KERNEL_DOWNDATE, True, launches=16)
    for i, (u, z, R, k) in enumerate(steps):
        if i == 2:
            e.timing_read(L.EKF_KERNEL_DOWNDATE)      # two warm-up passes dropped
        e.predict(u); e.correct(z, R, k)
    e.sync()
    cnt, ms = e.timing_read(L.EKF_KERNEL_DOWNDATE)
    e.timing_enable(L.EKF_KERNEL_DOWNDATE, False)
    pass_ms = ms / cnt
    pass_kernel = e.downdate_kernel_name()[0]
    n = 3 + 2 * N
    pass_bytes = w_bytes * n * (n + 1)
    out = {"state": name, "landmarks": N, "storage": storage, "tile": int(e.cfg.tile),
           "one_pair_pass": {"kernel": pass_kernel, "launches": cnt, "ms": pass_ms, "algorithmic_bytes": pass_bytes,
                             "GBps": pass_bytes / (pass_ms * 1e-3) / 1e9, "hbm_frac": pass_bytes / (pass_ms * 1e-3) / bench.HBM_PEAK},
           "first_call_ms_with_store_allocation": first_call_ms, "device_GB": e.device_bytes() / 1e9, "cases": []}
    cases = [("one_near_front", [3]), ("sixteen_spread", [int(i) for i in np.linspace(37, N - 41, 16)]), ("one_near_end", [N - 4])]
    e.timing_enable(L.EKF_KERNEL_COMPACT, True, launches=16)
    for cname, idx in cases:
        reps = []
        for rep in range(3):
            load()
            e.timing_read(L.EKF_KERNEL_COMPACT)
            t0 = time.perf_counter()
            e.remove_landmarks(idx)
            e.sync()
            host_ms = (time.perf_counter() - t0) * 1e3
            c, kms = e.timing_read(L.EKF_KERNEL_COMPACT)
            assert c == 1 and e.N == N - len(idx)
            reps.append((kms, host_ms))
        kms, host_ms = sorted(reps)[1]                 # the median repetition (by kernel time)
        kb, cb = traffic(N, int(e.cfg.tile), w_bytes, min(idx))
        out["cases"].append({"case": cname, "removed": len(idx), "lowest_index": min(idx),
                             "k_compact_tiles_ms": kms, "kernel_bytes": kb, "kernel_GBps": kb / (kms * 1e-3) / 1e9,
                             "kernel_hbm_frac": kb / (kms * 1e-3) / bench.HBM_PEAK, "copy_bytes": cb,
                             "whole_call_host_ms": host_ms, "whole_call_host_ms_all": [r[1] for r in reps],
                             "k_compact_tiles_ms_all": [r[0] for r in reps],
                             "kernel_over_one_pair_pass": kms / pass_ms, "whole_call_over_one_pair_pass": host_ms / pass_ms})
    e.timing_enable(L.EKF_KERNEL_COMPACT, False)
    if round_trip:
        # (2) what a caller could do before, on the same state: the whole covariance over PCIe and back
        load()
        idx = cases[1][1]
        ent = np.sort(np.concatenate([3 + 2 * np.asarray(idx), 4 + 2 * np.asarray(idx)]))
        t0 = time.perf_counter()
        xs, ss, P = e.get_x(), e.get_s(), e.get_P()
        t_get = time.perf_counter() - t0
        x2, s2 = np.delete(xs, ent), np.delete(ss, idx)
        P2 = np.delete(np.delete(P, ent, axis=0), ent, axis=1)
        t_del = time.perf_counter() - t0 - t_get
        e.set_state(x2, P2, s2)
        e.sync()
        total = time.perf_counter() - t0
        dev = next(c for c in out["cases"] if c["case"] == "sixteen_spread")["whole_call_host_ms"]
        out["host_round_trip"] = {"removed": len(idx), "get_s": t_get, "numpy_delete_s": t_del, "set_s": total - t_get - t_del,
                                  "total_s": total, "pcie_bytes": 2 * 8 * n * n, "device_call_ms": dev,
                                  "round_trip_over_device_call": total * 1e3 / dev}
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-40k", action="store_true")
    ap.add_argument("--skip-round-trip", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "remove_landmarks.json"))
    args = ap.parse_args()
    states = [measure_state("configs[2]", 10000, "f64", 128, 20260104, not args.skip_round_trip)]
    if not args.skip_40k:
        states.append(measure_state("configs[4] start", 40000, "f32", 256, 20260106, False))
    rec = {"metric": "ekf_remove_landmarks: k_compact_tiles time against the one-pair pass; whole call against the host round trip",
           "hbm_peak_GBps": bench.HBM_PEAK / 1e9, "data": "synthetic", "states": states}
    line = json.dumps(rec)
    print(line, flush=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
