#!/usr/bin/env python3
"""ekf_factor_map measured on low-rank loaded states: 10 000 landmarks on F64 tiles of edge 128 and 40 000 landmarks on float tiles of
edge 256.  Every figure is a median of the repeats, each from a RELOADED state, with the spread (max - min) / median between the repeats
beside it.  Reported, not asserted; no ratio is fixed in advance.

Per state:
  call_us        the whole call with one reference state, host clock, its waits included (the call synchronises)
  families       device time of its launches by family, each family timed in runs of its own: `setup` (k_factor_load, k_factor_rhs,
                 k_factor_finish; EKF_KERNEL_COMPACT), `diag_panel` (k_factor_diag and k_factor_panel, one count per tile column;
                 EKF_KERNEL_GATHER), `trail` (k_factor_trail, the F64 matrix cores; EKF_KERNEL_DOWNDATE)
  flops_per_s    n^3 / 3 over the sum of the three families, beside the project's own measured F64 MFMA rate (44-48 TFLOP/s,
                 scripts/probes/mfma_f64_rate.hip)
  trail_bytes    every tile of every trailing update read once and written once (its two operand tiles are re-read by a whole tile row
                 or column of workgroups and are not counted); at_pass_rate_us: the time those bytes take at the rate of ...
  one_pair_pass  the handle's pass over P for one pending pair (EKF_KERNEL_DOWNDATE, cfg.batch = 1), measured in the same run
The yardstick at 10 000 landmarks, in the same process on the same state: host_route, ekf_get_P + numpy.linalg.cholesky with the host
pool capped at 16 threads.  At 40 000 landmarks the host route would need a 51 GB dense matrix and is skipped; the large state is
repeated --reps-large times (a call takes seconds) and its families are timed in ONE run each.

    python scripts/bench_factor_map.py [--reps 7] [--reps-large 3] --out profiles/factor_map.json
"""
import argparse
import json
import os
import sys
import time

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = str(min(16, int(os.environ.get(_v, "16") or 16)))

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATES = ((10000, 128, "f64", 8, True), (40000, 256, "f32", 4, False))
TF = 64                                                       # the factor store's tile edge (launch/map_sizes.h: kFactorTile)
MFMA_F64_RATE = "44-48 TFLOP/s (scripts/probes/mfma_f64_rate.hip)"


def median(v):
    return float(sorted(v)[len(v) // 2])


def figure(v):
    return {"median": median(v), "spread": float((max(v) - min(v)) / median(v)) if median(v) else 0.0, "all": v}


def measure(N, tile, storage, elt, small, reps, host_reps):
    import bench
    from ekf_slam_amd import Engine, _lib
    world, x, s, d, U = bench.make_state(N, 20260104)
    g = Engine(capacity=N, tile=tile, storage=storage, batch=1)
    n = 3 + 2 * N
    nF = (2 * N + TF - 1) // TF
    nt = (2 * N + tile - 1) // tile
    store = elt * tile * tile * nt * (nt + 1) // 2
    trail_tiles = sum((nF - 1 - k) * (nF - k) // 2 for k in range(nF))
    out = {"landmarks": N, "storage": storage, "tile": tile, "factor_tile": TF, "n": n, "store_bytes": store,
           "factor_store_bytes": 8 * TF * TF * nF * (nF + 1) // 2, "trail_bytes": 2 * 8 * TF * TF * trail_tiles, "flops": n ** 3 / 3.0}
    ref = x + 0.01

    def reload():
        g.load_lowrank_state(x, s, d, U)
        g.sync()

    reload()
    info = g.factor_map(ref)                                  # warm-up: every kernel, the factor store's allocation
    out["info"] = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in info.items()}
    call = []
    for _ in range(reps):
        reload()
        t0 = time.perf_counter()
        g.factor_map(ref)
        call.append((time.perf_counter() - t0) * 1e6)
    out["call_us"] = figure(call)
    fam = {}
    for name, which, launches in (("setup", _lib.EKF_KERNEL_COMPACT, 2), ("diag_panel", _lib.EKF_KERNEL_GATHER, nF),
                                  ("trail", _lib.EKF_KERNEL_DOWNDATE, nF - 1)):
        dev = []
        for _ in range(reps if small else 1):
            reload()
            g.timing_enable(which, True, 2 * nF + 64)
            g.timing_read(which)
            g.factor_map(ref)
            cnt, ms = g.timing_read(which)
            g.timing_enable(which, False)
            assert cnt == launches, (name, cnt, launches)
            dev.append(1e3 * ms)
        fam[name] = dict(figure(dev), launches=launches)
    out["families"] = fam
    total_us = sum(f["median"] for f in fam.values())
    out["device_us"] = total_us
    out["flops_per_s"] = out["flops"] / (total_us * 1e-6)
    out["mfma_f64_rate_measured_here"] = MFMA_F64_RATE
    # the one-pair pass over the handle's own store, in the same run
    dxy = x[3 + 2 * 7:5 + 2 * 7] - x[0:2]
    z = [float(np.hypot(*dxy)), float(np.degrees(np.arctan2(dxy[1], dxy[0])) - x[2])]
    u, R = [0.1, 1.0], np.diag([0.1, 0.2])
    dev = []
    for _ in range(reps + 1):
        reload()
        g.timing_enable(_lib.EKF_KERNEL_DOWNDATE, True, 64)
        g.timing_read(_lib.EKF_KERNEL_DOWNDATE)
        g.predict(u); g.correct(z, R, 7); g.flush(); g.sync()
        cnt, ms = g.timing_read(_lib.EKF_KERNEL_DOWNDATE)
        g.timing_enable(_lib.EKF_KERNEL_DOWNDATE, False)
        assert cnt == 1, cnt
        dev.append(1e3 * ms)
    dev = dev[1:]                                             # (the first is the warm-up)
    pass_rate = 2 * store / (median(dev) * 1e-6)
    out["one_pair_pass"] = dict(figure(dev), bytes=2 * store, bytes_per_s=pass_rate)
    out["trail_at_pass_rate_us"] = out["trail_bytes"] / pass_rate * 1e6
    out["trail_over_its_bytes_at_pass_rate"] = fam["trail"]["median"] / out["trail_at_pass_rate_us"]
    if small:
        host, chol = [], []
        for _ in range(host_reps):
            reload()
            t0 = time.perf_counter()
            P = g.get_P()
            t1 = time.perf_counter()
            L = np.linalg.cholesky(P)
            host.append((time.perf_counter() - t0) * 1e6)
            chol.append((time.perf_counter() - t1) * 1e6)
        out["host_route"] = {"get_P_plus_cholesky_us": figure(host), "cholesky_alone_us": figure(chol), "threads": os.environ["OMP_NUM_THREADS"],
                             "logdet": float(2.0 * np.sum(np.log(np.diag(L))))}
        out["host_route_over_call"] = out["host_route"]["get_P_plus_cholesky_us"]["median"] / out["call_us"]["median"]
        del P, L
    else:
        out["host_route"] = "skipped: the dense matrix of %d landmarks is %.0f GB" % (N, 8.0 * n * n / 1e9)
    g.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--reps-large", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--states", default="small,large")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    rec = {"metric": "ekf_factor_map, the Cholesky factorisation of P on the device (host clock of the whole synchronising call with one "
           "reference state; device time of its launches by family), medians of the repeats, each from a reloaded state",
           "data": "synthetic", "reps": args.reps, "reps_large": args.reps_large, "host_reps": args.host_reps,
           "factor_tile": "64 is the one edge that is built; 128 was not measured", "states": []}
    for N, tile, storage, elt, small in STATES:
        if ("small" if small else "large") not in args.states.split(","):
            continue
        rec["states"].append(measure(N, tile, storage, elt, small, args.reps if small else args.reps_large, args.host_reps))
        print(json.dumps(rec["states"][-1]), flush=True)
        with open(args.out, "w") as fh:                       # (written after each state: the large one takes minutes)
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
