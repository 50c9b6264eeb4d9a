#!/usr/bin/env python3
"""The candidate search in front of a merge (ekf_nearest_landmarks) measured on the two benchmark states: configs[2]'s (10 000
landmarks, F64 tiles of edge 128, low-rank load) and configs[4]'s starting state (40 000 landmarks, float tiles of edge 256).  One
process per state; medians over repeated calls.

Per state:
  * the kernel (k_nearest) from the EKF_KERNEL_ASSOCIATE timer -- a known-correspondence handle launches nothing else under it;
  * the whole ekf_nearest_landmarks call, host clock to return (the call ends in a stream synchronisation);
  * IN THE SAME PROCESS the one-pair pass on that state (k_downdate_w through EKF_KERNEL_DOWNDATE, one ekf_correct at batch 1): the
    yardstick -- code this change does not touch.  The search reads the stored lower triangle once, w n_mm (n_mm + 1) / 2 bytes, half of
    what the pass moves (it reads AND writes every entry): the ideal is half the pass's time, the bar "no longer than the pass";
  * at 10 000 landmarks the route a caller had before: ekf_get_P, then a block-wise NumPy search.
The expectation is stated, not asserted.

    python scripts/bench_nearest.py --state 10k|40k [--reps K] [--skip-host-route] --out FILE
    python scripts/bench_nearest.py --combine A.json B.json --out profiles/nearest_landmarks.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATES = {"10k": ("configs[2]", 10000, "f64", 128, 20260104), "40k": ("configs[4] start", 40000, "f32", 256, 20260106)}
R_MERGE = np.array([[0.02, 0.005], [0.005, 0.03]])
HBM_PEAK = 8.0e12               # B/s, as bench.py


def median(v):
    return float(sorted(v)[len(v) // 2])


def numpy_search(x, P, R, block=256):
    """The search a caller could run on the host from ekf_get_x / ekf_get_P, block-wise over rows (lower triangle, lowest j wins)."""
    N = (x.size - 3) // 2
    L = x[3:].reshape(N, 2)
    own = np.stack([P[3 + 2 * np.arange(N) + a, 3 + 2 * np.arange(N) + b] for a in range(2) for b in range(2)], axis=1).reshape(N, 2, 2)
    d2, partner = np.full(N, np.inf), np.full(N, -1, dtype=np.int64)
    for r0 in range(0, N, block):
        r1 = min(r0 + block, N)
        C = P[3 + 2 * r0:3 + 2 * r1, 3:3 + 2 * r1].reshape(r1 - r0, 2, r1, 2).transpose(0, 2, 1, 3)
        S = own[r0:r1, None] + own[None, :r1] - C - C.transpose(0, 1, 3, 2) + R
        nu = L[None, :r1] - L[r0:r1, None]
        det = S[..., 0, 0] * S[..., 1, 1] - S[..., 0, 1] * S[..., 1, 0]
        with np.errstate(divide="ignore", invalid="ignore"):
            D = (nu[..., 0] ** 2 * S[..., 1, 1] - nu[..., 0] * nu[..., 1] * (S[..., 0, 1] + S[..., 1, 0]) + nu[..., 1] ** 2 * S[..., 0, 0]) / det
        D[~((S[..., 0, 0] > 0) & (det > 0)) | np.isnan(D) | (np.arange(r1)[None, :] >= np.arange(r0, r1)[:, None])] = np.inf
        j = np.argmin(D, axis=1)
        best = D[np.arange(r1 - r0), j]
        d2[r0:r1] = best
        partner[r0:r1] = np.where(np.isfinite(best), j, -1)
    return d2, partner


def measure_state(key, reps, host_route):
    import bench
    from ekf_slam_amd import Engine
    from ekf_slam_amd import _lib as L
    name, N, storage, tile, seed = STATES[key]
    world, x, s, d, U = bench.make_state(N, seed)
    steps = bench.make_steps(world, N, reps + 2, [.01, 5.0])
    e = Engine(capacity=N, tile=tile, storage=storage, batch=1)
    e.load_lowrank_state(x, s, d, U)
    e.sync()
    w_bytes = 8 if storage == "f64" else 4
    n_mm = 2 * N
    search_bytes = w_bytes * n_mm * (n_mm + 1) // 2
    pass_bytes = e.downdate_algorithmic_bytes()
    out = {"state": name, "landmarks": N, "storage": storage, "tile": int(e.cfg.tile), "reps": reps,
           "search_algorithmic_bytes": search_bytes, "one_pair_pass_algorithmic_bytes": pass_bytes}
    # ---- the yardstick: the one-pair pass on this state
    e.timing_enable(L.EKF_KERNEL_DOWNDATE, True, 4)
    u, z, R, k = steps[0]
    e.predict(u); e.correct(z, R, k); e.sync()               # warm-up
    e.timing_read(L.EKF_KERNEL_DOWNDATE)
    t = []
    for u, z, R, k in steps[1:reps + 1]:
        e.predict(u); e.correct(z, R, k)
        n, ms = e.timing_read(L.EKF_KERNEL_DOWNDATE)
        assert n == 1
        t.append(ms)
    pass_ms = median(t)
    out["one_pair_pass_kernel_ms"] = {"median": pass_ms, "all": t, "kernel": e.downdate_kernel_name()[0],
                                      "roofline_frac": pass_bytes / (pass_ms * 1e-3) / HBM_PEAK}
    e.timing_enable(L.EKF_KERNEL_DOWNDATE, False)
    # ---- the search
    e.timing_enable(L.EKF_KERNEL_ASSOCIATE, True, 4)
    got = e.nearest_landmarks(R_MERGE)                       # warm-up (allocates the result buffers)
    e.timing_read(L.EKF_KERNEL_ASSOCIATE)
    tk, tc = [], []
    for _ in range(reps):
        e.sync()
        t0 = time.perf_counter()
        e.nearest_landmarks(R_MERGE)
        tc.append((time.perf_counter() - t0) * 1e3)
        n, ms = e.timing_read(L.EKF_KERNEL_ASSOCIATE)
        assert n == 1
        tk.append(ms)
    k_ms = median(tk)
    out["nearest_kernel_ms"] = {"median": k_ms, "all": tk, "roofline_frac": search_bytes / (k_ms * 1e-3) / HBM_PEAK,
                                "achieved_GBps": search_bytes / (k_ms * 1e-3) / 1e9}
    out["nearest_call_ms"] = {"median": median(tc), "all": tc}
    out["kernel_over_one_pair_pass"] = k_ms / pass_ms
    out["expectation"] = "ideal 0.5 (half the bytes of the pass); the bar: <= 1.0 (stated, not asserted)"
    out["bar_met"] = k_ms <= pass_ms
    if host_route:
        t0 = time.perf_counter()
        xs, P = e.get_x(), e.get_P()
        t_get = time.perf_counter() - t0
        want = numpy_search(xs, P, R_MERGE)
        total = time.perf_counter() - t0
        n = 3 + 2 * N
        out["host_route"] = {"get_s": t_get, "numpy_s": total - t_get, "total_s": total, "pcie_bytes": 8 * n * n,
                             "over_device_call": total * 1e3 / median(tc), "partners_equal": bool((want[1] == got[1]).all()),
                             "max_rel_diff_d2": float(np.abs(got[0][1:] / want[0][1:] - 1.0).max())}
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--state", choices=sorted(STATES))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip-host-route", action="store_true")
    ap.add_argument("--combine", nargs="+", help="per-state outputs to join into one record")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    if args.combine:
        rec = {"metric": "ekf_nearest_landmarks: k_nearest (EKF_KERNEL_ASSOCIATE timer) and the whole call against the one-pair pass "
               "(k_downdate_w, EKF_KERNEL_DOWNDATE timer) measured in the same process on the same state; medians",
               "data": "synthetic", "states": [json.load(open(p)) for p in args.combine]}
    else:
        sys.path.insert(0, ROOT)
        rec = measure_state(args.state, args.reps, args.state == "10k" and not args.skip_host_route)
    line = json.dumps(rec)
    print(line, flush=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
