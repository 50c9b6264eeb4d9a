#!/usr/bin/env python3
"""ekf_join_map measured on the state of profiles/linear_obs.json's configs[2] (10 000 landmarks, F64 tiles of edge 128, low-rank load)
with F64 local maps of M = 100 and M = 1 000 landmarks.  Every figure is a median of the repeats, each from a RELOADED global state, with
the spread (max - min) / median between the repeats beside it.  Reported, not asserted.

Per M:
  call_us      the whole call, host clock, its waits included (the call synchronises both handles)
  launches_us  device time of its two launches under the EKF_KERNEL_APPEND timer: k_join_state and k_join_rows
  state_us     the same for a local map without landmarks (k_join_state alone over the global columns), so that
               rows_us = launches_us - state_us is k_join_rows' share
  roofline     the bytes k_join_rows writes, 8 (2M 2N + M (2M + 1)), against rows_us at 8 TB/s
The yardsticks, in the same process on the same state:
  append_model_x  ceil(M / 32) ekf_append_model calls of RELATIVE_XY entries (z = m_i, R = PL(m_i, m_i)): they write the same old-column
                  region, without the local map's cross-covariances and with the robot left where it is
  host_route      (M = 100 only) ekf_get_P on both handles, the join in NumPy, ekf_set_x / _s / _P

    python scripts/bench_join_map.py [--reps 7] [--landmarks 10000] --out profiles/join_map.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 180.0 / np.pi
LOCAL_SIZES = (100, 1000)
HBM_BYTES_PER_S = 8.0e12


def median(v):
    return float(sorted(v)[len(v) // 2])


def figure(v):
    return {"median": median(v), "spread": float((max(v) - min(v)) / median(v)) if median(v) else 0.0, "all": v}


def join_numpy(x, s, P, y, sL, PL, offset):
    """The join on the host, block by block (include/ekfslam.h): what the host route computes between its reads and its writes."""
    n, M = x.size, sL.size
    t = x[2] / K
    Rm = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])
    m = y[3:].reshape(M, 2)
    w = m @ Rm.T
    wq = Rm @ y[:2]
    J1 = np.eye(3); J1[0, 2], J1[1, 2] = -wq[1] / K, wq[0] / K
    J2 = np.eye(3); J2[:2, :2] = Rm
    G = np.zeros((2 * M, 3))
    G[0::2, 0] = 1.0; G[1::2, 1] = 1.0
    G[0::2, 2], G[1::2, 2] = -w[:, 1] / K, w[:, 0] / K
    D = np.kron(np.eye(M), Rm)
    out = np.empty((n + 2 * M, n + 2 * M))
    out[3:n, 3:n] = P[3:, 3:]
    out[:3, :3] = J1 @ P[:3, :3] @ J1.T + J2 @ PL[:3, :3] @ J2.T
    out[:3, 3:n] = J1 @ P[:3, 3:]
    out[:3, n:] = J1 @ P[:3, :3] @ G.T + J2 @ PL[:3, 3:] @ D.T
    out[n:, 3:n] = G @ P[:3, 3:]
    out[n:, n:] = G @ P[:3, :3] @ G.T + D @ PL[3:, 3:] @ D.T
    iu = np.triu_indices(n + 2 * M, 1)
    out[iu[1], iu[0]] = out[iu]
    xn = np.concatenate([x, (x[:2] + w).reshape(-1)])
    xn[:2] = x[:2] + wq
    xn[2] = (x[2] + y[2]) % 360.0
    return xn, np.concatenate([s, sL + offset]), out


def measure(N, reps):
    import bench
    from ekf_slam_amd import Engine, _lib
    world, x, s, d, U = bench.make_state(N, 20260104)
    g = Engine(capacity=N + max(LOCAL_SIZES), tile=128, storage="f64", batch=1)
    out = {"state": "configs[2]", "landmarks": N, "storage": "f64", "tile": 128, "reps": reps, "hbm_bytes_per_s": HBM_BYTES_PER_S, "local": {}}

    def reload():
        g.load_lowrank_state(x, s, d, U)
        g.sync()

    def timed_launches(fn, want):
        g.timing_enable(_lib.EKF_KERNEL_APPEND, True, 64)
        g.timing_read(_lib.EKF_KERNEL_APPEND)
        fn()
        launches, ms = g.timing_read(_lib.EKF_KERNEL_APPEND)
        g.timing_enable(_lib.EKF_KERNEL_APPEND, False)
        assert launches == want, (launches, want)
        return 1e3 * ms

    empty = Engine(capacity=1, storage="f64")
    empty.set_x([0.4, -0.3, 7.0]); empty.set_P(np.diag([0.01, 0.02, 0.3]))
    reload(); g.join_map(empty)                               # warm-up
    state_us = []
    for _ in range(reps):
        reload()
        state_us.append(timed_launches(lambda: g.join_map(empty), 1))
    out["state_us"] = figure(state_us)
    for M in LOCAL_SIZES:
        rng = np.random.default_rng(M)
        nl = 3 + 2 * M
        y = np.concatenate([[0.4, -0.3, 7.0], rng.uniform(-15.0, 15.0, 2 * M)])
        A = rng.normal(0.0, 0.05, (nl, 6))
        PL = A @ A.T + np.diag(rng.uniform(0.01, 0.05, nl))
        sL = 1e6 + np.arange(M, dtype=np.float64)
        lo = Engine(capacity=M, storage="f64")
        lo.set_x(y); lo.set_s(sL); lo.set_P(PL)
        lo.sync()
        scans = [[(4, y[3 + 2 * i:5 + 2 * i], PL[3 + 2 * i:5 + 2 * i, 3 + 2 * i:5 + 2 * i], sL[i]) for i in range(a, min(a + 32, M))] for a in range(0, M, 32)]

        def join():
            g.join_map(lo)

        def appends():
            for scan in scans:
                g.append_model(scan)
            g.sync()

        def host_route():
            xn, sn, Pn = join_numpy(g.get_x(), g.get_s(), g.get_P(), lo.get_x(), lo.get_s(), lo.get_P(), 0.0)
            g.set_x(xn); g.set_s(sn); g.set_P(Pn)

        rec = {"bytes_rows_written": 8 * (2 * M * 2 * N + M * (2 * M + 1))}
        legs = [("join_map", join, 2), ("append_model_x", appends, len(scans))] + ([("host_route", host_route, None)] if M == 100 else [])
        for leg, fn, launches in legs:
            reload(); fn()                                    # warm-up: every kernel the timed calls launch
            call, dev = [], []
            for _ in range(reps):
                reload()
                t0 = time.perf_counter()
                fn()
                call.append((time.perf_counter() - t0) * 1e6)
                assert g.N == N + M
            rec[leg] = {"call_us": figure(call)}
            if launches is not None:
                for _ in range(reps):
                    reload()
                    dev.append(timed_launches(fn, launches))
                rec[leg].update(launches_us=figure(dev), launches=launches)
        rows_us = rec["join_map"]["launches_us"]["median"] - out["state_us"]["median"]
        floor_us = 1e6 * rec["bytes_rows_written"] / HBM_BYTES_PER_S
        rec["rows_us"] = rows_us
        rec["roofline"] = {"floor_us": floor_us, "rows_over_floor": rows_us / floor_us if floor_us else None,
                           "rows_bytes_per_s": rec["bytes_rows_written"] / (rows_us * 1e-6) if rows_us > 0 else None}
        rec["ratios"] = {"launches_over_append_model_x": rec["join_map"]["launches_us"]["median"] / rec["append_model_x"]["launches_us"]["median"],
                         "call_over_append_model_x": rec["join_map"]["call_us"]["median"] / rec["append_model_x"]["call_us"]["median"]}
        if M == 100:
            rec["ratios"]["call_over_host_route"] = rec["join_map"]["call_us"]["median"] / rec["host_route"]["call_us"]["median"]
        out["local"][str(M)] = rec
        lo.close()
    empty.close()
    g.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--landmarks", type=int, default=10000)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    rec = {"metric": "ekf_join_map of a local map of M landmarks into 10 000 (host clock of the whole synchronising call; device time of its two "
           "launches under EKF_KERNEL_APPEND), medians of the repeats, each from a reloaded state", "data": "synthetic",
           "expectation": "the rows kernel is not slower per byte written than the append_model launches that write the same old-column region "
           "(an expectation, not an assertion)"}
    rec.update(measure(args.landmarks, args.reps))
    line = json.dumps(rec)
    print(line, flush=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
