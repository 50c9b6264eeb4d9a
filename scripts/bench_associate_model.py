#!/usr/bin/env python3
"""ekf_associate_model measured on the two states of profiles/linear_obs.json: configs[2]'s (10 000 landmarks, F64 tiles of edge 128,
low-rank load) and configs[4]'s starting state (40 000 landmarks, float tiles of edge 256, the pass in F32 arithmetic).  One process per
state; every figure is a median over repeated measurements, with the spread (max - min) / median between the repeats beside it.

Per state and per scan size m in {1, 8, 32}:
  call_us     the whole call, host clock around one ekf_associate_model of m observations (it returns with the results: one wait)
  launch_us   device time of its two launches under the EKF_KERNEL_ASSOCIATE timer: k_assoc_model, k_assoc_model_reduce
Beside them, in the same process and on the same state:
  associate_x_m        m ekf_associate calls (the reference-convention k_associate, one launch and one wait each), measured the same way
  innovation_x_Nm      what a filter driven through the model calls does today: one ekf_model_innovation per (observation, landmark).  200
                       calls are timed and the figure is SCALED to N * m calls -- an extrapolation, labelled as one

The expectations (stated, not asserted): a scan of 32 costs clearly less than 32 ekf_associate calls; the call is dominated by its one wait.

    python scripts/bench_associate_model.py --state 10k|40k [--reps K] --out FILE
    python scripts/bench_associate_model.py --combine A.json B.json --out profiles/associate_model.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATES = {"10k": ("configs[2]", 10000, "f64", 128, 20260104), "40k": ("configs[4] start", 40000, "f32_mixed", 256, 20260106)}
R_FIX = np.array([[0.02, 0.005], [0.005, 0.03]])
R_RB = np.array([[0.02, 0.01], [0.01, 1.2]])
SCANS = (1, 8, 32)
PROBES = 200


def median(v):
    return float(sorted(v)[len(v) // 2])


def spread(v):
    return float((max(v) - min(v)) / median(v))


def figure(v):
    return {"median": median(v), "spread": spread(v), "all": v}


def measure_state(key, reps):
    import bench
    from ekf_slam_amd import Engine, _lib
    name, N, storage, tile, seed = STATES[key]
    world, x, s, d, U = bench.make_state(N, seed)
    rng = np.random.default_rng(5)
    e = Engine(capacity=N, tile=tile, storage=storage, batch=1)
    e.load_lowrank_state(x, s, d, U)
    e.sync()
    out = {"state": name, "landmarks": N, "storage": storage, "tile": tile, "reps": reps, "scans": {}}
    for m in SCANS:
        entries = [dict(model=1, z=[rng.uniform(2.0, 25.0), rng.uniform(0.0, 360.0)], R=R_RB, gate=9.21) if b % 2 == 0 else
                   dict(model=4, z=rng.uniform(-15.0, 15.0, 2), R=R_FIX, gate=9.21) for b in range(m)]
        rows = [np.array([rng.uniform(2.0, 25.0), rng.uniform(0.0, 360.0), float(rng.integers(1, N + 1))]) for _ in range(m)]

        def scan():
            e.associate_model(entries)

        def singles():
            for z in rows:
                e.associate(z, R_RB)

        rec = {}
        for leg, fn, launches_want in (("associate_model", scan, 1), ("associate_x_m", singles, m)):
            fn()                                              # warm-up: every kernel the timed calls launch
            call, launch = [], []
            for _ in range(reps):
                e.sync()
                t0 = time.perf_counter()
                fn()
                call.append((time.perf_counter() - t0) * 1e6)
            for _ in range(reps):                             # the launches' device time, one reading per repeat
                e.timing_enable(_lib.EKF_KERNEL_ASSOCIATE, True, 2 * m)
                e.timing_read(_lib.EKF_KERNEL_ASSOCIATE)
                fn()
                launches, ms = e.timing_read(_lib.EKF_KERNEL_ASSOCIATE)
                e.timing_enable(_lib.EKF_KERNEL_ASSOCIATE, False)
                assert launches == launches_want              # (the two launches of a scan share one bracket)
                launch.append(1e3 * ms)
            rec[leg] = {"call_us": figure(call), "launch_us": figure(launch), "timed_brackets": launches_want}
        probe = []
        for _ in range(reps):
            e.sync()
            t0 = time.perf_counter()
            for q in range(PROBES):
                ent = entries[q % m]
                e.model_innovation(ent["model"], ent["z"], ent["R"], [(37 * q) % N], gate=ent["gate"])
            probe.append((time.perf_counter() - t0) * 1e6 / PROBES)
        rec["innovation_x_Nm"] = {"one_call_us": figure(probe), "timed_calls": PROBES, "scaled_to_calls": N * m,
                                  "extrapolated_us": median(probe) * N * m, "extrapolation": True}
        a, y = rec["associate_model"], rec["associate_x_m"]
        rec["ratios"] = {"call_over_m_associates": a["call_us"]["median"] / y["call_us"]["median"],
                         "launch_over_m_associates": a["launch_us"]["median"] / y["launch_us"]["median"],
                         "launch_share_of_call": a["launch_us"]["median"] / a["call_us"]["median"],
                         "call_over_extrapolated_innovations": a["call_us"]["median"] / rec["innovation_x_Nm"]["extrapolated_us"]}
        out["scans"][str(m)] = rec
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--state", choices=sorted(STATES))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--combine", nargs="+", help="per-state outputs to join into one record")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    if args.combine:
        rec = {"metric": "ekf_associate_model of m observations against m ekf_associate calls (host clock around the waited calls; device time of "
               "the launches under EKF_KERNEL_ASSOCIATE) and against N * m ekf_model_innovation calls (200 timed, scaled: an extrapolation), "
               "medians of the repeats", "data": "synthetic",
               "expectation": "a scan of 32 costs clearly less than 32 ekf_associate calls; the call is dominated by its one wait (expectations, "
               "not assertions)",
               "states": [json.load(open(p)) for p in args.combine]}
    else:
        sys.path.insert(0, ROOT)
        rec = measure_state(args.state, args.reps)
    line = json.dumps(rec)
    print(line, flush=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
