#!/usr/bin/env python3
"""ekf_assign_model measured on the two states of profiles/linear_obs.json: configs[2]'s (10 000 landmarks, F64 tiles of edge 128,
low-rank load) and configs[4]'s starting state (40 000 landmarks, float tiles of edge 256, the pass in F32 arithmetic).  One process per
state; every figure is a median over repeated measurements, with the spread (max - min) / median between the repeats beside it.

Per state, per scan size m in {1, 8, 32} and per crowding -- every observation's gate set from its own row of d2 so that 0, 4 or 40
landmarks lie inside it ("none", "four", "forty": the last keeps 32 of them):
  call_us     the whole call, host clock around one ekf_assign_model of m observations (it returns with the results: one wait)
  launch_us   device time of its three launches under the EKF_KERNEL_ASSOCIATE timer: k_assign_candidates, k_assign_select, k_assign_solve
Beside them, in the same process and on the same state:
  associate_model           ekf_associate_model without the matrix: the floor this call should stay close to
  associate_model_d2_solve  what the call replaces: ekf_associate_model(want_d2=True) -- the m x N matrix back on the host -- then the
                            candidates and the assignment there (NumPy; the readback and the solve timed together and apart)
Nothing is asserted on the times; the two paths are checked to reach the same total.

    python scripts/bench_assign_model.py --state 10k|40k [--reps K] --out FILE
    python scripts/bench_assign_model.py --combine A.json B.json --out profiles/assign_model.json
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
SCANS = (1, 8, 32)
CROWDING = {"none": 0, "four": 4, "forty": 40}
KEEP = 32
INF = float("inf")


def median(v):
    return float(sorted(v)[len(v) // 2])


def figure(v):
    return {"median": median(v), "spread": float((max(v) - min(v)) / median(v)), "all": v}


def host_solve(D, gates):
    """The assignment on the host from the m x N matrix: each row's KEEP cheapest in-gate landmarks, then shortest augmenting paths over
    their union and one private "left out" column per row.  Returns (landmark per row or -1, total)."""
    m = D.shape[0]
    rows = []
    for k in range(m):
        inside = np.flatnonzero(D[k] <= gates[k])
        rows.append(inside[np.lexsort((inside, D[k][inside]))][:KEEP])
    cols = sorted({int(i) for r in rows for i in r})
    at = {lm: c for c, lm in enumerate(cols)}
    w = len(cols) + m
    C = np.full((m, w), INF)
    for k in range(m):
        C[k, [at[int(i)] for i in rows[k]]] = D[k][rows[k]]
        C[k, len(cols) + k] = gates[k]
    u, v = np.zeros(m + 1), np.zeros(w + 1)
    p, way = np.zeros(w + 1, dtype=np.int64), np.zeros(w + 1, dtype=np.int64)
    for i in range(1, m + 1):
        p[0], j0 = i, 0
        minv, used = np.full(w + 1, INF), np.zeros(w + 1, dtype=bool)
        while True:
            used[j0] = True
            cur = C[p[j0] - 1] - u[p[j0]] - v[1:]
            free = ~used[1:]
            better = free & (cur < minv[1:])
            minv[1:][better] = cur[better]
            way[1:][better] = j0
            masked = np.where(free, minv[1:], INF)
            j1 = int(np.argmin(masked)) + 1
            delta = masked[j1 - 1]
            u[p[used]] += delta
            v[used] -= delta
            minv[1:][free] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            p[j0] = p[way[j0]]
            j0 = way[j0]
    landmark = np.full(m, -1, dtype=np.int64)
    for j in range(1, len(cols) + 1):
        if p[j]:
            landmark[p[j] - 1] = cols[j - 1]
    total = 0.0
    for k in range(m):
        total += D[k, landmark[k]] if landmark[k] >= 0 else gates[k]
    return landmark, total


def measure_state(key, reps):
    import bench
    from ekf_slam_amd import Engine, _lib
    name, N, storage, tile, seed = STATES[key]
    world, x, s, d, U = bench.make_state(N, seed)
    rng = np.random.default_rng(5)
    e = Engine(capacity=N, tile=tile, storage=storage, batch=1)
    e.load_lowrank_state(x, s, d, U)
    e.sync()
    xe = e.get_x()
    th = np.radians(xe[2])
    rot = np.array([[np.cos(th), np.sin(th)], [-np.sin(th), np.cos(th)]])
    out = {"state": name, "landmarks": N, "storage": storage, "tile": tile, "reps": reps, "scans": {}}
    for m in SCANS:
        # relative-position sightings of m landmarks spread over the map, a little beside where the state puts them
        targets = [int(t) for t in np.linspace(0, N - 1, m + 2)[1:-1]]
        aimed = [dict(model=4, z=rot @ (xe[3 + 2 * t:5 + 2 * t] - xe[:2]) + rng.normal(0.0, 0.05, 2), R=R_FIX, gate=1.0) for t in targets]
        D0 = e.associate_model(aimed, want_d2=True)["d2_all"]
        for crowd, inside in CROWDING.items():
            ordered = np.sort(D0, axis=1)
            gates = [float(ordered[k, 0]) / 2.0 if inside == 0 else float(ordered[k, inside - 1] + ordered[k, inside]) / 2.0 for k in range(m)]
            entries = [dict(ent, gate=g) for ent, g in zip(aimed, gates)]
            parts = {"readback_us": [], "solve_us": []}

            def assign():
                return e.assign_model(entries)

            def floor():
                return e.associate_model(entries)

            def replaced():
                t0 = time.perf_counter()
                D = e.associate_model(entries, want_d2=True)["d2_all"]
                t1 = time.perf_counter()
                res = host_solve(D, gates)
                parts["readback_us"].append((t1 - t0) * 1e6)
                parts["solve_us"].append((time.perf_counter() - t1) * 1e6)
                return res

            got, (lm_host, total_host) = assign(), replaced()
            within = got["within_gate"].tolist()
            same_total = bool(abs(got["total"] - total_host) <= 1e-12 * max(total_host, 1e-300))
            rec = {"within_gate": within, "ncand": got["ncand"].tolist(), "assigned": int((got["landmark"] >= 0).sum()),
                   "same_total_as_host_solve": same_total, "same_assignment_as_host_solve": bool(np.array_equal(got["landmark"], lm_host))}
            for leg, fn in (("assign_model", assign), ("associate_model", floor), ("associate_model_d2_solve", replaced)):
                fn()                                              # warm-up: every kernel the timed calls launch
                parts["readback_us"], parts["solve_us"] = [], []
                call, launch = [], []
                for _ in range(reps):
                    e.sync()
                    t0 = time.perf_counter()
                    fn()
                    call.append((time.perf_counter() - t0) * 1e6)
                split = {k: figure(v) for k, v in parts.items() if v}
                for _ in range(reps):                             # the launches' device time, one reading per repeat
                    e.timing_enable(_lib.EKF_KERNEL_ASSOCIATE, True, 4)
                    e.timing_read(_lib.EKF_KERNEL_ASSOCIATE)
                    fn()
                    launches, ms = e.timing_read(_lib.EKF_KERNEL_ASSOCIATE)
                    e.timing_enable(_lib.EKF_KERNEL_ASSOCIATE, False)
                    assert launches == 1                          # (the launches of one call share one bracket)
                    launch.append(1e3 * ms)
                rec[leg] = dict({"call_us": figure(call), "launch_us": figure(launch)}, **split)
            a, f, r = rec["assign_model"], rec["associate_model"], rec["associate_model_d2_solve"]
            rec["ratios"] = {"call_over_floor": a["call_us"]["median"] / f["call_us"]["median"],
                             "launch_over_floor": a["launch_us"]["median"] / f["launch_us"]["median"],
                             "call_over_replaced": a["call_us"]["median"] / r["call_us"]["median"]}
            out["scans"]["%d/%s" % (m, crowd)] = rec
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
        rec = {"metric": "ekf_assign_model of m observations with 0, 4 or 40 landmarks inside every gate (host clock around the waited call; device "
               "time of its launches under EKF_KERNEL_ASSOCIATE) beside ekf_associate_model without the matrix (the floor) and "
               "ekf_associate_model(want_d2) plus a host solve (what it replaces), medians of the repeats", "data": "synthetic",
               "expectation": "the call stays close to the floor and well below the matrix readback plus a host solve (expectations, not assertions)",
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
