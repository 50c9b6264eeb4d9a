#!/usr/bin/env python3
"""ekf_joint_search measured against the route it replaces, in one process on the same state: 10 000 landmarks on F64 tiles of edge 128
and 40 000 on float tiles of edge 256, low-rank load.  Every figure is a median of --reps measurements from a reloaded state, with the
spread (max - min) / median between them.

Per scan size m in {1, 4, 8, 32}, 0 or 4 candidates per entry, beam in {8, 64} and 0 / 31 pending pairs (cfg.batch = 32):
  search_call_us     the host clock around one ekf_joint_search (it returns with the result: every launch queued, one readback, one wait)
  search_device_us   device time of all its launches under the EKF_KERNEL_ASSOCIATE timer: the candidate part, the prepare launch and two
                     launches per scan index (device_us_per_level: that sum divided by m)
  host_route_us      today's route, search only, nothing applied: assign_model(want_candidates=True), then one joint_innovation call per
                     level whose hypotheses the host builds from the previous answer (measure_model_joint's loop); host_calls counts them
The scene with candidates is the cluster pattern tiled: the scan's landmarks moved, four a cluster on a 0.6 grid, clusters 6 apart, in
front of the robot with variance 0.01 and the robot's position variance raised to 1.0; every entry then has at least four candidates
and the search branches at every level.  The scene without candidates sights far outside the map: every level exits at once.
No figure is a pass/fail bar.

    python scripts/bench_joint_search.py [--reps K] --out profiles/joint_search.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20260104
STATES = ((10000, "f64", 128), (40000, "f32", 256))
R_FIX = np.array([[0.02, 0.005], [0.005, 0.03]])
SCANS, CANDS, BEAMS, PENDING = (1, 4, 8, 32), (0, 4), (8, 64), (0, 31)
GATE, JOINT_P = 9.21, 0.99


def median(v):
    return float(sorted(v)[len(v) // 2])


def figure(v):
    return {"median": median(v), "spread": float((max(v) - min(v)) / median(v)), "all": v}


def relative(xe, p):
    dx, dy = p[0] - xe[0], p[1] - xe[1]
    c, sn = np.cos(np.radians(xe[2])), np.sin(np.radians(xe[2]))
    return np.array([c * dx + sn * dy, -sn * dx + c * dy])


def clustered(x, d, lms):
    """The state with landmarks lms moved into clusters of four in front of the robot (0.6 apart, the clusters 6 apart), variance 0.01."""
    x, d = x.copy(), d.copy()
    d[0] = d[1] = 1.0
    c, sn = np.cos(np.radians(x[2])), np.sin(np.radians(x[2]))
    for q, lm in enumerate(lms):
        g, r = divmod(q, 4)
        fx, fy = 6.0 + 0.6 * (r % 2) + 6.0 * (g % 4), 3.0 + 0.6 * (r // 2) + 6.0 * (g // 4)
        x[3 + 2 * lm:5 + 2 * lm] = (x[0] + c * fx - sn * fy, x[1] + sn * fx + c * fy)
        d[3 + 2 * lm:5 + 2 * lm] = 0.01
    return x, d


def host_route(e, entries, thresholds, beam):
    """measure_model_joint's search as the parent commit runs it, nothing applied: (winner, calls made)."""
    m = len(entries)
    res = e.assign_model(entries, want_candidates=True)
    cands = [[int(i) for i in res["cand"][k][:min(4, int(res["ncand"][k]))]] for k in range(m)]
    searched = [k for k in range(m) if cands[k]]
    sub = [entries[k] for k in searched]
    alive, calls = [((), 0, 0.0)], 1
    for level, k in enumerate(searched):
        ext = [hyp + (c,) for hyp, _, _ in alive for c in cands[k] + [-1] if c < 0 or c not in hyp]
        pad = [-1] * (len(searched) - level - 1)
        ans = e.joint_innovation(sub, np.array([list(h) + pad for h in ext], dtype=np.int64).reshape(len(ext), len(searched)))
        calls += 1
        alive = []
        for h, d2 in zip(ext, np.asarray(ans["d2_prefix"])[:, level]):
            pairings = sum(1 for c in h if c >= 0)
            if float(d2) <= thresholds[2 * pairings]:              # (every entry of this script's scans is model 4: two rows a pairing)
                alive.append((h, pairings, float(d2)))
        alive.sort(key=lambda h: (-h[1], h[2], h[0]))
        alive = alive[:beam]
    winner = [-1] * m
    for k, c in zip(searched, alive[0][0]):
        winner[k] = c
    return winner, calls


def measure(reps):
    import bench
    from ekf_slam_amd import Engine, _lib
    from ekf_slam_amd.slam import chi2_quantile
    out = {"reps": reps, "legs": []}
    rng = np.random.default_rng(5)
    for N, storage, tile in STATES:
        world, x0, s, d0, U = bench.make_state(N, SEED)
        lms = [int(v) for v in rng.choice(N, max(SCANS), replace=False)]
        x, d = clustered(x0, d0, lms)
        for pending in PENDING:
            e = Engine(capacity=N, tile=tile, storage=storage, batch=32)

            def reload():
                e.load_lowrank_state(x, s, d, U)
                for q in range(pending):                      # update-steps that stay pending: sightings of landmarks spread over the map
                    k = (q * 313 + 7) % N
                    e.observe_model(4, relative(x, x[3 + 2 * k:5 + 2 * k]) + 0.01, R_FIX, [k])
                e.sync()
                assert e.pending() == pending
            for m in SCANS:
                for ncand in CANDS:
                    reload()
                    xe = e.get_x()
                    if ncand:
                        entries = [dict(model=4, z=relative(xe, xe[3 + 2 * lm:5 + 2 * lm]) + 0.01 * ((q % 3) - 1), R=R_FIX, gate=GATE) for q, lm in enumerate(lms[:m])]
                    else:
                        entries = [dict(model=4, z=np.array([5e4 + 10.0 * q, -5e4]), R=R_FIX, gate=GATE) for q in range(m)]
                    thr = [chi2_quantile(JOINT_P, dof) for dof in range(2 * m + 1)]
                    for beam in BEAMS:
                        got = e.joint_search(entries, thr, beam)
                        winner, calls = host_route(e, entries, thr, beam)
                        assert got["landmark"].tolist() == winner, (got["landmark"].tolist(), winner)
                        call, dev, host = [], [], []
                        for _ in range(reps):
                            reload()
                            e.joint_search(entries, thr, beam)            # warm-up on the reloaded state
                            e.sync()
                            t0 = time.perf_counter()
                            e.joint_search(entries, thr, beam)
                            call.append((time.perf_counter() - t0) * 1e6)
                            e.timing_enable(_lib.EKF_KERNEL_ASSOCIATE, True, 4 + 2 * m)
                            e.timing_read(_lib.EKF_KERNEL_ASSOCIATE)
                            e.joint_search(entries, thr, beam)
                            launches, ms = e.timing_read(_lib.EKF_KERNEL_ASSOCIATE)
                            e.timing_enable(_lib.EKF_KERNEL_ASSOCIATE, False)
                            assert launches == 2 + 2 * m
                            dev.append(1e3 * ms)
                            host_route(e, entries, thr, beam)
                            e.sync()
                            t0 = time.perf_counter()
                            host_route(e, entries, thr, beam)
                            host.append((time.perf_counter() - t0) * 1e6)
                        leg = {"landmarks": N, "storage": storage, "tile": tile, "m": m, "candidates": ncand, "beam": beam, "pending": pending,
                               "search_call_us": figure(call), "search_device_us": figure(dev), "host_route_us": figure(host), "host_calls": calls,
                               "pairings": int(got["pairings"]), "tested": int(got["tested"].sum()), "truncated": bool(got["truncated"]),
                               "device_us_per_level": median(dev) / m, "host_over_search": median(host) / median(call)}
                        print(json.dumps({k: (v["median"] if isinstance(v, dict) else v) for k, v in leg.items()}), file=sys.stderr, flush=True)
                        out["legs"].append(leg)
            e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    rec = {"metric": "one ekf_joint_search call (host clock around the waited call; device time of its launches under EKF_KERNEL_ASSOCIATE) "
           "against assign_model plus one joint_innovation call per level in the same process on the same state; medians of the repeats",
           "data": "synthetic", "expectation": "none: measured, not tuned"}
    rec.update(measure(args.reps))
    line = json.dumps(rec)
    print(line, flush=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
