#!/usr/bin/env python3
"""ekf_solve_map measured on low-rank loaded states: 10 000 landmarks on F64 tiles of edge 128 and 40 000 landmarks on float tiles of
edge 256, in the form of scripts/bench_sample_map.py.  Every figure is a median of the repeats, each from a RELOADED state, with the spread
(max - min) / median between the repeats beside it.  Reported, not asserted; no target is fixed in advance.

Per state:
  sweeps         device time of ONE chunk's forward sweep (k_solve_forward, one launch per tile column; one bracket under
                 EKF_KERNEL_ASSOCIATE) and backward sweep (k_solve_backward, one launch per tile row; EKF_KERNEL_APPEND) of a call with
                 k = 16 and the full form, the number of launches of each, the bytes they read (every off-diagonal tile once, the
                 inverse of a diagonal tile once per workgroup; and the store's unique bytes), time per launch, and
  sweep_at_pass_rate_us   the time the unique bytes take at the rate of
  one_pair_pass  the handle's pass over P for one pending pair (EKF_KERNEL_DOWNDATE, cfg.batch = 1), measured in the same run
  factor_call_us ekf_factor_map alone on the same state (no reference state), host clock: the call's floor
  call_us        the whole ekf_solve_map call per form at k = 1, 16 and 256, host clock, its waits included
The yardstick at 10 000 landmarks, in the same process on the same state: host_route, ekf_get_P + numpy.linalg.cholesky + two triangular
solves for each k, with the host pool capped at 16 threads.  At 40 000 landmarks the host route would need a 51 GB dense matrix and is
skipped, and the large state is repeated --reps-large times.

    python scripts/bench_solve_map.py [--reps 7] [--reps-large 3] --out profiles/solve_map.json
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


def built_constant(path, name):
    """The value of `constexpr int <name> = <integer>;` in a source file of the library: the shape figures below follow what is built."""
    import re
    m = re.search(r"constexpr int %s = (\d+);" % name, open(os.path.join(ROOT, "ekf_slam_amd", "csrc", path)).read())
    assert m, (path, name)
    return int(m.group(1))


TF, CHUNK = built_constant("launch/map_sizes.h", "kFactorTile"), built_constant("kernel_args.h", "kFactorChunk")
KS = (1, 16, 256)
FORMS = ("full", "half")


def median(v):
    return float(sorted(v)[len(v) // 2])


def figure(v):
    return {"median": median(v), "spread": float((max(v) - min(v)) / median(v)) if median(v) else 0.0, "all": v}


def triangular_solver():
    try:
        from scipy.linalg import solve_triangular
        return "scipy.linalg.solve_triangular", lambda L, B, trans: solve_triangular(L, B, lower=True, trans=trans, check_finite=False)
    except ImportError:
        return "numpy.linalg.solve", lambda L, B, trans: np.linalg.solve(L.T if trans else L, B)


def measure(N, tile, storage, elt, small, reps, host_reps):
    import bench
    from ekf_slam_amd import Engine, _lib
    world, x, s, d, U = bench.make_state(N, 20260104)
    g = Engine(capacity=N, tile=tile, storage=storage, batch=1)
    n = 3 + 2 * N
    nF = (2 * N + TF - 1) // TF
    nt = (2 * N + tile - 1) // tile
    store = elt * tile * tile * nt * (nt + 1) // 2
    tile_bytes = 8 * TF * TF
    out = {"landmarks": N, "storage": storage, "tile": tile, "factor_tile": TF, "chunk": CHUNK, "n": n, "store_bytes": store,
           "factor_store_bytes": tile_bytes * nF * (nF + 1) // 2, "inverse_bytes": tile_bytes * nF,
           "launches_per_chunk": {"forward": nF, "tail": 1, "backward": nF}}
    # one sweep: every off-diagonal tile once and, per workgroup, the inverse of the column's (row's) diagonal tile
    out["sweep_bytes_unique"] = tile_bytes * (nF * (nF - 1) // 2 + nF)
    out["sweep_bytes_requested"] = tile_bytes * (nF * (nF - 1) // 2 + nF * (nF + 1) // 2)
    B = np.random.default_rng(1).standard_normal((max(KS), n))

    def reload():
        g.load_lowrank_state(x, s, d, U)
        g.sync()

    reload()
    g.sample_map(B[:1])
    held = g.device_bytes()
    res, info = g.solve_map(B[:CHUNK + 1], "full")            # warm-up: every kernel, the scratch
    g.solve_map(B[:1], "half")
    out["solve_scratch_bytes"] = g.device_bytes() - held
    assert out["solve_scratch_bytes"] == out["inverse_bytes"], out["solve_scratch_bytes"]
    out["info"] = info
    fac, call = [], {f: {k: [] for k in KS} for f in FORMS}
    for _ in range(reps):
        reload()
        t0 = time.perf_counter()
        g.factor_map()
        fac.append((time.perf_counter() - t0) * 1e6)
        for f in FORMS:
            for k in KS:
                reload()
                t0 = time.perf_counter()
                g.solve_map(B[:k], f)
                call[f][k].append((time.perf_counter() - t0) * 1e6)
    out["factor_call_us"] = figure(fac)
    out["call_us"] = {f: {str(k): figure(v) for k, v in call[f].items()} for f in FORMS}
    out["call_minus_factor_call_us"] = {f: {str(k): median(v) - median(fac) for k, v in call[f].items()} for f in FORMS}
    # one chunk's sweeps: the forward and the backward bracket of a full call with exactly one chunk
    fwd, bwd = [], []
    for _ in range(reps if small else 2):
        reload()
        for which in (_lib.EKF_KERNEL_ASSOCIATE, _lib.EKF_KERNEL_APPEND):
            g.timing_enable(which, True, 64)
            g.timing_read(which)
        g.solve_map(B[:CHUNK], "full")
        for which, sink in ((_lib.EKF_KERNEL_ASSOCIATE, fwd), (_lib.EKF_KERNEL_APPEND, bwd)):
            cnt, ms = g.timing_read(which)
            g.timing_enable(which, False)
            assert cnt == 1, (which, cnt)
            sink.append(1e3 * ms)
    out["sweeps"] = {"forward_us": figure(fwd), "backward_us": figure(bwd),
                     "forward_us_per_launch": median(fwd) / nF, "backward_us_per_launch": median(bwd) / nF}
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
    out["sweep_at_pass_rate_us"] = out["sweep_bytes_unique"] / pass_rate * 1e6
    out["forward_over_its_bytes_at_pass_rate"] = median(fwd) / out["sweep_at_pass_rate_us"]
    out["backward_over_its_bytes_at_pass_rate"] = median(bwd) / out["sweep_at_pass_rate_us"]
    out["forward_bytes_per_s"] = out["sweep_bytes_unique"] / (median(fwd) * 1e-6)
    out["backward_bytes_per_s"] = out["sweep_bytes_unique"] / (median(bwd) * 1e-6)
    if small:
        name, tri = triangular_solver()
        host = {f: {k: [] for k in KS} for f in FORMS}
        order = np.concatenate([np.arange(3, n), np.arange(3)])
        for _ in range(host_reps):
            reload()
            t0 = time.perf_counter()
            P = g.get_P()
            L = np.linalg.cholesky(P[np.ix_(order, order)])
            t1 = time.perf_counter() - t0
            for k in KS:
                t0 = time.perf_counter()
                y = tri(L, B[:k][:, order].T, 0)
                th = time.perf_counter() - t0
                zz = tri(L, y, 1)
                tf = time.perf_counter() - t0
                host["half"][k].append((t1 + th) * 1e6)
                host["full"][k].append((t1 + tf) * 1e6)
            del P, L, y, zz
        out["host_route"] = {"get_P_plus_cholesky_plus_solves_us": {f: {str(k): figure(v) for k, v in host[f].items()} for f in FORMS},
                             "triangular_solver": name, "threads": os.environ["OMP_NUM_THREADS"]}
        out["host_route_over_call"] = {f: {str(k): median(host[f][k]) / median(call[f][k]) for k in KS} for f in FORMS}
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
    rec = {"metric": "ekf_solve_map, C^-1 B and P^-1 B from one factorisation on the device (host clock of the whole synchronising call; "
           "device time of one chunk's forward and backward sweeps), medians of the repeats, each from a reloaded state",
           "data": "synthetic", "reps": args.reps, "reps_large": args.reps_large, "host_reps": args.host_reps, "states": []}
    for N, tile, storage, elt, small in STATES:
        if ("small" if small else "large") not in args.states.split(","):
            continue
        rec["states"].append(measure(N, tile, storage, elt, small, args.reps if small else args.reps_large, args.host_reps))
        print(json.dumps(rec["states"][-1]), flush=True)
        with open(args.out, "w") as fh:                       # (written after each state: the large one takes minutes)
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
