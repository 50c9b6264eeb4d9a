#!/usr/bin/env python3
"""ekf_sample_map measured on low-rank loaded states: 10 000 landmarks on F64 tiles of edge 128 and 40 000 landmarks on float tiles of
edge 256, in the form of scripts/bench_factor_map.py.  Every figure is a median of the repeats, each from a RELOADED state, with the spread
(max - min) / median between the repeats beside it.  Reported, not asserted; no ratio is fixed in advance.

Per state:
  apply          device time of the apply passes (k_factor_apply, one per chunk of 16 draws; EKF_KERNEL_ASSOCIATE) of a call with
                 k = 256, per chunk; beside it the factor store's bytes, which a pass reads once, and
  apply_at_pass_rate_us   the time those bytes take at the rate of
  one_pair_pass  the handle's pass over P for one pending pair (EKF_KERNEL_DOWNDATE, cfg.batch = 1), measured in the same run
  sums           device time of everything EKF_KERNEL_COMPACT counts in the same call (the factorisation's load, right-hand sides and
                 tail, and k_factor_sample once per chunk), per chunk after the k = 1 call's figure is taken off
  factor_call_us ekf_factor_map alone on the same state (no reference state), host clock
  call_us        the whole ekf_sample_map call at k = 1, 16, 256 and 1 024, host clock, its waits included
The yardstick at 10 000 landmarks, in the same process on the same state: host_route, ekf_get_P + numpy.linalg.cholesky + the product
xi C' for each k, with the host pool capped at 16 threads.  At 40 000 landmarks the host route would need a 51 GB dense matrix and is
skipped, and the large state is repeated --reps-large times.

    python scripts/bench_sample_map.py [--reps 7] [--reps-large 3] --out profiles/sample_map.json
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


TF, SEGMENT = built_constant("launch/map_sizes.h", "kFactorTile"), built_constant("launch/map_sizes.h", "kFactorSegment")
CHUNK = built_constant("kernel_args.h", "kFactorChunk")
KS = (1, 16, 256, 1024)


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
    segments = sum(I // SEGMENT + 1 for I in range(nF))
    out = {"landmarks": N, "storage": storage, "tile": tile, "factor_tile": TF, "chunk": CHUNK, "segment": SEGMENT, "n": n, "store_bytes": store,
           "factor_store_bytes": 8 * TF * TF * nF * (nF + 1) // 2, "partial_bytes": 8 * TF * CHUNK * segments, "segments": segments}
    draws = np.random.default_rng(1).standard_normal((max(KS), n))

    def reload():
        g.load_lowrank_state(x, s, d, U)
        g.sync()

    reload()
    g.factor_map()
    held = g.device_bytes()
    samples, info = g.sample_map(draws[:CHUNK + 1])           # warm-up: every kernel, the scratch
    rows = nF * TF
    out["sample_scratch_bytes"] = g.device_bytes() - held     # two chunks, the partial blocks, per tile row its part of W' Xi
    assert out["sample_scratch_bytes"] == 8 * (2 * CHUNK * (rows + 4) + TF * CHUNK * segments + 3 * CHUNK * nF), out["sample_scratch_bytes"]
    out["info"] = info
    out["sample_0_minus_x_rms"] = float(np.sqrt(np.mean((samples[0] - x) ** 2)))
    fac, call = [], {k: [] for k in KS}
    for _ in range(reps):
        reload()
        t0 = time.perf_counter()
        g.factor_map()
        fac.append((time.perf_counter() - t0) * 1e6)
        for k in KS:
            reload()
            t0 = time.perf_counter()
            g.sample_map(draws[:k])
            call[k].append((time.perf_counter() - t0) * 1e6)
    out["factor_call_us"] = figure(fac)
    out["call_us"] = {str(k): figure(v) for k, v in call.items()}
    out["call_over_factor_call"] = {str(k): median(v) / median(fac) for k, v in call.items()}
    # the apply passes and the sums, each family in runs of its own
    kk = 256
    chunks = kk // CHUNK
    fam = {}
    for name, which, launches in (("apply", _lib.EKF_KERNEL_ASSOCIATE, chunks), ("sums", _lib.EKF_KERNEL_COMPACT, 2 + chunks)):
        dev, base = [], []
        for _ in range(reps if small else 1):
            for k_, sink in ((kk, dev), (1, base)):
                reload()
                g.timing_enable(which, True, 2 * chunks + 64)
                g.timing_read(which)
                g.sample_map(draws[:k_])
                cnt, ms = g.timing_read(which)
                g.timing_enable(which, False)
                assert cnt == (launches if k_ == kk else launches - chunks + 1), (name, k_, cnt, launches)
                sink.append(1e3 * ms)
        per = [(a - b) / (chunks - 1) for a, b in zip(dev, base)]
        fam[name] = {"k": kk, "chunks": chunks, "total_us": figure(dev), "at_k_1_us": figure(base), "per_chunk_us": figure(per)}
    out["families"] = fam
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
    out["apply_at_pass_rate_us"] = out["factor_store_bytes"] / pass_rate * 1e6
    out["apply_over_its_bytes_at_pass_rate"] = fam["apply"]["per_chunk_us"]["median"] / out["apply_at_pass_rate_us"]
    out["apply_bytes_per_s"] = out["factor_store_bytes"] / (fam["apply"]["per_chunk_us"]["median"] * 1e-6)
    out["apply_flops_per_s"] = 2.0 * TF * TF * CHUNK * nF * (nF + 1) / 2 / (fam["apply"]["per_chunk_us"]["median"] * 1e-6)
    if small:
        host = {k: [] for k in KS}
        for _ in range(host_reps):
            reload()
            t0 = time.perf_counter()
            P = g.get_P()
            order = np.concatenate([np.arange(3, n), np.arange(3)])
            L = np.linalg.cholesky(P[np.ix_(order, order)])
            t1 = time.perf_counter() - t0
            for k in KS:
                t0 = time.perf_counter()
                y = x[order][None, :] + draws[:k][:, order] @ L.T
                host[k].append((t1 + time.perf_counter() - t0) * 1e6)
            del P, L, y
        out["host_route"] = {"get_P_plus_cholesky_plus_product_us": {str(k): figure(v) for k, v in host.items()}, "threads": os.environ["OMP_NUM_THREADS"]}
        out["host_route_over_call"] = {str(k): median(host[k]) / median(call[k]) for k in KS}
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
    rec = {"metric": "ekf_sample_map, draws of the posterior from one factorisation on the device (host clock of the whole synchronising "
           "call; device time of the apply passes and of the sums per chunk of 16 draws), medians of the repeats, each from a reloaded state",
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
