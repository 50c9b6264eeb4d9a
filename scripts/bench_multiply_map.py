#!/usr/bin/env python3
"""ekf_multiply_map measured on low-rank loaded states: 10 000 landmarks on F64 tiles of edge 128 and 40 000 landmarks on float tiles of
edge 256, in the form of scripts/bench_sample_map.py.  Every figure is a median of the repeats, each from a RELOADED state, with the spread
(max - min) / median between the repeats beside it.  Reported, not asserted; no ratio is fixed in advance.

Per state:
  tile_pass      device time of the tile passes (k_multiply_tiles, one per chunk of 16 vectors; EKF_KERNEL_ASSOCIATE) of a call with
                 k = 256, per chunk; beside it the tile store's bytes, which a pass reads once (tile_pass_bytes_per_s), the partial
                 blocks it writes, and the F64 flops of the symmetric product (2 n_mm^2 16)
  sums           device time of k_multiply_sum (EKF_KERNEL_COMPACT) in the same call, per chunk
  one_pair_pass  the handle's pass over P for one pending pair (EKF_KERNEL_DOWNDATE, cfg.batch = 1), which reads AND writes the same
                 store, measured in the same process
  sample_apply   ekf_sample_map's apply pass (k_factor_apply over the F64 factor store of edge 64) per chunk, in the same process
  call_us        the whole ekf_multiply_map call at k = 1, 16 and 256, host clock, its waits included
The yardstick at 10 000 landmarks, in the same process on the same state: host_route, ekf_get_P + P @ B.T for each k, with the host pool
capped at 16 threads.  At 40 000 landmarks the host route would need a 51 GB dense matrix and is skipped.

    python scripts/bench_multiply_map.py [--reps 7] [--reps-large 7] --out profiles/multiply_map.json
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
CHUNK = 16
KS = (1, 16, 256)


def median(v):
    return float(sorted(v)[len(v) // 2])


def figure(v):
    return {"median": median(v), "spread": float((max(v) - min(v)) / median(v)) if median(v) else 0.0, "all": v}


def segment_of(tile):
    return 1 if tile >= 256 else 256 // tile


def measure(N, tile, storage, elt, small, reps, host_reps, with_sample):
    import bench
    from ekf_slam_amd import Engine, _lib
    world, x, s, d, U = bench.make_state(N, 20260104)
    g = Engine(capacity=N, tile=tile, storage=storage, batch=1)
    n = 3 + 2 * N
    nt = (2 * N + tile - 1) // tile
    rows = nt * tile
    store = elt * tile * tile * nt * (nt + 1) // 2
    seg = segment_of(tile)
    segments = sum(I // seg + 1 for I in range(nt))
    partial = 8 * (tile * CHUNK * (segments + nt * (nt + 1) // 2) + 3 * CHUNK * nt)
    out = {"landmarks": N, "storage": storage, "tile": tile, "chunk": CHUNK, "segment": seg, "n": n, "store_bytes": store, "segments": segments,
           "partial_bytes": partial, "transposed_partial_bytes_written_per_pass": 8 * tile * CHUNK * nt * (nt - 1) // 2}
    B = np.random.default_rng(1).standard_normal((max(KS), n))

    def reload():
        g.load_lowrank_state(x, s, d, U)
        g.sync()

    reload()
    held = g.device_bytes()
    first = g.multiply_map(B[:CHUNK + 1])                     # warm-up: every kernel, the scratch
    out["scratch_bytes"] = g.device_bytes() - held
    assert out["scratch_bytes"] == 8 * 2 * CHUNK * (rows + 4) + partial, (out["scratch_bytes"], partial)
    out["product_0_rms"] = float(np.sqrt(np.mean(first[0] ** 2)))
    call = {k: [] for k in KS}
    for _ in range(reps):
        for k in KS:
            reload()
            t0 = time.perf_counter()
            g.multiply_map(B[:k])
            call[k].append((time.perf_counter() - t0) * 1e6)
    out["call_us"] = {str(k): figure(v) for k, v in call.items()}
    # the tile passes and the sums, each family in runs of its own
    kk = 256
    chunks = kk // CHUNK
    fam = {}
    for name, which in (("tile_pass", _lib.EKF_KERNEL_ASSOCIATE), ("sums", _lib.EKF_KERNEL_COMPACT)):
        per = []
        for _ in range(reps):
            reload()
            g.timing_enable(which, True, 2 * chunks + 64)
            g.timing_read(which)
            g.multiply_map(B[:kk])
            cnt, ms = g.timing_read(which)
            g.timing_enable(which, False)
            assert cnt == chunks, (name, cnt, chunks)
            per.append(1e3 * ms / chunks)
        fam[name] = {"k": kk, "chunks": chunks, "per_chunk_us": figure(per)}
    out["families"] = fam
    t_pass = fam["tile_pass"]["per_chunk_us"]["median"] * 1e-6
    out["tile_pass_bytes_per_s"] = store / t_pass
    out["tile_pass_bytes_per_s_with_partials"] = (store + 2 * out["transposed_partial_bytes_written_per_pass"] + 8 * tile * CHUNK * segments) / t_pass
    out["tile_pass_flops_per_s"] = 2.0 * (2.0 * N) ** 2 * CHUNK / t_pass
    # the one-pair pass over the handle's own store, in the same process
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
    out["one_pair_pass"] = dict(figure(dev), bytes=2 * store, bytes_per_s=2 * store / (median(dev) * 1e-6))
    out["tile_pass_over_one_pair_pass"] = fam["tile_pass"]["per_chunk_us"]["median"] / median(dev)
    # ekf_sample_map's apply pass, in the same process: a call of two chunks against a call of one
    if with_sample:
        per = []
        for _ in range(reps if small else 1):
            t = []
            for k_ in (2 * CHUNK, CHUNK):
                reload()
                g.timing_enable(_lib.EKF_KERNEL_ASSOCIATE, True, 64)
                g.timing_read(_lib.EKF_KERNEL_ASSOCIATE)
                g.sample_map(B[:k_])
                cnt, ms = g.timing_read(_lib.EKF_KERNEL_ASSOCIATE)
                g.timing_enable(_lib.EKF_KERNEL_ASSOCIATE, False)
                assert cnt == k_ // CHUNK, cnt
                t.append(1e3 * ms)
            per.append(t[0] - t[1])
        nF = (2 * N + 63) // 64
        out["sample_apply"] = {"per_chunk_us": figure(per), "factor_store_bytes": 8 * 64 * 64 * nF * (nF + 1) // 2}
        out["tile_pass_over_sample_apply"] = fam["tile_pass"]["per_chunk_us"]["median"] / median(per)
    if small:
        host = {k: [] for k in KS}
        for _ in range(host_reps):
            reload()
            t0 = time.perf_counter()
            P = g.get_P()
            t1 = time.perf_counter() - t0
            for k in KS:
                t0 = time.perf_counter()
                y = (P @ B[:k].T).T
                host[k].append((t1 + time.perf_counter() - t0) * 1e6)
            del P, y
        out["host_route"] = {"get_P_plus_product_us": {str(k): figure(v) for k, v in host.items()}, "threads": os.environ["OMP_NUM_THREADS"]}
        out["host_route_over_call"] = {str(k): median(host[k]) / median(call[k]) for k in KS}
    else:
        out["host_route"] = "skipped: the dense matrix of %d landmarks is %.0f GB" % (N, 8.0 * n * n / 1e9)
    g.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--reps-large", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--states", default="small,large")
    ap.add_argument("--no-sample", action="store_true", help="leave ekf_sample_map's apply pass (a whole factorisation per call) out")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    rec = {"metric": "ekf_multiply_map, P B on the handle's own tile store (host clock of the whole synchronising call; device time of the "
           "tile pass and of the sums per chunk of 16 vectors), medians of the repeats, each from a reloaded state",
           "data": "synthetic", "reps": args.reps, "reps_large": args.reps_large, "host_reps": args.host_reps, "states": []}
    for N, tile, storage, elt, small in STATES:
        if ("small" if small else "large") not in args.states.split(","):
            continue
        rec["states"].append(measure(N, tile, storage, elt, small, args.reps if small else args.reps_large, args.host_reps, not args.no_sample))
        print(json.dumps(rec["states"][-1]), flush=True)
        with open(args.out, "w") as fh:                       # (written after each state)
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
