#!/usr/bin/env python3
"""Observations through a model (ekf_observe_model) measured on the two states of profiles/linear_obs.json: configs[2]'s (10 000
landmarks, F64 tiles of edge 128, low-rank load) and configs[4]'s starting state (40 000 landmarks, float tiles of edge 256, the pass in
F32 arithmetic).  One process per state; every figure is a median over repeated measurements.

Per state, per cfg.batch in {1, 32} and per model (the five models on landmarks, and the range and the bearing to an anchor):
  step_ms    one update-step, host clock over cfg.batch consecutive no-wait steps up to a stream synchronise, divided by cfg.batch
             (the batch's pass over P included: at batch 1 every step carries one)
  gather_us  device time of the launch under the EKF_KERNEL_GATHER timer: k_gather_model

The yardsticks, in the same process: ekf_observe_linear with the SAME block pattern and a constant H of the same values -- robot + one
landmark for models 1-4, robot only for the anchor forms, two landmarks for model 5 -- which differs from the model launch by the
small part's serial work alone (one atan2d, one sind / cosd pair, a square root and a few divisions on one lane per workgroup, and H
read from LDS instead of the argument block); and one ekf_correct step.  The parent commit's ekf_correct comes from its own library:
`--legs baseline --lib <its libekfslam.so> --commit <its hash>`, handed to the run of the new legs with --baseline-json.

The expectation (stated, not asserted): the launch takes no more than the matching linear launch plus 5 % plus the spread between
repeats, and at batch 1 the model step equals the linear step within that spread.  The spread of a quantity is (max - min) / median over
its repeats; a ratio's allowance adds the spreads of its two sides.

    python scripts/bench_model_obs.py --state 10k|40k [--legs new|baseline] [--lib FILE] [--commit LABEL] [--baseline-json FILE]
                                      [--reps K] --out FILE
    python scripts/bench_model_obs.py --combine A.json B.json --out profiles/model_obs.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ekf_observe_model", "ekf_model_innovation", "ekf_model_evaluate")
STATES = {"10k": ("configs[2]", 10000, "f64", 128, 20260104), "40k": ("configs[4] start", 40000, "f32_mixed", 256, 20260106)}
R_FIX = np.array([[0.02, 0.005], [0.005, 0.03]])
BATCHES = (1, 32)
ROWS = {1: 2, 2: 1, 3: 1, 4: 2, 5: 1}


def median(v):
    return float(sorted(v)[len(v) // 2])


def spread(v):
    return float((max(v) - min(v)) / median(v))


def measure_state(key, legs, reps):
    import bench
    from ekf_slam_amd import Engine, _lib
    name, N, storage, tile, seed = STATES[key]
    world, x, s, d, U = bench.make_state(N, seed)
    steps = bench.make_steps(world, N, 64, [.01, 5.0])
    at = lambda k: x[3 + 2 * k:5 + 2 * k]
    i, j = N // 3, N - 5
    anchor = x[:2] + [7.0, -4.0]
    # name -> (model, landmarks, anchor); z is placed 0.05 beside h(x) of the loaded state
    kinds = {"range_bearing": (1, (i,), None), "range": (2, (i,), None), "bearing": (3, (i,), None), "relative_xy": (4, (i,), None),
             "landmark_range": (5, (i, j), None), "anchor_range": (2, (), anchor), "anchor_bearing": (3, (), anchor)}
    out = {"state": name, "landmarks": N, "storage": storage, "tile": tile, "reps": reps, "batches": {}}
    for batch in BATCHES:
        e = Engine(capacity=N, tile=tile, storage=storage, batch=batch)
        e.load_lowrank_state(x, s, d, U)
        e.sync()
        obs = {}
        if legs == "new":
            for kind, (model, lms, anc) in kinds.items():
                t0 = at(lms[0]) if lms else anc
                hx, H = Engine.model_evaluate(model, x[:3], t0, at(lms[1]) if model == 5 else None, lib=e.lib)
                rows = ROWS[model]
                R = R_FIX if rows == 2 else np.array([[0.05, 0.0], [0.0, 0.0]])
                Rl = R_FIX if rows == 2 else np.array([[0.05, 0.0], [0.0, 1.0]])
                Hl = [H[:, 3 + 2 * b:5 + 2 * b] for b in range(len(lms))]
                Hx = H[:, :3] @ x[:3] + sum((Hl[b] @ at(lms[b]) for b in range(len(lms))), np.zeros(2))
                obs[kind] = dict(model=dict(model=model, z=hx[:rows] + 0.05, R=R, landmarks=lms, anchor=anc),
                                 linear=dict(z=Hx + 0.05 * (np.arange(2) < rows), R=Rl, Hr=H[:, :3], landmarks=lms, Hl=Hl))

        def correct_step(t):
            u, z, R, k = steps[t % len(steps)]
            e.predict(u); e.correct(z, R, k)

        def runner(leg):
            if leg == "correct":
                return correct_step
            kind, which = leg
            o = obs[kind][which]
            if which == "model":
                return lambda t: (e.predict(steps[t % len(steps)][0]), e.observe_model(o["model"], o["z"], o["R"], o["landmarks"], o["anchor"]))
            return lambda t: (e.predict(steps[t % len(steps)][0]), e.observe_linear(o["z"], o["R"], o["Hr"], o["landmarks"], o["Hl"]))

        def measure(leg):
            step = runner(leg)
            for t in range(batch):                            # warm-up: every kernel the timed steps launch, one whole batch
                step(t)
            e.sync()
            per_step = []
            for r in range(reps):
                t0 = time.perf_counter()
                for t in range(batch):
                    step(r * batch + t)
                e.sync()
                per_step.append((time.perf_counter() - t0) * 1e3 / batch)
            assert e.pending() == 0
            gather = []
            for r in range(reps):                             # the launch's device time, one reading per repeat: its spread is measured too
                e.timing_enable(_lib.EKF_KERNEL_GATHER, True, 2 * batch)
                e.timing_read(_lib.EKF_KERNEL_GATHER)
                for t in range(batch):
                    step(r * batch + t)
                launches, ms = e.timing_read(_lib.EKF_KERNEL_GATHER)
                e.timing_enable(_lib.EKF_KERNEL_GATHER, False)
                assert launches == batch
                gather.append(1e3 * ms / launches)
            e.flush(); e.sync()
            return {"step_ms": {"median": median(per_step), "spread": spread(per_step), "all": per_step},
                    "gather_us": {"median": median(gather), "spread": spread(gather), "all": gather}}

        rec = {"correct": measure("correct")}
        for kind in (sorted(kinds) if legs == "new" else []):
            rec[kind] = {"model": measure((kind, "model")), "linear": measure((kind, "linear"))}
        if legs == "new":
            irregular, gated = e.linear_rejections()
            assert (irregular, gated) == (0, 0), "a timed observation did not apply"
        rec["pass_kernel"] = e.downdate_kernel_name()[0]
        out["batches"][str(batch)] = rec
        e.close()
    return out


def with_ratios(new, base):
    """Per batch and model: the launch and the step over the matching linear observation's, with the allowance each is held against;
    the step over the correction's of the same process and of the parent's library."""
    r = {"expectation": "gather_over_linear <= 1.05 + the spreads of both sides; at batch 1 |step_over_linear - 1| <= the spreads of both sides "
                        "(expectations, not assertions)", "batches": {}}
    met = True
    for b, rec in new["batches"].items():
        own = rec["correct"]["step_ms"]["median"]
        par = base["batches"][b]["correct"]["step_ms"]["median"] if base else None
        rows = {}
        for k, v in rec.items():
            if not (isinstance(v, dict) and "model" in v):
                continue
            m, l = v["model"], v["linear"]
            g = m["gather_us"]["median"] / l["gather_us"]["median"]
            g_allow = 1.05 + m["gather_us"]["spread"] + l["gather_us"]["spread"]
            st = m["step_ms"]["median"] / l["step_ms"]["median"]
            st_allow = m["step_ms"]["spread"] + l["step_ms"]["spread"]
            row = {"gather_over_linear": g, "gather_allowance": g_allow, "gather_met": g <= g_allow, "step_over_linear": st, "step_spread": st_allow,
                   "step_over_own_correct": m["step_ms"]["median"] / own}
            if b == "1":
                row["step_met"] = abs(st - 1.0) <= st_allow
                met = met and row["step_met"]
            if par:
                row["step_over_parent_correct"] = m["step_ms"]["median"] / par
            met = met and row["gather_met"]
            rows[k] = row
        if par:
            rows["correct_over_parent_correct"] = own / par
        r["batches"][b] = rows
    r["met"] = met
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--state", choices=sorted(STATES))
    ap.add_argument("--legs", choices=["new", "baseline"], default="new")
    ap.add_argument("--lib", help="the libekfslam.so to measure (default: the tree's)")
    ap.add_argument("--commit", default="working tree", help="label of the code the library was built from")
    ap.add_argument("--baseline-json", help="output of a --legs baseline run of the same state on the parent commit")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--combine", nargs="+", help="per-state outputs to join into one record")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    if args.combine:
        rec = {"metric": "ekf_observe_model against ekf_observe_linear with the same block pattern and against one ekf_correct step (host clock over "
               "cfg.batch no-wait steps to a stream synchronise, per step; device time of the gather launch), medians of the repeats", "data": "synthetic",
               "states": [json.load(open(p)) for p in args.combine]}
    else:
        if args.lib:
            os.environ["EKF_LIB_PATH"] = os.path.abspath(args.lib)
        sys.path.insert(0, ROOT)
        from ekf_slam_amd import _lib
        if args.legs == "baseline":
            import ctypes
            raw = ctypes.CDLL(_lib.LIB_PATH)
            assert not any(hasattr(raw, n) for n in NEW_SYMBOLS), "--legs baseline wants a library WITHOUT the new entry points"
            for n in NEW_SYMBOLS:
                _lib.SIGNATURES.pop(n)
        res = measure_state(args.state, args.legs, args.reps)
        rec = {"commit": args.commit, "library": os.path.basename(_lib.LIB_PATH), "legs": args.legs, **res}
        base = json.load(open(args.baseline_json)) if args.baseline_json else None
        if base:
            assert base["landmarks"] == res["landmarks"] and base["storage"] == res["storage"]
        if args.legs == "new":
            rec = {"state": res["state"], "landmarks": res["landmarks"], "storage": res["storage"], "tile": res["tile"], "parent": base,
                   "this_change": rec, "ratios": with_ratios(res, base)}
    line = json.dumps(rec)
    print(line, flush=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
