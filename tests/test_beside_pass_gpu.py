"""GPU: the calls that run "no flush, beside an asynchronous pass" with a pass actually in flight.

cfg.async_flush runs the pass over P on a stream of its own into the other tile store while the main stream goes on.  At the 18-150
landmarks of the feature tests a pass is over before the host issues the next call; here the map has ~20 000 landmarks
(async_cases.placement), a pass lasts milliseconds, and the calls under test are issued 1-4 steps behind a batch boundary, while that
boundary's pass runs (asserted from the host clock and the pass timers, as tests/test_async_growth_gpu.py asserts its own premise):

  * append_model scans of 3-6 entries into the store the pass reads -- every one of them carries the map over a tile-row edge in one
    launch (filler scans of up to 32 bring the map up to the edge) -- whose rows the copy behind the pass must deliver;
  * the linear / model / iterated gathers on tilebuf[base] patched with frozen and new pairs: landmark, robot-position and heading fixes, a
    two-landmark H, all five models on the first, the last, a tile-row-edge landmark and an anchor, landmark ranges across tile rows in
    both orders;
  * predict_model chains of 1-3 steps, all three motion models, rewriting the strip next to a pass that consumes pairs made from the old one;
  * associate_model (4 observations, the m x N matrix), joint_innovation (8 pairings, 4 hypotheses), model_innovation, linear_innovation,
    which wait on the main stream only and must change neither pending() nor the number of passes;
  * one more leg: remove_landmarks, merge_landmarks and merge_landmarks_batch, which must retire the pass and its row copy before they compact.

The plan (beside_pass_cases.make_plan) is precomputed from the loaded state alone.  The asynchronous engine is driven ALONE through it;
its synchronous twin and the factored F64 oracle (oracle/ekf_factored.py, through the generic steps pinned to the dense forms in
tests/test_oracle_factored.py) follow.  Compared: x, the digests, every landmark's diagonal block, the two rows over all columns of one
landmark per tile row and of EVERY landmark append_model added.  From the oracle alone: two batches move every tile of the sampled rows,
and every appended row has in every tile column of the map before it an entry, of at least 20x the row tolerance.

The entry points added since (the joint updates, join / extract / transform / factor_map, observe_model_assigned, assign_model,
joint_search) meet a pass in flight in tests/test_beside_pass_newer_gpu.py, which reuses _engines and _passes.

Sizes and the measured premise (MI355X): see MEASURED below."""
import time

import numpy as np
import pytest

import async_cases
import beside_pass_cases as B
from helpers import rel_err

pytestmark = pytest.mark.gpu

MEASURED = """
On an MI355X, every leg at the size of async_cases.placement (no leg is halved: at ~20 000 landmarks a pass lasts 1.5-2.2 ms and the
later calls behind a boundary are issued 1.0-1.8 ms after it, so half the size would not leave twice the margin):

  leg                 landmarks        steps  pass kernel                     mean pass   host ms from the boundary's step, by kind
  a_f64               19951 -> 20354    68    k_flush_mfma<double,128,4,64>   2.1-2.2 ms  0.05-1.9; every kind 4-7 times of 7 within 1.6
  b_f32_mixed         19903 -> 20481   196    k_flush_mfma32<256,4,2,3,early> 1.53 ms     0.08-1.5; every kind 3-5 times of 5 within 1.14
  c_f32_split         19903 -> 20481   196    k_flush_split3<2>               1.56 ms     0.10-1.7; every kind 3-5 times of 5 within 1.17
  d_f64_two_shards    19951 -> 20354    68    k_flush_mfma<double,128,4,64>   2.05 ms     0.17-1.9; every kind 4-7 times of 7 within 1.5
  edits               19951 -> 20354    68    k_flush_mfma<double,128,4,64>   2.2 ms      remove 0.10, merge 0.05, merge batch 0.03

(The first boundary of a fresh process pays the queries' first allocations, 70-200 ms: those occurrences fall outside.)  The boundary's own
step first waits for the main stream: without that the first query behind a boundary waits ~1.3 ms for the gathers the host ran ahead of,
and only one query per boundary fits.

F64 (a, d, edits): asynchronous equals synchronous bit for bit, the queries' results included; against the oracle x 4e-16, rows 1.3e-13.
No fault of passes.h, append_model.h, the gathers or the edits was found.

Float tiles (b, c), with the inputs of beside_pass_cases.PLAN_INPUTS (its comment says why they differ from the F64 legs'): against the
oracle, mixed / split, both engines: rows 1.35e-7 / 1.17e-7 (bar 2e-7 of 14.9 / 10.7), x 5.0e-12 / 5.7e-12 (1.4e-9), robot strip
2.0e-9 / 1.7e-9 (3.2e-9), diagonal blocks 2.1e-10 / 5.3e-10 (3.2e-9); sensitivity 31 / 43 row tolerances over two batches, 406 / 559 in
the appended rows.  With the F64 legs' inputs the SYNCHRONOUS engine alone has rows 1.2e-6, strip 2.6e-8, diagonal blocks 5.3e-8; with
only the append noise raised (x 20, turns of 0.5 degrees, appends within 15) rows 1.1e-7 but strip 3.2e-8; with R x 100 and noise x 50
but the newest tile rows' first landmark as the edge target, rows 2.3e-7 and strip 1.9e-8.
The queries on float tiles are NOT bit for bit between the two engines and cannot be: every query reads x, and x differs (within the
float bar) because the two schedules' gathers read a tile once as the pass rounded it and once as the old store patched in F64.  All four
are therefore held to the float bar, 2 x 3.2e-9 relative, as provided for a result that tile reads make differ: measured nu 1.2e-9 /
2.1e-9, S 1.4e-10, d2 2.3e-9 / 4.2e-9, d2_all 2.8e-9 / 2.4e-9, d2_prefix 1.9e-9 / 1.8e-9.
"""


def _engines(leg_row, cap):
    from ekf_slam_amd import Engine
    from ekf_slam_amd.sharding import ShardGroup
    storage, T, batch, _, _, shards, _ = leg_row
    kw = dict(mode="known", capacity=cap, storage=storage, batch=batch)
    syn = Engine(**kw)
    asy = ShardGroup(shards, async_flush=True, **kw) if shards else Engine(async_flush=True, **kw)
    return syn, asy, (asy.shards if shards else [asy])


def _drive_alone(asy, aengines, steps, batch):
    """The asynchronous engine through the plan with nothing else on the host between its calls but the clock and, around a query,
    pending().  Returns (gaps: kind -> host ms from the boundary's step to each tested call of that kind, the queries' results, the pass
    kernel's names at the last boundary, the pending() pairs around the queries)."""
    boundary, gaps, results, pend, names = {}, {}, [], [], None
    first = aengines[0]
    for t, ops in enumerate(steps):
        k_b = (t + 1) // batch
        for q, (kind, payload, tested) in enumerate(ops):
            query = kind in B.QUERY_KINDS
            if query:
                before = first.pending()
            now = time.perf_counter()
            res = B.issue(asy, kind, payload)
            if q == len(ops) - 1 and (t + 1) % batch == 0:
                boundary[k_b] = now
            elif tested and kind != "predict":
                gaps.setdefault(kind, []).append(1e3 * (now - boundary[k_b]))
            if query:
                pend.append((before, first.pending()))
                results.append(res)
        if (t + 1) % batch == 0:
            names = tuple(e.downdate_kernel_name()[0] for e in aengines)
    return gaps, results, names, pend


def _passes(aengines):
    from ekf_slam_amd import _lib as L
    out = []
    for e in aengines:
        cnt, ms = e.timing_read(L.EKF_KERNEL_DOWNDATE)
        out.append((cnt, ms / max(cnt, 1)))
    return out


def _assert_premise(leg, gaps, passes, names, kernel, batches):
    mean = max(m for _, m in passes)
    print("%s: pass kernel %s; asynchronous passes per engine (count, mean ms): %s" % (leg, names, passes))
    for kind, g in sorted(gaps.items()):
        print("%s:   host ms from the boundary's step to %-24s %s" % (leg, kind + ":", " ".join("%.3f" % v for v in g)))
    assert all(nm.startswith(kernel) for nm in names), names
    # about one pass per batch (the four steps behind the last boundary are still pending); a query that started one would show here
    assert all(batches - 1 <= cnt <= batches + 1 and m >= 0.5 for cnt, m in passes), passes
    # the premise: every kind of call at least twice within 3/4 of a pass of the pass's launch (the run-ahead throttle blocks now and then)
    for kind, g in gaps.items():
        assert sum(v <= 0.75 * mean for v in g) >= 2, (kind, g, mean)


def _query_difference(a, b, worst):
    """worst[key]: largest relative difference of that entry between two query results (dicts of arrays), kept over the calls; whole
    numbers and the places of NaN must agree"""
    for key in a:
        va, vb = np.asarray(a[key]), np.asarray(b[key])
        if va.dtype.kind in "iub":
            np.testing.assert_array_equal(va, vb, err_msg=key)
            continue
        np.testing.assert_array_equal(np.isnan(va), np.isnan(vb), err_msg=key)
        ok = ~np.isnan(vb)
        if ok.any():
            worst[key] = max(worst.get(key, 0.0), float(np.abs(va[ok] - vb[ok]).max() / max(np.abs(vb[ok]).max(), 1e-300)))


def _no_rejections(engines):
    for e in engines:
        assert e.linear_rejections() == (0, 0)


@pytest.mark.parametrize("leg", list(B.LEGS))
def test_calls_issued_while_a_pass_is_in_flight(leg):
    from ekf_slam_amd import _lib as L
    from oracle.ekf_factored import FactoredEKF
    storage, T, batch, batches, kernel, shards, _ = B.LEGS[leg]
    N0 = async_cases.placement(T, batch)[0]
    (x, s, d, U), steps, info = B.leg_inputs(leg, N0)
    cap, appended = info["N"], info["appended"]
    tested = B.kinds_of(steps, tested_only=True)
    print("%s: %s, tile %d, batch %d: %d -> %d landmarks in %d steps; calls behind a boundary %s; %d of %d tested scans cross a tile-row edge"
          % (leg, storage, T, batch, N0, cap, len(steps), tested, info["crossing_scans"], tested["append_model"]))
    assert info["crossing_scans"] >= 3 and all(v >= 3 for v in tested.values())

    syn, asy, aengines = _engines(B.LEGS[leg], cap)
    ref = FactoredEKF(cap, "known", max_terms=len(steps) + 4, max_appends=len(appended))
    for e in (syn, asy, ref):
        e.load_lowrank_state(x, s, d, U)
    for e in aengines:
        e.timing_enable(L.EKF_KERNEL_DOWNDATE, True, launches=batches + 8)

    # 1. the asynchronous engine ALONE
    gaps, res_a, names, pend = _drive_alone(asy, aengines, steps, batch)
    passes = _passes(aengines)
    _assert_premise(leg, gaps, passes, names, kernel, batches)
    assert all(a == b for a, b in pend), pend                        # a query changes nothing that is pending

    # 2. the synchronous twin on the same plan
    res_s = []
    for ops in steps:
        for kind, payload, _ in ops:
            res = B.issue(syn, kind, payload)
            if kind in B.QUERY_KINDS:
                res_s.append(res)
    assert syn.N == cap and asy.N == cap
    _no_rejections([syn] + aengines)

    # 3. the oracle, with its sampled rows two batch boundaries apart
    snaps = B.run_oracle(ref, steps, batch, T)
    assert ref.N == cap
    tol_x, tol_P, tol_rows = B.tolerances(storage, len(steps))
    scale, moved, app_margin, ro_app = B.sensitivity(ref, snaps, appended, T, tol_rows)
    print("%s: sensitivity in row tolerances (%.2g of %.3g): smallest per-tile change of the sampled rows over two batches %.1f; smallest "
          "per-tile largest entry of the %d appended rows %.1f" % (leg, tol_rows, scale, moved, len(appended), app_margin))
    assert moved >= 20.0 and app_margin >= 20.0

    n = 3 + 2 * cap
    sampled = async_cases.sampled_landmarks(cap, T)
    lms = sampled + appended
    ro = np.concatenate([async_cases.oracle_rows(ref, sampled), ro_app])
    rs = async_cases.engine_rows(syn, lms, n)
    ra = async_cases.engine_rows(asy, lms, n)
    xs, xa = syn.get_x(), asy.get_x()
    ds, da = syn.digest(), asy.digest()
    Ds, Da = syn.get_P_diag_blocks(), aengines[0].get_P_diag_blocks()
    Dref = ref.diag_blocks()

    def report(rows, xv, Dv):
        pos = np.argwhere(np.abs(rows - ro) > tol_rows * scale)
        first = None
        if len(pos):
            q, _, c = pos[0]
            first = "landmark %d (tile row %d%s), column %d (tile column %d)" % (
                lms[q], 2 * lms[q] // T, ", appended" if q >= len(sampled) else "", c, max(c - 3, 0) // T)
        eq, _, ec = np.unravel_index(np.abs(rows[:, :, :3] - ro[:, :, :3]).argmax(), (len(lms), 2, 3))
        return {"worst_robot_entry": "landmark %d, column %d, %.3g of largest %.3g" % (lms[eq], ec, np.abs(ro[eq, :, ec]).max(), np.abs(ro[:, :, :3]).max()),
                "rows": float(np.abs(rows - ro).max()) / scale, "appended_rows": float(np.abs(rows - ro)[len(sampled):].max()) / scale,
                "x": rel_err(xv, ref.x), "robot_rows": rel_err(rows[:, :, :3], ro[:, :, :3]),
                "diag_blocks": float(np.abs(Dv[1:] - Dref).max() / np.abs(Dref).max()), "first_row_outside": first}

    es, ea = report(rs, xs, Ds), report(ra, xa, Da)
    print("%s: errors against the oracle (tolerances x %.2g, F64-kept %.2g, rows %.2g of %.3g): sync %s, async %s"
          % (leg, tol_x, tol_P, tol_rows, scale, es, ea))
    qdiff = {}
    for a, b in zip(res_a, res_s):
        _query_difference(a, b, qdiff)
    assert len(res_a) == len(res_s) == sum(v for k, v in B.kinds_of(steps).items() if k in B.QUERY_KINDS)
    print("%s: largest relative difference of the queries' results, asynchronous against synchronous: %s"
          % (leg, {k: float("%.3g" % v) for k, v in qdiff.items()}))
    if storage == "f64":
        # the asynchronous schedule runs the same kernels on the same operands in the same order: bit for bit
        bad = np.argwhere(ra != rs)
        assert bad.size == 0, "%s: async rows differ from sync at landmark %d (tile row %d), column %d: %r vs %r" % (
            leg, lms[bad[0][0]], 2 * lms[bad[0][0]] // T, bad[0][2], ra[tuple(bad[0])], rs[tuple(bad[0])])
        np.testing.assert_array_equal(xa, xs)
        np.testing.assert_array_equal(Da, Ds)
        if shards:
            np.testing.assert_allclose(da, ds, rtol=1e-12)         # the shards' digests add in another order
        else:
            np.testing.assert_array_equal(da, ds)
        for a, b in zip(res_a, res_s):
            for key in a:
                np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    else:
        # float tiles: the pass's stores interleave differently with the gathers' reads (tests/test_f32_mixed_gpu.py), not bitwise
        assert rel_err(xa, xs) <= 2 * tol_x
        assert float(np.abs(ra - rs).max()) <= 2 * tol_rows * scale, (leg, float(np.abs(ra - rs).max()) / scale)
        assert float(np.abs(Da - Ds).max()) <= 2 * tol_P * float(np.abs(Ds).max())
        assert float(np.max(np.abs(da - ds) / np.abs(ds))) <= 2 * tol_P
        assert ea["rows"] <= max(es["rows"], tol_rows / 2), (es, ea)      # the async rows are not the less accurate ones
    for tag, r in (("sync", es), ("async", ea)):
        assert r["rows"] <= tol_rows and r["x"] <= tol_x and r["robot_rows"] <= tol_P and r["diag_blocks"] <= tol_P, (leg, tag, r)
    if storage != "f64":
        # The queries on float tiles.  Every query reads x, and on float tiles x is not bit for bit (above: within 2 tol_x): the gathers of
        # the two schedules read the same tile once as the pass rounded it and once as the old store patched in F64.  That is the case the
        # float bar is for -- a result that differs because of tile reads -- and it reaches every query through x, not joint_innovation alone.
        assert max(qdiff.values()) <= 2 * tol_P, qdiff
    syn.close(); asy.close()


def test_map_edits_issued_while_a_pass_is_in_flight():
    """remove_landmarks on three landmarks of different tile rows, merge_landmarks and merge_landmarks_batch with 4 pairs, each once, as the
    first call behind a boundary; two more batches follow.  The asynchronous engine equals its synchronous twin bit for bit (the factored
    oracle does not follow removals; the small-map tests hold the edits' arithmetic to NumPy)."""
    from ekf_slam_amd import _lib as L
    storage, T, batch, batches, kernel, _, key = B.EDITS_LEG
    N0 = async_cases.placement(T, batch)[0]
    sigma, sigma_robot, RC = async_cases.INPUTS[key]
    (x, s, d, U), _ = async_cases.make_inputs(N0, 0, sigma, sigma_robot, RC)
    steps, info = B.make_plan(x, T, batch, batches, RC, edits=True)
    tested = B.kinds_of(steps, tested_only=True)
    assert all(tested.get(k, 0) == 1 for k in B.EDIT_KINDS), tested
    cap = N0 + B.appended_total(steps)
    syn, asy, aengines = _engines(B.EDITS_LEG, cap)
    for e in (syn, asy):
        e.load_lowrank_state(x, s, d, U)
    asy.timing_enable(L.EKF_KERNEL_DOWNDATE, True, launches=4 * batches)

    gaps, res_a, names, pend = _drive_alone(asy, aengines, steps, batch)
    passes = _passes(aengines)
    mean = passes[0][1]
    print("edits: pass kernel %s; asynchronous passes (count, mean ms): %s" % (names, passes))
    for kind in B.EDIT_KINDS:
        print("edits:   host ms from the boundary's step to %-24s %.3f" % (kind + ":", gaps[kind][0]))
    assert names[0].startswith(kernel) and passes[0][0] >= batches - 1 and mean >= 0.5, (names, passes)
    for kind in B.EDIT_KINDS:
        assert gaps[kind][0] <= 0.75 * mean, (kind, gaps[kind], mean)
    assert all(a == b for a, b in pend), pend

    for ops in steps:
        for kind, payload, _ in ops:
            B.issue(syn, kind, payload)
    assert syn.N == asy.N == info["N"]
    _no_rejections([syn, asy])
    N = syn.N
    lms = async_cases.sampled_landmarks(N, T)
    rs, ra = async_cases.engine_rows(syn, lms, 3 + 2 * N), async_cases.engine_rows(asy, lms, 3 + 2 * N)
    bad = np.argwhere(ra != rs)
    assert bad.size == 0, "edits: async rows differ from sync at landmark %d (tile row %d), column %d: %r vs %r" % (
        lms[bad[0][0]], 2 * lms[bad[0][0]] // T, bad[0][2], ra[tuple(bad[0])], rs[tuple(bad[0])])
    np.testing.assert_array_equal(asy.get_x(), syn.get_x())
    np.testing.assert_array_equal(asy.get_s(), syn.get_s())
    np.testing.assert_array_equal(asy.get_P_diag_blocks(), syn.get_P_diag_blocks())
    np.testing.assert_array_equal(asy.digest(), syn.digest())
    syn.close(); asy.close()
