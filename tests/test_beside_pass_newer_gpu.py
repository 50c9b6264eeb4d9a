"""GPU: the map calls and the joint updates issued while an asynchronous pass is in flight -- tests/test_beside_pass_gpu.py's premise for
the nine entry points added since: at ~20 000 landmarks (async_cases.placement(128, 8)) a pass lasts milliseconds and outlasts the host's
next call, so the ORDER between the pass stream and the main stream is exercised, not only the bookkeeping.

  * the synchronising calls (settle, materialize_predict, flush_pending -> retire_inflight, then kernels of their own on the main stream):
    observe_model_joint, observe_model_joint_iterated, join_map, extract_map, transform_map, factor_map -- each as the FIRST call behind a
    batch boundary, and five of them once more directly behind an append_model scan that has just carried the map over a tile-row edge
    beside the pass: the row copy is then queued on the pass stream behind the pass and the call's kernels walk the new rows straight after;
  * the calls that leave the pass alone: observe_model_assigned (one pair slot per entry; two scans straddle a batch boundary, so that a
    pass starts between two of their gathers), assign_model and joint_search in every place 1-4 behind a boundary;
  * the second handle of the two-handle calls with a pass of ITS OWN in flight: extract_map into such a destination, join_map of such a
    local map with an append beside the pass in front of the join.

The plan is beside_pass_cases.make_plan(newer=True), a pure function of the loaded state (tests/test_beside_pass_plan_cpu.py holds it to
the dense forms without a GPU).  The asynchronous engine is driven ALONE through it; its synchronous twin follows.  F64 tiles run the same
kernels on the same operands in the same order, so everything is compared bit for bit: x, s, the diagonal blocks, the digest, the two rows
over all columns of one landmark per tile row and of every landmark append_model or join_map added, every returned value, the whole state
of every extracted destination.  The arithmetic of each call is held to NumPy by the small-map files and, for the composition, by
test_the_newer_plan_against_the_dense_forms below; the at-size tests are about order.

No float-tile leg, deliberately: on float tiles the two schedules are not bit for bit (test_beside_pass_gpu.py says why), retire_inflight
and the row copy are exercised per storage kind by that file's legs b and c, and a float bar for these calls would be an unmeasured number.

The premise is asserted from the host clock and the pass timers, as there.  factor_map times its column launches under the pass's timer
id, so the timer is read (which waits) at an untested step in front of a factor_map window and straight behind the call, and that interval
-- the window's own pass and the factorisation -- is left out of the mean; everywhere else the count of timed launches must be exactly one
per boundary and one per joint update (its own in-place pass): a query or an assigned scan that started a pass would show there.

Sizes and the measured premise (MI355X): see MEASURED below."""
import time

import numpy as np
import pytest

import async_cases
import beside_pass_cases as B
import helpers
from test_beside_pass_gpu import _engines, _passes

pytestmark = pytest.mark.gpu

MEASURED = """
On an MI355X, at the size of async_cases.placement(128, 8) (test_beside_pass_gpu.py's MEASURED says why no leg is halved):

(a) 19951 -> 20674 landmarks, 162 steps, 21 batches of 8 pair slots; pass kernel k_flush_mfma<double,128,4,64>; outside the two factor_map
    windows 22 timed launches = 19 boundaries + 3 joint updates, mean 2.14-2.20 ms, so "beside the pass" is within 1.60-1.65 ms.  Host ms
    from the boundary's step to the call:
      observe_model_joint 0.057 0.067   observe_model_joint_iterated 0.077   join_map 0.108 0.082   extract_map 0.039 0.068
      transform_map 0.093 0.089 0.077   factor_map 0.085 0.084              (every synchronising occurrence: 0.04-0.11 of 1.6)
      observe_model_assigned 0.075 0.079 (the straddling scans, start to return) 1.54 1.50 (the scans of 3 in place 4)
      assign_model 0.06-1.06 (6 of 6 within)   joint_search 0.06-0.93 (6 of 6 within)   append_model 0.05-0.79 (11 of 11)
      the older kinds as in test_beside_pass_gpu.py: 0.06-1.9, each at least twice within.
    factor_map's two windows: 627 and 646 launches under the pass's timer id, 0.98 and 1.07 s (the extrapolated 1.3 s was not measured).
    Asynchronous equals synchronous bit for bit in everything compared.  Device bytes 34.6 GB (asynchronous 20.8, synchronous 13.8).
    Asynchronous run 2.4 s, synchronous run 2.4 s, the whole test 8.4 s (the plan 2.3 s of it).
(b) extract_map into a destination 0.157 ms behind its boundary's step (its passes: 2, mean 2.14 ms); join_map of a local map 0.071 ms
    behind its boundary's step with an append_model scan of 6 across a tile-row edge in between (its passes: 2, mean 2.06 ms).  Bit for bit
    against the twin pairs.  Summed device bytes of the six engines 51.9 GB (at most four of them alive at once); the whole test 2.6 s.
Small, against the dense forms: tile 16, 175 -> 346 landmarks: x 1.2e-15, P 4.7e-15, factor_map's logdet 1.0e-15, pivots 7.8e-15, d2 4.0e-15;
    extracted destinations 1.2e-15; 4.5 s.  Tile 64, 751 -> 1186 landmarks: x 1.5e-16, P 3.5e-15, logdet 3.0e-15, pivots 1.5e-14, d2 2.2e-15,
    extracted destinations 1.6e-15; 19-22 s, nearly all of it the dense forms on the host (24 tile rows of 64 are that large).

Sensitivity, checked once on a scratch build and not kept: with retire_inflight's row copy skipped (the landmarks appended beside the pass
then never reach the new store), (a) fails at the first synchronising call behind a crossing scan -- factor_map at step 32 reports P not
definite at index 39907, a row of that scan, where the twin reports definite.  No fault of passes.h, append_model.h or the nine entry
points' host code was found.
"""

LEG = B.LEGS["a_f64"]                        # f64, tile 128, batch 8: the pass kernel k_flush_mfma<double,128,..>
WITHIN = 0.75                                # of the mean pass: what "issued while the pass runs" means here, as in test_beside_pass_gpu.py


def _newer_inputs(T, batch, N0):
    sigma, sigma_robot, RC = async_cases.INPUTS[LEG[6]]
    state, _ = async_cases.make_inputs(N0, 0, sigma, sigma_robot, RC)
    steps, info = B.make_plan(state[0], T, batch, B.NEWER_BATCHES, RC, newer=True)
    return state, steps, info


def _source_blocks(src, idx):
    """P over the robot and the landmarks idx as get_P_block reads it from the source, row panel by row panel"""
    n = 3 + 2 * src.N
    sel = np.concatenate([np.arange(3)] + [[3 + 2 * k, 4 + 2 * k] for k in idx])
    rows = [src.get_P_block(0, 0, 3, n)] + [src.get_P_block(3 + 2 * k, 0, 2, n) for k in idx]
    return np.concatenate(rows)[:, sel], sel


def _check_map_extraction(src, dst, idx):
    """independent of any twin: a map-frame extraction is an indexing, 'every value keeping its bits'"""
    P, sel = _source_blocks(src, idx)
    np.testing.assert_array_equal(dst.get_P(), P)
    np.testing.assert_array_equal(dst.get_x(), src.get_x()[sel])
    np.testing.assert_array_equal(dst.get_s(), src.get_s()[np.asarray(idx)])


def _drive(eng, steps, info, batch, timed=False):
    """test_beside_pass_gpu.py's _drive_alone for a plan whose boundaries count pair slots (info['boundaries']) and whose calls return more
    than query dicts.  An engine through the newer plan with nothing else on the host between its calls but the clock and pending(): around a query, behind
    a synchronising call (where the pass is retired and nothing of the window is under test any more: a map-frame extraction is checked
    against its source there, the timer read behind factor_map).  The second handles are made ahead.  Returns a dict: 'gaps' (kind -> [(host
    ms from the boundary's step to the call, step)]; for a straddling scan the ms from its start to its return, which bounds how long
    behind the pass's launch its last gather was issued), 'results' [(step, kind, what the call returned)], 'pend' [(kind, pending()
    before or None, after)], 'clean' / 'dirty' [(count, total ms)] of the pass timer, 'names' (the pass kernel at the last boundary)."""
    from ekf_slam_amd import _lib as L
    second = iter(B.second_handles(steps))
    places = B.places(steps, batch)
    factor_steps = [t for t, ops in enumerate(steps) if any(op[0] == "factor_map" for op in ops)]
    read_before = {max(q for q in range(t) if places[q][0] == 5) for t in factor_steps} if timed else set()
    out = dict(gaps={}, results=[], pend=[], clean=[], dirty=[], names=None)
    boundary, scan_at = {}, None

    def read(into):
        cnt, ms = eng.timing_read(L.EKF_KERNEL_DOWNDATE)
        out[into].append((cnt, ms))

    def fetch():
        out["results"].append((scan_at, B.NEWER_PAIR_KIND, eng.assigned_scan_result()))

    for t, ops in enumerate(steps):
        p, k_b, _ = places[t]
        if t in read_before:
            read("clean")
        if scan_at is not None and not any(op[2] for op in ops):
            fetch()                                             # (the scan's own event, at an untested step)
            scan_at = None
        for q, (kind, payload, tested) in enumerate(ops):
            if kind == B.NEWER_PAIR_KIND and scan_at is not None:
                fetch()
            query = kind in B.QUERY_KINDS + B.NEWER_QUERY_KINDS
            before = eng.pending() if query else None
            now = time.perf_counter()
            res = B.issue(eng, kind, payload, second)
            done = time.perf_counter()
            ends_batch = q == len(ops) - 1 and t in info["boundaries"]
            if ends_batch:
                boundary[info["boundaries"][t]] = now
                if t in info["straddlers"]:
                    out["gaps"].setdefault(kind, []).append((1e3 * (done - now), t))
            elif tested and kind != "predict":
                out["gaps"].setdefault(kind, []).append((1e3 * (now - boundary[k_b]), t))
            if query or kind in B.SYNC_KINDS:
                out["pend"].append((kind, before, eng.pending()))
            if kind == B.NEWER_PAIR_KIND:
                scan_at = t
            elif res is not None:
                out["results"].append((t, kind, res))
            if kind == "extract_map" and payload[1] == "map":
                _check_map_extraction(eng, res, payload[0])
            if kind == "factor_map" and timed:
                read("dirty")
        if t in info["boundaries"]:
            out["names"] = eng.downdate_kernel_name()[0]
    if scan_at is not None:
        fetch()
    if timed:
        read("clean")
    return out


def _same_result(t, kind, a, b):
    where = "%s at step %d" % (kind, t)
    if kind == "join_map":
        assert a[0] == b[0], where
    elif kind == "extract_map":
        helpers.assert_same(a, b)
    else:
        assert set(a) == set(b), where
        for key in a:
            np.testing.assert_array_equal(a[key], b[key], err_msg="%s: %s" % (where, key))


def _same_at_size(a, b, T, extra=()):
    """x, s, the diagonal blocks, the digest and the sampled rows (and those of `extra`) of two engines at size, bit for bit"""
    N = a.N
    assert N == b.N
    lms = async_cases.sampled_landmarks(N, T) + list(extra)
    ra, rb = async_cases.engine_rows(a, lms, 3 + 2 * N), async_cases.engine_rows(b, lms, 3 + 2 * N)
    bad = np.argwhere(ra != rb)
    assert bad.size == 0, "rows differ at landmark %d (tile row %d), column %d: %r vs %r" % (
        lms[bad[0][0]], 2 * lms[bad[0][0]] // T, bad[0][2], ra[tuple(bad[0])], rb[tuple(bad[0])])
    np.testing.assert_array_equal(a.get_x(), b.get_x())
    np.testing.assert_array_equal(a.get_s(), b.get_s())
    np.testing.assert_array_equal(a.get_P_diag_blocks(), b.get_P_diag_blocks())
    np.testing.assert_array_equal(a.digest(), b.digest())


def test_newer_calls_issued_while_a_pass_is_in_flight():
    from ekf_slam_amd import _lib as L
    storage, T, batch, _, kernel, _, _ = LEG
    t_start = time.perf_counter()
    N0 = async_cases.placement(T, batch)[0]
    (x, s, d, U), steps, info = _newer_inputs(T, batch, N0)
    cap = info["N"]
    tested = B.kinds_of(steps, tested_only=True)
    print("newer: %d -> %d landmarks in %d steps, %d batches; calls behind a boundary %s; behind a crossing scan %s; straddling scans at %s"
          % (N0, cap, len(steps), B.NEWER_BATCHES, tested, info["behind_scan"], info["straddlers"]))
    assert len(info["behind_scan"]) == 5 and len(info["straddlers"]) == 2
    syn, asy, _ = _engines(LEG, cap)
    for e in (syn, asy):
        e.load_lowrank_state(x, s, d, U)
    asy.timing_enable(L.EKF_KERNEL_DOWNDATE, True, launches=1024)

    # 1. the asynchronous engine ALONE, then its synchronous twin
    t_run = time.perf_counter()
    ra = _drive(asy, steps, info, batch, timed=True)
    t_asy = time.perf_counter() - t_run
    rs = _drive(syn, steps, info, batch)
    t_syn = time.perf_counter() - t_run - t_asy
    assert syn.N == asy.N == cap

    # 2. the premise
    cnt = sum(c for c, _ in ra["clean"])
    mean = sum(ms for _, ms in ra["clean"]) / max(cnt, 1)
    joint = sum(1 for ops in steps for op in ops if op[0].startswith("observe_model_joint"))
    print("newer: pass kernel %s; timed launches outside the factor_map windows %d (%d boundaries there, %d joint updates), mean %.3f ms; "
          "in the factor_map windows (count, ms) %s" % (ra["names"], cnt, B.NEWER_BATCHES - 2, joint, mean, ra["dirty"]))
    for kind, g in sorted(ra["gaps"].items()):
        print("newer:   host ms from the boundary's step to %-30s %s" % (kind + ":", " ".join("%.3f" % v for v, _ in g)))
    assert ra["names"].startswith(kernel), ra["names"]
    assert cnt == B.NEWER_BATCHES - 2 + joint and mean >= 0.5, (ra["clean"], mean)
    for kind, g in ra["gaps"].items():
        if kind in B.SYNC_KINDS:
            assert all(v <= WITHIN * mean for v, _ in g), (kind, g, mean)            # every synchronising occurrence meets its pass
        else:
            assert sum(v <= WITHIN * mean for v, _ in g) >= 2, (kind, g, mean)
    assert set(B.SYNC_KINDS + B.NEWER_QUERY_KINDS + (B.NEWER_PAIR_KIND, "append_model")) <= set(ra["gaps"])

    # 3. pending(): 0 behind every synchronising call, unchanged around every query
    for run in (ra, rs):
        for kind, before, after in run["pend"]:
            assert after == (0 if kind in B.SYNC_KINDS else before), (kind, before, after)

    # 4. every returned value, bit for bit
    assert [(t, k) for t, k, _ in ra["results"]] == [(t, k) for t, k, _ in rs["results"]]
    by_step = {t: ops for t, ops in enumerate(steps)}
    for (t, kind, a), (_, _, b) in zip(ra["results"], rs["results"]):
        _same_result(t, kind, a, b)
        if kind == "factor_map":
            assert b["definite"] and a["definite"] and np.all(np.isfinite(b["d2"])), (t, b)
        if kind == B.NEWER_PAIR_KIND:
            # the scan had no choice: the synchronous engine assigned every entry to the landmark it sights, its only candidate
            np.testing.assert_array_equal(b["landmark"], by_step[t][-1][1][1])
            np.testing.assert_array_equal(b["ncand"], 1)
            assert np.all(b["outcome"] == L.EKF_LINEAR_APPLIED)
        if kind in ("observe_model_joint", "observe_model_joint_iterated"):
            assert b["outcome"] == L.EKF_LINEAR_APPLIED and b["pairings"] >= 6
    for run in (ra, rs):
        for _, kind, res in run["results"]:
            if kind == "extract_map":
                res.close()
            elif kind == "join_map":
                res[1].close()
    for e in (syn, asy):
        assert e.linear_rejections() == (0, 0)

    # 5. the state
    _same_at_size(asy, syn, T, info["appended"])
    print("newer: device bytes %.1f GB (asynchronous %.1f, synchronous %.1f); asynchronous run %.1f s, synchronous run %.1f s, whole test %.1f s"
          % ((asy.device_bytes() + syn.device_bytes()) / 1e9, asy.device_bytes() / 1e9, syn.device_bytes() / 1e9, t_asy, t_syn,
             time.perf_counter() - t_start))
    syn.close(); asy.close()


# ------------------------------------------------------------------------------------------------------------------
# the second handle
# ------------------------------------------------------------------------------------------------------------------
def _to_second_boundary(e, steps, info_boundary=15):
    """an engine through the first two batches of the plain plan: its second boundary's pass has just been queued when this returns.
    Returns the host clock at the boundary's step."""
    now = None
    for t, ops in enumerate(steps[:info_boundary + 1]):
        for q, (kind, payload, _) in enumerate(ops):
            if t == info_boundary and q == len(ops) - 1:
                now = time.perf_counter()
            B.issue(e, kind, payload)
    return now


def _nominal_after(x, steps):
    """the plan's nominal state behind `steps`, replayed from the plan alone"""
    import append_model_cases as A
    nom = B.Nominal(x)
    for ops in steps:
        for kind, payload, _ in ops:
            if kind == "predict":
                nom.predict(payload)
            elif kind == "predict_model":
                nom.predict_model(payload)
            elif kind == "append_model":
                for model, z, _, _ in payload:
                    nom.append(A.g_of(model, nom.pose, z))
    return nom


def _eight_more(e, twin, RC):
    """eight corrections on both: with batch 8 the asynchronous one starts a pass at the eighth, and reading the state retires it"""
    x = twin.get_x()
    N = twin.N
    for q in range(8):
        k = (q * 37 + 5) % N
        dlt = x[3 + 2 * k:5 + 2 * k] - x[:2]
        z = np.array([np.hypot(*dlt), (np.degrees(np.arctan2(dlt[1], dlt[0])) - x[2]) % 360.0])
        for g in (e, twin):
            g.predict([0.0, 0.0])
            g.correct(z + [0.01, 0.2], np.diag([z[0] * RC[0], z[1] * RC[1]]), k)
    assert e.pending() == 8 and twin.pending() == 0             # (the eight pairs are frozen in the pass in flight; the twin's pass ran in place)


def test_the_second_handle_has_a_pass_in_flight():
    """extract_map into a destination, and join_map of a local map, whose OWN asynchronous pass is in flight -- retire_inflight(dst) then
    clear_pairs(dst) then writes in place on dst's stream; the local map's retire and row copy (an append_model scan that crossed a tile-row
    edge beside the pass stands in front of the join) before the join's kernels read its tiles.  Each against a twin pair whose second
    handle is synchronous, bit for bit."""
    from ekf_slam_amd import Engine
    from ekf_slam_amd import _lib as L
    from removal_cases import lowrank_data
    storage, T, batch, _, kernel, _, key = LEG
    t_start = time.perf_counter()
    N0 = async_cases.placement(T, batch)[0]
    sigma, sigma_robot, RC = async_cases.INPUTS[key]
    (x, s, d, U), steps, info = B.leg_inputs("a_f64", N0)           # the plain plan: only its first two batches are driven
    cap = N0 + B.appended_total(steps[:17]) + 8
    kw = dict(mode="known", capacity=cap, storage=storage, batch=batch)
    total_bytes = 0

    def at_size(**more):
        e = Engine(**kw, **more)
        e.load_lowrank_state(x, s, d, U)
        return e

    # ---- extract_map(into=dst) ----
    src = at_size()
    idx = B.extract_indices(B.Nominal(x), np.random.default_rng(5), T // 2)
    digest_before = src.digest()
    dst_a, dst_s = at_size(async_flush=True), at_size()
    dst_a.timing_enable(L.EKF_KERNEL_DOWNDATE, True, launches=16)
    t_b = _to_second_boundary(dst_a, steps)
    t_call = time.perf_counter()
    assert src.extract_map(idx, "map", into=dst_a) is dst_a
    gap_extract = 1e3 * (t_call - t_b)
    (cnt, mean_extract), = _passes([dst_a])
    _to_second_boundary(dst_s, steps)
    src.extract_map(idx, "map", into=dst_s)
    print("second handle: extract_map into a destination %.3f ms behind its boundary's step; its passes (count, mean ms) (%d, %.3f), kernel %s"
          % (gap_extract, cnt, mean_extract, dst_a.downdate_kernel_name()[0]))
    assert cnt == 2 and mean_extract >= 0.5 and gap_extract <= WITHIN * mean_extract
    assert dst_a.pending() == dst_s.pending() == src.pending() == 0 and dst_a.N == dst_s.N == len(idx)
    np.testing.assert_array_equal(src.digest(), digest_before)
    helpers.assert_same(dst_a, dst_s)                               # the whole state: x, s, P, the diagonal blocks, the digest
    _check_map_extraction(src, dst_a, idx)
    _eight_more(dst_a, dst_s, RC)
    helpers.assert_same(dst_a, dst_s)
    total_bytes += sum(e.device_bytes() for e in (src, dst_a, dst_s))
    dst_a.close(); dst_s.close()

    # ---- join_map(local) ----
    nom = _nominal_after(x, steps[:16])
    before, half = nom.N, T // 2
    scan, _ = B.append_scan(nom, np.random.default_rng(6), 6, 3.0e6)
    # (the filler scans of the second batch left the map a landmark or two in front of a tile-row edge: the scan crosses it)
    assert before % half != 0 and (before - 1) // half != (nom.N - 1) // half, (before, nom.N)
    xs, ss, ds, Us = lowrank_data(200, 5)
    small_kw = dict(mode="known", capacity=200 + cap + 8, storage=storage, batch=batch, tile=T)
    runs = []
    for local in (at_size(async_flush=True), src):                 # (the extraction left its source as it was: it is the twin's local map)
        small = Engine(**small_kw)
        small.load_lowrank_state(xs, ss, ds, Us)
        asy = local is not src
        if asy:
            local.timing_enable(L.EKF_KERNEL_DOWNDATE, True, launches=16)
        t_b = _to_second_boundary(local, steps)
        first_new = local.append_model(scan)
        t_call = time.perf_counter()
        first = small.join_map(local, 5.0e6)
        if asy:
            gap_join = 1e3 * (t_call - t_b)
            (cnt, mean_join), = _passes([local])
            print("second handle: join_map of a local map %.3f ms behind its boundary's step, an append_model scan of 6 in between; its passes "
                  "(count, mean ms) (%d, %.3f)" % (gap_join, cnt, mean_join))
            assert cnt == 2 and mean_join >= 0.5 and gap_join <= WITHIN * mean_join
        assert first == 200 and first_new == nom.N - 6 and local.N == nom.N and small.N == 200 + nom.N
        assert small.pending() == 0 and local.pending() == 0
        runs.append((small, local))
    (small_a, local_a), (small_s, local_s) = runs
    new = [200 + k for k in range(nom.N - 6, nom.N)]                # the scan's landmarks in the joined map
    _same_at_size(small_a, small_s, T, new)
    _same_at_size(local_a, local_s, T, list(range(nom.N - 6, nom.N)))
    _eight_more(local_a, local_s, RC)
    _same_at_size(local_a, local_s, T)
    total_bytes += sum(e.device_bytes() for e in (small_a, local_a, small_s))
    print("second handle: summed device bytes of the six engines %.1f GB; whole test %.1f s" % (total_bytes / 1e9, time.perf_counter() - t_start))
    for e in (small_a, local_a, small_s, local_s):
        e.close()


# ------------------------------------------------------------------------------------------------------------------
# the composition against the dense forms, small
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [16, 64])
def test_the_newer_plan_against_the_dense_forms(tile):
    """The newer plan on a map of 24 tile rows through an asynchronous F64 engine and through apply_dense on one oracle.ekf_dense.EKF_SLAM:
    joins, transforms, joint updates and appends interleaved with pending pairs -- the arithmetic of the COMPOSITION, which no single-call
    file checks.  x and the whole P at every batch boundary that ends a step, factor_map's results and the extracted destinations, all to
    helpers.REL.  (Tile 64: 751 -> 1186 landmarks; the dense forms take most of a minute there, factor_dense's unblocked loop a third.)"""
    import transform_map_cases as Tm
    from ekf_slam_amd import Engine
    from ekf_slam_amd import _lib as L
    from oracle import ekf_dense
    batch = 8
    N0 = 24 * (tile // 2) - 2 * batch - 1
    (x, s, d, U), steps, info = _newer_inputs(tile, batch, N0)
    e = Engine(mode="known", capacity=info["N"], tile=tile, storage="f64", batch=batch, async_flush=True)
    e.load_lowrank_state(x, s, d, U)
    dense = ekf_dense.EKF_SLAM()
    dense.x, dense.P, dense.s = x.copy(), np.diag(d) + U @ U.T, list(s)
    worst = {}
    for t, ops in enumerate(steps):
        for kind, payload, _ in ops:
            got = B.issue(e, kind, payload)
            want = B.apply_dense(dense, kind, payload)
            if kind == "factor_map":
                assert got["definite"] and want["definite"] and got["n"] == want["n"] and got["bad_index"] == want["bad_index"] == -1
                for key in ("logdet", "logdet_map", "min_pivot", "max_pivot", "d2"):
                    err = helpers.rel_err(got[key], want[key])
                    worst[key] = max(worst.get(key, 0.0), err)
                    assert err < helpers.REL, (t, key, got[key], want[key])
            elif kind == "extract_map":
                label = "step %d: extract_map, frame %s" % (t, payload[1])
                if payload[1] == "map":
                    helpers.check_state(got, want[0], want[2], "f64", label, want[1])
                else:
                    Tm.check_robot_frame(got, want[0], want[2], "f64", label, want[1], (helpers.REL, helpers.TOL_X32, helpers.TOL_KEPT32, helpers.TOL_ROW32))
                got.close()
            elif kind == "join_map":
                got[1].close()
            elif kind in ("observe_model_joint", "observe_model_joint_iterated"):
                assert got["outcome"] == L.EKF_LINEAR_APPLIED and got["pairings"] == want["pairings"]
                assert abs(got["d2"] - want["d2"]) <= helpers.REL * max(want["d2"], 1.0)
            elif kind == B.NEWER_PAIR_KIND:
                rec = e.assigned_scan_result()
                np.testing.assert_array_equal(rec["landmark"], payload[1])
                np.testing.assert_array_equal(rec["ncand"], want["ncand"])
                assert np.all(rec["outcome"] == L.EKF_LINEAR_APPLIED)
            if kind in B.SYNC_KINDS:
                assert e.pending() == 0
        if t in info["boundaries"] and t not in info["straddlers"]:
            # (reading P flushes: at a boundary that ends a step nothing but the batch just completed is pending, and the places stay)
            helpers.check_state(e, dense.x, dense.P, "f64", "tile %d, step %d (boundary %d)" % (tile, t, info["boundaries"][t]), np.asarray(dense.s, dtype=np.float64))
    assert e.N == info["N"] and e.linear_rejections() == (0, 0)
    print("tile %d: factor_map against factor_dense, worst relative differences %s" % (tile, {k: float("%.3g" % v) for k, v in worst.items()}))
    e.close()
