"""GPU: a scan matched to the map under the models' conventions (ekf_associate_model; include/ekfslam.h) and the
observe-or-append policy on top of it (measure_model of ekf_slam_amd/slam.py).

The yardstick is the NumPy restatement of tests/associate_model_cases.py -- d2 of every (observation, landmark) pair, the top two by
(d2, index) -- applied to THE STATE THE ENGINE REPORTS; stores, tolerances and helpers are those of tests/helpers.py.  Where
the contract is equality -- every d2 against ekf_model_innovation's, a scan against its single calls, the shards against one engine, a
twin that never associated, a replayed log -- the comparison is assert_array_equal.

N = 150 landmarks are one workgroup of k_assoc_model, partly idle; N = 300 are two, so that the best and the second can sit in different
ones.  On the loaded states (CPU, the restatement): aimed at landmark k as below, the best and the second d2 of every range-and-bearing
observation differ by at least 7.9e-2 relative (N = 300) and 57 (range and bearing) / 53 (relative xy) of the 150 observations at N = 150
have two to four landmarks inside the gate 9.21 -- the unambiguous and the ambiguous case both occur without construction.  Each test
asserts the gap it relies on."""
import ctypes

import numpy as np
import pytest

import append_model_cases as AP
import associate_model_cases as A
import helpers
import model_obs_cases as M
from helpers import R2, REL, RPOS, U2, assert_same, check_state, engine, getters, state, status_of
from linear_obs_cases import STORES
from removal_cases import lowrank_data, observe

pytestmark = pytest.mark.gpu
RRB = np.diag([0.02, 0.5])
GATE = 9.21
KEYS = ("best", "second", "d2_best", "d2_second", "within_gate", "irregular")
MODELS = (M.RANGE_BEARING, M.RELATIVE_XY, M.RANGE, M.BEARING)


def aimed(x, model, k, gate=GATE):
    """An observation of `model` that lies a little beside h(x) at landmark k."""
    hx = M.h_of(model, x[:3], x[3 + 2 * k:5 + 2 * k])
    if model == M.RANGE_BEARING:
        return A.entry(model, hx + [0.05, -0.3], RRB, gate)
    if model == M.RELATIVE_XY:
        return A.entry(model, hx + [0.1, -0.1], RPOS, gate)
    if model == M.RANGE:
        return A.entry(model, hx[:1] + 0.05, 0.02, gate)
    return A.entry(model, hx[:1] - 0.3, 0.5, gate)


def edge_landmark(N, tile):
    per_row = tile // 2
    return per_row * max(1, (N // 2) // per_row) if per_row < N else N // 2


def scan_of_eight(x, N, tile):
    """All four models twice: the first, the last and a tile-row-edge landmark, and the two landmarks either side of the workgroup edge."""
    e = edge_landmark(N, tile)
    lms = [0, N - 1, e, e - 1, 255 if N > 256 else N // 3, 256 if N > 256 else N // 3 + 1, 17, N - 2]
    return [aimed(x, MODELS[q % 4], k, GATE if q % 2 == 0 else 4.0 * GATE) for q, k in enumerate(lms)], lms


def loaded(N, history=True, **kw):
    e = helpers.loaded(N, 5, **kw)
    if history:
        x = lowrank_data(N, 5)[0]
        for k in (5, edge_landmark(N, kw.get("tile", 16)), N - 3):
            e.predict(U2); e.correct(observe(x, k), R2, k)
    return e


def assert_equal_results(a, b, msg=""):
    assert set(a) == set(b), msg
    for key in a:
        np.testing.assert_array_equal(a[key], b[key], err_msg="%s %s" % (msg, key))


def against_restatement(got, x0, P0, entries, tol, label):
    want, D = A.match(x0, P0, entries)
    gap = A.relative_gap(want)
    assert np.all(gap > 1e-6), (label, gap)                   # the precondition: best and second are far apart on the restatement
    for key in ("best", "second", "within_gate", "irregular"):
        np.testing.assert_array_equal(got[key], want[key], err_msg="%s %s" % (label, key))
    errs = [float((np.abs(got[key] - want[key]) / want[key]).max()) for key in ("d2_best", "d2_second")]
    err_all = 0.0
    if "d2_all" in got:
        np.testing.assert_array_equal(np.isnan(got["d2_all"]), np.isnan(D), err_msg=label)
        ok = ~np.isnan(D)
        err_all = float((np.abs(got["d2_all"][ok] - D[ok]) / D[ok]).max())
    print("%s: rel err d2_best %.2e d2_second %.2e d2_all %.2e; smallest gap %.2e; within %s" % (label, errs[0], errs[1], err_all, gap.min(), want["within_gate"].tolist()))
    assert max(errs + [err_all]) < tol, label
    return want, D


# ------------------------------------------------------------------------------------------------------------------
# 1. against the dense restatement, every store
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [150, 300])
@pytest.mark.parametrize("tile,storage", STORES)
def test_a_scan_against_the_dense_restatement(tile, storage, N):
    e = loaded(N, capacity=N + 8, tile=tile, storage=storage)
    x0, _, P0 = state(e)
    entries, lms = scan_of_eight(x0, N, tile)
    got = e.associate_model(entries, want_d2=True)
    assert got["d2_all"].shape == (8, N)
    want, _ = against_restatement(got, x0, P0, entries, REL if storage == "f64" else 1e-9, "N = %d [T = %d %s]" % (N, tile, storage))
    # the two-row observations name the landmark they were aimed at
    for q, k in enumerate(lms):
        assert M.ROWS[entries[q]["model"]] == 1 or got["best"][q] == k
    assert_equal_results({k: v for k, v in got.items() if k != "d2_all"}, e.associate_model(entries), "without the matrix")
    e.close()


# ------------------------------------------------------------------------------------------------------------------
# 2. bit for bit what ekf_model_innovation says, pair by pair; nothing changes
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage", [(16, "f64"), (64, "f64"), (256, "f32_mixed")])
@pytest.mark.parametrize("pending", [0, 5])
def test_every_d2_is_bit_for_bit_that_of_model_innovation(tile, storage, pending):
    N = 150
    x = lowrank_data(N, 5)[0]
    kw = dict(capacity=N + 8, tile=tile, storage=storage, batch=8)
    e, twin = helpers.loaded(N, 5, **kw), helpers.loaded(N, 5, **kw)
    for q in (e, twin):
        for k in (5, edge_landmark(N, tile), N - 3, 11, 40)[:pending]:
            q.predict(U2); q.correct(observe(x, k), R2, k)
    assert e.pending() == pending
    xe = e.get_x()
    entries = [aimed(xe, m, k) for m, k in zip(MODELS + (M.RANGE_BEARING,), (3, N - 1, 77, 0, edge_landmark(N, tile)))]
    got = e.associate_model(entries, want_d2=True)
    assert e.pending() == pending
    D = np.array([[e.model_innovation(ent["model"], ent["z"], ent["R"], [i], gate=ent["gate"])["d2"] for i in range(N)] for ent in entries])
    np.testing.assert_array_equal(got["d2_all"], D)
    assert np.all(np.isfinite(D))
    for k in range(len(entries)):
        want = A.top_two(D[k], GATE)
        assert [got[key][k] for key in KEYS] == [want[key] for key in KEYS]
    assert e.pending() == twin.pending() == pending
    assert_same(e, twin)                                    # x, s, P, the diagonal blocks and the digest of a twin that never asked
    e.close(); twin.close()


# ------------------------------------------------------------------------------------------------------------------
# 3. a scan is its single calls
# ------------------------------------------------------------------------------------------------------------------
def test_a_scan_of_thirty_two_is_thirty_two_calls_of_one():
    N = 300
    e = loaded(N, capacity=N + 8, tile=64, batch=8)
    assert e.pending() == 3
    xe = e.get_x()
    entries = [aimed(xe, MODELS[q % 4], (37 * q + 5) % N, GATE * (1 + q % 3)) for q in range(32)]
    got = e.associate_model(entries, want_d2=True)
    for q, ent in enumerate(entries):
        one = e.associate_model([ent], want_d2=True)
        for key in KEYS:
            assert one[key][0] == got[key][q], (q, key)
        np.testing.assert_array_equal(one["d2_all"][0], got["d2_all"][q])
    assert e.pending() == 3
    e.close()


# ------------------------------------------------------------------------------------------------------------------
# 4. a recorded predict is carried out first
# ------------------------------------------------------------------------------------------------------------------
def test_a_recorded_predict_is_carried_out_first():
    N = 150
    kw = dict(capacity=N + 8, tile=16, batch=8)
    e, twin = loaded(N, **kw), loaded(N, **kw)
    x = lowrank_data(N, 5)[0]
    entries, _ = scan_of_eight(e.get_x(), N, 16)
    e.predict(U2); twin.predict(U2)
    got = e.associate_model(entries, want_d2=True)
    assert e.pending() == twin.pending() == 3
    z = observe(x, 9)
    e.correct(z, R2, 9); twin.correct(z, R2, 9)               # the twin's correction folds its predict in; e's was carried out by a launch of its own
    assert_same(e, twin)
    # ... and the association was made at the predicted state: the one a third engine reports after the same predict
    third = loaded(N, **kw)
    third.predict(U2)
    x0, _, P0 = state(third)
    against_restatement(got, x0, P0, entries, REL, "behind a recorded predict")
    assert_equal_results(got, third.associate_model(entries, want_d2=True), "after the state was read")
    for q in (e, twin, third):
        q.close()


# ------------------------------------------------------------------------------------------------------------------
# 5. edges
# ------------------------------------------------------------------------------------------------------------------
def _set_x(e, x):
    from ekf_slam_amd.engine import _p
    x = np.ascontiguousarray(x, dtype=np.float64)
    e._check(e.lib.ekf_set_x(e.h, _p(x), x.size))


def test_an_empty_map_and_a_map_of_one():
    from ekf_slam_amd import _lib as L
    e = engine(capacity=8, tile=16)
    e.timing_enable(L.EKF_KERNEL_ASSOCIATE)
    entries = [A.entry(M.RANGE_BEARING, [5.0, 30.0], RRB, GATE), A.entry(M.BEARING, [12.0], 0.5)]
    got = e.associate_model(entries, want_d2=True)
    assert got["best"].tolist() == got["second"].tolist() == [-1, -1] and got["d2_best"].tolist() == got["d2_second"].tolist() == [np.inf, np.inf]
    assert got["within_gate"].tolist() == got["irregular"].tolist() == [0, 0] and got["d2_all"].shape == (2, 0)
    assert e.timing_read(L.EKF_KERNEL_ASSOCIATE)[0] == 0                      # no launch
    x1 = np.array([0.1, -0.2, 10.0, 4.0, 3.0])
    e.set_state(x1, np.diag([0.01, 0.01, 0.001, 0.1, 0.2]), np.array([1.0]))
    ents = [aimed(x1, m, 0) for m in MODELS]
    got = e.associate_model(ents, want_d2=True)
    assert got["best"].tolist() == [0] * 4 and got["second"].tolist() == [-1] * 4 and np.all(np.isinf(got["d2_second"]))
    np.testing.assert_array_equal(got["d2_all"][:, 0], got["d2_best"])
    D = A.d2_matrix(x1, e.get_P(), ents)
    assert float((np.abs(got["d2_all"] - D) / D).max()) < REL and got["within_gate"].tolist() == [1] * 4
    assert e.timing_read(L.EKF_KERNEL_ASSOCIATE)[0] == 1                      # the two launches of one call under one bracket
    e.close()


def test_a_landmark_on_the_robot_is_irregular_and_never_the_best():
    N = 40
    e = loaded(N, history=False, capacity=N + 8, tile=16)
    x = e.get_x()
    x[3 + 2 * 13:5 + 2 * 13] = x[:2]
    _set_x(e, x)
    x0, _, P0 = state(e)
    entries = [aimed(x0, m, k) for m, k in zip(MODELS, (12, 14, 0, N - 1))] + [A.entry(M.RELATIVE_XY, [0.0, 0.0], RPOS, GATE)]
    got = e.associate_model(entries, want_d2=True)
    assert got["irregular"].tolist() == [1] * 5 and np.all(np.isnan(got["d2_all"][:, 13]))
    assert np.isnan(got["d2_all"]).sum() == 5 and 13 not in got["best"].tolist() + got["second"].tolist()
    want, D = A.match(x0, P0, entries)
    for key in ("best", "second", "within_gate", "irregular"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    assert e.model_innovation(M.RELATIVE_XY, [0.0, 0.0], RPOS, [13])["outcome"] == M.IRREGULAR       # what the single call says of that pair
    e.close()


def test_two_identical_landmarks_tie_and_the_lower_index_is_the_best():
    N = 40
    e = loaded(N, history=False, capacity=N + 8, tile=16)
    x, s, P = state(e)
    i, j = 9, 31
    a, b = 3 + 2 * i, 3 + 2 * j
    x[b:b + 2] = x[a:a + 2]
    P[b:b + 2, :] = P[a:a + 2, :]
    P[:, b:b + 2] = P[:, a:a + 2]
    P[b:b + 2, b:b + 2] = P[a:a + 2, a:a + 2]
    e.set_state(x, P, s)
    entries = [aimed(x, m, j) for m in MODELS]
    got = e.associate_model(entries, want_d2=True)
    np.testing.assert_array_equal(got["d2_all"][:, i], got["d2_all"][:, j])
    for q in (0, 1):                                          # the two-row observations: the pair is the top two, the lower index first
        assert (got["best"][q], got["second"][q]) == (i, j) and got["d2_best"][q] == got["d2_second"][q] == got["d2_all"][q, i]
    for q in range(4):
        want = A.top_two(got["d2_all"][q], GATE)
        assert [got[key][q] for key in KEYS] == [want[key] for key in KEYS]
    e.close()


# ------------------------------------------------------------------------------------------------------------------
# 6. beside an asynchronous pass
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage", [(16, "f64"), (64, "f64")])
def test_between_two_batches_of_an_asynchronous_pass(tile, storage):
    N = 150
    x = lowrank_data(N, 5)[0]
    kw = dict(capacity=N + 8, tile=tile, storage=storage, batch=4)
    e, twin = helpers.loaded(N, 5, async_flush=True, **kw), helpers.loaded(N, 5, **kw)
    steps = (5, edge_landmark(N, tile), N - 3, 11, 40, 77, 2, 120)
    for q in (e, twin):
        for k in steps[:4]:                                   # the batch completes: its pass starts (asynchronous: on the pass stream)
            q.predict(U2); q.correct(observe(x, k), R2, k)
    entries, _ = scan_of_eight(lowrank_data(N, 5)[0], N, tile)
    got, ref = e.associate_model(entries, want_d2=True), twin.associate_model(entries, want_d2=True)
    assert_equal_results(got, ref, "beside the pass")
    assert np.all(np.isfinite(got["d2_all"])) and np.all(got["best"] >= 0)
    for q in (e, twin):
        for k in steps[4:6]:
            q.predict(U2); q.correct(observe(x, k), R2, k)
    assert_equal_results(e.associate_model(entries), twin.associate_model(entries), "inside the next batch")
    for q in (e, twin):
        for k in steps[6:]:
            q.predict(U2); q.correct(observe(x, k), R2, k)
    assert_same(e, twin)
    e.close(); twin.close()


# ------------------------------------------------------------------------------------------------------------------
# 7. shards: every shard the same answer, no exchange
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_every_shard_answers_as_the_unsharded_engine(world):
    from ekf_slam_amd.engine import Engine
    from ekf_slam_amd.sharding import ShardGroup
    N = 150
    x, s, d, U = lowrank_data(N, 5)
    kw = dict(capacity=N + 16, tile=16, batch=4)
    g, one = ShardGroup(world, **kw), Engine(**kw)
    new = AP.scan(np.random.default_rng(4), 3)
    for q in (g, one):
        q.load_lowrank_state(x, s, d, U)
        for k in (5, 60, 149):
            q.predict(U2); q.correct(observe(x, k), R2, k)
        assert q.append_model(new) == N
    xe = one.get_x()
    for q in (g, one):
        q.predict(U2); q.correct(observe(xe, N + 1), R2, N + 1)
    xe = one.get_x()
    entries = [aimed(xe, MODELS[q % 4], k) for q, k in enumerate((0, N + 2, 75, 76, N - 1, N + 1, 23, 100))]
    ref = one.associate_model(entries, want_d2=True)
    assert ref["d2_all"].shape == (8, N + 3) and np.all(np.isfinite(ref["d2_all"]))
    for sh in g.shards:
        assert_equal_results(sh.associate_model(entries, want_d2=True), ref, "shard %d of %d" % (sh.cfg.rank, world))
    assert_equal_results(g.associate_model(entries, want_d2=True), ref, "the group")
    np.testing.assert_array_equal(g.get_x(), one.get_x())
    np.testing.assert_array_equal(g.get_P(), one.get_P())
    g.close(); one.close()


# ------------------------------------------------------------------------------------------------------------------
# 8. refusals, each before anything changes
# ------------------------------------------------------------------------------------------------------------------
def _raw(e, entries):
    arr = (e.lib.ekf_associate_model.argtypes[1]._type_ * max(len(entries), 1))()
    for k, ent in enumerate(entries):
        o = e._model_obs(ent["model"], ent["z"], ent["R"], (), (0.0, 0.0), ent["gate"])
        arr[k] = o
    return arr


def test_refusals_leave_the_state_alone():
    from ekf_slam_amd import _lib as L
    N = 60
    x = lowrank_data(N, 5)[0]
    e = helpers.loaded(N, 5, capacity=N + 4, tile=16, batch=4)
    for k in (4, 33):
        e.predict(U2); e.correct(observe(x, k), R2, k)
    before = getters(e)
    xe = e.get_x()
    good = [aimed(xe, m, k) for m, k in zip(MODELS, (1, 20, 41, 59))]
    out = (L.EkfModelMatch * 33)()
    for k in range(33):
        out[k].best = -7
    nan, inf = float("nan"), float("inf")

    def refused(name, rc, want=L.EKF_ERR_INVALID_ARG, handle_text=True):
        assert rc == want, name
        if handle_text:
            assert b"associate_model" in e.lib.ekf_last_error(e.h), name
        assert e.N == N and all(out[k].best == -7 for k in range(33)), name
        for got, ref in zip(getters(e), before):            # x, s, P, the diagonal blocks, ekf_P_digest
            np.testing.assert_array_equal(got, ref, err_msg=name)

    call = lambda arr, m, o=out, d=None: e.lib.ekf_associate_model(e.h, arr, m, o, d)
    refused("null handle", e.lib.ekf_associate_model(None, _raw(e, good), 4, out, None), handle_text=False)
    refused("null observations", call(None, 4))
    refused("null results", call(_raw(e, good), 4, None))
    for m in (0, -1, 33):
        refused("m = %d" % m, call(_raw(e, good * 9), m))
    cases = [("a landmark range", "model", None, M.LANDMARK_RANGE), ("model 0", "model", None, 0), ("model 6", "model", None, 6),
             ("a named landmark", "lm", 0, 3), ("a second landmark", "lm", 1, 0), ("lm -2", "lm", 0, -2),
             ("NaN z", "z", 0, nan), ("inf z", "z", 1, inf), ("inf R", "R", 0, inf), ("asymmetric R", "R", 1, 0.2), ("negative diagonal", "R", 3, -1.0),
             ("a NaN gate", "gate", None, nan)]
    for name, key, idx, v in cases:
        for b in (0, 1, 3):                                   # the bad entry first, in the middle, last (entries 0 and 1 are the two-row models)
            if key in ("z", "R") and idx in (1, 3) and b == 3:
                continue                                      # (a one-row model does not read z[1] or R[1..3])
            arr = _raw(e, good)
            if idx is None:
                setattr(arr[b], key, v)
            else:
                getattr(arr[b], key)[idx] = v
            refused("%s in entry %d" % (name, b), call(arr, 4))
    # the anchor is ignored, whatever it holds; +inf as a gate counts every regular landmark
    arr = _raw(e, good)
    arr[0].anchor[0], arr[1].anchor[1], arr[2].gate = nan, inf, inf
    assert call(arr, 4) == 0 and out[2].within_gate == N and out[0].best == 1 and out[4].best == -7
    for got, ref in zip(getters(e), before):
        np.testing.assert_array_equal(got, ref)
    e.close()


def test_refused_between_begin_and_finish_of_a_sharded_correction():
    from ekf_slam_amd import _lib as L
    N = 60
    x = lowrank_data(N, 5)[0]
    kw = dict(capacity=N + 4, tile=16)
    e, twin = helpers.loaded(N, 5, force_sharded=1, **kw), helpers.loaded(N, 5, **kw)
    harr = (ctypes.c_void_p * 1)(e.h)
    entries = [aimed(x, m, k) for m, k in zip(MODELS, (1, 20, 41, 59))]
    z = observe(x, 7)
    e.predict(U2); twin.predict(U2)
    e.correct_begin(z, R2, 7)
    st, msg = status_of(lambda: e.associate_model(entries))
    assert st == L.EKF_ERR_STATE and "associate_model" in msg and "begin and finish" in msg
    bad = [dict(entries[0], model=M.LANDMARK_RANGE)]
    assert status_of(lambda: e.associate_model(bad))[0] == L.EKF_ERR_INVALID_ARG            # the arguments come first
    assert e.lib.ekf_exchange_local(harr, 1) == 0
    e.correct_finish()
    twin.correct(z, R2, 7)
    assert_equal_results(e.associate_model(entries, want_d2=True), twin.associate_model(entries, want_d2=True), "a lone shard")
    assert_same(e, twin)
    e.close(); twin.close()


# ------------------------------------------------------------------------------------------------------------------
# 9. the policy end to end
# ------------------------------------------------------------------------------------------------------------------
def test_measure_model_end_to_end_and_its_replay(tmp_path):
    from ekf_slam_amd.slam import EKF_SLAM
    from ekf_slam_amd.trajectory import TrajectoryLog
    N, gate_new = 150, 60.0
    x, s, d, U = lowrank_data(N, 5)
    kw = dict(capacity=N + 8, tile=16, batch=8)

    def start(q):
        q.load_lowrank_state(x, s, d, U)
        for k in (5, edge_landmark(N, 16), N - 3):
            q.predict(U2); q.correct(observe(x, k), R2, k)
        q.flush()

    f = EKF_SLAM(**kw)
    start(f._e)
    f.log = TrajectoryLog()
    f.predict(U2)
    f.log.record(U2, None, [], [])                            # (what measure() records of a step without sightings)
    x0, s0, P0 = state(f._e)
    # chosen by the restatement among sightings of the first 40 landmarks: three with exactly one landmark inside the gate, one with several
    cand = [aimed(x0, M.RANGE_BEARING if k % 2 == 0 else M.RELATIVE_XY, k) for k in range(40)]
    res, _ = A.match(x0, P0, cand)
    assert np.all(A.relative_gap(res) > 1e-6)
    alone = [k for k in range(40) if res["within_gate"][k] == 1 and res["best"][k] == k][:3]
    crowd = [k for k in range(40) if res["within_gate"][k] >= 2][:1]
    assert len(alone) == 3 and len(crowd) == 1
    far = [A.entry(M.RANGE_BEARING, [150.0, 77.0], RRB), A.entry(M.RELATIVE_XY, [-90.0, 120.0], RPOS)]
    far_res, _ = A.match(x0, P0, far)
    assert np.all(far_res["d2_best"] > 10.0 * gate_new)
    picks = [cand[alone[0]], far[0], cand[crowd[0]], cand[alone[1]], far[1], cand[alone[2]]]
    scan = [(p["model"], p["z"], p["R"]) for p in picks]
    assert f._e.pending() == 0
    out = f.measure_model(scan, GATE, gate_new)
    assert out == [("matched", alone[0] + 1), ("new", N + 1), ("discarded", 0), ("matched", alone[1] + 1), ("new", N + 2), ("matched", alone[2] + 1)]
    assert f._e.N == N + 2 and f._e.pending() == 3
    # the dense restatement of those three steps and the one append
    ex, eP, es = x0, P0, s0
    for q in (0, 3, 5):
        o = M.obs(picks[q]["model"], picks[q]["z"], picks[q]["R"], [out[q][1] - 1], None, GATE)
        ex, eP, r = M.observe_model_dense(ex, eP, o)
        assert r["outcome"] == M.APPLIED
    ex, es, eP = AP.append_model_dense(ex, es, eP, [AP.entry(picks[q]["model"], picks[q]["z"], picks[q]["R"], N + 1 + b) for b, q in enumerate((1, 4))])
    check_state(f._e, ex, eP, "f64", "measure_model")
    np.testing.assert_array_equal(f.s, es)
    # a replay of the saved log leaves the same bits
    path = tmp_path / "measured.npz"
    f.log.save(path)
    log = TrajectoryLog.load(path)
    assert [e[1] for e in log.edits] == ["observe_model"] * 3 + ["append_model"]
    fresh = engine(**kw)
    start(fresh)
    log.replay(fresh)
    assert_same(fresh, f._e)
    fresh.close()
