"""GPU: a scan assigned to the map one-to-one (ekf_assign_model; include/ekfslam.h) and the policies on top of it
(measure_model_assigned, measure_model_joint(device_candidates=True) of ekf_slam_amd/slam.py).

The yardstick for the candidate lists and the assignment is the restatement of tests/assign_model_cases.py applied to
e.associate_model(entries, want_d2=True) OF THE SAME ENGINE IN THE SAME STATE: the m x N matrix comes from ekf_associate_model, which this
call does not touch, and the lists and the Hungarian from plain Python.  Every comparison of d2, of a list, of an assignment and of a
total is assert_array_equal / ==; each test asserts the gap it relies on -- the next-best assignment more than 1e-6 relative above the
optimum.  N = 150 landmarks are one workgroup of k_assign_candidates, partly idle; 300 are two and 600 three."""
import ctypes

import numpy as np
import pytest

import assign_model_cases as C
import associate_model_cases as A
import helpers
import joint_cases as J
import model_obs_cases as M
from helpers import R2, RPOS, U2, assert_same, check_state, engine, getters, line_program, state, status_of
from linear_obs_cases import STORES
from removal_cases import lowrank_data, observe

pytestmark = pytest.mark.gpu
RRB = np.diag([0.02, 0.5])
GATE = 9.21
INF = float("inf")
MATCH_KEYS = ("best", "second", "d2_best", "d2_second", "within_gate", "irregular")
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


def against_associate_model(e, entries, label, min_gap=1e-6):
    """One assign_model call against the restatement applied to the same engine's associate_model matrix: the records, every list entry,
    the assignment and the total.  Returns (the call's result, the matrix, the restatement's assignment)."""
    ref = e.associate_model(entries, want_d2=True)
    got = e.assign_model(entries, want_candidates=True)
    D = ref["d2_all"]
    gates = [ent["gate"] for ent in entries]
    for key in MATCH_KEYS:
        np.testing.assert_array_equal(got[key], ref[key], err_msg="%s %s" % (label, key))
    cand, cand_d2, ncand, within = C.candidate_lists(D, gates)
    np.testing.assert_array_equal(got["within_gate"], within, err_msg=label)
    np.testing.assert_array_equal(got["ncand"], ncand, err_msg=label)
    np.testing.assert_array_equal(got["cand"], cand, err_msg=label)
    np.testing.assert_array_equal(got["cand_d2"], cand_d2, err_msg=label)                 # the matrix entries, bit for bit
    want, Jw, rel = C.gap(D, gates)
    print("%s: J %.6g, the next assignment %.2e relative above it; kept %s; left out %d of %d" % (label, Jw, rel, ncand.tolist(), int((want < 0).sum()), len(entries)))
    assert rel > min_gap, (label, rel)
    np.testing.assert_array_equal(got["landmark"], want, err_msg=label)
    np.testing.assert_array_equal(got["d2"], [D[k, i] if i >= 0 else INF for k, i in enumerate(want)], err_msg=label)
    total = 0.0
    for k in range(len(entries)):
        total += got["d2"][k] if got["landmark"][k] >= 0 else gates[k]
    assert got["total"] == total, label                                                   # J summed in scan order from the returned d2
    assert_equal_results({k: v for k, v in got.items() if k not in ("cand", "cand_d2")}, e.assign_model(entries), label + ": without the lists")
    return got, D, want


# ------------------------------------------------------------------------------------------------------------------
# 1. equality with associate_model, every store
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [150, 300])
@pytest.mark.parametrize("tile,storage", STORES)
def test_a_mixed_scan_against_associate_model(tile, storage, N):
    e = loaded(N, capacity=N + 8, tile=tile, storage=storage)
    entries, _ = scan_of_eight(e.get_x(), N, tile)
    got, D, _ = against_associate_model(e, entries, "N = %d [T = %d %s]" % (N, tile, storage))
    assert np.any(got["ncand"] >= 2) and np.any(got["landmark"] >= 0)
    if N == 300:                                              # one observation's candidates on both sides of the workgroup edge
        assert any(np.any(got["cand"][k][:got["ncand"][k]] < 256) and np.any(got["cand"][k] >= 256) for k in range(8))
    e.close()


# ------------------------------------------------------------------------------------------------------------------
# 2. contention: observations that share their cheapest landmark
# ------------------------------------------------------------------------------------------------------------------
def contention_engine(**kw):
    x, s, d, U, scan, targets = C.contention_scene()
    e = engine(capacity=C.SCENE_N + 40, tile=16, **kw)
    e.load_lowrank_state(x, s, d, U)
    return e, scan, targets


def test_rows_that_share_their_best_landmark_are_assigned_apart():
    e, scan, targets = contention_engine()
    entries = [A.entry(model, z, R, C.SCENE_GATE) for model, z, R in scan]
    got, D, want = against_associate_model(e, entries, "contention")
    best = got["best"]
    assert len(set(best.tolist())) < 32                                                   # several rows share their cheapest column
    assert np.any((got["landmark"] >= 0) & (got["landmark"] != best))                     # ... so independent nearest neighbours do not pass
    used = got["landmark"][got["landmark"] >= 0]
    assert used.size == np.unique(used).size and used.size >= C.SCENE_COUNT
    e.close()


# ------------------------------------------------------------------------------------------------------------------
# 3. more than 32 inside the gate
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [150, 600])
def test_more_than_thirty_two_inside_the_gate(N):
    e = loaded(N, capacity=N + 8, tile=64)
    xe = e.get_x()
    entries = [aimed(xe, MODELS[q % 4], k, 1e6) for q, k in enumerate((0, 255 % N, 256 % N, N - 1, 37, 300 % N, 511 % N, 512 % N))]
    got, D, want = against_associate_model(e, entries, "N = %d, all inside" % N)
    assert got["ncand"].tolist() == [32] * 8 and got["within_gate"].tolist() == [N] * 8
    for k in range(8):                                        # the 32 smallest of the matrix row, in order
        order = sorted((float(D[k, i]), i) for i in range(N))[:32]
        assert got["cand"][k].tolist() == [i for _, i in order] and got["cand_d2"][k].tolist() == [v for v, _ in order]
    assert np.all(want >= 0)                                  # (the restatement ran on the FULL matrix: against_associate_model)
    e.close()


# ------------------------------------------------------------------------------------------------------------------
# 4. edges
# ------------------------------------------------------------------------------------------------------------------
def test_a_scan_of_one_and_a_map_of_one_and_fewer_landmarks_than_observations():
    from ekf_slam_amd import _lib as L
    e = loaded(150, capacity=158, tile=16)
    against_associate_model(e, [aimed(e.get_x(), M.RANGE_BEARING, 77)], "m = 1")
    e.close()
    e = engine(capacity=8, tile=16)
    e.timing_enable(L.EKF_KERNEL_ASSOCIATE)
    ents = [A.entry(M.RANGE_BEARING, [5.0, 30.0], RRB, GATE), A.entry(M.BEARING, [12.0], 0.5, 2.5)]
    got = e.assign_model(ents, want_candidates=True)          # N = 0: everything left out, no launch
    assert got["landmark"].tolist() == [-1, -1] and np.all(np.isinf(got["d2"])) and got["ncand"].tolist() == [0, 0] and got["total"] == GATE + 2.5
    assert np.all(got["cand"] == -1) and np.all(np.isinf(got["cand_d2"])) and got["best"].tolist() == [-1, -1] and got["within_gate"].tolist() == [0, 0]
    assert e.timing_read(L.EKF_KERNEL_ASSOCIATE)[0] == 0
    x1 = np.array([0.1, -0.2, 10.0, 4.0, 3.0])
    e.set_state(x1, np.diag([0.01, 0.01, 0.001, 0.1, 0.2]), np.array([1.0]))
    ents = [aimed(x1, m, 0) for m in MODELS]                  # N = 1 < m = 4: one observation has the landmark, three are left out
    got, D, want = against_associate_model(e, ents, "N = 1")
    assert (got["landmark"] == 0).sum() == 1 and (got["landmark"] == -1).sum() == 3 and got["ncand"].tolist() == [1] * 4
    assert e.timing_read(L.EKF_KERNEL_ASSOCIATE)[0] == 3      # (associate_model, assign_model twice: each call's launches under one bracket)
    e.close()
    e = loaded(3, history=False, capacity=8, tile=16)         # N = 3 < m = 5
    xe = e.get_x()
    got, D, want = against_associate_model(e, [aimed(xe, M.RELATIVE_XY if q % 2 else M.RANGE_BEARING, q % 3, 1e3) for q in range(5)], "N = 3, m = 5")
    assert (got["landmark"] >= 0).sum() == 3 and (got["landmark"] < 0).sum() == 2
    e.close()


def test_a_gate_below_every_d2_leaves_everything_out_and_a_landmark_on_the_robot_is_never_a_candidate():
    N = 40
    e = loaded(N, history=False, capacity=N + 8, tile=16)
    x = e.get_x()
    x[3 + 2 * 13:5 + 2 * 13] = x[:2]
    e._check(e.lib.ekf_set_x(e.h, x.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), x.size))
    x0 = e.get_x()
    ref = e.associate_model([aimed(x0, m, k) for m, k in zip(MODELS, (12, 14, 0, N - 1))], want_d2=True)
    low = float(np.nanmin(ref["d2_all"])) / 2.0
    tight = [aimed(x0, m, k, low / (q + 1)) for q, (m, k) in enumerate(zip(MODELS, (12, 14, 0, N - 1)))]
    got = e.assign_model(tight, want_candidates=True)
    assert got["landmark"].tolist() == [-1] * 4 and got["ncand"].tolist() == [0] * 4 and got["within_gate"].tolist() == [0] * 4
    assert got["total"] == ((low + low / 2) + low / 3) + low / 4 and np.all(got["cand"] == -1)
    wide = [aimed(x0, m, k, 1e9) for m, k in zip(MODELS, (12, 14, 0, N - 1))] + [A.entry(M.RELATIVE_XY, [0.0, 0.0], RPOS, 1e9)]
    got, D, _ = against_associate_model(e, wide, "a landmark on the robot")
    assert got["irregular"].tolist() == [1] * 5 and np.all(np.isnan(D[:, 13])) and got["within_gate"].tolist() == [N - 1] * 5
    assert 13 not in got["cand"].reshape(-1).tolist() and 13 not in got["landmark"].tolist()
    e.close()


def _raw(e, entries):
    arr = (e.lib.ekf_assign_model.argtypes[1]._type_ * max(len(entries), 1))()
    for k, ent in enumerate(entries):
        arr[k] = e._model_obs(ent["model"], ent["z"], ent["R"], (), (0.0, 0.0), ent["gate"])
    return arr


def test_refusals_leave_the_state_and_the_results_alone():
    from ekf_slam_amd import _lib as L
    N = 60
    x = lowrank_data(N, 5)[0]
    e = helpers.loaded(N, 5, capacity=N + 4, tile=16, batch=4)
    for k in (4, 33):
        e.predict(U2); e.correct(observe(x, k), R2, k)
    before = getters(e)
    xe = e.get_x()
    good = [aimed(xe, m, k) for m, k in zip(MODELS, (1, 20, 41, 59))]
    out, match = (L.EkfModelAssigned * 33)(), (L.EkfModelMatch * 33)()
    cand, cand_d2 = (ctypes.c_int64 * (33 * 32))(), (ctypes.c_double * (33 * 32))()
    total = ctypes.c_double(-7.0)
    for k in range(33):
        out[k].landmark = -7
    nan, inf = float("nan"), float("inf")

    def refused(name, rc, want=L.EKF_ERR_INVALID_ARG, handle_text=True):
        assert rc == want, name
        if handle_text:
            assert b"assign_model: " in e.lib.ekf_last_error(e.h), name
        assert e.N == N and all(out[k].landmark == -7 for k in range(33)) and total.value == -7.0, name
        for got, ref in zip(getters(e), before):
            np.testing.assert_array_equal(got, ref, err_msg=name)

    def call(arr, m, o=out, c=cand, cd=cand_d2):
        return e.lib.ekf_assign_model(e.h, arr, m, o, match, c, cd, ctypes.byref(total))

    refused("null handle", e.lib.ekf_assign_model(None, _raw(e, good), 4, out, match, cand, cand_d2, ctypes.byref(total)), handle_text=False)
    refused("null observations", call(None, 4))
    refused("null results", call(_raw(e, good), 4, None))
    for m in (0, -1, 33):
        refused("m = %d" % m, call(_raw(e, good * 9), m))
    cases = [("a landmark range", "model", None, M.LANDMARK_RANGE), ("model 0", "model", None, 0), ("a named landmark", "lm", 0, 3),
             ("NaN z", "z", 0, nan), ("inf R", "R", 0, inf), ("negative diagonal", "R", 3, -1.0), ("a NaN gate", "gate", None, nan),
             ("a gate of +inf", "gate", None, inf), ("a gate of -inf", "gate", None, -inf)]
    for name, key, idx, v in cases:
        for b in (0, 1, 3):
            if key == "R" and idx == 3 and b == 3:
                continue                                      # (a one-row model does not read R[1..3])
            arr = _raw(e, good)
            if idx is None:
                setattr(arr[b], key, v)
            else:
                getattr(arr[b], key)[idx] = v
            refused("%s in entry %d" % (name, b), call(arr, 4))
    refused("cand without cand_d2", call(_raw(e, good), 4, cd=None))
    refused("cand_d2 without cand", call(_raw(e, good), 4, c=None))
    assert b"together" in e.lib.ekf_last_error(e.h)
    arr = _raw(e, good)
    arr[1].gate = inf
    arr[2].model = M.LANDMARK_RANGE
    refused("associate_model's refusals come first", call(arr, 4))
    assert b"LANDMARK_RANGE" in e.lib.ekf_last_error(e.h)
    # every optional result left out: still a call
    assert e.lib.ekf_assign_model(e.h, _raw(e, good), 4, out, None, None, None, None) == 0 and out[0].landmark == 1 and out[4].landmark == -7
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
    st, msg = status_of(lambda: e.assign_model(entries))
    assert st == L.EKF_ERR_STATE and "assign_model" in msg and "begin and finish" in msg
    assert status_of(lambda: e.assign_model([dict(entries[0], gate=INF)]))[0] == L.EKF_ERR_INVALID_ARG       # the arguments come first
    assert e.lib.ekf_exchange_local(harr, 1) == 0
    e.correct_finish()
    twin.correct(z, R2, 7)
    assert_equal_results(e.assign_model(entries, want_candidates=True), twin.assign_model(entries, want_candidates=True), "a lone shard")
    assert_same(e, twin)
    e.close(); twin.close()


# ------------------------------------------------------------------------------------------------------------------
# 5. ties
# ------------------------------------------------------------------------------------------------------------------
def test_two_identical_landmarks_tie_and_the_host_build_returns_the_same_assignment(tmp_path_factory):
    host = line_program(tmp_path_factory, "assign_model_host")
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
    entries = [aimed(x, M.RANGE_BEARING, j, 4 * GATE), aimed(x, M.RELATIVE_XY, j, 4 * GATE), aimed(x, M.RELATIVE_XY, i, 4 * GATE), aimed(x, M.RANGE, 3, 4 * GATE)]
    gates = [ent["gate"] for ent in entries]
    ref = e.associate_model(entries, want_d2=True)
    D = ref["d2_all"]
    np.testing.assert_array_equal(D[:, i], D[:, j])           # equal bits
    got = e.assign_model(entries, want_candidates=True)
    cand, cand_d2, ncand, _ = C.candidate_lists(D, gates)
    np.testing.assert_array_equal(got["cand"], cand)
    np.testing.assert_array_equal(got["cand_d2"], cand_d2)
    for k in range(3):
        assert got["cand"][k][:2].tolist() == [i, j]          # the lower index first
    used = got["landmark"][got["landmark"] >= 0]
    assert used.size == np.unique(used).size and {i, j} <= set(used.tolist())
    for k, lm in enumerate(got["landmark"]):
        assert (lm < 0 and got["d2"][k] == INF) or got["d2"][k] == D[k, lm] <= gates[k]
    _, Jw = C.solve(D, gates)
    print("ties: total %.17g, the restatement's optimum %.17g" % (got["total"], Jw))
    assert abs(got["total"] - Jw) <= 1e-12 * Jw
    line = host([C.solve_line(1, got["cand"], got["cand_d2"], got["ncand"], gates), C.solve_line(64, got["cand"], got["cand_d2"], got["ncand"], gates)])
    assert line[0] == line[1]
    assert got["landmark"].tolist() == line[0][:4] and got["d2"].tolist() == line[0][4:8] and got["total"] == line[0][8]
    e.close()


# ------------------------------------------------------------------------------------------------------------------
# 6. nothing changes, nothing is flushed; a recorded predict is carried out first
# ------------------------------------------------------------------------------------------------------------------
def test_pending_pairs_stay_pending_and_the_state_keeps_its_bits():
    N = 150
    x = lowrank_data(N, 5)[0]
    kw = dict(capacity=N + 8, tile=16, batch=8)
    e, twin = helpers.loaded(N, 5, **kw), helpers.loaded(N, 5, **kw)
    for q in (e, twin):
        for k in (5, edge_landmark(N, 16), N - 3, 11, 40):
            q.predict(U2); q.correct(observe(x, k), R2, k)
    assert e.pending() == twin.pending() == 5
    x_before, s_before = e.get_x(), e.get_s()                 # (x and s are read without a flush; P is not)
    assert e.pending() == 5
    entries, _ = scan_of_eight(x_before, N, 16)
    got = e.assign_model(entries, want_candidates=True)
    assert e.pending() == 5 and np.any(got["landmark"] >= 0)
    np.testing.assert_array_equal(e.get_x(), x_before)
    np.testing.assert_array_equal(e.get_s(), s_before)
    assert e.pending() == twin.pending() == 5
    for a, b in zip(getters(e), getters(twin)):               # x, s, P, the diagonal blocks and the digest of a twin that never called it
        np.testing.assert_array_equal(a, b)
    against_associate_model(e, entries, "with five pairs pending")
    e.close(); twin.close()


def test_a_recorded_predict_is_carried_out_first():
    N = 150
    kw = dict(capacity=N + 8, tile=16, batch=8)
    e, third = loaded(N, **kw), loaded(N, **kw)
    entries, _ = scan_of_eight(e.get_x(), N, 16)
    e.predict(U2); third.predict(U2)
    got = e.assign_model(entries, want_candidates=True)
    third.associate_model(entries)                            # carries the predict out, by a launch of its own, and flushes nothing
    assert_equal_results(got, third.assign_model(entries, want_candidates=True), "predict, then the call")
    assert e.pending() == third.pending() == 3
    x = lowrank_data(N, 5)[0]
    z = observe(x, 9)
    e.correct(z, R2, 9); third.correct(z, R2, 9)
    assert_same(e, third)
    e.close(); third.close()


# ------------------------------------------------------------------------------------------------------------------
# 7. shards, 8. determinism
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_every_shard_answers_as_the_unsharded_engine(world):
    from ekf_slam_amd.engine import Engine
    from ekf_slam_amd.sharding import ShardGroup
    N = 150
    x, s, d, U = lowrank_data(N, 5)
    kw = dict(capacity=N + 16, tile=16, batch=4)
    g, one = ShardGroup(world, **kw), Engine(**kw)
    for q in (g, one):
        q.load_lowrank_state(x, s, d, U)
        for k in (5, 60, 149):
            q.predict(U2); q.correct(observe(x, k), R2, k)
    xe = one.get_x()
    entries = [aimed(xe, MODELS[q % 4], k, 4 * GATE) for q, k in enumerate((0, 75, 76, N - 1, 23, 100, 75, 23))]
    ref = one.assign_model(entries, want_candidates=True)
    assert np.any(ref["landmark"] >= 0) and np.any(ref["ncand"] >= 2)
    for sh in g.shards:
        assert_equal_results(sh.assign_model(entries, want_candidates=True), ref, "shard %d of %d" % (sh.cfg.rank, world))
    assert_equal_results(g.assign_model(entries, want_candidates=True), ref, "the group")
    np.testing.assert_array_equal(g.get_x(), one.get_x())
    np.testing.assert_array_equal(g.get_P(), one.get_P())
    g.close(); one.close()


def test_two_calls_give_the_same_bits():
    e, scan, _ = contention_engine()
    entries = [A.entry(model, z, R, C.SCENE_GATE) for model, z, R in scan]
    first = e.assign_model(entries, want_candidates=True)
    other = e.assign_model(entries[:5])                       # (another scan in between: the buffers are reused)
    assert other["landmark"].shape == (5,)
    assert_equal_results(first, e.assign_model(entries, want_candidates=True), "the second call")
    e.close()


# ------------------------------------------------------------------------------------------------------------------
# 9. the policies
# ------------------------------------------------------------------------------------------------------------------
def test_measure_model_assigned_matches_what_measure_model_discards_and_replays(tmp_path):
    from ekf_slam_amd.slam import EKF_SLAM
    from ekf_slam_amd.trajectory import TrajectoryLog
    x, s, d, U, scan, targets = C.contention_scene()
    kw = dict(capacity=C.SCENE_N + 40, tile=16, batch=8)
    gate_new = 4.0 * C.SCENE_GATE

    def start():
        f = EKF_SLAM(**kw)
        f._e.load_lowrank_state(x, s, d, U)
        return f

    old, new = start(), start()
    x0, s0, P0 = state(new._e)
    was = old.measure_model(scan, C.SCENE_GATE, gate_new)
    assert all(kind == "discarded" for kind, _ in was)        # several landmarks inside every gate: measure_model throws the scan away
    entries = [A.entry(model, z, R, C.SCENE_GATE) for model, z, R in scan]
    want, _, rel = C.gap(new._e.associate_model(entries, want_d2=True)["d2_all"], [C.SCENE_GATE] * 32)
    assert rel > 1e-6
    new.log = TrajectoryLog()
    out = new.measure_model_assigned(scan, C.SCENE_GATE, gate_new)
    assert out == [("matched", int(lm) + 1) if lm >= 0 else ("discarded", 0) for lm in want]
    matched = [k for k, (kind, _) in enumerate(out) if kind == "matched"]
    assert len(matched) >= C.SCENE_COUNT and new._e.N == C.SCENE_N
    # the dense restatement applies the same pairs in scan order, each gated again at the state it meets
    ex, eP, applied = x0, P0, 0
    for k in matched:
        o = M.obs(scan[k][0], scan[k][1], scan[k][2], [out[k][1] - 1], None, C.SCENE_GATE)
        ex, eP, r = M.observe_model_dense(ex, eP, o)
        assert abs(r["d2"] - C.SCENE_GATE) > 1e-6 * C.SCENE_GATE              # (no step sits on its gate)
        applied += r["outcome"] == M.APPLIED
    assert applied >= 1
    check_state(new._e, ex, eP, "f64", "measure_model_assigned")
    assert not np.array_equal(new._e.get_x(), old._e.get_x())
    new.predict(U2)
    new.log.record(U2, None, [], [])                          # (what measure() records of a step without sightings: the edits replay in front of it)
    path = tmp_path / "assigned.npz"
    new.log.save(path)
    log = TrajectoryLog.load(path)
    assert [ed[1] for ed in log.edits] == ["observe_model"] * len(matched)
    fresh = engine(**kw)
    fresh.load_lowrank_state(x, s, d, U)
    log.replay(fresh)
    assert_same(fresh, new._e)
    fresh.close()


def test_measure_model_joint_with_device_candidates_is_the_default_path(tmp_path):
    from ekf_slam_amd.slam import EKF_SLAM
    from ekf_slam_amd.trajectory import TrajectoryLog
    J.assert_scene_premises()
    x, s, d, U, scan = J.ambiguous_scene()
    kw = dict(capacity=J.N0 + 8, tile=16, batch=8)
    runs = []
    for device_candidates in (False, True):
        f = EKF_SLAM(**kw)
        f._e.load_lowrank_state(x, s, d, U)
        f.log = TrajectoryLog()
        out, truncated = f.measure_model_joint(scan, J.GATE, 25.0, device_candidates=device_candidates)
        path = tmp_path / ("joint%d.npz" % device_candidates)
        f.log.save(path)
        runs.append((f, out, truncated, np.load(path, allow_pickle=True)))
    (f0, out0, tr0, log0), (f1, out1, tr1, log1) = runs
    assert out0 == out1 == [("matched", J.LM_A + 1), ("matched", J.LM_B + 1)] and tr0 is tr1 is False
    assert_same(f0._e, f1._e)
    assert sorted(log0.files) == sorted(log1.files)
    for name in log0.files:
        a, b = log0[name], log1[name]
        assert a.dtype == b.dtype and a.shape == b.shape and (a.tobytes() == b.tobytes() if a.dtype != object else repr(a.tolist()) == repr(b.tolist())), name
