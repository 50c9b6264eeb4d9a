"""GPU: linear observations as update-steps (ekf_observe_linear, ekf_linear_innovation, ekf_linear_rejections; include/ekfslam.h,
DESIGN.md section 3i).

The yardstick is the NumPy restatement of tests/linear_obs_cases.py applied to THE STATE THE ENGINE REPORTED BEFORE THE CALL (so float
tiles start from the same rounded inputs).  Tolerances as tests/helpers.py states them: F64 tiles REL = 1e-6
(BASELINE.json's bar; the measured values are printed), float tiles DESIGN.md section 5's bounds for one step -- x 1e-9, the entries
of P kept in F64 (robot rows, the landmarks' own 2 x 2 blocks) 2e-9, float-stored entries 2e-7 of the row's largest.  Where two
engines must agree because they ran the same kernels on the same inputs, the comparison is assert_array_equal.

N0 = 150 landmarks are 300 columns: two workgroups of k_gather_linear, the second one partly idle."""
import ctypes

import numpy as np
import pytest

import linear_obs_cases as C
from decided_plans import PARAMS
from helpers import R2, REL, RPOS, U2, assert_same, check_state, engine, getters, loaded, rel_err, state, status_of
from linear_obs_cases import N0, STORES, edge_landmark
from removal_cases import lowrank_data, observe

pytestmark = pytest.mark.gpu


def send(e, o, wait=False):
    return e.observe_linear(o["z"][:o["rows"]], o["R"], o["Hr"], o["landmarks"], o["Hl"], gate=o["gate"], wrap=o["wrap"], rows=o["rows"], wait=wait)


def ask(e, o):
    return e.linear_innovation(o["z"][:o["rows"]], o["R"], o["Hr"], o["landmarks"], o["Hl"], gate=o["gate"], wrap=o["wrap"], rows=o["rows"])


# ------------------------------------------------------------------------------------------------------------------
# 1. every kind against the dense restatement
# ------------------------------------------------------------------------------------------------------------------
def _kind_list(T, x):
    """(name, observation): every kind, the landmark pairs in one tile, in different tile rows, adjacent, in both orders, first / last."""
    e = edge_landmark(T)
    rng = np.random.default_rng(8)
    at = lambda k: x[3 + 2 * k:5 + 2 * k]
    return [("landmark fix, first", C.landmark_fix(0, at(0) + [0.3, -0.2], RPOS)),
            ("landmark fix, last, small R", C.landmark_fix(N0 - 1, at(N0 - 1) + [-0.1, 0.2], np.diag([1e-3, 2e-3]))),
            ("position fix", C.position_fix(x[:2] + [0.05, -0.02], RPOS)),
            ("heading fix over +-180", C.heading_fix(x[2] - 359.5, 0.01)),
            ("general H, one tile, lm0 < lm1", C.general(rng, e + 1, e + 2, x, 0.3)),
            ("general H, adjacent over a tile edge, lm0 > lm1", C.general(rng, e, e - 1, x, 0.3)),
            ("general H, first and last", C.general(rng, 0, N0 - 1, x, 0.3)),
            ("general H, last and first", C.general(rng, N0 - 1, 0, x, 0.3)),
            ("scalar on a landmark", C.scalar_on_landmark(e, 0.6 * at(e)[0] - 0.8 * at(e)[1] + 0.2, 0.05)),
            ("relative, different tile rows", C.relative(3, N0 - 2, at(3) - at(N0 - 2) + [0.2, 0.1], RPOS))]


@pytest.mark.parametrize("tile,storage", STORES)
def test_every_kind_against_the_dense_restatement(tile, storage):
    e = loaded(N0, 5, capacity=N0 + 8, tile=tile, storage=storage)
    x = lowrank_data(N0, 5)[0]
    for k in (5, edge_landmark(tile), N0 - 3):               # some history first, so that P is not the loaded one
        e.predict(U2); e.correct(observe(x, k), R2, k)
    for name, o in _kind_list(tile, e.get_x()):
        x0, _, P0 = state(e)
        ex, eP, want = C.observe_dense(x0, P0, o)
        got = send(e, o, wait=True)
        assert got["outcome"] == want["outcome"] == C.APPLIED, name
        tol = REL if storage == "f64" else 1e-9               # F64 arithmetic on what the getters report, in every storage kind
        errs = (rel_err(got["nu"], want["nu"]) if np.abs(want["nu"]).max() > 0 else 0.0, rel_err(got["S"], want["S"]), abs(got["d2"] - want["d2"]) / want["d2"])
        print("%s [%s]: d2 %.4g rel err nu %.2e S %.2e d2 %.2e" % ((name, storage, got["d2"]) + errs))
        assert max(errs) < tol, name
        check_state(e, ex, eP, storage, name)
        if o["rows"] == 1:
            assert got["S"][0, 1] == 0.0 and got["S"][1].tolist() == [0.0, 1.0] and got["nu"][1] == 0.0
    assert e.N == N0 and e.linear_rejections() == (0, 0)


# ------------------------------------------------------------------------------------------------------------------
# 2. it is a deferred step
# ------------------------------------------------------------------------------------------------------------------
def _schedule(seed, N, steps, per_row):
    """A random schedule of predict / append / correct / observe as a pure function of its arguments (z from the loaded x, not from the
    engine); the appends carry the map over a tile-row edge."""
    rng = np.random.default_rng(seed)
    x = lowrank_data(N, 5)[0]
    pos = [x[3 + 2 * k:5 + 2 * k].copy() for k in range(N)]
    ops = []
    target = (N // per_row + 1) * per_row + 2
    for t in range(steps):
        r = rng.random()
        if len(pos) < target and r < 0.25:
            p = rng.uniform(-20, 20, 2)
            ops.append(("append", p, 900.0 + t)); pos.append(p)
            continue
        n = len(pos)
        xs = np.concatenate([x[:3]] + pos)
        if r < 0.6:
            k = int(rng.integers(0, n))
            ops.append(("correct", observe(xs, k, dr=0.02 * rng.standard_normal(), db=0.3 * rng.standard_normal()), k))
            continue
        kind = int(rng.integers(0, 5))
        i, j = (int(v) for v in rng.choice(n, 2, replace=False))
        if kind == 0:
            o = C.landmark_fix(i, pos[i] + 0.2 * rng.standard_normal(2), RPOS)
        elif kind == 1:
            o = C.position_fix(x[:2] + 0.1 * rng.standard_normal(2), RPOS)
        elif kind == 2:
            o = C.heading_fix(x[2] + (t + 1.0) + rng.standard_normal(), 0.5)  # (predict turns the robot by 1 degree per step)
        elif kind == 3:
            o = C.general(rng, i, j, xs, 0.2)
        else:
            o = C.relative(n - 1, j if j != n - 1 else i, pos[n - 1] - pos[j if j != n - 1 else i] + 0.1 * rng.standard_normal(2), RPOS)
        if rng.random() < 0.15:
            o["gate"] = 1e-6                                  # a gated one now and then: it takes its slot all the same
        ops.append(("observe", o))
    return ops


def _play(e, ops):
    pend = []
    for op in ops:
        e.predict(U2)
        if op[0] == "append":
            e.append(U2, R2, op[1], op[2])
        elif op[0] == "correct":
            e.correct(op[1], R2, op[2])
        else:
            send(e, op[1])
        pend.append(e.pending())
    return pend


@pytest.fixture(scope="module")
def schedule_reference():
    ops = _schedule(18, 20, 60, 8)
    one = loaded(20, 5, capacity=40, tile=16, batch=1)
    _play(one, ops)
    return ops, getters(one), one.linear_rejections()


@pytest.mark.parametrize("batch,asy", [(3, False), (8, False), (3, True), (8, True)])
def test_a_schedule_with_observations_is_deferred_like_corrections(schedule_reference, batch, asy):
    ops, want, rejected = schedule_reference
    assert sum(op[0] == "observe" for op in ops) >= 12 and sum(op[0] == "append" for op in ops) >= 5 and rejected[1] >= 1
    e = loaded(20, 5, capacity=40, tile=16, batch=batch, async_flush=asy)
    pend = _play(e, ops)
    assert max(pend) >= batch - 1 and (not asy or max(pend) > batch)      # the ring was in use (asynchronous: beyond one batch, so it wrapped)
    assert e.N > 24                                           # the appends crossed the tile-row edge at 24 landmarks
    for got, ref in zip(getters(e), want):
        np.testing.assert_array_equal(got, ref)
    assert e.linear_rejections() == rejected


def test_an_observation_waits_for_the_batch_boundary():
    from ekf_slam_amd import _lib as L
    x = lowrank_data(N0, 5)[0]
    e = loaded(N0, 5, capacity=N0 + 8, tile=64, batch=4)
    e.timing_enable(L.EKF_KERNEL_DOWNDATE, True, 16)
    e.timing_enable(L.EKF_KERNEL_GATHER, True, 16)
    e.timing_read(L.EKF_KERNEL_DOWNDATE); e.timing_read(L.EKF_KERNEL_GATHER)
    send(e, C.position_fix(x[:2] + 0.05, RPOS))
    assert e.pending() == 1
    assert e.timing_read(L.EKF_KERNEL_DOWNDATE)[0] == 0 and e.timing_read(L.EKF_KERNEL_GATHER)[0] == 1
    send(e, C.landmark_fix(7, x[17:19] + 0.1, RPOS)); e.correct(observe(x, 9), R2, 9)
    assert e.pending() == 3 and e.timing_read(L.EKF_KERNEL_DOWNDATE)[0] == 0
    send(e, C.heading_fix(x[2] + 1.0, 0.5))                  # the fourth step of the batch: the pass runs
    assert e.pending() == 0 and e.timing_read(L.EKF_KERNEL_DOWNDATE)[0] == 1 and e.downdate_kernel_name()[1] == 4


# ------------------------------------------------------------------------------------------------------------------
# 3. H = (+I, -I) against ekf_constrain_landmarks
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage", [(16, "f64"), (64, "f64")])
def test_plus_and_minus_identity_matches_constrain_landmarks(tile, storage):
    ed = edge_landmark(tile)
    x = lowrank_data(N0, 5)[0]
    for i, j, delta in ((ed, ed - 1, [0.3, -0.1]), (0, N0 - 1, None), (N0 - 1, 4, [1.0, 2.0])):
        e = loaded(N0, 5, capacity=N0 + 8, tile=tile, storage=storage, batch=4)
        twin = loaded(N0, 5, capacity=N0 + 8, tile=tile, storage=storage, batch=4)
        for q in (e, twin):
            q.predict(U2); q.correct(observe(x, i), R2, i)    # (a pair pending when the observation arrives)
        d = np.zeros(2) if delta is None else np.asarray(delta)
        got = send(e, C.relative(i, j, d, RPOS), wait=True)
        d2, S = twin.landmark_distance(i, j, delta, RPOS)
        twin.constrain_landmarks(i, j, delta, RPOS)
        errs = (abs(got["d2"] - d2) / d2, rel_err(got["S"], S), rel_err(e.get_x(), twin.get_x()), rel_err(e.get_P(), twin.get_P()),
                rel_err(e.get_P_diag_blocks(), twin.get_P_diag_blocks()))
        print("observe_linear (+I, -I) against constrain_landmarks (%d, %d) [T = %d]: rel diff d2 %.2e S %.2e x %.2e P %.2e blocks %.2e" % ((i, j, tile) + errs))
        assert max(errs) < REL


# ------------------------------------------------------------------------------------------------------------------
# 4. the innovation
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage,asy", [(16, "f64", False), (64, "f64", True), (256, "f32_mixed", False)])
def test_linear_innovation_reports_what_the_observation_will_and_changes_nothing(tile, storage, asy):
    x = lowrank_data(N0, 5)[0]
    kw = dict(capacity=N0 + 8, tile=tile, storage=storage, batch=8, async_flush=asy)
    e, twin = loaded(N0, 5, **kw), loaded(N0, 5, **kw)
    ks = (5, edge_landmark(tile), N0 - 3, 11, 12, 40, 41, 42, 43, 44, 45)      # a full batch (a pass in flight with async_flush) and three more
    for q in (e, twin):
        for k in ks:
            q.predict(U2); q.correct(observe(x, k), R2, k)
    pend = e.pending()
    assert pend >= 3
    for name, o in _kind_list(tile, x)[:7]:
        for q in (e, twin):
            q.predict(U2)
        x_before = e.get_x()
        want = ask(e, o)
        assert e.pending() == pend
        np.testing.assert_array_equal(e.get_x(), x_before)
        got = send(e, o, wait=True)
        send(twin, o)
        for key in ("nu", "S", "d2", "outcome"):
            np.testing.assert_array_equal(np.asarray(got[key]), np.asarray(want[key]), err_msg=name + " " + key)
        pend = e.pending()
    assert_same(e, twin)                                      # the twin never asked


# ------------------------------------------------------------------------------------------------------------------
# 5. gate and irregular S
# ------------------------------------------------------------------------------------------------------------------
def test_gated_and_irregular_observations_change_nothing():
    """A landmark fixed with R = 0 is left with an own block and rows that are zero up to rounding (checked); the second fix needs them
    EXACTLY zero for S = 0, so the state is reloaded with those rows zeroed -- rounding residue of 1e-18 is regular or not by chance
    (tests/test_merge_landmarks_gpu.py makes the same remark about its singular pair)."""
    from ekf_slam_amd import _lib as L
    x = lowrank_data(N0, 5)[0]
    kw = dict(capacity=N0 + 8, tile=64, batch=4)
    e, twin = loaded(N0, 5, **kw), engine(**kw)
    k, a = 70, 3 + 2 * 70
    fix0 = C.landmark_fix(k, x[a:a + 2] + [0.4, -0.3], np.zeros((2, 2)))
    assert send(e, fix0, wait=True)["outcome"] == L.EKF_LINEAR_APPLIED
    x1, s1, P1 = state(e)
    assert np.abs(P1[a:a + 2, :]).max() < 1e-12 * np.abs(P1).max() and np.abs(x1[a:a + 2] - fix0["z"]).max() < 1e-12
    P1[a:a + 2, :] = 0.0; P1[:, a:a + 2] = 0.0
    for q in (e, twin):
        q.set_state(x1, P1, s1)
        q.predict(U2); q.correct(observe(x1, 9), R2, 9)      # a pair pending
    assert e.linear_rejections() == (0, 0)
    before = getters(twin)
    gated = C.landmark_fix(12, x1[27:29] + [2.0, 1.0], RPOS, gate=3.0)
    fix1 = C.landmark_fix(k, fix0["z"] + [0.1, 0.0], np.zeros((2, 2)))
    # with a result: the outcome comes back, nothing read afterwards differs
    res = send(e, gated, wait=True)
    assert res["outcome"] == L.EKF_LINEAR_GATED and res["d2"] > 3.0 and e.pending() == 2
    st, msg = status_of(lambda: send(e, fix1, wait=True))
    assert st == L.EKF_ERR_STATE and "observe_linear" in msg and e.pending() == 3
    inn = ask(e, fix1)
    assert inn["outcome"] == L.EKF_LINEAR_IRREGULAR and np.isnan(inn["d2"]) and not inn["S"].any()
    assert e.linear_rejections() == (1, 1) and e.linear_rejections() == (0, 0)
    # without one: the state stays finite and unchanged, the no-ops are counted
    send(e, gated)                                            # (the fourth step: the pass runs over two zero pairs)
    send(e, fix1)
    assert e.pending() == 1
    assert e.linear_rejections() == (1, 1) and e.linear_rejections() == (0, 0)
    for got, ref in zip(getters(e), before):
        assert np.all(np.isfinite(got))
        np.testing.assert_array_equal(got, ref)
    # the same observation with a larger gate applies, and the handle goes on like a twin that never saw the no-ops
    gated["gate"] = res["d2"] * 1.5
    for q in (e, twin):
        assert send(q, gated, wait=True)["outcome"] == L.EKF_LINEAR_APPLIED
        q.predict(U2); q.correct(observe(x1, 12), R2, 12)
    assert_same(e, twin)
    assert rel_err(e.get_x()[27:29], before[0][27:29]) > 1e-6


# ------------------------------------------------------------------------------------------------------------------
# 6. refusals, in the header's order, each before anything changes
# ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_state_alone():
    from ekf_slam_amd import _lib as L
    x = lowrank_data(N0, 5)[0]
    kw = dict(capacity=N0 + 8, tile=64, batch=8)
    e, twin = loaded(N0, 5, **kw), loaded(N0, 5, **kw)
    for q in (e, twin):
        for k in (4, 77):
            q.predict(U2); q.correct(observe(x, k), R2, k)
    x_before, pend = e.get_x(), e.pending()
    nan, inf = float("nan"), float("inf")

    def make(**kw):
        o = C.general(np.random.default_rng(1), 5, 6, x)
        ob = e._linear_obs(o["z"], o["R"], o["Hr"], o["landmarks"], o["Hl"], o["gate"], o["wrap"], o["rows"])
        for key, (idx, v) in kw.items():
            if key == "Hl":
                ob.Hl[idx[0]][idx[1]] = v
            elif idx is None:
                setattr(ob, key, v)
            else:
                getattr(ob, key)[idx] = v
        return ob

    def both_lm(a, b):
        ob = make(); ob.lm[0], ob.lm[1] = a, b
        return ob

    cases = [("rows 0", make(rows=(None, 0)), L.EKF_ERR_INVALID_ARG), ("rows 3", make(rows=(None, 3)), L.EKF_ERR_INVALID_ARG),
             ("NaN z", make(z=(1, nan)), L.EKF_ERR_INVALID_ARG), ("inf Hr", make(Hr=(4, inf)), L.EKF_ERR_INVALID_ARG),
             ("NaN Hl", make(Hl=((1, 2), nan)), L.EKF_ERR_INVALID_ARG), ("inf R", make(R=(0, inf)), L.EKF_ERR_INVALID_ARG),
             ("NaN gate", make(gate=(None, nan)), L.EKF_ERR_INVALID_ARG), ("asymmetric R", make(R=(1, 0.2)), L.EKF_ERR_INVALID_ARG),
             ("negative diagonal", make(R=(3, -1.0)), L.EKF_ERR_INVALID_ARG), ("the same landmark twice", both_lm(5, 5), L.EKF_ERR_INVALID_ARG),
             ("-2", both_lm(-2, 6), L.EKF_ERR_INVALID_ARG), ("N", both_lm(5, N0), L.EKF_ERR_INDEX), ("N alone", both_lm(N0 + 3, -1), L.EKF_ERR_INDEX)]
    res = L.EkfLinearResult()
    for name, ob, want in cases:
        for entry, fn in (("observe_linear", lambda: e.lib.ekf_observe_linear(e.h, ctypes.byref(ob), None)),
                          ("observe_linear", lambda: e.lib.ekf_observe_linear(e.h, ctypes.byref(ob), ctypes.byref(res))),
                          ("linear_innovation", lambda: e.lib.ekf_linear_innovation(e.h, ctypes.byref(ob), ctypes.byref(res)))):
            assert fn() == want, (entry, name)
            assert entry.encode() in e.lib.ekf_last_error(e.h), (entry, name)
            assert e.pending() == pend and e.N == N0
            np.testing.assert_array_equal(e.get_x(), x_before)
    ok = make()
    assert e.lib.ekf_observe_linear(e.h, None, None) == L.EKF_ERR_INVALID_ARG
    assert e.lib.ekf_linear_innovation(e.h, ctypes.byref(ok), None) == L.EKF_ERR_INVALID_ARG
    # rows = 1 ignores row 1 altogether: garbage there is no reason to refuse, and only R00 >= 0 matters
    one = make(rows=(None, 1), z=(1, nan), R=(3, -5.0)); one.R[1] = 7.0; one.Hr[1] = inf
    assert e.lib.ekf_linear_innovation(e.h, ctypes.byref(one), ctypes.byref(res)) == L.EKF_OK and res.S[1] == 0.0 and res.S[3] == 1.0
    assert e.lib.ekf_linear_innovation(e.h, ctypes.byref(make(rows=(None, 1), R=(0, -1.0))), ctypes.byref(res)) == L.EKF_ERR_INVALID_ARG
    assert e.linear_rejections() == (0, 0)
    assert_same(e, twin)
    # sharded handles: refused, the message says why; the arguments are checked first and a pending exchange is an EKF_ERR_STATE
    sh = engine(capacity=64, tile=16, world=2, rank=0)
    for fn in (lambda: send(sh, C.position_fix([0.0, 0.0], RPOS)), lambda: ask(sh, C.position_fix([0.0, 0.0], RPOS))):
        st, msg = status_of(fn)
        assert st == L.EKF_ERR_INVALID_ARG and "shard" in msg
    st, msg = status_of(lambda: sh.observe_linear([0.0, nan], RPOS))
    assert st == L.EKF_ERR_INVALID_ARG and "shard" not in msg
    lone = loaded(N0, 5, capacity=N0 + 8, tile=64, force_sharded=1)
    lone.predict(U2); lone.correct_begin(observe(x, 3), R2, 3)
    st, msg = status_of(lambda: send(lone, C.position_fix(x[:2], RPOS)))
    assert st == L.EKF_ERR_STATE and "begin and finish" in msg
    harr = (ctypes.c_void_p * 1)(lone.h)
    assert lone.lib.ekf_exchange_local(harr, 1) == 0
    lone.correct_finish()


# ------------------------------------------------------------------------------------------------------------------
# 7. a lone shard
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 4])
def test_a_lone_shard_with_the_sharded_code_path_simply_works(batch):
    x = lowrank_data(N0, 5)[0]
    e = loaded(N0, 5, capacity=N0 + 8, tile=64, force_sharded=1, batch=batch)
    twin = loaded(N0, 5, capacity=N0 + 8, tile=64, batch=batch)
    harr = (ctypes.c_void_p * 1)(e.h)

    def corrections(ks):
        for k in ks:
            z = observe(x, k)
            e.predict(U2); twin.predict(U2)
            e.correct_begin(z, R2, k)
            assert e.lib.ekf_exchange_local(harr, 1) == 0
            e.correct_finish()
            twin.correct(z, R2, k)

    corrections((3, 30, 149))
    obs = _kind_list(64, x)
    for o in (obs[0][1], obs[2][1], obs[5][1]):
        for q in (e, twin):
            send(q, o)
    corrections((0, 30, 31, 100, 149))
    for q in (e, twin):
        assert send(q, obs[3][1], wait=True)["outcome"] == 1
    corrections((1, 148))
    assert_same(e, twin)


# ------------------------------------------------------------------------------------------------------------------
# 8. unknown correspondence: observations between the scans of the device-resident loops
# ------------------------------------------------------------------------------------------------------------------


def _uc_run(device_assoc, params):
    cap = N0 + 40
    e = loaded(N0, 3, "uc", capacity=cap, tile=64, batch=8, device_assoc=device_assoc, **params)
    lm_index = np.arange(1, cap + 1, dtype=np.float64)
    lm_loc = np.random.default_rng(5).uniform(-20, 20, (cap, 2))
    rng = np.random.default_rng(9)
    for t in range(3):
        e.predict(U2)
        x, s = e.get_x(), e.get_s()                           # (the pose the scan is taken from: the position cost is strict)
        ks = [9 + t, 70, 140 - t]
        rows = [list(observe(x, k)) + [s[k]] for k in ks] + [[3.0 + t, 45.0, 7e6 + t]]      # the last row matches nothing: appended
        e.measure(np.array(rows), U2, lm_index, lm_loc)
        # straight behind the scan: with device_assoc = 4 its rows are queued and nothing is settled when the observations arrive
        send(e, C.position_fix(x[:2] + [0.03, -0.02], RPOS))
        send(e, C.landmark_fix(ks[0], x[3 + 2 * ks[0]:5 + 2 * ks[0]] + [0.1, 0.05], RPOS))
        assert send(e, C.general(rng, 70, N0 - 1, x, 0.2), wait=True)["outcome"] == 1
        send(e, C.heading_fix(x[2] + 0.4, 0.3, gate=1e-9))   # gated: a zero pair in the ring between two scans
    assert e.N == N0 + 3 and e.linear_rejections() == (0, 3)
    return e


def test_observations_between_scans_signature_only():
    runs = {m: _uc_run(m, dict(w_pos=0.0)) for m in (1, 3)}
    assert_same(runs[3], runs[1])


def test_observations_between_scans_position_weighted():
    runs = {m: _uc_run(m, PARAMS) for m in (1, 4)}
    assert_same(runs[4], runs[1])


# ------------------------------------------------------------------------------------------------------------------
# 9. at size
# ------------------------------------------------------------------------------------------------------------------
def test_at_size_ten_thousand_landmarks_f64():
    N = 10000
    x, s, d, U = lowrank_data(N, 21)
    rng = np.random.default_rng(6)
    e = engine(capacity=N, storage="f64", tile=128, batch=8)
    e.load_lowrank_state(x, s, d, U)
    f = C.Factored(x, d, U)
    at = lambda k: f.x[3 + 2 * k:5 + 2 * k]
    fixes = [C.position_fix(x[:2] + [0.03, -0.02], RPOS), C.landmark_fix(N - 1, at(N - 1) + [0.2, -0.1], RPOS), C.general(rng, N // 2 + 1, 40, x, 0.2)]
    plan = [("c", 7), ("o", 0), ("c", N // 3), ("c", N - 1), ("o", 1), ("c", 40), ("o", 2), ("c", N // 2 + 1), ("c", 7), ("c", 5000)]
    d2 = []
    for what, q in plan:                                      # (no predict: F P F' leaves the factored form)
        if what == "c":
            z = observe(f.x, q)
            f.correct(z, R2, q)
            e.correct(z, R2, q)
        else:
            d2.append((f.observe(fixes[q])["d2"], send(e, fixes[q], wait=True)["d2"]))
    assert e.pending() == 2                                   # one pass of 8 pairs so far: the last fix was read patched with 6
    n = 3 + 2 * N
    errs = {"d2": max(abs(b - a) / a for a, b in d2), "x": rel_err(e.get_x(), f.x), "blocks": rel_err(e.get_P_diag_blocks(), f.diag_blocks()),
            "robot rows": rel_err(e.get_P_block(0, 0, 3, n), f.rows(0, 3))}
    for r in (3 + 2 * (N - 1) - 6, 3 + 2 * 40, 3 + 2 * (N // 2 + 1)):
        got, want = e.get_P_block(r, 0, 8, n), f.rows(r, 8)
        errs["rows %d" % r] = float((np.abs(got - want).max(axis=1) / np.abs(want).max(axis=1)).max())
    tr, sq = f.trace_and_squares()
    dg = e.digest()
    errs["trace"], errs["sum of squares"] = abs(dg[0] - tr) / tr, abs(dg[2] - sq) / sq
    print("at size N = %d: " % N + ", ".join("%s %.2e" % kv for kv in errs.items()))
    assert max(errs.values()) < REL
    e.close()


# ------------------------------------------------------------------------------------------------------------------
# 10. the slam.py wrappers and a replayed log
# ------------------------------------------------------------------------------------------------------------------
def test_a_run_with_fixes_replays_from_its_log(tmp_path):
    from ekf_slam_amd.slam import SLAM
    from ekf_slam_amd.trajectory import FORMAT_OBSERVE, TrajectoryLog
    from ekf_slam_amd.world import make_run
    _, run = make_run(40, 11, 24, policy="nearest", m=6)
    run = list(run)
    kw = dict(capacity=64, tile=16, batch=4)
    full = SLAM('EKF_SLAM', feed=run, landmark_method='SYNTHETIC', **kw)
    plain = SLAM('EKF_SLAM', feed=run, landmark_method='SYNTHETIC', **kw)
    full.slam.log = TrajectoryLog()
    for k in range(len(run)):
        full.runSlam(); plain.runSlam()
        xs = full.slam.x
        if k == 7:
            assert full.slam.fix_robot_position(xs[:2] + [0.05, -0.05], RPOS) is None
        if k == 12:
            res = full.slam.fix_landmark(3, xs[7:9] + [0.1, 0.0], RPOS, gate=50.0, wait=True)      # 1-based at this layer: entries 7, 8 of x
            assert res["outcome"] == 1 and 0 < res["d2"] < 50.0
            np.testing.assert_array_equal(res["nu"], (xs[7:9] + [0.1, 0.0]) - xs[7:9])
        if k == 18:
            want = full.slam.linear_innovation([xs[2] + 1.0], 0.5, [0.0, 0.0, 1.0], wrap=(1, 0), rows=1)
            got = full.slam.fix_robot_heading(xs[2] + 1.0, 0.5, wait=True)
            assert got["d2"] == want["d2"] and got["nu"][0] == want["nu"][0]
    path = tmp_path / "fixed_run.npz"
    full.slam.log.save(path)
    log = TrajectoryLog.load(path)
    assert str(np.load(path)["format"]) == FORMAT_OBSERVE and [(e[0], e[1], e[2].tolist()) for e in log.edits] == \
        [(8, "observe", []), (13, "observe", [3]), (19, "observe", [])]
    fresh = engine(**kw)
    log.replay(fresh)
    np.testing.assert_array_equal(fresh.get_x(), full.slam.x)
    np.testing.assert_array_equal(fresh.get_s(), full.slam.s)
    np.testing.assert_array_equal(fresh.get_P(), full.slam.P)
    assert full.slam.linear_rejections() == (0, 0)
    assert rel_err(full.slam.x, plain.slam.x) > 1e-6          # the fixes did move the map
