"""GPU: motion steps through a model with its true Jacobians, a chain per launch (ekf_predict_model, ekf_motion_evaluate;
include/ekfslam.h).

The yardstick is the NumPy restatement of tests/predict_model_cases.py applied to THE STATE THE ENGINE REPORTED BEFORE THE CALL; stores,
tolerances and helpers are those of tests/helpers.py.  Where two engines must agree because they ran the same arithmetic on
the same inputs -- a chain against single calls, batch b against batch 1, the asynchronous pass against the synchronous one, the device
loops against the waited one, shards against one engine, a replayed log -- the comparison is assert_array_equal.

N0 = 150 landmarks are 300 strip columns: two workgroups of k_predict_model, the second one partly idle."""
import ctypes

import numpy as np
import pytest

import append_model_cases as A
import model_obs_cases as M
import predict_model_cases as PM
from helpers import R2, REL, RPOS, U2, assert_same, check_state, engine, getters, loaded, rel_err, state, status_of
from linear_obs_cases import N0, STORES
from removal_cases import lowrank_data, observe

pytestmark = pytest.mark.gpu
M2 = np.array([[0.04, 0.01], [0.01, 0.09]])
M3 = np.array([[0.04, 0.01, 0.0], [0.01, 0.09, 0.02], [0.0, 0.02, 0.25]])


def history(engines, x, ks):
    for q in engines:
        for k in ks:
            q.predict(U2); q.correct(observe(x, k), R2, k)


def group_of(count, N, pending, **kw):
    """`count` engines with the same state and history: `pending` corrections, deferred where batch > pending."""
    x = lowrank_data(N, 5)[0]
    es = [loaded(N, 5, **kw) for _ in range(count)]
    history(es, x, (5, N // 2, N - 3, 11, 40)[:pending])
    return es


def same_state(a, b):
    assert a.N == b.N
    for name in ("get_x", "get_s", "get_P", "get_P_diag_blocks"):
        np.testing.assert_array_equal(getattr(a, name)(), getattr(b, name)(), err_msg=name)


def observe_through_model(e, model, k, noise):
    x = e.get_x()
    rows = M.ROWS[model]
    o = M.obs(model, np.zeros(rows), RPOS if rows == 2 else 0.05, [k])
    o["z"][:rows] = M.jacobian(x, o)[0][:rows] + noise[:rows]
    e.observe_model(o["model"], o["z"][:rows], o["R"], o["landmarks"])


# ------------------------------------------------------------------------------------------------------------------
# 1. against the dense restatement
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage", STORES)
@pytest.mark.parametrize("pending", [0, 5])
def test_chains_against_the_dense_restatement(tile, storage, pending):
    # e gets the calls; twin gets them too and is read BEFORE each (reading flushes it; e keeps its pairs pending); still gets none
    e, twin, still = group_of(3, N0, pending, capacity=N0 + 8, tile=tile, storage=storage, batch=8)
    assert e.pending() == pending
    rng = np.random.default_rng(3)
    mixed = PM.chain(rng, 9)
    assert {s[0] for s in mixed} == {1, 2, 3}
    for name, steps in (("turn and drive", [PM.step(PM.TURN_DRIVE, [1.5, 40.0], M2)]), ("an arc", [PM.step(PM.ARC, [2.0, -75.0], M2)]),
                        ("a pose increment", [PM.step(PM.POSE_DELTA, [0.4, -0.3, 200.0], M3)]), ("a mixed chain of nine", mixed)):
        x0, s0, P0 = state(twin)
        ex, eP, eQ = PM.predict_model_dense(x0, P0, steps)
        e.predict_model(steps)
        assert e.pending() == pending
        twin.predict_model(steps)
        check_state(e, ex, eP, storage, name)
        pending = 0                                           # (check_state read P: the pairs are applied now)
        # x, Prr and the strip rows are F64 in every store and carry this call's error alone
        x, P = e.get_x(), e.get_P()
        errs = (rel_err(x, ex), float(np.abs(P[:3] - eP[:3]).max() / np.abs(eP).max()), rel_err(e.get_Q3(), eQ))
        print("%s [%s]: rel err x %.2e robot rows of P %.2e Q %.2e" % ((name, storage) + errs))
        assert max(errs) < REL, name
        # the landmarks, the landmark block, its live diagonal blocks and s: the bits of an engine that got no predict
        np.testing.assert_array_equal(x[3:], still.get_x()[3:])
        np.testing.assert_array_equal(P[3:, 3:], still.get_P()[3:, 3:])
        np.testing.assert_array_equal(e.get_P_diag_blocks()[1:], still.get_P_diag_blocks()[1:])
        np.testing.assert_array_equal(e.get_s(), still.get_s())


# ------------------------------------------------------------------------------------------------------------------
# 2. a chain of m is m single calls, bit for bit
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage", STORES)
@pytest.mark.parametrize("m", [1, 2, 9, 32])
def test_a_chain_is_bit_for_bit_its_single_calls(tile, storage, m):
    e, twin = group_of(2, N0, 3, capacity=N0 + 8, tile=tile, storage=storage, batch=8)
    steps = PM.chain(np.random.default_rng(m), m)
    e.predict_model(steps)
    for st in steps:
        twin.predict_model([st])
    assert e.pending() == twin.pending() == 3
    np.testing.assert_array_equal(e.get_Q3(), twin.get_Q3())
    same_state(e, twin)
    assert np.all(np.isfinite(e.get_P()))
    # ... and both go on alike: corrections, a model observation, a scan of new landmarks, another chain
    x = e.get_x()
    scan = A.scan(np.random.default_rng(m), 3)
    for q in (e, twin):
        for k in (7, N0 - 1, 90):
            q.predict(U2); q.correct(observe(x, k), R2, k)
        observe_through_model(q, M.RELATIVE_XY, 33, np.array([0.05, -0.02]))
        q.append_model(scan)
        q.predict_model(steps[:2])
    same_state(e, twin)


# ------------------------------------------------------------------------------------------------------------------
# 3. a fresh handle: the known answer, the reference's pose, its different covariance, Q
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [0, 1])
def test_the_known_answer_on_a_fresh_handle(N):
    n = 3 + 2 * N
    x0 = np.array([0.0, 0.0, 0.0, 5.0, 3.0][:n])
    P0 = np.zeros((n, n)); P0[2, 2] = 4.0
    if N:
        P0[3, 3] = P0[4, 4] = 0.5
        P0[2, 3] = P0[3, 2] = 0.3
    s0 = np.arange(1.0, N + 1.0)
    e, twin = engine(capacity=4, tile=16), engine(capacity=4, tile=16)
    for q in (e, twin):
        q.set_state(x0, P0, s0)
    # P = diag(0, 0, 4 deg^2), theta = 0, drive 10 straight: P_yy = (10 pi / 180)^2 * 4 and P_xy = 0
    e.predict_model([(PM.TURN_DRIVE, [10.0, 0.0], np.zeros((2, 2)))])
    twin.predict([10.0, 0.0])
    want = (10.0 * np.pi / 180.0) ** 2 * 4.0
    Pe, Pt = e.get_P(), twin.get_P()
    print("N = %d: P_yy %.17g for %.17g; ekf_predict's %.17g, ratio %.6f for k^2 = %.6f" % (N, Pe[1, 1], want, Pt[1, 1], Pt[1, 1] / Pe[1, 1], PM.K ** 2))
    assert abs(Pe[1, 1] - want) < 1e-12 * want and Pe[0, 1] == 0.0 and Pe[1, 0] == 0.0 and Pe[0, 0] == 0.0 and Pe[2, 2] == 4.0
    np.testing.assert_array_equal(e.get_x(), twin.get_x())
    # the same f, another F: the twin's P_yy is k^2 times as large (its Q = (W C) W' has no y entry at theta = 0)
    assert Pt[1, 1] == 400.0 and abs(Pt[1, 1] / Pe[1, 1] - PM.K ** 2) < 1e-9 * PM.K ** 2
    ex, eP, _ = PM.predict_model_dense(x0, P0, [PM.step(PM.TURN_DRIVE, [10.0, 0.0], np.zeros((2, 2)))])
    assert rel_err(Pe, eP) < REL and (not N or abs(Pe[1, 3] - 10.0 / PM.K * 0.3) < 1e-12)
    # a step that turns, over 360: still the reference's pose, bit for bit
    e.predict_model([(PM.TURN_DRIVE, [3.7, 123.4], M2), (PM.TURN_DRIVE, [0.9, 300.0], M2)])
    twin.predict([3.7, 123.4]); twin.predict([0.9, 300.0])
    np.testing.assert_array_equal(e.get_x(), twin.get_x())
    assert e.get_x()[2] == 123.4 + 300.0 - 360.0
    # ekf_get_Q: the last step's V M V'
    xb, Pb = e.get_x(), e.get_P()
    steps = [PM.step(PM.POSE_DELTA, [0.1, 0.2, 3.0], M3), PM.step(PM.ARC, [2.0, 40.0], M2)]
    e.predict_model(steps)
    ex, eP, eQ = PM.predict_model_dense(xb, Pb, steps)
    assert rel_err(e.get_Q3(), eQ) < REL and rel_err(e.get_P(), eP) < REL and rel_err(e.get_x(), ex) < REL
    # the host's copy of the kernel's function agrees with the restatement
    xn, F, V = e.motion_evaluate(PM.ARC, xb[:3], [2.0, 40.0])
    wF, wV = PM.F_V_of(PM.ARC, xb[:3], [2.0, 40.0])
    assert rel_err(F, wF) < 1e-12 and rel_err(V[:, :2], wV) < 1e-12 and not V[:, 2].any()


# ------------------------------------------------------------------------------------------------------------------
# 4. inside the engine: a schedule with every kind of call, deferred and asynchronous against batch 1
# ------------------------------------------------------------------------------------------------------------------
def _schedule(seed, N, steps, cap):
    """Ops of a run from N landmarks; a recorded predict stands in front of every op, so every predict_model comes directly behind one.
    Four appends early: the map crosses the tile-row edge at 24 landmarks (T = 16) soon."""
    rng = np.random.default_rng(seed)
    n, ops, sig = N, [], 900.0
    for t in range(steps):
        r = rng.random()
        if (2 <= t < 6 or r < 0.12) and n + 3 <= cap:
            m = int(rng.integers(1, 4))
            ops.append(("append_model", A.scan(rng, m, sig))); n += m; sig += m
        elif r < 0.4:
            m = int(rng.integers(1, 5))
            ops.append(("predict_model", PM.chain(rng, 9 + m)[9:] if rng.random() < 0.7 else PM.chain(rng, 9)[3:3 + m]))
        elif r < 0.65:
            ops.append(("correct", int(rng.integers(0, n)), rng.uniform(0.01, 0.05), rng.uniform(0.1, 0.4)))
        elif r < 0.85:
            ops.append(("observe", int(rng.choice([M.RANGE_BEARING, M.RANGE, M.RELATIVE_XY])), int(rng.integers(0, n)), 0.1 * rng.standard_normal(2)))
        elif n > 12:
            ops.append(("remove", int(rng.integers(0, n)))); n -= 1
        else:
            ops.append(("correct", 0, 0.02, 0.2))
    return ops


def _play(e, ops):
    beside = 0
    for op in ops:
        e.predict(U2)
        if op[0] == "append_model":
            e.append_model(op[1])
        elif op[0] == "predict_model":
            beside += e.pending() > 0
            e.predict_model(op[1])
        elif op[0] == "correct":
            x = e.get_x()
            e.correct(observe(x, op[1], op[2], op[3]), R2, op[1])
        elif op[0] == "observe":
            observe_through_model(e, op[1], op[2], op[3])
        else:
            e.remove_landmarks([op[1]])
    return beside


@pytest.fixture(scope="module")
def schedule_reference():
    ops = _schedule(29, 18, 70, 44)
    one = loaded(18, 5, capacity=48, tile=16, batch=1)
    _play(one, ops)
    return ops, one.N, getters(one)


@pytest.mark.parametrize("batch,asy", [(1, True), (8, False), (8, True)])
def test_a_schedule_with_model_predicts_is_bit_for_bit_that_of_batch_one(schedule_reference, batch, asy):
    ops, N, want = schedule_reference
    kinds = [op[0] for op in ops]
    assert kinds.count("predict_model") >= 10 and kinds.count("append_model") >= 5 and kinds.count("remove") >= 2 and kinds.count("observe") >= 6
    assert all(np.all(np.isfinite(g)) for g in want) and N > 24               # the map crossed the tile-row edge at 24 landmarks
    e = loaded(18, 5, capacity=48, tile=16, batch=batch, async_flush=asy)
    beside = _play(e, ops)
    assert batch == 1 or beside >= 4                          # chains with pairs pending (asynchronous: beside the pass that holds them)
    assert e.N == N
    for got, ref in zip(getters(e), want):
        np.testing.assert_array_equal(got, ref)


# ------------------------------------------------------------------------------------------------------------------
# 5. between the scans of ekf_measure in UC mode: the waited loop, the device loop and the device-decided loop
# ------------------------------------------------------------------------------------------------------------------
def test_between_the_scans_of_the_device_decided_loop():
    from decided_plans import make_plan
    from decided_plans import PARAMS
    from ekf_slam_amd.engine import Engine
    plan = make_plan(7, 300, 24, 8)
    runs = {}
    for mode in (1, 4):
        e = Engine(mode="uc", capacity=300, device_assoc=mode, tile=16, batch=8, **PARAMS)
        for t, (u, rows, idx, loc) in enumerate(plan):
            e.predict(u)
            e.measure(rows, u, idx, loc)
            if t in (8, 9, 16):
                # straight behind the scan: with device_assoc = 4 its rows are queued and nothing is settled when the call arrives
                e.predict_model([(PM.POSE_DELTA, [0.0, 0.0, 0.0], M3 * 1e-4), (PM.ARC, [1e-3, 0.01 * t], M2 * 1e-4)])
        runs[mode] = e
    assert runs[4].N > 40
    assert_same(runs[4], runs[1])


def test_between_the_scans_of_the_device_resident_loop():
    # w_pos = 0, the reference's live likelihood: cfg.device_assoc = 3 is the device-resident loop (tests/test_config2_uc_gpu.py's setup)
    from ekf_slam_amd.slam import EKF_SLAM_UC, Landmark
    from ekf_slam_amd.world import make_run
    N = 60
    _, run = make_run(N, 20260102, 14, policy="nearest", m=6)
    run = list(run)
    gpus = {mode: EKF_SLAM_UC(capacity=N, tile=16, batch=8, device_assoc=mode) for mode in (1, 3)}
    lms = {k: Landmark('SYNTHETIC') for k in gpus}
    for t, (u, scan) in enumerate(run):
        for k, e in gpus.items():
            e.predict(u); e.measure(scan, u, lms[k])
            if t in (3, 4, 9):
                e.predict_model([(PM.POSE_DELTA, [0.0, 0.0, 0.0], M3 * 1e-4), (PM.ARC, [1e-3, 0.01 * t], M2 * 1e-4)])
    assert gpus[3]._e.cfg.device_assoc == 3 and gpus[1]._e.N > 6
    assert_same(gpus[3]._e, gpus[1]._e)


# ------------------------------------------------------------------------------------------------------------------
# 6. shards: the same call on every shard, no exchange
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("batch", [1, 4])
def test_shards_predict_without_an_exchange(world, batch):
    from ekf_slam_amd.engine import Engine
    from ekf_slam_amd.sharding import ShardGroup
    N = 123
    x, s, d, U = lowrank_data(N, 5)
    kw = dict(capacity=N + 16, tile=16, batch=batch)
    g, one = ShardGroup(world, **kw), Engine(**kw)
    steps = PM.chain(np.random.default_rng(4), 9)
    for q in (g, one):
        q.load_lowrank_state(x, s, d, U)
        for k in (5, 60):
            q.predict(U2); q.correct(observe(x, k), R2, k)
        q.predict_model(steps)
    xe = one.get_x()
    for q in (g, one):
        for k in (7, 100, 3):
            q.predict(U2); q.correct(observe(xe, k), R2, k)
        q.predict(U2)                                         # a recorded predict directly in front
        q.predict_model(steps[3:5])
        q.correct(observe(xe, 50), R2, 50)
    Pg = g.get_P()
    assert not np.isnan(Pg).any()
    np.testing.assert_array_equal(Pg, one.get_P())
    np.testing.assert_array_equal(g.get_x(), one.get_x())
    for sh in g.shards:
        np.testing.assert_array_equal(sh.get_x(), one.get_x())
        np.testing.assert_array_equal(sh.get_P_diag_blocks(), one.get_P_diag_blocks())
        np.testing.assert_array_equal(sh.get_Q3(), one.get_Q3())
    g.close(); one.close()


def test_refused_between_begin_and_finish_of_a_sharded_correction():
    from ekf_slam_amd import _lib as L
    N = 60
    x = lowrank_data(N, 5)[0]
    kw = dict(capacity=N + 4, tile=16)
    e, twin = loaded(N, 5, force_sharded=1, **kw), loaded(N, 5, **kw)
    harr = (ctypes.c_void_p * 1)(e.h)
    steps = PM.chain(np.random.default_rng(2), 4)
    z = observe(x, 7)
    e.predict(U2); twin.predict(U2)
    e.correct_begin(z, R2, 7)
    st, msg = status_of(lambda: e.predict_model(steps))
    assert st == L.EKF_ERR_STATE and "predict_model" in msg and "begin and finish" in msg
    bad = [(PM.TURN_DRIVE, [1.0, float("nan")], M2)]
    assert status_of(lambda: e.predict_model(bad))[0] == L.EKF_ERR_INVALID_ARG         # the arguments come first
    assert e.lib.ekf_exchange_local(harr, 1) == 0
    e.correct_finish()
    twin.correct(z, R2, 7)
    e.predict_model(steps); twin.predict_model(steps)                                   # a lone shard with the sharded code path simply works
    assert_same(e, twin)


# ------------------------------------------------------------------------------------------------------------------
# 7. refusals, each before anything changes
# ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_state_alone():
    from ekf_slam_amd import _lib as L
    N = 60
    x = lowrank_data(N, 5)[0]
    kw = dict(capacity=N + 4, tile=16, batch=8)
    e, twin = loaded(N, 5, **kw), loaded(N, 5, **kw)
    history([e, twin], x, (4, 33, 9))                         # pairs pending and a recorded predict behind them
    e.predict(U2); twin.predict(U2)
    x_before, s_before, pend = e.get_x(), e.get_s(), e.pending()      # (reading x carries out e's predict; the twin's stays recorded)
    e.predict(U2); twin.predict(U2)                           # ... and one more, recorded on both while the refusals come in
    nan, inf = float("nan"), float("inf")
    good = [PM.step(PM.TURN_DRIVE, [1.0, 20.0], M2), PM.step(PM.POSE_DELTA, [0.1, 0.2, 30.0], M3), PM.step(PM.ARC, [1.0, 20.0], M2)]

    def make(m=3, **kw):
        arr, _ = e._motions((good * 11)[:max(m, 1)])
        for key, (b, idx, v) in kw.items():
            if idx is None:
                setattr(arr[b], key, v)
            else:
                getattr(arr[b], key)[idx] = v
        return arr

    def unchanged(name):
        assert b"predict_model" in e.lib.ekf_last_error(e.h), name
        n = ctypes.c_int32()
        assert e.lib.ekf_pending(e.h, ctypes.byref(n)) == 0 and n.value == pend, name

    bad = L.EKF_ERR_INVALID_ARG
    call = lambda arr, m: e.lib.ekf_predict_model(e.h, arr, m)
    assert e.lib.ekf_predict_model(None, make(1), 1) == bad
    assert call(None, 1) == bad; unchanged("null steps")
    for m in (0, -1, 33):
        assert call(make(33), m) == bad; unchanged("m = %d" % m)
    # (step 0 and step 2 have two inputs, step 1 three: M column-major 3 x 3, the leading block at 0, 1, 3, 4)
    cases = [("model 0", 0, dict(model=(0, None, 0))), ("model 4", 0, dict(model=(0, None, 4))), ("reserved", 0, dict(reserved=(0, None, 1))),
             ("NaN d", 0, dict(u=(0, 0, nan))), ("inf turn", 0, dict(u=(0, 1, inf))), ("NaN turn of a pose increment", 1, dict(u=(1, 2, nan))),
             ("inf M", 0, dict(M=(0, 0, inf))), ("asymmetric M", 0, dict(M=(0, 1, 0.02))), ("negative diagonal", 0, dict(M=(0, 4, -1.0))),
             ("negative minor", 0, dict(M=(0, 1, 9.0))), ("NaN in row 2", 1, dict(M=(1, 8, nan))), ("asymmetric in row 2", 1, dict(M=(1, 2, 0.01))),
             ("negative M22", 1, dict(M=(1, 8, -0.25))), ("negative (0, 2) minor", 1, dict(M=(1, 2, 9.0)))]
    for name, b0, kw_ in cases:
        (key, (_, idx, v)), = kw_.items()
        for b in ((0, 2) if b0 == 0 else (1,)):               # (step 2 has step 0's inputs) the bad step first, in the middle, last
            arr = make(3, **{key: (b, idx, v)})
            if name == "negative minor":
                arr[b].M[3] = 9.0
            if name == "negative (0, 2) minor":
                arr[b].M[6] = 9.0
            assert call(arr, 3) == bad, name
            unchanged("%s in step %d" % (name, b))
    arr = make(3)
    for q, v in enumerate([1.0, 1.0, 1.0, 1.0, 1.0, -1.0, 1.0, -1.0, 1.0]):      # every 2 x 2 minor is 0, the determinant -4
        arr[1].M[q] = v
    assert call(arr, 3) == bad; unchanged("negative determinant")
    # what a model does not read may hold anything: the third input and row 2 of M of a model with two inputs
    arr = make(3, u=(0, 2, nan))
    arr[0].M[8] = nan; arr[2].M[2] = inf
    assert call(arr, 3) == 0
    twin.predict_model(good)
    # nothing of all that changed anything: the recorded predict and the pending pairs were still there
    assert e.pending() == twin.pending() == pend
    assert_same(e, twin)
    assert not np.array_equal(e.get_x()[:3], x_before[:3]) and np.array_equal(e.get_s(), s_before)


# ------------------------------------------------------------------------------------------------------------------
# 8. the slam.py wrappers and a replayed log
# ------------------------------------------------------------------------------------------------------------------
def test_a_run_with_model_predicts_replays_from_its_log(tmp_path):
    from ekf_slam_amd.slam import SLAM
    from ekf_slam_amd.trajectory import FORMAT_PREDICT, TrajectoryLog
    from ekf_slam_amd.world import make_run
    _, run = make_run(40, 11, 24, policy="nearest", m=6)
    run = list(run)
    kw = dict(capacity=64, tile=16, batch=4)
    full = SLAM('EKF_SLAM', feed=run, landmark_method='SYNTHETIC', **kw)
    plain = SLAM('EKF_SLAM', feed=run, landmark_method='SYNTHETIC', **kw)
    full.slam.log = TrajectoryLog()
    for k in range(len(run)):
        full.runSlam(); plain.runSlam()
        if k == 7:
            full.slam.predict_turn_drive(0.05, 2.0, M2 * 1e-2)
        if k == 12:
            full.slam.predict_arc([0.02, 0.03, 0.01], [1.0, -2.0, 0.5], M2 * 1e-2)
            full.slam.predict_pose_delta(0.0, 0.0, 0.0, M3 * 1e-3)
        if k == 18:
            full.slam.predict_model([(PM.POSE_DELTA, [0.01, -0.02, 1.0], M3 * 1e-3), (PM.TURN_DRIVE, [0.02, -1.0], M2 * 1e-2)])
    path = tmp_path / "moved_run.npz"
    full.slam.log.save(path)
    log = TrajectoryLog.load(path)
    assert str(np.load(path)["format"]) == FORMAT_PREDICT and [(e[0], e[1]) for e in log.edits] == \
        [(8, "predict_model"), (13, "predict_model"), (13, "predict_model"), (19, "predict_model")]
    assert [len(log.model_predicts[q]) for q in range(4)] == [1, 3, 1, 2]
    fresh = engine(**kw)
    log.replay(fresh)
    assert fresh.N == 40 and not np.array_equal(plain.slam.x, full.slam.x)
    np.testing.assert_array_equal(fresh.get_x(), full.slam.x)
    np.testing.assert_array_equal(fresh.get_s(), full.slam.s)
    np.testing.assert_array_equal(fresh.get_P(), full.slam.P)
    assert np.all(np.isfinite(fresh.get_P()))


# ------------------------------------------------------------------------------------------------------------------
# 9. at size: 20 000 strip columns, 79 workgroups
# ------------------------------------------------------------------------------------------------------------------
def test_a_chain_of_thirty_two_at_ten_thousand_landmarks():
    N = 10000
    e, twin = loaded(N, 5, capacity=N, tile=128), loaded(N, 5, capacity=N, tile=128)
    steps = PM.chain(np.random.default_rng(32), 32)
    e.predict_model(steps)
    for st in steps:
        twin.predict_model([st])
    np.testing.assert_array_equal(e.get_x(), twin.get_x())
    strip, strip_twin = e.get_P_block(0, 0, 3, 3 + 2 * N), twin.get_P_block(0, 0, 3, 3 + 2 * N)
    np.testing.assert_array_equal(strip, strip_twin)
    np.testing.assert_array_equal(e.digest(), twin.digest())
    np.testing.assert_array_equal(e.get_Q3(), twin.get_Q3())
    x0 = lowrank_data(N, 5)[0]
    assert np.all(np.isfinite(strip)) and not np.array_equal(e.get_x()[:3], x0[:3]) and np.array_equal(e.get_x()[3:], x0[3:])
