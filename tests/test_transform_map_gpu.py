"""GPU: the whole map moved into another frame, in place (ekf_transform_map; include/ekfslam.h).

The yardstick is the NumPy restatement of tests/transform_map_cases.py applied to THE STATE A TWIN REPORTED BEFORE THE CALL -- a twin with
the same history, because reading P flushes and the transform is to meet pending pairs and a recorded predict; stores, tolerances and
helpers are those of tests/helpers.py.  Where two engines hold the same values -- the robot frame against ekf_extract_map over every
landmark, a reloaded twin given the same steps, the asynchronous pass and the device-decided loop against waited twins, a replayed log --
the comparison is assert_array_equal.

N = 140 with T = 16 is 18 tile rows (the last one half empty) and two workgroups of k_transform_state; T = 256 crosses its first tile-row
edge at landmark 128; the production edges (128 for F64, 256 for float) run the full-width 16-byte paths over two and three tile rows."""
import ctypes

import numpy as np
import pytest

import transform_map_cases as X
from helpers import R2, REL, TOL_KEPT32, TOL_ROW32, TOL_X32, U2, assert_same, check_state, engine, getters, loaded, rel_err, state, status_of
from removal_cases import lowrank_data, observe

pytestmark = pytest.mark.gpu
TOLS = (REL, TOL_X32, TOL_KEPT32, TOL_ROW32)
STORES = [(16, "f64", 140), (64, "f64", 140), (16, "f32", 140), (256, "f32_mixed", 140), (128, "f64", 200), (256, "f32", 300)]


def source_pair(pending=3, n=140, **kw):
    """Two engines with the same state and history: `pending` corrections left in the ring where the batch allows it and a recorded
    predict behind them."""
    x = lowrank_data(n, 5)[0]
    kw.setdefault("batch", 8)
    e, twin = loaded(n, 5, capacity=n + 4, **kw), loaded(n, 5, capacity=n + 4, **kw)
    for q in (e, twin):
        for k in [(5 * j + 1) % n for j in range(pending)]:
            q.predict(U2); q.correct(observe(x, k), R2, k)
        q.predict(U2)
    return e, twin


def check(e, ex, eP, storage, label, es, form):
    if form == "robot":
        X.check_robot_frame(e, ex, eP, storage, label, es, TOLS)
    else:
        check_state(e, ex, eP, storage, label, es)
    assert np.all(np.isfinite(e.get_P())) and np.all(np.isfinite(e.get_x()))


# ------------------------------------------------------------------------------------------------------------------
# 1. against the dense restatement
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", X.FORMS)
@pytest.mark.parametrize("tile,storage,n", STORES)
def test_a_transform_against_the_dense_restatement(tile, storage, n, form):
    e, twin = source_pair(3, n, tile=tile, storage=storage)
    assert e.pending() == 3
    x, s, P = state(twin)                                     # (flushes the twin)
    ex, es, eP = X.transform_dense(x, s, P, form)
    e.transform_map(*X.form_args(form))
    assert e.pending() == 0 and e.N == n
    check(e, ex, eP, storage, "%s N=%d T=%d" % (form, n, tile), es, form)


def test_an_empty_map_is_a_robot_only_state():
    for form in X.FORMS:
        e = engine(capacity=8, tile=16)
        x0, P0 = np.array([1.0, -2.0, 40.0]), X.random_spd(np.random.default_rng(3), 3)
        e.set_x(x0); e.set_P(P0)
        ex, es, eP = X.transform_dense(x0, np.zeros(0), P0, form)
        e.transform_map(*X.form_args(form))
        assert e.N == 0 and e.pending() == 0
        if form == "robot":
            assert not e.get_x().any() and not e.get_P().any()
        else:
            assert rel_err(e.get_x(), ex) < REL and rel_err(e.get_P(), eP) < REL


# ------------------------------------------------------------------------------------------------------------------
# 2. the robot frame: the bits of ekf_extract_map over every landmark
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage,n", STORES)
def test_the_robot_frame_is_the_extraction_of_every_landmark(tile, storage, n):
    e, twin = source_pair(3, n, tile=tile, storage=storage)
    d = twin.extract_map(range(n), "robot", tile=tile, capacity=n + 4)
    assert d.cfg.storage == e.cfg.storage and d.cfg.pass_arith == e.cfg.pass_arith
    e.transform_map("robot")
    assert_same(e, d)                                         # x, s, P, the diagonal blocks and the digest of every tile of the active rows


def test_a_landmark_exactly_on_the_robot_is_regular():
    x, s, P = X.scene_on_robot(12, 6, which=4)
    e = X.set_state(engine(capacity=16, tile=16), x, s, P)
    e.transform_map("robot")
    ex, es, eP = X.transform_dense(x, s, P, "robot")
    check(e, ex, eP, "f64", "a landmark on the robot", es, "robot")
    xe = e.get_x()
    assert xe[3 + 2 * 4] == 0.0 and xe[4 + 2 * 4] == 0.0


# ------------------------------------------------------------------------------------------------------------------
# 3. the rigid form against the library itself: an empty handle that sits at the transform, then ekf_join_map
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["exact", "uncertain"])
@pytest.mark.parametrize("tile,storage,n", STORES)
def test_the_rigid_form_is_a_join_into_a_handle_at_the_transform(tile, storage, n, form):
    e, twin = source_pair(3, n, tile=tile, storage=storage)
    g = engine(capacity=n + 4, tile=tile, storage=storage)
    g.set_x(X.T_RIGID)
    g.set_P(X.SIGMA if form == "uncertain" else np.zeros((3, 3)))
    assert g.join_map(twin) == 0 and g.N == n
    e.transform_map(*X.form_args(form))
    xg, sg, Pg = state(g)
    np.testing.assert_array_equal(e.get_x(), xg)              # bit for bit: POSE_DELTA at (t, r), RELATIVE_XY's inverse at (t, l_i)
    check_state(e, xg, Pg, storage, "%s against join_map N=%d T=%d" % (form, n, tile), sg)


# ------------------------------------------------------------------------------------------------------------------
# 4. invariance: what the robot sees of a landmark does not depend on the frame
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["exact", "uncertain"])
@pytest.mark.parametrize("tile,storage", [(16, "f64"), (64, "f64")])
def test_innovations_do_not_depend_on_the_frame(tile, storage, form):
    e, twin = source_pair(3, 140, tile=tile, storage=storage)
    x = twin.get_x()
    e.transform_map(*X.form_args(form))
    scale = np.abs(e.get_P()).max()
    Rz = np.array([[0.05, 0.01], [0.01, 0.2]])
    worst = 0.0
    for k in (0, 7, 63, 64, 139):
        d = x[3 + 2 * k:5 + 2 * k] - x[0:2]
        rb = [np.hypot(*d) + 0.3, np.degrees(np.arctan2(d[1], d[0])) - x[2] + 2.0]
        xy = X.rot(x[2]).T @ d + [0.2, -0.1]
        for model, z in ((1, rb), (4, xy)):
            ref, got = twin.model_innovation(model, z, Rz, [k]), e.model_innovation(model, z, Rz, [k])
            worst = max(worst, np.abs(np.asarray(got["nu"]) - np.asarray(ref["nu"])).max() / scale,
                        np.abs(np.asarray(got["S"]) - np.asarray(ref["S"])).max() / scale)
    print("%s T=%d: nu and S of RANGE_BEARING and RELATIVE_XY before and after, against the largest entry of P': worst %.2e" % (form, tile, worst))
    assert worst < REL


# ------------------------------------------------------------------------------------------------------------------
# 5. invalidation: the handle goes on exactly as one that was loaded with the transformed state
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", X.FORMS)
@pytest.mark.parametrize("asy", [False, True])
def test_the_handle_goes_on_as_a_reloaded_twin(asy, form):
    n = 140
    x0 = lowrank_data(n, 5)[0]
    kw = dict(capacity=n + 4, tile=16, batch=4, async_flush=asy)
    e = loaded(n, 5, **kw)
    e.prefetch_next([3, 9])
    e.predict(U2); e.correct(observe(x0, 11), R2, 11)
    e.transform_map(*X.form_args(form))
    assert e.pending() == 0
    twin = X.set_state(engine(**kw), *state(e))
    assert_same(e, twin)
    x1 = e.get_x()
    Rz = np.array([[0.02, 0.005], [0.005, 0.03]])
    for q in (e, twin):
        for k in (3, 9, 70, 139, 3):
            q.predict(U2); q.correct(observe(x1, k), R2, k)
            xy = X.rot(x1[2]).T @ (x1[3 + 2 * k:5 + 2 * k] - x1[0:2])
            q.observe_model(4, xy + 0.05, Rz, [(k + 1) % n])
        q.flush()
    assert_same(e, twin)


# ------------------------------------------------------------------------------------------------------------------
# 6. beside the other machinery
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", X.FORMS)
def test_beside_an_asynchronous_pass_just_queued(form):
    n = 140
    x = lowrank_data(n, 5)[0]
    runs = []
    for asy in (True, False):
        e = loaded(n, 5, capacity=n + 4, tile=16, batch=3, async_flush=asy)
        for k in (5, 60, 100):                                # the batch completes: its pass is queued (asynchronous: on the pass stream)
            e.predict(U2); e.correct(observe(x, k), R2, k)
        e.predict(U2); e.correct(observe(x, 7), R2, 7)        # and one pair recorded behind it
        e.transform_map(*X.form_args(form))
        assert e.pending() == 0
        x1 = e.get_x()
        for k in (3, 9, n - 1):
            e.predict(U2); e.correct(observe(x1, k), R2, k)
        runs.append(e)
    assert_same(runs[0], runs[1])


def test_behind_an_unsettled_scan_of_the_device_decided_loop():
    from decided_plans import PARAMS, make_plan
    from ekf_slam_amd.engine import Engine
    scans = make_plan(7, 300, 12, 8)
    t_small, S_small = [0.05, -0.03, 0.5], 1e-4 * X.SIGMA
    runs = []
    for mode in (4, 1):
        e = Engine(mode="uc", capacity=300, device_assoc=mode, tile=16, batch=4, **PARAMS)
        for t, (u, rows, ix, loc) in enumerate(scans):
            e.predict(u)
            e.measure(rows, u, ix, loc)
            if t == 8:                                        # straight behind the scan: with device_assoc = 4 nothing of it is settled
                e.transform_map("map", t_small, S_small)
                assert e.pending() == 0
        runs.append(e)
    assert runs[0].N == runs[1].N > 0
    assert_same(runs[0], runs[1])


# ------------------------------------------------------------------------------------------------------------------
# 7. refusals, each with the handle as it was and nothing flushed
# ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_alone():
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd.sharding import ShardGroup
    n = 20
    e, twin = source_pair(3, n, tile=16, batch=8)
    assert e.pending() == 3
    dp = ctypes.POINTER(ctypes.c_double)

    def call(h, frame, t, Sg):
        tv = None if t is None else np.ascontiguousarray(t, dtype=np.float64)
        Sv = None if Sg is None else np.ascontiguousarray(np.asarray(Sg, dtype=np.float64).reshape(-1, order="F"))
        return e.lib.ekf_transform_map(h, ctypes.c_int32(frame), None if tv is None else tv.ctypes.data_as(dp),
                                       None if Sv is None else Sv.ctypes.data_as(dp))

    bad = L.EKF_ERR_INVALID_ARG
    t = X.T_RIGID
    unsym = X.SIGMA.copy(); unsym[0, 2] += 1e-9
    indefinite = np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    minor3 = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 0.0], [2.0, 0.0, 1.0]])
    nanS = X.SIGMA.copy(); nanS[1, 1] = np.nan
    assert call(None, 0, t, None) == bad
    cases = [("a frame that is neither", 2, t, None, b"frame"), ("a negative frame", -1, None, None, b"frame"),
             ("no t", 0, None, None, b"needs the transform"), ("t not finite", 0, [0.0, np.inf, 1.0], None, b"not finite"),
             ("t NaN", 0, [np.nan, 0.0, 1.0], None, b"not finite"), ("Sigma not finite", 0, t, nanS, b"not finite"),
             ("Sigma not symmetric", 0, t, unsym, b"symmetric"), ("a negative diagonal entry", 0, t, -np.eye(3), b"non-negative"),
             ("a negative second minor", 0, t, indefinite, b"non-negative"), ("a negative third minor", 0, t, minor3, b"non-negative"),
             ("the robot frame with t", 1, t, None, b"neither"), ("the robot frame with Sigma", 1, None, X.SIGMA, b"neither")]
    for name, frame, tv, Sg, word in cases:
        assert call(e.h, frame, tv, Sg) == bad, name
        msg = e.lib.ekf_last_error(e.h)
        assert b"transform_map" in msg and word in msg, (name, msg)
        assert e.pending() == 3, name
    # a shard group refuses with the library's error, and says what the sharded form would need
    grp = ShardGroup(2, capacity=n + 4, tile=16)
    grp.load_lowrank_state(*lowrank_data(n, 5))
    gx = grp.shards[0].get_x()
    st, msg = status_of(lambda: grp.transform_map("map", t))
    assert st == bad and "sharded" in msg and "transform_map" in msg and grp.N == n
    np.testing.assert_array_equal(grp.shards[0].get_x(), gx)
    grp.close()
    # a lone shard between begin and finish
    sh = loaded(n, 5, capacity=n + 4, tile=16, force_sharded=1)
    xs = sh.get_x()
    sh.predict(U2)
    sh.correct_begin(observe(xs, 4), R2, 4)
    st, msg = status_of(lambda: sh.transform_map("robot"))
    assert st == L.EKF_ERR_STATE and "begin and finish" in msg and "transform_map" in msg
    harr = (ctypes.c_void_p * 1)(sh.h)
    assert sh.lib.ekf_exchange_local(harr, 1) == 0
    sh.correct_finish()
    # nothing was changed and nothing flushed: the handle is bit for bit its twin, and goes on
    assert e.pending() == 3
    for got, ref in zip(getters(e), getters(twin)):          # x, s, P, the diagonal blocks, ekf_P_digest
        np.testing.assert_array_equal(got, ref)
    e.transform_map("map", t, X.SIGMA)
    assert e.pending() == 0


# ------------------------------------------------------------------------------------------------------------------
# 8. the loop with ekf_extract_map's robot frame and ekf_join_map closes
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [16, 64])
def test_recentering_then_joining_at_the_old_pose_gives_the_map_back(tile):
    """recenter_on_robot, then join_map of the result into a third handle that sits at the old robot pose.  Recentring folds the robot's
    own uncertainty into the landmarks and drops the three degrees of freedom of the frame, so with G the stack of the join's Gx_i
    (= -Rot Hr_i) and S = P(robot, landmarks) the joined landmark block is P_ll + G Prr G' - G S - S' G' for a handle that sits at the
    pose exactly.  It is the original P_ll where the robot carried no uncertainty (Prr = 0, S = 0: a map in the frame of a pose it knows,
    as every filter here starts) -- that case reproduces the landmarks AND P; a state with an uncertain robot reproduces the landmarks
    and that closed form.  Both are held to REL."""
    n = 140
    # (a) a map whose robot is certain: the original landmarks and P come back
    x, s, P = X.scene(n, 21)
    P[:3, :] = P[:, :3] = 0.0
    e = X.set_state(engine(capacity=n + 4, tile=tile), x, s, P)
    e.transform_map("robot")
    g = engine(capacity=n + 4, tile=tile)
    g.set_x(x[:3]); g.set_P(np.zeros((3, 3)))
    assert g.join_map(e) == 0
    xg, sg, Pg = state(g)
    np.testing.assert_array_equal(sg, s)
    np.testing.assert_array_equal(xg[:2], x[:2])              # the robot composes with a zero pose
    err_x, err_P = rel_err(xg[3:], x[3:]), rel_err(Pg, P)
    print("T=%d, a certain robot: recenter_on_robot, then join_map at the old pose: rel err landmarks %.2e P %.2e" % (tile, err_x, err_P))
    assert err_x < REL and err_P < REL and xg[2] == X.wrap360(x[2])
    # (b) an uncertain robot, pending pairs and a recorded predict: the landmarks come back, P is the closed form
    e, twin = source_pair(3, n, tile=tile)
    x, s, P = state(twin)
    e.transform_map("robot")
    g = engine(capacity=n + 4, tile=tile)
    g.set_x(x[:3]); g.set_P(np.zeros((3, 3)))
    assert g.join_map(e) == 0
    xg, sg, Pg = state(g)
    G = np.zeros((2 * n, 3))
    for i in range(n):
        w = x[3 + 2 * i:5 + 2 * i] - x[0:2]
        G[2 * i:2 * i + 2] = [[1, 0, -w[1] / X.K], [0, 1, w[0] / X.K]]
    S = P[:3, 3:]
    want = P[3:, 3:] + G @ P[:3, :3] @ G.T - G @ S - S.T @ G.T
    err_x, err_P = rel_err(xg[3:], x[3:]), rel_err(Pg[3:, 3:], want)
    print("T=%d, an uncertain robot: rel err landmarks %.2e P(landmarks) against P_ll + G Prr G' - G S - S' G' %.2e" % (tile, err_x, err_P))
    assert err_x < REL and err_P < REL and not Pg[:3, :].any()
    np.testing.assert_array_equal(sg, s)


# ------------------------------------------------------------------------------------------------------------------
# 9. a logged run with two transforms replays bit for bit
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage,tile", [("f64", 16), ("f32", 16)])
def test_a_logged_run_with_two_transforms_replays(tmp_path, storage, tile):
    from ekf_slam_amd.slam import EKF_SLAM
    from ekf_slam_amd.trajectory import FORMAT_TRANSFORM_MAP, TrajectoryLog
    n = 24
    x0, s0, d0, U0 = lowrank_data(n, 5)
    kw = dict(capacity=n + 4, tile=tile, storage=storage, batch=4)

    def start():
        f = EKF_SLAM(**kw)
        f._e.load_lowrank_state(x0, s0, d0, U0)
        return f
    f = start()
    f.log = TrajectoryLog()
    f.predict(U2)
    f.log.record(U2, None, [], np.zeros((0, 2)))              # one step: the edits behind it are replayed at the end of the log
    Rz = np.array([[0.02, 0.005], [0.005, 0.03]])

    def steps(ks):
        for k in ks:
            x = f._e.get_x()
            f.predict_model([(3, [0.2, -0.1, 3.0], np.diag([0.01, 0.02, 0.3]))])
            f.observe_model(4, X.rot(x[2]).T @ (x[3 + 2 * (k - 1):5 + 2 * (k - 1)] - x[0:2]) + 0.03, Rz, [k])
    steps([2, 9])
    t, rms = f.align_to_anchors([1, 5, 20], [[3.0, 4.0], [-6.0, 1.0], [0.5, -9.0]], X.SIGMA)
    assert np.all(np.isfinite(t)) and rms > 0
    steps([11, 2])
    f.recenter_on_robot()
    steps([24])
    f._e.flush()
    f.log.save(tmp_path / "run.npz")
    assert str(np.load(tmp_path / "run.npz")["format"]) == FORMAT_TRANSFORM_MAP
    back = TrajectoryLog.load(tmp_path / "run.npz")
    assert [e[1] for e in back.edits].count("transform_map") == 2
    g = start()
    back.replay(g._e)
    g._e.flush()
    assert_same(f._e, g._e)
