"""GPU: a linear observation with a dense k x n H (ekf_observe_dense, ekf_observe_dense_innovation; include/ekfslam.h, DESIGN.md section
3za) and the three policies on top of it (fix_centroid, constrain_displacements, condition_on).

The yardstick is the NumPy restatement of tests/observe_dense_cases.py applied to THE STATE A TWIN REPORTS: twin.get_x() / get_P() of a
twin with the same history (three pending pairs, a recorded predict, removals).  The state is held to the project's own tolerances
(helpers.check_state: REL on F64 stores, the float-tile tolerances of the joint update's tests on float stores -- the same pass, one
rounding per entry); S, nu and d2 to the DERIVED bars of the cases file, the worst ratio of error to bar printed before it is asserted
to be at most 1.  Where the contract is equality the comparison is assert_array_equal.

The stores are solve_map_cases.STORES (tile edges 16, 64, 128, 256; F64 and float tiles; N = 140, 200, 300), N = 96 at edge 64 (the map
ends on a tile edge), N = 1, and N = 0 (a robot-only H: no tile pass, no column lanes)."""
import ctypes

import numpy as np
import pytest

import helpers
import observe_dense_cases as C
import solve_map_cases as V
from helpers import R2, REL, U2, assert_same, engine, getters, loaded, rel_err, status_of
from removal_cases import lowrank_data, observe

pytestmark = pytest.mark.gpu
STORES = V.STORES + [(64, "f64", 96), (16, "f64", 1)]


def sources(count, pending=3, n=140, **kw):
    """`count` engines with the same state and history: `pending` corrections left in the ring where the batch allows it and a
    recorded predict behind them (test_multiply_map_gpu's sources)."""
    x = lowrank_data(n, 5)[0]
    kw.setdefault("batch", 8)
    out = [loaded(n, 5, capacity=n + 4, **kw) for _ in range(count)]
    for q in out:
        for k in [(5 * j + 1) % n for j in range(min(pending, n))]:
            q.predict(U2); q.correct(observe(x, k), R2, k)
        q.predict(U2)
    return out


def kind(storage):
    return "f64" if storage == "f64" else "f32"


def held_to_the_bars(e, x0, P0, H, z, R, label, gate=C.INF):
    """observe_dense on e; its S, nu and d2 against NumPy on (x0, P0) under the derived bars; the state under check_state's."""
    ex, eP, want = C.update_dense(x0, P0, H, z, R, gate)
    got = e.observe_dense(H, z, R, gate=gate)
    assert (got["rows"], got["outcome"], got["bad_row"]) == (want["rows"], want["outcome"], want["bad_row"]), label
    rS, rnu, rd2 = C.bar_ratios(x0, P0, H, z, R, got)
    print("%s: worst error / bar: S %.3f nu %.3f d2 %.3f (cond S %.1f)" % (label, rS, rnu, rd2, np.linalg.cond(want["S"])))
    assert rS <= 1.0 and rnu <= 1.0 and rd2 <= 1.0, (label, rS, rnu, rd2)
    np.testing.assert_array_equal(got["S"], got["S"].T)
    return got, ex, eP


# ------------------------------------------------------------------------------------------------------------------
# 1. against NumPy on the twin's state
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage,n", STORES)
@pytest.mark.parametrize("k", C.KS)
def test_dense_gaussian_rows_against_numpy_on_the_twins_state(tile, storage, n, k):
    e, twin = sources(2, 3, n, tile=tile, storage=storage)
    assert e.pending() == min(3, n)
    x0, _, P0 = helpers.state(twin)                            # (flushes the twin)
    H, z, R = C.scene(x0, P0, C.gaussian_H(k, x0.size, 10 + k))
    label = "Gaussian k=%d N=%d T=%d %s" % (k, n, tile, storage)
    _, ex, eP = held_to_the_bars(e, x0, P0, H, z, R, label)
    assert e.pending() == 0 and e.N == n
    name, pairs = e.downdate_kernel_name()
    assert pairs == (k + 1) // 2 and name
    helpers.check_state(e, ex, eP, kind(storage), label + " (" + name + ")")
    e.close(); twin.close()


@pytest.mark.parametrize("tile,storage,n", [(16, "f64", 140), (128, "f64", 200), (256, "f32", 300)])
def test_sparse_rows_a_centroid_over_40_landmarks_and_displacements(tile, storage, n):
    for what in ("centroid", "displacements"):
        e, twin = sources(2, 3, n, tile=tile, storage=storage)
        x0, _, P0 = helpers.state(twin)
        rows = C.centroid_H(x0.size) if what == "centroid" else C.displacement_H(x0.size, C.spread_pairs(n, 3))
        H, z, R = C.scene(x0, P0, rows)
        label = "%s N=%d T=%d %s" % (what, n, tile, storage)
        _, ex, eP = held_to_the_bars(e, x0, P0, H, z, R, label)
        helpers.check_state(e, ex, eP, kind(storage), label)
        e.close(); twin.close()


@pytest.mark.parametrize("tile,storage", [(16, "f64"), (64, "f64"), (256, "f32")])
def test_after_removals_the_rows_left_behind_do_not_count(tile, storage):
    e, twin = sources(2, 3, 140, tile=tile, storage=storage)
    for q in (e, twin):
        q.remove_landmarks(range(110, 140))
        q.remove_landmarks(range(50, 60))
    assert e.N == 100
    x0, _, P0 = helpers.state(twin)
    H, z, R = C.scene(x0, P0, C.gaussian_H(5, x0.size, 4))
    label = "N=140 less 30 less 10, k=5, T=%d %s" % (tile, storage)
    _, ex, eP = held_to_the_bars(e, x0, P0, H, z, R, label)
    helpers.check_state(e, ex, eP, kind(storage), label)
    e.close(); twin.close()


def test_no_landmark_at_all_is_the_robot_part_alone():
    P0 = np.array([[0.5, 0.1, -0.05], [0.1, 0.4, 0.02], [-0.05, 0.02, 0.3]])
    x0 = np.array([1.0, -2.0, 40.0])
    for k in (1, 2, 3):
        g = engine(capacity=8, tile=16)
        g.set_x(x0); g.set_P(P0)
        H, z, R = C.scene(x0, P0, C.gaussian_H(k, 3, 20 + k))
        _, ex, eP = held_to_the_bars(g, x0, P0, H, z, R, "N=0 k=%d" % k)
        assert rel_err(g.get_x(), ex) < REL and rel_err(g.get_P(), eP) < REL
        np.testing.assert_array_equal(g.get_P(), g.get_P().T)
        g.close()


# ------------------------------------------------------------------------------------------------------------------
# 2. against the library's own existing routes
# ------------------------------------------------------------------------------------------------------------------
def test_a_landmark_fix_and_a_displacement_against_observe_linear():
    n, la, lb = 140, 37, 101
    for what in ("landmark fix", "two-landmark displacement"):
        a, b = sources(2, 3, n, tile=16)
        x0, _, P0 = helpers.state(b)
        nx = x0.size
        if what == "landmark fix":
            H = np.zeros((2, nx)); H[0, 3 + 2 * la] = H[1, 4 + 2 * la] = 1.0
            lms, Hl = [la], [np.eye(2)]
        else:
            H = C.displacement_H(nx, [(la, lb)])
            lms, Hl = [la, lb], [np.eye(2), -np.eye(2)]
        H, z, R = C.scene(x0, P0, H)
        a.observe_dense(H, z, R)
        b.observe_linear(z, R, np.zeros((2, 3)), lms, Hl)
        b.flush()
        (xa, _, Pa), (xb, _, Pb) = helpers.state(a), helpers.state(b)
        err_x, err_P = rel_err(xa, xb), rel_err(Pa, Pb)
        print("%s: observe_dense against observe_linear + flush: rel err x %.2e P %.2e" % (what, err_x, err_P))
        assert err_x < REL and err_P < REL
        a.close(); b.close()


def test_two_rows_jointly_against_one_after_the_other():
    a, b = sources(2, 3, 140, tile=16)
    x0, _, P0 = helpers.state(b)
    H, z, R = C.scene(x0, P0, C.gaussian_H(2, x0.size, 31))
    R = np.diag(np.diag(R))
    a.observe_dense(H, z, R)
    for i in (0, 1):
        b.observe_dense(H[i], z[i:i + 1], R[i, i])
    (xa, _, Pa), (xb, _, Pb) = helpers.state(a), helpers.state(b)
    err_x, err_P = rel_err(xa, xb), rel_err(Pa, Pb)
    print("two rows jointly against one after the other: rel err x %.2e P %.2e" % (err_x, err_P))
    assert err_x < REL and err_P < REL
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------------------------
# 3. bit for bit
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage", [(16, "f64"), (256, "f32")])
@pytest.mark.parametrize("k", [1, 3])
def test_an_odd_k_is_the_call_with_the_empty_row_written_out(tile, storage, k):
    a, b = sources(2, 3, 140, tile=tile, storage=storage)
    twin = sources(1, 3, 140, tile=tile, storage=storage)[0]
    x0, _, P0 = helpers.state(twin)
    H, z, R = C.scene(x0, P0, C.gaussian_H(k, x0.size, 40 + k))
    ra = a.observe_dense(H, z, R)
    rb = b.observe_dense(*C.padded(H, z, R))
    assert ra["d2"] == rb["d2"] and ra["rows"] == k and rb["rows"] == k + 1
    np.testing.assert_array_equal(ra["nu"], rb["nu"][:k])
    np.testing.assert_array_equal(ra["S"], rb["S"][:k, :k])
    assert rb["nu"][k] == 0.0 and rb["S"][k, k] == 1.0 and not rb["S"][k, :k].any()
    assert a.downdate_kernel_name() == b.downdate_kernel_name()
    assert_same(a, b)
    for q in (a, b, twin):
        q.close()


def test_dense_innovation_gated_and_irregular_leave_a_twin_that_only_flushed():
    from ekf_slam_amd import _lib as L
    e, twin, other = sources(3, 3, 140, tile=16)
    assert e.pending() == 3
    twin.flush()
    x0, _, P0 = helpers.state(twin)
    H, z, R = C.scene(x0, P0, C.gaussian_H(5, x0.size, 50))
    probe = e.dense_innovation(H, z, R)
    assert e.pending() == 0 and probe["outcome"] == C.APPLIED
    assert_same(e, twin)
    # a gated call
    got = e.observe_dense(H, z, R, gate=0.5 * probe["d2"])
    assert got["outcome"] == C.GATED and got["d2"] == probe["d2"]
    for key in ("nu", "S"):
        np.testing.assert_array_equal(got[key], probe[key])
    assert_same(e, twin)
    # the same landmark entry fixed by two identical rows with R = 0: S = [[p, p], [p, p]], whose second pivot p - (p / sqrt p)^2 is
    # not positive for the entry chosen here (observe_dense_cases.singular_pivot_is_not_positive: S(0, 0) is P(c, c) exactly)
    c = next(c for c in range(3, x0.size) if C.singular_pivot_is_not_positive(P0[c, c]))
    Hs = np.zeros((2, x0.size)); Hs[:, c] = 1.0
    zs = np.array([x0[c] + 0.1, x0[c] + 0.1])
    seen = e.dense_innovation(Hs, zs, np.zeros((2, 2)))
    assert (seen["outcome"], seen["bad_row"]) == (C.IRREGULAR, 1) and np.isnan(seen["d2"])
    np.testing.assert_array_equal(seen["S"], np.full((2, 2), P0[c, c]))
    st, msg = status_of(lambda: e.observe_dense(Hs, zs, np.zeros((2, 2))))
    assert st == L.EKF_ERR_STATE and "observe_dense" in msg and "row 1" in msg
    assert_same(e, twin)
    assert e.linear_rejections() == (0, 0)
    # the applied call reports what the innovation reported, and the handle goes on working
    applied = e.observe_dense(H, z, R)
    ref = other.observe_dense(H, z, R)
    for key in ("d2", "rows", "outcome", "bad_row"):
        assert applied[key] == probe[key] == ref[key], key
    for key in ("nu", "S"):
        np.testing.assert_array_equal(applied[key], probe[key])
    assert_same(e, other)
    x = lowrank_data(140, 5)[0]
    for q in (e, other):
        q.predict(U2); q.correct(observe(x, 9), R2, 9); q.flush()
    assert_same(e, other)
    for q in (e, twin, other):
        q.close()


def test_a_replayed_log_reproduces_the_bits(tmp_path):
    from ekf_slam_amd.slam import EKF_SLAM
    from ekf_slam_amd.trajectory import FORMAT_OBSERVE_DENSE, TrajectoryLog
    n = 60
    kw = dict(capacity=n + 4, tile=16, batch=8)
    f = EKF_SLAM(**kw)
    f._e.load_lowrank_state(*lowrank_data(n, 5))
    x0, _, P0 = helpers.state(f._e)
    f.log = TrajectoryLog()
    H, z, R = C.scene(x0, P0, C.gaussian_H(3, x0.size, 60))
    f.observe_dense(H, z, R)
    f.fix_centroid(list(range(5, 45)), [0.3, -0.2] + C.centroid_H(x0.size, 40, 5) @ f._e.get_x(), 0.05 * np.eye(2), p=0.999)
    f.constrain_displacements([(1, 50), (20, 7)], [0.5, 0.5, -1.0, 2.0], 0.2 * np.eye(2))
    assert [ed[1] for ed in f.log.edits] == ["observe_dense"] * 3
    f.predict(U2)
    f.log.record(U2, None, [], [])
    path = tmp_path / "dense.npz"
    f.log.save(path)
    assert str(np.load(path)["format"]) == FORMAT_OBSERVE_DENSE == "ekfslam-trajectory-13"
    log = TrajectoryLog.load(path)
    fresh = helpers.engine(**kw)
    fresh.load_lowrank_state(*lowrank_data(n, 5))
    log.replay(fresh)
    assert_same(fresh, f._e)
    f._e.close(); fresh.close()


# ------------------------------------------------------------------------------------------------------------------
# 4. conditioning
# ------------------------------------------------------------------------------------------------------------------
def test_conditioning_on_a_landmark():
    from ekf_slam_amd.slam import EKF_SLAM
    n, j = 40, 17
    f = EKF_SLAM(capacity=n + 4, tile=16)
    f._e.load_lowrank_state(*lowrank_data(n, 5))
    x0, _, P0 = helpers.state(f._e)
    others = [i for i in range(n) if i != j]
    before = f.conditional_covariance(others)                  # given the robot and landmark j ...
    v = x0[3 + 2 * j:5 + 2 * j] + np.array([0.05, -0.02])
    res = f.condition_on([j], v)
    assert res["outcome"] == C.APPLIED and f._e.pending() == 0
    x1, _, P1 = helpers.state(f._e)
    np.testing.assert_array_equal(P1, P1.T)
    scale = np.abs(P0).max()
    err_x = np.abs(x1[3 + 2 * j:5 + 2 * j] - v).max() / np.abs(x0).max()
    err_row = np.abs(P1[3 + 2 * j:5 + 2 * j, :]).max() / scale
    print("condition_on: x_j against v %.2e of |x|, row j of P %.2e of |P|" % (err_x, err_row))
    assert err_x < REL and err_row < REL
    info = f.factor_map()
    assert not info["definite"] and info["bad_index"] in (3 + 2 * j, 4 + 2 * j)
    # ... the robot is still uncertain after the call, so the others' block of P is their covariance given landmark j ALONE; given the
    # robot too it is the Schur complement of that block on the robot, which is what `before` is
    co = np.array([3 + 2 * i + r for i in others for r in (0, 1)])
    Poo, Por, Prr = P1[np.ix_(co, co)], P1[np.ix_(co, np.arange(3))], P1[:3, :3]
    after = Poo - Por @ np.linalg.solve(Prr, Por.T)
    err = np.abs(after - before).max() / np.abs(before).max()
    print("conditional covariance before against the block after: %.2e of the bar %.2e" % (err, V.bar(P0)))
    assert err <= V.bar(P0)
    f._e.close()


# ------------------------------------------------------------------------------------------------------------------
# 5. behind an asynchronous pass
# ------------------------------------------------------------------------------------------------------------------
def test_behind_an_asynchronous_pass_just_queued():
    n = 140
    x = lowrank_data(n, 5)[0]
    runs = []
    for asy in (True, False):
        e = loaded(n, 5, capacity=n + 4, tile=16, batch=3, async_flush=asy)
        for k in (5, 60, 100):                                # the batch completes: its pass is queued (asynchronous: on the pass stream)
            e.predict(U2); e.correct(observe(x, k), R2, k)
        e.predict(U2); e.correct(observe(x, 7), R2, 7)        # and one pair recorded behind it
        H = C.gaussian_H(4, 3 + 2 * n, 70)
        runs.append((e, e.observe_dense(H, H @ x + 0.1, 0.5 * np.eye(4))))
        assert e.pending() == 0
    for key in ("d2", "nu", "S"):
        np.testing.assert_array_equal(runs[0][1][key], runs[1][1][key])
    assert_same(runs[0][0], runs[1][0])
    for e, _ in runs:
        e.close()


# ------------------------------------------------------------------------------------------------------------------
# 6. refusals, each with the handle as it was and nothing flushed
# ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_alone():
    from ekf_slam_amd import _lib as L
    n = 20
    e, twin = sources(2, 3, n, tile=16, batch=8)
    assert e.pending() == 3
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    nx = 3 + 2 * n
    H, z, R = np.zeros((2, nx)), np.zeros(2), np.eye(2)
    H[0, 4] = H[1, 9] = 1.0
    res = L.EkfObserveDenseResult()

    def call(h, H, k, z, R, gate=np.inf, res=res):
        ptr = lambda a: None if a is None else a.ctypes.data_as(dp)
        return e.lib.ekf_observe_dense(h, ptr(H), ctypes.c_int64(k), ptr(z), ptr(R), ctypes.cast(None, ip), ctypes.c_double(gate),
                                       None if res is None else ctypes.byref(res), None, None)

    def but(a, at, v):
        b = a.copy(); b[at] = v
        return b

    bad = L.EKF_ERR_INVALID_ARG
    assert call(None, H, 2, z, R) == bad
    cases = [("a null H", (None, 2, z, R), b"null"), ("a null z", (H, 2, None, R), b"null"), ("a null R", (H, 2, z, None), b"null"),
             ("k = 0", (H, 0, z, R), b"EKF_DENSE_MAX"), ("k = 17", (H, 17, z, R), b"EKF_DENSE_MAX"),
             ("z not finite", (H, 2, but(z, 1, np.nan), R), b"z is not finite"), ("R not finite", (H, 2, z, but(R, (0, 1), np.inf)), b"R is not finite"),
             ("R not symmetric", (H, 2, z, but(R, (0, 1), 1e-3)), b"not symmetric"), ("a negative diagonal", (H, 2, z, but(R, (1, 1), -1.0)), b"negative diagonal"),
             ("H not finite", (but(H, (1, 7), np.inf), 2, z, R), b"H is not finite")]
    for name, args, word in cases:
        assert call(e.h, *args) == bad, name
        msg = e.lib.ekf_last_error(e.h)
        assert b"observe_dense" in msg and word in msg, (name, msg)
        assert e.pending() == 3, name
    assert call(e.h, H, 2, z, R, res=None) == bad and call(e.h, H, 2, z, R, gate=np.nan) == bad and e.pending() == 3
    # the order: k before z before R before the gate before H
    assert call(e.h, but(H, (0, 0), np.nan), 0, but(z, 0, np.nan), R) == bad and b"EKF_DENSE_MAX" in e.lib.ekf_last_error(e.h)
    assert call(e.h, but(H, (0, 0), np.nan), 2, but(z, 0, np.nan), -R) == bad and b"z is not finite" in e.lib.ekf_last_error(e.h)
    assert call(e.h, but(H, (0, 0), np.nan), 2, z, -R, gate=np.nan) == bad and b"negative diagonal" in e.lib.ekf_last_error(e.h)
    assert call(e.h, but(H, (0, 0), np.nan), 2, z, R, gate=np.nan) == bad and b"gate" in e.lib.ekf_last_error(e.h)
    # a sharded handle refuses, the arguments first; a lone cfg.force_sharded shard equals the unsharded bits
    sh = helpers.engine(capacity=64, tile=16, world=2, rank=0)
    st, msg = status_of(lambda: sh.observe_dense(np.ones((1, 3)), [0.0], [1.0]))
    assert st == bad and "shard" in msg and "observe_dense" in msg
    sh.close()
    kw = dict(capacity=n + 4, tile=16)
    lone, plain = helpers.loaded(n, 5, force_sharded=1, **kw), helpers.loaded(n, 5, **kw)
    Hg = C.gaussian_H(3, nx, 80)
    ra, rb = lone.observe_dense(Hg, np.ones(3), np.eye(3)), plain.observe_dense(Hg, np.ones(3), np.eye(3))
    for key in ("d2", "nu", "S"):
        np.testing.assert_array_equal(ra[key], rb[key])
    assert_same(lone, plain)
    lone.close(); plain.close()
    # nothing was changed and nothing flushed: the handle is bit for bit its twin
    assert e.pending() == 3
    for got, ref in zip(getters(e), getters(twin)):
        np.testing.assert_array_equal(got, ref)
    e.close(); twin.close()
