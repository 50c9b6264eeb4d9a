"""GPU: a scan's pairings applied as ONE joint update, RELINEARISED (ekf_observe_model_joint_iterated; include/ekfslam.h, DESIGN.md
section 3r) and measure_model_joint(joint_update=True, joint_iterations=3) on top of it.

The yardstick is the NumPy restatement of tests/observe_joint_iter_cases.py applied to THE STATE THE ENGINE REPORTS before the call, under
the project's own bars (helpers.check_state).  Where the contract is equality -- one linearisation against ekf_observe_model_joint, the
record, nu and S against ekf_joint_innovation, pending work before the call against none, a gated or irregular call against a flush, a
lone shard against its unsharded twin, a replayed log -- the comparison is assert_array_equal.  N = 150 throughout: 19 tile rows of edge
16 and two column workgroups of the gather."""
import ctypes

import numpy as np
import pytest

import helpers
import joint_cases as J
import observe_joint_cases as C
import observe_joint_iter_cases as I
from helpers import R2, STORES_ALL, U2, assert_same, status_of
from removal_cases import observe

pytestmark = pytest.mark.gpu
N = J.N0
RECORD = ("d2", "dof", "pairings", "outcome", "first_irregular")
KW = dict(capacity=N + 8, tile=16, batch=8)


def wide(npair, offset=1.0, corrections=0, **kw):
    """(engine loaded with the wide-prior scene, entries, landmarks), with `corrections` predict-and-correct steps on landmarks outside
    the scan behind it."""
    x, s, d, U, ents, lms = I.wide_scene(npair, N, offset)
    e = helpers.engine(**dict(KW, **kw))
    e.load_lowrank_state(x, s, d, U)
    for k in [q for q in (5, 16, N - 3, 11, 40, 77, 2, 120, 63, 64, 100) if q not in lms][:corrections]:
        e.predict(U2); e.correct(observe(x, k), R2, k)
    return e, ents, lms


def iterated(e, ents, lms, iterations, tol=0.0, gate=C.INF):
    """ekf_observe_model_joint_iterated itself, whatever `iterations` is (Engine.observe_model_joint sends iterations = 1 to the old
    symbol): joint_result's dict with nu and S, and the iteration record under 'it'."""
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import marshal
    from ekf_slam_amd.engine import _p
    arr, m = marshal.scan_obs(ents)
    idx, _ = marshal.index_array([float(k) for k in lms])
    res, it = L.EkfJointResult(), L.EkfJointIterResult()
    nu, S = np.zeros(2 * m), np.zeros(4 * m * m)
    e._check(e.lib.ekf_observe_model_joint_iterated(e.h, arr, m, idx, float(gate), int(iterations), float(tol), ctypes.byref(res), ctypes.byref(it),
                                                    _p(nu), _p(S)))
    out = marshal.joint_result(res, m, nu, S)
    out["it"] = marshal.joint_iter_result(it)
    return out


# ------------------------------------------------------------------------------------------------------------------
# 1. one linearisation is ekf_observe_model_joint, bit for bit
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage", STORES_ALL)
@pytest.mark.parametrize("npair", I.NPS)
def test_one_linearisation_is_the_joint_update_bit_for_bit(tile, storage, npair):
    a, ents, lms = wide(npair, tile=tile, storage=storage)
    b, _, _ = wide(npair, tile=tile, storage=storage)
    ra = iterated(a, ents, lms, 1)
    rb = b.observe_model_joint(ents, lms, want_nu=True, want_S=True)
    for key in RECORD + ("nu", "S"):
        np.testing.assert_array_equal(ra[key], rb[key], err_msg=key)
    assert ra["it"]["used"] == 1 and ra["it"]["irregular_at"] == -1 and ra["outcome"] == C.APPLIED
    assert a.downdate_kernel_name()[1] == npair == b.downdate_kernel_name()[1] and a.pending() == 0
    assert_same(a, b)
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------------------------
# 2. against the restatement
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage", STORES_ALL)
@pytest.mark.parametrize("npair", I.NPS)
def test_iterated_update_against_the_restatement(tile, storage, npair):
    for n in (3, 8):
        e, ents, lms = wide(npair, tile=tile, storage=storage)
        x0, _, P0 = helpers.state(e)
        ex, eP, want, wit = I.joint_update_iterated_dense(x0, P0, ents, lms, n)
        got = iterated(e, ents, lms, n)
        assert want["outcome"] == C.APPLIED == got["outcome"] and got["pairings"] == npair
        np.testing.assert_allclose(got["d2"], want["d2"], rtol=1e-9)
        assert got["it"]["used"] == wit["used"] == n and got["it"]["irregular_at"] == -1
        np.testing.assert_allclose(got["it"]["step"], wit["step"], rtol=1e-4, atol=1e-12)
        np.testing.assert_allclose(got["it"]["x_sub"], wit["x_sub"], rtol=1e-9, atol=1e-9)
        assert e.pending() == 0 and e.downdate_kernel_name()[1] == npair
        helpers.check_state(e, ex, eP, "f64" if storage == "f64" else "f32", "iterated joint update, np = %d, %d linearisations, T = %d" % (npair, n, tile))
        e.close()


@pytest.mark.parametrize("npair", I.NPS)
def test_the_loop_stops_at_tol_where_the_restatement_does(npair):
    e, ents, lms = wide(npair, offset=I.NEAR)
    x0, _, P0 = helpers.state(e)
    steps = I.joint_update_iterated_dense(x0, P0, ents, lms, I.ITER_MAX)[3]["steps"]
    tol, used = I.pick_tol(steps)
    assert steps[used - 2] >= 10.0 * tol and tol >= 10.0 * steps[used - 1]
    ex, eP, want, wit = I.joint_update_iterated_dense(x0, P0, ents, lms, I.ITER_MAX, tol)
    got = e.observe_model_joint(ents, lms, iterations=I.ITER_MAX, tol=tol)         # through the Python layer: the three added keys
    assert (got["used"], got["converged"]) == (wit["used"], wit["converged"]) == (used, True)
    helpers.check_state(e, ex, eP, "f64", "iterated joint update, np = %d, tol = %.3g: %d linearisations" % (npair, tol, used))
    e.close()


# ------------------------------------------------------------------------------------------------------------------
# 3. the first linearisation's record, nu and S are joint_innovation's, bit for bit
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 8])
@pytest.mark.parametrize("npair", I.NPS)
def test_record_nu_and_S_are_joint_innovations(npair, n):
    e, ents, lms = wide(npair, corrections=3)
    if npair < 32:
        ents, lms = ents[:1] + [ents[0]] + ents[1:], lms[:1] + [-1] + lms[1:]      # one entry left out, in the middle of the scan
    e.flush()
    ref = e.joint_innovation(ents, [lms], want_prefix=False, want_nu=True, want_S=True)
    got = iterated(e, ents, lms, n)
    for key in RECORD + ("nu", "S"):
        np.testing.assert_array_equal(got[key], ref[key][0], err_msg=key)
    assert got["outcome"] == C.APPLIED and got["pairings"] == npair and got["it"]["used"] == n
    e.close()


# ------------------------------------------------------------------------------------------------------------------
# 4. gated at the first linearisation, irregular at a later one: nothing changes beyond the flush
# ------------------------------------------------------------------------------------------------------------------
def test_gated_and_irregular_later_change_nothing_beyond_the_flush():
    from ekf_slam_amd import _lib as L
    e, ents, lms = wide(5, corrections=3)
    twin, _, _ = wide(5, corrections=3)
    assert e.pending() == 3
    twin.flush()
    d2 = twin.joint_innovation(ents, [lms])["d2"][0]
    got = iterated(e, ents, lms, 3, gate=0.5 * d2)
    assert got["outcome"] == C.GATED and got["d2"] == d2 and got["it"]["used"] == 0 and e.pending() == 0
    for u, v in zip(helpers.getters(e), helpers.getters(twin)):
        np.testing.assert_array_equal(u, v)
    # a range of 1e200: regular at the first linearisation, not posed at the second
    far = [dict(ents[0], z=np.array([1e200, ents[0]["z"][1]]))] + ents[1:]
    assert twin.joint_innovation(far, [lms])["outcome"][0] == J.REGULAR
    st, msg = status_of(lambda: iterated(e, far, lms, 3))
    assert st == L.EKF_ERR_STATE and "observe_model_joint_iterated" in msg and "observation 0" in msg and "linearisation 1" in msg
    for u, v in zip(helpers.getters(e), helpers.getters(twin)):
        np.testing.assert_array_equal(u, v)
    assert e.linear_rejections() == (0, 0)
    # the handle goes on working: a regular scan, relinearised, on both
    ra, rb = iterated(e, ents, lms, 3), iterated(twin, ents, lms, 3)
    assert ra["outcome"] == C.APPLIED and ra["it"]["used"] == 3 and e.pending() == 0
    for key in RECORD + ("nu", "S"):
        np.testing.assert_array_equal(ra[key], rb[key], err_msg=key)
    assert_same(e, twin)
    e.close(); twin.close()


def test_refusals_in_their_order_and_the_empty_update():
    from ekf_slam_amd import _lib as L
    e, ents, lms = wide(5, corrections=3)
    bad = L.EKF_ERR_INVALID_ARG
    assert status_of(lambda: iterated(e, ents, [lms[0]] * 2 + lms[2:], 3))[0] == bad
    assert status_of(lambda: iterated(e, ents, lms, 3, gate=float("nan")))[0] == bad
    for n, tol in ((0, 0.0), (17, 0.0), (3, -1.0), (3, float("nan"))):
        st, msg = status_of(lambda: iterated(e, ents, lms, n, tol))
        assert st == bad and ("iterations" in msg or "tol" in msg)
    assert status_of(lambda: iterated(e, ents, lms[:4] + [N], 0))[0] == bad        # the controls before the index
    assert status_of(lambda: iterated(e, ents, lms[:4] + [N], 3))[0] == L.EKF_ERR_INDEX
    assert e.pending() == 3                                                         # refused before the flush
    got = iterated(e, ents, [-1] * 5, 3)
    assert (got["d2"], got["pairings"], got["outcome"]) == (0.0, 0, C.APPLIED) and (got["it"]["used"], got["it"]["converged"]) == (0, True)
    assert e.pending() == 3
    e.close()


# ------------------------------------------------------------------------------------------------------------------
# 5. pending work before the call
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("async_flush", [False, True])
@pytest.mark.parametrize("npair", I.NPS)
def test_pending_corrections_and_a_recorded_predict_in_front(npair, async_flush):
    a, ents, lms = wide(npair, corrections=5, batch=32, async_flush=async_flush)
    b, _, _ = wide(npair, corrections=5, batch=1)
    assert a.pending() == 5 and b.pending() == 0
    a.predict(U2); b.predict(U2)
    ra, rb = iterated(a, ents, lms, 3), iterated(b, ents, lms, 3)
    for key in RECORD + ("nu", "S"):
        np.testing.assert_array_equal(ra[key], rb[key], err_msg=key)
    assert ra["it"]["used"] == rb["it"]["used"] == 3 and ra["it"]["step"] == rb["it"]["step"]
    assert a.pending() == 0 and b.pending() == 0
    assert_same(a, b)
    a.close(); b.close()


def test_a_pass_in_flight_is_retired_first():
    a, ents, lms = wide(5, corrections=6, batch=4, async_flush=True)
    b, _, _ = wide(5, corrections=6, batch=1)
    assert a.pending() >= 2                                     # two pairs recorded behind the asynchronous pass of the first four
    ra, rb = iterated(a, ents, lms, 3), iterated(b, ents, lms, 3)
    for key in RECORD + ("nu", "S"):
        np.testing.assert_array_equal(ra[key], rb[key], err_msg=key)
    assert a.pending() == 0 and a.downdate_kernel_name()[1] == 5
    assert_same(a, b)
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------------------------
# 6. a lone shard; a replayed log; the policy
# ------------------------------------------------------------------------------------------------------------------
def test_a_lone_shard_equals_the_unsharded_bits():
    a, ents, lms = wide(5, force_sharded=1)
    b, _, _ = wide(5)
    ra, rb = iterated(a, ents, lms, 3), iterated(b, ents, lms, 3)
    for key in RECORD + ("nu", "S"):
        np.testing.assert_array_equal(ra[key], rb[key], err_msg=key)
    assert_same(a, b)
    a.close(); b.close()


def test_a_replayed_log_reproduces_the_run(tmp_path):
    from ekf_slam_amd.slam import EKF_SLAM
    from ekf_slam_amd.trajectory import FORMAT_JOINT_ITERATED, TrajectoryLog
    x, s, d, U, ents, lms = I.wide_scene(5, N)
    f = EKF_SLAM(**KW)
    f._e.load_lowrank_state(x, s, d, U)
    f.log = TrajectoryLog()
    got = f.observe_model_joint(ents, [k + 1 for k in lms], iterations=3, tol=1e-12)
    assert got["outcome"] == C.APPLIED and got["used"] == 3 and got["first_irregular"] == 0
    f.predict(U2)
    f.log.record(U2, None, [], [])
    path = tmp_path / "iterated.npz"
    f.log.save(path)
    assert str(np.load(path)["format"]) == FORMAT_JOINT_ITERATED
    log = TrajectoryLog.load(path)
    assert [ed[1] for ed in log.edits] == ["observe_model_joint_iterated"]
    fresh = helpers.engine(**KW)
    fresh.load_lowrank_state(x, s, d, U)
    log.replay(fresh)
    assert_same(fresh, f._e)
    f._e.close(); fresh.close()


def test_measure_model_joint_with_one_iterated_joint_update():
    from ekf_slam_amd.slam import EKF_SLAM
    from ekf_slam_amd.trajectory import TrajectoryLog
    J.assert_scene_premises()
    x, s, d, U, scan = J.ambiguous_scene()
    f = EKF_SLAM(**KW)
    f._e.load_lowrank_state(x, s, d, U)
    x0, _, P0 = helpers.state(f._e)
    f.log = TrajectoryLog()
    out, truncated = f.measure_model_joint(scan, J.GATE, 25.0, joint_update=True, joint_iterations=3)
    assert out == [("matched", J.LM_A + 1), ("matched", J.LM_B + 1)] and truncated is False and f._e.pending() == 0
    assert [ed[1] for ed in f.log.edits] == ["observe_model_joint_iterated"]
    ex, eP, want, wit = I.joint_update_iterated_dense(x0, P0, J.scene_entries(scan), [J.LM_A, J.LM_B], 3)
    assert want["outcome"] == C.APPLIED
    helpers.check_state(f._e, ex, eP, "f64", "measure_model_joint(joint_update=True, joint_iterations=3)")
    f._e.close()
