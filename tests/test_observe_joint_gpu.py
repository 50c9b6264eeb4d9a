"""GPU: a scan's pairings applied as ONE joint update (ekf_observe_model_joint; include/ekfslam.h) and
measure_model_joint(joint_update=True) on top of it.

The yardstick is the NumPy restatement of tests/observe_joint_cases.py applied to THE STATE THE ENGINE REPORTS before the call, under the
project's own bars (helpers.check_state).  Where the contract is equality -- the record, nu and S against ekf_joint_innovation, pending
work before the call against none, a gated or irregular call against a flush, a lone shard against its unsharded twin, a replayed log --
the comparison is assert_array_equal.  N = 150 throughout: 19 tile rows of edge 16 and two column workgroups of the gather."""
import numpy as np
import pytest

import helpers
import joint_cases as J
import model_obs_cases as M
import observe_joint_cases as C
from helpers import R2, REL, STORES_ALL, U2, assert_same, rel_err, status_of
from removal_cases import lowrank_data, observe

pytestmark = pytest.mark.gpu
N = J.N0
RECORD = ("d2", "dof", "pairings", "outcome", "first_irregular")


def loaded(corrections=0, **kw):
    """lowrank_data(150, 5), with `corrections` predict-and-correct steps behind it."""
    kw = dict(dict(capacity=N + 8, tile=16, batch=8), **kw)
    e = helpers.loaded(N, 5, **kw)
    x = lowrank_data(N, 5)[0]
    for k in (5, 16, N - 3, 11, 40, 77, 2, 120, 63, 64, 100)[:corrections]:
        e.predict(U2); e.correct(observe(x, k), R2, k)
    return e


def joint(e, ents, lms, gate=C.INF):
    return e.observe_model_joint(ents, lms, gate=gate, want_nu=True, want_S=True)


def _set_x(e, x):
    from ekf_slam_amd.engine import _p
    x = np.ascontiguousarray(x, dtype=np.float64)
    e._check(e.lib.ekf_set_x(e.h, _p(x), x.size))


def assert_record(got, want, msg=""):
    assert (got["dof"], got["pairings"], got["outcome"], got["first_irregular"]) == \
           (want["dof"], want["pairings"], want["outcome"], want["first_irregular"]), msg
    np.testing.assert_allclose(got["d2"], want["d2"], rtol=1e-9, err_msg=msg)


# ------------------------------------------------------------------------------------------------------------------
# 1. against the restatement
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage", STORES_ALL)
@pytest.mark.parametrize("npair", C.NPS)
def test_joint_update_against_the_restatement(tile, storage, npair):
    e = loaded(0, tile=tile, storage=storage)
    x0, _, P0 = helpers.state(e)
    ents, lms = C.scan_of(x0, npair)
    ex, eP, want = C.joint_update_dense(x0, P0, ents, lms)
    got = joint(e, ents, lms)
    assert_record(got, want)
    np.testing.assert_allclose(got["nu"], want["nu"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(got["S"], want["S"], rtol=1e-9, atol=1e-14)
    assert e.pending() == 0
    name, pairs = e.downdate_kernel_name()
    assert pairs == npair and name
    helpers.check_state(e, ex, eP, "f64" if storage == "f64" else "f32", "joint update, np = %d, T = %d (%s)" % (npair, tile, name))
    e.close()


# ------------------------------------------------------------------------------------------------------------------
# 2. against joint_innovation, bit for bit
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage", STORES_ALL)
@pytest.mark.parametrize("npair", C.NPS)
def test_record_nu_and_S_are_joint_innovations(tile, storage, npair):
    e = loaded(3, tile=tile, storage=storage)
    ents, lms = C.scan_of(lowrank_data(N, 5)[0], npair)
    if npair < 32:
        ents, lms = ents[:1] + [ents[0]] + ents[1:], lms[:1] + [-1] + lms[1:]      # one entry left out, in the middle of the scan
    e.flush()
    ref = e.joint_innovation(ents, [lms], want_prefix=False, want_nu=True, want_S=True)
    got = joint(e, ents, lms)
    for key in RECORD + ("nu", "S"):
        np.testing.assert_array_equal(got[key], ref[key][0], err_msg=key)
    assert got["outcome"] == C.APPLIED and got["pairings"] == npair
    e.close()


# ------------------------------------------------------------------------------------------------------------------
# 3. pending work before the call
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("async_flush", [False, True])
@pytest.mark.parametrize("npair", C.NPS)
def test_pending_corrections_and_a_recorded_predict_in_front(npair, async_flush):
    a, b = loaded(5, batch=32, async_flush=async_flush), loaded(5, batch=1)
    assert a.pending() == 5 and b.pending() == 0
    ents, lms = C.scan_of(lowrank_data(N, 5)[0], npair)
    a.predict(U2); b.predict(U2)
    ra, rb = joint(a, ents, lms), joint(b, ents, lms)
    for key in RECORD + ("nu", "S"):
        np.testing.assert_array_equal(ra[key], rb[key], err_msg=key)
    assert a.pending() == 0 and b.pending() == 0
    assert a.downdate_kernel_name()[1] == npair and b.downdate_kernel_name()[1] == npair
    assert_same(a, b)
    a.close(); b.close()


def test_a_pass_in_flight_is_retired_first():
    a, b = loaded(6, batch=4, async_flush=True), loaded(6, batch=1)
    assert a.pending() >= 2                                     # two pairs recorded behind the asynchronous pass of the first four
    ents, lms = C.scan_of(lowrank_data(N, 5)[0], 8)
    ra, rb = joint(a, ents, lms), joint(b, ents, lms)
    for key in RECORD + ("nu", "S"):
        np.testing.assert_array_equal(ra[key], rb[key], err_msg=key)
    assert a.pending() == 0 and a.downdate_kernel_name()[1] == 8
    assert_same(a, b)
    # ... and the handle goes on as an asynchronous one: four more corrections start the next pass
    x = lowrank_data(N, 5)[0]
    for q in (a, b):
        for k in (9, 33, 71, 140):
            q.predict(U2); q.correct(observe(x, k), R2, k)
    assert_same(a, b)
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------------------------
# 4. against the device's own sequence of linear observations
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npair", C.NPS)
def test_joint_update_against_the_frozen_sequence_on_the_device(npair):
    a, b = loaded(0), loaded(0)
    x0, _, P0 = helpers.state(a)
    ents, lms = C.scan_of(x0, npair)
    joint(a, ents, lms)
    for Hk, zk, Rk, lm in C.frozen_steps(x0, P0, ents, lms):
        b.observe_linear(zk, Rk, Hk[:, :3], [lm], [Hk[:, 3 + 2 * lm:5 + 2 * lm]])
    (xa, _, Pa), (xb, _, Pb) = helpers.state(a), helpers.state(b)
    err_x, err_P = rel_err(xa, xb), rel_err(Pa, Pb)
    print("np = %d: joint update against %d linear observations on the device: rel err x %.2e P %.2e" % (npair, npair, err_x, err_P))
    assert err_x < REL and err_P < REL
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------------------------
# 5. gated and irregular: nothing changes beyond the flush
# ------------------------------------------------------------------------------------------------------------------
def test_gated_and_irregular_change_nothing_beyond_the_flush():
    from ekf_slam_amd import _lib as L
    e, twin = loaded(3), loaded(3)
    assert e.pending() == 3
    ents, lms = C.scan_of(lowrank_data(N, 5)[0], 8)
    twin.flush()
    d2 = twin.joint_innovation(ents, [lms])["d2"][0]
    got = joint(e, ents, lms, gate=0.5 * d2)
    assert got["outcome"] == C.GATED and got["d2"] == d2 and e.pending() == 0
    for u, v in zip(helpers.getters(e), helpers.getters(twin)):
        np.testing.assert_array_equal(u, v)
    # landmark lms[2] on the robot: the third pairing has no d2
    for q in (e, twin):
        x = q.get_x()
        x[3 + 2 * lms[2]:5 + 2 * lms[2]] = x[:2]
        _set_x(q, x)
    st, msg = status_of(lambda: joint(e, ents, lms))
    assert st == L.EKF_ERR_STATE and "observe_model_joint" in msg and "observation 2" in msg
    for u, v in zip(helpers.getters(e), helpers.getters(twin)):
        np.testing.assert_array_equal(u, v)
    assert e.linear_rejections() == (0, 0)
    # the handle goes on working
    for q in (e, twin):
        res = q.observe_model(ents[0]["model"], ents[0]["z"], ents[0]["R"], [lms[0]], wait=True)
        assert res["outcome"] == M.APPLIED
    got = joint(e, ents[:2], lms[:2])
    assert got["outcome"] == C.APPLIED and e.pending() == 0
    e.close(); twin.close()


def test_no_pairing_is_the_empty_update():
    e, twin = loaded(3), loaded(3)
    ents, _ = C.scan_of(lowrank_data(N, 5)[0], 3)
    got = joint(e, ents, [-1, -1, -1])
    assert (got["d2"], got["dof"], got["pairings"], got["outcome"], got["first_irregular"]) == (0.0, 0, 0, C.APPLIED, -1)
    np.testing.assert_array_equal(got["S"], np.eye(6))
    assert not got["nu"].any() and e.pending() == 3           # no flush
    assert_same(e, twin)
    e.close(); twin.close()


# ------------------------------------------------------------------------------------------------------------------
# 6. sharding
# ------------------------------------------------------------------------------------------------------------------
def test_sharded_handles_are_refused_and_a_lone_shard_equals_the_unsharded_bits():
    from ekf_slam_amd import _lib as L
    x = lowrank_data(N, 5)[0]
    ents, lms = C.scan_of(x, 8)
    sh = helpers.engine(capacity=64, tile=16, world=2, rank=0)
    st, msg = status_of(lambda: sh.observe_model_joint(ents[:3], [1, 2, 3]))
    assert st == L.EKF_ERR_INVALID_ARG and "shard" in msg
    st, msg = status_of(lambda: sh.observe_model_joint(ents[:3], [1, 2, 1]))
    assert st == L.EKF_ERR_INVALID_ARG and "shard" not in msg           # the arguments come first
    sh.close()
    kw = dict(capacity=N + 8, tile=16)
    e, twin = helpers.loaded(N, 5, force_sharded=1, **kw), helpers.loaded(N, 5, **kw)
    ra, rb = joint(e, ents, lms), joint(twin, ents, lms)
    for key in RECORD + ("nu", "S"):
        np.testing.assert_array_equal(ra[key], rb[key], err_msg=key)
    assert_same(e, twin)
    e.close(); twin.close()


def test_refusals_in_their_order():
    from ekf_slam_amd import _lib as L
    e = loaded(3)
    ents, lms = C.scan_of(lowrank_data(N, 5)[0], 3)
    bad = L.EKF_ERR_INVALID_ARG
    assert status_of(lambda: joint(e, ents, [3, 10, 3]))[0] == bad
    assert status_of(lambda: joint(e, ents, [3, -2, 17]))[0] == bad
    assert status_of(lambda: joint(e, ents, lms, gate=float("nan")))[0] == bad
    assert status_of(lambda: joint(e, ents, [3, N, 3]))[0] == bad                  # the arguments before the index
    assert status_of(lambda: joint(e, ents, [3, 10, N]))[0] == L.EKF_ERR_INDEX
    assert e.pending() == 3                                                         # refused before the flush
    e.close()


# ------------------------------------------------------------------------------------------------------------------
# 7. the policy
# ------------------------------------------------------------------------------------------------------------------
def test_measure_model_joint_with_one_joint_update_and_its_replay(tmp_path):
    from ekf_slam_amd.slam import EKF_SLAM
    from ekf_slam_amd.trajectory import FORMAT_JOINT, TrajectoryLog
    J.assert_scene_premises()
    x, s, d, U, scan = J.ambiguous_scene()
    kw = dict(capacity=N + 8, tile=16, batch=8)
    f = EKF_SLAM(**kw)
    f._e.load_lowrank_state(x, s, d, U)
    x0, _, P0 = helpers.state(f._e)
    f.log = TrajectoryLog()
    out, truncated = f.measure_model_joint(scan, J.GATE, 25.0, joint_update=True)
    assert out == [("matched", J.LM_A + 1), ("matched", J.LM_B + 1)] and truncated is False and f._e.pending() == 0
    assert [ed[1] for ed in f.log.edits] == ["observe_model_joint"]
    ex, eP, want = C.joint_update_dense(x0, P0, J.scene_entries(scan), [J.LM_A, J.LM_B])
    assert want["outcome"] == C.APPLIED
    helpers.check_state(f._e, ex, eP, "f64", "measure_model_joint(joint_update=True)")
    f.predict(U2)
    f.log.record(U2, None, [], [])                            # (what measure() records of a step without sightings: the edits replay in front of it)
    path = tmp_path / "joint_update.npz"
    f.log.save(path)
    assert str(np.load(path)["format"]) == FORMAT_JOINT
    log = TrajectoryLog.load(path)
    assert [ed[1] for ed in log.edits] == ["observe_model_joint"] and len(log) == 1
    fresh = helpers.engine(**kw)
    fresh.load_lowrank_state(x, s, d, U)
    log.replay(fresh)
    assert_same(fresh, f._e)
    f._e.close(); fresh.close()
