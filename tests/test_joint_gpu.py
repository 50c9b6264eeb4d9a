"""GPU: the joint compatibility of a scan's pairings (ekf_joint_innovation; include/ekfslam.h) and the
joint-compatibility policy on top of it (measure_model_joint of ekf_slam_amd/slam.py).

The yardstick is the NumPy restatement of tests/joint_cases.py applied to THE STATE THE ENGINE REPORTS.  Where the contract is equality --
a pairing's block against ekf_model_innovation's, a prefix against the hypothesis cut there, entries left out against the shorter scan,
one call of many hypotheses against many calls of one, before a flush against after it, a lone shard against its unsharded twin, a
replayed log -- the comparison is assert_array_equal.  N = 150 throughout: 19 tile rows of edge 16, one tile of edge 256."""
import ctypes

import numpy as np
import pytest

import associate_model_cases as A
import helpers
import joint_cases as J
import model_obs_cases as M
from helpers import R2, RPOS, U2, assert_same, status_of
from removal_cases import lowrank_data, observe

pytestmark = pytest.mark.gpu
N = J.N0
KEYS = ("d2", "dof", "pairings", "outcome", "first_irregular", "d2_prefix", "nu", "S")


def loaded(corrections=0, **kw):
    """lowrank_data(150, 5) with `corrections` predict-and-correct steps behind it (batch 8: 3 stay pending, 11 wrap the ring)."""
    kw = dict(dict(capacity=N + 8, tile=16, batch=8), **kw)
    e = helpers.loaded(N, 5, **kw)
    x = lowrank_data(N, 5)[0]
    for k in (5, 16, N - 3, 11, 40, 77, 2, 120, 63, 64, 100)[:corrections]:
        e.predict(U2); e.correct(observe(x, k), R2, k)
    return e


def ask(e, ents, hyps, **kw):
    return e.joint_innovation(ents, hyps, want_prefix=True, want_nu=True, want_S=True, **kw)


def assert_equal_results(a, b, msg=""):
    for key in KEYS:
        np.testing.assert_array_equal(a[key], b[key], err_msg="%s %s" % (msg, key))


def _set_x(e, x):
    from ekf_slam_amd.engine import _p
    x = np.ascontiguousarray(x, dtype=np.float64)
    e._check(e.lib.ekf_set_x(e.h, _p(x), x.size))


# ------------------------------------------------------------------------------------------------------------------
# a. one pairing: the block is ekf_model_innovation's
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage", [(16, "f64"), (64, "f64"), (128, "f64"), (256, "f32")])
@pytest.mark.parametrize("pending", [0, 3])
def test_one_pairing_is_model_innovation(tile, storage, pending):
    e = loaded(pending, tile=tile, storage=storage)
    assert e.pending() == pending
    ents = J.cycle_scan(e.get_x(), [7, 40, 99, N - 1])
    worst = 0.0
    for ent, lm in zip(ents, (7, 40, 99, N - 1)):
        got = ask(e, [ent], [[lm]])
        ref = e.model_innovation(ent["model"], ent["z"], ent["R"], [lm])
        np.testing.assert_array_equal(got["S"][0], ref["S"])
        np.testing.assert_array_equal(got["nu"][0], ref["nu"])
        worst = max(worst, abs(got["d2"][0] - ref["d2"]) / ref["d2"])
        assert got["d2"][0] == got["d2_prefix"][0, 0] and got["dof"][0] == M.ROWS[ent["model"]] and got["pairings"][0] == 1
        assert (got["outcome"][0], got["first_irregular"][0], ref["outcome"]) == (J.REGULAR, -1, M.APPLIED)
    print("T = %d %s, %d pending: worst relative difference of d2 (Cholesky against the 2 x 2 inverse) %.2e" % (tile, storage, pending, worst))
    assert worst <= 1e-12 and e.pending() == pending
    e.close()


# ------------------------------------------------------------------------------------------------------------------
# b. the off-diagonal blocks against get_P
# ------------------------------------------------------------------------------------------------------------------
# tile 16 holds 8 landmarks a tile row: 2, 3, 5 share the diagonal tile; 16, 17 are neighbours in tile row 2; 7, 8 straddle a tile edge;
# 120 and 40 are far from everything; the order makes l_a < l_b and l_a > l_b both occur
BLOCK_LMS = [3, 2, 7, 8, 120, 17, 16, 5, 40]


@pytest.mark.parametrize("tile,storage,pending", [(16, "f64", 3), (16, "f64", 0), (256, "f32", 0)])
def test_off_diagonal_blocks_against_the_state_read_after_the_call(tile, storage, pending):
    e = loaded(pending, tile=tile, storage=storage)
    ents = J.cycle_scan(e.get_x(), BLOCK_LMS)
    got = ask(e, ents, [BLOCK_LMS])
    x0, P0 = e.get_x(), e.get_P()                       # AFTER the call: with float tiles and nothing pending, exactly what the kernel read
    want = J.joint_dense(x0, P0, ents, BLOCK_LMS)
    bound = J.cross_bound(x0, P0, ents, BLOCK_LMS)
    m = len(BLOCK_LMS)
    off = np.ones((2 * m, 2 * m), dtype=bool)
    for k in range(m):
        off[2 * k:2 * k + 2, 2 * k:2 * k + 2] = False
    diff = np.abs(got["S"][0] - want["S"])
    live = off & (bound > 0.0)
    print("T = %d %s, %d pending: worst |dS_ab| / bound %.3g" % (tile, storage, pending, (diff[live] / bound[live]).max()))
    assert np.all(diff[off] <= bound[off])
    np.testing.assert_array_equal(got["S"][0][off], got["S"][0].T[off])
    np.testing.assert_allclose(got["S"][0], want["S"], rtol=1e-9, atol=1e-14)
    np.testing.assert_allclose(got["nu"][0], want["nu"], rtol=1e-9, atol=1e-9)
    e.close()


# ------------------------------------------------------------------------------------------------------------------
# c. d2 and the prefixes against solve
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,models", [(5, (1, 2, 3, 4)), (32, (1, 4))])
def test_d2_and_prefixes_against_solve_on_the_returned_S(m, models):
    e = loaded(3)
    lms = np.random.default_rng(1).choice(N, m, replace=False).tolist()
    ents = J.cycle_scan(e.get_x(), lms, models)
    got = ask(e, ents, [lms])
    cond = J.cond_of(got["S"][0], lms)
    ref = J.solve_prefixes(got["S"][0], got["nu"][0], lms)
    err = np.abs(got["d2_prefix"][0] - ref) / ref
    print("m = %d: cond(S) %.3g, worst relative error of the prefixes %.2e, d2 = %.4g, dof = %d" % (m, cond, err.max(), got["d2"][0], got["dof"][0]))
    assert cond <= 1e3 and err.max() <= 1e-9 and got["d2"][0] == got["d2_prefix"][0, -1]
    assert got["dof"][0] == sum(M.ROWS[en["model"]] for en in ents) and got["outcome"][0] == J.REGULAR
    want = J.joint_dense(e.get_x(), e.get_P(), ents, lms)
    np.testing.assert_allclose(got["d2_prefix"][0], want["d2_prefix"], rtol=1e-9)
    e.close()


# ------------------------------------------------------------------------------------------------------------------
# d. bit-for-bit equalities
# ------------------------------------------------------------------------------------------------------------------
def test_prefixes_sub_scans_and_batches_bit_for_bit():
    e = loaded(3)
    m = 9
    lms = np.random.default_rng(3).choice(N, m, replace=False).tolist()
    ents = J.cycle_scan(e.get_x(), lms)
    hyp = list(lms)
    hyp[2] = hyp[6] = -1
    cuts = [hyp[:k + 1] + [-1] * (m - k - 1) for k in range(m)]
    rng = np.random.default_rng(4)
    more = [[int(v) for v in np.where(rng.random(m) < 0.3, -1, rng.choice(N, m, replace=False))] for _ in range(40 - m - 2)]
    hyps = [hyp] + cuts + [[-1] * m] + more
    assert len(hyps) == 40
    got = ask(e, ents, hyps)
    # the prefix property
    np.testing.assert_array_equal(got["d2_prefix"][0], got["d2"][1:1 + m])
    assert got["d2_prefix"][0, 2] == got["d2_prefix"][0, 1]
    # a hypothesis with no pairing
    k0 = 1 + m
    assert (got["d2"][k0], got["dof"][k0], got["pairings"][k0], got["outcome"][k0], got["first_irregular"][k0]) == (0.0, 0, 0, J.REGULAR, -1)
    np.testing.assert_array_equal(got["S"][k0], np.eye(2 * m))
    assert not got["nu"][k0].any() and not got["d2_prefix"][k0].any()
    # 40 hypotheses in one call are 40 calls of one
    for i, h in enumerate(hyps):
        one = ask(e, ents, [h])
        for key in KEYS:
            np.testing.assert_array_equal(one[key][0], got[key][i], err_msg="hypothesis %d %s" % (i, key))
    # the sub-scan property
    keep = [k for k in range(m) if hyp[k] >= 0]
    short = ask(e, [ents[k] for k in keep], [[hyp[k] for k in keep]])
    rows = [2 * k + r for k in keep for r in range(2)]
    assert short["d2"][0] == got["d2"][0] and short["dof"][0] == got["dof"][0]
    np.testing.assert_array_equal(short["d2_prefix"][0], got["d2_prefix"][0][keep])
    np.testing.assert_array_equal(short["S"][0], got["S"][0][np.ix_(rows, rows)])
    np.testing.assert_array_equal(short["nu"][0], got["nu"][0][rows])
    assert np.all(np.isfinite(got["d2"]))
    e.close()


# ------------------------------------------------------------------------------------------------------------------
# e. pending pairs: the call reads the tiles patched, and changes nothing
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leg", ["3 pending", "11 corrections: the ring wrapped", "beside an asynchronous pass"])
def test_before_a_flush_equals_after_it_and_nothing_changes(leg):
    kw = dict(batch=4, async_flush=True) if leg.startswith("beside") else {}
    steps = {"3": 3, "1": 11, "b": 6}[leg[0]]
    e, twin = loaded(steps, **kw), loaded(steps, **kw)
    pend = e.pending()
    assert pend == twin.pending() and (leg[0] == "b" or pend == 3) and pend >= 2       # (beside the pass its frozen pairs may still count)
    x_before = e.get_x()
    lms = [3, 2, 7, 8, 120, 17, 16, 5, 40, 77, 63, 64]       # corrected landmarks and their tile-row neighbours among them
    ents = J.cycle_scan(x_before, lms)
    hyps = [lms, lms[::-1][:6] + [-1] * 6, [-1, 5] + [-1] * 10]
    got = ask(e, ents, hyps)
    assert e.pending() == pend
    np.testing.assert_array_equal(e.get_x(), x_before)
    assert_same(e, twin)                                      # x, s, P, the diagonal blocks and the digest of a twin that never asked
    e.flush()
    assert e.pending() == 0
    assert_equal_results(ask(e, ents, hyps), got, leg)
    assert np.all(np.isfinite(got["d2"])) and np.all(got["outcome"] == J.REGULAR)
    e.close(); twin.close()


# ------------------------------------------------------------------------------------------------------------------
# f. irregular hypotheses
# ------------------------------------------------------------------------------------------------------------------
def test_a_landmark_on_the_robot_in_the_middle_of_a_hypothesis():
    e = loaded(0)
    lms = [12, 30, 13, 14, 90]
    ents = J.cycle_scan(e.get_x(), lms, (1, 4))
    others = [[12, 30, -1, 14, 90], [90, 14, -1, 30, 12], [12, 30, -1, -1, -1]]
    clean = ask(e, ents, others)
    x = e.get_x()
    x[3 + 2 * 13:5 + 2 * 13] = x[:2]
    _set_x(e, x)
    got = ask(e, ents, [others[0], lms, others[1], others[2]])
    assert (got["outcome"][1], got["first_irregular"][1], got["pairings"][1], got["dof"][1]) == (J.IRREGULAR, 2, 5, 10) and np.isnan(got["d2"][1])
    np.testing.assert_array_equal(got["d2_prefix"][1, :2], got["d2_prefix"][3, :2])          # what they would be without it
    assert np.all(np.isfinite(got["d2_prefix"][1, :2])) and np.all(np.isnan(got["d2_prefix"][1, 2:]))
    for i, j in ((0, 0), (2, 1), (3, 2)):                     # the other hypotheses of the same call are untouched
        for key in KEYS:
            np.testing.assert_array_equal(got[key][i], clean[key][j], err_msg=key)
    assert e.model_innovation(ents[2]["model"], ents[2]["z"], ents[2]["R"], [13])["outcome"] == M.IRREGULAR
    e.close()


def test_a_pivot_that_is_not_positive_is_reported_and_everything_stays_finite():
    e = loaded(0)
    x, s, P = helpers.state(e)
    lms = [12, 30, 90]
    a = 3 + 2 * 30
    for lo, hi in ((0, 3), (a, a + 2)):                       # the robot's rows too: H_r Prr H_r' alone would keep S positive
        P[lo:hi, :] = 0.0
        P[:, lo:hi] = 0.0
    e.set_state(x, P, s)
    ents = J.cycle_scan(x, lms, (4, 2, 1))
    ents[1] = A.entry(M.RANGE, ents[1]["z"], 0.0)
    got = ask(e, ents, [lms, [12, -1, 90]])
    assert (got["outcome"][0], got["first_irregular"][0]) == (J.IRREGULAR, 1) and got["S"][0][2, 2] == 0.0
    assert np.isfinite(got["d2_prefix"][0, 0]) and got["d2_prefix"][0, 0] == got["d2_prefix"][1, 0] and np.all(np.isnan(got["d2_prefix"][0, 1:]))
    assert np.all(np.isfinite(got["S"])) and np.all(np.isfinite(got["nu"]))
    assert got["outcome"][1] == J.REGULAR and np.isfinite(got["d2"][1])
    np.testing.assert_array_equal(e.get_P(), P)
    assert np.all(np.isfinite(e.get_x()))
    e.close()


# ------------------------------------------------------------------------------------------------------------------
# g. refusals, in the stated order
# ------------------------------------------------------------------------------------------------------------------
def _raw(e, ents, hyps, m=None, nh=None, out=True):
    from ekf_slam_amd import _lib as L
    arr = (L.EkfModelObs * max(len(ents), 1))()
    for k, ent in enumerate(ents):
        arr[k] = e._model_obs(ent["model"], ent["z"], ent["R"], (), (0.0, 0.0), ent["gate"])
    hyp = np.ascontiguousarray(hyps, dtype=np.int64)
    res = (L.EkfJointResult * max(hyp.shape[0], 1))()
    return e.lib.ekf_joint_innovation(e.h, arr, len(ents) if m is None else m, hyp.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                      hyp.shape[0] if nh is None else nh, res if out else None, None, None, None)


def test_refusals_in_their_order_and_nothing_changes():
    from ekf_slam_amd import _lib as L
    e, twin = loaded(3), loaded(3)
    before = helpers.getters(twin)                              # (reading P flushes: the twin is read, e keeps its three pairs pending)
    ents = J.cycle_scan(e.get_x(), [1, 20, 41])
    big = J.cycle_scan(e.get_x(), list(range(33)))
    bad = L.EKF_ERR_INVALID_ARG
    assert _raw(e, ents, [[1, 20, 1]]) == bad and b"twice" in e.lib.ekf_last_error(e.h)
    assert _raw(e, ents, [[1, -2, 3]]) == bad
    assert _raw(e, ents, np.full((257, 3), -1), nh=257) == bad and _raw(e, ents, [[1, 2, 3]], nh=0) == bad
    assert _raw(e, big, np.full((1, 33), -1), m=33) == bad and _raw(e, ents, [[1, 2, 3]], m=0) == bad
    assert _raw(e, ents, [[1, 2, 3]], out=False) == bad
    assert _raw(e, [dict(ents[0], model=M.LANDMARK_RANGE)] + ents[1:], [[1, 2, 3]]) == bad
    assert _raw(e, [dict(ents[0], gate=float("nan"))] + ents[1:], [[1, 2, 3]]) == bad
    assert _raw(e, ents, [[1, 2, N]]) == L.EKF_ERR_INDEX and _raw(e, ents, [[1, 2, N - 1]]) == 0
    assert _raw(e, ents, [[1, N, 1]]) == bad                      # the arguments before the index
    assert e.pending() == 3
    for got, ref in zip(helpers.getters(e), before):
        np.testing.assert_array_equal(got, ref)
    # sharded handles: refused, and the message says why; the arguments are checked first, the index last
    sh = helpers.engine(capacity=64, tile=16, world=2, rank=0)
    st, msg = status_of(lambda: sh.joint_innovation(ents, [[1, 2, 3]]))
    assert st == bad and "shard" in msg
    st, msg = status_of(lambda: sh.joint_innovation(ents, [[1, 2, 1]]))
    assert st == bad and "shard" not in msg
    e.close(); twin.close(); sh.close()


def test_a_lone_shard_works_and_is_refused_between_begin_and_finish():
    from ekf_slam_amd import _lib as L
    x = lowrank_data(N, 5)[0]
    kw = dict(capacity=N + 8, tile=16)
    e, twin = helpers.loaded(N, 5, force_sharded=1, **kw), helpers.loaded(N, 5, **kw)
    harr = (ctypes.c_void_p * 1)(e.h)
    lms = [3, 2, 7, 8, 120, 17]
    ents = J.cycle_scan(x, lms)
    z = observe(x, 7)
    e.predict(U2); twin.predict(U2)
    e.correct_begin(z, R2, 7)
    st, msg = status_of(lambda: e.joint_innovation(ents, [lms]))
    assert st == L.EKF_ERR_STATE and "joint_innovation" in msg and "begin and finish" in msg
    assert status_of(lambda: e.joint_innovation(ents, [[3, 3, 7, 8, 120, 17]]))[0] == L.EKF_ERR_INVALID_ARG      # the arguments come first ...
    assert status_of(lambda: e.joint_innovation(ents, [[3, 2, 7, 8, 120, N]]))[0] == L.EKF_ERR_STATE             # ... and the index last
    assert e.lib.ekf_exchange_local(harr, 1) == 0
    e.correct_finish()
    twin.correct(z, R2, 7)
    hyps = [lms, lms[::-1], [-1, 2, -1, 8, -1, 17]]
    assert_equal_results(ask(e, ents, hyps), ask(twin, ents, hyps), "a lone shard")
    assert_same(e, twin)
    e.close(); twin.close()


# ------------------------------------------------------------------------------------------------------------------
# h. the policy on the real engine
# ------------------------------------------------------------------------------------------------------------------
def test_measure_model_joint_matches_what_measure_model_discards_and_replays(tmp_path):
    from ekf_slam_amd.slam import EKF_SLAM
    from ekf_slam_amd.trajectory import TrajectoryLog
    J.assert_scene_premises()
    x, s, d, U, scan = J.ambiguous_scene()
    kw = dict(capacity=N + 8, tile=16, batch=8)

    def start():
        f = EKF_SLAM(**kw)
        f._e.load_lowrank_state(x, s, d, U)
        return f

    old, new, hand = start(), start(), start()
    assert old.measure_model(scan, J.GATE, 25.0) == [("discarded", 0), ("discarded", 0)] and old._e.pending() == 0
    new.log = TrajectoryLog()
    out, truncated = new.measure_model_joint(scan, J.GATE, 25.0)
    assert out == [("matched", J.LM_A + 1), ("matched", J.LM_B + 1)] and truncated is False and new._e.pending() == 2
    for (model, z, R), lm in zip(scan, (J.LM_A, J.LM_B)):
        hand.observe_model(model, z, R, [lm + 1], gate=J.GATE)
    assert_same(new._e, hand._e)
    assert not np.array_equal(new._e.get_x(), old._e.get_x())
    new.predict(U2)
    new.log.record(U2, None, [], [])                          # (what measure() records of a step without sightings: the edits replay in front of it)
    path = tmp_path / "joint.npz"
    new.log.save(path)
    log = TrajectoryLog.load(path)
    assert [ed[1] for ed in log.edits] == ["observe_model"] * 2 and len(log) == 1
    fresh = helpers.engine(**kw)
    fresh.load_lowrank_state(x, s, d, U)
    log.replay(fresh)
    assert_same(fresh, new._e)
    for q in (old._e, new._e, hand._e, fresh):
        q.close()
