"""GPU: model observations relinearised on the device (ekf_observe_model_iterated, ekf_model_innovation_iterated; include/ekfslam.h,
DESIGN.md section 3o).

The yardstick is the NumPy restatement of tests/model_iter_cases.py applied to the state a twin engine with the same history reported
before the call; tolerances and helpers are those of tests/helpers.py.  Where two engines ran the same arithmetic on the same inputs --
one linearisation against ekf_observe_model, the probe against the step, a replayed log -- the comparison is assert_array_equal.

N = 130 landmarks are 260 columns: two workgroups of k_gather_model_iter, the second one nearly idle, and a tile edge crossed at every
tile size used.  The priors are wide (a heading known to 5 degrees, landmarks to 1-2 m) so that relinearising moves the result by far
more than any tolerance here."""
import numpy as np
import pytest

import model_iter_cases as I
import model_obs_cases as M
from helpers import R2, REL, TOL_X32, U2, assert_same, check_state, engine, getters, rel_err, state, status_of
from removal_cases import lowrank_data, observe

pytestmark = pytest.mark.gpu
N = 130
RB = np.diag([0.01, 0.25])
STORES = [(64, "f64"), (256, "f32")]


def wide_engine(tile, storage, batch=4, **kw):
    x, s, d, U = lowrank_data(N, 5)
    d = d.copy()
    d[:3] = [0.25, 0.25, 25.0]
    d[3:] *= 20.0
    e = engine(capacity=N + 8, tile=tile, storage=storage, batch=batch, **kw)
    e.load_lowrank_state(x, s, d, U)
    return e, x


def history(engines, x, ks=(5, 70, N - 3)):
    for q in engines:
        for k in ks:
            q.predict(U2); q.correct(observe(x, k), R2, k)


def edge(tile):
    """The first landmark of the second tile row: it and its predecessor are adjacent over a tile edge."""
    return tile // 2


def specs(tile, x):
    """(name, observation): a range and bearing on the last landmark, a landmark range across the tile edge (its cross block is read
    through the pending chain), both about one sigma of the prior off h(x)."""
    out = []
    o = M.obs(M.RANGE_BEARING, [0, 0], RB, [N - 1])
    o["z"] = M.jacobian(x, o)[0] + np.array([0.8, 4.0])
    out.append(("range and bearing, last landmark", o))
    o = M.obs(M.LANDMARK_RANGE, [0], 0.01, [edge(tile), edge(tile) - 1])
    o["z"][0] = M.jacobian(x, o)[0][0] + 1.5
    out.append(("landmark range across the tile edge", o))
    return out


def send(e, o, n, tol=0.0, wait=True):
    return e.observe_model_iterated(o["model"], o["z"][:o["rows"]], o["R"], o["landmarks"], o["anchor"], gate=o["gate"], iterations=n, tol=tol, wait=wait)


def ask(e, o, n, tol=0.0):
    return e.model_innovation_iterated(o["model"], o["z"][:o["rows"]], o["R"], o["landmarks"], o["anchor"], gate=o["gate"], iterations=n, tol=tol)


def same_result(a, b, name=""):
    for key in ("nu", "S", "d2", "outcome"):
        np.testing.assert_array_equal(np.asarray(a[key]), np.asarray(b[key]), err_msg=name + " " + key)
    if "iterated" in a and "iterated" in b:
        for key in ("S", "nu", "used", "converged", "last_step", "x_local"):
            np.testing.assert_array_equal(np.asarray(a["iterated"][key]), np.asarray(b["iterated"][key]), err_msg=name + " iterated " + key)


# ------------------------------------------------------------------------------------------------------------------
# 7. one linearisation is today's call
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage", STORES)
def test_one_linearisation_writes_the_bits_of_observe_model(tile, storage):
    for which in (0, 1):
        (a, x), (b, _) = wide_engine(tile, storage), wide_engine(tile, storage)
        history([a, b], x)
        assert a.pending() == b.pending() == 3
        name, o = specs(tile, x)[which]
        ra = a.observe_model(o["model"], o["z"][:o["rows"]], o["R"], o["landmarks"], o["anchor"], gate=o["gate"], wait=True)
        rb = send(b, o, 1)
        assert a.pending() == b.pending() == 0               # the fourth step of the batch: the pass ran, over the same four pairs
        assert ra["outcome"] == M.APPLIED
        same_result(ra, rb, name)
        # the pair's record is the first linearisation's
        np.testing.assert_array_equal(rb["iterated"]["S"], rb["S"]); np.testing.assert_array_equal(rb["iterated"]["nu"], rb["nu"])
        assert rb["iterated"]["used"] == 1
        np.testing.assert_array_equal(a.get_x(), b.get_x(), err_msg=name)
        np.testing.assert_array_equal(a.get_P(), b.get_P(), err_msg=name)
        assert_same(a, b)
        a.close(); b.close()


# ------------------------------------------------------------------------------------------------------------------
# 8. four linearisations against the restatement
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage", STORES)
def test_four_linearisations_against_the_dense_restatement(tile, storage):
    for which in (0, 1):
        (e, x), (twin, _) = wide_engine(tile, storage), wide_engine(tile, storage)
        history([e, twin], x)
        x0, _, P0 = state(twin)                                # (reading P flushes: the twin is read, e keeps its three pairs pending)
        assert e.pending() == 3
        name, o = specs(tile, x0)[which]
        ex, eP, wfirst, wit = I.iterate_dense(x0, P0, o, 4)
        ex1 = I.iterate_dense(x0, P0, o, 1)[0]
        assert wfirst["outcome"] == M.APPLIED and wit["used"] == 4
        assert rel_err(ex, ex1) > 100.0 * REL                  # relinearising matters here: four land elsewhere than one
        got = send(e, o, 4)
        it = got["iterated"]
        tol = REL                                              # F64 arithmetic on what the getters report, in every storage kind
        errs = (rel_err(got["nu"], wfirst["nu"]), rel_err(got["S"], wfirst["S"]), abs(got["d2"] - wfirst["d2"]) / wfirst["d2"],
                rel_err(it["S"], wit["S"]), float(np.abs(it["nu"] - wit["nu"]).max() / max(np.abs(wfirst["nu"]).max(), 1.0)),
                rel_err(it["x_local"], wit["x_local"]), abs(it["last_step"] - wit["last_step"]) / max(wit["last_step"], 1e-300))
        print("%s [T = %d %s]: rel err nu0 %.2e S0 %.2e d2 %.2e S %.2e r %.2e x_local %.2e last step %.2e (%.3g)" % ((name, tile, storage) + errs + (it["last_step"],)))
        assert got["outcome"] == M.APPLIED and it["used"] == wit["used"] == 4 and not it["converged"]
        assert max(errs[:6]) < tol and errs[6] < 1e-3, name
        e.flush()
        check_state(e, ex, eP, storage, name)
        loc = I.local_rows(o)
        xl = np.zeros(7); xl[:len(loc)] = e.get_x()[loc]
        assert rel_err(it["x_local"], xl) < (REL if storage == "f64" else TOL_X32), name
        e.close(); twin.close()


# ------------------------------------------------------------------------------------------------------------------
# 9. the probe equals the step and changes nothing
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage", STORES)
def test_the_probe_reports_the_step_and_changes_nothing(tile, storage):
    (e, x), (twin, _) = wide_engine(tile, storage, batch=8), wide_engine(tile, storage, batch=8)
    history([e, twin], x)
    for name, o in specs(tile, x):
        for n, tol in ((1, 0.0), (4, 0.0), (16, 1e-9)):
            before_x, pend = e.get_x(), e.pending()           # (the digest flushes: it is compared below, once the twin has been)
            want = ask(e, o, n, tol)
            assert e.pending() == pend
            np.testing.assert_array_equal(e.get_x(), before_x)
            plain = e.model_innovation(o["model"], o["z"][:o["rows"]], o["R"], o["landmarks"], o["anchor"], gate=o["gate"])
            same_result(plain, want, name)                    # `first` is ekf_model_innovation's
            got = send(e, o, n, tol)
            send(twin, o, n, tol, wait=False)
            same_result(got, want, name)
            if tol > 0.0:
                assert got["iterated"]["converged"] and got["iterated"]["used"] < 16
    assert_same(e, twin)                                      # the twin never asked, and never waited
    before_x, before_d = e.get_x(), e.digest()
    for name, o in specs(tile, x):
        ask(e, o, 4)
    np.testing.assert_array_equal(e.get_x(), before_x); np.testing.assert_array_equal(e.digest(), before_d)


# ------------------------------------------------------------------------------------------------------------------
# 10. no-ops and refusals
# ------------------------------------------------------------------------------------------------------------------
def test_gated_and_irregular_calls_change_nothing():
    from ekf_slam_amd import _lib as L
    (e, x), (twin, _) = wide_engine(64, "f64"), wide_engine(64, "f64")
    history([e, twin], x, (9,))
    assert e.linear_rejections() == (0, 0)
    before = getters(twin)
    name, o = specs(64, x)[0]
    d2 = ask(e, o, 4)["d2"]
    gated = dict(o, gate=d2 / 3.0)
    res = send(e, gated, 4)
    assert res["outcome"] == L.EKF_LINEAR_GATED and res["d2"] == d2 and res["iterated"]["used"] == 0 and e.pending() == 2
    on_robot = M.obs(M.RANGE, [1.0], 0.5, anchor=e.get_x()[:2])
    st, msg = status_of(lambda: send(e, on_robot, 4))
    assert st == L.EKF_ERR_STATE and "observe_model_iterated" in msg and e.pending() == 3
    assert e.linear_rejections() == (1, 1) and e.linear_rejections() == (0, 0)
    send(e, gated, 4, wait=False)                             # the fourth step: the pass runs over zero pairs
    assert e.pending() == 0 and e.linear_rejections() == (0, 1)
    for got, ref in zip(getters(e), before):
        assert np.all(np.isfinite(got))
        np.testing.assert_array_equal(got, ref)
    # argument checks, before anything changes
    for n, tol in ((0, 0.0), (17, 0.0), (-1, 0.0), (3, -1e-9), (3, float("nan"))):
        st, msg = status_of(lambda: send(e, o, n, tol))
        assert st == L.EKF_ERR_INVALID_ARG and "observe_model_iterated" in msg, (n, tol)
        st, msg = status_of(lambda: ask(e, o, n, tol))
        assert st == L.EKF_ERR_INVALID_ARG and "model_innovation_iterated" in msg, (n, tol)
    assert e.pending() == 0
    for got, ref in zip(getters(e), before):
        np.testing.assert_array_equal(got, ref)
    # sharded handles are refused with the message of the unsharded rung; the arguments are checked first
    sh = engine(capacity=64, tile=16, world=2, rank=0)
    for fn in (lambda: send(sh, M.obs(M.RANGE, [1.0], 0.5, [0]), 3), lambda: ask(sh, M.obs(M.BEARING, [1.0], 0.5, anchor=[3.0, 4.0]), 3)):
        st, msg = status_of(fn)
        assert st == L.EKF_ERR_INVALID_ARG and "shard" in msg
    st, msg = status_of(lambda: send(sh, M.obs(M.RANGE, [1.0], 0.5, anchor=[3.0, 4.0]), 17))
    assert st == L.EKF_ERR_INVALID_ARG and "shard" not in msg


def test_an_iterate_on_the_anchor_is_an_irregular_no_op():
    """The scene of tests/test_model_iter_cpu.py in an engine: the first step puts the robot exactly on the anchor, so the second
    linearisation has no Jacobian and the whole call is irregular -- while one linearisation applies."""
    from ekf_slam_amd import _lib as L
    x3, P3, o = I.anchor_hit_scene()
    x = np.concatenate([x3, [7.0, 3.0, -5.0, 6.0]])
    P = np.zeros((7, 7)); P[:3, :3] = P3; P[3:, 3:] = 0.5 * np.eye(4)
    e = engine(capacity=8, tile=16, batch=4)
    e.set_state(x, P, [1.0, 2.0])
    before = getters(e)
    probe = ask(e, o, 2)
    assert probe["outcome"] == L.EKF_LINEAR_IRREGULAR and probe["iterated"]["used"] == 1 and probe["d2"] == 32.0
    assert np.all(np.isfinite(probe["iterated"]["S"])) and np.all(np.isfinite(probe["iterated"]["x_local"]))
    st, msg = status_of(lambda: send(e, o, 2))
    assert st == L.EKF_ERR_STATE and "nothing was changed" in msg and e.pending() == 1
    send(e, o, 16, wait=False)
    assert e.pending() == 2 and e.linear_rejections() == (2, 0)
    for got, ref in zip(getters(e), before):
        assert np.all(np.isfinite(got))
        np.testing.assert_array_equal(got, ref)
    got = send(e, o, 1)
    assert got["outcome"] == L.EKF_LINEAR_APPLIED and got["iterated"]["x_local"][:3].tolist() == [4.0, 0.0, -4.0]
    np.testing.assert_array_equal(e.get_x()[:3], [4.0, 0.0, -4.0])


# ------------------------------------------------------------------------------------------------------------------
# 11. end to end: the wrapper, the MAP cost, the log
# ------------------------------------------------------------------------------------------------------------------
def test_iterating_lowers_the_map_cost_end_to_end_and_replays_from_its_log(tmp_path):
    from ekf_slam_amd.slam import EKF_SLAM
    from ekf_slam_amd.trajectory import FORMAT_ITERATED, TrajectoryLog
    x5, P5, o = I.map_scene(M.RANGE_BEARING)
    x = np.concatenate([x5, [-6.0, 8.0, 3.0, -12.0]])
    P = np.zeros((9, 9)); P[:5, :5] = P5; P[5:, 5:] = np.diag([1.0, 2.0, 3.0, 4.0])
    s = [1.0, 2.0, 3.0]
    kw = dict(capacity=8, tile=16, batch=4)
    runs = {}
    for n in (1, 8):
        f = EKF_SLAM(**kw)
        f._e.set_state(x, P, s)
        f.log = TrajectoryLog()
        f._e.predict(U2); f.log.record(U2, None, [], np.zeros((0, 2)))
        prior_x, prior_P = f.x, f.P
        res = f.observe_range_bearing(1, o["z"], o["R"], wait=True, iterations=n)
        assert res["outcome"] == 1 and (n == 1) == ("iterated" not in res)
        runs[n] = (f, prior_x, prior_P, f.x)
    np.testing.assert_array_equal(runs[1][1], runs[8][1]); np.testing.assert_array_equal(runs[1][2], runs[8][2])
    x0, P0 = runs[1][1], runs[1][2]
    o9 = dict(o)
    want = {n: I.map_cost(I.iterate_dense(x0, P0, o9, n)[0], x0, P0, o9) for n in (1, 8)}
    gap = want[1] - want[8]
    J = {n: I.map_cost(runs[n][3], x0, P0, o9) for n in (1, 8)}
    print("J after one linearisation %.4f (restatement %.4f), after eight %.4f (%.4f)" % (J[1], want[1], J[8], want[8]))
    assert gap >= 0.05 and J[8] < J[1] - 0.5 * gap
    f = runs[8][0]
    path = tmp_path / "iterated.npz"
    f.log.save(path)
    log = TrajectoryLog.load(path)
    assert str(np.load(path)["format"]) == FORMAT_ITERATED and [(e[0], e[1], e[2].tolist()) for e in log.edits] == [(1, "observe_model_iterated", [1])]
    fresh = engine(**kw)
    fresh.set_state(x, P, s)
    log.replay(fresh)
    np.testing.assert_array_equal(fresh.get_x(), f.x)
    np.testing.assert_array_equal(fresh.get_P(), f.P)
    # the plain run's log is written as before: no ninth kind, no format 8
    runs[1][0].log.save(tmp_path / "plain.npz")
    assert str(np.load(tmp_path / "plain.npz")["format"]) == "ekfslam-trajectory-5"
