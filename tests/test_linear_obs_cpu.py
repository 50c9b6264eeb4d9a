"""CPU: the arithmetic of a linear observation (tests/linear_obs_cases.py: hand-derived answers, dense against information form, dense
against merge_cases for H = (+I, -I)), the fifth kind of the trajectory log, and the argument handling of the Python layers over a
stand-in for the library.  No GPU."""

import numpy as np
import pytest

import linear_obs_cases as C
from helpers import RPOS, RecorderBase
from merge_cases import constrain_dense


# ------------------------------------------------------------------------------------------------------------------
# hand-derived answers
# ------------------------------------------------------------------------------------------------------------------
def test_a_landmark_fix_is_the_product_of_two_gaussians():
    # one landmark, uncorrelated with the robot: N((2, -1), diag(3, 1)) times N((4, 1), diag(1, 1))
    #   variances 3 * 1 / (3 + 1) = 3/4 and 1 * 1 / (1 + 1) = 1/2; means 2 + 3/4 * (4 - 2) = 3.5 and -1 + 1/2 * (1 + 1) = 0
    x = np.array([0.0, 0.0, 0.0, 2.0, -1.0])
    P = np.diag([0.1, 0.1, 0.1, 3.0, 1.0])
    x2, P2, res = C.observe_dense(x, P, C.landmark_fix(0, [4.0, 1.0], np.eye(2)))
    np.testing.assert_allclose(P2[3:, 3:], np.diag([0.75, 0.5]), atol=1e-15)
    np.testing.assert_allclose(x2, [0.0, 0.0, 0.0, 3.5, 0.0], atol=1e-15)
    np.testing.assert_allclose(P2[:3, :3], 0.1 * np.eye(3), atol=0)
    # S = diag(4, 2), nu = (2, 2): d2 = 4/4 + 4/2 = 3
    assert res["outcome"] == C.APPLIED and res["d2"] == pytest.approx(3.0, abs=1e-15)
    np.testing.assert_array_equal(res["S"], np.diag([4.0, 2.0]))


def test_a_robot_position_fix_moves_a_correlated_landmark():
    # robot x ~ N(0, 1), landmark x = robot x + 5 exactly correlated through P(0, 3) = 1, P(3, 3) = 2; a fix x = 1 with R = 1:
    #   S = 2, K(0) = 1/2, K(3) = 1/2: robot x -> 0.5, landmark x -> 5.5; P(0,0) -> 1/2, P(3,3) -> 2 - 1/2 = 3/2, P(0,3) -> 1/2
    x = np.array([0.0, 0.0, 0.0, 5.0, 0.0])
    P = np.diag([1.0, 1.0, 1.0, 2.0, 1.0]); P[0, 3] = P[3, 0] = 1.0
    x2, P2, res = C.observe_dense(x, P, C.position_fix([1.0, 0.0], np.eye(2)))
    np.testing.assert_allclose(x2, [0.5, 0.0, 0.0, 5.5, 0.0], atol=1e-15)
    assert P2[0, 0] == pytest.approx(0.5) and P2[3, 3] == pytest.approx(1.5) and P2[0, 3] == pytest.approx(0.5) and P2[1, 1] == pytest.approx(0.5)
    assert res["d2"] == pytest.approx(0.5)


def test_a_heading_fix_across_180_degrees_turns_the_short_way():
    # state 179 deg, reading -179 deg: nu = -358 wrapped to +2; variance 4 against var 4: the heading moves by half of nu
    x = np.array([0.0, 0.0, 179.0])
    P = np.diag([1.0, 1.0, 4.0])
    x2, P2, res = C.observe_dense(x, P, C.heading_fix(-179.0, 4.0))
    assert res["nu"].tolist() == [2.0, 0.0]
    np.testing.assert_array_equal(res["S"], [[8.0, 0.0], [0.0, 1.0]])           # rows = 1: the second row is exactly empty
    assert x2[2] == 180.0 and P2[2, 2] == 2.0 and res["d2"] == 0.5
    np.testing.assert_array_equal(P2[:2, :2], np.eye(2))
    # without the wrap the same reading would drag the heading through 0
    o = C.heading_fix(-179.0, 4.0); o["wrap"] = (0, 0)
    assert C.observe_dense(x, P, o)[2]["nu"][0] == -358.0
    assert C.wrap180(180.0) == 180.0 and C.wrap180(-180.0) == 180.0 and C.wrap180(540.0) == 180.0 and C.wrap180(-179.0) == -179.0


def test_gate_and_irregular_S_leave_the_state():
    rng = np.random.default_rng(3)
    x, P, _ = C.random_state(rng, 6)
    o = C.landmark_fix(2, x[7:9] + [3.0, -2.0], RPOS)
    d2 = C.observe_dense(x, P, o)[2]["d2"]
    o["gate"] = 0.5 * d2
    x2, P2, res = C.observe_dense(x, P, o)
    assert res["outcome"] == C.GATED and res["d2"] == d2
    np.testing.assert_array_equal(x2, x); np.testing.assert_array_equal(P2, P)
    # a landmark fixed with R = 0 has a zero own block afterwards: fixing it again gives S = 0
    x3, P3, _ = C.observe_dense(x, P, C.landmark_fix(2, [1.0, 1.0], np.zeros((2, 2))))
    assert np.abs(P3[7:9, :]).max() < 1e-12 and np.abs(x3[7:9] - 1.0).max() < 1e-12
    P3[7:9, :] = 0.0; P3[:, 7:9] = 0.0
    res = C.observe_dense(x3, P3, C.landmark_fix(2, [1.5, 1.0], np.zeros((2, 2))))[2]
    assert res["outcome"] == C.IRREGULAR and np.isnan(res["d2"])


# ------------------------------------------------------------------------------------------------------------------
# dense against the information form, and against merge_cases for H = (+I, -I)
# ------------------------------------------------------------------------------------------------------------------
def _kinds(rng, x, N):
    return {"landmark fix": C.landmark_fix(N - 1, x[3 + 2 * (N - 1):5 + 2 * (N - 1)] + [0.3, -0.2], RPOS),
            "position fix": C.position_fix(x[:2] + [0.2, 0.1], RPOS),
            "heading fix": C.heading_fix(x[2] + 365.0, 0.7),
            "general H": C.general(rng, 4, 1, x),
            "scalar on a landmark": C.scalar_on_landmark(0, 0.6 * x[3] - 0.8 * x[4] + 0.4, 0.05)}


def test_dense_update_equals_the_information_form():
    rng = np.random.default_rng(11)
    N = 7
    x, P, _ = C.random_state(rng, N)
    for name, o in _kinds(rng, x, N).items():
        xd, Pd, res = C.observe_dense(x, P, o)
        xi, Pi = C.observe_information(x, P, o)
        assert res["outcome"] == C.APPLIED, name
        np.testing.assert_allclose(Pd, Pi, rtol=0, atol=1e-11 * np.abs(P).max(), err_msg=name)
        np.testing.assert_allclose(xd, xi, rtol=0, atol=1e-10 * np.abs(x).max(), err_msg=name)
        np.testing.assert_allclose(Pd, Pd.T, rtol=0, atol=1e-14)
        # the observed combination is better known afterwards, nothing is worse known
        assert np.all(np.diag(Pd) <= np.diag(P) + 1e-14), name
    # rows = 1 IS the rank-2 update with the empty second row: the same numbers as a true scalar update
    o = _kinds(rng, x, N)["scalar on a landmark"]
    h = C.jacobian(x.size, o)[0]
    g = h @ P
    s = g @ h + o["R"][0, 0]
    xs = x + g / s * (o["z"][0] - h @ x)
    xd, Pd, res = C.observe_dense(x, P, o)
    np.testing.assert_allclose(xd, xs, rtol=0, atol=1e-13 * np.abs(x).max())
    np.testing.assert_allclose(Pd, P - np.outer(g, g) / s, rtol=0, atol=1e-15)
    assert res["S"][1].tolist() == [0.0, 1.0] and res["S"][0, 1] == 0.0 and res["nu"][1] == 0.0


def test_dense_update_with_plus_and_minus_identity_is_the_constraint():
    rng = np.random.default_rng(12)
    x, P, _ = C.random_state(rng, 9)
    for i, j, delta, R in ((2, 6, [0.3, -0.1], RPOS), (8, 0, None, np.zeros((2, 2))), (3, 4, [1.0, 2.0], np.diag([0.5, 0.1]))):
        d = np.zeros(2) if delta is None else np.asarray(delta)
        xd, Pd, res = C.observe_dense(x, P, C.relative(i, j, d, R))
        xc, Pc, d2, S = constrain_dense(x, P, i, j, delta, R)
        np.testing.assert_allclose(xd, xc, rtol=0, atol=1e-13 * np.abs(x).max())
        np.testing.assert_allclose(Pd, Pc, rtol=0, atol=1e-14 * np.abs(P).max())
        assert res["d2"] == pytest.approx(d2, rel=1e-12)
        np.testing.assert_allclose(res["S"], S, rtol=0, atol=1e-14)


def test_factored_form_follows_the_dense_one():
    rng = np.random.default_rng(13)
    from removal_cases import lowrank_data, observe
    N = 12
    x, s, d, U = lowrank_data(N, 4)
    f = C.Factored(x, d, U)
    P = np.diag(d) + U @ U.T
    xd = x.copy()
    for o in (C.position_fix(x[:2] + 0.05, RPOS), C.landmark_fix(5, x[13:15] + 0.1, RPOS), C.general(rng, 2, 9, x, 0.1), C.heading_fix(x[2] + 0.5, 0.2)):
        xd, P, _ = C.observe_dense(xd, P, o)
        f.observe(o)
    np.testing.assert_allclose(f.x, xd, rtol=0, atol=1e-12)
    np.testing.assert_allclose(f.rows(0, x.size), P, rtol=0, atol=1e-15)
    # the correction it carries for the test at size is the filter's own: nu ~ (0.01, 0.2) from removal_cases.observe
    before = f.x.copy()
    f.correct(observe(f.x, 3), np.diag([0.1, 0.2]), 3)
    assert 0 < np.abs(f.x - before).max() < 0.5 and np.all(np.diag(f.rows(0, x.size)) <= np.diag(P) + 1e-15)


# ------------------------------------------------------------------------------------------------------------------
# the trajectory log
# ------------------------------------------------------------------------------------------------------------------
class _Replayed:
    def __init__(self):
        self.calls = []

    def predict(self, u):
        self.calls.append(("predict",))

    def measure(self, *a):
        self.calls.append(("measure",))

    def remove_landmarks(self, idx):
        self.calls.append(("remove", list(idx)))

    def observe_linear(self, z, R, Hr, landmarks, Hl, gate, wrap, rows):
        self.calls.append(("observe", np.asarray(z).tolist(), np.asarray(R).tolist(), np.asarray(Hr).tolist(), list(landmarks),
                           [np.asarray(b).tolist() for b in Hl], gate, tuple(wrap), rows))


def _steps(log, n):
    for k in range(n):
        log.record([0.1, 1.0 + k], np.array([[1.0, 2.0, 3.0]]) if k % 2 else None, [1.0, 2.0], [[0.0, 1.0], [2.0, 3.0]])


def test_trajectory_format_four_round_trip_and_the_older_formats(tmp_path):
    from ekf_slam_amd.trajectory import FORMAT, FORMAT_BATCH, FORMAT_EDITS, FORMAT_OBSERVE, TrajectoryLog
    assert FORMAT_OBSERVE == "ekfslam-trajectory-4"
    base_keys = {"format", "u", "obs_ptr", "obs", "lm_ptr", "lm_index", "lm_loc"}
    edit_keys = base_keys | {"edit_step", "edit_kind", "edit_ptr", "edit_idx", "edit_delta", "edit_R"}
    # logs without an observation are written as versions 1 - 3, with the arrays they always had
    one = TrajectoryLog(); _steps(one, 3)
    two = TrajectoryLog(); _steps(two, 2); two.record_edit("constrain", [1, 2], [0.5, 0.0], RPOS)
    three = TrajectoryLog(); _steps(three, 2); three.record_edit("merge_batch", [3, 5, 1, 2])
    for log, name, fmt, keys in ((one, "one", FORMAT, base_keys), (two, "two", FORMAT_EDITS, edit_keys), (three, "three", FORMAT_BATCH, edit_keys)):
        log.save(tmp_path / (name + ".npz"))
        g = np.load(tmp_path / (name + ".npz"))
        assert str(g["format"]) == fmt and set(g.files) == keys
        back = TrajectoryLog.load(tmp_path / (name + ".npz"))
        assert len(back) == len(log) and len(back.edits) == len(log.edits) and back.observations == {}
    # version 4: observations among the other edits
    Hr = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    Hl = [np.array([[1.0, 2.0], [3.0, 4.0]]), -np.eye(2)]
    four = TrajectoryLog(); _steps(four, 2)
    four.record_edit("remove", [7])
    four.record_observation([1.0, 2.0], RPOS, Hr, [4, 2], Hl, gate=9.21, wrap=(0, 1), rows=2)
    _steps(four, 2)
    four.record_observation([175.0], [[0.5, 0.0], [0.0, 0.0]], [[0.0, 0.0, 1.0], [0.0, 0.0, 0.0]], wrap=(1, 0), rows=1)
    four.save(tmp_path / "four.npz")
    g = np.load(tmp_path / "four.npz")
    assert str(g["format"]) == FORMAT_OBSERVE and g["edit_kind"].tolist() == [0, 4, 4] and g["observe_edit"].tolist() == [1, 2]
    assert set(g.files) == edit_keys | {"observe_edit", "observe_Hr", "observe_Hl", "observe_gate", "observe_wrap", "observe_rows"}
    back = TrajectoryLog.load(tmp_path / "four.npz")
    assert len(back) == 4 and [(e[0], e[1], e[2].tolist()) for e in back.edits] == [(2, "remove", [7]), (2, "observe", [4, 2]), (4, "observe", [])]
    np.testing.assert_array_equal(back.edits[1][3], [1.0, 2.0]); np.testing.assert_array_equal(back.edits[1][4], RPOS)
    o = back.observations[1]
    np.testing.assert_array_equal(o["Hr"], Hr); np.testing.assert_array_equal(o["Hl"], np.array(Hl))
    assert o["gate"] == 9.21 and o["wrap"].tolist() == [0, 1] and o["rows"] == 2 and back.observations[2]["gate"] == float("inf")
    r = _Replayed()
    back.replay(r)
    assert r.calls == [("predict",), ("predict",), ("measure",), ("remove", [6]),
                       ("observe", [1.0, 2.0], RPOS.tolist(), Hr.tolist(), [3, 1], [Hl[0].tolist(), Hl[1].tolist()], 9.21, (0, 1), 2),
                       ("predict",), ("predict",), ("measure",),
                       ("observe", [175.0], [[0.5, 0.0], [0.0, 0.0]], [[0.0, 0.0, 1.0], [0.0, 0.0, 0.0]], [], [], float("inf"), (1, 0), 1)]
    # bad shapes are refused and nothing is recorded
    bad = TrajectoryLog()
    for kw in (dict(landmarks=[1.5], Hl=[np.eye(2)]), dict(landmarks=[1, 2, 3], Hl=[np.eye(2)] * 3), dict(landmarks=[1], Hl=[]), dict(rows=3)):
        with pytest.raises(ValueError):
            bad.record_observation([0.0, 0.0], RPOS, **kw)
    with pytest.raises(ValueError):
        bad.record_edit("observe", [1])                       # observations have their own recorder
    assert bad.edits == [] and bad.observations == {}


# ------------------------------------------------------------------------------------------------------------------
# the Python layers over a stand-in for the library
# ------------------------------------------------------------------------------------------------------------------
class _Recorder(RecorderBase):
    last_error = b"observe_linear: injected"

    def __init__(self):
        self.calls, self.fail = [], 0

    def _note(self, name, pobs, pres):
        o = pobs._obj
        self.calls.append((name, list(o.z), list(o.R), list(o.Hr), list(o.lm), [list(o.Hl[0]), list(o.Hl[1])], o.gate, list(o.wrap_deg), o.rows,
                           pres is not None))
        if self.fail:
            return self.fail
        if pres is not None:
            r = pres._obj
            r.nu[0], r.nu[1] = 0.5, -0.25
            r.S[0], r.S[1], r.S[2], r.S[3] = 1.0, 2.0, 3.0, 4.0
            r.d2, r.outcome = 1.5, 2
        return 0

    def ekf_observe_linear(self, h, pobs, pres):
        return self._note("observe", pobs, pres)

    def ekf_linear_innovation(self, h, pobs, pres):
        return self._note("innovation", pobs, pres)

    def ekf_linear_rejections(self, h, pa, pb):
        pa._obj.value, pb._obj.value = 3, 4
        return 0


def test_engine_and_slam_layers_marshal_an_observation_once(monkeypatch):
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import engine as E
    from ekf_slam_amd import slam as S
    from ekf_slam_amd.trajectory import TrajectoryLog
    inf = float("inf")
    rec = _Recorder()
    monkeypatch.setattr(L, "lib", lambda: rec)
    e = E.Engine(capacity=16)
    Hr = [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]
    Hl = [[[1.0, 2.0], [3.0, 4.0]], [[5.0, 6.0], [7.0, 8.0]]]
    assert e.observe_linear([1.0, 2.0], [[0.5, 0.1], [0.1, 0.25]], Hr, [4, 2], Hl, gate=9.0, wrap=(0, 1)) is None
    # column-major blocks, 0-based landmarks, no result asked for
    assert rec.calls[-1] == ("observe", [1.0, 2.0], [0.5, 0.1, 0.1, 0.25], [1.0, 4.0, 2.0, 5.0, 3.0, 6.0], [4, 2],
                             [[1.0, 3.0, 2.0, 4.0], [5.0, 7.0, 6.0, 8.0]], 9.0, [0, 1], 2, False)
    out = e.observe_linear([1.0, 2.0], np.eye(2), Hr, wait=True)
    assert rec.calls[-1][4] == [-1, -1] and rec.calls[-1][-1] is True and rec.calls[-1][6] == inf
    assert out["nu"].tolist() == [0.5, -0.25] and out["S"].tolist() == [[1.0, 3.0], [2.0, 4.0]] and out["d2"] == 1.5 and out["outcome"] == L.EKF_LINEAR_GATED
    assert e.linear_innovation([7.0], 0.5, [0.0, 0.0, 1.0], wrap=(1, 0), rows=1)["d2"] == 1.5
    assert rec.calls[-1] == ("innovation", [7.0, 0.0], [0.5, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0, 1.0, 0.0], [-1, -1], [[0.0] * 4, [0.0] * 4],
                             inf, [1, 0], 1, True)
    assert e.linear_rejections() == (3, 4)
    n = len(rec.calls)
    for bad in (dict(rows=3), dict(landmarks=[1, 2, 3], Hl=[np.eye(2)] * 3), dict(landmarks=[1], Hl=[]), dict(Hr=[1.0, 2.0]),
                dict(landmarks=[1], Hl=[[1.0, 2.0, 3.0]])):
        with pytest.raises(ValueError):
            e.observe_linear([1.0, 2.0], np.eye(2), **bad)
    with pytest.raises(ValueError):
        e.observe_linear([1.0], np.eye(2))                   # two rows need two values
    with pytest.raises(ValueError):
        e.observe_linear([1.0, 2.0], [1.0, 2.0, 3.0])
    assert len(rec.calls) == n
    for cls in (S.EKF_SLAM, S.EKF_SLAM_UC):
        rec = _Recorder()
        monkeypatch.setattr(L, "lib", lambda: rec)
        f = cls(capacity=16)
        f.log = TrajectoryLog()
        f.fix_landmark(5, [1.0, 2.0], RPOS, gate=6.0)         # 1-based here: reaches the library as landmark 4
        assert rec.calls[-1] == ("observe", [1.0, 2.0], [0.02, 0.005, 0.005, 0.03], [0.0] * 6, [4, -1], [[1.0, 0.0, 0.0, 1.0], [0.0] * 4], 6.0, [0, 0], 2, False)
        f.fix_robot_position([3.0, 4.0], RPOS)
        assert rec.calls[-1][3] == [1.0, 0.0, 0.0, 1.0, 0.0, 0.0] and rec.calls[-1][4] == [-1, -1] and rec.calls[-1][6] == inf
        assert f.fix_robot_heading(-179.0, 0.5, wait=True)["outcome"] == 2
        assert rec.calls[-1] == ("observe", [-179.0, 0.0], [0.5, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0, 1.0, 0.0], [-1, -1], [[0.0] * 4, [0.0] * 4], inf,
                                 [1, 0], 1, True)
        f.observe_linear([0.0, 0.0], None, None, [2, 7], [np.eye(2), -np.eye(2)])
        assert rec.calls[-1][4] == [1, 6] and rec.calls[-1][2] == [0.0] * 4
        assert [(k, kind, idx.tolist()) for k, kind, idx, _, _ in f.log.edits] == [(0, "observe", [5]), (0, "observe", []), (0, "observe", []),
                                                                                 (0, "observe", [2, 7])]
        assert f.log.observations[2]["rows"] == 1 and f.log.observations[2]["wrap"].tolist() == [1, 0] and f.log.observations[0]["gate"] == 6.0
        np.testing.assert_array_equal(f.log.observations[3]["Hl"], [np.eye(2), -np.eye(2)])
        n = len(rec.calls)
        with pytest.raises(ValueError):
            f.fix_landmark(1.5, [1.0, 2.0], RPOS)
        with pytest.raises(ValueError):
            f.observe_linear([0.0, 0.0], RPOS, None, [2.5], [np.eye(2)])
        with pytest.raises(ValueError):
            f.fix_robot_position([1.0, 2.0, 3.0], RPOS)
        assert len(rec.calls) == n and len(f.log.edits) == 4
        # a refused call raises and is not logged
        rec.fail = L.EKF_ERR_STATE
        with pytest.raises(L.EkfError) as info:
            f.fix_landmark(1, [0.0, 0.0], None, wait=True)
        assert info.value.status == L.EKF_ERR_STATE and "observe_linear" in str(info.value) and len(f.log.edits) == 4
        # the log holds what the library received, field by field: the four calls above and one with every block general
        rec.fail = 0
        f.observe_linear([1.5, -2.5], [[0.5, 0.1], [0.2, 0.25]], Hr, [4, 2], Hl, gate=9.0, wrap=(0, 1))
        sent = [c for c in rec.calls if c[0] == "observe"]
        del sent[4]                                           # the refused one
        assert len(sent) == len(f.log.edits) == 5 and sent[4][3] == [1.0, 4.0, 2.0, 5.0, 3.0, 6.0] and sent[4][2] == [0.5, 0.2, 0.1, 0.25]
        for (_, z, Rc, Hrc, lm, Hlc, gate, wrap, rows, _), (_, _, idx, zl, Rl), q in zip(sent, f.log.edits, range(5)):
            o = f.log.observations[q]
            assert zl.tolist() == z and Rl.reshape(-1, order="F").tolist() == Rc and o["Hr"].reshape(-1, order="F").tolist() == Hrc
            assert [k - 1 for k in idx.tolist()] + [-1] * (2 - idx.size) == lm
            assert [o["Hl"][b].reshape(-1, order="F").tolist() for b in range(2)] == Hlc
            assert (o["gate"], o["wrap"].tolist(), o["rows"]) == (gate, wrap, rows)
