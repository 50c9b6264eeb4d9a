"""CPU: the observation models of ekf_observe_model (tests/model_obs_cases.py: hand-derived answers; the compiled ekfm::model_eval of
ekf_slam_amd/csrc/device_math.h against the closed forms and finite differences), the sixth kind of the trajectory log, and the argument
handling of the Python layers over a stand-in for the library.  No GPU."""
import subprocess

import numpy as np
import pytest

import model_obs_cases as M
from helpers import RPOS, RecorderBase, host_build, line_program, same_npz

INF = float("inf")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """The stand-alone host build of ekfm::model_eval / model_small: host(lines) -> one list of floats per line."""
    return line_program(tmp_path_factory, "model_eval_host")


def eval_line(model, xr, t0, t1=None, anchored=False):
    t1 = [0.0, 0.0] if t1 is None else t1
    return "eval %d %d %s" % (model, 0 if anchored else 1, M.fmt(list(xr) + ([0.0, 0.0] if anchored else list(t0)) + list(t1) + list(t0 if anchored else [0.0, 0.0])))


# ------------------------------------------------------------------------------------------------------------------
# hand-derived answers
# ------------------------------------------------------------------------------------------------------------------
def test_a_range_of_six_to_a_landmark_five_away(host):
    # robot at the origin, theta = 0, Prr = I3; landmark at (3, 4), block I2, uncorrelated; range 6 observed with variance 2:
    #   e = (0.6, 0.8), H = [-e, 0, e]; S = e'e + e'e + 2 = 4; nu = 6 - 5 = 1; d2 = 1/4; K = P H' / S = (-e, 0, e) / 4
    x = np.array([0.0, 0.0, 0.0, 3.0, 4.0])
    P = np.eye(5)
    o = M.obs(M.RANGE, [6.0], 2.0, [0])
    hx, H = M.jacobian(x, o)
    assert hx[0] == 5.0 and H[0].tolist() == [-0.6, -0.8, 0.0, 0.6, 0.8] and not H[1].any()
    x2, P2, res = M.observe_model_dense(x, P, o)
    assert res["outcome"] == M.APPLIED and res["nu"].tolist() == [1.0, 0.0] and res["d2"] == pytest.approx(0.25, abs=1e-15)
    np.testing.assert_allclose(res["S"], [[4.0, 0.0], [0.0, 1.0]], atol=1e-15)
    np.testing.assert_allclose(x2, [-0.15, -0.2, 0.0, 3.15, 4.2], atol=1e-15)
    # the compiled function: the same H bit for bit (3/5 and 4/5 are correctly rounded divisions), S, nu, d2
    ev, sm = host([eval_line(M.RANGE, x[:3], x[3:5]), M.small_line(o, x, P)])
    assert ev[0] == 1 and ev[1:3] == [5.0, 0.0] and ev[3:10] == [-0.6, -0.8, 0.0, 0.6, 0.8, 0.0, 0.0] and not any(ev[10:])
    assert sm[:2] == [1, 1] and sm[3:5] == [1.0, 0.0] and sm[2] == pytest.approx(0.25, abs=1e-15)
    np.testing.assert_allclose(sm[5:9], [4.0, 0.0, 0.0, 1.0], atol=1e-15)
    assert sm[6:9] == [0.0, 0.0, 1.0]                        # a one-row model: the second row is exactly empty
    np.testing.assert_allclose(sm[9:16], [-0.6, -0.8, 0.0, 0.6, 0.8, 0.0, 0.0], atol=1e-15)      # Gs row 0 = H P = H


def test_a_bearing_across_180_degrees_is_wrapped(host):
    # theta = 170, the landmark in direction -175 degrees: h = -345; z = 16 gives nu = 361 -> +1, not 361
    th = np.radians(-175.0)
    x = np.array([1.0, -2.0, 170.0, 1.0 + 10.0 * np.cos(th), -2.0 + 10.0 * np.sin(th)])
    P = np.diag([0.5, 0.5, 4.0, 1.0, 1.0])
    for model, z, row in ((M.BEARING, [16.0], 0), (M.RANGE_BEARING, [10.0, 16.0], 1)):
        o = M.obs(model, z, np.diag([0.1, 0.3]) if model == M.RANGE_BEARING else 0.3, [0])
        res = M.observe_model_dense(x, P, o)[2]
        assert res["nu"][row] == pytest.approx(1.0, abs=1e-12)
        sm = host([M.small_line(o, x, P)])[0]
        assert sm[1] == 1 and sm[3 + row] == pytest.approx(1.0, abs=1e-12)
        np.testing.assert_allclose(sm[5:9], res["S"].reshape(-1), rtol=0, atol=1e-13 * np.abs(res["S"]).max())
        assert sm[2] == pytest.approx(res["d2"], rel=1e-11)
    # an anchor as the target: the same h, no landmark block, only the robot is corrected
    o = M.obs(M.BEARING, [16.0], 0.3, anchor=x[3:5])
    x2, P2, res = M.observe_model_dense(x[:3], P[:3, :3], o)
    assert res["nu"][0] == pytest.approx(1.0, abs=1e-12) and x2[2] < 170.0       # dh/dtheta = -1: a larger bearing turns the robot back
    ev = host([eval_line(M.BEARING, x[:3], x[3:5], anchored=True)])[0]
    assert ev[0] == 1 and ev[5] == -1.0 and not any(ev[6:10]) and not any(ev[10:])


def test_relative_xy_at_exactly_ninety_degrees(host):
    # theta = 90: c = 0, s = 1 exactly; the robot at (1, 2) looks along +y: a target at (1 - 3, 2 + 5) lies 5 ahead and 3 to the left
    xr, t = [1.0, 2.0, 90.0], [-2.0, 7.0]
    assert M.h_of(M.RELATIVE_XY, xr, t).tolist() == [5.0, 3.0]
    H = M.H_of(M.RELATIVE_XY, xr, t)
    assert H[:, :2].tolist() == [[-0.0, -1.0], [1.0, -0.0]] and H[:, 3:5].tolist() == [[0.0, 1.0], [-1.0, 0.0]]
    assert H[0, 2] == 3.0 / M.K and H[1, 2] == -5.0 / M.K
    ev = host([eval_line(M.RELATIVE_XY, xr, t)])[0]
    assert ev[0] == 1 and ev[1:3] == [5.0, 3.0]
    np.testing.assert_array_equal(np.array(ev[3:]).reshape(2, 7), H)


# ------------------------------------------------------------------------------------------------------------------
# the compiled model_eval against the closed forms and finite differences
# ------------------------------------------------------------------------------------------------------------------
def _random_cases(rng, n):
    cases = []
    for _ in range(n):
        xr = np.array([rng.uniform(-30, 30), rng.uniform(-30, 30), rng.uniform(-720, 720)])
        t0 = xr[:2] + rng.uniform(1.0, 40.0) * np.array([np.cos(a := rng.uniform(0, 2 * np.pi)), np.sin(a)])
        t1 = t0 + rng.uniform(1.0, 40.0) * np.array([np.cos(b := rng.uniform(0, 2 * np.pi)), np.sin(b)])
        cases.append((xr, t0, t1))
    return cases


def test_compiled_model_eval_matches_closed_forms_and_finite_differences(host):
    rng = np.random.default_rng(21)
    cases = _random_cases(rng, 40)
    models = (M.RANGE_BEARING, M.RANGE, M.BEARING, M.RELATIVE_XY, M.LANDMARK_RANGE)
    # the finite-difference error of the NumPy forms themselves at step 1e-6, measured here: the yardstick for the compiled H
    fd_err = 0.0
    for xr, t0, t1 in cases:
        for m in models:
            t1m = t1 if m == M.LANDMARK_RANGE else None
            H = M.H_of(m, xr, t0, t1m)
            fd_err = max(fd_err, np.abs(M.H_fd(m, xr, t0, t1m) - H).max() / np.abs(H).max())
    print("finite differences (step 1e-6) against the NumPy closed forms: worst rel err %.2e" % fd_err)
    assert 0.0 < fd_err < 1e-6
    lines, keys = [], []
    for xr, t0, t1 in cases:
        for m in models:
            lines.append(eval_line(m, xr, t0, t1 if m == M.LANDMARK_RANGE else None)); keys.append((m, xr, t0, t1))
    worst_cf = worst_fd = worst_h = 0.0
    for (m, xr, t0, t1), row in zip(keys, host(lines)):
        t1m = t1 if m == M.LANDMARK_RANGE else None
        assert row[0] == 1
        hx, H = np.array(row[1:3]), np.array(row[3:]).reshape(2, 7)
        want_h, want_H = M.h_of(m, xr, t0, t1m), M.H_of(m, xr, t0, t1m)
        worst_h = max(worst_h, np.abs(M.wrap180(hx - want_h) if m in (M.RANGE_BEARING, M.BEARING) else hx - want_h).max() / max(np.abs(want_h).max(), 1.0))
        worst_cf = max(worst_cf, np.abs(H - want_H).max() / np.abs(want_H).max())
        worst_fd = max(worst_fd, np.abs(H - M.H_fd(m, xr, t0, t1m)).max() / np.abs(want_H).max())
        assert np.all((H == 0.0) == (want_H == 0.0)), m       # the blocks and rows a model does not have are exactly empty
    print("compiled model_eval: rel err h %.2e, H against the closed form %.2e, against finite differences %.2e" % (worst_h, worst_cf, worst_fd))
    assert worst_h < 1e-12 and worst_cf < 1e-12 and worst_fd < 10.0 * fd_err


def test_a_target_on_the_robot_is_irregular_and_finite(host):
    x = np.array([1.5, -2.5, 33.0, 1.5, -2.5, 1.5, -2.5])
    P = np.eye(7)
    lines = []
    for m in (M.RANGE_BEARING, M.RANGE, M.BEARING, M.RELATIVE_XY):
        lines.append(eval_line(m, x[:3], x[3:5]))
        lines.append(eval_line(m, x[:3], x[:2], anchored=True))
    lines.append(eval_line(M.LANDMARK_RANGE, x[:3], x[3:5], x[5:7]))
    lines.append(eval_line(M.RANGE, [INF, 0.0, 0.0], [1.0, 1.0]))
    lines.append(eval_line(M.BEARING, [0.0, 0.0, float("nan")], [1.0, 1.0]))
    for row in host(lines):
        assert row[0] == 0 and not any(row[1:])              # h and H are zero: nothing that is not finite leaves the function
    o = M.obs(M.RANGE, [1.0], 0.5, [0])
    sm = host([M.small_line(o, x, P), M.small_line(M.obs(M.RANGE_BEARING, [1.0, 2.0], RPOS, anchor=x[:2]), x[:3], P[:3, :3])])
    for row in sm:
        assert row[:2] == [0, 0] and np.isnan(row[2]) and np.all(np.isfinite(row[3:])) and not any(row[9:])
    x2, P2, res = M.observe_model_dense(x, P, o)
    assert res["outcome"] == M.IRREGULAR and np.isnan(res["d2"])
    np.testing.assert_array_equal(x2, x); np.testing.assert_array_equal(P2, P)


def test_dense_update_with_a_model_is_the_linear_update_with_its_jacobian():
    import linear_obs_cases as C
    rng = np.random.default_rng(5)
    x, P, _ = C.random_state(rng, 6)
    for o in (M.obs(M.RANGE_BEARING, [0.0, 0.0], RPOS, [2]), M.obs(M.RELATIVE_XY, [0.0, 0.0], RPOS, [5]), M.obs(M.LANDMARK_RANGE, [0.0], 0.1, [4, 1]),
              M.obs(M.BEARING, [0.0], 0.2, anchor=[40.0, -3.0]), M.obs(M.RANGE, [0.0], 0.2, [0], gate=1e-9)):
        hx, H = M.jacobian(x, o)
        o["z"][:o["rows"]] = hx[:o["rows"]] + 0.3 * rng.standard_normal(o["rows"])
        lin = C.obs(o["z"] - hx + H @ x, o["R"], H[:, :3], o["landmarks"], [H[:, 3 + 2 * k:5 + 2 * k] for k in o["landmarks"]], gate=o["gate"], rows=2)
        lin["R"] = M.effective_R(o)
        xm, Pm, rm = M.observe_model_dense(x, P, o)
        xl, Pl, rl = C.observe_dense(x, P, lin)
        assert rm["outcome"] == rl["outcome"] == (M.GATED if o["gate"] < 1.0 else M.APPLIED)
        np.testing.assert_allclose(xm, xl, rtol=0, atol=1e-12 * np.abs(x).max())
        np.testing.assert_array_equal(Pm, Pl)


# ------------------------------------------------------------------------------------------------------------------
# the kernel sources, compiled for the host
# ------------------------------------------------------------------------------------------------------------------
def test_kernel_sources_on_the_host_match_the_linear_gather_bit_for_bit(tmp_path):
    """tests/support/model_obs_host_emulation.cpp: k_gather_model against k_gather_linear handed the Jacobian model_eval gives the host,
    with 0 and 3 pairs pending, tiles of edge 16 and 64; k_model_probe against the launch; a target on the robot as a finite no-op."""
    exe = host_build("model_obs_host_emulation", str(tmp_path / "model_obs_host_emulation"))
    r = subprocess.run([exe], capture_output=True, text=True)
    lines = r.stdout.strip().split("\n")
    assert r.returncode == 0, r.stdout[-3000:]
    assert len(lines) == 36 and all(ln.endswith(": 0 differences") for ln in lines), r.stdout[-3000:]


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
        self.calls.append(("observe", np.asarray(z).tolist(), list(landmarks), rows))

    def observe_model(self, model, z, R, landmarks, anchor=None, gate=INF):
        self.calls.append(("observe_model", model, np.asarray(z).tolist(), np.asarray(R).tolist(), list(landmarks),
                           None if anchor is None else np.asarray(anchor).tolist(), gate))


def _steps(log, n):
    for k in range(n):
        log.record([0.1, 1.0 + k], np.array([[1.0, 2.0, 3.0]]) if k % 2 else None, [1.0, 2.0], [[0.0, 1.0], [2.0, 3.0]])


def test_trajectory_format_five_round_trip_and_the_older_formats(tmp_path):
    from ekf_slam_amd.trajectory import FORMAT, FORMAT_BATCH, FORMAT_EDITS, FORMAT_MODEL, FORMAT_OBSERVE, TrajectoryLog
    assert FORMAT_MODEL == "ekfslam-trajectory-5"
    base_keys = {"format", "u", "obs_ptr", "obs", "lm_ptr", "lm_index", "lm_loc"}
    edit_keys = base_keys | {"edit_step", "edit_kind", "edit_ptr", "edit_idx", "edit_delta", "edit_R"}
    observe_keys = edit_keys | {"observe_edit", "observe_Hr", "observe_Hl", "observe_gate", "observe_wrap", "observe_rows"}
    # logs without a model observation are written as versions 1 - 4, with the arrays they always had, and a loaded one saves
    # byte for byte what it was loaded from
    one = TrajectoryLog(); _steps(one, 3)
    two = TrajectoryLog(); _steps(two, 2); two.record_edit("constrain", [1, 2], [0.5, 0.0], RPOS)
    three = TrajectoryLog(); _steps(three, 2); three.record_edit("merge_batch", [3, 5, 1, 2])
    four = TrajectoryLog(); _steps(four, 2); four.record_edit("remove", [7])
    four.record_observation([1.0, 2.0], RPOS, np.ones((2, 3)), [4, 2], [np.eye(2), -np.eye(2)], gate=9.21, wrap=(0, 1), rows=2)
    for log, name, fmt, keys in ((one, "one", FORMAT, base_keys), (two, "two", FORMAT_EDITS, edit_keys), (three, "three", FORMAT_BATCH, edit_keys),
                                 (four, "four", FORMAT_OBSERVE, observe_keys)):
        log.save(tmp_path / (name + ".npz"))
        g = np.load(tmp_path / (name + ".npz"))
        assert str(g["format"]) == fmt and set(g.files) == keys
        back = TrajectoryLog.load(tmp_path / (name + ".npz"))
        assert len(back) == len(log) and len(back.edits) == len(log.edits) and back.model_observations == {}
        back.save(tmp_path / (name + "_again.npz"))
        assert same_npz(tmp_path / (name + ".npz"), tmp_path / (name + "_again.npz"))
    # version 5: model observations among the other edits, with and without linear ones
    five = TrajectoryLog(); _steps(five, 2)
    five.record_edit("remove", [7])
    five.record_model_observation(M.RANGE_BEARING, [5.0, 30.0], RPOS, [4], gate=9.21)
    five.record_observation([175.0], [[0.5, 0.0], [0.0, 0.0]], [[0.0, 0.0, 1.0], [0.0, 0.0, 0.0]], wrap=(1, 0), rows=1)
    _steps(five, 2)
    five.record_model_observation(M.RANGE, [7.5], [[0.5, 0.0], [0.0, 0.0]], anchor=[10.0, -4.0])
    five.record_model_observation(M.LANDMARK_RANGE, [2.5], [[0.1, 0.0], [0.0, 0.0]], [3, 9], gate=4.0)
    five.save(tmp_path / "five.npz")
    g = np.load(tmp_path / "five.npz")
    assert str(g["format"]) == FORMAT_MODEL and g["edit_kind"].tolist() == [0, 5, 4, 5, 5]
    assert g["model_edit"].tolist() == [1, 3, 4] and g["model_id"].tolist() == [1, 2, 5] and g["observe_edit"].tolist() == [2]
    assert set(g.files) == observe_keys | {"model_edit", "model_id", "model_anchor", "model_gate"}
    back = TrajectoryLog.load(tmp_path / "five.npz")
    assert len(back) == 4 and [(e[0], e[1], e[2].tolist()) for e in back.edits] == \
        [(2, "remove", [7]), (2, "observe_model", [4]), (2, "observe", []), (4, "observe_model", []), (4, "observe_model", [3, 9])]
    assert back.model_observations[1] == dict(model=1, anchor=None, gate=9.21) and back.model_observations[4]["gate"] == 4.0
    assert back.model_observations[3]["anchor"].tolist() == [10.0, -4.0] and back.model_observations[3]["gate"] == INF
    np.testing.assert_array_equal(back.edits[1][3], [5.0, 30.0]); np.testing.assert_array_equal(back.edits[1][4], RPOS)
    back.save(tmp_path / "five_again.npz")
    assert same_npz(tmp_path / "five.npz", tmp_path / "five_again.npz")
    r = _Replayed()
    back.replay(r)
    assert r.calls == [("predict",), ("predict",), ("measure",), ("remove", [6]),
                       ("observe_model", 1, [5.0, 30.0], RPOS.tolist(), [3], None, 9.21), ("observe", [175.0], [], 1),
                       ("predict",), ("predict",), ("measure",),
                       ("observe_model", 2, [7.5, 0.0], [[0.5, 0.0], [0.0, 0.0]], [], [10.0, -4.0], INF),
                       ("observe_model", 5, [2.5, 0.0], [[0.1, 0.0], [0.0, 0.0]], [2, 8], None, 4.0)]
    only = TrajectoryLog(); _steps(only, 1)
    only.record_model_observation(M.BEARING, [12.0], [[0.3, 0.0], [0.0, 0.0]], [2])
    only.save(tmp_path / "only.npz")
    back = TrajectoryLog.load(tmp_path / "only.npz")
    assert str(np.load(tmp_path / "only.npz")["format"]) == FORMAT_MODEL and back.observations == {} and list(back.model_observations) == [0]
    # bad shapes are refused and nothing is recorded
    bad = TrajectoryLog()
    for kw in (dict(landmarks=[1.5]), dict(landmarks=[1, 2, 3])):
        with pytest.raises(ValueError):
            bad.record_model_observation(M.RANGE, [1.0], None, **kw)
    with pytest.raises(ValueError):
        bad.record_edit("observe_model", [1])                 # model observations have their own recorder
    assert bad.edits == [] and bad.model_observations == {}


# ------------------------------------------------------------------------------------------------------------------
# the Python layers over a stand-in for the library
# ------------------------------------------------------------------------------------------------------------------
class _Recorder(RecorderBase):
    last_error = b"observe_model: injected"

    def __init__(self):
        self.calls, self.fail = [], 0

    def _note(self, name, pobs, pres):
        o = pobs._obj
        self.calls.append((name, o.model, list(o.z), list(o.R), list(o.lm), list(o.anchor), o.gate, pres is not None))
        if self.fail:
            return self.fail
        if pres is not None:
            r = pres._obj
            r.nu[0], r.nu[1] = 0.5, -0.25
            r.S[0], r.S[1], r.S[2], r.S[3] = 1.0, 2.0, 3.0, 4.0
            r.d2, r.outcome = 1.5, 2
        return 0

    def ekf_observe_model(self, h, pobs, pres):
        return self._note("observe", pobs, pres)

    def ekf_model_innovation(self, h, pobs, pres):
        return self._note("innovation", pobs, pres)

    def ekf_model_evaluate(self, model, xr, t0, t1, hx, H):
        self.calls.append(("evaluate", model, [xr[i] for i in range(3)], [t0[0], t0[1]], None if not t1 else [t1[0], t1[1]]))
        hx[0], H[13] = 7.0, 9.0
        return self.fail


def test_engine_and_slam_layers_marshal_a_model_observation_once(monkeypatch):
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import engine as E
    from ekf_slam_amd import slam as S
    from ekf_slam_amd.trajectory import TrajectoryLog
    rec = _Recorder()
    monkeypatch.setattr(L, "lib", lambda: rec)
    e = E.Engine(capacity=16)
    assert e.observe_model(L.EKF_MODEL_RANGE_BEARING, [5.0, 30.0], [[0.5, 0.1], [0.1, 0.25]], [4], gate=9.0) is None
    assert rec.calls[-1] == ("observe", 1, [5.0, 30.0], [0.5, 0.1, 0.1, 0.25], [4, -1], [0.0, 0.0], 9.0, False)
    out = e.observe_model(L.EKF_MODEL_RANGE, [7.5], 0.5, anchor=[10.0, -4.0], wait=True)
    assert rec.calls[-1] == ("observe", 2, [7.5, 0.0], [0.5, 0.0, 0.0, 0.0], [-1, -1], [10.0, -4.0], INF, True)
    assert out["nu"].tolist() == [0.5, -0.25] and out["S"].tolist() == [[1.0, 3.0], [2.0, 4.0]] and out["d2"] == 1.5 and out["outcome"] == L.EKF_LINEAR_GATED
    assert e.model_innovation(L.EKF_MODEL_LANDMARK_RANGE, [2.5], 0.1, [3, 9])["d2"] == 1.5
    assert rec.calls[-1] == ("innovation", 5, [2.5, 0.0], [0.1, 0.0, 0.0, 0.0], [3, 9], [0.0, 0.0], INF, True)
    hx, H = E.Engine.model_evaluate(L.EKF_MODEL_BEARING, [1.0, 2.0, 3.0], [4.0, 5.0])
    assert rec.calls[-1] == ("evaluate", 3, [1.0, 2.0, 3.0], [4.0, 5.0], None) and hx[0] == 7.0 and H.shape == (2, 7) and H[1, 6] == 9.0
    E.Engine.model_evaluate(L.EKF_MODEL_LANDMARK_RANGE, [1.0, 2.0, 3.0], [4.0, 5.0], [6.0, 7.0])
    assert rec.calls[-1][4] == [6.0, 7.0]
    n = len(rec.calls)
    for bad in (dict(model=0), dict(model=6), dict(z=[1.0]), dict(landmarks=[1, 2, 3]), dict(landmarks=[1], anchor=[0.0, 0.0]), dict(landmarks=[]),
                dict(landmarks=[], anchor=[1.0, 2.0, 3.0]), dict(R=[1.0, 2.0, 3.0])):
        kw = dict(model=1, z=[1.0, 2.0], R=np.eye(2), landmarks=[1]); kw.update(bad)
        with pytest.raises(ValueError):
            e.observe_model(**kw)
    assert len(rec.calls) == n
    for cls in (S.EKF_SLAM, S.EKF_SLAM_UC):
        rec = _Recorder()
        monkeypatch.setattr(L, "lib", lambda: rec)
        f = cls(capacity=16)
        f.log = TrajectoryLog()
        f.observe_range_bearing(5, [5.0, 30.0], RPOS, gate=6.0)                 # 1-based here: reaches the library as landmark 4
        assert rec.calls[-1] == ("observe", 1, [5.0, 30.0], [0.02, 0.005, 0.005, 0.03], [4, -1], [0.0, 0.0], 6.0, False)
        f.observe_range(2, 7.5, 0.5)
        assert rec.calls[-1] == ("observe", 2, [7.5, 0.0], [0.5, 0.0, 0.0, 0.0], [1, -1], [0.0, 0.0], INF, False)
        assert f.observe_bearing(3, -12.0, 0.3, wait=True)["outcome"] == 2
        assert rec.calls[-1] == ("observe", 3, [-12.0, 0.0], [0.3, 0.0, 0.0, 0.0], [2, -1], [0.0, 0.0], INF, True)
        f.observe_relative_xy(1, [2.0, -1.0], RPOS)
        assert rec.calls[-1][1] == 4 and rec.calls[-1][4] == [0, -1]
        f.observe_landmark_range(2, 7, 2.5, 0.1, gate=4.0)
        assert rec.calls[-1] == ("observe", 5, [2.5, 0.0], [0.1, 0.0, 0.0, 0.0], [1, 6], [0.0, 0.0], 4.0, False)
        f.observe_anchor_range([10.0, -4.0], 7.5, 0.5)
        assert rec.calls[-1] == ("observe", 2, [7.5, 0.0], [0.5, 0.0, 0.0, 0.0], [-1, -1], [10.0, -4.0], INF, False)
        f.observe_anchor_bearing([10.0, -4.0], 33.0, 0.2)
        assert rec.calls[-1][1] == 3 and rec.calls[-1][5] == [10.0, -4.0]
        assert f.model_innovation(L.EKF_MODEL_RANGE, [1.0], 0.5, [6])["d2"] == 1.5 and rec.calls[-1][0] == "innovation" and rec.calls[-1][4] == [5, -1]
        assert [(k, kind, idx.tolist()) for k, kind, idx, _, _ in f.log.edits] == \
            [(0, "observe_model", [5]), (0, "observe_model", [2]), (0, "observe_model", [3]), (0, "observe_model", [1]), (0, "observe_model", [2, 7]),
             (0, "observe_model", []), (0, "observe_model", [])]
        assert f.log.model_observations[0] == dict(model=1, anchor=None, gate=6.0) and f.log.model_observations[5]["anchor"].tolist() == [10.0, -4.0]
        n = len(rec.calls)
        with pytest.raises(ValueError):
            f.observe_range(1.5, 2.0, 0.5)
        with pytest.raises(ValueError):
            f.observe_landmark_range(2, 2.5, 1.0, 0.5)
        with pytest.raises(ValueError):
            f.observe_anchor_range([1.0, 2.0, 3.0], 1.0, 0.5)
        assert len(rec.calls) == n and len(f.log.edits) == 7
        # a refused call raises and is not logged
        rec.fail = L.EKF_ERR_STATE
        with pytest.raises(L.EkfError) as info:
            f.observe_range(1, 0.0, 0.5, wait=True)
        assert info.value.status == L.EKF_ERR_STATE and "observe_model" in str(info.value) and len(f.log.edits) == 7
        # the log holds what the library received, field by field: the seven calls above and one with a general R
        rec.fail = 0
        f.observe_model(L.EKF_MODEL_RELATIVE_XY, [1.5, -2.5], [[0.5, 0.1], [0.2, 0.25]], [4], gate=9.0)
        sent = [c for c in rec.calls if c[0] == "observe"]
        del sent[7]                                           # the refused one
        assert len(sent) == len(f.log.edits) == 8 and sent[7][3] == [0.5, 0.2, 0.1, 0.25]
        for (_, model, z, Rc, lm, anchor, gate, _), (_, _, idx, zl, Rl), q in zip(sent, f.log.edits, range(8)):
            o = f.log.model_observations[q]
            assert zl.tolist() == z and Rl.reshape(-1, order="F").tolist() == Rc and (o["model"], o["gate"]) == (model, gate)
            assert [k - 1 for k in idx.tolist()] + [-1] * (2 - idx.size) == lm
            assert (anchor == [0.0, 0.0] and o["anchor"] is None) if idx.size else o["anchor"].tolist() == anchor
