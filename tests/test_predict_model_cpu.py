"""CPU: ekf_predict_model without a GPU -- the compiled ekfm::motion_eval of ekf_slam_amd/csrc/device_math.h against hand-derived answers,
the radian restatement of tests/predict_model_cases.py and finite differences; g = sin a / a and g' against mpmath across the series
switch; the known answer of a heading variance turned into a lateral one; k_predict_model's source compiled for the host (a chain against
single launches bit for bit, every case against the dense restatement); the eighth kind of the trajectory log; the argument handling of the
Python layers over a stand-in for the library.  (The MEX gateway's command: tests/test_predict_model_mex_cpu.py.)"""
import ctypes
import subprocess

import numpy as np
import pytest

import predict_model_cases as PM
from helpers import REL, RecorderBase, host_build, line_program, same_npz

M2 = np.array([[0.04, 0.01], [0.01, 0.09]])
M3 = np.array([[0.04, 0.01, 0.0], [0.01, 0.09, 0.02], [0.0, 0.02, 0.25]])


# ------------------------------------------------------------------------------------------------------------------
# the compiled motion_eval
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """The stand-alone host build of ekfm::motion_eval / motion_chord / motion_noise_entry: host(lines) -> one row of floats per line."""
    return line_program(tmp_path_factory, "motion_eval_host")


def _eval(host, cases):
    lines = ["eval %d %s" % (m, " ".join(repr(float(v)) for v in list(xr) + (list(u) + [0.0])[:3])) for m, xr, u in cases]
    return [dict(ok=r[0] == 1, x=np.array(r[1:4]), fa=r[4], fb=r[5], V=np.array(r[6:15]).reshape(3, 3)) for r in host(lines)]


def test_hand_derived_answers_at_right_angles(host):
    k = PM.K
    td, pd, arc0, circle, half = _eval(host, [(PM.TURN_DRIVE, [1.0, 2.0, 90.0], [5.0, 0.0]), (PM.POSE_DELTA, [1.0, 2.0, 90.0], [5.0, 3.0, 270.0]),
                                              (PM.ARC, [1.0, 2.0, 90.0], [5.0, 0.0]), (PM.ARC, [1.0, 2.0, 30.0], [5.0, 360.0]),
                                              (PM.ARC, [0.0, 0.0, 0.0], [np.pi, 180.0])])
    # heading +y, drive 5: (1, 7); turning the robot moves the end point along -x, by 5 per radian
    assert td["ok"] and td["x"].tolist() == [1.0, 7.0, 90.0] and [td["fa"], td["fb"]] == [-5.0 / k, 0.0]
    assert td["V"].tolist() == [[0.0, -5.0 / k, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]
    # 5 ahead and 3 to the left of a robot that looks along +y is (1 - 3, 2 + 5); 90 + 270 = 360 stays 360 (wrapTo360)
    assert pd["ok"] and pd["x"].tolist() == [-2.0, 7.0, 360.0] and [pd["fa"], pd["fb"]] == [-5.0 / k, -3.0 / k]
    assert pd["V"].tolist() == [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]
    # an arc that does not turn is the straight line: g = 1, g' = 0, and a turn moves the end point sideways by d / 2 per radian
    assert arc0["ok"] and arc0["x"].tolist() == [1.0, 7.0, 90.0] and [arc0["fa"], arc0["fb"]] == [-5.0 / k, 0.0]
    assert arc0["V"].tolist() == [[0.0, -5.0 / (2.0 * k), 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]
    # a whole circle ends where it began: the chord is exactly 0 (sind(180) = 0), and so is the heading column of F
    assert circle["ok"] and circle["x"].tolist() == [1.0, 2.0, 390.0 - 360.0] and [circle["fa"], circle["fb"]] == [0.0, 0.0]
    # half a circle of radius 1 from the origin, heading +x: ends at (0, 2)
    assert abs(half["x"][0]) < 1e-15 and abs(half["x"][1] - 2.0) < 1e-15 and half["x"][2] == 180.0
    for m in (0, 4, -1):
        assert not _eval(host, [(m, [1.0, 2.0, 3.0], [4.0, 5.0, 6.0])])[0]["ok"]


def _random_cases(rng, n):
    out = []
    for _ in range(n):
        xr = np.array([rng.uniform(-30, 30), rng.uniform(-30, 30), rng.uniform(0, 360)])
        out.append((PM.TURN_DRIVE, xr, np.array([rng.uniform(-3, 10), rng.uniform(-400, 400)])))
        out.append((PM.ARC, xr, np.array([rng.uniform(-3, 10), rng.uniform(-360, 360)])))
        out.append((PM.ARC, xr, np.array([rng.uniform(0.5, 10), rng.uniform(-1, 1) * 10.0 ** rng.uniform(-9, 1)])))      # the series
        out.append((PM.POSE_DELTA, xr, np.array([rng.uniform(-5, 5), rng.uniform(-5, 5), rng.uniform(-400, 400)])))
    return out


def test_the_restatement_arc_is_the_circle_and_its_jacobians_are_the_derivatives():
    rng = np.random.default_rng(5)
    worst = 0.0
    for model, xr, u in _random_cases(rng, 60):
        # (the circle's own form cancels as the turn goes to 0: its error is about 2 eps d / turn -- 3e-14 d at one degree)
        if model == PM.ARC and abs(u[1]) > 1.0:
            worst = max(worst, np.abs(PM.f_of(model, xr, u) - PM.arc_on_the_circle(xr, u)).max() / max(abs(u[0]), 1.0))
    print("ARC in chord form against the circle: worst err %.2e" % worst)
    assert worst < 1e-12


def test_compiled_motion_eval_matches_the_restatement_and_finite_differences(host):
    rng = np.random.default_rng(31)
    cases = _random_cases(rng, 60)
    fd_err = 0.0
    for m, xr, u in cases:                                    # the finite-difference error of the NumPy forms themselves: the yardstick
        F, V = PM.F_V_of(m, xr, u)
        fF, fV = PM.F_V_fd(m, xr, u)
        fd_err = max(fd_err, np.abs(fF - F).max() / np.abs(F).max(), np.abs(fV - V).max() / np.abs(V).max())
    print("finite differences (step 1e-5) against the NumPy closed forms: worst rel err %.2e" % fd_err)
    assert 0.0 < fd_err < 1e-6
    worst = dict(x=0.0, F=0.0, V=0.0, fd=0.0)
    for (m, xr, u), got in zip(cases, _eval(host, cases)):
        assert got["ok"]
        nu = PM.INPUTS[m]
        F = np.eye(3); F[0, 2], F[1, 2] = got["fa"], got["fb"]
        V = got["V"][:, :nu]
        assert not got["V"][:, nu:].any()
        wF, wV = PM.F_V_of(m, xr, u)
        fF, fV = PM.F_V_fd(m, xr, u)
        want = PM.f_of(m, xr, u)
        scale = max(np.abs(xr[:2]).max(), np.abs(u[:2]).max(), 1.0)
        worst["x"] = max(worst["x"], np.abs(got["x"][:2] - want[:2]).max() / scale, abs(got["x"][2] - PM.wrap360(want[2])) / 360.0)
        worst["F"] = max(worst["F"], np.abs(F - wF).max() / np.abs(wF).max())
        worst["V"] = max(worst["V"], np.abs(V - wV).max() / np.abs(wV).max())
        worst["fd"] = max(worst["fd"], np.abs(F - fF).max() / np.abs(wF).max(), np.abs(V - fV).max() / np.abs(wV).max())
    print("compiled motion_eval: rel err %s" % ", ".join("%s %.2e" % kv for kv in worst.items()))
    assert worst["x"] < 1e-12 and worst["F"] < 1e-12 and worst["V"] < 1e-12 and worst["fd"] < 10.0 * fd_err


def test_chord_factor_and_its_derivative_against_mpmath_across_the_series_switch(host):
    """g = sin a / a and g' = (a cos a - sin a) / a^2 as motion_eval forms them from the turn t (a = t / (2k), sin a = sind(t / 2)) against
    50 digits.  The bound is measured: twice the worst relative error of the closed forms above the switch, found by this test; the series
    side must stay below it."""
    import mpmath
    mpmath.mp.dps = 50
    switch = 0.5                                              # ekfm::kMotionSeries

    def a_of(turn):
        return host(["chord %r" % float(turn)])[0][0]
    # the turns whose a lies one ulp below the switch and at it, found by stepping the turn
    t = 2.0 * PM.K * switch
    while a_of(t) >= switch:
        t = np.nextafter(t, 0.0)
    below = t
    while a_of(t) < switch:
        t = np.nextafter(t, np.inf)
    at = t
    assert a_of(below) == np.nextafter(switch, 0.0) and a_of(at) == switch
    series = [s * 2.0 * PM.K * a for a in [1e-300, 1e-9] + list(np.logspace(-12, np.log10(0.49), 300)) for s in (1.0, -1.0)] + [below, -below, 0.0]
    closed = [s * 2.0 * PM.K * a for a in list(np.logspace(np.log10(0.51), np.log10(np.pi), 300)) for s in (1.0, -1.0)]
    closed += [at, -at, np.nextafter(at, np.inf), 180.0, -180.0, 360.0, -360.0]           # the switch and an ulp above it, a = pi / 2, a = pi
    rows = host(["chord %r" % float(v) for v in series + closed])

    def errors(turns, rows, side):
        worst_g = worst_gp = 0.0
        for turn, (a, g, gp) in zip(turns, rows):
            assert (abs(a) < switch) == (side == "series"), (turn, a)
            if turn == 0.0:
                assert (g, gp) == (1.0, 0.0)
                continue
            ae = mpmath.mpf(float(turn)) * mpmath.pi / 360
            ge = mpmath.sin(ae) / ae
            if abs(ae) < 1e-10:                               # 50 digits do not hold a cos a - sin a there; the next term is a^5 / 840
                gpe = -ae / 3 + ae ** 3 / 30
            else:
                gpe = (ae * mpmath.cos(ae) - mpmath.sin(ae)) / ae ** 2
            if abs(turn) == 360.0:
                assert g == 0.0                               # sind(180) is exactly 0; the true sin(pi) / pi too
            else:
                worst_g = max(worst_g, float(abs((mpmath.mpf(g) - ge) / ge)))
            worst_gp = max(worst_gp, float(abs((mpmath.mpf(gp) - gpe) / gpe)))
        return worst_g, worst_gp
    cg, cgp = errors(closed, rows[len(series):], "closed")
    sg, sgp = errors(series, rows[:len(series)], "series")
    print("closed forms, |a| >= %.2f: worst rel err g %.2e g' %.2e; series below: g %.2e g' %.2e (bounds: %.2e, %.2e)" % (switch, cg, cgp, sg, sgp, 2 * cg, 2 * cgp))
    assert 0.0 < cg < 1e-14 and 0.0 < cgp < 1e-13            # (the yardstick itself is rounding, not a wrong formula)
    assert sg <= 2.0 * cg and sgp <= 2.0 * cgp


def test_a_heading_variance_becomes_the_lateral_variance_of_the_issue(host):
    # P = diag(0, 0, 4 deg^2), theta = 0, drive 10 straight: P_yy = (10 pi / 180)^2 * 4 = 0.12185, P_xy = 0 -- not ekf_predict's 10^2 * 4
    want = (10.0 * np.pi / 180.0) ** 2 * 4.0
    assert abs(want - 0.12185) < 1e-5
    P0 = np.diag([0.0, 0.0, 4.0])
    for model, u in ((PM.TURN_DRIVE, [10.0, 0.0]), (PM.ARC, [10.0, 0.0]), (PM.POSE_DELTA, [10.0, 0.0, 0.0])):
        nu = PM.INPUTS[model]
        got = _eval(host, [(model, [0.0, 0.0, 0.0], u)])[0]
        F = np.eye(3); F[0, 2], F[1, 2] = got["fa"], got["fb"]
        P = F @ P0 @ F.T
        assert abs(P[1, 1] - want) < 1e-12 * want and P[0, 1] == 0.0 and P[0, 0] == 0.0 and got["x"].tolist() == [10.0, 0.0, 0.0]
        x, Pd, _ = PM.predict_model_dense(np.zeros(3), P0, [PM.step(model, u, np.zeros((nu, nu)))])
        assert abs(Pd[1, 1] - want) < 1e-12 * want and abs(Pd[0, 1]) < 1e-18 and x.tolist() == [10.0, 0.0, 0.0]
        assert abs(100.0 * 4.0 / P[1, 1] - PM.K ** 2) < 1e-9 * PM.K ** 2          # the reference's F gives k^2 = 3283 times as much


def test_compiled_noise_entry_is_V_M_Vt(host):
    rng = np.random.default_rng(4)
    for _ in range(10):
        V = rng.uniform(-1, 1, (3, 3))
        A = rng.uniform(-1, 1, (3, 3))
        M = A @ A.T
        M = (M + M.T) / 2.0
        m6 = [M[0, 0], M[1, 0], M[1, 1], M[2, 0], M[2, 1], M[2, 2]]
        Q = np.array(host(["noise " + " ".join(repr(float(v)) for v in list(V.reshape(-1)) + m6)])[0]).reshape(3, 3)
        assert np.abs(Q - V @ M @ V.T).max() < 1e-14 * np.abs(Q).max()
        assert Q[1, 0] == Q[0, 1] or abs(Q[1, 0] - Q[0, 1]) < 1e-15           # (the kernel forms the lower triangle and mirrors it)


# ------------------------------------------------------------------------------------------------------------------
# the kernel source, compiled for the host
# ------------------------------------------------------------------------------------------------------------------
def test_kernel_source_on_the_host_chains_bit_for_bit_and_matches_the_dense_restatement(tmp_path):
    """tests/support/predict_model_host_emulation.cpp: k_predict_model with a chain of m = 1, 2, 9, 32 steps against m launches of one, with
    0, 1 and 150 landmarks; then every case against predict_model_dense on the state before."""
    chain = PM.chain(np.random.default_rng(12), 32)
    assert {s[0] for s in chain[:9]} == {1, 2, 3} and any(not s[1].any() and not s[2].any() for s in chain[:9])
    raw = np.zeros((32, 13))
    for b, (model, u, M) in enumerate(chain):
        raw[b, 0] = model
        raw[b, 1:1 + u.size] = u
        full = np.zeros((3, 3)); full[:u.size, :u.size] = M
        raw[b, 4:] = full.reshape(-1)
    raw.tofile(tmp_path / "chain.bin")
    exe = host_build("predict_model_host_emulation", str(tmp_path / "predict_model_host_emulation"))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    lines = r.stdout.strip().split("\n")
    assert r.returncode == 0, r.stdout[-3000:]
    assert len(lines) == 12 and all(ln.endswith(": 0 differences") for ln in lines), r.stdout[-3000:]
    worst, ups, downs = 0.0, 0, 0
    for N in (0, 1, 150):
        n = 3 + 2 * N
        before = np.fromfile(tmp_path / ("before_%d.bin" % N))
        assert before.size == n + 9 + 6 * N
        x0 = before[:n]
        P0 = np.zeros((n, n))
        P0[:3, :3] = before[n:n + 9].reshape(3, 3)
        P0[:3, 3:] = before[n + 9:].reshape(3, 2 * N)
        P0[3:, :3] = P0[:3, 3:].T
        P0[3:, 3:] = np.eye(2 * N)                            # (the launch neither reads nor writes the landmark block)
        for m in (1, 2, 9, 32):
            after = np.fromfile(tmp_path / ("after_%d_%d.bin" % (N, m)))
            assert after.size == before.size + 9
            ex, eP, eQ = PM.predict_model_dense(x0, P0, chain[:m])
            gx, gprr, gstrip, gQ = after[:n], after[n:n + 9].reshape(3, 3), after[n + 9:n + 9 + 6 * N].reshape(3, 2 * N), after[-9:].reshape(3, 3)
            np.testing.assert_array_equal(eP[3:, 3:], P0[3:, 3:])
            errs = [np.abs(gx - ex).max() / np.abs(ex).max(), np.abs(gprr - eP[:3, :3]).max() / np.abs(eP).max(),
                    np.abs(gQ - eQ).max() / max(np.abs(eQ).max(), 1e-300)]
            if N:
                errs.append(np.abs(gstrip - eP[:3, 3:]).max() / np.abs(eP).max())
            worst = max(worst, max(errs))
            assert max(errs) < REL, (N, m, errs)
            assert 0.0 <= gx[2] <= 360.0
        th = x0[2]
        for model, u, _ in chain:                             # the chain does cross 360 upward and 0 downward from this heading
            t = th + u[-1] if model == PM.POSE_DELTA else th + u[1]
            ups += t >= 360.0; downs += t < 0.0
            th = PM.wrap360(t)
    print("k_predict_model on the host against the dense restatement: worst rel err %.2e" % worst)
    assert ups >= 3 and downs >= 3 and worst < 1e-12          # F64 throughout: rounding alone


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

    def append_model(self, entries):
        self.calls.append(("append_model", len(entries)))

    def predict_model(self, steps):
        self.calls.append(("predict_model", [(m, u.tolist(), M.tolist()) for m, u, M in steps]))


def _steps(log, n):
    for k in range(n):
        log.record([0.1, 1.0 + k], np.array([[1.0, 2.0, 3.0]]) if k % 2 else None, [1.0, 2.0], [[0.0, 1.0], [2.0, 3.0]])


def test_trajectory_format_seven_round_trip_and_the_older_formats(tmp_path):
    import append_model_cases as A
    from ekf_slam_amd import trajectory as TR
    from ekf_slam_amd.trajectory import TrajectoryLog
    assert TR.FORMAT_PREDICT == "ekfslam-trajectory-7" and TR.PREDICT_MODEL == "predict_model"
    assert TR.EDIT_KINDS == ("remove", "constrain", "merge", "merge_batch")
    predict_keys = {"predict_edit", "predict_ptr", "predict_model", "predict_u", "predict_M"}
    # logs without the kind keep their formats and their arrays, and a loaded one saves byte for byte what it was loaded from
    RP = np.array([[0.02, 0.005], [0.005, 0.03]])
    one = TrajectoryLog(); _steps(one, 3)
    two = TrajectoryLog(); _steps(two, 2); two.record_edit("constrain", [1, 2], [0.5, 0.0], RP)
    three = TrajectoryLog(); _steps(three, 2); three.record_edit("merge_batch", [3, 5, 1, 2])
    four = TrajectoryLog(); _steps(four, 2); four.record_observation([1.0, 2.0], RP, np.ones((2, 3)), [4, 2], [np.eye(2), -np.eye(2)], gate=9.21, wrap=(0, 1))
    five = TrajectoryLog(); _steps(five, 2); five.record_model_observation(1, [5.0, 30.0], RP, [4], gate=9.21)
    six = TrajectoryLog(); _steps(six, 2); six.record_model_append(A.scan(np.random.default_rng(1), 3, 700.0))
    for v, log in enumerate((one, two, three, four, five, six), 1):
        p = tmp_path / ("v%d.npz" % v)
        log.save(p)
        g = np.load(p)
        assert str(g["format"]) == "ekfslam-trajectory-%d" % v and not (set(g.files) & predict_keys)
        back = TrajectoryLog.load(p)
        assert len(back) == len(log) and len(back.edits) == len(log.edits) and back.model_predicts == {}
        back.save(tmp_path / ("v%d_again.npz" % v))
        assert same_npz(p, tmp_path / ("v%d_again.npz" % v))
    # version 7: chains of motion steps among the other edits
    chain = PM.chain(np.random.default_rng(3), 5)
    seven = TrajectoryLog(); _steps(seven, 2)
    seven.record_edit("remove", [7])
    seven.record_model_predict(chain)
    seven.record_model_append(A.scan(np.random.default_rng(1), 2, 700.0))
    _steps(seven, 2)
    seven.record_model_predict([(PM.POSE_DELTA, [0.0, 0.0, 0.0], M3)])
    seven.save(tmp_path / "seven.npz")
    g = np.load(tmp_path / "seven.npz")
    assert str(g["format"]) == TR.FORMAT_PREDICT and g["edit_kind"].tolist() == [0, 7, 6, 7] and predict_keys <= set(g.files)
    assert {"append_edit", "model_edit", "observe_edit"} <= set(g.files)
    assert g["predict_edit"].tolist() == [1, 3] and g["predict_ptr"].tolist() == [0, 5, 6] and g["predict_model"].tolist() == [1, 2, 3, 3, 1, 3]
    assert g["predict_u"].shape == (6, 3) and g["predict_M"].shape == (6, 3, 3)
    back = TrajectoryLog.load(tmp_path / "seven.npz")
    assert len(back) == 4 and [(e[0], e[1]) for e in back.edits] == [(2, "remove"), (2, "predict_model"), (2, "append_model"), (4, "predict_model")]
    assert sorted(back.model_predicts) == [1, 3] and sorted(back.model_appends) == [2]
    for got, want in zip(back.model_predicts[1], chain):
        assert got[0] == want[0]
        np.testing.assert_array_equal(got[1], want[1]); np.testing.assert_array_equal(got[2], want[2])
    back.save(tmp_path / "seven_again.npz")
    assert same_npz(tmp_path / "seven.npz", tmp_path / "seven_again.npz")
    r = _Replayed()
    back.replay(r)
    assert r.calls == [("predict",), ("predict",), ("measure",), ("remove", [6]),
                       ("predict_model", [(m, u.tolist(), M.tolist()) for m, u, M in chain]), ("append_model", 2),
                       ("predict",), ("predict",), ("measure",), ("predict_model", [(3, [0.0, 0.0, 0.0], M3.tolist())])]
    only = TrajectoryLog(); _steps(only, 1)
    only.record_model_predict(chain[:1])
    only.save(tmp_path / "only.npz")
    back = TrajectoryLog.load(tmp_path / "only.npz")
    assert str(np.load(tmp_path / "only.npz")["format"]) == TR.FORMAT_PREDICT and back.model_appends == {} and list(back.model_predicts) == [0]
    # bad shapes are refused and nothing is recorded
    bad = TrajectoryLog()
    for steps in ([], [(1, [1.0], M2)], [(1, [1.0, 2.0], M3)], [(3, [1.0, 2.0, 3.0], M2)], [(1, [1.0, 2.0])]):
        with pytest.raises(ValueError):
            bad.record_model_predict(steps)
    with pytest.raises(ValueError):
        bad.record_edit("predict_model", [])                  # chains of motion steps have their own recorder
    assert bad.edits == [] and bad.model_predicts == {}


# ------------------------------------------------------------------------------------------------------------------
# the Python layers over a stand-in for the library
# ------------------------------------------------------------------------------------------------------------------
class _Recorder(RecorderBase):
    status_string = b"invalid argument"
    last_error = b"predict_model: injected"

    def __init__(self):
        self.calls, self.fail = [], 0

    def ekf_predict_model(self, h, arr, m):
        self.calls.append(("predict_model", m, [(o.model, o.reserved, list(o.u), list(o.M)) for o in list(arr)[:m]]))
        return self.fail

    def ekf_motion_evaluate(self, model, xr, u, xn, F, V):
        self.calls.append(("evaluate", model, [xr[i] for i in range(3)], [u[i] for i in range(3)]))
        xn[2], F[6], V[1] = 7.0, 8.0, 9.0
        return self.fail


def test_engine_and_slam_layers_marshal_a_chain_once(monkeypatch):
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import engine as E
    from ekf_slam_amd import slam as S
    from ekf_slam_amd.trajectory import TrajectoryLog
    assert ctypes.sizeof(L.EkfMotion) == 104 and L.EKF_PREDICT_MODEL_MAX == 32
    assert (L.EKF_MOTION_TURN_DRIVE, L.EKF_MOTION_ARC, L.EKF_MOTION_POSE_DELTA) == (1, 2, 3)
    assert "ekf_predict_model" in L.SIGNATURES and "ekf_motion_evaluate" in L.SIGNATURES
    rec = _Recorder()
    monkeypatch.setattr(L, "lib", lambda: rec)
    e = E.Engine(capacity=16)
    Masym = [[1.0, 2.0], [3.0, 4.0]]
    e.predict_model([(1, [5.0, 30.0], Masym), (3, [1.0, 2.0, 3.0], M3)])
    # M travels column-major in the 3 x 3 slot; a model with two inputs fills the leading block and two entries of u
    assert rec.calls[-1] == ("predict_model", 2, [(1, 0, [5.0, 30.0, 0.0], [1.0, 3.0, 0.0, 2.0, 4.0, 0.0, 0.0, 0.0, 0.0]),
                                                  (3, 0, [1.0, 2.0, 3.0], list(M3.reshape(-1, order="F")))])
    xn, F, V = E.Engine.motion_evaluate(2, [1.0, 2.0, 3.0], [4.0, 5.0])
    assert rec.calls[-1] == ("evaluate", 2, [1.0, 2.0, 3.0], [4.0, 5.0, 0.0]) and xn[2] == 7.0 and F[0, 2] == 8.0 and V[1, 0] == 9.0
    n = len(rec.calls)
    for bad in ([(1, [5.0], M2)], [(1, [5.0, 30.0, 1.0], M2)], [(1, [5.0, 30.0], M3)], [(3, [1.0, 2.0, 3.0], M2)], [(1, [5.0, 30.0])]):
        with pytest.raises(ValueError):
            e.predict_model(bad)
    assert len(rec.calls) == n
    for cls in (S.EKF_SLAM, S.EKF_SLAM_UC):
        rec = _Recorder()
        monkeypatch.setattr(L, "lib", lambda: rec)
        f = cls(capacity=16)
        f.log = TrajectoryLog()
        f.predict_turn_drive(5.0, 30.0, M2)
        assert rec.calls[-1] == ("predict_model", 1, [(1, 0, [5.0, 30.0, 0.0], [0.04, 0.01, 0.0, 0.01, 0.09, 0.0, 0.0, 0.0, 0.0])])
        f.predict_arc([1.0, 2.0, 3.0], [10.0, 20.0, 30.0], M2)                # a list of steps, one M for all
        assert rec.calls[-1][1] == 3 and [c[0] for c in rec.calls[-1][2]] == [2, 2, 2] and [c[2][:2] for c in rec.calls[-1][2]] == [[1.0, 10.0], [2.0, 20.0], [3.0, 30.0]]
        f.predict_pose_delta(0.0, 0.0, 0.0, M3)
        assert rec.calls[-1] == ("predict_model", 1, [(3, 0, [0.0, 0.0, 0.0], list(M3.reshape(-1, order="F")))])
        f.predict_pose_delta([1.0, 2.0], [0.0, 0.5], [3.0, -3.0], np.array([M3, 2 * M3]))       # ... or one per step
        assert rec.calls[-1][1] == 2 and rec.calls[-1][2][1][3] == list((2 * M3).reshape(-1, order="F"))
        f.predict_model((2, [1.0, 2.0], M2))                                  # one step as it stands
        f.predict_model([(1, [1.0, 2.0], M2), (3, [1.0, 2.0, 3.0], M3)])
        assert [(k, kind) for k, kind, _, _, _ in f.log.edits] == [(0, "predict_model")] * 6
        assert [len(f.log.model_predicts[q]) for q in range(6)] == [1, 3, 1, 2, 1, 2] and f.log.model_predicts[5][1][2].shape == (3, 3)
        n = len(rec.calls)
        for bad in ([], [(1, [1.0, 2.0], M2)] * 33, [(0, [1.0, 2.0], M2)], [(4, [1.0, 2.0, 3.0], M3)], [(1, [1.0], M2)], [(1, [1.0, 2.0], M3)],
                    [(1, [1.0, 2.0])], [(1, [1.0, 2.0], M2, 1.0)]):
            with pytest.raises(ValueError):
                f.predict_model(bad)
        with pytest.raises(ValueError):
            f.predict_arc([1.0, 2.0], [1.0], M2)
        assert len(rec.calls) == n and len(f.log.edits) == 6
        for name in ("predict_model", "predict_turn_drive", "predict_arc", "predict_pose_delta"):
            assert "The reference has no such method" in getattr(cls, name).__doc__
        # a refused call raises and is not logged
        rec.fail = L.EKF_ERR_INVALID_ARG
        with pytest.raises(L.EkfError) as info:
            f.predict_turn_drive(5.0, 30.0, M2)
        assert info.value.status == L.EKF_ERR_INVALID_ARG and "predict_model" in str(info.value) and len(f.log.edits) == 6


def test_shard_group_sends_the_chain_to_every_shard(monkeypatch):
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd.sharding import ShardGroup
    rec = _Recorder()
    monkeypatch.setattr(L, "lib", lambda: rec)
    g = ShardGroup(3, capacity=16)
    g.predict_model(iter(PM.chain(np.random.default_rng(2), 4)))             # (an iterator is read once and handed to all three)
    got = [c for c in rec.calls if c[0] == "predict_model"]
    assert len(got) == 3 and got[0][1:] == got[1][1:] == got[2][1:] and got[0][1] == 4
