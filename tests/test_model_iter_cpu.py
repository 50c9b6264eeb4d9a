"""CPU: the iterated model observation (ekf_observe_model_iterated).  The compiled ekfm::model_iterate of ekf_slam_amd/csrc/device_math.h
-- the text ekf_model_iterate and lane 0 of k_gather_model_iter run -- against the NumPy restatement of tests/model_iter_cases.py, as a
descent of the MAP cost, its stopping rule and its all-or-nothing outcomes; the kernel sources on the host; the ninth kind of the trajectory
log; the Python layers over a stand-in for the library.  No GPU."""
import subprocess

import numpy as np
import pytest

import model_iter_cases as I
import model_obs_cases as M
from helpers import REL, RPOS, RecorderBase, host_build, line_program, rel_err, same_npz

INF = float("inf")
MODELS2 = (M.RANGE_BEARING, M.RELATIVE_XY)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """The stand-alone host build of ekfm::model_iterate: host(lines) -> one list of floats per line."""
    return line_program(tmp_path_factory, "model_iter_host")


def run_iter(host, o, x, P, n, tol=0.0):
    return I.parse_iter(host([I.iter_line(o, x, P, n, tol)])[0])


# ------------------------------------------------------------------------------------------------------------------
# 1. known answers
# ------------------------------------------------------------------------------------------------------------------
def test_compiled_loop_matches_the_restatement_for_every_model(host):
    cases = I.cases_all_models(np.random.default_rng(17))
    assert {c[3]["model"] for c in cases} == {1, 2, 3, 4, 5} and sum(1 for c in cases if c[3]["anchor"] is not None) == 4
    lines, keys = [], []
    for name, x, P, o in cases:
        for n in (1, 2, 5, 16):
            lines.append(I.iter_line(o, x, P, n, 0.0)); keys.append((name, x, P, o, n))
    worst = 0.0
    moved = {}
    for (name, x, P, o, n), row in zip(keys, host(lines)):
        first, it, H, Gs = I.parse_iter(row)
        x2, P2, wfirst, wit = I.iterate_dense(x, P, o, n)
        assert first["outcome"] == wfirst["outcome"] == M.APPLIED, name
        # a step of exactly 0 ends the loop (the header's exception); whether the last bits of a converged step are 0 is rounding, so
        # `used` is compared where the restatement's steps are well above it
        if wit["last_step"] > 1e-12 and it["last_step"] > 1e-12:
            assert it["used"] == wit["used"] == n and not it["converged"], (name, n)
        errs = [rel_err(first["S"], wfirst["S"]), rel_err(first["nu"], wfirst["nu"]), abs(first["d2"] - wfirst["d2"]) / wfirst["d2"],
                rel_err(it["S"], wit["S"]), rel_err(it["x_local"], wit["x_local"]),
                float(np.abs(it["nu"] - wit["nu"]).max() / max(np.abs(wfirst["nu"]).max(), 1.0))]
        worst = max(worst, max(errs))
        assert max(errs) < REL, (name, n, errs)
        loc = I.local_rows(o)
        np.testing.assert_allclose(it["x_local"][:len(loc)], x2[loc], rtol=0, atol=REL * np.abs(x2).max())     # xi_used IS the new state
        assert not it["x_local"][len(loc):].any()
        if n in (1, 16):
            moved[(name, n)] = it["x_local"]
    print("compiled model_iterate against the NumPy restatement: worst rel err %.2e" % worst)
    # the cases are no fixed points of one linearisation: 16 linearisations land elsewhere than one
    for name, _, _, o in cases:
        assert np.abs(moved[(name, 16)] - moved[(name, 1)]).max() > 1e-6, name


def test_one_linearisation_is_the_plain_small_part_bit_for_bit(host):
    cases = I.cases_all_models(np.random.default_rng(18))
    for name, x, P, o in cases:
        for gate in (INF, 1e-3):
            o = dict(o, gate=gate)
            it_row, sm_row = host([I.iter_line(o, x, P, 1, 0.0), M.small_line(o, x, P)])
            first, it, H, Gs = I.parse_iter(it_row)
            # small: outcome d2 nu[2] S[4] | H[14] Gs[14]
            assert first["outcome"] == int(sm_row[0]) == (M.GATED if gate < 1.0 else M.APPLIED), name
            assert np.array([first["d2"]]).tobytes() == np.array([sm_row[1]]).tobytes()
            assert first["nu"].tobytes() == np.array(sm_row[2:4]).tobytes() and first["S"].tobytes() == np.array(sm_row[4:8]).tobytes(), name
            # ... and the pair's operands are that linearisation's
            assert it["S"].tobytes() == first["S"].tobytes() and it["nu"].tobytes() == first["nu"].tobytes()
            assert H.tobytes() == np.array(sm_row[8:22]).tobytes() and Gs.tobytes() == np.array(sm_row[22:36]).tobytes(), name
            assert it["used"] == (0 if gate < 1.0 else 1)


# ------------------------------------------------------------------------------------------------------------------
# 2. it is the MAP step
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS2)
def test_iterating_descends_the_map_cost_to_its_stationary_point(host, model):
    x0, P, o = I.map_scene(model)
    J = {n: I.map_cost(I.iterate_dense(x0, P, o, n)[0], x0, P, o) for n in (1, 8)}
    gap = J[1] - J[8]
    print("model %d: the restatement's J after 1 linearisation %.4f, after 8 %.4f" % (model, J[1], J[8]))
    assert gap >= 0.05                                       # the precondition: there is something to gain in this scene
    it8 = run_iter(host, o, x0, P, 8)[1]
    it1 = run_iter(host, o, x0, P, 1)[1]
    Jc1, Jc8 = I.map_cost(it1["x_local"][:5], x0, P, o), I.map_cost(it8["x_local"][:5], x0, P, o)
    print("          the compiled loop's %.4f and %.4f" % (Jc1, Jc8))
    assert Jc8 < J[1] - 0.5 * gap and abs(Jc1 - J[1]) < 1e-9
    it16 = run_iter(host, o, x0, P, 16)[1]
    assert it16["last_step"] <= 1e-9
    want = np.abs(I.cost_gradient(I.iterate_dense(x0, P, o, 16)[0], x0, P, o)).max()
    got = np.abs(I.cost_gradient(it16["x_local"][:5], x0, P, o)).max()
    first_grad = np.abs(I.cost_gradient(it1["x_local"][:5], x0, P, o)).max()
    print("          |grad J| at xi_16: the restatement %.2e, the compiled loop %.2e (after one linearisation %.2e)" % (want, got, first_grad))
    assert got <= 10.0 * want and first_grad > 1e4 * want


# ------------------------------------------------------------------------------------------------------------------
# 3. stopping
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS2)
def test_the_tolerance_stops_the_loop_where_the_restatement_stops(host, model):
    x0, P, o = I.map_scene(model)
    want = I.iterate_dense(x0, P, o, 16, 1e-9)[3]
    it = run_iter(host, o, x0, P, 16, 1e-9)[1]
    assert it["used"] == want["used"] < 16 and it["converged"] and it["last_step"] <= 1e-9
    # tol = 0 runs them all and reports no convergence ...
    for n in (2, 5, 8):
        it = run_iter(host, o, x0, P, n, 0.0)[1]
        assert it["used"] == n and not it["converged"] and it["last_step"] > 0.0


def test_a_step_of_exactly_zero_counts_as_converged_even_under_tol_zero(host):
    # ... with ONE exception: a step of exactly 0 satisfies step <= tol for tol = 0.  A landmark range between two landmarks known
    # exactly (P = 0 on both) is linear in effect: G = 0, the first step is 0 and the loop stops at used = 1
    x = np.array([1.0, 2.0, 30.0, 4.0, 6.0, -3.0, 1.0])
    P = np.zeros((7, 7))
    P[:3, :3] = np.diag([0.5, 0.5, 9.0])
    o = M.obs(M.LANDMARK_RANGE, [8.1], 0.04, [0, 1])
    for tol in (0.0, 1e-9):
        first, it, _, _ = run_iter(host, o, x, P, 16, tol)
        assert first["outcome"] == M.APPLIED and it["used"] == 1 and it["converged"] and it["last_step"] == 0.0
        np.testing.assert_array_equal(it["x_local"], x)
        want = I.iterate_dense(x, P, o, 16, tol)[3]
        assert want["used"] == 1 and want["converged"]


# ------------------------------------------------------------------------------------------------------------------
# 4. all or nothing
# ------------------------------------------------------------------------------------------------------------------
def test_an_iterate_on_the_anchor_makes_the_whole_call_irregular(host):
    x, P, o = I.anchor_hit_scene()
    one = run_iter(host, o, x, P, 1)
    assert one[0]["outcome"] == M.APPLIED and one[1]["x_local"].tolist() == [4.0, 0.0, -4.0, 0.0, 0.0, 0.0, 0.0]        # exact coincidence
    for n in (2, 16):
        first, it, H, Gs = run_iter(host, o, x, P, n)
        assert first["outcome"] == M.IRREGULAR and it["used"] == 1 and not it["converged"]
        # the first record keeps the first linearisation's finite values; nothing that is not finite leaves the function
        assert first["nu"].tolist() == [8.0, 0.0] and first["S"].tolist() == [[2.0, 0.0], [0.0, 1.0]] and first["d2"] == 32.0
        assert np.all(np.isfinite(it["S"])) and np.all(np.isfinite(it["nu"])) and not H.any()
        x2, P2, wfirst, wit = I.iterate_dense(x, P, o, n)
        assert wfirst["outcome"] == M.IRREGULAR and wit["used"] == 1
        np.testing.assert_array_equal(x2, x); np.testing.assert_array_equal(P2, P)


def test_an_irregular_first_linearisation_stops_before_any_step(host):
    # R = 0, the robot known exactly and the landmark uncertain along the line of sight only: the bearing row has H P H' = 0, S is singular
    # at the first linearisation already -- today's irregular outcome, with used = 0 and every iteration count
    x = np.array([0.0, 0.0, 0.0, 5.0, 0.0])
    P = np.zeros((5, 5)); P[3, 3] = 4.0
    o = M.obs(M.RANGE_BEARING, [6.0, 0.0], np.zeros((2, 2)), [0])
    for n in (1, 4):
        first, it, _, _ = run_iter(host, o, x, P, n)
        assert first["outcome"] == M.IRREGULAR and it["used"] == 0 and np.isnan(first["d2"]) and np.all(np.isfinite(it["x_local"]))


def test_a_gated_first_linearisation_stops_before_any_step(host):
    x0, P, o = I.map_scene(M.RANGE_BEARING)
    d2 = I.iterate_dense(x0, P, o, 1)[2]["d2"]
    for n in (1, 8):
        first, it, _, _ = run_iter(host, dict(o, gate=0.5 * d2), x0, P, n)
        assert first["outcome"] == M.GATED and first["d2"] == pytest.approx(d2, rel=1e-9) and it["used"] == 0 and not it["converged"]
        np.testing.assert_array_equal(it["x_local"][:5], x0)
        first, it, _, _ = run_iter(host, dict(o, gate=2.0 * d2), x0, P, n)
        assert first["outcome"] == M.APPLIED and it["used"] == n


def test_the_library_function_is_the_same_loop_and_checks_its_arguments(host):
    """ekf_model_iterate of the built library (a pure host function: it runs without a GPU) against the stand-alone host build of the
    same text, bit for bit, and its refusals."""
    import ctypes
    import ekf_slam_amd
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd.engine import Engine, _p
    ekf_slam_amd.build()
    lib = ekf_slam_amd.lib()
    for name, x, P, o in I.cases_all_models(np.random.default_rng(19)):
        sm = [float(v) for v in M.small_line(o, x, P).split()[-38:]]
        for n, tol in ((1, 0.0), (5, 0.0), (16, 1e-9)):
            first, it, _, _ = run_iter(host, o, x, P, n, tol)
            z = o["z"].copy()
            if o["rows"] == 1:
                z[1] = 0.0
            got = Engine.model_iterate(o["model"], sm, z, M.effective_R(o), anchor=o["anchor"], has_landmark=bool(o["landmarks"]), gate=o["gate"],
                                       iterations=n, tol=tol, lib=lib)
            assert got["outcome"] == first["outcome"] and np.array([got["d2"]]).tobytes() == np.array([first["d2"]]).tobytes(), name
            assert got["nu"].tobytes() == first["nu"].tobytes() and np.ascontiguousarray(got["S"]).tobytes() == first["S"].tobytes(), name
            gi = got["iterated"]
            assert np.ascontiguousarray(gi["S"]).tobytes() == it["S"].tobytes() and gi["nu"].tobytes() == it["nu"].tobytes(), name
            assert (gi["used"], gi["converged"], gi["last_step"]) == (it["used"], it["converged"], it["last_step"]), name
            assert gi["x_local"].tobytes() == it["x_local"].tobytes(), name
    first, itr = L.EkfLinearResult(), L.EkfIteratedResult()
    sm, two, R = np.zeros(38), np.zeros(2), np.array([1.0, 0.0, 0.0, 1.0])
    call = lambda model=2, n=3, tol=0.0, gate=INF, f=ctypes.byref(first): lib.ekf_model_iterate(model, _p(sm), _p(two), 1, _p(two), _p(R), gate, n, tol, f,
                                                                                                  ctypes.byref(itr))
    assert call() == L.EKF_OK and first.outcome == L.EKF_LINEAR_IRREGULAR and itr.used == 0          # a state of zeros: the target on the robot
    for kw in (dict(model=0), dict(model=6), dict(n=0), dict(n=17), dict(n=-1), dict(tol=-1e-300), dict(tol=float("nan")), dict(gate=float("nan")),
               dict(f=None)):
        assert call(**kw) == L.EKF_ERR_INVALID_ARG, kw
    assert lib.ekf_model_iterate(2, None, _p(two), 1, _p(two), _p(R), INF, 3, 0.0, ctypes.byref(first), None) == L.EKF_ERR_INVALID_ARG
    assert lib.ekf_model_iterate(2, _p(sm), _p(two), 1, _p(two), _p(R), INF, 3, 0.0, ctypes.byref(first), None) == L.EKF_OK      # `it` may be NULL


# ------------------------------------------------------------------------------------------------------------------
# 5. the kernel sources, compiled for the host
# ------------------------------------------------------------------------------------------------------------------
def test_kernel_sources_on_the_host(tmp_path):
    """tests/support/model_iter_host_emulation.cpp: k_gather_model_iter on 3 landmarks -- with one linearisation k_gather_model's x,
    strip, diagonal blocks, pair and record bit for bit; with four the dense restatement; the probe's records the launch's."""
    import linear_obs_cases as C
    rng = np.random.default_rng(29)
    N = 3
    x, P, _ = C.random_state(rng, N)
    x[3:] = [12.0, 3.0, -8.0, 9.0, 5.0, -14.0]
    P = 0.5 * P
    P[2, 2] += 20.0
    obs = [M.obs(M.RANGE_BEARING, [0, 0], np.diag([0.01, 0.25]), [2]), M.obs(M.LANDMARK_RANGE, [0], 0.01, [0, 2]),
           M.obs(M.BEARING, [0], 0.25, anchor=[3.0, -16.0]), M.obs(M.RELATIVE_XY, [0, 0], 0.01 * np.eye(2), [1])]
    cases = []
    for o in obs:
        hx = M.jacobian(x, o)[0]
        o["z"][:o["rows"]] = hx[:o["rows"]] + (2.0 if o["model"] == M.BEARING else 0.5) * rng.standard_normal(o["rows"])
        for n in (1, 4):
            cases.append((o, n, 0.0))
    cases.append((dict(obs[0], gate=1e-6), 4, 0.0))                                   # gated: a zero pair, one count
    raw = [float(N)] + list(x) + list(P.reshape(-1)) + [float(len(cases))]
    for o, n, tol in cases:
        lm = o["landmarks"] + [-1, -1]
        anchor = [0.0, 0.0] if o["anchor"] is None else list(o["anchor"])
        z = o["z"].copy()
        if o["rows"] == 1:
            z[1] = 0.0
        raw += [o["model"], lm[0], lm[1], float(o["anchor"] is not None)] + anchor + list(z) + list(M.effective_R(o).reshape(-1)) + [o["gate"], n, tol, 0.0]
    np.array(raw, dtype=np.float64).tofile(tmp_path / "cases.bin")
    exe = host_build("model_iter_host_emulation", str(tmp_path / "model_iter_host_emulation"))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    lines = r.stdout.strip().split("\n")
    assert r.returncode == 0, r.stdout[-3000:]
    assert len(lines) == len(cases) and all(ln.endswith(": 0 differences") for ln in lines), r.stdout[-3000:]
    n_state = 3 + 2 * N
    worst = 0.0
    for k, (o, n, tol) in enumerate(cases):
        d = np.fromfile(tmp_path / ("case_%d.bin" % k))
        parts = np.split(d, np.cumsum([n_state, 9, 6 * N, 3 * N, 4 * N, 4 * N, 8, 16]))
        xk, prr, strip, diag, G, Kp, rec, itrec, cnt = parts
        x2, P2, first, it = I.iterate_dense(x, P, o, n, tol)
        assert int(rec[7]) == first["outcome"] and int(itrec[6]) == it["used"] == (0 if o["gate"] < 1.0 else n)
        assert cnt.tolist() == ([0.0, 1.0] if first["outcome"] == M.GATED else [0.0, 0.0])
        if first["outcome"] == M.GATED:
            assert not G.any() and not Kp.any()
            np.testing.assert_array_equal(xk, x)
            continue
        strip = strip.reshape(3, 2 * N)
        blocks = np.array([[P2[3 + 2 * j, 3 + 2 * j], P2[4 + 2 * j, 3 + 2 * j], P2[4 + 2 * j, 4 + 2 * j]] for j in range(N)]).reshape(-1)
        Hlast = it["H"]
        Gw = Hlast @ P
        Kw = (P @ Hlast.T @ np.linalg.inv(it["S"]))
        errs = [rel_err(xk, x2), rel_err(prr.reshape(3, 3), P2[:3, :3]), rel_err(strip, P2[:3, 3:]), rel_err(diag, blocks),
                rel_err(G.reshape(2 * N, 2), Gw[:, 3:].T), rel_err(Kp.reshape(2 * N, 2), Kw[3:, :]),
                rel_err(rec[:4].reshape(2, 2), first["S"]), rel_err(itrec[:4].reshape(2, 2), it["S"]), rel_err(itrec[9:16], it["x_local"])]
        worst = max(worst, max(errs))
        assert max(errs) < REL, (k, errs)
    print("the emulated k_gather_model_iter against the dense restatement: worst rel err %.2e" % worst)


# ------------------------------------------------------------------------------------------------------------------
# 6. the layers
# ------------------------------------------------------------------------------------------------------------------
class _Replayed:
    def __init__(self):
        self.calls = []

    def predict(self, u):
        self.calls.append(("predict",))

    def measure(self, *a):
        self.calls.append(("measure",))

    def observe_model(self, model, z, R, landmarks, anchor=None, gate=INF):
        self.calls.append(("observe_model", model, list(landmarks)))

    def observe_model_iterated(self, model, z, R, landmarks, anchor=None, gate=INF, iterations=3, tol=0.0):
        self.calls.append(("observe_model_iterated", model, np.asarray(z).tolist(), np.asarray(R).tolist(), list(landmarks),
                           None if anchor is None else np.asarray(anchor).tolist(), gate, iterations, tol))

    def predict_model(self, steps):
        self.calls.append(("predict_model", len(steps)))


def _steps(log, n):
    for k in range(n):
        log.record([0.1, 1.0 + k], np.array([[1.0, 2.0, 3.0]]) if k % 2 else None, [1.0, 2.0], [[0.0, 1.0], [2.0, 3.0]])


def test_trajectory_format_eight_only_with_an_iterated_observation(tmp_path):
    from ekf_slam_amd.trajectory import FORMAT_ITERATED, FORMAT_MODEL, FORMAT_PREDICT, TrajectoryLog
    assert FORMAT_ITERATED == "ekfslam-trajectory-8"
    # logs without one are written as before, and a loaded one saves byte for byte what it was loaded from
    five = TrajectoryLog(); _steps(five, 2); five.record_model_observation(M.RANGE, [7.5], [[0.5, 0.0], [0.0, 0.0]], [3])
    seven = TrajectoryLog(); _steps(seven, 2); seven.record_model_predict([(1, [0.5, 3.0], np.eye(2))])
    for log, name, fmt in ((five, "five", FORMAT_MODEL), (seven, "seven", FORMAT_PREDICT)):
        log.save(tmp_path / (name + ".npz"))
        g = np.load(tmp_path / (name + ".npz"))
        assert str(g["format"]) == fmt and not any(k.startswith("iter_") for k in g.files)
        back = TrajectoryLog.load(tmp_path / (name + ".npz"))
        assert back.model_iterations == {}
        back.save(tmp_path / (name + "_again.npz"))
        assert same_npz(tmp_path / (name + ".npz"), tmp_path / (name + "_again.npz"))
    eight = TrajectoryLog(); _steps(eight, 2)
    eight.record_model_observation(M.RANGE, [7.5], [[0.5, 0.0], [0.0, 0.0]], [3])
    eight.record_model_observation_iterated(M.RANGE_BEARING, [5.0, 30.0], RPOS, [4], gate=9.21, iterations=5, tol=1e-8)
    _steps(eight, 1)
    eight.record_model_observation_iterated(M.BEARING, [12.0], [[0.3, 0.0], [0.0, 0.0]], anchor=[10.0, -4.0], iterations=16)
    eight.record_model_observation_iterated(M.LANDMARK_RANGE, [2.5], [[0.1, 0.0], [0.0, 0.0]], [3, 9], iterations=2, tol=0.5)
    eight.save(tmp_path / "eight.npz")
    g = np.load(tmp_path / "eight.npz")
    assert str(g["format"]) == FORMAT_ITERATED and g["edit_kind"].tolist() == [5, 8, 8, 8]
    assert g["iter_edit"].tolist() == [1, 2, 3] and g["iter_model"].tolist() == [1, 3, 5] and g["iter_iterations"].tolist() == [5, 16, 2]
    assert g["iter_tol"].tolist() == [1e-8, 0.0, 0.5] and g["model_edit"].tolist() == [0] and g["predict_edit"].size == 0
    back = TrajectoryLog.load(tmp_path / "eight.npz")
    assert [(e[0], e[1], e[2].tolist()) for e in back.edits] == \
        [(2, "observe_model", [3]), (2, "observe_model_iterated", [4]), (3, "observe_model_iterated", []), (3, "observe_model_iterated", [3, 9])]
    assert back.model_iterations[1] == dict(model=1, anchor=None, gate=9.21, iterations=5, tol=1e-8)
    assert back.model_iterations[2]["anchor"].tolist() == [10.0, -4.0] and back.model_iterations[2]["gate"] == INF
    back.save(tmp_path / "eight_again.npz")
    assert same_npz(tmp_path / "eight.npz", tmp_path / "eight_again.npz")
    r = _Replayed()
    back.replay(r)
    assert r.calls == [("predict",), ("predict",), ("measure",), ("observe_model", 2, [2]),
                       ("observe_model_iterated", 1, [5.0, 30.0], RPOS.tolist(), [3], None, 9.21, 5, 1e-8), ("predict",),
                       ("observe_model_iterated", 3, [12.0, 0.0], [[0.3, 0.0], [0.0, 0.0]], [], [10.0, -4.0], INF, 16, 0.0),
                       ("observe_model_iterated", 5, [2.5, 0.0], [[0.1, 0.0], [0.0, 0.0]], [2, 8], None, INF, 2, 0.5)]
    bad = TrajectoryLog()
    for kw in (dict(landmarks=[1.5]), dict(landmarks=[1, 2, 3])):
        with pytest.raises(ValueError):
            bad.record_model_observation_iterated(M.RANGE, [1.0], None, **kw)
    with pytest.raises(ValueError):
        bad.record_edit("observe_model_iterated", [1])
    assert bad.edits == [] and bad.model_iterations == {}


class _Recorder(RecorderBase):
    last_error = b"observe_model_iterated: injected"

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
            r.d2, r.outcome = 1.5, 1
        return 0

    def _note_iter(self, name, pobs, iterations, tol, pfirst, pit):
        rc = self._note(name, pobs, pfirst)
        self.calls[-1] = self.calls[-1] + (iterations, tol, pit is not None)
        if not rc and pit is not None:
            it = pit._obj
            it.S[0], it.S[1], it.S[2], it.S[3] = 5.0, 6.0, 7.0, 8.0
            it.nu[0], it.nu[1] = 0.125, -0.5
            it.used, it.converged, it.last_step = 3, 1, 2.5e-10
            for k in range(7):
                it.x_local[k] = 10.0 + k
        return rc

    def ekf_observe_model(self, h, pobs, pres):
        return self._note("observe", pobs, pres)

    def ekf_observe_model_iterated(self, h, pobs, iterations, tol, pfirst, pit):
        return self._note_iter("observe_iterated", pobs, iterations, tol, pfirst, pit)

    def ekf_model_innovation_iterated(self, h, pobs, iterations, tol, pfirst, pit):
        return self._note_iter("innovation_iterated", pobs, iterations, tol, pfirst, pit)


def test_engine_and_slam_layers_marshal_an_iterated_observation_once(monkeypatch):
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import engine as E
    from ekf_slam_amd import slam as S
    from ekf_slam_amd.trajectory import TrajectoryLog
    assert L.EKF_MODEL_ITER_MAX == 16
    for name in ("ekf_observe_model_iterated", "ekf_model_innovation_iterated", "ekf_model_iterate"):
        assert name in L.SIGNATURES
    rec = _Recorder()
    monkeypatch.setattr(L, "lib", lambda: rec)
    e = E.Engine(capacity=16)
    assert e.observe_model_iterated(L.EKF_MODEL_RANGE_BEARING, [5.0, 30.0], [[0.5, 0.1], [0.1, 0.25]], [4], gate=9.0, iterations=5, tol=1e-8) is None
    assert rec.calls[-1] == ("observe_iterated", 1, [5.0, 30.0], [0.5, 0.1, 0.1, 0.25], [4, -1], [0.0, 0.0], 9.0, False, 5, 1e-8, False)
    out = e.observe_model_iterated(L.EKF_MODEL_RANGE, [7.5], 0.5, anchor=[10.0, -4.0], iterations=2, wait=True)
    assert rec.calls[-1] == ("observe_iterated", 2, [7.5, 0.0], [0.5, 0.0, 0.0, 0.0], [-1, -1], [10.0, -4.0], INF, True, 2, 0.0, True)
    assert out["nu"].tolist() == [0.5, -0.25] and out["S"].tolist() == [[1.0, 3.0], [2.0, 4.0]] and out["d2"] == 1.5 and out["outcome"] == 1
    it = out["iterated"]
    assert it["S"].tolist() == [[5.0, 7.0], [6.0, 8.0]] and it["nu"].tolist() == [0.125, -0.5] and it["used"] == 3 and it["converged"] is True
    assert it["last_step"] == 2.5e-10 and it["x_local"].tolist() == [10.0, 11.0, 12.0, 13.0, 14.0, 15.0, 16.0]
    assert e.model_innovation_iterated(L.EKF_MODEL_LANDMARK_RANGE, [2.5], 0.1, [3, 9], iterations=16, tol=0.25)["iterated"]["used"] == 3
    assert rec.calls[-1] == ("innovation_iterated", 5, [2.5, 0.0], [0.1, 0.0, 0.0, 0.0], [3, 9], [0.0, 0.0], INF, True, 16, 0.25, True)
    n = len(rec.calls)
    with pytest.raises(ValueError):
        e.observe_model_iterated(0, [1.0, 2.0], np.eye(2), [1])
    assert len(rec.calls) == n
    for cls in (S.EKF_SLAM, S.EKF_SLAM_UC):
        rec = _Recorder()
        monkeypatch.setattr(L, "lib", lambda: rec)
        f = cls(capacity=16)
        f.log = TrajectoryLog()
        # the defaults of every wrapper keep calling ekf_observe_model
        f.observe_range_bearing(5, [5.0, 30.0], RPOS, gate=6.0)
        f.observe_range(2, 7.5, 0.5)
        f.observe_bearing(3, -12.0, 0.3)
        f.observe_relative_xy(1, [2.0, -1.0], RPOS)
        f.observe_landmark_range(2, 7, 2.5, 0.1)
        f.observe_anchor_range([10.0, -4.0], 7.5, 0.5)
        f.observe_anchor_bearing([10.0, -4.0], 33.0, 0.2)
        f.observe_model(L.EKF_MODEL_RANGE, [7.5], 0.5, [2])
        f.observe_range(2, 7.5, 0.5, iterations=1, tol=0.0)
        assert [c[0] for c in rec.calls] == ["observe"] * 9 and all(len(c) == 8 for c in rec.calls)
        assert [kind for _, kind, _, _, _ in f.log.edits] == ["observe_model"] * 9
        # iterations > 1 (or a tolerance) goes to ekf_observe_model_iterated, 1-based landmarks converted once
        f.observe_range_bearing(5, [5.0, 30.0], RPOS, gate=6.0, iterations=8)
        assert rec.calls[-1] == ("observe_iterated", 1, [5.0, 30.0], [0.02, 0.005, 0.005, 0.03], [4, -1], [0.0, 0.0], 6.0, False, 8, 0.0, False)
        f.observe_range(2, 7.5, 0.5, iterations=3, tol=1e-6)
        assert rec.calls[-1] == ("observe_iterated", 2, [7.5, 0.0], [0.5, 0.0, 0.0, 0.0], [1, -1], [0.0, 0.0], INF, False, 3, 1e-6, False)
        assert f.observe_bearing(3, -12.0, 0.3, wait=True, iterations=2)["iterated"]["used"] == 3
        assert rec.calls[-1][0] == "observe_iterated" and rec.calls[-1][4] == [2, -1] and rec.calls[-1][7:] == (True, 2, 0.0, True)
        f.observe_relative_xy(1, [2.0, -1.0], RPOS, iterations=4)
        assert rec.calls[-1][:2] == ("observe_iterated", 4) and rec.calls[-1][4] == [0, -1]
        f.observe_landmark_range(2, 7, 2.5, 0.1, gate=4.0, iterations=2)
        assert rec.calls[-1] == ("observe_iterated", 5, [2.5, 0.0], [0.1, 0.0, 0.0, 0.0], [1, 6], [0.0, 0.0], 4.0, False, 2, 0.0, False)
        f.observe_anchor_range([10.0, -4.0], 7.5, 0.5, iterations=2)
        assert rec.calls[-1][:2] == ("observe_iterated", 2) and rec.calls[-1][5] == [10.0, -4.0]
        f.observe_anchor_bearing([10.0, -4.0], 33.0, 0.2, iterations=1, tol=1e-3)
        assert rec.calls[-1][:2] == ("observe_iterated", 3) and rec.calls[-1][8:10] == (1, 1e-3)
        f.observe_model_iterated(L.EKF_MODEL_RANGE, [7.5], 0.5, [2], iterations=1)           # asked for by name: the iterated entry point
        assert rec.calls[-1][0] == "observe_iterated" and rec.calls[-1][8] == 1
        assert f.model_innovation_iterated(L.EKF_MODEL_RANGE, [1.0], 0.5, [6], iterations=7)["iterated"]["used"] == 3
        assert rec.calls[-1][0] == "innovation_iterated" and rec.calls[-1][4] == [5, -1] and rec.calls[-1][8] == 7
        assert [kind for _, kind, _, _, _ in f.log.edits][9:] == ["observe_model_iterated"] * 8
        assert f.log.model_iterations[9] == dict(model=1, anchor=None, gate=6.0, iterations=8, tol=0.0)
        assert f.log.model_iterations[14]["anchor"].tolist() == [10.0, -4.0] and f.log.edits[13][2].tolist() == [2, 7]
        n, m = len(rec.calls), len(f.log.edits)
        with pytest.raises(ValueError):
            f.observe_range(1.5, 2.0, 0.5, iterations=3)
        assert len(rec.calls) == n
        rec.fail = L.EKF_ERR_STATE
        with pytest.raises(L.EkfError) as info:
            f.observe_range(1, 0.0, 0.5, wait=True, iterations=3)
        assert info.value.status == L.EKF_ERR_STATE and "observe_model_iterated" in str(info.value) and len(f.log.edits) == m
        # the log holds what the library received, field by field: the eight iterated calls above and one with a general R
        rec.fail = 0
        f.observe_model_iterated(L.EKF_MODEL_RELATIVE_XY, [1.5, -2.5], [[0.5, 0.1], [0.2, 0.25]], [4], gate=9.0, iterations=7, tol=0.125)
        sent = [c for c in rec.calls if c[0] == "observe_iterated"]
        del sent[8]                                           # the refused one
        assert len(sent) == 9 and len(f.log.edits) == 18 and sent[8][3] == [0.5, 0.2, 0.1, 0.25]
        for (_, model, z, Rc, lm, anchor, gate, _, iterations, tol, _), (_, _, idx, zl, Rl), q in zip(sent, f.log.edits[9:], range(9, 18)):
            o = f.log.model_iterations[q]
            assert zl.tolist() == z and Rl.reshape(-1, order="F").tolist() == Rc
            assert (o["model"], o["gate"], o["iterations"], o["tol"]) == (model, gate, iterations, tol)
            assert [k - 1 for k in idx.tolist()] + [-1] * (2 - idx.size) == lm
            assert (anchor == [0.0, 0.0] and o["anchor"] is None) if idx.size else o["anchor"].tolist() == anchor
