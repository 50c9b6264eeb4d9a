"""CPU: a scan's pairings applied as ONE joint update, RELINEARISED (ekf_observe_model_joint_iterated / ekf_joint_iterate; DESIGN.md
section 3r).
  (a) the NumPy restatement of tests/observe_joint_iter_cases.py: one linearisation is observe_joint_cases' update, one pairing is
      model_iter_cases' single iterated update, the MAP gradient vanishes at convergence, scan order does not matter, the scene's premises;
  (b) ekf_joint_iterate of the built library (a pure host function: no GPU) against the restatement;
  (c) tests/support/observe_joint_iter_host_emulation.cpp: the kernel SOURCES of k_joint_factor_iter, k_gather_joint and the pass's pair
      loop, compiled for the host, against the restatement -- and once more under the address and undefined-behaviour sanitizers;
  (d) the Python layers over a stand-in for the library, format 10 of the trajectory log, measure_model_joint(joint_iterations=3).
No GPU."""
import os
import subprocess

import numpy as np
import pytest

import associate_model_cases as A
import joint_cases as J
import model_iter_cases as MI
import model_obs_cases as M
import observe_joint_cases as C
import observe_joint_iter_cases as I
import test_observe_joint_cpu as T
from helpers import ROOT, RPOS, host_build, same_npz

GOLDEN = os.path.join(ROOT, "tests", "golden", "trajectory")
BAR = 1e-12                     # the project's bar for a restated update against the device's text (test_observe_joint_cpu.py)


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


@pytest.fixture(scope="module")
def premises():
    return I.assert_scene_premises()


# ------------------------------------------------------------------------------------------------------------------
# (a) the restatement
# ------------------------------------------------------------------------------------------------------------------
def test_scene_premises(premises):
    assert [row[0] for row in premises] == list(I.NPS)


def test_one_linearisation_is_the_joint_update_exactly():
    for npair in I.NPS:
        x, P, ents, lms = I.scene_dense(npair)
        x1, P1, rec, it = I.joint_update_iterated_dense(x, P, ents, lms, 1)
        xj, Pj, rj = C.joint_update_dense(x, P, ents, lms)
        np.testing.assert_array_equal(x1, xj); np.testing.assert_array_equal(P1, Pj)
        assert rec["d2"] == rj["d2"] and rec["outcome"] == rj["outcome"] == C.APPLIED and it["used"] == 1
    x, P = J.dense_state()
    ents, lms = C.scan_of(x, 5)
    hyp = [lms[0], -1] + lms[2:]
    x1, P1, _, _ = I.joint_update_iterated_dense(x, P, ents, hyp, 1)
    xj, Pj, _ = C.joint_update_dense(x, P, ents, hyp)
    np.testing.assert_array_equal(x1, xj); np.testing.assert_array_equal(P1, Pj)


def test_one_pairing_is_the_single_iterated_update():
    x, P, ents, lms = I.scene_dense(5)
    for ent, lm in zip(ents, lms):
        o = J.pairing_obs(ent, lm)
        for n in (1, 3, 8):
            xs, Ps, first, its = MI.iterate_dense(x, P, o, n)
            xj, Pj, rec, it = I.joint_update_iterated_dense(x, P, [ent], [lm], n)
            err = max(rel(xj, xs), rel(Pj, Ps))
            print("model %d at landmark %d, %d linearisations: one pairing against the single iterated update %.2e" % (ent["model"], lm, n, err))
            assert err <= 1e-12 and it["used"] == its["used"] == n and rec["outcome"] == first["outcome"] == C.APPLIED


def test_the_map_gradient_vanishes_at_convergence(premises):
    for npair in I.NPS:
        x, P, ents, lms = I.scene_dense(npair)
        _, _, _, it = I.joint_update_iterated_dense(x, P, ents, lms, I.ITER_MAX)
        xq = x.copy()
        xq[I.sub_rows(lms)] = it["x_sub"]
        g0, g = I.map_gradient(x, x, P, ents, lms), I.map_gradient(xq, x, P, ents, lms)
        ratio = float(np.abs(g).max() / np.abs(g0).max())
        print("np = %2d: MAP gradient at xi_16 over its value at xi_0: %.2e" % (npair, ratio))
        assert ratio <= 1e-8


def test_the_result_does_not_depend_on_scan_order():
    x, P, ents, lms = I.scene_dense(5)
    xa, Pa, _, ia = I.joint_update_iterated_dense(x, P, ents, lms, 3)
    back = list(range(5))[::-1]
    xb, Pb, _, ib = I.joint_update_iterated_dense(x, P, [ents[k] for k in back], [lms[k] for k in back], 3)
    assert rel(xb, xa) <= 1e-12 and rel(Pb, Pa) <= 1e-12 and ia["used"] == ib["used"] == 3


def test_gated_and_irregular_leave_the_dense_state_alone():
    x, P, ents, lms = I.scene_dense(2)
    d2 = J.joint_dense(x, P, ents, lms)["d2"]
    xg, Pg, rg, ig = I.joint_update_iterated_dense(x, P, ents, lms, 3, gate=0.5 * d2)
    assert rg["outcome"] == C.GATED and ig["used"] == 0
    np.testing.assert_array_equal(xg, x); np.testing.assert_array_equal(Pg, P)
    x, P, ents, lms = I.later_irregular()
    xi, Pi, ri, ii = I.joint_update_iterated_dense(x, P, ents, lms, 3)
    assert (ri["outcome"], ii["irregular_at"], ii["used"]) == (C.IRREGULAR, 1, 1)
    np.testing.assert_array_equal(xi, x); np.testing.assert_array_equal(Pi, P)
    x1 = I.joint_update_iterated_dense(x, P, ents, lms, 1)[2]
    assert x1["outcome"] == C.APPLIED                        # one linearisation never sees the second


# ------------------------------------------------------------------------------------------------------------------
# (b) the library's host function
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import ekf_slam_amd
    ekf_slam_amd.build()
    return ekf_slam_amd.lib()


def _sub(x, P, lms):
    loc = I.sub_rows(lms)
    return x[loc], P[np.ix_(loc, loc)], loc


def test_joint_iterate_against_the_restatement(lib, premises):
    """ekf_joint_iterate through the built library.  One linearisation: 1e-12, test_observe_joint_cpu.py's bar.  3 and 8: the bar is
    max(1e-12, 4 x the float64 restatement's own distance from the same loop in numpy.longdouble) -- the factor 4 for a different
    summation order over at most 67 terms.  Measured: the restatement is within 1.3e-14 of longdouble on these scans (np = 32, 8
    linearisations, P; x: 1.2e-15), so the bar is 1e-12 throughout; the library is within 2.9e-14 of the restatement."""
    from ekf_slam_amd.engine import Engine
    for npair in I.NPS:
        x, P, ents, lms = I.scene_dense(npair)
        xs, Ps, loc = _sub(x, P, lms)
        for n in (1, 3, 8):
            ex, eP, rec, want = I.joint_update_iterated_dense(x, P, ents, lms, n)
            xl, Pl = I.iterate_sub_longdouble(xs, Ps, ents, n)
            own = max(rel(ex[loc], xl), rel(eP[np.ix_(loc, loc)], Pl))
            bar = BAR if n == 1 else max(BAR, 4.0 * own)
            gx, gP, it = Engine.joint_iterate(xs, Ps, ents, n, 0.0, lib=lib)
            err = max(rel(gx, ex[loc]), rel(gP, eP[np.ix_(loc, loc)]), rel(it["x_sub"], want["x_sub"]))
            print("np = %2d, %d linearisations: restatement against longdouble %.2e, bar %.2e, library against restatement %.2e"
                  % (npair, n, own, bar, err))
            assert err <= bar
            assert (it["used"], it["converged"], it["irregular_at"]) == (want["used"], want["converged"], -1) and want["used"] == n
            np.testing.assert_allclose(it["step"], want["step"], rtol=1e-6, atol=1e-13)
            np.testing.assert_allclose(it["d2_last"], want["d2_last"], rtol=1e-9)
            np.testing.assert_array_equal(gP, gP.T)


def test_joint_iterate_stops_at_tol_where_the_restatement_does(lib, premises):
    from ekf_slam_amd.engine import Engine
    for (npair, _, _, _, tol, used) in premises:
        x, P, ents, lms = I.scene_dense(npair, offset=I.NEAR)
        xs, Ps, loc = _sub(x, P, lms)
        ex, eP, _, want = I.joint_update_iterated_dense(x, P, ents, lms, I.ITER_MAX, tol)
        gx, gP, it = Engine.joint_iterate(xs, Ps, ents, I.ITER_MAX, tol, lib=lib)
        assert (it["used"], it["converged"]) == (want["used"], want["converged"]) == (used, True), npair
        assert max(rel(gx, ex[loc]), rel(gP, eP[np.ix_(loc, loc)])) <= BAR
        # one linearisation fewer than that does not converge
        short = Engine.joint_iterate(xs, Ps, ents, used - 1, tol, lib=lib)[2]
        assert (short["used"], short["converged"]) == (used - 1, False)


def test_joint_iterate_irregular_later_and_refusals(lib):
    import ctypes
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import marshal
    from ekf_slam_amd.engine import Engine, _p
    x, P, ents, lms = I.later_irregular()
    xs, Ps, _ = _sub(x, P, lms)
    gx, gP, it = Engine.joint_iterate(xs, Ps, ents, 3, 0.0, lib=lib)
    assert (it["irregular_at"], it["irregular_obs"], it["used"], it["converged"]) == (1, 0, 1, False)
    np.testing.assert_array_equal(gx, xs); np.testing.assert_array_equal(gP, Ps)
    gx, gP, it = Engine.joint_iterate(xs, Ps, ents, 1, 0.0, lib=lib)
    assert it["irregular_at"] == -1 and it["used"] == 1 and not np.array_equal(gx, xs)
    # the first linearisation irregular: the landmark on the robot
    on = xs.copy(); on[3:5] = on[:2]
    gx, gP, it = Engine.joint_iterate(on, Ps, ents, 3, 0.0, lib=lib)
    assert (it["irregular_at"], it["irregular_obs"], it["used"]) == (0, 0, 0)
    np.testing.assert_array_equal(gx, on); np.testing.assert_array_equal(gP, Ps)
    arr, m = marshal.scan_obs(ents)
    rec, xo, Po = L.EkfJointIterResult(), np.zeros(xs.size), np.zeros(Ps.size)
    Pf = np.ascontiguousarray(Ps.T)
    call = lambda n=3, tol=0.0, count=m, px=_p(xs), r=ctypes.byref(rec): lib.ekf_joint_iterate(px, _p(Pf), arr, count, n, tol, r, _p(xo), _p(Po))
    assert call() == L.EKF_OK
    for kw in (dict(n=0), dict(n=17), dict(n=-1), dict(tol=-1e-300), dict(tol=float("nan")), dict(count=0), dict(count=33), dict(px=None), dict(r=None)):
        assert call(**kw) == L.EKF_ERR_INVALID_ARG, kw
    assert L.EKF_JOINT_ITER_MAX == L.EKF_MODEL_ITER_MAX == 16 and ctypes.sizeof(L.EkfJointIterResult) == 40 + 8 * 67


# ------------------------------------------------------------------------------------------------------------------
# (c) the kernel sources on the host
# ------------------------------------------------------------------------------------------------------------------
def _read_cases(path):
    raw = np.fromfile(path, dtype=np.float64)
    pos = 0
    while pos < raw.size:
        n, m, outcome, iterations = (int(v) for v in raw[pos:pos + 4]); pos += 4
        ents, hyp = [], []
        for _ in range(m):
            model, z, R, lm = int(raw[pos]), raw[pos + 1:pos + 3], raw[pos + 3:pos + 7].reshape(2, 2), int(raw[pos + 7]); pos += 8
            rows = M.ROWS[model]
            ents.append(A.entry(model, z[:rows], R if rows == 2 else R[0, 0]))
            hyp.append(lm)
        x0 = raw[pos:pos + n].copy(); pos += n
        P0 = raw[pos:pos + n * n].reshape(n, n).copy(); pos += n * n
        x1 = raw[pos:pos + n].copy(); pos += n
        P1 = raw[pos:pos + n * n].reshape(n, n).copy(); pos += n * n
        d2, used, converged, irr_at = raw[pos:pos + 4]; pos += 4
        yield ents, hyp, outcome, iterations, x0, P0, x1, P1, d2, int(used), int(irr_at)


def test_kernel_sources_on_the_host_against_the_restatement(tmp_path):
    """observe_joint_iter_host_emulation.cpp runs k_joint_factor_iter, k_gather_joint and the pass's pair loop on N = 40 and N = 41 (a
    padded tail), T = 16, for np = 1, 2, 5 and 32 and 1, 3 and 8 linearisations, one gated and one irregular-later case, and writes the
    state before and after; here the restatement is applied to the state before.  The program itself compares the block of one
    linearisation with k_joint_factor's byte for byte."""
    exe = host_build("observe_joint_iter_host_emulation", str(tmp_path / "observe_joint_iter_host_emulation"))
    out = tmp_path / "cases.bin"
    r = subprocess.run([exe, str(out)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    seen = []
    for ents, hyp, outcome, iterations, x0, P0, x1, P1, d2, used, irr_at in _read_cases(out):
        gate = 0.0 if outcome == C.GATED else C.INF
        ex, eP, want, wit = I.joint_update_iterated_dense(x0, P0, ents, hyp, iterations, 0.0, gate)
        assert want["outcome"] == outcome and wit["irregular_at"] == irr_at
        npair = sum(1 for h in hyp if h >= 0)
        if outcome == C.APPLIED:
            err_x, err_P = rel(x1, ex), rel(P1, eP)
            print("np = %2d, %d linearisations: emulated kernels against the restatement: rel err x %.2e P %.2e" % (npair, iterations, err_x, err_P))
            assert err_x <= BAR and err_P <= BAR and used == wit["used"] == iterations
            np.testing.assert_allclose(d2, want["d2"], rtol=1e-10)
            np.testing.assert_array_equal(P1, P1.T)
        else:
            np.testing.assert_array_equal(x1, x0); np.testing.assert_array_equal(P1, P0)
            assert used == wit["used"]
        seen.append((npair, iterations, outcome))
    applied = sorted((p, n) for p, n, o in seen if o == C.APPLIED)
    assert applied == sorted((p, n) for n in (1, 3, 8) for p in (1, 2, 5, 32, 32)) and {o for _, _, o in seen} == {C.APPLIED, C.GATED, C.IRREGULAR}


def test_kernel_sources_on_the_host_under_the_sanitizers(tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined runs clean (nothing loaded into python is involved)."""
    exe = host_build("observe_joint_iter_host_emulation", str(tmp_path / "emulation_sanitized"),
                     flags=["-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe, str(tmp_path / "cases.bin")], capture_output=True, text=True)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]


# ------------------------------------------------------------------------------------------------------------------
# (d) the Python layers over a stand-in for the library
# ------------------------------------------------------------------------------------------------------------------
class _Lib(T._Lib):
    last_error = b"observe_model_joint_iterated: injected"

    def ekf_observe_model_joint_iterated(self, h, arr, m, lm, gate, iterations, tol, pres, pit, nu, S):
        hyp = [int(lm[k]) for k in range(m)]
        ents = self._entries(arr, m)
        self.calls.append(("observe_joint_iterated", m, [(e["model"], e["z"].tolist()) for e in ents], hyp, gate, iterations, tol, bool(nu), bool(S)))
        if self.fail:
            return self.fail
        x1, P1, r, it = I.joint_update_iterated_dense(self.x, self.P, ents, hyp, iterations, tol, gate)
        res, out = pres._obj, pit._obj
        res.d2, res.dof, res.pairings, res.outcome, res.first_irregular = r["d2"], r["dof"], r["pairings"], r["outcome"], r["first_irregular"]
        out.used, out.converged, out.last_step, out.d2_last, out.irregular_at, out.irregular_obs = \
            it["used"], int(it["converged"]), it["step"], it["d2_last"], it["irregular_at"], it["irregular_obs"]
        out.ns = len(it["x_sub"])
        for q, v in enumerate(it["x_sub"]):
            out.x_sub[q] = v
        if nu:
            for q in range(2 * m):
                nu[q] = r["nu"][q]
        self.x, self.P = x1, P1
        return 0


def _engine(monkeypatch, x, P):
    from ekf_slam_amd import _lib as L
    rec = _Lib(x, P)
    monkeypatch.setattr(L, "lib", lambda: rec)
    return rec


def _filter(monkeypatch, x, P):
    from ekf_slam_amd import slam as S
    from ekf_slam_amd.trajectory import TrajectoryLog
    rec = _engine(monkeypatch, x, P)
    f = S.EKF_SLAM_UC(capacity=256)
    f.log = TrajectoryLog()
    return f, rec


def test_defaults_call_the_old_symbol_and_iterations_the_new_one(monkeypatch):
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import engine as E
    assert len(L.SIGNATURES["ekf_observe_model_joint_iterated"][1]) == 11 and len(L.SIGNATURES["ekf_joint_iterate"][1]) == 9
    x, P, ents, lms = I.scene_dense(5)
    rec = _engine(monkeypatch, x, P)
    e = E.Engine(capacity=256)
    plain = e.observe_model_joint(ents, lms)
    assert rec.calls[-1][0] == "observe_joint" and "used" not in plain
    rec.x, rec.P = x, P
    also = e.observe_model_joint(ents, lms, iterations=1, tol=0.5)
    assert rec.calls[-1][0] == "observe_joint" and also == plain
    rec.x, rec.P = x, P
    want, wit = I.joint_update_iterated_dense(x, P, ents, lms, 3, 1e-3)[2:]
    got = e.observe_model_joint(ents, lms, gate=1e9, want_nu=True, iterations=3, tol=1e-3)
    assert rec.calls[-1] == ("observe_joint_iterated", 5, [(en["model"], en["z"].tolist()) for en in ents], lms, 1e9, 3, 1e-3, True, False)
    assert len(rec.calls) == 3                                # one library call each
    for key in ("d2", "dof", "pairings", "outcome", "first_irregular"):
        assert got[key] == want[key], key
    assert (got["used"], got["converged"], got["step"]) == (wit["used"], wit["converged"], wit["step"])
    np.testing.assert_array_equal(got["nu"], want["nu"])
    # the 1-based wrapper: the old kind by default, the new kind with the controls, logged from the one array
    f, rec = _filter(monkeypatch, x, P)
    f.observe_model_joint(ents, [k + 1 for k in lms], gate=50.0)
    rec.x, rec.P = x, P
    one = f.observe_model_joint(ents, [k + 1 for k in lms], gate=50.0, iterations=3, tol=1e-3)
    assert [c[0] for c in rec.calls] == ["observe_joint", "observe_joint_iterated"] and rec.calls[-1][3:7] == (lms, 50.0, 3, 1e-3)
    assert one["first_irregular"] == 0 and one["used"] == wit["used"]
    assert [ed[1] for ed in f.log.edits] == ["observe_model_joint", "observe_model_joint_iterated"]
    step, kind, idx, slot, Rm = f.log.edits[1]
    assert (step, idx.tolist(), slot.tolist(), Rm.tolist()) == (0, [], [50.0, 1e-3], [[3.0, 0.0], [0.0, 0.0]])
    assert [(m, lm) for m, _, _, lm in f.log.model_joint_iterations[1]] == [(en["model"], lm + 1) for en, lm in zip(ents, lms)]
    assert list(f.log.model_joints) == [0]


def test_refusals_in_the_documented_order_and_a_failure_is_not_logged(monkeypatch):
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import engine as E
    x, P, ents, lms = I.scene_dense(2)
    f, rec = _filter(monkeypatch, x, P)
    e = E.Engine(capacity=256)
    for bad in ([1.5, 2], [-1, 2]):
        with pytest.raises(ValueError):
            f.observe_model_joint(ents, bad, iterations=3)
    with pytest.raises(ValueError):
        f.observe_model_joint([dict(ents[0], model=9)] + ents[1:], [1, 2], iterations=3)
    for bad in ([1], [1, 2, 3]):
        with pytest.raises(ValueError):
            f.observe_model_joint(ents, bad, iterations=3)
    with pytest.raises(ValueError):
        e.observe_model_joint(ents, lms, iterations=2.5)
    assert rec.calls == [] and f.log.edits == []
    rec.fail = L.EKF_ERR_STATE
    with pytest.raises(L.EkfError) as info:
        f.observe_model_joint(ents, [k + 1 for k in lms], iterations=3)
    assert info.value.status == L.EKF_ERR_STATE and "observe_model_joint_iterated" in str(info.value) and len(rec.calls) == 1 and f.log.edits == []


ITER_A = (T.JOINT_A[0], 11.5, 3, 1e-6)
ITER_LAST = (T.JOINT_LAST[0], float("inf"), 16, 0.0)


def make10():
    """test_observe_joint_cpu.make9()'s log with one relinearised joint update behind group B and one after the last step."""
    from ekf_slam_amd.trajectory import TrajectoryLog
    gen = T._generator()
    log = TrajectoryLog()
    gen.step(log, 0)
    gen.group_a(log, 8)
    log.record_model_observation_joint(*T.JOINT_A)
    gen.step(log, 1)
    gen.group_b(log, 8)
    log.record_model_observation_joint_iterated(*ITER_A)
    gen.step(log, 2)
    log.record_edit("constrain", [2, 1], None, None)
    log.record_model_observation_joint(*T.JOINT_LAST)
    log.record_model_observation_joint_iterated(*ITER_LAST)
    return log


def test_format_10_round_trip_and_replay(tmp_path):
    import test_trajectory_formats_cpu as F
    from ekf_slam_amd.trajectory import FORMAT_JOINT_ITERATED, _FORMATS, TrajectoryLog
    assert FORMAT_JOINT_ITERATED == _FORMATS[9] == "ekfslam-trajectory-10" and len(_FORMATS) == 10
    fixture = os.path.join(GOLDEN, "format10.npz")
    make10().save(tmp_path / "made.npz")
    assert same_npz(fixture, tmp_path / "made.npz")           # the recorders reproduce the pinned file
    assert str(np.load(fixture)["format"]) == FORMAT_JOINT_ITERATED
    log = TrajectoryLog.load(fixture)
    kinds = [ed[1] for ed in log.edits]
    assert len(log) == 3 and kinds.count("observe_model_joint_iterated") == 2 and kinds.count("observe_model_joint") == 2
    log.save(tmp_path / "again.npz")
    assert same_npz(fixture, tmp_path / "again.npz")

    class _Engine(F._Engine):
        def observe_model_joint(self, entries, landmarks, gate, iterations=1, tol=0.0):
            self.calls.append(("observe_model_joint", [(en["model"], F._l(en["z"]), F._l(en["R"])) for en in entries], list(landmarks), gate)
                              + ((iterations, tol) if iterations != 1 else ()))

    def call(spec):
        ents, gate = spec[:2]
        return ("observe_model_joint", [(m, list(z), np.asarray(R).tolist()) for m, z, R, _ in ents], [lm - 1 for _, _, _, lm in ents], gate) + tuple(spec[2:])

    want = F._step(0) + F._held(F.GROUP_A, 8) + [call(T.JOINT_A)] + F._step(1) + F._held(F.GROUP_B, 8) + [call(ITER_A)] + F._step(2) + \
        F._held(F.LAST, 8) + [call(T.JOINT_LAST), call(ITER_LAST)]
    whole = _Engine()
    log.replay(whole)
    assert whole.calls == want
    split = _Engine()
    log.replay(split, 0, 2)
    log.replay(split, 2)
    assert split.calls == want


def test_a_log_without_the_kind_still_saves_as_its_old_format(tmp_path):
    from ekf_slam_amd.trajectory import _FORMATS
    gen = T._generator()
    for n in range(1, 9):
        gen.make(n).save(tmp_path / ("format%d.npz" % n))
        assert same_npz(os.path.join(GOLDEN, "format%d.npz" % n), tmp_path / ("format%d.npz" % n)), n
        assert str(np.load(tmp_path / ("format%d.npz" % n))["format"]) == _FORMATS[n - 1]
    T.make9().save(tmp_path / "format9.npz")                  # (format 9's log is built beside its tests, not by make_logs.py)
    assert same_npz(os.path.join(GOLDEN, "format9.npz"), tmp_path / "format9.npz")
    assert str(np.load(tmp_path / "format9.npz")["format"]) == _FORMATS[8]


def test_measure_model_joint_applies_the_winner_as_one_iterated_joint_update(monkeypatch):
    x, P, _ = J.assert_scene_premises()
    scan = J.ambiguous_scene()[4]
    far = (M.RELATIVE_XY, [300.0, 300.0], RPOS, 77.0)
    # the default paths: the same calls as ever, whatever joint_iterations says without joint_update
    f, rec = _filter(monkeypatch, x, P)
    out, truncated = f.measure_model_joint([far, scan[1], scan[0]], J.GATE, 25.0, joint_iterations=3)
    assert out == [("new", J.N0 + 1), ("matched", J.LM_B + 1), ("matched", J.LM_A + 1)] and truncated is False
    assert [c[0] for c in rec.calls] == ["associate", "joint", "joint", "observe", "observe", "append"]
    f, rec = _filter(monkeypatch, x, P)
    f.measure_model_joint([far, scan[1], scan[0]], J.GATE, 25.0, joint_update=True)
    assert [c[0] for c in rec.calls] == ["associate", "joint", "joint", "observe_joint", "append"]
    assert [kind for _, kind, _, _, _ in f.log.edits] == ["observe_model_joint", "append_model"]
    # joint_update=True, joint_iterations=3: ONE iterated joint call with the winner's pairings in scan order, then the append
    f, rec = _filter(monkeypatch, x, P)
    out2, truncated2 = f.measure_model_joint([far, scan[1], scan[0]], J.GATE, 25.0, joint_update=True, joint_iterations=3, joint_tol=1e-9)
    assert out2 == out and truncated2 is False
    assert [c[0] for c in rec.calls] == ["associate", "joint", "joint", "observe_joint_iterated", "append"]
    call = [c for c in rec.calls if c[0] == "observe_joint_iterated"][0]
    assert call[1] == 2 and call[3] == [J.LM_B, J.LM_A] and call[4:7] == (C.INF, 3, 1e-9)
    assert [(m, z) for m, z in call[2]] == [(M.RELATIVE_XY, np.asarray(scan[1][1]).tolist()), (M.RELATIVE_XY, np.asarray(scan[0][1]).tolist())]
    assert [kind for _, kind, _, _, _ in f.log.edits] == ["observe_model_joint_iterated", "append_model"]
