"""CPU: a scan's pairings applied as ONE joint update (ekf_observe_model_joint).
  (a) the NumPy restatement of tests/observe_joint_cases.py: one pairing is model_obs_cases' single update, the joint update is the
      frozen-linearisation sequence, the premises of the shared scans;
  (b) tests/support/observe_joint_host_emulation.cpp: the kernel SOURCES of k_joint_factor and k_gather_joint and the pair loop of the pass,
      compiled for the host, against the restatement;
  (c) the Python layers' refusals over a stand-in for the library, in the documented order;
  (d) format 9 of the trajectory log;
  (e) measure_model_joint(joint_update=True) against a recording engine.
No GPU."""
import importlib.util
import os
import subprocess

import numpy as np
import pytest

import associate_model_cases as A
import joint_cases as J
import model_obs_cases as M
import observe_joint_cases as C
from helpers import ROOT, RPOS, RecorderBase, host_build, same_npz

GOLDEN = os.path.join(ROOT, "tests", "golden", "trajectory")


@pytest.fixture(scope="module")
def dense():
    return J.dense_state()


# ------------------------------------------------------------------------------------------------------------------
# (a) the restatement
# ------------------------------------------------------------------------------------------------------------------
def test_one_pairing_is_the_single_model_update(dense):
    x, P = dense
    ents, lms = C.scan_of(x, 4)
    for ent, lm in zip(ents, lms):
        o = J.pairing_obs(ent, lm)
        xs, Ps, single = M.observe_model_dense(x, P, o)
        xj, Pj, rec = C.joint_update_dense(x, P, [ent], [lm])
        err = max(np.abs(xj - xs).max() / np.abs(xs).max(), np.abs(Pj - Ps).max() / np.abs(Ps).max())
        print("model %d at landmark %d: joint update of one pairing against the single update %.2e" % (ent["model"], lm, err))
        assert err <= 1e-12 and rec["outcome"] == C.APPLIED == single["outcome"]
        np.testing.assert_allclose(rec["d2"], single["d2"], rtol=1e-12)
        np.testing.assert_array_equal(rec["nu"], single["nu"])
        assert rec["dof"] == M.ROWS[ent["model"]]


def test_the_joint_update_is_the_frozen_sequence_and_the_scans_premises_hold(dense):
    x, P = dense
    for npair, cond, eig, chol, frozen in C.assert_scan_premises():
        assert frozen <= 1e-12
    # an entry left out occupies no rows; scan order does not matter to the joint update
    ents, lms = C.scan_of(x, 5)
    hyp = list(lms)
    hyp[1] = -1
    xa, Pa, ra = C.joint_update_dense(x, P, ents, hyp)
    keep = [0, 2, 3, 4]
    xb, Pb, rb = C.joint_update_dense(x, P, [ents[k] for k in keep], [lms[k] for k in keep])
    np.testing.assert_array_equal(xa, xb); np.testing.assert_array_equal(Pa, Pb)
    xf, Pf = C.frozen_sequence(x, P, ents, hyp)
    assert np.abs(xf - xa).max() / np.abs(xa).max() <= 1e-12 and np.abs(Pf - Pa).max() / np.abs(Pa).max() <= 1e-12
    back = keep[::-1]
    xc, Pc, _ = C.joint_update_dense(x, P, [ents[k] for k in back], [lms[k] for k in back])
    assert np.abs(xc - xa).max() / np.abs(xa).max() <= 1e-12 and np.abs(Pc - Pa).max() / np.abs(Pa).max() <= 1e-12
    assert (ra["pairings"], ra["dof"]) == (4, sum(M.ROWS[ents[k]["model"]] for k in keep))


def test_gated_and_irregular_leave_the_dense_state_alone(dense):
    x, P = dense
    ents, lms = C.scan_of(x, 3)
    d2 = J.joint_dense(x, P, ents, lms)["d2"]
    xg, Pg, rg = C.joint_update_dense(x, P, ents, lms, gate=0.5 * d2)
    assert rg["outcome"] == C.GATED and rg["d2"] == d2
    np.testing.assert_array_equal(xg, x); np.testing.assert_array_equal(Pg, P)
    on_robot = x.copy()
    on_robot[3 + 2 * lms[1]:5 + 2 * lms[1]] = x[:2]
    xi, Pi, ri = C.joint_update_dense(on_robot, P, ents, lms)
    assert (ri["outcome"], ri["first_irregular"]) == (C.IRREGULAR, 1)
    np.testing.assert_array_equal(xi, on_robot); np.testing.assert_array_equal(Pi, P)
    xe, Pe, re_ = C.joint_update_dense(x, P, ents, [-1, -1, -1])
    assert (re_["outcome"], re_["d2"], re_["pairings"]) == (C.APPLIED, 0.0, 0)
    np.testing.assert_array_equal(xe, x); np.testing.assert_array_equal(Pe, P)


# ------------------------------------------------------------------------------------------------------------------
# (b) the kernel sources on the host
# ------------------------------------------------------------------------------------------------------------------
def test_kernel_sources_on_the_host_against_the_restatement(tmp_path):
    """observe_joint_host_emulation.cpp runs k_joint_factor, k_gather_joint and the pass's pair loop on N = 40 and N = 41 (a padded tail),
    T = 16, for np = 1, 2, 5 and 32 and writes, per case, the state before and after; here the restatement is applied to the state
    before."""
    exe = host_build("observe_joint_host_emulation", str(tmp_path / "observe_joint_host_emulation"))
    out = tmp_path / "cases.bin"
    r = subprocess.run([exe, str(out)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    raw = np.fromfile(out, dtype=np.float64)
    pos, seen = 0, []
    while pos < raw.size:
        n, m, outcome = int(raw[pos]), int(raw[pos + 1]), int(raw[pos + 2]); pos += 3
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
        d2 = raw[pos]; pos += 1
        ex, eP, want = C.joint_update_dense(x0, P0, ents, hyp, gate=C.INF if outcome != C.GATED else 0.0)
        assert want["outcome"] == outcome
        npair = sum(1 for h in hyp if h >= 0)
        if outcome == C.APPLIED:
            err_x, err_P = np.abs(x1 - ex).max() / np.abs(ex).max(), np.abs(P1 - eP).max() / np.abs(eP).max()
            print("np = %2d (m = %d): emulated kernels against the restatement: rel err x %.2e P %.2e, d2 %.6g" % (npair, m, err_x, err_P, d2))
            assert err_x <= 1e-12 and err_P <= 1e-12
            np.testing.assert_allclose(d2, want["d2"], rtol=1e-10)
            np.testing.assert_array_equal(P1, P1.T)
        else:
            np.testing.assert_array_equal(x1, x0); np.testing.assert_array_equal(P1, P0)
        seen.append((npair, outcome))
    assert sorted(p for p, o in seen if o == C.APPLIED) == [1, 2, 5, 32, 32] and {o for _, o in seen} == {C.APPLIED, C.GATED, C.IRREGULAR}


# ------------------------------------------------------------------------------------------------------------------
# (c) - (e) the Python layers over a stand-in for the library
# ------------------------------------------------------------------------------------------------------------------
class _Lib(RecorderBase):
    last_error = b"observe_model_joint: injected"

    def __init__(self, x, P):
        self.x, self.P, self.calls, self.fail = np.asarray(x), np.asarray(P), [], 0

    @property
    def N(self):
        return (self.x.size - 3) // 2

    @staticmethod
    def _entries(arr, m):
        out = []
        for k in range(m):
            Rm = np.array(list(arr[k].R)).reshape(2, 2, order="F")
            rows = M.ROWS[arr[k].model]
            out.append(A.entry(arr[k].model, list(arr[k].z), Rm if rows == 2 else Rm[0, 0], arr[k].gate))
        return out

    def ekf_num_landmarks(self, h, pn):
        pn._obj.value = self.N
        return 0

    def ekf_associate_model(self, h, arr, m, out, d2_all):
        ents = self._entries(arr, m)
        self.calls.append(("associate", m, bool(d2_all)))
        res, D = A.match(self.x, self.P, ents)
        for k in range(m):
            out[k].best, out[k].second, out[k].d2_best, out[k].d2_second = int(res["best"][k]), int(res["second"][k]), res["d2_best"][k], res["d2_second"][k]
            out[k].within_gate, out[k].irregular = int(res["within_gate"][k]), int(res["irregular"][k])
        if d2_all:
            for q, v in enumerate(D.reshape(-1)):
                d2_all[q] = v
        return 0

    def ekf_joint_innovation(self, h, arr, m, hyp, nh, out, prefix, nu, S):
        hyps = [[int(hyp[i * m + k]) for k in range(m)] for i in range(nh)]
        self.calls.append(("joint", m, hyps))
        ents = self._entries(arr, m)
        for i, hy in enumerate(hyps):
            r = J.joint_dense(self.x, self.P, ents, hy)
            out[i].d2, out[i].dof, out[i].pairings, out[i].outcome, out[i].first_irregular = r["d2"], r["dof"], r["pairings"], r["outcome"], r["first_irregular"]
            for k in range(m):
                if prefix:
                    prefix[i * m + k] = r["d2_prefix"][k]
        return 0

    def ekf_observe_model_joint(self, h, arr, m, lm, gate, pres, nu, S):
        hyp = [int(lm[k]) for k in range(m)]
        ents = self._entries(arr, m)
        self.calls.append(("observe_joint", m, [(e["model"], e["z"].tolist()) for e in ents], hyp, gate, bool(nu), bool(S)))
        if self.fail:
            return self.fail
        x1, P1, r = C.joint_update_dense(self.x, self.P, ents, hyp, gate)
        res = pres._obj
        res.d2, res.dof, res.pairings, res.outcome, res.first_irregular = r["d2"], r["dof"], r["pairings"], r["outcome"], r["first_irregular"]
        if nu:
            for q in range(2 * m):
                nu[q] = r["nu"][q]
        if S:
            for q, v in enumerate(r["S"].reshape(-1, order="F")):
                S[q] = v
        self.x, self.P = x1, P1
        return 0

    def ekf_observe_model(self, h, pobs, pres):
        o = pobs._obj
        self.calls.append(("observe", o.model, list(o.z), list(o.lm), o.gate, pres is not None))
        return 0

    def ekf_append_model(self, h, arr, m, pfirst):
        self.calls.append(("append", m))
        pfirst._obj.value = self.N
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


def test_engine_and_wrapper_marshal_once_and_unpack(monkeypatch, dense):
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import engine as E
    assert "ekf_observe_model_joint" in L.SIGNATURES and len(L.SIGNATURES["ekf_observe_model_joint"][1]) == 8
    x, P = dense
    rec = _engine(monkeypatch, x, P)
    e = E.Engine(capacity=256)
    ents, lms = C.scan_of(x, 3)
    hyp = [lms[0], -1, lms[2]]
    want = C.joint_update_dense(x, P, ents, hyp)[2]
    got = e.observe_model_joint(ents, hyp, want_nu=True, want_S=True)
    assert rec.calls[-1][1:] == (3, [(en["model"], en["z"].tolist()) for en in ents], hyp, C.INF, True, True)
    for key in ("d2", "dof", "pairings", "outcome", "first_irregular"):
        assert got[key] == want[key], key
    np.testing.assert_array_equal(got["nu"], want["nu"]); np.testing.assert_array_equal(got["S"], want["S"])
    lean = e.observe_model_joint(ents, hyp, gate=0.0)
    assert rec.calls[-1][4:] == (0.0, False, False) and "nu" not in lean and "S" not in lean and lean["outcome"] == C.GATED
    # the 1-based wrapper: 0 = left out, first_irregular 1-based with 0 = none; ONE struct array, sent and logged from
    f, rec = _filter(monkeypatch, x, P)
    one = f.observe_model_joint(ents, [lms[0] + 1, 0, lms[2] + 1], gate=50.0)
    assert rec.calls[-1][3] == hyp and rec.calls[-1][4] == 50.0 and one["first_irregular"] == 0 and one["pairings"] == 2
    (step, kind, idx, slot, Rm), = f.log.edits
    assert (step, kind, idx.tolist(), slot.tolist(), Rm.tolist()) == (0, "observe_model_joint", [], [50.0, 0.0], [[0.0, 0.0], [0.0, 0.0]])
    logged = f.log.model_joints[0]
    assert [(m, lm) for m, _, _, lm in logged] == [(en["model"], lm) for en, lm in zip(ents, [lms[0] + 1, 0, lms[2] + 1])]
    for (m, z, Rk, _), en in zip(logged, ents):
        rows = M.ROWS[m]
        np.testing.assert_array_equal(z[:rows], en["z"]); assert not z[rows:].any()
        np.testing.assert_array_equal(Rk if rows == 2 else Rk[0, 0], en["R"])


def test_refusals_in_the_documented_order_and_a_failure_is_not_logged(monkeypatch, dense):
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import engine as E
    x, P = dense
    f, rec = _filter(monkeypatch, x, P)
    e = E.Engine(capacity=256)
    ents, lms = C.scan_of(x, 3)
    # the wrapper: whole numbers, then 1-based with 0 = left out, then the entries' shapes, then the count -- before the library is asked
    for bad in ([1.5, 0, 2], [-1, 0, 2]):
        with pytest.raises(ValueError):
            f.observe_model_joint(ents, bad)
    with pytest.raises(ValueError):
        f.observe_model_joint([dict(ents[0], model=9)] + ents[1:], [1, 2, 3])
    with pytest.raises(ValueError):
        f.observe_model_joint([dict(ents[0], R=np.eye(3))] + ents[1:], [1, 2, 3])
    for bad in ([1, 2], [1, 2, 3, 4]):
        with pytest.raises(ValueError):
            f.observe_model_joint(ents, bad)
    for bad in ([0, 1], [0.5, 1, 2]):
        with pytest.raises(ValueError):
            e.observe_model_joint(ents, bad)
    assert rec.calls == [] and f.log.edits == []
    # what the library refuses arrives as EkfError with the call's name, and nothing is logged
    rec.fail = L.EKF_ERR_STATE
    with pytest.raises(L.EkfError) as info:
        f.observe_model_joint(ents, [k + 1 for k in lms])
    assert info.value.status == L.EKF_ERR_STATE and "observe_model_joint" in str(info.value) and len(rec.calls) == 1 and f.log.edits == []


# ------------------------------------------------------------------------------------------------------------------
# (d) format 9
# ------------------------------------------------------------------------------------------------------------------
def _generator():
    spec = importlib.util.spec_from_file_location("make_logs", os.path.join(GOLDEN, "make_logs.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


JOINT_A = ([(1, [5.0, 30.0], np.array([[0.5, 0.125], [0.125, 0.25]]), 4), (2, [7.5, 0.0], [[0.5, 0.0], [0.0, 0.0]], 0),
            (4, [2.0, -1.0], [[1.0, 0.25], [0.25, 0.5]], 2)], 11.5)
JOINT_LAST = ([(3, [12.0, 0.0], [[0.25, 0.0], [0.0, 0.0]], 6)], float("inf"))


def make9():
    """make_logs.make(8)'s log with one joint update behind group A and one after the last step."""
    from ekf_slam_amd.trajectory import TrajectoryLog
    gen = _generator()
    log = TrajectoryLog()
    gen.step(log, 0)
    gen.group_a(log, 8)
    log.record_model_observation_joint(*JOINT_A)
    gen.step(log, 1)
    gen.group_b(log, 8)
    gen.step(log, 2)
    log.record_edit("constrain", [2, 1], None, None)
    log.record_model_observation_joint(*JOINT_LAST)
    return log


def test_format_9_round_trip_and_replay(tmp_path):
    import test_trajectory_formats_cpu as F
    from ekf_slam_amd.trajectory import FORMAT_JOINT, _FORMATS, TrajectoryLog
    assert FORMAT_JOINT == _FORMATS[8] == "ekfslam-trajectory-9"
    fixture = os.path.join(GOLDEN, "format9.npz")
    make9().save(tmp_path / "made.npz")
    assert same_npz(fixture, tmp_path / "made.npz")           # the recorders reproduce the pinned file
    assert str(np.load(fixture)["format"]) == FORMAT_JOINT
    log = TrajectoryLog.load(fixture)
    assert len(log) == 3 and [ed[1] for ed in log.edits].count("observe_model_joint") == 2
    log.save(tmp_path / "again.npz")
    assert same_npz(fixture, tmp_path / "again.npz")

    class _Engine(F._Engine):
        def observe_model_joint(self, entries, landmarks, gate):
            self.calls.append(("observe_model_joint", [(en["model"], F._l(en["z"]), F._l(en["R"])) for en in entries], list(landmarks), gate))

    def call(spec):
        ents, gate = spec
        return ("observe_model_joint", [(m, list(z), np.asarray(R).tolist()) for m, z, R, _ in ents], [lm - 1 for _, _, _, lm in ents], gate)

    want = F._step(0) + F._held(F.GROUP_A, 8) + [call(JOINT_A)] + F._step(1) + F._held(F.GROUP_B, 8) + F._step(2) + F._held(F.LAST, 8) + [call(JOINT_LAST)]
    whole = _Engine()
    log.replay(whole)
    assert whole.calls == want
    split = _Engine()
    log.replay(split, 0, 2)
    log.replay(split, 2)
    assert split.calls == want


def test_a_log_without_the_kind_still_saves_as_its_old_format(tmp_path):
    from ekf_slam_amd.trajectory import _FORMATS
    gen = _generator()
    for n in range(1, 9):
        gen.make(n).save(tmp_path / ("format%d.npz" % n))
        assert same_npz(os.path.join(GOLDEN, "format%d.npz" % n), tmp_path / ("format%d.npz" % n)), n
        assert str(np.load(tmp_path / ("format%d.npz" % n))["format"]) == _FORMATS[n - 1]


# ------------------------------------------------------------------------------------------------------------------
# (e) the policy
# ------------------------------------------------------------------------------------------------------------------
def test_measure_model_joint_applies_the_winner_as_one_joint_update(monkeypatch):
    x, P, _ = J.assert_scene_premises()
    scan = J.ambiguous_scene()[4]
    far = (M.RELATIVE_XY, [300.0, 300.0], RPOS, 77.0)
    # today's path: the same calls as ever
    f, rec = _filter(monkeypatch, x, P)
    out, truncated = f.measure_model_joint([far, scan[1], scan[0]], J.GATE, 25.0)
    assert out == [("new", J.N0 + 1), ("matched", J.LM_B + 1), ("matched", J.LM_A + 1)] and truncated is False
    assert [c[0] for c in rec.calls] == ["associate", "joint", "joint", "observe", "observe", "append"]
    assert [c[3] for c in rec.calls if c[0] == "observe"] == [[J.LM_B, -1], [J.LM_A, -1]]
    assert [kind for _, kind, _, _, _ in f.log.edits] == ["observe_model", "observe_model", "append_model"]
    # joint_update=True: ONE joint call with the winner's pairings in scan order, then the append
    f, rec = _filter(monkeypatch, x, P)
    out2, truncated2 = f.measure_model_joint([far, scan[1], scan[0]], J.GATE, 25.0, joint_update=True)
    assert out2 == out and truncated2 is False
    assert [c[0] for c in rec.calls] == ["associate", "joint", "joint", "observe_joint", "append"]
    call = [c for c in rec.calls if c[0] == "observe_joint"][0]
    assert call[1] == 2 and call[3] == [J.LM_B, J.LM_A] and call[4] == C.INF
    assert [(m, z) for m, z in call[2]] == [(M.RELATIVE_XY, np.asarray(scan[1][1]).tolist()), (M.RELATIVE_XY, np.asarray(scan[0][1]).tolist())]
    assert [kind for _, kind, _, _, _ in f.log.edits] == ["observe_model_joint", "append_model"]
    # nothing matched: no joint call at all
    f, rec = _filter(monkeypatch, x, P)
    out3, _ = f.measure_model_joint([far], J.GATE, 25.0, joint_update=True)
    assert out3 == [("new", J.N0 + 1)] and [c[0] for c in rec.calls] == ["associate", "append"]
