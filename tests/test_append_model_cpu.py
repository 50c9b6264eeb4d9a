"""CPU: ekf_append_model without a GPU -- the compiled ekfm::model_invert of ekf_slam_amd/csrc/device_math.h against the closed forms of
tests/append_model_cases.py, finite differences and the Jacobian relations with ekfm::model_eval; k_append_model's source compiled for the
host (a batch against single launches bit for bit, every case against the dense restatement); the seventh kind of the trajectory log;
the argument handling of the Python layers over a stand-in for the library; the MEX gateway's command under the MEX mock."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import append_model_cases as A
import model_obs_cases as M
from helpers import REL, RPOS, RecorderBase, host_build, line_program, same_npz
from mex_harness import PRELUDE_SHOWN, ROOT, driver, driver_without, transcript_of


# ------------------------------------------------------------------------------------------------------------------
# the compiled model_invert
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """The stand-alone host build of ekfm::model_invert (and model_eval at the point it returns): host(cases) -> one dict per case."""
    rows_of = line_program(tmp_path_factory, "model_invert_host")

    def run(cases):
        lines = ["invert %d %s" % (m, " ".join(repr(float(v)) for v in list(xr) + list(z))) for m, xr, z in cases]
        return [dict(ok=r[0] == 1, t=np.array(r[1:3]), gth=np.array(r[3:5]), Gz=np.array(r[5:9]).reshape(2, 2), posed=r[9] == 1,
                     hx=np.array(r[10:12]), H=np.array(r[12:26]).reshape(2, 7)) for r in rows_of(lines)]
    return run


def _random_cases(rng, n):
    out = []
    for _ in range(n):
        xr = np.array([rng.uniform(-30, 30), rng.uniform(-30, 30), rng.uniform(-720, 720)])
        out.append((M.RANGE_BEARING, xr, np.array([rng.uniform(0.5, 40.0), rng.uniform(-400, 400)])))
        out.append((M.RELATIVE_XY, xr, rng.uniform(-30, 30, 2)))
    return out


def test_hand_derived_answers_at_right_angles(host):
    # theta = 90, bearing 90: the landmark lies 5 along -x; cosd / sind are exact there, so t and Gz are exact
    rb, xy, xy0 = host([(M.RANGE_BEARING, [1.0, 2.0, 90.0], [5.0, 90.0]), (M.RELATIVE_XY, [1.0, 2.0, 90.0], [5.0, 3.0]),
                        (M.RELATIVE_XY, [1.0, 2.0, 33.0], [0.0, 0.0])])
    assert rb["ok"] and rb["t"].tolist() == [-4.0, 2.0] and rb["Gz"][:, 0].tolist() == [-1.0, 0.0]
    assert rb["gth"].tolist() == [-0.0, -5.0 / M.K] and rb["Gz"][:, 1].tolist() == rb["gth"].tolist()
    # the robot looks along +y: 5 ahead and 3 to the left is (1 - 3, 2 + 5); turning the robot moves that point along (-5, -3) / k
    assert xy["ok"] and xy["t"].tolist() == [-2.0, 7.0] and xy["Gz"].tolist() == [[0.0, -1.0], [1.0, 0.0]]
    assert xy["gth"].tolist() == [-5.0 / M.K, -3.0 / M.K]
    assert xy["hx"].tolist() == [5.0, 3.0]                    # tests/test_model_obs_cpu.py's case, run backwards
    # a relative position of zero is the robot's own position: a point, though no model observes it (q = 0)
    assert xy0["ok"] and xy0["t"].tolist() == [1.0, 2.0] and not xy0["gth"].any() and not xy0["posed"]
    # the models that do not determine a point are refused
    for m in (0, M.RANGE, M.BEARING, M.LANDMARK_RANGE, 6):
        assert not host([(m, [1.0, 2.0, 3.0], [4.0, 5.0])])[0]["ok"]


def test_compiled_model_invert_matches_closed_forms_finite_differences_and_the_model(host):
    rng = np.random.default_rng(31)
    cases = _random_cases(rng, 40)
    fd_err = 0.0
    for m, xr, z in cases:                                    # the finite-difference error of the NumPy forms themselves: the yardstick
        Gx, Gz = A.G_of(m, xr, z)
        fx, fz = A.G_fd(m, xr, z)
        fd_err = max(fd_err, np.abs(fx - Gx).max() / np.abs(Gx).max(), np.abs(fz - Gz).max() / np.abs(Gz).max())
    print("finite differences (step 1e-6) against the NumPy closed forms: worst rel err %.2e" % fd_err)
    assert 0.0 < fd_err < 1e-6
    worst = dict(t=0.0, G=0.0, fd=0.0, back=0.0, HtGz=0.0, HrGx=0.0)
    for (m, xr, z), got in zip(cases, host(cases)):
        assert got["ok"] and got["posed"]
        Gx = np.array([[1.0, 0.0, got["gth"][0]], [0.0, 1.0, got["gth"][1]]])
        wGx, wGz = A.G_of(m, xr, z)
        fx, fz = A.G_fd(m, xr, z)
        scale = max(np.abs(xr[:2]).max(), np.abs(z).max(), 1.0)
        worst["t"] = max(worst["t"], np.abs(got["t"] - A.g_of(m, xr, z)).max() / scale)
        worst["G"] = max(worst["G"], np.abs(Gx - wGx).max() / np.abs(wGx).max(), np.abs(got["Gz"] - wGz).max() / np.abs(wGz).max())
        worst["fd"] = max(worst["fd"], np.abs(Gx - fx).max() / np.abs(wGx).max(), np.abs(got["Gz"] - fz).max() / np.abs(wGz).max())
        # h(g(x, z)) = z: the compiled model_eval at the compiled t (a bearing up to whole turns)
        back = got["hx"] - z
        if m == M.RANGE_BEARING:
            back[1] = M.wrap180(back[1])
        worst["back"] = max(worst["back"], np.abs(back).max() / max(np.abs(z).max(), 1.0))
        # H_t Gz = I and H_r + H_t Gx = 0, with the closed forms of tests/model_obs_cases.py at the compiled t and with the compiled H
        for H in (M.H_of(m, xr, got["t"]), got["H"]):
            Hr, Ht = H[:, :3], H[:, 3:5]
            worst["HtGz"] = max(worst["HtGz"], np.abs(Ht @ got["Gz"] - np.eye(2)).max())
            worst["HrGx"] = max(worst["HrGx"], np.abs(Hr + Ht @ Gx).max() / max(np.abs(Hr).max(), 1.0))
    print("compiled model_invert: rel err %s" % ", ".join("%s %.2e" % kv for kv in worst.items()))
    assert worst["t"] < 1e-12 and worst["G"] < 1e-12 and worst["fd"] < 10.0 * fd_err
    assert worst["back"] < 1e-12 and worst["HtGz"] < 1e-12 and worst["HrGx"] < 1e-12


def test_the_dense_restatement_is_the_block_form_of_the_joint_covariance():
    # (x_r, old map, z_0, z_1, ..) are jointly Gaussian with covariance blockdiag(P, R_0, R_1, ..); the new state is a function of them
    # with the Jacobian J = [I 0; A Gz]: P' = J blockdiag(P, R) J'
    import linear_obs_cases as C
    rng = np.random.default_rng(8)
    x, P, _ = C.random_state(rng, 5)
    s = np.arange(1.0, 6.0)
    entries = A.scan(rng, 4)
    x2, s2, P2 = A.append_model_dense(x, s, P, entries)
    n, m = x.size, len(entries)
    J = np.zeros((n + 2 * m, n + 2 * m))
    J[:n, :n] = np.eye(n)
    big = np.zeros((n + 2 * m, n + 2 * m))
    big[:n, :n] = P
    for b, (model, z, R, sig) in enumerate(entries):
        Gx, Gz = A.G_of(model, x[:3], z)
        J[n + 2 * b:n + 2 * b + 2, :3] = Gx
        J[n + 2 * b:n + 2 * b + 2, n + 2 * b:n + 2 * b + 2] = Gz
        big[n + 2 * b:n + 2 * b + 2, n + 2 * b:n + 2 * b + 2] = R
        np.testing.assert_array_equal(x2[n + 2 * b:n + 2 * b + 2], A.g_of(model, x[:3], z))
    np.testing.assert_allclose(P2, J @ big @ J.T, rtol=0, atol=1e-13 * np.abs(P2).max())
    assert s2.tolist() == s.tolist() + [e[3] for e in entries] and np.linalg.eigvalsh(P2).min() > 0.0
    # ... and the observation of the same z then finds nu = 0 and S = 2 R
    for b, (model, z, R, sig) in enumerate(entries):
        res = M.observe_model_dense(x2, P2, M.obs(model, z, R, [5 + b]))[2]
        assert np.abs(res["nu"]).max() < 1e-12 * max(np.abs(z).max(), 1.0) and np.abs(res["S"] - 2 * R).max() < 1e-12 * np.abs(R).max() * 1e3


# ------------------------------------------------------------------------------------------------------------------
# the kernel source, compiled for the host
# ------------------------------------------------------------------------------------------------------------------
def test_kernel_source_on_the_host_batches_bit_for_bit_and_matches_the_dense_restatement(tmp_path):
    """tests/support/append_model_host_emulation.cpp: k_append_model with m = 1, 3, 9 entries against m launches of one, tiles of edge 16
    and 64, double and float, 0 and 3 pairs pending; then every case's new rows against append_model_dense on the live state before."""
    exe = host_build("append_model_host_emulation", str(tmp_path / "append_model_host_emulation"))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    lines = r.stdout.strip().split("\n")
    assert r.returncode == 0, r.stdout[-3000:]
    assert len(lines) == 24 and all(ln.endswith(": 0 differences") for ln in lines), r.stdout[-3000:]
    worst = {}
    for ts in ("double", "float"):
        for T in (16, 64):
            for pending in (0, 3):
                raw = np.fromfile(tmp_path / ("before_%s_%d_%d.bin" % (ts, T, pending)))
                n0 = int(raw[0]); N = (n0 - 3) // 2
                x0, s0, P0 = raw[1:1 + n0], raw[1 + n0:1 + n0 + N], raw[1 + n0 + N:].reshape(n0, n0)
                assert N == 123 and raw.size == 1 + n0 + N + n0 * n0
                for m in (1, 3, 9):
                    raw = np.fromfile(tmp_path / ("after_%s_%d_%d_%d.bin" % (ts, T, pending, m)))
                    n1 = n0 + 2 * m
                    ent, xt, st, rows = raw[:8 * m].reshape(m, 8), raw[8 * m:10 * m], raw[10 * m:11 * m], raw[11 * m:].reshape(2 * m, n1)
                    entries = [A.entry(int(e[0]), e[1:3], [[e[3], e[4]], [e[5], e[6]]], e[7]) for e in ent]
                    assert {e[0] for e in entries} <= {M.RANGE_BEARING, M.RELATIVE_XY} and (m == 1 or len({e[0] for e in entries}) == 2)
                    ex, es, eP = A.append_model_dense(x0, s0, P0, entries)
                    np.testing.assert_array_equal(st, es[N:])
                    err_x = np.abs(xt - ex[n0:]).max() / np.abs(ex).max()
                    err_P = np.abs(rows - eP[n0:]).max() / np.abs(eP).max()
                    worst[ts] = max(worst.get(ts, 0.0), err_x, err_P)
                    assert err_x < REL and err_P < REL, (ts, T, pending, m, err_x, err_P)
    print("k_append_model on the host against the dense restatement: worst rel err %s" % worst)
    assert worst["double"] < 1e-12                            # F64 tiles: rounding alone; float tiles: one float rounding of the largest entry


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

    def observe_model(self, model, z, R, landmarks, anchor=None, gate=float("inf")):
        self.calls.append(("observe_model", model, list(landmarks)))

    def append_model(self, entries):
        self.calls.append(("append_model", [(m, z.tolist(), R.tolist(), s) for m, z, R, s in entries]))


def _steps(log, n):
    for k in range(n):
        log.record([0.1, 1.0 + k], np.array([[1.0, 2.0, 3.0]]) if k % 2 else None, [1.0, 2.0], [[0.0, 1.0], [2.0, 3.0]])


def test_trajectory_format_six_round_trip_and_the_older_formats(tmp_path):
    from ekf_slam_amd.trajectory import (FORMAT, FORMAT_APPEND, FORMAT_BATCH, FORMAT_EDITS, FORMAT_MODEL, FORMAT_OBSERVE, TrajectoryLog)
    assert FORMAT_APPEND == "ekfslam-trajectory-6"
    base_keys = {"format", "u", "obs_ptr", "obs", "lm_ptr", "lm_index", "lm_loc"}
    edit_keys = base_keys | {"edit_step", "edit_kind", "edit_ptr", "edit_idx", "edit_delta", "edit_R"}
    observe_keys = edit_keys | {"observe_edit", "observe_Hr", "observe_Hl", "observe_gate", "observe_wrap", "observe_rows"}
    model_keys = observe_keys | {"model_edit", "model_id", "model_anchor", "model_gate"}
    # logs without a model append are written as versions 1 - 5, with the arrays they always had, and a loaded one saves byte for
    # byte what it was loaded from
    one = TrajectoryLog(); _steps(one, 3)
    two = TrajectoryLog(); _steps(two, 2); two.record_edit("constrain", [1, 2], [0.5, 0.0], RPOS)
    three = TrajectoryLog(); _steps(three, 2); three.record_edit("merge_batch", [3, 5, 1, 2])
    four = TrajectoryLog(); _steps(four, 2); four.record_edit("remove", [7])
    four.record_observation([1.0, 2.0], RPOS, np.ones((2, 3)), [4, 2], [np.eye(2), -np.eye(2)], gate=9.21, wrap=(0, 1), rows=2)
    five = TrajectoryLog(); _steps(five, 2); five.record_model_observation(M.RANGE_BEARING, [5.0, 30.0], RPOS, [4], gate=9.21)
    five.record_observation([175.0], [[0.5, 0.0], [0.0, 0.0]], [[0.0, 0.0, 1.0], [0.0, 0.0, 0.0]], wrap=(1, 0), rows=1)
    for log, name, fmt, keys in ((one, "one", FORMAT, base_keys), (two, "two", FORMAT_EDITS, edit_keys), (three, "three", FORMAT_BATCH, edit_keys),
                                 (four, "four", FORMAT_OBSERVE, observe_keys), (five, "five", FORMAT_MODEL, model_keys)):
        log.save(tmp_path / (name + ".npz"))
        g = np.load(tmp_path / (name + ".npz"))
        assert str(g["format"]) == fmt and set(g.files) == keys
        back = TrajectoryLog.load(tmp_path / (name + ".npz"))
        assert len(back) == len(log) and len(back.edits) == len(log.edits) and back.model_appends == {}
        back.save(tmp_path / (name + "_again.npz"))
        assert same_npz(tmp_path / (name + ".npz"), tmp_path / (name + "_again.npz"))
    # version 6: scans of new landmarks among the other edits
    scan3 = A.scan(np.random.default_rng(1), 3, 700.0)
    six = TrajectoryLog(); _steps(six, 2)
    six.record_edit("remove", [7])
    six.record_model_append(scan3)
    six.record_model_observation(M.RELATIVE_XY, [2.0, -1.0], RPOS, [9])
    _steps(six, 2)
    six.record_model_append([(M.RANGE_BEARING, [4.0, 370.0], RPOS, 41.0)])
    six.save(tmp_path / "six.npz")
    g = np.load(tmp_path / "six.npz")
    assert str(g["format"]) == FORMAT_APPEND and g["edit_kind"].tolist() == [0, 6, 5, 6]
    assert set(g.files) == model_keys | {"append_edit", "append_ptr", "append_model", "append_z", "append_R", "append_signature"}
    assert g["append_edit"].tolist() == [1, 3] and g["append_ptr"].tolist() == [0, 3, 4] and g["append_model"].tolist() == [1, 4, 1, 1]
    assert g["append_signature"].tolist() == [700.0, 701.0, 702.0, 41.0] and g["observe_edit"].size == 0 and g["model_edit"].tolist() == [2]
    back = TrajectoryLog.load(tmp_path / "six.npz")
    assert len(back) == 4 and [(e[0], e[1], e[2].tolist()) for e in back.edits] == \
        [(2, "remove", [7]), (2, "append_model", []), (2, "observe_model", [9]), (4, "append_model", [])]
    assert sorted(back.model_appends) == [1, 3] and len(back.model_appends[1]) == 3
    for got, want in zip(back.model_appends[1], scan3):
        assert got[0] == want[0] and got[3] == want[3]
        np.testing.assert_array_equal(got[1], want[1]); np.testing.assert_array_equal(got[2], want[2])
    back.save(tmp_path / "six_again.npz")
    assert same_npz(tmp_path / "six.npz", tmp_path / "six_again.npz")
    r = _Replayed()
    back.replay(r)
    assert r.calls == [("predict",), ("predict",), ("measure",), ("remove", [6]),
                       ("append_model", [(m, z.tolist(), R.tolist(), s) for m, z, R, s in scan3]), ("observe_model", 4, [8]),
                       ("predict",), ("predict",), ("measure",),
                       ("append_model", [(1, [4.0, 370.0], RPOS.tolist(), 41.0)])]
    only = TrajectoryLog(); _steps(only, 1)
    only.record_model_append(scan3[:1])
    only.save(tmp_path / "only.npz")
    back = TrajectoryLog.load(tmp_path / "only.npz")
    assert str(np.load(tmp_path / "only.npz")["format"]) == FORMAT_APPEND and back.observations == {} and back.model_observations == {}
    assert list(back.model_appends) == [0]
    # bad shapes are refused and nothing is recorded
    bad = TrajectoryLog()
    for entries in ([], [(1, [1.0], RPOS, 1.0)], [(1, [1.0, 2.0], [1.0, 2.0], 1.0)], [(1, [1.0, 2.0], RPOS)]):
        with pytest.raises(ValueError):
            bad.record_model_append(entries)
    with pytest.raises(ValueError):
        bad.record_edit("append_model", [])                   # scans of new landmarks have their own recorder
    assert bad.edits == [] and bad.model_appends == {}


# ------------------------------------------------------------------------------------------------------------------
# the Python layers over a stand-in for the library
# ------------------------------------------------------------------------------------------------------------------
class _Recorder(RecorderBase):
    status_string = b"landmark capacity exhausted"
    last_error = b"append_model: injected"

    def __init__(self, N=7):
        self.calls, self.fail, self.N = [], 0, N

    def ekf_num_landmarks(self, h, pn):
        pn._obj.value = self.N
        return 0

    def ekf_append_model(self, h, arr, m, pfirst):
        self.calls.append(("append_model", m, [(o.model, o.reserved, list(o.z), list(o.R), o.signature) for o in list(arr)[:m]]))
        if self.fail:
            return self.fail
        pfirst._obj.value = self.N
        self.N += m
        return 0

    def ekf_model_invert(self, model, xr, z, t, Gx, Gz):
        self.calls.append(("invert", model, [xr[i] for i in range(3)], [z[0], z[1]]))
        t[1], Gx[5], Gz[2] = 7.0, 8.0, 9.0
        return self.fail


def test_engine_and_slam_layers_marshal_a_scan_once(monkeypatch):
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import engine as E
    from ekf_slam_amd import slam as S
    from ekf_slam_amd.trajectory import TrajectoryLog
    assert ctypes.sizeof(L.EkfModelInit) == 64 and L.EKF_APPEND_MODEL_MAX == 32
    rec = _Recorder()
    monkeypatch.setattr(L, "lib", lambda: rec)
    e = E.Engine(capacity=16)
    R = [[0.5, 0.1], [0.1, 0.25]]
    assert e.append_model([(1, [5.0, 30.0], R, 77.0), (4, [2.0, -1.0], RPOS, 78.0)]) == 7
    assert rec.calls[-1] == ("append_model", 2, [(1, 0, [5.0, 30.0], [0.5, 0.1, 0.1, 0.25], 77.0), (4, 0, [2.0, -1.0], [0.02, 0.005, 0.005, 0.03], 78.0)])
    assert e.append_model([(4, [2.0, -1.0], [[1.0, 2.0], [3.0, 4.0]], 5.0)]) == 9
    assert rec.calls[-1][2][0][3] == [1.0, 3.0, 2.0, 4.0]     # R travels column-major
    t, Gx, Gz = E.Engine.model_invert(4, [1.0, 2.0, 3.0], [4.0, 5.0])
    assert rec.calls[-1] == ("invert", 4, [1.0, 2.0, 3.0], [4.0, 5.0]) and t[1] == 7.0 and Gx.shape == (2, 3) and Gx[1, 2] == 8.0 and Gz[1, 0] == 9.0
    n = len(rec.calls)
    for bad in ([(1, [5.0], R, 1.0)], [(1, [5.0, 30.0], [1.0, 2.0], 1.0)], [(1, [5.0, 30.0], R)], [(1, [5.0, 30.0, 1.0], R, 1.0)]):
        with pytest.raises(ValueError):
            e.append_model(bad)
    assert len(rec.calls) == n
    for cls in (S.EKF_SLAM, S.EKF_SLAM_UC):
        rec = _Recorder()
        monkeypatch.setattr(L, "lib", lambda: rec)
        f = cls(capacity=16)
        f.log = TrajectoryLog()
        # 1-based numbers come back; a signature left out is the landmark's own number
        assert f.add_landmark_range_bearing([5.0, 30.0], R) == 8
        assert rec.calls[-1] == ("append_model", 1, [(1, 0, [5.0, 30.0], [0.5, 0.1, 0.1, 0.25], 8.0)])
        assert f.add_landmark_relative_xy([2.0, -1.0], RPOS, signature=500.0) == 9
        assert rec.calls[-1] == ("append_model", 1, [(4, 0, [2.0, -1.0], [0.02, 0.005, 0.005, 0.03], 500.0)])
        assert f.add_landmarks_model([(1, [5.0, 30.0], R), (4, [1.0, 1.0], RPOS, 44.0), (4, [2.0, 2.0], RPOS, None)]) == [10, 11, 12]
        assert [c[4] for c in rec.calls[-1][2]] == [10.0, 44.0, 12.0]
        assert [(k, kind, idx.tolist()) for k, kind, idx, _, _ in f.log.edits] == [(0, "append_model", [])] * 3
        assert [len(f.log.model_appends[q]) for q in range(3)] == [1, 1, 3] and f.log.model_appends[2][2][3] == 12.0
        n = len(rec.calls)
        for bad in ([], [(1, [1.0, 2.0], R)] * 33, [(2, [1.0, 2.0], R)], [(3, [1.0, 2.0], R)], [(5, [1.0, 2.0], R)], [(1, [1.0], R)],
                    [(1, [1.0, 2.0], [1.0, 2.0])], [(1, [1.0, 2.0])], [(1, [1.0, 2.0], R, 1.0, 2.0)]):
            with pytest.raises(ValueError):
                f.add_landmarks_model(bad)
        assert len(rec.calls) == n and len(f.log.edits) == 3
        # a refused call raises and is not logged
        rec.fail = L.EKF_ERR_CAPACITY
        with pytest.raises(L.EkfError) as info:
            f.add_landmark_range_bearing([5.0, 30.0], R)
        assert info.value.status == L.EKF_ERR_CAPACITY and "append_model" in str(info.value) and len(f.log.edits) == 3


def test_shard_group_sends_the_scan_to_every_shard(monkeypatch):
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd.sharding import ShardGroup
    recs = []

    def new_lib():
        return recs[0]
    recs.append(_Recorder())
    monkeypatch.setattr(L, "lib", new_lib)
    g = ShardGroup(3, capacity=16)
    scan = A.scan(np.random.default_rng(2), 2)
    assert g.append_model(iter(scan)) == 7                    # (an iterator is read once and handed to all three)
    got = [c for c in recs[0].calls if c[0] == "append_model"]
    assert len(got) == 3 and got[0][1:] == got[1][1:] == got[2][1:] and got[0][1] == 2


# ------------------------------------------------------------------------------------------------------------------
# the MEX gateway
# ------------------------------------------------------------------------------------------------------------------

_STUB = r'''
#include <stdio.h>
#include "ekfslam.h"
void stub_fail_next(ekf_handle *h);
static int fail_armed;
void arm_failure(void) { fail_armed = 1; }
int32_t ekf_append_model(ekf_handle *h, const ekf_model_init *o, int64_t m, int64_t *first) {
    printf("ABI ekf_append_model m=%lld first=%d", (long long)m, first != 0);
    for (int64_t b = 0; b < m; ++b)
        printf(" | model=%d reserved=%d z=%g,%g R=%g,%g,%g,%g s=%g", (int)o[b].model, (int)o[b].reserved, o[b].z[0], o[b].z[1], o[b].R[0], o[b].R[1], o[b].R[2],
               o[b].R[3], o[b].signature);
    printf("\n");
    if (fail_armed) { fail_armed = 0; stub_fail_next(h); return ekf_flush(h); }
    if (first) *first = 40;
    return EKF_OK;
}
'''

_DRIVER = driver(r'''
    /* one entry: range and bearing */
    const mxArray *z1 = mock_double(1, 2, (const double[]){ 7, 8 }), *R1 = mock_double(2, 2, (const double[]){ 4, 1, 1, 9 });
    const mxArray *one[6] = { mock_string("append_model"), h, D1(1), z1, R1, D1(41) };
    if (call("append_model", 1, 6, one)) return 1;
    /* a scan of three: z is 3 x 2 column-major, R 2 x 2 x 3 */
    const mxArray *model3 = mock_double(3, 1, (const double[]){ 1, 4, 4 }), *z3 = mock_double(3, 2, (const double[]){ 5, 2, 3, 30, -1, -2 });
    const double r3[12] = { 4, 1, 1, 9, 0.5, 0, 0, 0.25, 2, 0.1, 0.1, 3 };
    const mxArray *R3 = mock_double(4, 3, r3), *s3 = mock_double(3, 1, (const double[]){ 41, 42, 900 });
    const mxArray *three[6] = { mock_string("append_model"), h, model3, z3, R3, s3 };
    if (call("append_model three", 1, 6, three)) return 1;
    const mxArray *bad[6];
    for (int q = 0; q < 6; ++q) bad[q] = three[q];
    if (!call("append_model", 1, 5, three)) return 1;
    bad[2] = mock_double(0, 0, 0);
    if (!call("append_model none", 1, 6, bad)) return 1;
    double many[33] = { 0 };
    bad[2] = mock_double(33, 1, many);
    if (!call("append_model many", 1, 6, bad)) return 1;
    bad[2] = model3; bad[3] = z1;
    if (!call("append_model badz", 1, 6, bad)) return 1;
    bad[3] = z3; bad[4] = R1;
    if (!call("append_model badr", 1, 6, bad)) return 1;
    bad[4] = R3; bad[5] = D1(1);
    if (!call("append_model bads", 1, 6, bad)) return 1;
    bad[5] = s3; bad[1] = D1(1);
    if (!call("append_model noh", 1, 6, bad)) return 1;
    arm_failure();
    if (!call("append_model", 1, 6, one)) return 1;
''', PRELUDE_SHOWN)

_DRIVER_WITHOUT = driver_without(r'''
    const mxArray *ap[6] = { mock_string("append_model"), h, D1(1), mock_double(1, 2, (const double[]){ 7, 8 }), mock_double(2, 2, (const double[]){ 4, 1, 1, 9 }), D1(41) };
    if (!call("append_model", 1, 6, ap)) return 1;
''')


def test_mex_gateway_marshals_a_scan_once(tmp_path):
    t = transcript_of(tmp_path, _STUB, _DRIVER)
    # R column-major as MATLAB holds it; the ABI's 0-based first index comes back as 1-based numbers, one per entry
    i = t.index("ABI ekf_append_model m=1 first=1 | model=1 reserved=0 z=7,8 R=4,1,1,9 s=41")
    assert t[i + 1] == "MEX append_model nrhs=6 -> ok out0=1x1[41]"
    i = t.index("ABI ekf_append_model m=3 first=1 | model=1 reserved=0 z=5,30 R=4,1,1,9 s=41 | model=4 reserved=0 z=2,-1 R=0.5,0,0,0.25 s=42"
                " | model=4 reserved=0 z=3,-2 R=2,0.1,0.1,3 s=900")
    assert t[i + 1] == "MEX append_model three nrhs=6 -> ok out0=3x1[41,42,43]"
    assert any(ln.startswith("MEX append_model nrhs=5 -> ERROR ekfslam:usage") and "needs 6 arguments" in ln for ln in t)
    for which, what in (("none", "between 1 and 32 entries"), ("many", "between 1 and 32 entries"), ("badz", "z needs m x 2 elements"),
                        ("badr", "R needs 2 x 2 x m elements"), ("bads", "signature needs m elements")):
        assert any(ln.startswith("MEX append_model %s nrhs=6 -> ERROR ekfslam:usage" % which) and what in ln for ln in t), which
    assert any(ln.startswith("MEX append_model noh nrhs=6 -> ERROR ekfslam:handle") for ln in t)
    assert sum(ln.startswith("ABI ekf_append_model") for ln in t) == 3            # the two good calls and the injected failure
    assert "MEX append_model nrhs=6 -> ERROR ekfslam:status | call not valid in the current state: injected failure" in t
    assert t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_the_gateway_still_links_against_a_library_without_the_symbol(tmp_path):
    t = transcript_of(tmp_path, _DRIVER_WITHOUT)
    assert any(ln.startswith("MEX append_model ") and "ERROR ekfslam:usage" in ln and "this libekfslam has no ekf_append_model" in ln for ln in t)
    assert "MEX predict nrhs=3 -> ok" in t and t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_matlab_methods_forward_to_the_gateway_command():
    text = open(os.path.join(ROOT, "matlab", "EKF_SLAM.m")).read()
    m = re.search(r"function\s+idx\s*=\s*addLandmarksModel\(h,\s*model,\s*z,\s*R,\s*signature\)(.*?)\n        end\b", text, re.S)
    assert m and "h.gateway('append_model'," in m.group(1) and "numel(h.s) + (1:m)'" in m.group(1)
    for name, inner in (("addLandmarkRangeBearing", r"h\.addLandmarksModel\(1,"), ("addLandmarkRelativeXY", r"h\.addLandmarksModel\(4,")):
        m = re.search(r"function\s+idx\s*=\s*%s\((.*?)\n        end\b" % name, text, re.S)
        assert m and re.search(inner, m.group(1)), name
    src = open(os.path.join(ROOT, "matlab", "ekfslam_mex.c")).read()
    assert 'strcmp(cmd, "append_model")' in src and "#pragma weak ekf_append_model" in src
