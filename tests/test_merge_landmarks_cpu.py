"""CPU: the surfaces of landmark fusion (ekf_constrain_landmarks, ekf_merge_landmarks, ekf_landmark_distance; include/ekfslam.h,
DESIGN.md section 3f) that need no GPU -- the library exports the three entry points and the ctypes layer binds them; the NumPy
restatement the GPU tests compare against gives the hand-checkable answer and agrees with an independent information-form
restatement; Engine (0-based) and the 1-based methods of ekf_slam_amd/slam.py reach the library with the right indices; the MEX
gateway (compiled against the MEX mock with a recording stand-in of its own for the new entry points) converts MATLAB's 1-based
numbers once, and still links against a stand-in that lacks the new symbols."""
import ctypes
import os
import re

import numpy as np
import pytest

from helpers import RecorderBase
from merge_cases import Factored, constrain_dense, constrain_information, merge_dense
from mex_harness import ROOT, driver, driver_without, prelude, transcript_of
from removal_cases import expected_after, lowrank_data


def test_library_exports_and_binds_the_entry_points():
    import ekf_slam_amd
    from ekf_slam_amd import _lib
    ekf_slam_amd.build()
    L = ekf_slam_amd.lib()
    vp, i64, dp = ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_double)
    want = {"ekf_constrain_landmarks": [vp, i64, i64, dp, dp], "ekf_merge_landmarks": [vp, i64, i64, dp],
            "ekf_landmark_distance": [vp, i64, i64, dp, dp, dp, dp]}
    for name, args in want.items():
        assert hasattr(L, name)
        res, sig = _lib.SIGNATURES[name]
        assert res is ctypes.c_int32 and sig == args and getattr(L, name).argtypes == args
    assert L.ekf_abi_version() == 1                          # added entry points are compatible
    assert _lib.EKF_KERNEL_COUNT == 8                        # no new timing id
    # a null handle is refused without touching a device
    assert L.ekf_constrain_landmarks(None, 0, 1, None, None) == _lib.EKF_ERR_INVALID_ARG
    assert L.ekf_merge_landmarks(None, 0, 1, None) == _lib.EKF_ERR_INVALID_ARG
    d2 = ctypes.c_double()
    assert L.ekf_landmark_distance(None, 0, 1, None, None, ctypes.byref(d2), None) == _lib.EKF_ERR_INVALID_ARG
    header = open(os.path.join(ROOT, "include", "ekfslam.h")).read()
    for name in want:
        assert re.search(r"int32_t\s+%s\(ekf_handle \*h" % name, header)


def _known_answer_state():
    """Two landmarks uncorrelated with each other and with the robot: P_aa = diag(3, 1), P_bb = diag(1, 1), l_a = (0, 0),
    l_b = (4, 2)."""
    x = np.array([0.5, -0.25, 30.0, 0.0, 0.0, 4.0, 2.0])
    P = np.diag([0.1, 0.1, 0.01, 3.0, 1.0, 1.0, 1.0])
    return x, np.array([1.0, 2.0]), P


@pytest.mark.parametrize("keep,drop", [(0, 1), (1, 0)])
def test_known_answer(keep, drop):
    x, s, P = _known_answer_state()
    x2, P2, d2, S = constrain_dense(x, P, keep, drop, None, None)            # delta = 0, R = 0
    np.testing.assert_allclose(S, np.diag([4.0, 2.0]), rtol=0, atol=1e-15)
    assert abs(d2 - 6.0) < 1e-14                                             # 16 / 4 + 4 / 2
    np.testing.assert_allclose(x2[3:], [3.0, 1.0, 3.0, 1.0], rtol=0, atol=1e-14)     # both landmarks move to (3, 1)
    np.testing.assert_array_equal(x2[:3], x[:3])                             # the robot is uncorrelated with both
    mx, ms, mP = merge_dense(x, s, P, keep, drop, None)
    assert ms.tolist() == [s[keep]]                                          # keep retains its signature
    np.testing.assert_allclose(mx, [0.5, -0.25, 30.0, 3.0, 1.0], rtol=0, atol=1e-14)
    np.testing.assert_allclose(mP[3:, 3:], np.diag([0.75, 0.5]), rtol=0, atol=1e-15)  # the product of the two Gaussians
    np.testing.assert_allclose(mP[:3, :3], P[:3, :3], rtol=0, atol=0)
    # the Mahalanobis distance is symmetric in the pair, and a delta equal to the current offset makes it zero
    assert abs(constrain_dense(x, P, drop, keep)[2] - d2) < 1e-14
    assert constrain_dense(x, P, 1, 0, [4.0, 2.0], None)[2] == 0.0


@pytest.mark.parametrize("i,j", [(7, 150), (150, 7), (63, 64), (299, 0)])
def test_kalman_form_against_information_form(i, j):
    x, s, d, U = lowrank_data(300, 5)
    P = np.diag(d) + U @ U.T
    R = np.diag([0.01, 0.02])
    delta = np.array([0.3, -0.1])
    xk, Pk, d2, S = constrain_dense(x, P, i, j, delta, R)
    xi, Pi = constrain_information(x, P, i, j, delta, R)
    ex = np.abs(xk - xi).max() / np.abs(xi).max()
    eP = np.abs(Pk - Pi).max() / np.abs(Pi).max()
    print("pair (%d, %d): rel diff x %.2e P %.2e, cond S %.2f, d2 %.1f" % (i, j, ex, eP, np.linalg.cond(S), d2))
    assert ex < 1e-10 and eP < 1e-10
    assert np.linalg.eigvalsh(0.5 * (Pk + Pk.T)).min() > 0.0                 # P' positive definite
    # the factored form the tests at size use is the same update
    f = Factored(x, d, U)
    fd2, fS = f.constrain(i, j, delta, R)
    assert abs(fd2 - d2) <= 1e-12 * d2
    np.testing.assert_allclose(fS, S, rtol=1e-13, atol=0)
    np.testing.assert_allclose(f.x, xk, rtol=0, atol=1e-12)
    np.testing.assert_allclose(f.rows(0, 3 + 2 * 300), Pk, rtol=0, atol=1e-15)
    blocks = f.diag_blocks()
    np.testing.assert_allclose(blocks[0], Pk[:2, :2], rtol=0, atol=1e-16)
    np.testing.assert_allclose(blocks[1 + j], Pk[3 + 2 * j:5 + 2 * j, 3 + 2 * j:5 + 2 * j], rtol=0, atol=1e-15)
    tr, sq = f.trace_and_squares(block=128)
    low = np.tril(Pk)
    assert abs(tr - np.trace(Pk)) <= 1e-12 * np.trace(Pk) and abs(sq - (low * low).sum()) <= 1e-12 * sq
    f.remove([j])
    mx, ms, mP = merge_dense(x, s, P, i, j, R)                               # (delta = 0 there: compare the removal alone)
    ex2, _, eP2 = expected_after(xk, s, Pk, [j])
    np.testing.assert_allclose(f.x, ex2, rtol=0, atol=1e-12)
    np.testing.assert_allclose(f.rows(0, f.x.size), eP2, rtol=0, atol=1e-15)
    assert mx.size == ex2.size and ms.size == 299 and mP.shape == eP2.shape


class _Recorder(RecorderBase):
    """Stand-in for the loaded library: records the calls of the three entry points and of ekf_remove_landmarks (no GPU here)."""

    status_string = b"landmark index out of range"
    last_error = b"merge_landmarks: landmark index outside the state"

    def __init__(self, status=0):
        self.calls, self.status = [], status

    @staticmethod
    def _v(p, n):
        return None if p is None else [float(p[k]) for k in range(n)]

    def ekf_constrain_landmarks(self, h, i, j, delta, R):
        self.calls.append(("constrain", int(i), int(j), self._v(delta, 2), self._v(R, 4)))
        return self.status

    def ekf_merge_landmarks(self, h, keep, drop, R):
        self.calls.append(("merge", int(keep), int(drop), self._v(R, 4)))
        return self.status

    def ekf_landmark_distance(self, h, i, j, delta, R, d2, S):
        self.calls.append(("distance", int(i), int(j), self._v(delta, 2), self._v(R, 4)))
        ctypes.cast(d2, ctypes.POINTER(ctypes.c_double)).contents.value = 6.5
        for k, v in enumerate((1.0, 2.0, 3.0, 4.0)):                      # column-major: S = [[1, 3], [2, 4]]
            S[k] = v
        return self.status

    def ekf_remove_landmarks(self, h, arr, m):
        self.calls.append(("remove", [int(arr[k]) for k in range(m)]))
        return self.status


def test_engine_and_slam_layers_reach_the_library_with_the_right_indices(monkeypatch):
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import engine as E
    from ekf_slam_amd import slam as S
    from ekf_slam_amd.trajectory import TrajectoryLog
    rec = _Recorder()
    monkeypatch.setattr(L, "lib", lambda: rec)
    e = E.Engine(capacity=16)
    R = np.array([[0.5, 0.1], [0.1, 0.25]])
    e.constrain_landmarks(5, 0)                              # 0-based; delta and R default to NULL
    e.constrain_landmarks(2, 9, [0.5, -1.0], R)
    e.merge_landmarks(3, 7)
    e.merge_landmarks(7, 3, np.diag([2.0, 3.0]))
    d2, Sm = e.landmark_distance(1, 4, (0.25, 0.75), R)
    assert rec.calls == [("constrain", 5, 0, None, None), ("constrain", 2, 9, [0.5, -1.0], [0.5, 0.1, 0.1, 0.25]),
                         ("merge", 3, 7, None), ("merge", 7, 3, [2.0, 0.0, 0.0, 3.0]),
                         ("distance", 1, 4, [0.25, 0.75], [0.5, 0.1, 0.1, 0.25])]
    assert d2 == 6.5 and Sm.tolist() == [[1.0, 3.0], [2.0, 4.0]]
    for cls in (S.EKF_SLAM, S.EKF_SLAM_UC):
        rec.calls.clear()
        f = cls(capacity=16)
        f.log = TrajectoryLog()
        f.constrain_landmarks(3, 1)                          # 1-based like every index of that layer
        f.constrain_landmarks(2.0, 6.0, [1.0, 2.0], R)       # MATLAB-style doubles that hold whole numbers
        f.merge_landmarks(4, 8, R)
        assert f.landmark_distance(5, 2)[0] == 6.5
        f.remove_landmarks([3, 1])
        assert rec.calls == [("constrain", 2, 0, None, None), ("constrain", 1, 5, [1.0, 2.0], [0.5, 0.1, 0.1, 0.25]),
                             ("merge", 3, 7, [0.5, 0.1, 0.1, 0.25]), ("distance", 4, 1, None, None), ("remove", [2, 0])]
        for bad in (lambda: f.constrain_landmarks(1.5, 2), lambda: f.merge_landmarks(1, 2.5), lambda: f.landmark_distance(0.5, 1)):
            with pytest.raises(ValueError):
                bad()
        # the edits went into the log with the 1-based numbers this layer consumed; landmark_distance is no edit
        assert [(k, kind, idx.tolist()) for k, kind, idx, _, _ in f.log.edits] == \
            [(0, "constrain", [3, 1]), (0, "constrain", [2, 6]), (0, "merge", [4, 8]), (0, "remove", [3, 1])]
        assert f.log.edits[1][3].tolist() == [1.0, 2.0] and f.log.edits[2][4].tolist() == R.tolist()
    # a refused call raises EkfError with the library's status and message, and is not logged
    bad = _Recorder(status=L.EKF_ERR_INDEX)
    monkeypatch.setattr(L, "lib", lambda: bad)
    f = S.EKF_SLAM_UC(capacity=16)
    f.log = TrajectoryLog()
    with pytest.raises(L.EkfError) as ex:
        f.merge_landmarks(1, 0)                              # landmark 0 does not exist in a 1-based numbering: -1 at the ABI
    assert ex.value.status == L.EKF_ERR_INDEX and bad.calls == [("merge", 0, -1, None)] and "outside the state" in str(ex.value)
    assert f.log.edits == []


_STUB = r'''
#include <stdio.h>
#include "ekfslam.h"
void stub_fail_next(ekf_handle *h);
static int fail_armed;
void arm_failure(void) { fail_armed = 1; }
static int32_t status(ekf_handle *h) { if (fail_armed) { fail_armed = 0; stub_fail_next(h); return ekf_flush(h); } return EKF_OK; }
int32_t ekf_constrain_landmarks(ekf_handle *h, int64_t i, int64_t j, const double delta[2], const double R[4]) {
    printf("ABI ekf_constrain_landmarks i0=%lld j0=%lld delta=%g,%g R=%g,%g,%g,%g\n", (long long)i, (long long)j, delta[0], delta[1], R[0], R[1], R[2], R[3]);
    return status(h);
}
int32_t ekf_merge_landmarks(ekf_handle *h, int64_t keep, int64_t drop, const double R[4]) {
    printf("ABI ekf_merge_landmarks keep0=%lld drop0=%lld R=%g,%g,%g,%g\n", (long long)keep, (long long)drop, R[0], R[1], R[2], R[3]);
    return status(h);
}
int32_t ekf_landmark_distance(ekf_handle *h, int64_t i, int64_t j, const double delta[2], const double R[4], double *d2, double S[4]) {
    printf("ABI ekf_landmark_distance i0=%lld j0=%lld delta=%g,%g R=%g,%g,%g,%g S=%s\n", (long long)i, (long long)j, delta[0], delta[1], R[0], R[1], R[2], R[3], S ? "yes" : "no");
    *d2 = 6.5;
    if (S) { S[0] = 1; S[1] = 2; S[2] = 3; S[3] = 4; }
    return status(h);
}
'''

_SHOWN = prelude(r'''    if (out[0]) printf(" d2=%g", mxGetScalar(out[0]));
    if (out[1]) printf(" S=%zux%zu[%g,%g,%g,%g]", mxGetM(out[1]), mxGetN(out[1]), mxGetPr(out[1])[0], mxGetPr(out[1])[1], mxGetPr(out[1])[2], mxGetPr(out[1])[3]);
''')

_DRIVER = driver(r'''
    const mxArray *delta = mock_double(2, 1, (const double[]){ 0.5, -1 }), *R = mock_double(2, 2, (const double[]){ 4, 1, 1, 9 });
    const mxArray *con[6] = { mock_string("constrain_landmarks"), h, mock_double(1, 1, (const double[]){ 3 }), mock_double(1, 1, (const double[]){ 7 }), delta, R };
    const mxArray *mer[5] = { mock_string("merge_landmarks"), h, mock_double(1, 1, (const double[]){ 8 }), mock_double(1, 1, (const double[]){ 2 }), R };
    const mxArray *dis[6] = { mock_string("landmark_distance"), h, mock_double(1, 1, (const double[]){ 1 }), mock_double(1, 1, (const double[]){ 5 }), delta, R };
    const mxArray *badd[6] = { mock_string("constrain_landmarks"), h, mock_double(1, 1, (const double[]){ 3 }), mock_double(1, 1, (const double[]){ 7 }), mock_double(1, 3, (const double[]){ 1, 2, 3 }), R };
    const mxArray *badr[5] = { mock_string("merge_landmarks"), h, mock_double(1, 1, (const double[]){ 8 }), mock_double(1, 1, (const double[]){ 2 }), delta };
    const mxArray *nohandle[5] = { mock_string("merge_landmarks"), mock_double(1, 1, (const double[]){ 1 }), mock_double(1, 1, (const double[]){ 8 }), mock_double(1, 1, (const double[]){ 2 }), R };
    if (call("constrain_landmarks", 0, 6, con) || call("merge_landmarks", 0, 5, mer)) return 1;
    if (call("landmark_distance", 2, 6, dis) || call("landmark_distance", 1, 6, dis)) return 1;
    if (!call("constrain_landmarks", 0, 5, con) || !call("merge_landmarks", 0, 4, mer) || !call("landmark_distance", 1, 5, dis)) return 1;
    if (!call("constrain_landmarks", 0, 6, badd) || !call("merge_landmarks", 0, 5, badr) || !call("merge_landmarks", 0, 5, nohandle)) return 1;
    arm_failure();
    if (!call("constrain_landmarks", 0, 6, con)) return 1;
    arm_failure();
    if (!call("merge_landmarks", 0, 5, mer)) return 1;
    arm_failure();
    if (!call("landmark_distance", 2, 6, dis)) return 1;
''', _SHOWN)

_DRIVER_WITHOUT = driver_without(r'''
    const mxArray *delta = mock_double(2, 1, (const double[]){ 0, 0 }), *R = mock_double(2, 2, (const double[]){ 0, 0, 0, 0 });
    const mxArray *one = mock_double(1, 1, (const double[]){ 1 }), *two = mock_double(1, 1, (const double[]){ 2 });
    const mxArray *con[6] = { mock_string("constrain_landmarks"), h, one, two, delta, R };
    const mxArray *mer[5] = { mock_string("merge_landmarks"), h, one, two, R };
    const mxArray *dis[6] = { mock_string("landmark_distance"), h, one, two, delta, R };
    if (!call("constrain_landmarks", 1, 6, con) || !call("merge_landmarks", 1, 5, mer) || !call("landmark_distance", 1, 6, dis)) return 1;
''')


@pytest.fixture(scope="module")
def transcript(tmp_path_factory):
    return transcript_of(tmp_path_factory.mktemp("mexmerge"), _STUB, _DRIVER)


def test_mex_gateway_hands_one_based_numbers_on_as_zero_based(transcript):
    t = transcript
    i = t.index("ABI ekf_constrain_landmarks i0=2 j0=6 delta=0.5,-1 R=4,1,1,9")        # (3, 7) -> (2, 6), converted once
    assert t[i + 1] == "MEX constrain_landmarks nrhs=6 -> ok"
    i = t.index("ABI ekf_merge_landmarks keep0=7 drop0=1 R=4,1,1,9")
    assert t[i + 1] == "MEX merge_landmarks nrhs=5 -> ok"
    i = t.index("ABI ekf_landmark_distance i0=0 j0=4 delta=0.5,-1 R=4,1,1,9 S=yes")
    assert t[i + 1] == "MEX landmark_distance nrhs=6 -> ok d2=6.5 S=2x2[1,2,3,4]"      # [d2, S] = ...
    assert "MEX landmark_distance nrhs=6 -> ok d2=6.5" in t                            # d2 = ... alone: S is not leaked
    assert any(ln.startswith("MEX constrain_landmarks nrhs=5 -> ERROR ekfslam:usage") and "needs 6 arguments" in ln for ln in t)
    assert any(ln.startswith("MEX merge_landmarks nrhs=4 -> ERROR ekfslam:usage") and "needs 5 arguments" in ln for ln in t)
    assert any(ln.startswith("MEX landmark_distance nrhs=5 -> ERROR ekfslam:usage") and "needs 6 arguments" in ln for ln in t)
    assert any(ln.startswith("MEX constrain_landmarks nrhs=6 -> ERROR ekfslam:usage") and "delta needs 2 elements" in ln for ln in t)
    assert any(ln.startswith("MEX merge_landmarks nrhs=5 -> ERROR ekfslam:usage") and "R needs 2 x 2 elements" in ln for ln in t)
    assert any(ln.startswith("MEX merge_landmarks nrhs=5 -> ERROR ekfslam:handle") for ln in t)
    # a failing status becomes a MATLAB error that carries ekf_last_error
    for cmd, n in (("constrain_landmarks", 6), ("merge_landmarks", 5), ("landmark_distance", 6)):
        assert "MEX %s nrhs=%d -> ERROR ekfslam:status | call not valid in the current state: injected failure" % (cmd, n) in t
    assert t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_the_gateway_still_links_against_a_library_without_the_new_symbols(tmp_path):
    t = transcript_of(tmp_path, _DRIVER_WITHOUT)
    for cmd, sym in (("constrain_landmarks", "ekf_constrain_landmarks"), ("merge_landmarks", "ekf_merge_landmarks"),
                     ("landmark_distance", "ekf_landmark_distance")):
        assert any(ln.startswith("MEX %s " % cmd) and "ERROR ekfslam:usage" in ln and "this libekfslam has no %s" % sym in ln for ln in t)
    assert "MEX predict nrhs=3 -> ok" in t and t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_matlab_methods_forward_to_the_gateway_commands():
    """matlab/EKF_SLAM.m::constrainLandmarks / mergeLandmarks / landmarkDistance (inherited by EKF_SLAM_UC) pass the (command,
    handle, numbers, delta, R) shapes the driver above ran."""
    text = open(os.path.join(ROOT, "matlab", "EKF_SLAM.m")).read()

    def body(sig):
        m = re.search(r"function\s+" + sig + r"(.*?)\n        end\b", text, re.S)
        assert m, sig
        return m.group(1)

    assert re.search(r"h\.gateway\('constrain_landmarks',\s*double\(i\),\s*double\(j\),\s*double\(delta\(:\)\),\s*double\(R\)\)",
                     body(r"constrainLandmarks\(h,\s*i,\s*j,\s*delta,\s*R\)"))
    assert re.search(r"h\.gateway\('merge_landmarks',\s*double\(keep\),\s*double\(drop\),\s*double\(R\)\)",
                     body(r"mergeLandmarks\(h,\s*keep,\s*drop,\s*R\)"))
    assert re.search(r"\[d2,\s*S\]\s*=\s*h\.gateway\('landmark_distance',\s*double\(i\),\s*double\(j\),\s*double\(delta\(:\)\),\s*double\(R\)\)",
                     body(r"\[d2,\s*S\]\s*=\s*landmarkDistance\(h,\s*i,\s*j,\s*delta,\s*R\)"))
    assert re.search(r"classdef\s+EKF_SLAM_UC\s*<\s*EKF_SLAM\b", open(os.path.join(ROOT, "matlab", "EKF_SLAM_UC.m")).read())
    src = open(os.path.join(ROOT, "matlab", "ekfslam_mex.c")).read()
    for cmd in ("constrain_landmarks", "merge_landmarks", "landmark_distance"):
        assert 'strcmp(cmd, "%s")' % cmd in src and "#pragma weak ekf_%s" % cmd in src
