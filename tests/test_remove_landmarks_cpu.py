"""CPU: the surfaces of landmark removal (ekf_remove_landmarks, include/ekfslam.h) that need no GPU -- the library exports the
entry point and the ctypes layer binds it; the MEX gateway (compiled against the MEX mock of tests/support/mex_mock/ with a
recording stand-in of its own for the new entry point) converts MATLAB's 1-based landmark numbers once; Engine.remove_landmarks
(0-based) and the 1-based method of ekf_slam_amd/slam.py reach the library with the right indices; and the NumPy expectation
the GPU tests compare against is right on a case written out by hand."""
import ctypes
import os
import re

import numpy as np
import pytest

from helpers import RecorderBase
from mex_harness import ROOT, driver, transcript_of
from removal_cases import expected_after, lowrank_data, lowrank_minus, removal_sets


def test_library_exports_and_binds_the_entry_point():
    import ekf_slam_amd
    from ekf_slam_amd import _lib
    ekf_slam_amd.build()
    L = ekf_slam_amd.lib()
    assert hasattr(L, "ekf_remove_landmarks")
    res, args = _lib.SIGNATURES["ekf_remove_landmarks"]
    assert res is ctypes.c_int32 and args == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_int64]
    assert L.ekf_remove_landmarks.argtypes == args
    assert L.ekf_abi_version() == 1                          # an added entry point is compatible
    assert _lib.EKF_KERNEL_COMPACT == 7 and _lib.EKF_KERNEL_COUNT == 8
    header = open(os.path.join(ROOT, "include", "ekfslam.h")).read()
    assert re.search(r"EKF_KERNEL_COMPACT\s*=\s*7\b", header) and re.search(r"EKF_KERNEL_COUNT\s*=\s*8\b", header)
    # a null handle is refused without touching a device
    assert L.ekf_remove_landmarks(None, None, 0) == _lib.EKF_ERR_INVALID_ARG


_STUB = r'''
#include <stdio.h>
#include "ekfslam.h"
void stub_fail_next(ekf_handle *h);
static int fail_armed;
void arm_failure(void) { fail_armed = 1; }
int32_t ekf_remove_landmarks(ekf_handle *h, const int64_t *idx, int64_t m) {
    printf("ABI ekf_remove_landmarks m=%lld idx0=", (long long)m);
    for (int64_t i = 0; i < m; ++i) printf("%s%lld", i ? "," : "", (long long)idx[i]);
    printf("\n");
    if (fail_armed) { fail_armed = 0; stub_fail_next(h); return ekf_flush(h); }
    return EKF_OK;
}
'''

_DRIVER = driver(r'''
    const mxArray *row[3] = { mock_string("remove_landmarks"), h, mock_double(1, 3, (const double[]){ 3, 1, 7 }) };
    const mxArray *col[3] = { mock_string("remove_landmarks"), h, mock_double(2, 1, (const double[]){ 5, 4 }) };
    const mxArray *none[3] = { mock_string("remove_landmarks"), h, mock_double(0, 0, (const double[]){ 0 }) };
    const mxArray *few[2] = { mock_string("remove_landmarks"), h };
    const mxArray *nohandle[3] = { mock_string("remove_landmarks"), mock_double(1, 1, (const double[]){ 1 }), mock_double(1, 1, (const double[]){ 1 }) };
    if (call("remove_landmarks", 1, 3, row) || call("remove_landmarks", 1, 3, col) || call("remove_landmarks", 1, 3, none)) return 1;
    if (!call("remove_landmarks", 1, 2, few)) return 1;
    if (!call("remove_landmarks", 1, 3, nohandle)) return 1;
    arm_failure();
    if (!call("remove_landmarks", 1, 3, row)) return 1;
''')


@pytest.fixture(scope="module")
def transcript(tmp_path_factory):
    return transcript_of(tmp_path_factory.mktemp("mexremove"), _STUB, _DRIVER)


def test_mex_gateway_hands_one_based_numbers_on_as_zero_based(transcript):
    t = transcript
    i = t.index("ABI ekf_remove_landmarks m=3 idx0=2,0,6")          # [3 1 7] -> {2, 0, 6}, m = 3, order kept
    assert t[i + 1] == "MEX remove_landmarks nrhs=3 -> ok"
    assert "ABI ekf_remove_landmarks m=2 idx0=4,3" in t              # a column vector: the shape does not matter
    assert "ABI ekf_remove_landmarks m=0 idx0=" in t                 # [] removes nothing and is no error
    assert any(ln.startswith("MEX remove_landmarks nrhs=2 -> ERROR ekfslam:usage") and "needs 3 arguments" in ln for ln in t)
    assert any(ln.startswith("MEX remove_landmarks nrhs=3 -> ERROR ekfslam:handle") for ln in t)
    # a failing status becomes a MATLAB error that carries ekf_last_error
    assert "MEX remove_landmarks nrhs=3 -> ERROR ekfslam:status | call not valid in the current state: injected failure" in t
    assert t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_matlab_method_forwards_to_the_gateway_command():
    """matlab/EKF_SLAM.m::removeLandmarks(idx) (inherited by EKF_SLAM_UC) passes the column of landmark numbers to the
    gateway's 'remove_landmarks' -- the (command, handle, idx) shape the driver above ran."""
    text = open(os.path.join(ROOT, "matlab", "EKF_SLAM.m")).read()
    m = re.search(r"function\s+removeLandmarks\(h,\s*idx\)(.*?)\n\s*end\b", text, re.S)
    assert m and re.search(r"h\.gateway\('remove_landmarks',\s*double\(idx\(:\)\)\)", m.group(1))
    g = re.search(r"function\s+varargout\s*=\s*gateway\(h,\s*cmd,\s*varargin\)[^\n]*\n\s*\[varargout\{1:nargout\}\]\s*=\s*"
                  r"ekfslam_mex\(cmd,\s*h\.hnd,\s*varargin\{:\}\);", text)
    assert g
    assert re.search(r"classdef\s+EKF_SLAM_UC\s*<\s*EKF_SLAM\b", open(os.path.join(ROOT, "matlab", "EKF_SLAM_UC.m")).read())
    assert '"remove_landmarks"' in open(os.path.join(ROOT, "matlab", "ekfslam_mex.c")).read()


class _Recorder(RecorderBase):
    """Stand-in for the loaded library: records ekf_remove_landmarks calls (no GPU here)."""

    status_string = b"landmark index out of range"
    last_error = b"remove_landmarks: landmark index outside the state"

    def __init__(self, status=0):
        self.calls, self.status = [], status

    def ekf_remove_landmarks(self, h, arr, m):
        self.calls.append(([int(arr[i]) for i in range(m)], int(m)))
        return self.status


def test_engine_and_slam_layers_reach_the_library_with_the_right_indices(monkeypatch):
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import engine as E
    from ekf_slam_amd import slam as S
    rec = _Recorder()
    monkeypatch.setattr(L, "lib", lambda: rec)
    e = E.Engine(capacity=16)
    e.remove_landmarks([5, 0, 9])                          # 0-based, order kept
    e.remove_landmarks(np.array([2], dtype=np.int32))      # any iterable of ints
    e.remove_landmarks(iter(()))                           # nothing: still one call, m = 0
    assert rec.calls == [([5, 0, 9], 3), ([2], 1), ([], 0)]
    for cls in (S.EKF_SLAM, S.EKF_SLAM_UC):
        rec.calls.clear()
        f = cls(capacity=16)
        f.remove_landmarks([3, 1, 7])                      # 1-based like every index of that layer
        f.remove_landmarks(4)
        f.remove_landmarks(np.array([2.0, 6.0]))           # MATLAB-style doubles that hold whole numbers
        assert rec.calls == [([2, 0, 6], 3), ([3], 1), ([1, 5], 2)]
        with pytest.raises(ValueError):
            f.remove_landmarks([1.5])
    # the layer's error behaviour: a refused call raises EkfError with the library's status and message
    bad = _Recorder(status=L.EKF_ERR_INDEX)
    monkeypatch.setattr(L, "lib", lambda: bad)
    f = S.EKF_SLAM_UC(capacity=16)
    with pytest.raises(L.EkfError) as ex:
        f.remove_landmarks([0])                            # landmark 0 does not exist in a 1-based numbering: -1 at the ABI
    assert ex.value.status == L.EKF_ERR_INDEX and bad.calls == [([-1], 1)] and "outside the state" in str(ex.value)


def test_expected_after_on_a_hand_written_case():
    # three landmarks; P(i, j) = 10 i + j with 1-based i, j as in the reference's notation
    x = np.array([1.0, 2.0, 30.0, 11.0, 12.0, 21.0, 22.0, 31.0, 32.0])
    s = np.array([7.0, 8.0, 9.0])
    P = np.array([[10.0 * (i + 1) + (j + 1) for j in range(9)] for i in range(9)])
    ex, es, eP = expected_after(x, s, P, [1])              # the middle landmark: entries 6, 7 (1-based) of x, rows / columns 6, 7
    np.testing.assert_array_equal(ex, [1.0, 2.0, 30.0, 11.0, 12.0, 31.0, 32.0])
    np.testing.assert_array_equal(es, [7.0, 9.0])
    keep = [1, 2, 3, 4, 5, 8, 9]
    np.testing.assert_array_equal(eP, [[10.0 * i + j for j in keep] for i in keep])
    ex, es, eP = expected_after(x, s, P, [2, 0])           # unsorted; landmark 2 (1-based) survives alone
    np.testing.assert_array_equal(ex, [1.0, 2.0, 30.0, 21.0, 22.0])
    np.testing.assert_array_equal(es, [8.0])
    keep = [1, 2, 3, 6, 7]
    np.testing.assert_array_equal(eP, [[10.0 * i + j for j in keep] for i in keep])
    ex, es, eP = expected_after(x, s, P, [0, 1, 2])
    assert ex.tolist() == [1.0, 2.0, 30.0] and es.size == 0 and eP.shape == (3, 3) and eP[2, 2] == 33.0
    ex, es, eP = expected_after(x, s, P, [])
    np.testing.assert_array_equal(eP, P)
    with pytest.raises(AssertionError):
        expected_after(x, s, P, [1, 1])
    with pytest.raises(AssertionError):
        expected_after(x, s, P, [3])


def test_removal_sets_and_lowrank_twin_are_what_the_gpu_tests_assume():
    for T in (16, 64, 128, 256):
        sets = removal_sets(300, T, 11)
        assert sets == removal_sets(300, T, 11)                                   # a pure function of (N, T, seed)
        assert set(sets) == {"first", "last", "middle", "adjacent_over_tile_edge", "whole_tile_row", "every_second",
                             "random_tenth", "all"}
        a, b = sorted(sets["adjacent_over_tile_edge"])
        assert b == a + 1 and (2 * b) % T == 0                                    # the pair straddles a tile edge
        row = sorted(sets["whole_tile_row"])
        assert row == list(range(row[0], row[0] + len(row))) and (2 * row[0]) % T == 0 and len(row) == min(T // 2, 300 - row[0])
        assert sets["every_second"] != sorted(sets["every_second"])               # handed over unsorted
        assert len(sets["random_tenth"]) == 30 and sorted(sets["all"]) == list(range(300))
    # a low-rank state minus rows == numpy.delete of the dense state (exactly: every entry comes from its own two rows of U)
    x, s, d, U = lowrank_data(12, 3)
    P = np.diag(d) + U @ U.T
    idx = [4, 0, 11]
    x2, s2, d2, U2 = lowrank_minus(x, s, d, U, idx)
    ex, es, eP = expected_after(x, s, P, idx)
    np.testing.assert_array_equal(x2, ex)
    np.testing.assert_array_equal(s2, es)
    np.testing.assert_allclose(np.diag(d2) + U2 @ U2.T, eP, rtol=0, atol=1e-18)
