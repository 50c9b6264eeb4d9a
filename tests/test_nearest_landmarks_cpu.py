"""CPU: the surfaces of the candidate search (ekf_nearest_landmarks; include/ekfslam.h) that need no GPU -- the
library exports the entry point and the ctypes layer binds it; the vectorised NumPy restatement the GPU tests compare against agrees
with a plain double loop over the restatement of ekf_landmark_distance and gives the hand-checkable answers; Engine (0-based) and
the 1-based methods of ekf_slam_amd/slam.py convert indices once and fuse in the stated order; the MEX gateway (compiled against
the MEX mock with a recording stand-in for the new entry point) hands out 1-based partners with 0 for none, and still links against
a stand-in that lacks the symbol."""
import ctypes
import os
import re

import numpy as np
import pytest

from helpers import RPOS, RecorderBase
from merge_cases import constrain_dense
from mex_harness import PRELUDE_SHOWN, ROOT, driver, driver_without, transcript_of
from nearest_cases import fuse_dense, nearest_dense, nearest_lowrank, pair_matrix, plant_duplicates
from removal_cases import lowrank_data


def test_library_exports_and_binds_the_entry_point():
    import ekf_slam_amd
    from ekf_slam_amd import _lib
    ekf_slam_amd.build()
    L = ekf_slam_amd.lib()
    vp, dp, ip = ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
    assert hasattr(L, "ekf_nearest_landmarks")
    res, sig = _lib.SIGNATURES["ekf_nearest_landmarks"]
    assert res is ctypes.c_int32 and sig == [vp, dp, dp, ip] and L.ekf_nearest_landmarks.argtypes == sig
    assert L.ekf_abi_version() == 1                          # an added entry point is compatible
    assert _lib.EKF_KERNEL_COUNT == 8                        # no new timing id: the launch counts under EKF_KERNEL_ASSOCIATE
    # a null handle is refused without touching a device
    d2, partner = (ctypes.c_double * 4)(), (ctypes.c_int64 * 4)()
    assert L.ekf_nearest_landmarks(None, None, d2, partner) == _lib.EKF_ERR_INVALID_ARG
    header = open(os.path.join(ROOT, "include", "ekfslam.h")).read()
    assert re.search(r"int32_t\s+ekf_nearest_landmarks\(ekf_handle \*h,\s*const double R\[4\][^;]*double \*d2[^;]*int64_t \*partner[^;]*\);", header)


def test_the_arithmetic_lives_in_one_place():
    """constrain_impl (ekf_landmark_distance) and k_nearest call the same function for d2."""
    csrc = os.path.join(ROOT, "ekf_slam_amd", "csrc")
    math_h = open(os.path.join(csrc, "device_math.h")).read()
    assert re.search(r"EKF_MHD\s+bool\s+constrain_d2\(", math_h)
    abi = open(os.path.join(csrc, "host", "edits.h")).read()      # the host layer's map-edit family holds constrain_impl
    impl = abi[abi.index("int32_t constrain_impl("):abi.index("int32_t ekf_constrain_landmarks(")]
    assert "ekfm::constrain_d2(" in impl and "ekfm::inv2(" not in impl
    nearest = open(os.path.join(csrc, "nearest.h")).read()
    assert "ekfm::constrain_S(" in nearest and "ekfm::constrain_d2(" in nearest
    assert "-ffp-contract=off" in open(os.path.join(csrc, "Makefile")).read()


@pytest.mark.parametrize("R", [None, RPOS], ids=["R0", "Rpos"])
def test_vectorised_restatement_against_a_plain_double_loop(R):
    N = 40
    x, s, d, U = lowrank_data(N, 7)
    x = plant_duplicates(x, [(0, 9), (3, 39), (15, 16)])
    P = np.diag(d) + U @ U.T
    D = pair_matrix(x, P, R)
    best, partner, ratio = nearest_dense(x, P, R)
    assert partner[0] == -1 and np.isinf(best[0]) and np.isinf(D[np.triu_indices(N)]).all()
    for i in range(1, N):
        row = np.array([constrain_dense(x, P, i, j, None, R)[2] for j in range(i)])
        np.testing.assert_allclose(D[i, :i], row, rtol=1e-12, atol=0)
        assert partner[i] == int(np.argmin(row)) and abs(best[i] / row.min() - 1.0) < 1e-12
        if i >= 2:
            assert abs(ratio[i] / (np.sort(row)[1] / row.min()) - 1.0) < 1e-9
    assert partner[9] == 0 and partner[39] == 3 and partner[16] == 15
    # the block-wise low-rank form is the same function
    b2, p2, r2 = nearest_lowrank(x, d, U, np.arange(N), R)
    np.testing.assert_array_equal(p2, partner)
    np.testing.assert_allclose(b2[1:], best[1:], rtol=1e-12, atol=0)
    sub = np.array([0, 5, 16, 39])
    b3, p3, _ = nearest_lowrank(x, d, U, sub, R)
    np.testing.assert_array_equal(p3, partner[sub])


def _known_answer_state():
    """tests/test_merge_landmarks_cpu.py's state and a third uncorrelated landmark at (0, 1) with block diag(1, 1)."""
    x = np.array([0.5, -0.25, 30.0, 0.0, 0.0, 4.0, 2.0, 0.0, 1.0])
    P = np.diag([0.1, 0.1, 0.01, 3.0, 1.0, 1.0, 1.0, 1.0, 1.0])
    return x, np.array([1.0, 2.0, 3.0]), P


def test_known_answer_and_the_tie_rule():
    x, s, P = _known_answer_state()
    D = pair_matrix(x, P)
    assert abs(D[1, 0] - 6.0) < 1e-14 and abs(D[2, 0] - 0.5) < 1e-15 and abs(D[2, 1] - 8.5) < 1e-14     # 16/4 + 4/2; 1/2; 16/2 + 1/2
    best, partner, _ = nearest_dense(x, P)
    assert partner.tolist() == [-1, 0, 0] and np.isinf(best[0]) and abs(best[1] - 6.0) < 1e-14 and abs(best[2] - 0.5) < 1e-15
    # mirrored: landmarks 0 and 1 at equal distance from landmark 2 -- an exact tie, the lower index wins
    xm = np.array([0.5, -0.25, 30.0, -4.0, 0.0, 4.0, 0.0, 0.0, 0.0])
    Pm = np.diag([0.1, 0.1, 0.01, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0])
    Dm = pair_matrix(xm, Pm)
    assert Dm[2, 0] == Dm[2, 1] == 8.0
    best, partner, ratio = nearest_dense(xm, Pm)
    assert partner.tolist() == [-1, 0, 0] and best[2] == 8.0 and ratio[2] == 1.0
    # an irregular pair (S = 0) is masked, never a NaN
    xs = np.array([0.0, 0.0, 0.0, 2.0, 1.0, 2.0, 1.0])
    Ps = np.diag([0.1, 0.1, 0.01, 1.0, 0.5, 1.0, 0.5])
    Ps[3:5, 5:7] = Ps[5:7, 3:5] = np.diag([1.0, 0.5])
    best, partner, _ = nearest_dense(xs, Ps)
    assert partner.tolist() == [-1, -1] and np.isinf(best).all()


def test_the_numpy_fusion_loop_merges_the_planted_pairs_in_order_of_distance():
    x, s, d, U = lowrank_data(60, 7)
    pairs = [(2, 30), (10, 11), (40, 59)]
    x = plant_duplicates(x, pairs, scale=0.4)
    P = np.diag(d) + U @ U.T
    minima = np.sort(nearest_dense(x, P, RPOS)[0][1:])
    assert minima[3] >= 2.0 * minima[2]
    gate = float(np.sqrt(minima[2] * minima[3]))
    x2, s2, P2, merges = fuse_dense(x, s, P, gate, RPOS)
    # the planted pairs in the order of their distances on the untouched state (they share no landmark, and a merge moves the other
    # pairs' d2 by far less than they differ), each with the numbers it has once the earlier drops are gone
    order = sorted(pairs, key=lambda p: constrain_dense(x, P, p[1], p[0], None, RPOS)[2])
    want, gone = [], []
    for keep, drop in order:
        want.append((keep - sum(g < keep for g in gone), drop - sum(g < drop for g in gone)))
        gone.append(drop)
    assert [(k, dr) for k, dr, _ in merges] == want
    assert merges[0][2] == minima[0] and s2.size == 57 and x2.size == 3 + 2 * 57 and P2.shape == (x2.size, x2.size)
    assert s2.tolist() == [v for v in s.tolist() if v not in (31.0, 12.0, 60.0)]          # each keep retains its signature
    assert fuse_dense(x, s, P, gate, RPOS, max_merges=1)[3] == merges[:1]


class _Recorder(RecorderBase):
    """Stand-in for the loaded library (no GPU here): five landmarks; landmark 0 has no partner, landmark 3 neither."""

    status_string = b"ok"
    last_error = b""

    D2 = [np.inf, 0.25, 7.0, np.inf, 0.125]
    PARTNER = [-1, 0, 0, -1, 2]

    def __init__(self):
        self.calls = []
        self.N = 5
        self.D2, self.PARTNER = list(self.D2), list(self.PARTNER)

    def ekf_num_landmarks(self, h, pn):
        pn._obj.value = self.N
        return 0

    def ekf_nearest_landmarks(self, h, R, d2, partner):
        self.calls.append(("nearest", None if R is None else [float(R[k]) for k in range(4)]))
        for k in range(self.N):
            d2[k] = self.D2[k]
            partner[k] = self.PARTNER[k]
        return 0

    def ekf_merge_landmarks(self, h, keep, drop, R):
        self.calls.append(("merge", int(keep), int(drop), None if R is None else [float(R[k]) for k in range(4)]))
        # the stand-in's map after a merge: the merged row and whatever pointed at it are gone
        k = int(drop)
        del self.D2[k], self.PARTNER[k]
        self.PARTNER = [-1 if p == k else (p - 1 if p > k else p) for p in self.PARTNER]
        self.D2 = [np.inf if p < 0 else v for v, p in zip(self.D2, self.PARTNER)]
        self.N -= 1
        return 0


def test_engine_and_slam_layers_convert_indices_once(monkeypatch):
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import engine as E
    from ekf_slam_amd import slam as S
    from ekf_slam_amd.trajectory import TrajectoryLog
    rec = _Recorder()
    monkeypatch.setattr(L, "lib", lambda: rec)
    e = E.Engine(capacity=16)
    R = np.array([[0.5, 0.1], [0.1, 0.25]])
    d2, partner = e.nearest_landmarks()
    assert partner.dtype == np.int64 and partner.tolist() == [-1, 0, 0, -1, 2] and d2.tolist() == [np.inf, 0.25, 7.0, np.inf, 0.125]
    e.nearest_landmarks(R)
    assert rec.calls == [("nearest", None), ("nearest", [0.5, 0.1, 0.1, 0.25])]
    # the gate filters, (d2, i) orders; 0-based (i, j, d2)
    assert e.duplicate_candidates(1.0) == [(4, 2, 0.125), (1, 0, 0.25)]
    assert e.duplicate_candidates(7.0, R) == [(4, 2, 0.125), (1, 0, 0.25), (2, 0, 7.0)] and e.duplicate_candidates(0.1) == []
    for cls in (S.EKF_SLAM, S.EKF_SLAM_UC):
        rec = _Recorder()
        monkeypatch.setattr(L, "lib", lambda: rec)
        f = cls(capacity=16)
        f.log = TrajectoryLog()
        d2, partner = f.nearest_landmarks(R)
        assert partner.tolist() == [0, 1, 1, 0, 3] and d2.tolist() == [np.inf, 0.25, 7.0, np.inf, 0.125]     # 1-based, 0 = none
        assert f.duplicate_candidates(1.0) == [(5, 3, 0.125), (2, 1, 0.25)]
        rec.calls.clear()
        merges = f.fuse_duplicates(1.0, R)
        # search; merge(keep = j, drop = i) of the smallest (d2, i) -- 1-based (3, 5) reaches the library as (2, 4); search again; ...
        Rl = [0.5, 0.1, 0.1, 0.25]
        assert rec.calls == [("nearest", Rl), ("merge", 2, 4, Rl), ("nearest", Rl), ("merge", 0, 1, Rl), ("nearest", Rl)]
        assert merges == [(3, 5, 0.125), (1, 2, 0.25)]
        # every merge went through merge_landmarks: the log has them, with the 1-based numbers, and nothing else
        assert [(kind, idx.tolist()) for _, kind, idx, _, _ in f.log.edits] == [("merge", [3, 5]), ("merge", [1, 2])]
        rec2 = _Recorder()
        monkeypatch.setattr(L, "lib", lambda: rec2)
        g = cls(capacity=16)
        assert g.fuse_duplicates(1.0, None, max_merges=1) == [(3, 5, 0.125)]
        assert rec2.calls == [("nearest", None), ("merge", 2, 4, None)]
        assert g.fuse_duplicates(0.01) == []


_STUB = r'''
#include <math.h>
#include <stdio.h>
#include "ekfslam.h"
void stub_fail_next(ekf_handle *h);
static int fail_armed;
void arm_failure(void) { fail_armed = 1; }
int32_t ekf_nearest_landmarks(ekf_handle *h, const double R[4], double *d2, int64_t *partner) {
    int64_t N;
    ekf_num_landmarks(h, &N);
    printf("ABI ekf_nearest_landmarks N=%lld R=%g,%g,%g,%g\n", (long long)N, R[0], R[1], R[2], R[3]);
    if (fail_armed) { fail_armed = 0; stub_fail_next(h); return ekf_flush(h); }
    for (int64_t i = 0; i < N; ++i) { d2[i] = i ? 0.5 * (double)i : INFINITY; partner[i] = i - 1; }     /* -1, 0, 1, ... */
    return EKF_OK;
}
'''

_DRIVER = driver(r'''
    const mxArray *R = mock_double(2, 2, (const double[]){ 4, 1, 1, 9 });
    const mxArray *near[3] = { mock_string("nearest_landmarks"), h, R };
    if (call("nearest_landmarks", 2, 3, near)) return 1;                       /* the empty map */
    const mxArray *sx[3] = { mock_string("set_x"), h, mock_double(1, 9, (const double[]){ 0, 0, 0, 1, 2, 3, 4, 5, 6 }) };
    if (call("set_x", 0, 3, sx)) return 1;
    if (call("nearest_landmarks", 2, 3, near) || call("nearest_landmarks", 1, 3, near)) return 1;
    const mxArray *badr[3] = { mock_string("nearest_landmarks"), h, mock_double(2, 1, (const double[]){ 1, 2 }) };
    const mxArray *noh[3] = { mock_string("nearest_landmarks"), mock_double(1, 1, (const double[]){ 1 }), R };
    if (!call("nearest_landmarks", 2, 2, near) || !call("nearest_landmarks", 2, 3, badr) || !call("nearest_landmarks", 2, 3, noh)) return 1;
    arm_failure();
    if (!call("nearest_landmarks", 2, 3, near)) return 1;
''', PRELUDE_SHOWN)

_DRIVER_WITHOUT = driver_without(r'''
    const mxArray *near[3] = { mock_string("nearest_landmarks"), h, mock_double(2, 2, (const double[]){ 0, 0, 0, 0 }) };
    if (!call("nearest_landmarks", 1, 3, near)) return 1;
''')


def test_mex_gateway_hands_out_one_based_partners(tmp_path):
    t = transcript_of(tmp_path, _STUB, _DRIVER)
    i = t.index("ABI ekf_nearest_landmarks N=0 R=4,1,1,9")
    assert t[i + 1] == "MEX nearest_landmarks nrhs=3 -> ok out0=0x1[] out1=0x1[]"
    i = t.index("ABI ekf_nearest_landmarks N=3 R=4,1,1,9")
    # the ABI's partners -1, 0, 1 arrive as 0 (none), 1, 2: converted once
    assert t[i + 1] == "MEX nearest_landmarks nrhs=3 -> ok out0=3x1[inf,0.5,1] out1=3x1[0,1,2]"
    assert "MEX nearest_landmarks nrhs=3 -> ok out0=3x1[inf,0.5,1]" in t                # d2 = ... alone: partner is not leaked
    assert any(ln.startswith("MEX nearest_landmarks nrhs=2 -> ERROR ekfslam:usage") and "needs 3 arguments" in ln for ln in t)
    assert any(ln.startswith("MEX nearest_landmarks nrhs=3 -> ERROR ekfslam:usage") and "R needs 2 x 2 elements" in ln for ln in t)
    assert any(ln.startswith("MEX nearest_landmarks nrhs=3 -> ERROR ekfslam:handle") for ln in t)
    assert "MEX nearest_landmarks nrhs=3 -> ERROR ekfslam:status | call not valid in the current state: injected failure" in t
    assert t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_the_gateway_still_links_against_a_library_without_the_symbol(tmp_path):
    t = transcript_of(tmp_path, _DRIVER_WITHOUT)
    assert any(ln.startswith("MEX nearest_landmarks ") and "ERROR ekfslam:usage" in ln and "this libekfslam has no ekf_nearest_landmarks" in ln
               for ln in t)
    assert "MEX predict nrhs=3 -> ok" in t and t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_matlab_methods_forward_to_the_gateway_command():
    text = open(os.path.join(ROOT, "matlab", "EKF_SLAM.m")).read()
    m = re.search(r"function\s+\[d2,\s*partner\]\s*=\s*nearestLandmarks\(h,\s*R\)(.*?)\n        end\b", text, re.S)
    assert m and re.search(r"\[d2,\s*partner\]\s*=\s*h\.gateway\('nearest_landmarks',\s*double\(R\)\)", m.group(1))
    m = re.search(r"function\s+merges\s*=\s*fuseDuplicates\(h,\s*gate,\s*R,\s*maxMerges\)(.*?)\n        end\b", text, re.S)
    assert m and "h.nearestLandmarks(R)" in m.group(1) and re.search(r"h\.mergeLandmarks\(partner\(k\),\s*k,\s*R\)", m.group(1))
    src = open(os.path.join(ROOT, "matlab", "ekfslam_mex.c")).read()
    assert 'strcmp(cmd, "nearest_landmarks")' in src and "#pragma weak ekf_nearest_landmarks" in src
