"""CPU: the surfaces of the batch fusion (ekf_merge_landmarks_batch; include/ekfslam.h) that need no GPU -- the
hand-checkable answer of the definition's NumPy restatement; header, library and ctypes binding agree on the new symbol; Engine
(0-based) and the 1-based layer of ekf_slam_amd/slam.py convert indices once and log ONE 'merge_batch' edit (none for a refused
call); the selection rule of fuse_duplicates_batched as a pure function; the trajectory log's third format; the MEX gateway under the
MEX mock with a recording stand-in for the new entry point, and linked against a stand-in that lacks it."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import RPOS, RecorderBase, host_build
from merge_batch_cases import INDEX, INVALID_ARG, MERGE_BATCH_MAX, chain_regularity, dense_of, merge_batch_dense, planted, refusal, survivor_index
from merge_cases import merge_dense
from mex_harness import PRELUDE_SHOWN, ROOT, driver, driver_without, transcript_of


# ------------------------------------------------------------------------------------------------------------------
# the definition, by hand
# ------------------------------------------------------------------------------------------------------------------
def test_three_uncorrelated_landmarks_fuse_into_the_product_of_three_gaussians():
    x = np.array([0.5, -0.25, 30.0, 0.0, 0.0, 3.0, 0.0, 0.0, 3.0])
    P = np.diag([0.1, 0.1, 0.01, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0])
    s = np.array([1.0, 2.0, 3.0])
    x2, s2, P2, d2 = merge_batch_dense(x, s, P, [(0, 1), (0, 2)], None)
    np.testing.assert_allclose(d2, [4.5, 7.5], rtol=1e-14)   # 9 / 2; then (1.5^2 + 3^2) / 1.5
    np.testing.assert_allclose(x2, [0.5, -0.25, 30.0, 1.0, 1.0], rtol=1e-14)
    np.testing.assert_allclose(P2[3:, 3:], np.eye(2) / 3.0, rtol=1e-14)
    np.testing.assert_array_equal(P2[:3, :3], P[:3, :3])
    assert s2.tolist() == [1.0]
    # m = 1 is a merge
    a, b = merge_batch_dense(x, s, P, [(2, 0)], RPOS), merge_dense(x, s, P, 2, 0, RPOS)
    for u, v in zip(a[:3], b):
        np.testing.assert_array_equal(u, v)


def test_the_refusal_predicate_and_the_survivor_rule():
    assert refusal(10, [(1, 2), (1, 3)]) is None             # a shared keep is fine
    assert refusal(10, [(1, 1)]) == INVALID_ARG and refusal(10, [(1, 2), (3, 2)]) == INVALID_ARG
    assert refusal(10, [(1, 2), (2, 3)]) == INVALID_ARG       # a keep that is dropped: chains are the caller's to order
    assert refusal(10, [(1, 10)]) == INDEX and refusal(10, [(-1, 2)]) == INDEX
    assert refusal(100, [(k, 50 + k) for k in range(MERGE_BATCH_MAX)]) is None
    assert refusal(100, [(k, 50 + k) for k in range(MERGE_BATCH_MAX + 1)]) == INVALID_ARG
    assert refusal(10, [(1, 1), (1, 10)]) == INVALID_ARG      # arguments before indices
    assert [survivor_index([(5, 2), (5, 7), (9, 0)], k) for k in (1, 5, 9)] == [0, 3, 6]


def test_the_planted_map_is_regular_for_the_reference_route():
    x, s, d, U, pairs = planted()
    assert len(pairs) == 16 and len({dr for _, dr in pairs}) == 16 and len({kp for kp, _ in pairs}) == 14
    assert all(kp < 150 <= dr for kp, dr in pairs) and pairs[14][0] == pairs[0][0] and pairs[15][0] == pairs[1][0]
    assert refusal(300, pairs) is None
    P = dense_of(d, U)
    for R, floor in ((None, 0.028), (RPOS, 0.037)):
        worst, d2 = chain_regularity(x, P, pairs, R)
        assert worst > floor and d2.max() < 0.08
        assert np.linalg.eigvalsh(merge_batch_dense(x, s, P, pairs, R)[2]).min() > 0.9e-3


# ------------------------------------------------------------------------------------------------------------------
# header, library, binding
# ------------------------------------------------------------------------------------------------------------------
def test_library_exports_and_binds_the_entry_point():
    import ekf_slam_amd
    from ekf_slam_amd import _lib
    ekf_slam_amd.build()
    L = ekf_slam_amd.lib()
    vp, dp, ip = ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
    assert hasattr(L, "ekf_merge_landmarks_batch")
    res, sig = _lib.SIGNATURES["ekf_merge_landmarks_batch"]
    assert res is ctypes.c_int32 and sig == [vp, ip, ip, ctypes.c_int64, dp, dp] and L.ekf_merge_landmarks_batch.argtypes == sig
    assert L.ekf_abi_version() == 1                          # an added entry point is compatible
    assert _lib.EKF_KERNEL_COUNT == 8                        # no new timing id: EKF_KERNEL_GATHER and EKF_KERNEL_DOWNDATE count the launches
    header = open(os.path.join(ROOT, "include", "ekfslam.h")).read()
    assert re.search(r"int32_t\s+ekf_merge_landmarks_batch\(ekf_handle \*h,\s*const int64_t \*keep,\s*const int64_t \*drop,\s*int64_t m,"
                     r"\s*const double R\[4\][^;]*double \*d2[^;]*\);", header)
    m = re.search(r"#define\s+EKF_MERGE_BATCH_MAX\s+(\d+)", header)
    assert m and int(m.group(1)) == _lib.EKF_MERGE_BATCH_MAX == MERGE_BATCH_MAX == 32
    assert "EKF_KERNEL_COUNT = 8" in header
    # a null handle is refused without touching a device
    k = (ctypes.c_int64 * 1)(0)
    assert L.ekf_merge_landmarks_batch(None, k, k, 1, None, None) == _lib.EKF_ERR_INVALID_ARG


def test_the_device_side_is_where_the_design_says():
    csrc = os.path.join(ROOT, "ekf_slam_amd", "csrc")
    constrain = open(os.path.join(csrc, "constrain.h")).read()
    assert "void k_gather_constrain(DevState st, ConstrainArgs a, double *__restrict__ rec)" in constrain and "k_gather_constrain_chain" not in constrain
    assert "constrain_row_pair_chain" in constrain and "ekfm::constrain_d2(" in constrain
    fused = open(os.path.join(csrc, "merge_pass.h")).read()
    assert "k_merge_pass" in fused and "rank2_apply(" in fused and "__shared__" not in fused
    edits = open(os.path.join(csrc, "host", "edits.h")).read()
    impl = edits[edits.index("int32_t ekf_merge_landmarks_batch("):]
    impl = impl[:impl.index("\n}\n")]
    assert "EKF_KERNEL_DOWNDATE" in impl and "EKF_KERNEL_COMPACT" not in impl and "h->npend" not in impl and "h->pstart" not in impl
    assert "merge_pass.h" in open(os.path.join(csrc, "Makefile")).read()


def test_the_kernel_sources_emulated_on_the_host_give_the_sequence_bit_for_bit(tmp_path):
    """tests/support/merge_batch_host_emulation.cpp: the chain of gathers and the fused pass, compiled for the host behind a thread-index
    shim, against the one-pair gather (the same kernel with nothing pending and no record) + pass + compaction route -- x, strip, Prr, diagonal blocks, s, tiles and d2, bit for bit, with a
    shared keep, keep > drop, drops at landmark 0 and N - 1, an adjacent pair, R = 0 and R > 0; address and UB sanitizers on."""
    exe = host_build("merge_batch_host_emulation", str(tmp_path / "emulation"),
                     ["-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and len(lines) == 4 and all(ln.endswith(")") and ": 0 differences" in ln for ln in lines), r.stdout[-2000:] + r.stderr[-4000:]


# ------------------------------------------------------------------------------------------------------------------
# the Python layers
# ------------------------------------------------------------------------------------------------------------------
class _Recorder(RecorderBase):
    """Stand-in for the loaded library (no GPU here)."""

    last_error = b"merge_landmarks_batch: pair 1: injected"

    def __init__(self, N=9):
        self.calls, self.N, self.fail = [], N, 0

    def ekf_num_landmarks(self, h, pn):
        pn._obj.value = self.N
        return 0

    def ekf_merge_landmarks_batch(self, h, keep, drop, m, R, d2):
        self.calls.append(("merge_batch", [int(keep[k]) for k in range(m)], [int(drop[k]) for k in range(m)],
                           None if R is None else [float(R[k]) for k in range(4)]))
        if self.fail:
            return self.fail
        for k in range(m):
            d2[k] = 0.25 * (k + 1)
        self.N -= m
        return 0

    def ekf_predict(self, h, u):
        self.calls.append(("predict",))
        return 0

    def ekf_remove_landmarks(self, h, idx, m):
        self.calls.append(("remove", [int(idx[k]) for k in range(m)]))
        return 0


def test_engine_and_slam_layers_convert_indices_once_and_log_one_edit(monkeypatch):
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import engine as E
    from ekf_slam_amd import slam as S
    from ekf_slam_amd.trajectory import TrajectoryLog
    rec = _Recorder()
    monkeypatch.setattr(L, "lib", lambda: rec)
    e = E.Engine(capacity=16)
    R = np.array([[0.5, 0.1], [0.1, 0.25]])
    Rl = [0.5, 0.1, 0.1, 0.25]
    d2 = e.merge_landmarks_batch([(2, 4), (0, 1), (2, 7)], R)
    assert d2.tolist() == [0.25, 0.5, 0.75]
    assert e.merge_landmarks_batch([], None).size == 0
    assert rec.calls == [("merge_batch", [2, 0, 2], [4, 1, 7], Rl), ("merge_batch", [], [], None)]
    with pytest.raises(ValueError):
        e.merge_landmarks_batch([(1.5, 2)])
    with pytest.raises(ValueError):
        e.merge_landmarks_batch([(1, 2, 3)])
    assert len(rec.calls) == 2
    for cls in (S.EKF_SLAM, S.EKF_SLAM_UC):
        rec = _Recorder()
        monkeypatch.setattr(L, "lib", lambda: rec)
        f = cls(capacity=16)
        f.log = TrajectoryLog()
        d2 = f.merge_landmarks_batch([(3, 5), (1, 2)], R)    # 1-based here: reaches the library as (2, 4), (0, 1)
        assert d2.tolist() == [0.25, 0.5]
        assert rec.calls == [("merge_batch", [2, 0], [4, 1], Rl)]
        assert [(step, kind, idx.tolist(), Rm.tolist()) for step, kind, idx, _, Rm in f.log.edits] == [(0, "merge_batch", [3, 5, 1, 2], R.tolist())]
        with pytest.raises(ValueError):
            f.merge_landmarks_batch([(1.5, 2)])
        # a refused call raises and is not logged
        rec.fail = L.EKF_ERR_STATE
        with pytest.raises(L.EkfError) as info:
            f.merge_landmarks_batch([(1, 2)])
        assert info.value.status == L.EKF_ERR_STATE and "pair 1" in str(info.value)
        assert len(f.log.edits) == 1 and len(rec.calls) == 2


def test_select_merge_batch():
    from ekf_slam_amd.slam import select_merge_batch
    # a triple: landmarks 5 and 9 both duplicate landmark 2 -- a shared keep, one batch
    assert select_merge_batch([(5, 2, 0.1), (9, 2, 0.2)], 32) == [(2, 5, 0.1), (2, 9, 0.2)]
    # 9's partner is 5, which was just dropped: the row waits for the next search; 7 -> 3 is unrelated and goes
    assert select_merge_batch([(5, 2, 0.1), (9, 5, 0.2), (7, 3, 0.3)], 32) == [(2, 5, 0.1), (3, 7, 0.3)]
    # i already a keep: (6 <- 8) made 6 a keep, so dropping 6 must wait
    assert select_merge_batch([(8, 6, 0.1), (6, 1, 0.2)], 32) == [(6, 8, 0.1)]
    # i already a drop never repeats
    assert select_merge_batch([(8, 6, 0.1), (8, 2, 0.2)], 32) == [(6, 8, 0.1)]
    rows = [(10 + k, k, 0.01 * k) for k in range(1, 8)]
    assert select_merge_batch(rows, 3) == [(1, 11, 0.01), (2, 12, 0.02), (3, 13, 0.03)]
    assert select_merge_batch(rows, 0) == [] and select_merge_batch([], 5) == []
    out = select_merge_batch(rows, 32)
    assert refusal(20, [(k, d) for k, d, _ in out]) is None


class _Policy:
    """fuse_duplicates_batched over a scripted sequence of searches"""

    def __init__(self, searches):
        self.searches, self.batches = list(searches), []

    def duplicate_candidates(self, gate, R=None):
        return self.searches.pop(0) if self.searches else []

    def merge_landmarks_batch(self, pairs, R=None):
        self.batches.append(list(pairs))
        return np.array([0.5 + k for k in range(len(pairs))])


def test_fuse_duplicates_batched_is_search_select_one_batch():
    from ekf_slam_amd import slam as S
    fuse = S._EkfBase.fuse_duplicates_batched
    p = _Policy([[(5, 2, 0.1), (9, 5, 0.2), (7, 3, 0.3)], [(8, 2, 0.15)], []])
    merges = fuse(p, 1.0)
    assert p.batches == [[(2, 5), (3, 7)], [(2, 8)]]
    assert merges == [(2, 5, 0.5), (3, 7, 1.5), (2, 8, 0.5)]  # d2 as the batch call reported it
    p = _Policy([[(5, 2, 0.1), (9, 5, 0.2), (7, 3, 0.3)], [(8, 2, 0.15)], []])
    assert fuse(p, 1.0, None, max_merges=1) == [(2, 5, 0.5)] and p.batches == [[(2, 5)]]
    p = _Policy([[(100 + k, k, 0.01) for k in range(1, 41)], []])
    assert len(fuse(p, 1.0)) == MERGE_BATCH_MAX and len(p.batches[0]) == MERGE_BATCH_MAX      # one call takes at most the maximum
    # fuse_duplicates itself is a different policy and still says so
    assert "not the fastest" in S._EkfBase.fuse_duplicates.__doc__


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

    def constrain_landmarks(self, i, j, delta, R):
        self.calls.append(("constrain", i, j))

    def merge_landmarks(self, keep, drop, R):
        self.calls.append(("merge", keep, drop))

    def merge_landmarks_batch(self, pairs, R):
        self.calls.append(("merge_batch", list(pairs), np.asarray(R).tolist()))


def _steps(log, n):
    for k in range(n):
        log.record([0.1, 1.0 + k], np.array([[1.0, 2.0, 3.0]]) if k % 2 else None, [1.0, 2.0], [[0.0, 1.0], [2.0, 3.0]])


def test_trajectory_format_three_round_trip_and_the_older_formats(tmp_path):
    from ekf_slam_amd.trajectory import EDIT_KINDS, FORMAT, FORMAT_BATCH, FORMAT_EDITS, TrajectoryLog
    assert EDIT_KINDS == ("remove", "constrain", "merge", "merge_batch") and FORMAT_BATCH == "ekfslam-trajectory-3"
    base_keys = {"format", "u", "obs_ptr", "obs", "lm_ptr", "lm_index", "lm_loc"}
    edit_keys = base_keys | {"edit_step", "edit_kind", "edit_ptr", "edit_idx", "edit_delta", "edit_R"}
    # format 1: no edits; format 2: the three older kinds -- written exactly as before
    one = TrajectoryLog(); _steps(one, 3)
    one.save(tmp_path / "one.npz")
    g = np.load(tmp_path / "one.npz")
    assert str(g["format"]) == FORMAT == "ekfslam-trajectory-1" and set(g.files) == base_keys
    two = TrajectoryLog(); _steps(two, 2)
    two.record_edit("remove", [4, 2]); two.record_edit("constrain", [1, 2], [0.5, 0.0], RPOS); _steps(two, 1); two.record_edit("merge", [3, 1], None, RPOS)
    two.save(tmp_path / "two.npz")
    g = np.load(tmp_path / "two.npz")
    assert str(g["format"]) == FORMAT_EDITS == "ekfslam-trajectory-2" and set(g.files) == edit_keys
    assert g["edit_kind"].tolist() == [0, 1, 2] and g["edit_idx"].tolist() == [4, 2, 1, 2, 3, 1] and g["edit_ptr"].tolist() == [0, 2, 4, 6]
    assert [e[1] for e in TrajectoryLog.load(tmp_path / "two.npz").edits] == ["remove", "constrain", "merge"]
    # format 3: a merge_batch among them
    three = TrajectoryLog(); _steps(three, 2)
    three.record_edit("remove", [7])
    three.record_edit("merge_batch", [3, 5, 1, 2, 3, 6], None, RPOS)
    _steps(three, 2)
    three.record_edit("merge_batch", [2, 4])
    three.save(tmp_path / "three.npz")
    g = np.load(tmp_path / "three.npz")
    assert str(g["format"]) == FORMAT_BATCH and set(g.files) == edit_keys and g["edit_kind"].tolist() == [0, 3, 3]
    back = TrajectoryLog.load(tmp_path / "three.npz")
    assert len(back) == 4 and [(e[0], e[1], e[2].tolist()) for e in back.edits] == [(2, "remove", [7]), (2, "merge_batch", [3, 5, 1, 2, 3, 6]),
                                                                                  (4, "merge_batch", [2, 4])]
    np.testing.assert_array_equal(back.edits[1][4], RPOS)
    np.testing.assert_array_equal(back.edits[2][4], np.zeros((2, 2)))
    # replay order: the edits in front of their step, 0-based pairs, the last one after the last step
    r = _Replayed()
    back.replay(r)
    assert r.calls == [("predict",), ("predict",), ("measure",), ("remove", [6]), ("merge_batch", [(2, 4), (0, 1), (2, 5)], RPOS.tolist()),
                       ("predict",), ("predict",), ("measure",), ("merge_batch", [(1, 3)], [[0.0, 0.0], [0.0, 0.0]])]
    # bad shapes
    bad = TrajectoryLog()
    for idx in ([], [1], [1, 2, 3], [1.5, 2]):
        with pytest.raises(ValueError):
            bad.record_edit("merge_batch", idx)
    with pytest.raises(ValueError):
        bad.record_edit("merge_many", [1, 2])
    assert bad.edits == []
    np.savez_compressed(tmp_path / "four.npz", format=np.array("ekfslam-trajectory-4"))
    with pytest.raises(ValueError):
        TrajectoryLog.load(tmp_path / "four.npz")


# ------------------------------------------------------------------------------------------------------------------
# the MEX gateway under the mock
# ------------------------------------------------------------------------------------------------------------------
_STUB = r'''
#include <stdio.h>
#include "ekfslam.h"
void stub_fail_next(ekf_handle *h);
static int fail_armed;
void arm_failure(void) { fail_armed = 1; }
int32_t ekf_merge_landmarks_batch(ekf_handle *h, const int64_t *keep, const int64_t *drop, int64_t m, const double R[4], double *d2) {
    printf("ABI ekf_merge_landmarks_batch m=%lld R=%g,%g,%g,%g pairs=", (long long)m, R[0], R[1], R[2], R[3]);
    for (int64_t k = 0; k < m; ++k) printf("(%lld<-%lld)", (long long)keep[k], (long long)drop[k]);
    printf("\n");
    if (fail_armed) { fail_armed = 0; stub_fail_next(h); return ekf_flush(h); }
    for (int64_t k = 0; k < m; ++k) d2[k] = 0.5 * (double)(k + 1);
    return EKF_OK;
}
'''

_DRIVER = driver(r'''
    const mxArray *R = mock_double(2, 2, (const double[]){ 4, 1, 1, 9 });
    /* pairs = [3 5; 1 2; 3 8], column-major: the keeps, then the drops */
    const mxArray *pairs = mock_double(3, 2, (const double[]){ 3, 1, 3, 5, 2, 8 });
    const mxArray *mb[4] = { mock_string("merge_landmarks_batch"), h, pairs, R };
    if (call("merge_landmarks_batch", 1, 4, mb)) return 1;
    double big[2 * 33];
    for (int i = 0; i < 33; ++i) { big[i] = 1 + i; big[33 + i] = 101 + i; }
    const mxArray *wide[4] = { mock_string("merge_landmarks_batch"), h, mock_double(2, 3, (const double[]){ 1, 2, 3, 4, 5, 6 }), R };
    const mxArray *flat[4] = { mock_string("merge_landmarks_batch"), h, mock_double(1, 3, (const double[]){ 1, 2, 3 }), R };
    const mxArray *many[4] = { mock_string("merge_landmarks_batch"), h, mock_double(33, 2, big), R };
    const mxArray *frac[4] = { mock_string("merge_landmarks_batch"), h, mock_double(1, 2, (const double[]){ 1.5, 2 }), R };
    const mxArray *nanp[4] = { mock_string("merge_landmarks_batch"), h, mock_double(1, 2, (const double[]){ 1, 0.0 / 0.0 }), R };
    if (!call("merge_landmarks_batch frac", 1, 4, frac) || !call("merge_landmarks_batch nanp", 1, 4, nanp)) return 1;
    const mxArray *badr[4] = { mock_string("merge_landmarks_batch"), h, pairs, mock_double(2, 1, (const double[]){ 1, 2 }) };
    const mxArray *noh[4] = { mock_string("merge_landmarks_batch"), mock_double(1, 1, (const double[]){ 1 }), pairs, R };
    if (!call("merge_landmarks_batch", 1, 3, mb) || !call("merge_landmarks_batch wide", 1, 4, wide) || !call("merge_landmarks_batch flat", 1, 4, flat) ||
        !call("merge_landmarks_batch many", 1, 4, many) || !call("merge_landmarks_batch badr", 1, 4, badr) || !call("merge_landmarks_batch noh", 1, 4, noh))
        return 1;
    arm_failure();
    if (!call("merge_landmarks_batch", 1, 4, mb)) return 1;
''', PRELUDE_SHOWN)

_DRIVER_WITHOUT = driver_without(r'''
    const mxArray *mb[4] = { mock_string("merge_landmarks_batch"), h, mock_double(1, 2, (const double[]){ 1, 2 }), mock_double(2, 2, (const double[]){ 0, 0, 0, 0 }) };
    if (!call("merge_landmarks_batch", 1, 4, mb)) return 1;
''')


def test_mex_gateway_converts_the_pairs_once(tmp_path):
    t = transcript_of(tmp_path, _STUB, _DRIVER)
    # MATLAB's [3 5; 1 2; 3 8] arrives as 0-based (2<-4)(0<-1)(2<-7), R column-major as MATLAB holds it
    i = t.index("ABI ekf_merge_landmarks_batch m=3 R=4,1,1,9 pairs=(2<-4)(0<-1)(2<-7)")
    assert t[i + 1] == "MEX merge_landmarks_batch nrhs=4 -> ok out0=3x1[0.5,1,1.5]"
    assert any(ln.startswith("MEX merge_landmarks_batch nrhs=3 -> ERROR ekfslam:usage") and "needs 4 arguments" in ln for ln in t)
    for which in ("wide", "flat"):
        assert any(ln.startswith("MEX merge_landmarks_batch %s nrhs=4 -> ERROR ekfslam:usage" % which) and "pairs needs k x 2 elements" in ln for ln in t)
    for which in ("frac", "nanp"):
        assert any(ln.startswith("MEX merge_landmarks_batch %s nrhs=4 -> ERROR ekfslam:usage" % which) and "whole numbers" in ln for ln in t)
    assert any(ln.startswith("MEX merge_landmarks_batch many nrhs=4 -> ERROR ekfslam:usage") and "at most 32 pairs" in ln for ln in t)
    assert any(ln.startswith("MEX merge_landmarks_batch badr nrhs=4 -> ERROR ekfslam:usage") and "R needs 2 x 2 elements" in ln for ln in t)
    assert any(ln.startswith("MEX merge_landmarks_batch noh nrhs=4 -> ERROR ekfslam:handle") for ln in t)
    assert sum(ln.startswith("ABI ekf_merge_landmarks_batch") for ln in t) == 2       # the good call and the injected failure: no refused shape got through
    assert "MEX merge_landmarks_batch nrhs=4 -> ERROR ekfslam:status | call not valid in the current state: injected failure" in t
    assert t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_the_gateway_still_links_against_a_library_without_the_symbol(tmp_path):
    t = transcript_of(tmp_path, _DRIVER_WITHOUT)
    assert any(ln.startswith("MEX merge_landmarks_batch ") and "ERROR ekfslam:usage" in ln and "this libekfslam has no ekf_merge_landmarks_batch" in ln
               for ln in t)
    assert "MEX predict nrhs=3 -> ok" in t and t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_matlab_methods_forward_to_the_gateway_command():
    text = open(os.path.join(ROOT, "matlab", "EKF_SLAM.m")).read()
    m = re.search(r"function\s+d2\s*=\s*mergeLandmarksBatch\(h,\s*pairs,\s*R\)(.*?)\n        end\b", text, re.S)
    assert m and re.search(r"d2\s*=\s*h\.gateway\('merge_landmarks_batch',\s*double\(reshape\(pairs,\s*\[\],\s*2\)\),\s*double\(R\)\)", m.group(1))
    m = re.search(r"function\s+merges\s*=\s*fuseDuplicatesBatched\(h,\s*gate,\s*R,\s*maxMerges\)(.*?)\n        end\n        function", text, re.S)
    assert m and "h.nearestLandmarks(R)" in m.group(1) and "h.mergeLandmarksBatch(pairs, R)" in m.group(1)
    src = open(os.path.join(ROOT, "matlab", "ekfslam_mex.c")).read()
    assert 'strcmp(cmd, "merge_landmarks_batch")' in src and "#pragma weak ekf_merge_landmarks_batch" in src
