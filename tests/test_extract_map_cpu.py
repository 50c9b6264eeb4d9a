"""CPU: ekf_extract_map without a GPU -- the NumPy restatement of tests/extract_map_cases.py against a finite-difference Jacobian of the
robot-frame map and against the table of include/ekfslam.h block by block; k_extract_state and k_extract_rows compiled for the host on a
source and a destination state (all four storage pairs, both frames) against that restatement; the Python layers over a stand-in for the
library (one marshal per call, 1-based to 0-based, the refusal of a bad frame, split_submap's log); the MEX gateway's command under the MEX
mock; the trajectory formats, which the extraction leaves alone."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import extract_map_cases as X
from helpers import REL, ROOT, TOL_KEPT32, TOL_ROW32, TOL_X32, RecorderBase, host_build, rel_err, same_npz
from mex_harness import PRELUDE_SHOWN, driver, driver_without, transcript_of

SIZES = [(13, 0, None), (13, 1, None), (13, 13, "shuffled"), (40, 21, "scattered")]


def plan_of(N, m, plan):
    if m == 0:
        return []
    if m == 1:
        return [7]
    return X.PLANS[plan](N, m, seed=N + m)


# ------------------------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------------------------
def test_the_index_plans_hold_both_ends_and_no_landmark_twice():
    for name, plan in X.PLANS.items():
        for N, m in ((13, 2), (13, 13), (40, 21), (140, 131)):
            idx = plan(N, m, seed=3)
            assert len(idx) == m and len(set(idx)) == m and 0 in idx and N - 1 in idx and all(0 <= i < N for i in idx), name
        assert plan(13, 0) == [] and plan(13, 1) == [0]
    assert X.plan_run(40, 5) == sorted(X.plan_run(40, 5)) and X.plan_scattered(40, 21, 1) == sorted(X.plan_scattered(40, 21, 1))
    assert X.plan_reversed(40, 21, 1) == sorted(X.plan_scattered(40, 21, 1), reverse=True)
    assert X.plan_shuffled(40, 21, 1) != sorted(X.plan_shuffled(40, 21, 1))
    assert sorted(X.complement(13, [3, 0, 12]) + [3, 0, 12]) == list(range(13))


@pytest.mark.parametrize("N,m,plan", SIZES)
def test_the_restatement_agrees_with_a_finite_difference_jacobian(N, m, plan):
    idx = plan_of(N, m, plan)
    x, s, P = X.scene(N, 100 + 7 * N + m)
    Jm = X.extract_jacobian(x, idx, "robot")
    fd = np.zeros_like(Jm)
    h = 1e-6
    for k in range(x.size):
        up, dn = x.copy(), x.copy()
        up[k] += h
        dn[k] -= h
        fd[:, k] = (X.extract_fn(up, idx, "robot") - X.extract_fn(dn, idx, "robot")) / (2 * h)
    err = np.abs(fd - Jm).max() / max(np.abs(Jm).max(), 1.0)
    print("N=%d m=%d: finite differences (step 1e-6) against J: worst rel err %.2e" % (N, m, err))
    assert err < 1e-7
    xn, sn, Pn = X.extract_dense(x, s, P, idx, "robot")
    if m:
        assert rel_err(Pn, fd @ P @ fd.T) < 1e-7
    # the table of the issue, block by block
    tol = 1e-13 * np.abs(Pn).max()
    assert not xn[:3].any() and not Pn[:3, :].any() and not Pn[:, :3].any()
    np.testing.assert_array_equal(sn, s[idx] if m else np.zeros(0))
    Prr = P[:3, :3]
    for k, lk in enumerate(idx):
        mk, Hrk, Hl = X.extract_blocks(x, lk)
        np.testing.assert_allclose(xn[3 + 2 * k:5 + 2 * k], mk, rtol=0, atol=1e-13 * np.abs(x).max())
        assert np.abs(mk - X.rot(x[2]).T @ (x[3 + 2 * lk:5 + 2 * lk] - x[:2])).max() < 1e-12
        for a, la in enumerate(idx):
            _, Hra, _ = X.extract_blocks(x, la)
            sk, sa = P[:3, 3 + 2 * lk:5 + 2 * lk], P[:3, 3 + 2 * la:5 + 2 * la]
            want = Hrk @ Prr @ Hra.T + Hrk @ sa @ Hl.T + Hl @ sk.T @ Hra.T + Hl @ P[3 + 2 * lk:5 + 2 * lk, 3 + 2 * la:5 + 2 * la] @ Hl.T
            assert np.abs(Pn[3 + 2 * k:5 + 2 * k, 3 + 2 * a:5 + 2 * a] - want).max() < tol


@pytest.mark.parametrize("N,m,plan", SIZES)
def test_the_map_frame_is_an_indexing(N, m, plan):
    idx = plan_of(N, m, plan)
    x, s, P = X.scene(N, 5 + N + m)
    sel = np.concatenate([[0, 1, 2]] + [[3 + 2 * l, 4 + 2 * l] for l in idx]).astype(int)
    xn, sn, Pn = X.extract_dense(x, s, P, idx, "map")
    np.testing.assert_array_equal(Pn, P[np.ix_(sel, sel)])
    np.testing.assert_array_equal(xn, x[sel])
    np.testing.assert_array_equal(sn, s[idx] if m else np.zeros(0))
    J = X.extract_jacobian(x, idx, "map")
    np.testing.assert_array_equal(J @ P @ J.T, Pn)            # a selection matrix: exact
    with pytest.raises(AssertionError):
        X.extract_fn(x, idx, "world")


def test_a_landmark_on_the_robot_is_regular():
    x, s, P = X.scene_on_robot(6, 2, which=1)
    xn, _, Pn = X.extract_dense(x, s, P, [1, 4], "robot")
    assert not xn[3:5].any() and np.all(np.isfinite(Pn))
    _, Hr, _ = X.extract_blocks(x, 1)
    assert not Hr[:, 2].any()                                 # a zero heading column


# ------------------------------------------------------------------------------------------------------------------
# both kernels compiled for the host
# ------------------------------------------------------------------------------------------------------------------
def _write_cases(d):
    with open(os.path.join(str(d), "cases.txt"), "w") as f:
        for N, m, plan in SIZES:
            f.write(" ".join(str(v) for v in [N, m] + plan_of(N, m, plan)) + "\n")


@pytest.fixture(scope="module")
def emulation(tmp_path_factory):
    d = tmp_path_factory.mktemp("extract_map_emulation")
    _write_cases(d)
    exe = host_build("extract_map_host_emulation", str(d / "emu"))
    r = subprocess.run([exe, str(d)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    return d, r.stdout


def _read(path):
    v = np.fromfile(path)
    N, m, frame = int(v[0]), int(v[1]), int(v[2])
    pos = [3]

    def take(count, shape=None):
        out = v[pos[0]:pos[0] + count]
        pos[0] += count
        return out.reshape(shape) if shape else out
    idx = [int(i) for i in take(m)]
    n, nn = 3 + 2 * N, 3 + 2 * m
    x, s, P = take(n), take(N), take(n * n, (n, n))
    xn, sn, Pn = take(nn), take(m), take(nn * nn, (nn, nn))
    assert pos[0] == v.size
    return idx, X.FRAMES[frame], (x, s, P), (xn, sn, Pn)


@pytest.mark.parametrize("frame", [0, 1])
@pytest.mark.parametrize("pair", ["dd", "df", "fd", "ff"])     # destination tiles, then source tiles: d = F64, f = float
def test_host_emulation_of_both_kernels_against_the_restatement(emulation, pair, frame):
    d, out = emulation
    for N, m, plan in SIZES:
        assert "%s frame=%d N=%d m=%d: 0 differences" % (pair, frame, N, m) in out
        idx, fname, (x, s, P), (xn, sn, Pn) = _read(os.path.join(str(d), "%s_%d_%d_%d.bin" % (pair, frame, N, m)))
        assert idx == plan_of(N, m, plan) and fname == X.FRAMES[frame]
        assert x[5] == x[0] and x[6] == x[1]                  # the emulation puts landmark 1 on the robot
        ex, es, eP = X.extract_dense(x, s, P, idx, fname)
        np.testing.assert_array_equal(sn, es)
        np.testing.assert_array_equal(Pn, Pn.T)
        assert np.all(np.isfinite(Pn))
        if frame == 0 and pair[0] == "d":                     # F64 -> F64 and float -> F64 in the map frame: the widening is exact
            np.testing.assert_array_equal(xn, ex)
            np.testing.assert_array_equal(Pn, eP)
            continue
        n = ex.size
        kept = np.zeros((n, n), dtype=bool)
        kept[:3, :] = kept[:, :3] = True
        for a in range(3, n, 2):
            kept[a:a + 2, a:a + 2] = True
        if frame == 0:                                        # an F64-kept value is never rounded, whatever the stores
            np.testing.assert_array_equal(xn, ex)
            np.testing.assert_array_equal(Pn[kept], eP[kept])
        scale = max(np.abs(eP).max(), 1e-300)
        err_x, err_P = rel_err(xn, ex), float(np.abs(Pn - eP).max() / scale)
        err_kept = float(np.abs(Pn - eP)[kept].max() / scale)
        rows = np.abs(eP).max(axis=1)
        err_row = float((np.abs(Pn - eP).max(axis=1)[rows > 0] / rows[rows > 0]).max(initial=0.0))
        print("%s %s N=%d m=%d: rel err x %.2e P %.2e F64-kept %.2e worst row %.2e" % (pair, fname, N, m, err_x, err_P, err_kept, err_row))
        assert err_x < TOL_X32 and err_kept < TOL_KEPT32 and err_row <= TOL_ROW32
        if pair[0] == "d":                                    # an F64 destination rounds nothing: F64 arithmetic on either source
            assert err_P < REL * 1e-6


def test_kernel_sources_on_the_host_under_the_sanitizers(tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined runs clean: no lane of either kernel reads or writes outside
    the buffers of the two states (nothing loaded into python is involved)."""
    _write_cases(tmp_path)
    exe = host_build("extract_map_host_emulation", str(tmp_path / "emulation_sanitized"),
                     flags=["-O1", "-g", "-mfma", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]


# ------------------------------------------------------------------------------------------------------------------
# the Python layers over a stand-in for the library
# ------------------------------------------------------------------------------------------------------------------
class _Recorder(RecorderBase):
    status_string = b"landmark capacity exhausted"
    last_error = b"extract_map: injected"

    def __init__(self):
        self.calls, self.fail, self.N, self.handles, self.created, self.destroyed = [], 0, {}, 0, [], []

    def ekf_create(self, pcfg, ph):
        from ekf_slam_amd import _lib as L
        cfg = ctypes.cast(pcfg, ctypes.POINTER(L.EkfConfig)).contents
        self.handles += 1
        self.created.append(dict(capacity=cfg.capacity_landmarks, storage=cfg.storage, pass_arith=cfg.pass_arith, tile=cfg.tile, mode=cfg.mode))
        ctypes.cast(ph, ctypes.POINTER(ctypes.c_void_p)).contents.value = 0x1000 * self.handles
        return 0

    def ekf_destroy(self, h):
        self.destroyed.append(h.value if hasattr(h, "value") else h)
        return 0

    def set_count(self, e, N):
        self.N[e.h.value] = N

    def ekf_num_landmarks(self, h, pn):
        pn._obj.value = self.N.get(h.value, 0)
        return 0

    def ekf_extract_map(self, h, idx, m, frame, dst):
        assert isinstance(frame, ctypes.c_int32)              # marshalled once, by marshal.extract_args
        self.calls.append(("extract_map", h.value, [idx[k] for k in range(m)], frame.value, dst.value))
        if self.fail:
            return self.fail
        self.N[dst.value] = m
        return 0

    def ekf_remove_landmarks(self, h, idx, m):
        self.calls.append(("remove", h.value, [idx[k] for k in range(m)]))
        self.N[h.value] = self.N.get(h.value, 0) - m
        return 0

    def ekf_get_x(self, h, p):
        self.calls.append(("get_x", h.value))
        vals = [1.0, 2.0, 30.0, 1.0, 2.5, 10.0, 2.0, 1.0, 4.0, -2.0, 2.0]          # landmarks at distance 0.5, 9, 2, 3 of the robot
        for k in range(3 + 2 * self.N.get(h.value, 0)):
            p[k] = vals[k]
        return 0


def test_layers_marshal_an_extraction_once(monkeypatch):
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import engine as E
    from ekf_slam_amd import marshal
    from ekf_slam_amd import slam as S
    from ekf_slam_amd.sharding import ShardGroup
    from ekf_slam_amd.trajectory import TrajectoryLog
    assert L.SIGNATURES["ekf_extract_map"] == (ctypes.c_int32, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_int64, ctypes.c_int32,
                                                                ctypes.c_void_p])
    assert (L.EKF_FRAME_MAP, L.EKF_FRAME_ROBOT) == (0, 1)
    header = open(os.path.join(ROOT, "include", "ekfslam.h")).read()
    assert "enum { EKF_FRAME_MAP = 0, EKF_FRAME_ROBOT = 1 };" in header
    assert "int32_t ekf_extract_map(ekf_handle *h, const int64_t *idx, int64_t m, int32_t frame, ekf_handle *dst);" in header
    rec = _Recorder()
    monkeypatch.setattr(L, "lib", lambda: rec)
    made = []
    real = marshal.extract_args
    monkeypatch.setattr(marshal, "extract_args", lambda *a, **k: made.append(a) or real(*a, **k))
    g = E.Engine(capacity=32, storage="f32_mixed", tile=256)
    rec.set_count(g, 9)
    # a destination of its own: capacity max(m, 1), the source's storage kind, unless a keyword says otherwise
    d = g.extract_map([4, 0, 8], "robot")
    assert isinstance(d, E.Engine) and d is not g and d.N == 3
    assert rec.calls == [("extract_map", g.h.value, [4, 0, 8], L.EKF_FRAME_ROBOT, d.h.value)] and len(made) == 1
    assert rec.created[-1]["capacity"] == 3 and rec.created[-1]["storage"] == L.EKF_STORE_F32 and rec.created[-1]["pass_arith"] == L.EKF_ARITH_F32
    d0 = g.extract_map([])
    assert rec.calls[-1][2:4] == ([], L.EKF_FRAME_MAP) and rec.created[-1]["capacity"] == 1 and d0.N == 0
    d2 = g.extract_map([1], storage="f64", tile=16, capacity=40)
    assert rec.created[-1]["capacity"] == 40 and rec.created[-1]["storage"] == L.EKF_STORE_F64 and rec.created[-1]["tile"] == 16
    # into an engine that exists: nothing is created, and it is what comes back
    ncreated = len(rec.created)
    assert g.extract_map((2, 3), frame="map", into=d2) is d2 and len(rec.created) == ncreated
    assert rec.calls[-1] == ("extract_map", g.h.value, [2, 3], L.EKF_FRAME_MAP, d2.h.value) and d2.N == 2
    n, nmade = len(rec.calls), len(made)
    for bad in ("world", "MAP", 0, None, b"map"):            # the refusal of a bad frame, in marshal, before anything is sent
        with pytest.raises(ValueError) as info:
            g.extract_map([1], bad)
        assert "frame is 'map' or 'robot'" in str(info.value)
    with pytest.raises(TypeError):
        g.extract_map([1], into="not an engine")
    with pytest.raises(TypeError):
        g.extract_map([1], into=d2, tile=16)
    assert len(rec.calls) == n and len(rec.created) == ncreated and len(made) == nmade + 7
    # a refused call raises; the destination it made for the call is closed again
    rec.fail = L.EKF_ERR_INDEX
    with pytest.raises(L.EkfError) as info:
        g.extract_map([50])
    assert info.value.status == L.EKF_ERR_INDEX and "extract_map" in str(info.value)
    assert len(rec.created) == ncreated + 1 and rec.destroyed[-1] == 0x1000 * rec.handles
    # a shard group hands the call to the library, whose refusal it is
    rec.fail = L.EKF_ERR_INVALID_ARG
    grp = ShardGroup(2, capacity=16)
    with pytest.raises(L.EkfError) as info:
        grp.extract_map([0], "map", d2)
    assert info.value.status == L.EKF_ERR_INVALID_ARG and rec.calls[-1][0] == "extract_map" and rec.calls[-1][1] == grp.shards[0].h.value
    rec.fail = 0
    for cls in (S.EKF_SLAM, S.EKF_SLAM_UC):
        rec.calls.clear()
        del made[:]
        f = cls(capacity=32, tile=64)
        rec.set_count(f._e, 4)
        f.log = TrajectoryLog()
        sub = f.extract_map([3, 1], "robot", tile=16)        # 1-based numbers in, 0-based on the wire
        assert type(sub) is cls and sub._e is not f._e and sub.log is None and sub._e.N == 2
        assert rec.calls == [("extract_map", f._e.h.value, [2, 0], L.EKF_FRAME_ROBOT, sub._e.h.value)] and len(made) == 1
        assert made[0][0] == [2, 0] and rec.created[-1]["tile"] == 16 and rec.created[-1]["mode"] == f._e.cfg.mode
        assert (cls is S.EKF_SLAM_UC) == hasattr(sub, "correspondence")
        assert f.extract_map(2)._e.N == 1 and rec.calls[-1][2] == [1]            # a number is a list of one
        with pytest.raises(ValueError):
            f.extract_map([1.5])
        with pytest.raises(ValueError):
            f.extract_map([1], "body")
        assert f.log.edits == []                              # an extraction changes nothing here: nothing is logged
        # the neighbourhood, from one read of x
        rec.calls.clear()
        assert f.landmarks_near_robot(2.5) == [1, 3] and f.landmarks_near_robot(0.1) == [] and f.landmarks_near_robot(100) == [1, 2, 3, 4]
        assert [c[0] for c in rec.calls] == ["get_x"] * 3
        # the policy: extract, then remove; the log holds the removal alone
        rec.calls.clear()
        del made[:]
        arch = f.split_submap([4, 2], tile=16)
        assert type(arch) is cls and arch._e.N == 2 and f._e.N == 2
        assert rec.calls == [("extract_map", f._e.h.value, [3, 1], L.EKF_FRAME_MAP, arch._e.h.value), ("remove", f._e.h.value, [3, 1])]
        assert len(made) == 1
        assert [(kind, [int(i) for i in idx]) for _, kind, idx, _, _ in f.log.edits] == [("remove", [4, 2])]
        # a refused extraction raises before anything is removed or logged
        rec.fail = L.EKF_ERR_CAPACITY
        with pytest.raises(L.EkfError):
            f.split_submap([1])
        assert [c[0] for c in rec.calls] == ["extract_map", "remove", "extract_map"] and len(f.log.edits) == 1
        rec.fail = 0


def test_the_trajectory_formats_are_left_alone(tmp_path):
    """An extraction changes nothing in the source, so there is no log kind and no format for it: the ten golden logs and a format-11 log
    built here come out byte for byte."""
    from ekf_slam_amd import trajectory as T
    assert len(T._ALL_FORMATS) == 11 and T._ALL_FORMATS[-1] == T.FORMAT_JOIN_MAP == "ekfslam-trajectory-11"
    assert not [name for name in dir(T) if "extract" in name.lower()]
    assert "extract" not in open(T.__file__).read().lower()
    golden = os.path.join(ROOT, "tests", "golden", "trajectory")
    for n in range(1, 11):
        src = os.path.join(golden, "format%d.npz" % n)
        T.TrajectoryLog.load(src).save(tmp_path / ("again%d.npz" % n))
        assert same_npz(src, tmp_path / ("again%d.npz" % n)), n
    log = T.TrajectoryLog()
    log.record([0.1, 1.0], None, [], np.zeros((0, 2)))
    log.record_edit("remove", [2])
    log.record_map_join(np.arange(7.0), [5.0, 6.0], np.eye(7), 3.0)
    log.save(tmp_path / "eleven.npz")
    assert str(np.load(tmp_path / "eleven.npz")["format"]) == T.FORMAT_JOIN_MAP
    T.TrajectoryLog.load(tmp_path / "eleven.npz").save(tmp_path / "eleven_again.npz")
    assert same_npz(tmp_path / "eleven.npz", tmp_path / "eleven_again.npz")


# ------------------------------------------------------------------------------------------------------------------
# the MEX gateway
# ------------------------------------------------------------------------------------------------------------------
_STUB = r'''
#include <stdio.h>
#include "ekfslam.h"
void stub_fail_next(ekf_handle *h);
static int fail_armed;
void arm_failure(void) { fail_armed = 1; }
int32_t ekf_extract_map(ekf_handle *h, const int64_t *idx, int64_t m, int32_t frame, ekf_handle *dst) {
    printf("ABI ekf_extract_map distinct=%d dst=%d m=%d frame=%d idx=", h != dst, dst != 0, (int)m, (int)frame);
    for (int64_t k = 0; k < m; ++k) printf(k ? ",%d" : "%d", (int)idx[k]);
    printf("\n");
    if (fail_armed) { fail_armed = 0; stub_fail_next(h); return ekf_flush(h); }
    return EKF_OK;
}
'''

_DRIVER = driver(r'''
    const mxArray *cr2[3] = { mock_string("create"), D1(1), D1(16) };
    if (call("create dst", 1, 3, cr2)) return 1;
    const mxArray *hd = out[0];
    const mxArray *em[5] = { mock_string("extract_map"), h, mock_double(3, 1, (const double[]){ 5, 1, 3 }), D1(1), hd };
    if (call("extract_map", 0, 5, em)) return 1;
    const mxArray *e0[5] = { em[0], h, mock_double(0, 1, (const double[]){ 0 }), D1(0), hd };
    if (call("extract_map none", 0, 5, e0)) return 1;
    if (!call("extract_map", 0, 4, em)) return 1;
    const mxArray *bad[5] = { em[0], h, em[2], D1(2), hd };
    if (!call("extract_map badframe", 0, 5, bad)) return 1;
    bad[3] = D1(0); bad[4] = D1(3);
    if (!call("extract_map nodst", 0, 5, bad)) return 1;
    bad[4] = hd; bad[1] = D1(1);
    if (!call("extract_map noh", 0, 5, bad)) return 1;
    arm_failure();
    if (!call("extract_map", 0, 5, em)) return 1;
    const mxArray *de2[2] = { mock_string("destroy"), hd };
    if (call("destroy dst", 0, 2, de2)) return 1;
''', PRELUDE_SHOWN)

_DRIVER_WITHOUT = driver_without(r'''
    const mxArray *em[5] = { mock_string("extract_map"), h, D1(1), D1(0), h };
    if (!call("extract_map", 0, 5, em)) return 1;
''')


def test_mex_gateway_reaches_the_abi_with_zero_based_indices(tmp_path):
    t = transcript_of(tmp_path, _STUB, _DRIVER)
    i = t.index("ABI ekf_extract_map distinct=1 dst=1 m=3 frame=1 idx=4,0,2")
    assert t[i + 1].startswith("MEX extract_map nrhs=5 -> ok")
    assert "ABI ekf_extract_map distinct=1 dst=1 m=0 frame=0 idx=" in t
    assert any(ln.startswith("MEX extract_map nrhs=4 -> ERROR ekfslam:usage") and "needs 5 arguments" in ln for ln in t)
    assert any(ln.startswith("MEX extract_map badframe nrhs=5 -> ERROR ekfslam:usage") and "frame is 0 (map) or 1 (robot)" in ln for ln in t)
    assert any(ln.startswith("MEX extract_map nodst nrhs=5 -> ERROR ekfslam:handle") and "destination" in ln for ln in t)
    assert any(ln.startswith("MEX extract_map noh nrhs=5 -> ERROR ekfslam:handle") for ln in t)
    assert sum(ln.startswith("ABI ekf_extract_map") for ln in t) == 3          # the two good calls and the injected failure
    assert "MEX extract_map nrhs=5 -> ERROR ekfslam:status | call not valid in the current state: injected failure" in t
    assert t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_the_gateway_still_links_against_a_library_without_the_symbol(tmp_path):
    t = transcript_of(tmp_path, _DRIVER_WITHOUT)
    assert any(ln.startswith("MEX extract_map ") and "ERROR ekfslam:usage" in ln and "this libekfslam has no ekf_extract_map" in ln for ln in t)
    assert "MEX predict nrhs=3 -> ok" in t and t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_matlab_method_forwards_to_the_gateway_command():
    text = open(os.path.join(ROOT, "matlab", "EKF_SLAM.m")).read()
    m = re.search(r"function\s+extractMap\(h,\s*idx,\s*frame,\s*dst\)(.*?)\n        end\b", text, re.S)
    assert m and "h.gateway('extract_map', double(idx(:)), f, dst.hnd);" in m.group(1)
    src = open(os.path.join(ROOT, "matlab", "ekfslam_mex.c")).read()
    assert 'strcmp(cmd, "extract_map")' in src and "#pragma weak ekf_extract_map" in src
    assert "extractMap" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
