"""CPU: ekf_join_map without a GPU -- the NumPy restatement of tests/join_map_cases.py against a finite-difference Jacobian of the
composite map; k_join_state and k_join_rows compiled for the host on a global and a local state (all four storage pairs) against that
restatement; the Python layers over a stand-in for the library (one marshal per call, the `join_map` log entry, format 11, older logs
written as before); the MEX gateway's command under the MEX mock."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import join_map_cases as J
from helpers import REL, ROOT, TOL_KEPT32, TOL_ROW32, TOL_X32, RecorderBase, host_build, rel_err, same_npz
from mex_harness import PRELUDE_SHOWN, driver, driver_without, transcript_of

CASES = [(0, 3), (5, 1), (8, 8), (13, 21)]


# ------------------------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,M", CASES + [(4, 0)])
def test_the_restatement_agrees_with_a_finite_difference_jacobian(N, M):
    rng = np.random.default_rng(100 + 7 * N + M)
    x, s, P = J.random_state(rng, N)
    y, sL, PL = J.random_state(rng, M, pose=[0.7, -0.4, 12.0])
    Jm = J.join_jacobian(x, y)
    v = np.concatenate([x, y])
    fd = np.zeros_like(Jm)
    h = 1e-6
    for k in range(v.size):                                   # central differences of the unwrapped map (the wrap is piecewise constant)
        up, dn = v.copy(), v.copy()
        up[k] += h
        dn[k] -= h
        fd[:, k] = (J.join_fn(up[:x.size], up[x.size:], wrap=False) - J.join_fn(dn[:x.size], dn[x.size:], wrap=False)) / (2 * h)
    err = np.abs(fd - Jm).max() / np.abs(Jm).max()
    print("N=%d M=%d: finite differences (step 1e-6) against J: worst rel err %.2e" % (N, M, err))
    assert err < 1e-7
    xn, sn, Pn = J.join_dense(x, s, P, y, sL, PL, 500.0)
    B = np.zeros((v.size, v.size))
    B[:x.size, :x.size] = P
    B[x.size:, x.size:] = PL
    assert rel_err(Pn, fd @ B @ fd.T) < 1e-7
    # the table of the issue, block by block
    n, k = x.size, J.K
    Rm = J.rot(x[2])
    w = Rm @ y[0:2]
    J1 = np.array([[1.0, 0.0, -w[1] / k], [0.0, 1.0, w[0] / k], [0.0, 0.0, 1.0]])
    J2 = np.eye(3)
    J2[:2, :2] = Rm
    Gx = []
    for i in range(M):
        wi = Rm @ y[3 + 2 * i:5 + 2 * i]
        Gx.append(np.array([[1.0, 0.0, -wi[1] / k], [0.0, 1.0, wi[0] / k]]))
    tol = 1e-13 * np.abs(Pn).max()
    assert np.abs(Pn[:3, :3] - (J1 @ P[:3, :3] @ J1.T + J2 @ PL[:3, :3] @ J2.T)).max() < tol
    assert np.abs(Pn[:3, 3:n] - J1 @ P[:3, 3:n]).max(initial=0.0) < tol
    np.testing.assert_array_equal(Pn[3:n, 3:n], 0.5 * (P[3:n, 3:n] + P[3:n, 3:n].T))
    for i in range(M):
        r = n + 2 * i
        assert np.abs(Pn[:3, r:r + 2] - (J1 @ P[:3, :3] @ Gx[i].T + J2 @ PL[:3, 3 + 2 * i:5 + 2 * i] @ Rm.T)).max() < tol
        assert np.abs(Pn[r:r + 2, 3:n] - Gx[i] @ P[:3, 3:n]).max(initial=0.0) < tol
        for a in range(i + 1):
            c = n + 2 * a
            assert np.abs(Pn[r:r + 2, c:c + 2] - (Gx[i] @ P[:3, :3] @ Gx[a].T + Rm @ PL[3 + 2 * i:5 + 2 * i, 3 + 2 * a:5 + 2 * a] @ Rm.T)).max() < tol
    np.testing.assert_array_equal(sn, np.concatenate([s, sL + 500.0]))
    np.testing.assert_array_equal(xn[3:n], x[3:n])
    assert xn[2] == J.wrap360(x[2] + y[2]) and 0.0 <= xn[2] <= 360.0


# ------------------------------------------------------------------------------------------------------------------
# both kernels compiled for the host
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emulation(tmp_path_factory):
    d = tmp_path_factory.mktemp("join_map_emulation")
    exe = host_build("join_map_host_emulation", str(d / "emu"))
    r = subprocess.run([exe, str(d)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    return d, r.stdout


def _read(path):
    v = np.fromfile(path)
    N, M, offset = int(v[0]), int(v[1]), v[2]
    pos = [3]

    def take(count, shape=None):
        out = v[pos[0]:pos[0] + count]
        pos[0] += count
        return out.reshape(shape) if shape else out
    n, nl, nn = 3 + 2 * N, 3 + 2 * M, 3 + 2 * (N + M)
    x, s, P = take(n), take(N), take(n * n, (n, n))
    y, sL, PL = take(nl), take(M), take(nl * nl, (nl, nl))
    xn, sn, Pn = take(nn), take(N + M), take(nn * nn, (nn, nn))
    assert pos[0] == v.size
    return (x, s, P), (y, sL, PL), offset, (xn, sn, Pn)


@pytest.mark.parametrize("pair", ["dd", "df", "fd", "ff"])
def test_host_emulation_of_both_kernels_against_the_restatement(emulation, pair):
    d, out = emulation
    for N, M in CASES:
        assert "%s N=%d M=%d: 0 differences" % (pair, N, M) in out
        (x, s, P), (y, sL, PL), offset, (xn, sn, Pn) = _read(os.path.join(str(d), "%s_%d_%d.bin" % (pair, N, M)))
        ex, es, eP = J.join_dense(x, s, P, y, sL, PL, offset)
        np.testing.assert_array_equal(sn, es)
        np.testing.assert_array_equal(Pn, Pn.T)
        np.testing.assert_array_equal(Pn[3:3 + 2 * N, 3:3 + 2 * N], P[3:, 3:])             # P(old, old): the same bits
        np.testing.assert_array_equal(xn[3:3 + 2 * N], x[3:])
        n = ex.size
        kept = np.zeros((n, n), dtype=bool)
        kept[:3, :] = kept[:, :3] = True
        for a in range(3, n, 2):
            kept[a:a + 2, a:a + 2] = True
        err_x, err_P = rel_err(xn, ex), rel_err(Pn, eP)
        err_kept = float(np.abs(Pn - eP)[kept].max() / np.abs(eP).max())
        err_row = float((np.abs(Pn - eP).max(axis=1) / np.abs(eP).max(axis=1)).max())
        print("%s N=%d M=%d: rel err x %.2e P %.2e F64-kept %.2e worst row %.2e" % (pair, N, M, err_x, err_P, err_kept, err_row))
        if pair[0] == "d":                                    # F64 destination tiles: the local tiles' values are exact doubles either way
            assert err_x < REL and err_P < REL
        else:                                                 # float destination tiles: DESIGN.md section 5
            assert err_x < TOL_X32 and err_kept < TOL_KEPT32 and err_row <= TOL_ROW32


def test_kernel_sources_on_the_host_under_the_sanitizers(tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined runs clean: no lane of either kernel reads or writes outside
    the buffers of the two states (nothing loaded into python is involved)."""
    exe = host_build("join_map_host_emulation", str(tmp_path / "emulation_sanitized"),
                     flags=["-O1", "-g", "-mfma", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]


# ------------------------------------------------------------------------------------------------------------------
# the Python layers over a stand-in for the library
# ------------------------------------------------------------------------------------------------------------------
class _Recorder(RecorderBase):
    status_string = b"landmark capacity exhausted"
    last_error = b"join_map: injected"

    def __init__(self):
        self.calls, self.fail, self.N, self.handles = [], 0, {}, 0

    def ekf_create(self, pcfg, ph):
        self.handles += 1
        ctypes.cast(ph, ctypes.POINTER(ctypes.c_void_p)).contents.value = 0x1000 * self.handles
        return 0

    def set_count(self, e, N):
        self.N[e.h.value] = N

    def ekf_num_landmarks(self, h, pn):
        pn._obj.value = self.N.get(h.value, 0)
        return 0

    def ekf_join_map(self, h, local, offset, pfirst):
        assert isinstance(offset, ctypes.c_double)            # marshalled once, by marshal.join_offset
        self.calls.append(("join_map", h.value, local.value, offset.value))
        if self.fail:
            return self.fail
        pfirst._obj.value = self.N.get(h.value, 0)
        self.N[h.value] = self.N.get(h.value, 0) + self.N.get(local.value, 0)
        return 0

    def _get(self, h, p, count, value):
        self.calls.append(("get", h.value))
        for k in range(count):
            p[k] = value + k
        return 0

    def ekf_get_x(self, h, p):
        return self._get(h, p, 3 + 2 * self.N.get(h.value, 0), 10.0)

    def ekf_get_s(self, h, p):
        return self._get(h, p, self.N.get(h.value, 0), 20.0)

    def ekf_get_P(self, h, p):
        n = 3 + 2 * self.N.get(h.value, 0)
        return self._get(h, p, n * n, 30.0)


def test_layers_marshal_a_join_once_and_log_it(monkeypatch, tmp_path):
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import engine as E
    from ekf_slam_amd import marshal
    from ekf_slam_amd import slam as S
    from ekf_slam_amd.sharding import ShardGroup
    from ekf_slam_amd.trajectory import FORMAT_JOIN_MAP, JOIN_MAP, TrajectoryLog
    assert L.SIGNATURES["ekf_join_map"] == (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.POINTER(ctypes.c_int64)])
    assert FORMAT_JOIN_MAP == "ekfslam-trajectory-11"
    rec = _Recorder()
    monkeypatch.setattr(L, "lib", lambda: rec)
    made = []
    real = marshal.join_offset
    monkeypatch.setattr(marshal, "join_offset", lambda *a, **k: made.append(a) or real(*a, **k))
    g, lo = E.Engine(capacity=32), E.Engine(capacity=8)
    rec.set_count(g, 7)
    rec.set_count(lo, 2)
    assert g.join_map(lo, 100.0) == 7 and g.N == 9
    assert rec.calls == [("join_map", g.h.value, lo.h.value, 100.0)] and len(made) == 1
    assert g.join_map(lo) == 9 and rec.calls[-1][3] == 0.0 and len(made) == 2
    n = len(rec.calls)
    with pytest.raises(TypeError):
        g.join_map("not an engine")
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            g.join_map(lo, bad)
    assert len(rec.calls) == n
    # a shard group hands the call to the library, whose refusal it is
    rec.fail = L.EKF_ERR_INVALID_ARG
    grp = ShardGroup(2, capacity=16)
    with pytest.raises(L.EkfError) as info:
        grp.join_map(lo)
    assert info.value.status == L.EKF_ERR_INVALID_ARG and rec.calls[-1][0] == "join_map"
    rec.fail = 0
    for cls in (S.EKF_SLAM, S.EKF_SLAM_UC):
        rec.calls.clear()
        del made[:]
        f, sub = cls(capacity=32), cls(capacity=8)
        rec.set_count(f._e, 5)
        rec.set_count(sub._e, 3)
        f.log = TrajectoryLog()
        assert f.join_map(sub, signature_offset=40.0) == [6, 7, 8]          # 1-based numbers
        assert len(made) == 1 and [c for c in rec.calls if c[0] == "join_map"] == [("join_map", f._e.h.value, sub._e.h.value, 40.0)]
        # the local state is read once, after the call
        assert [c[0] for c in rec.calls] == ["join_map", "get", "get", "get"] and all(c[1] == sub._e.h.value for c in rec.calls[1:])
        assert [(k, kind, idx.tolist()) for k, kind, idx, _, _ in f.log.edits] == [(0, JOIN_MAP, [])]
        p = f.log.map_joins[0]
        assert p["offset"] == 40.0 and p["x"].tolist() == [10.0 + k for k in range(9)] and p["s"].tolist() == [20.0, 21.0, 22.0]
        assert p["P"].shape == (9, 9) and p["P"][0, 1] == 9.0 + 30.0       # get_P arrives column-major
        with pytest.raises(TypeError):                        # anything else is refused here, as the Engine layer refuses it
            f.join_map("not a filter")
        assert len(f.log.edits) == 1
        # the policy without a gate is the join alone; an Engine serves as the local map too
        new, fused = f.join_submap(sub._e, signature_offset=1.0)
        assert new == [9, 10, 11] and fused == [] and len(f.log.edits) == 2
        # a refused call raises and is not logged
        rec.fail = L.EKF_ERR_CAPACITY
        with pytest.raises(L.EkfError) as info:
            f.join_map(sub)
        assert info.value.status == L.EKF_ERR_CAPACITY and "join_map" in str(info.value) and len(f.log.edits) == 2
        rec.fail = 0
        # format 11: saved, loaded, saved again
        f.log.record([0.1, 1.0], None, [], np.zeros((0, 2)))
        f.log.save(tmp_path / "eleven.npz")
        g11 = np.load(tmp_path / "eleven.npz")
        assert str(g11["format"]) == FORMAT_JOIN_MAP
        for name in ("join_edit", "join_x_ptr", "join_x", "join_s_ptr", "join_s", "join_P_ptr", "join_P", "join_offset"):
            assert name in g11.files
        assert "join_offset_ptr" not in g11.files                             # one number per join: no offsets of its own
        assert g11["join_x_ptr"].tolist() == [0, 9, 18] and g11["join_P_ptr"].tolist() == [0, 81, 162] and g11["join_offset"].tolist() == [40.0, 1.0]
        back = TrajectoryLog.load(tmp_path / "eleven.npz")
        assert sorted(back.map_joins) == [0, 1]
        for q in (0, 1):
            for key in ("x", "s", "P"):
                np.testing.assert_array_equal(back.map_joins[q][key], f.log.map_joins[q][key])
            assert back.map_joins[q]["offset"] == f.log.map_joins[q]["offset"]
        back.save(tmp_path / "eleven_again.npz")
        assert same_npz(tmp_path / "eleven.npz", tmp_path / "eleven_again.npz")
    bad = TrajectoryLog()
    for args in ((np.zeros(4), np.zeros(0), np.zeros((4, 4))), (np.zeros(5), np.zeros(2), np.zeros((5, 5))), (np.zeros(5), np.zeros(1), np.zeros((4, 4)))):
        with pytest.raises(ValueError):
            bad.record_map_join(*args)
    assert bad.edits == [] and bad.map_joins == {}


def test_a_replay_joins_from_a_scratch_engine(monkeypatch):
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import engine as E
    from ekf_slam_amd.trajectory import TrajectoryLog
    rec = _Recorder()
    sets = []
    for name in ("ekf_set_x", "ekf_set_s", "ekf_set_P"):
        setattr(rec, name, (lambda nm: lambda h, p, n: sets.append((nm, h.value, int(n))) or 0)(name))
    rec.ekf_predict = lambda h, u: rec.calls.append(("predict",)) or 0
    rec.ekf_remove_landmarks = lambda h, idx, m: rec.calls.append(("remove", [idx[k] for k in range(m)])) or 0
    monkeypatch.setattr(L, "lib", lambda: rec)
    destroyed = []
    rec.ekf_destroy = lambda h: destroyed.append(h.value if hasattr(h, "value") else h) or 0
    log = TrajectoryLog()
    log.record([0.1, 1.0], None, [], np.zeros((0, 2)))
    log.record_edit("remove", [2])
    log.record_map_join(np.arange(7.0), [5.0, 6.0], np.eye(7), 3.0)
    target = E.Engine(capacity=16)
    log.replay(target)
    # (the edits recorded after the last step are applied at the end: the removal, then the join from a scratch engine that is closed again)
    assert [c[0] for c in rec.calls] == ["predict", "remove", "join_map"] and rec.calls[1] == ("remove", [1])
    joins = [c for c in rec.calls if c[0] == "join_map"]
    assert len(joins) == 1 and joins[0][1] == target.h.value and joins[0][2] != target.h.value and joins[0][3] == 3.0
    assert [(nm, n) for nm, h, n in sets if h == joins[0][2]] == [("ekf_set_x", 7), ("ekf_set_s", 2), ("ekf_set_P", 7)]
    assert joins[0][2] in destroyed


def test_logs_without_a_join_are_written_as_before(tmp_path):
    from ekf_slam_amd.trajectory import _ALL_FORMATS, TrajectoryLog
    golden = os.path.join(ROOT, "tests", "golden", "trajectory")
    assert len(_ALL_FORMATS) == 11
    for n in range(1, 11):
        src = os.path.join(golden, "format%d.npz" % n)
        log = TrajectoryLog.load(src)
        assert log.map_joins == {}
        log.save(tmp_path / ("again%d.npz" % n))
        assert same_npz(src, tmp_path / ("again%d.npz" % n)), n
        assert not any(name.startswith("join_") for name in np.load(src).files)


# ------------------------------------------------------------------------------------------------------------------
# the MEX gateway
# ------------------------------------------------------------------------------------------------------------------
_STUB = r'''
#include <stdio.h>
#include "ekfslam.h"
void stub_fail_next(ekf_handle *h);
static int fail_armed;
void arm_failure(void) { fail_armed = 1; }
int32_t ekf_join_map(ekf_handle *h, ekf_handle *local, double offset, int64_t *first) {
    int64_t N = 0;
    ekf_num_landmarks(h, &N);
    printf("ABI ekf_join_map distinct=%d local=%d offset=%g first=%d\n", h != local, local != 0, offset, first != 0);
    if (fail_armed) { fail_armed = 0; stub_fail_next(h); return ekf_flush(h); }
    if (first) *first = N;
    return EKF_OK;
}
'''

_DRIVER = driver(r'''
    const mxArray *cr2[3] = { mock_string("create"), D1(1), D1(16) };
    if (call("create local", 1, 3, cr2)) return 1;
    const mxArray *hl = out[0];
    const mxArray *jm[4] = { mock_string("join_map"), h, hl, D1(250) };
    if (call("join_map", 1, 4, jm)) return 1;
    if (!call("join_map", 1, 3, jm)) return 1;
    const mxArray *bad[4] = { jm[0], h, D1(3), D1(0) };
    if (!call("join_map nolocal", 1, 4, bad)) return 1;
    bad[2] = hl; bad[3] = mock_double(2, 1, (const double[]){ 1, 2 });
    if (!call("join_map badoffset", 1, 4, bad)) return 1;
    bad[3] = D1(0); bad[1] = D1(1);
    if (!call("join_map noh", 1, 4, bad)) return 1;
    arm_failure();
    if (!call("join_map", 1, 4, jm)) return 1;
    const mxArray *de2[2] = { mock_string("destroy"), hl };
    if (call("destroy local", 0, 2, de2)) return 1;
''', PRELUDE_SHOWN)

_DRIVER_WITHOUT = driver_without(r'''
    const mxArray *jm[4] = { mock_string("join_map"), h, h, D1(0) };
    if (!call("join_map", 1, 4, jm)) return 1;
''')


def test_mex_gateway_reaches_the_abi_with_both_handles(tmp_path):
    t = transcript_of(tmp_path, _STUB, _DRIVER)
    i = t.index("ABI ekf_join_map distinct=1 local=1 offset=250 first=1")
    assert t[i + 1].startswith("MEX join_map nrhs=4 -> ok out0=0x1[")      # the stand-in's map does not grow: no new numbers
    assert any(ln.startswith("MEX join_map nrhs=3 -> ERROR ekfslam:usage") and "needs 4 arguments" in ln for ln in t)
    assert any(ln.startswith("MEX join_map nolocal nrhs=4 -> ERROR ekfslam:handle") and "local map" in ln for ln in t)
    assert any(ln.startswith("MEX join_map badoffset nrhs=4 -> ERROR ekfslam:usage") and "signature_offset is one number" in ln for ln in t)
    assert any(ln.startswith("MEX join_map noh nrhs=4 -> ERROR ekfslam:handle") for ln in t)
    assert sum(ln.startswith("ABI ekf_join_map") for ln in t) == 2             # the good call and the injected failure
    assert "MEX join_map nrhs=4 -> ERROR ekfslam:status | call not valid in the current state: injected failure" in t
    assert t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_the_gateway_still_links_against_a_library_without_the_symbol(tmp_path):
    t = transcript_of(tmp_path, _DRIVER_WITHOUT)
    assert any(ln.startswith("MEX join_map ") and "ERROR ekfslam:usage" in ln and "this libekfslam has no ekf_join_map" in ln for ln in t)
    assert "MEX predict nrhs=3 -> ok" in t and t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_matlab_method_forwards_to_the_gateway_command():
    text = open(os.path.join(ROOT, "matlab", "EKF_SLAM.m")).read()
    m = re.search(r"function\s+idx\s*=\s*joinMap\(h,\s*local,\s*signatureOffset\)(.*?)\n        end\b", text, re.S)
    assert m and "h.gateway('join_map', local.hnd," in m.group(1)
    src = open(os.path.join(ROOT, "matlab", "ekfslam_mex.c")).read()
    assert 'strcmp(cmd, "join_map")' in src and "#pragma weak ekf_join_map" in src
