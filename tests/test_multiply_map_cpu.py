"""CPU: ekf_multiply_map without a GPU -- the kernels of ekf_slam_amd/csrc/multiply_map.h compiled for the host (tile edges 16, 64, 128
with F64 tiles and 256 with float tiles, the matrix-core loops as their plain-FMA twins in the same k order) against NumPy within the
derived bar, and bit for bit where the header promises bits; the Python layers over a stand-in for the library (one marshal per call,
the refusals before any call, the three policies against NumPy); the MEX gateway's command under the MEX mock.

THE BAR (multiply_map_cases): |got - P b|_i <= 2 n 2^-53 (|P| |b|)_i entry by entry, P the matrix as the handle holds it
(sample_map_cases.as_held for float tiles); bar_ratio is the worst quotient, printed before it is asserted to be at most 1.

THE EMULATED STORE is hostile on purpose (tests/support/multiply_map_host_emulation.cpp): every row and column below the map is NaN, in
the tiles and in the strip; the tile entries of the landmarks' own 2 x 2 blocks hold a wrong value, so that only the diag copies give
the right answer; the upper triangle of every diagonal tile holds garbage, so that only the canonical lower triangle does."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import factor_map_cases as F
import multiply_map_cases as M
import sample_map_cases as S
from helpers import ROOT, RecorderBase, host_build
from mex_harness import PRELUDE_SHOWN, driver, driver_without, transcript_of

dp = ctypes.POINTER(ctypes.c_double)
PTHREAD = ["-O2", "-mfma", "-ffp-contract=off", "-pthread"]
# (tile edge, float tiles, landmarks): N = 140 leaves the last tile row partial at edges 64, 128 and 256 and gives edge 16 eighteen tile
# rows, the last two of two segments; N = 96 at edge 64 ends exactly on a tile edge; N = 1 is one partial tile
STORES = [(16, 0, 140), (64, 0, 140), (128, 0, 140), (256, 1, 140), (64, 0, 96), (16, 0, 1), (256, 1, 1)]
NBATCH = 3 * M.CHUNK + 5


def _name(T, fl, N, what):
    return "%s_T%d_%s_N%d" % (what, T, "f" if fl else "d", N)


def _scenes():
    """name -> (T, float, N, P as held, B).  Per store: "all" (the batch of 3 * 16 + 5 rows with its repeats and its zero row, then the
    unit vectors of 19 spread indices), "alone" (row 0 by itself) and "part" (rows 10 .. 29: other positions, another chunking)."""
    out = {}
    for T, fl, N in STORES:
        x, s, P = F.spd_scene(N, 100 + N)
        H = S.as_held(P, fl)
        n = x.size
        batch = M.batch_rows(n)
        out[_name(T, fl, N, "all")] = (T, fl, N, H, np.vstack([batch, np.eye(n)[M.spread_units(n)]]))
        out[_name(T, fl, N, "alone")] = (T, fl, N, H, batch[:1])
        out[_name(T, fl, N, "part")] = (T, fl, N, H, batch[10:30])
    x, s, P = F.spd_scene(0, 100)
    out["none"] = (16, 0, 0, P, np.vstack([np.eye(3), M.gaussian_rows(2, 3, 4)]))
    return out


def _write_cases(d, scenes, names=None):
    with open(os.path.join(str(d), "cases.txt"), "w") as f:
        for name, (T, fl, N, H, B) in scenes.items():
            if names is not None and name not in names:
                continue
            f.write("%s %d %d %d %d\n" % (name, T, fl, N, B.shape[0]))
            np.concatenate([H.reshape(-1, order="F"), B.reshape(-1)]).tofile(os.path.join(str(d), name + ".in"))


def _run_split(exe, d, parts=4):
    """The cases of d/cases.txt dealt out to `parts` processes that run side by side; their outputs joined."""
    lines = open(os.path.join(str(d), "cases.txt")).read().splitlines()
    procs = []
    for p in range(parts):
        with open(os.path.join(str(d), "cases_%d.txt" % p), "w") as f:
            f.write("".join(ln + "\n" for ln in lines[p::parts]))
        procs.append(subprocess.Popen([exe, str(d), "cases_%d.txt" % p], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    out = ""
    for pr in procs:
        so, se = pr.communicate()
        assert pr.returncode == 0, so[-3000:] + se[-2000:]
        out += so
    return out


def _output(d, name, scenes):
    B = scenes[name][4]
    return np.fromfile(os.path.join(str(d), name + ".out")).reshape(B.shape)


@pytest.fixture(scope="module")
def emulation(tmp_path_factory):
    d = tmp_path_factory.mktemp("multiply_map_emulation")
    scenes = _scenes()
    _write_cases(d, scenes)
    exe = host_build("multiply_map_host_emulation", str(d / "emu"), flags=PTHREAD)
    out = _run_split(exe, d)
    print(out)
    return d, out, scenes


# ------------------------------------------------------------------------------------------------------------------
# the kernels compiled for the host
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,fl,N", STORES)
def test_host_emulation_of_the_kernels_within_the_bar(emulation, T, fl, N):
    """Gaussian rows and unit vectors against NumPy on the symmetric matrix as the handle holds it -- which the product equals only
    if the rows below the map, the own blocks' tile entries and the upper triangles of the diagonal tiles were never read; the result
    chunk (packed poisoned) written in its live entries alone, nothing of the state written."""
    d, out, scenes = emulation
    for what in ("all", "alone", "part"):
        name = _name(T, fl, N, what)
        assert "%s: 0 differences" % name in out
        _, _, _, H, B = scenes[name]
        ratio = M.bar_ratio(H, B, _output(d, name, scenes))
        print("%s: worst |got - P b| / (2 n u |P||b|) = %.3f" % (name, ratio))
        assert ratio <= 1.0, (name, ratio)


@pytest.mark.parametrize("T,fl,N", STORES)
def test_host_emulation_keeps_the_promised_bits(emulation, T, fl, N):
    """(1) a vector gives the same bits alone, behind a chunk boundary, first in a chunk, last of a partial chunk and in another
    batch; (2) the zero row gives 0 in every entry; (3) a unit vector returns its column of P entry for entry."""
    d, out, scenes = emulation
    H = scenes[_name(T, fl, N, "all")][3]
    got = _output(d, _name(T, fl, N, "all"), scenes)
    batch, units = got[:NBATCH], got[NBATCH:]
    alone = _output(d, _name(T, fl, N, "alone"), scenes)[0]
    assert alone.any()
    for i in M.REPEATS:
        np.testing.assert_array_equal(batch[i], alone)
    assert not batch[2].any() and not np.array_equal(batch[1], alone)
    np.testing.assert_array_equal(_output(d, _name(T, fl, N, "part"), scenes), batch[10:30])
    idx = M.spread_units(H.shape[0])
    assert units.shape[0] == idx.size == min(19, H.shape[0])
    np.testing.assert_array_equal(units, H[:, idx].T)


def test_host_emulation_of_an_empty_map(emulation):
    """N = 0: out = Prr b from k_multiply_robot alone."""
    d, out, scenes = emulation
    assert "none: 0 differences" in out
    _, _, _, P, B = scenes["none"]
    got = _output(d, "none", scenes)
    np.testing.assert_array_equal(got[:3], P)
    assert M.bar_ratio(P, B, got) <= 1.0


def test_kernel_sources_on_the_host_under_the_sanitizers(tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined runs clean per tile edge and storage kind: no lane of the
    new kernels reads or writes outside the chunks, the partial blocks or the state (nothing loaded into python is involved)."""
    scenes = _scenes()
    names = [_name(16, 0, 140, "part"), _name(64, 0, 96, "part"), _name(128, 0, 140, "alone"), _name(256, 1, 140, "part"), _name(256, 1, 1, "alone"), "none"]
    _write_cases(tmp_path, scenes, names)
    exe = host_build("multiply_map_host_emulation", str(tmp_path / "emulation_sanitized"),
                     flags=["-O1", "-g", "-mfma", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    for name in names:
        assert "%s: 0 differences" % name in r.stdout


def test_the_sources_keep_what_the_header_promises():
    """No atomics in the kernels; one k order, chunk_k of map_blocks.h, named by the twins of both parts of a tile and defined nowhere
    else; the host layer never touches the factor store."""
    src = open(os.path.join(ROOT, "ekf_slam_amd", "csrc", "multiply_map.h")).read()
    code = src.split("// -----")[-1]
    assert "atomic" not in code and code.count("chunk_k(s, t)") == 2 and code.count("#if defined(EKF_FACTOR_FMA_TWIN)") == 2
    assert "multiply_k" not in src and "int chunk_k(" not in src
    assert "int chunk_k(int s, int t) { return 8 * (s >> 1) + 2 * t + (s & 1); }" in open(os.path.join(ROOT, "ekf_slam_amd", "csrc", "map_blocks.h")).read()
    host = open(os.path.join(ROOT, "ekf_slam_amd", "csrc", "host", "multiply_map.h")).read()
    assert "factor_alloc" not in host and "d_ftiles" not in host and "d_fsample" not in host


# ------------------------------------------------------------------------------------------------------------------
# the Python layers over a stand-in for the library
# ------------------------------------------------------------------------------------------------------------------
def _p7():
    A = np.random.default_rng(21).normal(0.0, 0.3, (7, 7))
    return A @ A.T + 0.2 * np.eye(7)


class _Recorder(RecorderBase):
    """ekf_multiply_map as NumPy's product (and ekf_solve_map as NumPy's solve) on a fixed two-landmark Gaussian."""
    status_string = b"invalid argument"
    last_error = b"multiply_map: not built for sharded handles (world > 1): injected"

    def __init__(self):
        self.calls, self.fail, self.N, self.P = [], 0, 2, _p7()

    def ekf_num_landmarks(self, h, pn):
        pn._obj.value = self.N
        return 0

    def ekf_multiply_map(self, h, B, k, out):
        assert isinstance(k, ctypes.c_int64)                                  # marshalled once, by marshal.multiply_args
        n = 3 + 2 * self.N
        rows = np.array([B[i] for i in range(k.value * n)]).reshape(k.value, n)
        self.calls.append(("multiply_map", h.value, rows))
        if self.fail:
            return self.fail
        for i, v in enumerate((rows @ self.P).reshape(-1)):
            out[i] = v
        return 0

    def ekf_solve_map(self, h, form, B, k, out, info):
        n = 3 + 2 * self.N
        rhs = np.array([B[i] for i in range(k.value * n)]).reshape(k.value, n)
        self.calls.append(("solve_map", h.value, rhs))
        info._obj.n, info._obj.definite, info._obj.bad_index = n, 1, -1
        for i, v in enumerate(np.linalg.solve(self.P, rhs.T).T.reshape(-1)):
            out[i] = v
        return 0


def test_layers_marshal_a_product_once(monkeypatch):
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import engine as E
    from ekf_slam_amd import marshal
    from ekf_slam_amd import slam as SL
    from ekf_slam_amd.sharding import ShardGroup
    from ekf_slam_amd.trajectory import TrajectoryLog
    assert L.SIGNATURES["ekf_multiply_map"] == (ctypes.c_int32, [ctypes.c_void_p, dp, ctypes.c_int64, dp])
    header = open(os.path.join(ROOT, "include", "ekfslam.h")).read()
    assert "int32_t ekf_multiply_map(ekf_handle *h, const double *B" in header
    assert "masked by selection" in header and "NO entry is wrapped" in header
    rec = _Recorder()
    monkeypatch.setattr(L, "lib", lambda: rec)
    made = []
    real = marshal.multiply_args
    monkeypatch.setattr(marshal, "multiply_args", lambda *a, **k: made.append(a) or real(*a, **k))
    g = E.Engine(capacity=32, tile=16)
    one = np.arange(7.0) / 7.0
    out = g.multiply_map(one)
    assert len(rec.calls) == 1 and len(made) == 1 and rec.calls[0][1] == g.h.value
    np.testing.assert_array_equal(rec.calls[0][2], one[None, :])
    np.testing.assert_array_equal(out, one[None, :] @ rec.P)
    assert out.shape == (1, 7) and out.dtype == np.float64 and out.flags["C_CONTIGUOUS"]
    five = np.asfortranarray(np.random.default_rng(2).standard_normal((5, 7)).astype(np.float32))      # neither F64 nor C-contiguous
    out = g.multiply_map(five)
    np.testing.assert_array_equal(rec.calls[-1][2], five.astype(np.float64))
    np.testing.assert_array_equal(out, five.astype(np.float64) @ rec.P)
    assert out.shape == (5, 7) and len(made) == 2
    # the refusals, in marshal, before anything is sent
    ncalls = len(rec.calls)
    bad_nan = one.copy()
    bad_nan[4] = np.nan
    for B in (None, np.zeros((0, 7)), np.zeros(6), np.zeros((2, 9)), bad_nan, np.full((2, 7), np.inf), np.zeros((2, 1, 7))):
        with pytest.raises(ValueError) as err:
            g.multiply_map(B)
        assert "multiply_map" in str(err.value)
    assert len(rec.calls) == ncalls
    # the library's refusal raises; a shard group hands the call to its first shard so that the refusal is the library's
    rec.fail = L.EKF_ERR_INVALID_ARG
    with pytest.raises(L.EkfError) as err:
        g.multiply_map(one)
    assert err.value.status == L.EKF_ERR_INVALID_ARG and "multiply_map" in str(err.value)
    grp = ShardGroup(2, capacity=16)
    with pytest.raises(L.EkfError) as err:
        grp.multiply_map(one)
    assert rec.calls[-1][0] == "multiply_map" and rec.calls[-1][1] == grp.shards[0].h.value and "sharded" in str(err.value)
    rec.fail = 0
    # the policy layer: one call each (solve_residual: the solve and one product), nothing logged
    for cls in (SL.EKF_SLAM, SL.EKF_SLAM_UC):
        rec.calls.clear()
        del made[:]
        f = cls(capacity=32, tile=64)
        f.log = TrajectoryLog()
        np.testing.assert_array_equal(f.multiply_map(five), five.astype(np.float64) @ rec.P)
        f.covariance_of(five)
        np.testing.assert_array_equal(rec.calls[-1][2], five.astype(np.float64))
        f.cross_covariance([1], [0, 1])
        np.testing.assert_array_equal(rec.calls[-1][2], np.eye(7)[5:7])                 # the unit vectors of the SHORTER list
        f.cross_covariance(None, [0])
        np.testing.assert_array_equal(rec.calls[-1][2], np.eye(7)[3:5])
        assert len(rec.calls) == 4 and len(made) == 4 and len(f.log.edits) == 0
        f.solve_residual(five)
        assert [c[0] for c in rec.calls[4:]] == ["solve_map", "multiply_map"] and len(f.log.edits) == 0


def test_the_three_policies_against_numpy(monkeypatch):
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import slam as SL
    rec = _Recorder()
    monkeypatch.setattr(L, "lib", lambda: rec)
    P = rec.P
    f = SL.EKF_SLAM(capacity=32, tile=64)
    A = np.random.default_rng(5).standard_normal((3, 7))
    cov = f.covariance_of(A)
    assert cov.shape == (3, 3) and np.abs(cov - A @ P @ A.T).max() <= 64 * M.U * (np.abs(A) @ np.abs(P) @ np.abs(A).T).max()
    np.testing.assert_array_equal(cov, cov.T)
    centroid = np.zeros(7)
    centroid[[3, 5]] = 0.5                                                      # the x coordinate of the two landmarks' centroid
    var = f.covariance_of(centroid)
    assert var.shape == (1, 1) and abs(var[0, 0] - 0.25 * (P[3, 3] + 2 * P[3, 5] + P[5, 5])) <= 64 * M.U * np.abs(P).max()
    for ia, ib, ca, cb in (([1], [0], [5, 6], [3, 4]), ([1, 0], [0], [5, 6, 3, 4], [3, 4]), ([0], [1, 0], [3, 4], [5, 6, 3, 4]),
                           (None, [1], [0, 1, 2], [5, 6]), ([0, 1], None, [3, 4, 5, 6], [0, 1, 2]), (None, None, [0, 1, 2], [0, 1, 2])):
        ncalls = len(rec.calls)
        got = f.cross_covariance(ia, ib)
        np.testing.assert_array_equal(got, P[np.ix_(ca, cb)])
        assert len(rec.calls) == ncalls + 1 and rec.calls[-1][2].shape[0] == min(len(ca), len(cb))
    B = np.random.default_rng(6).standard_normal((4, 7))
    z, r = f.solve_residual(B)
    np.testing.assert_array_equal(z, np.linalg.solve(P, B.T).T)
    np.testing.assert_array_equal(r, z @ P - B)
    assert np.abs(r).max() < 1e-13
    z1, r1 = f.solve_residual(B[0])
    assert z1.shape == (1, 7) and r1.shape == (1, 7)
    # refusals of the policies, before any call
    ncalls = len(rec.calls)
    for call in (lambda: f.covariance_of(np.zeros((2, 6))), lambda: f.covariance_of(np.zeros((0, 7))), lambda: f.covariance_of(np.zeros((1, 2, 7))),
                 lambda: f.cross_covariance([2], [0]), lambda: f.cross_covariance([0, 0], None), lambda: f.cross_covariance([], [1])):
        with pytest.raises(ValueError):
            call()
    assert len(rec.calls) == ncalls


# ------------------------------------------------------------------------------------------------------------------
# the MEX gateway
# ------------------------------------------------------------------------------------------------------------------
_STUB = r'''
#include <math.h>
#include <stdio.h>
#include "ekfslam.h"
void stub_fail_next(ekf_handle *h);
static int fail_armed;
void arm_failure(void) { fail_armed = 1; }
int32_t ekf_multiply_map(ekf_handle *h, const double *B, int64_t k, double *out) {
    int64_t N;
    ekf_num_landmarks(h, &N);
    const int64_t n = 3 + 2 * N;
    printf("ABI ekf_multiply_map k=%d B0=%g BLast=%g\n", (int)k, B[0], B[k * n - 1]);
    if (fail_armed) { fail_armed = 0; stub_fail_next(h); return ekf_flush(h); }
    for (int64_t i = 0; i < k * n; ++i) out[i] = 100.0 + B[i];
    return EKF_OK;
}
'''

_DRIVER = driver(r'''
    const mxArray *sx[3] = { mock_string("set_x"), h, mock_double(7, 1, (const double[]){ 1, 2, 3, 4, 5, 6, 7 }) };
    if (call("set_x", 0, 3, sx)) return 1;
    const mxArray *two = mock_double(7, 2, (const double[]){ 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14 });
    const mxArray *mm[3] = { mock_string("multiply_map"), h, two };
    if (call("multiply_map", 1, 3, mm)) return 1;
    if (!call("multiply_map", 1, 2, mm)) return 1;
    const mxArray *bad[3] = { mm[0], h, mock_double(5, 1, (const double[]){ 1, 2, 3, 4, 5 }) };
    if (!call("multiply_map badsize", 1, 3, bad)) return 1;
    bad[2] = mock_double(0, 0, (const double[]){ 0 });
    if (!call("multiply_map empty", 1, 3, bad)) return 1;
    arm_failure();
    if (!call("multiply_map", 1, 3, mm)) return 1;
''', PRELUDE_SHOWN)

_DRIVER_WITHOUT = driver_without(r'''
    const mxArray *mm[3] = { mock_string("multiply_map"), h, mock_double(7, 1, (const double[]){ 1, 2, 3, 4, 5, 6, 7 }) };
    if (!call("multiply_map", 1, 3, mm)) return 1;
''')


def test_mex_gateway_reaches_the_abi(tmp_path):
    t = transcript_of(tmp_path, _STUB, _DRIVER)
    i = t.index("ABI ekf_multiply_map k=2 B0=1 BLast=14")
    assert t[i + 1] == "MEX multiply_map nrhs=3 -> ok out0=7x2[101,102,103,104,105,106,107,108,109,110,111,112,113,114]"
    assert any(ln.startswith("MEX multiply_map nrhs=2 -> ERROR ekfslam:usage") and "needs 3 arguments" in ln for ln in t)
    for name in ("badsize", "empty"):
        assert any(ln.startswith("MEX multiply_map %s nrhs=3 -> ERROR ekfslam:usage" % name) and "B is n x k" in ln for ln in t), name
    assert sum(ln.startswith("ABI ekf_multiply_map") for ln in t) == 2              # the good call and the injected failure
    assert "MEX multiply_map nrhs=3 -> ERROR ekfslam:status | call not valid in the current state: injected failure" in t
    assert t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_the_gateway_still_links_against_a_library_without_the_symbol(tmp_path):
    t = transcript_of(tmp_path, _DRIVER_WITHOUT)
    assert any(ln.startswith("MEX multiply_map ") and "ERROR ekfslam:usage" in ln and "this libekfslam has no ekf_multiply_map" in ln for ln in t)
    assert "MEX predict nrhs=3 -> ok" in t and t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_matlab_method_and_documents_name_the_call():
    text = open(os.path.join(ROOT, "matlab", "EKF_SLAM.m")).read()
    m = re.search(r"function\s+out\s*=\s*multiplyMap\(h,\s*B\)(.*?)\n        end\b", text, re.S)
    assert m and "h.gateway('multiply_map', double(B));" in m.group(1)
    src = open(os.path.join(ROOT, "matlab", "ekfslam_mex.c")).read()
    assert src.count('strcmp(cmd, "multiply_map")') == 1 and "#pragma weak ekf_multiply_map" in src
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        body = open(os.path.join(ROOT, doc)).read()
        assert "multiply_map" in body, doc
    assert "multiplyMap" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for word in ("k_multiply_tiles", "k_multiply_sum", "k_multiply_robot", "3z"):
        assert word in design, word
