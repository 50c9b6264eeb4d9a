"""CPU: ekf_sample_map without a GPU -- the NumPy restatement of tests/sample_map_cases.py against numpy.linalg.cholesky of the permuted
P; the kernels of ekf_slam_amd/csrc/sample_map.h (behind those of factor_map.h) compiled for the host (factor tile edges 16 and 32, segments of 2 tiles, F64 and float
sources, the matrix-core loops as their plain-FMA twins in the same k order) against that restatement, and bit for bit where the header
promises bits; the Python layers over a stand-in for the library (one marshal per call, the refusals before any call, seeded draws, the
two policies against closed forms); the MEX gateway's command under the MEX mock."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import factor_map_cases as F
import sample_map_cases as S
from helpers import REL, ROOT, RecorderBase, host_build
from mex_harness import PRELUDE_SHOWN, driver, driver_without, transcript_of

dp = ctypes.POINTER(ctypes.c_double)
SIZES = [0, 1, 13, 16, 40]          # N = 16 at edge 32 ends exactly on a tile edge; N = 40 at edge 16 has five tile columns
PTHREAD = ["-O2", "-mfma", "-ffp-contract=off", "-pthread"]
CSRC = os.path.join(ROOT, "ekf_slam_amd", "csrc")


# ------------------------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [0, 1, 13, 40])
def test_the_restatement_agrees_with_numpy_cholesky(N):
    x, s, P = F.spd_scene(N, 40 + N)
    n = x.size
    C = S.factor_in_x_order(F.factor_dense(x, P)["L"])
    want = S.cholesky_in_x_order(P)
    err_c = np.abs(C - want).max() / np.abs(want).max()
    err_p = np.abs(C @ C.T - P).max() / np.abs(P).max()
    print("N=%d: C against numpy.linalg.cholesky of the permuted P %.2e, C C' against P %.2e" % (N, err_c, err_p))
    assert err_c < 1e-12 and err_p < 1e-13
    order = F.elimination_order(n)
    assert not np.triu(C[np.ix_(order, order)], 1).any()      # lower-triangular in elimination order, not in x's
    xi = S.unit_draws(n)
    got = S.sample_dense(x, P, xi)
    assert np.abs(S.recovered_factor(x, got) - C).max() < 1e-12           # (x + c) - x: what x's size takes of c's last bits
    assert np.abs(got[n:] - (x + xi[n:] @ want.T)).max() < 1e-12 * max(np.abs(got).max(), 1.0)
    np.testing.assert_array_equal(S.sample_dense(x, P, np.zeros((2, n))), np.vstack([x, x]))
    xb, sb, Pb = F.indefinite_scene(13, 3 + 7)
    assert np.isnan(S.sample_dense(xb, Pb, np.ones((3, xb.size)))).all()


# ------------------------------------------------------------------------------------------------------------------
# the kernels compiled for the host
# ------------------------------------------------------------------------------------------------------------------
def _bit_draws(n):
    """zero, the unit vectors, a Gaussian draw g at the start of a chunk's middle, another draw, g again at the end: n + 4 rows."""
    g = S.gaussian_draws(2, n, 77)
    return np.vstack([np.zeros((1, n)), np.eye(n), g[0], g[1], g[0]])


def _scenes():
    """name -> (TF, Tsrc, float, N, x, P, xi)."""
    out = {}
    for TF in (16, 32):
        for fl in (0, 1):
            for N in SIZES:
                x, s, P = F.spd_scene(N, 100 + N)
                for k in S.KS:
                    out["spd_F%d_%s_N%d_k%d" % (TF, "f" if fl else "d", N, k)] = (TF, 48 - TF, fl, N, x, P, S.gaussian_draws(k, x.size, 1000 + k))
        for N in (13, 40):
            x, s, P = F.spd_scene(N, 100 + N)
            g = S.gaussian_draws(2, x.size, 77)
            out["bits_F%d_N%d" % (TF, N)] = (TF, 48 - TF, 0, N, x, P, _bit_draws(x.size))
            out["alone_F%d_N%d" % (TF, N)] = (TF, 48 - TF, 0, N, x, P, g[:1])
            batch = S.gaussian_draws(2 * S.CHUNK + 3, x.size, 5)
            batch[0], batch[S.CHUNK + 1], batch[-1] = g[0], g[0], g[0]
            out["batch_F%d_N%d" % (TF, N)] = (TF, 48 - TF, 0, N, x, P, batch)
        x, s, P = F.spd_scene(13, 113)
        x = x.copy()
        x[[1, 4, 28]] = -0.0                                   # a robot entry, a landmark entry, the last entry
        e5 = np.zeros(x.size)
        e5[5] = 1.0
        out["negzero_F%d" % TF] = (TF, 48 - TF, 0, 13, x, P, np.vstack([np.zeros(x.size), e5]))
    for name, TF, bad, zero in (("neg_first_tile", 16, 3 + 5, False), ("neg_third_tile", 16, 3 + 32, False), ("neg_last_row", 32, 3 + 79, False),
                                ("neg_robot", 16, 1, False), ("zero_landmark", 16, 3 + 41, True)):
        x, s, P = F.indefinite_scene(40, bad, zero)
        out[name] = (TF, 48 - TF, 0, 40, x, P, S.gaussian_draws(S.CHUNK + 1, x.size, 3))
    x, s, P = F.spd_scene(13, 9)
    P[:3, :] = 0.0
    P[:, :3] = 0.0
    out["known_pose"] = (32, 16, 1, 13, x, P, S.gaussian_draws(2, x.size, 3))
    return out


INFO_TWINS = ("neg_first_tile", "neg_third_tile", "neg_last_row", "neg_robot", "zero_landmark", "known_pose", "spd_F16_f_N40_k1", "spd_F32_d_N13_k17")


def _write_cases(d, scenes, names=None, factor_form=False):
    """cases.txt and the inputs; factor_form: as factor_map_host_emulation reads them, with no reference states."""
    with open(os.path.join(str(d), "cases.txt"), "w") as f:
        for name, (TF, Tsrc, fl, N, x, P, xi) in scenes.items():
            if names is not None and name not in names:
                continue
            f.write("%s %d %d %d %d %d\n" % (name, TF, Tsrc, fl, N, 0 if factor_form else xi.shape[0]))
            parts = [x, P.reshape(-1, order="F")] + ([] if factor_form else [xi.reshape(-1)])
            np.concatenate(parts).tofile(os.path.join(str(d), name + ".in"))


@pytest.fixture(scope="module")
def emulation(tmp_path_factory):
    d = tmp_path_factory.mktemp("sample_map_emulation")
    scenes = _scenes()
    _write_cases(d, scenes)
    exe = host_build("sample_map_host_emulation", str(d / "emu"), flags=PTHREAD)
    r = subprocess.run([exe, str(d)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    return d, r.stdout, scenes


def _output(d, name, scenes):
    """(the result block and the pivots, the samples) of a case."""
    return _output_with_factor(d, name, scenes)[:2]


def _output_with_factor(d, name, scenes):
    """... and the factor the launches applied, [L 0; W' L_r] in elimination order as the emulation read it out of the store."""
    TF, _, _, N, x, _, xi = scenes[name]
    v = np.fromfile(os.path.join(str(d), name + ".out"))
    rows = -(-2 * N // TF) * TF
    n = x.size
    assert v.size == 16 + rows + xi.size + n * n
    head = 16 + rows
    return v[:head], v[head:head + xi.size].reshape(xi.shape), v[head + xi.size:].reshape(n, n)


@pytest.mark.parametrize("fl", [0, 1])
@pytest.mark.parametrize("TF", [16, 32])
def test_host_emulation_of_the_kernels_against_the_restatement(emulation, TF, fl):
    """Every size and every k, the source's tile edge different from the factor's: the samples at helpers.REL of the restatement on the
    matrix as the handle holds it; every partial block written whole, nothing of the state written."""
    d, out, scenes = emulation
    worst = 0.0
    for N in SIZES:
        for k in S.KS:
            name = "spd_F%d_%s_N%d_k%d" % (TF, "f" if fl else "d", N, k)
            assert "%s: 0 differences" % name in out
            _, _, sfl, _, x, P, xi = scenes[name]
            want = S.sample_dense(x, S.as_held(P, sfl), xi)
            _, got = _output(d, name, scenes)
            err = np.abs(got - want).max() / max(np.abs(want).max(), 1.0)
            worst = max(worst, err)
            assert err < REL, (name, err)
    print("edge %d, %s source: worst error of a sample against the restatement %.2e" % (TF, "float" if fl else "F64", worst))


@pytest.mark.parametrize("N", [13, 40])
@pytest.mark.parametrize("TF", [16, 32])
def test_host_emulation_keeps_the_promised_bits(emulation, TF, N):
    """xi = 0 gives x; the unit vectors return the columns of C, bit for bit: sample j is fl(x + C[:, j]) with C the factor the launches
    applied, which the emulation writes out (and which is lower-triangular in elimination order, NumPy's factor and C C' = P within
    REL); a draw gives the same bits alone, and at the start, in the middle and at the end of larger batches."""
    d, out, scenes = emulation
    names = ["%s_F%d_N%d" % (w, TF, N) for w in ("bits", "alone", "batch")]
    for name in names:
        assert "%s: 0 differences" % name in out
    _, _, _, _, x, P, xi = scenes[names[0]]
    n = x.size
    _, got, Le = _output_with_factor(d, names[0], scenes)
    np.testing.assert_array_equal(got[0], x)
    # THE UNIT VECTORS RETURN THE COLUMNS OF C, exactly: with xi = e_j every chain keeps the one term fma(C_ij, 1, +0) = C_ij and adds
    # zeros, so sample j is fl(x + C[:, j]) with C the factor the launches applied, bit for bit
    assert not np.triu(Le, 1).any()                           # lower-triangular in elimination order: exact zeros
    C = S.factor_in_x_order(Le)
    for j in range(n):
        np.testing.assert_array_equal(got[1 + j], x + C[:, j])
    # ... and that factor is the Cholesky factor of P: against NumPy's, and C C' against P
    want = S.cholesky_in_x_order(P)
    assert np.abs(C - want).max() < REL * np.abs(want).max() and np.abs(C @ C.T - P).max() < REL * np.abs(P).max()
    alone = _output(d, names[1], scenes)[1][0]
    batch = _output(d, names[2], scenes)[1]
    for row in (got[n + 1], got[n + 3], batch[0], batch[S.CHUNK + 1], batch[-1]):
        np.testing.assert_array_equal(row, alone)
    assert not np.array_equal(got[n + 2], alone)


@pytest.mark.parametrize("TF", [16, 32])
def test_host_emulation_returns_x_with_its_signed_zeros(emulation, TF):
    """xi = 0 gives x bit for bit, entries that are -0.0 included (assert_array_equal alone cannot tell -0.0 from +0.0); a unit vector
    leaves them alone wherever its column of C is zero."""
    d, out, scenes = emulation
    name = "negzero_F%d" % TF
    assert "%s: 0 differences" % name in out
    x = scenes[name][4]
    _, got, Le = _output_with_factor(d, name, scenes)
    assert got[0].tobytes() == x.tobytes() and np.signbit(got[0][[1, 4, 28]]).all()
    C = S.factor_in_x_order(Le)
    assert C[4, 5] == 0.0 and C[28, 5] != 0.0 and C[1, 5] != 0.0      # entry 4 comes before entry 5 in the elimination order, 28 and the robot after
    np.testing.assert_array_equal(got[1], x + C[:, 5])
    assert np.signbit(got[1][4]) and got[1][28] == C[28, 5] and got[1][1] == C[1, 5]


def test_host_emulation_of_a_matrix_that_is_not_definite(emulation, tmp_path):
    """All-NaN samples, and the result block and the pivots bit for bit those of the factor emulation on the same scene -- for the
    scenes that are not definite and for two that are."""
    d, out, scenes = emulation
    _write_cases(tmp_path, scenes, INFO_TWINS, factor_form=True)
    exe = host_build("factor_map_host_emulation", str(tmp_path / "emu"), flags=PTHREAD)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    for name in INFO_TWINS:
        assert "%s: 0 differences" % name in out
        block, got, Le = _output_with_factor(d, name, scenes)
        np.testing.assert_array_equal(block, np.fromfile(os.path.join(str(tmp_path), name + ".out")))
        if name.startswith("spd"):
            assert block[0] == 0.0 and np.isfinite(got).all() and np.isfinite(Le).all()
        else:
            assert block[0] != 0.0 and np.isnan(got).all() and np.isnan(Le).all()


def test_kernel_sources_on_the_host_under_the_sanitizers(tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined runs clean on definite and not-definite scenes per factor
    tile edge: no lane of the two new kernels reads or writes outside the chunks, the partial blocks, the factor store or the state
    (nothing loaded into python is involved)."""
    _write_cases(tmp_path, _scenes(), ("spd_F16_f_N40_k35", "spd_F32_d_N13_k17", "spd_F32_d_N0_k1", "spd_F32_d_N16_k16", "neg_third_tile", "known_pose"))
    exe = host_build("sample_map_host_emulation", str(tmp_path / "emulation_sanitized"),
                     flags=["-O1", "-g", "-mfma", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]


def test_the_twin_runs_the_matrix_instructions_k_order():
    """The plain-FMA twin of a tile's product with a chunk and its matrix-core loop name their k index through the same function,
    chunk_k, in the ONE place that holds them, tile_mac of map_blocks.h; the apply pass goes through it once per tile and holds no
    matrix instruction of its own; the finish stores the rest of L_r only where it is asked to."""
    mac = _tile_mac()
    assert mac.count("chunk_k(s, t)") == 3 and mac.count("chunk_k(s, lr)") == 3
    twin, _, device = mac.partition("#else")
    assert "#if defined(EKF_FACTOR_FMA_TWIN)" in twin and "__builtin_amdgcn_mfma" not in twin and "#endif" in device
    assert mac.count("__builtin_amdgcn_mfma") == 1 and "__builtin_amdgcn_mfma_f64_16x16x4f64(av[s], bv[s], acc, 0, 0, 0)" in device
    src = open(os.path.join(CSRC, "sample_map.h")).read()
    assert "__builtin_amdgcn_mfma" not in src and "EKF_FACTOR_FMA_TWIN" not in src
    body = src[src.index("void k_factor_apply("):src.index("void k_factor_sample(")]
    assert body.count("tile_mac<") == 1 and body.count("tile_mac<TF, false, false>") == 1 and body.count("__syncthreads()") == 2
    assert "atomicAdd" not in src and "__hip_atomic" not in src
    assert "if (a.lr_off) {" in open(os.path.join(CSRC, "factor_map.h")).read()


def _tile_mac():
    """The text of tile_mac in map_blocks.h: from its name to the next function."""
    blocks = open(os.path.join(CSRC, "map_blocks.h")).read()
    rest = blocks[blocks.index("void tile_mac("):]
    return rest[:rest.index("__device__", 1)]


def test_segment_of_inverts_factor_segment_base(tmp_path):
    """segment_of, the decode both segment kernels share, compiled for the host: for S in {1, 2, 16} and every tile-row count nF <= 40
    it visits every (I, seg), I < nF, exactly once over w in [0, factor_segment_base(nF, S)), in factor_segment_base's order, with
    J0 = seg S and J1 = min(J0 + S, I + 1) -- nF = 1, I = S - 1, I = S and w = base - 1, where the square root's guess can be off by
    one, among them.  The program prints one line "S nF I seg J0 J1" per w; the expectation is built here."""
    exe = host_build("segment_of_host", str(tmp_path / "segment_of_host"), flags=PTHREAD)
    r = subprocess.run([exe, "40", "1", "2", "16"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = {}
    for ln in r.stdout.split("\n"):
        if ln:
            v = [int(t) for t in ln.split()]
            got.setdefault((v[0], v[1]), []).append(tuple(v[2:]))
    assert sorted(got) == [(S, nF) for S in (1, 2, 16) for nF in range(1, 41)]
    for (S, nF), rows in got.items():
        want = [(I, seg, seg * S, min(seg * S + S, I + 1)) for I in range(nF) for seg in range(I // S + 1)]
        assert rows == want, (S, nF)
        assert len(set((I, seg) for I, seg, _, _ in rows)) == len(rows) == sum(I // S + 1 for I in range(nF))


# ------------------------------------------------------------------------------------------------------------------
# the Python layers over a stand-in for the library
# ------------------------------------------------------------------------------------------------------------------
X7 = np.array([1.0, -2.0, 30.0, 4.0, 5.0, -3.0, 6.0])


def _p7():
    A = np.random.default_rng(21).normal(0.0, 0.3, (7, 7))
    return A @ A.T + 0.2 * np.eye(7)


class _Recorder(RecorderBase):
    """ekf_sample_map as the NumPy restatement on a fixed two-landmark Gaussian."""
    status_string = b"invalid argument"
    last_error = b"sample_map: not built for sharded handles (world > 1): injected"

    def __init__(self):
        self.calls, self.fail, self.N, self.definite, self.P = [], 0, 2, 1, _p7()

    def ekf_num_landmarks(self, h, pn):
        pn._obj.value = self.N
        return 0

    def ekf_sample_map(self, h, xi, k, out, info):
        assert isinstance(k, ctypes.c_int64)                   # marshalled once, by marshal.sample_args
        n = 3 + 2 * self.N
        draws = np.array([xi[i] for i in range(k.value * n)]).reshape(k.value, n)
        self.calls.append(("sample_map", h.value, draws))
        if self.fail:
            return self.fail
        info._obj.n, info._obj.definite, info._obj.bad_index, info._obj.logdet = n, self.definite, -1 if self.definite else 4, -3.5
        res = S.sample_dense(X7, self.P, draws) if self.definite else np.full((k.value, n), np.nan)
        for i, v in enumerate(res.reshape(-1)):
            out[i] = v
        return 0


def test_layers_marshal_a_sampling_call_once(monkeypatch):
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import engine as E
    from ekf_slam_amd import marshal
    from ekf_slam_amd import slam as SL
    from ekf_slam_amd.sharding import ShardGroup
    from ekf_slam_amd.trajectory import TrajectoryLog
    assert L.SIGNATURES["ekf_sample_map"] == (ctypes.c_int32, [ctypes.c_void_p, dp, ctypes.c_int64, dp, ctypes.POINTER(L.EkfFactorInfo)])
    header = open(os.path.join(ROOT, "include", "ekfslam.h")).read()
    assert "int32_t ekf_sample_map(ekf_handle *h, const double *xi" in header and "ELIMINATION ORDER" in header and "[L 0; W' L_r]" in header
    assert "THE LIBRARY GENERATES NO RANDOM NUMBERS" in header and "NOT wrapped" in header
    rec = _Recorder()
    monkeypatch.setattr(L, "lib", lambda: rec)
    made = []
    real = marshal.sample_args
    monkeypatch.setattr(marshal, "sample_args", lambda *a, **k: made.append(a) or real(*a, **k))
    g = E.Engine(capacity=32, tile=16)
    one = np.arange(7.0) / 7.0
    samples, info = g.sample_map(one)
    assert len(rec.calls) == 1 and len(made) == 1 and rec.calls[0][1] == g.h.value
    np.testing.assert_array_equal(rec.calls[0][2], one[None, :])
    np.testing.assert_array_equal(samples, S.sample_dense(X7, rec.P, one))
    assert samples.shape == (1, 7) and samples.dtype == np.float64 and samples.flags["C_CONTIGUOUS"]
    assert sorted(info) == sorted(F.KEYS) and info["definite"] is True and info["n"] == 7 and info["bad_index"] == -1
    five = np.asfortranarray(np.random.default_rng(2).standard_normal((5, 7)).astype(np.float32))      # neither F64 nor C-contiguous
    samples, info = g.sample_map(five)
    np.testing.assert_array_equal(rec.calls[-1][2], five.astype(np.float64))
    assert samples.shape == (5, 7) and len(made) == 2
    # the refusals, in marshal, before anything is sent
    ncalls = len(rec.calls)
    bad_nan = one.copy()
    bad_nan[4] = np.nan
    for xi in (None, np.zeros((0, 7)), np.zeros(6), np.zeros((2, 9)), bad_nan, np.full((2, 7), np.inf), np.zeros((2, 1, 7))):
        with pytest.raises(ValueError) as err:
            g.sample_map(xi)
        assert "sample_map" in str(err.value)
    assert len(rec.calls) == ncalls
    # the library's refusal raises; a shard group hands the call to its first shard so that the refusal is the library's
    rec.fail = L.EKF_ERR_INVALID_ARG
    with pytest.raises(L.EkfError) as err:
        g.sample_map(one)
    assert err.value.status == L.EKF_ERR_INVALID_ARG and "sample_map" in str(err.value)
    grp = ShardGroup(2, capacity=16)
    with pytest.raises(L.EkfError) as err:
        grp.sample_map(one)
    assert rec.calls[-1][0] == "sample_map" and rec.calls[-1][1] == grp.shards[0].h.value and "sharded" in str(err.value)
    rec.fail = 0
    # the policy layer: the caller's draws or seeded ones, one call each, nothing logged
    for cls in (SL.EKF_SLAM, SL.EKF_SLAM_UC):
        rec.calls.clear()
        del made[:]
        f = cls(capacity=32, tile=64)
        f.log = TrajectoryLog()
        a, _ = f.sample_map(xi=five)
        np.testing.assert_array_equal(rec.calls[-1][2], five.astype(np.float64))
        b, _ = f.sample_map(6, seed=3)
        c, _ = f.sample_map(k=6, seed=3)
        d, _ = f.sample_map(6, seed=4)
        np.testing.assert_array_equal(rec.calls[1][2], np.random.default_rng(3).standard_normal((6, 7)))
        np.testing.assert_array_equal(b, c)
        assert b.shape == (6, 7) and not np.array_equal(b, d)
        assert len(rec.calls) == 4 and len(made) == 4 and len(f.log.edits) == 0
        for kw in (dict(), dict(k=0), dict(k=3, xi=five), dict(seed=1, xi=five)):
            with pytest.raises(ValueError) as err:
                f.sample_map(**kw)
            assert "sample_map" in str(err.value)
        assert len(rec.calls) == 4


SEED, DRAWS, SIGMAS = 12, 4000, 4.0


def test_the_two_policies_against_closed_forms(monkeypatch):
    """On a two-landmark Gaussian: E of the landmarks' difference is mu_d, E |d|^2 = |mu_d|^2 + tr Sigma_d, and
    P(landmark 1's first coordinate > its mean + sigma / 2) = 1 - Phi(1/2).  Each estimate within SIGMAS = 4 of ITS OWN reported
    standard error with the fixed seed: under the normal approximation a miss of one such comparison has probability 6e-5, and the seed
    is fixed, so the test is deterministic.  The stand-in library is the NumPy restatement, so this is also the check that the
    restatement alone passes with that seed and multiple."""
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import slam as SL
    rec = _Recorder()
    monkeypatch.setattr(L, "lib", lambda: rec)
    P = rec.P
    A = np.zeros((2, 7))
    A[0, 3], A[0, 5], A[1, 4], A[1, 6] = 1.0, -1.0, 1.0, -1.0                  # d = landmark 1 - landmark 2
    mu_d, Sig_d = A @ X7, A @ P @ A.T
    f = SL.EKF_SLAM(capacity=32, tile=64)
    mean, se = f.posterior_expectation(lambda v: A @ v, DRAWS, seed=SEED)
    assert mean.shape == (2,) and se.shape == (2,) and np.all(se > 0)
    assert np.all(np.abs(mean - mu_d) <= SIGMAS * se), (mean, mu_d, se)
    assert np.allclose(se, np.sqrt(np.diag(Sig_d) / DRAWS), rtol=0.1)
    m2, se2 = f.posterior_expectation(lambda v: float((A @ v) @ (A @ v)), DRAWS, seed=SEED)
    want2 = float(mu_d @ mu_d + np.trace(Sig_d))
    assert np.ndim(m2) == 0 and abs(m2 - want2) <= SIGMAS * se2, (m2, want2, se2)
    sigma = math.sqrt(P[3, 3])
    p, sep = f.probability(lambda v: v[3] > X7[3] + 0.5 * sigma, DRAWS, seed=SEED)
    want_p = 1.0 - 0.5 * (1.0 + math.erf(0.5 / math.sqrt(2.0)))
    assert abs(p - want_p) <= SIGMAS * sep and abs(sep - math.sqrt(want_p * (1 - want_p) / DRAWS)) < 0.1 * sep, (p, want_p, sep)
    assert len(rec.calls) == 3 and all(c[2].shape == (DRAWS, 7) for c in rec.calls)
    # the restatement alone, with no layer in between, on the same draws
    direct = S.sample_dense(X7, P, np.random.default_rng(SEED).standard_normal((DRAWS, 7)))
    assert np.allclose((direct @ A.T).mean(axis=0), mean, rtol=1e-12, atol=0.0)
    # a P that is not definite: both raise and name factor_map
    rec.definite = 0
    for call in (lambda: f.posterior_expectation(lambda v: v[0], 10), lambda: f.probability(lambda v: True, 10)):
        with pytest.raises(ValueError) as err:
            call()
        assert "factor_map" in str(err.value)
    with pytest.raises(ValueError):
        f.posterior_expectation(lambda v: v[0], 1)


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
int32_t ekf_sample_map(ekf_handle *h, const double *xi, int64_t k, double *out, ekf_factor_info *info) {
    int64_t N;
    ekf_num_landmarks(h, &N);
    const int64_t n = 3 + 2 * N;
    printf("ABI ekf_sample_map k=%d xi0=%g xiLast=%g\n", (int)k, xi[0], xi[k * n - 1]);
    if (fail_armed) { fail_armed = 0; stub_fail_next(h); return ekf_flush(h); }
    info->n = n; info->definite = 1; info->bad_index = -1; info->bad_pivot = 0.0; info->logdet = -1.5; info->logdet_map = -2.5;
    info->min_pivot = 0.25; info->max_pivot = 4.0;
    for (int64_t i = 0; i < k * n; ++i) out[i] = 100.0 + xi[i];
    return EKF_OK;
}
'''

_DRIVER = driver(r'''
    const mxArray *sx[3] = { mock_string("set_x"), h, mock_double(7, 1, (const double[]){ 1, 2, 3, 4, 5, 6, 7 }) };
    if (call("set_x", 0, 3, sx)) return 1;
    const mxArray *two = mock_double(7, 2, (const double[]){ 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14 });
    const mxArray *sm[3] = { mock_string("sample_map"), h, two };
    if (call("sample_map", 2, 3, sm)) return 1;
    if (call("sample_map one_output", 1, 3, sm)) return 1;
    if (!call("sample_map", 2, 2, sm)) return 1;
    const mxArray *bad[3] = { sm[0], h, mock_double(5, 1, (const double[]){ 1, 2, 3, 4, 5 }) };
    if (!call("sample_map badsize", 2, 3, bad)) return 1;
    bad[2] = mock_double(0, 0, (const double[]){ 0 });
    if (!call("sample_map empty", 2, 3, bad)) return 1;
    arm_failure();
    if (!call("sample_map", 2, 3, sm)) return 1;
''', PRELUDE_SHOWN)

_DRIVER_WITHOUT = driver_without(r'''
    const mxArray *sm[3] = { mock_string("sample_map"), h, mock_double(7, 1, (const double[]){ 1, 2, 3, 4, 5, 6, 7 }) };
    if (!call("sample_map", 1, 3, sm)) return 1;
''')


def test_mex_gateway_reaches_the_abi(tmp_path):
    t = transcript_of(tmp_path, _STUB, _DRIVER)
    i = t.index("ABI ekf_sample_map k=2 xi0=1 xiLast=14")
    assert t[i + 1] == "MEX sample_map nrhs=3 -> ok out0=7x2[101,102,103,104,105,106,107,108,109,110,111,112,113,114] out1=1x8[7,1,0,0,-1.5,-2.5,0.25,4]"
    assert any(ln.startswith("MEX sample_map one_output nrhs=3 -> ok out0=7x2[") and "out1" not in ln for ln in t)
    assert any(ln.startswith("MEX sample_map nrhs=2 -> ERROR ekfslam:usage") and "needs 3 arguments" in ln for ln in t)
    for name in ("badsize", "empty"):
        assert any(ln.startswith("MEX sample_map %s nrhs=3 -> ERROR ekfslam:usage" % name) and "xi is n x k" in ln for ln in t), name
    assert sum(ln.startswith("ABI ekf_sample_map") for ln in t) == 3            # the two good calls and the injected failure
    assert "MEX sample_map nrhs=3 -> ERROR ekfslam:status | call not valid in the current state: injected failure" in t
    assert t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_the_gateway_still_links_against_a_library_without_the_symbol(tmp_path):
    t = transcript_of(tmp_path, _DRIVER_WITHOUT)
    assert any(ln.startswith("MEX sample_map ") and "ERROR ekfslam:usage" in ln and "this libekfslam has no ekf_sample_map" in ln for ln in t)
    assert "MEX predict nrhs=3 -> ok" in t and t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_matlab_method_and_documents_name_the_call():
    text = open(os.path.join(ROOT, "matlab", "EKF_SLAM.m")).read()
    m = re.search(r"function\s+\[samples,\s*info\]\s*=\s*sampleMap\(h,\s*xi\)(.*?)\n        end\b", text, re.S)
    assert m and "h.gateway('sample_map', double(xi));" in m.group(1)
    src = open(os.path.join(ROOT, "matlab", "ekfslam_mex.c")).read()
    assert src.count('strcmp(cmd, "sample_map")') == 1 and "#pragma weak ekf_sample_map" in src
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        body = open(os.path.join(ROOT, doc)).read()
        assert "sample_map" in body, doc
    assert "sampleMap" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "k_factor_apply" in design and "k_factor_sample" in design
