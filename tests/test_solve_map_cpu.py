"""CPU: ekf_solve_map without a GPU -- the NumPy restatement of tests/solve_map_cases.py against numpy.linalg.solve and a triangular
solve with numpy.linalg.cholesky of the permuted P; the kernels of ekf_slam_amd/csrc/solve_map.h (behind those of factor_map.h) compiled
for the host (factor tile edges 16 and 32, F64 and float sources, the matrix-core loops as their plain-FMA twins in the same k order)
against NumPy, and bit for bit where the header promises bits; the closed loops with the sample and the factor emulations; the Python
layers over a stand-in for the library (one marshal per call, the refusals before any call, the three policies against closed forms);
the MEX gateway's command under the MEX mock.

THE BAR of every comparison with NumPy is solve_map_cases.bar(P) = 64 cond_2(P) 2^-53 on max-abs over the max-abs of the expected
result, P the matrix as the handle holds it (sample_map_cases.as_held for float tiles); it is also asserted below helpers.REL."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import factor_map_cases as F
import sample_map_cases as S
import solve_map_cases as V
from helpers import REL, ROOT, RecorderBase, host_build
from mex_harness import PRELUDE_SHOWN, driver, driver_without, transcript_of

dp = ctypes.POINTER(ctypes.c_double)
SIZES = [0, 1, 13, 16, 40]          # at edge 16, N = 16 ends exactly on a tile edge and N = 40 has five tile columns
PTHREAD = ["-O2", "-mfma", "-ffp-contract=off", "-pthread"]
FORM_NAMES = ((V.FULL, "full"), (V.HALF, "half"))


# ------------------------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [0, 1, 13, 40])
def test_the_restatement_agrees_with_numpy(N):
    x, s, P = F.spd_scene(N, 40 + N)
    n = x.size
    B = np.vstack([np.eye(n), S.gaussian_draws(3, n, 1)])
    bar = V.bar(P)
    assert bar < REL
    for form, name in FORM_NAMES:
        got = V.solve_dense(x, P, B, form)
        err = V.rel_err(got, V.expected(P, B, form))
        print("N=%d %s: the restatement against NumPy %.2e (bar %.2e)" % (N, name, err, bar))
        assert err < bar
        assert not V.solve_dense(x, P, np.zeros((2, n)), form).any()
    half = V.solve_dense(x, P, B, V.HALF)
    assert V.rel_err(np.sum(half * half, axis=1), np.einsum("qi,qi->q", B, np.linalg.solve(P, B.T).T)) < bar       # |C^-1 b|^2 = b' P^-1 b
    C = S.cholesky_in_x_order(P)
    xi = S.gaussian_draws(4, n, 2)
    assert V.rel_err(V.solve_dense(x, P, xi @ C.T, V.HALF), xi) < bar                   # C^-1 (C xi) = xi
    xb, sb, Pb = F.indefinite_scene(13, 3 + 7)
    assert np.isnan(V.solve_dense(xb, Pb, np.ones((3, xb.size)), V.FULL)).all()


# ------------------------------------------------------------------------------------------------------------------
# the kernels compiled for the host
# ------------------------------------------------------------------------------------------------------------------
def _scenes():
    """name -> (TF, Tsrc, float, N, x, P, B, form)."""
    out = {}
    for TF in (16, 32):
        for fl in (0, 1):
            for N in SIZES:
                x, s, P = F.spd_scene(N, 100 + N)
                for k in S.KS:
                    for form, fname in FORM_NAMES:
                        out["spd_F%d_%s_N%d_k%d_%s" % (TF, "f" if fl else "d", N, k, fname)] = (TF, 48 - TF, fl, N, x, P, S.gaussian_draws(k, x.size, 1000 + k), form)
        for N in (13, 40):
            x, s, P = F.spd_scene(N, 100 + N)
            g = S.gaussian_draws(2, x.size, 77)
            batch = S.gaussian_draws(2 * S.CHUNK + 3, x.size, 5)
            batch[0], batch[S.CHUNK + 1], batch[-1] = g[0], g[0], g[0]
            for form, fname in FORM_NAMES:
                out["bits_F%d_N%d_%s" % (TF, N, fname)] = (TF, 48 - TF, 0, N, x, P, np.vstack([np.zeros((1, x.size)), g[0], g[1], g[0]]), form)
                out["alone_F%d_N%d_%s" % (TF, N, fname)] = (TF, 48 - TF, 0, N, x, P, g[:1], form)
                out["batch_F%d_N%d_%s" % (TF, N, fname)] = (TF, 48 - TF, 0, N, x, P, batch, form)
    for name, TF, bad, zero in (("neg_first_tile", 16, 3 + 5, False), ("neg_third_tile", 16, 3 + 32, False), ("neg_last_row", 32, 3 + 79, False),
                                ("neg_robot", 16, 1, False), ("zero_landmark", 16, 3 + 41, True)):
        x, s, P = F.indefinite_scene(40, bad, zero)
        out[name] = (TF, 48 - TF, 0, 40, x, P, S.gaussian_draws(S.CHUNK + 1, x.size, 3), V.FULL if TF == 16 else V.HALF)
    x, s, P = F.spd_scene(13, 9)
    P[:3, :] = 0.0
    P[:, :3] = 0.0
    out["known_pose"] = (32, 16, 1, 13, x, P, S.gaussian_draws(2, x.size, 3), V.FULL)
    return out


INFO_TWINS = ("neg_first_tile", "neg_third_tile", "neg_last_row", "neg_robot", "zero_landmark", "known_pose", "spd_F16_f_N40_k1_full", "spd_F32_d_N13_k17_half")
LOOPS = [(16, 40), (32, 13), (32, 16)]                         # (factor tile edge, N) of the closed loops


def _write_cases(d, scenes, names=None, kind="solve", refs=None):
    """cases.txt and the inputs, as the emulation of that kind reads them: "solve" (this file's), "sample" (the right-hand sides as
    draws, no form) or "factor" (no right-hand sides; refs: name -> reference states)."""
    with open(os.path.join(str(d), "cases.txt"), "w") as f:
        for name, (TF, Tsrc, fl, N, x, P, B, form) in scenes.items():
            if names is not None and name not in names:
                continue
            r = np.zeros((0, x.size)) if refs is None else refs[name]
            last = {"solve": "%d %d" % (B.shape[0], form), "sample": "%d" % B.shape[0], "factor": "%d" % r.shape[0]}[kind]
            f.write("%s %d %d %d %d %s\n" % (name, TF, Tsrc, fl, N, last))
            np.concatenate([x, P.reshape(-1, order="F"), (r if kind == "factor" else B).reshape(-1)]).tofile(os.path.join(str(d), name + ".in"))


def _run(exe, d):
    r = subprocess.run([exe, str(d)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    return r.stdout


def _run_split(exe, d, parts=4):
    """The cases of d/cases.txt dealt out to `parts` processes of the solve emulation that run side by side (a workgroup's lanes are
    threads, and a process runs one workgroup at a time); their outputs joined."""
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
    """(the result block and the pivots, the results, the factor [L 0; W' L_r] in elimination order) of a case of the solve or of the
    sample emulation."""
    TF, _, _, N, x, _, B, _ = scenes[name]
    v = np.fromfile(os.path.join(str(d), name + ".out"))
    rows = -(-2 * N // TF) * TF
    n = x.size
    assert v.size == 16 + rows + B.size + n * n
    head = 16 + rows
    return v[:head], v[head:head + B.size].reshape(B.shape), v[head + B.size:].reshape(n, n)


@pytest.fixture(scope="module")
def emulation(tmp_path_factory):
    d = tmp_path_factory.mktemp("solve_map_emulation")
    scenes = _scenes()
    _write_cases(d, scenes)
    exe = host_build("solve_map_host_emulation", str(d / "emu"), flags=PTHREAD)
    out = _run_split(exe, d)
    print(out)
    return d, out, scenes, exe


@pytest.fixture(scope="module")
def siblings(tmp_path_factory):
    """The sample and the factor emulations, built once."""
    d = tmp_path_factory.mktemp("solve_map_siblings")
    return [host_build(name + "_host_emulation", str(d / name), flags=PTHREAD) for name in ("sample_map", "factor_map")]


@pytest.mark.parametrize("fl", [0, 1])
@pytest.mark.parametrize("TF", [16, 32])
def test_host_emulation_of_the_kernels_against_numpy(emulation, TF, fl):
    """Every size, every k and both forms, the source's tile edge different from the factor's: within the bar of NumPy on the matrix
    as the handle holds it, and of the restatement; the result chunk (packed poisoned) written whole, nothing of the state written."""
    d, out, scenes, _ = emulation
    worst = 0.0
    for N in SIZES:
        for k in S.KS:
            for form, fname in FORM_NAMES:
                name = "spd_F%d_%s_N%d_k%d_%s" % (TF, "f" if fl else "d", N, k, fname)
                assert "%s: 0 differences" % name in out
                _, _, sfl, _, x, P, B, _ = scenes[name]
                H = S.as_held(P, sfl)
                bar = V.bar(H)
                _, got, _ = _output(d, name, scenes)
                err = max(V.rel_err(got, V.expected(H, B, form)), V.rel_err(got, V.solve_dense(x, H, B, form)))
                worst = max(worst, err / bar)
                assert err < bar < REL, (name, err, bar)
    print("edge %d, %s source: worst error against NumPy and the restatement %.3f of the bar" % (TF, "float" if fl else "F64", worst))


@pytest.mark.parametrize("form,fname", FORM_NAMES)
@pytest.mark.parametrize("N", [13, 40])
@pytest.mark.parametrize("TF", [16, 32])
def test_host_emulation_keeps_the_promised_bits(emulation, TF, N, form, fname):
    """B = 0 gives 0 in every entry; a right-hand side gives the same bits alone, and at the start, in the middle and at the end of
    larger batches across chunk boundaries."""
    d, out, scenes, _ = emulation
    names = ["%s_F%d_N%d_%s" % (w, TF, N, fname) for w in ("bits", "alone", "batch")]
    for name in names:
        assert "%s: 0 differences" % name in out
    got = _output(d, names[0], scenes)[1]
    assert not got[0].any()
    alone = _output(d, names[1], scenes)[1][0]
    batch = _output(d, names[2], scenes)[1]
    for row in (got[1], got[3], batch[0], batch[S.CHUNK + 1], batch[-1]):
        np.testing.assert_array_equal(row, alone)
    assert alone.any() and not np.array_equal(got[2], alone)


@pytest.mark.parametrize("TF,N", LOOPS)
def test_host_emulation_closes_the_loops(emulation, siblings, tmp_path, TF, N):
    """HALF of the columns of C that the sample emulation wrote out returns the unit vectors; FULL of the columns of P returns the unit
    vectors; |HALF(x - ref)|^2 is the factor emulation's d2 (heading differences of a few degrees: no wrap).  All within the bar."""
    _, _, _, exe = emulation
    x, s, P = F.spd_scene(N, 100 + N)
    n = x.size
    bar = V.bar(P)
    assert bar < REL
    draw = {"c": (TF, 48 - TF, 0, N, x, P, np.zeros((1, n)), 0)}
    ds = tmp_path / "sample"
    ds.mkdir()
    _write_cases(ds, draw, kind="sample")
    _run(siblings[0], ds)
    C = S.factor_in_x_order(_output(ds, "c", draw)[2])
    refs = F.reference_states(x, 2, 6)
    nu = x[None, :] - refs
    assert np.abs(nu[:, 2]).max() < 90.0
    df = tmp_path / "factor"
    df.mkdir()
    _write_cases(df, draw, kind="factor", refs={"c": refs})
    _run(siblings[1], df)
    d2 = np.fromfile(os.path.join(str(df), "c.out"))[8:10]
    loops = {"half_C": (TF, 48 - TF, 0, N, x, P, C.T.copy(), V.HALF), "full_P": (TF, 48 - TF, 0, N, x, P, P.copy(), V.FULL),
             "half_nu": (TF, 48 - TF, 0, N, x, P, nu, V.HALF)}
    dl = tmp_path / "loops"
    dl.mkdir()
    _write_cases(dl, loops)
    out = _run(exe, dl)
    for name in loops:
        assert "%s: 0 differences" % name in out
    e_c = np.abs(_output(dl, "half_C", loops)[1] - np.eye(n)).max()
    e_p = np.abs(_output(dl, "full_P", loops)[1] - np.eye(n)).max()
    half = _output(dl, "half_nu", loops)[1]
    e_d = V.rel_err(np.sum(half * half, axis=1), d2)
    print("edge %d N=%d: C^-1 C - I %.2e, P^-1 P - I %.2e, |C^-1 nu|^2 against d2 %.2e (bar %.2e)" % (TF, N, e_c, e_p, e_d, bar))
    assert e_c < bar and e_p < bar and e_d < bar


def test_host_emulation_of_a_matrix_that_is_not_definite(emulation, siblings, tmp_path):
    """All-NaN output, and the result block and the pivots bit for bit those of the factor emulation on the same scene -- for the
    scenes that are not definite (a failing pivot in the first tile, in a later tile, in the robot tail) and for two that are."""
    d, out, scenes, _ = emulation
    _write_cases(tmp_path, scenes, INFO_TWINS, kind="factor")
    _run(siblings[1], tmp_path)
    for name in INFO_TWINS:
        assert "%s: 0 differences" % name in out
        block, got, Le = _output(d, name, scenes)
        np.testing.assert_array_equal(block, np.fromfile(os.path.join(str(tmp_path), name + ".out")))
        if name.startswith("spd"):
            assert block[0] == 0.0 and np.isfinite(got).all() and np.isfinite(Le).all()
        else:
            assert block[0] != 0.0 and np.isnan(got).all() and np.isnan(Le).all()


def test_kernel_sources_on_the_host_under_the_sanitizers(tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined runs clean on definite and not-definite scenes per factor
    tile edge: no lane of the new kernels reads or writes outside the chunks, the inverse tiles, the factor store or the state (nothing
    loaded into python is involved)."""
    _write_cases(tmp_path, _scenes(), ("spd_F16_f_N40_k35_full", "spd_F16_d_N16_k17_half", "spd_F32_d_N13_k17_full", "spd_F32_d_N0_k1_half",
                                       "spd_F32_d_N16_k16_full", "neg_third_tile", "neg_last_row", "neg_robot", "known_pose"))
    exe = host_build("solve_map_host_emulation", str(tmp_path / "emulation_sanitized"),
                     flags=["-O1", "-g", "-mfma", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]


def test_the_twin_runs_the_matrix_instructions_k_order():
    """The plain-FMA twin of the sweeps' product and its matrix-core loop name their k index through the same function, chunk_k, in
    the ONE place that holds them, tile_mac of map_blocks.h; both sweeps go through that one product and hold no matrix instruction
    of their own; no atomics anywhere."""
    csrc = os.path.join(ROOT, "ekf_slam_amd", "csrc")
    blocks = open(os.path.join(csrc, "map_blocks.h")).read()
    rest = blocks[blocks.index("void tile_mac("):]
    body = rest[:rest.index("__device__", 1)]                  # up to the next function
    assert body.count("chunk_k(s, t)") == 3 and body.count("chunk_k(s, lr)") == 3
    twin, _, device = body.partition("#else")
    assert "#if defined(EKF_FACTOR_FMA_TWIN)" in twin and "__builtin_amdgcn_mfma" not in twin and "#endif" in device
    assert body.count("__builtin_amdgcn_mfma") == 1 and "__builtin_amdgcn_mfma_f64_16x16x4f64(av[s], bv[s], acc, 0, 0, 0)" in device
    assert "__builtin_amdgcn_mfma" not in blocks.replace(body, "")
    src = open(os.path.join(csrc, "solve_map.h")).read()
    assert "__builtin_amdgcn_mfma" not in src and "EKF_FACTOR_FMA_TWIN" not in src
    fwd = src[src.index("void k_solve_forward("):src.index("void k_solve_tail(")]
    bwd = src[src.index("void k_solve_backward("):]
    assert fwd.count("tile_mac<TF, false, ") == 2 and bwd.count("tile_mac<TF, true, ") == 2
    assert fwd.count("tile_mac<") == 2 and bwd.count("tile_mac<") == 2
    assert fwd.count("__syncthreads()") == 2 and bwd.count("__syncthreads()") == 2
    assert "atomic" not in src.split("// -----")[-1] and "atomic" not in blocks.split("// -----")[-1]


# ------------------------------------------------------------------------------------------------------------------
# the Python layers over a stand-in for the library
# ------------------------------------------------------------------------------------------------------------------
X7 = np.array([1.0, -2.0, 30.0, 4.0, 5.0, -3.0, 6.0])


def _p7():
    A = np.random.default_rng(21).normal(0.0, 0.3, (7, 7))
    return A @ A.T + 0.2 * np.eye(7)


class _Recorder(RecorderBase):
    """ekf_solve_map as the NumPy restatement on a fixed two-landmark Gaussian."""
    status_string = b"invalid argument"
    last_error = b"solve_map: not built for sharded handles (world > 1): injected"

    def __init__(self):
        self.calls, self.fail, self.N, self.definite, self.P = [], 0, 2, 1, _p7()

    def ekf_num_landmarks(self, h, pn):
        pn._obj.value = self.N
        return 0

    def ekf_solve_map(self, h, form, B, k, out, info):
        assert isinstance(k, ctypes.c_int64) and isinstance(form, ctypes.c_int32)      # marshalled once, by marshal.solve_args
        n = 3 + 2 * self.N
        rhs = np.array([B[i] for i in range(k.value * n)]).reshape(k.value, n)
        self.calls.append(("solve_map", h.value, form.value, rhs))
        if self.fail:
            return self.fail
        info._obj.n, info._obj.definite, info._obj.bad_index, info._obj.logdet = n, self.definite, -1 if self.definite else 4, -3.5
        res = V.solve_dense(X7, self.P, rhs, form.value) if self.definite else np.full((k.value, n), np.nan)
        for i, v in enumerate(res.reshape(-1)):
            out[i] = v
        return 0


def test_layers_marshal_a_solve_once(monkeypatch):
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import engine as E
    from ekf_slam_amd import marshal
    from ekf_slam_amd import slam as SL
    from ekf_slam_amd.sharding import ShardGroup
    from ekf_slam_amd.trajectory import TrajectoryLog
    assert L.SIGNATURES["ekf_solve_map"] == (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32, dp, ctypes.c_int64, dp, ctypes.POINTER(L.EkfFactorInfo)])
    header = open(os.path.join(ROOT, "include", "ekfslam.h")).read()
    assert "int32_t ekf_solve_map(ekf_handle *h, int32_t form, const double *B" in header and "enum { EKF_SOLVE_FULL = 0, EKF_SOLVE_HALF = 1 };" in header
    assert "STREAM ORDER IS THE ONLY ORDER" in header and "NO entry is wrapped" in header
    assert marshal.SOLVE_FORMS == V.FORMS
    rec = _Recorder()
    monkeypatch.setattr(L, "lib", lambda: rec)
    made = []
    real = marshal.solve_args
    monkeypatch.setattr(marshal, "solve_args", lambda *a, **k: made.append(a) or real(*a, **k))
    g = E.Engine(capacity=32, tile=16)
    one = np.arange(7.0) / 7.0
    out, info = g.solve_map(one)
    assert len(rec.calls) == 1 and len(made) == 1 and rec.calls[0][1] == g.h.value and rec.calls[0][2] == V.FULL
    np.testing.assert_array_equal(rec.calls[0][3], one[None, :])
    np.testing.assert_array_equal(out, V.solve_dense(X7, rec.P, one, V.FULL))
    assert out.shape == (1, 7) and out.dtype == np.float64 and out.flags["C_CONTIGUOUS"]
    assert sorted(info) == sorted(F.KEYS) and info["definite"] is True and info["n"] == 7 and info["bad_index"] == -1
    five = np.asfortranarray(np.random.default_rng(2).standard_normal((5, 7)).astype(np.float32))      # neither F64 nor C-contiguous
    out, info = g.solve_map(five, form="half")
    np.testing.assert_array_equal(rec.calls[-1][3], five.astype(np.float64))
    np.testing.assert_array_equal(out, V.solve_dense(X7, rec.P, five.astype(np.float64), V.HALF))
    assert out.shape == (5, 7) and len(made) == 2 and rec.calls[-1][2] == V.HALF
    # the refusals, in marshal, before anything is sent
    ncalls = len(rec.calls)
    bad_nan = one.copy()
    bad_nan[4] = np.nan
    for B in (None, np.zeros((0, 7)), np.zeros(6), np.zeros((2, 9)), bad_nan, np.full((2, 7), np.inf), np.zeros((2, 1, 7))):
        with pytest.raises(ValueError) as err:
            g.solve_map(B)
        assert "solve_map" in str(err.value)
    for form in ("quarter", 0, None):
        with pytest.raises(ValueError) as err:
            g.solve_map(one, form)
        assert "solve_map" in str(err.value) and "form" in str(err.value)
    assert len(rec.calls) == ncalls
    # the library's refusal raises; a shard group hands the call to its first shard so that the refusal is the library's
    rec.fail = L.EKF_ERR_INVALID_ARG
    with pytest.raises(L.EkfError) as err:
        g.solve_map(one)
    assert err.value.status == L.EKF_ERR_INVALID_ARG and "solve_map" in str(err.value)
    grp = ShardGroup(2, capacity=16)
    with pytest.raises(L.EkfError) as err:
        grp.solve_map(one, "half")
    assert rec.calls[-1][0] == "solve_map" and rec.calls[-1][1] == grp.shards[0].h.value and "sharded" in str(err.value)
    rec.fail = 0
    # the policy layer: one call each, nothing logged
    for cls in (SL.EKF_SLAM, SL.EKF_SLAM_UC):
        rec.calls.clear()
        del made[:]
        f = cls(capacity=32, tile=64)
        f.log = TrajectoryLog()
        a, _ = f.solve_map(five, "half")
        np.testing.assert_array_equal(rec.calls[-1][3], five.astype(np.float64))
        f.information_columns([1])
        np.testing.assert_array_equal(rec.calls[-1][3], np.eye(7)[5:7])
        f.mahalanobis(X7, X7 + 1.0)
        assert len(rec.calls) == 3 and len(made) == 3 and len(f.log.edits) == 0
        assert [c[2] for c in rec.calls] == [V.HALF, V.FULL, V.HALF]


def test_the_three_policies_against_closed_forms(monkeypatch):
    """On a two-landmark Gaussian, the stand-in library being the NumPy restatement: information_columns against inv(P)[:, cols],
    conditional_covariance against the Schur complement P_AA - P_AB inv(P_BB) P_BA, mahalanobis with a heading pair that straddles
    +-180 (179 against -179: a difference of -2, not 358)."""
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import slam as SL
    rec = _Recorder()
    monkeypatch.setattr(L, "lib", lambda: rec)
    P = rec.P
    bar = V.bar(P)
    Lam = np.linalg.inv(P)
    f = SL.EKF_SLAM(capacity=32, tile=64)
    rob = f.information_columns()
    assert rob.shape == (7, 3) and V.rel_err(rob, Lam[:, :3]) < bar
    both = f.information_columns([1, 0])
    assert both.shape == (7, 4) and V.rel_err(both, Lam[:, [5, 6, 3, 4]]) < bar
    assert len(rec.calls) == 2 and all(c[2] == V.FULL for c in rec.calls)
    for idx, A, Bc in (([1], [5, 6], [0, 1, 2, 3, 4]), ([1, 0], [5, 6, 3, 4], [0, 1, 2])):
        schur = P[np.ix_(A, A)] - P[np.ix_(A, Bc)] @ np.linalg.solve(P[np.ix_(Bc, Bc)], P[np.ix_(Bc, A)])
        cc = f.conditional_covariance(idx)
        assert cc.shape == schur.shape and V.rel_err(cc, schur) < bar * np.linalg.cond(schur) < REL
        np.testing.assert_array_equal(cc, cc.T)
        assert np.all(np.linalg.eigvalsh(P[np.ix_(A, A)] - cc) > -1e-12)             # conditioning never adds uncertainty
    a, b = X7.copy(), X7 + np.array([0.3, -0.2, 0.0, 0.1, 0.4, -0.5, 0.2])
    a[2], b[2] = 179.0, -179.0
    d = a - b
    d[2] = -2.0
    want = float(d @ Lam @ d)
    ncalls = len(rec.calls)
    got = f.mahalanobis(a, b)
    assert abs(got - want) < bar * want and len(rec.calls) == ncalls + 1 and rec.calls[-1][2] == V.HALF
    assert rec.calls[-1][3][0, 2] == -2.0
    unwrapped = a - b
    assert abs(got - float(unwrapped @ Lam @ unwrapped)) > 1.0                      # (358 degrees would have been another number)
    assert abs(f.mahalanobis(b, a) - want) < bar * want and rec.calls[-1][3][0, 2] == 2.0
    # refusals of the policies, before any call; a P that is not definite raises and names factor_map
    ncalls = len(rec.calls)
    for call in (lambda: f.information_columns([2]), lambda: f.information_columns([0, 0]), lambda: f.information_columns([]),
                 lambda: f.conditional_covariance(None), lambda: f.mahalanobis(a, b[:5])):
        with pytest.raises(ValueError):
            call()
    assert len(rec.calls) == ncalls
    rec.definite = 0
    for call in (lambda: f.information_columns(), lambda: f.conditional_covariance([0]), lambda: f.mahalanobis(a, b)):
        with pytest.raises(ValueError) as err:
            call()
        assert "factor_map" in str(err.value)


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
int32_t ekf_solve_map(ekf_handle *h, int32_t form, const double *B, int64_t k, double *out, ekf_factor_info *info) {
    int64_t N;
    ekf_num_landmarks(h, &N);
    const int64_t n = 3 + 2 * N;
    printf("ABI ekf_solve_map form=%d k=%d B0=%g BLast=%g\n", (int)form, (int)k, B[0], B[k * n - 1]);
    if (fail_armed) { fail_armed = 0; stub_fail_next(h); return ekf_flush(h); }
    info->n = n; info->definite = 1; info->bad_index = -1; info->bad_pivot = 0.0; info->logdet = -1.5; info->logdet_map = -2.5;
    info->min_pivot = 0.25; info->max_pivot = 4.0;
    for (int64_t i = 0; i < k * n; ++i) out[i] = (form ? 200.0 : 100.0) + B[i];
    return EKF_OK;
}
'''

_DRIVER = driver(r'''
    const mxArray *sx[3] = { mock_string("set_x"), h, mock_double(7, 1, (const double[]){ 1, 2, 3, 4, 5, 6, 7 }) };
    if (call("set_x", 0, 3, sx)) return 1;
    const mxArray *two = mock_double(7, 2, (const double[]){ 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14 });
    const mxArray *sm[4] = { mock_string("solve_map"), h, two, mock_double(1, 1, (const double[]){ 0 }) };
    if (call("solve_map", 2, 4, sm)) return 1;
    if (call("solve_map one_output", 1, 4, sm)) return 1;
    const mxArray *hf[4] = { sm[0], h, two, mock_double(1, 1, (const double[]){ 1 }) };
    if (call("solve_map half", 2, 4, hf)) return 1;
    if (!call("solve_map", 2, 3, sm)) return 1;
    const mxArray *bad[4] = { sm[0], h, mock_double(5, 1, (const double[]){ 1, 2, 3, 4, 5 }), sm[3] };
    if (!call("solve_map badsize", 2, 4, bad)) return 1;
    bad[2] = mock_double(0, 0, (const double[]){ 0 });
    if (!call("solve_map empty", 2, 4, bad)) return 1;
    arm_failure();
    if (!call("solve_map", 2, 4, sm)) return 1;
''', PRELUDE_SHOWN)

_DRIVER_WITHOUT = driver_without(r'''
    const mxArray *sm[4] = { mock_string("solve_map"), h, mock_double(7, 1, (const double[]){ 1, 2, 3, 4, 5, 6, 7 }), mock_double(1, 1, (const double[]){ 0 }) };
    if (!call("solve_map", 1, 4, sm)) return 1;
''')


def test_mex_gateway_reaches_the_abi(tmp_path):
    t = transcript_of(tmp_path, _STUB, _DRIVER)
    i = t.index("ABI ekf_solve_map form=0 k=2 B0=1 BLast=14")
    assert t[i + 1] == "MEX solve_map nrhs=4 -> ok out0=7x2[101,102,103,104,105,106,107,108,109,110,111,112,113,114] out1=1x8[7,1,0,0,-1.5,-2.5,0.25,4]"
    assert any(ln.startswith("MEX solve_map one_output nrhs=4 -> ok out0=7x2[") and "out1" not in ln for ln in t)
    j = t.index("ABI ekf_solve_map form=1 k=2 B0=1 BLast=14")
    assert t[j + 1].startswith("MEX solve_map half nrhs=4 -> ok out0=7x2[201,202,")
    assert any(ln.startswith("MEX solve_map nrhs=3 -> ERROR ekfslam:usage") and "needs 4 arguments" in ln for ln in t)
    for name in ("badsize", "empty"):
        assert any(ln.startswith("MEX solve_map %s nrhs=4 -> ERROR ekfslam:usage" % name) and "B is n x k" in ln for ln in t), name
    assert sum(ln.startswith("ABI ekf_solve_map") for ln in t) == 4             # the three good calls and the injected failure
    assert "MEX solve_map nrhs=4 -> ERROR ekfslam:status | call not valid in the current state: injected failure" in t
    assert t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_the_gateway_still_links_against_a_library_without_the_symbol(tmp_path):
    t = transcript_of(tmp_path, _DRIVER_WITHOUT)
    assert any(ln.startswith("MEX solve_map ") and "ERROR ekfslam:usage" in ln and "this libekfslam has no ekf_solve_map" in ln for ln in t)
    assert "MEX predict nrhs=3 -> ok" in t and t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_matlab_method_and_documents_name_the_call():
    text = open(os.path.join(ROOT, "matlab", "EKF_SLAM.m")).read()
    m = re.search(r"function\s+\[out,\s*info\]\s*=\s*solveMap\(h,\s*B,\s*form\)(.*?)\n        end\b", text, re.S)
    assert m and "h.gateway('solve_map', double(B), double(strcmp(form, 'half')));" in m.group(1)
    src = open(os.path.join(ROOT, "matlab", "ekfslam_mex.c")).read()
    assert src.count('strcmp(cmd, "solve_map")') == 1 and "#pragma weak ekf_solve_map" in src
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        body = open(os.path.join(ROOT, doc)).read()
        assert "solve_map" in body, doc
    assert "solveMap" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for kernel in ("k_solve_invert", "k_solve_forward", "k_solve_tail", "k_solve_backward"):
        assert kernel in design, kernel
    assert "3y" in design
