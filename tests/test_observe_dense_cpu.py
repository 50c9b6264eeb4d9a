"""CPU: what ekf_observe_dense needs checked without a GPU (include/ekfslam.h) -- NumPy alone inside the derived
bars of tests/observe_dense_cases.py; the Python layers over a stand-in for the library (one marshalling per call, the refusals in the
ABI's order, the three policies and their chi-square gate); the trajectory log (format 13 only where needed, older formats still load, a
replay sends what was sent); the header, the binding and the documents; the MEX gateway under the mock; the kernel sources of
k_dense_gram, k_dense_factor and k_gather_dense compiled for the host (tests/support/observe_dense_host_emulation.cpp) against the
restatement."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

import observe_dense_cases as C
from helpers import ROOT, RecorderBase

dp = ctypes.POINTER(ctypes.c_double)


# ------------------------------------------------------------------------------------------------------------------
# the bars
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 96, 140])
@pytest.mark.parametrize("k", C.KS)
def test_numpy_alone_stays_inside_every_bar(N, k):
    """float64 NumPy against the same expressions in extended precision: well inside the bars that allow for TWO float64 sides."""
    rng = np.random.default_rng(N + k)
    n = 3 + 2 * N
    A = rng.normal(0.0, 0.3, (n, 6))
    P = A @ A.T + np.diag(rng.uniform(0.05, 0.2, n))
    x = rng.normal(0.0, 20.0, n)
    for H in [C.gaussian_H(k, n, 10 + k)] + ([C.centroid_H(n), C.displacement_H(n, C.spread_pairs(N, 3))] if k == 2 and N >= 96 else []):
        H, z, R = C.scene(x, P, H)
        nu, S = C.innovation_dense(x, P, H, z, R)
        assert np.linalg.cond(S) <= C.COND_MAX
        ld = np.longdouble
        Hl, Pl, xl = H.astype(ld), P.astype(ld), x.astype(ld)
        Sl, nul = Hl @ (Pl @ Hl.T) + R.astype(ld), z.astype(ld) - Hl @ xl
        d2l = float(nul @ np.linalg.solve(Sl.astype(np.float64), nul.astype(np.float64)))        # (the solve itself is what 64 cond u allows for)
        rS = C.ratio((S - Sl).astype(np.float64), C.S_bar(P, H, S))
        rnu = C.ratio((nu - nul).astype(np.float64), C.nu_bar(x, H, nu))
        d2 = float(nu @ np.linalg.solve(S, nu))
        rd2 = abs(d2 - d2l) / d2 / C.d2_bar(x, P, H, nu, S)
        assert rS <= 0.5 and rnu <= 0.5 and rd2 <= 0.5, (rS, rnu, rd2)
        # ... and the restatement's update is the textbook one
        xn, Pn, rec = C.update_dense(x, P, H, z, R)
        K = P @ H.T @ np.linalg.inv(S)
        assert np.abs(xn - (x + K @ nu)).max() <= 1e-9 * np.abs(x).max() and np.abs(Pn - (P - K @ H @ P)).max() <= 1e-9 * np.abs(P).max()
        assert rec["outcome"] == C.APPLIED and abs(rec["d2"] - d2) <= 1e-9 * d2
        # an odd k written out with the empty row is the same update
        Hp, zp, Rp = C.padded(H, z, R)
        xp, Pp, recp = C.update_dense(x, P, Hp, zp, Rp)
        assert np.abs(xp - xn).max() <= 1e-12 * np.abs(x).max() and np.abs(Pp - Pn).max() <= 1e-12 * np.abs(P).max() and abs(recp["d2"] - rec["d2"]) <= 1e-12 * d2


def test_the_restatement_gates_and_finds_the_singular_pivot():
    n = 7
    A = np.random.default_rng(1).normal(0.0, 0.3, (n, n))
    P, x = A @ A.T + 0.2 * np.eye(n), np.arange(7.0)
    H, z, R = C.scene(x, P, C.gaussian_H(3, n, 2))
    d2 = C.update_dense(x, P, H, z, R)[2]["d2"]
    xg, Pg, rec = C.update_dense(x, P, H, z, R, gate=0.5 * d2)
    assert rec["outcome"] == C.GATED and rec["d2"] == d2 and np.array_equal(xg, x) and np.array_equal(Pg, P)
    c = next(c for c in range(3, n) if C.singular_pivot_is_not_positive(P[c, c]))
    Hs = np.zeros((2, n)); Hs[:, c] = 1.0
    _, _, rec = C.update_dense(x, P, Hs, [1.0, 1.0], np.zeros((2, 2)))
    assert (rec["outcome"], rec["bad_row"]) == (C.IRREGULAR, 1)


# ------------------------------------------------------------------------------------------------------------------
# the Python layers over a stand-in for the library
# ------------------------------------------------------------------------------------------------------------------
def _p7():
    A = np.random.default_rng(21).normal(0.0, 0.3, (7, 7))
    return A @ A.T + 0.2 * np.eye(7)


class _Recorder(RecorderBase):
    """ekf_observe_dense as the NumPy restatement on a two-landmark Gaussian that the call updates."""
    status_string = b"call not valid in the current state"
    last_error = b"observe_dense: row 1: the pivot of S = H P H' + R is not finite and positive"

    def __init__(self):
        self.calls, self.N, self.P, self.x = [], 2, _p7(), np.array([1.0, -2.0, 30.0, 4.0, 5.0, -6.0, 7.0])

    def ekf_num_landmarks(self, h, pn):
        pn._obj.value = self.N
        return 0

    def _run(self, name, H, k, z, R, wrap, gate, res, nu, S, apply):
        assert isinstance(k, int) and not isinstance(H, np.ndarray)                     # marshalled once, by marshal.dense_args
        n = 3 + 2 * self.N
        Hv = np.array([H[i] for i in range(k * n)]).reshape(k, n)
        zv, Rv = np.array([z[i] for i in range(k)]), np.array([R[i] for i in range(k * k)]).reshape(k, k).T
        wv = None if wrap is None else [int(wrap[i]) for i in range(k)]
        self.calls.append((name, Hv, zv, Rv, wv, gate))
        xn, Pn, rec = C.update_dense(self.x, self.P, Hv, zv, Rv, gate, wv)
        r = res._obj
        r.d2, r.rows, r.outcome, r.bad_row = rec["d2"], k, rec["outcome"], rec["bad_row"]
        for i in range(k):
            nu[i] = rec["nu"][i]
            for j in range(k):
                S[i + j * k] = rec["S"][i, j]
        if apply and rec["outcome"] == C.IRREGULAR:
            return 7                                            # EKF_ERR_STATE
        if apply:
            self.x, self.P = xn, Pn
        return 0

    def ekf_observe_dense(self, h, H, k, z, R, wrap, gate, res, nu, S):
        return self._run("observe_dense", H, k, z, R, wrap, gate, res, nu, S, True)

    def ekf_observe_dense_innovation(self, h, H, k, z, R, wrap, res, nu, S):
        return self._run("dense_innovation", H, k, z, R, wrap, C.INF, res, nu, S, False)


def _engine(monkeypatch):
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import engine as E
    rec = _Recorder()
    monkeypatch.setattr(L, "lib", lambda: rec)
    return rec, E.Engine(capacity=32, tile=16)


def test_the_binding_and_the_header_agree():
    from ekf_slam_amd import _lib as L
    i32p = ctypes.POINTER(ctypes.c_int32)
    resp = ctypes.POINTER(L.EkfObserveDenseResult)
    assert L.SIGNATURES["ekf_observe_dense"] == (ctypes.c_int32, [ctypes.c_void_p, dp, ctypes.c_int64, dp, dp, i32p, ctypes.c_double, resp, dp, dp])
    assert L.SIGNATURES["ekf_observe_dense_innovation"] == (ctypes.c_int32, [ctypes.c_void_p, dp, ctypes.c_int64, dp, dp, i32p, resp, dp, dp])
    assert ctypes.sizeof(L.EkfObserveDenseResult) == 24 and L.EKF_DENSE_MAX == 16
    header = open(os.path.join(ROOT, "include", "ekfslam.h")).read()
    assert "#define EKF_DENSE_MAX 16" in header and "int32_t ekf_observe_dense(ekf_handle *h, const double *H" in header
    assert "ekf_observe_dense_innovation(ekf_handle *h" in header
    host = open(os.path.join(ROOT, "ekf_slam_amd", "csrc", "host", "dense_obs.h")).read()
    assert "EKF_DENSE_MAX == kFactorChunk" in host and "EKF_DENSE_MAX <= 2 * EKF_MERGE_BATCH_MAX" in host


def test_layers_marshal_an_observation_once_and_refuse_in_the_abis_order(monkeypatch):
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import marshal
    rec, g = _engine(monkeypatch)
    made = []
    real = marshal.dense_args
    monkeypatch.setattr(marshal, "dense_args", lambda *a, **k: made.append(a) or real(*a, **k))
    x0, P0 = rec.x.copy(), rec.P.copy()
    H = np.asfortranarray(np.random.default_rng(2).standard_normal((3, 7)).astype(np.float32))      # neither F64 nor C-contiguous
    z, R = [0.5, -1.0, 2.0], np.diag([0.1, 0.2, 0.3])
    probe = g.dense_innovation(H, z, R, wrap_deg=[0, 1, 0])
    assert rec.calls[-1][0] == "dense_innovation" and rec.calls[-1][4] == [0, 1, 0] and np.array_equal(rec.x, x0)
    got = g.observe_dense(H, z, R, wrap_deg=[0, 1, 0])
    assert len(rec.calls) == 2 and len(made) == 2
    np.testing.assert_array_equal(rec.calls[-1][1], H.astype(np.float64))
    np.testing.assert_array_equal(rec.calls[-1][3], R)
    want = C.update_dense(x0, P0, H.astype(np.float64), z, R, wrap_deg=[0, 1, 0])[2]
    for key in ("d2", "rows", "outcome", "bad_row"):
        assert got[key] == want[key] == probe[key], key
    np.testing.assert_array_equal(got["nu"], want["nu"])
    np.testing.assert_array_equal(got["S"], want["S"])
    # the sparse form of H, the diagonal of R, one row
    g.observe_dense([{0: 1.0, 5: -2.0}, {6: 0.5}], [1.0, 2.0], [0.1, 0.2])
    Hs = np.zeros((2, 7)); Hs[0, 0], Hs[0, 5], Hs[1, 6] = 1.0, -2.0, 0.5
    np.testing.assert_array_equal(rec.calls[-1][1], Hs)
    np.testing.assert_array_equal(rec.calls[-1][3], np.diag([0.1, 0.2]))
    g.observe_dense(np.arange(7.0), [1.0], 0.5)
    assert rec.calls[-1][1].shape == (1, 7) and rec.calls[-1][3].shape == (1, 1) and rec.calls[-1][4] is None
    # the refusals, in marshal, before anything is sent -- and in the ABI's order: k, z, R (finite, symmetric, diagonal), the gate, H
    ncalls = len(rec.calls)
    ok_H, ok_z, ok_R = np.ones((2, 7)), [0.0, 0.0], np.eye(2)
    nanH, nanz = np.full((2, 7), np.nan), [np.nan, 0.0]
    ladder = [((np.ones((17, 7)), np.full(17, np.nan), np.eye(17)), {}, "between 1 and 16"),
              ((np.ones((0, 7)), [], np.zeros((0, 0))), {}, "between 1 and 16"),
              ((nanH, [0.0], -np.eye(2)), dict(gate=np.nan), "one value per row"),
              ((nanH, nanz, -np.eye(2)), dict(gate=np.nan), "z is not finite"),
              ((nanH, ok_z, np.eye(3)), dict(gate=np.nan), "R is k x k"),
              ((nanH, ok_z, [[np.inf, 1.0], [0.0, -1.0]]), dict(gate=np.nan), "R is not finite"),
              ((nanH, ok_z, [[1.0, 1e-3], [0.0, -1.0]]), dict(gate=np.nan), "not symmetric"),
              ((nanH, ok_z, -np.eye(2)), dict(gate=np.nan), "negative diagonal"),
              ((nanH, ok_z, ok_R), dict(gate=np.nan), "gate is NaN"),
              ((nanH, ok_z, ok_R), {}, "H is not finite"),
              ((ok_H, ok_z, ok_R), dict(wrap_deg=[1]), "one flag per row"),
              ((np.ones((2, 6)), ok_z, ok_R), {}, "k x 7"),
              (([{7: 1.0}], [0.0], [1.0]), {}, "outside 0 .. 6")]
    for args, kw, word in ladder:
        with pytest.raises(ValueError) as err:
            g.observe_dense(*args, **kw)
        assert "observe_dense" in str(err.value) and word in str(err.value), (word, str(err.value))
    with pytest.raises(ValueError) as err:
        g.dense_innovation(nanH, ok_z, ok_R)
    assert "dense_innovation" in str(err.value)
    assert len(rec.calls) == ncalls
    # the library's refusal raises with its message; R = 0 is sent, not refused
    c = next(c for c in range(3, 7) if C.singular_pivot_is_not_positive(rec.P[c, c]))
    with pytest.raises(L.EkfError) as err:
        g.observe_dense([{c: 1.0}, {c: 1.0}], [0.0, 0.0], np.zeros((2, 2)))
    assert "observe_dense" in str(err.value) and len(rec.calls) == ncalls + 1


def test_the_three_policies_and_their_chi_square_gate(monkeypatch):
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import slam as SL
    from ekf_slam_amd.trajectory import TrajectoryLog
    rec = _Recorder()
    monkeypatch.setattr(L, "lib", lambda: rec)
    f = SL.EKF_SLAM(capacity=32, tile=64)
    f.log = TrajectoryLog()
    # fix_centroid: two rows of weights 1 / m over the group's x and y entries
    x0 = rec.x.copy()
    res = f.fix_centroid([1, 0], [4.0, 1.0], 0.1 * np.eye(2))
    Hc = np.zeros((2, 7)); Hc[0, [3, 5]] = 0.5; Hc[1, [4, 6]] = 0.5
    np.testing.assert_array_equal(rec.calls[-1][1], Hc)
    assert rec.calls[-1][5] == C.INF and res["outcome"] == C.APPLIED and not np.array_equal(rec.x, x0)
    # the gate of a policy: the chi-square quantile for its rows; a far reading is gated and changes nothing
    x1 = rec.x.copy()
    res = f.fix_centroid([0, 1], [400.0, 100.0], 0.1 * np.eye(2), p=0.99)
    assert rec.calls[-1][5] == SL.chi2_quantile(0.99, 2) and abs(rec.calls[-1][5] - 9.2103403719761836) < 1e-9
    assert res["outcome"] == C.GATED and res["d2"] > rec.calls[-1][5] and np.array_equal(rec.x, x1)
    # constrain_displacements: two rows per pair, +1 on i and -1 on j; one shared 2 x 2 R becomes the block diagonal
    f.constrain_displacements([(1, 0)], [1.0, -1.0], 0.2 * np.eye(2), p=0.5)
    np.testing.assert_array_equal(rec.calls[-1][1], C.displacement_H(7, [(1, 0)]))
    assert rec.calls[-1][5] == SL.chi2_quantile(0.5, 2)
    # condition_on: unit rows, R = 0; the landmark takes the value and its rows of P vanish
    res = f.condition_on([1], [10.0, -10.0])
    np.testing.assert_array_equal(rec.calls[-1][1], np.eye(7)[5:7])
    assert not rec.calls[-1][3].any() and res["outcome"] == C.APPLIED
    assert np.abs(rec.x[5:7] - [10.0, -10.0]).max() < 1e-12 and np.abs(rec.P[5:7]).max() < 1e-12
    # every applied or gated call is logged as one edit; the innovation is not
    f.dense_innovation(np.ones((1, 7)), [0.0], [1.0])
    assert [ed[1] for ed in f.log.edits] == ["observe_dense"] * 4
    # refusals of the policies, before any call
    ncalls = len(rec.calls)
    for call in (lambda: f.fix_centroid([2], [0, 0], np.eye(2)), lambda: f.fix_centroid([0, 0], [0, 0], np.eye(2)),
                 lambda: f.fix_centroid([0], [0, 0], np.eye(2), p=1.0), lambda: f.constrain_displacements([(0, 0)], [0, 0], np.eye(2)),
                 lambda: f.constrain_displacements([(0, 2)], [0, 0], np.eye(2)), lambda: f.constrain_displacements([(0, 1)], [0, 0, 0], np.eye(2)),
                 lambda: f.constrain_displacements([], [], np.eye(2)), lambda: f.condition_on([0], [1.0]), lambda: f.condition_on([5], [1.0, 2.0])):
        with pytest.raises(ValueError):
            call()
    assert len(rec.calls) == ncalls


# ------------------------------------------------------------------------------------------------------------------
# the trajectory log
# ------------------------------------------------------------------------------------------------------------------
def test_log_round_trip_and_format_13_only_where_needed(monkeypatch, tmp_path):
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import slam as SL
    from ekf_slam_amd import trajectory as T
    assert T.FORMAT_OBSERVE_DENSE == T._FORMATS_ON_DISK[12] == "ekfslam-trajectory-13" and len(T._FORMATS_ON_DISK) == 13
    assert len(T._EVERY_FORMAT) == 12 and len(T._ALL_FORMATS) == 11 and len(T._FORMATS) == 10          # the older tuples keep their contents
    assert T._KINDS[-1] == T.TRANSFORM_MAP and T._KINDS_ON_DISK == T._KINDS + (T.OBSERVE_DENSE,) and T._KIND[T.OBSERVE_DENSE].format == 13
    rec = _Recorder()
    monkeypatch.setattr(L, "lib", lambda: rec)
    f = SL.EKF_SLAM(capacity=32, tile=64)
    f.log = T.TrajectoryLog()
    H = np.zeros((3, 7)); H[0, [0, 5]] = [1.0, -2.0]; H[2, 6] = 0.25              # row 1 is empty
    f.observe_dense(H, [1.0, 0.0, 2.0], np.diag([0.1, 1.0, 0.3]), gate=50.0, wrap_deg=[0, 0, 1])
    f.condition_on([0], [3.0, 4.0])
    sent = [c for c in rec.calls if c[0] == "observe_dense"]
    f.log.record([0.1, 1.0], None, [], [])
    path = tmp_path / "dense.npz"
    f.log.save(path)
    g = np.load(path)
    assert str(g["format"]) == T.FORMAT_OBSERVE_DENSE
    np.testing.assert_array_equal(g["dense_row"], [0, 0, 2, 0, 1])                  # H travels as triplets: five non-zero entries in all
    np.testing.assert_array_equal(g["dense_col"], [0, 5, 6, 3, 4])
    np.testing.assert_array_equal(g["dense_val"], [1.0, -2.0, 0.25, 1.0, 1.0])
    log = T.TrajectoryLog.load(path)
    assert [ed[1] for ed in log.edits] == ["observe_dense"] * 2 and len(log.dense_observations) == 2
    o = log.dense_observations[0]
    assert (o["rows"], o["n"], o["gate"]) == (3, 7, 50.0) and o["R"].shape == (3, 3) and list(o["wrap"]) == [0, 0, 1]

    class _Replayed:
        def __init__(self):
            self.calls = []

        def observe_dense(self, H, z, R, gate, wrap_deg):
            self.calls.append((np.asarray(H), np.asarray(z), np.asarray(R), gate, list(wrap_deg)))

        def predict(self, u):
            pass

    r = _Replayed()
    log.replay(r)
    assert len(r.calls) == 2
    for (Hr, zr, Rr, gr, wr), (_, Hs, zs, Rs, ws, gs) in zip(r.calls, sent):
        np.testing.assert_array_equal(Hr, Hs); np.testing.assert_array_equal(zr, zs); np.testing.assert_array_equal(Rr, Rs)
        assert gr == gs and wr == (ws if ws is not None else [0] * len(zs))
    # a log without such an edit is written in the format it always was, and every older fixture still loads
    plain = T.TrajectoryLog()
    plain.record([0.1, 1.0], None, [], [])
    plain.save(tmp_path / "plain.npz")
    assert str(np.load(tmp_path / "plain.npz")["format"]) == T.FORMAT
    plain.record_edit("remove", [1])
    plain.save(tmp_path / "edit.npz")
    assert str(np.load(tmp_path / "edit.npz")["format"]) == T.FORMAT_EDITS
    fixtures = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "trajectory", "format*.npz")))
    assert len(fixtures) >= 10
    for fx in fixtures:
        old = T.TrajectoryLog.load(fx)
        assert not old.dense_observations
        n = int(re.search(r"format(\d+)\.npz", fx).group(1))
        assert str(np.load(fx)["format"]) == T._FORMATS_ON_DISK[n - 1]


def test_the_documents_name_the_call():
    for doc in ("README.md", "DESIGN.md"):
        body = open(os.path.join(ROOT, doc)).read()
        assert "ekf_observe_dense" in body and "observe_dense_innovation" in body, doc
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "k_dense_gram" in design and "k_dense_factor" in design and "k_gather_dense" in design
    for out_of_scope in ("Sharded handles", "k > 16", "pending ring", "row-panels", "nonlinear dense model"):
        assert out_of_scope in design, out_of_scope


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
int32_t ekf_observe_dense(ekf_handle *h, const double *H, int64_t k, const double *z, const double *R, const int32_t *wrap_deg, double gate,
                          ekf_observe_dense_result *res, double *nu, double *S) {
    int64_t N;
    ekf_num_landmarks(h, &N);
    const int64_t n = 3 + 2 * N;
    printf("ABI ekf_observe_dense k=%d H0=%g HLast=%g z0=%g RLast=%g gate=%g wrap=%d\n", (int)k, H[0], H[k * n - 1], z[0], R[k * k - 1], gate,
           wrap_deg ? (int)wrap_deg[k - 1] : -1);
    if (fail_armed) { fail_armed = 0; stub_fail_next(h); return ekf_flush(h); }
    res->d2 = 2.5; res->rows = (int32_t)k; res->outcome = EKF_LINEAR_APPLIED; res->bad_row = -1;
    for (int64_t i = 0; i < k; ++i) nu[i] = 10.0 + z[i];
    for (int64_t i = 0; i < k * k; ++i) S[i] = 100.0 + R[i];
    return EKF_OK;
}
'''

def _drivers():
    from mex_harness import PRELUDE_SHOWN, driver, driver_without
    body = r'''
    const mxArray *sx[3] = { mock_string("set_x"), h, mock_double(7, 1, (const double[]){ 1, 2, 3, 4, 5, 6, 7 }) };
    if (call("set_x", 0, 3, sx)) return 1;
    const mxArray *H = mock_double(7, 2, (const double[]){ 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14 });
    const mxArray *od[7] = { mock_string("observe_dense"), h, H, mock_double(2, 1, (const double[]){ 0.5, -0.5 }),
                             mock_double(2, 2, (const double[]){ 1, 0, 0, 2 }), D1(9.25), mock_double(2, 1, (const double[]){ 0, 1 }) };
    if (call("observe_dense", 2, 7, od)) return 1;
    od[6] = mock_double(0, 0, (const double[]){ 0 });
    if (call("observe_dense nowrap", 1, 7, od)) return 1;
    if (!call("observe_dense", 1, 6, od)) return 1;
    const mxArray *bad[7] = { od[0], h, mock_double(5, 1, (const double[]){ 1, 2, 3, 4, 5 }), od[3], od[4], od[5], od[6] };
    if (!call("observe_dense badsize", 1, 7, bad)) return 1;
    bad[2] = H; bad[3] = mock_double(3, 1, (const double[]){ 1, 2, 3 });
    if (!call("observe_dense badz", 1, 7, bad)) return 1;
    arm_failure();
    if (!call("observe_dense", 1, 7, od)) return 1;
'''
    without = r'''
    const mxArray *od[7] = { mock_string("observe_dense"), h, mock_double(7, 1, (const double[]){ 1, 2, 3, 4, 5, 6, 7 }), D1(1), D1(1), D1(1), D1(0) };
    if (!call("observe_dense", 1, 7, od)) return 1;
'''
    return driver(body, PRELUDE_SHOWN), driver_without(without)


def test_mex_gateway_reaches_the_abi(tmp_path):
    from mex_harness import transcript_of
    t = transcript_of(tmp_path, _STUB, _drivers()[0])
    i = t.index("ABI ekf_observe_dense k=2 H0=1 HLast=14 z0=0.5 RLast=2 gate=9.25 wrap=1")
    assert t[i + 1] == "MEX observe_dense nrhs=7 -> ok out0=1x4[2.5,2,1,0] out1=2x1[10.5,9.5]"
    assert "ABI ekf_observe_dense k=2 H0=1 HLast=14 z0=0.5 RLast=2 gate=9.25 wrap=-1" in t
    assert any(ln.startswith("MEX observe_dense nrhs=6 -> ERROR ekfslam:usage") and "needs 7 arguments" in ln for ln in t)
    assert any(ln.startswith("MEX observe_dense badsize nrhs=7 -> ERROR ekfslam:usage") and "H is n x k" in ln for ln in t)
    assert any(ln.startswith("MEX observe_dense badz nrhs=7 -> ERROR ekfslam:usage") and "z needs k" in ln for ln in t)
    assert sum(ln.startswith("ABI ekf_observe_dense") for ln in t) == 3               # the two good calls and the injected failure
    assert "MEX observe_dense nrhs=7 -> ERROR ekfslam:status | call not valid in the current state: injected failure" in t
    assert t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_the_gateway_still_links_against_a_library_without_the_symbol(tmp_path):
    from mex_harness import transcript_of
    t = transcript_of(tmp_path, _drivers()[1])
    assert any(ln.startswith("MEX observe_dense ") and "ERROR ekfslam:usage" in ln and "this libekfslam has no ekf_observe_dense" in ln for ln in t)
    assert "MEX predict nrhs=3 -> ok" in t and t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_matlab_method_names_the_call():
    text = open(os.path.join(ROOT, "matlab", "EKF_SLAM.m")).read()
    m = re.search(r"function\s+\[res, nu, S\]\s*=\s*observeDense\(h, H, z, R, gate, wrap\)(.*?)\n        end\b", text, re.S)
    assert m and "h.gateway('observe_dense', double(H).'" in m.group(1)
    src = open(os.path.join(ROOT, "matlab", "ekfslam_mex.c")).read()
    assert src.count('strcmp(cmd, "observe_dense")') == 1 and "#pragma weak ekf_observe_dense" in src


# ------------------------------------------------------------------------------------------------------------------
# the kernel sources on the host
# ------------------------------------------------------------------------------------------------------------------
def test_host_emulation_of_the_kernels_against_the_restatement(tmp_path):
    """k_dense_gram, k_dense_factor and k_gather_dense compiled for the host (tests/support/observe_dense_host_emulation.cpp) and the pair
    loop of the pass: the record, nu and S under the derived bars, x', the strip, the diagonal blocks, Prr' and the tiles -- read back
    as one dense P' -- against the restatement.  The program itself checks what is bit for bit (a gated and an irregular case change
    nothing, zero pairs over the padded tail, the live diagonal blocks are the tiles' own)."""
    import subprocess

    from helpers import host_build
    exe = host_build("observe_dense_host_emulation", str(tmp_path / "observe_dense_host_emulation"))
    out = tmp_path / "cases.bin"
    r = subprocess.run([exe, str(out)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    raw = np.fromfile(out, dtype=np.float64)
    pos, seen = 0, []

    def take(count, shape=None):
        nonlocal pos
        v = raw[pos:pos + count].copy()
        pos += count
        return v if shape is None else v.reshape(shape)

    while pos < raw.size:
        n, k, outcome, bad_row = (int(v) for v in take(4))
        H, z, R = take(k * n, (k, n)), take(k), take(k * k, (k, k))
        x0, P0, x1, P1 = take(n), take(n * n, (n, n)), take(n), take(n * n, (n, n))
        d2, nu, S = float(take(1)[0]), take(k), take(k * k, (k, k))
        gate = 0.0 if outcome == C.GATED else C.INF
        ex, eP, want = C.update_dense(x0, P0, H, z, R, gate)
        label = "n = %d, k = %d" % (n, k)
        assert (outcome, bad_row) == (want["outcome"], want["bad_row"]), label
        seen.append((n, k, outcome))
        np.testing.assert_array_equal(S, S.T)
        if outcome == C.IRREGULAR:
            assert np.isnan(d2) and np.array_equal(x1, x0) and np.array_equal(P1, P0), label
            np.testing.assert_array_equal(S, want["S"])       # unit rows: every sum has one product
            continue
        rS, rnu, rd2 = C.bar_ratios(x0, P0, H, z, R, dict(S=S, nu=nu, d2=d2))
        print("%s: worst error / bar: S %.3f nu %.3f d2 %.3f" % (label, rS, rnu, rd2))
        assert rS <= 1.0 and rnu <= 1.0 and rd2 <= 1.0, (label, rS, rnu, rd2)
        err_x, err_P = np.abs(x1 - ex).max() / np.abs(ex).max(), np.abs(P1 - eP).max() / np.abs(eP).max()
        print("%s: rel err x %.2e P %.2e" % (label, err_x, err_P))
        assert err_x < 1e-12 and err_P < 1e-12, label
        np.testing.assert_array_equal(P1, P1.T)
        if outcome == C.GATED:
            assert np.array_equal(x1, x0) and np.array_equal(P1, P0), label
    assert seen == [(83, 1, 1), (85, 2, 1), (85, 3, 1), (283, 16, 1), (283, 5, 1), (3, 3, 1), (85, 2, 2), (85, 2, 0)]
