"""CPU: ekf_factor_map without a GPU -- the NumPy restatement of tests/factor_map_cases.py against numpy.linalg.slogdet and
numpy.linalg.solve, and the builder of the scenes that are not positive definite; the kernels of ekf_slam_amd/csrc/factor_map.h compiled
for the host (factor tile edges 16 and 32, F64 and float sources, the matrix-core loop as its plain-FMA twin in the same k order) against
that restatement; the Python layers over a stand-in for the library (one marshal per call, the refusals before any call, the three
policies); the MEX gateway's command under the MEX mock."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import factor_map_cases as F
from helpers import REL, ROOT, RecorderBase, host_build
from mex_harness import PRELUDE_SHOWN, driver, driver_without, transcript_of
from removal_cases import lowrank_data

SIZES = [0, 1, 13, 16, 40]          # N = 16 at edge 32 ends exactly on a tile edge
PTHREAD = ["-O2", "-mfma", "-ffp-contract=off", "-pthread"]


def close(a, b):
    """|a - b| within helpers.REL of the expectation's size (of 1 where the expectation is smaller)."""
    return abs(a - b) <= REL * max(abs(b), 1.0)


# ------------------------------------------------------------------------------------------------------------------
# the restatement and the builder
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [0, 1, 13, 40, 140])
def test_the_restatement_agrees_with_slogdet_and_solve(N):
    x, s, d, U = lowrank_data(N, 11 + N)
    P = np.diag(d) + U @ U.T
    refs = F.reference_states(x, 3, N)
    refs[1, 2] += 360.0                                       # the heading difference is wrapped
    res = F.factor_dense(x, P, refs)
    sign, logdet = np.linalg.slogdet(P)
    assert sign == 1.0 and res["definite"] and res["bad_index"] == -1 and res["bad_pivot"] == 0.0 and res["n"] == 3 + 2 * N
    err = abs(res["logdet"] - logdet) / max(abs(logdet), 1.0)
    sign_m, logdet_m = np.linalg.slogdet(P[3:, 3:]) if N else (1.0, 0.0)
    err_m = abs(res["logdet_map"] - logdet_m) / max(abs(logdet_m), 1.0)
    worst = 0.0
    for q in range(3):
        nu = x - refs[q]
        nu[2] = F.wrap180(nu[2])
        want = float(nu @ np.linalg.solve(P, nu))
        worst = max(worst, abs(res["d2"][q] - want) / want)
    print("N=%d: log det against slogdet %.2e, of the landmark block %.2e, d2 against solve %.2e" % (N, err, err_m, worst))
    assert err < 1e-12 and err_m < 1e-12 and worst < 1e-10
    assert res["min_pivot"] == res["pivots"].min() and res["max_pivot"] == res["pivots"].max()
    L = res["L"]
    order = F.elimination_order(x.size)
    assert np.abs(L @ L.T - P[np.ix_(order, order)]).max() < 1e-14 * max(np.abs(P).max(), 1.0)


def test_the_builder_places_the_failing_pivot_where_it_is_asked_to():
    for N, bad, zero in ((40, 3 + 5, False), (40, 3 + 32, False), (40, 3 + 79, False), (40, 1, False), (40, 2, False), (40, 3 + 41, True), (1, 4, False)):
        x, s, P = F.indefinite_scene(N, bad, zero)
        res = F.factor_dense(x, P, F.reference_states(x, 2, 1))
        np.testing.assert_array_equal(P, P.T)
        assert not res["definite"] and res["bad_index"] == bad and np.isnan(res["logdet"]) and np.isnan(res["d2"]).all()
        assert np.isnan(res["logdet_map"]) == (bad >= 3)
        assert (res["bad_pivot"] == 0.0) if zero else (res["bad_pivot"] < 0.0)
    x, s, P = F.spd_scene(6, 2)
    P[:3, :] = 0.0
    P[:, :3] = 0.0                                            # a filter that starts at a known pose
    res = F.factor_dense(x, P)
    sign, logdet_m = np.linalg.slogdet(P[3:, 3:])
    assert not res["definite"] and res["bad_index"] == 0 and res["bad_pivot"] == 0.0 and abs(res["logdet_map"] - logdet_m) < 1e-12


# ------------------------------------------------------------------------------------------------------------------
# the kernels compiled for the host
# ------------------------------------------------------------------------------------------------------------------
def as_held(P, fl):
    """P as a handle with that storage kind reports it: with float tiles every entry of the landmark block outside the landmarks' own
    2 x 2 blocks is rounded to float; Prr, the strip and the own blocks stay F64."""
    if not fl:
        return P.copy()
    H = P.copy()
    n = P.shape[0]
    H[3:, 3:] = P[3:, 3:].astype(np.float32).astype(np.float64)
    for a in range(3, n, 2):
        H[a:a + 2, a:a + 2] = P[a:a + 2, a:a + 2]
    return H


def _scenes():
    """name -> (TF, Tsrc, float, N, x, P, refs)."""
    out = {}
    for TF in (16, 32):
        for fl in (0, 1):
            for N in SIZES:
                x, s, P = F.spd_scene(N, 100 + N)
                out["spd_F%d_%s_N%d" % (TF, "f" if fl else "d", N)] = (TF, 48 - TF, fl, N, x, P, F.reference_states(x, 3, N))
        x, s, P = F.spd_scene(40, 5)
        out["same_edge_F%d" % TF] = (TF, TF, 0, 40, x, P, F.reference_states(x, 8, 2))
        out["no_refs_F%d" % TF] = (TF, 16, 1, 13, *F.spd_scene(13, 6)[0::2], np.zeros((0, 29)))
    # not definite: the first tile, the first row of the third tile, the last active row of a partly empty last tile (N = 40 at edge 32:
    # rows 64 .. 79 of 64 .. 95), the robot tail, an exact zero at a landmark, a robot that starts at a known pose
    for name, TF, bad, zero in (("neg_first_tile", 16, 3 + 5, False), ("neg_third_tile", 16, 3 + 32, False), ("neg_last_row", 32, 3 + 79, False),
                                ("neg_robot", 16, 1, False), ("zero_landmark", 16, 3 + 41, True)):
        x, s, P = F.indefinite_scene(40, bad, zero)
        out[name] = (TF, 48 - TF, 0, 40, x, P, F.reference_states(x, 2, 3))
    x, s, P = F.spd_scene(13, 9)
    P[:3, :] = 0.0
    P[:, :3] = 0.0
    out["known_pose"] = (32, 16, 1, 13, x, P, F.reference_states(x, 1, 3))
    return out


def _write_cases(d, names=None):
    scenes = _scenes()
    with open(os.path.join(str(d), "cases.txt"), "w") as f:
        for name, (TF, Tsrc, fl, N, x, P, refs) in scenes.items():
            if names is not None and name not in names:
                continue
            f.write("%s %d %d %d %d %d\n" % (name, TF, Tsrc, fl, N, refs.shape[0]))
            np.concatenate([x, P.reshape(-1, order="F"), refs.reshape(-1)]).tofile(os.path.join(str(d), name + ".in"))
    return scenes


@pytest.fixture(scope="module")
def emulation(tmp_path_factory):
    d = tmp_path_factory.mktemp("factor_map_emulation")
    scenes = _write_cases(d)
    exe = host_build("factor_map_host_emulation", str(d / "emu"), flags=PTHREAD)
    r = subprocess.run([exe, str(d)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    return d, r.stdout, scenes


def _result(d, name, N):
    """What host/factor_map.h makes of the result block and the pivots, restated: the dict of Engine.factor_map."""
    v = np.fromfile(os.path.join(str(d), name + ".out"))
    res, piv = v[:16], v[16:]
    status = int(res[0])
    taken = list(piv[:int(res[1]) - 3 if status == 1 else 2 * N])
    logdet_map = float("nan") if status == 1 else 2.0 * float(np.sum(np.log(taken)))
    if status != 1:
        taken += list(res[3:3 + int(res[6])])
    sq = np.array(taken) ** 2
    return dict(n=3 + 2 * N, definite=status == 0, bad_index=-1 if status == 0 else int(res[1]), bad_pivot=0.0 if status == 0 else float(res[2]),
                logdet=2.0 * float(np.sum(np.log(taken))) if status == 0 else float("nan"), logdet_map=logdet_map,
                min_pivot=float(sq.min()) if sq.size else float("nan"), max_pivot=float(sq.max()) if sq.size else float("nan"),
                d2=res[8:16] if status == 0 else np.full(8, np.nan))


@pytest.mark.parametrize("fl", [0, 1])
@pytest.mark.parametrize("TF", [16, 32])
def test_host_emulation_of_the_kernels_against_the_restatement(emulation, TF, fl):
    """Every size, the source's tile edge different from the factor's: log det, the landmark block's, the extreme pivots and d2 of three
    references at helpers.REL against the restatement on the matrix as the handle holds it; nothing of the state written."""
    d, out, scenes = emulation
    names = ["spd_F%d_%s_N%d" % (TF, "f" if fl else "d", N) for N in SIZES] + ["same_edge_F%d" % TF] * (1 - fl) + ["no_refs_F%d" % TF] * fl
    for name in names:
        assert "%s: 0 differences" % name in out
        _, _, sfl, N, x, P, refs = scenes[name]
        want = F.factor_dense(x, as_held(P, sfl), refs)
        got = _result(d, name, N)
        assert got["definite"] and want["definite"] and got["bad_index"] == -1 and got["n"] == want["n"]
        errs = [abs(got[k] - want[k]) / max(abs(want[k]), 1.0) for k in ("logdet", "logdet_map", "min_pivot", "max_pivot")]
        errs += [abs(got["d2"][q] - want["d2"][q]) / max(abs(want["d2"][q]), 1.0) for q in range(refs.shape[0])]
        print("%s: worst error against the restatement %.2e" % (name, max(errs)))
        assert max(errs) < REL
        assert not got["d2"][refs.shape[0]:].any()            # the columns no reference uses stay zero


def test_host_emulation_stops_at_the_first_failing_pivot(emulation):
    d, out, scenes = emulation
    for name, bad, zero in (("neg_first_tile", 8, False), ("neg_third_tile", 35, False), ("neg_last_row", 82, False), ("neg_robot", 1, False),
                            ("zero_landmark", 44, True), ("known_pose", 0, True)):
        assert "%s: 0 differences" % name in out
        _, _, sfl, N, x, P, refs = scenes[name]
        want = F.factor_dense(x, as_held(P, sfl), refs)
        got = _result(d, name, N)
        assert not got["definite"] and got["bad_index"] == want["bad_index"] == bad and np.isnan(got["logdet"])
        if zero:
            assert got["bad_pivot"] == 0.0
        else:
            assert got["bad_pivot"] < 0.0 and close(got["bad_pivot"], want["bad_pivot"])
        if bad < 3:
            assert close(got["logdet_map"], want["logdet_map"])
        else:
            assert np.isnan(got["logdet_map"])
        assert close(got["min_pivot"], want["min_pivot"]) and close(got["max_pivot"], want["max_pivot"])


def test_kernel_sources_on_the_host_under_the_sanitizers(tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined runs clean on a definite and a not-definite scene per factor
    tile edge: no lane of any kernel reads or writes outside the factor store, the right-hand sides, the result block or the state
    (nothing loaded into python is involved)."""
    _write_cases(tmp_path, ("spd_F16_f_N40", "spd_F32_d_N13", "spd_F32_d_N0", "neg_third_tile", "neg_last_row", "known_pose"))
    exe = host_build("factor_map_host_emulation", str(tmp_path / "emulation_sanitized"),
                     flags=["-O1", "-g", "-mfma", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]


def test_the_twin_runs_the_matrix_instructions_k_order():
    """The plain-FMA twin and the matrix-core loop name their k index through the same function, and no kernel spills by design: the
    panel's row and the finish's sums are indexed statically."""
    src = open(os.path.join(ROOT, "ekf_slam_amd", "csrc", "factor_map.h")).read()
    assert src.count("factor_k<TF>(s, t)") == 2 and src.count("factor_k<TF>(s, lr)") == 2
    assert "__builtin_amdgcn_mfma_f64_16x16x4f64(av[s], bv[s], acc[b], 0, 0, 0)" in src


# ------------------------------------------------------------------------------------------------------------------
# the Python layers over a stand-in for the library
# ------------------------------------------------------------------------------------------------------------------
class _Recorder(RecorderBase):
    status_string = b"invalid argument"
    last_error = b"factor_map: not built for sharded handles (world > 1): injected"

    def __init__(self):
        self.calls, self.fail, self.N, self.info = [], 0, 2, dict(definite=1, bad_index=-1, logdet=-3.5, logdet_map=-2.0, min_pivot=0.1, max_pivot=2.0)

    def ekf_num_landmarks(self, h, pn):
        pn._obj.value = self.N
        return 0

    def ekf_factor_map(self, h, ref, nref, info, d2):
        assert isinstance(nref, ctypes.c_int32)                # marshalled once, by marshal.factor_args
        n = 3 + 2 * self.N
        self.calls.append(("factor_map", h.value, None if ref is None else [ref[k] for k in range(nref.value * n)], nref.value, d2 is not None))
        if self.fail:
            return self.fail
        info._obj.n = n
        for k, v in self.info.items():
            setattr(info._obj, k, v)
        for q in range(nref.value):
            d2[q] = 10.0 + q
        return 0


def test_layers_marshal_a_factorisation_once(monkeypatch):
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import engine as E
    from ekf_slam_amd import marshal
    from ekf_slam_amd import slam as S
    from ekf_slam_amd.sharding import ShardGroup
    from ekf_slam_amd.trajectory import TrajectoryLog
    dp = ctypes.POINTER(ctypes.c_double)
    assert L.SIGNATURES["ekf_factor_map"] == (ctypes.c_int32, [ctypes.c_void_p, dp, ctypes.c_int32, ctypes.POINTER(L.EkfFactorInfo), dp])
    assert ctypes.sizeof(L.EkfFactorInfo) == 64 and L.EkfFactorInfo.bad_index.offset == 16 and L.EkfFactorInfo.max_pivot.offset == 56
    header = open(os.path.join(ROOT, "include", "ekfslam.h")).read()
    assert "int32_t ekf_factor_map(ekf_handle *h, const double *ref" in header and "THE LANDMARK BLOCK FIRST" in header
    rec = _Recorder()
    monkeypatch.setattr(L, "lib", lambda: rec)
    made = []
    real = marshal.factor_args
    monkeypatch.setattr(marshal, "factor_args", lambda *a, **k: made.append(a) or real(*a, **k))
    g = E.Engine(capacity=32, tile=16)
    res = g.factor_map()
    assert rec.calls == [("factor_map", g.h.value, None, 0, False)] and len(made) == 1
    assert res["definite"] is True and res["bad_index"] == -1 and res["logdet"] == -3.5 and res["n"] == 7 and res["d2"].size == 0
    assert sorted(res) == sorted(F.KEYS + ("d2",))
    one = np.arange(7.0)
    res = g.factor_map(one)
    assert rec.calls[-1] == ("factor_map", g.h.value, list(one), 1, True) and res["d2"].tolist() == [10.0]
    three = np.arange(21.0).reshape(3, 7)
    res = g.factor_map(three)
    assert rec.calls[-1][2:] == (list(three.reshape(-1)), 3, True) and res["d2"].tolist() == [10.0, 11.0, 12.0] and len(made) == 3
    # the refusals, in marshal, before anything is sent
    n = len(rec.calls)
    bad_nan = one.copy()
    bad_nan[4] = np.nan
    for ref in (np.zeros((0, 7)), np.zeros((9, 7)), np.zeros(6), np.zeros((2, 9)), bad_nan, np.full((2, 7), np.inf), np.zeros((2, 1, 7))):
        with pytest.raises(ValueError) as info:
            g.factor_map(ref)
        assert "factor_map" in str(info.value)
    assert len(rec.calls) == n
    # the library's refusal raises; a shard group hands the call to its first shard so that the refusal is the library's
    rec.fail = L.EKF_ERR_INVALID_ARG
    with pytest.raises(L.EkfError) as info:
        g.factor_map()
    assert info.value.status == L.EKF_ERR_INVALID_ARG and "factor_map" in str(info.value)
    grp = ShardGroup(2, capacity=16)
    with pytest.raises(L.EkfError) as info:
        grp.factor_map()
    assert rec.calls[-1][0] == "factor_map" and rec.calls[-1][1] == grp.shards[0].h.value and "sharded" in str(info.value)
    rec.fail = 0
    # the policies: one call each, nothing logged
    for cls in (S.EKF_SLAM, S.EKF_SLAM_UC):
        rec.calls.clear()
        del made[:]
        f = cls(capacity=32, tile=64)
        f.log = TrajectoryLog()
        d2, dof = f.nees(one)
        assert (d2, dof) == (10.0, 7) and rec.calls[-1][2:] == (list(one), 1, True)
        inside, d2, (lo, hi) = f.nees_within(one, 0.95)
        assert lo == S.chi2_quantile(0.5 * (1.0 - 0.95), 7) and hi == S.chi2_quantile(0.5 * (1.0 + 0.95), 7) and 1.68 < lo < 1.70 and 16.0 < hi < 16.02 and d2 == 10.0 and inside is (lo <= 10.0 <= hi)
        assert f.nees_within(one, 0.2)[0] is False            # 10 is outside the narrow interval around the median of 7 degrees of freedom
        assert f.map_entropy() == 0.5 * (7 * math.log(2.0 * math.pi * math.e) - 3.5)
        assert f.factor_map(three)["d2"].size == 3
        assert len(rec.calls) == 5 and len(made) == 5 and len(f.log.edits) == 0
        with pytest.raises(ValueError):
            f.nees_within(one, 1.0)
        with pytest.raises(ValueError):
            f.nees(np.zeros(5))
        rec.info["definite"], rec.info["logdet"] = 0, float("nan")
        assert math.isnan(f.map_entropy())
        rec.info["definite"], rec.info["logdet"] = 1, -3.5


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
int32_t ekf_factor_map(ekf_handle *h, const double *ref, int32_t nref, ekf_factor_info *info, double *d2) {
    int64_t N;
    ekf_num_landmarks(h, &N);
    printf("ABI ekf_factor_map nref=%d", (int)nref);
    if (ref) printf(" ref0=%g refLast=%g d2=%s\n", ref[0], ref[nref * (3 + 2 * N) - 1], d2 ? "given" : "null"); else printf(" ref=null d2=%s\n", d2 ? "given" : "null");
    if (fail_armed) { fail_armed = 0; stub_fail_next(h); return ekf_flush(h); }
    info->n = 3 + 2 * N; info->definite = 0; info->bad_index = 4; info->bad_pivot = -0.5; info->logdet = NAN; info->logdet_map = -2.5;
    info->min_pivot = 0.25; info->max_pivot = 4.0;
    for (int q = 0; q < nref; ++q) d2[q] = 7.0 + q;
    return EKF_OK;
}
'''

_DRIVER = driver(r'''
    const mxArray *sx[3] = { mock_string("set_x"), h, mock_double(7, 1, (const double[]){ 1, 2, 3, 4, 5, 6, 7 }) };
    if (call("set_x", 0, 3, sx)) return 1;
    const mxArray *none = mock_double(0, 0, (const double[]){ 0 });
    const mxArray *two = mock_double(7, 2, (const double[]){ 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14 });
    const mxArray *fm[3] = { mock_string("factor_map"), h, two };
    if (call("factor_map", 2, 3, fm)) return 1;
    const mxArray *fn[3] = { fm[0], h, none };
    if (call("factor_map none", 2, 3, fn)) return 1;
    if (call("factor_map one_output", 1, 3, fm)) return 1;
    if (!call("factor_map", 2, 2, fm)) return 1;
    const mxArray *bad[3] = { fm[0], h, mock_double(5, 1, (const double[]){ 1, 2, 3, 4, 5 }) };
    if (!call("factor_map badsize", 2, 3, bad)) return 1;
    bad[2] = mock_double(7, 9, (const double[63]){ 0 });
    if (!call("factor_map toomany", 2, 3, bad)) return 1;
    arm_failure();
    if (!call("factor_map", 2, 3, fm)) return 1;
''', PRELUDE_SHOWN)

_DRIVER_WITHOUT = driver_without(r'''
    const mxArray *fm[3] = { mock_string("factor_map"), h, mock_double(0, 0, (const double[]){ 0 }) };
    if (!call("factor_map", 1, 3, fm)) return 1;
''')


def test_mex_gateway_reaches_the_abi(tmp_path):
    t = transcript_of(tmp_path, _STUB, _DRIVER)
    i = t.index("ABI ekf_factor_map nref=2 ref0=1 refLast=14 d2=given")
    assert t[i + 1] == "MEX factor_map nrhs=3 -> ok out0=1x8[7,0,5,-0.5,nan,-2.5,0.25,4] out1=2x1[7,8]" or \
        t[i + 1] == "MEX factor_map nrhs=3 -> ok out0=1x8[7,0,5,-0.5,-nan,-2.5,0.25,4] out1=2x1[7,8]"
    j = t.index("ABI ekf_factor_map nref=0 ref=null d2=null")
    assert t[j + 1].startswith("MEX factor_map none nrhs=3 -> ok out0=1x8[7,0,5,-0.5,") and t[j + 1].endswith(" out1=0x1[]")
    assert any(ln.startswith("MEX factor_map one_output nrhs=3 -> ok out0=1x8[") and "out1" not in ln for ln in t)
    assert any(ln.startswith("MEX factor_map nrhs=2 -> ERROR ekfslam:usage") and "needs 3 arguments" in ln for ln in t)
    for name in ("badsize", "toomany"):
        assert any(ln.startswith("MEX factor_map %s nrhs=3 -> ERROR ekfslam:usage" % name) and "ref is empty or n x q" in ln for ln in t), name
    assert sum(ln.startswith("ABI ekf_factor_map") for ln in t) == 4            # the three good calls and the injected failure
    assert "MEX factor_map nrhs=3 -> ERROR ekfslam:status | call not valid in the current state: injected failure" in t
    assert t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_the_gateway_still_links_against_a_library_without_the_symbol(tmp_path):
    t = transcript_of(tmp_path, _DRIVER_WITHOUT)
    assert any(ln.startswith("MEX factor_map ") and "ERROR ekfslam:usage" in ln and "this libekfslam has no ekf_factor_map" in ln for ln in t)
    assert "MEX predict nrhs=3 -> ok" in t and t[-2:] == ["LOCKS 0", "MISUSE 0"]


def test_matlab_method_and_documents_name_the_call():
    text = open(os.path.join(ROOT, "matlab", "EKF_SLAM.m")).read()
    m = re.search(r"function\s+\[info,\s*d2\]\s*=\s*factorMap\(h,\s*ref\)(.*?)\n        end\b", text, re.S)
    assert m and "h.gateway('factor_map', double(ref));" in m.group(1)
    src = open(os.path.join(ROOT, "matlab", "ekfslam_mex.c")).read()
    assert 'strcmp(cmd, "factor_map")' in src and "#pragma weak ekf_factor_map" in src
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        body = open(os.path.join(ROOT, doc)).read()
        assert "factor_map" in body, doc
    assert "factorMap" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "extract_map" in readme and "elimination order" in open(os.path.join(ROOT, "DESIGN.md")).read()
