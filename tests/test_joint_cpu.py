"""CPU: ekf_joint_innovation's host-and-device functions (ekfm::joint_pairing, joint_cross_block, the joint_factor_* steps and
joint_prefix_add of ekf_slam_amd/csrc/device_math.h, built for the host and put together in the kernel's phases by
tests/support/joint_host.cpp) against the dense restatement of tests/joint_cases.py and against the existing small part; chi2_quantile;
and the Python layers -- Engine.joint_innovation with its chunking, the 1-based wrapper, the policy measure_model_joint -- over a stand-in
for the library that answers from the restatement.  No GPU."""
import ctypes

import numpy as np
import pytest

import associate_model_cases as A
import joint_cases as J
import model_obs_cases as M
from helpers import RPOS, RecorderBase, line_program

INF = float("inf")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """The stand-alone host build of the joint functions: host(lines) -> one list of floats per line."""
    return line_program(tmp_path_factory, "joint_host")


@pytest.fixture(scope="module")
def small_host(tmp_path_factory):
    return line_program(tmp_path_factory, "model_eval_host")


@pytest.fixture(scope="module")
def dense():
    return J.dense_state()


def joint_line(x, P, entries, hyp):
    """One hypothesis with the operands k_joint_innovation loads for it."""
    vals = []
    for ent, lm in zip(entries, hyp):
        o = M.obs(ent["model"], ent["z"], ent["R"], [0])
        z = o["z"].copy()
        if o["rows"] == 1:
            z[1] = 0.0
        vals.append("%d %s %d" % (ent["model"], M.fmt(list(z) + list(M.effective_R(o).reshape(-1))), lm))
    paired = [int(lm) for lm in hyp if lm >= 0]
    nums = list(P[:3, :3].reshape(-1)) + list(x[:3])
    for lm in paired:
        a = 3 + 2 * lm
        nums += [P[t, a + r] for t in range(3) for r in range(2)] + [P[a, a], P[a + 1, a], P[a + 1, a + 1]] + list(x[a:a + 2])
    for pa in range(1, len(paired)):
        for pb in range(pa):
            a, b = 3 + 2 * paired[pa], 3 + 2 * paired[pb]
            nums += [P[a + r, b + c] for r in range(2) for c in range(2)]
    return "joint %d %s %s" % (len(entries), " ".join(vals), M.fmt(nums))


def parse(row, m):
    """A line of the host program as Engine.joint_innovation's fields for one hypothesis."""
    row = list(row)
    S = np.array(row[5 + 3 * m:5 + 3 * m + 4 * m * m]).reshape(2 * m, 2 * m, order="F")
    return dict(outcome=int(row[0]), first_irregular=int(row[1]), dof=int(row[2]), pairings=int(row[3]), d2=row[4],
                d2_prefix=np.array(row[5:5 + m]), nu=np.array(row[5 + m:5 + 3 * m]), S=S)


def scan_of(x, m, seed=1):
    lms = np.random.default_rng(seed).choice(J.N0, m, replace=False).tolist()
    return J.cycle_scan(x, lms), lms


# ------------------------------------------------------------------------------------------------------------------
# 1. the host build against the dense restatement
# ------------------------------------------------------------------------------------------------------------------
def test_host_build_matches_H_P_Ht_plus_R_and_solve_at_every_size(host, dense):
    x, P = dense
    worst_block, worst_d2 = 0.0, 0.0
    for m in (1, 2, 5, 16, 32):
        ents, lms = scan_of(x, m)
        got = parse(host([joint_line(x, P, ents, lms)])[0], m)
        want = J.joint_dense(x, P, ents, lms)
        cond = J.cond_of(got["S"], lms)
        assert cond <= 1e3
        assert (got["outcome"], got["first_irregular"], got["dof"], got["pairings"]) == (J.REGULAR, -1, want["dof"], m)
        assert got["dof"] == sum(M.ROWS[e["model"]] for e in ents)
        # off-diagonal blocks, componentwise, and the rest of S and nu
        bound = J.cross_bound(x, P, ents, lms)
        off = np.ones((2 * m, 2 * m), dtype=bool)
        for k in range(m):
            off[2 * k:2 * k + 2, 2 * k:2 * k + 2] = False
        diff = np.abs(got["S"] - want["S"])
        live = off & (bound > 0.0)                                      # (a one-row model's empty row: the bound and the block are exactly zero)
        ratio = (diff[live] / bound[live]).max() if m > 1 else 0.0
        worst_block = max(worst_block, ratio)
        assert np.all(diff[off] <= bound[off])
        np.testing.assert_allclose(got["S"], want["S"], rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(got["nu"], want["nu"], rtol=1e-12, atol=1e-12)
        np.testing.assert_array_equal(got["S"][off], got["S"].T[off])
        # d2 and every prefix against solve on the SAME S and nu
        ref = J.solve_prefixes(got["S"], got["nu"], lms)
        err = np.abs(got["d2_prefix"] - ref) / ref
        worst_d2 = max(worst_d2, err.max(), abs(got["d2"] - ref[-1]) / ref[-1])
        print("m = %2d: cond(S) %.3g, worst |dS_ab| / bound %.3g, worst relative error of d2 and prefixes %.2e, d2 = %.4g" % (m, cond, ratio, err.max(), got["d2"]))
        assert err.max() <= 1e-9 and abs(got["d2"] - ref[-1]) <= 1e-9 * ref[-1]
        np.testing.assert_allclose(got["d2_prefix"], want["d2_prefix"], rtol=1e-9)
    print("worst over all sizes: blocks %.3g of the bound, d2 %.2e" % (worst_block, worst_d2))


# ------------------------------------------------------------------------------------------------------------------
# 2. bit-for-bit equalities
# ------------------------------------------------------------------------------------------------------------------
def test_diagonal_blocks_and_nu_are_model_small_bit_for_bit(host, small_host, dense):
    x, P = dense
    m = 8
    ents, lms = scan_of(x, m, seed=2)
    got = parse(host([joint_line(x, P, ents, lms)])[0], m)
    old = small_host([M.small_line(M.obs(e["model"], e["z"], e["R"], [lm]), x, P) for e, lm in zip(ents, lms)])
    for k, o in enumerate(old):
        np.testing.assert_array_equal(got["nu"][2 * k:2 * k + 2], o[3:5])
        np.testing.assert_array_equal(got["S"][2 * k:2 * k + 2, 2 * k:2 * k + 2].reshape(-1), o[5:9])        # row-major, S01 and S10 each its own


def test_prefix_k_is_d2_of_the_hypothesis_cut_after_entry_k_bit_for_bit(host, dense):
    x, P = dense
    m = 9
    ents, lms = scan_of(x, m, seed=3)
    hyp = list(lms)
    hyp[2] = hyp[6] = -1
    whole = parse(host([joint_line(x, P, ents, hyp)])[0], m)
    cuts = host([joint_line(x, P, ents, hyp[:k + 1] + [-1] * (m - k - 1)) for k in range(m)])
    np.testing.assert_array_equal(whole["d2_prefix"], [parse(r, m)["d2"] for r in cuts])
    assert whole["d2_prefix"][2] == whole["d2_prefix"][1] and whole["d2"] == whole["d2_prefix"][-1]
    empty = parse(host([joint_line(x, P, ents, [-1] * m)])[0], m)
    assert (empty["d2"], empty["dof"], empty["pairings"], empty["outcome"], empty["first_irregular"]) == (0.0, 0, 0, J.REGULAR, -1)
    np.testing.assert_array_equal(empty["S"], np.eye(2 * m))


def test_entries_left_out_equal_the_same_pairings_as_a_shorter_scan_bit_for_bit(host, dense):
    x, P = dense
    m = 9
    ents, lms = scan_of(x, m, seed=4)
    hyp = list(lms)
    hyp[0] = hyp[4] = hyp[8] = -1
    keep = [k for k in range(m) if hyp[k] >= 0]
    long_, short = host([joint_line(x, P, ents, hyp), joint_line(x, P, [ents[k] for k in keep], [hyp[k] for k in keep])])
    long_, short = parse(long_, m), parse(short, len(keep))
    assert long_["d2"] == short["d2"] and long_["dof"] == short["dof"]
    np.testing.assert_array_equal(long_["d2_prefix"][keep], short["d2_prefix"])
    rows = [2 * k + r for k in keep for r in range(2)]
    np.testing.assert_array_equal(long_["S"][np.ix_(rows, rows)], short["S"])
    np.testing.assert_array_equal(long_["nu"][rows], short["nu"])


def test_an_irregular_pairing_stops_the_prefixes_there_and_leaves_the_earlier_ones(host, dense):
    x, P = dense
    m = 5
    ents, lms = scan_of(x, m, seed=5)
    on_robot = x.copy()
    on_robot[3 + 2 * lms[2]:5 + 2 * lms[2]] = x[:2]
    bad, good = (parse(r, m) for r in host([joint_line(on_robot, P, ents, lms), joint_line(x, P, ents, lms[:2] + [-1] * 3)]))
    assert (bad["outcome"], bad["first_irregular"]) == (J.IRREGULAR, 2) and np.isnan(bad["d2"])
    np.testing.assert_array_equal(bad["d2_prefix"][:2], good["d2_prefix"][:2])
    assert np.all(np.isnan(bad["d2_prefix"][2:]))
    want = J.joint_dense(on_robot, P, ents, lms)
    assert (want["outcome"], want["first_irregular"]) == (J.IRREGULAR, 2)
    # a pivot that is not positive: the landmark's and the robot's rows of P zero (H_r Prr H_r' alone would keep S positive) and a
    # one-row model with R = 0
    flat = P.copy()
    a = 3 + 2 * lms[1]
    for lo, hi in ((0, 3), (a, a + 2)):
        flat[lo:hi, :] = 0.0
        flat[:, lo:hi] = 0.0
    ents0 = list(ents)
    ents0[1] = A.entry(M.RANGE, ents[1]["z"], 0.0)
    sing = parse(host([joint_line(x, flat, ents0, lms)])[0], m)
    assert (sing["outcome"], sing["first_irregular"]) == (J.IRREGULAR, 1) and np.isfinite(sing["d2_prefix"][0]) and np.all(np.isnan(sing["d2_prefix"][1:]))
    assert np.all(np.isfinite(sing["S"])) and np.all(np.isfinite(sing["nu"]))


# ------------------------------------------------------------------------------------------------------------------
# 3. chi2_quantile
# ------------------------------------------------------------------------------------------------------------------
def test_chi2_quantile_known_values():
    from ekf_slam_amd.slam import chi2_quantile
    for (p, dof), want in (((0.99, 1), 6.635), ((0.99, 2), 9.210), ((0.99, 4), 13.277), ((0.99, 10), 23.209), ((0.95, 2), 5.991)):
        got = chi2_quantile(p, dof)
        print("chi2_quantile(%g, %d) = %.6f" % (p, dof, got))
        assert abs(got - want) <= 1e-3
    assert chi2_quantile(0.99, 0) == 0.0
    assert abs(chi2_quantile(0.99, 6) - J.chi2_table(0.99, 6)) < 1e-9
    for bad in ((0.0, 2), (1.0, 2), (0.5, -1)):
        with pytest.raises(ValueError):
            chi2_quantile(*bad)


# ------------------------------------------------------------------------------------------------------------------
# 4. the Python layers over a stand-in that answers from the restatement
# ------------------------------------------------------------------------------------------------------------------
class _Lib(RecorderBase):
    last_error = b"joint_innovation: injected"

    def __init__(self, x, P):
        self.x, self.P, self.calls, self.fail, self.canned = np.asarray(x), np.asarray(P), [], 0, None

    @property
    def N(self):
        return (self.x.size - 3) // 2

    @staticmethod
    def _entries(arr, m):
        out = []
        for k in range(m):
            Rm = np.array(list(arr[k].R)).reshape(2, 2, order="F")
            rows = M.ROWS[arr[k].model]
            out.append(A.entry(arr[k].model, list(arr[k].z), Rm if rows == 2 else Rm[0, 0], arr[k].gate))
        return out

    def ekf_num_landmarks(self, h, pn):
        pn._obj.value = self.N
        return 0

    def ekf_associate_model(self, h, arr, m, out, d2_all):
        ents = self._entries(arr, m)
        self.calls.append(("associate", m, bool(d2_all)))
        res, D = A.match(self.x, self.P, ents)
        for k in range(m):
            out[k].best, out[k].second, out[k].d2_best, out[k].d2_second = int(res["best"][k]), int(res["second"][k]), res["d2_best"][k], res["d2_second"][k]
            out[k].within_gate, out[k].irregular = int(res["within_gate"][k]), int(res["irregular"][k])
        if d2_all:
            for q, v in enumerate(D.reshape(-1)):
                d2_all[q] = v
        return 0

    def ekf_joint_innovation(self, h, arr, m, hyp, nh, out, prefix, nu, S):
        hyps = [[int(hyp[i * m + k]) for k in range(m)] for i in range(nh)]
        self.calls.append(("joint", m, hyps, bool(prefix), bool(nu), bool(S)))
        if self.fail:
            return self.fail
        ents = self._entries(arr, m)
        for i, hy in enumerate(hyps):
            r = J.joint_dense(self.x, self.P, ents, hy)
            if self.canned is not None:
                r = dict(r, d2_prefix=np.array(self.canned(hy)))
            out[i].d2, out[i].dof, out[i].pairings, out[i].outcome, out[i].first_irregular = r["d2_prefix"][-1], r["dof"], r["pairings"], r["outcome"], r["first_irregular"]
            for k in range(m):
                if prefix:
                    prefix[i * m + k] = r["d2_prefix"][k]
            if nu:
                for q in range(2 * m):
                    nu[i * 2 * m + q] = r["nu"][q]
            if S:
                for q, v in enumerate(r["S"].reshape(-1, order="F")):
                    S[i * 4 * m * m + q] = v
        return 0

    def ekf_observe_model(self, h, pobs, pres):
        o = pobs._obj
        self.calls.append(("observe", o.model, list(o.z), list(o.lm), o.gate, pres is not None))
        return 0

    def ekf_append_model(self, h, arr, m, pfirst):
        self.calls.append(("append", m))
        pfirst._obj.value = self.N
        self.x = np.concatenate([self.x, np.zeros(2 * m)])
        return 0


def _engine(monkeypatch, x, P):
    from ekf_slam_amd import _lib as L
    rec = _Lib(x, P)
    monkeypatch.setattr(L, "lib", lambda: rec)
    return rec


def _filter(monkeypatch, x, P):
    from ekf_slam_amd import slam as S
    from ekf_slam_amd.trajectory import TrajectoryLog
    rec = _engine(monkeypatch, x, P)
    f = S.EKF_SLAM_UC(capacity=256)
    f.log = TrajectoryLog()
    return f, rec


def test_engine_layer_marshals_chunks_and_unpacks(monkeypatch, dense):
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import engine as E
    from ekf_slam_amd import slam as S
    assert ctypes.sizeof(L.EkfJointResult) == 24 and (L.EKF_JOINT_MAX, L.EKF_JOINT_HYP_MAX) == (32, 256) and "ekf_joint_innovation" in L.SIGNATURES
    x, P = dense
    rec = _engine(monkeypatch, x, P)
    e = E.Engine(capacity=256)
    ents, lms = scan_of(x, 3, seed=7)
    rng = np.random.default_rng(8)
    hyps = [[int(v) for v in np.where(rng.random(3) < 0.3, -1, rng.choice(J.N0, 3, replace=False))] for _ in range(600)]
    got = e.joint_innovation(ents, hyps, want_nu=True, want_S=True)
    want = J.joint_many(x, P, ents, hyps)
    joint_calls = [c for c in rec.calls if c[0] == "joint"]
    assert [len(c[2]) for c in joint_calls] == [256, 256, 88] and all(c[1] == 3 and c[3:] == (True, True, True) for c in joint_calls)
    assert sum((c[2] for c in joint_calls), []) == hyps
    for key in ("d2", "dof", "pairings", "outcome", "first_irregular", "d2_prefix", "nu", "S"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)             # chunked == the unchunked restatement
    lean = e.joint_innovation(ents, hyps[:2], want_prefix=False)
    assert rec.calls[-1][3:] == (False, False, False) and "d2_prefix" not in lean and "S" not in lean
    # the 1-based wrapper: 0 = left out, first_irregular 1-based with 0 = none
    f = S.EKF_SLAM(capacity=256)
    one = f.joint_innovation(ents, [[lms[0] + 1, 0, lms[2] + 1]])
    assert rec.calls[-1][2] == [[lms[0], -1, lms[2]]] and one["first_irregular"].tolist() == [0] and one["pairings"].tolist() == [2]
    for bad in ([[1.5, 0, 2]], [[-1, 0, 2]], [1, 0, 2]):
        with pytest.raises(ValueError):
            f.joint_innovation(ents, bad)
    for bad in ([[1, 2]], np.zeros((0, 3)), [[0.5, 1, 2]]):
        with pytest.raises(ValueError):
            e.joint_innovation(ents, bad)
    n = len(rec.calls)
    rec.fail = L.EKF_ERR_STATE
    with pytest.raises(L.EkfError) as info:
        e.joint_innovation(ents, hyps[:1])
    assert info.value.status == L.EKF_ERR_STATE and "joint_innovation" in str(info.value) and len(rec.calls) == n + 1


def test_the_scene_measure_model_discards_is_matched_by_measure_model_joint(monkeypatch):
    x, P, _ = J.assert_scene_premises()
    scan = J.ambiguous_scene()[4]
    f, rec = _filter(monkeypatch, x, P)
    assert f.measure_model(scan, J.GATE, 25.0) == [("discarded", 0), ("discarded", 0)]
    assert [c[0] for c in rec.calls] == ["associate"]
    rec.calls.clear()
    out, truncated = f.measure_model_joint(scan, J.GATE, 25.0)
    assert out == [("matched", J.LM_A + 1), ("matched", J.LM_B + 1)] and truncated is False
    assert [(kd, lm + 1 if kd == "matched" else 0) for kd, lm in J.search_brute(x, P, scan, J.GATE, 25.0)] == out
    kinds = [c[0] for c in rec.calls]
    assert kinds == ["associate", "joint", "joint", "observe", "observe"] and rec.calls[0][2] is True       # ONE call per level
    assert [c[3] for c in rec.calls if c[0] == "observe"] == [[J.LM_A, -1], [J.LM_B, -1]] and all(c[4] == J.GATE for c in rec.calls if c[0] == "observe")
    assert [kind for _, kind, _, _, _ in f.log.edits] == ["observe_model", "observe_model"]
    # a beam of one keeps a single hypothesis per level and says so
    rec.calls.clear()
    out1, truncated1 = f.measure_model_joint(scan, J.GATE, 25.0, beam=1)
    assert truncated1 is True and all(len(c[2]) <= 5 for c in rec.calls if c[0] == "joint")


def test_new_and_discarded_entries_ride_along_and_the_new_ones_are_appended_once(monkeypatch):
    x, P, _ = J.assert_scene_premises()
    scan = J.ambiguous_scene()[4]
    far = (M.RELATIVE_XY, [300.0, 300.0], RPOS, 77.0)
    f, rec = _filter(monkeypatch, x, P)
    out, _ = f.measure_model_joint([far, scan[0], far, scan[1]], J.GATE, 25.0, wait=True)
    assert out == [("new", J.N0 + 1), ("matched", J.LM_A + 1), ("new", J.N0 + 2), ("matched", J.LM_B + 1)]
    assert [c[0] for c in rec.calls] == ["associate", "joint", "joint", "observe", "observe", "append"] and rec.calls[-1] == ("append", 2)
    assert all(c[1] == 2 for c in rec.calls if c[0] == "joint") and all(c[5] is True for c in rec.calls if c[0] == "observe")
    assert [kind for _, kind, _, _, _ in f.log.edits] == ["observe_model", "observe_model", "append_model"]


def test_ties_are_resolved_by_pairings_then_d2_then_the_hypothesis(monkeypatch):
    x, P, _ = J.assert_scene_premises()
    scan = J.ambiguous_scene()[4]
    f, rec = _filter(monkeypatch, x, P)
    # every hypothesis equally good: the most pairings win, then the lowest landmarks entry by entry
    rec.canned = lambda hy: [0.5 * sum(1 for c in hy[:k + 1] if c >= 0) for k in range(len(hy))]
    out, _ = f.measure_model_joint(scan, J.GATE, 25.0)
    cands = [sorted(i for i in range(J.N0) if A.pair_d2(x, P, e, i) <= J.GATE) for e in J.scene_entries(scan)]
    first = min((a, b) for a in cands[0] for b in cands[1] if a != b)
    assert out == [("matched", first[0] + 1), ("matched", first[1] + 1)]
    # a smaller joint d2 beats a lower landmark at equal pairings
    rec.canned = lambda hy: [0.0 if k == 0 else (0.1 if hy == [J.LM_B, J.LM_A] else 0.5) * sum(1 for c in hy if c >= 0) for k in range(len(hy))]
    out, _ = f.measure_model_joint(scan, J.GATE, 25.0)
    assert out == [("matched", J.LM_B + 1), ("matched", J.LM_A + 1)]


def test_measure_model_joint_refuses_bad_arguments_before_anything_is_asked_of_the_library(monkeypatch, dense):
    x, P = dense
    f, rec = _filter(monkeypatch, x, P)
    scan = J.ambiguous_scene()[4]
    for kw in (dict(gate_match=9.0, gate_new=8.9), dict(gate_match=float("nan"), gate_new=9.0), dict(gate_match=9.0, gate_new=25.0, joint_p=1.0),
               dict(gate_match=9.0, gate_new=25.0, joint_p=0.0), dict(gate_match=9.0, gate_new=25.0, beam=0), dict(gate_match=9.0, gate_new=25.0, beam=2.5)):
        with pytest.raises(ValueError):
            f.measure_model_joint(scan, **kw)
    for bad in ([], list(scan) * 17, [(2, [5.0], 0.5)], [(5, [5.0], 0.5)], [(1, [5.0, 30.0])]):
        with pytest.raises(ValueError):
            f.measure_model_joint(bad, 9.0, 25.0)
    assert rec.calls == [] and f.log.edits == []
