"""CPU: what ekf_joint_search adds to ekf_slam_amd/csrc/device_math.h, built for the host by tests/support/joint_search_host.cpp -- the
row-append of the joint factorisation against the right-looking one run on the whole matrix (bit for bit), the order of the survivors
against Python's tuple order, the cut -- the same program under the address and undefined-behaviour sanitizers, the NumPy restatement
of the search against the brute-force enumeration of tests/joint_cases.py, and the Python layers over a stand-in for the library."""
import ctypes
import itertools
import subprocess

import numpy as np
import pytest

import associate_model_cases as A
import joint_cases as J
import joint_search_cases as S
import model_obs_cases as M
from helpers import RecorderBase, host_build, line_program


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return line_program(tmp_path_factory, "joint_search_host")


def spd(n, seed):
    rng = np.random.default_rng(seed)
    B = rng.normal(size=(n, n + 3))
    return B @ B.T + 0.1 * np.eye(n), rng.normal(size=n)


def append_line(S_, nu, lanes=1):
    return "append %d %d %s %s" % (len(nu), lanes, " ".join(repr(float(v)) for v in np.asarray(S_).reshape(-1)), " ".join(repr(float(v)) for v in nu))


def parse_append(row, n):
    np_ = n // 2
    return int(row[0]), int(row[1]), int(row[2]), np.array(row[3:3 + np_]), np.array(row[3 + np_:3 + 2 * np_])


# the tolerance tests/test_joint_cpu.py uses for a prefix against numpy.linalg.solve on the same S
RTOL_SOLVE = 1e-9


@pytest.mark.parametrize("n", [2, 4, 6, 16, 64])
@pytest.mark.parametrize("lanes", [1, 7, 64])
def test_rows_appended_two_at_a_time_are_the_right_looking_factorisation_bit_for_bit(host, n, lanes):
    S_, nu = spd(n, n)
    mism, bad, bad2, pre, pre2 = parse_append(host([append_line(S_, nu, lanes)])[0], n)
    assert (mism, bad, bad2) == (0, n // 2, n // 2)
    np.testing.assert_array_equal(pre, pre2)
    want = [float(nu[:2 * p + 2] @ np.linalg.solve(S_[:2 * p + 2, :2 * p + 2], nu[:2 * p + 2])) for p in range(n // 2)]
    np.testing.assert_allclose(pre2, want, rtol=RTOL_SOLVE)


def test_a_one_row_pairing_appends_an_empty_second_row(host):
    S_, nu = spd(6, 9)
    for i in (3,):                                            # pairing 1 is a one-row model: [[s, 0], [0, 1]], nu_1 = 0
        S_[i, :] = 0.0; S_[:, i] = 0.0; S_[i, i] = 1.0; nu[i] = 0.0
    mism, bad, bad2, pre, pre2 = parse_append(host([append_line(S_, nu)])[0], 6)
    assert (mism, bad, bad2) == (0, 3, 3)
    keep = [0, 1, 2, 4, 5]
    np.testing.assert_allclose(pre2[2], nu[keep] @ np.linalg.solve(S_[np.ix_(keep, keep)], nu[keep]), rtol=RTOL_SOLVE)
    np.testing.assert_array_equal(pre, pre2)


@pytest.mark.parametrize("where", [0, 2, 4])
@pytest.mark.parametrize("row", [0, 1])
def test_a_failing_pivot_stops_both_at_the_same_pairing(host, where, row):
    n = 10
    S_, nu = spd(n, 21)
    i = 2 * where + row
    S_[i, i] = -abs(S_[i, i])                                 # the pivot of that row ends below zero
    mism, bad, bad2, pre, pre2 = parse_append(host([append_line(S_, nu, 3)])[0], n)
    assert (mism, bad, bad2) == (0, where, where)
    assert np.all(np.isfinite(pre2[:where])) and np.all(np.isnan(pre2[where:])) and np.all(np.isnan(pre[where:]))
    np.testing.assert_array_equal(pre[:where], pre2[:where])
    S_[i, i] = float("nan")
    assert parse_append(host([append_line(S_, nu)])[0], n)[:3] == (0, where, where)


def before_line(a, b):
    """a, b: (hypothesis tuple, pairings, d2), the hypotheses equally long; the last entry travels apart, as the kernel holds it."""
    part = lambda h: "%d %r %s %d" % (h[1], float(h[2]), " ".join(str(v) for v in h[0][:-1]), h[0][-1])
    return "before %d %s %s" % (len(a[0]) - 1, part(a), part(b))


def test_the_order_is_pythons_tuple_order(host):
    rng = np.random.default_rng(4)
    hyps = []
    for _ in range(60):
        h = tuple(int(v) for v in rng.choice([-1, 3, 4, 7, 40, 41], 4))
        hyps.append((h, sum(c >= 0 for c in h), float(rng.choice([0.0, 0.25, 0.5, 1.0 / 3.0]))))      # exact d2 ties, ties in pairings
    hyps = list({h[0]: h for h in hyps}.values())
    pairs = list(itertools.permutations(range(len(hyps)), 2))
    got = host([before_line(hyps[i], hyps[j]) for i, j in pairs])
    for (i, j), g in zip(pairs, got):
        assert bool(g[0]) == (S.order_key(hyps[i]) < S.order_key(hyps[j])), (hyps[i], hyps[j])
    # ranks counted from it are the positions of the sorted list: the select step's rule
    rank = [sum(int(g[0]) for (i, j), g in zip(pairs, got) if j == q) for q in range(len(hyps))]
    assert [hyps[q] for q in np.argsort(rank)] == sorted(hyps, key=S.order_key) and sorted(rank) == list(range(len(hyps)))
    # a hypothesis never stands before itself; -1 sorts before every landmark
    same = ((5, -1), 1, 0.5)
    assert host([before_line(same, same)])[0][0] == 0
    assert host([before_line(((5, -1), 1, 0.5), ((5, 0), 1, 0.5))])[0][0] == 1


def test_nan_never_passes_and_exactly_beam_survivors_is_no_cut(host):
    rows = host(["passes nan 5.0", "passes 5.0 5.0", "passes 5.000000000000001 5.0", "passes 0.0 0.0", "passes inf 5.0",
                 "cut 64 64", "cut 65 64", "cut 1 64", "cut 3 2", "cut 2 2"])
    assert [int(r[0]) for r in rows[:5]] == [0, 1, 0, 1, 0]
    assert [(int(r[0]), int(r[1])) for r in rows[5:]] == [(64, 0), (64, 1), (1, 0), (2, 1), (2, 0)]


def test_the_host_program_is_clean_under_the_sanitizers(tmp_path):
    exe = host_build("joint_search_host", str(tmp_path / "joint_search_host_san"), ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                                                                    "-mfma", "-ffp-contract=off"])
    lines = [append_line(*spd(n, n), lanes=5) for n in (2, 6, 64)]
    bad_S, bad_nu = spd(8, 3)
    bad_S[5, 5] = -1.0
    lines += [append_line(bad_S, bad_nu), before_line(((1, 2, -1), 2, 0.5), ((1, 2, 3), 3, 0.5)), "cut 65 64", "passes nan 1.0"]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    assert len(r.stdout.strip().split("\n")) == len(lines)


# ------------------------------------------------------------------------------------------------------------------
# the NumPy restatement the GPU tests lean on
# ------------------------------------------------------------------------------------------------------------------
def test_the_cluster_scenes_hold_their_premises():
    for K, beam in ((4, 64), (6, 64), (8, 64), (4, 2), (6, 2), (8, 2)):
        S.cluster_reference(K, beam)


def test_the_restated_search_agrees_with_the_enumeration_on_the_two_entry_scene_and_the_small_cluster():
    x, P, ents = J.assert_scene_premises()
    ents = [dict(en, gate=J.GATE) for en in ents]
    got = S.numpy_search(x, P, ents, S.thresholds_even(2), 64)
    _, _, _, _, scan = J.ambiguous_scene()
    brute = J.search_brute(x, P, scan, J.GATE, 25.0)
    assert got["landmark"].tolist() == [lm for _, lm in brute] == [J.LM_A, J.LM_B] and not got["truncated"]
    x4, P4, ents4, thr4, ref4 = S.cluster_reference(4, 64)
    scan4 = S.cluster_scene(4)[4]
    assert ref4["landmark"].tolist() == [lm for _, lm in J.search_brute(x4, P4, scan4, S.GATE, 25.0)]


# ------------------------------------------------------------------------------------------------------------------
# the Python layers over a stand-in for the library
# ------------------------------------------------------------------------------------------------------------------
class Recorder(RecorderBase):
    """ekf_joint_search answered by the NumPy search on a dense state; every other call the policy makes is recorded."""
    last_error = b"joint_search: injected"

    def __init__(self, x, P):
        self.x, self.P, self.calls, self.fail = np.asarray(x), np.asarray(P), [], 0

    def ekf_num_landmarks(self, h, pn):
        pn._obj.value = (self.x.size - 3) // 2
        return 0

    def ekf_joint_search(self, h, arr, m, thr, beam, pres, match, cand, cand_d2, alive, alive_d2):
        from ekf_slam_amd import _lib as L
        self.calls.append(("search", m, beam, bool(cand), bool(alive)))
        if self.fail:
            return self.fail
        ents = []
        for k in range(m):
            Rm = np.array(list(arr[k].R)).reshape(2, 2, order="F")
            ents.append(A.entry(arr[k].model, list(arr[k].z), Rm if M.ROWS[arr[k].model] == 2 else Rm[0, 0], arr[k].gate))
        r = S.numpy_search(self.x, self.P, ents, [thr[d] for d in range(2 * m + 1)], beam)
        res = pres._obj
        for k in range(L.EKF_JOINT_MAX):
            res.lm[k] = int(r["landmark"][k]) if k < m else -1
            res.tested[k] = int(r["tested"][k]) if k < m else 0
            res.survived[k] = int(r["survived"][k]) if k < m else 0
        res.d2, res.dof, res.pairings, res.truncated, res.nalive, res.irregular = r["d2"], r["dof"], r["pairings"], int(r["truncated"]), r["nalive"], 0
        top = A.match(self.x, self.P, ents)[0]
        for k in range(m):
            match[k].best, match[k].second, match[k].d2_best, match[k].d2_second = int(top["best"][k]), int(top["second"][k]), top["d2_best"][k], top["d2_second"][k]
            match[k].within_gate, match[k].irregular = int(top["within_gate"][k]), int(top["irregular"][k])
        if alive:
            for s_, h_ in enumerate(r["alive"]):
                for k in range(m):
                    alive[s_ * m + k] = int(h_[k])
                alive_d2[s_] = float(r["alive_d2"][s_])
        return 0

    def ekf_observe_model(self, h, pobs, pres):
        self.calls.append(("observe", int(pobs._obj.lm[0])))
        return 0


def test_the_python_layers_marshal_once_and_the_policy_makes_one_call(monkeypatch):
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import slam
    assert ctypes.sizeof(L.EkfJointSearchResult) == 544 and (L.EKF_JOINT_SEARCH_CAND, L.EKF_JOINT_SEARCH_BEAM_MAX) == (4, 64)
    assert "ekf_joint_search" in L.SIGNATURES
    x, P, ents, thr, ref = S.cluster_reference(4, 64)
    rec = Recorder(x, P)
    monkeypatch.setattr(L, "lib", lambda: rec)
    f = slam.EKF_SLAM(capacity=160)
    got = f._e.joint_search(ents, thr, 64, want_alive=True)
    for key in ("landmark", "tested", "survived", "alive"):
        np.testing.assert_array_equal(got[key], ref[key])
    assert got["nalive"] == 64 and got["alive"].shape == (64, 4) and not got["truncated"] and "cand" not in got
    assert np.all(got["within_gate"] >= 4) and "match_irregular" in got
    one = f.joint_search(ents, beam=2)
    assert one["landmark"].tolist() == [41, 42, 43, 44] and one["truncated"] and rec.calls[-1] == ("search", 4, 2, False, False)
    with pytest.raises(ValueError):
        f._e.joint_search(ents, thr[:-1])
    with pytest.raises(ValueError):
        f.joint_search(ents, joint_p=1.0)
    scan = [(en["model"], en["z"], en["R"]) for en in ents]
    n = len(rec.calls)
    out, truncated = f.measure_model_joint(scan, S.GATE, 25.0, device_search=True)
    assert out == [("matched", 41 + q) for q in range(4)] and truncated is False
    assert [c[0] for c in rec.calls[n:]] == ["search"] + ["observe"] * 4                     # ONE call in front of the updates
    with pytest.raises(ValueError):
        f.measure_model_joint(scan, S.GATE, 25.0, beam=65, device_search=True)
    rec.fail = L.EKF_ERR_STATE
    with pytest.raises(L.EkfError) as info:
        f._e.joint_search(ents, thr)
    assert info.value.status == L.EKF_ERR_STATE and "joint_search" in str(info.value)


def test_the_python_layers_refuse_in_their_order_before_anything_reaches_the_library(monkeypatch):
    """The stand-in answers every call, so what is refused here is refused by the Python layers: each pair of faults names the one that
    is checked first, and no call is made."""
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import slam
    x, P, ents, thr, _ = S.cluster_reference(4, 64)
    rec = Recorder(x, P)
    monkeypatch.setattr(L, "lib", lambda: rec)
    f = slam.EKF_SLAM(capacity=160)
    scan = [(en["model"], en["z"], en["R"]) for en in ents]

    def refused(fn, word):
        n = len(rec.calls)
        with pytest.raises(ValueError) as info:
            fn()
        assert word in str(info.value) and len(rec.calls) == n, str(info.value)
    # Engine.joint_search: the thresholds before the beam
    refused(lambda: f._e.joint_search(ents, thr[:-1], 2.5), "thresholds")
    refused(lambda: f._e.joint_search(ents, thr + [1.0], 64), "thresholds")
    refused(lambda: f._e.joint_search(ents, thr, 2.5), "beam")
    # the filters' joint_search: joint_p before the engine's checks
    refused(lambda: f.joint_search(ents, joint_p=0.0, beam=2.5), "joint_p")
    refused(lambda: f.joint_search(ents, joint_p=0.5, beam=2.5), "beam")
    # the policy: the gates, joint_p, the beam as a number, the entries, then the device search's own limit
    refused(lambda: f.measure_model_joint(scan, 9.0, 5.0, joint_p=2.0, beam=0, device_search=True), "gate_new")
    refused(lambda: f.measure_model_joint(scan, 9.0, 25.0, joint_p=2.0, beam=0, device_search=True), "joint_p")
    refused(lambda: f.measure_model_joint(scan * 9, 9.0, 25.0, beam=0, device_search=True), "beam")
    refused(lambda: f.measure_model_joint(scan * 9, 9.0, 25.0, beam=65, device_search=True), "entries")
    refused(lambda: f.measure_model_joint([(M.RANGE, [1.0], 0.1)], 9.0, 25.0, beam=65, device_search=True), "one-row model")
    refused(lambda: f.measure_model_joint(scan, 9.0, 25.0, beam=65, device_search=True), "EKF_JOINT_SEARCH_BEAM_MAX")
    # the library's own refusals travel up as EkfError with its status
    rec.fail = L.EKF_ERR_INVALID_ARG
    with pytest.raises(L.EkfError) as info:
        f.measure_model_joint(scan, 9.0, 25.0, device_search=True)
    assert info.value.status == L.EKF_ERR_INVALID_ARG and rec.calls[-1][0] == "search"
