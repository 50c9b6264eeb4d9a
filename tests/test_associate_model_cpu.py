"""CPU: ekf_associate_model's host-and-device functions (ekfm::assoc_model_d2, ekfm::Match2 of ekf_slam_amd/csrc/device_math.h, built for
the host) against the dense restatement of tests/associate_model_cases.py and against the existing small part, and the Python layers --
Engine.associate_model, the 1-based wrapper, the observe-or-append policy measure_model -- over a stand-in for the library.  No GPU."""
import ctypes

import numpy as np
import pytest

import associate_model_cases as A
import model_obs_cases as M
from helpers import RPOS, line_program
from removal_cases import lowrank_data

INF = float("inf")
N0 = 150


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """The stand-alone host build of ekfm::assoc_model_d2 / Match2: host(lines) -> one list of floats per line."""
    return line_program(tmp_path_factory, "associate_model_host")


@pytest.fixture(scope="module")
def small_host(tmp_path_factory):
    """... and the existing one of ekfm::model_eval / model_small (tests/support/model_eval_host.cpp)."""
    return line_program(tmp_path_factory, "model_eval_host")


@pytest.fixture(scope="module")
def dense():
    """x and the dense P = diag(d) + U U' of lowrank_data(150, 5)."""
    x, _, d, U = lowrank_data(N0, 5)
    return x, np.diag(d) + U @ U.T


def scan(x):
    """One observation per model, each a little beside h(x) at a landmark of its own."""
    out = []
    for model, k, dz, R in ((M.RANGE_BEARING, 7, (0.05, -0.3), np.diag([0.02, 0.5])), (M.RANGE, 40, (0.1,), 0.05), (M.BEARING, 99, (-0.4,), 0.3),
                            (M.RELATIVE_XY, N0 - 1, (0.1, -0.1), RPOS)):
        rows = M.ROWS[model]
        hx = M.h_of(model, x[:3], x[3 + 2 * k:5 + 2 * k])
        out.append(A.entry(model, hx[:rows] + np.asarray(dz), R, 9.21))
    return out


def d2_line(ent, x, P, i):
    """The operands k_assoc_model's lane i loads, for the `d2` line of the host program."""
    o = M.obs(ent["model"], ent["z"], ent["R"], [i])
    z = o["z"].copy()
    if o["rows"] == 1:
        z[1] = 0.0
    a = 3 + 2 * i
    strip6 = [P[t, a + r] for t in range(3) for r in range(2)]
    diag3 = [P[a, a], P[a + 1, a], P[a + 1, a + 1]]
    return "d2 %d %s" % (ent["model"], M.fmt(list(z) + list(M.effective_R(o).reshape(-1)) + list(P[:3, :3].reshape(-1)) + strip6 + diag3 + list(x[:3]) + list(x[a:a + 2])))


# ------------------------------------------------------------------------------------------------------------------
# assoc_model_d2
# ------------------------------------------------------------------------------------------------------------------
def test_assoc_model_d2_matches_the_dense_restatement_for_every_model_and_landmark(host, dense):
    x, P = dense
    entries = scan(x)
    want = A.d2_matrix(x, P, entries)
    got = host([d2_line(ent, x, P, i) for ent in entries for i in range(N0)])
    got_d2 = np.array([r[1] for r in got]).reshape(len(entries), N0)
    assert all(r[0] == 1.0 for r in got) and np.all(np.isfinite(want))
    err = np.abs(got_d2 - want) / want
    print("d2 of %d pairs: worst relative error %.2e; d2 from %.3g to %.3g" % (want.size, err.max(), want.min(), want.max()))
    assert err.max() < 1e-11
    # the observed landmark lies inside the gate; a two-row observation names it (a range or a bearing alone fits other landmarks too)
    for k, lm in enumerate((7, 40, 99, N0 - 1)):
        assert got_d2[k, lm] < 9.21 and (M.ROWS[entries[k]["model"]] == 1 or int(np.argmin(got_d2[k])) == lm)


def test_assoc_model_d2_is_model_small_and_constrain_d2_bit_for_bit(host, small_host, dense):
    x, P = dense
    entries = scan(x)
    lines_new, lines_old = [], []
    for ent in entries:
        for i in range(N0):
            lines_new.append(d2_line(ent, x, P, i))
            lines_old.append(M.small_line(M.obs(ent["model"], ent["z"], ent["R"], [i], None, ent["gate"]), x, P))
    new, old = host(lines_new), small_host(lines_old)
    np.testing.assert_array_equal([r[1] for r in new], [r[2] for r in old])        # d2, through %.17g: equal numbers are equal bits
    assert [r[0] for r in new] == [r[0] for r in old] == [1.0] * len(new)


def test_a_target_on_the_robot_a_non_finite_state_and_a_singular_S_have_no_d2(host, small_host, dense):
    x, P = dense
    ent = A.entry(M.RANGE_BEARING, [3.0, 10.0], np.diag([0.02, 0.5]))
    on_robot = x.copy(); on_robot[3:5] = x[:2]
    lost = x.copy(); lost[3] = np.nan
    flat = np.zeros_like(P)
    cases = [(on_robot, P, ent), (lost, P, ent), (x, flat, A.entry(M.RELATIVE_XY, [1.0, 2.0], np.zeros((2, 2))))]
    got = host([d2_line(e, xs, Ps, 0) for xs, Ps, e in cases])
    old = small_host([M.small_line(M.obs(e["model"], e["z"], e["R"], [0]), xs, Ps) for xs, Ps, e in cases])
    for g, o in zip(got, old):
        assert g[0] == 0.0 and np.isnan(g[1]) and np.isnan(o[2]) and o[1] == M.IRREGULAR


# ------------------------------------------------------------------------------------------------------------------
# Match2
# ------------------------------------------------------------------------------------------------------------------
def match_line(d2, regular, gate, cuts, reverse):
    pairs = " ".join("%s %d" % (repr(float(v)) if np.isfinite(v) else ("nan" if np.isnan(v) else "inf"), r) for v, r in zip(d2, regular))
    return "match %s %d %s %d %s %d" % (repr(float(gate)) if np.isfinite(gate) else "inf", len(d2), pairs, len(cuts) + 1, " ".join(str(c) for c in cuts), int(reverse))


def _lists():
    rng = np.random.default_rng(11)
    big = rng.uniform(0.5, 50.0, 700)
    big[[3, 90, 300, 699]] = 0.25                 # an exact four-way tie for the best
    big[[64, 65]] = 0.375                         # ... and a pair tied just behind it
    reg = np.ones(700, dtype=int)
    reg[[5, 256, 511]] = 0                        # irregular entries: never candidates, counted
    big[[5, 256]] = np.nan
    big[511] = 0.001                              # (an irregular entry's d2 is not looked at)
    big[640] = np.inf                             # a regular landmark at +inf is a candidate, behind every finite one
    tie_second = np.array([4.0, 1.0, 2.0, 2.0, 7.0])
    return [("700 with ties", big, reg), ("tie for second", tie_second, np.ones(5, dtype=int)),
            ("a single candidate", np.array([np.nan, 3.5, np.nan]), np.array([0, 1, 0])), ("only +inf", np.array([np.inf, np.inf]), np.array([1, 1])),
            ("none", np.array([np.nan, np.nan]), np.array([0, 0])), ("empty", np.zeros(0), np.zeros(0, dtype=int))]


def test_match2_merge_gives_the_sequential_record_for_every_partition(host):
    rng = np.random.default_rng(12)
    for name, d2, reg in _lists():
        n = len(d2)
        row = np.where(reg == 1, d2, np.nan)
        for gate in (9.21, INF, 0.25):
            want = A.top_two(row, gate)
            splits = [[], list(range(64, n, 64)), list(range(256, n, 256)), sorted(rng.integers(0, n + 1, 9).tolist()), list(range(1, n))]
            lines = [match_line(d2, reg, gate, cuts, rev) for cuts in splits for rev in (0, 1)]
            for r in host(lines):
                whole, merged = r[:6], r[6:]
                np.testing.assert_array_equal(whole, merged, err_msg=name)
                assert whole == [want["best"], want["second"], want["d2_best"], want["d2_second"], want["within_gate"], want["irregular"]], name
    ties = A.top_two(np.where(_lists()[0][2] == 1, _lists()[0][1], np.nan), 0.25)
    assert (ties["best"], ties["second"], ties["within_gate"], ties["irregular"]) == (3, 90, 4, 3)      # the lower index wins, in both places
    assert A.top_two([np.nan, 3.5, np.nan], INF) == dict(best=1, second=-1, d2_best=3.5, d2_second=INF, within_gate=1, irregular=2)
    assert A.top_two([np.inf, np.inf], INF)["second"] == 1 and A.top_two([np.inf, np.inf], 5.0)["within_gate"] == 0
    assert A.top_two([], 1.0) == dict(best=-1, second=-1, d2_best=INF, d2_second=INF, within_gate=0, irregular=0)


# ------------------------------------------------------------------------------------------------------------------
# the Python layers over a stand-in for the library
# ------------------------------------------------------------------------------------------------------------------
class _Lib:
    """Answers ekf_associate_model with canned matches and records what the policy then asks of the library."""

    def __init__(self, N, canned):
        self.N, self.canned, self.calls, self.fail = N, canned, [], 0

    def ekf_config_default(self, pcfg, mode):
        from ekf_slam_amd import _lib as L
        cfg = ctypes.cast(pcfg, ctypes.POINTER(L.EkfConfig)).contents
        cfg.mode, cfg.batch = mode, 1
        return 0

    def ekf_create(self, pcfg, ph):
        ctypes.cast(ph, ctypes.POINTER(ctypes.c_void_p)).contents.value = 0x1000
        return 0

    def ekf_destroy(self, h):
        return 0

    def ekf_num_landmarks(self, h, pn):
        pn._obj.value = self.N
        return 0

    def ekf_associate_model(self, h, arr, m, out, d2_all):
        self.calls.append(("associate", [(arr[k].model, list(arr[k].z), list(arr[k].R), list(arr[k].lm), list(arr[k].anchor), arr[k].gate) for k in range(m)],
                           bool(d2_all)))
        if self.fail:
            return self.fail
        for k in range(m):
            out[k].best, out[k].second, out[k].d2_best, out[k].d2_second, out[k].within_gate, out[k].irregular = self.canned[k]
        if d2_all:
            for q in range(m * self.N):
                d2_all[q] = 100.0 + q
        return 0

    def ekf_observe_model(self, h, pobs, pres):
        o = pobs._obj
        self.calls.append(("observe", o.model, list(o.z), list(o.R), list(o.lm), o.gate, pres is not None))
        return 0

    def ekf_append_model(self, h, arr, m, pfirst):
        self.calls.append(("append", [(arr[b].model, list(arr[b].z), list(arr[b].R), arr[b].signature) for b in range(m)]))
        pfirst._obj.value = self.N
        self.N += m
        return 0

    def ekf_status_string(self, rc):
        return b"call not valid in the current state"

    def ekf_last_error(self, h):
        return b"associate_model: injected"


def test_engine_and_slam_layers_marshal_a_scan_once(monkeypatch):
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import engine as E
    from ekf_slam_amd import slam as S
    assert ctypes.sizeof(L.EkfModelMatch) == 48 and L.EKF_ASSOCIATE_MODEL_MAX == 32 and "ekf_associate_model" in L.SIGNATURES
    canned = [(4, 2, 0.5, 7.0, 1, 0), (-1, -1, INF, INF, 0, 3)]
    rec = _Lib(3, canned)
    monkeypatch.setattr(L, "lib", lambda: rec)
    e = E.Engine(capacity=16)
    ents = [dict(model=1, z=[5.0, 30.0], R=[[0.5, 0.1], [0.1, 0.25]], gate=9.0), dict(model=2, z=[7.5], R=0.5)]
    res = e.associate_model(ents)
    assert rec.calls[-1] == ("associate", [(1, [5.0, 30.0], [0.5, 0.1, 0.1, 0.25], [-1, -1], [0.0, 0.0], 9.0),
                                           (2, [7.5, 0.0], [0.5, 0.0, 0.0, 0.0], [-1, -1], [0.0, 0.0], INF)], False)
    assert res["best"].tolist() == [4, -1] and res["second"].tolist() == [2, -1] and res["d2_best"].tolist() == [0.5, INF]
    assert res["within_gate"].tolist() == [1, 0] and res["irregular"].tolist() == [0, 3] and "d2_all" not in res
    full = e.associate_model(ents, want_d2=True)
    assert rec.calls[-1][2] is True and full["d2_all"].shape == (2, 3) and full["d2_all"].tolist() == [[100.0, 101.0, 102.0], [103.0, 104.0, 105.0]]
    f = S.EKF_SLAM(capacity=16)
    one = f.associate_model(ents)                               # 1-based above the engine, 0 = none
    assert one["best"].tolist() == [5, 0] and one["second"].tolist() == [3, 0] and one["d2_second"].tolist() == [7.0, INF]
    rec.fail = L.EKF_ERR_STATE
    with pytest.raises(L.EkfError) as info:
        e.associate_model(ents)
    assert info.value.status == L.EKF_ERR_STATE and "associate_model" in str(info.value)


def _filter(monkeypatch, N, canned):
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import slam as S
    from ekf_slam_amd.trajectory import TrajectoryLog
    rec = _Lib(N, canned)
    monkeypatch.setattr(L, "lib", lambda: rec)
    f = S.EKF_SLAM_UC(capacity=64)
    f.log = TrajectoryLog()
    return f, rec


RB = np.array([[0.02, 0.0], [0.0, 0.5]])
ENTRIES = [(1, [5.0, 30.0], RB), (4, [2.0, -1.0], RPOS, 77.0), (1, [6.0, 10.0], RB), (4, [3.0, 3.0], RPOS), (1, [9.0, -45.0], RB), (4, [-4.0, 1.0], RPOS),
           (1, [2.5, 170.0], RB)]


def test_measure_model_observes_the_matched_appends_the_new_and_discards_the_rest(monkeypatch):
    # (best, second, d2_best, d2_second, within_gate, irregular), 0-based, as the library answers with gate = gate_match = 9
    canned = [(4, 2, 0.5, 30.0, 1, 0),            # matched: landmark 4 alone inside the gate
              (9, 1, 40.0, 55.0, 0, 0),           # new: the best lies beyond gate_new = 25
              (7, 8, 1.0, 2.0, 2, 0),             # ambiguous: two inside the gate
              (3, 5, 12.0, 90.0, 0, 0),           # between the gates
              (4, 6, 0.75, 80.0, 1, 0),           # matched to landmark 4 as well, with the larger d2: loses it
              (6, 0, 2.0, 70.0, 1, 0),            # matched, tied with the last entry for landmark 6: the lower entry keeps it
              (6, 0, 2.0, 60.0, 1, 0)]
    f, rec = _filter(monkeypatch, 10, canned)
    out = f.measure_model(ENTRIES, 9.0, 25.0)
    assert out == [("matched", 5), ("new", 11), ("discarded", 0), ("discarded", 0), ("discarded", 0), ("matched", 7), ("discarded", 0)]
    res = {k: np.array([c[q] for c in canned]) for q, k in enumerate(("best", "second", "d2_best", "d2_second", "within_gate", "irregular"))}
    # the pure restatement of the policy agrees (it does not number the new landmarks)
    assert [(kd, lm + 1) for kd, lm in A.policy(res, 25.0)] == [(kd, lm if kd != "new" else 0) for kd, lm in out]
    assert [c[0] for c in rec.calls] == ["associate", "observe", "observe", "append"]
    assoc = rec.calls[0]
    assert [a[0] for a in assoc[1]] == [1, 4, 1, 4, 1, 4, 1] and all(a[3] == [-1, -1] and a[5] == 9.0 for a in assoc[1]) and assoc[2] is False
    assert rec.calls[1] == ("observe", 1, [5.0, 30.0], [0.02, 0.0, 0.0, 0.5], [4, -1], 9.0, False)          # scan order, the step gated again
    assert rec.calls[2] == ("observe", 4, [-4.0, 1.0], [0.02, 0.005, 0.005, 0.03], [6, -1], 9.0, False)
    assert rec.calls[3] == ("append", [(4, [2.0, -1.0], [0.02, 0.005, 0.005, 0.03], 77.0)])
    # everything that changed the state went through the logged methods, in that order; the association is not logged
    assert [kind for _, kind, _, _, _ in f.log.edits] == ["observe_model", "observe_model", "append_model"]


def test_measure_model_on_an_empty_map_appends_the_whole_scan_in_one_call(monkeypatch):
    f, rec = _filter(monkeypatch, 0, [(-1, -1, INF, INF, 0, 0)] * 3)
    out = f.measure_model(ENTRIES[:3], 9.0, 9.0, wait=True)
    assert out == [("new", 1), ("new", 2), ("new", 3)]
    assert [c[0] for c in rec.calls] == ["associate", "append"]
    assert [(e[0], e[3]) for e in rec.calls[1][1]] == [(1, 1.0), (4, 77.0), (1, 3.0)]      # a signature left out: the landmark's own number


def test_measure_model_waits_for_the_matched_steps_when_asked(monkeypatch):
    f, rec = _filter(monkeypatch, 10, [(4, 2, 0.5, 30.0, 1, 0)])
    assert f.measure_model(ENTRIES[:1], 9.0, 25.0, wait=True) == [("matched", 5)]
    assert rec.calls[1] == ("observe", 1, [5.0, 30.0], [0.02, 0.0, 0.0, 0.5], [4, -1], 9.0, True)


def test_measure_model_refuses_bad_arguments_before_anything_is_asked_of_the_library(monkeypatch):
    f, rec = _filter(monkeypatch, 10, [(4, 2, 0.5, 30.0, 1, 0)] * 40)
    for kw in (dict(gate_match=9.0, gate_new=8.9), dict(gate_match=float("nan"), gate_new=9.0), dict(gate_match=1.0, gate_new=float("nan"))):
        with pytest.raises(ValueError):
            f.measure_model(ENTRIES[:2], **kw)
    for bad in ([], ENTRIES * 5, [(2, [5.0], 0.5)], [(3, [5.0], 0.5)], [(5, [5.0], 0.5)], [(1, [5.0, 30.0])]):
        with pytest.raises(ValueError):
            f.measure_model(bad, 9.0, 25.0)
    assert rec.calls == [] and f.log.edits == []
