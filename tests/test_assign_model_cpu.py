"""CPU: ekf_assign_model's host-and-device arithmetic (ekfm::CandList and ekfm::assign_solve of ekf_slam_amd/csrc/assign_math.h, built for
the host by tests/support/assign_model_host.cpp) against the restatement of tests/assign_model_cases.py -- itself pinned by enumeration --
and the Python layers over a stand-in for the library.  No GPU.

The solver runs with a team of 1 lane and with an emulated team of 64 (the kernel's): both must print the same line.  Totals are compared
within 1e-12 relative: both are sums of at most 32 non-negative doubles, good to 31 * 2^-53, and at most 32 * 32 price updates accumulate
2^-53 each of the largest cost, about 1.2e-13.  Assignments are compared where the next-best assignment lies more than 1e-6 relative above
the optimum."""
import ctypes

import numpy as np
import pytest

import assign_model_cases as C
from helpers import RPOS, line_program

INF = float("inf")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return line_program(tmp_path_factory, "assign_model_host")


def num(v):
    return repr(float(v)) if np.isfinite(v) else ("nan" if np.isnan(v) else "inf")


# ------------------------------------------------------------------------------------------------------------------
# the restatement itself
# ------------------------------------------------------------------------------------------------------------------
def small_instances(rng, count, ties):
    for _ in range(count):
        m, N = int(rng.integers(1, 6)), int(rng.integers(0, 7))
        D = rng.integers(1, 6, (m, N)).astype(np.float64) if ties else rng.uniform(0.1, 10.0, (m, N))
        D[rng.random((m, N)) < 0.15] = np.nan
        gates = rng.integers(2, 6, m).astype(np.float64) if ties else rng.uniform(1.0, 8.0, m)
        yield D, gates


def test_the_hungarian_of_the_restatement_is_pinned_by_enumeration():
    rng = np.random.default_rng(21)
    for ties in (False, True):
        for D, gates in small_instances(rng, 150, ties):
            landmark, J = C.solve(D, gates)
            best, optimal = C.brute(D, gates)
            assert abs(J - best) <= 1e-12 * max(best, 1.0)
            used = [i for i in landmark if i >= 0]
            assert len(used) == len(set(used)) and all(D[k, i] <= gates[k] for k, i in enumerate(landmark) if i >= 0)
            if ties:
                assert tuple(int(i) for i in landmark) in optimal
            else:
                assert optimal == [tuple(int(i) for i in landmark)]
                others = [C.total_of(a, D, gates) for a in _all_assignments(D, gates) if a != optimal[0]]
                nxt = C.second_best(D, gates, landmark)
                assert (nxt == INF and not others) or abs(nxt - min(others)) <= 1e-12 * min(others)


def _all_assignments(D, gates):
    import itertools
    options = [[-1] + [int(i) for i in np.flatnonzero(D[k] <= gates[k])] for k in range(D.shape[0])]
    for a in itertools.product(*options):
        used = [i for i in a if i >= 0]
        if len(used) == len(set(used)):
            yield a


def test_the_hungarian_of_the_restatement_against_scipy():
    opt = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(22)
    for _ in range(40):
        m, N = int(rng.integers(1, 33)), int(rng.integers(1, 200))
        D = rng.uniform(0.1, 30.0, (m, N))
        gates = rng.uniform(2.0, 12.0, m)
        _, J = C.solve(D, gates)
        cost = C.dense_costs(D, gates)
        cost[~np.isfinite(cost)] = 1e9
        r, c = opt.linear_sum_assignment(cost)
        assert abs(J - cost[r, c].sum()) <= 1e-12 * J


def test_the_m_cheapest_columns_of_every_row_hold_an_optimum():
    """Why the kept lists suffice: the optimum over each row's m cheapest in-gate columns is the optimum over the full matrix."""
    rng = np.random.default_rng(23)
    for q in range(60):
        m, N = int(rng.integers(1, 13)), int(rng.integers(1, 120))
        D = rng.integers(1, 9, (m, N)).astype(np.float64) if q % 3 == 0 else rng.uniform(0.1, 10.0, (m, N))
        gates = rng.uniform(3.0, 9.0, m)
        _, J = C.solve(D, gates)
        cand, cand_d2, ncand, _ = C.candidate_lists(D, gates, keep=m)
        Ds, _ = C.dense_of_lists(cand, cand_d2, ncand)
        _, Js = C.solve(Ds, gates)
        assert abs(J - Js) <= 1e-12 * J


# ------------------------------------------------------------------------------------------------------------------
# the candidate list
# ------------------------------------------------------------------------------------------------------------------
def merge_line(d2, regular, gate, cuts, reverse):
    pairs = " ".join("%s %d" % (num(v), r) for v, r in zip(d2, regular))
    return "merge %s %d %s %d %s %d" % (num(gate), len(d2), pairs, len(cuts) + 1, " ".join(str(c) for c in cuts), int(reverse))


def _key_lists():
    rng = np.random.default_rng(11)
    big = rng.uniform(0.5, 50.0, 700)
    big[[3, 90, 300, 699]] = 0.25                 # an exact four-way tie for the first place
    big[[64, 65]] = 0.375                         # ... and a pair tied just behind it
    big[100:140] = 2.0                            # forty equal keys: the cut at 32 falls inside a tie
    reg = np.ones(700, dtype=int)
    reg[[5, 256, 511]] = 0                        # irregular entries: never candidates
    big[[5, 256]] = np.nan
    big[511] = 0.001                              # (an irregular entry's d2 is not looked at)
    return [("700 with ties", big, reg), ("five", np.array([4.0, 1.0, 2.0, 2.0, 7.0]), np.ones(5, dtype=int)),
            ("a single candidate", np.array([np.nan, 3.5, np.nan]), np.array([0, 1, 0])), ("none", np.array([np.nan, np.nan]), np.array([0, 0])),
            ("empty", np.zeros(0), np.zeros(0, dtype=int))]


def test_cand_merge_gives_the_sequential_list_for_every_partition(host):
    rng = np.random.default_rng(12)
    seen = set()
    for name, d2, reg in _key_lists():
        n = len(d2)
        row = np.where(reg == 1, d2, np.nan)
        for gate in (9.21, 1e6, 0.25, 0.1):         # some inside, more than 32 inside, the tie alone, none
            cand, cand_d2, ncand, within = C.candidate_lists(row[None, :], [gate])
            seen.add((int(within[0]) > 32, int(within[0]) == 0))
            want = [float(ncand[0])] + [float(i) for i in cand[0]] + list(cand_d2[0])
            splits = [[], list(range(64, n, 64)), list(range(256, n, 256)), sorted(rng.integers(0, n + 1, 9).tolist()), list(range(1, n))]
            lines = [merge_line(d2, reg, gate, cuts, rev) for cuts in splits for rev in (0, 1)]
            for r in host(lines):
                whole, merged = r[:65], r[65:]
                np.testing.assert_array_equal(whole, merged, err_msg=name)
                np.testing.assert_array_equal(whole, want, err_msg=name)
    assert (True, False) in seen and (False, True) in seen and (False, False) in seen
    cand, _, ncand, within = C.candidate_lists(np.where(_key_lists()[0][2] == 1, _key_lists()[0][1], np.nan)[None, :], [2.0])
    assert cand[0][:6].tolist() == [3, 90, 300, 699, 64, 65] and within[0] > 32 and ncand[0] == 32      # the lower index first, in every place
    tied = [int(i) for i in cand[0] if 100 <= i < 140]
    assert tied == list(range(100, 100 + len(tied))) and 0 < len(tied) < 40 and cand[0][-1] == tied[-1]  # the cut falls inside the forty equal keys


# ------------------------------------------------------------------------------------------------------------------
# the solver
# ------------------------------------------------------------------------------------------------------------------
def run_solver(host, cand, cand_d2, ncand, gates):
    """(landmark, d2, total) of the host build, run with a team of 1 and with an emulated team of 64: the two lines must be equal."""
    one, wide = host([C.solve_line(1, cand, cand_d2, ncand, gates), C.solve_line(64, cand, cand_d2, ncand, gates)])
    np.testing.assert_array_equal(one, wide)
    m = len(ncand)
    return np.array(one[:m], dtype=np.int64), np.array(one[m:2 * m]), one[2 * m]


def check_feasible(landmark, d2, total, cand, cand_d2, ncand, gates):
    used = [int(i) for i in landmark if i >= 0]
    assert len(used) == len(set(used))
    J = 0.0
    for k, i in enumerate(landmark):
        if i >= 0:
            s = list(cand[k][:ncand[k]]).index(i)
            assert d2[k] == cand_d2[k][s]
            J += d2[k]
        else:
            assert d2[k] == INF
            J += gates[k]
    assert total == J


def sparse_instance(rng, q):
    """m rows with 0 to 32 candidates each out of a pool of landmarks small enough that rows share columns."""
    m = 1 + q % 32
    pool = int(rng.integers(1, 4)) * m + int(rng.integers(1, 40))
    lms = rng.choice(5000, pool, replace=False)
    gates = rng.uniform(4.0, 12.0, m)
    D = np.full((m, 5000), np.nan)
    for k in range(m):
        n = 0 if rng.random() < 0.1 else int(rng.integers(0, min(pool, 32) + 1))
        pick = rng.choice(lms, n, replace=False)
        D[k, pick] = rng.integers(1, 5, n).astype(np.float64) if q % 3 == 0 else rng.uniform(0.01, gates[k], n)
    return D, gates


def test_the_solver_on_random_sparse_instances(host):
    rng = np.random.default_rng(31)
    compared, worst, sizes = 0, 0.0, set()
    for q in range(320):
        D, gates = sparse_instance(rng, q)
        cols = np.flatnonzero(np.any(~np.isnan(D), axis=0))
        Dc = D[:, cols] if cols.size else np.full((D.shape[0], 1), np.nan)
        cand, cand_d2, ncand, _ = C.candidate_lists(D, gates)
        landmark, d2, total = run_solver(host, cand, cand_d2, ncand, gates)
        check_feasible(landmark, d2, total, cand, cand_d2, ncand, gates)
        want, J, rel = C.gap(Dc, gates)
        worst = max(worst, abs(total - J) / J)
        assert abs(total - J) <= 1e-12 * J, (q, total, J)
        if rel > 1e-6:
            compared += 1
            np.testing.assert_array_equal(landmark, np.where(want >= 0, cols[np.maximum(want, 0)] if cols.size else -1, -1), err_msg=str(q))
        sizes.add((D.shape[0], int(ncand.min()), int(ncand.max())))
    print("320 instances: worst relative error of the total %.2e; the assignment itself compared on %d" % (worst, compared))
    assert compared >= 150 and {s[0] for s in sizes} == set(range(1, 33)) and any(s[1] == 0 for s in sizes) and any(s[2] == 32 for s in sizes)


def lists_of(rows):
    """cand, cand_d2, ncand of rows given as {landmark: d2}, ordered by (d2, landmark)."""
    m = len(rows)
    cand, cand_d2, ncand = np.full((m, 32), -1, dtype=np.int64), np.full((m, 32), INF), np.zeros(m, dtype=np.int64)
    for k, row in enumerate(rows):
        for s, (d2, lm) in enumerate(sorted((d2, lm) for lm, d2 in row.items())):
            cand[k, s], cand_d2[k, s] = lm, d2
        ncand[k] = len(row)
    return cand, cand_d2, ncand


def test_the_solver_where_greedy_nearest_neighbour_is_wrong(host):
    cand, cand_d2, ncand = lists_of([{1: 1.0, 2: 1.2}, {1: 1.1, 2: 5.0}])
    landmark, d2, total = run_solver(host, cand, cand_d2, ncand, [4.0, 4.0])
    assert landmark.tolist() == [2, 1] and d2.tolist() == [1.2, 1.1] and total == 1.2 + 1.1 and abs(total - 2.3) < 1e-15
    # (the second row's 5.0 lies outside its gate in the call itself; the solver takes the lists as they are given)
    want, J = C.solve(np.array([[np.nan, 1.0, 1.2], [np.nan, 1.1, 5.0]]), [4.0, 4.0])
    assert want.tolist() == [2, 1] and abs(J - 2.3) < 1e-15


def test_thirty_two_rows_contend_for_three_columns(host):
    rng = np.random.default_rng(32)
    rows = [{7: float(rng.uniform(0.5, 3.0)), 300: float(rng.uniform(0.5, 3.0)), 39999: float(rng.uniform(0.5, 3.0))} for _ in range(32)]
    gates = [4.0] * 32
    cand, cand_d2, ncand = lists_of(rows)
    landmark, d2, total = run_solver(host, cand, cand_d2, ncand, gates)
    check_feasible(landmark, d2, total, cand, cand_d2, ncand, gates)
    assert sorted(int(i) for i in landmark if i >= 0) == [7, 300, 39999] and (landmark < 0).sum() == 29
    D, lms = C.dense_of_lists(cand, cand_d2, ncand)
    want, J, rel = C.gap(D, gates)
    assert rel > 1e-6 and abs(total - J) <= 1e-12 * J
    np.testing.assert_array_equal(landmark, [lms[i] if i >= 0 else -1 for i in want])


def test_every_gate_below_every_d2_leaves_every_row_out(host):
    # what the call hands the solver then: rows without a candidate
    cand, cand_d2, ncand = lists_of([{}] * 5)
    gates = [0.5, 0.25, 1.0, 0.125, 2.0]
    landmark, d2, total = run_solver(host, cand, cand_d2, ncand, gates)
    assert landmark.tolist() == [-1] * 5 and np.all(np.isinf(d2)) and total == sum(gates)
    # ... and a gate that is simply the cheaper choice although candidates are listed
    cand, cand_d2, ncand = lists_of([{3: 2.0, 4: 3.0}, {3: 2.5}])
    landmark, _, total = run_solver(host, cand, cand_d2, ncand, [1.0, 1.5])
    assert landmark.tolist() == [-1, -1] and total == 2.5


def test_exact_ties_return_one_of_the_enumerated_optima(host):
    rng = np.random.default_rng(33)
    hits = 0
    for D, gates in small_instances(rng, 120, True):
        cand, cand_d2, ncand, _ = C.candidate_lists(D, gates)
        landmark, d2, total = run_solver(host, cand, cand_d2, ncand, gates)
        check_feasible(landmark, d2, total, cand, cand_d2, ncand, gates)
        best, optimal = C.brute(D, gates)
        assert total == best and tuple(int(i) for i in landmark) in optimal        # (small whole numbers: the sums are exact)
        hits += len(optimal) > 1
    assert hits >= 30
    # two identical landmarks seen by two observations: four pairs, two optimal assignments
    cand, cand_d2, ncand = lists_of([{9: 1.5, 31: 1.5}, {9: 2.5, 31: 2.5}])
    landmark, _, total = run_solver(host, cand, cand_d2, ncand, [9.0, 9.0])
    assert sorted(landmark.tolist()) == [9, 31] and total == 4.0


# ------------------------------------------------------------------------------------------------------------------
# the Python layers over a stand-in for the library
# ------------------------------------------------------------------------------------------------------------------
class _Lib:
    """Answers ekf_assign_model with canned results and records what the policy then asks of the library."""

    def __init__(self, N, assigned, matches):
        self.N, self.assigned, self.matches, self.calls = N, assigned, matches, []

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

    def ekf_assign_model(self, h, arr, m, out, match, cand, cand_d2, total):
        self.calls.append(("assign", [(arr[k].model, list(arr[k].lm), arr[k].gate) for k in range(m)], bool(cand), bool(cand_d2)))
        J = 0.0
        for k in range(m):
            out[k].landmark, out[k].d2, out[k].ncand = self.assigned[k]
            match[k].best, match[k].second, match[k].d2_best, match[k].d2_second, match[k].within_gate, match[k].irregular = self.matches[k]
            J += out[k].d2 if out[k].landmark >= 0 else arr[k].gate
            if cand:
                cand[k * 32] = out[k].landmark if out[k].landmark >= 0 else match[k].best
                cand_d2[k * 32] = match[k].d2_best
        total._obj.value = J
        return 0

    def ekf_observe_model(self, h, pobs, pres):
        o = pobs._obj
        self.calls.append(("observe", o.model, list(o.lm), o.gate))
        return 0

    def ekf_append_model(self, h, arr, m, pfirst):
        self.calls.append(("append", m))
        pfirst._obj.value = self.N
        self.N += m
        return 0

    def ekf_status_string(self, rc):
        return b"call not valid in the current state"

    def ekf_last_error(self, h):
        return b"assign_model: injected"


RB = np.array([[0.02, 0.0], [0.0, 0.5]])
ENTRIES = [(1, [5.0, 30.0], RB), (4, [2.0, -1.0], RPOS, 77.0), (1, [6.0, 10.0], RB), (4, [3.0, 3.0], RPOS), (1, [9.0, -45.0], RB)]


def test_the_layers_and_the_policy_over_a_stand_in(monkeypatch):
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import engine as E
    from ekf_slam_amd import slam as S
    from ekf_slam_amd.trajectory import TrajectoryLog
    assert ctypes.sizeof(L.EkfModelAssigned) == 32 and L.EKF_ASSIGN_MODEL_MAX == 32 and L.EKF_ASSIGN_CANDIDATES == 32
    # (landmark, d2, ncand) and (best, second, d2_best, d2_second, within_gate, irregular), 0-based, gate_match = 9, gate_new = 25
    assigned = [(4, 0.5, 2), (-1, INF, 0), (2, 1.5, 2), (-1, INF, 0), (-1, INF, 1)]
    matches = [(4, 2, 0.5, 0.75, 2, 0),          # matched: two inside the gate, the assignment decides
               (9, 1, 40.0, 55.0, 0, 0),         # new: nothing inside the gate and the best beyond gate_new
               (4, 2, 1.0, 1.5, 2, 0),           # matched to its SECOND: the first entry keeps landmark 4
               (3, 5, 12.0, 90.0, 0, 0),         # between the gates: discarded
               (4, 6, 3.0, 80.0, 1, 0)]          # left out although landmark 4 is inside its gate: discarded
    rec = _Lib(10, assigned, matches)
    monkeypatch.setattr(L, "lib", lambda: rec)
    e = E.Engine(capacity=16)
    ents = [dict(model=int(en[0]), z=en[1], R=en[2], gate=9.0) for en in ENTRIES]
    res = e.assign_model(ents)
    assert rec.calls[-1] == ("assign", [(en[0], [-1, -1], 9.0) for en in ENTRIES], False, False)
    assert res["landmark"].tolist() == [4, -1, 2, -1, -1] and res["ncand"].tolist() == [2, 0, 2, 0, 1] and res["total"] == 0.5 + 9.0 + 1.5 + 9.0 + 9.0
    assert res["best"].tolist() == [4, 9, 4, 3, 4] and res["within_gate"].tolist() == [2, 0, 2, 0, 1] and "cand" not in res
    full = e.assign_model(ents, want_candidates=True)
    assert rec.calls[-1][2:] == (True, True) and full["cand"].shape == full["cand_d2"].shape == (5, 32) and full["cand"][0, 0] == 4 and full["cand"][0, 1] == -1
    f = S.EKF_SLAM(capacity=16)
    one = f.assign_model(ents, want_candidates=True)             # 1-based above the engine, 0 = left out or none
    assert one["landmark"].tolist() == [5, 0, 3, 0, 0] and one["best"].tolist() == [5, 10, 5, 4, 5] and one["cand"][0, :2].tolist() == [5, 0]
    f.log = TrajectoryLog()
    del rec.calls[:]
    out = f.measure_model_assigned(ENTRIES, 9.0, 25.0)
    assert out == [("matched", 5), ("new", 11), ("matched", 3), ("discarded", 0), ("discarded", 0)]
    assert rec.calls == [("assign", [(en[0], [-1, -1], 9.0) for en in ENTRIES], False, False), ("observe", 1, [4, -1], 9.0), ("observe", 1, [2, -1], 9.0),
                         ("append", 1)]
    assert [kind for _, kind, _, _, _ in f.log.edits] == ["observe_model", "observe_model", "append_model"]         # the assignment is not logged
    with pytest.raises(ValueError):
        f.measure_model_assigned(ENTRIES, 9.0, 5.0)
    with pytest.raises(ValueError):
        f.measure_model_assigned([(2, [5.0], 0.1)], 9.0, 25.0)
