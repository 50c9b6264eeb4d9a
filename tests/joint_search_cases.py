"""Shared side of the ekf_joint_search tests: the cluster scenes, the level-synchronous search restated in NumPy on the dense state (the
loop of measure_model_joint, over ALL scan indices as the device walks it), the same loop driven through an engine's own assign_model and
joint_innovation calls (the GPU tests' yardstick), and the premises of the scenes asserted where they are built.  No GPU, no library."""
import functools

import numpy as np

import associate_model_cases as A
import joint_cases as J
import model_obs_cases as M
from helpers import RPOS
from removal_cases import lowrank_data

N0 = J.N0
GATE, JOINT_P = J.GATE, 0.99
CAND, BEAM_MAX = 4, 64
LM0 = 40                                   # the cluster's first landmark (0-based)
ROWS_OF = M.ROWS


def cluster_scene(K, N=N0, lm0=LM0):
    """(x, s, d, U, scan): lowrank_data(N = 150, 5) with the robot position variances raised to 1.0, landmarks lm0 = 40 .. 40 + K - 1 on a
    0.6 grid from (6.0, 3.0), four a row, with variance 0.01, and one RELATIVE_XY sighting of each: h(x) plus uniform(-0.04, 0.04) noise,
    R = RPOS."""
    x, s, d, U = lowrank_data(N, 5)
    x, d = x.copy(), d.copy()
    d[0] = d[1] = 1.0
    for q in range(K):
        lm = lm0 + q
        x[3 + 2 * lm:5 + 2 * lm] = (6.0 + 0.6 * (q % 4), 3.0 + 0.6 * (q // 4))
        d[3 + 2 * lm:5 + 2 * lm] = 0.01
    rng = np.random.default_rng(11)
    scan = []
    for q in range(K):
        lm = lm0 + q
        scan.append((M.RELATIVE_XY, M.h_of(M.RELATIVE_XY, x[:3], x[3 + 2 * lm:5 + 2 * lm]) + rng.uniform(-0.04, 0.04, 2), RPOS))
    return x, s, d, U, scan


def mixed_scan(x, LM0=LM0):
    """Entries for the K = 4 cluster state that take every path of a level: a two-row sighting, a FAR sighting with no candidate, the
    one-row models RANGE and BEARING, another two-row sighting."""
    at = lambda lm: x[3 + 2 * lm:5 + 2 * lm]
    rng = np.random.default_rng(12)
    h = lambda model, lm: M.h_of(model, x[:3], at(lm))[:ROWS_OF[model]]
    return [A.entry(M.RELATIVE_XY, h(M.RELATIVE_XY, LM0) + rng.uniform(-0.04, 0.04, 2), RPOS, GATE),
            A.entry(M.RELATIVE_XY, np.array([400.0, -300.0]), RPOS, GATE),
            A.entry(M.RANGE, h(M.RANGE, LM0 + 1) + rng.uniform(-0.02, 0.02, 1), J.R_OF[M.RANGE], GATE),
            A.entry(M.BEARING, h(M.BEARING, LM0 + 2) + rng.uniform(-0.2, 0.2, 1), J.R_OF[M.BEARING], GATE),
            A.entry(M.RELATIVE_XY, h(M.RELATIVE_XY, LM0 + 3) + rng.uniform(-0.04, 0.04, 2), RPOS, GATE)]


def thresholds_even(m, p=JOINT_P):
    """threshold[dof] for dof 0 .. 2m from joint_cases.chi2_table; the odd entries (never read by a scan of two-row models) repeat the
    even one below them."""
    return [J.chi2_table(p, dof - (dof & 1)) for dof in range(2 * m + 1)]


def order_key(h):
    """(hypothesis, pairings, d2) -> the search's order: pairings descending, d2 ascending, hypothesis ascending (Python's tuple order)."""
    return (-h[1], h[2], h[0])


def walk(m, cands, rows, thresholds, beam, d2_of):
    """The level-synchronous search over scan indices 0 .. m - 1.  cands[k]: entry k's candidates in list order (at most CAND are read);
    rows[k]: its real rows; d2_of(level k, extensions as full tuples of k + 1 entries) -> their joint d2 at scan index k.  Returns the
    device call's dict: 'landmark', 'd2', 'dof', 'pairings', 'truncated', 'nalive', 'irregular', 'tested', 'survived', 'alive', 'alive_d2'."""
    alive, truncated, irregular = [((), 0, 0.0, 0)], False, 0          # (hypothesis, pairings, d2, dof)
    tested, survived = [0] * m, [0] * m
    for k in range(m):
        ck = list(cands[k])[:CAND]
        if not ck:
            alive = [(h + (-1,), p, d2, dof) for h, p, d2, dof in alive]
            continue
        ext = [(h + (c,), p + (c >= 0), dof + (rows[k] if c >= 0 else 0), d2) for h, p, d2, dof in alive for c in ck + [-1] if c < 0 or c not in h]
        d2s = d2_of(k, [e[0] for e in ext if e[0][-1] >= 0])
        it = iter(d2s)
        nxt = []
        for h, p, dof, parent_d2 in ext:
            d2 = float(next(it)) if h[-1] >= 0 else parent_d2
            irregular += int(np.isnan(d2))
            if d2 <= thresholds[dof]:
                nxt.append((h, p, d2, dof))
        tested[k], survived[k] = len(ext), len(nxt)
        nxt.sort(key=order_key)
        if len(nxt) > beam:
            nxt, truncated = nxt[:beam], True
        alive = nxt
    best = alive[0]
    return dict(landmark=np.array(best[0], dtype=np.int64), d2=best[2], dof=best[3], pairings=best[1], truncated=truncated, nalive=len(alive),
                irregular=irregular, tested=np.array(tested, dtype=np.int64), survived=np.array(survived, dtype=np.int64),
                alive=np.array([a[0] for a in alive], dtype=np.int64).reshape(len(alive), m), alive_d2=np.array([a[2] for a in alive]))


def candidates_dense(x, P, entries):
    """Per entry the landmarks inside its gate by (d2, index), all of them."""
    D = A.d2_matrix(x, P, entries)
    return [[i for _, i in sorted((float(v), i) for i, v in enumerate(D[k]) if v <= entries[k]["gate"])] for k in range(len(entries))]


def numpy_search(x, P, entries, thresholds, beam, margin=None):
    """walk() on the dense state through joint_dense.  margin: a list that receives |d2 - threshold| / threshold of every tested pairing."""
    m = len(entries)
    rows = [ROWS_OF[e["model"]] for e in entries]
    cands = candidates_dense(x, P, entries)

    def d2_of(k, hyps):
        out = []
        for h in hyps:
            r = J.joint_dense(x, P, entries[:k + 1], list(h))
            out.append(r["d2"])
            if margin is not None and r["dof"] > 0:
                margin.append(abs(r["d2"] - thresholds[r["dof"]]) / thresholds[r["dof"]])
        return out
    res = walk(m, cands, rows, thresholds, beam, d2_of)
    res["ncand"] = [len(c) for c in cands]
    return res


def library_search(e, entries, thresholds, beam):
    """walk() through the engine's own calls on its live state: assign_model(want_candidates=True), then ONE joint_innovation call per
    level with the candidates, as measure_model_joint walks it.  Returns (walk's dict, the assign_model dict)."""
    m = len(entries)
    rows = [ROWS_OF[en["model"]] for en in entries]
    asg = e.assign_model(entries, want_candidates=True)
    cands = [[int(i) for i in asg["cand"][k][:int(asg["ncand"][k])]] for k in range(m)]

    def d2_of(k, hyps):
        if not hyps:
            return []
        full = np.array([list(h) + [-1] * (m - k - 1) for h in hyps], dtype=np.int64).reshape(len(hyps), m)
        return np.asarray(e.joint_innovation(entries, full)["d2_prefix"])[:, k]
    return walk(m, cands, rows, thresholds, beam, d2_of), asg


SEARCH_KEYS = ("landmark", "d2", "dof", "pairings", "truncated", "nalive", "irregular", "tested", "survived", "alive", "alive_d2")


def assert_search_equal(got, want, msg=""):
    """Every field of the search bit for bit (NaN nowhere: a NaN does not survive)."""
    for key in SEARCH_KEYS:
        np.testing.assert_array_equal(np.asarray(got[key]), np.asarray(want[key]), err_msg="%s %s" % (msg, key))


# K -> (d2 of the winner, survivors before the cut per level, extensions per level, truncated) at beam 64
PREMISES = {4: (0.1175, [5, 14, 33, 64], [5, 21, 52, 109], False),
            6: (0.1862, [5, 20, 66, 145, 128, 113], [5, 22, 81, 223, 190, 153], True),
            8: (0.2445, None, None, True)}


@functools.lru_cache(maxsize=None)
def cluster_reference(K, beam):
    """(x, P, entries, thresholds, numpy_search's dict) of the K-cluster at that beam, computed once and shared; the premises asserted."""
    x, _, d, U, scan = cluster_scene(K)
    P = np.diag(d) + U @ U.T
    ents = J.scene_entries(scan, GATE)
    thr = thresholds_even(K)
    margin = []
    ref = numpy_search(x, P, ents, thr, beam, margin)
    truth = list(range(LM0, LM0 + K))
    assert all(n >= CAND for n in ref["ncand"]), ref["ncand"]
    assert ref["landmark"].tolist() == truth and ref["irregular"] == 0
    assert min(margin) > 1e-9, "an extension lies on its threshold: move the seed"
    d2s = np.sort(ref["alive_d2"])
    gaps = np.diff(d2s) / d2s[1:]
    print("cluster K = %d beam %d: d2 %.4f survived %s tested %s truncated %s, closest to a threshold %.2e, smallest gap in the final beam %.2e"
          % (K, beam, ref["d2"], ref["survived"].tolist(), ref["tested"].tolist(), ref["truncated"], min(margin), gaps.min() if gaps.size else 1.0))
    if beam == BEAM_MAX:
        d2, survived, tested, truncated = PREMISES[K]
        assert abs(ref["d2"] - d2) < 5e-4 and ref["truncated"] == truncated
        if survived is not None:
            assert ref["survived"].tolist() == survived and ref["tested"].tolist() == tested
        else:
            assert ref["tested"].max() == 259
    if beam == 2:
        assert ref["truncated"] and np.all(ref["survived"] > 2)
    return x, P, ents, thr, ref
