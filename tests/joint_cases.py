"""Pure-NumPy side of the ekf_joint_innovation tests: the dense restatement of a hypothesis (the stacked H, S = H P H' + blockdiag(R),
d2 and its prefixes through numpy.linalg.solve), the scans and scenes the CPU and GPU tests share, the branch and bound of
measure_model_joint restated by brute force, and the premises of the scenes asserted where they are built.  No GPU, no library."""
import itertools

import numpy as np

import associate_model_cases as A
import model_obs_cases as M
from helpers import RPOS
from removal_cases import lowrank_data

N0 = 150
R_OF = {M.RANGE_BEARING: np.diag([0.02, 0.5]), M.RANGE: 0.05, M.BEARING: 0.3, M.RELATIVE_XY: RPOS}
REGULAR, IRREGULAR = 1, 0
U53 = 2.0 ** -53


def dense_state(N=N0, seed=5):
    """x and the dense P = diag(d) + U U' of lowrank_data(N, seed)."""
    x, _, d, U = lowrank_data(N, seed)
    return x, np.diag(d) + U @ U.T


def cycle_scan(x, landmarks, models=(1, 2, 3, 4), seed=3):
    """One entry per landmark of the list, the models cycling, each a little beside h(x) at its landmark (bearings well inside the wrap)."""
    rng = np.random.default_rng(seed)
    out = []
    for q, lm in enumerate(landmarks):
        model = models[q % len(models)]
        rows = M.ROWS[model]
        hx = M.h_of(model, x[:3], x[3 + 2 * lm:5 + 2 * lm])
        out.append(A.entry(model, hx[:rows] + rng.uniform(-0.1, 0.1, rows), R_OF[model]))
    return out


def pairing_obs(ent, lm):
    return M.obs(ent["model"], ent["z"], ent["R"], [int(lm)])


def joint_dense(x, P, entries, hyp):
    """One hypothesis on the dense state: what ekf_joint_innovation reports for it, every output by scan index."""
    x, P = np.asarray(x, dtype=np.float64), np.asarray(P, dtype=np.float64)
    m = len(entries)
    paired = [k for k in range(m) if hyp[k] >= 0]
    nu, S = np.zeros(2 * m), np.eye(2 * m)
    H = np.zeros((2 * m, x.size))
    posed = {}
    for k in paired:
        o = pairing_obs(entries[k], hyp[k])
        hx, Hk = M.jacobian(x, o)
        posed[k] = Hk is not None
        z = o["z"].copy()
        if o["rows"] == 1:
            z[1] = 0.0
        if Hk is None:
            hx, Hk = np.zeros(2), np.zeros((2, x.size))
        H[2 * k:2 * k + 2] = Hk
        nu[2 * k:2 * k + 2] = z - hx
        for r in range(2):
            if M.WRAP[o["model"]][r]:
                nu[2 * k + r] = M.wrap180(nu[2 * k + r])
    rows = [2 * k + r for k in paired for r in range(2)]
    if rows:
        Sp = H[rows] @ P @ H[rows].T
        for q, k in enumerate(paired):
            Sp[2 * q:2 * q + 2, 2 * q:2 * q + 2] += M.effective_R(pairing_obs(entries[k], hyp[k]))
        S[np.ix_(rows, rows)] = Sp
    prefix, acc, bad = np.zeros(m), 0.0, -1
    for k in range(m):
        if hyp[k] >= 0 and bad < 0:
            lead = [2 * q + r for q in paired if q <= k for r in range(2)]
            Sl = S[np.ix_(lead, lead)]
            ok = posed[k] and np.all(np.isfinite(Sl))
            if ok:
                try:
                    np.linalg.cholesky(Sl)
                except np.linalg.LinAlgError:
                    ok = False
            if ok:
                acc = float(nu[lead] @ np.linalg.solve(Sl, nu[lead]))
            else:
                bad, acc = k, float("nan")
        prefix[k] = acc
    dof = sum(M.ROWS[entries[k]["model"]] for k in paired)
    return dict(d2=acc, dof=dof, pairings=len(paired), outcome=IRREGULAR if bad >= 0 else REGULAR, first_irregular=bad, d2_prefix=prefix,
                nu=nu, S=S, H=H)


def joint_many(x, P, entries, hyps):
    """Engine.joint_innovation's dict for a list of hypotheses, from joint_dense."""
    rows = [joint_dense(x, P, entries, h) for h in hyps]
    out = {key: np.array([r[key] for r in rows]) for key in ("d2", "dof", "pairings", "outcome", "first_irregular")}
    for key in ("d2_prefix", "nu", "S"):
        out[key] = np.array([r[key] for r in rows])
    return out


def cross_bound(x, P, entries, hyp):
    """The componentwise bound of the off-diagonal blocks, by scan index: 32 * 2^-53 * (|H_a| |P| |H_b|') -- each entry is a sum of at most
    49 products with at most three roundings each."""
    H = np.abs(joint_dense(x, P, entries, hyp)["H"])
    return 32.0 * U53 * (H @ np.abs(P) @ H.T)


def cond_of(res_S, hyp):
    rows = [2 * k + r for k in range(len(hyp)) if hyp[k] >= 0 for r in range(2)]
    return float(np.linalg.cond(np.asarray(res_S)[np.ix_(rows, rows)])) if rows else 1.0


def solve_prefixes(S, nu, hyp):
    """d2 and every prefix through numpy.linalg.solve on the SAME S and nu (by scan index)."""
    m = len(hyp)
    out, acc = np.zeros(m), 0.0
    for k in range(m):
        if hyp[k] >= 0:
            lead = [2 * q + r for q in range(k + 1) if hyp[q] >= 0 for r in range(2)]
            acc = float(nu[lead] @ np.linalg.solve(S[np.ix_(lead, lead)], nu[lead]))
        out[k] = acc
    return out


# ------------------------------------------------------------------------------------------------------------------
# the scene in which only a joint test can tell two landmarks apart
# ------------------------------------------------------------------------------------------------------------------
GATE, CHI2_4 = 9.21, 13.277
LM_A, LM_B = 40, 41               # 0-based


def ambiguous_scene():
    """(x, s, d, U, the two sightings as (model, z, R) tuples): lowrank_data(150, 5) with the robot position variance raised to 1.0 and
    landmarks 40 and 41 moved to (6.0, 3.0) and (6.6, 3.0) with variance 0.01; two RELATIVE_XY sightings of them with R = RPOS."""
    x, s, d, U = lowrank_data(N0, 5)
    x, d = x.copy(), d.copy()
    d[0] = d[1] = 1.0
    for lm, pos in ((LM_A, (6.0, 3.0)), (LM_B, (6.6, 3.0))):
        x[3 + 2 * lm:5 + 2 * lm] = pos
        d[3 + 2 * lm:5 + 2 * lm] = 0.01
    noise = ((0.03, -0.02), (-0.02, 0.03))
    scan = [(M.RELATIVE_XY, M.h_of(M.RELATIVE_XY, x[:3], x[3 + 2 * lm:5 + 2 * lm]) + np.asarray(dz), RPOS) for lm, dz in zip((LM_A, LM_B), noise)]
    return x, s, d, U, scan


def scene_entries(scan, gate=A.INF):
    return [A.entry(e[0], e[1], e[2], gate) for e in scan]


def assert_scene_premises():
    """All four individual d2 lie inside the 9.21 gate, the swapped joint d2 beyond chi2(0.99, 4) = 13.277, the correct one below 1."""
    x, _, d, U, scan = ambiguous_scene()
    P = np.diag(d) + U @ U.T
    ents = scene_entries(scan)
    single = np.array([[A.pair_d2(x, P, ent, lm) for lm in (LM_A, LM_B)] for ent in ents])
    right, swapped = joint_dense(x, P, ents, [LM_A, LM_B]), joint_dense(x, P, ents, [LM_B, LM_A])
    print("scene: individual d2 %s, joint d2 correct %.3g swapped %.3g" % (np.round(single, 3).tolist(), right["d2"], swapped["d2"]))
    assert single.max() < GATE and swapped["d2"] > CHI2_4 and right["d2"] < 1.0
    return x, P, ents


def chi2_table(p, dof):
    """chi2 quantiles the restated search needs, from a fine bisection on the series of the regularised incomplete gamma function for an
    even dof: P(dof / 2, q / 2) = 1 - exp(-q / 2) sum_{j < dof / 2} (q / 2)^j / j!."""
    assert dof % 2 == 0
    if dof == 0:
        return 0.0
    import math
    cdf = lambda q: 1.0 - math.exp(-q / 2.0) * sum((q / 2.0) ** j / math.factorial(j) for j in range(dof // 2))
    lo, hi = 0.0, 1000.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if cdf(mid) < p else (lo, mid)
    return 0.5 * (lo + hi)


def search_brute(x, P, scan, gate_match, gate_new, joint_p=0.99):
    """measure_model_joint's decisions without a beam, by enumeration: [(kind, landmark 0-based or -1)] per entry."""
    ents = scene_entries(scan, gate_match)
    D = A.d2_matrix(x, P, ents)
    cands, kinds = [], []
    for k in range(len(ents)):
        inside = sorted((float(v), i) for i, v in enumerate(D[k]) if v <= gate_match)
        cands.append([i for _, i in inside[:4]])
        best = np.nanmin(D[k]) if D.shape[1] else np.inf
        kinds.append("search" if cands[k] else ("new" if best > gate_new else "discarded"))
    searched = [k for k in range(len(ents)) if kinds[k] == "search"]
    sub = [ents[k] for k in searched]
    alive = []
    for h in itertools.product(*[cands[k] + [-1] for k in searched]):
        used = [c for c in h if c >= 0]
        if len(set(used)) != len(used):
            continue
        r = joint_dense(x, P, sub, list(h))
        # every prefix must pass its own threshold: the search prunes level by level
        pairs = np.cumsum([c >= 0 for c in h])
        if all(r["d2_prefix"][q] <= chi2_table(joint_p, 2 * int(pairs[q])) for q in range(len(h))):
            alive.append((h, len(used), r["d2"]))
    alive.sort(key=lambda t: (-t[1], t[2], t[0]))
    winner = dict(zip(searched, alive[0][0])) if searched else {}
    return [("matched", winner[k]) if winner.get(k, -1) >= 0 else (kinds[k] if kinds[k] == "new" else "discarded", -1) for k in range(len(ents))]
