"""Pure-NumPy side of the ekf_associate_model tests: d2 of every (observation, landmark) pair as the dense restatement of
tests/model_obs_cases.py gives it, the top two of a row under the order (d2, index), and the observe-or-append policy of
measure_model as a pure function.  No GPU, no library."""
import numpy as np

import model_obs_cases as M

INF = float("inf")


def entry(model, z, R, gate=INF):
    """One observation as Engine.associate_model takes it."""
    rows = M.ROWS[model]
    return dict(model=int(model), z=np.asarray(z, dtype=np.float64).reshape(-1)[:rows].copy(), R=np.asarray(R, dtype=np.float64).copy(), gate=float(gate))


def pair_d2(x, P, ent, i):
    """d2 of entry `ent` with landmark i (0-based) as its target on the dense state (x, P); NaN where the pair has none.  H is zero outside
    the robot's and the landmark's columns, so the restatement runs on those five rows and columns of P."""
    o = M.obs(ent["model"], ent["z"], ent["R"], [0], None, ent["gate"])
    rows = [0, 1, 2, 3 + 2 * i, 4 + 2 * i]
    return M.observe_model_dense(np.asarray(x)[rows], np.asarray(P)[np.ix_(rows, rows)], o)[2]["d2"]


def d2_matrix(x, P, entries):
    """m x N: pair_d2 of every pair."""
    N = (np.asarray(x).size - 3) // 2
    return np.array([[pair_d2(x, P, ent, i) for i in range(N)] for ent in entries]).reshape(len(entries), N)


def top_two(row, gate):
    """ekf_model_match of one row of d2: candidates are the entries that are not NaN, ordered by (d2, index)."""
    row = np.asarray(row, dtype=np.float64)
    cand = sorted((float(v), i) for i, v in enumerate(row) if not np.isnan(v))
    best = cand[0] if cand else (INF, -1)
    second = cand[1] if len(cand) > 1 else (INF, -1)
    return dict(best=best[1], second=second[1], d2_best=best[0], d2_second=second[0],
                within_gate=int(sum(1 for v, _ in cand if v <= gate)), irregular=int(np.isnan(row).sum()))


def match(x, P, entries):
    """(what Engine.associate_model returns, as arrays; the m x N matrix)."""
    D = d2_matrix(x, P, entries)
    rows = [top_two(D[k], entries[k]["gate"]) for k in range(len(entries))]
    out = {key: np.array([r[key] for r in rows]) for key in ("best", "second", "d2_best", "d2_second", "within_gate", "irregular")}
    return out, D


def relative_gap(res):
    """(d2_second - d2_best) / d2_best per observation: what must stay far above rounding for best / second to be comparable."""
    return (np.asarray(res["d2_second"]) - np.asarray(res["d2_best"])) / np.asarray(res["d2_best"])


def policy(res, gate_new):
    """measure_model's decisions from an association made with gate = gate_match (0-based `res`): [(kind, landmark 0-based or -1)]."""
    m = len(res["best"])
    kinds = []
    for k in range(m):
        if res["within_gate"][k] == 1:
            kinds.append("matched")
        elif res["best"][k] < 0 or res["d2_best"][k] > gate_new:
            kinds.append("new")
        else:
            kinds.append("discarded")
    matched = [k for k in range(m) if kinds[k] == "matched"]
    out = []
    for k in range(m):
        keeps = kinds[k] == "matched" and k == min((q for q in matched if res["best"][q] == res["best"][k]), key=lambda q: (res["d2_best"][q], q))
        kind = kinds[k] if kinds[k] != "matched" or keeps else "discarded"
        out.append((kind, int(res["best"][k]) if kind == "matched" else -1))
    return out
