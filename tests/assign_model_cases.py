"""The restatement of ekf_assign_model in NumPy / plain Python, for tests/test_assign_model_*.py: the candidate lists of an m x N matrix of
d2 under the (d2, index) order, the optimal one-to-one assignment by an O(n^3) Hungarian on the DENSE m x (N + m) problem -- the N landmarks
and one private "left out" column per observation at the price of its gate -- a brute-force enumeration that pins the Hungarian for small m,
and second_best: how far the next assignment lies above the optimum.  Nothing of the code under test is used here."""
import itertools

import numpy as np

KEEP = 32
INF = float("inf")


def candidate_lists(D, gates, keep=KEEP):
    """(cand m x keep, cand_d2 m x keep, ncand, within) of the m x N matrix D (NaN: no d2): per row the landmarks with d2 <= gate ordered by
    (d2, index), the first `keep` kept; -1 / +inf behind them."""
    D = np.asarray(D, dtype=np.float64).reshape(len(gates), -1)
    m = D.shape[0]
    cand, cand_d2 = np.full((m, keep), -1, dtype=np.int64), np.full((m, keep), INF)
    ncand, within = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64)
    for k in range(m):
        inside = sorted((float(D[k, i]), int(i)) for i in np.flatnonzero(D[k] <= gates[k]))       # (NaN compares false)
        within[k], ncand[k] = len(inside), min(len(inside), keep)
        for s, (d2, i) in enumerate(inside[:keep]):
            cand[k, s], cand_d2[k, s] = i, d2
    return cand, cand_d2, ncand, within


def dense_costs(D, gates):
    """The m x (N + m) cost matrix: D where it is inside the row's gate, +inf (forbidden) elsewhere, then the private columns."""
    D = np.asarray(D, dtype=np.float64).reshape(len(gates), -1)
    m, N = D.shape
    C = np.full((m, N + m), INF)
    for k in range(m):
        ok = D[k] <= gates[k]
        C[k, :N][ok] = D[k][ok]
        C[k, N + k] = gates[k]
    return C


def hungarian(C):
    """Rows of the n x w cost matrix C (n <= w, +inf = forbidden, every row has a finite entry no other row needs) assigned to distinct
    columns at the smallest total: the classical O(n^2 w) shortest-augmenting-path form with row and column potentials.  Returns the
    column of every row."""
    C = np.asarray(C, dtype=np.float64)
    n, w = C.shape
    u, v = np.zeros(n + 1), np.zeros(w + 1)
    p, way = np.zeros(w + 1, dtype=np.int64), np.zeros(w + 1, dtype=np.int64)        # p[j]: the row (1-based) column j is assigned to
    for i in range(1, n + 1):
        p[0] = i
        j0 = 0
        minv = np.full(w + 1, INF)
        used = np.zeros(w + 1, dtype=bool)
        while True:
            used[j0] = True
            i0 = p[j0]
            cur = C[i0 - 1] - u[i0] - v[1:]
            free = ~used[1:]
            better = free & (cur < minv[1:])
            minv[1:][better] = cur[better]
            way[1:][better] = j0
            masked = np.where(free, minv[1:], INF)
            j1 = int(np.argmin(masked)) + 1
            delta = masked[j1 - 1]
            assert np.isfinite(delta), "no augmenting path: a row without a finite column of its own"
            u[p[used]] += delta
            v[used] -= delta
            minv[1:][free] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    col = np.full(n, -1, dtype=np.int64)
    for j in range(1, w + 1):
        if p[j]:
            col[p[j] - 1] = j - 1
    return col


def total_of(landmark, D, gates):
    """J of an assignment (landmark per row, -1 = left out), summed in scan order."""
    J = 0.0
    for k, i in enumerate(landmark):
        J += float(D[k][int(i)]) if i >= 0 else float(gates[k])
    return J


def solve(D, gates):
    """(landmark per row or -1, J) of the optimal assignment of the m x N matrix D under the gates."""
    D = np.asarray(D, dtype=np.float64).reshape(len(gates), -1)
    N = D.shape[1]
    col = hungarian(dense_costs(D, gates))
    landmark = np.where(col < N, col, -1)
    return landmark, total_of(landmark, D, gates)


def brute(D, gates):
    """(J, [every optimal assignment]) by enumeration of all injective partial maps over the in-gate pairs: m <= 5."""
    D = np.asarray(D, dtype=np.float64).reshape(len(gates), -1)
    m = D.shape[0]
    assert m <= 5
    options = [[-1] + [int(i) for i in np.flatnonzero(D[k] <= gates[k])] for k in range(m)]
    best, argbest = INF, []
    for a in itertools.product(*options):
        used = [i for i in a if i >= 0]
        if len(used) != len(set(used)):
            continue
        J = total_of(a, D, gates)
        if J < best:
            best, argbest = J, [a]
        elif J == best:
            argbest.append(a)
    return best, argbest


def second_best(D, gates, landmark):
    """The smallest J among the assignments that differ from `landmark` (the optimum) in at least one row: the optimum with each row's
    choice forbidden in turn (a left-out row must then take a landmark; +inf where it cannot)."""
    D = np.asarray(D, dtype=np.float64).reshape(len(gates), -1)
    N = D.shape[1]
    out = INF
    for k, i in enumerate(landmark):
        C = dense_costs(D, gates)
        C[k, int(i) if i >= 0 else N + k] = INF
        if not np.any(np.isfinite(C[k])):
            continue
        # the row keeps an escape at a price no optimum pays, so that the Hungarian always ends; a solution through it does not count
        big = 4.0 * (np.sum(C[np.isfinite(C)]) + 1.0)
        C = np.hstack([C, np.full((C.shape[0], 1), INF)])
        C[k, -1] = big
        col = hungarian(C)
        if col[k] == C.shape[1] - 1:
            continue
        out = min(out, float(sum(C[r, col[r]] for r in range(C.shape[0]))))
    return out


def gap(D, gates):
    """(landmark, J, the relative distance of second_best above J) -- what a test asserts before it compares assignments."""
    landmark, J = solve(D, gates)
    nxt = second_best(D, gates, landmark)
    return landmark, J, (nxt - J) / max(J, 1e-300)


def dense_of_lists(cand, cand_d2, ncand):
    """The m x C matrix (NaN where a row does not list a landmark) of m kept lists, and the landmark of every column."""
    lms = sorted({int(cand[k][s]) for k in range(len(ncand)) for s in range(int(ncand[k]))})
    at = {lm: c for c, lm in enumerate(lms)}
    D = np.full((len(ncand), max(len(lms), 1)), np.nan)
    for k in range(len(ncand)):
        for s in range(int(ncand[k])):
            D[k, at[int(cand[k][s])]] = cand_d2[k][s]
    return D, lms


def solve_line(nlanes, cand, cand_d2, ncand, gates):
    """The `solve` line of tests/support/assign_model_host.cpp for m kept lists."""
    parts = ["solve %d %d" % (nlanes, len(ncand))]
    for k in range(len(ncand)):
        parts.append("%.17g %d" % (gates[k], ncand[k]))
        parts.extend("%d %.17g" % (cand[k][s], cand_d2[k][s]) for s in range(int(ncand[k])))
    return " ".join(parts)


# ------------------------------------------------------------------------------------------------------------------
# a scene in which observations compete for landmarks
# ------------------------------------------------------------------------------------------------------------------
SCENE_N, SCENE_FIRST, SCENE_COUNT, SCENE_GATE = 150, 20, 13, 30.0


def contention_scene(m=32, seed=1):
    """(x, s, d, U, scan, targets): lowrank_data(150, 5) with the robot's position variance raised to 1.0 and landmarks 20..32 set on a
    line 0.3 apart, variance 0.01; m RELATIVE_XY sightings (model, z, R) aimed in pairs and triples at neighbouring landmarks of that line,
    0.2 of noise on each.  Where the pose is this uncertain every sighting has most of the line inside a wide gate, and the sightings
    that share a target cannot all have it."""
    import model_obs_cases as M
    from helpers import RPOS
    from removal_cases import lowrank_data
    x, s, d, U = lowrank_data(SCENE_N, 5)
    x, d = x.copy(), d.copy()
    d[0] = d[1] = 1.0
    for j in range(SCENE_COUNT):
        lm = SCENE_FIRST + j
        x[3 + 2 * lm:5 + 2 * lm] = (6.0 + 0.3 * j, 3.0)
        d[3 + 2 * lm:5 + 2 * lm] = 0.01
    targets = []
    j = 0
    while len(targets) < m:
        targets.extend([SCENE_FIRST + j % SCENE_COUNT] * (2 + j % 2))
        j += 1
    targets = targets[:m]
    rng = np.random.default_rng(seed)
    scan = [(M.RELATIVE_XY, M.h_of(M.RELATIVE_XY, x[:3], x[3 + 2 * lm:5 + 2 * lm]) + rng.normal(0.0, 0.2, 2), RPOS) for lm in targets]
    return x, s, d, U, scan, targets
