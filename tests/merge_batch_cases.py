"""Pure-NumPy side of the batch-fusion tests (ekf_merge_landmarks_batch): the definition restated with the dense helpers of the
one-pair tests, the refusal predicate of include/ekfslam.h, and the map with planted duplicates the GPU tests start from.
No GPU, no library."""
import numpy as np

from merge_cases import constrain_dense
from removal_cases import expected_after, lowrank_data

MERGE_BATCH_MAX = 32
INVALID_ARG, INDEX = "invalid_arg", "index"


def merge_batch_dense(x, s, P, pairs, R=None):
    """(x', s', P', d2) of MergeBatch(pairs, R), pairs = [(keep, drop)] 0-based in the numbering before the call: the constraints
    'l_keep - l_drop = 0 with noise R' in list order (merge_cases.constrain_dense), then ONE removal of all drops
    (removal_cases.expected_after).  d2[k] is the distance of pair k under the state after constraints 0 .. k-1."""
    x, P = np.array(x, dtype=np.float64), np.array(P, dtype=np.float64)
    d2 = []
    for keep, drop in pairs:
        x, P, d, _ = constrain_dense(x, P, int(keep), int(drop), None, R)
        d2.append(d)
    xs, ss, Ps = expected_after(x, s, P, [int(d) for _, d in pairs])
    return xs, ss, Ps, np.array(d2)


def chain_regularity(x, P, pairs, R=None):
    """min over the chain of min(S00, det S), and the d2 values: what must be comfortably positive before an engine is asked."""
    x, P = np.array(x, dtype=np.float64), np.array(P, dtype=np.float64)
    worst, d2 = np.inf, []
    for keep, drop in pairs:
        x, P, d, S = constrain_dense(x, P, int(keep), int(drop), None, R)
        worst = min(worst, S[0, 0], np.linalg.det(S))
        d2.append(d)
    return float(worst), np.array(d2)


def refusal(N, pairs):
    """None, or how ekf_merge_landmarks_batch refuses `pairs` on a map of N landmarks: INVALID_ARG (too many pairs, keep == drop, a
    landmark dropped twice, a keep that is also a drop) before INDEX (an index outside [0, N)) -- the order of the header."""
    pairs = [(int(k), int(d)) for k, d in pairs]
    if len(pairs) > MERGE_BATCH_MAX:
        return INVALID_ARG
    drops = [d for _, d in pairs]
    if any(k == d for k, d in pairs) or len(set(drops)) != len(drops) or any(k in set(drops) for k, _ in pairs):
        return INVALID_ARG
    if any(not (0 <= v < N) for p in pairs for v in p):
        return INDEX
    return None


def survivor_index(pairs, k):
    """the index of surviving landmark k after the batch: k - #{drop < k}"""
    return int(k) - sum(1 for _, d in pairs if d < k)


def planted(N=300, seed=7, n_keeps=14, n_drops=16):
    """(x, s, d, U, pairs): lowrank_data(N, seed) with n_drops duplicates planted -- n_keeps keeps drawn from [0, N/2), n_drops
    distinct drops from [N/2, N), the first keeps reused for the last drops (shared keeps); drop k sits at
    keep + (0.05, -0.03) (1 + 0.1 k).  pairs = [(keep, drop)] in planting order, 0-based; keep < drop throughout, as a search that
    only looks at earlier landmarks reports them."""
    x, s, d, U = lowrank_data(N, seed)
    rng = np.random.default_rng(seed + 1000)
    keeps = [int(v) for v in rng.choice(N // 2, size=n_keeps, replace=False)]
    drops = [int(v) for v in N // 2 + rng.choice(N - N // 2, size=n_drops, replace=False)]
    keeps = keeps + keeps[:n_drops - n_keeps]
    x = np.array(x)
    for k, (kp, dr) in enumerate(zip(keeps, drops)):
        x[3 + 2 * dr:5 + 2 * dr] = x[3 + 2 * kp:5 + 2 * kp] + np.array([0.05, -0.03]) * (1.0 + 0.1 * k)
    return x, s, d, U, list(zip(keeps, drops))


def dense_of(d, U):
    return np.diag(d) + U @ U.T


def nearest_dense(x, P, R=None):
    """(d2, partner) as ekf_nearest_landmarks defines them, by brute force: for every landmark i the j < i of smallest d2(i, j)."""
    N = (x.size - 3) // 2
    R = np.zeros((2, 2)) if R is None else np.asarray(R, dtype=np.float64)
    d2, partner = np.full(N, np.inf), np.full(N, -1, dtype=np.int64)
    for i in range(1, N):
        a = 3 + 2 * i
        for j in range(i):
            b = 3 + 2 * j
            S = P[a:a + 2, a:a + 2] - P[a:a + 2, b:b + 2] - P[b:b + 2, a:a + 2] + P[b:b + 2, b:b + 2] + R
            det = S[0, 0] * S[1, 1] - S[0, 1] * S[1, 0]
            if not (np.isfinite(S).all() and S[0, 0] > 0 and det > 0):
                continue
            nu = -(x[a:a + 2] - x[b:b + 2])
            v = float(nu @ np.linalg.solve(S, nu))
            if v < d2[i]:
                d2[i], partner[i] = v, j
    return d2, partner
