"""Pure-NumPy side of the candidate-search tests (ekf_nearest_landmarks): for every landmark i the j < i that minimises
d2(i, j) = nu' S^-1 nu of "l_i - l_j = 0", S = P_ii + P_jj - P_ij - P_ij' + R, restated in vectorised form (dense P) and block-wise
for the states P = diag(d) + U U' the tests at size start from.  No GPU, no library."""
import numpy as np

# landmark 128 starts a tile row for every tile edge the tests use (T / 2 = 8, 32, 64, 128 landmarks per row); N0 = 300
PLANTS = [(0, 17), (5, 299), (127, 128), (63, 64), (31, 32), (100, 250), (129, 255), (256, 257), (10, 290), (200, 201)]


def plant_duplicates(x, pairs=PLANTS, scale=1.0):
    """x with landmark `drop` of every pair moved to within 0.1 * scale of its `keep` (keep < drop: the duplicate is the later
    append), each by an offset of its own so that no two planted distances tie."""
    x = np.array(x, dtype=np.float64)
    for k, (keep, drop) in enumerate(pairs):
        assert keep < drop
        x[3 + 2 * drop:5 + 2 * drop] = x[3 + 2 * keep:5 + 2 * keep] + scale * np.array([0.05 + 0.004 * k, -0.03 + 0.003 * k])
    return x


def _R(R):
    return np.zeros((2, 2)) if R is None else np.asarray(R, dtype=np.float64).reshape(2, 2)


def _d2_of(S, nu):
    """d2 and the `regular` mask for S (.., 2, 2) and nu (.., 2): nu' S^-1 nu through the adjugate."""
    det = S[..., 0, 0] * S[..., 1, 1] - S[..., 0, 1] * S[..., 1, 0]
    regular = np.isfinite(S).all(axis=(-1, -2)) & (S[..., 0, 0] > 0.0) & (det > 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = nu[..., 0] ** 2 * S[..., 1, 1] - nu[..., 0] * nu[..., 1] * (S[..., 0, 1] + S[..., 1, 0]) + nu[..., 1] ** 2 * S[..., 0, 0]
        d2 = q / det
    regular &= ~np.isnan(d2)
    return np.where(regular, d2, np.inf), regular


def _reduce(D):
    """Row minima of D (inf = not admissible), the lowest column that attains each (-1: none) and runner-up / minimum per row
    (inf where a row has fewer than two admissible entries or its minimum is 0)."""
    n = D.shape[0]
    if D.shape[1] == 0:
        return np.full(n, np.inf), np.full(n, -1, dtype=np.int64), np.full(n, np.inf)
    partner = np.argmin(D, axis=1).astype(np.int64)          # the FIRST minimum: the lowest index wins ties
    best = D[np.arange(n), partner]
    partner[~np.isfinite(best)] = -1
    best = np.where(partner >= 0, best, np.inf)
    if D.shape[1] >= 2:
        second = np.partition(D, 1, axis=1)[:, 1]
    else:
        second = np.full(n, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(np.isfinite(second) & (best > 0.0), second / best, np.inf)
    return best, partner, ratio


def pair_matrix(x, P, R=None, blocks=None):
    """D (N x N): d2(i, j) for j < i, inf elsewhere and for irregular pairs.  blocks ((N, 2, 2), optional): the landmarks' own 2 x 2
    blocks where they are not to be taken from P (Engine.get_P_diag_blocks()[1:])."""
    x, P = np.asarray(x, dtype=np.float64), np.asarray(P, dtype=np.float64)
    N = (x.size - 3) // 2
    L = x[3:].reshape(N, 2)
    C = P[3:, 3:].reshape(N, 2, N, 2).transpose(0, 2, 1, 3)              # C[i, j] = P(l_i, l_j)
    own = C[np.arange(N), np.arange(N)] if blocks is None else np.asarray(blocks, dtype=np.float64)
    S = own[:, None] + own[None, :] - C - C.transpose(0, 1, 3, 2) + _R(R)
    nu = -(L[:, None, :] - L[None, :, :])
    D, _ = _d2_of(S, nu)
    D[np.triu_indices(N)] = np.inf                                       # only j < i
    return D


def nearest_dense(x, P, R=None, blocks=None):
    """(d2, partner, runner-up ratio) as ekf_nearest_landmarks defines them, from a dense P."""
    return _reduce(pair_matrix(x, P, R, blocks))


def nearest_lowrank(x, d, U, rows, R=None, cross_dtype=np.float64):
    """The same for the landmarks `rows` of the state P = diag(d) + U U', with all their columns j < i, never forming P.  The own
    blocks are F64 (the live copies); the cross blocks are rounded to cross_dtype (np.float32 for float tile stores)."""
    x, d, U = np.asarray(x, dtype=np.float64), np.asarray(d, dtype=np.float64), np.asarray(U, dtype=np.float64)
    N = (x.size - 3) // 2
    L = x[3:].reshape(N, 2)
    Um, dm = U[3:].reshape(N, 2, -1), d[3:].reshape(N, 2)
    own = np.einsum("nak,nbk->nab", Um, Um)
    own[:, 0, 0] += dm[:, 0]
    own[:, 1, 1] += dm[:, 1]
    rows = np.asarray(rows, dtype=np.int64)
    best, partner, ratio = np.empty(rows.size), np.empty(rows.size, dtype=np.int64), np.empty(rows.size)
    for b0 in range(0, rows.size, 128):
        rr = rows[b0:b0 + 128]
        jmax = int(rr.max())                                             # columns 0 .. jmax - 1
        C = np.einsum("iak,jbk->ijab", Um[rr], Um[:jmax]).astype(cross_dtype).astype(np.float64)
        S = own[rr][:, None] + own[:jmax][None, :] - C - C.transpose(0, 1, 3, 2) + _R(R)
        nu = -(L[rr][:, None, :] - L[:jmax][None, :, :])
        D, _ = _d2_of(S, nu)
        D[np.arange(jmax)[None, :] >= rr[:, None]] = np.inf
        best[b0:b0 + 128], partner[b0:b0 + 128], ratio[b0:b0 + 128] = _reduce(D)
    return best, partner, ratio


def fuse_dense(x, s, P, gate, R=None, max_merges=None):
    """The greedy loop of EKF_SLAM.fuse_duplicates on a dense state: search, merge the candidate with the smallest (d2, i) at or
    below the gate, again.  Returns (x, s, P, merges) with merges as 0-based (keep, drop, d2)."""
    from merge_cases import merge_dense
    merges = []
    while max_merges is None or len(merges) < max_merges:
        d2, partner, _ = nearest_dense(x, P, R)
        rows = np.nonzero((partner >= 0) & (d2 <= gate))[0]
        if rows.size == 0:
            break
        i = int(rows[np.lexsort((rows, d2[rows]))][0])
        j = int(partner[i])
        merges.append((j, i, float(d2[i])))
        x, s, P = merge_dense(x, s, P, j, i, R)
    return x, s, P, merges
