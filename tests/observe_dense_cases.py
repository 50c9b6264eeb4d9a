"""What the observe_dense tests share (tests/test_observe_dense_cpu.py, tests/test_observe_dense_gpu.py): the NumPy restatement of
ekf_observe_dense -- the symmetric form of include/ekfslam.h, float64, from a dense P --, the scenes and the bars.  Nothing of
ekf_slam_amd is imported here.

THE BARS are derived, not measured; u = 2^-53, n = 3 + 2 N, P what a twin with the same history reports through get_P().
  S.   S_ij = sum_a H_ia (sum_b P_ab H_jb) + R_ij: two chained sums of n products.  The inner sum (the device's G = P H', or NumPy's) is
       within gamma_n (|P||H'|) of its exact value, the outer one adds gamma_n of (|H||G|) <= (1 + gamma_n)(|H||P||H'|): each side is
       within 2 n u (|H||P||H'|)_ij of the exact H P H' to first order (Higham, Accuracy and Stability of Numerical Algorithms, section
       3.1; multiply_map_cases derives its bar the same way for ONE sum), the two sides differ by twice that, and adding R rounds once
       on each side:
           |S - (H P H' + R)|_ij <= 4 n u (|H||P||H'|)_ij + 2 u |S_ij|.
  nu.  nu_i = z_i - sum_a H_ia x_a, ONE sum of n products and one subtraction on each side, by the same rule:
           |nu - (z - H x)|_i <= 2 n u (|H||x|)_i + 2 u |nu_i|.
       (A wrapped row moves both sides by the same exact multiple of 360.)
  d2.  d2 = nu' S^-1 nu.  With a = S^-1 nu, a change (dS, dnu) moves it by 2 a' dnu - a' dS a to first order, so the S and nu bars above
       (bS, bnu) propagate to 2 |a|' bnu + |a|' bS |a|.  On top comes the error of the solve itself, for which solve_map_cases' bar is
       the precedent, applied to S: 64 cond_2(S) u, relative.  Relative to NumPy's d2:
           |d2 - d2_np| / d2_np <= 64 cond_2(S) u + (2 |a|' bnu + |a|' bS |a|) / d2_np.
The scenes keep cond_2(S) <= 1e4 (R = rho I with rho a hundredth of the mean diagonal of H P H', so cond_2(S) <= 100 k + 1), which the
tests assert; tests/test_observe_dense_cpu.py checks that NumPy alone, against an extended-precision evaluation, stays inside every bar."""
import numpy as np

U = 2.0 ** -53
DENSE_MAX = 16
APPLIED, IRREGULAR, GATED = 1, 0, 2
INF = float("inf")
KS = (1, 2, 3, 16)                # a scalar row; one full pair; odd, two pairs; the full chunk
COND_MAX = 1e4


def wrap180(a):
    return a if -180.0 < a <= 180.0 else a - 360.0 * np.ceil((a - 180.0) / 360.0)


def innovation_dense(x, P, H, z, R, wrap_deg=None):
    """(nu, S) of the header: S = H (P H') + R, nu = z - H x with the flagged rows wrapped into (-180, 180]."""
    H = np.asarray(H, dtype=np.float64).reshape(-1, x.size)
    S = H @ (P @ H.T) + np.asarray(R, dtype=np.float64).reshape(H.shape[0], H.shape[0])
    nu = np.asarray(z, dtype=np.float64).reshape(-1) - H @ x
    if wrap_deg is not None:
        nu = np.array([wrap180(v) if w else v for v, w in zip(nu, wrap_deg)])
    return nu, S


def update_dense(x, P, H, z, R, gate=INF, wrap_deg=None):
    """(x', P', record) of ekf_observe_dense from a dense P: with L L' = S, W = L^-1 H P and y = L^-1 nu, d2 = |y|^2, x' = x + W' y,
    P' = P - W' W; record = {'d2', 'rows', 'outcome', 'bad_row', 'nu', 'S'}.  Gated or irregular: x and P unchanged."""
    x, P = np.asarray(x, dtype=np.float64), np.asarray(P, dtype=np.float64)
    H = np.asarray(H, dtype=np.float64).reshape(-1, x.size)
    k = H.shape[0]
    nu, S = innovation_dense(x, P, H, z, R, wrap_deg)
    rec = dict(rows=k, nu=nu, S=S, bad_row=-1)
    L = np.zeros((k, k))
    for i in range(k):                                        # row by row, so that the first bad pivot has a number
        for j in range(i):
            L[i, j] = (S[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
        piv = S[i, i] - L[i, :i] @ L[i, :i]
        if not (np.isfinite(piv) and piv > 0.0):
            rec.update(d2=np.nan, outcome=IRREGULAR, bad_row=i)
            return x.copy(), P.copy(), rec
        L[i, i] = np.sqrt(piv)
    y = np.linalg.solve(L, nu)
    W = np.linalg.solve(L, H @ P)
    rec["d2"] = float(y @ y)
    if not rec["d2"] <= gate:
        rec["outcome"] = GATED
        return x.copy(), P.copy(), rec
    rec["outcome"] = APPLIED
    Pn = P - W.T @ W
    return x + W.T @ y, 0.5 * (Pn + Pn.T), rec


# ---- the bars ----
def S_bar(P, H, S):
    H = np.abs(np.asarray(H, dtype=np.float64).reshape(-1, P.shape[0]))
    return 4.0 * P.shape[0] * U * (H @ np.abs(P) @ H.T) + 2.0 * U * np.abs(S)


def nu_bar(x, H, nu):
    H = np.abs(np.asarray(H, dtype=np.float64).reshape(-1, x.size))
    return 2.0 * x.size * U * (H @ np.abs(x)) + 2.0 * U * np.abs(nu)


def d2_bar(x, P, H, nu, S):
    """The relative bar on d2 (the docstring's last formula), from NumPy's own nu and S."""
    a = np.abs(np.linalg.solve(S, nu))
    d2 = float(nu @ np.linalg.solve(S, nu))
    return 64.0 * np.linalg.cond(S) * U + (2.0 * a @ nu_bar(x, H, nu) + a @ S_bar(P, H, S) @ a) / d2


def ratio(err, bound):
    """The worst err / bound over the entries whose bound is not zero; an entry whose bound is zero must be exact (inf otherwise)."""
    err, bound = np.abs(np.asarray(err, dtype=np.float64)), np.asarray(bound, dtype=np.float64)
    if np.any(err[bound == 0.0] != 0.0) or not np.isfinite(err).all():
        return np.inf
    nz = bound > 0.0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


def bar_ratios(x, P, H, z, R, got, wrap_deg=None):
    """(S, nu, d2): each the worst |got - NumPy| over its bar, NumPy's values from (x, P)."""
    nu, S = innovation_dense(x, P, H, z, R, wrap_deg)
    d2 = float(nu @ np.linalg.solve(S, nu))
    return (ratio(got["S"] - S, S_bar(P, H, S)), ratio(got["nu"] - nu, nu_bar(x, H, nu)),
            abs(got["d2"] - d2) / d2 / d2_bar(x, P, H, nu, S))


# ---- the scenes ----
def gaussian_H(k, n, seed):
    return np.random.default_rng(seed).standard_normal((k, n))


def centroid_H(n, count=40, first=2):
    """Two rows: the mean of `count` landmarks from landmark `first` on (fewer where the map is smaller), x then y."""
    N = (n - 3) // 2
    lms = np.arange(min(first, max(N - 1, 0)), min(first + count, N))
    H = np.zeros((2, n))
    H[0, 3 + 2 * lms] = 1.0 / lms.size
    H[1, 4 + 2 * lms] = 1.0 / lms.size
    return H


def displacement_H(n, pairs):
    """Two rows per pair (i, j): l_i - l_j."""
    H = np.zeros((2 * len(pairs), n))
    for q, (i, j) in enumerate(pairs):
        for r in (0, 1):
            H[2 * q + r, 3 + 2 * i + r], H[2 * q + r, 3 + 2 * j + r] = 1.0, -1.0
    return H


def spread_pairs(N, m):
    """m pairs of different landmarks spread over the map, no landmark twice."""
    idx = np.unique(np.linspace(0, N - 1, 2 * m).round().astype(int))
    assert idx.size == 2 * m
    return [(int(idx[2 * q]), int(idx[2 * q + 1])) for q in range(m)]


def noise_for(P, H, frac=0.01):
    """R = rho I, rho = frac of the mean diagonal entry of H P H': cond_2(S) <= k / frac + 1."""
    H = np.asarray(H, dtype=np.float64).reshape(-1, P.shape[0])
    return frac * np.trace(H @ P @ H.T) / H.shape[0] * np.eye(H.shape[0])


def reading_for(x, P, H, R, seed=3, size=0.7):
    """z = H x + size * sqrt(diag S) * g, g Gaussian: an innovation of the size S expects."""
    H = np.asarray(H, dtype=np.float64).reshape(-1, x.size)
    S = H @ P @ H.T + R
    return H @ x + size * np.sqrt(np.diag(S)) * np.random.default_rng(seed).standard_normal(H.shape[0])


def scene(x, P, H, seed=3):
    """(H, z, R) for the rows H on the state (x, P), with the premise cond_2(S) <= COND_MAX asserted."""
    R = noise_for(P, H)
    z = reading_for(x, P, H, R, seed)
    assert np.linalg.cond(np.asarray(H).reshape(-1, x.size) @ P @ np.asarray(H).reshape(-1, x.size).T + R) <= COND_MAX
    return np.asarray(H, dtype=np.float64).reshape(-1, x.size), z, R


def padded(H, z, R):
    """An odd k written out as k + 1 rows: the exactly empty last row (H = 0, R's row and column 0 but a 1 on the diagonal, z = 0)."""
    k = H.shape[0]
    Hp, zp, Rp = np.vstack([H, np.zeros((1, H.shape[1]))]), np.concatenate([z, [0.0]]), np.zeros((k + 1, k + 1))
    Rp[:k, :k], Rp[k, k] = R, 1.0
    return Hp, zp, Rp


def singular_pivot_is_not_positive(p):
    """Whether the second pivot of [[p, p], [p, p]] comes out <= 0 in the factorisation's own arithmetic (float64, no contraction):
    p - (p / sqrt(p))^2.  About half of all p give exactly 0, the rest a last-bit residue of either sign."""
    p = np.float64(p)
    q = p / np.sqrt(p)
    return bool(p - q * q <= 0.0)
