"""What the multiply_map tests share (tests/test_multiply_map_cpu.py, tests/test_multiply_map_gpu.py): the bar, the vectors the tests use
and the scenes of the host emulation.  Nothing of ekf_slam_amd is imported here.

THE BAR is derived, not measured.  The device and NumPy both form entry i of P b as a sum of n = 3 + 2 N products in some order; each
such sum is within gamma_n (|P| |b|)_i = n 2^-53 / (1 - n 2^-53) (|P| |b|)_i of the exact value (Higham, Accuracy and Stability of
Numerical Algorithms, section 3.1; an FMA chain only saves roundings), so the two differ by at most twice that: entry by entry
    |got - P b|_i <= 2 n 2^-53 (|P| |b|)_i,
P being what a twin with the same history reports through get_P()."""
import numpy as np

CHUNK = 16                        # the vectors of one tile pass (kFactorChunk)
U = 2.0 ** -53


def bar_ratio(P, B, got):
    """The worst |got - B P|_qi / (2 n 2^-53 (|B| |P|)_qi) over the entries whose bound is not zero; an entry whose bound is zero
    must be zero itself (inf otherwise).  P is symmetric, so row q of B @ P is P b_q."""
    P = np.asarray(P, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64).reshape(-1, P.shape[0])
    got = np.asarray(got, dtype=np.float64).reshape(B.shape)
    err = np.abs(got - B @ P)
    bound = 2.0 * P.shape[0] * U * (np.abs(B) @ np.abs(P))
    if np.any(err[bound == 0.0] != 0.0) or not np.isfinite(got).all():
        return np.inf
    nz = bound > 0.0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


def gaussian_rows(k, n, seed):
    return np.random.default_rng(seed).standard_normal((k, n))


def spread_units(n, units=19):
    """`units` spread indices into x, the first and the last among them."""
    return np.unique(np.linspace(0, n - 1, min(units, n)).round().astype(int))


def batch_rows(n, seed=5):
    """3 * 16 + 5 rows with row 0 repeated behind a chunk boundary, in the middle and at the end; a zero row at 2."""
    B = gaussian_rows(3 * CHUNK + 5, n, seed)
    B[CHUNK + 1] = B[0]
    B[2 * CHUNK] = B[0]
    B[-1] = B[0]
    B[2] = 0.0
    return B


REPEATS = (0, CHUNK + 1, 2 * CHUNK, -1)
