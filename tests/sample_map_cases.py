"""What the sample_map tests share (tests/test_sample_map_cpu.py, tests/test_sample_map_gpu.py): the NumPy restatement of ekf_sample_map
-- x + C xi with C the factor of factor_map_cases.factor_dense (the library's elimination order: the landmark block first, the robot
last) mapped back to x's order -- and the draws the tests use.  Nothing of ekf_slam_amd is imported here."""
import numpy as np

from factor_map_cases import elimination_order, factor_dense

CHUNK = 16                        # the draws of one apply pass (kFactorChunk)
KS = (1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)


def as_held(P, fl):
    """P as a handle with that storage kind reports it: with float tiles every entry of the landmark block outside the landmarks' own
    2 x 2 blocks is rounded to float; Prr, the strip and the own blocks stay F64."""
    H = np.array(P, dtype=np.float64)
    if fl:
        H[3:, 3:] = H[3:, 3:].astype(np.float32).astype(np.float64)
        for a in range(3, H.shape[0], 2):
            H[a:a + 2, a:a + 2] = P[a:a + 2, a:a + 2]
    return H


def factor_in_x_order(L):
    """C with C[order, order] = L: the factor in elimination order mapped back to x's order, so that C C' = P as get_P reports it."""
    n = L.shape[0]
    order = elimination_order(n)
    C = np.zeros((n, n))
    C[np.ix_(order, order)] = L
    return C


def sample_dense(x, P, xi):
    """What Engine.sample_map returns as samples, from a dense P: row q is x + C xi_q; all NaN where P is not positive definite."""
    x = np.asarray(x, dtype=np.float64)
    xi = np.asarray(xi, dtype=np.float64).reshape(-1, x.size)
    L = factor_dense(x, P)["L"]
    if L is None:
        return np.full(xi.shape, np.nan)
    return x[None, :] + xi @ factor_in_x_order(L).T


def cholesky_in_x_order(P):
    """The same C by numpy.linalg.cholesky of the permuted P (the Cholesky factor with a positive diagonal is unique)."""
    order = elimination_order(P.shape[0])
    return factor_in_x_order(np.linalg.cholesky(P[np.ix_(order, order)]))


def gaussian_draws(k, n, seed):
    return np.random.default_rng(seed).standard_normal((k, n))


def unit_draws(n, extra=3, seed=1):
    """The n unit vectors (the samples minus x are then the columns of C) and `extra` Gaussian rows behind them."""
    return np.vstack([np.eye(n), gaussian_draws(extra, n, seed)])


def recovered_factor(x, samples):
    """C from the samples of unit_draws: column j is sample j minus x."""
    n = x.size
    return (samples[:n] - x[None, :]).T
