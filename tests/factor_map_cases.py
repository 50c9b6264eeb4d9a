"""What the factor_map tests share (tests/test_factor_map_cpu.py, tests/test_factor_map_gpu.py): the NumPy restatement of ekf_factor_map
-- a plain unblocked Cholesky in the library's elimination order, the landmark block first (rows ascending) and the robot last -- and the
builder of the scenes whose P is NOT positive definite.  Nothing of ekf_slam_amd is imported here."""
import numpy as np

KEYS = ("n", "definite", "bad_index", "bad_pivot", "logdet", "logdet_map", "min_pivot", "max_pivot")


def elimination_order(n):
    """The indices into x in the order their pivots are taken: 3, 4, .., n - 1, then 0, 1, 2."""
    return list(range(3, n)) + [0, 1, 2]


def wrap180(a):
    """a (degrees) in (-180, 180]."""
    return a - 360.0 * np.ceil((a - 180.0) / 360.0)


def factor_dense(x, P, refs=None):
    """What Engine.factor_map returns, from a dense P: an unblocked right-looking Cholesky of P taken in elimination_order, stopped at the
    first pivot that is <= 0 or not finite.  Also 'pivots' (the values under the square roots, in elimination order, the failing one
    last) and 'L' (the factor in elimination order; None where not definite)."""
    x, P = np.asarray(x, dtype=np.float64), np.asarray(P, dtype=np.float64)
    n = x.size
    assert P.shape == (n, n)
    order = elimination_order(n)
    A = P[np.ix_(order, order)].copy()
    pivots, bad = [], -1
    for j in range(n):
        d = A[j, j]
        pivots.append(float(d))
        if not (d > 0.0 and np.isfinite(d)):
            bad = j
            break
        l = np.sqrt(d)
        A[j, j] = l
        A[j + 1:, j] /= l
        A[j + 1:, j + 1:] -= np.outer(A[j + 1:, j], A[j + 1:, j])
    taken = np.array(pivots[:-1] if bad >= 0 else pivots)
    nm = n - 3
    out = dict(n=n, definite=bad < 0, bad_index=-1 if bad < 0 else order[bad], bad_pivot=0.0 if bad < 0 else pivots[-1],
               logdet=float(np.sum(np.log(taken))) if bad < 0 else float("nan"),
               logdet_map=float(np.sum(np.log(taken[:nm]))) if bad < 0 or bad >= nm else float("nan"),
               min_pivot=float(taken.min()) if taken.size else float("nan"), max_pivot=float(taken.max()) if taken.size else float("nan"),
               pivots=np.array(pivots), L=np.tril(A) if bad < 0 else None)
    if refs is None:
        out["d2"] = np.zeros(0)
        return out
    refs = np.asarray(refs, dtype=np.float64).reshape(-1, n)
    d2 = np.full(refs.shape[0], np.nan)
    if bad < 0:
        for q, ref in enumerate(refs):
            nu = x - ref
            nu[2] = wrap180(nu[2])
            y = np.linalg.solve(out["L"], nu[order])          # (L is triangular; the general solver is as good here)
            d2[q] = float(y @ y)
    out["d2"] = d2
    return out


def reference_states(x, count, seed):
    """`count` reference states near x: a metre or so off on every position entry and a few degrees on the heading."""
    rng = np.random.default_rng(seed)
    x = np.asarray(x, dtype=np.float64)
    refs = x[None, :] + rng.normal(0.0, 0.5, (count, x.size))
    refs[:, 2] = x[2] + rng.normal(0.0, 3.0, count)
    return refs


def spd_scene(N, seed):
    """(x, s, P): a well-conditioned full covariance P = L L' with the diagonal of L in [0.8, 1.2] (in elimination order)."""
    x, s, P, _ = _ldl_scene(N, seed, None)
    return x, s, P


def _ldl_scene(N, seed, negative_at):
    rng = np.random.default_rng(seed)
    n = 3 + 2 * N
    order = elimination_order(n)
    L = np.tril(rng.normal(0.0, 0.05, (n, n)), -1) + np.diag(rng.uniform(0.8, 1.2, n))
    D = np.ones(n)
    if negative_at is not None:
        D[order.index(negative_at)] = -1.0
    Pe = (L * D) @ L.T
    Pe = 0.5 * (Pe + Pe.T)
    P = np.empty_like(Pe)
    P[np.ix_(order, order)] = Pe
    x = np.concatenate([rng.uniform(-5, 5, 2), [rng.uniform(20.0, 300.0)], rng.uniform(-20, 20, 2 * N)])
    return x, np.arange(1, N + 1, dtype=np.float64), P, order


def indefinite_scene(N, bad_index, zero=False, seed=7):
    """(x, s, P) whose factorisation stops at index `bad_index` of x, decisively: P = L D L' in elimination order with D = -1 at that
    pivot and +1 elsewhere, so that pivot is -L_jj^2 <= -0.64 and every earlier one is L_ii^2 >= 0.64; or, with zero=True, a positive
    definite P whose row and column `bad_index` are exactly zero, so that pivot is exactly 0.0.  The builder ASSERTS, through
    factor_dense, that the failing pivot is <= -1e-3 max|P| (exactly 0.0 for a zero scene) and every earlier pivot >= +1e-3 max|P|:
    neither rounding nor the blocked order of the device can move the index."""
    x, s, P, order = _ldl_scene(N, seed, None if zero else bad_index)
    if zero:
        P[bad_index, :] = 0.0
        P[:, bad_index] = 0.0
    res = factor_dense(x, P)
    big = np.abs(P).max()
    assert not res["definite"] and res["bad_index"] == bad_index, (res["bad_index"], bad_index)
    assert res["pivots"].size == order.index(bad_index) + 1
    if zero:
        assert res["bad_pivot"] == 0.0 and res["pivots"][-1] == 0.0
    else:
        assert res["bad_pivot"] <= -1e-3 * big
    assert np.all(res["pivots"][:-1] >= 1e-3 * big)
    return x, s, P
