"""Pure-NumPy side of the landmark-fusion tests (ekf_constrain_landmarks / ekf_merge_landmarks / ekf_landmark_distance): the
linear Kalman update between two landmarks as include/ekfslam.h states it, an independent information-form restatement, and a
factored form for the states P = diag(d) + U U' the tests at size start from.  No GPU, no library."""
import numpy as np

from removal_cases import expected_after, observe


def _args(x, i, j, delta, R):
    n = np.asarray(x).size
    N = (n - 3) // 2
    assert i != j and 0 <= i < N and 0 <= j < N
    delta = np.zeros(2) if delta is None else np.asarray(delta, dtype=np.float64).reshape(2)
    R = np.zeros((2, 2)) if R is None else np.asarray(R, dtype=np.float64).reshape(2, 2)
    return n, 3 + 2 * i, 3 + 2 * j, delta, R


def jacobian(n, ai, aj):
    """H = [0 .. +I2 (columns a_i) .. -I2 (columns a_j) .. 0] of 'l_i - l_j'."""
    H = np.zeros((2, n))
    H[0, ai] = H[1, ai + 1] = 1.0
    H[0, aj] = H[1, aj + 1] = -1.0
    return H


def constrain_dense(x, P, i, j, delta=None, R=None):
    """(x', P', d2, S) of 'l_i - l_j was observed as delta with noise covariance R' (0-based landmarks), as written:
    G = H P, S = G H' + R, nu = delta - (l_i - l_j), K = G' S^-1, x += K nu, P -= K G."""
    x, P = np.asarray(x, dtype=np.float64), np.asarray(P, dtype=np.float64)
    n, ai, aj, delta, R = _args(x, i, j, delta, R)
    G = P[ai:ai + 2, :] - P[aj:aj + 2, :]
    S = G[:, ai:ai + 2] - G[:, aj:aj + 2] + R
    nu = delta - (x[ai:ai + 2] - x[aj:aj + 2])
    Si = np.linalg.inv(S)
    K = G.T @ Si
    return x + K @ nu, P - K @ G, float(nu @ Si @ nu), S


def merge_dense(x, s, P, keep, drop, R=None):
    """(x', s', P') of Merge(keep, drop, R): constrain(keep, drop, delta = 0, R), then the removal of `drop`."""
    x2, P2, _, _ = constrain_dense(x, P, keep, drop, None, R)
    return expected_after(x2, s, P2, [drop])


def constrain_information(x, P, i, j, delta, R):
    """The same update in information form (R > 0): Lambda' = P^-1 + H' R^-1 H, x' = Lambda'^-1 (P^-1 x + H' R^-1 delta).
    Shares no intermediate with constrain_dense."""
    x, P = np.asarray(x, dtype=np.float64), np.asarray(P, dtype=np.float64)
    n, ai, aj, delta, R = _args(x, i, j, delta, R)
    H = jacobian(n, ai, aj)
    Ri = np.linalg.inv(R)
    L = np.linalg.inv(P)
    L2 = L + H.T @ Ri @ H
    P2 = np.linalg.inv(L2)
    return P2 @ (L @ x + H.T @ Ri @ delta), P2


class Factored:
    """P = diag(d) + U U' - sum_q K_q G_q without ever forming P: what a constrain does to a low-rank-loaded state in O(n k).
    G = H P needs two rows of P, which are two rows of diag(d) + U U' minus the earlier pairs' contributions."""

    def __init__(self, x, d, U):
        self.x, self.d, self.U = np.array(x, dtype=np.float64), np.asarray(d, dtype=np.float64), np.asarray(U, dtype=np.float64)
        self.K, self.G = [], []                       # n x 2 and 2 x n per constraint applied so far

    def rows(self, r0, nr):
        """P(r0 : r0 + nr, :)"""
        out = self.U[r0:r0 + nr] @ self.U.T
        out[np.arange(nr), r0 + np.arange(nr)] += self.d[r0:r0 + nr]
        for K, G in zip(self.K, self.G):
            out -= K[r0:r0 + nr] @ G
        return out

    def diag_blocks(self):
        """(N + 1) x 2 x 2 like Engine.get_P_diag_blocks: P(1:2,1:2), then every landmark's own block."""
        n = self.x.size
        starts = np.concatenate([[0], np.arange(3, n, 2)])
        out = np.empty((starts.size, 2, 2))
        for a in range(2):
            for b in range(2):
                v = np.einsum("ik,ik->i", self.U[starts + a], self.U[starts + b])
                if a == b:
                    v = v + self.d[starts + a]
                for K, G in zip(self.K, self.G):
                    v = v - np.einsum("ik,ki->i", K[starts + a], G[:, starts + b])
                out[:, a, b] = v
        return out

    def trace_and_squares(self, block=512):
        """trace and sum of squares over the lower triangle of P (entries 0 and 2 of ekf_P_digest), accumulated block-wise."""
        n = self.x.size
        tr, sq = 0.0, 0.0
        for r0 in range(0, n, block):
            nr = min(block, n - r0)
            rows = self.rows(r0, nr)
            for q in range(nr):
                c = r0 + q
                tr += rows[q, c]
                sq += float(rows[q, :c + 1] @ rows[q, :c + 1])
        return tr, sq

    def constrain(self, i, j, delta=None, R=None):
        """Applies the constraint; returns (d2, S)."""
        n, ai, aj, delta, R = _args(self.x, i, j, delta, R)
        G = self.rows(ai, 2) - self.rows(aj, 2)
        S = G[:, ai:ai + 2] - G[:, aj:aj + 2] + R
        nu = delta - (self.x[ai:ai + 2] - self.x[aj:aj + 2])
        Si = np.linalg.inv(S)
        K = G.T @ Si
        self.x = self.x + K @ nu
        self.K.append(K); self.G.append(G)
        return float(nu @ Si @ nu), S

    def remove(self, idx):
        """Drops landmarks idx (0-based) from the description."""
        idx = np.asarray(sorted(int(i) for i in idx), dtype=np.int64)
        ent = np.sort(np.concatenate([3 + 2 * idx, 4 + 2 * idx]))
        self.x, self.d, self.U = np.delete(self.x, ent), np.delete(self.d, ent), np.delete(self.U, ent, axis=0)
        self.K = [np.delete(K, ent, axis=0) for K in self.K]
        self.G = [np.delete(G, ent, axis=1) for G in self.G]


def tile_edge_landmark(T, N):
    """First landmark of a tile row near the middle of a map of N landmarks (tile edge T elements)."""
    per_row = T // 2
    return per_row * max(1, (N // 2) // per_row)


def continuation(ex, es, tile, batch, capacity, hole):
    """Operations (pure function of the state after the merge): appends that cross a tile-row edge, measure() scans with corrections
    around the merged pair and new landmarks, two full batches of corrections."""
    N = es.size
    per_row = tile // 2
    ops = []
    n_app = per_row - N % per_row + 3
    assert N + n_app + 8 <= capacity
    rng = np.random.default_rng(2)
    for i in range(n_app):
        ops.append(("append", rng.uniform(-20, 20, 2), 5000.0 + i))
    around = sorted({max(hole - 1, 0), min(hole, N - 1), min(hole + 1, N - 1), 1, N - 2, N // 3})
    lm_index = np.arange(1, capacity + 1, dtype=np.float64)
    lm_loc = np.random.default_rng(3).uniform(-20, 20, (capacity, 2))
    for t in range(3):
        rows = [list(observe(ex, k, dr=0.01 * (t + 1))) + [float(es[k])] for k in around[t::2] + around[:2]]
        rows.append([3.0 + t, 45.0, 9e6 + t])                # matches no signature: appended (EKF_SLAM_UC.m:121-123)
        ops.append(("measure", np.array(rows), lm_index, lm_loc))
    for i in range(2 * batch):
        k = around[i % len(around)] if i % 3 else int(rng.integers(0, N))
        ops.append(("correct", observe(ex, k, dr=0.02), k))
    return ops
