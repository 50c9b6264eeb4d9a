"""Pure-NumPy side of the linear-observation tests (ekf_observe_linear / ekf_linear_innovation): the dense Kalman update for a general
constant H as include/ekfslam.h states it, an independent information-form restatement for R > 0, the observation kinds the tests
use, and a factored form for the states P = diag(d) + U U' the test at size starts from.  No GPU, no library."""
import numpy as np

import merge_cases

INF = float("inf")
APPLIED, IRREGULAR, GATED = 1, 0, 2


def wrap180(a):
    """a (degrees) wrapped into (-180, 180]."""
    a = np.asarray(a, dtype=np.float64)
    return a - 360.0 * np.ceil((a - 180.0) / 360.0)


def obs(z, R, Hr=None, landmarks=(), Hl=(), gate=INF, wrap=(0, 0), rows=2):
    """One observation as a dict of full-size arrays (0-based landmarks): what Engine.observe_linear takes as keywords."""
    rows = int(rows)
    zv = np.zeros(2); zv[:rows] = np.asarray(z, dtype=np.float64).reshape(-1)[:rows]
    Rm = np.zeros((2, 2))
    Ra = np.asarray(R, dtype=np.float64)
    if Ra.size == 1:
        Rm[0, 0] = float(Ra.reshape(-1)[0])
    else:
        Rm[:] = Ra.reshape(2, 2)
    Hrm = np.zeros((2, 3))
    if Hr is not None:
        Ha = np.asarray(Hr, dtype=np.float64)
        if Ha.size == 3:
            Hrm[0] = Ha.reshape(-1)
        else:
            Hrm[:] = Ha.reshape(2, 3)
    blocks = []
    for b in Hl:
        Ba = np.asarray(b, dtype=np.float64)
        Bm = np.zeros((2, 2))
        if Ba.size == 2:
            Bm[0] = Ba.reshape(-1)
        else:
            Bm[:] = Ba.reshape(2, 2)
        blocks.append(Bm)
    return dict(z=zv, R=Rm, Hr=Hrm, landmarks=[int(k) for k in landmarks], Hl=blocks, gate=float(gate), wrap=tuple(wrap), rows=rows)


def effective(o):
    """(z, R, Hr, Hl) with rows == 1 run as the exactly empty second row: H(1, :) = 0, R01 = R10 = 0, R11 = 1, z1 = 0."""
    z, R, Hr, Hl = o["z"].copy(), o["R"].copy(), o["Hr"].copy(), [b.copy() for b in o["Hl"]]
    if o["rows"] == 1:
        z[1] = 0.0
        R[0, 1] = R[1, 0] = 0.0; R[1, 1] = 1.0
        Hr[1] = 0.0
        for b in Hl:
            b[1] = 0.0
    return z, R, Hr, Hl


def jacobian(n, o):
    """The 2 x n matrix H of an observation on a state of n entries."""
    _, _, Hr, Hl = effective(o)
    H = np.zeros((2, n))
    H[:, 0:3] = Hr
    for k, b in zip(o["landmarks"], Hl):
        H[:, 3 + 2 * k:5 + 2 * k] = b
    return H


def innovation(x, o, H):
    z = effective(o)[0]
    nu = z - H @ np.asarray(x, dtype=np.float64)
    for r in range(2):
        if o["wrap"][r]:
            nu[r] = wrap180(nu[r])
    return nu


def decide(S, nu, gate):
    """(outcome, d2) as the header defines them: irregular where S is not finite, S00 <= 0 or det S <= 0."""
    det = S[0, 0] * S[1, 1] - S[0, 1] * S[1, 0]
    if not (np.all(np.isfinite(S)) and S[0, 0] > 0.0 and det > 0.0):
        return IRREGULAR, float("nan")
    d2 = float(nu @ np.linalg.solve(S, nu))
    return (GATED if d2 > gate else APPLIED), d2


def observe_dense(x, P, o):
    """(x', P', result) of one observation, as written: G = H P, S = G H' + R, nu = z - H x (wrapped where asked), K = G' S^-1,
    x += K nu, P -= K G, d2 = nu' S^-1 nu; an observation that does not apply leaves x and P as they are."""
    x, P = np.asarray(x, dtype=np.float64), np.asarray(P, dtype=np.float64)
    H = jacobian(x.size, o)
    R = effective(o)[1]
    G = H @ P
    S = G @ H.T + R
    nu = innovation(x, o, H)
    outcome, d2 = decide(S, nu, o["gate"])
    res = dict(nu=nu, S=S, d2=d2, outcome=outcome)
    if outcome != APPLIED:
        return x.copy(), P.copy(), res
    K = G.T @ np.linalg.inv(S)
    return x + K @ nu, P - K @ G, res


def observe_information(x, P, o):
    """The same update in information form (R > 0, no gate): Lambda' = P^-1 + H' R^-1 H, x' = x + Lambda'^-1 H' R^-1 nu.  Shares no
    intermediate with observe_dense (no G, S or K)."""
    x, P = np.asarray(x, dtype=np.float64), np.asarray(P, dtype=np.float64)
    H = jacobian(x.size, o)
    Ri = np.linalg.inv(effective(o)[1])
    P2 = np.linalg.inv(np.linalg.inv(P) + H.T @ Ri @ H)
    return x + P2 @ (H.T @ (Ri @ innovation(x, o, H))), P2


# ---- the observation kinds ----
def landmark_fix(k, pos, R, gate=INF):
    return obs(pos, R, None, [k], [np.eye(2)], gate=gate)


def position_fix(pos, R, gate=INF):
    return obs(pos, R, [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], gate=gate)


def heading_fix(theta_deg, var, gate=INF):
    return obs([theta_deg], var, [0.0, 0.0, 1.0], gate=gate, wrap=(1, 0), rows=1)


def relative(i, j, delta, R, gate=INF):
    """'l_i - l_j = delta': ekf_constrain_landmarks' H."""
    return obs(delta, R, None, [i, j], [np.eye(2), -np.eye(2)], gate=gate)


def general(rng, i, j, x, scale=1.0, R=None):
    """A dense random H over the robot and two landmarks with a z near H x."""
    Hr = rng.standard_normal((2, 3)) * np.array([1.0, 1.0, 0.05])
    Hl = [rng.standard_normal((2, 2)), rng.standard_normal((2, 2))]
    o = obs([0.0, 0.0], np.array([[0.3, 0.05], [0.05, 0.2]]) if R is None else R, Hr, [i, j], Hl)
    o["z"] = jacobian(np.asarray(x).size, o) @ np.asarray(x) + scale * rng.standard_normal(2)
    return o


def scalar_on_landmark(k, value, var, row=(0.6, -0.8), gate=INF):
    """rows = 1: one linear combination of a landmark's coordinates."""
    return obs([value], var, None, [k], [np.array(row)], gate=gate, rows=1)


class Factored(merge_cases.Factored):
    """merge_cases.Factored with a general linear observation: G = H P from at most seven rows of P, in O(n k)."""

    def observe(self, o):
        n = self.x.size
        H = jacobian(n, o)
        G = H[:, 0:3] @ self.rows(0, 3)
        for k in o["landmarks"]:
            G = G + H[:, 3 + 2 * k:5 + 2 * k] @ self.rows(3 + 2 * k, 2)
        S = G @ H.T + effective(o)[1]
        nu = innovation(self.x, o, H)
        outcome, d2 = decide(S, nu, o["gate"])
        if outcome == APPLIED:
            K = G.T @ np.linalg.inv(S)
            self.x = self.x + K @ nu
            self.K.append(K); self.G.append(G)
        return dict(nu=nu, S=S, d2=d2, outcome=outcome)

    def correct(self, z, R, k):
        """The range / bearing correction of landmark k (0-based) as the filter writes it (EKF_SLAM.m:125-145): H_s over the robot
        and landmark k from delta = landmark - robot, z_k = [sqrt(q); wrapTo360(atan2d(dy, dx) - theta)], nu = z - z_k not wrapped."""
        a = 3 + 2 * k
        d0, d1 = self.x[a] - self.x[0], self.x[a + 1] - self.x[1]
        q = d0 * d0 + d1 * d1
        sq = np.sqrt(q)
        Hs = np.array([[-sq * d0, -sq * d1, 0.0, sq * d0, sq * d1], [d1, -d0, -q, -d1, d0]]) / q
        zk = np.array([sq, (np.degrees(np.arctan2(d1, d0)) - self.x[2]) % 360.0])
        G = Hs[:, 0:3] @ self.rows(0, 3) + Hs[:, 3:5] @ self.rows(a, 2)
        S = G[:, [0, 1, 2, a, a + 1]] @ Hs.T + np.asarray(R, dtype=np.float64)
        K = G.T @ np.linalg.inv(S)
        self.x = self.x + K @ (np.asarray(z, dtype=np.float64) - zk)
        self.K.append(K); self.G.append(G)


def random_state(rng, N, corr=0.6):
    """A well-conditioned dense state of N landmarks with every block correlated."""
    n = 3 + 2 * N
    A = rng.standard_normal((n, n + 4)) * corr
    P = A @ A.T / (n + 4) + np.diag(0.2 + rng.random(n))
    x = np.concatenate([[1.0, -2.0, 30.0], 20.0 * rng.standard_normal(2 * N)])
    return x, P, np.arange(1, N + 1, dtype=np.float64)


# ------------------------------------------------------------------------------------------------------------------
# the shapes shared by the GPU tests of the linear and the model families
# ------------------------------------------------------------------------------------------------------------------
N0 = 150                        # 300 columns: two workgroups of a gather, the second one partly idle
STORES = [(16, "f64"), (64, "f64"), (256, "f32"), (256, "f32_mixed"), (256, "f32_split")]       # helpers.STORES_ALL without tile 128, as this family has run since ekf_observe_linear


def edge_landmark(T):
    """First landmark of a tile row near the middle of the map; the middle itself where one tile row holds the whole map."""
    per_row = T // 2
    return per_row * max(1, (N0 // 2) // per_row) if per_row < N0 else N0 // 2
