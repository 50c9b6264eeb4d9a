"""Pure-NumPy side of the model-observation tests (ekf_observe_model / ekf_model_innovation / ekf_model_evaluate): the five models' h(x)
and Jacobians as include/ekfslam.h tabulates them, the dense EKF update with nu = z - h(x), and a finite-difference Jacobian.  No GPU,
no library."""
import numpy as np

from linear_obs_cases import APPLIED, GATED, INF, IRREGULAR, decide, wrap180  # noqa: F401

RANGE_BEARING, RANGE, BEARING, RELATIVE_XY, LANDMARK_RANGE = 1, 2, 3, 4, 5
ROWS = {RANGE_BEARING: 2, RANGE: 1, BEARING: 1, RELATIVE_XY: 2, LANDMARK_RANGE: 1}
WRAP = {RANGE_BEARING: (0, 1), RANGE: (0, 0), BEARING: (1, 0), RELATIVE_XY: (0, 0), LANDMARK_RANGE: (0, 0)}
K = 180.0 / np.pi


def obs(model, z, R, landmarks=(), anchor=None, gate=INF):
    """One observation as a dict (0-based landmarks): what Engine.observe_model takes as keywords."""
    rows = ROWS[model]
    zv = np.zeros(2); zv[:rows] = np.asarray(z, dtype=np.float64).reshape(-1)[:rows]
    Rm = np.zeros((2, 2))
    Ra = np.asarray(R, dtype=np.float64)
    if Ra.size == 1:
        Rm[0, 0] = float(Ra.reshape(-1)[0])
    else:
        Rm[:] = Ra.reshape(2, 2)
    return dict(model=int(model), z=zv, R=Rm, landmarks=[int(k) for k in landmarks],
                anchor=None if anchor is None else np.asarray(anchor, dtype=np.float64).reshape(2).copy(), gate=float(gate), rows=rows)


def h_of(model, xr, t0, t1=None):
    """h(x) (2 values; a one-row model leaves h[1] = 0) at the robot state xr = (x, y, theta in degrees) and the target(s)."""
    xr, t0 = np.asarray(xr, dtype=np.float64), np.asarray(t0, dtype=np.float64)
    d = t0 - (np.asarray(t1, dtype=np.float64) if model == LANDMARK_RANGE else xr[:2])
    r = np.sqrt(d @ d)
    bearing = np.degrees(np.arctan2(d[1], d[0])) - xr[2]
    if model == RANGE_BEARING:
        return np.array([r, bearing])
    if model in (RANGE, LANDMARK_RANGE):
        return np.array([r, 0.0])
    if model == BEARING:
        return np.array([bearing, 0.0])
    c, s = np.cos(np.radians(xr[2])), np.sin(np.radians(xr[2]))
    if xr[2] % 90.0 == 0.0:                                    # cosd / sind are exact at multiples of 90 degrees
        c, s = [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)][int(xr[2] // 90.0) % 4]
    return np.array([c * d[0] + s * d[1], -s * d[0] + c * d[1]])


def H_of(model, xr, t0, t1=None):
    """The 2 x 7 Jacobian over (x, y, theta | t0 | t1), the table of include/ekfslam.h."""
    xr, t0 = np.asarray(xr, dtype=np.float64), np.asarray(t0, dtype=np.float64)
    H = np.zeros((2, 7))
    d = t0 - (np.asarray(t1, dtype=np.float64) if model == LANDMARK_RANGE else xr[:2])
    q = d @ d
    r = np.sqrt(q)
    rng_r, rng_t = np.array([-d[0] / r, -d[1] / r, 0.0]), np.array([d[0] / r, d[1] / r])
    brg_r, brg_t = np.array([K * d[1] / q, -K * d[0] / q, -1.0]), np.array([-K * d[1] / q, K * d[0] / q])
    if model == RANGE_BEARING:
        H[0, :3], H[0, 3:5], H[1, :3], H[1, 3:5] = rng_r, rng_t, brg_r, brg_t
    elif model == RANGE:
        H[0, :3], H[0, 3:5] = rng_r, rng_t
    elif model == BEARING:
        H[0, :3], H[0, 3:5] = brg_r, brg_t
    elif model == RELATIVE_XY:
        h = h_of(model, xr, t0)
        c, s = np.cos(np.radians(xr[2])), np.sin(np.radians(xr[2]))
        if xr[2] % 90.0 == 0.0:
            c, s = [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)][int(xr[2] // 90.0) % 4]
        H[0, :3], H[0, 3:5] = [-c, -s, h[1] / K], [c, s]
        H[1, :3], H[1, 3:5] = [s, -c, -h[0] / K], [-s, c]
    else:
        H[0, 3:5], H[0, 5:7] = rng_t, -rng_t
    return H


def H_fd(model, xr, t0, t1=None, step=1e-6):
    """Central finite differences of h_of over the same seven entries."""
    v = np.concatenate([np.asarray(xr, dtype=np.float64), np.asarray(t0, dtype=np.float64),
                        np.zeros(2) if t1 is None else np.asarray(t1, dtype=np.float64)])
    H = np.zeros((2, 7))
    for i in range(7):
        if t1 is None and i >= 5:
            continue
        hi, lo = v.copy(), v.copy()
        hi[i] += step; lo[i] -= step
        f = lambda w: h_of(model, w[:3], w[3:5], w[5:7] if t1 is not None else None)
        H[:, i] = (f(hi) - f(lo)) / (2.0 * step)
    return H


def targets(x, o):
    """(t0, t1, columns of t0 in x or None, columns of t1 or None)."""
    lm = o["landmarks"]
    if o["model"] == LANDMARK_RANGE:
        a, b = 3 + 2 * lm[0], 3 + 2 * lm[1]
        return x[a:a + 2], x[b:b + 2], a, b
    if lm:
        a = 3 + 2 * lm[0]
        return x[a:a + 2], None, a, None
    return o["anchor"], None, None, None


def jacobian(x, o):
    """(h(x), the 2 x n matrix H) of an observation on the state x; (None, None) where q is 0 or not finite."""
    x = np.asarray(x, dtype=np.float64)
    t0, t1, a, b = targets(x, o)
    d = t0 - (t1 if t1 is not None else x[:2])
    q = d @ d
    if not (np.isfinite(q) and q > 0.0):
        return None, None
    H7 = H_of(o["model"], x[:3], t0, t1)
    H = np.zeros((2, x.size))
    H[:, :3] = H7[:, :3]
    if a is not None:
        H[:, a:a + 2] = H7[:, 3:5]
    if b is not None:
        H[:, b:b + 2] = H7[:, 5:7]
    return h_of(o["model"], x[:3], t0, t1), H


def effective_R(o):
    R = o["R"].copy()
    if o["rows"] == 1:
        R[0, 1] = R[1, 0] = 0.0; R[1, 1] = 1.0
    return R


def observe_model_dense(x, P, o):
    """(x', P', result) of one model observation: H = dh/dx at x, G = H P, S = G H' + R, nu = z - h(x) (bearings wrapped), K = G' S^-1,
    x += K nu, P -= K G, d2 = nu' S^-1 nu.  An observation that does not apply -- gated, S irregular, or q = 0 / not finite (reported as
    irregular, d2 NaN) -- leaves x and P as they are."""
    x, P = np.asarray(x, dtype=np.float64), np.asarray(P, dtype=np.float64)
    hx, H = jacobian(x, o)
    z = o["z"].copy()
    if o["rows"] == 1:
        z[1] = 0.0
    if H is None:
        return x.copy(), P.copy(), dict(nu=z, S=effective_R(o), d2=float("nan"), outcome=IRREGULAR)
    G = H @ P
    S = G @ H.T + effective_R(o)
    nu = z - hx
    for r in range(2):
        if WRAP[o["model"]][r]:
            nu[r] = wrap180(nu[r])
    outcome, d2 = decide(S, nu, o["gate"])
    res = dict(nu=nu, S=S, d2=d2, outcome=outcome)
    if outcome != APPLIED:
        return x.copy(), P.copy(), res
    Kg = G.T @ np.linalg.inv(S)
    return x + Kg @ nu, P - Kg @ G, res


def fmt(vals):
    """A line of operands for the host programs of tests/support: every value with all its digits."""
    return " ".join(repr(float(v)) for v in vals)


def small_line(o, x, P):
    """The 38 operands of linear_small for observation o on the dense state (x, P)."""
    lm = o["landmarks"]
    rows = list(range(3)) + sum(([3 + 2 * k, 4 + 2 * k] for k in lm), [])
    Ps, xs = np.zeros((7, 7)), np.zeros(7)
    Ps[:len(rows), :len(rows)] = P[np.ix_(rows, rows)]
    xs[:len(rows)] = x[rows]
    sm = list(Ps[:3, :3].reshape(-1))
    for b in range(2):
        sm += [Ps[t, 3 + 2 * b + r] for t in range(3) for r in range(2)]
    for b in range(2):
        a = 3 + 2 * b
        sm += [Ps[a, a], Ps[a + 1, a], Ps[a + 1, a + 1]]
    sm += [Ps[3 + r, 5 + c] for r in range(2) for c in range(2)]
    sm += list(xs)
    R = effective_R(o)
    anchor = [0.0, 0.0] if o["anchor"] is None else o["anchor"]
    z = o["z"].copy()
    if o["rows"] == 1:
        z[1] = 0.0
    return "small %d %d %s" % (o["model"], 1 if lm else 0, fmt(list(z) + list(R.reshape(-1)) + [o["gate"]] + list(anchor) + sm))
