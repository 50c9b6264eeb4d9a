"""Pure-NumPy side of the iterated model observation (ekf_observe_model_iterated / ekf_model_innovation_iterated / ekf_model_iterate):
the loop of ekfm::model_iterate restated on a dense P, the MAP cost it descends, and the scenes the CPU and GPU tests share.  No GPU, no
library."""
import numpy as np

import model_obs_cases as M
from model_obs_cases import APPLIED, GATED, INF, IRREGULAR, decide, wrap180  # noqa: F401

ITER_MAX = 16


def local_rows(o):
    """The rows of the state the loop runs over: the robot and the observation's landmarks, in its order."""
    return list(range(3)) + sum(([3 + 2 * k, 4 + 2 * k] for k in o["landmarks"]), [])


def _z(o):
    z = o["z"].copy()
    if o["rows"] == 1:
        z[1] = 0.0
    return z


def _wrapped(o, v):
    v = v.copy()
    for r in range(2):
        if M.WRAP[o["model"]][r]:
            v[r] = wrap180(v[r])
    return v


def iterate_dense(x, P, o, iterations, tol=0.0):
    """(x', P', first, it) of one iterated observation on the dense state.
        xi_0 = x0;  (h_i, H_i) at xi_i;  S_i = H_i P H_i' + R;  r_i = wrap(z - h_i) - H_i (x0 - xi_i);  xi_{i+1} = x0 + P H_i' S_i^-1 r_i
    over the rows of the robot and the observation's landmarks, stopped after `iterations` or where max |xi_{i+1} - xi_i| <= tol; the
    last linearisation's H, S and r then update the WHOLE state: K = P H' S^-1, x += K r, P -= K H P.
    first = {'nu', 'S', 'd2', 'outcome'}: the first linearisation's, the call's outcome (gated there, or irregular at ANY iterate: x and
    P unchanged).  it = {'S', 'nu', 'used', 'converged', 'last_step', 'x_local' (7: absent landmarks 0), 'H' (2 x n: the pair's Jacobian)}."""
    x, P = np.asarray(x, dtype=np.float64), np.asarray(P, dtype=np.float64)
    n = x.size
    loc = local_rows(o)
    R, z = M.effective_R(o), _z(o)
    x0 = x.copy()
    xi = x0.copy()
    first, used, converged, last_step = None, 0, False, 0.0
    outcome = APPLIED
    S = r = H = None
    for i in range(int(iterations)):
        hx, H = M.jacobian(xi, o)
        posed = H is not None and np.isfinite(xi[2])
        if not posed:
            hx, H = np.zeros(2), np.zeros((2, n))
        S = H @ P @ H.T + R
        r = _wrapped(o, z - hx)
        if i == 0:
            outcome, d2 = decide(S, r, o["gate"])
            if not posed:
                outcome, d2 = IRREGULAR, float("nan")
            first = dict(nu=r.copy(), S=S.copy(), d2=d2, outcome=outcome)
        else:
            r = r - H @ (x0 - xi)
            if not posed or decide(S, r, INF)[0] == IRREGULAR:
                outcome = IRREGULAR
        if outcome != APPLIED:
            break
        new = x0.copy()
        new[loc] = x0[loc] + (P[np.ix_(loc, loc)] @ H[:, loc].T) @ np.linalg.solve(S, r)
        last_step = float(np.abs(new - xi).max())
        xi = new
        used = i + 1
        converged = last_step <= tol
        if converged:
            break
    first["outcome"] = outcome
    xl = np.zeros(7)
    xl[:len(loc)] = xi[loc]
    it = dict(S=S, nu=r, used=used, converged=bool(converged), last_step=last_step, x_local=xl, H=H)
    if outcome != APPLIED:
        return x.copy(), P.copy(), first, it
    K = P @ H.T @ np.linalg.inv(S)
    return x + K @ r, P - K @ (H @ P), first, it


def map_cost(xq, x0, P, o):
    """J(x) = (x - x0)' P^-1 (x - x0) + nu(x)' R^-1 nu(x), nu = z - h(x) with the bearings wrapped (two-row models, R > 0)."""
    hx, _ = M.jacobian(xq, o)
    nu = _wrapped(o, _z(o) - hx)
    d = np.asarray(xq) - np.asarray(x0)
    return float(d @ np.linalg.solve(P, d) + nu @ np.linalg.solve(M.effective_R(o), nu))


def cost_gradient(xq, x0, P, o, step=1e-6):
    """The gradient of map_cost by central differences."""
    g = np.zeros(len(xq))
    for k in range(len(xq)):
        hi, lo = np.array(xq, dtype=np.float64), np.array(xq, dtype=np.float64)
        hi[k] += step; lo[k] -= step
        g[k] = (map_cost(hi, x0, P, o) - map_cost(lo, x0, P, o)) / (2.0 * step)
    return g


def map_scene(model):
    """The scene of the MAP tests: a robot known to 0.5 m and 10 degrees, one landmark known to 2 m at 10 m, a sensor far better than
    either, and a z drawn 0.6-1.2 sigma off the prior in every direction.  Returns (x0, P, o) with o on landmark 0."""
    x0 = np.array([0.3, -0.2, 5.0, 10.0, 1.0])
    A = 0.1 * np.random.default_rng(3).standard_normal((5, 5))
    P = np.diag([0.25, 0.25, 100.0, 4.0, 4.0]) + A @ A.T
    truth = x0 + np.linalg.cholesky(P) @ np.array([0.8, -0.6, 1.2, -0.9, 0.7])
    R = np.diag([0.01, 0.25]) if model == M.RANGE_BEARING else 0.01 * np.eye(2)
    o = M.obs(model, [0.0, 0.0], R, [0])
    o["z"] = M.jacobian(truth, o)[0]
    return x0, P, o


def anchor_hit_scene():
    """An anchored bearing whose first step puts the robot EXACTLY on the anchor, in powers of two: x0 = 0, the anchor at (4, 0), so
    H = [0, -k/4, -1]; P = [[2, 0, -1], [0, 0, 0], [-1, 0, 1]] gives G = (1, 0, -1) and S = 1 + R = 2; z = 8 degrees gives
    xi_1 = (0.5 * 8, 0, -0.5 * 8) = (4, 0, -4): q = 0 at the second linearisation."""
    x = np.zeros(3)
    P = np.array([[2.0, 0.0, -1.0], [0.0, 0.0, 0.0], [-1.0, 0.0, 1.0]])
    return x, P, M.obs(M.BEARING, [8.0], 1.0, anchor=[4.0, 0.0])


def iter_line(o, x, P, iterations, tol):
    """One line for tests/support/model_iter_host.cpp: model_obs_cases.small_line's operands, then iterations and tol."""
    return "iter" + M.small_line(o, x, P)[len("small"):] + " %d %r" % (int(iterations), float(tol))


def parse_iter(row):
    """A row of the host program's answer as (first, it, H (2 x 7), Gs (2 x 7))."""
    first = dict(outcome=int(row[0]), d2=row[1], nu=np.array(row[2:4]), S=np.array(row[4:8]).reshape(2, 2))
    it = dict(S=np.array(row[8:12]).reshape(2, 2), nu=np.array(row[12:14]), used=int(row[14]), converged=bool(row[15]), last_step=row[16],
              x_local=np.array(row[17:24]))
    return first, it, np.array(row[24:38]).reshape(2, 7), np.array(row[38:52]).reshape(2, 7)


def cases_all_models(rng):
    """(name, x, P, o) over the five models, landmark and anchor targets, on a correlated state of 4 landmarks: priors wide enough for
    the iterates to move, targets 8-25 away."""
    import linear_obs_cases as C
    x, P, _ = C.random_state(rng, 4)
    x[3:] = x[:2].repeat(4).reshape(2, 4).T.reshape(-1) + np.array([12.0, 3.0, -8.0, 9.0, 5.0, -14.0, -20.0, -6.0])
    P = P * 0.5
    P[2, 2] += 20.0
    out = []

    def near(o, sigma):
        hx = M.jacobian(x, o)[0]
        o["z"][:o["rows"]] = hx[:o["rows"]] + sigma * rng.standard_normal(o["rows"])
        return o
    out.append(("range and bearing", x, P, near(M.obs(M.RANGE_BEARING, [0, 0], np.diag([0.01, 0.25]), [2]), 0.5)))
    out.append(("range", x, P, near(M.obs(M.RANGE, [0], 0.01, [0]), 0.5)))
    out.append(("bearing", x, P, near(M.obs(M.BEARING, [0], 0.25, [3]), 2.0)))
    out.append(("relative xy", x, P, near(M.obs(M.RELATIVE_XY, [0, 0], 0.01 * np.eye(2), [1]), 0.5)))
    out.append(("landmark range", x, P, near(M.obs(M.LANDMARK_RANGE, [0], 0.01, [3, 1]), 0.5)))
    out.append(("range and bearing, anchor", x, P, near(M.obs(M.RANGE_BEARING, [0, 0], np.diag([0.01, 0.25]), anchor=[15.0, 4.0]), 0.5)))
    out.append(("range, anchor", x, P, near(M.obs(M.RANGE, [0], 0.01, anchor=[-9.0, 7.0]), 0.5)))
    out.append(("bearing, anchor", x, P, near(M.obs(M.BEARING, [0], 0.25, anchor=[3.0, -16.0]), 2.0)))
    out.append(("relative xy, anchor", x, P, near(M.obs(M.RELATIVE_XY, [0, 0], 0.01 * np.eye(2), anchor=[15.0, 4.0]), 0.5)))
    return out
