"""Pure-NumPy side of the ekf_observe_model_joint_iterated tests: the dense restatement of the relinearised joint update built on
joint_cases.joint_dense's H, S and nu, the same loop in numpy.longdouble (the restatement's own error), the MAP cost it descends, and the
wide-prior scene the CPU and GPU tests share, with its premises asserted where it is built.  No GPU, no library."""
import numpy as np

import associate_model_cases as A
import joint_cases as J
import model_obs_cases as M
import observe_joint_cases as C
from removal_cases import lowrank_data

APPLIED, IRREGULAR, GATED, INF = C.APPLIED, C.IRREGULAR, C.GATED, C.INF
ITER_MAX = 16
NPS = (1, 2, 5, 32)
R_OF = {M.RANGE_BEARING: np.diag([0.01, 0.25]), M.RANGE: 0.01, M.BEARING: 0.25, M.RELATIVE_XY: 0.01 * np.eye(2)}


def sub_rows(hyp):
    """The rows of the state the loop runs over: the robot, then the paired landmarks in scan order."""
    return [0, 1, 2] + [3 + 2 * int(l) + c for l in hyp if l >= 0 for c in range(2)]


def joint_update_iterated_dense(x, P, entries, hyp, iterations, tol=0.0, gate=INF):
    """(x', P', record, it) of ekf_observe_model_joint_iterated on the dense state.
        xi_0 = x0;  H_i, nu_i, S_i = H_i P H_i' + R: joint_dense at xi_i with the PRIOR P;  r_i = nu_i - H_i (x0 - xi_i) (i = 0: nu_0)
        xi_{i+1} = x0 + P H_i' S_i^-1 r_i over the rows of the robot and the paired landmarks;  step = max |xi_{i+1} - xi_i|
    stopped after `iterations` or where step <= tol; the last linearisation's H, S and r update the WHOLE state in
    observe_joint_cases.joint_update_dense's form: K = (S^-1 H P)', x' = x + K r, P' = P - K H P.  The record is the FIRST linearisation's
    (joint_dense's) with the call's outcome: gated there, or irregular at ANY iterate -- x and P unchanged.  it = {'used', 'converged',
    'step', 'steps' (every step taken), 'd2_last', 'irregular_at', 'irregular_obs', 'x_sub', 'H', 'S', 'r' (the last linearisation's paired
    rows)}."""
    x, P = np.asarray(x, dtype=np.float64), np.asarray(P, dtype=np.float64)
    rows = C.paired_rows(hyp)
    loc = sub_rows(hyp)
    with np.errstate(all="ignore"):
        rec = J.joint_dense(x, P, entries, hyp)
    it = dict(used=0, converged=False, step=0.0, steps=[], d2_last=rec["d2"], irregular_at=-1, irregular_obs=-1, x_sub=x[loc].copy(), H=None, S=None, r=None)
    if rec["outcome"] != J.REGULAR:
        return x.copy(), P.copy(), dict(rec, outcome=IRREGULAR), dict(it, irregular_at=0, irregular_obs=rec["first_irregular"])
    if not rec["d2"] <= gate:
        return x.copy(), P.copy(), dict(rec, outcome=GATED), it
    if not rows:
        return x.copy(), P.copy(), dict(rec, outcome=APPLIED), dict(it, converged=True)
    xi = x.copy()
    lin = rec
    for i in range(int(iterations)):
        if i > 0:
            with np.errstate(all="ignore"):
                lin = J.joint_dense(xi, P, entries, hyp)
            if lin["outcome"] != J.REGULAR:
                return x.copy(), P.copy(), dict(rec, outcome=IRREGULAR), dict(it, irregular_at=i, irregular_obs=lin["first_irregular"], x_sub=xi[loc].copy())
        H, S, r = lin["H"][rows], lin["S"][np.ix_(rows, rows)], lin["nu"][rows]
        if i > 0:
            r = r - H @ (x - xi)
        G = H @ P
        with np.errstate(all="ignore"):
            new = x.copy()
            new[loc] = x[loc] + np.linalg.solve(S, G[:, loc]).T @ r
            step = float(np.nanmax(np.abs(new - xi)))
            d2 = float(r @ np.linalg.solve(S, r))
        xi = new
        it["steps"].append(step)
        it.update(used=i + 1, converged=step <= tol, step=step, d2_last=d2, H=H, S=S, r=r)
        if it["converged"]:
            break
    it["x_sub"] = xi[loc].copy()
    K = np.linalg.solve(S, G).T                              # joint_update_dense's expressions: iterations = 1 is that update exactly
    return x + K @ r, P - K @ G, dict(rec, outcome=APPLIED), it


# ------------------------------------------------------------------------------------------------------------------
# the same loop in numpy.longdouble on the sub-state: what the float64 restatement's own rounding amounts to
# ------------------------------------------------------------------------------------------------------------------
LD = np.longdouble
PI_LD = 4 * np.arctan(LD(1))
K_LD = LD(180) / PI_LD


def _wrap_ld(v):
    return v - LD(360) * np.ceil((v - LD(180)) / LD(360))


def _lin_ld(xi, entries):
    """(H (2 np x ns), nu, blockdiag R) of every pairing at xi over the sub-state, pairing p on its own landmark, in longdouble."""
    npair = len(entries)
    ns = 3 + 2 * npair
    H, nu, Rb = np.zeros((2 * npair, ns), dtype=LD), np.zeros(2 * npair, dtype=LD), np.zeros((2 * npair, 2 * npair), dtype=LD)
    for p, ent in enumerate(entries):
        model = ent["model"]
        o = M.obs(model, ent["z"], ent["R"], [0])
        d = xi[3 + 2 * p:5 + 2 * p] - xi[:2]
        q = d @ d
        r = np.sqrt(q)
        th = xi[2]
        rng_r, rng_t = np.array([-d[0] / r, -d[1] / r, LD(0)]), np.array([d[0] / r, d[1] / r])
        brg_r, brg_t = np.array([K_LD * d[1] / q, -K_LD * d[0] / q, LD(-1)]), np.array([-K_LD * d[1] / q, K_LD * d[0] / q])
        bearing = np.arctan2(d[1], d[0]) * K_LD - th
        c, s = np.cos(th / K_LD), np.sin(th / K_LD)
        hx = np.zeros(2, dtype=LD)
        Hr, Ht = np.zeros((2, 3), dtype=LD), np.zeros((2, 2), dtype=LD)
        if model == M.RANGE_BEARING:
            hx[:] = [r, bearing]; Hr[0], Ht[0], Hr[1], Ht[1] = rng_r, rng_t, brg_r, brg_t
        elif model == M.RANGE:
            hx[0] = r; Hr[0], Ht[0] = rng_r, rng_t
        elif model == M.BEARING:
            hx[0] = bearing; Hr[0], Ht[0] = brg_r, brg_t
        else:
            hx[:] = [c * d[0] + s * d[1], -s * d[0] + c * d[1]]
            Hr[0], Ht[0] = [-c, -s, hx[1] / K_LD], [c, s]
            Hr[1], Ht[1] = [s, -c, -hx[0] / K_LD], [-s, c]
        z = o["z"].astype(LD)
        if o["rows"] == 1:
            z[1] = 0
        v = z - hx
        for rr in range(2):
            if M.WRAP[model][rr]:
                v[rr] = _wrap_ld(v[rr])
        H[2 * p:2 * p + 2, :3], H[2 * p:2 * p + 2, 3 + 2 * p:5 + 2 * p] = Hr, Ht
        nu[2 * p:2 * p + 2] = v
        Rb[2 * p:2 * p + 2, 2 * p:2 * p + 2] = M.effective_R(o).astype(LD)
    return H, nu, Rb


def _solve_ld(S, B):
    """S^-1 B through a Cholesky factorisation, in longdouble (numpy.linalg has none)."""
    n = S.shape[0]
    Lc = np.zeros_like(S)
    for j in range(n):
        Lc[j, j] = np.sqrt(S[j, j] - Lc[j, :j] @ Lc[j, :j])
        for i in range(j + 1, n):
            Lc[i, j] = (S[i, j] - Lc[i, :j] @ Lc[j, :j]) / Lc[j, j]
    Y = np.array(B, dtype=LD)
    for i in range(n):
        Y[i] = (Y[i] - Lc[i, :i] @ Y[:i]) / Lc[i, i]
    for i in range(n - 1, -1, -1):
        Y[i] = (Y[i] - Lc[i + 1:, i] @ Y[i + 1:]) / Lc[i, i]
    return Y


def iterate_sub_longdouble(x_sub, P_sub, entries, iterations):
    """(x', P') of the loop over the sub-state alone (every entry paired with its own landmark, tol = 0), every operation in longdouble."""
    x0, P = np.asarray(x_sub).astype(LD), np.asarray(P_sub).astype(LD)
    xi = x0.copy()
    for i in range(int(iterations)):
        H, r, Rb = _lin_ld(xi, entries)
        if i > 0:
            r = r - H @ (x0 - xi)
        G = H @ P
        S = G @ H.T + Rb
        new = x0 + _solve_ld(S, G).T @ r
        step = np.abs(new - xi).max()
        xi = new
        if step == 0:
            break
    Kt = _solve_ld(S, G)
    return x0 + Kt.T @ r, P - Kt.T @ G


def map_cost(xq, x0, P, entries, hyp):
    """J(x) = (x - x0)' P_sub^-1 (x - x0) + nu(x)' R^-1 nu(x) over the sub-state's rows, nu by joint_dense (bearings wrapped)."""
    loc, rows = sub_rows(hyp), C.paired_rows(hyp)
    lin = J.joint_dense(xq, P, entries, hyp)
    nu = lin["nu"][rows]
    Rb = lin["S"][np.ix_(rows, rows)] - lin["H"][rows] @ P @ lin["H"][rows].T
    d = (np.asarray(xq) - np.asarray(x0))[loc]
    return float(d @ np.linalg.solve(P[np.ix_(loc, loc)], d) + nu @ np.linalg.solve(Rb, nu))


def map_gradient(xq, x0, P, entries, hyp):
    """Half the gradient of map_cost over the sub-state: P_sub^-1 (xi - x0) - H' R^-1 wrap(z - h(xi))."""
    loc, rows = sub_rows(hyp), C.paired_rows(hyp)
    lin = J.joint_dense(xq, P, entries, hyp)
    H, nu = lin["H"][rows][:, loc], lin["nu"][rows]
    Rb = lin["S"][np.ix_(rows, rows)] - lin["H"][rows] @ P @ lin["H"][rows].T
    return np.linalg.solve(P[np.ix_(loc, loc)], (np.asarray(xq) - np.asarray(x0))[loc]) - H.T @ np.linalg.solve(Rb, nu)


# ------------------------------------------------------------------------------------------------------------------
# the wide-prior scene
# ------------------------------------------------------------------------------------------------------------------
NEAR = 0.15


def wide_scene(npair, N=J.N0, offset=1.0):
    """(x, s, d, U, entries, landmarks): lowrank_data(N, 5) with the robot known to 0.5 m and 10 degrees, the scan's landmarks
    (7 q + 3) mod N known to 2 m (d = 4, plus five times the correlations of U) and moved to 5-30 m around the robot, and a sensor far
    better than either -- R = diag(0.01 m^2, 0.25 deg^2) and its one-row parts -- the models cycling 1, 2, 3, 4; z = h(truth) with the truth
    `offset` times 0.6-1.2 sigma off the prior in every direction of the sub-state.  offset = 1 is the scene of every leg but the `tol`
    leg: there Gauss-Newton converges linearly at 7-50 a step (the prior's residual does not vanish at the mode), so no two neighbouring
    steps leave a tolerance a factor 10 of room on both sides; with the truth NEAR = 0.15 times as far off the rate is 60-6000 a step and
    pick_tol finds its gap among the first four steps, far above rounding."""
    x, s, d, U = lowrank_data(N, 5)
    x, d, U = x.copy(), d.copy(), 5.0 * U
    lms = C.scan_landmarks(npair, N)
    d[:3] = [0.25, 0.25, 100.0]
    rng = np.random.default_rng(11)
    for q, lm in enumerate(lms):
        r, phi = 5.0 + 25.0 * ((q * 0.37) % 1.0), 2.0 * np.pi * ((0.11 + q * 0.618) % 1.0)
        x[3 + 2 * lm:5 + 2 * lm] = x[:2] + r * np.array([np.cos(phi), np.sin(phi)])
        d[3 + 2 * lm:5 + 2 * lm] = 4.0
    P = np.diag(d) + U @ U.T
    loc = sub_rows(lms)
    draw = offset * rng.uniform(0.6, 1.2, len(loc)) * rng.choice([-1.0, 1.0], len(loc))
    truth = x.copy()
    truth[loc] = x[loc] + np.linalg.cholesky(P[np.ix_(loc, loc)]) @ draw
    ents = []
    for q, lm in enumerate(lms):
        model = 1 + q % 4
        hx = M.h_of(model, truth[:3], truth[3 + 2 * lm:5 + 2 * lm])
        ents.append(A.entry(model, hx[:M.ROWS[model]], R_OF[model]))
    return x, s, d, U, ents, lms


def scene_dense(npair, N=J.N0, offset=1.0):
    x, _, d, U, ents, lms = wide_scene(npair, N, offset)
    return x, np.diag(d) + U @ U.T, ents, lms


def pick_tol(steps):
    """(tol, used): a tolerance between two neighbouring steps of the restatement with a factor >= 10 of room on either side -- the first
    such gap behind the second step -- so that `used` cannot flip by rounding."""
    for k in range(2, len(steps)):
        if steps[k - 1] >= 100.0 * steps[k] and steps[k] > 0.0:
            return float(np.sqrt(steps[k - 1] * steps[k])), k + 1
    raise AssertionError("no two neighbouring steps a factor 100 apart: %s" % steps)


def later_irregular(npair=2):
    """The wide scene with the first entry's range replaced by 1e200: the first linearisation is regular, xi_1 lies ~1e200 away, where
    q = |d|^2 overflows -- the second linearisation is not posed.  Returns (x, P, entries, landmarks)."""
    x, P, ents, lms = scene_dense(npair)
    assert ents[0]["model"] == M.RANGE_BEARING
    ents = [dict(ents[0], z=np.array([1e200, ents[0]["z"][1]]))] + ents[1:]
    return x, P, ents, lms


def assert_scene_premises():
    """Per np of NPS on the wide scene, asserted and returned as (np, steps, J1, J3, tol, used_at_tol):
      * Gauss-Newton converges: the steps decrease from the second on (down to 1e-12: below that a step is rounding of entries of size
        10-30, a few 1e-15, and no longer ordered), and are below 1e-9 by 16 linearisations;
      * the MAP cost after 3 linearisations is strictly below the cost after 1;
      * no step of the first 8 is exactly 0, so tol = 0 runs all of them;
      * on the NEAR scene, a tol with a factor >= 10 of room to the neighbouring steps on either side;
    and the irregular-later input: regular at the first linearisation, irregular at the second."""
    out = []
    for npair in NPS:
        x, P, ents, lms = scene_dense(npair)
        _, _, rec, it = joint_update_iterated_dense(x, P, ents, lms, ITER_MAX)
        steps = it["steps"]
        assert rec["outcome"] == APPLIED and rec["pairings"] == npair and len(steps) == ITER_MAX
        assert all(steps[k] < steps[k - 1] for k in range(2, ITER_MAX) if steps[k - 1] > 1e-12), steps
        assert steps[-1] < 1e-9 and all(v > 0.0 for v in steps[:8]), steps
        x1 = joint_update_iterated_dense(x, P, ents, lms, 1)[0]
        x3 = joint_update_iterated_dense(x, P, ents, lms, 3)[0]
        J1, J3 = map_cost(x1, x, P, ents, lms), map_cost(x3, x, P, ents, lms)
        assert J3 < J1, (J1, J3)
        near = joint_update_iterated_dense(*scene_dense(npair, offset=NEAR), ITER_MAX)[3]["steps"]
        tol, used = pick_tol(near)
        assert near[used - 2] >= 10.0 * tol and tol >= 10.0 * near[used - 1] and near[used - 1] > 1e-10
        print("np = %2d: steps %s; J after 1: %.6g, after 3: %.6g; tol %.3g stops after %d" % (npair, ["%.2e" % v for v in steps[:9]], J1, J3, tol, used))
        out.append((npair, steps, J1, J3, tol, used))
    x, P, ents, lms = later_irregular()
    _, _, rec, it = joint_update_iterated_dense(x, P, ents, lms, 3)
    with np.errstate(all="ignore"):                       # (d2 of the far range overflows: the first linearisation is regular all the same)
        assert J.joint_dense(x, P, ents, lms)["outcome"] == J.REGULAR
    assert (rec["outcome"], it["irregular_at"], it["irregular_obs"], it["used"]) == (IRREGULAR, 1, 0, 1)
    return out
