"""Pure-NumPy side of the ekf_predict_model tests: the three motion models as include/ekfslam.h states them, restated in radians with
np.sin / np.cos, their finite-difference Jacobians, the exact circle that ARC's chord form must equal, and the dense restatement of a chain
of steps (the n x n F, F @ P @ F.T plus the embedded V M V').  No GPU, no library; not a transcription of the kernel."""
import numpy as np

K = 180.0 / np.pi
TURN_DRIVE, ARC, POSE_DELTA = 1, 2, 3
INPUTS = {TURN_DRIVE: 2, ARC: 2, POSE_DELTA: 3}


def wrap360(a):
    """mod(a, 360) with positive multiples of 360 mapped to 360."""
    w = float(np.mod(a, 360.0))
    return 360.0 if w == 0.0 and a > 0.0 else w


def chord(a):
    """g = sin a / a and g' = (a cos a - sin a) / a^2; below 1e-3 the two leading terms of the series (the next: a^4 / 120 < 1e-14)."""
    if abs(a) < 1e-3:
        return 1.0 - a * a / 6.0, -a / 3.0 + a ** 3 / 30.0
    return np.sin(a) / a, (a * np.cos(a) - np.sin(a)) / (a * a)


def f_of(model, xr, u):
    """The new pose, the heading NOT wrapped (so that it can be differentiated)."""
    x, y, th = (float(v) for v in xr)
    u = np.asarray(u, dtype=np.float64)
    if model == TURN_DRIVE:
        phi = np.radians(th + u[1])
        return np.array([x + u[0] * np.cos(phi), y + u[0] * np.sin(phi), th + u[1]])
    if model == ARC:
        a = np.radians(u[1]) / 2.0
        g = chord(a)[0]
        phi = np.radians(th) + a
        return np.array([x + u[0] * g * np.cos(phi), y + u[0] * g * np.sin(phi), th + u[1]])
    assert model == POSE_DELTA
    c, s = np.cos(np.radians(th)), np.sin(np.radians(th))
    return np.array([x + c * u[0] - s * u[1], y + s * u[0] + c * u[1], th + u[2]])


def arc_on_the_circle(xr, u):
    """ARC without the chord: the circle of radius d / turn through the pose, tangent to the heading (turn != 0)."""
    x, y, th = (float(v) for v in xr)
    t = np.radians(u[1])
    r = u[0] / t
    a0 = np.radians(th)
    return np.array([x + r * (np.sin(a0 + t) - np.sin(a0)), y - r * (np.cos(a0 + t) - np.cos(a0)), th + u[1]])


def F_V_of(model, xr, u):
    """(F, V): df/dx_r (3 x 3) and df/du (3 x inputs), the table of include/ekfslam.h with theta in degrees."""
    th = float(xr[2])
    u = np.asarray(u, dtype=np.float64)
    F = np.eye(3)
    if model == TURN_DRIVE:
        phi = np.radians(th + u[1])
        c, s = np.cos(phi), np.sin(phi)
        F[0, 2], F[1, 2] = -u[0] * s / K, u[0] * c / K
        V = np.array([[c, F[0, 2]], [s, F[1, 2]], [0.0, 1.0]])
    elif model == ARC:
        a = np.radians(u[1]) / 2.0
        g, gp = chord(a)
        phi = np.radians(th) + a
        c, s = np.cos(phi), np.sin(phi)
        F[0, 2], F[1, 2] = -u[0] * g * s / K, u[0] * g * c / K
        V = np.array([[g * c, u[0] * (gp * c - g * s) / (2.0 * K)], [g * s, u[0] * (gp * s + g * c) / (2.0 * K)], [0.0, 1.0]])
    else:
        assert model == POSE_DELTA
        c, s = np.cos(np.radians(th)), np.sin(np.radians(th))
        F[0, 2], F[1, 2] = (-s * u[0] - c * u[1]) / K, (c * u[0] - s * u[1]) / K
        V = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    return F, V


def F_V_fd(model, xr, u, step=1e-5):
    """Central finite differences of f_of over (x, y, theta) and over u."""
    nu = INPUTS[model]
    v = np.concatenate([np.asarray(xr, dtype=np.float64), np.asarray(u, dtype=np.float64)[:nu]])
    J = np.zeros((3, 3 + nu))
    for i in range(3 + nu):
        hi, lo = v.copy(), v.copy()
        hi[i] += step; lo[i] -= step
        J[:, i] = (f_of(model, hi[:3], hi[3:]) - f_of(model, lo[:3], lo[3:])) / (2.0 * step)
    return J[:, :3], J[:, 3:]


def step(model, u, M):
    nu = INPUTS[int(model)]
    return (int(model), np.asarray(u, dtype=np.float64).reshape(-1)[:nu].copy(), np.asarray(M, dtype=np.float64).reshape(nu, nu).copy())


def predict_model_dense(x, P, steps):
    """(x', P', Q of the last step) after the chain: per step the dense n x n F (the identity over the map) and the noise V M V' embedded in
    the robot block."""
    x, P = np.array(x, dtype=np.float64), np.array(P, dtype=np.float64)
    n = x.size
    Q = np.zeros((3, 3))
    for model, u, M in steps:
        F3, V = F_V_of(model, x[:3], u)
        F = np.eye(n)
        F[:3, :3] = F3
        Q = V @ M @ V.T
        noise = np.zeros((n, n))
        noise[:3, :3] = Q
        P = F @ P @ F.T + noise
        P = (P + P.T) / 2.0
        pose = f_of(model, x[:3], u)
        x[:3] = [pose[0], pose[1], wrap360(pose[2])]
    return x, P, Q


def _M(rng, nu, scale):
    A = rng.uniform(-1.0, 1.0, (nu, nu))
    return (A @ A.T + 0.1 * np.eye(nu)) * scale * scale


def chain(rng, m):
    """m steps, seeded.  The first nine are built: from any heading in [0, 360] the turns +250, +250 carry it over 360 upward and -300, -300,
    -300 below 0 downward; a step of all zeros; an arc that turns too little for the closed forms (the series) and one of a whole circle;
    all three models.  Random ones follow."""
    M2, M3 = _M(rng, 2, 0.3), _M(rng, 3, 0.2)
    built = [step(TURN_DRIVE, [1.5, 250.0], M2), step(ARC, [2.0, 250.0], M2 * 2.0), step(POSE_DELTA, [0.0, 0.0, 0.0], np.zeros((3, 3))),
             step(POSE_DELTA, [0.4, -0.3, -300.0], M3), step(TURN_DRIVE, [0.7, -300.0], np.diag([0.04, 0.0])), step(ARC, [1.1, -300.0], M2),
             step(ARC, [0.9, 1e-3], M2), step(ARC, [3.0, 360.0], M2), step(POSE_DELTA, [-0.2, 0.5, 33.0], M3 * 0.5)]
    out = built[:m]
    while len(out) < m:
        model = int(rng.integers(1, 4))
        if model == POSE_DELTA:
            out.append(step(model, [rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-200, 200)], _M(rng, 3, 0.2)))
        else:
            out.append(step(model, [rng.uniform(-0.5, 2.0), rng.uniform(-200, 200)], _M(rng, 2, 0.3)))
    return out
