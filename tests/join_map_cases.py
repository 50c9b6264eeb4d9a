"""What the join_map tests share (tests/test_join_map_cpu.py, tests/test_join_map_gpu.py): the NumPy restatement of ekf_join_map through
the Jacobian J of the composite map, that map itself (for finite differences), and the builders of local states.  Nothing of ekf_slam_amd
is imported here: the builders take the engines they drive."""
import numpy as np

K = 180.0 / np.pi


def wrap360(a):
    """mod(a, 360) with positive multiples of 360 mapped to 360, as the library's wrapTo360."""
    w = np.mod(a, 360.0)
    return 360.0 if (w == 0.0 and a > 0.0) else float(w)


def rot(theta_deg):
    t = theta_deg / K
    return np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])


def join_fn(x, y, wrap=True):
    """The composite map: the joined state of the global state x = [r; l_1 .. l_N] and the local state y = [q; m_1 .. m_M] that is
    expressed in the frame of r."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    Rm = rot(x[2])
    out = np.concatenate([x, np.zeros(y.size - 3)])
    out[0:2] = x[0:2] + Rm @ y[0:2]
    out[2] = wrap360(x[2] + y[2]) if wrap else x[2] + y[2]
    for i in range((y.size - 3) // 2):
        out[x.size + 2 * i:x.size + 2 * i + 2] = x[0:2] + Rm @ y[3 + 2 * i:5 + 2 * i]
    return out


def join_jacobian(x, y):
    """J = d join_fn / d [x; y], heading entries in degrees: rows of the robot [J1 0 J2 0], of the old landmarks [0 I 0 0], of new landmark
    i [Gx_i 0 0 Rot at m_i]."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n, nl = x.size, y.size
    Rm = rot(x[2])
    J = np.zeros((n + nl - 3, n + nl))
    J[:n, :n] = np.eye(n)
    w = Rm @ y[0:2]
    J[0, 2], J[1, 2] = -w[1] / K, w[0] / K                 # J1
    J[0:2, n:n + 2] = Rm                                   # J2
    J[2, n + 2] = 1.0
    for i in range((nl - 3) // 2):
        r = n + 2 * i
        w = Rm @ y[3 + 2 * i:5 + 2 * i]
        J[r, 0] = J[r + 1, 1] = 1.0                        # Gx_i
        J[r, 2], J[r + 1, 2] = -w[1] / K, w[0] / K
        J[r:r + 2, n + 3 + 2 * i:n + 5 + 2 * i] = Rm       # Gz
    return J


def join_dense(x, s, P, y, sL, PL, offset=0.0):
    """(x', s', P') of ekf_join_map: x' = join_fn(x, y), s' = [s; sL + offset], P' = J blockdiag(P, PL) J'."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n, nl = x.size, y.size
    J = join_jacobian(x, y)
    B = np.zeros((n + nl, n + nl))
    B[:n, :n] = P
    B[n:, n:] = PL
    Pn = J @ B @ J.T
    return join_fn(x, y), np.concatenate([np.asarray(s, dtype=np.float64).reshape(-1), np.asarray(sL, dtype=np.float64).reshape(-1) + offset]), \
        0.5 * (Pn + Pn.T)


def random_spd(rng, n, scale=0.05):
    A = rng.standard_normal((n, n)) * np.sqrt(scale / max(n, 1))
    return A @ A.T + scale * 0.2 * np.eye(n)


def random_state(rng, N, pose=None, spread=20.0, scale=0.05):
    """(x, s, P) with N landmarks and a full covariance."""
    x = np.concatenate([rng.uniform(-5, 5, 2), [rng.uniform(20.0, 300.0)], rng.uniform(-spread, spread, 2 * N)])
    if pose is not None:
        x[:3] = pose
    return x, np.arange(1, N + 1, dtype=np.float64), random_spd(rng, 3 + 2 * N, scale)


def set_state(e, x, s, P):
    """An engine brought to (x, s, P) through the setters."""
    e.set_x(x)
    if np.asarray(s).size:
        e.set_s(s)
    e.set_P(P)
    return e


def stir_local(e, rng, pending):
    """A local engine made to look like a submap in use: a few model predicts (a non-zero pose, a full P) and corrections of its
    landmarks; `pending` of them are left in the ring where the engine's batch allows it."""
    R = np.array([[0.02, 0.005], [0.005, 0.03]])
    Mq = np.diag([0.01, 0.02, 0.3])
    M = e.N
    for k in range(3):
        e.predict_model([(3, [0.3 + 0.1 * k, -0.2, 4.0 + k], Mq)])
        if M:
            x = e.get_x()
            i = int(rng.integers(0, M))
            z = rot(x[2]).T @ (x[3 + 2 * i:5 + 2 * i] - x[0:2]) + rng.normal(0, 0.05, 2)
            e.observe_model(4, z, R, [i])
    e.flush()
    for k in range(pending if M else 0):
        x = e.get_x()
        i = int(rng.integers(0, M))
        z = rot(x[2]).T @ (x[3 + 2 * i:5 + 2 * i] - x[0:2]) + rng.normal(0, 0.05, 2)
        e.observe_model(4, z, R, [i])
    return e
