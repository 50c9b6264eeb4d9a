"""Pure-NumPy side of the ekf_append_model tests: the inverse of the two models that determine a point, as include/ekfslam.h states it,
its finite-difference Jacobians, and the dense restatement of a scan of new landmarks.  No GPU, no library."""
import numpy as np

from model_obs_cases import K, RANGE_BEARING, RELATIVE_XY  # noqa: F401


def _cs(deg):
    if deg % 90.0 == 0.0:                                      # cosd / sind are exact at multiples of 90 degrees
        return [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)][int(deg // 90.0) % 4]
    return np.cos(np.radians(deg)), np.sin(np.radians(deg))


def g_of(model, xr, z):
    """The landmark that z observes from the robot state xr = (x, y, theta in degrees)."""
    xr, z = np.asarray(xr, dtype=np.float64), np.asarray(z, dtype=np.float64)
    if model == RANGE_BEARING:
        c, s = _cs(xr[2] + z[1])
        return xr[:2] + z[0] * np.array([c, s])
    assert model == RELATIVE_XY
    c, s = _cs(xr[2])
    return xr[:2] + np.array([c * z[0] - s * z[1], s * z[0] + c * z[1]])


def G_of(model, xr, z):
    """(Gx, Gz): dg/dx_r (2 x 3) and dg/dz (2 x 2), the table of include/ekfslam.h."""
    xr, z = np.asarray(xr, dtype=np.float64), np.asarray(z, dtype=np.float64)
    if model == RANGE_BEARING:
        c, s = _cs(xr[2] + z[1])
        gth = np.array([-z[0] * s / K, z[0] * c / K])
        Gz = np.array([[c, gth[0]], [s, gth[1]]])
    else:
        assert model == RELATIVE_XY
        c, s = _cs(xr[2])
        w = np.array([c * z[0] - s * z[1], s * z[0] + c * z[1]])
        gth = np.array([-w[1] / K, w[0] / K])
        Gz = np.array([[c, -s], [s, c]])
    return np.array([[1.0, 0.0, gth[0]], [0.0, 1.0, gth[1]]]), Gz


def G_fd(model, xr, z, step=1e-6):
    """Central finite differences of g_of over (x, y, theta) and over z."""
    v = np.concatenate([np.asarray(xr, dtype=np.float64), np.asarray(z, dtype=np.float64)])
    J = np.zeros((2, 5))
    for i in range(5):
        hi, lo = v.copy(), v.copy()
        hi[i] += step; lo[i] -= step
        J[:, i] = (g_of(model, hi[:3], hi[3:]) - g_of(model, lo[:3], lo[3:])) / (2.0 * step)
    return J[:, :3], J[:, 3:]


def entry(model, z, R, signature):
    return (int(model), np.asarray(z, dtype=np.float64).reshape(2).copy(), np.asarray(R, dtype=np.float64).reshape(2, 2).copy(), float(signature))


def append_model_dense(x, s, P, entries):
    """(x', s', P') after one scan: every entry inverted at the SAME robot state, entry b the landmark N + b.
         x' = [x; t_0; ..]   P' = [P, P A'; A P, A P A' + blockdiag(Gz_b R_b Gz_b')]   A = [Gx_0 0; Gx_1 0; ..] over (robot | old landmarks)
    -- new landmarks of one scan are correlated with each other through the robot block only."""
    x, s, P = np.asarray(x, dtype=np.float64), np.asarray(s, dtype=np.float64), np.asarray(P, dtype=np.float64)
    n, m = x.size, len(entries)
    A = np.zeros((2 * m, n))
    noise = np.zeros((2 * m, 2 * m))
    t, sig = [], []
    for b, (model, z, R, signature) in enumerate(entries):
        Gx, Gz = G_of(model, x[:3], z)
        A[2 * b:2 * b + 2, :3] = Gx
        noise[2 * b:2 * b + 2, 2 * b:2 * b + 2] = Gz @ R @ Gz.T
        t.append(g_of(model, x[:3], z))
        sig.append(signature)
    AP = A @ P
    Pn = np.zeros((n + 2 * m, n + 2 * m))
    Pn[:n, :n] = P
    Pn[n:, :n] = AP
    Pn[:n, n:] = AP.T
    C = AP @ A.T + noise
    Pn[n:, n:] = (C + C.T) / 2.0
    return np.concatenate([x] + t), np.concatenate([s, sig]), Pn


def scan(rng, m, first_signature=5000.0):
    """m entries, the two models alternating, seeded: ranges 2 .. 25, bearings over the whole circle, a full R."""
    out = []
    for b in range(m):
        R = np.array([[0.02, 0.004], [0.004, 0.03]]) * (1.0 + 0.1 * b)
        if b % 2 == 0:
            out.append(entry(RANGE_BEARING, [rng.uniform(2.0, 25.0), rng.uniform(-180.0, 540.0)], R * [[1.0, 3.0], [3.0, 40.0]], first_signature + b))
        else:
            out.append(entry(RELATIVE_XY, rng.uniform(-15.0, 15.0, 2), R, first_signature + b))
    return out
