"""What the transform_map tests share (tests/test_transform_map_cpu.py, tests/test_transform_map_gpu.py): the NumPy restatement of
ekf_transform_map -- the map (x, t) -> x', its Jacobians T = dx'/dx and A = dx'/dt and P' = T P T' + A Sigma A' --, the forms, the scenes
and the comparison the float robot-frame legs need.  Nothing of ekf_slam_amd is imported here: the builders take the engines they drive."""
import numpy as np

from extract_map_cases import extract_dense, extract_fn, extract_jacobian, scene, scene_on_robot  # noqa: F401  (re-exported)
from join_map_cases import K, random_spd, rot, set_state, wrap360  # noqa: F401  (re-exported)

FORMS = ("exact", "uncertain", "robot")
T_RIGID = np.array([3.5, -2.25, 37.0])
SIGMA = np.array([[0.04, 0.01, 0.02], [0.01, 0.09, -0.03], [0.02, -0.03, 0.5]])


def form_args(form, t=T_RIGID, Sigma=SIGMA):
    """(frame, t, Sigma) of a form as Engine.transform_map takes them."""
    return {"exact": ("map", t, None), "uncertain": ("map", t, Sigma), "robot": ("robot", None, None)}[form]


def transform_fn(x, t, wrap=True):
    """x' of the rigid transform t = (tx, ty, phi): the robot t (+) r, every landmark t_xy + Rot(phi) l."""
    x, t = np.asarray(x, dtype=np.float64), np.asarray(t, dtype=np.float64)
    Rm = rot(t[2])
    out = np.empty_like(x)
    out[0:2] = t[0:2] + Rm @ x[0:2]
    out[2] = wrap360(t[2] + x[2]) if wrap else t[2] + x[2]
    out[3:] = (t[0:2][:, None] + Rm @ x[3:].reshape(-1, 2).T).T.reshape(-1)
    return out


def transform_jacobians(x, t):
    """(T, A): T = blockdiag(V, Rot, .., Rot) with V = blockdiag(Rot, 1); A = (F; A_1; ..; A_N), every block [1 0 -w1/k; 0 1 w0/k] at
    w = Rot v, the robot's closed by the row (0, 0, 1)."""
    x, t = np.asarray(x, dtype=np.float64), np.asarray(t, dtype=np.float64)
    n = x.size
    Rm = rot(t[2])
    T = np.zeros((n, n))
    T[0:2, 0:2] = Rm
    T[2, 2] = 1.0
    A = np.zeros((n, 3))
    w = Rm @ x[0:2]
    A[0:3] = np.array([[1, 0, -w[1] / K], [0, 1, w[0] / K], [0, 0, 1]])
    for a in range(3, n, 2):
        T[a:a + 2, a:a + 2] = Rm
        w = Rm @ x[a:a + 2]
        A[a:a + 2] = np.array([[1, 0, -w[1] / K], [0, 1, w[0] / K]])
    return T, A


def transform_dense(x, s, P, form, t=T_RIGID, Sigma=SIGMA):
    """(x', s', P') of ekf_transform_map for one of FORMS; s' = s.  The robot form is extract_map's restatement over every landmark."""
    x, s, P = np.asarray(x, dtype=np.float64), np.asarray(s, dtype=np.float64).reshape(-1), np.asarray(P, dtype=np.float64)
    if form == "robot":
        return extract_dense(x, s, P, list(range((x.size - 3) // 2)), "robot")
    T, A = transform_jacobians(x, t)
    Pn = T @ P @ T.T
    if form == "uncertain":
        Pn = Pn + A @ np.asarray(Sigma, dtype=np.float64) @ A.T
    else:
        assert form == "exact"
    return transform_fn(x, t), s.copy(), 0.5 * (Pn + Pn.T)


def check_robot_frame(e, ex, eP, storage, label, es, tols):
    """A handle that holds a robot-frame map against (ex, es, eP): the robot rows and columns of P exactly zero, then the measures of
    helpers.check_state taken over the landmark rows (a zero row has no scale to measure against).  tols = (REL, TOL_X32, TOL_KEPT32,
    TOL_ROW32) of helpers.py."""
    REL, TOL_X32, TOL_KEPT32, TOL_ROW32 = tols
    x, s, P = e.get_x(), e.get_s(), e.get_P()
    blocks = e.get_P_diag_blocks()
    assert e.N == es.size
    np.testing.assert_array_equal(s, es)
    np.testing.assert_array_equal(P, P.T)
    assert not P[:3, :].any() and not x[:3].any() and not blocks[0].any()
    if es.size == 0:
        return
    n = ex.size
    kept = np.zeros((n, n), dtype=bool)
    for a in range(3, n, 2):
        kept[a:a + 2, a:a + 2] = True
    scale = np.abs(eP).max()
    err_x = float(np.abs(x - ex).max() / np.abs(ex).max())
    err_P = float(np.abs(P - eP).max() / scale)
    err_b = float(np.abs(blocks[1:] - np.array([eP[a:a + 2, a:a + 2] for a in range(3, n, 2)])).max() / scale)
    err_kept = float(np.abs(P - eP)[kept].max() / scale)
    err_row = float((np.abs(P - eP)[3:].max(axis=1) / np.abs(eP)[3:].max(axis=1)).max())
    print("%s [%s]: rel err x %.2e P %.2e blocks %.2e F64-kept %.2e worst landmark row %.2e" % (label, storage, err_x, err_P, err_b, err_kept, err_row))
    if storage == "f64":
        assert err_x < REL and err_P < REL and err_b < REL
    else:
        assert err_x < TOL_X32 and err_kept < TOL_KEPT32 and err_b < TOL_KEPT32 and err_row <= TOL_ROW32
