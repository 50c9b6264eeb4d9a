"""What the extract_map tests share (tests/test_extract_map_cpu.py, tests/test_extract_map_gpu.py): the NumPy restatement of
ekf_extract_map -- the map x -> x', its Jacobian J and P' = J P J' --, the index plans and the scenes.  Nothing of ekf_slam_amd is imported
here: the builders take the engines they drive."""
import numpy as np

from join_map_cases import K, random_spd, random_state, rot, set_state  # noqa: F401  (re-exported: the tests take them from here)

FRAMES = ("map", "robot")


def _sel(idx):
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    ent = np.stack([3 + 2 * idx, 4 + 2 * idx], axis=1).reshape(-1) if idx.size else np.zeros(0, dtype=np.int64)
    return idx, np.concatenate([np.arange(3), ent])


def extract_fn(x, idx, frame):
    """x' of the extraction of landmarks idx (0-based, any order): the selection in the map frame; in the robot frame the zero pose and
    m_k = Rot(theta)' (l_idx[k] - p)."""
    x = np.asarray(x, dtype=np.float64)
    idx, sel = _sel(idx)
    if frame == "map":
        return x[sel].copy()
    assert frame == "robot"
    Rt = rot(x[2]).T
    out = np.zeros(3 + 2 * idx.size)
    for k, l in enumerate(idx):
        out[3 + 2 * k:5 + 2 * k] = Rt @ (x[3 + 2 * l:5 + 2 * l] - x[0:2])
    return out


def extract_blocks(x, l):
    """(m, Hr, Hl) of RELATIVE_XY at (r, landmark l): h, its 2 x 3 block on the robot (heading in degrees) and its 2 x 2 block on l."""
    t = x[2] / K
    c, s = np.cos(t), np.sin(t)
    dx, dy = x[3 + 2 * l] - x[0], x[4 + 2 * l] - x[1]
    m = np.array([c * dx + s * dy, c * dy - s * dx])
    return m, np.array([[-c, -s, m[1] / K], [s, -c, -m[0] / K]]), np.array([[c, s], [-s, c]])


def extract_jacobian(x, idx, frame):
    """J = d extract_fn / d x, (3 + 2 m) x (3 + 2 N): rows of a selection matrix in the map frame; in the robot frame zero robot rows and
    [Hr_k .. Hl at l_idx[k] ..] for landmark k."""
    x = np.asarray(x, dtype=np.float64)
    idx, sel = _sel(idx)
    J = np.zeros((3 + 2 * idx.size, x.size))
    if frame == "map":
        J[np.arange(sel.size), sel] = 1.0
        return J
    assert frame == "robot"
    for k, l in enumerate(idx):
        _, Hr, Hl = extract_blocks(x, l)
        J[3 + 2 * k:5 + 2 * k, 0:3] = Hr
        J[3 + 2 * k:5 + 2 * k, 3 + 2 * l:5 + 2 * l] = Hl
    return J


def extract_dense(x, s, P, idx, frame):
    """(x', s', P') of ekf_extract_map.  The map frame is an indexing (bits kept); the robot frame is J P J', symmetrised."""
    x, s, P = np.asarray(x, dtype=np.float64), np.asarray(s, dtype=np.float64).reshape(-1), np.asarray(P, dtype=np.float64)
    idx, sel = _sel(idx)
    if frame == "map":
        return x[sel].copy(), s[idx].copy(), P[np.ix_(sel, sel)].copy()
    J = extract_jacobian(x, idx, frame)
    Pn = J @ P @ J.T
    return extract_fn(x, idx, frame), s[idx].copy(), 0.5 * (Pn + Pn.T)


# ------------------------------------------------------------------------------------------------------------------
# index plans: each holds landmarks 0 and N - 1 (m >= 2), distinct, a pure function of (N, m, seed)
# ------------------------------------------------------------------------------------------------------------------
def plan_run(N, m, seed=0):
    """ascending: landmark 0, then a run that ends with landmark N - 1"""
    return [0] + list(range(N - (m - 1), N)) if m >= 2 else [0][:m]


def plan_scattered(N, m, seed=0):
    """ascending, scattered over the whole map"""
    if m < 2:
        return [0][:m]
    inner = np.random.default_rng(seed).choice(np.arange(1, N - 1), size=m - 2, replace=False)
    return [int(i) for i in np.sort(np.concatenate([[0, N - 1], inner]))]


def plan_reversed(N, m, seed=0):
    return plan_scattered(N, m, seed)[::-1]


def plan_shuffled(N, m, seed=0):
    asc = plan_scattered(N, m, seed)
    return [asc[i] for i in np.random.default_rng(seed + 1).permutation(len(asc))]


PLANS = {"run": plan_run, "scattered": plan_scattered, "reversed": plan_reversed, "shuffled": plan_shuffled}


def complement(N, idx):
    chosen = set(int(i) for i in idx)
    return [l for l in range(N) if l not in chosen]


# ------------------------------------------------------------------------------------------------------------------
# scenes
# ------------------------------------------------------------------------------------------------------------------
def scene(N, seed):
    """(x, s, P): N landmarks around the robot, a full covariance with robot-landmark correlations, signatures 101 .. 100 + N."""
    rng = np.random.default_rng(seed)
    x, _, P = random_state(rng, N)
    return x, 100.0 + np.arange(1, N + 1, dtype=np.float64), P


def scene_on_robot(N, seed, which=1):
    """scene() with landmark `which` exactly on the robot: regular for the extraction, m = 0 there."""
    x, s, P = scene(N, seed)
    x[3 + 2 * which:5 + 2 * which] = x[0:2]
    return x, s, P
