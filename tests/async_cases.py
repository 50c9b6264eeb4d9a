"""What the tests of the asynchronous pass at size share (tests/test_async_growth_gpu.py, tests/test_beside_pass_gpu.py): the inputs of a
~20 000-landmark state, where one pass over P lasts longer than a step, the placement of tile-row crossings behind batch boundaries, the
rows sampled from every tile row -- read from the factored oracle (oracle/ekf_factored.py) and from an engine or the shards of a group --
and the sensitivity of those rows to the batches a skipped tile would lack.  No GPU is touched when this module is imported."""
import numpy as np

SEED = 20260101 + 5
# Inputs: P = diag(d) + U U' (d ~ U(0.01, 0.1)), U ~ N(0, sigma) in the landmark rows and N(0, sigma_robot) in the robot rows, range /
# bearing variance factors RC.  The correlations must be strong enough that two batches move every tile of the sampled rows well beyond
# the row tolerance; float tiles keep U as small as that allows, since the float rounding of the rows each correction reads reaches x
# and the F64-kept parts in proportion.  The bearing factor (0.5 instead of configs[4]'s 5) keeps the appended landmarks' own blocks, the
# largest entries and so the scale of the row tolerance, near 2.
INPUTS = {"f64": (0.1, 0.1, (.01, .5)), "float": (0.04, 0.04, (.01, .5)), "float_b": (0.03, 0.03, (.01, .5))}


def placement(T, batch):
    """(N0, steps): ~20 000 landmarks; the first crossing 2 steps after the second batch boundary, two more every T / 2 appends after it
    (the batch divides T / 2, so they all land at the same place behind a boundary)"""
    half = T // 2
    assert half % batch == 0
    first = 2 * batch + 1
    N0 = (20000 + first) // half * half - first
    return N0, first + 3 * half + 4


def crossings(N0, steps, T, batch):
    """steps t whose append makes ceil(2N / T) grow (N0 + t landmarks before it, a multiple of T / 2), and those of them that fall 1-4
    steps after a batch boundary other than the first (boundary: the correction of step kB - 1 completes batch k)"""
    cross = [t for t in range(steps) if (N0 + t) % (T // 2) == 0 and N0 + t > 0]
    counted = [t for t in cross if 1 <= (t + 1) % batch <= 4 and (t + 1) // batch >= 2]
    return cross, counted


def make_inputs(N0, steps, sigma, sigma_robot, RC):
    from ekf_slam_amd.world import World
    cap = N0 + steps
    w = World(cap, SEED)
    rng = np.random.default_rng(77)
    n0 = 3 + 2 * N0
    x = np.concatenate([[0.0, 0.0, 0.0], w.landmarks[:N0].reshape(-1)])
    d = rng.uniform(0.01, 0.1, n0)
    U = rng.normal(0.0, sigma, (n0, 8))
    U[:3] = rng.normal(0.0, sigma_robot, (3, 8))
    s = np.arange(1, N0 + 1.0)
    plan = []
    for t in range(steps):
        u = w.step()
        k = (t * 37) % N0 if t % 7 else N0 + (t * 5) % (t + 1)     # every 7th step: a landmark appended on the way (incl. the newest)
        (_, r, b), = w.observe([k])
        R = np.diag([r * RC[0], b * RC[1]])
        plan.append((u, R, w.landmarks[N0 + t].copy(), float(N0 + t + 1), np.array([r, b]), k))
    return (x, s, d, U), plan


def sampled_landmarks(N, T):
    """one landmark per tile row of the landmark block (its two rows lie in tile row 2L // T), spread over the rows' positions"""
    nt = -(-2 * N // T)
    half = T // 2
    return [min(I * half + (I * 37) % half, N - 1) for I in range(nt)]


def oracle_rows(ref, lms):
    """P(3 + 2L : 5 + 2L, :) of the factored oracle for every landmark L of lms: (len(lms), 2, n), the correction terms in one product"""
    m = ref.m
    js = np.array([2 * L for L in lms])
    base = np.stack([ref._base_rows(int(j)) for j in js])          # (k, 2, m)
    if ref.nt:
        Lm, Rm = ref._terms()
        rows = np.concatenate([js, js + 1])
        upd = Lm[rows, :2 * ref.nt] @ Rm[:2 * ref.nt, :m]
        base[:, 0] += upd[:len(js)]
        base[:, 1] += upd[len(js):]
    strip = np.stack([ref.Pmr[j:j + 2] for j in js])                # (k, 2, 3)
    return np.concatenate([strip, base], axis=2)


def tile_change_margin(before, after, lms, N_before, T, tol_abs):
    """smallest over the sampled rows q and over every tile column range J of (largest change in those columns) / tol_abs[q]"""
    m = 2 * N_before
    worst = np.inf
    for q, L in enumerate(lms):
        if L >= N_before:
            continue
        dlt = np.abs(after[q][:, 3:3 + m] - before[q][:, 3:3 + m])
        for J in range(-(-m // T)):
            worst = min(worst, float(dlt[:, J * T:min(m, (J + 1) * T)].max()) / tol_abs[q])
    return worst


def engine_rows(eng, lms, n):
    """the same rows read from an engine, or merged from the shards of a group (NaN where a shard does not hold a tile)"""
    out = []
    for L in lms:
        if hasattr(eng, "shards"):
            merged = np.full((2, n), np.nan)
            for e in eng.shards:
                b = e.get_P_block(3 + 2 * L, 0, 2, n)
                hole = np.isnan(merged)
                merged[hole] = b[hole]
            assert not np.isnan(merged).any()
            out.append(merged)
        else:
            out.append(eng.get_P_block(3 + 2 * L, 0, 2, n))
    return np.stack(out)
