"""Pure-NumPy side of the landmark-removal tests (ekf_remove_landmarks): what the state must be afterwards, the removal
sets the GPU tests walk through, and the low-rank states they start from.  No GPU, no library."""
import numpy as np


def expected_after(x, s, P, idx):
    """The state after removing landmarks idx (0-based, any order): numpy.delete on x (two entries per landmark), on s and
    on both axes of P.  Marginalising a landmark out of a Gaussian in covariance form is exactly that."""
    x, s, P = np.asarray(x), np.asarray(s), np.asarray(P)
    idx = np.asarray(sorted(int(i) for i in idx), dtype=np.int64)
    N = s.size
    assert x.size == 3 + 2 * N and P.shape == (x.size, x.size)
    assert idx.size == np.unique(idx).size and (idx.size == 0 or (idx[0] >= 0 and idx[-1] < N))
    ent = np.sort(np.concatenate([3 + 2 * idx, 4 + 2 * idx])) if idx.size else np.zeros(0, dtype=np.int64)
    return np.delete(x, ent), np.delete(s, idx), np.delete(np.delete(P, ent, axis=0), ent, axis=1)


def removal_sets(N, T, seed):
    """name -> landmark indices (0-based; handed over UNSORTED where there are several), a pure function of (N, T, seed).
    T is the tile edge in elements: a tile row holds T / 2 landmarks."""
    per_row = T // 2
    assert N > per_row + 2
    edge = per_row * max(1, (N // 2) // per_row)          # first landmark of a tile row near the middle of the map
    width = min(per_row, N - edge)
    sets = {
        "first": [0],
        "last": [N - 1],
        "middle": [N // 2],
        "adjacent_over_tile_edge": [edge - 1, edge],
        "whole_tile_row": list(range(edge, edge + width)),
        "every_second": list(range(0, N, 2)),
        "random_tenth": [int(i) for i in np.random.default_rng(seed).choice(N, size=max(1, N // 10), replace=False)],
        "all": list(range(N)),
    }
    out = {}
    for name, idx in sets.items():
        assert len(set(idx)) == len(idx) and all(0 <= i < N for i in idx), name
        if len(idx) > 1:
            idx = [idx[i] for i in np.random.default_rng(seed + 1).permutation(len(idx))]
        out[name] = [int(i) for i in idx]
    return out


def lowrank_data(N, seed, k=3):
    """x, s, d, U of a state P = diag(d) + U U' (ekf_load_lowrank_state); signatures 1 .. N."""
    rng = np.random.default_rng(seed)
    n = 3 + 2 * N
    x = np.concatenate([[0.1, -0.2, 10.0], rng.uniform(-20, 20, 2 * N)])
    s = np.arange(1, N + 1, dtype=np.float64)
    d = np.concatenate([[0.01, 0.01, 0.001], rng.uniform(0.05, 0.2, 2 * N)])
    U = rng.normal(0.0, 0.02, (n, k))
    return x, s, d, U


def lowrank_minus(x, s, d, U, idx):
    """The same low-rank description without landmarks idx: their rows of U and entries of d, x, s deleted."""
    idx = np.asarray(sorted(int(i) for i in idx), dtype=np.int64)
    ent = np.sort(np.concatenate([3 + 2 * idx, 4 + 2 * idx])) if idx.size else np.zeros(0, dtype=np.int64)
    return np.delete(x, ent), np.delete(s, idx), np.delete(d, ent), np.delete(U, ent, axis=0)


def observe(x, k, dr=0.01, db=0.2):
    """[range, bearing_deg] of landmark k (0-based) seen from the pose in x, slightly off the exact geometry."""
    dx, dy = x[3 + 2 * k] - x[0], x[4 + 2 * k] - x[1]
    b = (np.degrees(np.arctan2(dy, dx)) - x[2]) % 360.0
    return np.array([np.hypot(dx, dy) + dr, b + db])
