"""GPU: the candidate search in front of a merge (ekf_nearest_landmarks; include/ekfslam.h).

Two yardsticks.  (1) The definition: d2[i] IS ekf_landmark_distance(i, partner[i], NULL, R) -- assert_array_equal, in every store.
(2) The NumPy restatement of tests/nearest_cases.py applied to THE STATE THE ENGINE REPORTS (get_x, get_P, get_P_diag_blocks: float
handles start from the same rounded inputs): d2 within REL = 1e-6 (BASELINE.json's bar; the measured error is printed and sits near
1e-14), partner equal on every row -- the restatement's runner-up must be more than 1 + 1e-6 times its minimum on every row,
which each test asserts on the reference before it compares (a seed that violates it is replaced, the band is not widened)."""
import ctypes

import numpy as np
import pytest

from decided_plans import PARAMS
from helpers import R2, REL, RPOS, STORES_ALL, U2, check_state, engine, loaded, status_of
from nearest_cases import PLANTS, fuse_dense, nearest_dense, nearest_lowrank, plant_duplicates
from removal_cases import lowrank_data, observe

pytestmark = pytest.mark.gpu
BAND = 1.0 + 1e-6               # a row whose runner-up lies inside this factor of its minimum has no unambiguous partner
N0 = 300


def planted(seed=5, mode="known", history=(5, 128, 290), **kw):
    """N0 landmarks with the ten planted near-duplicates, and a few corrections so that P is not the loaded one."""
    e = loaded(N0, seed, mode, x=plant_duplicates(lowrank_data(N0, seed)[0]), **kw)
    for k in history:
        e.predict(U2); e.correct(observe(e.get_x(), k), R2, k)
    return e


def reference(e, R):
    return nearest_dense(e.get_x(), e.get_P(), R, e.get_P_diag_blocks()[1:])


def check_against_numpy(e, R, label):
    """d2 within REL, partner equal on every row; the precondition on the reference first."""
    want_d2, want_p, ratio = reference(e, R)
    assert (ratio > BAND).all(), "%s: the reference has an ambiguous row (runner-up ratio %.9f): pick another seed" % (label, ratio.min())
    d2, partner = e.nearest_landmarks(R)
    assert d2.shape == (e.N,) and partner.shape == (e.N,) and partner.dtype == np.int64
    assert not np.isnan(d2).any()
    has = want_p >= 0
    err = float(np.abs(d2[has] / want_d2[has] - 1.0).max()) if has.any() else 0.0
    print("%s: N %d, rel err d2 %.2e, smallest runner-up ratio %.6f, smallest d2 %.4g" % (label, e.N, err, ratio.min(), want_d2.min()))
    np.testing.assert_array_equal(partner, want_p)
    assert err < REL
    assert np.isinf(d2[~has]).all() and (d2[~has] > 0).all()
    return d2, partner


# ------------------------------------------------------------------------------------------------------------------
# 1. hand-checked states
# ------------------------------------------------------------------------------------------------------------------
def known_answer_state():
    """tests/test_merge_landmarks_cpu.py::_known_answer_state and a third uncorrelated landmark at (0, 1) with block diag(1, 1)."""
    x = np.array([0.5, -0.25, 30.0, 0.0, 0.0, 4.0, 2.0, 0.0, 1.0])
    P = np.diag([0.125, 0.125, 0.015625, 3.0, 1.0, 1.0, 1.0, 1.0, 1.0])
    return x, np.array([1.0, 2.0, 3.0]), P


def mirrored_state():
    """Landmarks 0 and 1 mirror images of each other about landmark 2: d2(2, 0) == d2(2, 1) == 16 / 2 exactly."""
    x = np.array([0.5, -0.25, 30.0, -4.0, 0.0, 4.0, 0.0, 0.0, 0.0])
    P = np.diag([0.125, 0.125, 0.015625, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0])
    return x, np.array([1.0, 2.0, 3.0]), P


@pytest.mark.parametrize("tile,storage", STORES_ALL)
def test_hand_checked_answers(tile, storage):
    e = engine(capacity=8, tile=tile, storage=storage)
    e.set_state(*[known_answer_state()[k] for k in (0, 2, 1)])
    d2, partner = e.nearest_landmarks()
    assert partner.tolist() == [-1, 0, 0]
    assert d2.tolist() == [np.inf, 6.0, 0.5]                 # 16/4 + 4/2;  min(0 + 1/2, 16/2 + 1/2)
    assert e.landmark_distance(2, 1)[0] == 8.5
    e.set_state(*[mirrored_state()[k] for k in (0, 2, 1)])
    d2, partner = e.nearest_landmarks()
    assert partner.tolist() == [-1, 0, 0]                    # the tie goes to the lower index
    assert d2.tolist() == [np.inf, 32.0, 8.0]
    assert e.landmark_distance(2, 0)[0] == e.landmark_distance(2, 1)[0] == 8.0
    # R enters S: diag(2, 2) + diag(2, 6) -> 16/4
    d2, partner = e.nearest_landmarks(np.diag([2.0, 6.0]))
    assert d2.tolist() == [np.inf, 16.0, 4.0] and partner.tolist() == [-1, 0, 0]
    empty = engine(capacity=8, tile=tile, storage=storage)
    d2, partner = empty.nearest_landmarks()
    assert d2.size == 0 and partner.size == 0
    assert empty.lib.ekf_nearest_landmarks(empty.h, None, None, None) == 0       # N == 0: nothing written, nothing needed


# ------------------------------------------------------------------------------------------------------------------
# 2. against NumPy, 3. the definition bit for bit, 4. changes nothing
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage", STORES_ALL)
@pytest.mark.parametrize("R", [RPOS, None], ids=["Rpos", "R0"])
def test_against_numpy_with_planted_duplicates(tile, storage, R):
    e = planted(capacity=N0 + 8, tile=tile, storage=storage, batch=8)
    d2, partner = check_against_numpy(e, R, "planted [%d %s]" % (tile, storage))
    for keep, drop in PLANTS:                                # every planted duplicate found its original
        assert partner[drop] == keep and d2[drop] < 0.1


@pytest.mark.parametrize("tile,storage", STORES_ALL)
@pytest.mark.parametrize("R", [RPOS, None], ids=["Rpos", "R0"])
def test_every_value_is_the_landmark_distance_of_its_pair_bit_for_bit(tile, storage, R):
    e = planted(capacity=N0 + 8, tile=tile, storage=storage, batch=8)
    d2, partner = e.nearest_landmarks(R)
    assert partner[0] == -1 and (partner[1:] >= 0).all() and (partner < np.arange(N0)).all()
    want = np.array([e.landmark_distance(i, int(partner[i]), None, R)[0] for i in range(1, N0)])
    np.testing.assert_array_equal(d2[1:], want)
    # ... and no EARLIER landmark is strictly closer (a sample of rows, all their columns)
    for i in (1, 2, 17, 128, 129, 257, N0 - 1):
        row = np.array([e.landmark_distance(i, j, None, R)[0] for j in range(i)])
        assert d2[i] == row.min() and partner[i] == int(np.argmin(row))


@pytest.mark.parametrize("tile,storage", STORES_ALL)
def test_the_search_changes_nothing(tile, storage):
    e = planted(capacity=N0 + 8, tile=tile, storage=storage, batch=8)
    x0, s0, P0, b0, dg0 = e.get_x(), e.get_s(), e.get_P(), e.get_P_diag_blocks(), e.digest()
    first = e.nearest_landmarks(RPOS)
    again = e.nearest_landmarks(RPOS)
    np.testing.assert_array_equal(first[0], again[0])
    np.testing.assert_array_equal(first[1], again[1])
    assert e.pending() == 0 and e.N == N0
    np.testing.assert_array_equal(e.get_x(), x0)
    np.testing.assert_array_equal(e.get_s(), s0)
    np.testing.assert_array_equal(e.get_P(), P0)
    np.testing.assert_array_equal(e.get_P_diag_blocks(), b0)
    np.testing.assert_array_equal(e.digest(), dg0)


# ------------------------------------------------------------------------------------------------------------------
# 5. ordering with the engine
# ------------------------------------------------------------------------------------------------------------------
def test_pending_pairs_and_a_lazy_predict_are_carried_out_first():
    x = plant_duplicates(lowrank_data(N0, 5)[0])
    runs = []
    for batch in (8, 1):
        e = loaded(N0, 5, x=x, capacity=N0 + 8, tile=64, batch=batch)
        for k in (7, 150, 151, 299, 42):
            e.predict(U2); e.correct(observe(x, k), R2, k)
        assert e.pending() == (5 if batch == 8 else 0)
        e.predict(np.array([0.2, -2.0]))
        runs.append(e.nearest_landmarks(RPOS))
        assert e.pending() == 0
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    np.testing.assert_array_equal(runs[0][1], runs[1][1])


def test_right_after_queued_scans_on_a_device_decided_asynchronous_handle():
    cap = N0 + 40
    x = plant_duplicates(lowrank_data(N0, 3)[0])
    lm_index = np.arange(1, cap + 1, dtype=np.float64)
    lm_loc = np.random.default_rng(5).uniform(-20, 20, (cap, 2))
    runs = []
    for kw in (dict(device_assoc=4, async_flush=True), dict(device_assoc=1)):
        e = loaded(N0, 3, "uc", x=x, capacity=cap, tile=64, batch=8, **kw, **PARAMS)
        for t in range(2):                                   # two scans that correct and append; with device_assoc = 4 nothing is settled
            e.predict(U2)
            x0 = e.get_x()                                   # (the pose the scan is taken from: the position cost is strict)
            rows = np.array([list(observe(x0, 9 + t)) + [10.0 + t], [3.0 + t, 45.0, 7e6 + t], [4.0, 50.0 + 9 * t, 8e6 + t],
                             list(observe(x0, 250 - t)) + [251.0 - t]])
            e.measure(rows, U2, lm_index, lm_loc)
        got = e.nearest_landmarks(RPOS)                      # the last scan's rows are still queued when this arrives
        runs.append((got, e.N))
    (a, Na), (b, Nb) = runs
    assert Na == Nb == N0 + 4 and a[0].size == Na
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------------------------
# 6. a map that changed shape
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage", STORES_ALL)
def test_after_appends_a_removal_and_a_merge(tile, storage):
    per_row = tile // 2
    cap = N0 + per_row + 16
    e = planted(mode="uc", capacity=cap, tile=tile, storage=storage, batch=8)
    rng = np.random.default_rng(2)
    n_app = per_row - N0 % per_row + 3                       # across the next tile-row edge
    for i in range(n_app):
        e.predict(U2); e.append(U2, R2, rng.uniform(-20, 20, 2), 5000.0 + i)
    assert e.N % per_row == 3
    d2, partner = check_against_numpy(e, RPOS, "after %d appends [%d %s]" % (n_app, tile, storage))
    assert (partner[N0:] >= 0).all()
    e.remove_landmarks([0, 31, 127, 128, e.N - 1])
    assert e.N % per_row != 0
    d2, partner = check_against_numpy(e, RPOS, "after a removal [%d %s]" % (tile, storage))
    assert partner[62] == 61                                 # the planted pair (63, 64), two places down
    e.merge_landmarks(61, 62, RPOS)
    assert e.N % per_row != 0
    check_against_numpy(e, None, "after a merge [%d %s]" % (tile, storage))
    # a map shrunk below one group of rows and one tile
    e.remove_landmarks(list(range(3, e.N)))
    check_against_numpy(e, RPOS, "three landmarks left [%d %s]" % (tile, storage))


# ------------------------------------------------------------------------------------------------------------------
# 7. an irregular pair never wins
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage", STORES_ALL)
def test_two_identical_perfectly_correlated_landmarks(tile, storage):
    """S = 0 exactly (every value is representable in float): the pair is skipped."""
    x = np.array([0.5, -0.25, 30.0, 2.0, 1.0, 2.0, 1.0])
    P = np.diag([0.125, 0.125, 0.015625, 1.0, 0.5, 1.0, 0.5])
    P[3:5, 5:7] = P[5:7, 3:5] = np.diag([1.0, 0.5])
    e = engine(capacity=8, tile=tile, storage=storage)
    e.set_state(x, P, np.array([1.0, 2.0]))
    assert np.isnan(e.landmark_distance(1, 0)[0])
    d2, partner = e.nearest_landmarks()
    assert partner.tolist() == [-1, -1] and np.isinf(d2).all() and (d2 > 0).all()
    # a third landmark: its own row is regular; and with a twin of landmark 0 BEHIND it, the twin's row reports its next-best
    x3 = np.array([0.5, -0.25, 30.0, 2.0, 1.0, 0.0, 1.0, 2.0, 1.0])
    P3 = np.diag([0.125, 0.125, 0.015625, 1.0, 0.5, 1.0, 1.0, 1.0, 0.5])
    P3[3:5, 7:9] = P3[7:9, 3:5] = np.diag([1.0, 0.5])
    e.set_state(x3, P3, np.array([1.0, 2.0, 3.0]))
    assert np.isnan(e.landmark_distance(2, 0)[0])
    d2, partner = e.nearest_landmarks()
    assert partner.tolist() == [-1, 0, 1] and d2.tolist() == [np.inf, 2.0, 2.0]      # 4 / 2 both times
    assert not np.isnan(d2).any()
    # R > 0 makes the pair regular again: nu = 0 -> d2 = 0, the closest there is
    d2, partner = e.nearest_landmarks(np.diag([1.0, 1.0]))
    assert partner.tolist() == [-1, 0, 0] and d2[2] == 0.0


def test_an_irregular_pair_inside_a_large_map():
    e = loaded(N0, 5, capacity=N0 + 8, tile=64, batch=8)
    x, s, P = e.get_x(), e.get_s(), e.get_P()
    a, b = 3 + 2 * 10, 3 + 2 * 200
    x[b:b + 2] = x[a:a + 2]
    P[b:b + 2, :] = P[a:a + 2, :]
    P[:, b:b + 2] = P[:, a:a + 2]
    P[b:b + 2, b:b + 2] = P[a:a + 2, a:a + 2]
    e.set_state(x, P, s)
    assert np.isnan(e.landmark_distance(200, 10)[0])
    d2, partner = check_against_numpy(e, None, "irregular pair (200, 10)")
    assert partner[200] not in (-1, 10) and np.isfinite(d2[200])
    assert e.nearest_landmarks(RPOS)[1][200] == 10           # regular with R > 0, and then the nearest: nu = 0


# ------------------------------------------------------------------------------------------------------------------
# 8. refusals; a lone shard
# ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_state_alone():
    from ekf_slam_amd import _lib as L
    e = planted(capacity=N0 + 8, tile=64, batch=8, history=())
    x = e.get_x()
    for k in (4, 77, 200):
        e.predict(U2); e.correct(observe(x, k), R2, k)
    assert e.pending() == 3
    dg, x_before = e.digest(), e.get_x()
    dp = lambda *v: (ctypes.c_double * len(v))(*v)
    d2 = (ctypes.c_double * N0)()
    pa = (ctypes.c_int64 * N0)()
    inf = float("inf")
    ok_R = dp(0.02, 0.005, 0.005, 0.03)
    assert e.lib.ekf_nearest_landmarks(None, ok_R, d2, pa) == L.EKF_ERR_INVALID_ARG
    cases = [("null d2", ok_R, None, pa), ("null partner", ok_R, d2, None), ("inf R", dp(inf, 0.0, 0.0, 1.0), d2, pa),
             ("asymmetric R", dp(1.0, 0.1, 0.2, 1.0), d2, pa), ("negative diagonal", dp(-1.0, 0.0, 0.0, 1.0), d2, pa),
             ("negative determinant", dp(1.0, 2.0, 2.0, 1.0), d2, pa)]
    for name, R, a, b in cases:
        assert e.lib.ekf_nearest_landmarks(e.h, R, a, b) == L.EKF_ERR_INVALID_ARG, name
        assert b"nearest_landmarks" in e.lib.ekf_last_error(e.h), name
        np.testing.assert_array_equal(e.digest(), dg)
        np.testing.assert_array_equal(e.get_x(), x_before)
    assert e.lib.ekf_nearest_landmarks(e.h, ok_R, d2, pa) == 0
    # sharded handles: refused, and the message says why
    sh = engine(capacity=64, tile=16, world=2, rank=0)
    st, msg = status_of(lambda: sh.nearest_landmarks())
    assert st == L.EKF_ERR_INVALID_ARG and "shard" in msg


def test_a_lone_shard_works_and_refuses_between_begin_and_finish():
    from ekf_slam_amd import _lib as L
    x = plant_duplicates(lowrank_data(N0, 5)[0])
    e = loaded(N0, 5, x=x, capacity=N0 + 8, tile=64, force_sharded=1)
    twin = loaded(N0, 5, x=x, capacity=N0 + 8, tile=64)
    harr = (ctypes.c_void_p * 1)(e.h)
    for k in (3, 30, 269):
        z = observe(twin.get_x(), k)
        e.predict(U2); twin.predict(U2)
        e.correct_begin(z, R2, k)
        st, msg = status_of(lambda: e.nearest_landmarks(RPOS))
        assert st == L.EKF_ERR_STATE and "begin and finish" in msg
        assert e.lib.ekf_exchange_local(harr, 1) == 0
        e.correct_finish()
        twin.correct(z, R2, k)
    a, b = e.nearest_landmarks(RPOS), twin.nearest_landmarks(RPOS)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    assert (a[1][[drop for _, drop in PLANTS]] == [keep for keep, _ in PLANTS]).all()


# ------------------------------------------------------------------------------------------------------------------
# 9. fuse_duplicates on a handle
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage", [(16, "f64"), (128, "f64"), (256, "f32"), (256, "f32_mixed")])
def test_fuse_duplicates_makes_the_merges_of_the_numpy_mirror(tile, storage):
    from ekf_slam_amd.slam import EKF_SLAM_UC
    f = EKF_SLAM_UC(capacity=N0 + 8, tile=tile, storage=storage, batch=8)
    x0, s0, d, U = lowrank_data(N0, 5)
    # (the duplicates planted at 0.4 of the module's offsets: seed 5 has a natural pair at d2 = 0.053, and the gate needs a gap)
    f._e.load_lowrank_state(plant_duplicates(x0, scale=0.4), s0, d, U)
    for k in (5, 128, 290):
        f._e.predict(U2); f._e.correct(observe(f._e.get_x(), k), R2, k)
    x, s, P = f.x, f.s, f.P
    minima = np.sort(nearest_dense(x, P, RPOS)[0][1:])
    lo, hi = minima[len(PLANTS) - 1], minima[len(PLANTS)]
    assert hi >= 2.0 * lo, "no gap behind the planted duplicates: %.4g, %.4g" % (lo, hi)
    gate = float(np.sqrt(lo * hi))
    mx, ms, mP, want = fuse_dense(x, s, P, gate, RPOS)
    assert len(want) == len(PLANTS)
    cand = f.duplicate_candidates(gate, RPOS)
    assert sorted((i, j) for i, j, _ in cand) == sorted((drop + 1, keep + 1) for keep, drop in PLANTS)
    assert [c[2] for c in cand] == sorted(c[2] for c in cand)
    merges = f.fuse_duplicates(gate, RPOS)
    assert [(k, dr) for k, dr, _ in merges] == [(k + 1, dr + 1) for k, dr, _ in want]          # 1-based at this layer
    err = max(abs(a[2] / b[2] - 1.0) for a, b in zip(merges, want))
    print("fuse [%d %s]: %d merges, gate %.4g in the gap (%.4g, %.4g), rel err of the d2 %.2e" % (tile, storage, len(merges), gate, lo, hi, err))
    assert err < (REL if storage == "f64" else 1e-5)
    assert f._e.N == N0 - len(PLANTS) and f.duplicate_candidates(gate, RPOS) == []
    check_state(f._e, mx, mP, storage, "after %d fusions" % len(merges), es=ms)
    # max_merges stops the loop
    g = EKF_SLAM_UC(capacity=N0 + 8, tile=tile, storage=storage, batch=8)
    g._e.set_state(x, P, s)
    two = g.fuse_duplicates(gate, RPOS, max_merges=2)
    assert [(k, dr) for k, dr, _ in two] == [(k, dr) for k, dr, _ in merges[:2]] and g._e.N == N0 - 2


# ------------------------------------------------------------------------------------------------------------------
# 10. at size
# ------------------------------------------------------------------------------------------------------------------
def _at_size(N, seed, storage, rows, **kw):
    """The reference comes from the low-rank description diag(d) + U U', evaluated block-wise (cross entries rounded to float where
    the store is float)."""
    x, s, d, U = lowrank_data(N, seed)
    per_row = kw["tile"] // 2
    pairs = [(0, per_row), (per_row - 1, per_row + 1), (N // 2, N - 1), (7, N - 2), (3 * per_row, 5 * per_row - 1)]
    x = plant_duplicates(x, pairs)
    e = engine(capacity=N, storage=storage, **kw)
    e.load_lowrank_state(x, s, d, U)
    rows = np.arange(N) if rows is None else np.unique(np.asarray(rows))
    want_d2, want_p, ratio = nearest_lowrank(x, d, U, rows, RPOS, np.float64 if storage == "f64" else np.float32)
    assert (ratio > BAND).all(), "the reference has an ambiguous row (runner-up ratio %.9f): pick another seed" % ratio.min()
    d2, partner = e.nearest_landmarks(RPOS)
    assert d2.size == N and not np.isnan(d2).any()
    has = want_p >= 0
    err = float(np.abs(d2[rows][has] / want_d2[has] - 1.0).max())
    print("at size N = %d [%s]: %d rows, rel err d2 %.2e, smallest runner-up ratio %.7f" % (N, storage, rows.size, err, ratio.min()))
    np.testing.assert_array_equal(partner[rows], want_p)
    assert err < REL
    for keep, drop in pairs:
        assert partner[drop] == keep
    assert partner[0] == -1 and np.isinf(d2[0])
    # the definition, on a sample
    for i in [int(r) for r in rows[-3:]] + [drop for _, drop in pairs]:
        assert d2[i] == e.landmark_distance(i, int(partner[i]), None, RPOS)[0]
    e.close()


def test_at_size_ten_thousand_landmarks_f64_all_rows():
    _at_size(10000, 24, "f64", None, tile=128)


def test_at_size_forty_thousand_landmarks_float_tiles_sampled_rows():
    N, per_row = 40000, 128
    edges = [per_row * k for k in (1, 2, 77, 156, 310, 311)]
    rows = [0, 1, 2, N - 1, N - 2] + edges + [r - 1 for r in edges] + [r + per_row - 1 for r in edges]
    rows += [int(r) for r in np.random.default_rng(8).choice(N, 256, replace=False)]
    rows += [drop for drop in (per_row, per_row + 1, N - 1, N - 2, 5 * per_row - 1)]
    _at_size(N, 22, "f32", rows, tile=256)
