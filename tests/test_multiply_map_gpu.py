"""GPU: the plain product P B on the device (ekf_multiply_map; include/ekfslam.h).

The yardstick is NumPy on THE MATRIX A TWIN REPORTS: twin.get_P() of a twin with the same history (pending pairs, a recorded predict,
removals).  THE BAR is multiply_map_cases' derived one, entry by entry: |got - P b|_i <= 2 n 2^-53 (|P| |b|)_i; bar_ratio is the worst
quotient of the two sides, printed before it is asserted to be at most 1.

The stores are solve_map_cases.STORES: tile edges 16, 64, 128 and 256, F64 and float tiles; N = 140 leaves the last tile row partial at
every edge but 16 and gives edge 16 tile rows of two segments, N = 96 at edge 64 ends exactly on a tile edge, N = 1 and N = 0 are the
smallest maps."""
import ctypes

import numpy as np
import pytest

import multiply_map_cases as M
import solve_map_cases as V
from helpers import R2, RPOS, U2, assert_same, engine, getters, loaded, status_of
from removal_cases import lowrank_data, observe

pytestmark = pytest.mark.gpu
CHUNK = M.CHUNK


def sources(count, pending=3, n=140, **kw):
    """`count` engines with the same state and history: `pending` corrections left in the ring where the batch allows it and a
    recorded predict behind them."""
    x = lowrank_data(n, 5)[0]
    kw.setdefault("batch", 8)
    out = [loaded(n, 5, capacity=n + 4, **kw) for _ in range(count)]
    for q in out:
        for k in [(5 * j + 1) % n for j in range(pending)]:
            q.predict(U2); q.correct(observe(x, k), R2, k)
        q.predict(U2)
    return out


def vectors(n, seed=1):
    """The unit vectors of 19 spread indices and 3 Gaussian rows: two chunks."""
    return np.vstack([np.eye(n)[M.spread_units(n)], M.gaussian_rows(3, n, seed)])


def within_the_bar(e, P, label, B=None):
    B = vectors(P.shape[0]) if B is None else B
    got = e.multiply_map(B)
    assert got.shape == B.shape and got.dtype == np.float64
    ratio = M.bar_ratio(P, B, got)
    print("%s: worst |got - P b| / (2 n u |P||b|) = %.3f" % (label, ratio))
    assert ratio <= 1.0, (label, ratio)
    return got


# ------------------------------------------------------------------------------------------------------------------
# 1. against NumPy on the twin's P
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage,n", V.STORES)
def test_products_against_numpy_on_the_twins_matrix(tile, storage, n):
    e, twin = sources(2, 3, n, tile=tile, storage=storage)
    assert e.pending() == 3
    P = twin.get_P()                                          # (flushes the twin)
    within_the_bar(e, P, "N=%d T=%d %s" % (n, tile, storage))
    assert e.pending() == 0 and e.N == n


def test_a_map_that_ends_exactly_on_a_tile_edge():
    e, twin = sources(2, 3, 96, tile=64)                      # 192 rows: exactly three tiles of 64
    within_the_bar(e, twin.get_P(), "N=96 T=64")


def test_one_landmark_and_none():
    e, twin = sources(2, 1, 1, tile=16)
    within_the_bar(e, twin.get_P(), "N=1")
    g = engine(capacity=8, tile=16)
    P0 = np.array([[0.5, 0.1, -0.05], [0.1, 0.4, 0.02], [-0.05, 0.02, 0.3]])
    g.set_x(np.array([1.0, -2.0, 40.0])); g.set_P(P0)
    B = np.vstack([np.eye(3), [[0.3, -1.0, 2.0]]])
    got = within_the_bar(g, P0, "N=0, an SPD Prr", B)         # out = Prr b
    np.testing.assert_array_equal(got[:3], P0)


# ------------------------------------------------------------------------------------------------------------------
# 2. rows that removals left behind below the map
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage", [(16, "f64"), (64, "f64"), (256, "f32")])
def test_after_removals_the_rows_left_behind_do_not_count(tile, storage):
    e, twin = sources(2, 3, 140, tile=tile, storage=storage)
    for q in (e, twin):
        q.remove_landmarks(range(110, 140))
        q.remove_landmarks(range(50, 60))
    assert e.N == 100
    within_the_bar(e, twin.get_P(), "N=140 less 30 less 10, T=%d %s" % (tile, storage))


# ------------------------------------------------------------------------------------------------------------------
# 3. the promised bits
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage", [(16, "f64"), (256, "f32")])
def test_a_row_depends_on_its_own_vector_alone(tile, storage):
    n = 140
    e, twin = sources(2, 3, n, tile=tile, storage=storage)
    nx = 3 + 2 * n
    G = M.batch_rows(nx)                                      # 3 * 16 + 5 rows: four chunks, the last partial; row 2 is zero
    whole = e.multiply_map(G)
    assert e.pending() == 0
    zero = e.multiply_map(np.zeros((2, nx)))
    assert zero.shape == (2, nx) and not zero.any() and not whole[2].any()             # B = 0 gives 0 in every entry
    np.testing.assert_array_equal(e.multiply_map(G[0])[0], whole[0])                 # alone
    for i in M.REPEATS:
        np.testing.assert_array_equal(whole[i], whole[0])     # behind a chunk boundary, first in a chunk, last of a partial chunk
    for k in (CHUNK, CHUNK + 1):
        np.testing.assert_array_equal(e.multiply_map(G[:k]), whole[:k])
    np.testing.assert_array_equal(e.multiply_map(G[2 * CHUNK + 1:]), whole[2 * CHUNK + 1:])           # another position in its chunk
    np.testing.assert_array_equal(e.multiply_map(np.vstack([G] * 2))[G.shape[0]:], whole)            # more than the pinned slots hold
    np.testing.assert_array_equal(e.multiply_map(G), whole)   # from call to call
    ratio = M.bar_ratio(twin.get_P(), G, whole)
    print("N=140 T=%d %s, %d Gaussian rows: %.3f of the bar" % (tile, storage, G.shape[0], ratio))
    assert ratio <= 1.0


@pytest.mark.parametrize("tile,storage,n", V.STORES)
def test_unit_vectors_return_the_columns_of_get_P(tile, storage, n):
    e, twin = sources(2, 3, n, tile=tile, storage=storage)
    P = twin.get_P()
    idx = M.spread_units(P.shape[0])
    assert idx.size == 19 and idx[0] == 0 and idx[-1] == P.shape[0] - 1
    np.testing.assert_array_equal(e.multiply_map(np.eye(P.shape[0])[idx]), P[:, idx].T)
    np.testing.assert_array_equal(P, e.get_P())


# ------------------------------------------------------------------------------------------------------------------
# 4. the call changes nothing
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage", [(16, "f64"), (256, "f32_mixed")])
def test_the_call_changes_nothing(tile, storage):
    n = 140
    e, twin = sources(2, 3, n, tile=tile, storage=storage, batch=4)
    before = e.device_bytes()
    G = M.gaussian_rows(CHUNK + 1, 3 + 2 * n, 2)
    e.multiply_map(G[0])
    held = e.device_bytes()
    rows = -(-2 * n // tile) * tile
    assert held >= before + 8 * 2 * CHUNK * rows              # a chunk in and a chunk out at the least
    # ... and no factor store: factor_map's alone is rows_64 (rows_64 + 64) / 2 doubles, far more than this call's scratch at edge 256
    e.multiply_map(np.vstack([G] * 5))                        # more vectors: the same scratch
    assert e.device_bytes() == held and e.pending() == 0
    assert held - before == scratch_of_a_fresh_handle(n, tile, storage)          # the same bytes on a handle that never called anything else
    twin.flush()
    for got, ref in zip(getters(e), getters(twin)):           # x, s, P, the diagonal blocks and the digest of a twin that only flushed
        np.testing.assert_array_equal(got, ref)
    x1 = e.get_x()
    for q in (e, twin):
        for k in (3, 9, 70, 139, 3):
            q.predict(U2); q.correct(observe(x1, k), R2, k)
        q.flush()
    assert_same(e, twin)


def scratch_of_a_fresh_handle(n, tile, storage):
    """What a first multiply_map adds to device_bytes() of a third handle of the same shape -- and that factor_map, called
    afterwards, adds its own store on top (so the product's scratch held none)."""
    other = loaded(n, 5, capacity=n + 4, tile=tile, storage=storage)
    b0 = other.device_bytes()
    other.multiply_map(np.zeros(3 + 2 * other.N))
    b1 = other.device_bytes()
    other.factor_map()
    rows64 = -(-2 * other.N // 64) * 64
    assert other.device_bytes() - b1 >= 8 * rows64 * (rows64 + 64) // 2             # the factor store is allocated only now
    return b1 - b0


# ------------------------------------------------------------------------------------------------------------------
# 5. cross-checks inside the library
# ------------------------------------------------------------------------------------------------------------------
def test_policies_against_the_librarys_own_innovation_and_solve():
    from ekf_slam_amd.slam import EKF_SLAM
    n = 40
    f = EKF_SLAM(capacity=n + 4, tile=16)
    f._e.load_lowrank_state(*lowrank_data(n, 5))
    P = f._e.get_P()
    nx = P.shape[0]
    # a two-landmark fix: z = Hr x_r + H_a l_a + H_b l_b
    Hr = np.array([[0.3, -0.2, 0.01], [0.1, 0.5, -0.02]])
    Ha, Hb = np.array([[1.0, 0.2], [-0.3, 0.9]]), np.array([[-1.0, 0.1], [0.25, -0.8]])
    la, lb = 7, 31                                            # 0-based
    H = np.zeros((2, nx))
    H[:, :3], H[:, 3 + 2 * la:5 + 2 * la], H[:, 3 + 2 * lb:5 + 2 * lb] = Hr, Ha, Hb
    got = f.covariance_of(H) + RPOS
    S = np.asarray(f.linear_innovation([0.0, 0.0], RPOS, Hr, [la + 1, lb + 1], [Ha, Hb])["S"], dtype=np.float64).reshape(2, 2)
    bound = 64.0 * M.U * (np.abs(H) @ np.abs(P) @ np.abs(H).T + np.abs(RPOS))
    print("covariance_of(H) + R against linear_innovation's S: worst %.3f of 64 u (|H||P||H|' + |R|)" % (np.abs(got - S) / bound).max())
    assert np.all(np.abs(got - S) <= bound)
    np.testing.assert_array_equal(got, got.T)
    # the cross-covariance of two arbitrary groups, and of a group with the robot: the entries of get_P themselves
    ia, ib = [5, 39, 0], [12, 3]
    ca = np.array([3 + 2 * i + r for i in ia for r in (0, 1)])
    cb = np.array([3 + 2 * i + r for i in ib for r in (0, 1)])
    np.testing.assert_array_equal(f.cross_covariance(ia, ib), P[np.ix_(ca, cb)])
    np.testing.assert_array_equal(f.cross_covariance(ib, ia), P[np.ix_(cb, ca)])
    np.testing.assert_array_equal(f.cross_covariance(None, ia), P[np.ix_(np.arange(3), ca)])
    np.testing.assert_array_equal(f.cross_covariance(ia, None), P[np.ix_(ca, np.arange(3))])
    # the residual of a solve: P z - b within the product bar on z
    B = M.gaussian_rows(CHUNK + 2, nx, 9)
    z, r = f.solve_residual(B)
    want = z @ P - B
    # r = a - b and want = a' - b with |a - a'| within the product bar on z; both subtractions are exact (a and a' equal b to a few
    # ulps: Sterbenz)
    bound = 2.0 * nx * M.U * (np.abs(z) @ np.abs(P))
    print("solve_residual: |r| %.2e, against NumPy's P z - b worst %.3f of the product bar on z" % (np.abs(r).max(), (np.abs(r - want) / bound).max()))
    assert np.all(np.abs(r - want) <= bound)
    assert np.abs(r).max() < V.bar(P) * np.abs(B).max()       # ... and small: the solve was one


# ------------------------------------------------------------------------------------------------------------------
# 6. refusals, each with the handle as it was and nothing flushed
# ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_alone():
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd.sharding import ShardGroup
    n = 20
    e, twin = sources(2, 3, n, tile=16, batch=8)
    assert e.pending() == 3
    dp = ctypes.POINTER(ctypes.c_double)
    nx = 3 + 2 * n
    good, out = np.zeros((2, nx)), np.zeros((2, nx))
    nonfinite = good.copy()
    nonfinite[1, 7] = np.inf

    def call(h, B, k, o):
        return e.lib.ekf_multiply_map(h, None if B is None else B.ctypes.data_as(dp), ctypes.c_int64(k), None if o is None else o.ctypes.data_as(dp))

    bad = L.EKF_ERR_INVALID_ARG
    assert call(None, good, 2, out) == bad
    cases = [("a null B", None, 2, out, b"null B"), ("a null out", good, 2, None, b"null out"), ("k = 0", good, 0, out, b"at least 1"),
             ("k = -3", good, -3, out, b"at least 1"), ("a B entry that is not finite", nonfinite, 2, out, b"not finite")]
    for name, B, k, o, word in cases:
        assert call(e.h, B, k, o) == bad, name
        msg = e.lib.ekf_last_error(e.h)
        assert b"multiply_map" in msg and word in msg, (name, msg)
        assert e.pending() == 3, name
    assert not out.any()
    # a shard group refuses with the library's error
    grp = ShardGroup(2, capacity=n + 4, tile=16)
    grp.load_lowrank_state(*lowrank_data(n, 5))
    gx = grp.shards[0].get_x()
    st, msg = status_of(lambda: grp.multiply_map(good))
    assert st == bad and "sharded" in msg and "multiply_map" in msg and "own tiles" in msg and grp.N == n
    np.testing.assert_array_equal(grp.shards[0].get_x(), gx)
    grp.close()
    # a lone shard between begin and finish; afterwards it works
    sh = loaded(n, 5, capacity=n + 4, tile=16, force_sharded=1)
    xs = sh.get_x()
    sh.predict(U2)
    sh.correct_begin(observe(xs, 4), R2, 4)
    st, msg = status_of(lambda: sh.multiply_map(good))
    assert st == L.EKF_ERR_STATE and "begin and finish" in msg and "multiply_map" in msg
    harr = (ctypes.c_void_p * 1)(sh.h)
    assert sh.lib.ekf_exchange_local(harr, 1) == 0
    sh.correct_finish()
    within_the_bar(sh, sh.get_P(), "a lone cfg.force_sharded shard")
    # nothing was changed and nothing flushed: the handle is bit for bit its twin, and goes on
    assert e.pending() == 3
    for got, ref in zip(getters(e), getters(twin)):          # x, s, P, the diagonal blocks, ekf_P_digest
        np.testing.assert_array_equal(got, ref)
    assert not e.multiply_map(good).any() and e.pending() == 0


# ------------------------------------------------------------------------------------------------------------------
# 7. beside an asynchronous pass
# ------------------------------------------------------------------------------------------------------------------
def test_behind_an_asynchronous_pass_just_queued():
    n = 140
    x = lowrank_data(n, 5)[0]
    G = M.gaussian_rows(CHUNK + 2, 3 + 2 * n, 8)
    runs = []
    for asy in (True, False):
        e = loaded(n, 5, capacity=n + 4, tile=16, batch=3, async_flush=asy)
        for k in (5, 60, 100):                                # the batch completes: its pass is queued (asynchronous: on the pass stream)
            e.predict(U2); e.correct(observe(x, k), R2, k)
        e.predict(U2); e.correct(observe(x, 7), R2, 7)        # and one pair recorded behind it
        runs.append((e, e.multiply_map(G)))
        assert e.pending() == 0
    np.testing.assert_array_equal(runs[0][1], runs[1][1])
    assert_same(runs[0][0], runs[1][0])
