"""GPU: draws from the posterior on the device (ekf_sample_map; include/ekfslam.h).

The yardstick is NumPy on THE MATRIX A TWIN REPORTS, as in tests/test_factor_map_gpu.py: twin.get_x() / twin.get_P() of a twin with the
same history (pending pairs, a recorded predict), numpy.linalg.cholesky of that P permuted into the library's elimination order, and the
restatement of tests/sample_map_cases.py.  Both sides work on the same doubles, float stores included, so every comparison is held to
helpers.REL.  The draws are the n unit vectors -- their samples minus x are the columns of C -- and a few Gaussian rows.

The factor store's tiles have edge 64 and a tile row is cut into segments of 16 tiles: N = 140 is five tile columns (the last tile row
holds 24 of 64 rows), N = 96 ends exactly on a tile edge, N = 1 and N = 0 leave the robot tail alone, and N = 1100 is the one size at
which a tile row has more than one segment."""
import ctypes

import numpy as np
import pytest

import factor_map_cases as F
import sample_map_cases as S
from helpers import R2, REL, U2, assert_same, engine, getters, loaded, status_of
from removal_cases import lowrank_data, observe

pytestmark = pytest.mark.gpu
STORES = [(16, "f64", 140), (64, "f64", 140), (16, "f32", 140), (256, "f32_mixed", 140), (128, "f64", 200), (256, "f32", 300)]   # test_factor_map_gpu's
CHUNK = S.CHUNK


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


def same_info(a, b):
    for k in F.KEYS:
        np.testing.assert_array_equal(a[k], b[k])


def against_numpy(e, x, P, label, dense=True, extra=3):
    """The unit vectors and `extra` Gaussian rows through e.sample_map: C against numpy.linalg.cholesky of the permuted P, C C' against
    P, the samples against the restatement (dense) or against x + xi C' with NumPy's C."""
    n = x.size
    xi = S.unit_draws(n, extra)
    samples, info = e.sample_map(xi)
    assert samples.shape == xi.shape and info["definite"] and info["bad_index"] == -1 and info["n"] == n
    C = S.recovered_factor(x, samples)
    want = S.cholesky_in_x_order(P)
    order = F.elimination_order(n)
    assert not np.triu(C[np.ix_(order, order)], 1).any()      # lower-triangular in elimination order: exact zeros
    err_c = np.abs(C - want).max() / np.abs(want).max()
    err_p = np.abs(C @ C.T - P).max() / np.abs(P).max()
    expect = S.sample_dense(x, P, xi) if dense else x[None, :] + xi @ want.T
    err_s = np.abs(samples - expect).max() / max(np.abs(expect).max(), 1.0)
    print("%s: C against numpy.linalg.cholesky %.2e, C C' against P %.2e, the samples %.2e" % (label, err_c, err_p, err_s))
    assert err_c < REL and err_p < REL and err_s < REL
    return samples, info


# ------------------------------------------------------------------------------------------------------------------
# 1. against NumPy on the same matrix
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage,n", STORES)
def test_samples_against_numpy_on_the_same_matrix(tile, storage, n):
    e, twin, other = sources(3, 3, n, tile=tile, storage=storage)
    assert e.pending() == 3
    x, P = twin.get_x(), twin.get_P()                         # (flushes the twin)
    _, info = against_numpy(e, x, P, "N=%d T=%d %s" % (n, tile, storage))
    assert e.pending() == 0 and e.N == n
    want = other.factor_map()
    del want["d2"]
    same_info(info, want)                                     # bit for bit what factor_map reports on the same state


def test_a_map_that_ends_exactly_on_a_tile_edge():
    e, twin = sources(2, 3, 96, tile=64)                      # 192 rows: exactly three tiles of 64
    against_numpy(e, twin.get_x(), twin.get_P(), "N=96 T=64")


def test_one_landmark_and_none():
    e, twin = sources(2, 1, 1, tile=16)
    against_numpy(e, twin.get_x(), twin.get_P(), "N=1")
    g = engine(capacity=8, tile=16)
    x0 = np.array([1.0, -2.0, 40.0])
    P0 = np.array([[0.5, 0.1, -0.05], [0.1, 0.4, 0.02], [-0.05, 0.02, 0.3]])
    g.set_x(x0); g.set_P(P0)
    samples, info = against_numpy(g, x0, P0, "N=0, an SPD Prr")
    assert info["logdet_map"] == 0.0 and info["n"] == 3


def test_a_tile_row_of_two_full_segments_and_a_partial_one():
    """N = 1100: 2200 rows are 35 tile rows of 64 (the last holds 24), so the longest tile row has 35 tiles = two full segments of 16
    and a partial one of 3, and every count of segments from one to three occurs.  F64; numpy.linalg.cholesky is the yardstick (the
    restatement's Python loop is too slow here).  All 2203 unit vectors: 138 chunks, so the staging slots go round many times."""
    n = 1100
    e = loaded(n, 5, capacity=n + 4, tile=64)
    twin = loaded(n, 5, capacity=n + 4, tile=64)
    against_numpy(e, twin.get_x(), twin.get_P(), "N=1100 T=64", dense=False, extra=5)


# ------------------------------------------------------------------------------------------------------------------
# 2. the promised bits
# ------------------------------------------------------------------------------------------------------------------
def test_a_row_depends_on_its_own_draw_alone():
    n = 140
    e, twin = sources(2, 3, n, tile=16)
    nx = 3 + 2 * n
    big = 3 * CHUNK + 5                                       # four chunks, the last partial
    G = S.gaussian_draws(big, nx, 11)
    G[CHUNK + 4], G[-1] = G[0], G[0]                          # the first draw again in the middle and at the end
    whole, info = e.sample_map(G)
    assert info["definite"] and e.pending() == 0
    twin.flush()
    np.testing.assert_array_equal(e.sample_map(np.zeros((2, nx)))[0], np.vstack([twin.get_x()] * 2))       # xi = 0 gives x
    for k in (1, CHUNK, CHUNK + 1):
        part, _ = e.sample_map(G[:k])
        np.testing.assert_array_equal(part, whole[:k])
    np.testing.assert_array_equal(whole[CHUNK + 4], whole[0])
    np.testing.assert_array_equal(whole[-1], whole[0])
    np.testing.assert_array_equal(e.sample_map(G[2 * CHUNK + 1:])[0], whole[2 * CHUNK + 1:])               # another position in its chunk
    again, info2 = e.sample_map(G)                            # from call to call
    np.testing.assert_array_equal(again, whole)
    same_info(info, info2)
    err = np.abs(whole - S.sample_dense(twin.get_x(), twin.get_P(), G)).max() / np.abs(whole).max()
    print("N=140, %d Gaussian draws against the restatement: %.2e" % (big, err))
    assert err < REL


def test_zero_draws_return_x_with_its_signed_zeros():
    """assert_array_equal cannot tell -0.0 from +0.0: the bytes are compared.  A robot entry, a landmark entry and the last entry of x are
    -0.0; with the unit vector e_5 the entry before it in the elimination order (index 4) has a zero deviation and keeps its sign."""
    n = 13
    e = loaded(n, 5, capacity=n + 4, tile=16)
    x = e.get_x().copy()
    x[[1, 4, 28]] = -0.0
    e.set_x(x)
    assert e.get_x().tobytes() == x.tobytes()
    e5 = np.zeros(x.size)
    e5[5] = 1.0
    samples, info = e.sample_map(np.vstack([np.zeros(x.size), e5]))
    assert info["definite"] and samples[0].tobytes() == x.tobytes() and np.signbit(samples[0][[1, 4, 28]]).all()
    assert np.signbit(samples[1][4]) and samples[1][3] == x[3] and samples[1][5] > x[5] and samples[1][28] != 0.0 and samples[1][1] != 0.0


@pytest.mark.parametrize("tile,storage", [(16, "f64"), (256, "f32_mixed")])
def test_the_call_changes_nothing(tile, storage):
    n = 140
    e, twin = sources(2, 3, n, tile=tile, storage=storage, batch=4)
    before = e.device_bytes()
    e.factor_map()
    factored = e.device_bytes()
    G = S.gaussian_draws(CHUNK + 1, 3 + 2 * n, 2)
    first, _ = e.sample_map(G)
    held = e.device_bytes()
    assert factored > before and held >= factored + 8 * 2 * CHUNK * (2 * n + 3)       # the chunks and the partial blocks are counted
    e.sample_map(np.vstack([G] * 5))                          # more draws: the same scratch
    assert e.device_bytes() == held and e.pending() == 0
    twin.flush()
    assert_same(e, twin)                                      # x, s, P, the diagonal blocks and the digest of a twin that only flushed
    x1 = e.get_x()
    for q in (e, twin):
        for k in (3, 9, 70, 139, 3):
            q.predict(U2); q.correct(observe(x1, k), R2, k)
        q.flush()
    assert_same(e, twin)


# ------------------------------------------------------------------------------------------------------------------
# 3. not positive definite: NaN samples with EKF_OK
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where,bad", [("the first tile column", 3 + 5), ("a later tile column", 3 + 128), ("the robot tail", 1)])
def test_a_pivot_that_fails_is_a_result(where, bad):
    n = 140
    x, s, P = F.indefinite_scene(n, bad)
    pair = []
    for _ in range(2):
        g = engine(capacity=n + 4, tile=16)
        g.set_x(x); g.set_s(s); g.set_P(P)
        pair.append(g)
    e, other = pair
    got = []
    st, msg = status_of(lambda: got.append(e.sample_map(S.gaussian_draws(CHUNK + 3, x.size, 4))))
    assert st == 0, msg
    samples, info = got[0]
    assert samples.shape == (CHUNK + 3, x.size) and np.isnan(samples).all()
    assert not info["definite"] and info["bad_index"] == bad
    want = other.factor_map()
    del want["d2"]
    same_info(info, want)
    xg, sg, Pg = F.spd_scene(n, 3)                            # a second call on a repaired P succeeds
    e.set_P(Pg)
    against_numpy(e, x, Pg, "repaired after %s" % where)


# ------------------------------------------------------------------------------------------------------------------
# 4. refusals, each with the handle as it was and nothing flushed
# ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_alone():
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd.sharding import ShardGroup
    n = 20
    e, twin = sources(2, 3, n, tile=16, batch=8)
    assert e.pending() == 3
    dp = ctypes.POINTER(ctypes.c_double)
    info = L.EkfFactorInfo()
    nx = 3 + 2 * n
    good, out = np.zeros((2, nx)), np.zeros((2, nx))
    nonfinite = good.copy()
    nonfinite[1, 7] = np.inf

    def call(h, xi, k, o, pinfo):
        return e.lib.ekf_sample_map(h, None if xi is None else xi.ctypes.data_as(dp), ctypes.c_int64(k),
                                    None if o is None else o.ctypes.data_as(dp), pinfo)

    bad = L.EKF_ERR_INVALID_ARG
    assert call(None, good, 2, out, ctypes.byref(info)) == bad
    cases = [("a null xi", None, 2, out, ctypes.byref(info), b"null xi"), ("a null out", good, 2, None, ctypes.byref(info), b"null out"),
             ("a null info", good, 2, out, None, b"null info"), ("k = 0", good, 0, out, ctypes.byref(info), b"at least 1"),
             ("k = -3", good, -3, out, ctypes.byref(info), b"at least 1"),
             ("an xi entry that is not finite", nonfinite, 2, out, ctypes.byref(info), b"not finite")]
    for name, xi, k, o, pinfo, word in cases:
        assert call(e.h, xi, k, o, pinfo) == bad, name
        msg = e.lib.ekf_last_error(e.h)
        assert b"sample_map" in msg and word in msg, (name, msg)
        assert e.pending() == 3, name
    assert not out.any()
    # a shard group refuses with the library's error
    grp = ShardGroup(2, capacity=n + 4, tile=16)
    grp.load_lowrank_state(*lowrank_data(n, 5))
    gx = grp.shards[0].get_x()
    st, msg = status_of(lambda: grp.sample_map(good))
    assert st == bad and "sharded" in msg and "sample_map" in msg and "own tiles" in msg and grp.N == n
    np.testing.assert_array_equal(grp.shards[0].get_x(), gx)
    grp.close()
    # a lone shard between begin and finish
    sh = loaded(n, 5, capacity=n + 4, tile=16, force_sharded=1)
    xs = sh.get_x()
    sh.predict(U2)
    sh.correct_begin(observe(xs, 4), R2, 4)
    st, msg = status_of(lambda: sh.sample_map(good))
    assert st == L.EKF_ERR_STATE and "begin and finish" in msg and "sample_map" in msg
    harr = (ctypes.c_void_p * 1)(sh.h)
    assert sh.lib.ekf_exchange_local(harr, 1) == 0
    sh.correct_finish()
    # nothing was changed and nothing flushed: the handle is bit for bit its twin, and goes on
    assert e.pending() == 3
    for got, ref in zip(getters(e), getters(twin)):          # x, s, P, the diagonal blocks, ekf_P_digest
        np.testing.assert_array_equal(got, ref)
    assert e.sample_map(good)[1]["definite"] and e.pending() == 0


# ------------------------------------------------------------------------------------------------------------------
# 5. other handles and layers
# ------------------------------------------------------------------------------------------------------------------
def test_a_lone_shard_works_and_the_policies_reach_the_device():
    from ekf_slam_amd.slam import EKF_SLAM
    n = 40
    sh = loaded(n, 5, capacity=n + 4, tile=16, force_sharded=1)
    against_numpy(sh, sh.get_x(), sh.get_P(), "a lone cfg.force_sharded shard")
    f = EKF_SLAM(capacity=n + 4, tile=16)
    f._e.load_lowrank_state(*lowrank_data(n, 5))
    x, P = f._e.get_x(), f._e.get_P()
    draws = np.random.default_rng(9).standard_normal((200, x.size))
    want = S.sample_dense(x, P, draws)
    samples, info = f.sample_map(200, seed=9)
    assert info["definite"] and np.abs(samples - want).max() < REL * np.abs(want).max()
    mean, se = f.posterior_expectation(lambda v: v[3:5] - v[0:2], 200, seed=9)
    vals = want[:, 3:5] - want[:, 0:2]
    assert np.abs(mean - vals.mean(axis=0)).max() < REL * np.abs(vals).max() and np.allclose(se, vals.std(axis=0, ddof=1) / np.sqrt(200), rtol=1e-6)
    p, sep = f.probability(lambda v: v[3] > x[3], 200, seed=9)
    assert p == np.mean(want[:, 3] > x[3]) and 0.3 < p < 0.7 and sep > 0


def test_behind_an_asynchronous_pass_just_queued():
    n = 140
    x = lowrank_data(n, 5)[0]
    G = S.gaussian_draws(CHUNK + 2, 3 + 2 * n, 8)
    runs = []
    for asy in (True, False):
        e = loaded(n, 5, capacity=n + 4, tile=16, batch=3, async_flush=asy)
        for k in (5, 60, 100):                                # the batch completes: its pass is queued (asynchronous: on the pass stream)
            e.predict(U2); e.correct(observe(x, k), R2, k)
        e.predict(U2); e.correct(observe(x, 7), R2, 7)        # and one pair recorded behind it
        runs.append((e, e.sample_map(G)))
        assert e.pending() == 0
    assert runs[0][1][1]["definite"]
    np.testing.assert_array_equal(runs[0][1][0], runs[1][1][0])
    same_info(runs[0][1][1], runs[1][1][1])
    assert_same(runs[0][0], runs[1][0])
