"""GPU: C^-1 B and P^-1 B on the device (ekf_solve_map; include/ekfslam.h).

The yardstick is NumPy on THE MATRIX A TWIN REPORTS, as in tests/test_sample_map_gpu.py: twin.get_x() / twin.get_P() of a twin with the
same history (pending pairs, a recorded predict); the expected full form is numpy.linalg.solve(P, b), the expected half form a
triangular solve with numpy.linalg.cholesky of the permuted P (solve_map_cases.expected).  THE BAR is solve_map_cases.bar(P) =
64 cond_2(P) 2^-53 on the relative error, max-abs over the max-abs of the expected result: both routes are backward-stable solves whose
forward error is a small multiple of cond u, 64 is the margin over that multiple; it is also asserted below helpers.REL.

The factor store's tiles have edge 64: N = 140 is five tile columns (the last tile row holds 24 of 64 rows), N = 96 ends exactly on a
tile edge, N = 1 and N = 0 leave the robot tail alone, and N = 1100 is 35 tile columns, so that each sweep is a chain of 35 dependent
launches."""
import ctypes

import numpy as np
import pytest

import factor_map_cases as F
import sample_map_cases as S
import solve_map_cases as V
from helpers import R2, REL, U2, assert_same, engine, getters, loaded, status_of
from removal_cases import lowrank_data, observe

pytestmark = pytest.mark.gpu
CHUNK = V.CHUNK


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


def against_numpy(e, P, label, B=None):
    """Both forms of B (by default the unit vectors of 19 spread indices and 3 Gaussian rows: two chunks) against NumPy on P, within
    the bar; the figures printed before they are asserted.  Returns the info of the last call."""
    n = P.shape[0]
    B = V.spread_rhs(n) if B is None else B
    bar = V.bar(P)
    assert bar < REL
    info = None
    for name, form in V.FORMS.items():
        out, info = e.solve_map(B, name)
        assert out.shape == B.shape and info["definite"] and info["bad_index"] == -1 and info["n"] == n
        err = V.rel_err(out, V.expected(P, B, form))
        print("%s, %s: %.2e against NumPy (bar %.2e, cond %.1e)" % (label, name, err, bar, np.linalg.cond(P)))
        assert err < bar, (label, name, err, bar)
    return info


# ------------------------------------------------------------------------------------------------------------------
# 1. against NumPy on the same matrix
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage,n", V.STORES)
def test_solves_against_numpy_on_the_same_matrix(tile, storage, n):
    e, twin, other = sources(3, 3, n, tile=tile, storage=storage)
    assert e.pending() == 3
    P = twin.get_P()                                          # (flushes the twin)
    info = against_numpy(e, P, "N=%d T=%d %s" % (n, tile, storage))
    assert e.pending() == 0 and e.N == n
    want = other.factor_map()
    del want["d2"]
    same_info(info, want)                                     # bit for bit what factor_map reports on the same state


def test_a_map_that_ends_exactly_on_a_tile_edge():
    e, twin = sources(2, 3, 96, tile=64)                      # 192 rows: exactly three tiles of 64
    against_numpy(e, twin.get_P(), "N=96 T=64")


def test_one_landmark_and_none():
    e, twin = sources(2, 1, 1, tile=16)
    against_numpy(e, twin.get_P(), "N=1")
    g = engine(capacity=8, tile=16)
    P0 = np.array([[0.5, 0.1, -0.05], [0.1, 0.4, 0.02], [-0.05, 0.02, 0.3]])
    g.set_x(np.array([1.0, -2.0, 40.0])); g.set_P(P0)
    B = np.vstack([np.eye(3), [[0.3, -1.0, 2.0]]])
    info = against_numpy(g, P0, "N=0, an SPD Prr", B)
    assert info["logdet_map"] == 0.0 and info["n"] == 3
    assert V.rel_err(g.solve_map(B)[0], np.linalg.solve(P0, B.T).T) < V.bar(P0)          # out = Prr^-1 b


def test_a_long_sequential_chain():
    """N = 1100: 2200 rows are 35 tile columns of 64 (the last holds 24 rows); k = 19 is two chunks."""
    n = 1100
    e = loaded(n, 5, capacity=n + 4, tile=64)
    twin = loaded(n, 5, capacity=n + 4, tile=64)
    against_numpy(e, twin.get_P(), "N=1100 T=64", V.spread_rhs(3 + 2 * n, 16, 3))


def test_the_round_trip_with_the_librarys_own_draws():
    """solve_map(sample_map(xi) - x, "half") returns xi, and |half|^2 of x - ref is factor_map's d2, both within the bar."""
    n = 140
    e, twin = sources(2, 3, n, tile=64)
    x, P = twin.get_x(), twin.get_P()
    bar = V.bar(P)
    xi = S.gaussian_draws(CHUNK + 3, x.size, 21)
    samples, _ = e.sample_map(xi)
    back, info = e.solve_map(samples - x[None, :], "half")
    err = V.rel_err(back, xi)
    print("C^-1 (sample - x) against the draws: %.2e (bar %.2e)" % (err, bar))
    assert info["definite"] and err < bar < REL
    refs = F.reference_states(x, 3, 4)                        # a few degrees off on the heading: nowhere near +-180
    nu = x[None, :] - refs
    assert np.abs(nu[:, 2]).max() < 90.0
    half, _ = e.solve_map(nu, "half")
    d2 = e.factor_map(refs)["d2"]
    err = V.rel_err(np.sum(half * half, axis=1), d2)
    print("|C^-1 (x - ref)|^2 against factor_map's d2: %.2e" % err)
    assert err < bar


# ------------------------------------------------------------------------------------------------------------------
# 2. the promised bits
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["full", "half"])
def test_a_row_depends_on_its_own_right_hand_side_alone(form):
    n = 140
    e, twin = sources(2, 3, n, tile=16)
    nx = 3 + 2 * n
    big = 3 * CHUNK + 5                                       # four chunks, the last partial
    G = S.gaussian_draws(big, nx, 11)
    G[CHUNK + 4], G[-1] = G[0], G[0]                          # the first right-hand side again in the middle and at the end
    whole, info = e.solve_map(G, form)
    assert info["definite"] and e.pending() == 0
    zero = e.solve_map(np.zeros((2, nx)), form)[0]
    assert zero.shape == (2, nx) and not zero.any()           # B = 0 gives 0 in every entry
    np.testing.assert_array_equal(e.solve_map(G[0], form)[0][0], whole[0])           # alone
    for k in (CHUNK, CHUNK + 1):
        part, _ = e.solve_map(G[:k], form)
        np.testing.assert_array_equal(part, whole[:k])
    np.testing.assert_array_equal(whole[CHUNK + 4], whole[0])
    np.testing.assert_array_equal(whole[-1], whole[0])
    np.testing.assert_array_equal(e.solve_map(G[2 * CHUNK + 1:], form)[0], whole[2 * CHUNK + 1:])          # another position in its chunk
    again, info2 = e.solve_map(G, form)                       # from call to call
    np.testing.assert_array_equal(again, whole)
    same_info(info, info2)
    P = twin.get_P()
    err = V.rel_err(whole, V.expected(P, G, V.FORMS[form]))
    print("N=140, %d Gaussian right-hand sides, %s: %.2e (bar %.2e)" % (big, form, err, V.bar(P)))
    assert err < V.bar(P) < REL


@pytest.mark.parametrize("tile,storage", [(16, "f64"), (256, "f32_mixed")])
def test_the_call_changes_nothing(tile, storage):
    n = 140
    e, twin = sources(2, 3, n, tile=tile, storage=storage, batch=4)
    e.sample_map(np.zeros(3 + 2 * n))
    sampled = e.device_bytes()
    G = S.gaussian_draws(CHUNK + 1, 3 + 2 * n, 2)
    e.solve_map(G, "full")
    held = e.device_bytes()
    assert held >= sampled + 8 * 64 * 2 * n                   # the inverses of the diagonal tiles are counted
    e.solve_map(np.vstack([G] * 5), "half")                   # more right-hand sides: the same scratch
    assert e.device_bytes() == held and e.pending() == 0
    twin.flush()
    for got, ref in zip(getters(e), getters(twin)):           # x, s, P, the diagonal blocks and the digest of a twin that only flushed
        np.testing.assert_array_equal(got, ref)
    x1 = e.get_x()
    for q in (e, twin):
        for k in (3, 9, 70, 139, 3):
            q.predict(U2); q.correct(observe(x1, k), R2, k)
        q.flush()
    assert_same(e, twin)


# ------------------------------------------------------------------------------------------------------------------
# 3. not positive definite: NaN output with EKF_OK
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
    want = other.factor_map()
    del want["d2"]
    for form in ("full", "half"):
        got = []
        st, msg = status_of(lambda: got.append(e.solve_map(S.gaussian_draws(CHUNK + 3, x.size, 4), form)))
        assert st == 0, msg
        out, info = got[0]
        assert out.shape == (CHUNK + 3, x.size) and np.isnan(out).all()
        assert not info["definite"] and info["bad_index"] == bad
        same_info(info, want)
    xg, sg, Pg = F.spd_scene(n, 3)                            # a second call on a repaired P succeeds
    e.set_P(Pg)
    against_numpy(e, Pg, "repaired after %s" % where)


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

    def call(h, form, B, k, o, pinfo):
        return e.lib.ekf_solve_map(h, ctypes.c_int32(form), None if B is None else B.ctypes.data_as(dp), ctypes.c_int64(k),
                                   None if o is None else o.ctypes.data_as(dp), pinfo)

    bad = L.EKF_ERR_INVALID_ARG
    assert call(None, 0, good, 2, out, ctypes.byref(info)) == bad
    cases = [("a null B", 0, None, 2, out, ctypes.byref(info), b"null B"), ("a null out", 0, good, 2, None, ctypes.byref(info), b"null out"),
             ("a null info", 1, good, 2, out, None, b"null info"), ("k = 0", 0, good, 0, out, ctypes.byref(info), b"at least 1"),
             ("k = -3", 1, good, -3, out, ctypes.byref(info), b"at least 1"),
             ("form 2", 2, good, 2, out, ctypes.byref(info), b"EKF_SOLVE_FULL"), ("form -1", -1, good, 2, out, ctypes.byref(info), b"EKF_SOLVE_FULL"),
             ("a B entry that is not finite", 0, nonfinite, 2, out, ctypes.byref(info), b"not finite")]
    for name, form, B, k, o, pinfo, word in cases:
        assert call(e.h, form, B, k, o, pinfo) == bad, name
        msg = e.lib.ekf_last_error(e.h)
        assert b"solve_map" in msg and word in msg, (name, msg)
        assert e.pending() == 3, name
    assert not out.any()
    # a shard group refuses with the library's error
    grp = ShardGroup(2, capacity=n + 4, tile=16)
    grp.load_lowrank_state(*lowrank_data(n, 5))
    gx = grp.shards[0].get_x()
    st, msg = status_of(lambda: grp.solve_map(good))
    assert st == bad and "sharded" in msg and "solve_map" in msg and "own tiles" in msg and grp.N == n
    np.testing.assert_array_equal(grp.shards[0].get_x(), gx)
    grp.close()
    # a lone shard between begin and finish
    sh = loaded(n, 5, capacity=n + 4, tile=16, force_sharded=1)
    xs = sh.get_x()
    sh.predict(U2)
    sh.correct_begin(observe(xs, 4), R2, 4)
    st, msg = status_of(lambda: sh.solve_map(good, "half"))
    assert st == L.EKF_ERR_STATE and "begin and finish" in msg and "solve_map" in msg
    harr = (ctypes.c_void_p * 1)(sh.h)
    assert sh.lib.ekf_exchange_local(harr, 1) == 0
    sh.correct_finish()
    # nothing was changed and nothing flushed: the handle is bit for bit its twin, and goes on
    assert e.pending() == 3
    for got, ref in zip(getters(e), getters(twin)):          # x, s, P, the diagonal blocks, ekf_P_digest
        np.testing.assert_array_equal(got, ref)
    assert e.solve_map(good)[1]["definite"] and e.pending() == 0


# ------------------------------------------------------------------------------------------------------------------
# 5. other handles and layers
# ------------------------------------------------------------------------------------------------------------------
def test_a_lone_shard_works_and_the_policies_reach_the_device():
    from ekf_slam_amd.slam import EKF_SLAM
    n = 40
    sh = loaded(n, 5, capacity=n + 4, tile=16, force_sharded=1)
    against_numpy(sh, sh.get_P(), "a lone cfg.force_sharded shard")
    f = EKF_SLAM(capacity=n + 4, tile=16)
    f._e.load_lowrank_state(*lowrank_data(n, 5))
    x, P = f._e.get_x(), f._e.get_P()
    bar = V.bar(P)
    Lam = np.linalg.inv(P)
    idx = [7, 2, 39]
    cols = np.array([3 + 2 * i + r for i in idx for r in (0, 1)])
    got = f.information_columns(idx)
    assert got.shape == (x.size, 6) and V.rel_err(got, Lam[:, cols]) < bar
    assert V.rel_err(f.information_columns(), Lam[:, :3]) < bar
    rest = np.setdiff1d(np.arange(x.size), cols)
    schur = P[np.ix_(cols, cols)] - P[np.ix_(cols, rest)] @ np.linalg.solve(P[np.ix_(rest, rest)], P[np.ix_(rest, cols)])
    cc = f.conditional_covariance(idx)
    print("conditional_covariance against the Schur complement: %.2e (bar %.2e)" % (V.rel_err(cc, schur), bar))
    # (the policy inverts Lambda_AA on the host: its entries are within the bar, and the inverse of a 6 x 6 matrix takes a relative
    # perturbation times its own condition number)
    assert V.rel_err(cc, schur) < bar * np.linalg.cond(schur) < REL
    a = x + np.random.default_rng(3).normal(0.0, 0.5, x.size)
    a[2] = x[2] + 355.0                                       # the heading difference wraps to -5
    d = a - x
    d[2] = -5.0
    want = float(d @ np.linalg.solve(P, d))
    assert abs(f.mahalanobis(a, x) - want) < bar * want
    assert abs(f.mahalanobis(a, x) - f.nees(2.0 * x - a)[0]) < bar * want           # factor_map's d2 of x against x - d wraps the same way


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
        runs.append((e, e.solve_map(G, "full")))
        assert e.pending() == 0
    assert runs[0][1][1]["definite"]
    np.testing.assert_array_equal(runs[0][1][0], runs[1][1][0])
    same_info(runs[0][1][1], runs[1][1][1])
    assert_same(runs[0][0], runs[1][0])
