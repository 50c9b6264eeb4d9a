"""GPU: a local map joined into the map on the device (ekf_join_map; include/ekfslam.h).

The yardstick is the NumPy restatement of tests/join_map_cases.py (P' = J blockdiag(P, PL) J') applied to THE STATE BOTH ENGINES REPORTED
BEFORE THE CALL -- reported by twins with the same history, because reading P flushes and the join is to meet pending pairs; stores,
tolerances and helpers are those of tests/helpers.py.  Where two engines ran the same arithmetic on the same inputs -- M = 0 against a
POSE_DELTA predict, a scan-like local map against ekf_append_model, the asynchronous pass and the device-decided loop against waited twins,
a replayed log -- the comparison is assert_array_equal.

A tile row of T = 16 holds 8 landmarks; landmark 128 is column 256, the second workgroup of k_join_state's 256-lane column grid, the second
256-landmark column group of a k_join_rows row and the first tile-row edge of T = 256: (N, M) = (123, 40) crosses all of them."""
import ctypes

import numpy as np
import pytest

import join_map_cases as J
from helpers import R2, REL, RPOS, TOL_ROW32, U2, assert_same, check_state, engine, getters, loaded, rel_err, state, status_of
from removal_cases import lowrank_data, observe

pytestmark = pytest.mark.gpu
GLOBAL_STORES = [(16, "f64"), (64, "f64"), (16, "f32"), (256, "f32_mixed")]
LOCAL_STORES = [(32, "f64"), (16, "f32")]
SIZES = [(0, 3), (5, 1), (13, 21), (123, 40)]
PENDING = [(0, 0), (5, 3), (5, 0), (0, 3)]                   # (global, local) pairs left pending; which size meets which rotates with the stores


def global_pair(N, pending, **kw):
    """Two engines with the same state and history: `pending` corrections (and a recorded predict behind them), deferred where the
    batch allows it."""
    x = lowrank_data(N, 5)[0]
    e, twin = loaded(N, 5, **kw), loaded(N, 5, **kw)
    for q in (e, twin):
        for k in ([(5 * j + 1) % N for j in range(pending)] if N else []):
            q.predict(U2); q.correct(observe(x, k), R2, k)
        q.predict(U2)
    return e, twin


def local_pair(M, pending, seed=9, **kw):
    """Two local engines with the same state and history: `loaded`, then stir_local's predicts and corrections."""
    out = []
    for _ in range(2):
        e = loaded(M, seed, capacity=max(M, 1) + 2, batch=8, **kw)
        out.append(J.stir_local(e, np.random.default_rng(seed + 1), pending))
    return out


def expectation(g_twin, l_twin, offset):
    x, s, P = state(g_twin)
    y, sL, PL = state(l_twin)
    return J.join_dense(x, s, P, y, sL, PL, offset)


# ------------------------------------------------------------------------------------------------------------------
# 1. against the dense restatement
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ltile,lstorage", LOCAL_STORES)
@pytest.mark.parametrize("tile,storage", GLOBAL_STORES)
def test_a_join_against_the_dense_restatement(tile, storage, ltile, lstorage):
    turn = GLOBAL_STORES.index((tile, storage)) + LOCAL_STORES.index((ltile, lstorage))
    for q, (N, M) in enumerate(SIZES):
        gp, lp = PENDING[(q + turn) % 4]
        gp = gp if N else 0
        g, g_twin = global_pair(N, gp, capacity=N + M + 4, tile=tile, storage=storage, batch=8)
        lo, lo_twin = local_pair(M, lp, tile=ltile, storage=lstorage)
        assert g.pending() == gp and lo.pending() == lp
        ex, es, eP = expectation(g_twin, lo_twin, 1000.0)
        assert g.join_map(lo, 1000.0) == N
        assert g.pending() == 0 and lo.pending() == 0 and g.N == N + M and lo.N == M
        np.testing.assert_array_equal(g.get_s(), es)         # the signature offset is applied
        check_state(g, ex, eP, storage, "N=%d M=%d pending %d/%d local %s" % (N, M, gp, lp, lstorage), es)
        assert np.all(np.isfinite(g.get_P()))
        for e in (g, g_twin, lo, lo_twin):
            e.close()


# ------------------------------------------------------------------------------------------------------------------
# 2. known answer: M = 0 is a POSE_DELTA predict
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage", GLOBAL_STORES)
def test_a_local_map_without_landmarks_is_a_pose_delta_predict(tile, storage):
    N = 130
    g, twin = global_pair(N, 3, capacity=N + 4, tile=tile, storage=storage, batch=8)
    q = np.array([0.8, -0.45, 11.5])
    PLqq = np.array([[0.04, 0.01, 0.002], [0.01, 0.03, -0.004], [0.002, -0.004, 0.5]])
    lo = J.set_state(engine(capacity=2, tile=16), q, [], PLqq)
    assert g.join_map(lo) == N and g.N == N and g.pending() == 0
    twin.flush()
    twin.predict_model([(3, q, PLqq)])
    for name in ("get_x", "get_s", "get_P", "get_P_diag_blocks"):
        np.testing.assert_array_equal(getattr(g, name)(), getattr(twin, name)(), err_msg=name)


# ------------------------------------------------------------------------------------------------------------------
# 3. known answer: a local map that is a scan
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage", [(16, "f64"), (64, "f64"), (256, "f32")])
def test_a_scan_like_local_map_is_an_append_model(tile, storage):
    N, M = 123, 9
    g, twin = loaded(N, 5, capacity=N + M + 4, tile=tile, storage=storage), loaded(N, 5, capacity=N + M + 4, tile=tile, storage=storage)
    assert 0.0 <= g.get_x()[2] < 360.0
    rng = np.random.default_rng(31)
    m = rng.uniform(-15, 15, (M, 2))
    blocks = [RPOS * (1.0 + 0.1 * i) for i in range(M)]
    y = np.concatenate([np.zeros(3), m.reshape(-1)])
    PL = np.zeros((3 + 2 * M, 3 + 2 * M))
    for i, B in enumerate(blocks):
        PL[3 + 2 * i:5 + 2 * i, 3 + 2 * i:5 + 2 * i] = B
    sL = 50.0 + np.arange(M)
    lo = J.set_state(engine(capacity=M + 2, tile=32), y, sL, PL)
    assert g.join_map(lo, 7000.0) == N
    assert twin.append_model([(4, m[i], blocks[i], sL[i] + 7000.0) for i in range(M)]) == N
    for name in ("get_x", "get_s", "get_P", "get_P_diag_blocks"):
        np.testing.assert_array_equal(getattr(g, name)(), getattr(twin, name)(), err_msg=name)
    assert np.all(np.isfinite(g.get_P()))


# ------------------------------------------------------------------------------------------------------------------
# 4. what makes it a join: the submap's internal geometry does not depend on where it is attached
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage,ltile,lstorage", [(16, "f64", 32, "f64"), (64, "f64", 16, "f32"), (16, "f32", 32, "f64")])
def test_innovations_inside_the_submap_are_those_of_the_local_map(tile, storage, ltile, lstorage):
    N, M = 123, 12
    g, _ = global_pair(N, 3, capacity=N + M + 4, tile=tile, storage=storage, batch=8)
    lo, _ = local_pair(M, 0, tile=ltile, storage=lstorage)
    assert g.join_map(lo) == N
    floaty = "f32" in storage or "f32" in lstorage
    Pg = g.get_P()
    worst = dict(nu=0.0, S=0.0, nu2=0.0, S2=0.0)
    rng = np.random.default_rng(4)
    R1 = [[0.05, 0.0], [0.0, 0.0]]                            # a one-row model: the variance of its row
    for i in (0, 4, M - 1):
        z = rng.uniform(-10, 10, 2)
        a, b = g.model_innovation(4, z, RPOS, [N + i]), lo.model_innovation(4, z, RPOS, [i])
        worst["nu"] = max(worst["nu"], np.abs(a["nu"] - b["nu"]).max() / max(np.abs(b["nu"]).max(), 1.0))
        worst["S"] = max(worst["S"], rel_err(a["S"], b["S"]))
    for i, j in ((0, M - 1), (5, 2)):
        # the landmark-distance model between two new landmarks: its S reads their cross block, i.e. the tiles
        a, b = g.model_innovation(5, [3.0], R1, [N + i, N + j]), lo.model_innovation(5, [3.0], R1, [i, j])
        rows = Pg[[3 + 2 * (N + i), 4 + 2 * (N + i), 3 + 2 * (N + j), 4 + 2 * (N + j)], :]
        scale = np.abs(rows).max() if floaty else np.abs(b["S"]).max()
        worst["nu2"] = max(worst["nu2"], np.abs(a["nu"] - b["nu"]).max() / max(np.abs(b["nu"]).max(), 1.0))
        worst["S2"] = max(worst["S2"], np.abs(a["S"] - b["S"]).max() / scale)
    print("global %s local %s: relative-xy nu %.2e S %.2e; landmark range nu %.2e S %.2e%s" %
          (storage, lstorage, worst["nu"], worst["S"], worst["nu2"], worst["S2"], " (S of the range against the largest entry of the rows read)" if floaty else ""))
    # one landmark's S reads nothing but F64-kept entries on every store; the pair's S reads a cross block that a float store rounded to
    # 6e-8 of ITS size -- the global robot's uncertainty, which cancels in S -- and enters S four times through unit rows of H: measured
    # against the largest entry of the rows read, as DESIGN.md section 5 defines its row bound, and held to that bound itself
    assert worst["nu"] < REL and worst["nu2"] < REL
    if floaty:
        assert worst["S"] < TOL_ROW32 and worst["S2"] <= TOL_ROW32
    else:
        assert worst["S"] < REL and worst["S2"] < REL


# ------------------------------------------------------------------------------------------------------------------
# 5. the local map is left as it was
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ltile,lstorage", LOCAL_STORES)
def test_the_local_map_is_untouched_and_may_be_destroyed_at_once(ltile, lstorage):
    N, M = 13, 21
    g, g_twin = global_pair(N, 3, capacity=N + 2 * M + 4, tile=16, batch=8)
    lo, lo_twin = local_pair(M, 3, tile=ltile, storage=lstorage)
    lo.flush()
    before = getters(lo)
    ex, es, eP = expectation(g_twin, lo_twin, 100.0)
    assert g.join_map(lo, 100.0) == N
    assert lo.N == M
    for got, ref in zip(getters(lo), before):                # x, s, P, the diagonal blocks, the digest: bit for bit
        np.testing.assert_array_equal(got, ref)
    # a second join, the local map destroyed while the first reader of the global state has yet to come
    ex2, es2, eP2 = J.join_dense(ex, es, eP, *state(lo_twin), 200.0)
    assert g.join_map(lo, 200.0) == N + M
    lo.close()
    check_state(g, ex2, eP2, "f64", "two joins, the local map destroyed at once", es2)


# ------------------------------------------------------------------------------------------------------------------
# 6. beside the other machinery
# ------------------------------------------------------------------------------------------------------------------
def test_beside_an_asynchronous_pass_just_queued():
    N, M = 123, 21
    x = lowrank_data(N, 5)[0]
    runs = []
    for asy in (True, False):
        g = loaded(N, 5, capacity=N + M + 4, tile=16, batch=3, async_flush=asy)
        lo, _ = local_pair(M, 0, tile=32, storage="f64")
        for k in (5, 60, 100):                                # the batch completes: its pass is queued (asynchronous: on the pass stream)
            g.predict(U2); g.correct(observe(x, k), R2, k)
        g.predict(U2); g.correct(observe(x, 7), R2, 7)        # and one pair recorded behind it
        assert g.join_map(lo, 10.0) == N and g.pending() == 0
        x1 = g.get_x()
        for k in (N + 3, 9, N + M - 1):
            g.predict(U2); g.correct(observe(x1, k), R2, k)
        runs.append(g)
    assert_same(runs[0], runs[1])


def test_behind_an_unsettled_scan_of_the_device_decided_loop():
    from decided_plans import PARAMS, make_plan
    from ekf_slam_amd.engine import Engine
    plan = make_plan(7, 300, 12, 8)
    runs, firsts = [], []
    for mode in (4, 1):
        g = Engine(mode="uc", capacity=300, device_assoc=mode, tile=16, batch=4, **PARAMS)
        lo, _ = local_pair(5, 0, tile=32, storage="f64")
        for t, (u, rows, idx, loc) in enumerate(plan):
            g.predict(u)
            g.measure(rows, u, idx, loc)
            if t == 8:                                        # straight behind the scan: with device_assoc = 4 nothing of it is settled
                firsts.append(g.join_map(lo, 9000.0))
        runs.append(g)
    assert firsts[0] == firsts[1] > 8 and runs[0].N == runs[1].N
    assert_same(runs[0], runs[1])


# ------------------------------------------------------------------------------------------------------------------
# 7. the engine goes on
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage", [(16, "f64"), (64, "f64")])
def test_the_engine_goes_on_after_a_join(tile, storage):
    N, M = 13, 21
    kw = dict(capacity=N + 2 * M + 8, tile=tile, storage=storage, batch=4)
    g, g_twin = global_pair(N, 0, **kw)
    lo, lo_twin = local_pair(M, 0, tile=32, storage="f64")
    ex, es, eP = expectation(g_twin, lo_twin, 100.0)
    assert g.join_map(lo, 100.0) == N
    twin = J.set_state(engine(**kw), ex, es, eP)
    x1 = g.get_x()
    rng = np.random.default_rng(8)
    scan = [(4, rng.uniform(-8, 8, 2), RPOS, 900.0 + b) for b in range(3)]
    for q in (g, twin):
        for k in (4, N + 6, N + M - 1):                       # an old landmark, new ones on both sides of a tile-row edge
            q.predict(U2); q.correct(observe(x1, k), R2, k)
        assert q.append_model(scan) == N + M
        q.remove_landmarks([N + 2])
    check_state(g, *[state(twin)[k] for k in (0, 2)], storage, "corrections, an append and a removal behind a join", state(twin)[1])
    y, sL, PL = state(lo_twin)
    ex2, es2, eP2 = J.join_dense(*state(twin), y, sL, PL, 200.0)
    assert g.join_map(lo, 200.0) == N + M + 2
    check_state(g, ex2, eP2, storage, "a second join", es2)


# ------------------------------------------------------------------------------------------------------------------
# 8. the policy: join, then fuse what both maps saw; the replayed log
# ------------------------------------------------------------------------------------------------------------------
def test_join_submap_fuses_the_landmarks_both_maps_saw_and_replays(tmp_path):
    from ekf_slam_amd.slam import EKF_SLAM
    from ekf_slam_amd.trajectory import FORMAT_JOIN_MAP, TrajectoryLog
    rng = np.random.default_rng(12)
    N, M, shared = 12, 7, [2, 5, 8, 11]
    grid = np.array([[6.0 * (k % 4) - 9.0, 6.0 * (k // 4) - 6.0] for k in range(N + M)])      # 6 apart: no two landmarks near each other
    pose = np.array([0.5, -0.3, 40.0])
    x0 = np.concatenate([pose, (grid[:N] + rng.normal(0, 0.02, (N, 2))).reshape(-1)])
    P0 = J.random_spd(rng, 3 + 2 * N, 0.002)
    Rt = J.rot(pose[2]).T
    world = np.concatenate([grid[shared], grid[N:N + M - len(shared)]])
    y = np.concatenate([[0.0, 0.0, 0.0], ((world - pose[:2]) @ Rt.T + rng.normal(0, 0.02, (M, 2))).reshape(-1)])
    PL = J.random_spd(rng, 3 + 2 * M, 0.002)
    PL[:3, :] = PL[:, :3] = 0.0                               # a submap started at the pose: x = 0, P = 0 there
    kw = dict(capacity=N + M + 4, tile=16, batch=4)
    f, sub = EKF_SLAM(**kw), EKF_SLAM(capacity=M + 2, tile=32)
    f.x = x0; f.s = np.arange(1.0, N + 1); f.P = P0
    sub.x = y; sub.s = np.arange(1.0, M + 1); sub.P = PL
    f.log = TrajectoryLog()
    f.predict(U2)
    f.log.record(U2, None, [], np.zeros((0, 2)))
    gate, R = 13.8, np.zeros((2, 2))
    new, fused = f.join_submap(sub, gate, R, signature_offset=100.0)
    assert new == list(range(N + 1, N + M + 1))
    assert sorted((k, d) for k, d, _ in fused) == [(shared[q] + 1, N + 1 + q) for q in range(4)] and all(d2 <= gate for _, _, d2 in fused)
    assert f._e.N == N + M - 4
    assert f.s.tolist() == list(range(1, N + 1)) + [100.0 + k for k in range(5, M + 1)]     # the kept landmarks keep their signatures
    assert [e[1] for e in f.log.edits] == ["join_map", "merge_batch"]
    f.log.save(tmp_path / "joined.npz")
    assert str(np.load(tmp_path / "joined.npz")["format"]) == FORMAT_JOIN_MAP
    log = TrajectoryLog.load(tmp_path / "joined.npz")
    fresh = J.set_state(engine(**kw), x0, np.arange(1.0, N + 1), P0)
    log.replay(fresh)
    np.testing.assert_array_equal(fresh.get_x(), f.x)
    np.testing.assert_array_equal(fresh.get_s(), f.s)
    np.testing.assert_array_equal(fresh.get_P(), f.P)
    assert np.all(np.isfinite(f.P))


def test_a_float_local_map_replays_bit_for_bit_from_an_f64_scratch_engine(tmp_path):
    from ekf_slam_amd.slam import EKF_SLAM
    from ekf_slam_amd.trajectory import TrajectoryLog
    N, M = 13, 21
    kw = dict(capacity=N + M + 4, tile=16, batch=4)
    x0, s0, P0 = J.random_state(np.random.default_rng(3), N)
    f = EKF_SLAM(**kw)
    f.x = x0; f.s = s0; f.P = P0
    lo, _ = local_pair(M, 3, tile=16, storage="f32")
    f.log = TrajectoryLog()
    f.predict(U2)
    f.log.record(U2, None, [], np.zeros((0, 2)))
    assert f.join_map(lo, 5.0) == list(range(N + 1, N + M + 1))
    f.log.save(tmp_path / "float_local.npz")
    fresh = J.set_state(engine(**kw), x0, s0, P0)
    TrajectoryLog.load(tmp_path / "float_local.npz").replay(fresh)
    np.testing.assert_array_equal(fresh.get_x(), f.x)
    np.testing.assert_array_equal(fresh.get_s(), f.s)
    np.testing.assert_array_equal(fresh.get_P(), f.P)


# ------------------------------------------------------------------------------------------------------------------
# 9. refusals, each with both handles as they were
# ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_both_handles_alone():
    from ekf_slam_amd import _lib as L
    N, M = 20, 6
    x = lowrank_data(N, 5)[0]
    g = loaded(N, 5, capacity=N + M - 1, tile=16, batch=4)   # one landmark short of the local map
    for k in (4, 11):
        g.predict(U2); g.correct(observe(x, k), R2, k)
    lo, _ = local_pair(M, 0, tile=32, storage="f64")
    sharded = loaded(N, 5, capacity=N + M + 4, tile=16, force_sharded=1)
    roomy = loaded(N, 5, capacity=N + M + 4, tile=16)
    before = {id(e): getters(e) for e in (g, lo, sharded, roomy)}
    first = ctypes.c_int64(-7)

    def unchanged(name, *engines):
        for e in engines:
            for got, ref in zip(getters(e), before[id(e)]):  # x, s, P, the diagonal blocks, ekf_P_digest
                np.testing.assert_array_equal(got, ref, err_msg=name)
        assert first.value == -7, name

    bad = L.EKF_ERR_INVALID_ARG
    call = lambda h, l, off=0.0: g.lib.ekf_join_map(h, l, ctypes.c_double(off), ctypes.byref(first))
    assert call(None, lo.h) == bad and call(g.h, None) == bad
    unchanged("NULL", g, lo)
    assert b"join_map" in g.lib.ekf_last_error(g.h)
    assert call(g.h, g.h) == bad; unchanged("self-join", g)
    assert b"itself" in g.lib.ekf_last_error(g.h)
    for off in (float("nan"), float("inf")):
        assert call(roomy.h, lo.h, off) == bad; unchanged("a non-finite offset", roomy, lo)
    assert call(sharded.h, lo.h) == bad; unchanged("a sharded global handle", sharded, lo)
    assert call(roomy.h, sharded.h) == bad; unchanged("a sharded local handle", roomy, sharded)
    assert b"sharded" in roomy.lib.ekf_last_error(roomy.h)
    assert call(g.h, lo.h) == L.EKF_ERR_CAPACITY; unchanged("capacity: all or nothing", g, lo)
    st, msg = status_of(lambda: g.join_map(lo))
    assert st == L.EKF_ERR_CAPACITY and "join_map" in msg and g.N == N
    # the shard group refuses with the library's error
    from ekf_slam_amd.sharding import ShardGroup
    grp = ShardGroup(2, capacity=N + M + 4, tile=16)
    grp.load_lowrank_state(*lowrank_data(N, 5))
    assert status_of(lambda: grp.join_map(lo))[0] == bad and grp.N == N
    grp.close()
    # ... and the handles that were refused go on: the roomy one takes the join
    assert roomy.join_map(lo, 1.0) == N and roomy.N == N + M
