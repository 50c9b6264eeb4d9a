"""GPU: a batch of landmark fusions in one call (ekf_merge_landmarks_batch; include/ekfslam.h).

The definition is the yardstick: the call leaves what ekf_constrain_landmarks pair by pair in list order, then ONE
ekf_remove_landmarks of all drops would leave.  With F64 tiles that is checked with assert_array_equal against a twin that makes
exactly those public calls; in every storage kind against tests/merge_batch_cases.merge_batch_dense applied to the state the engine
reported before the call, by the ONE-step tolerances of tests/helpers.py (the batch rounds a float entry once).

Float contingency (the bounds are not loosened): where a float bound does not hold on these inputs the bar is
max(bound, 2 x the error the sequential route measures on the same inputs); both routes' errors are printed."""
import ctypes

import numpy as np
import pytest

from helpers import R2, REL, RPOS, STORES_ALL, TOL_KEPT32, TOL_ROW32, TOL_X32, U2, assert_same, blocks_of, engine, loaded, rel_err, run_ops, state, status_of
from merge_batch_cases import MERGE_BATCH_MAX, chain_regularity, dense_of, merge_batch_dense, nearest_dense, planted, survivor_index
from merge_cases import Factored, continuation, tile_edge_landmark
from removal_cases import lowrank_data, observe

pytestmark = pytest.mark.gpu
N0 = 300
SEED = 7
FUSED = "k_merge_pass"


def planted_engine(mode="known", **kw):
    x, s, d, U, pairs = planted(N0, SEED)
    e = engine(mode, **kw)
    e.load_lowrank_state(x, s, d, U)
    return e, pairs


def history(e, ks=(5, 120, 290)):
    """some corrections first, so that P is not the loaded one"""
    for k in ks:
        e.predict(U2); e.correct(observe(e.get_x(), k), R2, k)


def sequence(e, pairs, R):
    """the definition, through the existing public calls; returns the d2 read in front of each constraint"""
    d2 = []
    for keep, drop in pairs:
        d2.append(e.landmark_distance(keep, drop, None, R)[0])
        e.constrain_landmarks(keep, drop, None, R)
    e.remove_landmarks([d for _, d in pairs])
    return np.array(d2)


def regular_on_the_numpy_side(e, pairs, R, floor=1e-3):
    x, _, P = state(e)
    worst, d2 = chain_regularity(x, P, pairs, R)
    assert worst > floor and np.isfinite(d2).all(), (worst, d2)


# ------------------------------------------------------------------------------------------------------------------
# 1. F64: the same bits as the sequence of public calls
# ------------------------------------------------------------------------------------------------------------------
def _bit_cases(T):
    edge = tile_edge_landmark(T, N0)
    pl = planted(N0, SEED)[4]
    used = {v for p in pl for v in p}
    extra_keeps = [k for k in range(0, N0 // 2) if k not in used][:16]
    extra_drops = [d for d in range(N0 // 2, N0) if d not in used][:16]
    return {"one": ([(edge + 1, edge + 2)], RPOS),
            "shared_keep": ([pl[0], pl[14], pl[1], pl[15]], None),
            "keep_lt_and_gt_drop": ([(10, 200), (250, 20), (21, 22), (31, 30)], RPOS),
            "drops_first_and_last": ([(5, 0), (6, N0 - 1)], None),
            "adjacent_over_a_tile_edge": ([(edge, edge - 1), (edge + 1, edge + 2)], RPOS),
            "sixteen": (pl, None),
            "the_maximum": (pl + list(zip(extra_keeps, extra_drops)), RPOS)}


@pytest.mark.parametrize("tile", [16, 64, 128])
@pytest.mark.parametrize("name", ["one", "shared_keep", "keep_lt_and_gt_drop", "drops_first_and_last", "adjacent_over_a_tile_edge", "sixteen",
                                  "the_maximum"])
def test_f64_the_batch_is_the_sequence_bit_for_bit(tile, name):
    pairs, R = _bit_cases(tile)[name]
    assert name != "the_maximum" or len(pairs) == MERGE_BATCH_MAX
    kw = dict(capacity=N0 + 8, tile=tile, batch=4)
    a, _ = planted_engine(**kw)
    b, _ = planted_engine(**kw)
    for q in (a, b):
        history(q)
    regular_on_the_numpy_side(a, pairs, R)
    s0 = a.get_s()
    got = a.merge_landmarks_batch(pairs, R)
    want = sequence(b, pairs, R)
    assert a.pending() == 0 and a.N == N0 - len(pairs)
    assert_same(a, b)
    np.testing.assert_array_equal(got, want)
    for keep, _ in pairs:                                    # every keep survives, with its signature, at keep - #{drop < keep}
        assert a.get_s()[survivor_index(pairs, keep)] == s0[keep]
    if len(pairs) == 1:
        c, _ = planted_engine(**kw)
        history(c)
        c.merge_landmarks(pairs[0][0], pairs[0][1], R)
        assert_same(a, c)
    history(a, (3, 100, 200)); history(b, (3, 100, 200))     # and both go on alike
    assert_same(a, b)


# ------------------------------------------------------------------------------------------------------------------
# 2. one fused pass, no compaction, m gathers
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage", [(64, "f64"), (128, "f64"), (256, "f32"), (64, "f32")])
@pytest.mark.parametrize("m", [1, 5, 16])
def test_the_batch_is_m_gathers_and_one_fused_pass(tile, storage, m):
    from ekf_slam_amd import _lib as L
    e, pairs = planted_engine(capacity=N0 + 8, tile=tile, storage=storage)
    history(e)
    e.sync()
    for which in (L.EKF_KERNEL_DOWNDATE, L.EKF_KERNEL_COMPACT, L.EKF_KERNEL_GATHER):
        e.timing_enable(which, True, 64)
    e.merge_landmarks_batch(pairs[:m], RPOS)
    assert e.timing_read(L.EKF_KERNEL_DOWNDATE)[0] == 1
    assert e.timing_read(L.EKF_KERNEL_COMPACT)[0] == 0
    assert e.timing_read(L.EKF_KERNEL_GATHER)[0] == m
    name, npairs = e.downdate_kernel_name()
    assert name.startswith(FUSED) and npairs == m, (name, npairs)


# ------------------------------------------------------------------------------------------------------------------
# 3. every store against the dense restatement
# ------------------------------------------------------------------------------------------------------------------
def _errors(e, ex, es, eP):
    x, s, P = state(e)
    blocks = e.get_P_diag_blocks()
    assert e.N == es.size
    np.testing.assert_array_equal(s, es)
    np.testing.assert_array_equal(P, P.T)
    n = ex.size
    kept = np.zeros((n, n), dtype=bool)                      # what float handles keep in F64
    kept[:3, :] = kept[:, :3] = True
    for a in range(3, n, 2):
        kept[a:a + 2, a:a + 2] = True
    return {"x": rel_err(x, ex), "P": rel_err(P, eP), "blocks": rel_err(blocks, blocks_of(eP)),
            "kept": float(np.abs(P - eP)[kept].max() / np.abs(eP).max()),
            "row": float((np.abs(P - eP).max(axis=1) / np.abs(eP).max(axis=1)).max())}


@pytest.mark.parametrize("tile,storage", STORES_ALL)
@pytest.mark.parametrize("rname", ["R0", "Rpos"])
def test_every_store_against_the_dense_restatement(tile, storage, rname):
    R = None if rname == "R0" else RPOS
    kw = dict(capacity=N0 + 8, tile=tile, storage=storage, batch=8)
    e, pairs = planted_engine(**kw)
    twin, _ = planted_engine(**kw)
    for q in (e, twin):
        history(q)
    x0, s0, P0 = state(e)
    worst, d2_np = chain_regularity(x0, P0, pairs, R)
    assert worst > 1e-3 and d2_np.max() < 0.1                # the reference route stays regular on these inputs
    ex, es, eP, want_d2 = merge_batch_dense(x0, s0, P0, pairs, R)
    assert np.linalg.eigvalsh(eP).min() > 1e-4
    got_d2 = e.merge_landmarks_batch(pairs, R)
    sequence(twin, pairs, R)
    err, seq = _errors(e, ex, es, eP), _errors(twin, ex, es, eP)
    err["d2"] = float(np.abs(got_d2 - want_d2).max() / want_d2.max())
    print("batch of %d, %s [%s]: " % (len(pairs), rname, storage) + ", ".join("%s %.2e (sequence %.2e)" % (k, v, seq.get(k, np.nan)) for k, v in err.items()))
    if storage == "f64":
        assert err["x"] < REL and err["P"] < REL and err["blocks"] < REL and err["d2"] < REL
    else:
        bar = lambda bound, key: max(bound, 2.0 * seq[key])
        assert err["x"] < bar(TOL_X32, "x") and err["kept"] < bar(TOL_KEPT32, "kept") and err["blocks"] < bar(TOL_KEPT32, "blocks")
        assert err["row"] <= bar(TOL_ROW32, "row")
        assert err["d2"] < TOL_ROW32 * 10                    # S is formed in F64 from float-rounded entries both sides read alike


@pytest.mark.parametrize("tile", [16, 64, 128])
def test_small_float_tiles_against_the_dense_restatement(tile):
    """Float tiles of edge 16 .. 128 (a lane's 16 bytes cover two landmarks of a narrower row; not among the stores above): the same
    check with the same one-step bounds and the same contingency."""
    test_every_store_against_the_dense_restatement(tile, "f32", "Rpos")


# ------------------------------------------------------------------------------------------------------------------
# 4. whatever is in front of the call
# ------------------------------------------------------------------------------------------------------------------
def _front(e, x, mode):
    """5 corrections recorded and a predict still lazy"""
    ks = [7, 150, 151, 299, 42]
    if mode == "known":
        for k in ks:
            e.predict(U2); e.correct(observe(x, k), R2, k)
    else:
        rows = np.array([list(observe(x, k)) + [float(k + 1)] for k in ks] + [[3.0, 45.0, 7e6], [4.0, 50.0, 8e6]])
        lm_index = np.arange(1, N0 + 41, dtype=np.float64)
        lm_loc = np.random.default_rng(1).uniform(-20, 20, (N0 + 40, 2))
        e.predict(U2); e.measure(rows, U2, lm_index, lm_loc)
    e.predict(np.array([0.2, -2.0]))


@pytest.mark.parametrize("mode,batch,asy,device_assoc", [("known", 8, False, None), ("known", 32, False, None), ("known", 8, True, None),
                                                         ("known", 32, True, None), ("uc", 8, False, 3), ("uc", 8, False, 4), ("uc", 32, True, 4)])
def test_pending_work_in_front_of_the_call_is_settled_first(mode, batch, asy, device_assoc):
    kw = dict(capacity=N0 + 40, tile=64, batch=batch, async_flush=asy)
    if device_assoc is not None:
        kw["device_assoc"] = device_assoc
    if device_assoc == 4:
        kw.update(w_pos=1.0, Rc=(0.01, 0.01), s_thresh=0.5)
    d, pairs = planted_engine(mode, **kw)
    twin, _ = planted_engine(mode, **kw)
    x = planted(N0, SEED)[0]
    _front(d, x, mode)
    _front(twin, x, mode)
    twin.flush(); twin.sync(); twin.get_x(); twin.digest()   # the twin synchronises first: nothing is pending, the predict is carried out
    assert twin.pending() == 0
    got = d.merge_landmarks_batch(pairs, RPOS)
    want = twin.merge_landmarks_batch(pairs, RPOS)
    assert d.pending() == 0 and d.N == twin.N
    assert_same(d, twin)
    np.testing.assert_array_equal(got, want)
    for q in (d, twin):
        for k in (0, 149, 270):
            q.predict(U2); q.correct(observe(q.get_x(), k), R2, k)
    assert_same(d, twin)


# ------------------------------------------------------------------------------------------------------------------
# 5. the engine goes on like a twin that was given the expected state
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage,batch,asy", [(16, "f64", 8, False), (64, "f64", 8, True), (128, "f64", 32, False),
                                                    (256, "f32", 8, False), (256, "f32_mixed", 64, True), (256, "f32_split", 32, False)])
def test_the_engine_goes_on_like_a_twin_given_the_expected_state(tile, storage, batch, asy):
    cap = N0 + 160
    kw = dict(capacity=cap, tile=tile, storage=storage, batch=batch, async_flush=asy)
    e, pairs = planted_engine("uc", **kw)
    history(e)
    e.merge_landmarks_batch(pairs, RPOS)
    ex, es, eP = state(e)
    twin = engine("uc", **kw)
    twin.set_state(ex, eP, es)
    ops = continuation(ex, es, tile, batch, cap, survivor_index(pairs, pairs[3][1]))      # appends over a tile-row edge, UC scans, corrections
    run_ops(e, ops)
    run_ops(twin, ops)
    assert e.N == twin.N and e.N > es.size + 3
    if storage == "f64":
        assert_same(e, twin)
    else:
        assert rel_err(e.get_x(), twin.get_x()) < 1e-9 + 2e-12 * len(ops)
        Pe, Pt = e.get_P(), twin.get_P()
        assert float((np.abs(Pe - Pt).max(axis=1) / np.abs(Pt).max(axis=1)).max()) <= TOL_ROW32
        assert rel_err(e.get_P_diag_blocks(), twin.get_P_diag_blocks()) < 2e-9 + 6e-12 * len(ops)


# ------------------------------------------------------------------------------------------------------------------
# 6. refusals
# ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_state_alone():
    from ekf_slam_amd import _lib as L
    e, pairs = planted_engine(capacity=N0 + 8, tile=64, batch=8)
    twin, _ = planted_engine(capacity=N0 + 8, tile=64, batch=8)
    x = planted(N0, SEED)[0]
    for q in (e, twin):
        for k in (4, 77, 200):
            q.predict(U2); q.correct(observe(x, k), R2, k)
    assert e.pending() == 3
    dg, x_before, s_before, P_before = e.digest(), e.get_x(), e.get_s(), e.get_P()
    twin.digest()
    i64 = lambda *v: (ctypes.c_int64 * len(v))(*v)
    dp = lambda *v: (ctypes.c_double * len(v))(*v)
    ok_R = dp(0.02, 0.005, 0.005, 0.03)
    many = list(range(MERGE_BATCH_MAX + 1))
    cases = [("m < 0", i64(1), i64(2), -1, ok_R, L.EKF_ERR_INVALID_ARG),
             ("m > max", i64(*many), i64(*[v + 100 for v in many]), MERGE_BATCH_MAX + 1, ok_R, L.EKF_ERR_INVALID_ARG),
             ("keep NULL", None, i64(2), 1, ok_R, L.EKF_ERR_INVALID_ARG), ("drop NULL", i64(1), None, 1, ok_R, L.EKF_ERR_INVALID_ARG),
             ("keep == drop", i64(1, 5), i64(2, 5), 2, ok_R, L.EKF_ERR_INVALID_ARG),
             ("a drop twice", i64(1, 3), i64(7, 7), 2, ok_R, L.EKF_ERR_INVALID_ARG),
             ("a keep that is dropped", i64(1, 7), i64(7, 9), 2, ok_R, L.EKF_ERR_INVALID_ARG),
             ("inf R", i64(1), i64(2), 1, dp(float("inf"), 0.0, 0.0, 1.0), L.EKF_ERR_INVALID_ARG),
             ("asymmetric R", i64(1), i64(2), 1, dp(1.0, 0.1, 0.2, 1.0), L.EKF_ERR_INVALID_ARG),
             ("negative determinant", i64(1), i64(2), 1, dp(1.0, 2.0, 2.0, 1.0), L.EKF_ERR_INVALID_ARG),
             ("-1", i64(1, -1), i64(2, 3), 2, ok_R, L.EKF_ERR_INDEX), ("N", i64(1, 4), i64(2, N0), 2, ok_R, L.EKF_ERR_INDEX)]
    d2 = dp(*([-1.0] * (MERGE_BATCH_MAX + 1)))
    for name, keep, drop, m, R, want in cases:
        assert e.lib.ekf_merge_landmarks_batch(e.h, keep, drop, m, R, d2) == want, name
        assert b"merge_landmarks_batch" in e.lib.ekf_last_error(e.h), name
        assert e.N == N0, name
        np.testing.assert_array_equal(e.digest(), dg)
        np.testing.assert_array_equal(e.get_x(), x_before)
        np.testing.assert_array_equal(e.get_s(), s_before)
        np.testing.assert_array_equal(e.get_P(), P_before)
    assert e.lib.ekf_merge_landmarks_batch(e.h, None, None, 0, ok_R, None) == L.EKF_OK      # m == 0: nothing happens
    assert e.N == N0
    np.testing.assert_array_equal(e.digest(), dg)
    assert list(d2) == [-1.0] * (MERGE_BATCH_MAX + 1)
    # the handle is usable: the same batch on both
    for q in (e, twin):
        q.predict(U2); q.correct(observe(x, 9), R2, 9)
        q.merge_landmarks_batch(pairs[:4], RPOS)
    assert_same(e, twin)
    # sharded handles: refused, and the message says why
    sh = engine(capacity=64, tile=16, world=2, rank=0)
    st, msg = status_of(lambda: sh.merge_landmarks_batch([(0, 1)]))
    assert st == L.EKF_ERR_INVALID_ARG and "shard" in msg


def test_a_lone_shard_works_and_refuses_between_begin_and_finish():
    from ekf_slam_amd import _lib as L
    e, pairs = planted_engine(capacity=N0 + 8, tile=64, force_sharded=1)
    twin, _ = planted_engine(capacity=N0 + 8, tile=64)
    harr = (ctypes.c_void_p * 1)(e.h)

    def corrections(ks, refused=False):
        for k in ks:
            z = observe(twin.get_x(), k)
            e.predict(U2); twin.predict(U2)
            e.correct_begin(z, R2, k)
            if refused:                                      # between begin and finish: EKF_ERR_STATE, and nothing changes
                st, msg = status_of(lambda: e.merge_landmarks_batch(pairs, RPOS))
                assert st == L.EKF_ERR_STATE and "merge_landmarks_batch" in msg and "begin and finish" in msg, msg
                assert e.N == N0
            assert e.lib.ekf_exchange_local(harr, 1) == 0
            e.correct_finish()
            twin.correct(z, R2, k)

    corrections((3, 30, 269), refused=True)
    assert_same(e, twin)                                     # the refused calls left x, s, P, the blocks and the digest alone
    got, want = e.merge_landmarks_batch(pairs, RPOS), twin.merge_landmarks_batch(pairs, RPOS)
    np.testing.assert_array_equal(got, want)
    assert_same(e, twin)
    corrections((3, 200, 30, 249, 250))
    assert_same(e, twin)


# ------------------------------------------------------------------------------------------------------------------
# 7. an irregular pair in the middle: all or nothing
# ------------------------------------------------------------------------------------------------------------------
def test_an_irregular_pair_in_the_middle_leaves_the_state_as_it_was():
    """Two perfectly correlated identical landmarks with R = 0 give S = 0 exactly -- third of four pairs.  The two pairs in front
    of it lie above both landmarks, so that they change the rows of the identical pair in identical ways."""
    from ekf_slam_amd import _lib as L
    e = loaded(N0, 5, capacity=N0 + 8, tile=64, batch=8)
    twin = engine(capacity=N0 + 8, tile=64, batch=8)
    x, s, P = state(e)
    a, b = 3 + 2 * 10, 3 + 2 * 200
    x[b:b + 2] = x[a:a + 2]
    P[b:b + 2, :] = P[a:a + 2, :]
    P[:, b:b + 2] = P[:, a:a + 2]
    P[b:b + 2, b:b + 2] = P[a:a + 2, a:a + 2]
    for q in (e, twin):
        q.set_state(x, P, s)
    x0, s0, P0 = state(e)
    dg, b0 = e.digest(), e.get_P_diag_blocks()
    twin.digest()
    bad = [(210, 220), (230, 240), (10, 200), (250, 260)]
    st, msg = status_of(lambda: e.merge_landmarks_batch(bad, None))
    assert st == L.EKF_ERR_STATE and "merge_landmarks_batch" in msg and "pair 2" in msg, msg
    assert e.N == N0 and e.pending() == 0
    np.testing.assert_array_equal(e.get_x(), x0)
    np.testing.assert_array_equal(e.get_s(), s0)
    np.testing.assert_array_equal(e.get_P(), P0)
    np.testing.assert_array_equal(e.get_P_diag_blocks(), b0)
    np.testing.assert_array_equal(e.digest(), dg)
    # the handle goes on: a valid batch (the same pairs with R > 0 are regular) equals the sequence on the twin
    got = e.merge_landmarks_batch(bad, RPOS)
    want = sequence(twin, bad, RPOS)
    np.testing.assert_array_equal(got, want)
    assert got[2] == 0.0                                     # nu = 0 for the identical pair
    assert_same(e, twin)


# ------------------------------------------------------------------------------------------------------------------
# 8. memory
# ------------------------------------------------------------------------------------------------------------------
def test_device_bytes_grow_at_the_first_batch_call_only():
    e, pairs = planted_engine(capacity=N0 + 8, tile=64)
    b0 = e.device_bytes()
    e.merge_landmarks_batch(pairs[:3], RPOS)
    b1 = e.device_bytes()
    ldm = 64 * -(-(2 * (N0 + 8)) // 64)
    assert b1 - b0 >= 2 * MERGE_BATCH_MAX * 2 * ldm * 8      # at least the private ring: G and K slots of 2 ldm doubles
    e.merge_landmarks_batch([(survivor_index(pairs[:3], k), survivor_index(pairs[:3], d)) for k, d in pairs[3:6]], RPOS)
    assert e.device_bytes() == b1


# ------------------------------------------------------------------------------------------------------------------
# 9. checkpoint, 10. replay
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage", [(64, "f64"), (256, "f32_mixed")])
def test_checkpoint_after_a_batch(tile, storage, tmp_path):
    cap = N0 + 160
    kw = dict(capacity=cap, tile=tile, storage=storage, batch=8)
    e, pairs = planted_engine("uc", **kw)
    e.merge_landmarks_batch(pairs, RPOS)
    ex, es, eP = state(e)
    path = str(tmp_path / "after_batch.ckpt")
    e.checkpoint_save(path)
    fresh = engine("uc", **kw)
    fresh.checkpoint_load(path)
    np.testing.assert_array_equal(fresh.get_P(), eP)
    ops = continuation(ex, es, tile, 8, cap, 100)
    run_ops(e, ops)
    run_ops(fresh, ops)
    assert_same(e, fresh)


@pytest.mark.parametrize("tile,storage", [(16, "f64"), (256, "f32")])
def test_a_run_with_a_batch_replays_from_its_log(tile, storage, tmp_path):
    from ekf_slam_amd.slam import SLAM
    from ekf_slam_amd.trajectory import FORMAT_BATCH, TrajectoryLog
    from ekf_slam_amd.world import make_run
    _, run = make_run(40, 11, 24, policy="nearest", m=6)
    run = list(run)
    kw = dict(capacity=64, tile=tile, storage=storage, batch=4)
    full = SLAM('EKF_SLAM', feed=run, landmark_method='SYNTHETIC', **kw)
    full.slam.log = TrajectoryLog()
    for k in range(len(run)):
        full.runSlam()
    N = full.slam._e.N                                       # the batch after the last step: it is replayed behind it
    assert N >= 8
    d2 = full.slam.merge_landmarks_batch([(3, N - 2), (5, 4), (3, N)], np.diag([1.0, 1.0]))
    assert d2.shape == (3,) and full.slam._e.N == N - 3
    path = tmp_path / "batch_run.npz"
    full.slam.log.save(path)
    log = TrajectoryLog.load(path)
    assert str(np.load(path)["format"]) == FORMAT_BATCH and [(e[0], e[1]) for e in log.edits] == [(len(run), "merge_batch")]
    fresh = engine(**kw)
    log.replay(fresh)
    np.testing.assert_array_equal(fresh.get_x(), full.slam.x)
    np.testing.assert_array_equal(fresh.get_s(), full.slam.s)
    np.testing.assert_array_equal(fresh.get_P(), full.slam.P)


# ------------------------------------------------------------------------------------------------------------------
# 11. the policy on top
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage", [(64, "f64"), (256, "f32_mixed")])
def test_fuse_duplicates_batched_removes_the_planted_duplicates(tile, storage):
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd.slam import EKF_SLAM
    from ekf_slam_amd.trajectory import TrajectoryLog
    x, s, d, U, pairs = planted(N0, SEED)
    gate = 0.1
    nd2, _ = nearest_dense(x, dense_of(d, U), RPOS)          # on the NumPy side first: the gate separates the planted rows from the rest
    assert sorted(int(i) for i in np.nonzero(nd2 <= gate)[0]) == sorted(dr for _, dr in pairs) and nd2[nd2 > gate].min() > 1.5 * gate
    f = EKF_SLAM(capacity=N0 + 8, tile=tile, storage=storage)
    f._e.load_lowrank_state(x, s, d, U)
    f.log = TrajectoryLog()
    x0, s0, P0 = state(f._e)
    f._e.sync()
    f._e.timing_enable(L.EKF_KERNEL_ASSOCIATE, True, 64)
    merges = f.fuse_duplicates_batched(gate, RPOS)
    searches = f._e.timing_read(L.EKF_KERNEL_ASSOCIATE)[0]
    assert len(merges) == len(pairs) and f._e.N == N0 - len(pairs)
    assert 0 < searches < len(merges), searches
    np.testing.assert_array_equal(f.s, np.delete(s0, [dr for _, dr in pairs]))      # exactly the planted landmarks are gone
    # the state: merge_batch_dense replaying the batches as the log recorded them (1-based there)
    ex, es, eP, k = x0, s0, P0, 0
    for _, kind, idx, _, R in f.log.edits:
        assert kind == "merge_batch"
        batch = [(int(a) - 1, int(b) - 1) for a, b in zip(idx[0::2], idx[1::2])]
        assert [(kp - 1, dr - 1) for kp, dr, _ in merges[k:k + len(batch)]] == batch
        ex, es, eP, d2 = merge_batch_dense(ex, es, eP, batch, R)
        got = np.array([m[2] for m in merges[k:k + len(batch)]])
        assert np.abs(got - d2).max() / d2.max() < (REL if storage == "f64" else 10 * TOL_ROW32)
        k += len(batch)
    assert k == len(merges)
    err = _errors(f._e, ex, es, eP)
    print("fuse_duplicates_batched [%s]: %d merges in %d batches, %d searches; " % (storage, len(merges), len(f.log.edits), searches)
          + ", ".join("%s %.2e" % kv for kv in err.items()))
    if storage == "f64":
        assert err["x"] < REL and err["P"] < REL and err["blocks"] < REL
    else:                                                    # two batches: two roundings of a float entry
        assert err["x"] < 2 * TOL_X32 and err["kept"] < 2 * TOL_KEPT32 and err["blocks"] < 2 * TOL_KEPT32 and err["row"] <= 2 * TOL_ROW32


# ------------------------------------------------------------------------------------------------------------------
# 12. at size
# ------------------------------------------------------------------------------------------------------------------
def _at_size(N, storage, m, **kw):
    x, s, d, U = lowrank_data(N, 21)
    rng = np.random.default_rng(6)
    pairs = [(40 + 101 * k, N // 2 + 1 + 37 * k) for k in range(m - 2)] + [(40, N - 1), (N - 2, 0)]       # a shared keep; keep > drop; both ends
    x = np.array(x)
    for k, (kp, dr) in enumerate(pairs):
        x[3 + 2 * dr:5 + 2 * dr] = x[3 + 2 * kp:5 + 2 * kp] + np.array([0.05, -0.03]) * (1.0 + 0.1 * k)
    e = engine(capacity=N, storage=storage, **kw)
    e.load_lowrank_state(x, s, d, U)
    f = Factored(x, d, U)
    want_d2 = np.array([f.constrain(kp, dr, None, RPOS)[0] for kp, dr in pairs])
    f.remove([dr for _, dr in pairs])
    got_d2 = e.merge_landmarks_batch(pairs, RPOS)
    M, n = N - m, 3 + 2 * (N - m)
    assert e.N == M and e.pending() == 0
    f64 = storage == "f64"
    tol_x, tol_kept, tol_row = (REL, REL, REL) if f64 else (TOL_X32, TOL_KEPT32, TOL_ROW32)
    errs = {"d2": float(np.abs(got_d2 - want_d2).max() / want_d2.max()), "x": rel_err(e.get_x(), f.x),
            "blocks": rel_err(e.get_P_diag_blocks(), f.diag_blocks()), "robot rows": rel_err(e.get_P_block(0, 0, 3, n), f.rows(0, 3))}
    np.testing.assert_array_equal(e.get_s(), np.delete(s, [dr for _, dr in pairs]))
    rows = [3 + 2 * survivor_index(pairs, kp) for kp, _ in pairs[:4]] + [3 + 2 * survivor_index(pairs, N - 2)]
    for r in rows + [int(v) for v in rng.integers(3, n - 8, 3)]:
        r0 = min(max(r - 3, 0), n - 8)
        got, want = e.get_P_block(r0, 0, 8, n), f.rows(r0, 8)
        errs["rows %d" % r0] = float((np.abs(got - want).max(axis=1) / np.abs(want).max(axis=1)).max())
    tr, sq = f.trace_and_squares()
    dg = e.digest()
    errs["trace"], errs["sum of squares"] = abs(dg[0] - tr) / tr, abs(dg[2] - sq) / sq
    print("at size N = %d [%s], %d pairs, d2 <= %.3f: " % (N, storage, m, want_d2.max()) + ", ".join("%s %.2e" % kv for kv in errs.items()))
    assert errs["d2"] < (REL if f64 else TOL_ROW32) and errs["x"] < tol_x and errs["blocks"] < tol_kept and errs["robot rows"] < tol_kept
    assert all(v <= tol_row for k, v in errs.items() if k.startswith("rows "))
    assert errs["trace"] < tol_kept and errs["sum of squares"] < tol_row
    if f64:                                                  # and the sequence of public calls leaves the same bits here too
        twin = engine(capacity=N, storage=storage, **kw)
        twin.load_lowrank_state(x, s, d, U)
        np.testing.assert_array_equal(sequence(twin, pairs, RPOS), got_d2)
        np.testing.assert_array_equal(e.get_x(), twin.get_x())
        np.testing.assert_array_equal(e.digest(), twin.digest())
        np.testing.assert_array_equal(e.get_P_diag_blocks(), twin.get_P_diag_blocks())
        twin.close()
    e.close()


def test_at_size_ten_thousand_landmarks_f64():
    _at_size(10000, "f64", 16, tile=128, batch=20)


def test_at_size_twenty_thousand_landmarks_f32_mixed():
    _at_size(20000, "f32_mixed", 16, tile=256, batch=64)
