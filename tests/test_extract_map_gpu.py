"""GPU: part of a map taken out into a handle of its own (ekf_extract_map; include/ekfslam.h).

The yardstick is the NumPy restatement of tests/extract_map_cases.py applied to THE STATE A TWIN REPORTED BEFORE THE CALL -- a twin with the
same history, because reading P flushes and the extraction is to meet pending pairs and a recorded predict; stores, tolerances and helpers
are those of tests/helpers.py.  Where two engines hold the same values -- the map frame against a twin that removed the complement, a
shuffled list against an indexing of P, a reused destination against a fresh one, the asynchronous pass and the device-decided loop against
waited twins -- the comparison is assert_array_equal.

N = 140 with T = 16 (8 landmarks per tile row); m = 131 crosses k_extract_state's second workgroup (column 256) and the second 256-landmark
column group of a k_extract_rows row; the T = 256 float store crosses its first tile-row edge at landmark 128."""
import ctypes

import numpy as np
import pytest

import extract_map_cases as X
import join_map_cases as J
from helpers import R2, REL, TOL_KEPT32, TOL_ROW32, TOL_X32, U2, assert_same, blocks_of, check_state, engine, getters, loaded, rel_err, state
from helpers import status_of
from removal_cases import lowrank_data, observe

pytestmark = pytest.mark.gpu
N = 140
SOURCES = [(16, "f64"), (64, "f64"), (16, "f32"), (256, "f32_mixed")]
DESTS = [(32, "f64"), (16, "f32")]
MS = [0, 1, 5, 40, 131]
PLAN_OF = {0: "run", 1: "run", 5: "shuffled", 40: "scattered", 131: "reversed"}


def source_pair(pending=3, n=N, **kw):
    """Two engines with the same state and history: `pending` corrections left in the ring where the batch allows it and a recorded
    predict behind them."""
    x = lowrank_data(n, 5)[0]
    kw.setdefault("batch", 8)
    e, twin = loaded(n, 5, capacity=n + 4, **kw), loaded(n, 5, capacity=n + 4, **kw)
    for q in (e, twin):
        for k in [(5 * j + 1) % n for j in range(pending)]:
            q.predict(U2); q.correct(observe(x, k), R2, k)
        q.predict(U2)
    return e, twin


def plan(m, seed=0):
    return X.PLANS[PLAN_OF.get(m, "shuffled")](N, m, seed)


def check_extracted(d, ex, eP, storage, label, es, frame):
    """helpers.check_state; in the robot frame the robot rows and columns of P are asserted to be exactly zero first, and on a float
    destination the measures of check_state are then taken over the landmark rows (a zero row has no scale to measure against)."""
    if frame == "map" or storage == "f64":
        if frame == "robot":
            assert not d.get_P()[:3, :].any() and not d.get_x()[:3].any()
        with np.errstate(invalid="ignore", divide="ignore"):
            check_state(d, ex, eP, storage, label, es)
        return
    x, s, P = state(d)
    blocks = d.get_P_diag_blocks()
    assert d.N == es.size
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
    err_x, err_b = rel_err(x, ex), rel_err(blocks, blocks_of(eP))
    err_kept = float(np.abs(P - eP)[kept].max() / scale)
    err_row = float((np.abs(P - eP)[3:].max(axis=1) / np.abs(eP)[3:].max(axis=1)).max())
    print("%s [%s]: rel err x %.2e blocks %.2e F64-kept %.2e worst landmark row %.2e" % (label, storage, err_x, err_b, err_kept, err_row))
    assert err_x < TOL_X32 and err_kept < TOL_KEPT32 and err_b < TOL_KEPT32 and err_row <= TOL_ROW32


# ------------------------------------------------------------------------------------------------------------------
# 1. against the dense restatement
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", X.FRAMES)
@pytest.mark.parametrize("dtile,dstorage", DESTS)
@pytest.mark.parametrize("tile,storage", SOURCES)
def test_an_extraction_against_the_dense_restatement(tile, storage, dtile, dstorage, frame):
    turn = SOURCES.index((tile, storage)) + DESTS.index((dtile, dstorage)) + X.FRAMES.index(frame)
    e, twin = source_pair(3, tile=tile, storage=storage)
    assert e.pending() == 3
    x, s, P = state(twin)                                     # (flushes the twin)
    before = getters(twin)
    d = engine(capacity=N, tile=dtile, storage=dstorage)
    for q in range(len(MS)):
        m = MS[(q + turn) % len(MS)]                          # which size meets the pending pairs and the recorded predict rotates
        idx = plan(m, seed=turn)
        ex, es, eP = X.extract_dense(x, s, P, idx, frame)
        assert e.extract_map(idx, frame, into=d) is d
        assert e.pending() == 0 and d.pending() == 0 and d.N == m and e.N == N
        check_extracted(d, ex, eP, dstorage, "%s N=%d m=%d from %s" % (frame, N, m, storage), es, frame)
        assert np.all(np.isfinite(d.get_P()))
        if q == 0:                                            # the source is only flushed: bit for bit the flushed twin
            for got, ref in zip(getters(e), before):
                np.testing.assert_array_equal(got, ref)
    for got, ref in zip(getters(e), before):
        np.testing.assert_array_equal(got, ref)


# ------------------------------------------------------------------------------------------------------------------
# 2. the map frame between stores of one kind: the bits of a twin that removed the complement
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("other_tile", [False, True])
@pytest.mark.parametrize("tile,storage", SOURCES)
def test_the_map_frame_keeps_the_bits_of_a_removal(tile, storage, other_tile):
    dtile = {16: 64, 64: 16, 256: 64}[tile] if other_tile else tile
    # (the F32-arithmetic pass exists for tile edge 256 only: its other edge is a plain float store, the same storage kind)
    kind = dict(storage="f32") if (storage == "f32_mixed" and other_tile) else {}
    for m, which in ((40, "scattered"), (131, "run"), (5, "run")):
        e, twin = source_pair(3, tile=tile, storage=storage)
        idx = X.PLANS[which](N, m, seed=m)
        assert idx == sorted(idx)
        d = e.extract_map(idx, "map", tile=dtile, capacity=m + 3, **kind)        # by default the source's storage kind
        assert d.cfg.storage == e.cfg.storage
        twin.remove_landmarks(X.complement(N, idx))
        assert d.N == twin.N == m
        for name in ("get_x", "get_s", "get_P", "get_P_diag_blocks"):
            np.testing.assert_array_equal(getattr(d, name)(), getattr(twin, name)(), err_msg="%s m=%d" % (name, m))
        for q in (e, twin, d):
            q.close()


# ------------------------------------------------------------------------------------------------------------------
# 3. any order: a shuffled list over the whole map is a permutation of P
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,dtile", [(16, 32), (64, 16)])
def test_a_shuffled_list_over_the_whole_map_permutes_P(tile, dtile):
    e, twin = source_pair(3, tile=tile)
    x, s, P = state(twin)
    perm = [int(i) for i in np.random.default_rng(17).permutation(N)]
    d = e.extract_map(perm, "map", tile=dtile)
    sel = np.concatenate([[0, 1, 2]] + [[3 + 2 * l, 4 + 2 * l] for l in perm]).astype(int)
    np.testing.assert_array_equal(d.get_P(), P[sel][:, sel])
    np.testing.assert_array_equal(d.get_x(), x[sel])
    np.testing.assert_array_equal(d.get_s(), s[perm])
    np.testing.assert_array_equal(d.get_P_diag_blocks(), blocks_of(P[sel][:, sel]))


def test_a_float_store_widens_exactly_and_an_f64_store_is_rounded_once():
    e, twin = source_pair(3, tile=16, storage="f32")
    x, s, P = state(twin)
    idx = plan(40, 2)
    ex, es, eP = X.extract_dense(x, s, P, idx, "map")
    d = e.extract_map(idx, "map", storage="f64", tile=32)
    np.testing.assert_array_equal(d.get_P(), eP)              # float -> F64: exact
    np.testing.assert_array_equal(d.get_x(), ex)
    e2, twin2 = source_pair(3, tile=16, storage="f64")
    x, s, P = state(twin2)
    ex, es, eP = X.extract_dense(x, s, P, idx, "map")
    d2 = e2.extract_map(idx, "map", storage="f32", tile=16)
    got = d2.get_P()
    n = ex.size
    kept = np.zeros((n, n), dtype=bool)
    kept[:3, :] = kept[:, :3] = True
    for a in range(3, n, 2):
        kept[a:a + 2, a:a + 2] = True
    np.testing.assert_array_equal(got[kept], eP[kept])        # the F64-kept parts: exact
    np.testing.assert_array_equal(d2.get_x(), ex)
    np.testing.assert_array_equal(got[~kept], eP[~kept].astype(np.float32).astype(np.float64))        # one rounding per tile entry


# ------------------------------------------------------------------------------------------------------------------
# 4. the robot frame: RELATIVE_XY's own h, and the library's own independent H P H'
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage,dtile", [(16, "f64", 32), (64, "f64", 16), (16, "f32", 32)])
def test_the_robot_frame_is_the_relative_xy_model(tile, storage, dtile):
    from ekf_slam_amd.engine import Engine
    e, twin = source_pair(3, tile=tile, storage=storage)
    x = state(twin)[0]
    Rz = 1e-6 * np.eye(2)
    for m in (1, 5, 32, 131):
        idx = plan(m, seed=4)
        d = e.extract_map(idx, "robot", storage="f64", tile=dtile)
        xd = d.get_x()
        assert not xd[:3].any()
        for k, l in enumerate(idx):
            hx, _ = Engine.model_evaluate(4, x[:3], x[3 + 2 * l:5 + 2 * l], lib=e.lib)
            np.testing.assert_array_equal(xd[3 + 2 * k:5 + 2 * k], hx, err_msg="m=%d k=%d" % (m, k))
        if m <= 32:
            scan = [dict(model=4, z=[0.3 * k, -0.2 * k], R=Rz) for k in range(m)]
            S = e.joint_innovation(scan, [idx], want_prefix=False, want_S=True)["S"][0]
            want = S - np.kron(np.eye(m), Rz)
            got = d.get_P()[3:, 3:]
            err = rel_err(got, want)
            print("%s T=%d m=%d: the landmark block against ekf_joint_innovation's S - R: rel err %.2e" % (storage, tile, m, err))
            assert err < REL
        d.close()


def test_a_landmark_exactly_on_the_robot_is_regular():
    x, s, P = X.scene_on_robot(12, 6, which=4)
    e = J.set_state(engine(capacity=16, tile=16), x, s, P)
    idx = [7, 4, 0]
    d = e.extract_map(idx, "robot")
    ex, es, eP = X.extract_dense(x, s, P, idx, "robot")
    check_extracted(d, ex, eP, "f64", "a landmark on the robot", es, "robot")
    xd = d.get_x()
    assert xd[5] == 0.0 and xd[6] == 0.0 and np.all(np.isfinite(d.get_P()))


# ------------------------------------------------------------------------------------------------------------------
# 5. frame invariance: the distance between two landmarks does not depend on the frame they are expressed in
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", X.FRAMES)
def test_landmark_distances_are_those_of_the_source(frame):
    e, _ = source_pair(3, tile=16)
    idx = plan(40, seed=8)
    d = e.extract_map(idx, frame, tile=32)
    R1 = [[0.05, 0.0], [0.0, 0.0]]
    worst = 0.0
    for k, a in ((0, 39), (39, 0), (5, 2), (17, 18), (30, 11)):
        got = d.model_innovation(5, [3.0], R1, [k, a])
        ref = e.model_innovation(5, [3.0], R1, [idx[k], idx[a]])
        if frame == "map":
            for key in ("nu", "S", "d2"):
                np.testing.assert_array_equal(got[key], ref[key], err_msg="%s (%d, %d)" % (key, k, a))
        else:
            worst = max(worst, np.abs(got["nu"] - ref["nu"]).max() / max(np.abs(ref["nu"]).max(), 1.0), rel_err(got["S"], ref["S"]))
    print("%s frame: the landmark-distance innovation against the source's: worst rel err %.2e" % (frame, worst))
    assert worst < REL


# ------------------------------------------------------------------------------------------------------------------
# 6. refusals, each with both handles as they were
# ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_both_handles_alone():
    from ekf_slam_amd import _lib as L
    n = 20
    x = lowrank_data(n, 5)[0]
    e = loaded(n, 5, capacity=n + 4, tile=16, batch=4)
    for k in (4, 11):
        e.predict(U2); e.correct(observe(x, k), R2, k)
    small = loaded(3, 6, capacity=4, tile=16)
    sharded = loaded(n, 5, capacity=n + 4, tile=16, force_sharded=1)
    roomy = loaded(5, 7, capacity=n + 4, tile=32)
    before = {id(q): getters(q) for q in (e, small, sharded, roomy)}

    def unchanged(name, *engines):
        for q in engines:
            for got, ref in zip(getters(q), before[id(q)]):  # x, s, P, the diagonal blocks, ekf_P_digest
                np.testing.assert_array_equal(got, ref, err_msg=name)

    def call(h, idx, frame, dst, m=None):
        arr = (ctypes.c_int64 * max(len(idx), 1))(*idx)
        return e.lib.ekf_extract_map(h, arr, len(idx) if m is None else m, ctypes.c_int32(frame), dst)

    bad = L.EKF_ERR_INVALID_ARG
    assert call(None, [1], 0, roomy.h) == bad and call(e.h, [1], 0, None) == bad
    unchanged("NULL", e, roomy)
    assert b"extract_map" in e.lib.ekf_last_error(e.h)
    assert call(e.h, [1], 0, e.h) == bad; unchanged("into itself", e)
    assert b"itself" in e.lib.ekf_last_error(e.h)
    assert e.lib.ekf_extract_map(e.h, None, 2, ctypes.c_int32(0), roomy.h) == bad; unchanged("a null list", e, roomy)
    assert call(e.h, [1], 0, roomy.h, m=-1) == bad; unchanged("a negative count", e, roomy)
    assert call(e.h, [3, 7, 3], 0, roomy.h) == bad; unchanged("a landmark named twice", e, roomy)
    assert b"twice" in e.lib.ekf_last_error(e.h)
    for frame in (2, -1):
        assert call(e.h, [1], frame, roomy.h) == bad; unchanged("a frame that is neither", e, roomy)
    assert b"frame" in e.lib.ekf_last_error(e.h)
    assert call(sharded.h, [1], 0, roomy.h) == bad; unchanged("a sharded source", sharded, roomy)
    assert b"sharded" in sharded.lib.ekf_last_error(sharded.h)
    assert call(e.h, [1], 0, sharded.h) == bad; unchanged("a sharded destination", e, sharded)
    assert b"sharded" in e.lib.ekf_last_error(e.h)
    for idx in ([0, n], [-1], [n + 100, 2]):
        assert call(e.h, idx, 1, roomy.h) == L.EKF_ERR_INDEX; unchanged("an index outside the map", e, roomy)
    assert b"index" in e.lib.ekf_last_error(e.h)
    assert call(e.h, [0, 1, 2, 3, 4], 0, small.h) == L.EKF_ERR_CAPACITY; unchanged("capacity: all or nothing", e, small)
    st, msg = status_of(lambda: e.extract_map(range(5), into=small))
    assert st == L.EKF_ERR_CAPACITY and "extract_map" in msg and small.N == 3
    # the shard group refuses with the library's error
    from ekf_slam_amd.sharding import ShardGroup
    grp = ShardGroup(2, capacity=n + 4, tile=16)
    grp.load_lowrank_state(*lowrank_data(n, 5))
    assert status_of(lambda: grp.extract_map([0], "map", roomy))[0] == bad and grp.N == n
    unchanged("a shard group", roomy)
    grp.close()
    # ... and the handles that were refused go on
    assert e.extract_map([0, 1, 2, 3], "robot", into=small) is small and small.N == 4 and e.pending() == 0


# ------------------------------------------------------------------------------------------------------------------
# 7. a destination that is used again keeps nothing of what it held
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", X.FRAMES)
@pytest.mark.parametrize("dtile,dstorage", DESTS)
def test_a_reused_destination_keeps_nothing_of_the_first_extraction(dtile, dstorage, frame):
    e, _ = source_pair(3, tile=16)
    kw = dict(capacity=N, tile=dtile, storage=dstorage, batch=4)
    d = engine(**kw)
    bytes_fresh = d.device_bytes()
    e.extract_map(plan(131, 1), frame, into=d)
    bytes_used = d.device_bytes()
    assert bytes_used - bytes_fresh == 4 * N                  # the index list the destination keeps: capacity int32 entries, allocated once
    xd = d.get_x()
    d.predict(U2); d.correct(observe(xd, 7), R2, 7)          # the destination is in use: a pending pair and a recorded predict, both dropped
    d.predict(U2)
    for m in (5, 0):
        idx = plan(m, 3)
        held = d.device_bytes()
        e.extract_map(idx, frame, into=d)
        assert d.device_bytes() == held
        fresh = e.extract_map(idx, frame, into=engine(**kw))
        assert d.N == m and d.pending() == 0
        assert_same(d, fresh)                                 # x, s, P, the diagonal blocks and the digest of every tile of the active rows


# ------------------------------------------------------------------------------------------------------------------
# 8. what comes out is an ordinary handle: joined into a third one and corrected
# ------------------------------------------------------------------------------------------------------------------
def test_the_extracted_map_is_joined_into_a_third_handle_and_corrected():
    e, _ = source_pair(3, tile=16)
    idx = plan(40, 5)
    lo = e.extract_map(idx, "robot", tile=32)                 # q = 0, PL_qq = 0, PL(q, .) = 0: what join_map expects of a local map
    M, n3 = 40, 13
    kw = dict(capacity=n3 + M + 4, tile=16, batch=4)
    g = loaded(n3, 9, **kw)
    ex, es, eP = J.join_dense(*state(g), *state(lo), 500.0)
    assert g.join_map(lo, 500.0) == n3 and g.N == n3 + M
    check_state(g, ex, eP, "f64", "an extracted map joined into a third handle", es)
    twin = J.set_state(engine(**kw), ex, es, eP)
    x1 = g.get_x()
    for q in (g, twin):
        for k in (4, n3 + 6, n3 + M - 1):
            q.predict(U2); q.correct(observe(x1, k), R2, k)
    check_state(g, *[state(twin)[k] for k in (0, 2)], "f64", "corrections behind that join", state(twin)[1])
    # ... and the map frame goes on as a filter of its own
    sub = e.extract_map(idx, "map", tile=32, batch=4)
    twin2 = J.set_state(engine(capacity=M, tile=32, batch=4), *state(sub))
    x2 = sub.get_x()
    for q in (sub, twin2):
        for k in (0, 17, M - 1):
            q.predict(U2); q.correct(observe(x2, k), R2, k)
        q.remove_landmarks([3])
    check_state(sub, *[state(twin2)[k] for k in (0, 2)], "f64", "corrections and a removal on an extracted map", state(twin2)[1])


# ------------------------------------------------------------------------------------------------------------------
# 9. beside the other machinery
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", X.FRAMES)
def test_beside_an_asynchronous_pass_just_queued(frame):
    x = lowrank_data(N, 5)[0]
    idx = plan(40, 6)
    runs, outs = [], []
    for asy in (True, False):
        e = loaded(N, 5, capacity=N + 4, tile=16, batch=3, async_flush=asy)
        for k in (5, 60, 100):                                # the batch completes: its pass is queued (asynchronous: on the pass stream)
            e.predict(U2); e.correct(observe(x, k), R2, k)
        e.predict(U2); e.correct(observe(x, 7), R2, 7)        # and one pair recorded behind it
        outs.append(e.extract_map(idx, frame, tile=32))
        assert e.pending() == 0
        x1 = e.get_x()
        for k in (3, 9, N - 1):
            e.predict(U2); e.correct(observe(x1, k), R2, k)
        runs.append(e)
    assert_same(outs[0], outs[1])
    assert_same(runs[0], runs[1])


def test_behind_an_unsettled_scan_of_the_device_decided_loop():
    from decided_plans import PARAMS, make_plan
    from ekf_slam_amd.engine import Engine
    scans = make_plan(7, 300, 12, 8)
    runs, outs = [], []
    for mode in (4, 1):
        e = Engine(mode="uc", capacity=300, device_assoc=mode, tile=16, batch=4, **PARAMS)
        for t, (u, rows, ix, loc) in enumerate(scans):
            e.predict(u)
            e.measure(rows, u, ix, loc)
            if t == 8:                                        # straight behind the scan: with device_assoc = 4 nothing of it is settled
                outs.append(e.extract_map([5, 0, 3], "robot", mode="known", tile=32))
        runs.append(e)
    assert outs[0].N == outs[1].N == 3 and runs[0].N == runs[1].N
    assert_same(outs[0], outs[1])
    assert_same(runs[0], runs[1])
