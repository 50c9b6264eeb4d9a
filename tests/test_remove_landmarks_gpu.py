"""GPU: landmark removal on the device (ekf_remove_landmarks, include/ekfslam.h).

Marginalising landmarks out of the filter is an order-preserving compaction of x, s and the tiled P with no arithmetic, so the
yardstick is numpy.delete and the comparison is assert_array_equal -- for float tiles too.  What is checked: the state right after
the call (every storage kind, removal sets that hit tile edges), the call with corrections pending and a predict still lazy, the
engine's life afterwards against a twin that was GIVEN the expected state, the association on the renumbered map in every
device_assoc mode, the structured oracle, the refusals, a checkpoint, and two states at benchmark size against low-rank-loaded
twins (k_lowrank_tiles forms every entry from its own two rows of U: the twin without those rows holds the survivors' bits)."""
import ctypes

import numpy as np
import pytest

from decided_plans import PARAMS
from helpers import R2, REL, STORES_ALL, U2, assert_same, engine, loaded, rel_err, run_ops, state, status_of
from removal_cases import expected_after, lowrank_data, lowrank_minus, observe, removal_sets

pytestmark = pytest.mark.gpu
N0 = 300
SET_NAMES = ["first", "last", "middle", "adjacent_over_tile_edge", "whole_tile_row", "every_second", "random_tenth", "all"]


# ------------------------------------------------------------------------------------------------------------------
# 1. bit for bit against numpy.delete
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage", STORES_ALL)
@pytest.mark.parametrize("name", SET_NAMES)
def test_bit_for_bit_against_numpy_delete(tile, storage, name):
    idx = removal_sets(N0, tile, 11)[name]
    e = loaded(N0, 5, capacity=N0 + 8, tile=tile, storage=storage)
    x0, s0, P0 = state(e)
    blocks0 = e.get_P_diag_blocks()
    ex, es, eP = expected_after(x0, s0, P0, idx)
    e.remove_landmarks(idx)
    assert e.N == N0 - len(idx) and e.pending() == 0
    np.testing.assert_array_equal(e.get_x(), ex)
    np.testing.assert_array_equal(e.get_s(), es)
    np.testing.assert_array_equal(e.get_P(), eP)
    np.testing.assert_array_equal(e.get_P_diag_blocks(), np.delete(blocks0, 1 + np.asarray(sorted(idx)), axis=0))
    # the premise of the tests at size: a handle low-rank-loaded WITHOUT the removed rows holds the survivors' bits
    x, s, d, U = lowrank_data(N0, 5)
    twin = engine(capacity=N0 + 8, tile=tile, storage=storage)
    twin.load_lowrank_state(*lowrank_minus(x, s, d, U, idx))
    assert_same(e, twin)
    # ... and a second removal on the same handle (the stores have swapped once by now) is as exact as the first
    if e.N > 40:
        again = [int(e.N) - 1, 0, 17, 18]
        ex, es, eP = expected_after(ex, es, eP, again)
        e.remove_landmarks(again)
        np.testing.assert_array_equal(e.get_x(), ex)
        np.testing.assert_array_equal(e.get_s(), es)
        np.testing.assert_array_equal(e.get_P(), eP)


def test_a_lone_shard_with_the_sharded_code_path_simply_works():
    """world == 1 with cfg.force_sharded owns every tile: the removal works, and the sharded correction (row-panel extraction ->
    exchange, here ekf_exchange_local over the one handle -> gather) goes on from the compacted store like an unsharded twin."""
    idx = removal_sets(N0, 64, 11)["random_tenth"]
    e = loaded(N0, 5, capacity=N0 + 8, tile=64, force_sharded=1)
    ex, es, eP = expected_after(*state(e), idx)
    e.remove_landmarks(idx)
    np.testing.assert_array_equal(e.get_P(), eP)
    twin = engine(capacity=N0 + 8, tile=64)
    twin.set_state(ex, eP, es)
    harr = (ctypes.c_void_p * 1)(e.h)
    for k in (3, 200, 269):
        z = observe(ex, k)
        e.predict(U2); twin.predict(U2)
        e.correct_begin(z, R2, k)
        assert e.lib.ekf_exchange_local(harr, 1) == 0
        e.correct_finish()
        twin.correct(z, R2, k)
    assert_same(e, twin)


# ------------------------------------------------------------------------------------------------------------------
# 2. with work pending
# ------------------------------------------------------------------------------------------------------------------
def _pending_calls(e, mode, x, idx):
    """5 corrections recorded, a predict still lazy, then the removal."""
    ks = [7, 150, 151, 299, 42]
    if mode == "known":
        for k in ks:
            e.predict(U2); e.correct(observe(x, k), R2, k)
    else:
        rows = np.array([list(observe(x, k)) + [float(k + 1)] for k in ks])
        lm_index = np.arange(1, N0 + 9, dtype=np.float64)
        lm_loc = np.random.default_rng(1).uniform(-20, 20, (N0 + 8, 2))
        e.predict(U2); e.measure(rows, U2, lm_index, lm_loc)
    e.predict(np.array([0.2, -2.0]))
    e.remove_landmarks(idx)


@pytest.mark.parametrize("mode", ["known", "uc"])
@pytest.mark.parametrize("batch,asy", [(8, False), (32, False), (8, True), (32, True)])
def test_with_corrections_pending_and_a_lazy_predict(mode, batch, asy):
    idx = [150, 3, 298, 64, 63]                      # one of them was corrected a moment ago
    x = lowrank_data(N0, 5)[0]
    d = loaded(N0, 5, mode, capacity=N0 + 8, tile=64, batch=batch, async_flush=asy)
    one = loaded(N0, 5, mode, capacity=N0 + 8, tile=64, batch=1)
    _pending_calls(d, mode, x, idx)
    _pending_calls(one, mode, x, idx)
    assert d.pending() == 0 and d.N == N0 - len(idx)
    assert_same(d, one)
    for q in (d, one):                               # and the next corrections see the same state
        for k in (0, 149, 294):
            q.predict(U2); q.correct(observe(q.get_x(), k), R2, k)
    assert_same(d, one)


# ------------------------------------------------------------------------------------------------------------------
# 3. the engine goes on correctly
# ------------------------------------------------------------------------------------------------------------------
def _continuation(ex, es, tile, batch, capacity, removed):
    """Operations (pure function of the expected state): appends that cross a tile-row edge, measure() scans with corrections on both
    sides of the removed landmarks and new landmarks, two full batches of corrections."""
    N = es.size
    per_row = tile // 2
    ops = []
    n_app = per_row - N % per_row + 3
    assert N + n_app + 8 <= capacity
    rng = np.random.default_rng(2)
    for i in range(n_app):
        ops.append(("append", rng.uniform(-20, 20, 2), 5000.0 + i))
    lo, hi = min(removed), max(removed) - len(removed)       # new indices just below / at the first and last hole
    near = sorted({max(lo - 1, 0), min(lo, N - 1), max(hi, 0), min(hi + 1, N - 1), 1, N - 2})
    lm_index = np.arange(1, capacity + 1, dtype=np.float64)
    lm_loc = np.random.default_rng(3).uniform(-20, 20, (capacity, 2))
    for t in range(3):
        rows = [list(observe(ex, k, dr=0.01 * (t + 1))) + [float(es[k])] for k in near[t::2] + near[:2]]
        rows.append([3.0 + t, 45.0, 9e6 + t])                # matches no signature: appended (EKF_SLAM_UC.m:121-123)
        ops.append(("measure", np.array(rows), lm_index, lm_loc))
    for i in range(2 * batch):
        k = near[i % len(near)] if i % 3 else int(rng.integers(0, N))
        ops.append(("correct", observe(ex, k, dr=0.02), k))
    return ops


@pytest.mark.parametrize("tile,storage,batch,asy", [(16, "f64", 8, False), (64, "f64", 8, True), (128, "f64", 32, False),
                                                    (256, "f32", 8, False), (256, "f32_mixed", 8, False), (256, "f32_mixed", 64, True),
                                                    (256, "f32_split", 32, False)])
@pytest.mark.parametrize("which", ["random_tenth", "adjacent_over_tile_edge"])
def test_the_engine_goes_on_like_a_twin_given_the_expected_state(tile, storage, batch, asy, which):
    cap = N0 + 160
    idx = removal_sets(N0, tile, 11)[which]
    kw = dict(capacity=cap, tile=tile, storage=storage, batch=batch, async_flush=asy)
    e = loaded(N0, 5, "uc", **kw)
    for k in (5, 120, 290):                                  # some history first, so that P is not the loaded one
        e.predict(U2); e.correct(observe(e.get_x(), k), R2, k)
    ex, es, eP = expected_after(*state(e), idx)
    e.remove_landmarks(idx)
    twin = engine("uc", **kw)
    twin.set_state(ex, eP, es)
    ops = _continuation(ex, es, tile, batch, cap, idx)
    run_ops(e, ops)
    run_ops(twin, ops)
    assert e.N == twin.N and e.N > es.size + 3
    if storage != "f64":
        # DESIGN.md section 5's tolerances at the least (x, F64-kept entries; float-stored entries against the row's largest) ...
        assert rel_err(e.get_x(), twin.get_x()) < 1e-9 + 2e-12 * len(ops)
        Pe, Pt = e.get_P(), twin.get_P()
        assert float((np.abs(Pe - Pt).max(axis=1) / np.abs(Pt).max(axis=1)).max()) <= 2e-7
    # ... and in fact the same bits: the expected state survives the F64 round trip of ekf_set_P exactly, and nothing else differs
    assert_same(e, twin)


# ------------------------------------------------------------------------------------------------------------------
# 4. association sees the new map
# ------------------------------------------------------------------------------------------------------------------
K_GONE = 100


def _assoc_run(device_assoc, params, early):
    cap = N0 + 40
    e = loaded(N0, 3, "uc", capacity=cap, tile=64, batch=8, device_assoc=device_assoc, **params)
    lm_index = np.arange(1, cap + 1, dtype=np.float64)
    lm_loc = np.random.default_rng(5).uniform(-20, 20, (cap, 2))
    if early:
        # a scan that appends: with device_assoc = 4 its rows are queued and nothing is settled when the removal arrives
        e.predict(U2)
        x0 = e.get_x()                                       # (the pose the scan is taken from: the position cost is strict)
        rows = np.array([list(observe(x0, 9)) + [10.0], [3.0, 45.0, 7e6], [4.0, 50.0, 8e6], list(observe(x0, 250)) + [251.0]])
        e.measure(rows, U2, lm_index, lm_loc)
    e.remove_landmarks([K_GONE])
    N = e.N
    x, s = e.get_x(), e.get_s()
    assert s[K_GONE] == K_GONE + 2.0                         # old landmark K_GONE + 1 moved down
    z = np.array(list(observe(x, K_GONE)) + [s[K_GONE]])
    Rz = np.diag([z[0] * e.cfg.Rc[0], z[1] * e.cfg.Rc[1]])
    is_new, got = e.associate(z, Rz)
    assert (is_new, got) == (False, K_GONE)
    # a scan: old landmark K_GONE + 1, a row with the removed landmark's signature, two more landmarks on either side
    gone = [2.5, 30.0, float(K_GONE + 1)] if params.get("w_pos", 0.0) == 0.0 else [2.5, 30.0, 6e6]
    e.predict(U2)
    x = e.get_x()
    rows = np.array([list(observe(x, K_GONE)) + [s[K_GONE]], gone, list(observe(x, 5)) + [s[5]], list(observe(x, 270)) + [s[270]]])
    e.measure(rows, U2, lm_index, lm_loc)
    assert e.N == N + 1                                      # the removed landmark's signature matches nothing: appended as new
    return e


@pytest.mark.parametrize("early", [False, True])
def test_association_sees_the_new_map_signature_only(early):
    params = dict(w_pos=0.0)
    runs = {m: _assoc_run(m, params, early) for m in (0, 1, 2, 3)}
    for m in (0, 2, 3):
        assert_same(runs[m], runs[1])
    assert runs[1].get_s()[-1] == runs[1].N                  # the reference's convention: signature N + 1 at the time of the append


@pytest.mark.parametrize("early", [False, True])
def test_association_sees_the_new_map_position_weighted(early):
    runs = {m: _assoc_run(m, PARAMS, early) for m in (0, 1, 4)}
    for m in (0, 4):                                         # mode 4 with `early`: the removal arrives on unsettled rows
        assert_same(runs[m], runs[1])


# ------------------------------------------------------------------------------------------------------------------
# 5. against the oracle
# ------------------------------------------------------------------------------------------------------------------
def test_against_the_structured_oracle(oracle_lib):
    from oracle.ekf_structured import StructuredEKF
    cap = 120
    ref = StructuredEKF(cap, "uc")
    e = engine("uc", capacity=cap, tile=16, batch=4)
    rng = np.random.default_rng(8)
    pos = rng.uniform(-15, 15, (cap, 2))

    def both(fn):
        fn(ref); fn(e)

    def step(k_obs, sig):
        """predict, then one row of EKF_SLAM_UC.measure by hand on both: associate -> append | correct (1-based on the oracle)."""
        u = np.array([0.1, 2.0])
        both(lambda q: q.predict(u))
        xr = ref.x
        z = np.array(list(observe(xr, k_obs)) + [sig]) if k_obs is not None else np.array([4.0, 33.0, sig])
        Rz = np.diag([z[0] * 0.1, z[1] * 5.0])
        new_r, idx_r = ref.associate(z, Rz)
        new_e, idx_e = e.associate(z, Rz)
        assert (new_r, idx_r) == (new_e, idx_e + 1)
        if new_r:
            ref.append(u, Rz, pos[ref.N], idx_r); e.append(u, Rz, pos[e.N], idx_e + 1)
        else:
            ref.correct(z, Rz, idx_r); e.correct(z, Rz, idx_e)

    for i in range(60):                                      # 60 landmarks with signatures 10, 20, ...
        both(lambda q: q.predict(U2))
        both(lambda q: q.append(U2, R2, pos[i], 10.0 * (i + 1)))
    for k in (3, 30, 59, 17, 44):
        step(k, 10.0 * (k + 1))
    idx = [40, 3, 17, 18, 59]
    rx, rs, rP = expected_after(ref.x, ref.s, ref.P, idx)     # the oracle as it is: it is GIVEN numpy.delete of its own state
    ref.set_state(rx, rP, rs)
    e.remove_landmarks(idx)
    assert e.N == ref.N == 55
    np.testing.assert_array_equal(e.get_s(), ref.s)
    assert rel_err(e.get_x(), ref.x) < REL and rel_err(e.get_P(), ref.P) < REL
    s_now = ref.s
    for k in (0, 2, 3, 15, 16, 38, 54):                      # survivors on both sides of every hole, by their kept signatures
        step(k, float(s_now[k]))
    step(None, 180.0)                                        # the signature of removed landmark 17 (0-based): a new landmark now
    step(None, 7777.0)
    for i in range(12):                                      # growth across tile rows of edge 16
        both(lambda q: q.predict(U2))
        both(lambda q: q.append(U2, R2, pos[60 + i], 900.0 + i))
    for k in (56, 60, 1, 68):
        step(k, float(ref.s[k]))
    assert e.N == ref.N == 69
    np.testing.assert_array_equal(e.get_s(), ref.s)
    ex, eP = rel_err(e.get_x(), ref.x), rel_err(e.get_P(), ref.P)
    print("oracle: rel err x %.2e P %.2e" % (ex, eP))
    assert ex < REL and eP < REL


# ------------------------------------------------------------------------------------------------------------------
# 6. errors leave the state alone
# ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_state_alone():
    from ekf_slam_amd import _lib as L
    e = loaded(N0, 5, capacity=N0 + 8, tile=64, batch=8)
    twin = loaded(N0, 5, capacity=N0 + 8, tile=64, batch=8)
    x = lowrank_data(N0, 5)[0]
    for q in (e, twin):
        for k in (4, 77, 200):
            q.predict(U2); q.correct(observe(x, k), R2, k)
    assert e.pending() == 3
    e.remove_landmarks([])                                   # m = 0: EKF_OK, nothing happens -- not even a flush
    assert e.pending() == 3 and e.N == N0
    dg, x_before = e.digest(), e.get_x()
    twin.digest()
    i64 = lambda *v: (ctypes.c_int64 * len(v))(*v)
    cases = [("duplicate", i64(3, 9, 3), 3, L.EKF_ERR_INVALID_ARG), ("null", None, 2, L.EKF_ERR_INVALID_ARG),
             ("negative count", i64(1), -1, L.EKF_ERR_INVALID_ARG), ("-1", i64(5, -1), 2, L.EKF_ERR_INDEX),
             ("N", i64(N0, 2), 2, L.EKF_ERR_INDEX)]
    for name, arr, m, want in cases:
        rc = e.lib.ekf_remove_landmarks(e.h, arr, m)
        assert rc == want, name
        assert b"remove_landmarks" in e.lib.ekf_last_error(e.h), name
        assert e.N == N0
        np.testing.assert_array_equal(e.digest(), dg)
        np.testing.assert_array_equal(e.get_x(), x_before)
    for q in (e, twin):
        q.predict(U2); q.correct(observe(x, 9), R2, 9)
    assert_same(e, twin)
    # sharded handles: refused, and the message says why
    sh = engine(capacity=64, tile=16, world=2, rank=0)
    st, msg = status_of(lambda: sh.remove_landmarks([0]))
    assert st == L.EKF_ERR_INVALID_ARG and "shard" in msg
    sh.remove_landmarks([])                                  # nothing to do is no error anywhere


def test_the_second_store_is_counted_and_kept():
    e = loaded(N0, 5, capacity=N0 + 8, tile=64)
    a = loaded(N0, 5, capacity=N0 + 8, tile=64, batch=4, async_flush=True)
    b0, a0 = e.device_bytes(), a.device_bytes()
    e.remove_landmarks([5]); a.remove_landmarks([5])
    nt = (2 * (N0 + 8) + 63) // 64
    store = nt * (nt + 1) // 2 * 64 * 64 * 8
    assert e.device_bytes() - b0 >= store                    # allocated at the first removal, reported
    assert a.device_bytes() - a0 < store                     # cfg.async_flush: the second store was there already
    b1 = e.device_bytes()
    e.remove_landmarks([7, 200])
    assert e.device_bytes() == b1                            # ... and kept


# ------------------------------------------------------------------------------------------------------------------
# 7. checkpoint
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage", [(64, "f64"), (256, "f32_mixed")])
def test_checkpoint_after_a_removal(tile, storage, tmp_path):
    cap = N0 + 160
    idx = removal_sets(N0, tile, 11)["random_tenth"]
    kw = dict(capacity=cap, tile=tile, storage=storage, batch=8)
    e = loaded(N0, 5, "uc", **kw)
    ex, es, eP = expected_after(*state(e), idx)
    e.remove_landmarks(idx)
    path = str(tmp_path / "after_removal.ckpt")
    e.checkpoint_save(path)
    fresh = engine("uc", **kw)
    fresh.checkpoint_load(path)
    np.testing.assert_array_equal(fresh.get_P(), eP)
    ops = _continuation(ex, es, tile, 8, cap, idx)
    run_ops(e, ops)
    run_ops(fresh, ops)
    assert_same(e, fresh)


# ------------------------------------------------------------------------------------------------------------------
# 8. at size
# ------------------------------------------------------------------------------------------------------------------
def _at_size(N, idx, corrections, **kw):
    x, s, d, U = lowrank_data(N, 21)
    e = engine(capacity=N, **kw)
    e.load_lowrank_state(x, s, d, U)
    e.remove_landmarks(idx)
    x2, s2, d2, U2m = lowrank_minus(x, s, d, U, idx)
    twin = engine(capacity=N, **kw)
    twin.load_lowrank_state(x2, s2, d2, U2m)
    M = N - len(idx)
    n = 3 + 2 * M
    assert e.N == twin.N == M
    np.testing.assert_array_equal(e.get_x(), x2)
    np.testing.assert_array_equal(e.get_s(), s2)
    np.testing.assert_array_equal(e.digest(), twin.digest())
    np.testing.assert_array_equal(e.get_P_diag_blocks(), twin.get_P_diag_blocks())
    np.testing.assert_array_equal(e.get_P_block(0, 0, 3, n), twin.get_P_block(0, 0, 3, n))
    for q, i in enumerate(sorted(idx)):                      # the rows around every hole, full width
        r0 = min(max(3 + 2 * (i - q) - 4, 0), n - 8)
        np.testing.assert_array_equal(e.get_P_block(r0, 0, 8, n), twin.get_P_block(r0, 0, 8, n))
    rng = np.random.default_rng(4)
    near = [max(i - q - 1, 0) for q, i in enumerate(sorted(idx))]
    for t in range(corrections):
        k = near[t % len(near)] if t % 2 else int(rng.integers(0, M))
        z = observe(x2, k)
        for q in (e, twin):
            q.predict(U2); q.correct(z, R2, k)
    np.testing.assert_array_equal(e.get_x(), twin.get_x())
    np.testing.assert_array_equal(e.digest(), twin.digest())
    np.testing.assert_array_equal(e.get_P_diag_blocks(), twin.get_P_diag_blocks())
    e.close(); twin.close()


def test_at_size_ten_thousand_landmarks_f64():
    N = 10000
    idx = [int(i) for i in np.linspace(37, N - 41, 16)]
    _at_size(N, idx[::-1], 40, tile=128, batch=20)


def test_at_size_twenty_thousand_landmarks_f32_mixed_loses_a_tile_row():
    N = 20000                                                # 40 000 rows: 157 tile rows of edge 256, the last one 64 rows deep
    idx = [int(i) for i in np.linspace(11, N - 3, 40)]       # 40 landmarks fewer: 39 920 rows fit 156 tile rows
    assert (2 * N + 255) // 256 == 157 and (2 * (N - len(idx)) + 255) // 256 == 156
    _at_size(N, idx, 128, tile=256, storage="f32_mixed", batch=64)
