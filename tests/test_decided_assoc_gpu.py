"""GPU: the device-decided branch (cfg.device_assoc = 4, include/ekfslam.h) -- EKF_SLAM_UC.m's measure loop with ANY w_pos, the
association evaluated, decided AND carried out on the device (k_gather<.., kDecide>: correction, append or nothing), the host
queueing a whole scan without a wait.  Held to the waited mode (device_assoc = 1) bit for bit with F64 tiles, to DESIGN.md
section 5's tolerances with float tiles, to the same error at the same row, and to the structured oracle."""
import os
import time

import numpy as np
import pytest

from decided_plans import PARAMS, make_plan, oracle_run
from helpers import REL, rel_err

pytestmark = pytest.mark.gpu


def engine(device_assoc, capacity, **kw):
    from ekf_slam_amd.engine import Engine
    p = dict(PARAMS)
    p.update(kw)
    return Engine(mode="uc", capacity=capacity, device_assoc=device_assoc, **p)


def drive(e, plan):
    for u, rows, idx, loc in plan:
        e.predict(u)
        e.measure(rows, u, idx, loc)


def assert_same(a, b):
    assert a.N == b.N
    np.testing.assert_array_equal(a.get_x(), b.get_x())
    np.testing.assert_array_equal(a.get_s(), b.get_s())
    np.testing.assert_array_equal(a.get_P(), b.get_P())


@pytest.mark.parametrize("tile", [16, 64, 128])
@pytest.mark.parametrize("batch,asy", [(1, False), (8, False), (32, False), (8, True), (32, True)])
def test_bitwise_against_the_waited_mode(tile, batch, asy, oracle_lib):
    from oracle.ekf_structured import StructuredEKF
    plan = make_plan(7, 400, 30, 8)
    ref = StructuredEKF(400, "uc", Rc=PARAMS["Rc"], w_pos=1.0, s_thresh=PARAMS["s_thresh"])
    differ = oracle_run(ref, plan)
    assert differ >= 10                      # rows a signature-only prediction would get wrong
    dec = engine(4, 400, tile=tile, batch=batch, async_flush=asy)
    wai = engine(1, 400, tile=tile, batch=batch, async_flush=asy)
    drive(dec, plan)
    drive(wai, plan)
    assert_same(dec, wai)
    assert dec.N == ref.N
    assert rel_err(dec.get_x(), ref.x) < REL and rel_err(dec.get_P(), ref.P) < REL
    np.testing.assert_array_equal(dec.get_s(), ref.s)


@pytest.mark.parametrize("batch", [1, 8])
def test_signature_only_likelihood_matches_the_device_resident_loop(batch):
    plan = make_plan(11, 300, 25, 8)
    dec = engine(4, 300, tile=64, batch=batch, w_pos=0.0, s_thresh=1e9)
    loop = engine(3, 300, tile=64, batch=batch, w_pos=0.0, s_thresh=1e9)
    drive(dec, plan)
    drive(loop, plan)
    assert_same(dec, loop)


@pytest.mark.parametrize("storage", ["f32", "f32_mixed", "f32_split"])
def test_float_tiles(storage):
    # float tiles against the F64 engine, relative to the largest entry
    plan = make_plan(13, 400, 30, 8)
    f = engine(4, 400, tile=256, storage=storage, batch=32)
    d64 = engine(4, 400, tile=128, batch=32)
    w = engine(1, 400, tile=256, storage=storage, batch=32)
    for e in (f, d64, w):
        drive(e, plan)
    assert f.N == d64.N == w.N
    np.testing.assert_array_equal(f.get_s(), d64.get_s())
    for other in (d64, w):
        assert rel_err(f.get_x(), other.get_x()) < 1e-5
        assert rel_err(f.get_P(), other.get_P()) < 1e-5


def _scan_at(e, ks, new_sigs, pose=None):
    """Rows observing filter landmarks ks (exact geometry from the filter's x) then rows with signatures no landmark carries."""
    x = e.get_x()
    rows = []
    for k in ks:
        dx, dy = x[3 + 2 * k] - x[0], x[4 + 2 * k] - x[1]
        b = (np.degrees(np.arctan2(dy, dx)) - x[2]) % 360.0
        rows.append((np.hypot(dx, dy) + 0.01, b + 0.2, float(k + 1)))
    for sgn in new_sigs:
        rows.append((3.0, 45.0, float(sgn)))
    return np.array(rows, dtype=np.float64)


def _loaded(device_assoc, N, capacity, seed=3, **kw):
    rng = np.random.default_rng(seed)
    n = 3 + 2 * N
    x = np.concatenate([[0.1, -0.2, 10.0], rng.uniform(-20, 20, 2 * N)])
    s = np.arange(1, N + 1, dtype=np.float64)
    d = np.concatenate([[0.01, 0.01, 0.001], rng.uniform(0.05, 0.2, 2 * N)])
    U = rng.normal(0.0, 0.02, (n, 3))
    e = engine(device_assoc, capacity, **kw)
    e.load_lowrank_state(x, s, d, U)
    return e


def test_no_wait_inside_measure():
    """ekf_measure queues the whole scan and returns while a spin kernel still holds the stream; the waited mode cannot."""
    import torch
    N = 1000
    dec = _loaded(4, N, N + 64, batch=8)
    wai = _loaded(1, N, N + 64, batch=8)
    s = torch.cuda.Stream()                  # (not the null stream: ekf_set_stream(NULL) means the handle's own stream)
    torch.cuda.set_stream(s)
    for e in (dec, wai):
        e.set_stream(s.cuda_stream)
    lm_index = np.arange(1, N + 65, dtype=np.float64)
    lm_loc = np.random.default_rng(5).uniform(-20, 20, (N + 64, 2))
    u = np.array([0.1, 1.0])
    warm = _scan_at(dec, [3, 17], [9e6])
    for e in (dec, wai):
        e.predict(u); e.measure(warm, u, lm_index, lm_loc)
    torch.cuda.synchronize()
    scan = _scan_at(dec, [5, 400, 999, 42, 7], [8e6, 7e6, 6e6])    # corrections and appends
    assert len(scan) == 8
    # a bounded spin of at least 100 ms, calibrated with events
    cycles = 1 << 22
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); torch.cuda._sleep(cycles); b.record(); b.synchronize()
        if a.elapsed_time(b) >= 100.0:
            gate = a.elapsed_time(b) / 1000.0
            break
        cycles *= 2
    times = {}
    for name, e in (("dec", dec), ("wai", wai)):
        e.predict(u)
        torch.cuda._sleep(cycles)
        t0 = time.perf_counter()
        e.measure(scan, u, lm_index, lm_loc)
        times[name] = time.perf_counter() - t0
        torch.cuda.synchronize()
    torch.cuda.set_stream(torch.cuda.default_stream())
    assert times["dec"] < gate / 4, (times, gate)
    assert times["wai"] >= 0.75 * gate, (times, gate)      # sensitivity: the waited mode does wait
    assert dec.N == wai.N and dec.N > N + 1
    assert_same(dec, wai)


def _err_status(fn):
    from ekf_slam_amd._lib import EkfError
    try:
        fn()
    except EkfError as ex:
        return ex.status
    return 0


def test_errors_and_settling(tmp_path):
    from ekf_slam_amd import _lib as L
    u = np.array([0.1, 1.0])
    # capacity exhausted in the middle of a scan
    a, b = _loaded(4, 40, 42, batch=8), _loaded(1, 40, 42, batch=8)
    idx = np.arange(1, 60, dtype=np.float64)
    loc = np.random.default_rng(1).uniform(-20, 20, (59, 2))
    scan = _scan_at(a, [1, 2], [5e6, 6e6, 7e6])
    st = [_err_status(lambda e=e: (e.predict(u), e.measure(scan, u, idx, loc))) for e in (a, b)]
    assert st[0] == st[1] == L.EKF_ERR_CAPACITY
    assert_same(a, b)
    # a landmark-list key missing in the middle of a scan
    a, b = _loaded(4, 40, 80, batch=8), _loaded(1, 40, 80, batch=8)
    idx = np.array([41.0, 43.0]); loc = np.array([[1.0, 2.0], [3.0, 4.0]])
    scan = _scan_at(a, [1], [5e6, 6e6, 7e6])
    st = [_err_status(lambda e=e: (e.predict(u), e.measure(scan, u, idx, loc))) for e in (a, b)]
    assert st[0] == st[1] == L.EKF_ERR_LOOKUP
    assert_same(a, b)
    # the empty map (EKF_SLAM_UC.m:110-111: the list must hold one non-zero index, so an append after the first row cannot
    # resolve its key -- whatever happens, it happens alike)
    a, b = engine(4, 20, s_thresh=1e9), engine(1, 20, s_thresh=1e9)
    scan = np.array([[2.0, 10.0, 1.0], [2.0, 10.0, 1.0], [3.0, 50.0, 1.0]])
    st = [_err_status(lambda e=e: (e.predict(u), e.measure(scan, u, np.array([0.0, 1.0]), np.array([[9.0, 9.0], [1.5, 0.5]]))))
          for e in (a, b)]
    assert st[0] == st[1] == 0
    assert a.N == 1
    assert_same(a, b)
    a, b = engine(4, 20), engine(1, 20)
    st = [_err_status(lambda e=e: (e.predict(u), e.measure(scan, u, np.array([1.0]), np.array([[1.5, 0.5]])))) for e in (a, b)]
    assert st[0] == st[1]
    assert_same(a, b)
    # every other entry point sees the settled state
    a, b = _loaded(4, 60, 200, batch=8), _loaded(1, 60, 200, batch=8)
    idx = np.arange(1, 201, dtype=np.float64)
    loc = np.random.default_rng(2).uniform(-20, 20, (200, 2))
    scan = _scan_at(a, [4, 9, 33], [5e6, 6e6, 61.0])
    for e in (a, b):
        e.predict(u); e.measure(scan, u, idx, loc)
    assert a.N == b.N
    np.testing.assert_array_equal(a.get_P_diag_blocks(), b.get_P_diag_blocks())
    np.testing.assert_array_equal(a.digest(), b.digest())
    assert_same(a, b)
    for e in (a, b):
        e.predict(u); e.measure(scan, u, idx, loc)
    pa, pb = str(tmp_path / "a.ckpt"), str(tmp_path / "b.ckpt")
    a.checkpoint_save(pa); b.checkpoint_save(pb)
    assert open(pa, "rb").read() == open(pb, "rb").read()
    for e in (a, b):
        e.predict(u); e.measure(scan, u, idx, loc)
        e.append(u, np.diag([0.1, 0.2]), [1.0, 2.0], 77.0)
        e.predict(u); e.measure(scan, u, idx, loc)
        e.correct([3.0, 40.0], np.diag([0.1, 0.2]), 2)
        e.set_params(w_pos=0.0)
        e.predict(u); e.measure(scan, u, idx, loc)
        e.set_params(w_pos=1.0)
        e.predict(u); e.measure(scan, u, idx, loc)
    assert_same(a, b)
    for e in (a, b):
        e.checkpoint_load(pa)
        e.predict(u); e.measure(scan, u, idx, loc)
    assert_same(a, b)


def test_at_size_appends_beside_the_pass():
    """~20 000 landmarks, F64, asynchronous pass, batch 32: device-decided appends cross a tile-row edge while a pass is in flight."""
    N0 = 20030                     # 2 N0 = 40060: the tile row of edge 128 ends at 40064, two appends later
    cap = N0 + 64
    dec = _loaded(4, N0, cap, batch=32, async_flush=True)
    syn = _loaded(1, N0, cap, batch=32)
    idx = np.arange(1, cap + 1, dtype=np.float64)
    loc = np.random.default_rng(9).uniform(-20, 20, (cap, 2))
    u = np.array([0.1, 1.0])
    rng = np.random.default_rng(4)
    scans = [_scan_at(dec, list(rng.integers(0, N0, 8)), []) for _ in range(4)]          # 32 corrections: the pass starts
    scans.append(_scan_at(dec, [N0 - 1, 12], [5e6, 6e6, 7e6, 8e6]))                       # appends beside it, across the edge
    scans.append(_scan_at(dec, [N0 - 5], [4e6]) )
    for rows in scans:
        for e in (dec, syn):
            e.predict(u); e.measure(rows, u, idx, loc)
    follow = _scan_at(syn, [N0, N0 + 1, N0 + 2, 30], [3e6])                              # corrections of the appended landmarks
    for e in (dec, syn):
        e.predict(u); e.measure(follow, u, idx, loc)
    assert dec.N == syn.N and dec.N >= N0 + 4
    np.testing.assert_array_equal(dec.get_x(), syn.get_x())
    np.testing.assert_array_equal(dec.get_s(), syn.get_s())
    np.testing.assert_array_equal(dec.digest(), syn.digest())
    np.testing.assert_array_equal(dec.get_P_diag_blocks(), syn.get_P_diag_blocks())
    n = 3 + 2 * dec.N
    r0 = 2 * N0 - 8
    np.testing.assert_array_equal(dec.get_P_block(r0, 0, n - r0, n), syn.get_P_block(r0, 0, n - r0, n))


@pytest.mark.parametrize("kw", [dict(world=2, rank=0), dict(force_sharded=1)])
def test_sharded_configurations_are_refused(kw):
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd._lib import EkfError
    with pytest.raises(EkfError) as ex:
        engine(4, 64, **kw)
    assert ex.value.status == L.EKF_ERR_INVALID_ARG
