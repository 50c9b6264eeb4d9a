"""GPU: the in-place pass over P leaves out the work items of padding rows (PassJob::live_rows: k_downdate, k_downdate_w and
k_flush_mfma neither load nor store an item whose first row lies at or beyond 2 * landmarks).  K is zero there, so nothing may change:

  * F64 tiles: the one-pair kernel (batch 1) and the deferred pass (batch 4: k_flush_mfma at tile 128, k_downdate_w<..,true> at tile 64)
    stay bit-equal on maps WITH padding, and both follow the CPU oracle at tests/test_deferred_gpu.py's bar (helpers.REL);
  * the bound moves with the map: appends that cross a slab edge and a tile-row edge, an in-place pass between them;
  * float tiles with F64 pass arithmetic against the oracle at tests/test_f32_mixed_gpu.py's bars (1e-6 on x and on P: helpers.REL);
  * the asynchronous pass writes a second store and takes no bound: bit-equal to the synchronous engine with an append beside the pass.

Shapes (landmark-block rows 2N against tile edges 64 and 128, and 32 for the generic k_downdate with its 16-row slabs):
  N = 69 -> 138 rows: at tile 64 ten live rows in the last tile row, the one-pair kernel's 8-row slab at row 136 straddles the bound; at tile
            128 (and at tile 256 with float tiles) one 64-row k_flush_mfma item straddles it and one is wholly dead; at tile 32 one slab
            straddles and one is dead.
  N = 64 -> 128 rows: no padding with any of the edges, the bound equals the tile edge.
  N = 65 -> 130 rows: two live rows in the last tile row.
  N = 25 -> 50 rows: the smallest map the pass kernels see at batch 1 -- up to 24 landmarks (48 rows) do_correct takes the fused small-map
            form (k_gather<.., fused downdate>), which has no pass."""
import numpy as np
import pytest

from helpers import REL, rel_err

pytestmark = pytest.mark.gpu

SHAPES = [69, 64, 65, 25]
STEPS = 12


def _state(N, seed):
    rng = np.random.default_rng(seed)
    n = 3 + 2 * N
    x = np.concatenate([[0.3, -0.2, 40.0], rng.uniform(-20, 20, size=2 * N)])
    U = rng.normal(0, 0.05, size=(n, 6))
    return x, np.diag(rng.uniform(0.01, 0.1, size=n)) + U @ U.T, np.arange(1, N + 1.0)


def _steps(engines, ref, steps, seed):
    """`steps` seeded predict + correct steps on every engine (0-based landmark) and on the oracle (1-based)"""
    rng = np.random.default_rng(seed)
    for _ in range(steps):
        u = [0.1, 3.0]
        idx0 = int(rng.integers(0, engines[0].N))
        z = [rng.uniform(1, 30), rng.uniform(1, 359)]
        R = np.diag([z[0] * .01, z[1] * 5.0])
        for e in engines:
            e.predict(u); e.correct(z, R, idx0)
        ref.predict(u); ref.correct(z, R, idx0 + 1)


def _whole(e):
    """x, the whole P, and the landmark block with the robot strip beside it read as one block"""
    n = e.n
    return e.get_x(), e.get_P(), e.get_P_block(3, 0, n - 3, n)


def _assert_bit_equal(a, b):
    for ga, gb in zip(_whole(a), _whole(b)):
        assert ga.tobytes() == gb.tobytes()


@pytest.mark.parametrize("tile", [32, 64, 128])
@pytest.mark.parametrize("N", SHAPES)
def test_one_pair_and_deferred_pass_agree_bitwise_on_padded_maps(N, tile, oracle_lib):
    from ekf_slam_amd import Engine
    from oracle.ekf_structured import StructuredEKF
    x, P, s = _state(N, 100 + N)
    one = Engine(capacity=N, tile=tile, batch=1)
    dfr = Engine(capacity=N, tile=tile, batch=4)
    ref = StructuredEKF(N, "known")
    for e in (one, dfr, ref):
        e.set_state(x, P, s)
    _steps([one, dfr], ref, STEPS, N)
    assert one.downdate_kernel_name()[0].startswith("k_downdate<double,32,16>" if tile == 32 else "k_downdate_w<double,%d," % tile), \
        one.downdate_kernel_name()
    want = {32: "k_downdate<double,32,16>", 64: "k_downdate_w<double,64,64,true>", 128: "k_flush_mfma<double,128,"}[tile]
    assert dfr.downdate_kernel_name() == (dfr.downdate_kernel_name()[0], 4) and dfr.downdate_kernel_name()[0].startswith(want), \
        dfr.downdate_kernel_name()
    _assert_bit_equal(one, dfr)
    for e in (one, dfr):                                   # ... and not wrong together
        ex, eP = rel_err(e.get_x(), ref.x), rel_err(e.get_P(), ref.P)
        print("N %d tile %d batch %d: rel err x %.2e P %.2e" % (N, tile, e.cfg.batch, ex, eP))
        assert ex < REL and eP < REL
    np.testing.assert_array_equal(one.digest(), dfr.digest())


def test_the_bound_follows_the_map_as_it_grows_across_a_slab_and_a_tile_row(oracle_lib):
    """63 -> 67 landmarks at tile 64: the landmark-block rows go 126 -> 134, over the slab edge at 128 = the tile-row edge, an in-place pass
    between every two appends (batch 1: one per correction).  A bound kept from an earlier launch would leave the new rows out."""
    from ekf_slam_amd import Engine
    from oracle.ekf_structured import StructuredEKF
    N, N1 = 63, 67
    x, P, s = _state(N, 7)
    one = Engine(capacity=N1, tile=64, batch=1)
    dfr = Engine(capacity=N1, tile=64, batch=4)
    ref = StructuredEKF(N1, "known")
    for e in (one, dfr, ref):
        e.set_state(x, P, s)
    rng = np.random.default_rng(11)
    u = [0.1, 3.0]

    def correct(idx0):
        z = [rng.uniform(1, 30), rng.uniform(1, 359)]
        R = np.diag([z[0] * .01, z[1] * 5.0])
        for e in (one, dfr):
            e.predict(u); e.correct(z, R, idx0)
        ref.predict(u); ref.correct(z, R, idx0 + 1)

    correct(5)
    while one.N < N1:
        pos, sig = rng.uniform(-5, 5, 2), one.N + 1
        for e in (one, dfr, ref):
            e.append(u, np.diag([0.2, 40.0]), pos, sig)
        correct(one.N - 1)                                 # the landmark appended just now: its rows have to be inside the bound
        correct(int(rng.integers(0, one.N)))
        correct(int(rng.integers(0, one.N)))
    assert one.N == dfr.N == ref.N == N1
    _assert_bit_equal(one, dfr)
    for e in (one, dfr):
        ex, eP = rel_err(e.get_x(), ref.x), rel_err(e.get_P(), ref.P)
        print("growth 63 -> 67, batch %d: rel err x %.2e P %.2e" % (e.cfg.batch, ex, eP))
        assert ex < REL and eP < REL


@pytest.mark.parametrize("tile,batch,kernel", [(256, 1, "k_flush_mfma<float,256,"), (256, 4, "k_flush_mfma<float,256,"),
                                               (128, 1, "k_downdate_w<float,128,8,false"), (128, 5, "k_downdate_w<float,128,64,true>"),
                                               (64, 4, "k_downdate<float,64,")])
def test_float_tiles_with_f64_arithmetic_on_a_padded_map(tile, batch, kernel, oracle_lib):
    from ekf_slam_amd import Engine
    from oracle.ekf_structured import StructuredEKF
    N = 69
    x, P, s = _state(N, 169)
    e = Engine(capacity=N, tile=tile, storage="f32", batch=batch)
    ref = StructuredEKF(N, "known")
    e.set_state(x, P, s); ref.set_state(x, P, s)
    _steps([e], ref, STEPS, N)
    e.flush()
    assert e.downdate_kernel_name()[0].startswith(kernel), e.downdate_kernel_name()
    ex, eP = rel_err(e.get_x(), ref.x), rel_err(e.get_P(), ref.P)
    print("float tiles, tile %d batch %d (%s): rel err x %.2e P %.2e" % (tile, batch, e.downdate_kernel_name()[0], ex, eP))
    assert ex < REL and eP < REL


def test_the_asynchronous_pass_still_carries_every_row_into_the_second_store(oracle_lib):
    """cfg.async_flush: the pass writes the OTHER tile store and passes no bound.  With an append beside a pass in flight (its rows follow
    by k_copy_tile_rows) the result equals the synchronous engine's bit for bit."""
    from ekf_slam_amd import Engine
    from oracle.ekf_structured import StructuredEKF
    N = 69
    x, P, s = _state(N, 269)
    syn = Engine(capacity=N + 1, tile=128, batch=4)
    asy = Engine(capacity=N + 1, tile=128, batch=4, async_flush=True)
    ref = StructuredEKF(N + 1, "known")
    for e in (syn, asy, ref):
        e.set_state(x, P, s)
    _steps([syn, asy], ref, 4, 1)                          # a full batch: the asynchronous engine's pass is in flight ...
    pos = np.array([2.0, -3.0])
    for e in (syn, asy, ref):
        e.append([0.1, 3.0], np.diag([0.2, 40.0]), pos, N + 1)      # ... while the map grows
    _steps([syn, asy], ref, 8, 2)
    assert syn.N == asy.N == N + 1
    _assert_bit_equal(syn, asy)
    assert rel_err(syn.get_x(), ref.x) < REL and rel_err(syn.get_P(), ref.P) < REL
