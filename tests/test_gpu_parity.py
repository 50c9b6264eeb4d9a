"""GPU parity: the HIP path (through the C ABI) against the CPU oracle on identical seeded inputs.

Tolerance: BASELINE.json's north_star asks for 1e-6 relative F64 on state and covariance; REL below is
that tolerance, and the tests additionally report the (much smaller) error actually seen.
"""
import numpy as np
import pytest

from helpers import REL, rel_err

pytestmark = pytest.mark.gpu


def _random_spd_state(N, seed):
    rng = np.random.default_rng(seed)
    n = 3 + 2 * N
    x = np.concatenate([[0.3, -0.2, 40.0], rng.uniform(-20, 20, size=2 * N)])
    U = rng.normal(0, 0.05, size=(n, 6))
    d = rng.uniform(0.01, 0.1, size=n)
    P = np.diag(d) + U @ U.T
    s = np.arange(1, N + 1, dtype=np.float64)
    return x, P, s, d, U


def test_kat1_predict_from_constructor_state():
    """KAT-1: predict from the constructor state with u = [1, 0]."""
    from ekf_slam_amd import Engine
    e = Engine(capacity=4)
    e.predict([1.0, 0.0])
    np.testing.assert_allclose(e.get_x(), [1, 0, 0], atol=1e-15)
    np.testing.assert_allclose(e.get_P(), [[0.3, 0, 0], [0, 0.2, 0.1], [0, 0.1, 0.1]], atol=1e-15)
    np.testing.assert_allclose(e.get_Q3(), np.diag([0.2, 0, 0]), atol=1e-15)


def test_wrapto360_edge_in_predict():
    """KAT-2: theta + u2 == 360 stays 360, -90 -> 270."""
    from ekf_slam_amd import Engine
    e = Engine(capacity=4)
    e.predict([0.0, 360.0])
    assert e.get_x()[2] == 360.0
    e2 = Engine(capacity=4)
    e2.predict([0.0, -90.0])
    assert e2.get_x()[2] == 270.0


@pytest.mark.parametrize("mode", ["known", "uc"])
@pytest.mark.parametrize("tile", [16, 64])
def test_slam_run_20_landmarks(mode, tile, oracle_lib):
    """Config 1 shape: 20-landmark world, full predict/measure loop, against the structured oracle step by step."""
    from ekf_slam_amd.slam import EKF_SLAM, EKF_SLAM_UC, Landmark
    from ekf_slam_amd.world import SyntheticLandmark, make_run
    from oracle.ekf_structured import StructuredEKF
    _, run = make_run(20, 20260101, 40, policy="all")
    gpu = (EKF_SLAM if mode == "known" else EKF_SLAM_UC)(capacity=32, tile=tile)
    ref = StructuredEKF(32, mode)
    lg, lr = Landmark('SYNTHETIC'), SyntheticLandmark()
    worst = 0.0
    for t, (u, scan) in enumerate(run):
        gpu.predict(u); ref.predict(u)
        gpu.measure(scan, u, lg); ref.measure(scan, u, lr)
        assert gpu._e.N == ref.N
        ex, eP = rel_err(gpu.x, ref.x), rel_err(gpu.P, ref.P)
        worst = max(worst, ex, eP)
        assert ex < REL and eP < REL, "step %d: x %.3e P %.3e" % (t, ex, eP)
    np.testing.assert_array_equal(gpu.s, ref.s)
    print("worst rel err %s tile %d: %.3e" % (mode, tile, worst))


@pytest.mark.parametrize("tile", [16, 32, 64, 128])
def test_corrections_multi_tile(tile, oracle_lib):
    """Random SPD state with many tile rows; corrections on landmarks in first/middle/last tiles."""
    from ekf_slam_amd import Engine
    from oracle.ekf_structured import StructuredEKF
    N = 150
    x, P, s, _, _ = _random_spd_state(N, 7)
    e = Engine(capacity=N + 5, tile=tile)
    e.set_state(x, P, s)
    ref = StructuredEKF(N + 5, "known")
    ref.set_state(x, P, s)
    assert rel_err(e.get_P(), P) == 0.0
    rng = np.random.default_rng(3)
    for idx0 in [0, 1, N // 2, N - 1, 17, 0]:
        z = [rng.uniform(1, 30), rng.uniform(1, 359)]
        R = np.diag([z[0] * .01, z[1] * 5.0])
        e.correct(z, R, idx0)
        ref.correct(z, R, idx0 + 1)
        e.predict([0.1, 3.0]); ref.predict([0.1, 3.0])
        assert rel_err(e.get_x(), ref.x) < REL
        assert rel_err(e.get_P(), ref.P) < REL
    print("tile %d final rel err P %.3e" % (tile, rel_err(e.get_P(), ref.P)))


def test_append_across_tile_boundary(oracle_lib):
    from ekf_slam_amd import Engine
    from oracle.ekf_structured import StructuredEKF
    N = 30
    x, P, s, _, _ = _random_spd_state(N, 11)
    e = Engine(capacity=64, tile=16)
    ref = StructuredEKF(64, "known")
    e.set_state(x, P, s); ref.set_state(x, P, s)
    rng = np.random.default_rng(5)
    for k in range(12):   # crosses the 32- and 40-landmark tile-row edges for T=16 (8 landmarks per tile row)
        u = [0.1, 3.0]
        R = np.diag([0.2, 11.0])
        pos = rng.uniform(-5, 5, size=2)
        e.append(u, R, pos, N + k + 1); ref.append(u, R, pos, N + k + 1)
        z = [rng.uniform(1, 30), rng.uniform(1, 359)]
        e.correct(z, R, N + k); ref.correct(z, R, N + k + 1)
    assert e.N == ref.N == N + 12
    assert rel_err(e.get_x(), ref.x) < REL
    assert rel_err(e.get_P(), ref.P) < REL
    np.testing.assert_array_equal(e.get_s(), ref.s)


def test_associate_costs_and_decision(oracle_lib):
    from ekf_slam_amd import Engine
    from oracle.ekf_structured import StructuredEKF
    N = 700    # 3 association workgroups
    x, P, s, _, _ = _random_spd_state(N, 13)
    e = Engine(mode="uc", capacity=N, tile=64)
    ref = StructuredEKF(N, "uc")
    e.set_state(x, P, s); ref.set_state(x, P, s)
    R = np.diag([1.0, 50.0])
    for sig, expect_new in [(5.0, False), (700.0, False), (701.0, True), (1.05, False), (1.2, True)]:
        z = [7.0, 123.0, sig]
        new_g, idx_g, pc_g, sc_g = e.associate(z, R, want_costs=True)
        new_r, idx_r, pc_r, sc_r = ref.associate(z, R, want_costs=True)
        assert new_g == new_r == expect_new
        assert idx_g + 1 == idx_r
        assert rel_err(pc_g, pc_r) < REL
        assert rel_err(sc_g, sc_r) < REL
    # ties: duplicate signatures -> the first (lowest) index wins (Correspondence.m:81 strict '<')
    s2 = s.copy(); s2[400] = 9.0; s2[8] = 9.0; s2[650] = 9.0
    e.set_state(x, P, s2); ref.set_state(x, P, s2)
    new_g, idx_g = e.associate([7.0, 123.0, 9.0], R)
    assert (new_g, idx_g) == (False, 8)
    assert ref.associate([7.0, 123.0, 9.0], R) == (False, 9)


def test_lowrank_load_and_digest():
    from ekf_slam_amd import Engine
    N = 200
    x, P, s, d, U = _random_spd_state(N, 17)
    e = Engine(capacity=N, tile=64)
    e.load_lowrank_state(x, s, d, U)
    assert rel_err(e.get_P(), P) < 1e-13
    np.testing.assert_array_equal(e.get_x(), x)
    dg = e.digest()
    low = np.tril(P)
    np.testing.assert_allclose(dg, [np.trace(P), low.sum(), (low ** 2).sum()], rtol=1e-11)
    blk = e.get_P_block(3 + 2 * 77, 3 + 2 * 20, 2, 5)
    np.testing.assert_allclose(blk, P[3 + 154:3 + 156, 43:48], rtol=1e-13)


def test_error_statuses():
    from ekf_slam_amd import Engine, EkfError
    from ekf_slam_amd import _lib as L
    e = Engine(capacity=1)
    with pytest.raises(EkfError) as ei:
        e.correct([1, 1], np.eye(2), 0)
    assert ei.value.status == L.EKF_ERR_INDEX
    e.append([0.1, 1], np.eye(2), [1, 1], 1)
    with pytest.raises(EkfError) as ei:
        e.append([0.1, 1], np.eye(2), [2, 2], 2)
    assert ei.value.status == L.EKF_ERR_CAPACITY
    # empty-map row with two indexed landmarks in the table: the reference's append() call is malformed
    e2 = Engine(capacity=4)
    with pytest.raises(EkfError) as ei:
        e2.measure([[1.0, 10.0, 1.0]], [0.1, 1.0], [1.0, 2.0], [[0, 0], [1, 1]])
    assert ei.value.status == L.EKF_ERR_LOOKUP


def test_measure_with_position_weighted_association(oracle_lib):
    """w_pos = 1 is the commented-out likelihood of Correspondence.m:74 (Mahalanobis + signature): measure() must then
    run the device association kernels (the host mirror of s cannot decide), and agree with the oracle."""
    from ekf_slam_amd.slam import EKF_SLAM_UC, Landmark
    from ekf_slam_amd.world import SyntheticLandmark, make_run
    from oracle.ekf_structured import StructuredEKF
    _, run = make_run(30, 31, 14, policy="nearest", m=5)
    # a threshold that lets the position cost matter but still associates re-observed landmarks
    gpu = EKF_SLAM_UC(capacity=32, tile=16, batch=4, w_pos=1.0, s_thresh=1e12)
    ref = StructuredEKF(32, "uc", w_pos=1.0, s_thresh=1e12)
    lg, lr = Landmark('SYNTHETIC'), SyntheticLandmark()
    for u, scan in run:
        gpu.predict(u); ref.predict(u)
        gpu.measure(scan, u, lg); ref.measure(scan, u, lr)
        assert gpu._e.N == ref.N
    assert rel_err(gpu.x, ref.x) < REL and rel_err(gpu.P, ref.P) < REL
    np.testing.assert_array_equal(gpu.s, ref.s)


def test_soak_2000_update_steps_ring_and_throttle(oracle_lib):
    """A longer run (500 iterations x 4 observations at 300 landmarks, batch 7): exercises the pending-pair ring wrap,
    the run-ahead throttle and repeated flushes; final state against the oracle."""
    from ekf_slam_amd import Engine
    from oracle.ekf_structured import StructuredEKF
    N = 300
    x, P, s, _, _ = _random_spd_state(N, 71)
    e = Engine(capacity=N, batch=7, async_flush=True)
    e2 = Engine(capacity=N, batch=7)
    ref = StructuredEKF(N, "known")
    for o in (e, e2, ref):
        o.set_state(x, P, s)
    rng = np.random.default_rng(19)
    for it in range(500):
        u = [0.05, 1.0 + 0.01 * (it % 7)]
        for o in (e, e2, ref):
            o.predict(u)
        for _ in range(4):
            idx0 = int(rng.integers(0, N))
            z = [rng.uniform(1, 30), rng.uniform(20, 340)]
            R = np.diag([z[0] * .01, z[1] * 5.0])
            e.correct(z, R, idx0); e2.correct(z, R, idx0); ref.correct(z, R, idx0 + 1)
    np.testing.assert_array_equal(e.get_x(), e2.get_x())
    np.testing.assert_array_equal(e.get_P(), e2.get_P())
    assert np.isfinite(e.get_x()).all()
    assert rel_err(e.get_x(), ref.x) < REL and rel_err(e.get_P(), ref.P) < REL
    print("soak: x %.2e P %.2e" % (rel_err(e.get_x(), ref.x), rel_err(e.get_P(), ref.P)))
