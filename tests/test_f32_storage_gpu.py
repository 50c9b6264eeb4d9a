"""GPU: F32 tile storage with every solve in F64 (cfg.storage = EKF_STORE_F32; BASELINE.json configs[4]).

The landmark block is rounded to float at every write (float eps 6e-8, at most one rounding per entry and
flush), so parity with the F64 oracle degrades with the number of update-steps; SURVEY.md section 7 expects this
mode to need its own tolerance.  Asserted here, against the F64 oracle on the same inputs after a dozen
update-steps with appends: 1e-6 relative (max-norm) on both x and P; measured 1e-8 (x) and 6e-8 (P).  x, the
robot block, the robot/landmark strip and every innovation / gain stay in F64."""
import numpy as np
import pytest

from helpers import rel_err

pytestmark = pytest.mark.gpu
TOL_X, TOL_P = 1e-6, 1e-6


def _state(N, seed):
    rng = np.random.default_rng(seed)
    n = 3 + 2 * N
    x = np.concatenate([[0.3, -0.2, 40.0], rng.uniform(-20, 20, size=2 * N)])
    U = rng.normal(0, 0.05, size=(n, 6))
    return x, np.diag(rng.uniform(0.01, 0.1, size=n)) + U @ U.T, np.arange(1, N + 1.0)


@pytest.mark.parametrize("tile,batch", [(16, 1), (64, 1), (128, 1), (256, 1), (0, 8), (128, 8), (16, 5)])
def test_f32_storage_against_f64_oracle(tile, batch, oracle_lib):
    from ekf_slam_amd import Engine
    from oracle.ekf_structured import StructuredEKF
    N = 300
    x, P, s = _state(N, 61)
    e = Engine(capacity=N + 8, tile=tile, storage="f32", batch=batch)
    ref = StructuredEKF(N + 8, "known")
    e.set_state(x, P, s); ref.set_state(x, P, s)
    assert rel_err(e.get_P(), P) < 1e-7                     # one float rounding of the landmark block
    rng = np.random.default_rng(14)
    for step in range(12):
        u = [0.1, 3.0]
        e.predict(u); ref.predict(u)
        idx0 = int(rng.integers(0, e.N))
        z = [rng.uniform(1, 30), rng.uniform(1, 359)]
        R = np.diag([z[0] * .01, z[1] * 5.0])
        e.correct(z, R, idx0); ref.correct(z, R, idx0 + 1)
        if step in (3, 7):
            pos = rng.uniform(-5, 5, 2)
            e.append(u, R, pos, e.N + 1); ref.append(u, R, pos, ref.N + 1)
    ex, eP = rel_err(e.get_x(), ref.x), rel_err(e.get_P(), ref.P)
    print("f32 tile %d batch %d: x %.2e P %.2e" % (tile, batch, ex, eP))
    assert ex < TOL_X and eP < TOL_P


def test_f32_halves_the_tile_store():
    from ekf_slam_amd import Engine
    a = Engine(capacity=2000, storage="f64", tile=128).device_bytes()
    b = Engine(capacity=2000, storage="f32", tile=128).device_bytes()
    assert b < 0.56 * a


@pytest.mark.parametrize("tile,batch", [(16, 1), (256, 4), (128, 8)])
def test_f32_tiles_unknown_correspondence_device_loop_equals_host_decided(tile, batch, oracle_lib):
    """EKF_SLAM_UC.measure on F32 tiles: the device-resident loop (cfg.device_assoc = 3: the association evaluated in the gather
    kernel's epilogue from float tiles + f64 pending pairs) against the host-decided mode -- same decisions, so the same F32
    state bit for bit -- and against the F64 oracle at the short-run F32 tolerance."""
    from ekf_slam_amd.slam import EKF_SLAM_UC, Landmark
    from ekf_slam_amd.world import SyntheticLandmark, make_run
    from oracle.ekf_structured import StructuredEKF
    _, run = make_run(40, 5, 10, policy="nearest", m=6)
    dev = EKF_SLAM_UC(capacity=48, tile=tile, batch=batch, storage="f32")
    host = EKF_SLAM_UC(capacity=48, tile=tile, batch=batch, storage="f32", device_assoc=0)
    assert dev._e.cfg.device_assoc == 3
    ref = StructuredEKF(48, "uc")
    ld, lh, lr = Landmark('SYNTHETIC'), Landmark('SYNTHETIC'), SyntheticLandmark()
    for u, scan in run:
        for e, l in ((dev, ld), (host, lh), (ref, lr)):
            e.predict(u); e.measure(scan, u, l)
    assert dev._e.N == host._e.N == ref.N == 40
    np.testing.assert_array_equal(dev.x, host.x)
    np.testing.assert_array_equal(dev.P, host.P)
    assert rel_err(dev.x, ref.x) < TOL_X and rel_err(dev.P, ref.P) < TOL_P
