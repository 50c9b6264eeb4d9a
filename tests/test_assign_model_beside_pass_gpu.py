"""GPU: ekf_assign_model issued behind a batch boundary while that boundary's asynchronous pass (cfg.async_flush) is in flight: one more leg
beside those of tests/test_beside_pass_gpu.py, built from the same pieces (beside_pass_cases.Nominal / scan_entry for the scan).  The call
reads only the live F64 copies, which carry every pending pair, so it must return what the synchronous engine returns -- F64 tiles, equal
bits -- and both engines must end in the same state."""
import numpy as np
import pytest

import beside_pass_cases as B
import helpers
import model_obs_cases as M
from helpers import R2, U2, assert_same
from removal_cases import lowrank_data, observe

pytestmark = pytest.mark.gpu
MODELS = (M.RANGE_BEARING, M.RELATIVE_XY, M.RANGE, M.BEARING)


@pytest.mark.parametrize("tile", [16, 64])
def test_behind_a_batch_boundary_of_an_asynchronous_pass(tile):
    N, batch = 150, 4
    x = lowrank_data(N, 5)[0]
    kw = dict(capacity=N + 8, tile=tile, storage="f64", batch=batch)
    e, twin = helpers.loaded(N, 5, async_flush=True, **kw), helpers.loaded(N, 5, **kw)
    nom, rng = B.Nominal(x), np.random.default_rng(17)
    scan = [dict(B.scan_entry(nom, rng, k, MODELS[q % 4]), gate=9.21 * (1 + q % 3)) for q, k in enumerate((0, 75, 76, N - 1, 23, 75, 100, 23, 5, 149, 11, 76))]
    steps = (5, 70, N - 3, 11, 40, 77, 2, 120)
    for q in (e, twin):
        for k in steps[:batch]:                               # the batch completes: its pass starts (asynchronous: on the pass stream)
            q.predict(U2); q.correct(observe(x, k), R2, k)
    got, ref = e.assign_model(scan, want_candidates=True), twin.assign_model(scan, want_candidates=True)
    assert set(got) == set(ref)
    for key in got:
        np.testing.assert_array_equal(got[key], ref[key], err_msg="beside the pass: " + key)
    assert np.any(got["landmark"] >= 0) and np.any(got["ncand"] >= 2) and np.isfinite(got["total"])
    for q in (e, twin):
        for k in steps[batch:batch + 2]:
            q.predict(U2); q.correct(observe(x, k), R2, k)
    inside, ref = e.assign_model(scan), twin.assign_model(scan)
    for key in inside:
        np.testing.assert_array_equal(inside[key], ref[key], err_msg="inside the next batch: " + key)
    for q in (e, twin):
        for k in steps[batch + 2:]:
            q.predict(U2); q.correct(observe(x, k), R2, k)
    assert_same(e, twin)
    e.close(); twin.close()
