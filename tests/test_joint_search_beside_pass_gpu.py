"""GPU: ekf_joint_search issued behind a batch boundary while that boundary's asynchronous pass (cfg.async_flush) is in flight: one more leg
beside those of tests/test_beside_pass_gpu.py, after tests/test_assign_model_beside_pass_gpu.py.  The call reads the live F64 copies and
the tiles patched with the pending pairs, so it must return what the synchronous engine returns -- F64 tiles, equal bits -- must not retire
the pass, and both engines must end in the same state."""
import numpy as np
import pytest

import joint_cases as J
import joint_search_cases as S
from helpers import R2, U2, assert_same
from removal_cases import observe

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tile", [16, 64])
def test_behind_a_batch_boundary_of_an_asynchronous_pass(tile):
    import helpers
    from ekf_slam_amd.slam import chi2_quantile
    N, batch, K = S.N0, 4, 6
    x, s, d, U, scan = S.cluster_scene(K)
    ents = J.scene_entries(scan, S.GATE)
    thr = [chi2_quantile(S.JOINT_P, dof) for dof in range(2 * K + 1)]
    kw = dict(capacity=N + 8, tile=tile, storage="f64", batch=batch)
    e, twin = helpers.engine(async_flush=True, **kw), helpers.engine(**kw)
    steps = (5, 70, N - 3, 41, 40, 77, 2, 120)
    for q in (e, twin):
        q.load_lowrank_state(x, s, d, U)
        for k in steps[:batch]:                               # the batch completes: its pass starts (asynchronous: on the pass stream)
            q.predict(U2); q.correct(observe(x, k), R2, k)
    pend = e.pending()
    got = e.joint_search(ents, thr, 64, want_candidates=True, want_alive=True)
    assert e.pending() == pend                                # nothing retired, nothing flushed
    ref = twin.joint_search(ents, thr, 64, want_candidates=True, want_alive=True)
    assert set(got) == set(ref)
    for key in got:
        np.testing.assert_array_equal(got[key], ref[key], err_msg="beside the pass: " + key)
    assert got["pairings"] >= 1 and got["nalive"] >= 2 and np.all(np.isfinite(got["alive_d2"]))
    for q in (e, twin):
        for k in steps[batch:batch + 2]:
            q.predict(U2); q.correct(observe(x, k), R2, k)
    inside, ref = e.joint_search(ents, thr, 8), twin.joint_search(ents, thr, 8)
    for key in inside:
        np.testing.assert_array_equal(inside[key], ref[key], err_msg="inside the next batch: " + key)
    for q in (e, twin):
        for k in steps[batch + 2:]:
            q.predict(U2); q.correct(observe(x, k), R2, k)
    assert_same(e, twin)
    e.close(); twin.close()
