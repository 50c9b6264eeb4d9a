"""GPU: the joint-compatibility search on the device (ekf_joint_search; include/ekfslam.h) and the policy switch on
top of it (measure_model_joint(device_search=True) of ekf_slam_amd/slam.py).

The yardstick is THE LIBRARY ITSELF on the same handle: assign_model(want_candidates=True), then one joint_innovation call per level, as
measure_model_joint walks it (joint_search_cases.library_search).  The contract is equality -- the winner, every d2 of the final beam, the
counters, the lists -- so every comparison is assert_array_equal.  N = 150 throughout: 19 tile rows of edge 16, one tile of edge 256."""
import ctypes

import numpy as np
import pytest

import associate_model_cases as A
import helpers
import joint_cases as J
import joint_search_cases as S
import model_obs_cases as M
from helpers import R2, RPOS, U2, assert_same, same_npz, status_of
from removal_cases import observe

pytestmark = pytest.mark.gpu
N = S.N0
# (storage, tile, batch, corrections): batch 1 flushes every correction; batch 32 leaves 5 pairs pending
STORES = [("f64", 16, 1, 0), ("f64", 16, 32, 5), ("f32", 256, 1, 0), ("f32", 256, 32, 5)]


def scene(name):
    """(x, s, d, U, entries with the candidate gate) by name: 'two' = joint_cases.ambiguous_scene, 'K4' / 'K6' / 'K8' the clusters, 'mixed'."""
    if name == "two":
        x, s, d, U, scan = J.ambiguous_scene()
        return x, s, d, U, J.scene_entries(scan, S.GATE)
    x, s, d, U, scan = S.cluster_scene(4 if name == "mixed" else int(name[1:]))
    return x, s, d, U, (S.mixed_scan(x) if name == "mixed" else J.scene_entries(scan, S.GATE))


def thresholds(m):
    from ekf_slam_amd.slam import chi2_quantile
    return [chi2_quantile(S.JOINT_P, dof) for dof in range(2 * m + 1)]


def handle(name, storage="f64", tile=16, batch=8, corrections=0, **kw):
    x, s, d, U, ents = scene(name)
    e = helpers.engine(**dict(dict(capacity=N + 8, tile=tile, batch=batch, storage=storage), **kw))
    e.load_lowrank_state(x, s, d, U)
    for k in (5, 16, N - 3, 41, 77)[:corrections]:
        e.predict(U2); e.correct(observe(x, k), R2, k)
    return e, ents


def ask(e, ents, beam=64, thr=None):
    return e.joint_search(ents, thresholds(len(ents)) if thr is None else thr, beam, want_candidates=True, want_alive=True)


def assert_is_the_library_walk(e, ents, beam, msg):
    pend = e.pending()
    got = ask(e, ents, beam)
    assert e.pending() == pend
    want, asg = S.library_search(e, ents, thresholds(len(ents)), beam)
    S.assert_search_equal(got, want, msg)
    for key in ("best", "second", "d2_best", "d2_second", "within_gate", "irregular", "cand", "cand_d2"):
        np.testing.assert_array_equal(got["match_irregular" if key == "irregular" else key], asg[key], err_msg="%s %s" % (msg, key))
    return got


@pytest.mark.parametrize("storage,tile,batch,corrections", STORES)
@pytest.mark.parametrize("name,beam", [("two", 64), ("K4", 64), ("K4", 2), ("K6", 64), ("K6", 2), ("K8", 64), ("K8", 2), ("mixed", 64), ("mixed", 2)])
def test_the_search_is_the_library_walk_bit_for_bit_and_changes_nothing(name, beam, storage, tile, batch, corrections):
    kw = dict(storage=storage, tile=tile, batch=batch, corrections=corrections)
    (e, ents), (twin, _) = handle(name, **kw), handle(name, **kw)
    assert e.pending() == corrections
    got = assert_is_the_library_walk(e, ents, beam, "%s beam %d %s" % (name, beam, storage))
    print("%s beam %d %s T = %d, %d pending: winner %s d2 %.6g nalive %d tested %s survived %s truncated %s irregular %d"
          % (name, beam, storage, tile, corrections, got["landmark"].tolist(), got["d2"], got["nalive"], got["tested"].tolist(),
             got["survived"].tolist(), got["truncated"], got["irregular"]))
    if corrections == 0 and storage == "f64" and name.startswith("K"):     # the loaded state is the NumPy scene: its premises hold here too
        ref = S.cluster_reference(int(name[1:]), beam)[4]
        for key in ("landmark", "truncated", "nalive", "tested", "survived", "alive"):
            np.testing.assert_array_equal(got[key], ref[key], err_msg=key)
        np.testing.assert_allclose(got["alive_d2"], ref["alive_d2"], rtol=1e-9)
    if name == "mixed":
        assert got["tested"][1] == 0 and got["survived"][1] == 0 and got["landmark"][1] == -1 and got["within_gate"][1] == 0
    assert got["truncated"] or beam == 64
    assert_same(e, twin)                                     # x, s, P, the diagonal blocks and the digest of a twin that never asked
    e.close(); twin.close()


def test_an_empty_map_and_a_scan_without_candidates():
    _, _, _, _, ents = scene("K4")
    e = helpers.engine(capacity=16, tile=16)
    got = ask(e, ents)
    assert e.N == 0 and got["landmark"].tolist() == [-1] * 4 and got["d2"] == 0.0 and (got["dof"], got["pairings"], got["nalive"]) == (0, 0, 1)
    assert not got["truncated"] and got["irregular"] == 0 and not got["tested"].any() and not got["survived"].any()
    assert np.all(got["cand"] == -1) and np.all(np.isinf(got["cand_d2"])) and np.all(got["best"] == -1)
    assert got["alive"].tolist() == [[-1] * 4] and got["alive_d2"].tolist() == [0.0]
    e.close()
    e, _ = handle("K4")
    far = [A.entry(M.RELATIVE_XY, [400.0 + 7 * q, -300.0], RPOS, S.GATE) for q in range(3)]
    got = assert_is_the_library_walk(e, far, 64, "no candidates")
    assert got["landmark"].tolist() == [-1] * 3 and got["d2"] == 0.0 and got["nalive"] == 1 and not got["tested"].any()
    assert not np.any(got["within_gate"]) and np.all(got["best"] >= 0)
    e.close()


def test_a_landmark_on_the_robot_is_no_candidate_and_never_wins():
    from ekf_slam_amd.engine import _p
    e, _ = handle("K4")
    x = e.get_x()
    ents = [dict(en, gate=S.GATE) for en in J.cycle_scan(x, list(range(S.LM0, S.LM0 + 4)), (M.RANGE_BEARING,))]
    x[3 + 2 * (S.LM0 + 1):5 + 2 * (S.LM0 + 1)] = x[:2]
    x = np.ascontiguousarray(x)
    e._check(e.lib.ekf_set_x(e.h, _p(x), x.size))
    got = assert_is_the_library_walk(e, ents, 64, "a landmark on the robot")
    assert np.all(got["match_irregular"] == 1) and got["irregular"] == 0      # it has no individual d2, so no list holds it
    assert S.LM0 + 1 not in got["landmark"].tolist() and not np.any(got["cand"] == S.LM0 + 1) and not np.any(got["alive"] == S.LM0 + 1)
    assert np.isfinite(got["d2"]) and np.all(np.isfinite(got["alive_d2"]))
    e.close()


def test_a_pairing_whose_pivot_fails_is_irregular_counted_and_never_wins():
    """The cross covariance of landmarks 40 and 41 raised far beyond their variances (set_state takes any symmetric P): each pairing alone
    keeps its positive S and stays a candidate, but a hypothesis that holds both has a stacked S whose Schur complement is negative --
    the second pairing's pivot fails.  Such extensions have no d2: counted in `irregular`, never alive, never the winner."""
    e, ents = handle("K4")
    x, s, P = helpers.state(e)
    a, b = 3 + 2 * S.LM0, 5 + 2 * S.LM0
    P[b:b + 2, a:a + 2] = 50.0 * P[a:a + 2, a:a + 2]
    P[a:a + 2, b:b + 2] = P[b:b + 2, a:a + 2].T
    e.set_state(x, P, s)
    got = assert_is_the_library_walk(e, ents, 64, "a failing pivot")
    print("a failing pivot: irregular %d winner %s d2 %.3g nalive %d" % (got["irregular"], got["landmark"].tolist(), got["d2"], got["nalive"]))
    both = [h for h in got["alive"].tolist() if S.LM0 in h and S.LM0 + 1 in h]
    assert got["irregular"] > 0 and not both and np.all(np.isfinite(got["alive_d2"]))
    assert np.all(got["within_gate"] >= 4) and np.any(got["cand"][:, :4] == S.LM0) and np.any(got["cand"][:, :4] == S.LM0 + 1)
    e.close()


def _raw(e, ents, thr, beam=64, m=None, res=True, cand=(True, True), alive=(True, True)):
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd.engine import _p
    arr = (L.EkfModelObs * max(len(ents), 1))()
    for k, ent in enumerate(ents):
        arr[k] = e._model_obs(ent["model"], ent["z"], ent["R"], (), (0.0, 0.0), ent["gate"])
    m = len(ents) if m is None else m
    thr = None if thr is None else np.ascontiguousarray(thr, dtype=np.float64)
    out = L.EkfJointSearchResult()
    c, c2 = np.zeros((32, L.EKF_ASSIGN_CANDIDATES), dtype=np.int64), np.zeros((32, L.EKF_ASSIGN_CANDIDATES))
    h, h2 = np.zeros((64, 32), dtype=np.int64), np.zeros(64)
    i64p = ctypes.POINTER(ctypes.c_int64)
    return e.lib.ekf_joint_search(e.h, arr, m, None if thr is None else _p(thr), beam, ctypes.byref(out) if res else None, None,
                                  c.ctypes.data_as(i64p) if cand[0] else None, _p(c2) if cand[1] else None,
                                  h.ctypes.data_as(i64p) if alive[0] else None, _p(h2) if alive[1] else None)


def test_refusals_in_their_order_and_nothing_changes():
    from ekf_slam_amd import _lib as L
    (e, ents), (twin, _) = handle("K4", batch=8, corrections=3), handle("K4", batch=8, corrections=3)
    thr = thresholds(4)
    bad = L.EKF_ERR_INVALID_ARG
    err = lambda: e.lib.ekf_last_error(e.h)
    assert _raw(e, ents, thr) == 0
    assert _raw(e, ents, thr, res=False) == bad and _raw(e, ents, thr, m=0) == bad
    assert _raw(e, ents * 9, thresholds(36), m=33) == bad
    assert _raw(e, [dict(ents[0], model=M.LANDMARK_RANGE)] + ents[1:], thr) == bad
    assert _raw(e, ents, thr, cand=(True, False)) == bad and b"cand" in err()
    assert _raw(e, [dict(ents[0], gate=float("inf"))] + ents[1:], None, cand=(False, True)) == bad and b"cand" in err()      # the lists before the gate
    assert _raw(e, [dict(ents[0], gate=float("inf"))] + ents[1:], None) == bad and b"gate" in err()                        # the gate before the threshold
    assert _raw(e, ents, None, beam=0) == bad and b"threshold" in err()                                                    # the threshold before the beam
    for v in (float("nan"), float("inf"), -1.0):
        assert _raw(e, ents, thr[:8] + [v], beam=0) == bad and b"threshold" in err()
    assert _raw(e, ents, thr[:7] + [-1.0, 1.0]) == bad
    assert _raw(e, ents, thr, beam=0, alive=(True, False)) == bad and b"beam" in err()                                     # the beam before the beam's arrays
    assert _raw(e, ents, thr, beam=65) == bad and b"beam" in err()
    assert _raw(e, ents, thr, alive=(True, False)) == bad and b"alive" in err() and _raw(e, ents, thr, alive=(False, True)) == bad
    assert _raw(e, ents, thr, cand=(False, False), alive=(False, False)) == 0
    assert e.pending() == 3
    assert_same(e, twin)
    # sharded handles: refused, and the message says why; the arguments are checked first
    sh = helpers.engine(capacity=64, tile=16, world=2, rank=0)
    st, msg = status_of(lambda: sh.joint_search(ents, thr))
    assert st == bad and "shard" in msg
    st, msg = status_of(lambda: sh.joint_search(ents, thr, beam=65))
    assert st == bad and "shard" not in msg
    e.close(); twin.close(); sh.close()


def test_a_lone_forced_shard_equals_the_unsharded_handle_and_is_refused_between_begin_and_finish():
    from ekf_slam_amd import _lib as L
    (e, ents), (twin, _) = handle("K6", force_sharded=1), handle("K6")
    x = twin.get_x()
    harr = (ctypes.c_void_p * 1)(e.h)
    z = observe(x, 7)
    e.predict(U2); twin.predict(U2)
    e.correct_begin(z, R2, 7)
    st, msg = status_of(lambda: ask(e, ents))
    assert st == L.EKF_ERR_STATE and "joint_search" in msg and "begin and finish" in msg
    assert status_of(lambda: ask(e, ents, beam=65))[0] == L.EKF_ERR_INVALID_ARG        # the arguments come first
    assert e.lib.ekf_exchange_local(harr, 1) == 0
    e.correct_finish()
    twin.correct(z, R2, 7)
    a, b = ask(e, ents), ask(twin, ents)
    assert set(a) == set(b)
    for key in a:
        np.testing.assert_array_equal(a[key], b[key], err_msg="a lone shard: " + key)
    assert_same(e, twin)
    e.close(); twin.close()


def test_the_scratch_is_allocated_at_the_first_call_and_counted():
    e, ents = handle("K4")
    before = e.device_bytes()
    ask(e, ents)
    after = e.device_bytes()
    ask(e, ents)
    assert after > before and e.device_bytes() == after
    e.close()


@pytest.mark.parametrize("name", ["two", "K6"])
@pytest.mark.parametrize("joint_update", [False, True])
def test_the_policy_with_the_device_search_leaves_the_same_state_and_the_same_log(name, joint_update, tmp_path):
    from ekf_slam_amd.slam import EKF_SLAM
    from ekf_slam_amd.trajectory import TrajectoryLog
    x, s, d, U, ents = scene(name)
    scan = [(en["model"], en["z"], en["R"]) for en in ents]

    def run(device_search):
        f = EKF_SLAM(capacity=N + 8, tile=16, batch=8)
        f._e.load_lowrank_state(x, s, d, U)
        f.log = TrajectoryLog()
        out = f.measure_model_joint(scan, S.GATE, 25.0, joint_update=joint_update, device_search=device_search)
        f.predict(U2)
        f.log.record(U2, None, [], [])
        path = tmp_path / ("search_%d.npz" % device_search)
        f.log.save(path)
        return f, out, path

    (host, out_h, log_h), (dev, out_d, log_d) = run(False), run(True)
    assert out_d == out_h and out_d[1] is (name == "K6")
    assert [kind for kind, _ in out_d[0]] == ["matched"] * len(scan)
    assert_same(dev._e, host._e)
    assert same_npz(log_h, log_d)
    with pytest.raises(ValueError):
        dev.measure_model_joint(scan, S.GATE, 25.0, beam=65, device_search=True)
    wrapped = dev.joint_search(ents, want_alive=True)
    assert wrapped["landmark"].min() >= 0 and wrapped["alive"].min() >= 0
    host._e.close(); dev._e.close()
