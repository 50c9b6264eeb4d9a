"""GPU: a scan assigned, then applied, with no host wait between the two (ekf_observe_model_assigned / ekf_assigned_scan_result;
include/ekfslam.h) and the policy on top of it (measure_model_assigned(device_apply=True) of ekf_slam_amd/slam.py).

The yardstick is THE REFERENCE SEQUENCE of the header on a twin engine in the same state: ekf_assign_model, then per entry in scan order
ekf_observe_model at the assigned landmark, or -- for an entry left out -- ekf_observe_model at landmark 0 with a gate of -1, a step that
cannot apply.  Every comparison of a state, a record, an assignment and a total is assert_array_equal / ==.  N = 150 landmarks are two
workgroups of the step's launch; the scan is assign_model_cases.contention_scene(m=12) with the gates of entries 2, 5 and 9 at 1e-9, so
that no landmark lies inside them and the assignment leaves them out."""
import ctypes

import numpy as np
import pytest

import assign_model_cases as C
import associate_model_cases as A
import helpers
import model_obs_cases as M
from helpers import R2, RPOS, U2, assert_same, engine, status_of
from removal_cases import lowrank_data, observe

pytestmark = pytest.mark.gpu
INF = float("inf")
TIGHT = (2, 5, 9)
STORES = [(16, "f64"), (64, "f64"), (16, "f32"), (64, "f32")]
RESULT_KEYS = ("landmark", "d2", "ncand", "total")


def scene(m=12, seed=1):
    x, s, d, U, scan, _ = C.contention_scene(m=m, seed=seed)
    entries = [A.entry(model, z, R, 1e-9 if k in TIGHT else C.SCENE_GATE) for k, (model, z, R) in enumerate(scan)]
    return (x, s, d, U), entries


def started(data, history=0, **kw):
    """An engine loaded with the scene and `history` corrections behind it (pending in the ring where cfg.batch lets them)."""
    kw.setdefault("capacity", C.SCENE_N + 8)
    e = engine(**kw)
    e.load_lowrank_state(*data)
    for k in (5, 72, 140)[:history]:
        e.predict(U2); e.correct(observe(data[0], k), R2, k)
    return e


def reference_sequence(e, entries, omit=False, wait=False):
    """The header's sequence on e: (assign_model's result, the record of every assigned step where waited for)."""
    res = e.assign_model(entries)
    recs = {}
    for k, ent in enumerate(entries):
        lm = int(res["landmark"][k])
        if lm >= 0:
            recs[k] = e.observe_model(ent["model"], ent["z"], ent["R"], [lm], gate=ent["gate"], wait=wait)
        elif not omit:
            e.observe_model(ent["model"], ent["z"], ent["R"], [0], gate=-1.0)
    return res, recs


def assert_scene_premises(res):
    """Asserted on ekf_assign_model's own output: if this fails the input is wrong, not the code."""
    assert int((res["landmark"] < 0).sum()) >= 3 and int((res["landmark"] >= 0).sum()) >= 6
    assert all(res["landmark"][k] < 0 for k in TIGHT)


def assert_same_after(dev, twin):
    assert dev.pending() == twin.pending()
    assert_same(dev, twin)


# ------------------------------------------------------------------------------------------------------------------
# 1. the reference sequence on a twin engine
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("history", [0, 3])
@pytest.mark.parametrize("batch", [1, 4])
@pytest.mark.parametrize("tile,storage", STORES)
def test_the_scan_leaves_what_the_reference_sequence_leaves(tile, storage, batch, history):
    data, entries = scene()
    kw = dict(tile=tile, storage=storage, batch=batch)
    dev, twin = started(data, history, **kw), started(data, history, **kw)
    before = dev.pending()
    assert before == (history if batch == 4 else 0)
    dev.observe_model_assigned(entries)
    res, _ = reference_sequence(twin, entries)
    assert_scene_premises(res)
    assert dev.pending() == twin.pending() == (before + 12) % batch
    assert_same_after(dev, twin)
    if storage == "f64":                                      # ... and, flushed, the sequence with the left-out entries simply omitted
        short = started(data, history, **kw)
        reference_sequence(short, entries, omit=True)
        dev.flush(); short.flush()
        assert_same(dev, short)
        short.close()
    dev.close(); twin.close()


# ------------------------------------------------------------------------------------------------------------------
# 2. the result
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage,batch", [(16, "f64", 4), (64, "f32", 1)])
def test_the_result_is_the_assignment_and_the_records_of_the_steps(tile, storage, batch):
    from ekf_slam_amd import _lib as L
    data, entries = scene()
    kw = dict(tile=tile, storage=storage, batch=batch)
    dev, twin, short = started(data, 3, **kw), started(data, 3, **kw), started(data, 3, **kw)
    for e in (dev, short):
        e.linear_rejections()
    dev.observe_model_assigned(entries)
    got = dev.assigned_scan_result()
    res, recs = reference_sequence(twin, entries, wait=True)
    assert_scene_premises(res)
    for key in RESULT_KEYS:
        np.testing.assert_array_equal(got[key], res[key], err_msg=key)
    outcomes = set()
    for k in range(12):
        if k in recs:
            np.testing.assert_array_equal(got["nu"][k], recs[k]["nu"]); np.testing.assert_array_equal(got["S"][k], recs[k]["S"])
            np.testing.assert_array_equal(got["step_d2"][k], recs[k]["d2"])
            assert got["outcome"][k] == recs[k]["outcome"]
            outcomes.add(int(got["outcome"][k]))
        else:
            assert got["outcome"][k] == L.EKF_LINEAR_UNASSIGNED == 3 and np.isnan(got["step_d2"][k])
            assert not got["nu"][k].any() and not got["S"][k].any()
    assert L.EKF_LINEAR_APPLIED in outcomes
    # a left-out step is counted by neither counter: the counts are the omitted-entries sequence's
    reference_sequence(short, entries, omit=True)
    assert dev.linear_rejections() == short.linear_rejections()
    assert_same_after(dev, twin)
    for e in (dev, twin, short):
        e.close()


# ------------------------------------------------------------------------------------------------------------------
# 3. small maps
# ------------------------------------------------------------------------------------------------------------------
def test_an_empty_map_a_single_landmark_and_a_single_observation():
    from ekf_slam_amd import _lib as L
    _, entries = scene()
    e = engine(capacity=8, tile=16)
    x0, P0 = e.get_x(), e.get_P()
    e.observe_model_assigned(entries[:3])
    assert e.pending() == 0 and e.N == 0
    got = e.assigned_scan_result()
    assert got["landmark"].tolist() == [-1] * 3 and got["ncand"].tolist() == [0] * 3 and np.all(got["d2"] == INF)
    assert got["total"] == sum(ent["gate"] for ent in entries[:3]) and got["outcome"].tolist() == [L.EKF_LINEAR_UNASSIGNED] * 3
    np.testing.assert_array_equal(e.get_x(), x0); np.testing.assert_array_equal(e.get_P(), P0)
    e.close()
    # one landmark, three sightings of it: exactly one gets it
    x, s, d, U = lowrank_data(1, 5)
    kw = dict(capacity=4, tile=16, batch=4)
    one, twin = engine(**kw), engine(**kw)
    one.load_lowrank_state(x, s, d, U); twin.load_lowrank_state(x, s, d, U)
    hx = M.h_of(M.RELATIVE_XY, x[:3], x[3:5])
    three = [A.entry(M.RELATIVE_XY, hx + off, RPOS, 50.0) for off in ([0.05, -0.02], [-0.01, 0.03], [0.08, 0.06])]
    one.observe_model_assigned(three)
    got = one.assigned_scan_result()
    assert int((got["landmark"] == 0).sum()) == 1 and int((got["landmark"] == -1).sum()) == 2 and one.pending() == 3
    res, _ = reference_sequence(twin, three)
    np.testing.assert_array_equal(got["landmark"], res["landmark"])
    assert_same_after(one, twin)
    one.close(); twin.close()
    # one observation
    data, entries = scene()
    dev, twin = started(data, 3, tile=64, batch=4), started(data, 3, tile=64, batch=4)
    dev.observe_model_assigned(entries[:1])
    res, _ = reference_sequence(twin, entries[:1])
    assert res["landmark"][0] >= 0 and dev.assigned_scan_result()["landmark"].tolist() == res["landmark"].tolist()
    assert_same_after(dev, twin)
    dev.close(); twin.close()


# ------------------------------------------------------------------------------------------------------------------
# 4. refusals
# ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_state_and_the_ring_as_found():
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import marshal
    from ekf_slam_amd.sharding import ShardGroup
    data, entries = scene()
    dev, twin = started(data, 3, tile=16, batch=4), started(data, 3, tile=16, batch=4)
    assert dev.pending() == 3
    st, msg = status_of(dev.assigned_scan_result)
    assert st == L.EKF_ERR_STATE and "assigned_scan_result" in msg              # before any scan
    bad = L.EKF_ERR_INVALID_ARG
    arr33, _ = marshal.scan_obs(entries * 3)
    assert dev.lib.ekf_observe_model_assigned(dev.h, arr33, 0) == bad and "between 1 and" in dev.lib.ekf_last_error(dev.h).decode()
    assert dev.lib.ekf_observe_model_assigned(dev.h, arr33, 33) == bad and "between 1 and" in dev.lib.ekf_last_error(dev.h).decode()
    assert dev.lib.ekf_observe_model_assigned(dev.h, None, 3) == bad and "null" in dev.lib.ekf_last_error(dev.h).decode()
    for ent, text in ((dict(entries[0], gate=float("nan")), "NaN"), (dict(entries[0], gate=INF), "finite"), (dict(entries[0], gate=-INF), "finite"),
                      (dict(entries[0], model=5, z=entries[0]["z"][:1], R=0.1), "LANDMARK_RANGE")):
        st, msg = status_of(lambda: dev.observe_model_assigned(entries[:4] + [ent]))
        assert st == bad and "observe_model_assigned" in msg and text in msg, msg
    assert status_of(dev.assigned_scan_result)[0] == L.EKF_ERR_STATE            # a refused scan is no scan
    assert dev.pending() == 3
    assert_same(dev, twin)
    dev.close(); twin.close()
    # a shard group of 2 on one GPU: refused as observe_model is, the arguments first
    g, gt = ShardGroup(2, capacity=C.SCENE_N + 8, tile=16), ShardGroup(2, capacity=C.SCENE_N + 8, tile=16)
    g.load_lowrank_state(*data); gt.load_lowrank_state(*data)
    st, msg = status_of(lambda: g.observe_model_assigned(entries))
    assert st == bad and "shard" in msg
    st, msg = status_of(lambda: g.observe_model_assigned([dict(entries[0], gate=INF)]))
    assert st == bad and "shard" not in msg
    assert [e.pending() for e in g.shards] == [0, 0]
    np.testing.assert_array_equal(g.get_x(), gt.get_x()); np.testing.assert_array_equal(g.get_P(), gt.get_P())
    g.close(); gt.close()
    # between ekf_correct_begin and _finish (a lone shard on the sharded code path)
    N = 60
    x = lowrank_data(N, 5)[0]
    kw = dict(capacity=N + 4, tile=16)
    e, twin = helpers.loaded(N, 5, force_sharded=1, **kw), helpers.loaded(N, 5, **kw)
    few = [A.entry(M.RELATIVE_XY, M.h_of(M.RELATIVE_XY, x[:3], x[3 + 2 * k:5 + 2 * k]) + [0.05, -0.05], RPOS, 30.0) for k in (1, 20, 41)]
    z = observe(x, 7)
    e.predict(U2); twin.predict(U2)
    e.correct_begin(z, R2, 7)
    st, msg = status_of(lambda: e.observe_model_assigned(few))
    assert st == L.EKF_ERR_STATE and "observe_model_assigned" in msg and "begin and finish" in msg
    harr = (ctypes.c_void_p * 1)(e.h)
    assert e.lib.ekf_exchange_local(harr, 1) == 0
    e.correct_finish()
    twin.correct(z, R2, 7)
    assert_same_after(e, twin)
    e.close(); twin.close()


# ------------------------------------------------------------------------------------------------------------------
# 5. a recorded predict in front of the scan
# ------------------------------------------------------------------------------------------------------------------
def test_a_recorded_predict_is_carried_out_first():
    data, entries = scene()
    dev, twin = started(data, 3, tile=16, batch=4), started(data, 3, tile=16, batch=4)
    dev.predict(U2); twin.predict(U2)
    dev.observe_model_assigned(entries)
    res, _ = reference_sequence(twin, entries)
    for key in RESULT_KEYS:
        np.testing.assert_array_equal(dev.assigned_scan_result()[key], res[key], err_msg=key)
    assert_same_after(dev, twin)
    dev.close(); twin.close()


# ------------------------------------------------------------------------------------------------------------------
# 6. beside an asynchronous pass: the scan crosses batch boundaries and starts passes in the middle
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage", [(16, "f64"), (64, "f32")])
def test_a_scan_that_starts_asynchronous_passes_midway(tile, storage):
    data, entries = scene()
    kw = dict(tile=tile, storage=storage, batch=4, async_flush=1)
    dev, twin = started(data, 3, **kw), started(data, 3, **kw)
    dev.observe_model_assigned(entries)
    res, _ = reference_sequence(twin, entries)
    assert_scene_premises(res)
    assert_same_after(dev, twin)
    dev.close(); twin.close()


# ------------------------------------------------------------------------------------------------------------------
# 7. two scans queued, one fetch
# ------------------------------------------------------------------------------------------------------------------
def test_two_scans_queued_with_a_motion_step_between_them_and_one_fetch():
    from ekf_slam_amd import _lib as L
    data, first = scene()
    _, second = scene(m=8, seed=2)
    step = [(L.EKF_MOTION_TURN_DRIVE, [0.05, 0.5], np.diag([1e-4, 1e-2]))]
    dev, twin = started(data, 3, tile=16, batch=4), started(data, 3, tile=16, batch=4)
    dev.observe_model_assigned(first)
    dev.predict_model(step)
    dev.observe_model_assigned(second)
    reference_sequence(twin, first)
    twin.predict_model(step)
    res, _ = reference_sequence(twin, second)
    got = dev.assigned_scan_result()
    assert got["landmark"].size == 8 and np.any(res["landmark"] >= 0)
    for key in RESULT_KEYS:
        np.testing.assert_array_equal(got[key], res[key], err_msg=key)
    assert_same_after(dev, twin)
    dev.close(); twin.close()


# ------------------------------------------------------------------------------------------------------------------
# 8. two runs give the same bits
# ------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits():
    data, entries = scene()
    runs = []
    for _ in range(2):
        e = started(data, 3, tile=64, storage="f32", batch=4)
        e.observe_model_assigned(entries)
        got = e.assigned_scan_result()
        runs.append([got[key] for key in sorted(got)] + helpers.getters(e))
        e.close()
    for a, b in zip(*runs):
        np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------------------------------------------------------
# 9. the policy
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,gate_new,far", [(12, C.SCENE_GATE, True), (12, 4.0 * C.SCENE_GATE, True), (32, 4.0 * C.SCENE_GATE, False)])
def test_the_policy_on_the_device_is_the_default_path(tmp_path, m, gate_new, far):
    """The contention scene (m = 12, with one more sighting far from every landmark: a new one under either gate_new, classified from
    ncand alone where gate_new == gate_match and through the one associate_model call behind the steps where it is larger) and the scene of
    test_measure_model_assigned_matches_what_measure_model_discards_and_replays (m = 32)."""
    from ekf_slam_amd.slam import EKF_SLAM
    from ekf_slam_amd.trajectory import _FORMATS, TrajectoryLog
    x, s, d, U, scan, _ = C.contention_scene(m=m)
    if far:
        scan = scan + [(M.RELATIVE_XY, np.array([60.0, 45.0]), RPOS)]
    m = len(scan)
    for storage, tile in (("f64", 16), ("f32", 64)):
        kw = dict(capacity=C.SCENE_N + 40, tile=tile, storage=storage, batch=8 if m == 32 else 4)

        def start():
            f = EKF_SLAM(**kw)
            f._e.load_lowrank_state(x, s, d, U)
            return f

        old, new = start(), start()
        new.log = TrajectoryLog()
        want = old.measure_model_assigned(scan, C.SCENE_GATE, gate_new)
        out = new.measure_model_assigned(scan, C.SCENE_GATE, gate_new, device_apply=True)
        assert out == want and sum(kind == "matched" for kind, _ in out) >= 6
        assert (out[-1] == ("new", C.SCENE_N + 1)) == far and new._e.N == C.SCENE_N + far
        assert new._e.pending() == m % kw["batch"]
        if storage == "f64":                                  # flushed, the default path's state bit for bit
            assert_same(new._e, old._e)
        new.predict(U2)
        new.log.record(U2, None, [], [])                      # (what measure() records of a step without sightings: the edits replay in front of it)
        path = tmp_path / ("assigned_%s_%d.npz" % (storage, m))
        new.log.save(path)
        assert str(np.load(path)["format"]) in _FORMATS and len(_FORMATS) == 10
        log = TrajectoryLog.load(path)
        assert [ed[1] for ed in log.edits] == ["observe_model"] * m + ["append_model"] * far
        fresh = engine(**kw)
        fresh.load_lowrank_state(x, s, d, U)
        log.replay(fresh)
        assert_same(fresh, new._e)
        for e in (fresh, old._e, new._e):
            e.close()
