"""CPU: map edits in the trajectory log (ekf_slam_amd/trajectory.py).  A log with edits round-trips through its file (format 2);
a log without edits is still written as format 1 with the same arrays, and a file of that format loads; replay applies every
edit between the right steps, through the engine's methods of those names, with 0-based numbers."""
import numpy as np
import pytest

from ekf_slam_amd.trajectory import FORMAT, FORMAT_EDITS, TrajectoryLog


def _log(steps=4):
    rng = np.random.default_rng(3)
    t = TrajectoryLog()
    for k in range(steps):
        m = k % 3                                           # a step without observations among them
        t.record(rng.normal(size=2), rng.normal(size=(m, 3)), np.arange(1, 4 + k, dtype=np.float64), rng.normal(size=(3 + k, 2)))
    return t


class _Recording:
    def __init__(self):
        self.calls = []

    def predict(self, u):
        self.calls.append(("predict", tuple(u)))

    def measure(self, obs, u, idx, loc):
        self.calls.append(("measure", len(obs)))

    def remove_landmarks(self, idx):
        self.calls.append(("remove", list(idx)))

    def constrain_landmarks(self, i, j, delta=None, R=None):
        self.calls.append(("constrain", i, j, np.asarray(delta).tolist(), np.asarray(R).tolist()))

    def merge_landmarks(self, keep, drop, R=None):
        self.calls.append(("merge", keep, drop, np.asarray(R).tolist()))


def test_a_log_without_edits_is_saved_as_before_and_an_old_file_loads(tmp_path):
    t = _log()
    path = str(tmp_path / "plain.npz")
    t.save(path)
    g = np.load(path, allow_pickle=False)
    assert str(g["format"]) == FORMAT == "ekfslam-trajectory-1"
    assert sorted(g.files) == sorted(["format", "u", "obs_ptr", "obs", "lm_ptr", "lm_index", "lm_loc"])
    back = TrajectoryLog.load(path)
    assert len(back) == len(t) and back.edits == []
    for k in range(len(t)):
        np.testing.assert_array_equal(back.u[k], t.u[k])
        np.testing.assert_array_equal(back.obs[k], t.obs[k])
        np.testing.assert_array_equal(back.lm_index[k], t.lm_index[k])
        np.testing.assert_array_equal(back.lm_loc[k], t.lm_loc[k])
    # a file written by hand in the old format, with nothing but the old arrays
    old = str(tmp_path / "old.npz")
    np.savez_compressed(old, format=np.array("ekfslam-trajectory-1"), u=np.array([[0.1, 2.0]]), obs_ptr=np.array([0, 1]),
                        obs=np.array([[1.0, 2.0, 3.0]]), lm_ptr=np.array([0, 2]), lm_index=np.array([1.0, 2.0]), lm_loc=np.zeros((2, 2)))
    assert len(TrajectoryLog.load(old)) == 1
    bad = str(tmp_path / "bad.npz")
    np.savez_compressed(bad, format=np.array("something-else"), u=np.zeros((0, 2)))
    with pytest.raises(ValueError):
        TrajectoryLog.load(bad)


def test_a_log_with_edits_round_trips(tmp_path):
    t = TrajectoryLog()
    src = _log(4)
    R = np.array([[0.5, 0.1], [0.1, 0.25]])
    for k in range(4):
        if k == 2:
            t.record_edit("remove", [7, 2, 5])
            t.record_edit("merge", [3, 9], None, R)
        t.record(src.u[k], src.obs[k], src.lm_index[k], src.lm_loc[k])
        if k == 0:
            t.record_edit("constrain", np.array([4.0, 1.0]), [0.5, -1.0], None)
    t.record_edit("remove", 6)                              # after the last step
    assert [e[0] for e in t.edits] == [1, 2, 2, 4]
    path = str(tmp_path / "edited.npz")
    t.save(path)
    g = np.load(path, allow_pickle=False)
    assert str(g["format"]) == FORMAT_EDITS == "ekfslam-trajectory-2"
    assert {"edit_step", "edit_kind", "edit_ptr", "edit_idx", "edit_delta", "edit_R"} <= set(g.files)
    back = TrajectoryLog.load(path)
    assert len(back) == 4 and len(back.edits) == 4
    for a, b in zip(back.edits, t.edits):
        assert a[0] == b[0] and a[1] == b[1] and a[2].tolist() == b[2].tolist()
        np.testing.assert_array_equal(a[3], b[3])
        np.testing.assert_array_equal(a[4], b[4])
    assert back.edits[0][1:3] == ("constrain", ) + (back.edits[0][2],) and back.edits[0][2].tolist() == [4, 1]
    assert back.edits[0][3].tolist() == [0.5, -1.0] and back.edits[0][4].tolist() == [[0.0, 0.0], [0.0, 0.0]]
    assert back.edits[2][4].tolist() == R.tolist()
    for bad in (lambda: t.record_edit("drop", [1]), lambda: t.record_edit("merge", [1, 2, 3]), lambda: t.record_edit("remove", [1.5])):
        with pytest.raises(ValueError):
            bad()


def test_replay_applies_every_edit_between_the_right_steps():
    t = TrajectoryLog()
    src = _log(4)
    R = np.array([[0.5, 0.1], [0.1, 0.25]])
    for k in range(4):
        if k == 2:
            t.record_edit("remove", [7, 2])
            t.record_edit("merge", [3, 9], None, R)
        t.record(src.u[k], src.obs[k], src.lm_index[k], src.lm_loc[k])
        if k == 0:
            t.record_edit("constrain", [4, 1], [0.5, -1.0], None)
    t.record_edit("remove", [6])
    e = _Recording()
    t.replay(e)
    kinds = [c[0] for c in e.calls]
    # steps 0 and 3 have no observations (m = k % 3): predict alone
    assert kinds == ["predict", "predict", "constrain", "measure", "remove", "merge", "predict", "measure", "predict", "remove"] or \
        kinds == ["predict", "constrain", "predict", "measure", "remove", "merge", "predict", "measure", "predict", "remove"]
    assert kinds.index("constrain") == 1 + (0 if len(src.obs[0]) == 0 else 1)      # after step 0, before step 1's predict
    assert e.calls[kinds.index("constrain")] == ("constrain", 3, 0, [0.5, -1.0], [[0.0, 0.0], [0.0, 0.0]])    # 0-based at the engine
    assert ("remove", [6, 1]) in e.calls and ("merge", 2, 8, R.tolist()) in e.calls and e.calls[-1] == ("remove", [5])
    # a replay in two halves applies each edit exactly once
    a = _Recording()
    t.replay(a, 0, 2)
    t.replay(a, 2)
    assert a.calls == e.calls
