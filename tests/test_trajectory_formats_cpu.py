"""CPU: the eight file formats of the trajectory log against files written before the kinds moved into one table
(tests/golden/trajectory/format1.npz .. format8.npz, from make_logs.py beside them).  For every format: load, then save, gives the
fixture back member by member, and a replay hands an engine the calls written out below -- method, 0-based indices, values -- in one
piece and split at step 2.  No GPU."""
import os

import numpy as np
import pytest

from helpers import ROOT, same_npz

INF = float("inf")
GOLDEN = os.path.join(ROOT, "tests", "golden", "trajectory")
RPOS = [[0.5, 0.125], [0.125, 0.25]]
ZERO = [[0.0, 0.0], [0.0, 0.0]]
M2 = [[0.25, 0.0625], [0.0625, 0.5]]
M3 = [[0.5, 0.125, 0.0], [0.125, 0.25, 0.0625], [0.0, 0.0625, 2.0]]
FORMATS = range(1, 9)


def _l(a):
    return None if a is None else np.asarray(a).tolist()


class _Engine:
    """Records what replay hands over, every array as a list."""

    def __init__(self):
        self.calls = []

    def predict(self, u):
        self.calls.append(("predict", _l(u)))

    def measure(self, obs, u, idx, loc):
        self.calls.append(("measure", _l(obs), _l(u), _l(idx), _l(loc)))

    def remove_landmarks(self, idx):
        self.calls.append(("remove_landmarks", list(idx)))

    def constrain_landmarks(self, i, j, delta, R):
        self.calls.append(("constrain_landmarks", i, j, _l(delta), _l(R)))

    def merge_landmarks(self, keep, drop, R):
        self.calls.append(("merge_landmarks", keep, drop, _l(R)))

    def merge_landmarks_batch(self, pairs, R):
        self.calls.append(("merge_landmarks_batch", [tuple(p) for p in pairs], _l(R)))

    def observe_linear(self, z, R, Hr, landmarks, Hl, gate, wrap, rows):
        self.calls.append(("observe_linear", _l(z), _l(R), _l(Hr), list(landmarks), [_l(b) for b in Hl], gate, tuple(wrap), rows))

    def observe_model(self, model, z, R, landmarks, anchor, gate):
        self.calls.append(("observe_model", model, _l(z), _l(R), list(landmarks), _l(anchor), gate))

    def observe_model_iterated(self, model, z, R, landmarks, anchor, gate, iterations, tol):
        self.calls.append(("observe_model_iterated", model, _l(z), _l(R), list(landmarks), _l(anchor), gate, iterations, tol))

    def append_model(self, entries):
        self.calls.append(("append_model", [(m, _l(z), _l(R), s) for m, z, R, s in entries]))

    def predict_model(self, steps):
        self.calls.append(("predict_model", [(m, _l(u), _l(M)) for m, u, M in steps]))


# ------------------------------------------------------------------------------------------------------------------
# what a replay of format n's fixture hands over: the steps, and per kind the call it makes and the first format that holds it
# ------------------------------------------------------------------------------------------------------------------
TABLE = ([1.0, 2.0, 3.0], lambda k: [[0.0, 1.0], [2.0, 3.0], [4.0, 5.0 + k]])


def _step(k):
    calls = [("predict", [0.125, 1.0 + k])]
    if k != 1:                                                # the second step saw nothing: no measure
        calls.append(("measure", [[1.0 + k, 2.0, 3.0], [4.0, 5.0 + k, 6.0]], [0.125, 1.0 + k], TABLE[0], TABLE[1](k)))
    return calls


GROUP_A = [      # after step 0, in front of step 1
    (2, ("remove_landmarks", [6, 1])),
    (2, ("constrain_landmarks", 0, 1, [0.5, -0.25], RPOS)),
    (4, ("observe_linear", [1.0, 2.0], RPOS, [[1.0, 0.0, 0.5], [0.0, 1.0, -0.25]], [3, 1], [[[1.0, 2.0], [3.0, 4.0]], [[-1.0, -0.0], [-0.0, -1.0]]],
         9.25, (0, 1), 2)),
    (5, ("observe_model", 1, [5.0, 30.0], RPOS, [3], None, 9.25)),
    (6, ("append_model", [(1, [5.0, 30.0], RPOS, 11.0), (4, [2.0, -1.0], [[1.0, 0.25], [0.25, 0.5]], 12.0)])),
    (8, ("observe_model_iterated", 5, [2.5, 0.0], [[0.125, 0.0], [0.0, 0.0]], [2, 8], None, 4.0, 5, 0.5 ** 20)),
]
GROUP_B = [      # after step 1, in front of step 2
    (2, ("merge_landmarks", 2, 4, ZERO)),
    (3, ("merge_landmarks_batch", [(2, 4), (2, 5)], RPOS)),
    (4, ("observe_linear", [175.0], [[0.5, 0.0], [0.0, 0.0]], [[0.0, 0.0, 1.0], [0.0, 0.0, 0.0]], [], [], INF, (1, 0), 1)),
    (5, ("observe_model", 2, [7.5, 0.0], [[0.5, 0.0], [0.0, 0.0]], [], [10.0, -4.0], INF)),
    (7, ("predict_model", [(1, [0.5, 3.0], M2), (3, [0.25, -0.125, 1.5], M3)])),
    (8, ("observe_model_iterated", 3, [12.0, 0.0], [[0.25, 0.0], [0.0, 0.0]], [], [10.0, -4.0], INF, 16, 0.0)),
]
LAST = [(2, ("constrain_landmarks", 1, 0, [0.0, 0.0], ZERO))]       # after the last step


def _held(group, n):
    return [call for first, call in group if first <= n]


def expected_calls(n):
    return _step(0) + _held(GROUP_A, n) + _step(1) + _held(GROUP_B, n) + _step(2) + _held(LAST, n)


def fixture(n):
    return os.path.join(GOLDEN, "format%d.npz" % n)


@pytest.mark.parametrize("n", FORMATS)
def test_load_then_save_gives_the_fixture_back(tmp_path, n):
    from ekf_slam_amd.trajectory import _FORMATS, TrajectoryLog
    assert str(np.load(fixture(n))["format"]) == _FORMATS[n - 1] == "ekfslam-trajectory-%d" % n
    log = TrajectoryLog.load(fixture(n))
    assert len(log) == 3 and len(log.edits) == len(_held(GROUP_A + GROUP_B + LAST, n))
    log.save(tmp_path / "again.npz")
    assert same_npz(fixture(n), tmp_path / "again.npz")


@pytest.mark.parametrize("n", FORMATS)
def test_replay_hands_the_engine_the_calls_written_out(n):
    from ekf_slam_amd.trajectory import TrajectoryLog
    log = TrajectoryLog.load(fixture(n))
    whole = _Engine()
    log.replay(whole)
    assert whole.calls == expected_calls(n)
    split = _Engine()
    log.replay(split, 0, 2)
    assert split.calls == _step(0) + _held(GROUP_A, n) + _step(1)          # the edits in front of step 2 belong to the second piece
    log.replay(split, 2)
    assert split.calls == expected_calls(n)


def test_the_generator_reproduces_the_fixtures(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_logs", os.path.join(GOLDEN, "make_logs.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    for n in FORMATS:
        gen.make(n).save(tmp_path / ("format%d.npz" % n))
        assert same_npz(fixture(n), tmp_path / ("format%d.npz" % n)), n
