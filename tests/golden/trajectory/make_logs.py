#!/usr/bin/env python3
"""Generate format1.npz .. format8.npz in this directory: one trajectory log per file format of ekf_slam_amd/trajectory.py, written
through TrajectoryLog's recorders alone.  They pin the FILE FORMAT (member names, their order, dtypes, shapes, bytes) and what a replay
hands to an engine; tests/test_trajectory_formats_cpu.py holds the expectations.  The files in git were written by the module as it
stood before its kinds moved into one table; a later run of this script must reproduce them member by member.

Every log has three steps, the second without observations.  Log n holds every kind of edit that format n admits: group A after step 0,
group B after step 1, and one constraint after the last step.  Run from the repo root:  python tests/golden/trajectory/make_logs.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(HERE))))

from ekf_slam_amd.trajectory import TrajectoryLog  # noqa: E402

RPOS = np.array([[0.5, 0.125], [0.125, 0.25]])
M2 = np.array([[0.25, 0.0625], [0.0625, 0.5]])
M3 = np.array([[0.5, 0.125, 0.0], [0.125, 0.25, 0.0625], [0.0, 0.0625, 2.0]])
HR = np.array([[1.0, 0.0, 0.5], [0.0, 1.0, -0.25]])
HL = [np.array([[1.0, 2.0], [3.0, 4.0]]), -np.eye(2)]
VAR = lambda v: [[v, 0.0], [0.0, 0.0]]       # noqa: E731  (a one-row observation's R)


def step(log, k):
    obs = None if k == 1 else np.array([[1.0 + k, 2.0, 3.0], [4.0, 5.0 + k, 6.0]])
    log.record([0.125, 1.0 + k], obs, [1.0, 2.0, 3.0], [[0.0, 1.0], [2.0, 3.0], [4.0, 5.0 + k]])


def group_a(log, n):
    log.record_edit("remove", [7, 2])
    log.record_edit("constrain", [1, 2], [0.5, -0.25], RPOS)
    if n >= 4:
        log.record_observation([1.0, 2.0], RPOS, HR, [4, 2], HL, gate=9.25, wrap=(0, 1), rows=2)
    if n >= 5:
        log.record_model_observation(1, [5.0, 30.0], RPOS, [4], gate=9.25)                       # two rows, a landmark
    if n >= 6:
        log.record_model_append([(1, [5.0, 30.0], RPOS, 11.0), (4, [2.0, -1.0], 2.0 * RPOS, 12.0)])
    if n >= 8:
        log.record_model_observation_iterated(5, [2.5], VAR(0.125), [3, 9], gate=4.0, iterations=5, tol=0.5 ** 20)


def group_b(log, n):
    log.record_edit("merge", [3, 5])
    if n >= 3:
        log.record_edit("merge_batch", [3, 5, 3, 6], None, RPOS)                                 # the keep is shared
    if n >= 4:
        log.record_observation([175.0], VAR(0.5), [[0.0, 0.0, 1.0], [0.0, 0.0, 0.0]], wrap=(1, 0), rows=1)
    if n >= 5:
        log.record_model_observation(2, [7.5], VAR(0.5), anchor=[10.0, -4.0])                    # one row, an anchor
    if n >= 7:
        log.record_model_predict([(1, [0.5, 3.0], M2), (3, [0.25, -0.125, 1.5], M3)])
    if n >= 8:
        log.record_model_observation_iterated(3, [12.0], VAR(0.25), anchor=[10.0, -4.0], iterations=16)


def make(n):
    log = TrajectoryLog()
    step(log, 0)
    if n >= 2:
        group_a(log, n)
    step(log, 1)
    if n >= 2:
        group_b(log, n)
    step(log, 2)
    if n >= 2:
        log.record_edit("constrain", [2, 1], None, None)
    return log


if __name__ == "__main__":
    for n in range(1, 9):
        path = os.path.join(HERE, "format%d.npz" % n)
        make(n).save(path)
        print(path, str(np.load(path)["format"]), os.path.getsize(path), "bytes")
