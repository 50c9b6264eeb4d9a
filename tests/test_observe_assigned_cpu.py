"""CPU: ekf_observe_model_assigned without a GPU -- the kernel sources of k_gather_model_assigned compiled for the host and compared bit for
bit with k_gather_model (tests/support/model_assigned_host_emulation.cpp), the two symbols in the ctypes binding, and the argument handling
of the Python layers over a stand-in for the library."""
import ctypes
import subprocess

import numpy as np
import pytest

from helpers import RPOS, RecorderBase, host_build


def test_kernel_sources_on_the_host_match_the_host_named_step_bit_for_bit(tmp_path):
    """N = 150 (two workgroups), capacity 158, tiles of edge 16 and 64, 0 and 3 pairs pending.  Per shape: a slot naming landmark 72 (a tile
    edge at T = 16), 0 and N - 1 with models 1-4 against k_gather_model with a.a[0] set on the host (12 lines); a slot of -1 and one of N as
    skipped steps (2); a landmark behind a tight gate (1)."""
    exe = host_build("model_assigned_host_emulation", str(tmp_path / "model_assigned_host_emulation"))
    r = subprocess.run([exe], capture_output=True, text=True)
    lines = r.stdout.strip().split("\n")
    assert r.returncode == 0, r.stdout[-3000:]
    assert len(lines) == 4 * 15 and all(ln.endswith(": 0 differences") for ln in lines), r.stdout[-3000:]
    assert sum("against the host-named step" in ln for ln in lines) == 48 and sum("skipped step" in ln for ln in lines) == 8
    assert sum("tight gate" in ln for ln in lines) == 4


def test_both_symbols_are_bound_and_the_outcome_has_its_number():
    from ekf_slam_amd import _lib as L
    assert len(L.SIGNATURES["ekf_observe_model_assigned"][1]) == 3 and len(L.SIGNATURES["ekf_assigned_scan_result"][1]) == 5
    assert L.EKF_LINEAR_UNASSIGNED == 3
    assert len({L.EKF_LINEAR_IRREGULAR, L.EKF_LINEAR_APPLIED, L.EKF_LINEAR_GATED, L.EKF_LINEAR_UNASSIGNED}) == 4


class _Recorder(RecorderBase):
    """The library as far as a queued scan needs it: the scan is noted, the result says entry 1 of 3 went to landmark 4 and the rest was
    left out, entry 2 with a landmark inside its gate."""
    last_error = b"observe_model_assigned: injected"

    def __init__(self, N=6):
        self.calls, self.N = [], N

    def ekf_num_landmarks(self, h, pN):
        ctypes.cast(pN, ctypes.POINTER(ctypes.c_int64)).contents.value = self.N
        return 0

    def ekf_observe_model_assigned(self, h, arr, m):
        self.calls.append(("scan", [(arr[k].model, list(arr[k].z), list(arr[k].lm), arr[k].gate) for k in range(m)]))
        self.m = m
        return 0

    def ekf_assigned_scan_result(self, h, pm, out, res, ptotal):
        self.calls.append(("result",))
        pm._obj.value = self.m
        for k in range(self.m):
            out[k].landmark, out[k].d2, out[k].ncand = (4, 0.5, 2) if k == 1 else (-1, float("inf"), 1 if k == 2 else 0)
            res[k].outcome, res[k].d2 = (1, 0.25) if k == 1 else (3, float("nan"))
        ptotal._obj.value = 9.5
        return 0

    def ekf_append_model(self, h, arr, m, pfirst):
        self.calls.append(("append", m, arr[0].model, list(arr[0].z)))
        pfirst._obj.value = self.N
        self.N += m
        return 0


def test_python_layers_queue_one_scan_fetch_once_and_log_existing_kinds(monkeypatch):
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import engine as E
    from ekf_slam_amd import slam as S
    from ekf_slam_amd.trajectory import _FORMATS, TrajectoryLog
    rec = _Recorder()
    monkeypatch.setattr(L, "lib", lambda: rec)
    e = E.Engine(capacity=16)
    scan = [dict(model=1, z=[5.0, 30.0], R=RPOS, gate=9.0), dict(model=4, z=[1.0, 2.0], R=RPOS, gate=9.0), dict(model=1, z=[7.0, -3.0], R=RPOS, gate=9.0)]
    assert e.observe_model_assigned(scan) is None
    assert rec.calls == [("scan", [(1, [5.0, 30.0], [-1, -1], 9.0), (4, [1.0, 2.0], [-1, -1], 9.0), (1, [7.0, -3.0], [-1, -1], 9.0)])]
    res = e.assigned_scan_result()
    assert set(res) == {"landmark", "d2", "ncand", "total", "nu", "S", "outcome", "step_d2"}
    assert res["landmark"].tolist() == [-1, 4, -1] and res["ncand"].tolist() == [0, 2, 1] and res["total"] == 9.5
    assert res["outcome"].tolist() == [3, 1, 3] and res["step_d2"][1] == 0.25 and np.isnan(res["step_d2"][[0, 2]]).all()
    assert res["nu"].shape == (3, 2) and res["S"].shape == (3, 2, 2)
    for cls in (S.EKF_SLAM, S.EKF_SLAM_UC):
        rec = _Recorder()
        monkeypatch.setattr(L, "lib", lambda: rec)
        f = cls(capacity=16)
        f.log = TrajectoryLog()
        entries = [(1, [5.0, 30.0], RPOS), (4, [1.0, 2.0], RPOS), (1, [7.0, -3.0], RPOS)]
        # gate_new < gate_match is refused with device_apply=True as without, before anything reaches the library
        for device_apply in (False, True):
            with pytest.raises(ValueError):
                f.measure_model_assigned(entries, 9.0, 8.0, device_apply=device_apply)
        assert rec.calls == [] and f.log.edits == []
        out = f.measure_model_assigned(entries, 9.0, 9.0, device_apply=True)
        # entry 0: no candidate, gate_new == gate_match: new (landmark 7); entry 1: matched; entry 2: left out with a candidate: discarded
        assert out == [("new", 7), ("matched", 5), ("discarded", 0)]
        assert [c[0] for c in rec.calls] == ["scan", "result", "append"] and rec.calls[2][1:] == (1, 1, [5.0, 30.0])
        assert [g for _, _, _, g in rec.calls[0][1]] == [9.0, 9.0, 9.0]
        # the log: one observe_model per entry in scan order, then the append -- kinds and a format that exist already
        assert [(kind, idx.tolist()) for _, kind, idx, _, _ in f.log.edits] == \
            [("observe_model", [1]), ("observe_model", [5]), ("observe_model", [1]), ("append_model", [])]
        assert [f.log.model_observations[q]["gate"] for q in range(3)] == [-1.0, 9.0, -1.0]
        assert len(_FORMATS) == 10
