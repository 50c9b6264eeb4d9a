"""CPU: the Engine and slam methods that no other test_*_cpu.py reaches, over a stand-in for the loaded library -- the x, P and s
setters and set_state, associate and associate_finish with and without costs, the prefetch family, remove_landmarks, f, and a refused
ekf_create.  The expectations are written out by hand: the scalars, the array contents and the null-ness that arrive at each entry point,
and what comes back.  No GPU."""
import numpy as np
import pytest

from helpers import RecorderBase

R2 = [[0.5, 0.125], [0.25, 2.0]]             # not symmetric, so that the order it travels in shows: column-major 0.5, 0.25, 0.125, 2.0
R2_COLMAJOR = [0.5, 0.25, 0.125, 2.0]


class _Recorder(RecorderBase):
    status_string = b"landmark index outside the state"
    last_error = b"layer: injected"

    def __init__(self, N=3):
        self.calls, self.fail, self.N, self.create, self.handle = [], 0, N, 0, 0x1000

    def ekf_create(self, pcfg, ph):
        super().ekf_create(pcfg, ph)
        ph._obj.value = self.handle
        self.calls.append(("create",))
        return self.create

    def ekf_destroy(self, h):
        self.calls.append(("destroy", h.value))
        return 0

    def ekf_last_error(self, h):
        self.calls.append(("last_error", h.value))
        return self.last_error

    def ekf_num_landmarks(self, h, pn):
        pn._obj.value = self.N
        return 0

    def ekf_set_x(self, h, px, n):
        self.calls.append(("set_x", [px[i] for i in range(n)], n))
        return self.fail

    def ekf_set_s(self, h, ps, n):
        self.calls.append(("set_s", None if ps is None else [ps[i] for i in range(n)], n))
        return self.fail

    def ekf_set_P(self, h, pP, n):
        self.calls.append(("set_P", [pP[i] for i in range(n * n)], n))
        return self.fail

    def _answer(self, pnew, pidx, ppc, psc):
        pnew._obj.value, pidx._obj.value = 1, 2
        for k in range(self.N):
            if ppc is not None:
                ppc[k], psc[k] = 10.0 + k, 20.0 + k

    def ekf_associate(self, h, pz, pR, pnew, pidx, ppc, psc):
        self.calls.append(("associate", [pz[i] for i in range(3)], [pR[i] for i in range(4)], ppc is None, psc is None))
        self._answer(pnew, pidx, ppc, psc)
        return self.fail

    def ekf_associate_begin(self, h, pz, pR, want):
        self.calls.append(("associate_begin", [pz[i] for i in range(3)], [pR[i] for i in range(4)], want))
        return self.fail

    def ekf_associate_finish(self, h, pnew, pidx, ppc, psc):
        self.calls.append(("associate_finish", ppc is None, psc is None))
        self._answer(pnew, pidx, ppc, psc)
        return self.fail

    def _indices(self, name, arr, n):
        assert len(arr) >= n
        self.calls.append((name, [arr[i] for i in range(n)], n))
        return self.fail

    def ekf_prefetch_rows(self, h, arr, n):
        return self._indices("prefetch_rows", arr, n)

    def ekf_prefetch_next(self, h, arr, n):
        return self._indices("prefetch_next", arr, n)

    def ekf_prefetch_begin(self, h, arr, n):
        return self._indices("prefetch_begin", arr, n)

    def ekf_prefetch_finish(self, h):
        self.calls.append(("prefetch_finish",))
        return self.fail

    def ekf_remove_landmarks(self, h, arr, n):
        return self._indices("remove", arr, n)

    def ekf_motion_model(self, px, n, pu, pxn, pF):
        self.calls.append(("motion_model", [px[i] for i in range(n)], n, [pu[0], pu[1]]))
        for i in range(n):
            pxn[i] = 100.0 + i
        for i in range(n * n):
            pF[i] = float(i)
        return self.fail


def _engine(monkeypatch, rec, **kw):
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import engine as E
    monkeypatch.setattr(L, "lib", lambda: rec)
    return E.Engine(capacity=16, **kw)


def test_set_state_and_the_slam_setters_hand_over_the_same_three_calls(monkeypatch):
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import slam as S
    rec = _Recorder()
    e = _engine(monkeypatch, rec)
    x = [1.0, 2.0, 3.0, 4.0, 5.0]
    P = np.arange(25.0).reshape(5, 5)                        # row-major 0..24: column-major on the wire
    rec.calls.clear()
    e.set_state(x, P, [7.0])
    assert rec.calls == [("set_x", x, 5), ("set_s", [7.0], 1), ("set_P", P.T.reshape(-1).tolist(), 5)]      # x, then s, then P
    rec.calls.clear()
    e.set_state(np.array([[1.0, 2.0, 3.0]]), np.eye(3), [])          # no landmark: s travels as a null pointer and a count of 0
    assert rec.calls == [("set_x", [1.0, 2.0, 3.0], 3), ("set_s", None, 0), ("set_P", np.eye(3).reshape(-1).tolist(), 3)]
    for cls in (S.EKF_SLAM, S.EKF_SLAM_UC):
        f = cls(capacity=16)
        rec.calls.clear()
        f.x = np.array(x).reshape(1, 5)                      # the reference's 1 x n row vector
        f.P = P.tolist()
        f.s = (7.0,)
        f.s = []
        assert rec.calls == [("set_x", x, 5), ("set_P", P.T.reshape(-1).tolist(), 5), ("set_s", [7.0], 1), ("set_s", None, 0)]
        rec.fail = L.EKF_ERR_INDEX
        for assign in (lambda: setattr(f, "x", x), lambda: setattr(f, "P", P), lambda: setattr(f, "s", [1.0])):
            with pytest.raises(L.EkfError) as info:
                assign()
            assert info.value.status == L.EKF_ERR_INDEX and str(info.value) == "libekfslam status 5: landmark index outside the state: layer: injected"
        rec.fail = 0


def test_associate_with_and_without_costs_and_around_a_host_exchange(monkeypatch):
    from ekf_slam_amd import _lib as L
    rec = _Recorder(N=3)
    e = _engine(monkeypatch, rec)
    z = [1.0, 2.0, 3.0]
    assert e.associate(z, R2) == (True, 2)
    assert rec.calls[-1] == ("associate", z, R2_COLMAJOR, True, True)                  # no costs asked for: two null pointers
    is_new, idx, pc, sc = e.associate(z, R2, want_costs=True)
    assert rec.calls[-1] == ("associate", z, R2_COLMAJOR, False, False)
    assert (is_new, idx) == (True, 2) and pc.tolist() == [10.0, 11.0, 12.0] and sc.tolist() == [20.0, 21.0, 22.0]
    assert e.associate_finish() == (True, 2) and rec.calls[-1] == ("associate_finish", True, True)
    is_new, idx, pc, sc = e.associate_finish(want_costs=True)
    assert rec.calls[-1] == ("associate_finish", False, False) and pc.tolist() == [10.0, 11.0, 12.0] and sc.tolist() == [20.0, 21.0, 22.0]
    e.associate_begin(z, R2)
    assert rec.calls[-1] == ("associate_begin", z, R2_COLMAJOR, 0)
    e.associate_begin(z, R2, want_costs=True)
    assert rec.calls[-1] == ("associate_begin", z, R2_COLMAJOR, 1)
    with pytest.raises(ValueError):
        e.associate([1.0, 2.0], R2)                           # z is (range, bearing, signature)
    # an empty map: the cost arrays have one slot for the library to ignore, and come back empty
    rec.N = 0
    is_new, idx, pc, sc = e.associate(z, R2, want_costs=True)
    assert rec.calls[-1][3:] == (False, False) and pc.size == 0 and sc.size == 0
    rec.N = 3
    # the all-gather done by the host: begin, the exchange, finish -- only where the position cost needs the other shards
    e._host_exchange = lambda eng: rec.calls.append(("exchange",))
    n = len(rec.calls)
    assert e.associate(z, R2) == (True, 2)                                             # w_pos = 0, no costs: the plain call
    assert [c[0] for c in rec.calls[n:]] == ["associate"]
    n = len(rec.calls)
    out = e.associate(z, R2, want_costs=True)
    assert rec.calls[n:] == [("associate_begin", z, R2_COLMAJOR, 1), ("exchange",), ("associate_finish", False, False)] and out[2].tolist() == [10.0, 11.0, 12.0]
    e.cfg.w_pos = 0.5
    n = len(rec.calls)
    assert e.associate(z, R2) == (True, 2)
    assert rec.calls[n:] == [("associate_begin", z, R2_COLMAJOR, 0), ("exchange",), ("associate_finish", True, True)]
    rec.fail = L.EKF_ERR_INDEX
    for call in (lambda: e.associate_begin(z, R2), e.associate_finish):
        with pytest.raises(L.EkfError) as info:
            call()
        assert info.value.status == L.EKF_ERR_INDEX and "layer: injected" in str(info.value)


def test_estimate_correspondence_loads_a_scratch_engine_and_reports_one_based(monkeypatch):
    from ekf_slam_amd import slam as S
    rec = _Recorder(N=1)
    _engine(monkeypatch, rec).close()
    rec.calls.clear()
    c = S.Correspondence(1e-11, 1e9, "EKF_SLAM_UC")
    is_new, idx = c.estimateCorrespondence([1.0, 2.0, 3.0], R2, [1.0, 2.0, 3.0, 4.0, 5.0], np.eye(5), [9.0])
    assert (is_new, idx) == (True, 3) and c.position_cost.tolist() == [10.0] and c.signature_cost.tolist() == [20.0]
    assert rec.calls == [("create",), ("set_x", [1.0, 2.0, 3.0, 4.0, 5.0], 5), ("set_s", [9.0], 1), ("set_P", np.eye(5).reshape(-1).tolist(), 5),
                         ("associate", [1.0, 2.0, 3.0], R2_COLMAJOR, False, False), ("destroy", 0x1000)]


def test_the_prefetch_family_and_remove_landmarks_hand_over_int64_indices(monkeypatch):
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import slam as S
    rec = _Recorder()
    e = _engine(monkeypatch, rec)
    rec.calls.clear()
    e.prefetch_rows([4, 0, np.int64(7)])
    e.prefetch_next((2, 2))
    e.prefetch_begin([5])
    e.prefetch_finish()
    e.prefetch_rows([])
    assert rec.calls == [("prefetch_rows", [4, 0, 7], 3), ("prefetch_next", [2, 2], 2), ("prefetch_begin", [5], 1), ("prefetch_finish",),
                         ("prefetch_rows", [], 0)]
    e.remove_landmarks(iter([3, 1]))
    assert rec.calls[-1] == ("remove", [3, 1], 2)
    e.remove_landmarks([])
    assert rec.calls[-1] == ("remove", [], 0)
    # the host-run all-gather: prefetch_rows is begin, the exchange, finish; prefetch_next cannot run inside the library's flush
    e._host_exchange = lambda eng: rec.calls.append(("exchange",))
    rec.calls.clear()
    e.prefetch_rows([1, 6])
    assert rec.calls == [("prefetch_begin", [1, 6], 2), ("exchange",), ("prefetch_finish",)]
    with pytest.raises(L.EkfError) as info:
        e.prefetch_next([1])
    assert info.value.status == L.EKF_ERR_STATE and str(info.value) == \
        "libekfslam status 7: prefetch_next: the host-run all-gather cannot run inside the library's flush"
    assert len(rec.calls) == 3
    e._host_exchange = None
    rec.fail = L.EKF_ERR_INDEX
    for call in (lambda: e.prefetch_rows([1]), lambda: e.prefetch_next([1]), lambda: e.prefetch_begin([1]), e.prefetch_finish,
                 lambda: e.remove_landmarks([1])):
        with pytest.raises(L.EkfError) as info:
            call()
        assert info.value.status == L.EKF_ERR_INDEX
    rec.fail = 0
    # slam: 1-based, a number or any iterable, whole numbers; logged after the call
    from ekf_slam_amd.trajectory import TrajectoryLog
    f = S.EKF_SLAM(capacity=16)
    f.log = TrajectoryLog()
    f.remove_landmarks(4)
    assert rec.calls[-1] == ("remove", [3], 1)
    f.remove_landmarks([2.0, 7])
    assert rec.calls[-1] == ("remove", [1, 6], 2)
    assert [(k, kind, idx.tolist()) for k, kind, idx, _, _ in f.log.edits] == [(0, "remove", [4]), (0, "remove", [2, 7])]
    n = len(rec.calls)
    with pytest.raises(ValueError) as bad:
        f.remove_landmarks([1.5])
    assert str(bad.value) == "remove_landmarks: landmark indices are whole numbers" and len(rec.calls) == n and len(f.log.edits) == 2
    rec.fail = L.EKF_ERR_INDEX
    with pytest.raises(L.EkfError):
        f.remove_landmarks([1])
    assert len(f.log.edits) == 2                              # a refused call is not logged


def test_f_hands_the_motion_model_the_state_and_reads_F_column_major(monkeypatch):
    from ekf_slam_amd import _lib as L
    from ekf_slam_amd import slam as S
    rec = _Recorder()
    monkeypatch.setattr(L, "lib", lambda: rec)
    f = S.EKF_SLAM(capacity=16)
    x_new, F = f.f([[1.0, 2.0, 3.0, 4.0, 5.0]], [0.5, 30.0])
    assert rec.calls[-1] == ("motion_model", [1.0, 2.0, 3.0, 4.0, 5.0], 5, [0.5, 30.0])
    assert x_new.tolist() == [100.0, 101.0, 102.0, 103.0, 104.0] and F.shape == (5, 5) and F[1, 0] == 1.0 and F[0, 1] == 5.0 and F[4, 3] == 19.0
    n = len(rec.calls)
    with pytest.raises(ValueError):
        f.f([1.0, 2.0, 3.0], [0.5, 30.0, 1.0])                # u is (d, turn)
    assert len(rec.calls) == n
    rec.fail = L.EKF_ERR_INVALID_ARG
    with pytest.raises(L.EkfError) as info:
        f.f([1.0, 2.0, 3.0], [0.5, 30.0])
    assert info.value.status == L.EKF_ERR_INVALID_ARG and str(info.value) == "libekfslam status 1: ekf_motion_model"


def test_a_refused_create_reads_the_message_destroys_the_handle_and_raises(monkeypatch):
    from ekf_slam_amd import _lib as L
    rec = _Recorder()
    rec.create = L.EKF_ERR_CAPACITY
    with pytest.raises(L.EkfError) as info:
        _engine(monkeypatch, rec)
    assert info.value.status == L.EKF_ERR_CAPACITY and str(info.value) == "libekfslam status 4: landmark index outside the state: layer: injected"
    assert rec.calls == [("create",), ("last_error", 0x1000), ("destroy", 0x1000)]          # the message is read while the handle lives
    # no handle came back: nothing to ask for a message, nothing to destroy
    rec = _Recorder()
    rec.create, rec.handle = L.EKF_ERR_NO_DEVICE, None
    with pytest.raises(L.EkfError) as info:
        _engine(monkeypatch, rec)
    assert info.value.status == L.EKF_ERR_NO_DEVICE and str(info.value) == "libekfslam status 2: landmark index outside the state"
    assert rec.calls == [("create",)]
