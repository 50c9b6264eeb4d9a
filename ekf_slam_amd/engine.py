"""Thin object wrapper over the C ABI handle: one Engine == one ekf_handle == one filter state in HBM.  What turns arguments into
what the ABI takes lives in marshal.py; the methods here add the handle, the call and the status check."""
import ctypes

import numpy as np

from . import _lib as L
from . import marshal
from .marshal import _colmajor, _p, _vec, host_call, index_array, noise, p_or_null


class Engine:
    def __init__(self, mode="known", capacity=1024, tile=0, storage="f64", device=0, rank=0, world=1, batch=1,
                 async_flush=False, device_assoc=None, **overrides):
        self.lib = L.lib()
        cfg = L.EkfConfig()
        m = L.EKF_MODE_KNOWN if mode in ("known", "EKF_SLAM") else L.EKF_MODE_UC
        self._check(self.lib.ekf_config_default(ctypes.byref(cfg), m), None)
        cfg.capacity_landmarks = int(capacity)
        cfg.tile = int(tile)
        if storage not in ("f64", "f32", "f32_mixed", "f32_split"):
            raise TypeError("Engine: storage is 'f64', 'f32' (float tiles, F64 arithmetic), 'f32_mixed' (float tiles, the pass over P "
                            "in F32 arithmetic on the matrix pipe: cfg.pass_arith = EKF_ARITH_F32) or 'f32_split' (the same with every "
                            "float operand cut into three bfloat16 pieces, on the bf16 matrix pipe: EKF_ARITH_SPLIT3)")
        cfg.storage = L.EKF_STORE_F64 if storage == "f64" else L.EKF_STORE_F32
        cfg.pass_arith = {"f32_mixed": L.EKF_ARITH_F32, "f32_split": L.EKF_ARITH_SPLIT3}.get(storage, L.EKF_ARITH_F64)
        cfg.device, cfg.rank, cfg.world, cfg.batch = int(device), int(rank), int(world), int(batch)
        cfg.async_flush = 1 if async_flush else 0
        if device_assoc is not None:              # None: the mode's default (uc: 3, the device-resident loop); include/ekfslam.h
            cfg.device_assoc = int(device_assoc)  # 0: host mirror, 1: device, waited for, 2: device, verified before measure() returns
            #                                       4: device-decided branch -- decided AND carried out on the device, any w_pos, unsharded
        fields = {f[0] for f in L.EkfConfig._fields_}
        for k, v in overrides.items():
            if k not in fields:                   # (setattr on a ctypes struct would silently create a Python attribute)
                raise TypeError("Engine: unknown ekf_config field %r" % k)
            if k == "Rc":
                cfg.Rc[0], cfg.Rc[1] = float(v[0]), float(v[1])
            else:
                setattr(cfg, k, v)
        self.cfg = cfg
        self._host_exchange = None
        self._hints = False
        self._raw = None
        self.h = ctypes.c_void_p()
        rc = self.lib.ekf_create(ctypes.byref(cfg), ctypes.byref(self.h))
        if rc != L.EKF_OK:
            err = self._error(rc)                 # (the message is read while the handle lives)
            self.close()
            raise err

    def close(self):
        if getattr(self, "h", None):
            self.lib.ekf_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _error(self, rc, h="self"):
        msg = self.lib.ekf_last_error(self.h).decode() if (h == "self" and self.h) else ""
        return L.EkfError(rc, self.lib.ekf_status_string(rc).decode() + (": " + msg if msg else ""))

    def _check(self, rc, h="self"):
        if rc != L.EKF_OK:
            raise self._error(rc, h)

    # ---- hot path ----
    def predict(self, u):
        self._check(self.lib.ekf_predict(self.h, _p(_vec(u, 2))))

    # ---- pre-marshalled inputs (hosts that stream many steps: bench.py) ----
    # The plain methods convert their arguments on every call (numpy + ctypes: ~10 us per predict + correct in CPython, more
    # than a shard of an 8-GPU run spends on the GPU per update-step).  `marshal_steps` lays a whole run out once in three
    # contiguous arrays; `step_raw(i)` then issues predict + correct of step i with integer addresses only.
    def marshal_steps(self, steps):
        """steps: iterable of (u[2], z[2], R[2x2], idx0).  Returns an opaque run object for step_raw / prefetch use."""
        steps = list(steps)
        m = len(steps)
        U = np.empty((m, 2)); Z = np.empty((m, 2)); Rm = np.empty((m, 4)); K = np.empty(m, dtype=np.int64)
        for i, (u, z, R, k) in enumerate(steps):
            U[i] = np.asarray(u, dtype=np.float64).reshape(-1)[:2]
            Z[i] = np.asarray(z, dtype=np.float64).reshape(-1)[:2]
            Rm[i] = np.asarray(R, dtype=np.float64).reshape(2, 2).reshape(-1, order="F")       # column-major, as the ABI takes it
            K[i] = int(k)
        if self._raw is None:
            proto_p = ctypes.CFUNCTYPE(ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p)
            proto_c = ctypes.CFUNCTYPE(ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64)
            proto_h = ctypes.CFUNCTYPE(ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64)
            self._raw = (proto_p(("ekf_predict", self.lib)), proto_c(("ekf_correct", self.lib)),
                         proto_c(("ekf_correct_begin", self.lib)), proto_h(("ekf_hint_next", self.lib)))
        return {"U": U, "Z": Z, "R": Rm, "K": K, "k": K.tolist(), "u": U.ctypes.data, "z": Z.ctypes.data, "r": Rm.ctypes.data, "m": m}

    def step_raw(self, run, i):
        """predict(u_i) + correct(z_i, R_i, idx_i) of a marshalled run."""
        f_pred, f_corr, f_begin, f_hint = self._raw
        rc = f_pred(self.h, run["u"] + 16 * i)
        if rc:
            self._check(rc)
        if self._hints and i + 1 < run["m"]:     # sharded, library-owned communicator, batch 1: announce the next landmark
            f_hint(self.h, run["k"][i + 1])
        if self._host_exchange is not None:
            rc = f_begin(self.h, run["z"] + 16 * i, run["r"] + 32 * i, run["k"][i])
            if rc:
                self._check(rc)
            self._host_exchange(self)
            self.correct_finish()
            return
        rc = f_corr(self.h, run["z"] + 16 * i, run["r"] + 32 * i, run["k"][i])
        if rc:
            self._check(rc)

    def append(self, u, R, pos, signature):
        self._check(self.lib.ekf_append(self.h, _p(_vec(u, 2)), _p(_colmajor(R).reshape(-1, order="F")),
                                        _p(_vec(pos, 2)), float(signature)))

    def correct(self, z, R, idx0):
        if self._host_exchange is not None:      # sharded, all-gather done by the host (torch.distributed)
            self.correct_begin(z, R, idx0)
            self._host_exchange(self)
            self.correct_finish()
            return
        self._check(self.lib.ekf_correct(self.h, _p(_vec(z[:2], 2)), _p(_colmajor(R).reshape(-1, order="F")), int(idx0)))

    # ---- sharded correction, split so that the caller can run the all-gather (include/ekfslam.h, multi-GPU) ----
    def correct_begin(self, z, R, idx0):
        self._check(self.lib.ekf_correct_begin(self.h, _p(_vec(z[:2], 2)), _p(_colmajor(R).reshape(-1, order="F")),
                                               int(idx0)))

    def correct_finish(self):
        self._check(self.lib.ekf_correct_finish(self.h))

    def prefetch_rows(self, idx0_list):
        """One exchange for the base row-panels of the landmarks the next corrections touch (sharded handles)."""
        if self._host_exchange is not None:
            self.prefetch_begin(idx0_list)
            self._host_exchange(self)
            self.prefetch_finish()
            return
        self._check(self.lib.ekf_prefetch_rows(self.h, *index_array(idx0_list)))

    def prefetch_next(self, idx0_list):
        """Announce the landmarks of the batch AFTER the current one (ekf_prefetch_next): extracted in front of the current batch's
        pass as that pass will leave them, exchanged beside it.  Library-owned communicator or exchange hook only."""
        if self._host_exchange is not None:
            raise L.EkfError(L.EKF_ERR_STATE, "prefetch_next: the host-run all-gather cannot run inside the library's flush")
        self._check(self.lib.ekf_prefetch_next(self.h, *index_array(idx0_list)))

    def prefetch_begin(self, idx0_list):
        self._check(self.lib.ekf_prefetch_begin(self.h, *index_array(idx0_list)))

    def prefetch_finish(self):
        self._check(self.lib.ekf_prefetch_finish(self.h))

    def exchange_info(self):
        send, recv = ctypes.c_void_p(), ctypes.c_void_p()
        cnt, cap = ctypes.c_int64(), ctypes.c_int64()
        self._check(self.lib.ekf_exchange_info(self.h, ctypes.byref(send), ctypes.byref(recv), ctypes.byref(cnt),
                                               ctypes.byref(cap)))
        return send.value, recv.value, int(cnt.value), int(cap.value)

    def exchange_set_buffers(self, send_ptr, recv_ptr):
        self._check(self.lib.ekf_exchange_set_buffers(self.h, ctypes.c_void_p(send_ptr), ctypes.c_void_p(recv_ptr)))

    def comm_init(self, comm_id_bytes):
        assert len(comm_id_bytes) == L.EKF_COMM_ID_BYTES
        self._check(self.lib.ekf_comm_init(self.h, bytes(comm_id_bytes)))
        self._hints = self.cfg.batch <= 1 and not self.cfg.async_flush      # step_raw announces the next landmark (ekf_hint_next)

    def hint_next(self, idx0):
        self._check(self.lib.ekf_hint_next(self.h, int(idx0)))

    def associate(self, z, R, want_costs=False):
        if self._host_exchange is not None and (want_costs or self.cfg.w_pos != 0.0):
            # sharded, all-gather done by the host: the position cost needs the other shards' diagonal blocks
            self.associate_begin(z, R, want_costs)
            self._host_exchange(self)
            return self.associate_finish(want_costs)
        return self._association(want_costs, lambda *out: self.lib.ekf_associate(
            self.h, _p(_vec(z, 3)), _p(_colmajor(R).reshape(-1, order="F")), *out))

    def _association(self, want_costs, call):
        """The answer of ekf_associate / ekf_associate_finish: call(is_new, idx, position costs, signature costs) fills the outputs made
        here -- the cost arrays only where asked for, null otherwise."""
        is_new, idx = ctypes.c_int32(), ctypes.c_int64()
        N = self.N
        pc = np.zeros(max(N, 1)) if want_costs else None
        sc = np.zeros(max(N, 1)) if want_costs else None
        self._check(call(ctypes.byref(is_new), ctypes.byref(idx), p_or_null(pc), p_or_null(sc)))
        if want_costs:
            return bool(is_new.value), int(idx.value), pc[:N], sc[:N]
        return bool(is_new.value), int(idx.value)

    # ---- sharded association with position costs, split around the caller's all-gather (include/ekfslam.h) ----
    def associate_begin(self, z, R, want_costs=False):
        self._check(self.lib.ekf_associate_begin(self.h, _p(_vec(z, 3)), _p(_colmajor(R).reshape(-1, order="F")),
                                                 1 if want_costs else 0))

    def associate_finish(self, want_costs=False):
        return self._association(want_costs, lambda *out: self.lib.ekf_associate_finish(self.h, *out))

    def measure(self, observed_LL, u, lm_index, lm_loc):
        obs = np.asfortranarray(np.asarray(observed_LL, dtype=np.float64).reshape(-1, 3))
        idx = _vec(lm_index)
        loc = np.asfortranarray(np.asarray(lm_loc, dtype=np.float64).reshape(-1, 2))
        self._check(self.lib.ekf_measure(self.h, _p(obs.reshape(-1, order="F")), obs.shape[0], _p(_vec(u, 2)),
                                         _p(idx), _p(loc.reshape(-1, order="F")), idx.size))

    def set_params(self, C=None, Rc=None, s_cost=None, s_thresh=None, w_pos=None):
        c = self.cfg
        if C is not None: c.C = float(C)
        if Rc is not None: c.Rc[0], c.Rc[1] = float(Rc[0]), float(Rc[1])
        if s_cost is not None: c.s_cost = float(s_cost)
        if s_thresh is not None: c.s_thresh = float(s_thresh)
        if w_pos is not None: c.w_pos = float(w_pos)
        rc2 = (ctypes.c_double * 2)(c.Rc[0], c.Rc[1])
        self._check(self.lib.ekf_set_params(self.h, c.C, rc2, c.s_cost, c.s_thresh, c.w_pos))

    def flush(self):
        self._check(self.lib.ekf_flush(self.h))

    def pending(self):
        n = ctypes.c_int32()
        self._check(self.lib.ekf_pending(self.h, ctypes.byref(n)))
        return int(n.value)

    def sync(self):
        self._check(self.lib.ekf_sync(self.h))

    def set_stream(self, stream_ptr):
        self._check(self.lib.ekf_set_stream(self.h, ctypes.c_void_p(stream_ptr)))

    # ---- state ----
    @property
    def N(self):
        n = ctypes.c_int64()
        self._check(self.lib.ekf_num_landmarks(self.h, ctypes.byref(n)))
        return int(n.value)

    @property
    def n(self):
        return 3 + 2 * self.N

    def get_x(self):
        x = np.empty(self.n)
        self._check(self.lib.ekf_get_x(self.h, _p(x)))
        return x

    def get_s(self):
        s = np.empty(max(self.N, 1))
        self._check(self.lib.ekf_get_s(self.h, _p(s)))
        return s[:self.N]

    def get_P(self):
        n = self.n
        buf = np.empty(n * n)
        self._check(self.lib.ekf_get_P(self.h, _p(buf)))
        return buf.reshape(n, n, order="F")

    def get_P_block(self, r0, c0, nr, nc):
        buf = np.empty(nr * nc)
        self._check(self.lib.ekf_get_P_block(self.h, r0, c0, nr, nc, _p(buf)))
        return buf.reshape(nr, nc, order="F")

    def get_P_diag_blocks(self):
        """(N+1) x 2 x 2: P(1:2,1:2) and every landmark's diagonal block -- what plot() reads, one call."""
        nb = self.N + 1
        buf = np.empty(4 * nb)
        self._check(self.lib.ekf_get_P_diag_blocks(self.h, _p(buf)))
        return buf.reshape(nb, 2, 2).transpose(0, 2, 1).copy()      # each block arrives column-major

    def get_Q3(self):
        q = np.empty(9)
        self._check(self.lib.ekf_get_Q(self.h, _p(q)))
        return q.reshape(3, 3, order="F")

    def set_x(self, x):
        """x fixes the landmark count: (x.size - 3) / 2."""
        x = _vec(x)
        self._check(self.lib.ekf_set_x(self.h, _p(x), x.size))

    def set_s(self, s):
        s = _vec(s)
        self._check(self.lib.ekf_set_s(self.h, _p(s) if s.size else None, s.size))

    def set_P(self, P):
        Pf = _colmajor(P)
        self._check(self.lib.ekf_set_P(self.h, _p(Pf.reshape(-1, order="F")), Pf.shape[0]))

    def set_state(self, x, P, s):
        self.set_x(x)
        self.set_s(s)
        self.set_P(P)

    def remove_landmarks(self, indices):
        """Drop the landmarks `indices` (0-based, any iterable of ints, any order) from the map on the device
        (ekf_remove_landmarks): the survivors keep their order and their bits."""
        self._check(self.lib.ekf_remove_landmarks(self.h, *index_array(indices)))

    @staticmethod
    def _delta_R(delta, R):
        """(delta, R) of a constraint between two landmarks as pointers; null where left out (delta: (0, 0), R: zero)."""
        return p_or_null(None if delta is None else _vec(delta, 2)), p_or_null(noise(R))

    def constrain_landmarks(self, i, j, delta=None, R=None):
        """'l_i - l_j was observed as delta with noise covariance R' (0-based i != j; delta None: (0, 0), R None: zero): the exact
        linear Kalman update between two landmarks, formed and applied on the device before the call returns
        (ekf_constrain_landmarks)."""
        self._check(self.lib.ekf_constrain_landmarks(self.h, int(i), int(j), *self._delta_R(delta, R)))

    def merge_landmarks(self, keep, drop, R=None):
        """Fuse landmark `drop` into `keep` (0-based): constrain_landmarks(keep, drop, None, R), then remove_landmarks([drop]);
        keep's index afterwards is keep - (drop < keep) (ekf_merge_landmarks)."""
        self._check(self.lib.ekf_merge_landmarks(self.h, int(keep), int(drop), p_or_null(noise(R))))

    def merge_landmarks_batch(self, pairs, R=None):
        """Fuse every (keep, drop) of `pairs` (0-based, at most EKF_MERGE_BATCH_MAX, numbering before the call) in one call: what
        constrain_landmarks(keep, drop, None, R) pair by pair in list order, then ONE remove_landmarks(all drops) would leave -- m
        chained gathers and one fused downdate-and-compact pass on the device.  A keep may be shared; no keep may be dropped.
        Returns d2[k], the distance landmark_distance(keep_k, drop_k, None, R) would report just before constraint k
        (ekf_merge_landmarks_batch)."""
        rows = [tuple(p) for p in pairs]
        if any(len(p) != 2 for p in rows):
            raise ValueError("merge_landmarks_batch: pairs are (keep, drop)")
        v = np.asarray(rows, dtype=np.float64).reshape(-1, 2)
        if not np.all(v == np.floor(v)):
            raise ValueError("merge_landmarks_batch: landmark indices are whole numbers")
        (keep, m), (drop, _) = index_array(v[:, 0]), index_array(v[:, 1])
        d2 = np.empty(max(m, 1))
        self._check(self.lib.ekf_merge_landmarks_batch(self.h, keep, drop, m, p_or_null(noise(R)), _p(d2)))
        return d2[:m]

    def landmark_distance(self, i, j, delta=None, R=None):
        """(d2, S): the squared Mahalanobis distance nu' S^-1 nu of 'l_i - l_j = delta' under the current state and its 2 x 2
        innovation covariance -- what a caller gates a merge on.  Changes nothing (ekf_landmark_distance)."""
        d2 = ctypes.c_double()
        S = np.empty(4)
        self._check(self.lib.ekf_landmark_distance(self.h, int(i), int(j), *self._delta_R(delta, R), ctypes.byref(d2), _p(S)))
        return float(d2.value), S.reshape(2, 2, order="F")

    def nearest_landmarks(self, R=None):
        """(d2, partner): for every landmark i (0-based) the j < i that minimises landmark_distance(i, j, None, R)[0] and that
        minimum, bit for bit; partner is int64 with -1 (and d2 = +inf) where no pair is admissible -- landmark 0, rows whose pairs
        are all irregular.  The lowest index wins ties.  One read-only pass over P on the device (ekf_nearest_landmarks)."""
        Rp = p_or_null(noise(R))
        N = self.N
        d2 = np.empty(max(N, 1))
        partner = np.empty(max(N, 1), dtype=np.int64)
        self._check(self.lib.ekf_nearest_landmarks(self.h, Rp, _p(d2),
                                                   partner.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        return d2[:N], partner[:N]

    def duplicate_candidates(self, gate, R=None):
        """The rows of nearest_landmarks(R) with d2 <= gate as a list of (i, j, d2), 0-based, j = partner[i] < i, sorted by
        (d2, i): what a caller would hand to merge_landmarks(keep=j, drop=i, R).  A host-side filter of the N results."""
        d2, partner = self.nearest_landmarks(R)
        rows = np.nonzero((partner >= 0) & (d2 <= float(gate)))[0]
        rows = rows[np.lexsort((rows, d2[rows]))]
        return [(int(i), int(partner[i]), float(d2[i])) for i in rows]

    # ---- update-steps from one struct (marshal.py builds it; slam.py hands in the one it logs from) ----
    _linear_obs = staticmethod(marshal.linear_obs)
    _model_obs = staticmethod(marshal.model_obs)
    _model_inits = staticmethod(marshal.model_inits)
    _motions = staticmethod(marshal.motions)

    def _observe(self, name, o, wait):
        """ekf_observe_linear / ekf_observe_model / their _innovation twins on the struct o: the result dict where waited for."""
        res = L.EkfLinearResult() if wait else None
        self._check(getattr(self.lib, name)(self.h, ctypes.byref(o), ctypes.byref(res) if wait else None))
        return marshal.linear_result(res) if wait else None

    def _observe_iterated(self, name, o, iterations, tol, wait):
        """ekf_observe_model_iterated / ekf_model_innovation_iterated on the struct o."""
        first, it = (L.EkfLinearResult(), L.EkfIteratedResult()) if wait else (None, None)
        self._check(getattr(self.lib, name)(self.h, ctypes.byref(o), int(iterations), float(tol), ctypes.byref(first) if wait else None,
                                            ctypes.byref(it) if wait else None))
        return marshal.iterated_result(first, it) if wait else None

    # ---- linear observations: update-steps with a constant Jacobian (include/ekfslam.h: ekf_observe_linear) ----
    def observe_linear(self, z, R, Hr=None, landmarks=(), Hl=(), gate=float("inf"), wrap=(0, 0), rows=2, wait=False):
        """'H x was observed as z with noise covariance R' as an UPDATE-STEP (ekf_observe_linear): H = the 2 x 3 block Hr on the robot
        state (theta in degrees) plus one 2 x 2 block Hl[b] on each of up to two landmarks (0-based).  Enters the pending ring like a
        correction: nothing is flushed, and with wait=False nothing is waited for (returns None).  wait=True returns
        {'nu', 'S', 'd2', 'outcome'} of the launch (outcome: EKF_LINEAR_APPLIED / _GATED; an irregular S raises EkfError)."""
        return self._observe("ekf_observe_linear", marshal.linear_obs(z, R, Hr, landmarks, Hl, gate, wrap, rows), wait)

    def linear_innovation(self, z, R, Hr=None, landmarks=(), Hl=(), gate=float("inf"), wrap=(0, 0), rows=2):
        """{'nu', 'S', 'd2', 'outcome'} observe_linear(..., wait=True) would report under the current state, bit for bit; changes
        nothing and flushes nothing (ekf_linear_innovation).  An irregular S is reported (outcome EKF_LINEAR_IRREGULAR, d2 NaN)."""
        return self._observe("ekf_linear_innovation", marshal.linear_obs(z, R, Hr, landmarks, Hl, gate, wrap, rows), True)

    def linear_rejections(self):
        """(irregular, gated): observe_linear launches since the last call that did not apply; synchronises and resets the counts."""
        a, b = ctypes.c_int64(), ctypes.c_int64()
        self._check(self.lib.ekf_linear_rejections(self.h, ctypes.byref(a), ctypes.byref(b)))
        return int(a.value), int(b.value)

    # ---- observations through a model linearised on the device (include/ekfslam.h: ekf_observe_model) ----
    def observe_model(self, model, z, R, landmarks=(), anchor=None, gate=float("inf"), wait=False):
        """'h(x) was observed as z with noise covariance R' for one of the models EKF_MODEL_* (range and bearing, range, bearing,
        relative position, landmark range), linearised on the device at the live x (ekf_observe_model).  landmarks: the 0-based
        target (two for EKF_MODEL_LANDMARK_RANGE); anchor: a fixed point outside the map as the target instead.  An update-step like
        observe_linear: nothing is flushed; wait=True returns {'nu', 'S', 'd2', 'outcome'} (a target on the robot raises EkfError)."""
        return self._observe("ekf_observe_model", marshal.model_obs(model, z, R, landmarks, anchor, gate), wait)

    def model_innovation(self, model, z, R, landmarks=(), anchor=None, gate=float("inf")):
        """{'nu', 'S', 'd2', 'outcome'} observe_model(..., wait=True) would report under the current state, bit for bit; changes and
        flushes nothing (ekf_model_innovation)."""
        return self._observe("ekf_model_innovation", marshal.model_obs(model, z, R, landmarks, anchor, gate), True)

    # ---- ... relinearised on the device: the iterated EKF update (include/ekfslam.h: ekf_observe_model_iterated) ----
    def observe_model_iterated(self, model, z, R, landmarks=(), anchor=None, gate=float("inf"), iterations=3, tol=0.0, wait=False):
        """observe_model with h relinearised up to `iterations` times (1..16) on the device, Gauss-Newton on the MAP cost over the
        robot and the target(s); stops early where no entry moves by more than tol (ekf_observe_model_iterated).  One launch and one
        pair in the ring, like observe_model; the gate is read at the first linearisation.  wait=True returns observe_model's dict (the
        FIRST linearisation's nu, S, d2; the call's outcome) with 'iterated': {'S', 'nu', 'used', 'converged', 'last_step', 'x_local'}
        of the linearisation that made the pair.  An iterate without a Jacobian or with an irregular S raises EkfError; nothing is
        changed then."""
        o = marshal.model_obs(model, z, R, landmarks, anchor, gate)
        return self._observe_iterated("ekf_observe_model_iterated", o, iterations, tol, wait)

    def model_innovation_iterated(self, model, z, R, landmarks=(), anchor=None, gate=float("inf"), iterations=3, tol=0.0):
        """What observe_model_iterated(..., wait=True) would report under the current state, bit for bit; changes and flushes nothing
        (ekf_model_innovation_iterated).  An irregular outcome is reported, not raised."""
        o = marshal.model_obs(model, z, R, landmarks, anchor, gate)
        return self._observe_iterated("ekf_model_innovation_iterated", o, iterations, tol, True)

    @staticmethod
    def model_iterate(model, sm, z, R, anchor=None, has_landmark=True, gate=float("inf"), iterations=3, tol=0.0, lib=None):
        """The loop the kernel runs, on the host (ekf_model_iterate): sm = the 38 operands of the small part (include/ekfslam.h names the
        layout), R the 2 x 2 the kernel sees (a one-row model: [[r, 0], [0, 1]]).  Returns model_innovation_iterated's dict."""
        first, it = L.EkfLinearResult(), L.EkfIteratedResult()
        av = _vec(anchor, 2) if anchor is not None else np.zeros(2)
        Rf = noise(np.asarray(R, dtype=np.float64))           # (as an array: R is not optional here)
        host_call("ekf_model_iterate", lib, int(model), _p(_vec(sm, 38)), _p(av), int(bool(has_landmark)), _p(_vec(z, 2)), _p(Rf),
                  float(gate), int(iterations), float(tol), ctypes.byref(first), ctypes.byref(it))
        return marshal.iterated_result(first, it)

    @staticmethod
    def model_evaluate(model, xr, t0, t1=None, lib=None):
        """(h(x), H) of a model at the robot state xr = (x, y, theta in degrees) and the targets t0 (and t1: the second landmark of
        EKF_MODEL_LANDMARK_RANGE): the function the kernel runs, on the host (ekf_model_evaluate).  H is 2 x 7 over
        x, y, theta | t0 | t1; an anchor's block is simply not used."""
        hx, H = np.zeros(2), np.zeros(14)
        host_call("ekf_model_evaluate", lib, int(model), _p(_vec(xr, 3)), _p(_vec(t0, 2)), p_or_null(None if t1 is None else _vec(t1, 2)),
                  _p(hx), _p(H))
        return hx, H.reshape(2, 7)

    # ---- landmarks that start from a model's inverse (include/ekfslam.h: ekf_append_model) ----
    def append_model(self, entries):
        """One scan of new landmarks: entries = [(model, z, R, signature), ...] with model EKF_MODEL_RANGE_BEARING (z = range, bearing in
        degrees) or EKF_MODEL_RELATIVE_XY (z = the landmark in the robot frame), all inverted on the device at the live robot state and
        appended by one launch (ekf_append_model).  Returns the 0-based index of the first one; entry b becomes landmark first + b.
        Nothing is waited for or flushed."""
        return self._append_model(*marshal.model_inits(entries))

    def _append_model(self, arr, m):
        first = ctypes.c_int64(-1)
        self._check(self.lib.ekf_append_model(self.h, arr, m, ctypes.byref(first)))
        return int(first.value)

    # ---- a local map joined into this one (include/ekfslam.h: ekf_join_map) ----
    def join_map(self, local_engine, signature_offset=0.0):
        """Join the map of `local_engine` -- a filter of its own, started at this one's robot pose and independent of it, any tile edge
        and storage kind, on the same device -- into this one on the device: the robot composes with the local robot, local landmark i
        becomes landmark first + i with signature s_local[i] + signature_offset, the local cross-covariances kept (P' = J blockdiag(P,
        PL) J').  A synchronising call on both engines: pending is 0 on both afterwards and the local one, otherwise untouched, may be
        closed at once.  Returns the 0-based index of the first new landmark (ekf_join_map)."""
        if not isinstance(local_engine, Engine):
            raise TypeError("join_map: the local map is an Engine")
        return self._join_map(local_engine, marshal.join_offset(signature_offset))

    def _join_map(self, local_engine, offset):
        first = ctypes.c_int64(-1)
        self._check(self.lib.ekf_join_map(self.h, local_engine.h, offset, ctypes.byref(first)))
        return int(first.value)

    # ---- part of this map taken out into another engine (include/ekfslam.h: ekf_extract_map) ----
    def extract_map(self, indices, frame="map", into=None, **engine_kw):
        """Take the robot and the landmarks `indices` (0-based, distinct, any order) out into another engine on the same device, whose
        whole state is replaced: destination landmark k is landmark indices[k].  frame="map": the marginal as it is, every value
        keeping its bits; frame="robot": the landmarks relative to the robot (RELATIVE_XY), the robot's own uncertainty folded in, the
        destination's robot at zero with P = 0 -- the shape join_map expects of a local map.  `into`: an existing Engine of any tile
        edge and storage kind with capacity >= len(indices); None: one is made with capacity max(m, 1) and this engine's mode, device
        and storage kind unless `engine_kw` says otherwise.  A synchronising call on both engines; this one is only flushed.  Returns
        the destination Engine (ekf_extract_map)."""
        return self._extract_map(marshal.extract_args(indices, frame), into, engine_kw)

    def _storage_name(self):
        if self.cfg.storage == L.EKF_STORE_F64:
            return "f64"
        return {L.EKF_ARITH_F32: "f32_mixed", L.EKF_ARITH_SPLIT3: "f32_split"}.get(self.cfg.pass_arith, "f32")

    def _extract_map(self, args, into=None, engine_kw=None):
        arr, m, frame = args
        engine_kw = dict(engine_kw or {})
        made = into is None
        if made:
            kw = dict(mode="known" if self.cfg.mode == L.EKF_MODE_KNOWN else "uc", capacity=max(m, 1), storage=self._storage_name(),
                      device=self.cfg.device)
            kw.update(engine_kw)
            into = Engine(**kw)
        elif engine_kw:
            raise TypeError("extract_map: engine keywords make a new destination; `into` is an existing one")
        elif not isinstance(into, Engine):
            raise TypeError("extract_map: the destination is an Engine")
        try:
            self._check(self.lib.ekf_extract_map(self.h, arr, m, frame, into.h))
        except Exception:
            if made:
                into.close()
            raise
        return into

    # ---- the whole map moved into another frame, in place (include/ekfslam.h: ekf_transform_map) ----
    def transform_map(self, frame="map", t=None, Sigma=None):
        """Move the whole state into another frame on the device, in place.  frame="map": by the rigid transform t = (tx, ty, phi in
        degrees) whose 3 x 3 covariance is Sigma (None: exact) -- the robot composes behind t (POSE_DELTA), every landmark follows
        (RELATIVE_XY's inverse), P' = T P T' + A Sigma A'.  frame="robot": the robot's own pose becomes the origin, bit for bit what
        extract_map(range(N), "robot") writes into another engine; t and Sigma stay None.  N and s stay.  A synchronising call: pending
        is 0 afterwards (ekf_transform_map)."""
        self._transform_map(marshal.transform_args(frame, t, Sigma))

    def _transform_map(self, args):
        frame, tv, Sv = args
        self._check(self.lib.ekf_transform_map(self.h, frame, marshal.p_or_null(tv), marshal.p_or_null(Sv)))

    # ---- the factorisation of P: definiteness, log det, NEES (include/ekfslam.h: ekf_factor_map) ----
    def factor_map(self, ref=None):
        """One Cholesky factorisation of P on the device -- of exactly what get_P() would report, the landmark block eliminated first
        (rows ascending), the robot last.  Returns a dict: n = 3 + 2 N, definite, bad_index (-1, or the index into x of the first pivot
        that failed in that order: 3 + r for landmark row r, 0 .. 2 for the robot), bad_pivot, logdet (NaN where not definite),
        logdet_map (the landmark block alone), min_pivot, max_pivot, and d2: for each of the 1 to 8 reference states in `ref` (one
        state, or one per row) nu' P^-1 nu with nu = x - ref, the heading entry wrapped into (-180, 180]; NaN where not definite.
        A P that is not definite is a result, not an error.  Read-only and synchronising: pending is 0 afterwards; nothing is kept
        between calls (ekf_factor_map)."""
        return self._factor_map(marshal.factor_args(ref, 3 + 2 * self.N))

    def _factor_map(self, args):
        ref, nref, info, d2 = args
        self._check(self.lib.ekf_factor_map(self.h, marshal.p_or_null(ref), nref, ctypes.byref(info), marshal.p_or_null(d2)))
        return marshal.factor_result(args)

    # ---- draws from the posterior: x + C xi from the same factorisation (include/ekfslam.h: ekf_sample_map) ----
    def sample_map(self, xi):
        """(samples, info): row q of `samples` is x + C xi_q for the k draws in `xi` (one draw of 3 + 2 N entries, or one per row; in
        x's order, standard normal where samples of N(x, P) are wanted -- the library generates no random numbers).  C is the Cholesky
        factor of P in factor_map's elimination order (the landmark block first, the robot last) mapped back to x's order: C C' = P.
        `info` is factor_map()'s dict without d2; where P is not definite every sample is NaN and info says where the factorisation
        stopped.  One factorisation per call whatever k is; read-only and synchronising (ekf_sample_map)."""
        return self._sample_map(marshal.sample_args(xi, 3 + 2 * self.N))

    def _sample_map(self, args):
        xi, k, out, info = args
        self._check(self.lib.ekf_sample_map(self.h, _p(xi), k, _p(out), ctypes.byref(info)))
        return marshal.sample_result(args)

    # ---- the other direction: C^-1 B and P^-1 B from the same factorisation (include/ekfslam.h: ekf_solve_map) ----
    def solve_map(self, B, form="full"):
        """(out, info): row q of `out` is P^-1 b_q (form="full") or C^-1 b_q (form="half") for the k right-hand sides in `B` (one of
        3 + 2 N entries, or one per row; in x's order).  C is the Cholesky factor of P in factor_map's elimination order (the landmark
        block first, the robot last); the half form is C^-1 b mapped back to x's order, so |out_q|^2 = b_q' P^-1 b_q and the half form
        of sample_map's samples minus x returns the draws.  No entry is wrapped.  `info` is factor_map()'s dict without d2; where P
        is not definite every entry is NaN.  One factorisation per call whatever k is; read-only and synchronising (ekf_solve_map)."""
        return self._solve_map(marshal.solve_args(B, form, 3 + 2 * self.N))

    def _solve_map(self, args):
        form, B, k, out, info = args
        self._check(self.lib.ekf_solve_map(self.h, form, _p(B), k, _p(out), ctypes.byref(info)))
        return marshal.solve_result(args)

    # ---- the plain product P B on the tile store, no factorisation (include/ekfslam.h: ekf_multiply_map) ----
    def multiply_map(self, B):
        """`out`: row q is P b_q for the k vectors in `B` (one of 3 + 2 N entries, or one per row; in x's order), P exactly what get_P()
        reports, all arithmetic F64.  No entry is wrapped.  One read-only pass over the tile store per 16 vectors, no factorisation:
        a row depends on its own vector alone, B = 0 gives 0, a unit vector returns a column of P.  Read-only and synchronising
        (ekf_multiply_map)."""
        return self._multiply_map(marshal.multiply_args(B, 3 + 2 * self.N))

    def _multiply_map(self, args):
        B, k, out = args
        self._check(self.lib.ekf_multiply_map(self.h, _p(B), k, _p(out)))
        return marshal.multiply_result(args)

    # ---- a linear observation with a dense H behind that product (include/ekfslam.h: ekf_observe_dense) ----
    def observe_dense(self, H, z, R, gate=float("inf"), wrap_deg=None):
        """"H x = z +- R" for k <= 16 rows that may touch every landmark: H a k x (3 + 2 N) array in x's order, or a list of
        {state index: coefficient} rows; z the k values; R k x k (or its k diagonal entries; 0 conditions exactly); rows flagged in
        wrap_deg have their innovation wrapped into (-180, 180].  Exact, no linearisation: S = H P H' + R, nu = z - H x, and with
        L L' = S, W = L^-1 H P, y = L^-1 nu: x' = x + W' y, P' = P - W' W -- applied only if d2 = |y|^2 <= gate.  The pending pairs are
        flushed first, ONE product pass and ONE update pass over P follow; nothing is waited for at the end.  Returns {'d2', 'rows',
        'outcome', 'bad_row', 'nu' (k), 'S' (k x k)}, outcome EKF_LINEAR_APPLIED or EKF_LINEAR_GATED; an S with a pivot that is not
        finite and positive raises EkfError and changes nothing (ekf_observe_dense)."""
        return self._observe_dense(marshal.dense_args(H, z, R, 3 + 2 * self.N, gate, wrap_deg))

    def _observe_dense(self, args):
        H, k, z, R, wrap, gate, res, nu, S = args
        self._check(self.lib.ekf_observe_dense(self.h, _p(H), k, _p(z), _p(R), wrap, gate, ctypes.byref(res), _p(nu), _p(S)))
        return marshal.dense_result(args)

    def dense_innovation(self, H, z, R, wrap_deg=None):
        """What observe_dense would report -- the same dict, bit for bit, with no gate read -- and nothing changed beyond the flush;
        an irregular S is reported (outcome EKF_LINEAR_IRREGULAR, 'bad_row'), not raised (ekf_observe_dense_innovation)."""
        args = marshal.dense_args(H, z, R, 3 + 2 * self.N, marshal.INF, wrap_deg, who="dense_innovation")
        H, k, z, R, wrap, _, res, nu, S = args
        self._check(self.lib.ekf_observe_dense_innovation(self.h, _p(H), k, _p(z), _p(R), wrap, ctypes.byref(res), _p(nu), _p(S)))
        return marshal.dense_result(args)

    @staticmethod
    def model_invert(model, xr, z, lib=None):
        """(t, Gx, Gz): the landmark that z observes from the robot state xr = (x, y, theta in degrees) through EKF_MODEL_RANGE_BEARING
        or EKF_MODEL_RELATIVE_XY, with Gx = dt/dx_r (2 x 3) and Gz = dt/dz (2 x 2): the function the kernel runs, on the host
        (ekf_model_invert)."""
        t, Gx, Gz = np.zeros(2), np.zeros(6), np.zeros(4)
        host_call("ekf_model_invert", lib, int(model), _p(_vec(xr, 3)), _p(_vec(z, 2)), _p(t), _p(Gx), _p(Gz))
        return t, Gx.reshape(2, 3), Gz.reshape(2, 2)

    # ---- which landmark a sighting belongs to, under the models' conventions (include/ekfslam.h: ekf_associate_model) ----
    def associate_model(self, entries, want_d2=False):
        """One scan matched to the whole map: entries = [{'model', 'z', 'R', 'gate'}, ...] (models 1-4, at most
        EKF_ASSOCIATE_MODEL_MAX; a gate left out is +inf).  Returns {'best', 'second', 'd2_best', 'd2_second', 'within_gate',
        'irregular'}, one array entry per observation, landmarks 0-based and -1 = none; d2 of every (observation, landmark) is what
        model_innovation reports for that pair, bit for bit.  want_d2 adds 'd2_all', the m x N matrix (NaN where a pair has no d2).
        Changes, flushes and retires nothing (ekf_associate_model)."""
        arr, m = marshal.scan_obs(entries)
        out = (L.EkfModelMatch * max(m, 1))()
        N = self.N
        d2 = np.full((m, N), np.nan) if want_d2 else None
        self._check(self.lib.ekf_associate_model(self.h, arr, m, out, _p(d2) if want_d2 and d2.size else None))
        res = {"best": np.array([out[k].best for k in range(m)], dtype=np.int64),
               "second": np.array([out[k].second for k in range(m)], dtype=np.int64),
               "d2_best": np.array([out[k].d2_best for k in range(m)]), "d2_second": np.array([out[k].d2_second for k in range(m)]),
               "within_gate": np.array([out[k].within_gate for k in range(m)], dtype=np.int64),
               "irregular": np.array([out[k].irregular for k in range(m)], dtype=np.int64)}
        if want_d2:
            res["d2_all"] = d2
        return res

    # ---- ... and assigned to the map one-to-one (include/ekfslam.h: ekf_assign_model) ----
    def assign_model(self, entries, want_candidates=False):
        """One scan assigned to the whole map, each landmark to at most one observation: entries as for associate_model, every gate
        finite -- it is the price of leaving the observation out.  Returns 'landmark' (0-based, -1 = left out), 'd2' (that pair's, +inf
        where left out), 'ncand' (candidates kept: landmarks inside the gate, at most EKF_ASSIGN_CANDIDATES), one array entry per
        observation; 'total', the minimised sum of the assigned d2 and the gates of the left-out; the six keys of associate_model, the same
        bits; and with want_candidates 'cand' / 'cand_d2', m x EKF_ASSIGN_CANDIDATES, each row the kept landmarks by (d2, index) with
        -1 / +inf behind them.  Changes, flushes and retires nothing (ekf_assign_model)."""
        arr, m = marshal.scan_obs(entries)
        out, match = (L.EkfModelAssigned * max(m, 1))(), (L.EkfModelMatch * max(m, 1))()
        total = ctypes.c_double(0.0)
        cand = np.full((m, L.EKF_ASSIGN_CANDIDATES), -1, dtype=np.int64) if want_candidates else None
        cand_d2 = np.full((m, L.EKF_ASSIGN_CANDIDATES), np.inf) if want_candidates else None
        self._check(self.lib.ekf_assign_model(self.h, arr, m, out, match,
                                              cand.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)) if want_candidates else None,
                                              _p(cand_d2) if want_candidates else None, ctypes.byref(total)))
        return marshal.assigned_result(out, match, m, total.value, cand, cand_d2)

    # ---- ... and assigned, then applied, with no wait between the two (include/ekfslam.h: ekf_observe_model_assigned) ----
    def observe_model_assigned(self, entries):
        """One scan assigned to the map and applied by the device alone: assign_model's launches, then one observe_model step per entry
        whose landmark the launch reads on the device -- a finite no-op for an entry that was left out.  entries as for assign_model (every
        gate finite: the price of leaving the entry out and the gate of its step).  Queues everything and returns; nothing is waited for
        or flushed, pending grows by the number of entries (ekf_observe_model_assigned).  assigned_scan_result() fetches what happened."""
        self._observe_model_assigned(*marshal.scan_obs(entries))

    def _observe_model_assigned(self, arr, m):
        self._check(self.lib.ekf_observe_model_assigned(self.h, arr, m))

    def assigned_scan_result(self):
        """The latest observe_model_assigned scan, waited for (its own event alone): {'landmark', 'd2', 'ncand', 'total'} as assign_model
        would have returned them at the state the scan saw (0-based, -1 = left out), and per step 'nu' (m x 2), 'S' (m x 2 x 2),
        'outcome' (EKF_LINEAR_APPLIED / _GATED / _IRREGULAR, EKF_LINEAR_UNASSIGNED for a left-out entry) and 'step_d2' (NaN where there
        is none).  Outcomes are data, nothing raises for them; before any scan EkfError (ekf_assigned_scan_result)."""
        m = ctypes.c_int64(0)
        out, res = (L.EkfModelAssigned * L.EKF_ASSIGN_MODEL_MAX)(), (L.EkfLinearResult * L.EKF_ASSIGN_MODEL_MAX)()
        total = ctypes.c_double(0.0)
        self._check(self.lib.ekf_assigned_scan_result(self.h, ctypes.byref(m), out, res, ctypes.byref(total)))
        return marshal.assigned_scan_result(out, res, int(m.value), total.value)

    # ---- a scan's pairings judged jointly (include/ekfslam.h: ekf_joint_innovation) ----
    def joint_innovation(self, entries, hypotheses, want_prefix=True, want_nu=False, want_S=False):
        """The joint compatibility of a scan's pairings: entries as for associate_model (the gate is not read), hypotheses an nh x m
        array, row i pairing observation k with the 0-based landmark hypotheses[i][k] or leaving it out (-1).  Returns {'d2', 'dof',
        'pairings', 'outcome', 'first_irregular'} with one entry per hypothesis -- d2 = nu' S^-1 nu over the stacked paired rows, NaN
        where a pairing is irregular -- plus 'd2_prefix' (nh x m: the joint d2 of the pairings among observations 0..k), 'nu'
        (nh x 2m) and 'S' (nh x 2m x 2m) by scan index where asked.  More than EKF_JOINT_HYP_MAX hypotheses go out as several calls.
        Changes and flushes nothing (ekf_joint_innovation)."""
        arr, m = marshal.scan_obs(entries)
        hyp_in = np.asarray(hypotheses)
        if hyp_in.ndim != 2 or hyp_in.shape[1] != m or hyp_in.shape[0] < 1:
            raise ValueError("joint_innovation: hypotheses is nh x m, one landmark (or -1) per entry of the scan")
        if not np.all(hyp_in == np.floor(hyp_in)):
            raise ValueError("joint_innovation: landmark indices are whole numbers")
        hyp = np.ascontiguousarray(hyp_in, dtype=np.int64)
        nh = hyp.shape[0]
        res = {"d2": np.empty(nh), "dof": np.empty(nh, dtype=np.int64), "pairings": np.empty(nh, dtype=np.int64),
               "outcome": np.empty(nh, dtype=np.int64), "first_irregular": np.empty(nh, dtype=np.int64)}
        prefix = np.full((nh, m), np.nan) if want_prefix else None
        nu = np.zeros((nh, 2 * m)) if want_nu else None
        S = np.zeros((nh, 2 * m, 2 * m)) if want_S else None
        for lo in range(0, nh, L.EKF_JOINT_HYP_MAX):
            hi = min(nh, lo + L.EKF_JOINT_HYP_MAX)
            out = (L.EkfJointResult * (hi - lo))()
            part = np.ascontiguousarray(hyp[lo:hi])
            self._check(self.lib.ekf_joint_innovation(self.h, arr, m, part.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), hi - lo, out,
                                                      _p(prefix[lo:hi]) if want_prefix else None, _p(nu[lo:hi]) if want_nu else None,
                                                      _p(S[lo:hi]) if want_S else None))
            for key in res:
                res[key][lo:hi] = [getattr(out[i], key) for i in range(hi - lo)]
        if want_prefix:
            res["d2_prefix"] = prefix
        if want_nu:
            res["nu"] = nu
        if want_S:
            res["S"] = S.transpose(0, 2, 1).copy()      # column-major blocks
        return res

    # ---- ... and searched on the device (include/ekfslam.h: ekf_joint_search) ----
    def joint_search(self, entries, thresholds, beam=64, want_candidates=False, want_alive=False):
        """The joint-compatibility search over one scan, on the device with one readback: entries as for assign_model (every gate
        finite: it decides what a candidate is), thresholds[dof] for dof 0 .. 2m, beam in 1 .. EKF_JOINT_SEARCH_BEAM_MAX.  Level k
        extends every alive hypothesis by the first EKF_JOINT_SEARCH_CAND candidates of entry k and by "left out"; an extension
        survives where its joint d2 <= thresholds[dof]; survivors are ordered by (pairings descending, d2 ascending, hypothesis
        ascending) and cut at beam.  Returns the winner's 'landmark' (0-based, -1 = left out), 'd2', 'dof', 'pairings', 'truncated',
        'nalive', 'irregular' (extensions without a d2), 'tested' / 'survived' per scan index, the keys of associate_model (its per-entry
        'irregular' as 'match_irregular'), with want_candidates 'cand' /
        'cand_d2' as assign_model returns them and with want_alive 'alive' (nalive x m) / 'alive_d2', the final beam in order.  Every d2 is
        joint_innovation's d2_prefix for that hypothesis bit for bit.  Changes and flushes nothing (ekf_joint_search)."""
        arr, m = marshal.scan_obs(entries)
        thr = marshal.joint_search_thresholds(thresholds, m)
        if int(beam) != beam:
            raise ValueError("joint_search: beam is a whole number")
        res, match = L.EkfJointSearchResult(), (L.EkfModelMatch * max(m, 1))()
        cand = np.full((m, L.EKF_ASSIGN_CANDIDATES), -1, dtype=np.int64) if want_candidates else None
        cand_d2 = np.full((m, L.EKF_ASSIGN_CANDIDATES), np.inf) if want_candidates else None
        alive = np.full((L.EKF_JOINT_SEARCH_BEAM_MAX, max(m, 1)), -1, dtype=np.int64) if want_alive else None
        alive_d2 = np.full(L.EKF_JOINT_SEARCH_BEAM_MAX, np.nan) if want_alive else None
        i64p = ctypes.POINTER(ctypes.c_int64)
        self._check(self.lib.ekf_joint_search(self.h, arr, m, _p(thr), int(beam), ctypes.byref(res), match,
                                              cand.ctypes.data_as(i64p) if want_candidates else None, _p(cand_d2) if want_candidates else None,
                                              alive.ctypes.data_as(i64p) if want_alive else None, _p(alive_d2) if want_alive else None))
        return marshal.joint_search_result(res, match, m, cand, cand_d2, alive, alive_d2)

    # ---- ... and applied as ONE joint update (include/ekfslam.h: ekf_observe_model_joint) ----
    def observe_model_joint(self, entries, landmarks, gate=float("inf"), want_nu=False, want_S=False, iterations=1, tol=0.0):
        """One hypothesis of joint_innovation APPLIED as one joint update: entries as for associate_model (the per-entry gate is not
        read), landmarks the 0-based landmark each observation is paired with or -1 = left out.  All pairings are linearised once at the
        live state and stacked; x' = x + W' y, P' = P - W' W with W = L^-1 H P, L L' = S -- applied only if the joint d2 <= gate.  The
        pending pairs are flushed first and ONE pass over P applies all pairings; nothing is waited for at the end.  Returns {'d2',
        'dof', 'pairings', 'outcome', 'first_irregular'} -- joint_innovation's for that hypothesis on the flushed state, bit for bit;
        outcome EKF_LINEAR_APPLIED or EKF_LINEAR_GATED -- plus 'nu' (2m) and 'S' (2m x 2m) by scan index where asked.  A pairing with
        no d2 raises EkfError and changes nothing (ekf_observe_model_joint).
        iterations > 1 RELINEARISES the whole scan up to that many times on the device (Gauss-Newton over the robot and the paired
        landmarks, stopping where no entry moves by more than tol) and applies the last linearisation; the gate and the dict above are the
        first one's, and 'used', 'converged', 'step' are added.  An iterate that is irregular raises EkfError and changes nothing
        (ekf_observe_model_joint_iterated)."""
        arr, m = marshal.scan_obs(entries)
        return self._observe_joint(arr, m, landmarks, gate, want_nu, want_S, iterations, tol)

    def _observe_joint(self, arr, m, landmarks, gate=float("inf"), want_nu=False, want_S=False, iterations=1, tol=0.0):
        """ekf_observe_model_joint on the built scan (arr, m); iterations > 1: ekf_observe_model_joint_iterated."""
        lms = np.asarray(landmarks, dtype=np.float64).reshape(-1)
        if lms.size != m:
            raise ValueError("observe_model_joint: one landmark (or -1) per entry of the scan")
        if not np.all(lms == np.floor(lms)):
            raise ValueError("observe_model_joint: landmark indices are whole numbers")
        if int(iterations) != iterations:
            raise ValueError("observe_model_joint: iterations is a whole number")
        idx, _ = marshal.index_array(lms.tolist())
        res = L.EkfJointResult()
        nu = np.zeros(2 * m) if want_nu else None
        S = np.zeros(4 * m * m) if want_S else None
        if int(iterations) == 1:
            self._check(self.lib.ekf_observe_model_joint(self.h, arr, m, idx, float(gate), ctypes.byref(res), p_or_null(nu), p_or_null(S)))
            return marshal.joint_result(res, m, nu, S)
        it = L.EkfJointIterResult()
        self._check(self.lib.ekf_observe_model_joint_iterated(self.h, arr, m, idx, float(gate), int(iterations), float(tol), ctypes.byref(res),
                                                              ctypes.byref(it), p_or_null(nu), p_or_null(S)))
        out = marshal.joint_result(res, m, nu, S)
        more = marshal.joint_iter_result(it)
        out.update(used=more["used"], converged=more["converged"], step=more["step"])
        return out

    @staticmethod
    def joint_iterate(x_sub, P_sub, entries, iterations=3, tol=0.0, lib=None):
        """The loop the kernel runs, on the host (ekf_joint_iterate): x_sub = (x_r, l_0 .. l_{np-1}), P_sub its ns x ns covariance, entries
        as for associate_model, every one paired with its own landmark of the sub-state.  Returns (x', P', record) with the record
        {'used', 'converged', 'step', 'd2_last', 'irregular_at', 'irregular_obs', 'x_sub'}; an irregular linearisation leaves x' and P' equal
        to the inputs."""
        arr, m = marshal.scan_obs(entries)
        xs = np.ascontiguousarray(x_sub, dtype=np.float64).reshape(-1)
        ns = 3 + 2 * m
        Ps = np.asfortranarray(np.asarray(P_sub, dtype=np.float64))
        if xs.size != ns or Ps.shape != (ns, ns):
            raise ValueError("joint_iterate: x_sub has 3 + 2 np entries and P_sub is square of that size")
        Pf = np.ascontiguousarray(Ps.T)                            # (column-major in memory)
        xo, Po = np.zeros(ns), np.zeros((ns, ns))
        it = L.EkfJointIterResult()
        host_call("ekf_joint_iterate", lib, _p(xs), _p(Pf), arr, m, int(iterations), float(tol), ctypes.byref(it), _p(xo), _p(Po))
        return xo, Po.T.copy(), marshal.joint_iter_result(it)

    # ---- motion steps through a model with its true Jacobians (include/ekfslam.h: ekf_predict_model) ----
    def predict_model(self, steps):
        """A chain of motion steps: steps = [(model, u, M), ...] with model EKF_MOTION_TURN_DRIVE (u = d, turn), EKF_MOTION_ARC (u = arc
        length, turn) or EKF_MOTION_POSE_DELTA (u = dx, dy, turn in the robot frame); angles in degrees, M the covariance of u (2 x 2 or
        3 x 3).  x_r' = f(x_r, u), P' = F P F' + V M V' with the true Jacobians, step after step in ONE launch (ekf_predict_model).
        Eager: a recorded predict is carried out first.  Nothing is waited for or flushed."""
        self._predict_model(*marshal.motions(steps))

    def _predict_model(self, arr, m):
        self._check(self.lib.ekf_predict_model(self.h, arr, m))

    @staticmethod
    def motion_evaluate(model, xr, u, lib=None):
        """(x_new, F, V) of a motion model at the robot state xr = (x, y, theta in degrees): the new pose, F = df/dx_r (3 x 3) and
        V = df/du (3 x 3; a model with two inputs leaves the last column zero): the function the kernel runs, on the host
        (ekf_motion_evaluate)."""
        uin = np.zeros(3)
        uv = _vec(u)
        uin[:min(uv.size, 3)] = uv[:3]
        xn, F, V = np.zeros(3), np.zeros(9), np.zeros(9)
        host_call("ekf_motion_evaluate", lib, int(model), _p(_vec(xr, 3)), _p(uin), _p(xn), _p(F), _p(V))
        return xn, F.reshape(3, 3, order="F"), V.reshape(3, 3, order="F")

    def load_lowrank_state(self, x, s, d, U):
        x, s, d = _vec(x), _vec(s), _vec(d)
        U = np.asfortranarray(np.asarray(U, dtype=np.float64))
        N = (x.size - 3) // 2
        self._check(self.lib.ekf_load_lowrank_state(self.h, N, _p(x), _p(s) if s.size else _p(np.zeros(1)), _p(d),
                                                    _p(U.reshape(-1, order="F")), U.shape[1]))

    def checkpoint_save(self, path):
        self._check(self.lib.ekf_checkpoint_save(self.h, str(path).encode()))

    def checkpoint_load(self, path):
        self._check(self.lib.ekf_checkpoint_load(self.h, str(path).encode()))

    def digest(self):
        out = np.empty(3)
        self._check(self.lib.ekf_P_digest(self.h, _p(out)))
        return out

    def device_bytes(self):
        b = ctypes.c_int64()
        self._check(self.lib.ekf_device_bytes(self.h, ctypes.byref(b)))
        return int(b.value)

    # ---- measurement hooks ----
    def timing_enable(self, which, on=True, launches=0):
        """launches: event pairs to reserve up front (launches expected between two timing_read calls)."""
        self._check(self.lib.ekf_kernel_timing_enable(self.h, which, max(1, int(launches)) if on else 0))

    def downdate_kernel_name(self):
        """(name, pairs) of the kernel instance the last downdate / flush launch used, as the launcher chose it."""
        pairs = ctypes.c_int32()
        name = self.lib.ekf_downdate_kernel_name(self.h, ctypes.byref(pairs))
        return (name or b"").decode(), int(pairs.value)

    def timing_read(self, which):
        n, ms = ctypes.c_int64(), ctypes.c_double()
        self._check(self.lib.ekf_kernel_timing_read(self.h, which, ctypes.byref(n), ctypes.byref(ms)))
        return int(n.value), float(ms.value)

    def downdate_algorithmic_bytes(self):
        b = ctypes.c_int64()
        self._check(self.lib.ekf_downdate_algorithmic_bytes(self.h, ctypes.byref(b)))
        return int(b.value)
