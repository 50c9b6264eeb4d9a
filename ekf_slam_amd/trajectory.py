"""On-disk trajectory log: everything the EKF hot path consumed, step by step.

The reference has no recorded data of any kind (its inputs are live ROS topics).  A log holds, per SLAM iteration,
the odometry `u` handed to predict() (SLAM.m:105-110) and what measure() saw after the landmark front-end ran
(EKF_SLAM.m:102,111,120): `observed_LL` (m x 3) and the landmark table (index, loc).  Replaying a log into an
engine reproduces the run bit for bit on the same hardware, and is how a run on one machine is compared with
another (or with the CPU oracle).  Format: one .npz with ragged arrays (`*_ptr` are CSR-style offsets).

A map that can be edited (remove_landmarks / constrain_landmarks / merge_landmarks of ekf_slam_amd/slam.py) needs its edits in the
log too, or a replay no longer reproduces the run: `record_edit` notes one, with the 1-based landmark numbers that layer consumed,
at the position `len(log)` it was made at -- it is replayed after step len(log) - 1 and before step len(log).  A log without edits
is written exactly as before (format 1, the same arrays); one with edits as format 2, with the edit arrays added; one that holds a
'merge_batch' edit (merge_landmarks_batch: idx = [keep1, drop1, keep2, drop2, ...], R shared) as format 3, which has the arrays of
format 2 -- a reader of format 2 alone would not know the fourth kind; one that holds an 'observe' edit (observe_linear: a linear
observation made between two steps -- idx = the 0, 1 or 2 landmarks that carry a block, the delta slot = z, R, and per observation Hr,
the landmark blocks Hl, gate, wrap and rows in arrays of their own) as format 4; one that holds an 'observe_model' edit (observe_model:
idx = the 0, 1 or 2 landmarks, the delta slot = z, R, and per observation the model, the anchor (NaN where the target is a landmark) and
the gate in arrays of their own) as format 5, which has the arrays of format 4 (empty where no linear observation was made); one that
holds an 'append_model' edit (add_landmarks_model: one scan of new landmarks, idx empty, and per scan its entries -- model, z, R, signature
-- in arrays of their own behind CSR offsets) as format 6, which has the arrays of format 5 (empty where there is nothing to hold); one
that holds a 'predict_model' edit (predict_model: one chain of motion steps, idx empty, and per chain its steps -- model, u, M -- in arrays
of their own behind CSR offsets) as format 7, which has the arrays of format 6 (empty where there is nothing to hold); one that holds an
'observe_model_iterated' edit (observe_model_iterated: an 'observe_model' edit's slots, and per observation the model, the anchor, the
gate, iterations and tol in arrays of their own) as format 8, which has the arrays of format 7 (empty where there is nothing to hold).
"""
import numpy as np

FORMAT = "ekfslam-trajectory-1"
FORMAT_EDITS = "ekfslam-trajectory-2"
FORMAT_BATCH = "ekfslam-trajectory-3"
FORMAT_OBSERVE = "ekfslam-trajectory-4"
FORMAT_MODEL = "ekfslam-trajectory-5"
FORMAT_APPEND = "ekfslam-trajectory-6"
FORMAT_PREDICT = "ekfslam-trajectory-7"
FORMAT_ITERATED = "ekfslam-trajectory-8"
EDIT_KINDS = ("remove", "constrain", "merge", "merge_batch")        # what record_edit takes
OBSERVE = "observe"                                                  # the fifth kind: record_observation's, number 4 in a file
OBSERVE_MODEL = "observe_model"                                      # the sixth kind: record_model_observation's, number 5 in a file
APPEND_MODEL = "append_model"                                        # the seventh kind: record_model_append's, number 6 in a file
PREDICT_MODEL = "predict_model"                                      # the eighth kind: record_model_predict's, number 7 in a file
OBSERVE_MODEL_ITERATED = "observe_model_iterated"                    # the ninth kind: record_model_observation_iterated's, number 8 in a file
_KINDS = EDIT_KINDS + (OBSERVE, OBSERVE_MODEL, APPEND_MODEL, PREDICT_MODEL, OBSERVE_MODEL_ITERATED)
_FORMATS = (FORMAT, FORMAT_EDITS, FORMAT_BATCH, FORMAT_OBSERVE, FORMAT_MODEL, FORMAT_APPEND, FORMAT_PREDICT, FORMAT_ITERATED)
_STEP_ARRAYS = ("u", "obs_ptr", "obs", "lm_ptr", "lm_index", "lm_loc")
_EDIT_ARRAYS = ("edit_step", "edit_kind", "edit_ptr", "edit_idx", "edit_delta", "edit_R")
_MODEL_ARRAYS = ("model_edit", "model_id", "model_anchor", "model_gate")
_APPEND_ARRAYS = ("append_edit", "append_ptr", "append_model", "append_z", "append_R", "append_signature")
_PREDICT_ARRAYS = ("predict_edit", "predict_ptr", "predict_model", "predict_u", "predict_M")
_ITERATED_ARRAYS = ("iter_edit", "iter_model", "iter_anchor", "iter_gate", "iter_iterations", "iter_tol")
_OBSERVE_ARRAYS = ("observe_edit", "observe_Hr", "observe_Hl", "observe_gate", "observe_wrap", "observe_rows")


class TrajectoryLog:
    def __init__(self):
        self.u, self.obs, self.lm_index, self.lm_loc = [], [], [], []
        self.edits = []             # (step, kind, idx (1-based numbers), delta[2], R[2x2]) in the order they were made
        self.model_observations = {}  # position in self.edits of an 'observe_model' edit -> {model, anchor (2) or None, gate}
        self.model_appends = {}     # position in self.edits of an 'append_model' edit -> [(model, z (2), R (2x2), signature), ...]
        self.model_predicts = {}    # position in self.edits of a 'predict_model' edit -> [(model, u (2 or 3), M (2x2 or 3x3)), ...]
        self.model_iterations = {}  # position in self.edits of an 'observe_model_iterated' edit -> {model, anchor or None, gate, iterations, tol}
        self.observations = {}      # position in self.edits of an 'observe' edit -> {Hr (2x3), Hl (2x2x2), gate, wrap (2), rows}

    def __len__(self):
        return len(self.u)

    def record(self, u, observed_LL, lm_index, lm_loc):
        self.u.append(np.asarray(u, dtype=np.float64).reshape(2).copy())
        obs = np.zeros((0, 3)) if observed_LL is None or len(observed_LL) == 0 else np.asarray(observed_LL, dtype=np.float64)
        self.obs.append(obs.reshape(-1, 3).copy())
        self.lm_index.append(np.asarray(lm_index, dtype=np.float64).reshape(-1).copy())
        self.lm_loc.append(np.asarray(lm_loc, dtype=np.float64).reshape(-1, 2).copy())

    def record_edit(self, kind, idx, delta=None, R=None):
        """A map edit made now, i.e. after the len(self) steps recorded so far.  kind: 'remove' (idx: the landmarks), 'constrain'
        (idx: [i, j]), 'merge' (idx: [keep, drop]) or 'merge_batch' (idx: [keep1, drop1, keep2, drop2, ...], non-empty; R shared by
        all pairs); landmark numbers 1-based; delta None: (0, 0), R None: the zero matrix."""
        if kind not in EDIT_KINDS:
            raise ValueError("record_edit: kind is one of %s" % (EDIT_KINDS,))
        idx = np.asarray(idx, dtype=np.float64).reshape(-1)
        if not np.all(idx == np.floor(idx)):
            raise ValueError("record_edit: landmark indices are whole numbers")
        if kind == "merge_batch":
            if idx.size == 0 or idx.size % 2:
                raise ValueError("record_edit: 'merge_batch' names (keep, drop) pairs, at least one")
        elif kind != "remove" and idx.size != 2:
            raise ValueError("record_edit: '%s' names two landmarks" % kind)
        d = np.zeros(2) if delta is None else np.asarray(delta, dtype=np.float64).reshape(2).copy()
        Rm = np.zeros((2, 2)) if R is None else np.asarray(R, dtype=np.float64).reshape(2, 2).copy()
        self.edits.append((len(self), kind, idx.astype(np.int64), d, Rm))

    def record_observation(self, z, R, Hr=None, landmarks=(), Hl=(), gate=float("inf"), wrap=(0, 0), rows=2):
        """A linear observation (observe_linear of ekf_slam_amd/slam.py) made now, i.e. after the len(self) steps recorded so far:
        z, R (2 x 2), the robot block Hr (2 x 3, None: zeros), the 1-based landmarks that carry a block and their 2 x 2 blocks Hl,
        gate, wrap and rows -- full-size arrays, as the wrapper hands them to the engine."""
        lms = np.asarray(list(landmarks), dtype=np.float64).reshape(-1)
        if not np.all(lms == np.floor(lms)):
            raise ValueError("record_observation: landmark indices are whole numbers")
        blocks = [np.asarray(b, dtype=np.float64).reshape(2, 2) for b in Hl]
        if lms.size > 2 or len(blocks) != lms.size:
            raise ValueError("record_observation: at most two landmarks, one 2 x 2 block each")
        if int(rows) not in (1, 2):
            raise ValueError("record_observation: rows is 1 or 2")
        Hlm = np.zeros((2, 2, 2))
        for b, blk in enumerate(blocks):
            Hlm[b] = blk
        zv = np.zeros(2)
        zin = np.asarray(z, dtype=np.float64).reshape(-1)
        zv[:zin.size] = zin
        w = tuple(wrap) + (0, 0)
        self.observations[len(self.edits)] = dict(
            Hr=np.zeros((2, 3)) if Hr is None else np.asarray(Hr, dtype=np.float64).reshape(2, 3).copy(), Hl=Hlm, gate=float(gate),
            wrap=np.array([int(bool(w[0])), int(bool(w[1]))], dtype=np.int64), rows=int(rows))
        self.edits.append((len(self), OBSERVE, lms.astype(np.int64), zv,
                           np.zeros((2, 2)) if R is None else np.asarray(R, dtype=np.float64).reshape(2, 2).copy()))

    def record_model_observation(self, model, z, R, landmarks=(), anchor=None, gate=float("inf")):
        """An observation through a model (observe_model of ekf_slam_amd/slam.py) made now, i.e. after the len(self) steps recorded so
        far: the model's number, z, R (2 x 2), the 1-based landmarks, the anchor (None: the target is a landmark) and the gate."""
        lms = np.asarray(list(landmarks), dtype=np.float64).reshape(-1)
        if not np.all(lms == np.floor(lms)):
            raise ValueError("record_model_observation: landmark indices are whole numbers")
        if lms.size > 2:
            raise ValueError("record_model_observation: at most two landmarks")
        zv = np.zeros(2)
        zin = np.asarray(z, dtype=np.float64).reshape(-1)
        zv[:zin.size] = zin
        self.model_observations[len(self.edits)] = dict(
            model=int(model), anchor=None if anchor is None else np.asarray(anchor, dtype=np.float64).reshape(2).copy(), gate=float(gate))
        self.edits.append((len(self), OBSERVE_MODEL, lms.astype(np.int64), zv,
                           np.zeros((2, 2)) if R is None else np.asarray(R, dtype=np.float64).reshape(2, 2).copy()))

    def record_model_observation_iterated(self, model, z, R, landmarks=(), anchor=None, gate=float("inf"), iterations=1, tol=0.0):
        """A relinearised observation through a model (observe_model_iterated of ekf_slam_amd/slam.py) made now, i.e. after the len(self)
        steps recorded so far: record_model_observation's arguments, then the number of linearisations and the stopping tolerance."""
        lms = np.asarray(list(landmarks), dtype=np.float64).reshape(-1)
        if not np.all(lms == np.floor(lms)):
            raise ValueError("record_model_observation_iterated: landmark indices are whole numbers")
        if lms.size > 2:
            raise ValueError("record_model_observation_iterated: at most two landmarks")
        zv = np.zeros(2)
        zin = np.asarray(z, dtype=np.float64).reshape(-1)
        zv[:zin.size] = zin
        self.model_iterations[len(self.edits)] = dict(
            model=int(model), anchor=None if anchor is None else np.asarray(anchor, dtype=np.float64).reshape(2).copy(), gate=float(gate),
            iterations=int(iterations), tol=float(tol))
        self.edits.append((len(self), OBSERVE_MODEL_ITERATED, lms.astype(np.int64), zv,
                           np.zeros((2, 2)) if R is None else np.asarray(R, dtype=np.float64).reshape(2, 2).copy()))

    def record_model_append(self, entries):
        """One scan of new landmarks (add_landmarks_model of ekf_slam_amd/slam.py) made now, i.e. after the len(self) steps recorded so
        far: entries = [(model, z, R, signature), ...], at least one, as the wrapper hands them to the engine."""
        ents = [(int(m), np.asarray(z, dtype=np.float64).reshape(2).copy(), np.asarray(R, dtype=np.float64).reshape(2, 2).copy(), float(s))
                for m, z, R, s in entries]
        if not ents:
            raise ValueError("record_model_append: at least one entry")
        self.model_appends[len(self.edits)] = ents
        self.edits.append((len(self), APPEND_MODEL, np.zeros(0, dtype=np.int64), np.zeros(2), np.zeros((2, 2))))

    def record_model_predict(self, steps):
        """One chain of motion steps (predict_model of ekf_slam_amd/slam.py) made now, i.e. after the len(self) steps recorded so far:
        steps = [(model, u, M), ...], at least one, u and M of the size the model reads (2 and 2 x 2, or 3 and 3 x 3)."""
        sts = []
        for model, u, M in steps:
            uv, Mm = np.asarray(u, dtype=np.float64).reshape(-1).copy(), np.asarray(M, dtype=np.float64)
            if uv.size not in (2, 3) or Mm.size != uv.size * uv.size:
                raise ValueError("record_model_predict: u has 2 or 3 values and M is square of that size")
            sts.append((int(model), uv, Mm.reshape(uv.size, uv.size).copy()))
        if not sts:
            raise ValueError("record_model_predict: at least one step")
        self.model_predicts[len(self.edits)] = sts
        self.edits.append((len(self), PREDICT_MODEL, np.zeros(0, dtype=np.int64), np.zeros(2), np.zeros((2, 2))))

    def save(self, path):
        def ragged(parts, width):
            ptr = np.cumsum([0] + [len(p) for p in parts])
            data = np.concatenate(parts) if parts and ptr[-1] else np.zeros((0, width) if width else (0,))
            return ptr, data
        obs_ptr, obs = ragged(self.obs, 3)
        lm_ptr, lmi = ragged(self.lm_index, 0)
        _, lml = ragged(self.lm_loc, 2)
        arrays = dict(u=np.array(self.u).reshape(-1, 2), obs_ptr=obs_ptr, obs=obs, lm_ptr=lm_ptr, lm_index=lmi, lm_loc=lml)
        if not self.edits:
            np.savez_compressed(path, format=np.array(FORMAT), **arrays)
            return
        e_ptr, e_idx = ragged([e[2] for e in self.edits], 0)
        fmt = FORMAT_BATCH if any(e[1] == "merge_batch" for e in self.edits) else FORMAT_EDITS
        if self.observations or self.model_observations or self.model_appends or self.model_predicts or self.model_iterations:
            fmt = FORMAT_OBSERVE
            at = sorted(self.observations)
            ob = [self.observations[q] for q in at]
            arrays.update(observe_edit=np.array(at, dtype=np.int64), observe_Hr=np.array([o["Hr"] for o in ob]).reshape(-1, 2, 3),
                          observe_Hl=np.array([o["Hl"] for o in ob]).reshape(-1, 2, 2, 2), observe_gate=np.array([o["gate"] for o in ob]),
                          observe_wrap=np.array([o["wrap"] for o in ob], dtype=np.int64).reshape(-1, 2),
                          observe_rows=np.array([o["rows"] for o in ob], dtype=np.int64))
        if self.model_observations or self.model_appends or self.model_predicts or self.model_iterations:
            fmt = FORMAT_MODEL
            at = sorted(self.model_observations)
            mo = [self.model_observations[q] for q in at]
            arrays.update(model_edit=np.array(at, dtype=np.int64), model_id=np.array([o["model"] for o in mo], dtype=np.int64),
                          model_anchor=np.array([np.full(2, np.nan) if o["anchor"] is None else o["anchor"] for o in mo]).reshape(-1, 2),
                          model_gate=np.array([o["gate"] for o in mo]))
        if self.model_appends or self.model_predicts or self.model_iterations:
            fmt = FORMAT_APPEND
            at = sorted(self.model_appends)
            ents = [e for q in at for e in self.model_appends[q]]
            arrays.update(append_edit=np.array(at, dtype=np.int64), append_ptr=np.cumsum([0] + [len(self.model_appends[q]) for q in at]),
                          append_model=np.array([e[0] for e in ents], dtype=np.int64), append_z=np.array([e[1] for e in ents]).reshape(-1, 2),
                          append_R=np.array([e[2] for e in ents]).reshape(-1, 2, 2), append_signature=np.array([e[3] for e in ents]))
        if self.model_predicts or self.model_iterations:
            fmt = FORMAT_PREDICT
            at = sorted(self.model_predicts)
            sts = [e for q in at for e in self.model_predicts[q]]
            U, Mf = np.zeros((len(sts), 3)), np.zeros((len(sts), 3, 3))          # a model with two inputs: the leading entries
            for k, (_, u, M) in enumerate(sts):
                U[k, :u.size] = u
                Mf[k, :u.size, :u.size] = M
            arrays.update(predict_edit=np.array(at, dtype=np.int64), predict_ptr=np.cumsum([0] + [len(self.model_predicts[q]) for q in at]),
                          predict_model=np.array([e[0] for e in sts], dtype=np.int64), predict_u=U, predict_M=Mf)
        if self.model_iterations:
            fmt = FORMAT_ITERATED
            at = sorted(self.model_iterations)
            mo = [self.model_iterations[q] for q in at]
            arrays.update(iter_edit=np.array(at, dtype=np.int64), iter_model=np.array([o["model"] for o in mo], dtype=np.int64),
                          iter_anchor=np.array([np.full(2, np.nan) if o["anchor"] is None else o["anchor"] for o in mo]).reshape(-1, 2),
                          iter_gate=np.array([o["gate"] for o in mo]), iter_iterations=np.array([o["iterations"] for o in mo], dtype=np.int64),
                          iter_tol=np.array([o["tol"] for o in mo]))
        np.savez_compressed(path, format=np.array(fmt), edit_step=np.array([e[0] for e in self.edits], dtype=np.int64),
                            edit_kind=np.array([_KINDS.index(e[1]) for e in self.edits], dtype=np.int64), edit_ptr=e_ptr,
                            edit_idx=e_idx.astype(np.int64), edit_delta=np.array([e[3] for e in self.edits]).reshape(-1, 2),
                            edit_R=np.array([e[4] for e in self.edits]).reshape(-1, 2, 2), **arrays)

    @staticmethod
    def load(path):
        g = np.load(path, allow_pickle=False)
        fmt = str(g["format"])
        if fmt not in _FORMATS:
            raise ValueError("not an %s file" % " / ".join(_FORMATS))
        ver = _FORMATS.index(fmt) + 1
        need = (_STEP_ARRAYS + (_EDIT_ARRAYS if ver >= 2 else ()) + (_OBSERVE_ARRAYS if ver >= 4 else ())
                + (_MODEL_ARRAYS if ver >= 5 else ()) + (_APPEND_ARRAYS if ver >= 6 else ()) + (_PREDICT_ARRAYS if ver >= 7 else ()) + (_ITERATED_ARRAYS if ver >= 8 else ()))
        missing = [k for k in need if k not in g.files]
        if missing:
            raise ValueError("an %s file holds %s: %s is missing" % (fmt, ", ".join(need), ", ".join(missing)))
        t = TrajectoryLog()
        for k in range(len(g["u"])):
            a, b = g["obs_ptr"][k], g["obs_ptr"][k + 1]
            c, d = g["lm_ptr"][k], g["lm_ptr"][k + 1]
            t.record(g["u"][k], g["obs"][a:b], g["lm_index"][c:d], g["lm_loc"][c:d])
        if fmt != FORMAT:
            for q in range(len(g["edit_step"])):
                a, b = g["edit_ptr"][q], g["edit_ptr"][q + 1]
                t.edits.append((int(g["edit_step"][q]), _KINDS[int(g["edit_kind"][q])], g["edit_idx"][a:b].astype(np.int64),
                                g["edit_delta"][q].copy(), g["edit_R"][q].copy()))
        if ver >= 8:
            for k, q in enumerate(g["iter_edit"]):
                anchor = g["iter_anchor"][k].copy()
                t.model_iterations[int(q)] = dict(model=int(g["iter_model"][k]), anchor=None if np.all(np.isnan(anchor)) else anchor,
                                                  gate=float(g["iter_gate"][k]), iterations=int(g["iter_iterations"][k]), tol=float(g["iter_tol"][k]))
        if ver >= 7:
            from ._lib import EKF_MOTION_INPUTS
            for k, q in enumerate(g["predict_edit"]):
                a, b = int(g["predict_ptr"][k]), int(g["predict_ptr"][k + 1])
                sts = []
                for e in range(a, b):
                    model = int(g["predict_model"][e])
                    nu = EKF_MOTION_INPUTS.get(model, 3)
                    sts.append((model, g["predict_u"][e][:nu].copy(), g["predict_M"][e][:nu, :nu].copy()))
                t.model_predicts[int(q)] = sts
        if ver >= 6:
            for k, q in enumerate(g["append_edit"]):
                a, b = int(g["append_ptr"][k]), int(g["append_ptr"][k + 1])
                t.model_appends[int(q)] = [(int(g["append_model"][e]), g["append_z"][e].copy(), g["append_R"][e].copy(),
                                            float(g["append_signature"][e])) for e in range(a, b)]
        if ver >= 5:
            for k, q in enumerate(g["model_edit"]):
                anchor = g["model_anchor"][k].copy()
                t.model_observations[int(q)] = dict(model=int(g["model_id"][k]), anchor=None if np.all(np.isnan(anchor)) else anchor,
                                                    gate=float(g["model_gate"][k]))
        if ver >= 4:
            for k, q in enumerate(g["observe_edit"]):
                t.observations[int(q)] = dict(Hr=g["observe_Hr"][k].copy(), Hl=g["observe_Hl"][k].copy(), gate=float(g["observe_gate"][k]),
                                              wrap=g["observe_wrap"][k].astype(np.int64), rows=int(g["observe_rows"][k]))
        return t

    def replay(self, engine, start=0, stop=None):
        """predict + measure for steps [start, stop) on anything with predict(u) / measure(obs, u, idx, loc) -- an Engine.  The edits
        recorded at positions [start, stop) are applied in front of their step through the engine's remove_landmarks /
        constrain_landmarks / merge_landmarks / merge_landmarks_batch / observe_linear / observe_model / observe_model_iterated / append_model / predict_model (0-based there: the recorded 1-based numbers are converted here); the ones recorded
        at position len(self), after the last step, when stop is the end of the log."""
        stop = len(self) if stop is None else stop

        def apply_edits(at):
            for q, (step, kind, idx, delta, R) in enumerate(self.edits):
                if step != at:
                    continue
                idx0 = [int(i) - 1 for i in idx]
                if kind == OBSERVE:
                    o = self.observations[q]
                    engine.observe_linear(delta[:o["rows"]], R, o["Hr"], idx0, [o["Hl"][b] for b in range(len(idx0))], gate=o["gate"],
                                          wrap=tuple(int(w) for w in o["wrap"]), rows=o["rows"])
                elif kind == OBSERVE_MODEL:
                    o = self.model_observations[q]
                    engine.observe_model(o["model"], delta, R, idx0, anchor=o["anchor"], gate=o["gate"])
                elif kind == OBSERVE_MODEL_ITERATED:
                    o = self.model_iterations[q]
                    engine.observe_model_iterated(o["model"], delta, R, idx0, anchor=o["anchor"], gate=o["gate"], iterations=o["iterations"],
                                                  tol=o["tol"])
                elif kind == APPEND_MODEL:
                    engine.append_model(self.model_appends[q])
                elif kind == PREDICT_MODEL:
                    engine.predict_model(self.model_predicts[q])
                elif kind == "remove":
                    engine.remove_landmarks(idx0)
                elif kind == "constrain":
                    engine.constrain_landmarks(idx0[0], idx0[1], delta, R)
                elif kind == "merge":
                    engine.merge_landmarks(idx0[0], idx0[1], R)
                else:
                    engine.merge_landmarks_batch(list(zip(idx0[0::2], idx0[1::2])), R)

        for k in range(start, stop):
            apply_edits(k)
            engine.predict(self.u[k])
            if len(self.obs[k]):
                engine.measure(self.obs[k], self.u[k], self.lm_index[k], self.lm_loc[k])
        if stop == len(self) and stop > start:
            apply_edits(stop)
