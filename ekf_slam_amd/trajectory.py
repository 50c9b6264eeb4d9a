"""On-disk trajectory log: everything the EKF hot path consumed, step by step.

The reference has no recorded data of any kind (its inputs are live ROS topics).  A log holds, per SLAM iteration,
the odometry `u` handed to predict() (SLAM.m:105-110) and what measure() saw after the landmark front-end ran
(EKF_SLAM.m:102,111,120): `observed_LL` (m x 3) and the landmark table (index, loc).  Replaying a log into an
engine reproduces the run bit for bit on the same hardware, and is how a run on one machine is compared with
another (or with the CPU oracle).  Format: one .npz with ragged arrays (`*_ptr` are CSR-style offsets).

A map that can be edited (ekf_slam_amd/slam.py) needs its edits in the log too, or a replay no longer reproduces the run.  An edit is
(step, kind, idx, delta, R): the position `len(log)` it was made at -- it is replayed after step len(log) - 1 and before step len(log) --
its kind, the 1-based landmark numbers that layer consumed, and two slots of 2 and 2 x 2 doubles (delta and R of a constraint, z and R of
an observation).  What a kind holds beyond that is its PAYLOAD, kept in a dictionary of its own under the edit's position.  The kinds,
the format that first carries each, the arrays a file has for it and how a replay applies it are ONE table, `_KINDS_TABLE` below.  A file
is written in the highest format any of its edits needs (no edits: format 1, the same arrays as ever) and holds the arrays of every kind
up to that format, empty where nothing was recorded -- a reader of an older format alone would not know the newer kinds.

A scan the DEVICE assigned and applied (measure_model_assigned(..., device_apply=True) of ekf_slam_amd/slam.py) has NO kind of its own: once
its result has been fetched it is recorded as one 'observe_model' edit per entry, in scan order -- an assigned entry with its landmark and
the scan's gate, an entry that was left out with landmark 1 and a gate of -1.0.  On replay the latter is an observe_model that cannot
apply (d2 >= 0 > -1, or irregular): it leaves the zero pair in the ring slot the device's skipped step left, so a replay reproduces x, s
and P bit for bit on every storage kind and batch size.  Only what linear_rejections counts differs, by the left-out entries: the replay
counts each as gated (or irregular), the device's skipped step is counted by neither counter.
"""
from collections import namedtuple

import numpy as np

from ._lib import EKF_MOTION_INPUTS

FORMAT = "ekfslam-trajectory-1"
FORMAT_EDITS = "ekfslam-trajectory-2"
FORMAT_BATCH = "ekfslam-trajectory-3"
FORMAT_OBSERVE = "ekfslam-trajectory-4"
FORMAT_MODEL = "ekfslam-trajectory-5"
FORMAT_APPEND = "ekfslam-trajectory-6"
FORMAT_PREDICT = "ekfslam-trajectory-7"
FORMAT_ITERATED = "ekfslam-trajectory-8"
FORMAT_JOINT = "ekfslam-trajectory-9"
FORMAT_JOINT_ITERATED = "ekfslam-trajectory-10"
FORMAT_JOIN_MAP = "ekfslam-trajectory-11"
FORMAT_TRANSFORM_MAP = "ekfslam-trajectory-12"
FORMAT_OBSERVE_DENSE = "ekfslam-trajectory-13"
EDIT_KINDS = ("remove", "constrain", "merge", "merge_batch")        # what record_edit takes
OBSERVE = "observe"                                                  # record_observation's
OBSERVE_MODEL = "observe_model"                                      # record_model_observation's
APPEND_MODEL = "append_model"                                        # record_model_append's
PREDICT_MODEL = "predict_model"                                      # record_model_predict's
OBSERVE_MODEL_ITERATED = "observe_model_iterated"                    # record_model_observation_iterated's
OBSERVE_MODEL_JOINT = "observe_model_joint"                          # record_model_observation_joint's
OBSERVE_MODEL_JOINT_ITERATED = "observe_model_joint_iterated"        # record_model_observation_joint_iterated's
JOIN_MAP = "join_map"                                                # record_map_join's
TRANSFORM_MAP = "transform_map"                                      # record_map_transform's
OBSERVE_DENSE = "observe_dense"                                      # record_dense_observation's
_FORMATS = (FORMAT, FORMAT_EDITS, FORMAT_BATCH, FORMAT_OBSERVE, FORMAT_MODEL, FORMAT_APPEND, FORMAT_PREDICT, FORMAT_ITERATED, FORMAT_JOINT,
            FORMAT_JOINT_ITERATED)
# ... the ten formats of a log that speaks of ONE map; a log with a join also holds a second map's state and is written in the eleventh
_ALL_FORMATS = _FORMATS + (FORMAT_JOIN_MAP,)
# ... and every format a file may carry: the twelfth adds the map's change of frame (the two tuples above are counted by their users)
_EVERY_FORMAT = _ALL_FORMATS + (FORMAT_TRANSFORM_MAP,)
# ... and what save and load index: the thirteenth adds the linear observation with a dense H (the three tuples above keep their contents)
_FORMATS_ON_DISK = _EVERY_FORMAT + (FORMAT_OBSERVE_DENSE,)
_STEP_ARRAYS = ("u", "obs_ptr", "obs", "lm_ptr", "lm_index", "lm_loc")
_EDIT_ARRAYS = ("edit_step", "edit_kind", "edit_ptr", "edit_idx", "edit_delta", "edit_R")

# One array of a kind's payload in a file: `<prefix>_<suffix>`, one row of shape `tail` per payload (per entry, for a payload that is a
# list), taken from payload[key].  A smaller value fills the leading corner of its row; optional: None travels as NaN.
_Field = namedtuple("_Field", "suffix key dtype tail optional", defaults=(False,))
_F, _I = np.float64, np.int64
_ANCHOR = _Field("anchor", "anchor", _F, (2,), True)                 # NaN where the target is a landmark

# A kind of edit.  name: what an edit tuple carries; its position here is its number in a file's edit_kind.  format: the first that
# carries it.  replay(engine, idx0, delta, R, payload): applies one, landmarks 0-based.  store: the TrajectoryLog dictionary of its
# payloads (None: the edit tuple is all there is); prefix, fields: the file's arrays for them, behind `<prefix>_edit`, the positions of
# the edits they belong to.  entries: the payload is a list of tuples (fields keyed by index) behind the CSR offsets `<prefix>_ptr`.
# trim(entry): what a loaded entry is cut back to.  ragged: the payload is a dictionary; a field of tail None is an array whose size differs
# from edit to edit and travels flattened behind CSR offsets of its own, `<prefix>_<suffix>_ptr` (shape(key, flat) gives a loaded one its
# shape), a field of tail () is one number per edit.
_Kind = namedtuple("_Kind", "name format replay store prefix fields entries trim ragged shape",
                   defaults=(None, None, (), False, None, False, None))


def _replay_observe(engine, idx0, z, R, o):
    engine.observe_linear(z[:o["rows"]], R, o["Hr"], idx0, [o["Hl"][b] for b in range(len(idx0))], gate=o["gate"],
                          wrap=tuple(int(w) for w in o["wrap"]), rows=o["rows"])


def _replay_join(engine, idx0, d, R, o):
    """The local map into a scratch F64 engine on the engine's device, then the join: exact for a local map that had float tiles too,
    since every float is a double and the live diagonal copies are F64 on every storage kind."""
    from .engine import Engine
    M = o["s"].size
    local = Engine(mode="known", capacity=max(M, 1), storage="f64", device=int(engine.cfg.device))
    try:
        local.set_x(o["x"])
        if M:
            local.set_s(o["s"])
        local.set_P(o["P"])
        engine.join_map(local, o["offset"])
    finally:
        local.close()


def _join_shape(key, flat):
    if key == "P":
        n = int(round(flat.size ** 0.5))
        return flat.reshape(n, n)
    return flat


def _trim_motion(step):
    """u and M of the size the model reads: a model with two inputs left the rest of its row zero."""
    nu = EKF_MOTION_INPUTS.get(step[0], 3)
    return step[0], step[1][:nu].copy(), step[2][:nu, :nu].copy()


def _dense_H(o):
    """The k x n H of an 'observe_dense' payload from its (row, column, value) triplets."""
    H = np.zeros((o["rows"], o["n"]))
    H[o["row"], o["col"]] = o["val"]
    return H


def _replay_dense(engine, idx0, d, R, o):
    engine.observe_dense(_dense_H(o), o["z"], o["R"], gate=o["gate"], wrap_deg=[int(w) for w in o["wrap"]])


def _dense_shape(key, flat):
    if key == "R":
        k = int(round(flat.size ** 0.5))
        return flat.reshape(k, k)
    return flat


_KINDS_TABLE = (
    # the map edits of record_edit: idx names the landmarks, delta and R are the constraint's (zero where the kind has none)
    _Kind("remove", 2, lambda e, idx0, d, R, _: e.remove_landmarks(idx0)),
    _Kind("constrain", 2, lambda e, idx0, d, R, _: e.constrain_landmarks(idx0[0], idx0[1], d, R)),
    _Kind("merge", 2, lambda e, idx0, d, R, _: e.merge_landmarks(idx0[0], idx0[1], R)),
    # merge_landmarks_batch: idx = [keep1, drop1, keep2, drop2, ...], R shared.  Format 3 has the arrays of format 2
    _Kind("merge_batch", 3, lambda e, idx0, d, R, _: e.merge_landmarks_batch(list(zip(idx0[0::2], idx0[1::2])), R)),
    # observe_linear: idx = the 0, 1 or 2 landmarks that carry a block, the delta slot = z, R; per observation Hr, the landmark blocks
    # Hl, gate, wrap and rows
    _Kind(OBSERVE, 4, _replay_observe, "observations", "observe",
          (_Field("Hr", "Hr", _F, (2, 3)), _Field("Hl", "Hl", _F, (2, 2, 2)), _Field("gate", "gate", _F, ()), _Field("wrap", "wrap", _I, (2,)),
           _Field("rows", "rows", _I, ()))),
    # observe_model: idx = the 0, 1 or 2 landmarks, the delta slot = z, R; per observation the model, the anchor and the gate
    _Kind(OBSERVE_MODEL, 5, lambda e, idx0, z, R, o: e.observe_model(o["model"], z, R, idx0, anchor=o["anchor"], gate=o["gate"]),
          "model_observations", "model", (_Field("id", "model", _I, ()), _ANCHOR, _Field("gate", "gate", _F, ()))),
    # add_landmarks_model: one scan of new landmarks, idx empty; per scan its entries (model, z, R, signature)
    _Kind(APPEND_MODEL, 6, lambda e, idx0, d, R, entries: e.append_model(entries), "model_appends", "append",
          (_Field("model", 0, _I, ()), _Field("z", 1, _F, (2,)), _Field("R", 2, _F, (2, 2)), _Field("signature", 3, _F, ())), True),
    # predict_model: one chain of motion steps, idx empty; per chain its steps (model, u, M), u and M in the leading entries of 3 and 3 x 3
    _Kind(PREDICT_MODEL, 7, lambda e, idx0, d, R, steps: e.predict_model(steps), "model_predicts", "predict",
          (_Field("model", 0, _I, ()), _Field("u", 1, _F, (3,)), _Field("M", 2, _F, (3, 3))), True, _trim_motion),
    # observe_model_iterated: an observe_model edit's slots; per observation the model, the anchor, the gate, iterations and tol
    _Kind(OBSERVE_MODEL_ITERATED, 8,
          lambda e, idx0, z, R, o: e.observe_model_iterated(o["model"], z, R, idx0, anchor=o["anchor"], gate=o["gate"],
                                                            iterations=o["iterations"], tol=o["tol"]),
          "model_iterations", "iter", (_Field("model", "model", _I, ()), _ANCHOR, _Field("gate", "gate", _F, ()),
                                       _Field("iterations", "iterations", _I, ()), _Field("tol", "tol", _F, ()))),
    # observe_model_joint: one scan applied as one joint update, idx empty, the first value of the delta slot = the gate (R zero); per scan
    # its entries (model, z, R, landmark), the landmark 1-based and 0 = left out
    _Kind(OBSERVE_MODEL_JOINT, 9,
          lambda e, idx0, d, R, entries: e.observe_model_joint([dict(model=m, z=z, R=Rk) for m, z, Rk, _ in entries],
                                                               [lm - 1 for _, _, _, lm in entries], gate=float(d[0])),
          "model_joints", "joint",
          (_Field("model", 0, _I, ()), _Field("z", 1, _F, (2,)), _Field("R", 2, _F, (2, 2)), _Field("landmark", 3, _I, ())), True),
    # observe_model_joint_iterated: that scan relinearised, idx empty, the delta slot = (gate, tol), the first value of the R slot = the
    # number of linearisations; per scan its entries as above
    _Kind(OBSERVE_MODEL_JOINT_ITERATED, 10,
          lambda e, idx0, d, R, entries: e.observe_model_joint([dict(model=m, z=z, R=Rk) for m, z, Rk, _ in entries],
                                                               [lm - 1 for _, _, _, lm in entries], gate=float(d[0]),
                                                               iterations=int(R[0, 0]), tol=float(d[1])),
          "model_joint_iterations", "jointiter",
          (_Field("model", 0, _I, ()), _Field("z", 1, _F, (2,)), _Field("R", 2, _F, (2, 2)), _Field("landmark", 3, _I, ())), True),
    # join_map: a local map joined into the map, idx empty; per join the local x, s and dense P (as read once after the call's flush) and
    # the signature offset: the three arrays flattened behind CSR offsets of their own, the offset one number per join
    _Kind(JOIN_MAP, 11, _replay_join, "map_joins", "join",
          (_Field("x", "x", _F, None), _Field("s", "s", _F, None), _Field("P", "P", _F, None), _Field("offset", "offset", _F, ())),
          ragged=True, shape=_join_shape),
    # transform_map: the whole map moved into another frame, idx empty; per transform the frame (0: the rigid transform t with covariance
    # Sigma, None travelling as NaN: an exact one; 1: the robot's own frame, t and Sigma both None)
    _Kind(TRANSFORM_MAP, 12,
          lambda e, idx0, d, R, o: e.transform_map("robot" if o["frame"] else "map", o["t"], o["Sigma"]),
          "map_transforms", "transform",
          (_Field("frame", "frame", _I, ()), _Field("t", "t", _F, (3,), True), _Field("Sigma", "Sigma", _F, (3, 3), True))),
)
_KINDS = tuple(k.name for k in _KINDS_TABLE)
# ... the kinds of a file up to format 12, which their users count.  What save, load and replay go through is the table with the kinds
# added since behind them (a kind's position is its number in a file's edit_kind, so the older numbers stay what they were):
_KINDS_ON_DISK_TABLE = _KINDS_TABLE + (
    # observe_dense: a linear observation with a dense k x n H, idx empty; per observation k, n, the gate, H SPARSE as (row, column, value)
    # triplets of its non-zero entries in row-major order, z (k), R (k x k) and the wrap flags (k), each flattened behind CSR offsets of its own
    _Kind(OBSERVE_DENSE, 13, _replay_dense, "dense_observations", "dense",
          (_Field("rows", "rows", _I, ()), _Field("n", "n", _I, ()), _Field("gate", "gate", _F, ()), _Field("row", "row", _I, None),
           _Field("col", "col", _I, None), _Field("val", "val", _F, None), _Field("z", "z", _F, None), _Field("R", "R", _F, None),
           _Field("wrap", "wrap", _I, None)),
          ragged=True, shape=_dense_shape),
)
_KINDS_ON_DISK = tuple(k.name for k in _KINDS_ON_DISK_TABLE)
_KIND = {k.name: k for k in _KINDS_ON_DISK_TABLE}


def _arrays_of(kind):
    if kind.ragged:
        return (kind.prefix + "_edit",) + tuple(kind.prefix + "_" + f.suffix + t for f in kind.fields for t in (("_ptr", "") if f.tail is None else ("",)))
    return (kind.prefix + "_edit",) + ((kind.prefix + "_ptr",) if kind.entries else ()) + tuple(kind.prefix + "_" + f.suffix for f in kind.fields)


def _pack(kind, store):
    """The file's arrays for the payloads of one kind, in the order of their edits."""
    at = sorted(store)
    out = {kind.prefix + "_edit": np.array(at, dtype=np.int64)}
    items = [store[q] for q in at]
    if kind.ragged:
        for f in kind.fields:
            if f.tail is not None:
                out[kind.prefix + "_" + f.suffix] = np.array([it[f.key] for it in items], dtype=f.dtype)
                continue
            parts = [np.asarray(it[f.key], dtype=f.dtype).reshape(-1) for it in items]
            out[kind.prefix + "_" + f.suffix + "_ptr"] = np.cumsum([0] + [p.size for p in parts]).astype(np.int64)
            out[kind.prefix + "_" + f.suffix] = np.concatenate(parts) if parts else np.zeros(0, dtype=f.dtype)
        return out
    if kind.entries:
        out[kind.prefix + "_ptr"] = np.cumsum([0] + [len(p) for p in items])
        items = [e for p in items for e in p]
    for f in kind.fields:
        col = np.zeros((len(items),) + f.tail, dtype=f.dtype)
        for k, it in enumerate(items):
            v = np.full(f.tail, np.nan) if f.optional and it[f.key] is None else np.asarray(it[f.key])
            col[(k,) + tuple(slice(0, n) for n in v.shape)] = v
        out[kind.prefix + "_" + f.suffix] = col
    return out


def _unpack(kind, g, store):
    """_pack's inverse: the payloads of one kind from a file's arrays into a log's dictionary."""
    def value(f, row):
        v = g[kind.prefix + "_" + f.suffix][row]
        if f.tail == ():
            return int(v) if f.dtype is _I else float(v)
        if f.optional and np.all(np.isnan(v)):
            return None
        return v.astype(np.int64) if f.dtype is _I else v.copy()
    for k, q in enumerate(g[kind.prefix + "_edit"]):
        if kind.ragged:
            payload = {}
            for f in kind.fields:
                if f.tail is not None:
                    payload[f.key] = value(f, k)
                    continue
                ptr = g[kind.prefix + "_" + f.suffix + "_ptr"]
                payload[f.key] = kind.shape(f.key, g[kind.prefix + "_" + f.suffix][int(ptr[k]):int(ptr[k + 1])].copy())
            store[int(q)] = payload
        elif kind.entries:
            a, b = int(g[kind.prefix + "_ptr"][k]), int(g[kind.prefix + "_ptr"][k + 1])
            entries = [tuple(value(f, e) for f in kind.fields) for e in range(a, b)]
            store[int(q)] = [kind.trim(e) for e in entries] if kind.trim else entries
        else:
            store[int(q)] = {f.key: value(f, k) for f in kind.fields}


class TrajectoryLog:
    def __init__(self):
        self.u, self.obs, self.lm_index, self.lm_loc = [], [], [], []
        self.edits = []             # (step, kind, idx (1-based numbers), delta[2], R[2x2]) in the order they were made
        self.model_observations = {}  # position in self.edits of an 'observe_model' edit -> {model, anchor (2) or None, gate}
        self.model_appends = {}     # position in self.edits of an 'append_model' edit -> [(model, z (2), R (2x2), signature), ...]
        self.model_predicts = {}    # position in self.edits of a 'predict_model' edit -> [(model, u (2 or 3), M (2x2 or 3x3)), ...]
        self.model_iterations = {}  # position in self.edits of an 'observe_model_iterated' edit -> {model, anchor or None, gate, iterations, tol}
        self.model_joints = {}      # position in self.edits of an 'observe_model_joint' edit -> [(model, z (2), R (2x2), landmark 1-based or 0), ...]
        self.model_joint_iterations = {}  # position in self.edits of an 'observe_model_joint_iterated' edit -> the same list
        self.map_transforms = {}    # position in self.edits of a 'transform_map' edit -> {frame 0 / 1, t (3) or None, Sigma (3x3) or None}
        self.map_joins = {}         # position in self.edits of a 'join_map' edit -> {x (3 + 2 M), s (M), P dense, offset}: the local map
        self.dense_observations = {}  # position in self.edits of an 'observe_dense' edit -> {rows, n, gate, row, col, val (H's triplets), z, R (k x k), wrap}
        self.observations = {}      # position in self.edits of an 'observe' edit -> {Hr (2x3), Hl (2x2x2), gate, wrap (2), rows}

    def __len__(self):
        return len(self.u)

    def record(self, u, observed_LL, lm_index, lm_loc):
        self.u.append(np.asarray(u, dtype=np.float64).reshape(2).copy())
        obs = np.zeros((0, 3)) if observed_LL is None or len(observed_LL) == 0 else np.asarray(observed_LL, dtype=np.float64)
        self.obs.append(obs.reshape(-1, 3).copy())
        self.lm_index.append(np.asarray(lm_index, dtype=np.float64).reshape(-1).copy())
        self.lm_loc.append(np.asarray(lm_loc, dtype=np.float64).reshape(-1, 2).copy())

    @staticmethod
    def _landmarks(who, landmarks, most=None, refusal="at most two landmarks"):
        lms = np.asarray(landmarks, dtype=np.float64).reshape(-1)
        if not np.all(lms == np.floor(lms)):
            raise ValueError("%s: landmark indices are whole numbers" % who)
        if most is not None and lms.size > most:
            raise ValueError("%s: %s" % (who, refusal))
        return lms.astype(np.int64)

    def _record(self, kind, lms=(), z=(), R=None, payload=None):
        """An edit made now, i.e. after the len(self) steps recorded so far: z padded with zeros to the two values of its slot, R None:
        the zero matrix; the payload goes into the kind's dictionary under the edit's position."""
        zv = np.zeros(2)
        zin = np.asarray(z, dtype=np.float64).reshape(-1)
        zv[:zin.size] = zin
        Rm = np.zeros((2, 2)) if R is None else np.asarray(R, dtype=np.float64).reshape(2, 2).copy()
        if payload is not None:
            getattr(self, _KIND[kind].store)[len(self.edits)] = payload
        self.edits.append((len(self), kind, np.asarray(lms, dtype=np.int64), zv, Rm))

    def record_edit(self, kind, idx, delta=None, R=None):
        """A map edit made now, i.e. after the len(self) steps recorded so far.  kind: 'remove' (idx: the landmarks), 'constrain'
        (idx: [i, j]), 'merge' (idx: [keep, drop]) or 'merge_batch' (idx: [keep1, drop1, keep2, drop2, ...], non-empty; R shared by
        all pairs); landmark numbers 1-based; delta None: (0, 0), R None: the zero matrix."""
        if kind not in EDIT_KINDS:
            raise ValueError("record_edit: kind is one of %s" % (EDIT_KINDS,))
        idx = self._landmarks("record_edit", idx)
        if kind == "merge_batch":
            if idx.size == 0 or idx.size % 2:
                raise ValueError("record_edit: 'merge_batch' names (keep, drop) pairs, at least one")
        elif kind != "remove" and idx.size != 2:
            raise ValueError("record_edit: '%s' names two landmarks" % kind)
        self._record(kind, idx, () if delta is None else np.asarray(delta, dtype=np.float64).reshape(2), R)

    def record_observation(self, z, R, Hr=None, landmarks=(), Hl=(), gate=float("inf"), wrap=(0, 0), rows=2):
        """A linear observation (observe_linear of ekf_slam_amd/slam.py) made now, i.e. after the len(self) steps recorded so far:
        z, R (2 x 2), the robot block Hr (2 x 3, None: zeros), the 1-based landmarks that carry a block and their 2 x 2 blocks Hl,
        gate, wrap and rows -- full-size arrays, as the wrapper hands them to the engine."""
        who, refusal = "record_observation", "at most two landmarks, one 2 x 2 block each"
        lms = self._landmarks(who, list(landmarks), 2, refusal)
        blocks = [np.asarray(b, dtype=np.float64).reshape(2, 2) for b in Hl]
        if len(blocks) != lms.size:
            raise ValueError("%s: %s" % (who, refusal))
        if int(rows) not in (1, 2):
            raise ValueError("%s: rows is 1 or 2" % who)
        Hlm = np.zeros((2, 2, 2))
        for b, blk in enumerate(blocks):
            Hlm[b] = blk
        w = tuple(wrap) + (0, 0)
        self._record(OBSERVE, lms, z, R, dict(
            Hr=np.zeros((2, 3)) if Hr is None else np.asarray(Hr, dtype=np.float64).reshape(2, 3).copy(), Hl=Hlm, gate=float(gate),
            wrap=np.array([int(bool(w[0])), int(bool(w[1]))], dtype=np.int64), rows=int(rows)))

    def record_model_observation(self, model, z, R, landmarks=(), anchor=None, gate=float("inf")):
        """An observation through a model (observe_model of ekf_slam_amd/slam.py) made now, i.e. after the len(self) steps recorded so
        far: the model's number, z, R (2 x 2), the 1-based landmarks, the anchor (None: the target is a landmark) and the gate."""
        self._record(OBSERVE_MODEL, self._landmarks("record_model_observation", list(landmarks), 2), z, R, dict(
            model=int(model), anchor=None if anchor is None else np.asarray(anchor, dtype=np.float64).reshape(2).copy(), gate=float(gate)))

    def record_model_observation_iterated(self, model, z, R, landmarks=(), anchor=None, gate=float("inf"), iterations=1, tol=0.0):
        """A relinearised observation through a model (observe_model_iterated of ekf_slam_amd/slam.py) made now, i.e. after the len(self)
        steps recorded so far: record_model_observation's arguments, then the number of linearisations and the stopping tolerance."""
        self._record(OBSERVE_MODEL_ITERATED, self._landmarks("record_model_observation_iterated", list(landmarks), 2), z, R, dict(
            model=int(model), anchor=None if anchor is None else np.asarray(anchor, dtype=np.float64).reshape(2).copy(), gate=float(gate),
            iterations=int(iterations), tol=float(tol)))

    def record_model_observation_joint(self, entries, gate=float("inf")):
        """One scan applied as ONE joint update (observe_model_joint of ekf_slam_amd/slam.py) made now, i.e. after the len(self) steps
        recorded so far: entries = [(model, z, R, landmark), ...], at least one, z padded to two values and R 2 x 2 as the wrapper hands
        them to the engine, the landmark 1-based and 0 where the observation is left out; then the joint gate."""
        lms = self._landmarks("record_model_observation_joint", [e[3] for e in entries])
        ents = [(int(m), np.asarray(z, dtype=np.float64).reshape(2).copy(), np.asarray(R, dtype=np.float64).reshape(2, 2).copy(), int(lm))
                for (m, z, R, _), lm in zip(entries, lms)]
        if not ents:
            raise ValueError("record_model_observation_joint: at least one entry")
        self._record(OBSERVE_MODEL_JOINT, z=(float(gate),), payload=ents)

    def record_model_observation_joint_iterated(self, entries, gate=float("inf"), iterations=1, tol=0.0):
        """That scan RELINEARISED (observe_model_joint(..., iterations > 1) of ekf_slam_amd/slam.py) made now:
        record_model_observation_joint's arguments, then the number of linearisations and the stopping tolerance."""
        lms = self._landmarks("record_model_observation_joint_iterated", [e[3] for e in entries])
        ents = [(int(m), np.asarray(z, dtype=np.float64).reshape(2).copy(), np.asarray(R, dtype=np.float64).reshape(2, 2).copy(), int(lm))
                for (m, z, R, _), lm in zip(entries, lms)]
        if not ents:
            raise ValueError("record_model_observation_joint_iterated: at least one entry")
        self._record(OBSERVE_MODEL_JOINT_ITERATED, z=(float(gate), float(tol)), R=[[float(int(iterations)), 0.0], [0.0, 0.0]], payload=ents)

    def record_model_append(self, entries):
        """One scan of new landmarks (add_landmarks_model of ekf_slam_amd/slam.py) made now, i.e. after the len(self) steps recorded so
        far: entries = [(model, z, R, signature), ...], at least one, as the wrapper hands them to the engine."""
        ents = [(int(m), np.asarray(z, dtype=np.float64).reshape(2).copy(), np.asarray(R, dtype=np.float64).reshape(2, 2).copy(), float(s))
                for m, z, R, s in entries]
        if not ents:
            raise ValueError("record_model_append: at least one entry")
        self._record(APPEND_MODEL, payload=ents)

    def record_map_join(self, x, s, P, signature_offset=0.0):
        """A local map joined into the map (join_map of ekf_slam_amd/slam.py) made now, i.e. after the len(self) steps recorded so far:
        the local state x (3 + 2 M), its signatures s (M) and its dense covariance P as they were when the join read them, then the
        signature offset."""
        xv = np.asarray(x, dtype=np.float64).reshape(-1).copy()
        sv = np.asarray(s, dtype=np.float64).reshape(-1).copy()
        Pm = np.asarray(P, dtype=np.float64)
        if xv.size < 3 or (xv.size - 3) % 2 or sv.size != (xv.size - 3) // 2 or Pm.size != xv.size * xv.size:
            raise ValueError("record_map_join: x has 3 + 2 M values, s has M and P is square of x's size")
        self._record(JOIN_MAP, payload=dict(x=xv, s=sv, P=Pm.reshape(xv.size, xv.size).copy(), offset=float(signature_offset)))

    def record_map_transform(self, frame, t=None, Sigma=None):
        """The whole map moved into another frame (transform_map / recenter_on_robot of ekf_slam_amd/slam.py) now, i.e. after the
        len(self) steps recorded so far: frame "map" with the rigid transform t (3) and its covariance Sigma (3 x 3, None: exact), or
        frame "robot" with neither."""
        if frame not in ("map", "robot"):
            raise ValueError("record_map_transform: frame is 'map' or 'robot'")
        if (frame == "map") != (t is not None) or (frame == "robot" and Sigma is not None):
            raise ValueError("record_map_transform: 'map' takes t and maybe Sigma, 'robot' takes neither")
        tv = None if t is None else np.asarray(t, dtype=np.float64).reshape(3).copy()
        Sm = None if Sigma is None else np.asarray(Sigma, dtype=np.float64).reshape(3, 3).copy()
        self._record(TRANSFORM_MAP, payload=dict(frame=int(frame == "robot"), t=tv, Sigma=Sm))

    def record_dense_observation(self, H, z, R, gate=float("inf"), wrap_deg=None):
        """A linear observation with a dense H (observe_dense of ekf_slam_amd/slam.py) made now, i.e. after the len(self) steps recorded
        so far: H (k x n) as the wrapper handed it to the engine -- kept as the triplets of its non-zero entries --, z (k), R (k x k,
        symmetric), the gate and the wrap flags (None: none)."""
        Hv = np.asarray(H, dtype=np.float64)
        if Hv.ndim != 2 or Hv.shape[0] < 1:
            raise ValueError("record_dense_observation: H is k >= 1 rows")
        k, n = Hv.shape
        zv, Rm = np.asarray(z, dtype=np.float64).reshape(-1).copy(), np.asarray(R, dtype=np.float64)
        if zv.size != k or Rm.size != k * k:
            raise ValueError("record_dense_observation: z has k values and R is k x k")
        wv = np.zeros(k, dtype=np.int64) if wrap_deg is None else np.array([int(bool(w)) for w in wrap_deg], dtype=np.int64)
        if wv.size != k:
            raise ValueError("record_dense_observation: wrap_deg has k flags")
        row, col = np.nonzero(Hv)
        self._record(OBSERVE_DENSE, payload=dict(rows=int(k), n=int(n), gate=float(gate), row=row.astype(np.int64), col=col.astype(np.int64),
                                                 val=Hv[row, col].copy(), z=zv, R=Rm.reshape(k, k).copy(), wrap=wv))

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
        self._record(PREDICT_MODEL, payload=sts)

    def save(self, path):
        def ragged(parts, width):
            ptr = np.cumsum([0] + [len(p) for p in parts])
            data = np.concatenate(parts) if parts and ptr[-1] else np.zeros((0, width) if width else (0,))
            return ptr, data
        ver = max([1] + [_KIND[e[1]].format for e in self.edits])
        arrays = dict(format=np.array(_FORMATS_ON_DISK[ver - 1]))
        if self.edits:
            e_ptr, e_idx = ragged([e[2] for e in self.edits], 0)
            arrays.update(edit_step=np.array([e[0] for e in self.edits], dtype=np.int64),
                          edit_kind=np.array([_KINDS_ON_DISK.index(e[1]) for e in self.edits], dtype=np.int64), edit_ptr=e_ptr,
                          edit_idx=e_idx.astype(np.int64), edit_delta=np.array([e[3] for e in self.edits]).reshape(-1, 2),
                          edit_R=np.array([e[4] for e in self.edits]).reshape(-1, 2, 2))
        obs_ptr, obs = ragged(self.obs, 3)
        lm_ptr, lmi = ragged(self.lm_index, 0)
        _, lml = ragged(self.lm_loc, 2)
        arrays.update(u=np.array(self.u).reshape(-1, 2), obs_ptr=obs_ptr, obs=obs, lm_ptr=lm_ptr, lm_index=lmi, lm_loc=lml)
        for kind in _KINDS_ON_DISK_TABLE:
            if kind.store and kind.format <= ver:
                arrays.update(_pack(kind, getattr(self, kind.store)))
        np.savez_compressed(path, **arrays)

    @staticmethod
    def load(path):
        g = np.load(path, allow_pickle=False)
        fmt = str(g["format"])
        if fmt not in _FORMATS_ON_DISK:
            raise ValueError("not an %s file" % " / ".join(_FORMATS_ON_DISK))
        ver = _FORMATS_ON_DISK.index(fmt) + 1
        held = [kind for kind in _KINDS_ON_DISK_TABLE if kind.store and kind.format <= ver]
        need = _STEP_ARRAYS + (_EDIT_ARRAYS if ver >= 2 else ()) + tuple(name for kind in held for name in _arrays_of(kind))
        missing = [k for k in need if k not in g.files]
        if missing:
            raise ValueError("an %s file holds %s: %s is missing" % (fmt, ", ".join(need), ", ".join(missing)))
        g = {k: g[k] for k in need}
        t = TrajectoryLog()
        for k in range(len(g["u"])):
            a, b = g["obs_ptr"][k], g["obs_ptr"][k + 1]
            c, d = g["lm_ptr"][k], g["lm_ptr"][k + 1]
            t.record(g["u"][k], g["obs"][a:b], g["lm_index"][c:d], g["lm_loc"][c:d])
        if ver >= 2:
            for q in range(len(g["edit_step"])):
                a, b = g["edit_ptr"][q], g["edit_ptr"][q + 1]
                t.edits.append((int(g["edit_step"][q]), _KINDS_ON_DISK[int(g["edit_kind"][q])], g["edit_idx"][a:b].astype(np.int64),
                                g["edit_delta"][q].copy(), g["edit_R"][q].copy()))
        for kind in held:
            _unpack(kind, g, getattr(t, kind.store))
        return t

    def replay(self, engine, start=0, stop=None):
        """predict + measure for steps [start, stop) on anything with predict(u) / measure(obs, u, idx, loc) -- an Engine.  The edits
        recorded at positions [start, stop) are applied in front of their step through the engine's method of their kind (_KINDS_TABLE;
        0-based there: the recorded 1-based numbers are converted here); the ones recorded at position len(self), after the last step,
        when stop is the end of the log."""
        stop = len(self) if stop is None else stop

        def apply_edits(at):
            for q, (step, kind, idx, delta, R) in enumerate(self.edits):
                if step == at:
                    k = _KIND[kind]
                    k.replay(engine, [int(i) - 1 for i in idx], delta, R, getattr(self, k.store)[q] if k.store else None)

        for k in range(start, stop):
            apply_edits(k)
            engine.predict(self.u[k])
            if len(self.obs[k]):
                engine.measure(self.obs[k], self.u[k], self.lm_index[k], self.lm_loc[k])
        if stop == len(self) and stop > start:
            apply_edits(stop)
