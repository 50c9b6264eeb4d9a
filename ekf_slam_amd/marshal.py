"""What turns Python arguments into what the C ABI takes, and the ABI's result structs into what the callers get: every conversion that
needs no handle.  engine.py goes through these for each entry point; slam.py calls the struct builders itself, so that a wrapper builds
ONE struct per call, hands that object to the Engine and writes its log from it.  Functions only; nothing here touches the state."""
import ctypes

import numpy as np

from . import _lib as L

_dp = ctypes.POINTER(ctypes.c_double)
INF = float("inf")


# ---- pointers ----
def _vec(v, n=None):
    a = np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1))
    if n is not None and a.size != n:
        raise ValueError("expected %d values, got %d" % (n, a.size))
    return a


def _p(a):
    return a.ctypes.data_as(_dp)


def p_or_null(a):
    return None if a is None else _p(a)


def _colmajor(M):
    return np.asfortranarray(np.asarray(M, dtype=np.float64))


def index_array(indices):
    """(int64[], count) of any iterable of whole numbers; an empty one still has a slot to point at."""
    idx = [int(i) for i in indices]
    return (ctypes.c_int64 * max(len(idx), 1))(*idx), len(idx)


def _fill(dst, values):
    """The leading entries of a struct's array from an array or a list (one slice assignment: a third of the cost of entry by entry)."""
    values = values.tolist() if isinstance(values, np.ndarray) else list(values)
    dst[:len(values)] = values


# ---- the noise matrix ----
def noise(R, who=None, one_row=False, or_what=""):
    """R as the ABI takes it: the four doubles of a 2 x 2 matrix, column-major; None (a null pointer, or a struct's zeros) where R is
    None.  one_row: a single value is the variance of the one row, R(0, 0).  Any other size is refused as '<who>: R is 2 x 2<or_what>'
    (who None: by the reshape itself)."""
    if R is None:
        return None
    Ra = np.asarray(R, dtype=np.float64)
    if one_row and Ra.size == 1:
        return np.array([float(Ra.reshape(-1)[0]), 0.0, 0.0, 0.0])
    if who is not None and Ra.size != 4:
        raise ValueError("%s: R is 2 x 2%s" % (who, or_what))
    return np.ascontiguousarray(Ra.reshape(2, 2).reshape(-1, order="F"))


# ---- the structs ----
def linear_obs(z, R, Hr, landmarks, Hl, gate, wrap, rows):
    """struct ekf_linear_obs of observe_linear's arguments (landmarks 0-based): full-size blocks, zero where rows = 1 leaves them out."""
    who = "linear observation"
    rows = int(rows)
    if rows not in (1, 2):
        raise ValueError("%s: rows is 1 or 2" % who)
    o = L.EkfLinearObs()
    zin = _vec(z)
    if not rows <= zin.size <= 2:
        raise ValueError("%s: z has `rows` values" % who)
    _fill(o.z, zin[:rows])
    Rf = noise(R, who, rows == 1, " (or a variance with rows = 1)")
    if Rf is not None:
        _fill(o.R, Rf)

    def block(M, width, what):
        """2 x width, or its first row alone where rows = 1; column-major."""
        Ma = np.asarray(M, dtype=np.float64)
        full = np.zeros((2, width))
        if Ma.size == 2 * width:
            full[:] = Ma.reshape(2, width)
        elif rows == 1 and Ma.size == width:
            full[0] = Ma.reshape(-1)
        else:
            raise ValueError("%s: %s" % (who, what))
        return full.reshape(-1, order="F")
    if Hr is not None:
        _fill(o.Hr, block(Hr, 3, "Hr is 2 x 3 (or 3 values with rows = 1)"))
    lms = [int(k) for k in landmarks]
    blocks = list(Hl)
    if len(lms) > 2 or len(blocks) != len(lms):
        raise ValueError("%s: at most two landmarks, one 2 x 2 block each" % who)
    o.lm[0] = o.lm[1] = -1
    for b, (k, blk) in enumerate(zip(lms, blocks)):
        _fill(o.Hl[b], block(blk, 2, "a landmark block is 2 x 2 (or 2 values with rows = 1)"))
        o.lm[b] = k
    o.gate = float(gate)
    w = tuple(wrap) + (0, 0)
    o.wrap_deg[0], o.wrap_deg[1] = int(bool(w[0])), int(bool(w[1]))
    o.rows = rows
    return o


def model_obs(model, z, R, landmarks, anchor, gate):
    """struct ekf_model_obs of observe_model's arguments (landmarks 0-based; the target is they or the anchor)."""
    who = "model observation"
    model = int(model)
    rows = L.EKF_MODEL_ROWS.get(model)
    if rows is None:
        raise ValueError("%s: model is one of EKF_MODEL_* (1..5)" % who)
    o = L.EkfModelObs()
    o.model = model
    zin = _vec(z)
    if not rows <= zin.size <= 2:
        raise ValueError("%s: z has one value per row of the model" % who)
    _fill(o.z, zin[:rows])
    Rf = noise(R, who, rows == 1, " (or a variance for a one-row model)")
    if Rf is not None:
        _fill(o.R, Rf)
    lms = [int(k) for k in landmarks]
    if len(lms) > 2:
        raise ValueError("%s: at most two landmarks" % who)
    o.lm[0] = o.lm[1] = -1
    _fill(o.lm, lms)
    if anchor is not None:
        if lms:
            raise ValueError("%s: the target is a landmark or an anchor, not both" % who)
        av = _vec(anchor)
        if av.size != 2:
            raise ValueError("%s: the anchor is a point (2 values)" % who)
        o.anchor[0], o.anchor[1] = av[0], av[1]
    elif not lms:
        raise ValueError("%s: name the target, a landmark or an anchor" % who)
    o.gate = float(gate)
    return o


def scan_obs(entries):
    """(ekf_model_obs[], m) of a scan [{'model', 'z', 'R', 'gate'}, ...] that is matched against the whole map: no target named
    (lm = {-1, -1}), a gate left out is +inf."""
    entries = list(entries)
    arr = (L.EkfModelObs * max(len(entries), 1))()
    for k, ent in enumerate(entries):
        arr[k] = model_obs(ent["model"], ent["z"], ent["R"], (), (0.0, 0.0), ent.get("gate", INF))
    return arr, len(entries)


def join_offset(signature_offset, who="join_map"):
    """signature_offset of join_map as the ABI takes it: one finite double."""
    v = float(signature_offset)
    if not np.isfinite(v):
        raise ValueError("%s: signature_offset is finite" % who)
    return ctypes.c_double(v)


def extract_args(indices, frame, who="extract_map"):
    """(int64[], m, frame) of extract_map as the ABI takes them: the 0-based landmarks in the caller's order and EKF_FRAME_MAP /
    EKF_FRAME_ROBOT for frame = "map" / "robot"; anything else is refused here."""
    frames = {"map": L.EKF_FRAME_MAP, "robot": L.EKF_FRAME_ROBOT}
    if not isinstance(frame, str) or frame not in frames:
        raise ValueError("%s: frame is 'map' or 'robot'" % who)
    arr, m = index_array(indices)
    return arr, m, ctypes.c_int32(frames[frame])


def transform_args(frame, t, Sigma, who="transform_map"):
    """(frame, t[3] or None, Sigma[9] column-major or None) of transform_map as the ABI takes them, the arrays kept so that the caller
    logs from what was sent.  frame "map": t = (tx, ty, phi in degrees), finite; Sigma None (an exact transform) or 3 x 3, finite,
    symmetric, with a non-negative diagonal and non-negative leading principal minors.  frame "robot": neither.  Anything else is
    refused here, before any call."""
    frames = {"map": L.EKF_FRAME_MAP, "robot": L.EKF_FRAME_ROBOT}
    if not isinstance(frame, str) or frame not in frames:
        raise ValueError("%s: frame is 'map' or 'robot'" % who)
    if frame == "robot":
        if t is not None or Sigma is not None:
            raise ValueError("%s: frame 'robot' takes neither t nor Sigma" % who)
        return ctypes.c_int32(frames[frame]), None, None
    if t is None:
        raise ValueError("%s: frame 'map' needs the transform t = (tx, ty, phi)" % who)
    tv = _vec(t)
    if tv.size != 3 or not np.all(np.isfinite(tv)):
        raise ValueError("%s: t is three finite values (tx, ty, phi in degrees)" % who)
    Sv = None
    if Sigma is not None:
        Sm = np.asarray(Sigma, dtype=np.float64)
        if Sm.size != 9 or not np.all(np.isfinite(Sm)):
            raise ValueError("%s: Sigma is 3 x 3 and finite" % who)
        Sm = Sm.reshape(3, 3)
        S = [float(v) for v in Sm.reshape(-1)]                             # the library's own expressions, row-major
        m2 = S[0] * S[4] - S[1] * S[3]
        m3 = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6])
        if not np.array_equal(Sm, Sm.T) or np.any(np.diag(Sm) < 0) or m2 < 0 or m3 < 0:
            raise ValueError("%s: Sigma is symmetric with a non-negative diagonal and non-negative leading principal minors" % who)
        Sv = np.ascontiguousarray(Sm.reshape(-1, order="F"))
    return ctypes.c_int32(frames[frame]), tv, Sv


def factor_args(ref, n, who="factor_map"):
    """(ref or None, nref, info, d2 or None) of factor_map as the ABI takes them, the arrays kept so that factor_result reads what the
    call wrote.  ref: None, one reference state of n = 3 + 2 N finite entries, or 1 to 8 of them as the rows of a 2-D array.  Anything
    else is refused here, before any call."""
    info = L.EkfFactorInfo()
    if ref is None:
        return None, ctypes.c_int32(0), info, None
    rv = np.ascontiguousarray(np.asarray(ref, dtype=np.float64))
    if rv.ndim == 1:
        rv = rv.reshape(1, -1)
    if rv.ndim != 2 or not 1 <= rv.shape[0] <= L.EKF_FACTOR_REF_MAX:
        raise ValueError("%s: ref is 1 to %d reference states, one per row" % (who, L.EKF_FACTOR_REF_MAX))
    if rv.shape[1] != n:
        raise ValueError("%s: a reference state has 3 + 2 N = %d entries, got %d" % (who, n, rv.shape[1]))
    if not np.all(np.isfinite(rv)):
        raise ValueError("%s: ref is not finite" % who)
    return rv, ctypes.c_int32(rv.shape[0]), info, np.full(rv.shape[0], np.nan)


def factor_result(args):
    """What factor_map returns from what the call wrote: the fields of ekf_factor_info by name, and 'd2' -- one entry per reference
    state, empty without any."""
    _, _, info, d2 = args
    out = dict(n=int(info.n), definite=bool(info.definite), bad_index=int(info.bad_index), bad_pivot=float(info.bad_pivot),
               logdet=float(info.logdet), logdet_map=float(info.logdet_map), min_pivot=float(info.min_pivot), max_pivot=float(info.max_pivot))
    out["d2"] = np.zeros(0) if d2 is None else d2
    return out


def sample_args(xi, n, who="sample_map", what=("xi", "draw")):
    """(xi, k, out, info) of sample_map as the ABI takes them, the arrays kept so that sample_result reads what the call wrote.  xi: one
    draw of n = 3 + 2 N finite entries, or k >= 1 of them as the rows of a 2-D array (contiguous F64 from here on).  Anything else is
    refused here, before any call.  `what`: how the messages name the array and one row of it."""
    if xi is None:
        raise ValueError("%s: %s is the %ss, one per row" % (who, what[0], what[1]))
    xv = np.ascontiguousarray(np.asarray(xi, dtype=np.float64))
    if xv.ndim == 1:
        xv = xv.reshape(1, -1)
    if xv.ndim != 2 or xv.shape[0] < 1:
        raise ValueError("%s: %s is k >= 1 %ss, one per row" % (who, what[0], what[1]))
    if xv.shape[1] != n:
        raise ValueError("%s: a %s has 3 + 2 N = %d entries, got %d" % (who, what[1], n, xv.shape[1]))
    if not np.all(np.isfinite(xv)):
        raise ValueError("%s: %s is not finite" % (who, what[0]))
    return xv, ctypes.c_int64(xv.shape[0]), np.full(xv.shape, np.nan), L.EkfFactorInfo()


def sample_result(args):
    """What sample_map returns from what the call wrote: (the samples, one per row; the dict of factor_result without 'd2')."""
    _, _, out, info = args
    res = factor_result((None, None, info, None))
    del res["d2"]
    return out, res


SOLVE_FORMS = {"full": 0, "half": 1}        # EKF_SOLVE_FULL, EKF_SOLVE_HALF


def solve_args(B, form, n, who="solve_map"):
    """(form, B, k, out, info) of solve_map as the ABI takes them, the arrays kept so that solve_result reads what the call wrote.  B as
    sample_args takes xi: one right-hand side of n = 3 + 2 N finite entries, or k >= 1 of them as rows; form is "full" or "half"."""
    if form not in SOLVE_FORMS:
        raise ValueError('%s: form is "full" (P^-1 b) or "half" (C^-1 b)' % who)
    Bv, k, out, info = sample_args(B, n, who, ("B", "right-hand side"))
    return ctypes.c_int32(SOLVE_FORMS[form]), Bv, k, out, info


def solve_result(args):
    """What solve_map returns from what the call wrote: (out, one row per right-hand side; the dict of factor_result without 'd2')."""
    return sample_result(args[1:])


def multiply_args(B, n, who="multiply_map"):
    """(B, k, out) of multiply_map as the ABI takes them, the arrays kept so that multiply_result reads what the call wrote.  B as
    sample_args takes xi: one vector of n = 3 + 2 N finite entries, or k >= 1 of them as rows."""
    Bv, k, out, _ = sample_args(B, n, who, ("B", "vector"))
    return Bv, k, out


def multiply_result(args):
    """What multiply_map returns from what the call wrote: one row P b per vector."""
    return args[2]


def dense_rows(H, n, who="observe_dense"):
    """H of observe_dense as a k x n array: a k x n array (one row of n entries: k = 1), or a list of {state index: coefficient} rows
    (0-based indices into x; an index twice in a row cannot be written, an index outside the state is refused)."""
    if isinstance(H, (list, tuple)) and len(H) > 0 and all(isinstance(r, dict) for r in H):
        Hv = np.zeros((len(H), n))
        for i, row in enumerate(H):
            for col, v in row.items():
                c = int(col)
                if c != col or not 0 <= c < n:
                    raise ValueError("%s: a state index of row %d is outside 0 .. %d" % (who, i, n - 1))
                Hv[i, c] = float(v)
        return Hv
    Hv = np.asarray(H, dtype=np.float64)
    if Hv.ndim == 1:
        Hv = Hv.reshape(1, -1)
    if Hv.ndim != 2 or Hv.shape[1] != n:
        raise ValueError("%s: H is k x %d (one row per observation row, x's order)" % (who, n))
    return np.ascontiguousarray(Hv)


def dense_args(H, z, R, n, gate=INF, wrap_deg=None, who="observe_dense"):
    """(H, k, z, R, wrap, gate, res, nu, S) of observe_dense as the ABI takes them, the arrays kept so that dense_result reads what the
    call wrote.  Refused here, in the ABI's order: k outside 1 .. EKF_DENSE_MAX; z not k values or not finite; R not k x k (a single value
    with k = 1, or k values: the diagonal), not finite, not exactly symmetric, a negative diagonal entry; a NaN gate; H not finite;
    wrap_deg not k flags."""
    Hv = dense_rows(H, n, who)
    k = Hv.shape[0]
    if not 1 <= k <= L.EKF_DENSE_MAX:
        raise ValueError("%s: between 1 and %d rows" % (who, L.EKF_DENSE_MAX))
    zv = _vec(z)
    if zv.size != k:
        raise ValueError("%s: z has one value per row of H" % who)
    if not np.isfinite(zv).all():
        raise ValueError("%s: z is not finite" % who)
    Ra = np.asarray(R, dtype=np.float64)
    if Ra.size == k and Ra.ndim < 2:
        Ra = np.diag(Ra.reshape(-1))
    if Ra.size != k * k:
        raise ValueError("%s: R is k x k (or its k diagonal entries)" % who)
    Ra = Ra.reshape(k, k)
    if not np.isfinite(Ra).all():
        raise ValueError("%s: R is not finite" % who)
    if not np.array_equal(Ra, Ra.T):
        raise ValueError("%s: R is not symmetric" % who)
    if (np.diag(Ra) < 0.0).any():
        raise ValueError("%s: R has a negative diagonal entry" % who)
    gate = float(gate)
    if gate != gate:
        raise ValueError("%s: the gate is NaN" % who)
    if not np.isfinite(Hv).all():
        raise ValueError("%s: H is not finite" % who)
    wrap = None
    if wrap_deg is not None:
        flags = [1 if w else 0 for w in wrap_deg]
        if len(flags) != k:
            raise ValueError("%s: wrap_deg has one flag per row of H" % who)
        wrap = (ctypes.c_int32 * k)(*flags)
    Rv = np.ascontiguousarray(Ra.reshape(-1, order="F"))
    return Hv, k, zv, Rv, wrap, gate, L.EkfObserveDenseResult(), np.empty(k), np.empty(k * k)


def dense_result(args):
    """What observe_dense returns from what the call wrote: 'd2', 'rows', 'outcome', 'bad_row', 'nu' (k) and 'S' (k x k)."""
    k, res, nu, S = args[1], args[6], args[7], args[8]
    return {"d2": float(res.d2), "rows": int(res.rows), "outcome": int(res.outcome), "bad_row": int(res.bad_row), "nu": nu,
            "S": S.reshape(k, k).T.copy()}


def model_inits(entries, who="append_model"):
    """(ekf_model_init[], m) of a scan of new landmarks [(model, z, R, signature), ...]."""
    entries = list(entries)
    arr = (L.EkfModelInit * max(len(entries), 1))()
    for o, ent in zip(arr, entries):
        if len(ent) != 4:
            raise ValueError("%s: an entry is (model, z, R, signature)" % who)
        model, z, R, signature = ent
        o.model = int(model)
        zin = _vec(z)
        if zin.size != 2:
            raise ValueError("%s: z has two values" % who)
        _fill(o.z, zin)
        _fill(o.R, noise(np.asarray(R, dtype=np.float64), who))      # (as an array: R is not optional here)
        o.signature = float(signature)
    return arr, len(entries)


def motions(steps, known_models=False):
    """(ekf_motion[], m) of a chain of motion steps [(model, u, M), ...]: u and M of the size the model reads, M column-major in the
    3 x 3 slot.  A model without an entry in EKF_MOTION_INPUTS is refused here where known_models is set, else left to the library."""
    who = "predict_model"
    steps = list(steps)
    arr = (L.EkfMotion * max(len(steps), 1))()
    for o, st in zip(arr, steps):
        if len(st) != 3:
            raise ValueError("%s: a step is (model, u, M)" % who)
        model, u, M = st
        o.model = int(model)
        if known_models and o.model not in L.EKF_MOTION_INPUTS:
            raise ValueError("%s: model is EKF_MOTION_TURN_DRIVE (1), EKF_MOTION_ARC (2) or EKF_MOTION_POSE_DELTA (3)" % who)
        nu = L.EKF_MOTION_INPUTS.get(o.model, 3)
        uin = _vec(u)
        if uin.size != nu:
            raise ValueError("%s: u has %d values for this model" % (who, nu))
        _fill(o.u, uin)
        Ma = np.asarray(M, dtype=np.float64)
        if Ma.size != nu * nu:
            raise ValueError("%s: M is %d x %d for this model" % (who, nu, nu))
        full = np.zeros((3, 3))
        full[:nu, :nu] = Ma.reshape(nu, nu)
        _fill(o.M, full.reshape(-1, order="F"))
    return arr, len(steps)


# ---- the results ----
def linear_result(res):
    return {"nu": np.array(res.nu[:]), "S": np.array(res.S[:]).reshape(2, 2, order="F"), "d2": float(res.d2),
            "outcome": int(res.outcome)}


def iterated_result(first, it):
    out = linear_result(first)
    out["iterated"] = {"S": np.array(it.S[:]).reshape(2, 2, order="F"), "nu": np.array(it.nu[:]), "used": int(it.used),
                       "converged": bool(it.converged), "last_step": float(it.last_step), "x_local": np.array(it.x_local[:])}
    return out


def joint_result(res, m, nu=None, S=None):
    """One struct ekf_joint_result as a dict, with 'nu' (2m) and 'S' (2m x 2m, from the column-major buffer) by scan index where given."""
    out = {"d2": float(res.d2), "dof": int(res.dof), "pairings": int(res.pairings), "outcome": int(res.outcome),
           "first_irregular": int(res.first_irregular)}
    if nu is not None:
        out["nu"] = nu
    if S is not None:
        out["S"] = S.reshape(2 * m, 2 * m).T.copy()
    return out


def joint_iter_result(it):
    """One struct ekf_joint_iter_result as a dict: 'used', 'converged', 'step', 'd2_last', 'irregular_at', 'irregular_obs' and 'x_sub' (ns)."""
    return {"used": int(it.used), "converged": bool(it.converged), "step": float(it.last_step), "d2_last": float(it.d2_last),
            "irregular_at": int(it.irregular_at), "irregular_obs": int(it.irregular_obs), "x_sub": np.array(it.x_sub[:int(it.ns)])}


MATCH_KEYS = (("best", np.int64), ("second", np.int64), ("d2_best", np.float64), ("d2_second", np.float64), ("within_gate", np.int64),
              ("irregular", np.int64))


def match_result(match, m):
    """m structs ekf_model_match as {'best', 'second', 'd2_best', 'd2_second', 'within_gate', 'irregular'}, one array entry each."""
    return {key: np.array([getattr(match[k], key) for k in range(m)], dtype=dt) for key, dt in MATCH_KEYS}


def assigned_result(out, match, m, total, cand=None, cand_d2=None):
    """What ekf_assign_model returned, as arrays with one entry per observation (landmarks 0-based, -1 = left out or none): 'landmark',
    'd2', 'ncand', the six keys of match_result, the float 'total', and the m x EKF_ASSIGN_CANDIDATES 'cand' / 'cand_d2' where given."""
    res = {"landmark": np.array([out[k].landmark for k in range(m)], dtype=np.int64), "d2": np.array([out[k].d2 for k in range(m)], dtype=np.float64),
           "ncand": np.array([out[k].ncand for k in range(m)], dtype=np.int64), "total": float(total)}
    res.update(match_result(match, m))
    if cand is not None:
        res["cand"], res["cand_d2"] = cand, cand_d2
    return res


def joint_search_thresholds(thresholds, m):
    """The 2m + 1 thresholds of ekf_joint_search, by dof, as one contiguous float64 array."""
    thr = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float64).reshape(-1))
    if thr.size != 2 * m + 1:
        raise ValueError("joint_search: thresholds has 2 m + 1 entries, one per dof 0 .. 2 m")
    return thr


def joint_search_result(res, match, m, cand=None, cand_d2=None, alive_hyp=None, alive_d2=None):
    """What ekf_joint_search returned: the winner's 'landmark' (m, 0-based, -1 = left out), 'd2', 'dof', 'pairings', 'truncated' (bool),
    'nalive', 'irregular' (extensions without a d2), 'tested' / 'survived' (m, by scan index), the keys of match_result -- its per-entry
    count of landmarks without a d2 as 'match_irregular' -- and where given 'cand' / 'cand_d2' (m x EKF_ASSIGN_CANDIDATES) and 'alive'
    (nalive x m) / 'alive_d2' (nalive): the final beam in order."""
    out = {"landmark": np.array(res.lm[:m], dtype=np.int64), "d2": float(res.d2), "dof": int(res.dof), "pairings": int(res.pairings),
           "truncated": bool(res.truncated), "nalive": int(res.nalive), "irregular": int(res.irregular),
           "tested": np.array(res.tested[:m], dtype=np.int64), "survived": np.array(res.survived[:m], dtype=np.int64)}
    out.update({("match_irregular" if key == "irregular" else key): val for key, val in match_result(match, m).items()})
    if cand is not None:
        out["cand"], out["cand_d2"] = cand, cand_d2
    if alive_hyp is not None:
        out["alive"], out["alive_d2"] = alive_hyp[:out["nalive"]].copy(), alive_d2[:out["nalive"]].copy()
    return out


def assigned_scan_result(out, res, m, total):
    """What ekf_assigned_scan_result reported of a scan, as arrays with one entry per observation: the assignment's 'landmark' (0-based, -1 =
    left out), 'd2', 'ncand' and the float 'total'; each step's 'nu' (m x 2), 'S' (m x 2 x 2), 'outcome' and 'step_d2'."""
    steps = [linear_result(res[k]) for k in range(m)]
    return {"landmark": np.array([out[k].landmark for k in range(m)], dtype=np.int64), "d2": np.array([out[k].d2 for k in range(m)], dtype=np.float64),
            "ncand": np.array([out[k].ncand for k in range(m)], dtype=np.int64), "total": float(total),
            "nu": np.array([s["nu"] for s in steps]).reshape(m, 2), "S": np.array([s["S"] for s in steps]).reshape(m, 2, 2),
            "outcome": np.array([s["outcome"] for s in steps], dtype=np.int64), "step_d2": np.array([s["d2"] for s in steps], dtype=np.float64)}


# ---- the library's pure host functions ----
def host_call(name, lib, *args):
    """One of the functions that take no handle (the kernels' own text, compiled for the host): `lib` None is the loaded library; a
    status raises EkfError(status, name)."""
    rc = getattr(L.lib() if lib is None else lib, name)(*args)
    if rc:
        raise L.EkfError(rc, name)
