"""Pure-NumPy side of tests/test_beside_pass_gpu.py: a precomputed plan that mixes every update-step family, the model appends, the motion
chains, the read-only queries and the map edits around batch boundaries, and three interpreters of it -- an engine (or a group of shards),
the factored oracle (oracle/ekf_factored.py, through its generic steps) and one dense P (the dense forms of the *_cases.py files).  No
model is restated here: Jacobians, inverses and motions come from model_obs_cases, linear_obs_cases, append_model_cases,
predict_model_cases and model_iter_cases.  No GPU is touched when this module is imported.

The plan is a pure function of its arguments.  Every z is h(nominal state) plus drawn noise, the nominal state being the loaded x moved by
the planned motions (landmarks appended on the way sit where their z puts them from the nominal pose); nothing is read from an engine.

A plan is a list of steps; a step is a list of operations (kind, payload, tested), the last of them the one that takes the step's pair
slot.  `tested` marks the calls of steps 1-4 behind a batch boundary other than the first: those are issued while the boundary's
asynchronous pass runs."""
import numpy as np

import append_model_cases as A
import linear_obs_cases as C
import model_iter_cases as I
import model_obs_cases as M
import predict_model_cases as Pm

ITERATIONS = 3
A_MAX = 32                       # EKF_APPEND_MODEL_MAX
PAIR_KINDS = ("correct", "observe_linear", "observe_model", "observe_model_iterated")
QUERY_KINDS = ("associate_model", "joint_innovation", "model_innovation", "linear_innovation")
EDIT_KINDS = ("remove_landmarks", "merge_landmarks", "merge_landmarks_batch")
SHARDED_KINDS = ("predict", "predict_model", "append_model", "correct", "associate_model")
RPOS = np.array([[0.02, 0.005], [0.005, 0.03]])
R_MODEL = {M.RANGE_BEARING: np.diag([0.01, 0.25]), M.RANGE: 0.01, M.BEARING: 0.25, M.RELATIVE_XY: 0.01 * np.eye(2), M.LANDMARK_RANGE: 0.01}
SIGMA_Z = {M.RANGE_BEARING: (0.02, 0.2), M.RANGE: (0.02,), M.BEARING: (0.2,), M.RELATIVE_XY: (0.02, 0.02), M.LANDMARK_RANGE: (0.02,)}


class Nominal:
    """The state the plan's z are taken from: the pose moved by the planned motions, the landmarks where they were loaded or appended."""

    def __init__(self, x0):
        x0 = np.asarray(x0, dtype=np.float64)
        self.pose = x0[:3].copy()
        self.lm = [p.copy() for p in x0[3:].reshape(-1, 2)]
        self.ids = list(range(len(self.lm)))          # (the edits renumber: a landmark keeps its id)
        self.next_id = len(self.lm)

    @property
    def N(self):
        return len(self.lm)

    def x(self):
        return np.concatenate([self.pose] + self.lm)

    def predict(self, u):
        th = self.pose[2] + u[1]
        self.pose = np.array([self.pose[0] + u[0] * np.cos(np.radians(th)), self.pose[1] + u[0] * np.sin(np.radians(th)), Pm.wrap360(th)])

    def predict_model(self, chain):
        for model, u, _ in chain:
            p = Pm.f_of(model, self.pose, u)
            self.pose = np.array([p[0], p[1], Pm.wrap360(p[2])])

    def append(self, pos):
        self.lm.append(np.asarray(pos, dtype=np.float64).copy())
        self.ids.append(self.next_id)
        self.next_id += 1
        return self.ids[-1]

    def remove(self, indices):
        for k in sorted(indices, reverse=True):
            del self.lm[k], self.ids[k]


def model_obs(nom, rng, model, landmarks=(), anchor=None, R_scale=1.0):
    """One model observation of the nominal state with drawn noise."""
    o = M.obs(model, [0.0, 0.0], np.asarray(R_MODEL[model]) * R_scale, landmarks, anchor)
    hx = M.jacobian(nom.x(), o)[0]
    o["z"][:o["rows"]] = hx[:o["rows"]] + rng.normal(0.0, SIGMA_Z[model])
    return o


def scan_entry(nom, rng, k, model, R_scale=1.0):
    """An associate / joint entry that sights landmark k of the nominal state through a one-landmark model."""
    o = model_obs(nom, rng, model, [k], R_scale=R_scale)
    return dict(model=model, z=o["z"].copy(), R=o["R"].copy())


def append_scan(nom, rng, m, first_signature, duplicates=(), A_scale=1.0, reach=40.0):
    """m append_model entries, the two models alternating, 5-40 away from the nominal pose; `duplicates` (landmark indices) are sighted
    again instead: those entries start a second landmark where one already is."""
    out, ids = [], []
    for b in range(m):
        model = A.RANGE_BEARING if b % 2 == 0 else A.RELATIVE_XY
        R = RPOS * A_scale * (1.0 + 0.1 * b)
        if b < len(duplicates):
            d = nom.lm[duplicates[b]] - nom.pose[:2]
        else:
            r, a = rng.uniform(5.0, reach), rng.uniform(0.0, 2.0 * np.pi)
            d = r * np.array([np.cos(a), np.sin(a)])
        th = np.radians(nom.pose[2])
        if model == A.RANGE_BEARING:
            z = np.array([np.hypot(d[0], d[1]), np.degrees(np.arctan2(d[1], d[0])) - nom.pose[2]]) + rng.normal(0.0, (0.02, 0.2))
            R = R * np.array([[1.0, 3.0], [3.0, 10.0]])
        else:
            z = np.array([np.cos(th) * d[0] + np.sin(th) * d[1], -np.sin(th) * d[0] + np.cos(th) * d[1]]) + rng.normal(0.0, 0.02, 2)
        out.append(A.entry(model, z, R, first_signature + b))
        ids.append(nom.append(A.g_of(model, nom.pose, z)))
    return out, ids


def motion_chain(rng, length, first_model):
    """1-3 predict_model steps, the three models in turn from first_model."""
    out = []
    for q in range(length):
        model = 1 + (first_model + q) % 3
        a = rng.uniform(-1.0, 1.0, (3, 3))
        Mn = (a @ a.T + 0.5 * np.eye(3)) * np.outer([0.01, 0.01, 0.3], [0.01, 0.01, 0.3])
        if model == Pm.TURN_DRIVE:
            out.append(Pm.step(model, [0.1 + 0.02 * rng.random(), 3.0 + rng.normal(0.0, 0.1)], Mn[np.ix_([0, 2], [0, 2])]))
        elif model == Pm.ARC:
            out.append(Pm.step(model, [0.12 + 0.02 * rng.random(), 4.0 + rng.normal(0.0, 0.1)], Mn[np.ix_([0, 2], [0, 2])]))
        else:
            out.append(Pm.step(model, [0.08, 0.02 * rng.normal(), -2.0 + rng.normal(0.0, 0.1)], Mn))
    return out


def _bearing_ok(nom, k):
    d = nom.lm[k] - nom.pose[:2]
    b = (np.degrees(np.arctan2(d[1], d[0])) - nom.pose[2]) % 360.0
    return 30.0 <= b <= 330.0 and d @ d > 4.0


def make_plan(x0, T, batch, batches, RC, seed=11, sharded=False, edits=False, R_scale=1.0, A_scale=1.0, reach=40.0, turn=3.0, fix_scale=1.0, edge_back=(0, 1, 2)):
    """(steps, info): `batches` full batches and four more steps.  R_scale: a factor on the R of every linear and model observation,
    fix_scale: one more on the position and heading fixes; A_scale: a factor on the R of an appended landmark's sighting; reach: how far from
    the robot landmarks are appended; turn: degrees per plain predict; edge_back: the tile-row-edge target is the first landmark of the
    tile row that many rows before the last, the three in turn.  info: 'appended' (0-based index, at the end of the plan, of every
    landmark append_model added; None after edits), 'crossing_scans' (tested scans that carry the map over a tile-row edge), 'N' at the end."""
    rng = np.random.default_rng(seed)
    nom = Nominal(x0)
    half = T // 2
    nsteps = batches * batch + 4
    nfill = -(-half // A_MAX)
    stride = max(1, (batch - 6) // nfill)
    fill_at = [5 + q * stride for q in range(nfill)]
    assert fill_at[-1] < batch and batch % 4 == 0
    count = dict(lin=0, mod=0, it=0, scan=0, chain=0, lr=0)
    steps, appended_ids, crossing = [], [], 0
    dup_ids = []
    signature = 1.0e6

    def far_apart(c):
        """two landmarks in different tile rows, the order alternating"""
        a, b = (c * 997 + 13) % nom.N, (c * 613 + 5 * half + 1) % nom.N
        if a // half == b // half:
            b = (b + half) % nom.N
        if a // half == b // half:                    # (a map of one tile row)
            b = (a + 1) % nom.N
        return (a, b) if c % 2 == 0 else (b, a)

    def target(c):
        """the first landmark, the last one, the first of a tile row, an anchor"""
        which = c % 4
        if which == 0:
            return [0], None
        if which == 1:
            return [nom.N - 1], None
        if which == 2:
            return [max(0, (nom.N - 1) // half - edge_back[(c // 4) % 3]) * half], None
        return (), nom.pose[:2] + np.array([12.0 + c % 7, -9.0 + c % 5])

    def model_step(c):
        model = 1 + c % 5
        if model == M.LANDMARK_RANGE:
            count["lr"] += 1
            return model_obs(nom, rng, model, list(far_apart(count["lr"])), R_scale=R_scale)
        lms, anchor = target(c // 5 + c % 5)
        return model_obs(nom, rng, model, lms, anchor, R_scale=R_scale)

    def linear_step(c):
        which = c % 4
        if which == 0:
            k = (c * 331 + 7) % nom.N
            return C.landmark_fix(k, nom.lm[k] + rng.normal(0.0, 0.02, 2), RPOS * R_scale)
        if which == 1:
            return C.position_fix(nom.pose[:2] + rng.normal(0.0, 0.02, 2), RPOS * R_scale * fix_scale)
        if which == 2:
            return C.heading_fix(nom.pose[2] + rng.normal(0.0, 0.1), 0.05 * R_scale * fix_scale)
        i, j = far_apart(c + 3)
        if (c // 4) % 2:
            o = C.general(rng, i, j, nom.x(), scale=0.05, R=np.array([[0.3, 0.05], [0.05, 0.2]]) * R_scale)
            o["Hr"][:, 2] = 0.0                       # (no heading: the filter's and the nominal one may sit on either side of 360)
            o["z"] = C.jacobian(nom.x().size, o) @ nom.x() + 0.05 * rng.standard_normal(2)
            return o
        return C.relative(i, j, nom.lm[i] - nom.lm[j] + rng.normal(0.0, 0.02, 2), RPOS * R_scale)

    for t in range(nsteps):
        p, k_b = (t + 1) % batch, (t + 1) // batch
        tested = 1 <= p <= 4 and k_b >= 2
        ops = []
        # the motion in front of the step
        if (tested and (p + k_b) % 2 == 1) or (not tested and t % 5 == 3):
            chain = motion_chain(rng, 1 + count["chain"] % 3, count["chain"])
            count["chain"] += 1
            nom.predict_model(chain)
            ops.append(("predict_model", chain, tested))
        else:
            u = np.array([0.1 + rng.normal(0.0, 0.005), turn + rng.normal(0.0, 0.1)])
            nom.predict(u)
            ops.append(("predict", u, tested))
        # the map edits, once each, behind boundaries 3, 4 and 5
        if edits and tested and p == 1 and k_b in (3, 4, 5):
            if k_b == 3:
                gone = sorted({(5 * half + 3) % nom.N, (2 * half + 1) % nom.N, nom.N - 7 - 2 * half})
                assert len({g // half for g in gone}) == 3 and not {nom.ids[g] for g in gone} & {i for pr in dup_ids for i in pr}
                ops.append(("remove_landmarks", gone, tested))
                nom.remove(gone)
            elif k_b == 4:
                keep_id, drop_id = dup_ids.pop(0)
                keep, drop = nom.ids.index(keep_id), nom.ids.index(drop_id)
                ops.append(("merge_landmarks", (keep, drop, RPOS), tested))
                nom.remove([drop])
            else:
                pairs = [(nom.ids.index(a), nom.ids.index(b)) for a, b in dup_ids[:4]]
                del dup_ids[:4]
                ops.append(("merge_landmarks_batch", (pairs, RPOS), tested))
                nom.remove([b for _, b in pairs])
        # the appends: a tested scan of 3-6 entries 2 steps behind the boundary, carried over the next tile-row edge by the filler scans
        # of the batch before it
        m_next = 3 + count["scan"] % 4
        if tested and p == 2:
            before = nom.N
            dups = []
            if edits and k_b == 2:                    # five second sightings for the merges to fuse
                dups = [(q * 2 * half + 17) % nom.N for q in range(1, 6)]
            m = 5 if dups else m_next
            entries, ids = append_scan(nom, rng, m, signature, dups, A_scale, reach)
            dup_ids += [(nom.ids[k], i) for k, i in zip(dups, ids)]
            signature += m
            count["scan"] += 1
            appended_ids += ids
            crossing += (before - 1) // half != (nom.N - 1) // half and before % half != 0
            ops.append(("append_model", entries, tested))
        elif not tested and p in fill_at and k_b >= 1:
            lead = 1 + (m_next - 1) // 2              # landmarks of the tested scan that stay in front of the edge
            want = min(A_MAX, (-(nom.N + lead)) % half)
            if want and (k_b + 1) * batch + 1 < nsteps:
                entries, ids = append_scan(nom, rng, want, signature, A_scale=A_scale, reach=reach)
                signature += want
                appended_ids += ids
                ops.append(("append_model", entries, tested))
        # The boundary's own step first waits for the main stream (a query): the host runs ahead of the gathers within a batch, and
        # the pass starts only where the main stream reaches the boundary; so drained, it starts when the boundary's step is issued, and
        # the calls behind it wait for their own kernels alone
        if p == 0 and k_b >= 2:
            if sharded:
                ops.append(("associate_model", [dict(scan_entry(nom, rng, (k_b * 31) % nom.N, M.RANGE_BEARING), gate=9.0)], False))
            else:
                ops.append(("model_innovation", model_step(k_b), False))
        # the read-only queries, one per tested step, each kind in every place behind a boundary in turn
        if tested and not (sharded and p != 1):
            kind = QUERY_KINDS[0] if sharded else QUERY_KINDS[(p - 1 + k_b) % 4]
            if kind == "associate_model":
                ks = [0, nom.N - 1, (nom.N // 2 // half) * half, (k_b * 977) % nom.N]
                ops.append((kind, [dict(scan_entry(nom, rng, k, 1 + q % 4), gate=9.0 + q) for q, k in enumerate(ks)], tested))
            elif kind == "joint_innovation":
                ks = [(q * (2 * half + 1) * 3 + k_b) % nom.N for q in range(8)]
                entries = [scan_entry(nom, rng, k, 1 + q % 4) for q, k in enumerate(ks)]
                hyp = np.array([ks, ks, ks, ks])
                hyp[1, 2] = -1
                hyp[2, 5], hyp[2, 0] = (ks[5] + 1) % nom.N, -1      # one wrong pairing: the neighbour
                hyp[3, ::2] = -1
                ops.append((kind, (entries, hyp), tested))
            elif kind == "model_innovation":
                ops.append((kind, model_step(k_b + 2), tested))
            else:
                ops.append((kind, linear_step(k_b), tested))
        # the step's pair
        kind = "correct" if sharded else PAIR_KINDS[(t + k_b) % 4]
        if kind == "correct":
            k = (t * 37 + 11) % nom.N
            while not _bearing_ok(nom, k):
                k = (k + 101) % nom.N
            d = nom.lm[k] - nom.pose[:2]
            z = np.array([np.hypot(d[0], d[1]) + rng.normal(0.0, 0.02),
                          (np.degrees(np.arctan2(d[1], d[0])) - nom.pose[2]) % 360.0 + rng.normal(0.0, 0.5)])
            ops.append((kind, (z, np.diag([z[0] * RC[0], z[1] * RC[1]]), k), tested))
        elif kind == "observe_linear":
            ops.append((kind, linear_step(count["lin"]), tested))
            count["lin"] += 1
        elif kind == "observe_model":
            ops.append((kind, model_step(count["mod"]), tested))
            count["mod"] += 1
        else:
            ops.append((kind, model_step(count["it"] + 2), tested))
            count["it"] += 1
        steps.append(ops)
    appended = None if edits else [nom.ids.index(i) for i in appended_ids]
    return steps, dict(appended=appended, crossing_scans=int(crossing), N=nom.N)


def appended_total(steps):
    return sum(len(payload) for ops in steps for kind, payload, _ in ops if kind == "append_model")


# ------------------------------------------------------------------------------------------------------------------
# the interpreters
# ------------------------------------------------------------------------------------------------------------------
def _model_kw(o):
    return {k: v for k, v in o.items() if k != "rows"}


def issue(eng, kind, payload):
    """One operation on an engine or a group of shards; a query's result, else None."""
    if kind == "predict":
        return eng.predict(payload)
    if kind == "predict_model":
        return eng.predict_model(payload)
    if kind == "append_model":
        eng.append_model(payload)
        return None
    if kind == "correct":
        return eng.correct(*payload)
    if kind == "observe_linear":
        return eng.observe_linear(**payload)
    if kind == "observe_model":
        return eng.observe_model(**_model_kw(payload))
    if kind == "observe_model_iterated":
        return eng.observe_model_iterated(iterations=ITERATIONS, **_model_kw(payload))
    if kind == "associate_model":
        return eng.associate_model(payload, want_d2=True)
    if kind == "joint_innovation":
        return eng.joint_innovation(payload[0], payload[1], want_prefix=True, want_nu=True, want_S=True)
    if kind == "model_innovation":
        return eng.model_innovation(**_model_kw(payload))
    if kind == "linear_innovation":
        return eng.linear_innovation(**payload)
    if kind == "remove_landmarks":
        return eng.remove_landmarks(payload)
    if kind == "merge_landmarks":
        return eng.merge_landmarks(*payload)
    if kind == "merge_landmarks_batch":
        return eng.merge_landmarks_batch(*payload)
    raise ValueError(kind)


def _blocks(H, rows, landmarks):
    return H[:rows, :3], [H[:rows, 3 + 2 * k:5 + 2 * k] for k in landmarks]


def apply_factored(ref, kind, payload):
    """One operation on the factored oracle, through its generic steps (queries change nothing and are skipped)."""
    if kind == "predict":
        ref.predict(payload)
    elif kind == "predict_model":
        for model, u, Mn in payload:
            F, V = Pm.F_V_of(model, ref.x[:3], u)
            pose = Pm.f_of(model, ref.x[:3], u)
            ref.predict_affine(F, V @ Mn @ V.T, [pose[0], pose[1], Pm.wrap360(pose[2])])
    elif kind == "append_model":
        xr = ref.x[:3].copy()
        for model, z, R, signature in payload:
            Gx, Gz = A.G_of(model, xr, z)
            ref.append_jacobian(Gx, Gz, R, A.g_of(model, xr, z), signature)
    elif kind == "correct":
        z, R, k = payload
        ref.correct(z, R, k + 1)
    elif kind == "observe_linear":
        o = payload
        H = C.jacobian(ref.x.size, o)
        r = o["rows"]
        Hr, Hl = _blocks(H, r, o["landmarks"])
        ref.update_linear(Hr, o["landmarks"], Hl, C.innovation(ref.x, o, H)[:r], C.effective(o)[1][:r, :r])
    elif kind == "observe_model":
        o = payload
        hx, H = M.jacobian(ref.x, o)
        r = o["rows"]
        nu = o["z"] - hx
        for q in range(r):
            if M.WRAP[o["model"]][q]:
                nu[q] = M.wrap180(nu[q])
        Hr, Hl = _blocks(H, r, o["landmarks"])
        ref.update_linear(Hr, o["landmarks"], Hl, nu[:r], M.effective_R(o)[:r, :r])
    elif kind == "observe_model_iterated":
        # Gauss-Newton on the sub-state of the robot and the targets, read from the oracle's rows; the LAST linearisation's pair then
        # updates the whole state, as the kernel does
        o = payload
        loc = I.local_rows(o)
        Ps = np.vstack([ref.P_rows(0, 3)[:, loc]] + [ref.P_rows(3 + 2 * k, 2)[:, loc] for k in o["landmarks"]])
        sub = dict(o, landmarks=list(range(len(o["landmarks"]))))
        _, _, first, it = I.iterate_dense(ref.x[loc], Ps, sub, ITERATIONS)
        assert first["outcome"] == I.APPLIED and it["used"] == ITERATIONS
        r = o["rows"]
        Hr, Hl = _blocks(it["H"], r, sub["landmarks"])
        ref.update_linear(Hr, o["landmarks"], Hl, it["nu"][:r], M.effective_R(o)[:r, :r])
    elif kind not in QUERY_KINDS:
        raise ValueError(kind)


def apply_dense(dense, kind, payload):
    """One operation on a dense state (an oracle.ekf_dense.EKF_SLAM: x, P, s), by the dense forms of the *_cases.py files."""
    if kind == "predict":
        dense.predict(payload)
    elif kind == "predict_model":
        dense.x, dense.P, _ = Pm.predict_model_dense(dense.x, dense.P, payload)
    elif kind == "append_model":
        x, s, P = A.append_model_dense(dense.x, dense.s, dense.P, payload)
        dense.x, dense.s, dense.P = x, list(s), P
    elif kind == "correct":
        z, R, k = payload
        dense._correct(z, R, k + 1)
    elif kind == "observe_linear":
        dense.x, dense.P, res = C.observe_dense(dense.x, dense.P, payload)
        assert res["outcome"] == C.APPLIED
    elif kind == "observe_model":
        dense.x, dense.P, res = M.observe_model_dense(dense.x, dense.P, payload)
        assert res["outcome"] == M.APPLIED
    elif kind == "observe_model_iterated":
        dense.x, dense.P, first, _ = I.iterate_dense(dense.x, dense.P, payload, ITERATIONS)
        assert first["outcome"] == I.APPLIED
    elif kind not in QUERY_KINDS:
        raise ValueError(kind)


def kinds_of(steps, tested_only=False):
    out = {}
    for ops in steps:
        for kind, _, tested in ops:
            if tested or not tested_only:
                out[kind] = out.get(kind, 0) + 1
    return out


def appended_row_margin(rows, appended, N_at_append, T, tol_abs):
    """smallest over the appended landmarks' rows (rows[q]: 2 x n of landmark appended[q]) and over every tile column range of the map as it
    was at that landmark's append of (largest entry in those columns) / tol_abs: what a lost row copy would zero"""
    worst = np.inf
    for q, L in enumerate(appended):
        m = 2 * N_at_append[q]
        a = np.abs(rows[q][:, 3:3 + m])
        for J in range(-(-m // T)):
            worst = min(worst, float(a[:, J * T:min(m, (J + 1) * T)].max()) / tol_abs)
    return worst


# ------------------------------------------------------------------------------------------------------------------
# the legs at size and what the oracle alone says about them
# ------------------------------------------------------------------------------------------------------------------
# leg: storage, tile edge, batch, batches of the plan, the pass kernel the batch selects, shards (0: a plain engine), the key of
# async_cases.INPUTS.  Float tiles run 6 batches of 32 (196 steps), F64 ones 8 batches of 8 (68 steps).
LEGS = {
    "a_f64": ("f64", 128, 8, 8, "k_flush_mfma<double,128,", 0, "f64"),
    "b_f32_mixed": ("f32_mixed", 256, 32, 6, "k_flush_mfma32<256,", 0, "float"),
    "c_f32_split": ("f32_split", 256, 32, 6, "k_flush_split3<2>", 0, "float"),
    "d_f64_two_shards": ("f64", 128, 8, 8, "k_flush_mfma<double,128,", 2, "f64"),
}
EDITS_LEG = ("f64", 128, 8, 8, "k_flush_mfma<double,128,", 0, "f64")
# The plan's inputs by storage kind (make_plan's keywords).  Float tiles: the bars of tests/test_async_growth_gpu.py were fitted to weak
# corrections, and as there the inputs change, not the bars.  With the F64 inputs the SYNCHRONOUS float engine alone misses them (rows
# 1.2e-6 against 2e-7, entries kept in F64 5e-8 against 3e-9).  The landmarks of one scan share the robot's uncertainty, so with a small
# noise of their own their cross blocks are as large as any entry of P; a sharp observation of one of them then has K near 1 for its
# neighbours, which carries the float rounding of those cross blocks (6e-8 of them) straight into the robot strip and the diagonal blocks,
# and takes most of the shared part out in one pair, of which a pass of 32 pairs in F32 arithmetic loses ~sqrt(64) * 6e-8.  Hence
#   * A_scale: the noise of an appended landmark's own sighting 50-70 times larger, so that its own block (kept in F64) sets the scale of
#     the rows, as the bearing factor does in async_growth, and the cross blocks are a fraction of it;
#   * R_scale: R of the linear and model observations 100 times larger (range 1 m^2, bearing 25 deg^2: what the corrections have), so K
#     stays a fraction too -- which also keeps the robot uncertain and its strip near 1, the measure of that bar;
#   * edge_back: the tile-row-edge target among the loaded landmarks (40, 80, 120 tile rows before the last) instead of the first
#     landmark of the newest rows, which as a target every few steps is a sharp observation of the same fresh scan again and again.
# Measured on an MI355X, synchronous engine, each change alone leaves a bar missed: see tests/test_beside_pass_gpu.py.  The margins left
# (rows 1.3e-7 of 2e-7, strip 2e-9 of 3.2e-9, sensitivity 31 of 20) are why the mixed leg has 70 and the split leg 50.
PLAN_INPUTS = {"f64": {},
               "f32_mixed": dict(R_scale=100.0, A_scale=70.0, edge_back=(40, 80, 120)),
               "f32_split": dict(R_scale=100.0, A_scale=50.0, edge_back=(40, 80, 120))}


def tolerances(storage, nsteps):
    """(x, entries kept in F64, rows): tests/test_async_growth_gpu.py's bars"""
    if storage == "f64":
        return 1e-6, 1e-6, 1e-6
    return 1e-9 + 2e-12 * nsteps, 2e-9 + 6e-12 * nsteps, 2e-7


def leg_inputs(leg, N0):
    """((x, s, d, U), steps, info) of a leg on a map of N0 landmarks: the state of async_cases.make_inputs and the plan"""
    import async_cases
    storage, T, batch, batches, _, shards, key = LEGS[leg] if isinstance(leg, str) else leg
    sigma, sigma_robot, RC = async_cases.INPUTS[key]
    state, _ = async_cases.make_inputs(N0, 0, sigma, sigma_robot, RC)
    steps, info = make_plan(state[0], T, batch, batches, RC, sharded=bool(shards), **PLAN_INPUTS[storage])
    return state, steps, info


def run_oracle(ref, steps, batch, T):
    """The plan on the factored oracle.  Returns the sampled rows (async_cases.sampled_landmarks) at the last batch boundary and two
    boundaries before it -- what a tile that one pass skipped lacks -- as [(N, landmarks, rows), (N, landmarks, rows)]."""
    import async_cases
    nb = len(steps) // batch
    snap_at = [(nb - 2) * batch - 1, nb * batch - 1]
    snaps = []
    for t, ops in enumerate(steps):
        for kind, payload, _ in ops:
            apply_factored(ref, kind, payload)
        if t in snap_at:
            lms = snaps[0][1] if snaps else async_cases.sampled_landmarks(ref.N, T)
            snaps.append((ref.N, lms, async_cases.oracle_rows(ref, lms)))
    return snaps


def sensitivity(ref, snaps, appended, T, tol_rows):
    """(scale, margin of the sampled rows over two batches, margin of the appended rows, the appended rows): both margins in units of the
    row tolerance tol_rows * scale, scale the largest entry of the sampled rows at the end"""
    import async_cases
    lms = async_cases.sampled_landmarks(ref.N, T)
    scale = float(np.abs(async_cases.oracle_rows(ref, lms)).max())
    (N_b, lms_b, before), (_, _, after) = snaps
    moved = async_cases.tile_change_margin(before, after, lms_b, N_b, T, np.full(len(lms_b), tol_rows * scale))
    rows_app = async_cases.oracle_rows(ref, appended)
    return scale, moved, appended_row_margin(rows_app, appended, appended, T, tol_rows * scale), rows_app
