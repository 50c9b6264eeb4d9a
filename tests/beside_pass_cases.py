"""Pure-NumPy side of tests/test_beside_pass_gpu.py: a precomputed plan that mixes every update-step family, the model appends, the motion
chains, the read-only queries and the map edits around batch boundaries, and three interpreters of it -- an engine (or a group of shards),
the factored oracle (oracle/ekf_factored.py, through its generic steps) and one dense P (the dense forms of the *_cases.py files).  No
model is restated here: Jacobians, inverses and motions come from model_obs_cases, linear_obs_cases, append_model_cases,
predict_model_cases and model_iter_cases.  No GPU is touched when this module is imported.

The plan is a pure function of its arguments.  Every z is h(nominal state) plus drawn noise, the nominal state being the loaded x moved by
the planned motions (landmarks appended on the way sit where their z puts them from the nominal pose); nothing is read from an engine.

A plan is a list of steps; a step is a list of operations (kind, payload, tested), the last of them the one that takes the step's pair
slot.  `tested` marks the calls of steps 1-4 behind a batch boundary other than the first: those are issued while the boundary's
asynchronous pass runs.

make_plan(newer=True) is the plan of tests/test_beside_pass_newer_gpu.py: the same steps, and behind the boundaries the calls added since
-- the synchronising ones (SYNC_KINDS: joint updates, join / extract / transform / factor_map), observe_model_assigned as one more pair
kind, assign_model and joint_search as two more queries -- interpreted by `issue` and, through the dense forms of their own *_cases.py files,
by `apply_dense`.  `Nominal` follows them: a transform moves its pose and landmarks, a join appends the local landmarks, an extraction
leaves it alone."""
import hashlib

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
# make_plan(newer=True): the calls added since.  SYNC_KINDS retire the pass in flight; the others leave it alone.
SYNC_KINDS = ("observe_model_joint", "observe_model_joint_iterated", "join_map", "extract_map", "transform_map", "factor_map")
NEWER_QUERY_KINDS = ("assign_model", "joint_search")
NEWER_PAIR_KIND = "observe_model_assigned"
JOINT_GATE = 200.0               # finite, and far beyond a d2 of ~10 degrees of freedom made of the drawn noise alone
# An assigned entry sights a landmark whose nearest neighbour is ~2.3-3 m away (isolated_landmarks), up to 25 m from a robot whose heading
# is known to ~2 degrees (1 m across at that range): the neighbour's d2 is 9 or more (measured on the dense forms at tile 64: 9.3-80), the
# sighted landmark's own is the drawn noise and the little the filter has moved off the nominal state (measured 0.0002-0.25).  A gate of 2
# leaves a factor 4 on one side and 8 on the other; the 9 of the other scans would let a neighbour in.
ASSIGNED_GATE = 2.0
LOCAL_M = 40                     # landmarks of a joined local map
LOCAL_TILE = 32
# The windows behind batch boundaries 2, 3, ..: ("free",): the four tested steps of today, two more query kinds in the rotation;
# ("sync", kind, variant, behind a crossing scan): that call first behind the boundary, nothing else of the window is beside a pass;
# ("straddle",): an observe_model_assigned scan of 4 whose third gather is the first behind the boundary, so that the pass starts between two
# of its gathers -- the two new query kinds follow in places 3 and 4, the second beside one more assigned scan.  Robot-frame forms leave
# Prr = 0: factor_map stands a whole batch or more of motion steps away from them.
NEWER_WINDOWS = (
    ("free",), ("sync", "observe_model_joint", None, False), ("sync", "factor_map", None, True), ("free",),
    ("sync", "transform_map", "exact", False), ("sync", "transform_map", "uncertain", True), ("straddle",),
    ("sync", "extract_map", "robot", False), ("sync", "extract_map", "map", True), ("free",),
    ("sync", "join_map", None, False), ("sync", "join_map", None, True), ("free",),
    ("sync", "observe_model_joint_iterated", None, False), ("sync", "observe_model_joint", None, True), ("straddle",),
    ("sync", "transform_map", "robot", False), ("free",), ("sync", "factor_map", None, False), ("free",))
NEWER_BATCHES = len(NEWER_WINDOWS) + 1
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

    def _set_x(self, x):
        self.pose = np.asarray(x[:3], dtype=np.float64).copy()
        self.lm = [p.copy() for p in np.asarray(x[3:]).reshape(-1, 2)]

    def transform(self, form):
        """transform_map moves the pose and every landmark (transform_map_cases' own map)"""
        import transform_map_cases as Tm
        if form == "robot":
            self._set_x(Tm.extract_fn(self.x(), list(range(self.N)), "robot"))
        else:
            self._set_x(Tm.transform_fn(self.x(), Tm.T_RIGID))

    def join(self, y):
        """join_map composes the pose with the local one and appends the local landmarks where join_map_cases.join_fn puts them"""
        import join_map_cases as Jm
        n = 3 + 2 * self.N
        x = Jm.join_fn(self.x(), y)
        self.pose = x[:3].copy()
        return [self.append(p) for p in x[n:].reshape(-1, 2)]


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


# ------------------------------------------------------------------------------------------------------------------
# the payloads of make_plan(newer=True)
# ------------------------------------------------------------------------------------------------------------------
def _positions(nom):
    return np.array(nom.lm).reshape(-1, 2)


def _away(nom, k):
    d = nom.lm[k] - nom.pose[:2]
    return d @ d > 4.0


def joint_payload(nom, rng, half, c, npair, include=()):
    """(entries, landmarks, gate) of a joint update: npair pairings on landmarks of different tile rows (`include` first: landmarks of
    the scan in front), the four one-landmark models in turn, and one entry more that is left out (-1)"""
    lms = list(include)
    rows = {k // half for k in lms}
    q = 0
    while len(lms) < npair:
        k = (c * 733 + q * (3 * half + 1) + 5) % nom.N
        q += 1
        if k // half not in rows and _away(nom, k):
            lms.append(k)
            rows.add(k // half)
    out = 1 + c % (npair - 1)                                   # where the left-out entry stands
    hyp = lms[:out] + [-1] + lms[out:]
    sighted = lms[:out] + [(lms[0] + half) % nom.N] + lms[out:]
    entries = [scan_entry(nom, rng, k, 1 + q % 4) for q, k in enumerate(sighted)]
    return entries, hyp, JOINT_GATE


def local_map(nom, rng, M, c):
    """(y, sL, PL) of a scan-like local map, as tests/test_join_map_gpu.py builds one: the local robot at zero with P = 0 there (a submap
    started at the pose), M landmarks 5-40 away, each with a block of its own, and one shared direction so that no cross block is zero"""
    r, a = rng.uniform(5.0, 40.0, M), rng.uniform(0.0, 2.0 * np.pi, M)
    y = np.concatenate([np.zeros(3), np.stack([r * np.cos(a), r * np.sin(a)], axis=1).reshape(-1)])
    PL = np.zeros((3 + 2 * M, 3 + 2 * M))
    v = rng.uniform(0.05, 0.15, 2 * M) * rng.choice([-1.0, 1.0], 2 * M)
    PL[3:, 3:] = np.outer(v, v)
    for i in range(M):
        PL[3 + 2 * i:5 + 2 * i, 3 + 2 * i:5 + 2 * i] += RPOS * (1.0 + 0.1 * i)
    return y, 2.0e6 + 1000.0 * c + np.arange(M, dtype=np.float64), PL


def extract_indices(nom, rng, half, include=()):
    """about 40 landmarks in a shuffled order: the first, the last, one of every fifth tile row and `include`"""
    N = nom.N
    idx = {0, N - 1} | set(include) | {min(I * half + (I * 3) % half, N - 1) for I in range(0, -(-N // half), 5)}
    while len(idx) < min(40, N):
        idx.add(int(rng.integers(0, N)))
    idx = sorted(idx)
    return [idx[i] for i in rng.permutation(len(idx))]


def isolated_landmarks(nom, m, near=25.0):
    """the m landmarks 4-25 away from the robot whose nearest neighbour is farthest: ([landmarks], smallest of their neighbour distances)"""
    L = _positions(nom)
    r = np.hypot(*(L - nom.pose[:2]).T)
    cand = np.flatnonzero((r >= 4.0) & (r <= near))
    iso = np.empty(len(cand))
    for q, k in enumerate(cand):
        d = np.hypot(*(L - L[k]).T)
        d[k] = np.inf
        iso[q] = d.min()
    order = np.argsort(-iso, kind="stable")[:m]
    return [int(cand[q]) for q in order], float(iso[order].min())


def assigned_payload(nom, rng, m):
    """(entries, landmarks): m sightings with finite gates, each of a landmark with no other near it, so that the assignment has one
    candidate per entry and no choice -- RELATIVE_XY and RANGE_BEARING in turn (two rows: a one-row model has candidates all along a
    circle or a ray)"""
    lms, _ = isolated_landmarks(nom, m)
    entries = [dict(scan_entry(nom, rng, k, (M.RELATIVE_XY, M.RANGE_BEARING)[q % 2]), gate=ASSIGNED_GATE + 0.25 * q) for q, k in enumerate(lms)]
    return entries, lms


def assign_payload(nom, rng, c):
    """4-12 sightings for assign_model, some landmarks sighted twice, gates as tests/test_assign_model_beside_pass_gpu.py has them"""
    m = 4 + (3 * c) % 9
    ks = [(c * 211 + q * 977) % nom.N for q in range(m)]
    ks[m - 1] = ks[0]
    if m > 6:
        ks[4] = ks[1]
    ks = [k if _away(nom, k) else (k + 101) % nom.N for k in ks]
    return [dict(scan_entry(nom, rng, k, (M.RANGE_BEARING, M.RELATIVE_XY, M.RANGE, M.BEARING)[q % 4]), gate=9.21 * (1 + q % 3)) for q, k in enumerate(ks)]


def joint_search_payload(nom, rng, c):
    """(entries, thresholds) of a joint search: RELATIVE_XY sightings (joint_search_cases.cluster_scene's) of a landmark near the robot and
    its 3-5 nearest neighbours, joint_cases.scene_entries' entries, joint_search_cases.thresholds_even's thresholds"""
    import joint_cases as Jc
    import joint_search_cases as Sc
    K = 4 + c % 3
    L = _positions(nom)
    r = np.hypot(*(L - nom.pose[:2]).T)
    r[r < 4.0] = np.inf
    first = int(np.argsort(r, kind="stable")[c % 5])
    near = np.argsort(np.hypot(*(L - L[first]).T), kind="stable")[:K]
    scan = [(M.RELATIVE_XY, M.h_of(M.RELATIVE_XY, nom.pose, nom.lm[int(k)]) + rng.uniform(-0.04, 0.04, 2), RPOS) for k in near]
    return Jc.scene_entries(scan, Sc.GATE), Sc.thresholds_even(K)


def make_plan(x0, T, batch, batches, RC, seed=11, sharded=False, edits=False, R_scale=1.0, A_scale=1.0, reach=40.0, turn=3.0, fix_scale=1.0, edge_back=(0, 1, 2),
              newer=False):
    """(steps, info): `batches` full batches and four more steps.  R_scale: a factor on the R of every linear and model observation,
    fix_scale: one more on the position and heading fixes; A_scale: a factor on the R of an appended landmark's sighting; reach: how far from
    the robot landmarks are appended; turn: degrees per plain predict; edge_back: the tile-row-edge target is the first landmark of the
    tile row that many rows before the last, the three in turn.  info: 'appended' (0-based index, at the end of the plan, of every
    landmark append_model added; None after edits), 'crossing_scans' (tested scans that carry the map over a tile-row edge), 'N' at the end.

    A step takes one pair slot, an observe_model_assigned scan one per entry (assigned or left out: model_assigned.h runs finish_step for
    every entry), and a batch is complete when `batch` slots are: the places p and the boundaries k_b count slots.  Without `newer` that is
    the number of steps, and the plan is what it was before the keyword existed (tests/test_beside_pass_plan_cpu.py pins its digest).

    newer=True (`batches` is then NEWER_BATCHES): the windows of NEWER_WINDOWS behind the boundaries 2, 3, ..  info gains 'boundaries'
    (step -> k_b: the step whose pair completes batch k_b; a straddling scan completes it between two of its gathers), 'behind_scan' (the
    (step, kind) of the synchronising calls directly behind a crossing scan), 'straddlers' (steps) and 'appended' counts join_map's
    landmarks too."""
    rng = np.random.default_rng(seed)
    nom = Nominal(x0)
    half = T // 2
    nslots = batches * batch + 4
    nfill = -(-half // A_MAX)
    stride = max(1, (batch - 6) // nfill)
    fill_at = [5 + q * stride for q in range(nfill)]
    assert fill_at[-1] < batch and batch % 4 == 0
    assert not newer or (batches == NEWER_BATCHES and batch >= 8 and fill_at[-1] < batch - 1 and not sharded and not edits)
    count = dict(lin=0, mod=0, it=0, scan=0, chain=0, lr=0, free=0, straddle=0, sync=0, assign=0, search=0, local=0)
    steps, appended_ids, crossing = [], [], 0
    boundaries, behind_scan, straddlers = {}, [], []
    dup_ids = []
    signature = 1.0e6

    def window(k):
        return NEWER_WINDOWS[k - 2] if newer and 2 <= k < 2 + len(NEWER_WINDOWS) else ("free",)

    def newer_query(kind):
        if kind == "assign_model":
            count["assign"] += 1
            return assign_payload(nom, rng, count["assign"])
        count["search"] += 1
        return joint_search_payload(nom, rng, count["search"])

    def sync_call(kind, variant, scan_lms):
        """the payload of a synchronising call, the nominal state moved as the call moves the filter's"""
        c = count["sync"]
        count["sync"] += 1
        if kind in ("observe_model_joint", "observe_model_joint_iterated"):
            # (of a scan in front: its first and its last landmark, on either side of the tile-row edge it crossed)
            return joint_payload(nom, rng, half, c, 6 + c % 3, scan_lms[:1] + scan_lms[-1:])
        if kind == "join_map":
            y, sL, PL = local_map(nom, rng, LOCAL_M, c)
            ids = nom.join(y)
            appended_ids.extend(ids)
            return y, sL, PL
        if kind == "extract_map":
            return extract_indices(nom, rng, half, scan_lms), variant
        if kind == "transform_map":
            nom.transform(variant)
            return variant
        import factor_map_cases as Fm
        return Fm.reference_states(nom.x(), 2, 100 + c)

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

    t = slot = 0
    while slot < nslots:
        p, k_b = (slot + 1) % batch, (slot + 1) // batch
        win = window(k_b)
        # (behind a synchronising call nothing of its window is beside a pass: those steps are plain ones)
        tested = 1 <= p <= 4 and k_b >= 2 and not (win[0] == "sync" and p > 1)
        straddler = newer and p == batch - 1 and k_b >= 1 and window(k_b + 1)[0] == "straddle"
        taken = 1
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
        # (newer: a synchronising call that stands behind a scan has it as the FIRST operation behind the boundary, and no other has one)
        m_next = 3 + count["scan"] % 4
        scan_lms, crossed = [], False
        if tested and (p == 2 if win[0] != "sync" else win[3]):
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
            crossed = (before - 1) // half != (nom.N - 1) // half and before % half != 0
            crossing += crossed
            scan_lms = list(range(before, nom.N))
            ops.append(("append_model", entries, tested))
        elif not tested and p in fill_at and k_b >= 1:
            lead = 1 + (m_next - 1) // 2              # landmarks of the tested scan that stay in front of the edge
            want = min(A_MAX, (-(nom.N + lead)) % half)
            if want and (k_b + 1) * batch + 1 < nslots:
                entries, ids = append_scan(nom, rng, want, signature, A_scale=A_scale, reach=reach)
                signature += want
                appended_ids += ids
                ops.append(("append_model", entries, tested))
        # The boundary's own step first waits for the main stream (a query): the host runs ahead of the gathers within a batch, and
        # the pass starts only where the main stream reaches the boundary; so drained, it starts when the boundary's step is issued, and
        # the calls behind it wait for their own kernels alone
        if win[0] == "sync" and p == 1 and k_b >= 2:
            ops.append((win[1], sync_call(win[1], win[2], scan_lms), True))
            if win[3] and crossed:
                behind_scan.append((t, win[1]))
        if (p == 0 and k_b >= 2) or straddler:
            if sharded:
                ops.append(("associate_model", [dict(scan_entry(nom, rng, (k_b * 31) % nom.N, M.RANGE_BEARING), gate=9.0)], False))
            else:
                ops.append(("model_innovation", model_step(k_b), False))
        # the read-only queries, one per tested step, each kind in every place behind a boundary in turn
        if newer and k_b == 1 and 1 <= p <= 2:
            # (every query kind new here once in the first batch, untested: a kind's first call makes its allocations)
            ops.append((NEWER_QUERY_KINDS[p - 1], newer_query(NEWER_QUERY_KINDS[p - 1]), False))
        if tested and win[0] != "sync" and not (sharded and p != 1):
            kind = QUERY_KINDS[0] if sharded else QUERY_KINDS[(p - 1 + k_b) % 4]
            if newer and win[0] == "straddle":
                kind = NEWER_QUERY_KINDS[(p + count["straddle"]) % 2]
            elif newer:
                # six kinds, each in every place once over six free windows
                kind = (QUERY_KINDS + NEWER_QUERY_KINDS)[(p - 1 + count["free"]) % 6]
            if kind in NEWER_QUERY_KINDS:
                ops.append((kind, newer_query(kind), tested))
            elif kind == "associate_model":
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
        tested = tested and win[0] != "sync"
        if straddler or (newer and tested and win[0] == "straddle" and p == 4):
            # a scan of 4 whose first two entries complete the batch, or one of 3 in the last tested place
            entries, lms = assigned_payload(nom, rng, 4 if straddler else 3)
            taken = len(entries)
            if straddler:
                straddlers.append(t)
            ops.append((NEWER_PAIR_KIND, (entries, lms), straddler or tested))
        elif kind == "correct":
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
        if newer and p == 4 and k_b >= 2 and win[0] in ("free", "straddle"):
            count[win[0]] += 1
        if (slot + taken) // batch != slot // batch:
            boundaries[t] = (slot + taken) // batch
        t, slot = t + 1, slot + taken
    appended = None if edits else [nom.ids.index(i) for i in appended_ids]
    info = dict(appended=appended, crossing_scans=int(crossing), N=nom.N)
    if newer:
        info.update(boundaries=boundaries, behind_scan=behind_scan, straddlers=straddlers)
    return steps, info


def places(steps, batch):
    """[(p, k_b, slots)] per step, from the plan alone: the place of the step's first pair slot behind a batch boundary and that boundary,
    counted in pair slots -- one per step, one per entry of an observe_model_assigned scan -- and the slots the step takes"""
    out, slot = [], 0
    for ops in steps:
        kind, payload, _ = ops[-1]
        taken = len(payload[0]) if kind == NEWER_PAIR_KIND else 1
        out.append(((slot + 1) % batch, (slot + 1) // batch, taken))
        slot += taken
    return out


def _feed(h, v):
    if isinstance(v, dict):
        for k, w in v.items():
            h.update(str(k).encode())
            _feed(h, w)
    elif isinstance(v, (list, tuple)):
        h.update(b"[%d" % len(v))
        for w in v:
            _feed(h, w)
    elif isinstance(v, str):
        h.update(v.encode())
    elif v is None:
        h.update(b"None")
    else:
        a = np.asarray(v)
        a = a.astype(np.int64) if a.dtype.kind in "iub" else a.astype(np.float64)
        h.update(a.dtype.str.encode())
        h.update(np.ascontiguousarray(a).tobytes())


def plan_digest(steps):
    """sha256 over the plan: every operation's kind, its tested flag and the bytes of every float and integer array of its payload, in order"""
    h = hashlib.sha256()
    for ops in steps:
        h.update(b"step")
        for kind, payload, tested in ops:
            h.update(kind.encode())
            h.update(b"T" if tested else b"F")
            _feed(h, payload)
    return h.hexdigest()


def appended_total(steps):
    return sum(len(payload) for ops in steps for kind, payload, _ in ops if kind == "append_model")


# ------------------------------------------------------------------------------------------------------------------
# the interpreters
# ------------------------------------------------------------------------------------------------------------------
def _model_kw(o):
    return {k: v for k, v in o.items() if k != "rows"}


def second_handles(steps, **engine_kw):
    """The second handle of every two-handle call of the plan, in plan order, made AHEAD of the run (making an engine allocates and
    waits; behind a boundary that would outlast the pass): for a join_map the local engine brought to the payload's (x, s, P), for an
    extract_map a new engine of the capacity the indices need."""
    import join_map_cases as Jm
    from ekf_slam_amd import Engine
    out = []
    for ops in steps:
        for kind, payload, _ in ops:
            if kind == "join_map":
                y, sL, PL = payload
                out.append(Jm.set_state(Engine(mode="known", capacity=len(sL) + 2, tile=LOCAL_TILE, storage="f64", **engine_kw), y, sL, PL))
            elif kind == "extract_map":
                out.append(Engine(mode="known", capacity=max(len(payload[0]), 1), storage="f64", **engine_kw))
    return out


def issue(eng, kind, payload, second=None):
    """One operation on an engine or a group of shards; a query's result, else None.  second: an iterator over second_handles(steps)
    (None: the handle is made here).  join_map returns (first new landmark, the local engine), extract_map the destination;
    observe_model_assigned returns None: assigned_scan_result() fetches the scan, a wait the caller places."""
    if kind in SYNC_KINDS:
        import transform_map_cases as Tm
        if kind == "observe_model_joint":
            return eng.observe_model_joint(payload[0], payload[1], gate=payload[2], want_nu=True, want_S=True)
        if kind == "observe_model_joint_iterated":
            return eng.observe_model_joint(payload[0], payload[1], gate=payload[2], want_nu=True, want_S=True, iterations=ITERATIONS)
        if kind == "join_map":
            lo = next(second) if second is not None else second_handles([[(kind, payload, True)]])[0]
            return eng.join_map(lo, 0.0), lo
        if kind == "extract_map":
            return eng.extract_map(payload[0], payload[1], into=next(second) if second is not None else second_handles([[(kind, payload, True)]])[0])
        if kind == "transform_map":
            return eng.transform_map(*Tm.form_args(payload))
        return eng.factor_map(payload)
    if kind == NEWER_PAIR_KIND:
        return eng.observe_model_assigned(payload[0])
    if kind == "assign_model":
        return eng.assign_model(payload, want_candidates=True)
    if kind == "joint_search":
        return eng.joint_search(payload[0], payload[1], beam=64, want_alive=True)
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
    elif kind == NEWER_PAIR_KIND:
        for o in assigned_steps(payload):
            apply_factored(ref, "observe_model", o)
    elif kind not in QUERY_KINDS + NEWER_QUERY_KINDS:
        raise ValueError(kind)


def assigned_steps(payload):
    """an observe_model_assigned scan as what it amounts to: observe_model on the intended landmark, entry by entry, under the entry's gate"""
    return [M.obs(e["model"], e["z"], e["R"], [k], gate=e["gate"]) for e, k in zip(*payload)]


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
    elif kind in SYNC_KINDS or kind == NEWER_PAIR_KIND:
        return _apply_dense_newer(dense, kind, payload)
    elif kind not in QUERY_KINDS + NEWER_QUERY_KINDS:
        raise ValueError(kind)


def _apply_dense_newer(dense, kind, payload):
    """The calls of make_plan(newer=True) by their files' own dense forms.  Returns the joint record, factor_dense's dict, extract_dense's
    (x, s, P), or for an assigned scan the dense assignment's {'landmark', 'ncand'} at the state in front of the scan."""
    import associate_model_cases as Am
    import extract_map_cases as Xm
    import factor_map_cases as Fm
    import join_map_cases as Jm
    import observe_joint_cases as Oj
    import observe_joint_iter_cases as Oi
    import transform_map_cases as Tm
    if kind == "observe_model_joint":
        dense.x, dense.P, rec = Oj.joint_update_dense(dense.x, dense.P, payload[0], payload[1], payload[2])
        assert rec["outcome"] == Oj.APPLIED
        return rec
    if kind == "observe_model_joint_iterated":
        dense.x, dense.P, rec, it = Oi.joint_update_iterated_dense(dense.x, dense.P, payload[0], payload[1], ITERATIONS, gate=payload[2])
        assert rec["outcome"] == Oi.APPLIED and it["used"] == ITERATIONS
        return rec
    if kind == "join_map":
        x, s, P = Jm.join_dense(dense.x, dense.s, dense.P, *payload)
        dense.x, dense.s, dense.P = x, list(s), P
        return None
    if kind == "extract_map":
        return Xm.extract_dense(dense.x, dense.s, dense.P, payload[0], payload[1])
    if kind == "transform_map":
        x, s, P = Tm.transform_dense(dense.x, dense.s, dense.P, payload)
        dense.x, dense.s, dense.P = x, list(s), P
        return None
    if kind == "factor_map":
        return Fm.factor_dense(dense.x, dense.P, payload)
    D = Am.d2_matrix(dense.x, dense.P, payload[0])
    inside = [np.flatnonzero(D[q] <= e["gate"]) for q, e in enumerate(payload[0])]
    res = dict(landmark=np.array([int(i[0]) if len(i) == 1 else -1 for i in inside]), ncand=np.array([len(i) for i in inside]))
    for o in assigned_steps(payload):
        dense.x, dense.P, r = M.observe_model_dense(dense.x, dense.P, o)
        assert r["outcome"] == M.APPLIED
    return res


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
