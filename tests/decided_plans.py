"""Scan plans for the device-decided branch (cfg.device_assoc == 4) with the position-weighted likelihood (w_pos = 1,
Correspondence.m:74): seeded, and shaped so that the position cost rejects some signature matches -- rows whose decision a
signature-only prediction would get wrong.

A plan is a list of (u, rows) with rows an m x 3 array [range, bearing_deg, signature] as ekf_measure takes it, plus ONE landmark
list (index 1..K, loc) that resolves every key the filter can append under.  Observations are taken from a true pose of a
seeded world; a row's signature is that of the world landmark it sees (k + 1), so it matches the filter's landmark k as long as
the position cost agrees; rows of landmarks the filter has not seen yet carry a fresh signature and append."""
import math

import numpy as np

PARAMS = dict(w_pos=1.0, Rc=(0.01, 0.01), s_thresh=0.5)     # the position-weighted likelihood: its cost rejects some signature matches

_D2R = math.pi / 180.0


def _wrap360(a):
    w = math.fmod(a, 360.0)
    return w + 360.0 if w < 0.0 else w


def make_plan(seed, n_world, steps, m, known_frac=0.75):
    """Plan of `steps` scans (u, rows, lm_index, lm_loc) of m rows; scan 0 sights landmark 0 alone (it appends under the empty-map
    rule, EKF_SLAM_UC.m:110-111, which needs a landmark list of one entry).  Each later scan sights m landmarks: about known_frac of them among those seen before, the rest new, in
    the order of their world index (so that consecutive new sightings append consecutive keys, across tile-row edges)."""
    rng = np.random.default_rng(seed)
    span = 4.0 * math.sqrt(n_world / 20.0)
    pos = rng.uniform(-span, span, size=(n_world, 2))
    pose = np.array([0.0, 0.0, 0.0])
    seen = 0
    plan = []
    for t in range(steps):
        u = np.array([0.1 + rng.normal(0.0, 0.005), 3.0 + rng.normal(0.0, 0.1)])
        th = pose[2] + u[1]
        pose = np.array([pose[0] + u[0] * math.cos(th * _D2R), pose[1] + u[0] * math.sin(th * _D2R), th])
        if t == 0:
            ids = [0]
        else:
            ids = []
            for _ in range(m):
                now = seen + len({i for i in ids if i >= seen})      # including the ones first sighted earlier in this scan
                if rng.random() < known_frac or now >= n_world:
                    ids.append(int(rng.integers(0, now)))            # (may repeat a landmark appended earlier in the same scan)
                else:
                    ids.append(now)
        rows = []
        for k in ids:
            dx, dy = pos[k, 0] - pose[0], pos[k, 1] - pose[1]
            r = math.hypot(dx, dy) + rng.normal(0.0, 0.02)
            b = _wrap360(math.atan2(dy, dx) / _D2R - pose[2] + rng.normal(0.0, 0.5))
            rows.append((max(r, 1e-3), b, float(k + 1)))
        seen = max(seen, max(ids) + 1)
        lm_index = np.arange(1, (1 if t == 0 else n_world) + 1, dtype=np.float64)
        plan.append((u, np.array(rows, dtype=np.float64).reshape(-1, 3), lm_index, pos[:len(lm_index)].copy()))
    return plan


class _Entry:
    __slots__ = ("loc", "index")

    def __init__(self, loc, index):
        self.loc, self.index = loc, index


class _Source:
    def __init__(self, lm_index, lm_loc):
        self.landmark = [_Entry(np.asarray(lm_loc[i], dtype=np.float64), float(lm_index[i])) for i in range(len(lm_index))]


class PlanLandmarks:
    """The landmark-list surface the oracle's measure() reads, over a fixed plan row block and landmark list."""

    def __init__(self, lm_index, lm_loc):
        self.landmarkObj = _Source(lm_index, lm_loc)
        self.rows = None

    def getLandmark(self, laserdata, x):
        return self.rows


def oracle_run(ref, plan):
    """Drive the structured oracle (its w_pos as configured) through the plan, row by row as its measure() does; returns the
    number of rows whose decision the signature-only likelihood (w_pos = 0) would have taken differently on the same state."""
    from oracle.ekf_dense import _lookup_loc
    differ = 0
    for u, rows, lm_index, lm_loc in plan:
        ref.predict(u)
        src = PlanLandmarks(lm_index, lm_loc)
        for z in rows:
            R = np.array([[z[0] * ref.Rc[0], 0.0], [0.0, z[1] * ref.Rc[1]]])
            if ref.N == 0:
                ref.append(u, R, _lookup_loc(src, None), 1)
                continue
            new_lm, idx = ref.associate(z, R)
            w = ref.w_pos
            ref.w_pos = 0.0
            new0, idx0 = ref.associate(z, R)
            ref.w_pos = w
            differ += (new_lm, idx) != (new0, idx0)
            if new_lm:
                ref.append(u, R, _lookup_loc(src, idx), idx)
            else:
                ref.correct(z, R, idx)
    return differ
