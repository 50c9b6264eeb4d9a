"""Host mirror of the reference's MATLAB class surface over libekfslam (no arithmetic lives here).

Same names, argument meaning and 1-based landmark indices as the reference, so a user of
``EKF_SLAM`` / ``EKF_SLAM_UC`` / ``Correspondence`` / ``Landmark`` / ``SLAM`` / ``append`` finds the same calls:

    SLAM(name)                         SLAM.m:21-40       .predict(u) :42  .measure(laserdata,u) :52  .runSlam() :70
    EKF_SLAM() / EKF_SLAM_UC()         EKF_SLAM.m:26-34 / EKF_SLAM_UC.m:27-36
      .predict(u)                      EKF_SLAM.m:40-51
      [x_new,F] = .f(x,u)              EKF_SLAM.m:56-65
      .append(u,R,landmarkPos,sig)     EKF_SLAM.m:67-98
      .measure(laserData,u,lm_list)    EKF_SLAM.m:100-151 / EKF_SLAM_UC.m:102-152
      properties x P Q s C Rc ...      EKF_SLAM.m:5-22
    Correspondence(cost,thresh,method) Correspondence.m:12-25   .estimateCorrespondence(z,R,x,P,s) :28-88
    Landmark(method)                   Landmark.m:12-33         .getLandmark(laserdata,x)
    [x,P] = append(x,P,u,idx,R,pos)    append.m:1-27

Differences forced by the host language: x is a 1-D array (the reference's 1 x n row vector); plotting
(EKF_SLAM.m:154-234, out of scope) is replaced by ``plot_data()`` which returns what plot() reads (pose and
the 2x2 diagonal covariance blocks); the ROS subscribers of SLAM.m:23-24 are replaced by a scripted
(u, scan) feed.
"""
import math
import warnings

import numpy as np

from . import _lib as L
from . import marshal
from .engine import Engine
from .marshal import _p, _vec
from .world import SyntheticLandmark

_DEFAULT_CAPACITY = 1024


def _gamma_p(a, x):
    """The regularised lower incomplete gamma function P(a, x), a > 0, x >= 0: its series below a + 1, the continued fraction of its
    complement above."""
    if x <= 0.0:
        return 0.0
    front = math.exp(a * math.log(x) - x - math.lgamma(a))
    if x < a + 1.0:
        term = total = 1.0 / a
        n = a
        while abs(term) > abs(total) * 1e-17:
            n += 1.0
            term *= x / n
            total += term
        return front * total
    tiny = 1e-300
    b = x + 1.0 - a
    c, d = 1.0 / tiny, 1.0 / b
    frac = d
    for i in range(1, 10000):
        an = -i * (i - a)
        b += 2.0
        d = an * d + b
        d = tiny if abs(d) < tiny else d
        c = b + an / c
        c = tiny if abs(c) < tiny else c
        d = 1.0 / d
        delta = d * c
        frac *= delta
        if abs(delta - 1.0) < 1e-16:
            break
    return 1.0 - front * frac


def chi2_quantile(p, dof):
    """The value a chi-square variable with dof degrees of freedom stays below with probability p (0 < p < 1): Newton's iteration on the
    regularised incomplete gamma function, kept inside a bracket; dof = 0 gives 0.  What a joint d2 is gated against."""
    p, dof = float(p), int(dof)
    if not 0.0 < p < 1.0 or dof < 0:
        raise ValueError("chi2_quantile: 0 < p < 1 and dof >= 0")
    if dof == 0:
        return 0.0
    a = 0.5 * dof
    lo, hi = 0.0, max(1.0, a)
    while _gamma_p(a, hi) < p:
        lo, hi = hi, 2.0 * hi
    x = 0.5 * (lo + hi)
    for _ in range(200):
        f = _gamma_p(a, x) - p
        if f > 0.0:
            hi = x
        else:
            lo = x
        dens = math.exp((a - 1.0) * math.log(x) - x - math.lgamma(a))
        step = x - f / dens if dens > 0.0 else x
        nxt = step if lo < step < hi else 0.5 * (lo + hi)
        if abs(nxt - x) <= 1e-14 * x:
            x = nxt
            break
        x = nxt
    return 2.0 * x


def select_merge_batch(candidates, limit):
    """The pairs of ONE search that one merge_landmarks_batch call can take: walk the (i, j, d2) rows of duplicate_candidates in
    their (d2, i) order and accept (keep = j, drop = i) when i is not yet a keep or a drop and j is not yet a drop -- a keep may be
    shared, so a triple fuses in one batch; a row whose partner was just dropped waits for the next search.  Stops at `limit`
    pairs.  Returns [(keep, drop, d2)] with the candidates' d2.  A pure function: no engine involved."""
    keeps, drops, out = set(), set(), []
    for i, j, d2 in candidates:
        if len(out) >= limit:
            break
        if i in keeps or i in drops or j in drops:
            continue
        keeps.add(j)
        drops.add(i)
        out.append((j, i, d2))
    return out


class _EkfBase:
    _mode = "known"

    def __init__(self, capacity=_DEFAULT_CAPACITY, **engine_kw):
        self._e = Engine(mode=self._mode, capacity=capacity, **engine_kw)
        self.landmark_list = None
        self.observed = None
        self.log = None             # a TrajectoryLog records what predict / measure consume

    # ---- the reference's public properties, pulled from HBM on demand ----
    @property
    def x(self):
        return self._e.get_x()

    @x.setter
    def x(self, v):                 # assignable like the reference's (EKF_SLAM.m:6-9); x fixes the landmark count
        self._e.set_x(v)

    @property
    def P(self):
        return self._e.get_P()

    @P.setter
    def P(self, v):
        self._e.set_P(v)

    @property
    def s(self):
        return self._e.get_s()

    @s.setter
    def s(self, v):
        self._e.set_s(v)

    @property
    def Q(self):
        """zeros(size(P)) with the 3x3 process-noise block (EKF_SLAM.m:43-44)."""
        n = self._e.n
        Q = np.zeros((n, n))
        Q[0:3, 0:3] = self._e.get_Q3()
        return Q

    @property
    def C(self):
        return self._e.cfg.C

    @C.setter
    def C(self, v):
        self._e.set_params(C=v)

    @property
    def Rc(self):
        return [self._e.cfg.Rc[0], self._e.cfg.Rc[1]]

    @Rc.setter
    def Rc(self, v):
        self._e.set_params(Rc=v)

    @property
    def s_cost(self):               # public assignable properties of the reference (EKF_SLAM.m:14-16)
        return self._e.cfg.s_cost

    @s_cost.setter
    def s_cost(self, v):
        self._e.set_params(s_cost=v)

    @property
    def s_thresh(self):
        return self._e.cfg.s_thresh

    @s_thresh.setter
    def s_thresh(self, v):
        self._e.set_params(s_thresh=v)

    # ---- methods ----
    def predict(self, u):
        self._last_u = np.asarray(u, dtype=np.float64)
        self._e.predict(u)

    def f(self, x, u):
        x = _vec(x)
        n = x.size
        x_new = np.empty(n)
        F = np.empty(n * n)
        marshal.host_call("ekf_motion_model", self._e.lib, _p(x), n, _p(_vec(u, 2)), _p(x_new), _p(F))
        return x_new, F.reshape(n, n, order="F")

    def append(self, u, R, landmarkPos, signature):
        self._e.append(u, R, landmarkPos, signature)

    def remove_landmarks(self, idx):
        """Drop landmarks idx (1-based like every landmark index of this layer; a number or any iterable, any order) from
        the map: their entries of x, their signatures, their rows and columns of P -- on the device, survivors keep order
        and bits (ekf_remove_landmarks).  The reference has no such method and no policy for WHICH landmark to drop: that
        is the caller's.  Signatures are not renumbered (assign .s if the UC convention 'new signature = N + 1' collides)."""
        idx = np.asarray(idx).reshape(-1)
        if idx.size and not np.all(idx == np.floor(idx)):
            raise ValueError("remove_landmarks: landmark indices are whole numbers")
        self._e.remove_landmarks([int(i) - 1 for i in idx])
        if self.log is not None:
            self.log.record_edit("remove", idx)

    @staticmethod
    def _landmark_numbers(what, *idx):
        v = np.asarray(idx, dtype=np.float64).reshape(-1)
        if not np.all(v == np.floor(v)):
            raise ValueError("%s: landmark indices are whole numbers" % what)
        return [int(i) for i in v]

    def constrain_landmarks(self, i, j, delta=None, R=None):
        """'landmark i minus landmark j was observed as delta, with noise covariance R' (1-based i != j; delta None: (0, 0) -- the
        same point; R None: zero): a linear EKF correction between two landmarks, on the device (ekf_constrain_landmarks).
        The reference has no such method."""
        i, j = self._landmark_numbers("constrain_landmarks", i, j)
        self._e.constrain_landmarks(i - 1, j - 1, delta, R)
        if self.log is not None:
            self.log.record_edit("constrain", [i, j], delta, R)

    def merge_landmarks(self, keep, drop, R=None):
        """Fuse two landmarks that are the same point (1-based): constrain_landmarks(keep, drop, None, R), then
        remove_landmarks(drop).  `keep` retains its signature; its number afterwards is keep - (drop < keep).  WHICH pairs to
        merge is the caller's policy: landmark_distance is the gate (ekf_merge_landmarks)."""
        keep, drop = self._landmark_numbers("merge_landmarks", keep, drop)
        self._e.merge_landmarks(keep - 1, drop - 1, R)
        if self.log is not None:
            self.log.record_edit("merge", [keep, drop], None, R)

    def merge_landmarks_batch(self, pairs, R=None):
        """Fuse every (keep, drop) of `pairs` (1-based numbers as they are before the call, at most EKF_MERGE_BATCH_MAX pairs) in one
        call: constrain_landmarks(keep, drop, None, R) pair by pair in list order, then ONE remove_landmarks(all drops) -- the same
        bits with F64 tiles, one rounding instead of m with float tiles, and one pass over P instead of 2 m.  A keep may be shared;
        no keep may be dropped.  Returns d2[k] as landmark_distance(keep_k, drop_k, None, R) would report it just before
        constraint k (ekf_merge_landmarks_batch).  The reference has no such method."""
        rows = [tuple(p) for p in pairs]
        if any(len(p) != 2 for p in rows):
            raise ValueError("merge_landmarks_batch: pairs are (keep, drop)")
        flat = self._landmark_numbers("merge_landmarks_batch", *[a for p in rows for a in p])
        d2 = self._e.merge_landmarks_batch([(flat[2 * k] - 1, flat[2 * k + 1] - 1) for k in range(len(rows))], R)
        if self.log is not None and rows:
            self.log.record_edit("merge_batch", flat, None, R)
        return d2

    def landmark_distance(self, i, j, delta=None, R=None):
        """(d2, S) of 'landmark i minus landmark j = delta' under the current state (1-based): the squared Mahalanobis distance
        and the 2 x 2 innovation covariance.  Changes nothing (ekf_landmark_distance)."""
        i, j = self._landmark_numbers("landmark_distance", i, j)
        return self._e.landmark_distance(i - 1, j - 1, delta, R)

    def nearest_landmarks(self, R=None):
        """(d2, partner) for every landmark, 1-based: partner[k - 1] is the landmark j < k that minimises
        landmark_distance(k, j, None, R)[0], d2[k - 1] that minimum; partner 0 (and d2 = +inf) means none -- landmark 1, rows whose
        pairs are all singular.  The lowest number wins ties.  One read-only pass over P on the device; changes nothing
        (ekf_nearest_landmarks).  The reference has no such method."""
        d2, partner = self._e.nearest_landmarks(R)
        return d2, partner + 1

    def duplicate_candidates(self, gate, R=None):
        """[(i, j, d2)] of the landmarks whose nearest earlier landmark lies at or below `gate` (compare with a chi-square value,
        2 degrees of freedom), 1-based, j < i, sorted by (d2, i)."""
        return [(i + 1, j + 1, d2) for i, j, d2 in self._e.duplicate_candidates(gate, R)]

    def factor_map(self, ref=None):
        """The Cholesky factorisation of P on the device as a dict: definite, bad_index, bad_pivot, logdet, logdet_map, min_pivot,
        max_pivot and d2 per reference state (Engine.factor_map; ekf_factor_map).  Read-only: nothing goes into the trajectory log.
        For a SUBSET of the landmarks, extract_map them first and call factor_map on the small filter.  The reference has no such
        method."""
        return self._e.factor_map(ref)

    def nees(self, x_true):
        """(d2, dof): the normalised estimation error squared (x - x_true)' P^-1 (x - x_true) of the whole state against the ground
        truth x_true (3 + 2 N entries, the heading difference wrapped), and its degrees of freedom 3 + 2 N -- the standard consistency
        measure of EKF-SLAM.  NaN where P is not positive definite (factor_map says where)."""
        res = self._e.factor_map(np.asarray(x_true, dtype=np.float64).reshape(-1))
        return float(res["d2"][0]), res["n"]

    def nees_within(self, x_true, p=0.95):
        """(inside, d2, (lo, hi)): whether nees(x_true) lies inside the two-sided chi-square interval of probability p for 3 + 2 N degrees
        of freedom, lo = chi2_quantile((1 - p) / 2, dof) and hi = chi2_quantile((1 + p) / 2, dof).  Below lo the filter is too
        cautious, above hi it is overconfident; a P that is not definite is outside."""
        if not 0.0 < float(p) < 1.0:
            raise ValueError("nees_within: 0 < p < 1")
        d2, dof = self.nees(x_true)
        lo, hi = chi2_quantile(0.5 * (1.0 - float(p)), dof), chi2_quantile(0.5 * (1.0 + float(p)), dof)
        return bool(lo <= d2 <= hi), d2, (lo, hi)

    def map_entropy(self):
        """The differential entropy of the Gaussian the filter carries, 1/2 (n log(2 pi e) + log det P) in nats with n = 3 + 2 N: what an
        exploration planner or a 'is this submap worth keeping' policy ranks by.  NaN where P is not positive definite."""
        res = self._e.factor_map()
        return 0.5 * (res["n"] * math.log(2.0 * math.pi * math.e) + res["logdet"])

    def sample_map(self, k=None, seed=None, xi=None):
        """(samples, info): k joint draws of the posterior N(x, P) as the rows of `samples`, from ONE factorisation on the device
        (Engine.sample_map; ekf_sample_map).  With `xi` (one draw, or one per row) the standard-normal draws are the caller's and a
        sample is x + C xi; otherwise k draws come from numpy.random.default_rng(seed).standard_normal.  The heading entry is not
        wrapped.  Where P is not definite every sample is NaN and `info` (factor_map's dict without d2) says where.  Read-only:
        nothing goes into the trajectory log.  For a SUBSET of the landmarks, extract_map them first.  The reference has no such
        method."""
        if xi is None:
            if k is None or int(k) < 1:
                raise ValueError("sample_map: k >= 1 draws, or xi")
            xi = np.random.default_rng(seed).standard_normal((int(k), 3 + 2 * self._e.N))
        elif k is not None or seed is not None:
            raise ValueError("sample_map: xi carries the draws; k and seed go with draws made here")
        return self._e.sample_map(xi)

    def _definite_samples(self, who, k, seed):
        samples, info = self.sample_map(k, seed)
        if not info["definite"]:
            raise ValueError("%s: P is not positive definite (factor_map says where: bad_index %d)" % (who, info["bad_index"]))
        return samples

    def posterior_expectation(self, fn, k, seed=None):
        """(mean, standard error of the mean) of fn(sample) over k >= 2 draws of the posterior (sample_map(k, seed)); fn takes a state
        vector of 3 + 2 N entries and returns a scalar or a vector.  The standard error is the sample standard deviation (k - 1 in the
        denominator) over sqrt(k).  ValueError where P is not positive definite."""
        if int(k) < 2:
            raise ValueError("posterior_expectation: k >= 2 draws")
        vals = np.array([np.asarray(fn(row), dtype=np.float64) for row in self._definite_samples("posterior_expectation", k, seed)])
        return vals.mean(axis=0), vals.std(axis=0, ddof=1) / math.sqrt(vals.shape[0])

    def probability(self, event, k, seed=None):
        """(p, standard error): the share p of k draws of the posterior for which event(sample) is true, and its binomial standard error
        sqrt(p (1 - p) / k).  ValueError where P is not positive definite."""
        hits = sum(1 for row in self._definite_samples("probability", k, seed) if event(row))
        p = hits / float(int(k))
        return p, math.sqrt(p * (1.0 - p) / int(k))

    def solve_map(self, B, form="full"):
        """(out, info): P^-1 b (form="full") or the whitened C^-1 b (form="half") for the right-hand sides in the rows of B, from ONE
        factorisation on the device (Engine.solve_map; ekf_solve_map).  Plain linear algebra: no entry is wrapped.  Where P is not
        definite every entry is NaN and `info` (factor_map's dict without d2) says where.  Read-only: nothing goes into the
        trajectory log.  The reference has no such method."""
        return self._e.solve_map(B, form)

    def _definite_solve(self, who, B, form):
        out, info = self._e.solve_map(B, form)
        if not info["definite"]:
            raise ValueError("%s: P is not positive definite (factor_map says where: bad_index %d)" % (who, info["bad_index"]))
        return out

    def _state_columns(self, who, idx):
        """The indices into x of the robot (idx None) or of the landmarks idx, both entries of each, in idx's order."""
        if idx is None:
            return np.arange(3)
        lm = np.asarray(idx, dtype=np.int64).reshape(-1)
        if lm.size < 1 or lm.min() < 0 or lm.max() >= self._e.N or np.unique(lm).size != lm.size:
            raise ValueError("%s: idx is distinct landmarks 0 .. N - 1, or None for the robot" % who)
        return (3 + 2 * lm[:, None] + np.arange(2)[None, :]).reshape(-1)

    def information_columns(self, idx=None):
        """The columns of the information matrix Lambda = P^-1 that belong to the robot (idx None: 3 columns) or to the landmarks idx
        (two each, in idx's order), as an (3 + 2 N) x m array, by unit right-hand sides through one solve_map call.  An entry that
        is (nearly) zero means the two states are conditionally independent given the rest.  ValueError where P is not positive
        definite."""
        cols = self._state_columns("information_columns", idx)
        n = 3 + 2 * self._e.N
        B = np.zeros((cols.size, n))
        B[np.arange(cols.size), cols] = 1.0
        return self._definite_solve("information_columns", B, "full").T

    def conditional_covariance(self, idx):
        """inv(Lambda_AA) for the landmarks idx (2 m x 2 m, in idx's order): the covariance of that group GIVEN every other state, the
        Schur complement P_AA - P_AB inv(P_BB) P_BA, from information_columns(idx).  How much smaller it is than the marginal block
        of P says how much of what is known about the group is carried by the rest of the map."""
        if idx is None:
            raise ValueError("conditional_covariance: idx is the landmarks of the group")
        cols = self._state_columns("conditional_covariance", idx)
        Laa = self.information_columns(idx)[cols, :]
        cov = np.linalg.inv(0.5 * (Laa + Laa.T))
        return 0.5 * (cov + cov.T)

    def mahalanobis(self, a, b):
        """|C^-1 (a - b)|^2 = (a - b)' P^-1 (a - b) for two full states a and b (3 + 2 N entries each), the heading difference wrapped
        into (-180, 180] as factor_map wraps x - ref: nees(x_true) is mahalanobis(x, x_true).  ValueError where P is not positive
        definite."""
        n = 3 + 2 * self._e.N
        d = np.asarray(a, dtype=np.float64).reshape(-1) - np.asarray(b, dtype=np.float64).reshape(-1)
        if d.size != n:
            raise ValueError("mahalanobis: a state has 3 + 2 N = %d entries" % n)
        if not -180.0 < d[2] <= 180.0:
            d[2] = d[2] - 360.0 * math.ceil((d[2] - 180.0) / 360.0)
        w = self._definite_solve("mahalanobis", d, "half")[0]
        return float(w @ w)

    def multiply_map(self, B):
        """P b for the vectors in the rows of B, P exactly what get_P() reports, from one read-only pass over the tile store per 16
        vectors on the device -- no factorisation (Engine.multiply_map; ekf_multiply_map).  Plain linear algebra: no entry is wrapped.
        Read-only: nothing goes into the trajectory log.  The reference has no such method."""
        return self._e.multiply_map(B)

    def covariance_of(self, A):
        """A P A' (m x m, symmetrised) for the m linear functions of the state in the rows of A (m x (3 + 2 N), or one row): the
        covariance of a centroid, of the vector between two landmarks, of a path length, of any linear cost -- from ONE multiply_map
        call with A's rows."""
        n = 3 + 2 * self._e.N
        Av = np.asarray(A, dtype=np.float64)
        if Av.ndim == 1:
            Av = Av.reshape(1, -1)
        if Av.ndim != 2 or Av.shape[0] < 1 or Av.shape[1] != n:
            raise ValueError("covariance_of: A is m >= 1 rows of 3 + 2 N = %d entries" % n)
        cov = Av @ self._e.multiply_map(Av).T
        return 0.5 * (cov + cov.T)

    def cross_covariance(self, idx_a, idx_b):
        """The block P[a, b] between two arbitrary groups of states: each of idx_a, idx_b is a list of distinct landmarks (two rows or
        columns each, in the list's order) or None for the robot (three).  One multiply_map call with the unit vectors of the
        SHORTER list; P is symmetric, so the block of the longer one is the transpose of what comes back."""
        ca = self._state_columns("cross_covariance", idx_a)
        cb = self._state_columns("cross_covariance", idx_b)
        n = 3 + 2 * self._e.N
        short, other = (ca, cb) if ca.size <= cb.size else (cb, ca)
        E = np.zeros((short.size, n))
        E[np.arange(short.size), short] = 1.0
        block = self._e.multiply_map(E)[:, other]                # rows: P[short, other]
        return block if ca.size <= cb.size else block.T

    def solve_residual(self, B, form="full"):
        """(z, r): z = solve_map(B, form)[0] and r = P z - b for each right-hand side, the a-posteriori check of a solve -- for
        form="full" r is the residual of P z = b itself; for form="half" (z = C^-1 b) it is P z - b all the same, for a caller who
        wants that product.  Two device calls: the solve, then one multiply_map of its result.  ValueError where P is not positive
        definite."""
        Bv = np.asarray(B, dtype=np.float64)
        z = self._definite_solve("solve_residual", Bv, form)
        return z, self._e.multiply_map(z) - Bv.reshape(z.shape)

    def observe_dense(self, H, z, R, gate=float("inf"), wrap_deg=None):
        """A linear observation "H x = z +- R" whose k <= 16 rows may touch EVERY landmark: H a k x (3 + 2 N) array in x's order or a
        list of {state index: coefficient} rows (0-based indices into x), z the k values, R k x k (or its diagonal; 0 conditions
        exactly), wrap_deg the rows whose innovation is an angle in degrees.  Exact, no linearisation; applied only if d2 <= gate.  One
        product pass and one update pass over P on the device, the pending pairs flushed first (Engine.observe_dense;
        ekf_observe_dense).  Returns {'d2', 'rows', 'outcome', 'bad_row', 'nu', 'S'}; an S that is not positive definite raises
        EkfError and changes nothing.  Unsharded handles only.  The reference has no such method."""
        args = marshal.dense_args(H, z, R, 3 + 2 * self._e.N, gate, wrap_deg)            # the one set of arrays: sent, then logged from
        res = self._e._observe_dense(args)
        if self.log is not None:
            Hv, k, zv, Rv, wrap, g = args[:6]
            self.log.record_dense_observation(Hv, zv, Rv.reshape(k, k).T, g, None if wrap is None else list(wrap))
        return res

    def dense_innovation(self, H, z, R, wrap_deg=None):
        """What observe_dense would report (the same dict, no gate read), with nothing changed beyond the flush; an irregular S is
        reported in 'outcome' and 'bad_row', not raised (Engine.dense_innovation; ekf_observe_dense_innovation).  Nothing is logged."""
        return self._e.dense_innovation(H, z, R, wrap_deg)

    @staticmethod
    def _dense_gate(who, p, dof):
        """The gate of a policy below: +inf (p None), or the chi-square quantile of probability p for dof rows."""
        if p is None:
            return float("inf")
        if not 0.0 < float(p) < 1.0:
            raise ValueError("%s: p lies strictly between 0 and 1, or is None for no gate" % who)
        return chi2_quantile(p, dof)

    def fix_centroid(self, idx, z, R, p=None):
        """A position fix of the CENTROID of the landmarks idx (0-based, distinct, as cross_covariance takes them): the two rows
        mean(l_i) = z +- R (2 x 2) as ONE observe_dense call -- a GPS fix of a surveyed group.  p: applied only if d2 stays below the
        chi-square quantile of that probability for 2 rows (None: no gate).  Returns observe_dense's dict."""
        cols = self._state_columns("fix_centroid", idx)
        w = 1.0 / (cols.size // 2)
        rows = [{int(c): w for c in cols[0::2]}, {int(c): w for c in cols[1::2]}]
        return self.observe_dense(rows, z, R, self._dense_gate("fix_centroid", p, 2))

    def constrain_displacements(self, pairs, deltas, R, p=None):
        """Up to 8 displacement constraints l_i - l_j = delta +- R between landmark pairs (i, j) (0-based, i != j) as ONE joint update,
        the joint form of constrain_landmarks -- a fiducial board, the corners of a building.  deltas: one (dx, dy) per pair; R:
        2 m x 2 m over the stacked rows (pair 0's x, pair 0's y, pair 1's x, ...), or one 2 x 2 block that every pair shares.  p:
        as for fix_centroid, for 2 m rows.  Returns observe_dense's dict."""
        who = "constrain_displacements"
        pairs = [tuple(self._landmark_numbers(who, *pr)) for pr in pairs]
        m, N = len(pairs), self._e.N
        if not 1 <= m <= 8 or any(len(pr) != 2 or pr[0] == pr[1] or not (0 <= pr[0] < N and 0 <= pr[1] < N) for pr in pairs):
            raise ValueError("%s: 1 to 8 pairs (i, j) of different landmarks 0 .. N - 1" % who)
        d = np.asarray(deltas, dtype=np.float64)
        if d.size != 2 * m:
            raise ValueError("%s: one (dx, dy) per pair" % who)
        Ra = np.asarray(R, dtype=np.float64)
        if Ra.size == 4 and m > 1:
            Ra = np.kron(np.eye(m), Ra.reshape(2, 2))
        rows = [{3 + 2 * i + r: 1.0, 3 + 2 * j + r: -1.0} for i, j in pairs for r in (0, 1)]
        return self.observe_dense(rows, d.reshape(-1), Ra, self._dense_gate(who, p, 2 * m))

    def condition_on(self, idx, values, p=None):
        """The map CONDITIONED on up to 8 landmarks idx (0-based, distinct) whose positions became known exactly: l_i = values[i] with
        R = 0, ONE observe_dense call.  Afterwards those landmarks' rows of P are zero (to rounding), so P is no longer positive
        definite (factor_map says where) and the other landmarks carry their conditional covariance.  p: as for fix_centroid, for 2 m
        rows.  Returns observe_dense's dict."""
        cols = self._state_columns("condition_on", idx)
        if cols.size > 16:
            raise ValueError("condition_on: at most 8 landmarks")
        v = np.asarray(values, dtype=np.float64).reshape(-1)
        if v.size != cols.size:
            raise ValueError("condition_on: one (x, y) per landmark")
        return self.observe_dense([{int(c): 1.0} for c in cols], v, np.zeros((cols.size, cols.size)), self._dense_gate("condition_on", p, cols.size))

    def fuse_duplicates(self, gate, R=None, max_merges=None):
        """The SIMPLEST complete fusion policy, not the fastest: repeat { search; take the candidate with the smallest (d2, i) at or
        below `gate`; merge_landmarks(keep=j, drop=i, R) } until none is left or `max_merges` merges were made.  One search plus
        one merge per fusion (every merge changes P, hence every d2); batching disjoint pairs from one search is not built.
        Returns the merges made as [(keep, drop, d2)], 1-based numbers as they were when each merge was made.  Every merge goes
        through merge_landmarks, so an attached trajectory log records it."""
        merges = []
        while max_merges is None or len(merges) < max_merges:
            cand = self.duplicate_candidates(gate, R)
            if not cand:
                break
            i, j, d2 = cand[0]
            self.merge_landmarks(j, i, R)
            merges.append((j, i, d2))
        return merges

    def fuse_duplicates_batched(self, gate, R=None, max_merges=None):
        """fuse_duplicates with the pairs of one search fused in ONE call: repeat { search; select_merge_batch; one
        merge_landmarks_batch } until no candidate is left or `max_merges` merges were made -- a different policy from
        fuse_duplicates, which searches again after every merge: here the later pairs of a batch were gated on the state before the
        batch, and the d2 returned is the one the batch call reported (under the state after the batch's earlier pairs).
        Returns [(keep, drop, d2)], 1-based numbers as they were when their batch was made."""
        merges = []
        while max_merges is None or len(merges) < max_merges:
            limit = L.EKF_MERGE_BATCH_MAX if max_merges is None else min(L.EKF_MERGE_BATCH_MAX, max_merges - len(merges))
            batch = select_merge_batch(self.duplicate_candidates(gate, R), limit)
            if not batch:
                break
            d2 = self.merge_landmarks_batch([(k, d) for k, d, _ in batch], R)
            merges.extend((k, d, float(v)) for (k, d, _), v in zip(batch, d2))
        return merges

    def join_map(self, local, signature_offset=0.0):
        """Join the map of `local` -- another filter of this layer (or an Engine) that was started at this one's robot pose, typically with
        x = 0 and P = 0 at the moment this one stopped moving, and is independent of it -- into this one, on the device: the robot
        composes with the local robot, the local landmarks are appended behind this map's in the global frame with signature
        s_local + signature_offset, and the local map's own cross-covariances are kept (P' = J blockdiag(P, PL) J').  A synchronising
        call on both; `local` is left as it was and may be dropped at once.  Returns the 1-based numbers of the new landmarks
        (ekf_join_map).  The reference has no such method."""
        le = local._e if isinstance(local, _EkfBase) else local
        if not isinstance(le, Engine):
            raise TypeError("join_map: the local map is a filter of this layer or an Engine")
        offset = marshal.join_offset(signature_offset)                     # the one value: sent, then logged from
        first = self._e._join_map(le, offset)
        M = self._e.N - first
        if self.log is not None:
            self.log.record_map_join(le.get_x(), le.get_s(), le.get_P(), offset.value)     # (read once, after the call's flush)
        return [first + b + 1 for b in range(M)]

    def join_submap(self, local, gate=None, R=None, signature_offset=0.0):
        """The map-joining POLICY: join_map(local, signature_offset), then, when `gate` is given, fuse_duplicates_batched(gate, R) -- the
        landmarks both maps saw are found by the search and fused.  Returns (the 1-based numbers the new landmarks had right after the
        join, the fused pairs [(keep, drop, d2)] as fuse_duplicates_batched reports them).  Both halves go through logged methods."""
        new = self.join_map(local, signature_offset)
        fused = self.fuse_duplicates_batched(gate, R) if gate is not None else []
        return new, fused

    @classmethod
    def _around(cls, e):
        """A filter of this class around an engine that exists already (extract_map's destination)."""
        f = cls.__new__(cls)
        f._e, f.landmark_list, f.observed, f.log = e, None, None, None
        if cls._mode == "uc":
            f.correspondence = Correspondence(e.cfg.s_cost, e.cfg.s_thresh, 'EKF_SLAM_UC')
        return f

    def extract_map(self, idx, frame="map", **engine_kw):
        """The robot and landmarks idx (1-based, a number or any iterable, distinct, any order) taken out into a NEW filter of this class:
        its landmark k is landmark idx[k] of this one.  frame="map": their joint Gaussian as it is, bit for bit; frame="robot": the
        landmarks relative to the robot with the robot's own uncertainty folded in, the new filter's robot at zero with P = 0 -- a
        planner's small relative covariance, and what join_map expects of a local map.  O(m^2) on the device whatever the size of this
        map; this filter is only flushed, so nothing is logged.  `engine_kw` go to the new engine (tile, storage, capacity, ...; by
        default capacity max(m, 1) and this engine's storage kind) (ekf_extract_map).  The reference has no such method."""
        numbers = self._landmark_numbers("extract_map", *np.asarray(idx).reshape(-1))
        args = marshal.extract_args([i - 1 for i in numbers], frame)             # the one marshal: 0-based from here on
        return type(self)._around(self._e._extract_map(args, None, engine_kw))

    def landmarks_near_robot(self, radius):
        """The 1-based numbers of the landmarks within `radius` of the robot, ascending, from one read of x."""
        x = self._e.get_x()
        d = x[3:].reshape(-1, 2) - x[0:2]
        return [int(k) + 1 for k in np.nonzero(np.hypot(d[:, 0], d[:, 1]) <= float(radius))[0]]

    def split_submap(self, idx, frame="map", **engine_kw):
        """The archive-before-remove POLICY: extract_map(idx, frame), then remove_landmarks(idx) on this filter.  Returns the new filter
        that holds what was taken out.  The extraction changes nothing here, so the log holds the removal alone."""
        sub = self.extract_map(idx, frame, **engine_kw)
        self.remove_landmarks(idx)
        return sub

    def _transform(self, frame, t, Sigma):
        args = marshal.transform_args(frame, t, Sigma)                     # the one marshal: sent, then logged from
        self._e._transform_map(args)
        if self.log is not None:
            self.log.record_map_transform(frame, args[1], None if args[2] is None else args[2].reshape(3, 3, order="F"))

    def transform_map(self, t, Sigma=None):
        """Move the whole map by the rigid transform t = (tx, ty, phi in degrees), in place on the device: the robot becomes t (+) r, every
        landmark t_xy + Rot(phi) l, and P' = T P T' + A Sigma A' with Sigma the 3 x 3 covariance of t itself (None: an exact transform,
        the rotation alone) -- georeferencing a finished map into a surveyed frame.  The filter keeps its engine, its log and its
        landmark numbers (ekf_transform_map, EKF_FRAME_MAP).  The reference has no such method."""
        self._transform("map", t, Sigma)

    def recenter_on_robot(self):
        """Re-anchor the whole filter at the robot: its pose becomes the origin with P(robot, .) = 0 and every landmark is expressed
        relative to it, the robot's uncertainty folded into the landmarks -- the robocentric remedy for EKF-SLAM's inconsistency, and
        the shape join_map expects of a local map (ekf_transform_map, EKF_FRAME_ROBOT).  The reference has no such method."""
        self._transform("robot", None, None)

    def align_to_anchors(self, numbers, positions, Sigma=None):
        """The georeferencing POLICY: the closed-form 2-D rigid least-squares fit (rotation and translation, no scale) of the current
        estimates of landmarks `numbers` (1-based, at least two) onto their surveyed `positions` (one row each), on the host, then ONE
        transform_map(t, Sigma) through the logged method.  Returns (t, the rms residual of the fit)."""
        numbers = self._landmark_numbers("align_to_anchors", *np.asarray(numbers).reshape(-1))
        q = np.asarray(positions, dtype=np.float64).reshape(-1, 2)
        if len(numbers) < 2 or q.shape[0] != len(numbers):
            raise ValueError("align_to_anchors: at least two landmarks, one surveyed position each")
        x = self._e.get_x()
        p = np.array([x[3 + 2 * (i - 1):5 + 2 * (i - 1)] for i in numbers])
        pc, qc = p - p.mean(axis=0), q - q.mean(axis=0)
        phi = np.arctan2(np.sum(pc[:, 0] * qc[:, 1] - pc[:, 1] * qc[:, 0]), np.sum(pc[:, 0] * qc[:, 0] + pc[:, 1] * qc[:, 1]))
        c, s = np.cos(phi), np.sin(phi)
        Rot = np.array([[c, -s], [s, c]])
        txy = q.mean(axis=0) - Rot @ p.mean(axis=0)
        t = np.array([txy[0], txy[1], np.degrees(phi)])
        rms = float(np.sqrt(np.mean(np.sum((p @ Rot.T + txy - q) ** 2, axis=1))))
        self.transform_map(t, Sigma)
        return t, rms

    def observe_linear(self, z, R, Hr=None, landmarks=(), Hl=(), gate=float("inf"), wrap=(0, 0), rows=2, wait=False):
        """'H x was observed as z with noise covariance R' for a constant H: the 2 x 3 block Hr on the robot state (x, y, theta in
        degrees) plus one 2 x 2 block Hl[b] on each of up to two landmarks (1-based numbers) -- the exact Kalman update, as an
        UPDATE-STEP: it enters the pending ring like a correction of measure(), flushes nothing and, unless wait=True, waits for
        nothing.  Applied only if d2 = nu' S^-1 nu <= gate; rows named in `wrap` are angles in degrees whose innovation is wrapped
        into (-180, 180]; rows=1 is a scalar observation.  wait=True returns {'nu', 'S', 'd2', 'outcome'} (ekf_observe_linear).
        The reference has no such method."""
        lms = self._landmark_numbers("observe_linear", *list(landmarks))
        rows = int(rows)
        if rows not in (1, 2):
            raise ValueError("observe_linear: rows is 1 or 2")
        obs = marshal.linear_obs(z, R, Hr, [k - 1 for k in lms], Hl, gate, wrap, rows)      # the one struct: sent, then logged from
        out = self._e._observe("ekf_observe_linear", obs, wait)
        if self.log is not None:
            Rm = np.array(obs.R[:]).reshape(2, 2, order="F")
            Hrm = np.array(obs.Hr[:]).reshape(2, 3, order="F")
            blocks = [np.array(obs.Hl[b][:]).reshape(2, 2, order="F") for b in range(len(lms))]
            self.log.record_observation(np.array(obs.z[:]), Rm, Hrm, lms, blocks, gate, wrap, rows)
        return out

    def linear_innovation(self, z, R, Hr=None, landmarks=(), Hl=(), gate=float("inf"), wrap=(0, 0), rows=2):
        """{'nu', 'S', 'd2', 'outcome'} observe_linear(..., wait=True) would report now (1-based landmarks); changes and flushes
        nothing (ekf_linear_innovation)."""
        lms = self._landmark_numbers("linear_innovation", *list(landmarks))
        return self._e.linear_innovation(z, R, Hr, [k - 1 for k in lms], Hl, gate, wrap, rows)

    def linear_rejections(self):
        """(irregular, gated): observe_linear calls since the last look that did not apply; resets the counts."""
        return self._e.linear_rejections()

    def fix_landmark(self, i, pos, R, gate=float("inf"), wait=False):
        """'Landmark i (1-based) is the surveyed point pos, known to within the covariance R': H = I2 on that landmark."""
        (i,) = self._landmark_numbers("fix_landmark", i)
        return self.observe_linear(_vec(pos, 2), R, None, [i], [np.eye(2)], gate=gate, wait=wait)

    def fix_robot_position(self, pos, R, gate=float("inf"), wait=False):
        """'The robot is at pos, to within the covariance R' (a GPS fix): Hr = [I2 0]."""
        return self.observe_linear(_vec(pos, 2), R, np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), gate=gate, wait=wait)

    def fix_robot_heading(self, theta_deg, var, gate=float("inf"), wait=False):
        """'The heading reads theta_deg (degrees), with variance var' (a compass): one row, Hr(0, 2) = 1, the innovation wrapped
        into (-180, 180]."""
        return self.observe_linear([float(theta_deg)], [[float(var), 0.0], [0.0, 0.0]], np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 0.0]]),
                                   gate=gate, wrap=(1, 0), rows=1, wait=wait)

    def observe_model(self, model, z, R, landmarks=(), anchor=None, gate=float("inf"), wait=False, iterations=1, tol=0.0):
        """'h(x) was observed as z with noise covariance R' for one of the models EKF_MODEL_* of include/ekfslam.h -- range and
        bearing (1), range (2), bearing (3), the target's position in the robot frame (4), the distance between two landmarks (5) --
        linearised on the device at the live state, the bearing innovation wrapped.  landmarks: the 1-based target (two for model 5);
        anchor: a known point outside the map as the target instead (only the robot is corrected).  An UPDATE-STEP like
        observe_linear: flushes nothing and, unless wait=True, waits for nothing; applied only if d2 <= gate.  wait=True returns
        {'nu', 'S', 'd2', 'outcome'} (ekf_observe_model).  iterations > 1 (or a tol > 0) relinearises: observe_model_iterated.  The
        reference has no such method."""
        if int(iterations) != 1 or float(tol) != 0.0:
            return self.observe_model_iterated(model, z, R, landmarks, anchor, gate, iterations, tol, wait)
        lms = self._landmark_numbers("observe_model", *list(landmarks))
        obs = marshal.model_obs(model, z, R, [k - 1 for k in lms], anchor, gate)           # the one struct: sent, then logged from
        out = self._e._observe("ekf_observe_model", obs, wait)
        if self.log is not None:
            self.log.record_model_observation(*self._logged_model_obs(obs, lms), gate)
        return out

    @staticmethod
    def _logged_model_obs(obs, lms):
        """What the log holds of a model observation's struct: model, z, R (2 x 2), the 1-based landmarks, the anchor or None."""
        return obs.model, np.array(obs.z[:]), np.array(obs.R[:]).reshape(2, 2, order="F"), lms, None if lms else np.array(obs.anchor[:])

    def model_innovation(self, model, z, R, landmarks=(), anchor=None, gate=float("inf")):
        """{'nu', 'S', 'd2', 'outcome'} observe_model(..., wait=True) would report now (1-based landmarks); changes and flushes
        nothing (ekf_model_innovation)."""
        lms = self._landmark_numbers("model_innovation", *list(landmarks))
        return self._e.model_innovation(model, z, R, [k - 1 for k in lms], anchor, gate)

    def observe_model_iterated(self, model, z, R, landmarks=(), anchor=None, gate=float("inf"), iterations=3, tol=0.0, wait=False):
        """observe_model as the ITERATED EKF update: h is relinearised up to `iterations` times (1..16) on the device -- Gauss-Newton on
        the MAP cost over the robot and the target(s) -- until no entry moves by more than tol, and the last linearisation makes the
        step's one pair.  Worth it where the prior is wide against the sensor: a new landmark, a heading known to ten degrees, a precise
        fix.  One launch, no flush, like observe_model; the gate is read at the first linearisation.  wait=True returns observe_model's
        dict (the first linearisation's) with 'iterated': {'S', 'nu', 'used', 'converged', 'last_step', 'x_local'}
        (ekf_observe_model_iterated).  The reference has no such method."""
        lms = self._landmark_numbers("observe_model_iterated", *list(landmarks))
        obs = marshal.model_obs(model, z, R, [k - 1 for k in lms], anchor, gate)           # the one struct: sent, then logged from
        out = self._e._observe_iterated("ekf_observe_model_iterated", obs, iterations, tol, wait)
        if self.log is not None:
            self.log.record_model_observation_iterated(*self._logged_model_obs(obs, lms), gate, iterations, tol)
        return out

    def model_innovation_iterated(self, model, z, R, landmarks=(), anchor=None, gate=float("inf"), iterations=3, tol=0.0):
        """What observe_model_iterated(..., wait=True) would report now (1-based landmarks); changes and flushes nothing
        (ekf_model_innovation_iterated)."""
        lms = self._landmark_numbers("model_innovation_iterated", *list(landmarks))
        return self._e.model_innovation_iterated(model, z, R, [k - 1 for k in lms], anchor, gate, iterations, tol)

    def observe_range_bearing(self, i, z, R, gate=float("inf"), wait=False, iterations=1, tol=0.0):
        """'Landmark i (1-based) is seen at range z[0] and bearing z[1] (degrees, relative to the heading), covariance R'."""
        return self.observe_model(L.EKF_MODEL_RANGE_BEARING, _vec(z, 2), R, [i], gate=gate, wait=wait,
                                  iterations=iterations, tol=tol)

    def observe_range(self, i, r, var, gate=float("inf"), wait=False, iterations=1, tol=0.0):
        """'Landmark i is at distance r, with variance var' (a range-only beacon)."""
        return self.observe_model(L.EKF_MODEL_RANGE, [float(r)], [[float(var), 0.0], [0.0, 0.0]], [i], gate=gate, wait=wait,
                                  iterations=iterations, tol=tol)

    def observe_bearing(self, i, deg, var, gate=float("inf"), wait=False, iterations=1, tol=0.0):
        """'Landmark i is seen at bearing deg (degrees, relative to the heading), with variance var' (a camera)."""
        return self.observe_model(L.EKF_MODEL_BEARING, [float(deg)], [[float(var), 0.0], [0.0, 0.0]], [i], gate=gate, wait=wait,
                                  iterations=iterations, tol=tol)

    def observe_relative_xy(self, i, z, R, gate=float("inf"), wait=False, iterations=1, tol=0.0):
        """'Landmark i lies at z = (forward, left) in the robot frame, covariance R' (a lidar or stereo front end)."""
        return self.observe_model(L.EKF_MODEL_RELATIVE_XY, _vec(z, 2), R, [i], gate=gate, wait=wait,
                                  iterations=iterations, tol=tol)

    def observe_landmark_range(self, i, j, dist, var, gate=float("inf"), wait=False, iterations=1, tol=0.0):
        """'Landmarks i and j are dist apart, with variance var' (a tape measure between two beacons)."""
        return self.observe_model(L.EKF_MODEL_LANDMARK_RANGE, [float(dist)], [[float(var), 0.0], [0.0, 0.0]], [i, j], gate=gate, wait=wait,
                                  iterations=iterations, tol=tol)

    def observe_anchor_range(self, pos, r, var, gate=float("inf"), wait=False, iterations=1, tol=0.0):
        """'The known point pos, which is not in the map, is at distance r, with variance var' (a surveyed UWB anchor)."""
        return self.observe_model(L.EKF_MODEL_RANGE, [float(r)], [[float(var), 0.0], [0.0, 0.0]], anchor=_vec(pos, 2), gate=gate, wait=wait,
                                  iterations=iterations, tol=tol)

    def observe_anchor_bearing(self, pos, deg, var, gate=float("inf"), wait=False, iterations=1, tol=0.0):
        """'The known point pos, which is not in the map, is seen at bearing deg, with variance var'."""
        return self.observe_model(L.EKF_MODEL_BEARING, [float(deg)], [[float(var), 0.0], [0.0, 0.0]], anchor=_vec(pos, 2), gate=gate, wait=wait,
                                  iterations=iterations, tol=tol)

    def add_landmarks_model(self, entries):
        """One scan of NEW landmarks under observe_model's conventions: entries = [(model, z, R), ...] or [(model, z, R, signature),
        ...] with model EKF_MODEL_RANGE_BEARING (1: z = range, bearing in degrees relative to the heading) or EKF_MODEL_RELATIVE_XY (4:
        z = (forward, left) in the robot frame) -- a one-row model does not determine a point.  Every entry is inverted on the device at
        the live robot state and the whole scan is appended by one launch (ekf_append_model); waits for nothing, flushes nothing.  A
        signature left out (or None) is the landmark's own 1-based number.  Returns the 1-based numbers of the new landmarks.  The
        reference has no such method: its append takes the position from the caller's table."""
        entries = [tuple(e) for e in entries]
        if not 1 <= len(entries) <= L.EKF_APPEND_MODEL_MAX:
            raise ValueError("add_landmarks_model: between 1 and %d entries" % L.EKF_APPEND_MODEL_MAX)
        N = self._e.N
        full = []
        for b, e in enumerate(entries):
            if len(e) not in (3, 4):
                raise ValueError("add_landmarks_model: an entry is (model, z, R) or (model, z, R, signature)")
            if int(e[0]) not in (L.EKF_MODEL_RANGE_BEARING, L.EKF_MODEL_RELATIVE_XY):
                raise ValueError("add_landmarks_model: model is EKF_MODEL_RANGE_BEARING (1) or EKF_MODEL_RELATIVE_XY (4)")
            full.append(e[:3] + (e[3] if len(e) == 4 and e[3] is not None else N + b + 1,))
        arr, m = marshal.model_inits(full, "add_landmarks_model")           # the shapes are checked here; the one array: sent, then logged from
        first = self._e._append_model(arr, m)
        if self.log is not None:
            self.log.record_model_append([(o.model, np.array(o.z[:]), np.array(o.R[:]).reshape(2, 2, order="F"), o.signature) for o in arr[:m]])
        return [first + b + 1 for b in range(m)]

    def predict_model(self, steps):
        """Motion under observe_model's conventions: one step (model, u, M) or a list of them, model EKF_MOTION_TURN_DRIVE (1: u = (d, deg)
        -- turn, then drive), EKF_MOTION_ARC (2: u = (arc length, deg)) or EKF_MOTION_POSE_DELTA (3: u = (dx, dy, deg) in the robot frame);
        M the covariance of u.  x_r' = f(x_r, u) and P' = F P F' + V M V' with the true Jacobians (theta in degrees: the factor pi/180
        where it belongs), the whole list in one launch; waits for nothing, flushes nothing (ekf_predict_model).
        The reference has no such method: its predict keeps F at the pre-motion heading without pi/180 and a rank-one Q, and stays."""
        steps = list(steps)
        if len(steps) == 3 and np.isscalar(steps[0]):          # one step
            steps = [tuple(steps)]
        if not 1 <= len(steps) <= L.EKF_PREDICT_MODEL_MAX:
            raise ValueError("predict_model: between 1 and %d steps" % L.EKF_PREDICT_MODEL_MAX)
        arr, m = marshal.motions(steps, known_models=True)                  # the shapes are checked here; the one array: sent, then logged from
        self._e._predict_model(arr, m)
        if self.log is not None:
            sizes = [L.EKF_MOTION_INPUTS[o.model] for o in arr[:m]]   # u and M of the size the model reads
            self.log.record_model_predict([(o.model, np.array(o.u[:nu]), np.array(o.M[:]).reshape(3, 3, order="F")[:nu, :nu])
                                           for o, nu in zip(arr[:m], sizes)])

    @staticmethod
    def _motion_steps(model, cols, M):
        """One step from scalars, or a list of steps from equally long sequences (M: one matrix for all, or one per step)."""
        cols = [np.asarray(c, dtype=np.float64) for c in cols]
        if all(c.ndim == 0 for c in cols):
            return [(model, [float(c) for c in cols], M)]
        cols = [c.reshape(-1) for c in cols]
        m = cols[0].size
        if any(c.size != m for c in cols):
            raise ValueError("predict_model: the inputs of a list of steps are equally long")
        Ma = np.asarray(M, dtype=np.float64)
        Ms = [Ma[b] for b in range(m)] if Ma.ndim == 3 and Ma.shape[0] == m else [Ma] * m
        return [(model, [float(c[b]) for c in cols], Ms[b]) for b in range(m)]

    def predict_turn_drive(self, d, deg, M):
        """'The robot turned by deg degrees, then drove d; (d, deg) has the covariance M' -- one step, or a list of them from equally long
        sequences.  The reference has no such method: this is its f with the true Jacobians."""
        self.predict_model(self._motion_steps(L.EKF_MOTION_TURN_DRIVE, (d, deg), M))

    def predict_arc(self, d, deg, M):
        """'The robot drove an arc of length d while turning by deg degrees; (d, deg) has the covariance M' -- what wheel odometry
        integrates to over one increment; one step or a list.  The reference has no such method."""
        self.predict_model(self._motion_steps(L.EKF_MOTION_ARC, (d, deg), M))

    def predict_pose_delta(self, dx, dy, deg, M):
        """'The pose changed by (dx, dy, deg) in the robot frame, with covariance M (3 x 3)' -- a scan matcher's or integrated odometry's
        increment; with zeros, additive noise M in the robot frame; one step or a list.  The reference has no such method."""
        self.predict_model(self._motion_steps(L.EKF_MOTION_POSE_DELTA, (dx, dy, deg), M))

    def add_landmark_range_bearing(self, z, R, signature=None):
        """'A landmark that is not in the map yet is seen at range z[0] and bearing z[1] (degrees, relative to the heading), covariance
        R': it joins the map at the point that observation names.  Returns its 1-based number."""
        return self.add_landmarks_model([(L.EKF_MODEL_RANGE_BEARING, z, R, signature)])[0]

    def add_landmark_relative_xy(self, z, R, signature=None):
        """'A landmark that is not in the map yet lies at z = (forward, left) in the robot frame, covariance R'.  Returns its 1-based
        number."""
        return self.add_landmarks_model([(L.EKF_MODEL_RELATIVE_XY, z, R, signature)])[0]

    def associate_model(self, entries, want_d2=False):
        """WHICH landmark each sighting of a scan belongs to, under observe_model's conventions: entries = [{'model', 'z', 'R', 'gate'},
        ...] (models 1-4; a gate left out is +inf).  Returns {'best', 'second', 'd2_best', 'd2_second', 'within_gate', 'irregular'} with
        one entry per observation: the 1-based landmarks with the smallest and second-smallest d2 (0 = none, d2 = +inf), how many
        landmarks lie at or below the gate, how many have no d2.  Every d2 is what model_innovation reports for that pair, bit for bit;
        want_d2 adds 'd2_all' (m x N).  One small launch for the whole scan against the whole map; changes and flushes nothing, so it is
        not logged (ekf_associate_model).  The reference has no such method: its association keeps its own conventions."""
        res = dict(self._e.associate_model(entries, want_d2))
        res["best"] = res["best"] + 1
        res["second"] = res["second"] + 1
        return res

    def measure_model(self, entries, gate_match, gate_new, wait=False):
        """One scan under observe_model's conventions, observe-or-append: entries as for add_landmarks_model ([(model, z, R) or (model, z,
        R, signature), ...], models 1 and 4).  ONE associate_model call with gate = gate_match, then, on the host and deterministic:
          matched    exactly one landmark lies inside gate_match (within_gate == 1): that landmark, the entry's best;
          new        d2_best > gate_new, or the map is empty (gate_new >= gate_match is required);
          discarded  everything else: ambiguous (several inside the gate) or between the two gates.
        Where several entries are matched to one landmark the smallest d2_best keeps it (the lower entry on a tie) and the others are
        discarded.  The matched entries go to observe_model(..., [landmark], gate=gate_match) in scan order -- the step checks its gate
        again at the live state -- then ALL new ones to one add_landmarks_model call.  Returns [(kind, landmark)] per entry, landmark
        1-based and 0 for a discarded one.  Everything that changes the state goes through those two logged methods, so a replayed log
        reproduces the run.  Unsharded handles only, as observe_model."""
        gate_match, gate_new = float(gate_match), float(gate_new)
        if not gate_new >= gate_match:
            raise ValueError("measure_model: gate_new >= gate_match is required (and neither is NaN)")
        entries, scan = self._measure_scan("measure_model", entries, L.EKF_ASSOCIATE_MODEL_MAX, gate_match)
        res = self._e.associate_model(scan)
        kinds = []
        for k in range(len(entries)):
            if int(res["within_gate"][k]) == 1:
                kinds.append("matched")
            elif int(res["best"][k]) < 0 or float(res["d2_best"][k]) > gate_new:
                kinds.append("new")
            else:
                kinds.append("discarded")
        owner = {}                       # landmark -> the matched entry that keeps it: smallest d2_best, the lower entry on a tie
        for k, kind in enumerate(kinds):
            if kind == "matched":
                lm = int(res["best"][k])
                if lm not in owner or float(res["d2_best"][k]) < float(res["d2_best"][owner[lm]]):
                    owner[lm] = k
        return self._measure_carry_out(entries, kinds, {k: lm for lm, k in owner.items()}, gate_match, wait)

    def assign_model(self, entries, want_candidates=False):
        """WHICH observation of a scan gets WHICH landmark when they compete: the one-to-one assignment that minimises the summed d2, with
        the entry's gate as the price of leaving it out (entries as for associate_model, every gate finite).  Returns 'landmark' (1-based,
        0 = left out), 'd2', 'ncand', 'total', associate_model's six keys ('best' and 'second' 1-based, 0 = none) and, with
        want_candidates, 'cand' / 'cand_d2' (m x EKF_ASSIGN_CANDIDATES, 1-based, 0 behind a row's ncand entries).  Changes and flushes
        nothing, so it is not logged (ekf_assign_model).  The reference has no such method."""
        res = dict(self._e.assign_model(entries, want_candidates))
        for key in ("landmark", "best", "second") + (("cand",) if want_candidates else ()):
            res[key] = res[key] + 1
        return res

    def measure_model_assigned(self, entries, gate_match, gate_new, wait=False, device_apply=False):
        """measure_model with the ambiguity discard replaced by the global-nearest-neighbour ASSIGNMENT: entries, gate_match, gate_new and
        wait as there.  ONE assign_model call with gate = gate_match, then per entry
          matched    it has an assigned landmark;
          new        no landmark lies inside gate_match (ncand == 0) and d2_best > gate_new, or the map is empty;
          discarded  everything else: left out by the assignment although a landmark was inside its gate, or between the two gates.
        The matched entries go to observe_model(..., [landmark], gate=gate_match) in scan order, then ALL new ones to one
        add_landmarks_model call.  Returns [(kind, landmark)] per entry as measure_model.  Everything that changes the state goes through
        those two logged methods, so a replayed log reproduces the run.  Unsharded handles only, as observe_model.
        device_apply=True lets the DEVICE consume the assignment (ekf_observe_model_assigned): ONE observe_model_assigned call queues the
        assignment and a step per entry -- the matched ones applied as above, every other one a finite no-op that takes a ring slot --
        then the result is fetched: the one wait, now behind the queued steps instead of in front of them (wait is not read).  The kinds
        are the ones above, classified from WHAT THE RESULT BLOCK HOLDS, which has no match records: an entry is new where ncand == 0 and
        either the map was empty or gate_new == gate_match (ncand == 0 then says d2_best > gate_new); with gate_new > gate_match the
        d2_best of those entries alone comes from one associate_model call made AFTER the scan's steps -- at the state the new landmarks
        are started from, not the one the scan was assigned at.  Then ALL new entries go to one add_landmarks_model call.
        The log gets no new kind: the scan is recorded after the fetch through record_model_observation, one edit per entry in scan
        order -- a matched entry with its landmark and gate_match, every other one with landmark 1 and a gate of -1.0, an observe_model
        that cannot apply (d2 >= 0 > -1, or irregular) and leaves the same zero pair in the same ring slot.  A replay therefore
        reproduces x, s and P bit for bit on every storage kind and batch size; only what linear_rejections counts differs, by those
        entries.  On F64 tiles the state after a flush is the default path's bit for bit."""
        gate_match, gate_new = float(gate_match), float(gate_new)
        if not gate_new >= gate_match:
            raise ValueError("measure_model_assigned: gate_new >= gate_match is required (and neither is NaN)")
        entries, scan = self._measure_scan("measure_model_assigned", entries, L.EKF_ASSIGN_MODEL_MAX, gate_match)
        if device_apply:
            return self._measure_assigned_on_device(entries, scan, gate_match, gate_new)
        res = self._e.assign_model(scan)
        kinds, paired = [], {}
        for k in range(len(entries)):
            if int(res["landmark"][k]) >= 0:
                kinds.append("matched")
                paired[k] = int(res["landmark"][k])
            elif int(res["ncand"][k]) == 0 and (int(res["best"][k]) < 0 or float(res["d2_best"][k]) > gate_new):
                kinds.append("new")
            else:
                kinds.append("discarded")
        return self._measure_carry_out(entries, kinds, paired, gate_match, wait)

    def _measure_assigned_on_device(self, entries, scan, gate_match, gate_new):
        """measure_model_assigned(..., device_apply=True) behind its checks: the scan queued, the result fetched, the kinds, the log, the
        new landmarks."""
        arr, m = marshal.scan_obs(scan)                                     # the one array: sent, then logged from
        empty = self._e.N == 0
        self._e._observe_model_assigned(arr, m)
        res = self._e.assigned_scan_result()
        paired = {k: int(res["landmark"][k]) for k in range(m) if int(res["landmark"][k]) >= 0}
        loose = [k for k in range(m) if k not in paired and int(res["ncand"][k]) == 0]
        if loose and not empty and gate_new > gate_match:
            far = self._e.associate_model([scan[k] for k in loose])
            loose = [k for k, best, d2 in zip(loose, far["best"], far["d2_best"]) if int(best) < 0 or float(d2) > gate_new]
        if self.log is not None and not empty:                              # (an empty map: no step was queued)
            for k, o in enumerate(arr[:m]):
                z, R = np.array(o.z[:]), np.array(o.R[:]).reshape(2, 2, order="F")
                if k in paired:
                    self.log.record_model_observation(o.model, z, R, [paired[k] + 1], None, gate_match)
                else:
                    self.log.record_model_observation(o.model, z, R, [1], None, -1.0)
        out = [("matched", paired[k] + 1) if k in paired else ("discarded", 0) for k in range(m)]
        if loose:
            for k, number in zip(loose, self.add_landmarks_model([entries[k] for k in loose])):
                out[k] = ("new", number)
        return out

    @staticmethod
    def _measure_scan(who, entries, cap, gate_match):
        """The opening measure_model and measure_model_joint share: the entries as tuples, checked -- between 1 and cap of them, (model,
        z, R) or (model, z, R, signature), models 1 and 4 -- and the scan that ONE associate_model call takes, gate = gate_match."""
        entries = [tuple(e) for e in entries]
        if not 1 <= len(entries) <= cap:
            raise ValueError("%s: between 1 and %d entries" % (who, cap))
        for e in entries:
            if len(e) not in (3, 4):
                raise ValueError("%s: an entry is (model, z, R) or (model, z, R, signature)" % who)
            if int(e[0]) not in (L.EKF_MODEL_RANGE_BEARING, L.EKF_MODEL_RELATIVE_XY):
                raise ValueError("%s: model is EKF_MODEL_RANGE_BEARING (1) or EKF_MODEL_RELATIVE_XY (4): a one-row model does not start a "
                                 "landmark" % who)
        return entries, [dict(model=int(e[0]), z=e[1], R=e[2], gate=gate_match) for e in entries]

    def _measure_carry_out(self, entries, kinds, paired, gate_match, wait):
        """The close they share: entry k with a landmark in `paired` ({entry: 0-based landmark}) goes to observe_model(..., gate=gate_match),
        in scan order; then ALL entries whose kind is 'new' to one add_landmarks_model call; the rest is discarded.  Returns [(kind,
        landmark)] per entry, landmark 1-based and 0 for a discarded one."""
        out = [None] * len(entries)
        fresh = []
        for k, (kind, e) in enumerate(zip(kinds, entries)):
            if k in paired:
                self.observe_model(int(e[0]), e[1], e[2], [paired[k] + 1], gate=gate_match, wait=wait)
                out[k] = ("matched", paired[k] + 1)
            elif kind == "new":
                fresh.append(k)
            else:
                out[k] = ("discarded", 0)
        if fresh:
            for k, number in zip(fresh, self.add_landmarks_model([entries[k] for k in fresh])):
                out[k] = ("new", number)
        return out

    def joint_innovation(self, entries, hypotheses, want_prefix=True, want_nu=False, want_S=False):
        """The joint compatibility of a scan's pairings: entries as for associate_model, hypotheses nh x m with the 1-based landmark each
        observation is paired with, 0 = left out.  Returns {'d2', 'dof', 'pairings', 'outcome', 'first_irregular'} per hypothesis
        (first_irregular: the 1-based entry of the scan, 0 = none), d2 = nu' S^-1 nu over the stacked paired rows with S = H P H' +
        blockdiag(R) -- what a joint-compatibility search tests against chi2_quantile(p, dof) -- plus 'd2_prefix' (nh x m), 'nu' and 'S' by
        scan index where asked.  Changes and flushes nothing, so it is not logged (ekf_joint_innovation).  Unsharded handles only."""
        hyp = np.asarray(hypotheses, dtype=np.float64)
        if hyp.ndim != 2:
            raise ValueError("joint_innovation: hypotheses is nh x m")
        numbers = np.array(self._landmark_numbers("joint_innovation", *hyp.reshape(-1).tolist()), dtype=np.int64).reshape(hyp.shape)
        if np.any(numbers < 0):
            raise ValueError("joint_innovation: a landmark is 1-based, 0 = the observation is left out")
        res = dict(self._e.joint_innovation(entries, numbers - 1, want_prefix, want_nu, want_S))
        res["first_irregular"] = res["first_irregular"] + 1
        return res

    def joint_search(self, entries, joint_p=0.99, beam=64, want_candidates=False, want_alive=False):
        """The joint-compatibility SEARCH over a scan, on the device with one readback: entries as for assign_model (every gate finite: it
        decides what a candidate is).  Level k extends every alive hypothesis by the 4 closest candidates of entry k and by "left out"; an
        extension survives where its joint d2 <= chi2_quantile(joint_p, dof); survivors are ordered by (pairings descending, joint d2
        ascending, hypothesis ascending) and cut at beam (at most EKF_JOINT_SEARCH_BEAM_MAX).  Returns the winner's 'landmark' (1-based,
        0 = left out), 'd2', 'dof', 'pairings', 'truncated', 'nalive', 'irregular', 'tested' / 'survived' per entry, associate_model's
        keys ('best' and 'second' 1-based, 0 = none; its 'irregular' as 'match_irregular') and, where asked, 'cand' / 'cand_d2' as assign_model returns them and 'alive' /
        'alive_d2', the final beam in order (1-based, 0 = left out).  Every d2 is joint_innovation's d2_prefix for that hypothesis bit for
        bit.  Changes and flushes nothing, so it is not logged (ekf_joint_search).  Unsharded handles only.  The reference has no such
        method."""
        joint_p = float(joint_p)
        if not 0.0 < joint_p < 1.0:
            raise ValueError("joint_search: joint_p lies strictly between 0 and 1")
        entries = list(entries)
        thresholds = [chi2_quantile(joint_p, dof) for dof in range(2 * len(entries) + 1)]
        res = dict(self._e.joint_search(entries, thresholds, beam, want_candidates, want_alive))
        for key in ("landmark", "best", "second") + (("cand",) if want_candidates else ()) + (("alive",) if want_alive else ()):
            res[key] = res[key] + 1
        return res

    def observe_model_joint(self, entries, landmarks, gate=float("inf"), want_nu=False, want_S=False, iterations=1, tol=0.0):
        """One hypothesis of joint_innovation APPLIED as ONE joint update: entries as for associate_model ([{'model', 'z', 'R'}, ...],
        models 1-4), landmarks the 1-based landmark each observation is paired with, 0 = left out.  All pairings are linearised once, at
        the live state, and stacked: the update that runs is the one whose joint d2 is reported, it does not depend on scan order, and it
        costs one pass over P however many pairings there are (sequential observe_model steps relinearise after each one).  Applied only
        if the joint d2 <= gate.  The pending pairs are flushed first.  Returns {'d2', 'dof', 'pairings', 'outcome', 'first_irregular'}
        (first_irregular 1-based, 0 = none) plus 'nu' and 'S' by scan index where asked; a pairing with no d2 raises EkfError and
        changes nothing (ekf_observe_model_joint).  iterations > 1 relinearises the whole scan up to that many times (Gauss-Newton over
        the robot and the paired landmarks, stopping where no entry moves by more than tol), applies the last linearisation -- the gate
        and the dict are the first one's -- and adds 'used', 'converged', 'step' (ekf_observe_model_joint_iterated).  Unsharded handles
        only.  The reference has no such method."""
        numbers = self._landmark_numbers("observe_model_joint", *list(landmarks))
        if any(k < 0 for k in numbers):
            raise ValueError("observe_model_joint: a landmark is 1-based, 0 = the observation is left out")
        arr, m = marshal.scan_obs(entries)                                  # the one array: sent, then logged from
        iterated = iterations != 1
        res = dict(self._e._observe_joint(arr, m, [k - 1 for k in numbers], gate, want_nu, want_S, *((iterations, tol) if iterated else ())))
        res["first_irregular"] = res["first_irregular"] + 1
        if self.log is not None:
            logged = [(o.model, np.array(o.z[:]), np.array(o.R[:]).reshape(2, 2, order="F"), k) for o, k in zip(arr[:m], numbers)]
            if iterated:
                self.log.record_model_observation_joint_iterated(logged, gate, iterations, tol)
            else:
                self.log.record_model_observation_joint(logged, gate)
        return res

    def measure_model_joint(self, entries, gate_match, gate_new, joint_p=0.99, beam=64, wait=False, joint_update=False,
                            device_candidates=False, joint_iterations=1, joint_tol=0.0, device_search=False):
        """measure_model with the ambiguity discard replaced by a JOINT-compatibility search: entries, gate_match, gate_new and wait as
        there.  ONE associate_model(..., want_d2=True) call: the candidates of an entry are the landmarks with individual d2 <= gate_match,
        at most the 4 closest (by (d2, landmark)); an entry without a candidate is new where d2_best > gate_new (or the map is empty) and
        discarded otherwise.  Then a level-synchronous branch and bound over the entries that have candidates, in scan order: at level k
        every surviving partial hypothesis is extended by each candidate of entry k it has not used yet and by "left out", ALL extensions
        of a level go to ONE joint_innovation call, and an extension survives where its prefix d2 <= chi2_quantile(joint_p, dof).  Where
        more than `beam` survive, the best by (pairings descending, joint d2 ascending, hypothesis ascending) are kept.  The winner is the
        survivor first in that order: its pairings go to observe_model(..., gate=gate_match) in scan order, then ALL new entries to one
        add_landmarks_model call; the rest is discarded.  Returns ([(kind, landmark)] per entry as measure_model, whether the beam cut
        the search).  Everything that changes the state goes through those two logged methods, so a replayed log reproduces the run.
        joint_update=True applies the winner's pairings by ONE observe_model_joint(gate=inf) call instead -- the update whose joint d2 the
        search tested, one pass over P -- which is logged as well; joint_iterations > 1 (read only with joint_update=True) relinearises
        that update up to so many times, stopping at joint_tol (observe_model_joint's iterations and tol).  device_candidates=True takes the candidates and the best d2 from ONE
        assign_model(want_candidates=True) call instead: the same landmarks in the same order, so the outcome and the log are the same,
        and the m x N matrix does not come back to the host.  device_search=True lets the DEVICE walk the search: ONE joint_search call
        (gate = gate_match, thresholds chi2_quantile(joint_p, dof)) replaces both the candidate call and the level loop -- the same
        candidates, tests and order, every d2 the same bits, so the winner, `truncated`, the state and the log are the default path's; the
        kinds come from its match records (an entry has candidates where within_gate > 0).  beam is then at most
        EKF_JOINT_SEARCH_BEAM_MAX (ValueError); device_candidates is not read."""
        gate_match, gate_new, joint_p = float(gate_match), float(gate_new), float(joint_p)
        if not gate_new >= gate_match:
            raise ValueError("measure_model_joint: gate_new >= gate_match is required (and neither is NaN)")
        if not 0.0 < joint_p < 1.0:
            raise ValueError("measure_model_joint: joint_p lies strictly between 0 and 1")
        if int(beam) != beam or beam < 1:
            raise ValueError("measure_model_joint: beam is a whole number >= 1")
        entries, scan = self._measure_scan("measure_model_joint", entries, L.EKF_JOINT_MAX, gate_match)
        if device_search:
            if beam > L.EKF_JOINT_SEARCH_BEAM_MAX:
                raise ValueError("measure_model_joint: with device_search the beam is at most EKF_JOINT_SEARCH_BEAM_MAX")
            res = self._e.joint_search(scan, [chi2_quantile(joint_p, dof) for dof in range(2 * len(entries) + 1)], int(beam))
            kinds = ["search" if int(res["within_gate"][k]) > 0 else
                     "new" if int(res["best"][k]) < 0 or float(res["d2_best"][k]) > gate_new else "discarded" for k in range(len(entries))]
            winner = {k: int(lm) for k, lm in enumerate(res["landmark"]) if int(lm) >= 0}
            return self._measure_joint_close(entries, kinds, winner, res["truncated"], gate_match, wait, joint_update, joint_iterations, joint_tol)
        res = self._e.assign_model(scan, want_candidates=True) if device_candidates else self._e.associate_model(scan, want_d2=True)
        cands, kinds = [], []
        for k in range(len(entries)):
            if device_candidates:
                cands.append([int(i) for i in res["cand"][k][:min(4, int(res["ncand"][k]))]])          # (already ordered by (d2, landmark))
            else:
                row = np.asarray(res["d2_all"][k], dtype=np.float64)
                inside = sorted((float(row[i]), int(i)) for i in np.flatnonzero(row <= gate_match))   # (NaN compares false: never a candidate)
                cands.append([i for _, i in inside[:4]])
            if cands[k]:
                kinds.append("search")
            elif int(res["best"][k]) < 0 or float(res["d2_best"][k]) > gate_new:
                kinds.append("new")
            else:
                kinds.append("discarded")
        searched = [k for k, kind in enumerate(kinds) if kind == "search"]
        order = lambda h: (-h[1], h[2], h[0])                                   # (hypothesis, pairings, joint d2)
        alive, truncated = [((), 0, 0.0)], False
        sub = [scan[k] for k in searched]
        for level, k in enumerate(searched):
            ext = [hyp + (c,) for hyp, _, _ in alive for c in cands[k] + [-1] if c < 0 or c not in hyp]
            pad = [-1] * (len(searched) - level - 1)
            ans = self._e.joint_innovation(sub, np.array([list(h) + pad for h in ext], dtype=np.int64).reshape(len(ext), len(searched)))
            alive = []
            for h, d2 in zip(ext, np.asarray(ans["d2_prefix"])[:, level]):
                pairings = sum(1 for c in h if c >= 0)
                if float(d2) <= chi2_quantile(joint_p, 2 * pairings):             # (models 1 and 4: two rows a pairing; NaN never survives)
                    alive.append((h, pairings, float(d2)))
            alive.sort(key=order)
            if len(alive) > beam:
                alive, truncated = alive[:int(beam)], True
        winner = {k: c for k, c in zip(searched, alive[0][0]) if c >= 0} if searched else {}
        return self._measure_joint_close(entries, kinds, winner, truncated, gate_match, wait, joint_update, joint_iterations, joint_tol)

    def _measure_joint_close(self, entries, kinds, winner, truncated, gate_match, wait, joint_update, joint_iterations, joint_tol):
        """measure_model_joint behind its search, whichever side walked it: the winner ({entry: 0-based landmark}) applied, the new entries
        started, the rest discarded."""
        if joint_update and winner:
            # the winner's pairings in scan order as one joint update, then the close without them: the new entries and the discards
            self.observe_model_joint([dict(model=int(e[0]), z=e[1], R=e[2]) for e in (entries[k] for k in sorted(winner))],
                                     [winner[k] + 1 for k in sorted(winner)],
                                     **(dict(iterations=joint_iterations, tol=joint_tol) if joint_iterations != 1 else {}))
            out = self._measure_carry_out(entries, ["discarded" if k in winner else kind for k, kind in enumerate(kinds)], {}, gate_match, wait)
            for k in winner:
                out[k] = ("matched", winner[k] + 1)
            return out, truncated
        return self._measure_carry_out(entries, kinds, winner, gate_match, wait), truncated

    def _push_params(self):
        pass

    def measure(self, laserData, u, landmark_list):
        self._push_params()
        observed_LL = landmark_list.getLandmark(laserData, self.x)       # EKF_SLAM.m:102
        self.observed = observed_LL                                      # :103
        idx, loc = landmark_list.landmarkObj.table()
        if self.log is not None:
            self.log.record(u, observed_LL, idx, loc)
        if observed_LL is None or len(observed_LL) == 0:                 # :105
            return
        self._e.measure(observed_LL, u, idx, loc)

    def plot_data(self):
        """What plot() reads: pose and the 2x2 diagonal blocks of P (EKF_SLAM.m:180,205)."""
        return self.x, list(self._e.get_P_diag_blocks())

    def plot(self, landmark_list=None):
        """plot(h, landmark_list) (EKF_SLAM.m:154-234) minus the drawing: returns what the figure is made of -- pose,
        landmark positions, the 2x2 covariance blocks -- and forwards to the landmark source's own plot if it has one
        (EKF_SLAM.m:167)."""
        x, blocks = self.plot_data()
        src = getattr(landmark_list, "landmarkObj", None)
        if src is not None and hasattr(src, "plot"):
            src.plot(x, self.observed)
        return {"pose": x[:3], "landmarks": x[3:].reshape(-1, 2), "covariance_blocks": blocks}

    def sync(self):
        self._e.sync()


class EKF_SLAM(_EkfBase):
    """Known correspondence (EKF_SLAM.m)."""
    _mode = "known"


class EKF_SLAM_UC(_EkfBase):
    """Unknown correspondence (EKF_SLAM_UC.m); owns a Correspondence (EKF_SLAM_UC.m:16).  device_assoc=4 (an engine keyword) runs
    measure() with the position-weighted likelihood (w_pos != 0, Correspondence.m:74) without a host wait per observation: the
    device decides and carries out every row (include/ekfslam.h)."""
    _mode = "uc"

    def __init__(self, capacity=_DEFAULT_CAPACITY, **engine_kw):
        super().__init__(capacity, **engine_kw)
        # EKF_SLAM_UC.m:16: Correspondence(.00000000001, 1000000000, 'EKF_SLAM_UC') -- the engine's defaults (ekf_config_default);
        # s_cost / s_thresh given as engine keywords arrive here too, so that the property and the engine start out equal
        self.correspondence = Correspondence(self._e.cfg.s_cost, self._e.cfg.s_thresh, 'EKF_SLAM_UC')

    def _push_params(self):
        """measure() associates with h.correspondence's cost / threshold (EKF_SLAM_UC.m:16,119): the property is public and
        may be replaced or edited at any time, so its values go to the engine before every scan (as matlab/EKF_SLAM_UC.m's
        pushParams does)."""
        c = self.correspondence
        cfg = self._e.cfg
        if float(c.s_cost) != cfg.s_cost or float(c.s_thresh) != cfg.s_thresh:
            self._e.set_params(s_cost=float(c.s_cost), s_thresh=float(c.s_thresh))


class Correspondence:
    """Value class of Correspondence.m; the computation runs on the device through a scratch handle."""

    def __init__(self, cost, thresh, method):
        self.method = method
        self.s_cost = cost
        self.s_thresh = thresh
        if method != 'EKF_SLAM_UC':                                      # Correspondence.m:19-23
            warnings.warn('Improper method specified. Using ML as default.')
            self.method = 'ML'
        self.position_cost = None
        self.signature_cost = None

    def estimateCorrespondence(self, z, R, x, P, s, **engine_kw):
        x = _vec(x)
        N = (x.size - 3) // 2
        e = Engine(mode="uc", capacity=max(N, 1), s_cost=float(self.s_cost), s_thresh=float(self.s_thresh), **engine_kw)
        try:
            e.set_state(x, P, s)
            is_new, idx0, pc, sc = e.associate(z, R, want_costs=True)
        finally:
            e.close()
        self.position_cost, self.signature_cost = pc, sc
        return is_new, idx0 + 1                                          # 1-based like the reference


class Landmark:
    """Landmark.m surface.  'SYNTHETIC' is the seeded source of ekf_slam_amd.world; 'RANSAC' (Landmark.m:14-16) is the
    reference's landmark-list bookkeeping (ekf_slam_amd.ransac_bookkeeping) fed with wall foot-points -- the laser-scan
    line extraction itself needs ROS and MATLAB toolboxes and is out of scope."""

    def __init__(self, method):
        self.method = method
        if method == 'SYNTHETIC':
            self._src = SyntheticLandmark(method)
            self.landmarkObj = self._src.landmarkObj
        elif method == 'RANSAC':
            from .ransac_bookkeeping import RansacBookkeeping
            self.landmarkObj = RansacBookkeeping()
            self._src = self.landmarkObj
        else:
            warnings.warn('Improper landmark recognition method.')       # Landmark.m:18
            self._src = SyntheticLandmark('SYNTHETIC')
            self.landmarkObj = self._src.landmarkObj

    def getLandmark(self, laserdata, x):
        return self._src.getLandmark(laserdata, x)


def append(x, P, u, idx, R, pos, **engine_kw):
    """[x,P] = append(x,P,u,idx,R,pos)  (append.m:1-27): appends only if numOfLandmarks < idx."""
    x = _vec(x)
    N = (x.size - 3) // 2
    if not (N < idx):
        return x, np.asarray(P, dtype=np.float64)
    e = Engine(mode="known", capacity=N + 1, **engine_kw)
    try:
        e.set_state(x, P, np.zeros(N))
        e.append(u, R, pos, 0.0)
        return e.get_x(), e.get_P()
    finally:
        e.close()


class SLAM:
    """SLAM.m facade with the ROS subscribers replaced by a scripted feed of (u, scan) pairs."""

    def __init__(self, inputString, feed=None, capacity=_DEFAULT_CAPACITY, landmark_method='SYNTHETIC', **engine_kw):
        self.algorithmName = inputString
        self.feed = iter(feed) if feed is not None else None
        self.u = np.zeros(3)
        if inputString == 'EKF_SLAM':                                    # SLAM.m:26-35
            self.slam = EKF_SLAM(capacity, **engine_kw)
        elif inputString == 'EKF_SLAM_UC':
            self.slam = EKF_SLAM_UC(capacity, **engine_kw)
        else:
            self.slam = None
        self.LM = Landmark(landmark_method)       # SLAM.m:29,34 use 'RANSAC'

    def predict(self, u):
        if self.slam is not None:
            self.slam.predict(u)

    def measure(self, laserdata, u):
        if self.slam is not None:
            self.slam.measure(laserdata, u, self.LM)

    def plot(self):                               # SLAM.m:61-68
        if self.slam is not None:
            return self.slam.plot(self.LM)

    def runSlam(self):
        """One SLAM iteration: predict then measure (SLAM.m:105-116)."""
        u, scan = next(self.feed)
        self.u = np.asarray(u, dtype=np.float64)
        self.slam.predict(self.u)
        self.slam.measure(scan, self.u, self.LM)
