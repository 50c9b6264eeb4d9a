"""GPU: observations through a model linearised on the device (ekf_observe_model, ekf_model_innovation, ekf_model_evaluate;
include/ekfslam.h).

The yardstick is the NumPy restatement of tests/model_obs_cases.py applied to THE STATE THE ENGINE REPORTED BEFORE THE CALL; stores,
tolerances and helpers are those of tests/helpers.py.  Where two engines must agree because they ran the same arithmetic
on the same inputs -- k_gather_model against k_gather_linear handed the Jacobian the host evaluates, batch b against batch 1, the
device-resident association loops against the waited one, a replayed log -- the comparison is assert_array_equal.

N0 = 150 landmarks are 300 columns: two workgroups of k_gather_model, the second one partly idle."""
import ctypes

import numpy as np
import pytest

import model_obs_cases as M
from decided_plans import PARAMS
from helpers import R2, REL, RPOS, U2, assert_same, check_state, engine, getters, loaded, rel_err, state, status_of
from linear_obs_cases import N0, STORES, edge_landmark
from removal_cases import lowrank_data, observe

pytestmark = pytest.mark.gpu
NAMES = {M.RANGE_BEARING: "range and bearing", M.RANGE: "range", M.BEARING: "bearing", M.RELATIVE_XY: "relative xy", M.LANDMARK_RANGE: "landmark range"}


def send(e, o, wait=False):
    return e.observe_model(o["model"], o["z"][:o["rows"]], o["R"], o["landmarks"], o["anchor"], gate=o["gate"], wait=wait)


def ask(e, o):
    return e.model_innovation(o["model"], o["z"][:o["rows"]], o["R"], o["landmarks"], o["anchor"], gate=o["gate"])


def near(x, model, landmarks=(), anchor=None, dz=(0.3, -0.4), R=None, gate=M.INF):
    """An observation of `model` whose z lies dz beside h(x)."""
    rows = M.ROWS[model]
    o = M.obs(model, np.zeros(rows), (RPOS if rows == 2 else 0.05) if R is None else R, landmarks, anchor, gate)
    hx, _ = M.jacobian(np.asarray(x), o)
    o["z"][:rows] = hx[:rows] + np.asarray(dz, dtype=np.float64)[:rows]
    return o


def history(engines, x, ks):
    for q in engines:
        for k in ks:
            q.predict(U2); q.correct(observe(x, k), R2, k)


# ------------------------------------------------------------------------------------------------------------------
# 1. every model against the dense restatement
# ------------------------------------------------------------------------------------------------------------------
def _specs(T_):
    """(name, model, landmarks, anchor offset from the robot or None): every model at the first, the last and a tile-row-edge landmark,
    the anchor forms, and the landmark pairs in one tile, in different tile rows, adjacent over a tile edge, in both orders."""
    e = edge_landmark(T_)
    out = []
    for m in (M.RANGE_BEARING, M.RANGE, M.BEARING, M.RELATIVE_XY):
        for k, where in ((0, "first"), (N0 - 1, "last"), (e, "tile-row edge")):
            out.append(("%s, %s landmark" % (NAMES[m], where), m, [k], None))
        out.append(("%s, anchor" % NAMES[m], m, [], np.array([7.0, -4.0]) * (1.0 + 0.5 * m)))
    for i, j, where in ((e + 1, e + 2, "one tile"), (3, N0 - 2, "different tile rows"), (e, e - 1, "adjacent over a tile edge, l0 > l1"),
                        (e - 1, e, "adjacent over a tile edge, l0 < l1"), (N0 - 1, 0, "last and first")):
        out.append(("landmark range, %s" % where, M.LANDMARK_RANGE, [i, j], None))
    return out


@pytest.mark.parametrize("tile,storage", STORES)
def test_every_model_against_the_dense_restatement(tile, storage):
    e = loaded(N0, 5, capacity=N0 + 8, tile=tile, storage=storage)
    x = lowrank_data(N0, 5)[0]
    history([e], x, (5, edge_landmark(tile), N0 - 3))     # some history first, so that P is not the loaded one
    for name, m, lms, off in _specs(tile):
        x0, _, P0 = state(e)
        o = near(x0, m, lms, None if off is None else x0[:2] + off)
        ex, eP, want = M.observe_model_dense(x0, P0, o)
        got = send(e, o, wait=True)
        assert got["outcome"] == want["outcome"] == M.APPLIED, name
        tol = REL if storage == "f64" else 1e-9               # F64 arithmetic on what the getters report, in every storage kind
        errs = (rel_err(got["nu"], want["nu"]), rel_err(got["S"], want["S"]), abs(got["d2"] - want["d2"]) / want["d2"])
        print("%s [%s]: d2 %.4g rel err nu %.2e S %.2e d2 %.2e" % ((name, storage, got["d2"]) + errs))
        assert max(errs) < tol, name
        check_state(e, ex, eP, storage, name)
        if o["rows"] == 1:
            assert got["S"][0, 1] == 0.0 and got["S"][1].tolist() == [0.0, 1.0] and got["nu"][1] == 0.0
    assert e.N == N0 and e.linear_rejections() == (0, 0)


# ------------------------------------------------------------------------------------------------------------------
# 2. P does not depend on nu: the column arithmetic is k_gather_linear's, the host's H is the device's
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage", [(16, "f64"), (64, "f64"), (256, "f32_mixed")])
@pytest.mark.parametrize("pending", [0, 5])
def test_P_is_bit_for_bit_that_of_observe_linear_with_the_evaluated_jacobian(tile, storage, pending):
    from ekf_slam_amd.engine import Engine
    x = lowrank_data(N0, 5)[0]
    ed = edge_landmark(tile)
    kw = dict(capacity=N0 + 8, tile=tile, storage=storage, batch=8)
    for name, m, lms, off in (("range and bearing", M.RANGE_BEARING, [ed], None), ("range", M.RANGE, [N0 - 1], None), ("bearing", M.BEARING, [0], None),
                              ("relative xy", M.RELATIVE_XY, [ed], None), ("landmark range", M.LANDMARK_RANGE, [ed, ed - 1], None),
                              ("range and bearing, anchor", M.RANGE_BEARING, [], np.array([9.0, 5.0])), ("bearing, anchor", M.BEARING, [], np.array([-6.0, 11.0]))):
        e, twin = loaded(N0, 5, **kw), loaded(N0, 5, **kw)
        history([e, twin], x, (5, ed, N0 - 3, 11, 40)[:pending])
        assert e.pending() == pending
        xe = e.get_x()
        np.testing.assert_array_equal(xe, twin.get_x())
        o = near(xe, m, lms, None if off is None else xe[:2] + off)
        at = lambda k: xe[3 + 2 * k:5 + 2 * k]
        t0 = at(lms[0]) if lms else o["anchor"]
        hx, H = Engine.model_evaluate(m, xe[:3], t0, at(lms[1]) if m == M.LANDMARK_RANGE else None, lib=e.lib)
        nu = ask(e, o)["nu"]
        x7 = np.concatenate([xe[:3], at(lms[0]) if lms else np.zeros(2), at(lms[1]) if len(lms) > 1 else np.zeros(2)])
        Hl = [H[:, 3 + 2 * b:5 + 2 * b] for b in range(len(lms))]
        Hx = H[:, :3] @ x7[:3] + sum((Hl[b] @ x7[3 + 2 * b:5 + 2 * b] for b in range(len(lms))), np.zeros(2))
        got = send(e, o, wait=True)
        lin = twin.observe_linear(nu + Hx, M.effective_R(o), H[:, :3], lms, Hl, gate=M.INF, rows=2, wait=True)
        assert got["outcome"] == lin["outcome"] == M.APPLIED and e.pending() == twin.pending() == pending + 1, name
        np.testing.assert_array_equal(got["S"], lin["S"], err_msg=name)
        Pe, Pt = e.get_P(), twin.get_P()
        np.testing.assert_array_equal(Pe, Pt, err_msg=name)   # every tile, the strip rows and Prr
        np.testing.assert_array_equal(e.get_P_diag_blocks(), twin.get_P_diag_blocks(), err_msg=name)
        np.testing.assert_array_equal(e.get_P_block(0, 0, 3, 3 + 2 * N0), twin.get_P_block(0, 0, 3, 3 + 2 * N0), err_msg=name)
        err = np.abs(e.get_x() - twin.get_x()).max() / np.abs(xe).max()
        print("%s [T = %d %s, %d pending]: P bit-equal to observe_linear's, x rel diff %.2e, moved by %.2e" % (name, tile, storage, pending, err, np.abs(e.get_x() - xe).max()))
        assert err < 1e-12 and np.abs(e.get_x() - xe).max() > 1e-6, name
        e.close(); twin.close()


# ------------------------------------------------------------------------------------------------------------------
# 3. it is a deferred step
# ------------------------------------------------------------------------------------------------------------------
def _schedule(seed, N, steps, per_row):
    """A random schedule of predict / append / correct / observe_model as a pure function of its arguments (z from the loaded x, not
    from the engine); the appends carry the map over a tile-row edge."""
    rng = np.random.default_rng(seed)
    x = lowrank_data(N, 5)[0]
    pos = [x[3 + 2 * k:5 + 2 * k].copy() for k in range(N)]
    ops = []
    target = (N // per_row + 1) * per_row + 2
    for t in range(steps):
        r = rng.random()
        if len(pos) < target and r < 0.25:
            p = rng.uniform(-20, 20, 2)
            ops.append(("append", p, 900.0 + t)); pos.append(p)
            continue
        n = len(pos)
        xs = np.concatenate([x[:3]] + pos)
        if r < 0.6:
            k = int(rng.integers(0, n))
            ops.append(("correct", observe(xs, k, dr=0.02 * rng.standard_normal(), db=0.3 * rng.standard_normal()), k))
            continue
        model = int(rng.integers(1, 6))
        i, j = (int(v) for v in rng.choice(n, 2, replace=False))
        xt = xs.copy(); xt[2] += t + 1.0                     # (predict turns the robot by 1 degree per step)
        if model == M.LANDMARK_RANGE:
            o = near(xt, model, [n - 1, j if j != n - 1 else i], dz=0.1 * rng.standard_normal(2))
        elif rng.random() < 0.3:
            o = near(xt, model, [], anchor=x[:2] + rng.uniform(3, 15, 2), dz=0.1 * rng.standard_normal(2))
        else:
            o = near(xt, model, [i], dz=0.1 * rng.standard_normal(2))
        if rng.random() < 0.15:
            o["gate"] = 1e-6                                  # a gated one now and then: it takes its slot all the same
        ops.append(("observe", o))
    return ops


def _play(e, ops):
    pend = []
    for op in ops:
        e.predict(U2)
        if op[0] == "append":
            e.append(U2, R2, op[1], op[2])
        elif op[0] == "correct":
            e.correct(op[1], R2, op[2])
        else:
            send(e, op[1])
        pend.append(e.pending())
    return pend


@pytest.fixture(scope="module")
def schedule_reference():
    ops = _schedule(18, 20, 60, 8)
    one = loaded(20, 5, capacity=40, tile=16, batch=1)
    _play(one, ops)
    return ops, getters(one), one.linear_rejections()


@pytest.mark.parametrize("batch,asy", [(3, False), (8, False), (3, True), (8, True)])
def test_a_schedule_with_model_observations_is_deferred_like_corrections(schedule_reference, batch, asy):
    ops, want, rejected = schedule_reference
    assert sum(op[0] == "observe" for op in ops) >= 12 and sum(op[0] == "append" for op in ops) >= 5 and rejected[1] >= 1
    assert {op[1]["model"] for op in ops if op[0] == "observe"} == {1, 2, 3, 4, 5}
    assert all(np.all(np.isfinite(g)) for g in want)
    e = loaded(20, 5, capacity=40, tile=16, batch=batch, async_flush=asy)
    pend = _play(e, ops)
    assert max(pend) >= batch - 1 and (not asy or max(pend) > batch)      # the ring was in use (asynchronous: beyond one batch, so it wrapped)
    assert e.N > 24                                           # the appends crossed the tile-row edge at 24 landmarks
    for got, ref in zip(getters(e), want):
        np.testing.assert_array_equal(got, ref)
    assert e.linear_rejections() == rejected


def test_a_model_observation_waits_for_the_batch_boundary():
    from ekf_slam_amd import _lib as L
    x = lowrank_data(N0, 5)[0]
    e = loaded(N0, 5, capacity=N0 + 8, tile=64, batch=4)
    e.timing_enable(L.EKF_KERNEL_DOWNDATE, True, 16)
    e.timing_enable(L.EKF_KERNEL_GATHER, True, 16)
    e.timing_read(L.EKF_KERNEL_DOWNDATE); e.timing_read(L.EKF_KERNEL_GATHER)
    send(e, near(x, M.RANGE_BEARING, [7]))
    assert e.pending() == 1
    assert e.timing_read(L.EKF_KERNEL_DOWNDATE)[0] == 0 and e.timing_read(L.EKF_KERNEL_GATHER)[0] == 1      # counted under EKF_KERNEL_GATHER
    send(e, near(x, M.RANGE, [], anchor=x[:2] + [5.0, 5.0])); e.correct(observe(x, 9), R2, 9)
    assert e.pending() == 3 and e.timing_read(L.EKF_KERNEL_DOWNDATE)[0] == 0
    send(e, near(x, M.LANDMARK_RANGE, [3, 90]))              # the fourth step of the batch: the pass runs
    assert e.pending() == 0 and e.timing_read(L.EKF_KERNEL_DOWNDATE)[0] == 1 and e.downdate_kernel_name()[1] == 4


# ------------------------------------------------------------------------------------------------------------------
# 4. the innovation
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,storage,asy", [(16, "f64", False), (64, "f64", True), (256, "f32_mixed", False)])
def test_model_innovation_reports_what_the_observation_will_and_changes_nothing(tile, storage, asy):
    x = lowrank_data(N0, 5)[0]
    kw = dict(capacity=N0 + 8, tile=tile, storage=storage, batch=8, async_flush=asy)
    e, twin = loaded(N0, 5, **kw), loaded(N0, 5, **kw)
    history([e, twin], x, (5, edge_landmark(tile), N0 - 3, 11, 12, 40, 41, 42, 43, 44, 45))      # a full batch and three more
    pend = e.pending()
    assert pend >= 3
    for name, m, lms, off in _specs(tile)[::2]:
        for q in (e, twin):
            q.predict(U2)
        o = near(x, m, lms, None if off is None else x[:2] + off)
        before = e.get_x()
        want = ask(e, o)
        assert e.pending() == pend
        np.testing.assert_array_equal(e.get_x(), before)
        got = send(e, o, wait=True)
        send(twin, o)
        for key in ("nu", "S", "d2", "outcome"):
            np.testing.assert_array_equal(np.asarray(got[key]), np.asarray(want[key]), err_msg=name + " " + key)
        pend = e.pending()
    assert_same(e, twin)                                    # the twin never asked


# ------------------------------------------------------------------------------------------------------------------
# 5. gate and a target on the robot
# ------------------------------------------------------------------------------------------------------------------
def test_gated_and_irregular_observations_change_nothing():
    from ekf_slam_amd import _lib as L
    x = lowrank_data(N0, 5)[0]
    kw = dict(capacity=N0 + 8, tile=64, batch=4)
    e, twin = loaded(N0, 5, **kw), loaded(N0, 5, **kw)
    history([e, twin], x, (9,))                              # a pair pending
    assert e.linear_rejections() == (0, 0)
    before = getters(twin)
    xe = e.get_x()
    gated = near(xe, M.RANGE_BEARING, [12], dz=(2.0, 9.0))
    d2 = ask(e, gated)["d2"]
    assert d2 > 1.0
    gated["gate"] = d2 / 3.0                                  # a factor 3 on either side: rounding cannot decide
    on_robot = M.obs(M.RANGE, [1.0], 0.5, anchor=xe[:2])      # q = 0 exactly: the anchor is the position get_x reported
    # with a result: the outcome comes back, nothing read afterwards differs
    res = send(e, gated, wait=True)
    assert res["outcome"] == L.EKF_LINEAR_GATED and res["d2"] == d2 and e.pending() == 2
    st, msg = status_of(lambda: send(e, on_robot, wait=True))
    assert st == L.EKF_ERR_STATE and "observe_model" in msg and e.pending() == 3
    inn = ask(e, on_robot)
    assert inn["outcome"] == L.EKF_LINEAR_IRREGULAR and np.isnan(inn["d2"]) and np.all(np.isfinite(inn["S"])) and np.all(np.isfinite(inn["nu"]))
    assert e.linear_rejections() == (1, 1) and e.linear_rejections() == (0, 0)
    # without one: the state stays finite and unchanged, the no-ops are counted
    send(e, gated)                                            # (the fourth step: the pass runs over two zero pairs)
    send(e, M.obs(M.RELATIVE_XY, [1.0, 2.0], RPOS, anchor=xe[:2]))
    assert e.pending() == 1
    assert e.linear_rejections() == (1, 1) and e.linear_rejections() == (0, 0)
    for got, ref in zip(getters(e), before):
        assert np.all(np.isfinite(got))
        np.testing.assert_array_equal(got, ref)
    # the same observation with a gate a factor 3 above d2 applies, and the handle goes on like a twin that never saw the no-ops
    gated["gate"] = d2 * 3.0
    for q in (e, twin):
        assert send(q, gated, wait=True)["outcome"] == L.EKF_LINEAR_APPLIED
        q.predict(U2); q.correct(observe(x, 12), R2, 12)
    assert_same(e, twin)
    assert rel_err(e.get_x()[27:29], before[0][27:29]) > 1e-6


# ------------------------------------------------------------------------------------------------------------------
# 6. refusals, each before anything changes
# ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_state_alone():
    from ekf_slam_amd import _lib as L
    x = lowrank_data(N0, 5)[0]
    kw = dict(capacity=N0 + 8, tile=64, batch=8)
    e, twin = loaded(N0, 5, **kw), loaded(N0, 5, **kw)
    history([e, twin], x, (4, 77))
    x_before, pend = e.get_x(), e.pending()
    nan, inf = float("nan"), float("inf")

    def make(m=M.RANGE_BEARING, lm=(5, -1), **kw):
        ob = e._model_obs(m, [3.0, 20.0], RPOS, [k for k in lm if k >= 0] or [0], None, 9.0)
        ob.lm[0], ob.lm[1] = lm
        ob.anchor[0], ob.anchor[1] = 4.0, 5.0
        for key, (idx, v) in kw.items():
            if idx is None:
                setattr(ob, key, v)
            else:
                getattr(ob, key)[idx] = v
        return ob

    bad, idx = L.EKF_ERR_INVALID_ARG, L.EKF_ERR_INDEX
    cases = [("model 0", make(model=(None, 0)), bad), ("model 6", make(model=(None, 6)), bad),
             ("a second landmark for a range", make(M.RANGE, (5, 6)), bad), ("a second landmark for relative xy", make(M.RELATIVE_XY, (5, 0)), bad),
             ("a second landmark for an anchored bearing", make(M.BEARING, (-1, 6)), bad), ("lm[0] = -2", make(M.RANGE, (-2, -1)), bad),
             ("the same landmark twice", make(M.LANDMARK_RANGE, (5, 5)), bad), ("a landmark range with one landmark", make(M.LANDMARK_RANGE, (5, -1)), bad),
             ("a landmark range with none", make(M.LANDMARK_RANGE, (-1, -1)), bad), ("a landmark range from -1", make(M.LANDMARK_RANGE, (-1, 5)), bad),
             ("N", make(M.RANGE, (N0, -1)), idx), ("N in a pair", make(M.LANDMARK_RANGE, (5, N0 + 3)), idx),
             ("NaN z", make(z=(1, nan)), bad), ("inf z", make(M.RANGE, z=(0, inf)), bad), ("NaN anchor", make(M.RANGE, (-1, -1), anchor=(1, nan)), bad),
             ("inf R", make(R=(0, inf)), bad), ("asymmetric R", make(R=(1, 0.2)), bad), ("negative diagonal", make(R=(3, -1.0)), bad),
             ("negative variance", make(M.BEARING, R=(0, -0.1)), bad), ("NaN gate", make(gate=(None, nan)), bad)]
    res = L.EkfLinearResult()
    for name, ob, want in cases:
        for entry, fn in (("observe_model", lambda: e.lib.ekf_observe_model(e.h, ctypes.byref(ob), None)),
                          ("observe_model", lambda: e.lib.ekf_observe_model(e.h, ctypes.byref(ob), ctypes.byref(res))),
                          ("model_innovation", lambda: e.lib.ekf_model_innovation(e.h, ctypes.byref(ob), ctypes.byref(res)))):
            assert fn() == want, (entry, name)
            assert entry.encode() in e.lib.ekf_last_error(e.h), (entry, name)
            assert e.pending() == pend and e.N == N0
            np.testing.assert_array_equal(e.get_x(), x_before)
    assert e.lib.ekf_observe_model(e.h, None, None) == bad
    assert e.lib.ekf_model_innovation(e.h, ctypes.byref(make()), None) == bad
    # what a model does not read is no reason to refuse: row 1 of z and R for a one-row model, the anchor where a landmark is the target
    one = make(M.RANGE, z=(1, nan), R=(3, -5.0)); one.R[1] = 7.0; one.anchor[0] = nan
    assert e.lib.ekf_model_innovation(e.h, ctypes.byref(one), ctypes.byref(res)) == L.EKF_OK and res.S[1] == 0.0 and res.S[3] == 1.0
    assert e.linear_rejections() == (0, 0)
    assert_same(e, twin)
    # ekf_model_evaluate: pure, refuses what it cannot evaluate
    hx, H = np.zeros(2), np.zeros(14)
    p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    xr, t0 = np.array([1.0, 2.0, 30.0]), np.array([4.0, 6.0])
    assert e.lib.ekf_model_evaluate(0, p(xr), p(t0), None, p(hx), p(H)) == bad and e.lib.ekf_model_evaluate(5, p(xr), p(t0), None, p(hx), p(H)) == bad
    assert e.lib.ekf_model_evaluate(2, p(xr), p(t0), None, p(hx), p(H)) == L.EKF_OK and hx[0] == 5.0
    assert e.lib.ekf_model_evaluate(2, p(xr), p(xr[:2].copy()), None, p(hx), p(H)) == L.EKF_ERR_STATE and not H.any() and not hx.any()
    # sharded handles: refused, the anchor forms included, and the message says why; the arguments are checked first
    sh = engine(capacity=64, tile=16, world=2, rank=0)
    for fn in (lambda: send(sh, M.obs(M.RANGE, [1.0], 0.5, [0])), lambda: send(sh, M.obs(M.RANGE, [1.0], 0.5, anchor=[3.0, 4.0])),
               lambda: ask(sh, M.obs(M.BEARING, [1.0], 0.5, anchor=[3.0, 4.0]))):
        st, msg = status_of(fn)
        assert st == bad and "shard" in msg
    st, msg = status_of(lambda: send(sh, M.obs(M.RANGE, [nan], 0.5, anchor=[3.0, 4.0])))
    assert st == bad and "shard" not in msg


@pytest.mark.parametrize("batch", [1, 4])
def test_a_lone_shard_with_the_sharded_code_path_simply_works(batch):
    x = lowrank_data(N0, 5)[0]
    e = loaded(N0, 5, capacity=N0 + 8, tile=64, force_sharded=1, batch=batch)
    twin = loaded(N0, 5, capacity=N0 + 8, tile=64, batch=batch)
    harr = (ctypes.c_void_p * 1)(e.h)

    def corrections(ks):
        for k in ks:
            z = observe(x, k)
            e.predict(U2); twin.predict(U2)
            e.correct_begin(z, R2, k)
            assert e.lib.ekf_exchange_local(harr, 1) == 0
            e.correct_finish()
            twin.correct(z, R2, k)

    corrections((3, 30, 149))
    for o in (near(x, M.RANGE_BEARING, [30]), near(x, M.BEARING, [], anchor=x[:2] + [6.0, 2.0]), near(x, M.LANDMARK_RANGE, [31, 32])):
        for q in (e, twin):
            send(q, o)
    corrections((0, 30, 31, 100, 149))
    for q in (e, twin):
        assert send(q, near(x, M.RELATIVE_XY, [149]), wait=True)["outcome"] == 1
    corrections((1, 148))
    assert_same(e, twin)


# ------------------------------------------------------------------------------------------------------------------
# 7. unknown correspondence: model observations between the scans of the device-resident loops
# ------------------------------------------------------------------------------------------------------------------
def _uc_run(device_assoc, params):
    cap = N0 + 40
    e = loaded(N0, 3, "uc", capacity=cap, tile=64, batch=8, device_assoc=device_assoc, **params)
    lm_index = np.arange(1, cap + 1, dtype=np.float64)
    lm_loc = np.random.default_rng(5).uniform(-20, 20, (cap, 2))
    for t in range(3):
        e.predict(U2)
        x, s = e.get_x(), e.get_s()                           # (the pose the scan is taken from: the position cost is strict)
        ks = [9 + t, 70, 140 - t]
        rows = [list(observe(x, k)) + [s[k]] for k in ks] + [[3.0 + t, 45.0, 7e6 + t]]      # the last row matches nothing: appended
        e.measure(np.array(rows), U2, lm_index, lm_loc)
        # straight behind the scan: with device_assoc = 4 its rows are queued and nothing is settled when the observations arrive
        send(e, near(x, M.RANGE, [], anchor=x[:2] + [4.0, -3.0], dz=(0.05,)))
        send(e, near(x, M.RANGE_BEARING, [ks[0]], dz=(0.05, 0.2)))
        assert send(e, near(x, M.LANDMARK_RANGE, [70, N0 - 1], dz=(0.1,)), wait=True)["outcome"] == 1
        send(e, near(x, M.BEARING, [ks[2]], dz=(5.0,), gate=1e-9))     # gated: a zero pair in the ring between two scans
    assert e.N == N0 + 3 and e.linear_rejections() == (0, 3)
    return e


def test_model_observations_between_scans_signature_only():
    runs = {m: _uc_run(m, dict(w_pos=0.0)) for m in (1, 3)}
    assert_same(runs[3], runs[1])


def test_model_observations_between_scans_position_weighted():
    runs = {m: _uc_run(m, PARAMS) for m in (1, 4)}
    assert_same(runs[4], runs[1])


# ------------------------------------------------------------------------------------------------------------------
# 8. the slam.py wrappers and a replayed log
# ------------------------------------------------------------------------------------------------------------------
def test_a_run_with_model_observations_replays_from_its_log(tmp_path):
    from ekf_slam_amd.slam import SLAM
    from ekf_slam_amd.trajectory import FORMAT_MODEL, TrajectoryLog
    from ekf_slam_amd.world import make_run
    _, run = make_run(40, 11, 24, policy="nearest", m=6)
    run = list(run)
    kw = dict(capacity=64, tile=16, batch=4)
    full = SLAM('EKF_SLAM', feed=run, landmark_method='SYNTHETIC', **kw)
    plain = SLAM('EKF_SLAM', feed=run, landmark_method='SYNTHETIC', **kw)
    full.slam.log = TrajectoryLog()
    for k in range(len(run)):
        full.runSlam(); plain.runSlam()
        xs = full.slam.x
        at = lambda i: xs[1 + 2 * i:3 + 2 * i]                # 1-based at this layer: landmark i is entries 1 + 2 i, 2 + 2 i of x
        if k == 7:
            o = near(xs, M.RANGE, [], anchor=xs[:2] + [6.0, -2.0], dz=(0.05,))
            assert full.slam.observe_anchor_range(o["anchor"], o["z"][0], 0.05) is None
        if k == 12:
            o = near(xs, M.RANGE_BEARING, [2], dz=(0.05, 0.3))
            want = full.slam.model_innovation(M.RANGE_BEARING, o["z"], RPOS, [3], gate=50.0)
            res = full.slam.observe_range_bearing(3, o["z"], RPOS, gate=50.0, wait=True)
            assert res["outcome"] == 1 and 0 < res["d2"] < 50.0 and res["d2"] == want["d2"]
            np.testing.assert_allclose(res["nu"], [0.05, 0.3], rtol=0, atol=1e-9)
        if k == 18:
            d = at(1) - at(2)
            full.slam.observe_landmark_range(1, 2, np.sqrt(d @ d) + 0.05, 0.01)
            full.slam.observe_relative_xy(3, near(xs, M.RELATIVE_XY, [2], dz=(0.02, -0.03))["z"], RPOS)
            full.slam.observe_bearing(1, near(xs, M.BEARING, [0], dz=(0.4,))["z"][0], 0.2)
    path = tmp_path / "observed_run.npz"
    full.slam.log.save(path)
    log = TrajectoryLog.load(path)
    assert str(np.load(path)["format"]) == FORMAT_MODEL and [(e[0], e[1], e[2].tolist()) for e in log.edits] == \
        [(8, "observe_model", []), (13, "observe_model", [3]), (19, "observe_model", [1, 2]), (19, "observe_model", [3]), (19, "observe_model", [1])]
    fresh = engine(**kw)
    log.replay(fresh)
    np.testing.assert_array_equal(fresh.get_x(), full.slam.x)
    np.testing.assert_array_equal(fresh.get_s(), full.slam.s)
    np.testing.assert_array_equal(fresh.get_P(), full.slam.P)
    assert full.slam.linear_rejections() == (0, 0)
    assert rel_err(full.slam.x, plain.slam.x) > 1e-6        # the observations did move the map
