"""CPU: the factored oracle (oracle/ekf_factored.py: landmark block of P implicit, O(n (k + 2t)) per step -- the restatement that reaches
50 000 landmarks) pinned to the literal-dense restatement (oracle/ekf_dense.py) where the latter can run: N <= 200, 1e-11 relative
(max-norm) on x and P, known and unknown correspondence, appends, bulk-loaded low-rank states.  Both are the builder's restatements of
EKF_SLAM.m:40-145 / EKF_SLAM_UC.m:102-152 / Correspondence.m:28-88: parity with the MATLAB reference itself stays unpinned."""
import numpy as np
import pytest

from oracle import ekf_dense
from oracle.ekf_factored import FactoredEKF
from ekf_slam_amd.world import SyntheticLandmark, make_run

TOL = 1e-11


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("mode,N,steps,policy,m", [("known", 20, 30, "all", 0), ("uc", 20, 30, "all", 0), ("uc", 120, 40, "nearest", 6)])
def test_measure_loop_equals_the_dense_restatement(mode, N, steps, policy, m):
    kw = dict(policy=policy) if policy == "all" else dict(policy=policy, m=m)
    _, run = make_run(N, 20260101 + N, steps, **kw)
    dense = ekf_dense.EKF_SLAM() if mode == "known" else ekf_dense.EKF_SLAM_UC()
    fac = FactoredEKF(N + 4, mode, max_terms=steps * max(N if policy == "all" else m, 1) + 8)
    ld, lf = SyntheticLandmark(), SyntheticLandmark()
    for u, scan in run:
        dense.predict(u); fac.predict(u)
        dense.measure(scan, u, ld); fac.measure(scan, u, lf)
    assert fac.N == (len(dense.x) - 3) // 2 == N
    assert rel(fac.x, dense.x) < TOL and rel(fac.P, dense.P) < TOL
    np.testing.assert_array_equal(np.asarray(fac.s, float), np.asarray(dense.s, float))


def test_bulk_loaded_state_with_streaming_appends_equals_the_dense_restatement():
    """configs[4]'s shape in small: P = diag(d) + U U', then predict + append + correct per step (EKF_SLAM.m:40-51, :67-98, :124-145)"""
    rng = np.random.default_rng(5)
    N0, steps = 150, 60
    n0 = 3 + 2 * N0
    x = np.concatenate([[0.2, -0.1, 33.0], rng.uniform(-20, 20, 2 * N0)])
    d, U = rng.uniform(0.01, 0.1, n0), rng.normal(0, 0.05, (n0, 6))
    fac = FactoredEKF(N0 + steps, "known", max_terms=steps + 4)
    fac.load_lowrank_state(x, np.arange(1, N0 + 1.0), d, U)
    dense = ekf_dense.EKF_SLAM()
    dense.x, dense.P, dense.s = x.copy(), np.diag(d) + U @ U.T, list(np.arange(1, N0 + 1.0))
    assert rel(fac.P, dense.P) < 1e-15
    for t in range(steps):
        u = [0.1, 3.0]
        idx = int(rng.integers(1, fac.N + 1))
        z = [rng.uniform(1, 30), rng.uniform(1, 359)]
        R = np.diag([z[0] * .01, z[1] * 5.0])
        pos = rng.uniform(-5, 5, 2)
        for e in (fac, dense):
            e.predict(u)
            e.append(u, R, pos, e.N + 1 if e is fac else len(e.s) + 1)
            (e.correct if e is fac else e._correct)(z, R, idx)
        if t % 20 == 19:
            assert rel(fac.x, dense.x) < TOL and rel(fac.P, dense.P) < TOL
    # corrections of landmarks appended on the way (their rows come from the appended panels)
    for idx in (N0 + 1, N0 + steps, N0 + 7):
        z = [5.0, 100.0]
        R = np.diag([.05, 500.0])
        fac.correct(z, R, idx); dense._correct(z, R, idx)
    assert rel(fac.x, dense.x) < TOL and rel(fac.P, dense.P) < TOL
    # the readers the GPU tests use
    D = fac.diag_blocks()
    for k in (0, 17, N0, N0 + steps - 1):
        np.testing.assert_allclose(D[k], dense.P[3 + 2 * k:5 + 2 * k, 3 + 2 * k:5 + 2 * k], rtol=0, atol=TOL * np.abs(dense.P).max())
    np.testing.assert_allclose(fac.P_rows(3 + 2 * 40, 2), dense.P[3 + 80:3 + 82], rtol=0, atol=TOL * np.abs(dense.P).max())
    np.testing.assert_allclose(fac.P_rows(0, 3), dense.P[:3], rtol=0, atol=TOL * np.abs(dense.P).max())


def test_association_costs_equal_the_dense_restatement():
    """Correspondence.m:49-87 from the implicit block: position (Mahalanobis) and signature cost of every landmark, and the decision"""
    _, run = make_run(40, 11, 12, policy="all")
    dense, fac = ekf_dense.EKF_SLAM_UC(), FactoredEKF(44, "uc", max_terms=600)
    ld, lf = SyntheticLandmark(), SyntheticLandmark()
    for u, scan in run:
        dense.predict(u); fac.predict(u)
        dense.measure(scan, u, ld); fac.measure(scan, u, lf)
    z = [7.0, 123.0, 17.0]
    R = np.diag([z[0] * .1, z[1] * 5.0])
    nd, idd = dense.correspondence.estimateCorrespondence(z, R, dense.x, dense.P, dense.s)
    nf, idf = fac.estimateCorrespondence(z, R)
    assert (nd, idd) == (nf, idf)
    np.testing.assert_allclose(fac.last_position_cost, dense.correspondence.last_position_cost, rtol=1e-9)
    np.testing.assert_allclose(fac.last_signature_cost, dense.correspondence.last_signature_cost, rtol=1e-12)


# ------------------------------------------------------------------------------------------------------------------
# the generic steps (update_linear, append_jacobian, predict_affine) the newer families reduce to, driven through the plan of
# tests/beside_pass_cases.py, against the dense forms of the *_cases.py files on one dense P
# ------------------------------------------------------------------------------------------------------------------
def _small_state(N0, sigma, seed=5):
    rng = np.random.default_rng(seed)
    n0 = 3 + 2 * N0
    x = np.concatenate([[0.0, 0.0, 0.0], rng.uniform(-40, 40, 2 * N0)])
    d, U = rng.uniform(0.01, 0.1, n0), rng.normal(0, sigma, (n0, 8))
    return x, np.arange(1, N0 + 1.0), d, U


def test_a_plan_of_every_newer_family_equals_the_dense_forms():
    """>= 60 update-steps at N <= 200: corrections, the four linear kinds, the five models on landmarks and anchors (plain and iterated),
    model appends of 3-8 entries, motion chains of the three models: x and the whole P to 1e-11 at every batch boundary"""
    import beside_pass_cases as B
    N0, T, batch, batches = 120, 16, 8, 8
    x, s, d, U = _small_state(N0, 0.1)
    steps, info = B.make_plan(x, T, batch, batches, (.01, .5))
    kinds = B.kinds_of(steps)
    assert len(steps) >= 60 and info["N"] <= 200 and info["crossing_scans"] >= 3
    for kind in ("predict", "predict_model", "append_model") + B.PAIR_KINDS:
        assert kinds.get(kind, 0) >= 3, kinds
    models = {(p["model"], bool(p["landmarks"])) for ops in steps for k, p, _ in ops if k in ("observe_model", "observe_model_iterated")}
    assert {m for m, _ in models} == {1, 2, 3, 4, 5} and (1, False) in models
    cap = N0 + B.appended_total(steps)
    fac = FactoredEKF(cap, "known", max_terms=len(steps) + 4)
    fac.load_lowrank_state(x, s, d, U)
    dense = ekf_dense.EKF_SLAM()
    dense.x, dense.P, dense.s = x.copy(), np.diag(d) + U @ U.T, list(s)
    worst = 0.0
    for t, ops in enumerate(steps):
        for kind, payload, _ in ops:
            B.apply_factored(fac, kind, payload)
            B.apply_dense(dense, kind, payload)
        if (t + 1) % batch == 0 or t + 1 == len(steps):
            ex, eP = rel(fac.x, dense.x), rel(fac.P, dense.P)
            worst = max(worst, ex, eP)
            assert ex < TOL and eP < TOL, (t, ex, eP)
    assert fac.N == info["N"] == (dense.x.size - 3) // 2
    np.testing.assert_array_equal(np.asarray(fac.s, float), np.asarray(dense.s, float))
    print("factored against dense over %d steps (%s): worst relative difference %.2e" % (len(steps), kinds, worst))


def test_the_generic_steps_one_by_one():
    """a one-row step leaves the term's second row zero; an append's cross blocks within a scan; an affine motion on both strips"""
    import append_model_cases as A
    import linear_obs_cases as C
    import predict_model_cases as Pm
    x, s, d, U = _small_state(30, 0.2, seed=9)
    fac = FactoredEKF(40, "known", max_terms=8)
    fac.load_lowrank_state(x, s, d, U)
    P = np.diag(d) + U @ U.T
    o = C.scalar_on_landmark(7, 1.5, 0.3)
    H = C.jacobian(x.size, o)
    fac.update_linear(H[:1, :3], [7], [H[:1, 17:19]], C.innovation(x, o, H)[:1], [[0.3]])
    xd, Pd, _ = C.observe_dense(x, P, o)
    assert rel(fac.x, xd) < TOL and rel(fac.P, Pd) < TOL
    assert not fac.Lm[:, 1].any() and not fac.Rm[1].any() and fac.nt == 1
    rng = np.random.default_rng(2)
    entries = A.scan(rng, 4)
    for model, z, R, sig in entries:
        fac.append_jacobian(*A.G_of(model, xd[:3], z), R, A.g_of(model, xd[:3], z), sig)
    xd, sd, Pd = A.append_model_dense(xd, s, Pd, entries)
    assert rel(fac.x, xd) < TOL and rel(fac.P, Pd) < TOL and fac.N == 34
    chain = Pm.chain(rng, 5)
    for model, u, Mn in chain:
        F, V = Pm.F_V_of(model, fac.x[:3], u)
        pose = Pm.f_of(model, fac.x[:3], u)
        fac.predict_affine(F, V @ Mn @ V.T, [pose[0], pose[1], Pm.wrap360(pose[2])])
    xd, Pd, Q = Pm.predict_model_dense(xd, Pd, chain)
    assert rel(fac.x, xd) < TOL and rel(fac.P, Pd) < TOL and rel(fac.Q, Q) < TOL


@pytest.mark.parametrize("leg", ["a_f64", "b_f32_mixed", "c_f32_split", "d_f64_two_shards"])
def test_the_beside_pass_plans_are_sensitive_at_a_reduced_size(leg):
    """tests/test_beside_pass_gpu.py's legs, same inputs and plan generator on a map of 24 tile rows, from the oracle alone: two batches
    move every tile of the sampled rows, and every row that append_model adds has in every tile column of the map before it an entry,
    of at least 20x the leg's row tolerance -- a tile a pass skipped and a row the copy behind the pass lost would both show"""
    import beside_pass_cases as B
    storage, T, batch, batches, _, shards, _ = B.LEGS[leg]
    N0 = 24 * (T // 2) - 2 * batch - 1
    (x, s, d, U), steps, info = B.leg_inputs(leg, N0)
    assert info["crossing_scans"] >= 3
    tested = B.kinds_of(steps, tested_only=True)
    for kind in (("correct", "append_model", "predict_model", "associate_model") if shards else
                 B.PAIR_KINDS + B.QUERY_KINDS + ("append_model", "predict_model")):
        assert tested.get(kind, 0) >= 3, tested
    ref = FactoredEKF(info["N"], "known", max_terms=len(steps) + 4, max_appends=len(info["appended"]))
    ref.load_lowrank_state(x, s, d, U)
    snaps = B.run_oracle(ref, steps, batch, T)
    assert ref.N == info["N"]
    scale, moved, app, _ = B.sensitivity(ref, snaps, info["appended"], T, B.tolerances(storage, len(steps))[2])
    print("%s at %d landmarks: scale %.3g, sampled rows moved %.1f, appended rows %.1f row tolerances" % (leg, ref.N, scale, moved, app))
    assert moved >= 20.0 and app >= 20.0
