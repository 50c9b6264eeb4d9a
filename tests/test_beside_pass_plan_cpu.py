"""CPU: the plans of tests/beside_pass_cases.py, without a GPU.

1. make_plan without `newer` is what it was before that keyword existed: the digests below were taken from the four legs of LEGS and from
   EDITS_LEG, at the reduced size of test_oracle_factored.py's test_the_beside_pass_plans_are_sensitive_at_a_reduced_size, BEFORE the file
   was touched.  The float legs' inputs were fitted with small margins (rows 1.35e-7 of 2e-7, sensitivity 31 of 20): they must not move.
2. make_plan(newer=True), the plan of tests/test_beside_pass_newer_gpu.py: every new kind is there as often as that file needs it, five
   synchronising calls stand directly behind a scan that crosses a tile-row edge, an observe_model_assigned scan straddles a batch boundary
   -- all three derived from the plan alone, in pair slots --, the dense forms run it through with every gated update applied, every
   factor_map occurrence definite and P positive definite at every boundary, and the assigned scans have no choice: one candidate per
   entry, the intended landmark.
3. The plan at full size (~20 000 landmarks) is generated in seconds: it reads no engine and builds no dense P.

The dense run is at tile 16 (175 -> 346 landmarks, ~3 s).  At T = 128 the reduced map has 1519 landmarks and factor_dense's unblocked loop
alone would take minutes; the plan's own structure is checked at T = 128 too."""
import time

import numpy as np
import pytest

import async_cases
import beside_pass_cases as B

BATCH = 8
DIGESTS = {
    "a_f64": "92361c4d2feb1b410016b55a793edafe9fb4daa31cf100ac2fa2263a776ac090",
    "b_f32_mixed": "a1444957723e4e9069973b9ee1cbbc8c2d8d0aff0c62f5b318ce72d87ed264cc",
    "c_f32_split": "026c85476bb11da421ee5998069161e606c085f61424a6610c0db273b4e76bb3",
    "d_f64_two_shards": "fcc32a6cbf7b4d57885349fa909dfa1d8ec1dae71e725ae43f3a94c3b83a1590",
    "edits": "63d1d43ca540bad77b569579912b962843242b04301a3de8cc726acf33fd9460",
}


def reduced(T, batch):
    return 24 * (T // 2) - 2 * batch - 1


@pytest.mark.parametrize("leg", list(DIGESTS))
def test_the_plans_without_newer_are_what_they_were(leg):
    if leg == "edits":
        storage, T, batch, batches, _, _, key = B.EDITS_LEG
        sigma, sigma_robot, RC = async_cases.INPUTS[key]
        (x, _, _, _), _ = async_cases.make_inputs(reduced(T, batch), 0, sigma, sigma_robot, RC)
        steps, _ = B.make_plan(x, T, batch, batches, RC, edits=True)
    else:
        _, T, batch, _, _, _, _ = B.LEGS[leg]
        _, steps, _ = B.leg_inputs(leg, reduced(T, batch))
    assert B.plan_digest(steps) == DIGESTS[leg]
    assert all(taken == 1 for _, _, taken in B.places(steps, batch))


def test_the_digest_sees_every_part_of_a_plan():
    _, steps, _ = B.leg_inputs("a_f64", reduced(128, 8))
    base = B.plan_digest(steps)
    kind, payload, tested = steps[20][-1]
    for other in ((kind + "x", payload, tested), (kind, payload, not tested)):
        assert B.plan_digest(steps[:20] + [steps[20][:-1] + [other]] + steps[21:]) != base
    u = steps[0][0][1].copy()
    u[1] = np.nextafter(u[1], 1.0)
    assert B.plan_digest([[(steps[0][0][0], u, steps[0][0][2])] + steps[0][1:]] + steps[1:]) != base


def newer_plan(T, N0):
    sigma, sigma_robot, RC = async_cases.INPUTS["f64"]
    state, _ = async_cases.make_inputs(N0, 0, sigma, sigma_robot, RC)
    steps, info = B.make_plan(state[0], T, BATCH, B.NEWER_BATCHES, RC, newer=True)
    return state, steps, info


def structure(steps, T, N0):
    """From the plan alone: (boundaries: step -> k_b, the (step, kind) of the synchronising calls that stand directly behind a tested scan
    which is the first call behind a boundary and carries the map over a tile-row edge, the steps of the assigned scans that straddle a
    boundary, the (step, kind) of every synchronising call that is the first call behind a boundary)"""
    half, N = T // 2, N0
    boundaries, behind, straddle, first = {}, [], [], []
    slot = 0
    for t, (ops, (p, k_b, taken)) in enumerate(zip(steps, B.places(steps, BATCH))):
        calls = [op for op in ops if op[0] not in ("predict", "predict_model")]          # (the motion in front of the step aside)
        for q, (kind, payload, tested) in enumerate(calls):
            before = N
            if kind == "append_model":
                N += len(payload)
            elif kind == "join_map":
                N += len(payload[1])
            if kind in B.SYNC_KINDS and tested and p == 1 and k_b >= 2:
                if q == 0:
                    first.append((t, kind))
                elif q == 1 and calls[0][0] == "append_model" and calls[0][2]:
                    m = len(calls[0][1])
                    if (before - m - 1) // half != (before - 1) // half and (before - m) % half != 0:
                        behind.append((t, kind))
        if (slot + taken) // BATCH != slot // BATCH:
            boundaries[t] = (slot + taken) // BATCH
            if ops[-1][0] == B.NEWER_PAIR_KIND and ops[-1][2] and (slot + taken) % BATCH != 0:
                straddle.append(t)
        slot += taken
    return boundaries, behind, straddle, first


@pytest.mark.parametrize("T", [16, 128])
def test_the_newer_plan_places_every_call_where_the_gpu_test_needs_it(T):
    N0 = reduced(T, BATCH)
    _, steps, info = newer_plan(T, N0)
    boundaries, behind, straddle, first = structure(steps, T, N0)
    tested = B.kinds_of(steps, tested_only=True)
    print("T = %d: %d -> %d landmarks in %d steps; tested %s; behind a crossing scan %s; straddling %s" % (T, N0, info["N"], len(steps), tested, behind, straddle))
    assert boundaries == info["boundaries"] and behind == info["behind_scan"] and straddle == info["straddlers"]
    assert max(boundaries.values()) == B.NEWER_BATCHES
    # each synchronising kind as the first call behind a boundary (transform_map: the exact and the robot form; the uncertain one below) ...
    assert sorted(k for _, k in first) == sorted(["observe_model_joint", "observe_model_joint_iterated", "join_map", "extract_map", "factor_map"] + 2 * ["transform_map"])
    forms = [op[1] for ops in steps for op in ops if op[0] == "transform_map"]
    assert sorted(forms) == ["exact", "robot", "uncertain"]
    assert sorted(op[1][1] for ops in steps for op in ops if op[0] == "extract_map") == ["map", "robot"]
    # ... and five of them a second time directly behind a crossing scan
    assert sorted(k for _, k in behind) == sorted(["factor_map", "transform_map", "extract_map", "join_map", "observe_model_joint"])
    for t, kind in behind:
        calls = [op for op in steps[t] if op[0] not in ("predict", "predict_model")]
        scan = set(range(info_N_before(steps, t, N0), info_N_before(steps, t, N0) + len(calls[0][1])))
        if kind == "transform_map":
            assert calls[1][1] == "uncertain"
        if kind == "extract_map":
            assert scan <= set(calls[1][1][0])
        if kind == "observe_model_joint":
            assert len(scan & set(calls[1][1][1])) == 2
    # one synchronising call per boundary
    assert len({boundary_of(boundaries, t) for t, _ in first + behind}) == len(first) + len(behind)
    # the calls that leave the pass alone
    assert len(straddle) >= 1 and tested[B.NEWER_PAIR_KIND] >= 2
    assert all(tested[k] >= 3 for k in B.NEWER_QUERY_KINDS + B.QUERY_KINDS + B.PAIR_KINDS), tested
    for kind in B.NEWER_QUERY_KINDS:
        at = sorted(p for ops, (p, k_b, _) in zip(steps, B.places(steps, BATCH)) for op in ops if op[0] == kind and op[2])
        assert set(at) == {1, 2, 3, 4}, (kind, at)                     # every place behind a boundary
    # the payloads
    for ops in steps:
        for kind, payload, _ in ops:
            if kind in ("observe_model_joint", "observe_model_joint_iterated"):
                paired = [k for k in payload[1] if k >= 0]
                assert 6 <= len(paired) <= 8 and list(payload[1]).count(-1) == 1 and np.isfinite(payload[2])
                assert len({k // (T // 2) for k in paired}) == len(paired)
                assert {e["model"] for e in payload[0]} == {1, 2, 3, 4}
            elif kind == B.NEWER_PAIR_KIND:
                assert 3 <= len(payload[0]) <= 4 and all(np.isfinite(e["gate"]) for e in payload[0])
            elif kind == "assign_model":
                assert 4 <= len(payload) <= 12
            elif kind == "joint_search":
                assert 4 <= len(payload[0]) <= 6 and len(payload[1]) == 2 * len(payload[0]) + 1


def info_N_before(steps, t, N0):
    N = N0
    for ops in steps[:t]:
        for kind, payload, _ in ops:
            N += len(payload) if kind == "append_model" else len(payload[1]) if kind == "join_map" else 0
    return N


def boundary_of(boundaries, t):
    return max(k for s, k in boundaries.items() if s < t)


def test_the_newer_plan_runs_through_the_dense_forms():
    from oracle import ekf_dense
    T = 16
    N0 = reduced(T, BATCH)
    (x, s, d, U), steps, info = newer_plan(T, N0)
    dense = ekf_dense.EKF_SLAM()
    dense.x, dense.P, dense.s = x.copy(), np.diag(d) + U @ U.T, list(s)
    factors, since_robot_frame = 0, None
    for t, ops in enumerate(steps):
        for kind, payload, _ in ops:
            res = B.apply_dense(dense, kind, payload)             # (asserts APPLIED for every gated update)
            if kind in ("predict", "predict_model") and since_robot_frame is not None:
                since_robot_frame += 1
            if kind == "transform_map" and payload == "robot":
                assert not dense.P[:3].any()
                since_robot_frame = 0
            if kind == "factor_map":
                factors += 1
                assert res["definite"] and np.all(np.isfinite(res["d2"])) and res["min_pivot"] > 0.0
                assert since_robot_frame is None or since_robot_frame >= 1
            if kind == B.NEWER_PAIR_KIND:
                np.testing.assert_array_equal(res["landmark"], payload[1])
                np.testing.assert_array_equal(res["ncand"], 1)
            if kind == "extract_map":
                assert res[0].size == 3 + 2 * len(payload[0])
        if t in info["boundaries"]:
            assert np.abs(dense.P - dense.P.T).max() <= 1e-12 * np.abs(dense.P).max()
            np.linalg.cholesky(0.5 * (dense.P + dense.P.T))      # raises where P is not positive definite
    assert factors == 2 and (dense.x.size - 3) // 2 == info["N"] == len(dense.s)
    assert sorted(info["appended"]) == list(range(N0, info["N"]))


def test_the_newer_plan_at_full_size_is_made_in_seconds():
    T = 128
    N0 = async_cases.placement(T, BATCH)[0]
    sigma, sigma_robot, RC = async_cases.INPUTS["f64"]
    state, _ = async_cases.make_inputs(N0, 0, sigma, sigma_robot, RC)
    t0 = time.perf_counter()
    steps, info = B.make_plan(state[0], T, BATCH, B.NEWER_BATCHES, RC, newer=True)
    took = time.perf_counter() - t0
    print("the newer plan at %d -> %d landmarks: %.1f s" % (N0, info["N"], took))
    assert took < 30.0 and len(info["behind_scan"]) == 5 and len(info["straddlers"]) == 2 and N0 > 19000
