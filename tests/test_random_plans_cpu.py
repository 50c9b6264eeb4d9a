"""CPU: the plans of tests/test_random_schedules_gpu.py do what tests/random_plans.py claims (no GPU time on a generator that does not)."""
from collections import Counter

from random_plans import FLUSHING, NSEEDS, ROWS, expected_kernel, full_batch_stretches, landmark_counts, plan

PLANS = [plan(s) for s in range(NSEEDS)]


def test_every_row_of_the_configuration_table_is_present():
    kernels = {c["kernel"] for c, _ in PLANS}
    want = {"k_downdate_w<double,128,4,false", "k_flush_mfma<double,128,4,64>", "k_flush_mfma<double,128,4>", "k_flush_mfma<double,128,8>",
            "k_downdate<double,16,16>", "k_downdate<double,32,16>", "k_downdate_w<double,64,64,true>",
            "k_flush_mfma<float,256,4>", "k_flush_mfma<float,256,8>", "k_downdate<float,16,16>", "k_downdate_w<float,128,64,true>",
            "k_downdate_w<float,128,8,false", "k_flush_mfma32<256,4,2,3>", "k_flush_mfma32<256,4,2,3,early>", "k_flush_strip32<8>",
            "k_flush_split3<2>"}
    assert want <= kernels, sorted(want - kernels)
    for r, (storage, tiles, batches) in enumerate(ROWS):
        mine = [c for c, _ in PLANS if c["storage"] == storage and c["tile"] in tiles and c["batch"] in batches]
        assert {c["async_flush"] for c in mine} == {False, True}, (r, storage)
    f32_256 = {c["batch"] for c, _ in PLANS if c["storage"] == "f32" and c["tile"] == 256}
    assert {1, 8, 40, 64} <= f32_256
    f32_mixed = {c["batch"] for c, _ in PLANS if c["storage"] == "f32_mixed"}
    assert f32_mixed & {1, 2} and f32_mixed & {3, 4} and f32_mixed & set(range(5, 57)) and f32_mixed & set(range(57, 65))
    assert any(c["async_flush"] and c["batch"] == 1 for c, _ in PLANS)
    assert {c["shards"] for c, _ in PLANS} == {1, 2, 3, 4, "comm"}
    assert {c["device_assoc"] for c, _ in PLANS} == {0, 1, 2, 3}
    assert {c["w_pos"] for c, _ in PLANS} == {0.0, 1.0}
    assert {c["cadence"] for c, _ in PLANS} == {1, 4, 16}
    for c, _ in PLANS:
        assert c["kernel"] == expected_kernel(c["storage"], c["tile"], c["batch"])
        assert c["storage"] in ("f64", "f32") or c["tile"] == 256            # what ekf_create accepts
        assert c["tile"] != 256 or c["storage"] != "f64"


def _row(c):
    return next(r for r, (storage, tiles, batches) in enumerate(ROWS)
                if c["storage"] == storage and c["tile"] in tiles and c["batch"] in batches)


def test_every_row_is_crossed_with_every_association_mode_weight_and_shard_layout():
    """Within each row of the table, not merely somewhere among the 64 seeds: all four association modes, both weights (each with the
    asynchronous pass off and on), every shard layout, and the device-resident loop (device_assoc 3) running a measure() scan."""
    for r in range(len(ROWS)):
        mine = [(c, ops) for c, ops in PLANS if _row(c) == r]
        assert {c["device_assoc"] for c, _ in mine} == {0, 1, 2, 3}, r
        assert {c["shards"] for c, _ in mine} == {1, 2, 3, 4, "comm"}, r
        assert {(c["w_pos"], c["async_flush"]) for c, _ in mine} == {(0.0, False), (0.0, True), (1.0, False), (1.0, True)}, r
        assert any(c["device_assoc"] == 3 and any(o["op"] == "measure" for o in ops) for c, ops in mine), r
    # the device-resident loop meets float tiles with the asynchronous pass off and on
    loop_float = {c["async_flush"] for c, ops in PLANS if c["storage"] != "f64" and c["device_assoc"] == 3 and
                  any(o["op"] == "measure" for o in ops)}
    assert loop_float == {False, True}
    for c, ops in PLANS:
        assert any(o["op"] == "measure" for o in ops), c["seed"]


def test_sizes_sit_on_tile_row_edges():
    near = 0
    for c, _ in PLANS:
        N0 = c["N0"]
        if c["tile"] == 256:
            assert 100 <= N0 <= 700
            near += 1 <= (-N0) % 128 <= 8
        elif c["tile"] == 128:
            assert 40 <= N0 <= 400 and min(N0 % 64, 64 - N0 % 64) <= 8
        else:
            assert 3 <= N0 <= 120
        assert c["cap"] == N0 + 40
    assert near >= sum(c["tile"] == 256 for c, _ in PLANS) // 2 - 2


def test_every_seed_has_two_full_batch_stretches_and_its_length():
    for c, ops in PLANS:
        runs = full_batch_stretches(c, ops)
        assert sum(r // c["batch"] for r in runs) >= 2, (c["seed"], runs)
        assert len(ops) >= max(60, 3 * c["batch"] + 20), c["seed"]


def test_every_op_kind_appears_at_least_three_times():
    kinds = Counter(o["op"] for _, ops in PLANS for o in ops)
    for k in ("predict", "correct", "append", "associate", "measure", "pblock", "diag", "shrink", "lowrank", "save", "load", "hint",
              "prefetch", "prefetch_next"):
        assert kinds[k] >= 3, (k, kinds[k])
    assert sum(o["op"] == "associate" and o["costs"] for _, ops in PLANS for o in ops) >= 3
    assert sum(o["op"] == "correct" and o["local"] for _, ops in PLANS for o in ops) >= 3
    # lowrank both ways, hints both ways
    lr = [(n[i], o["N"]) for c, ops in PLANS for n in [landmark_counts(c, ops)] for i, o in enumerate(ops) if o["op"] == "lowrank"]
    assert sum(b < a for a, b in lr) >= 3 and sum(b > a for a, b in lr) >= 3
    hints = [(o["k"], ops[i + 2]["k"]) for _, ops in PLANS for i, o in enumerate(ops) if o["op"] == "hint"]
    assert sum(a == b for a, b in hints) >= 3 and sum(a != b for a, b in hints) >= 3


def test_plans_respect_the_libraries_preconditions():
    for c, ops in PLANS:
        Ns = landmark_counts(c, ops)
        saved = set()
        for i, o in enumerate(ops):
            N = Ns[i]
            assert 1 <= N <= c["cap"] and Ns[i + 1] <= c["cap"], (c["seed"], i)
            if o["op"] in ("correct", "associate"):
                assert 0 <= o["k"] < N
            if o["op"] == "shrink":
                assert 1 <= o["N"] < N
            if o["op"] == "measure":
                assert N + 1 < c["cap"] and all(0 <= k < N for k in o["ks"])
            if o["op"] in ("prefetch", "prefetch_next"):
                assert c["shards"] != 1 and 1 <= len(o["ks"]) <= c["batch"] and all(0 <= k < N for k in o["ks"])
            if o["op"] == "prefetch_next":
                assert c["batch"] > 1 and not c["async_flush"] and c["storage"] in ("f64", "f32")
            if o["op"] == "hint":
                assert c["shards"] != 1 and c["batch"] == 1 and ops[i + 1]["op"] == ops[i + 2]["op"] == "correct"
            if o["op"] == "save":
                saved.add(o["tag"])
            if o["op"] == "load":
                assert o["tag"] in saved and o["tag"] < i
            if o["op"] == "correct" and o["local"]:
                # a group corrects without an exchange only on a prefetched landmark before the batch boundary, no append between
                assert c["shards"] not in (1,)
                j = i - 1
                while ops[j]["op"] == "correct" and ops[j]["local"]:
                    j -= 1
                assert ops[j]["op"] in ("prefetch", "prefetch_next"), (c["seed"], i)
                assert o["k"] in ops[j]["ks"]


def _crosses_edge_after_reload(c, ops):
    Ns, half = landmark_counts(c, ops), c["half"]
    for i, o in enumerate(ops):
        if o["op"] in ("shrink", "lowrank", "load"):
            row = (Ns[i + 1] + half - 1) // half
            if any((Ns[j] + half - 1) // half > row for j in range(i + 1, len(Ns)) if all(
                    ops[q]["op"] not in ("shrink", "lowrank", "load") for q in range(i + 1, min(j, len(ops))))):
                return True
    return False


def test_reloads_are_followed_by_appends_across_a_tile_row_edge():
    assert sum(_crosses_edge_after_reload(c, ops) for c, ops in PLANS) >= 8
    for c, ops in PLANS:
        Ns = landmark_counts(c, ops)
        # every plan: a shrink, low-rank loads below and above the current size, and a checkpoint loaded into a handle that has grown
        # since the save
        assert any(o["op"] == "shrink" for o in ops), c["seed"]
        lr = [(Ns[i], o["N"]) for i, o in enumerate(ops) if o["op"] == "lowrank"]
        assert any(b < a for a, b in lr) and any(b > a for a, b in lr), (c["seed"], lr)
        loads = [(Ns[i], Ns[o["tag"]]) for i, o in enumerate(ops) if o["op"] == "load"]
        assert loads and all(now > then for now, then in loads), (c["seed"], loads)


def test_async_passes_stay_in_flight_across_appends_and_read_free_stretches():
    n = 0
    for c, ops in PLANS:
        if not c["async_flush"] or c["cadence"] == 1:
            continue
        since, appended, free = 0, False, 0
        for i, o in enumerate(ops):
            if o["op"] in FLUSHING:
                since, appended, free = 0, False, 0
                continue
            if o["op"] == "correct":
                since += 1
            if since >= c["batch"]:                 # a pass in flight from here until the next flushing op
                appended |= o["op"] == "append"
                free = free + 1 if (i + 1) % c["cadence"] else 0
                if appended and free >= 3:
                    n += 1
                    break
    assert n >= 8, n


def test_plans_are_deterministic():
    for s in range(NSEEDS):
        assert plan(s) == PLANS[s]
