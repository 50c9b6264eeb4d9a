"""GPU: every pass that writes float tiles, held PER ENTRY against an F64-tile twin.

The idea.  A float handle keeps x, the robot rows, the strip and the landmarks' own 2 x 2 blocks in F64, and its gathers read tile
operands widened and patch them with the pending pairs in F64.  Loaded with a state whose tile entries ARE floats
(float_pass_cases.representable_state), a float handle and an F64-tile twin of the same cfg.batch given the same update-steps in one
batch produce the same pairs bit for bit; the only difference is the pass, and the twin's is P0 - sum K_i G_i as an F64 fma chain, exact
for float purposes (its own error is at most 2 np 2^-53 A).  The premise is asserted in every case, not assumed: get_x(), get_P()[:3, :]
and get_P_diag_blocks() of the two handles are assert_array_equal after the pass -- they depend on every pair -- and that is a test of
its own: a float handle's gathers equal an F64 handle's on representable tiles (the twin's tile edge differs where F64 tiles have no 256).
For pass after pass on one float handle its x, s and P are read after a pass (tile entries are floats again) and loaded into a fresh twin.

The bars (float_pass_cases.py; A = sum_i |K_i| |G_i| per entry from the NumPy restatement of the same steps, u = 2^-24,
q = |got - twin| / (u A + ulp32(twin) / 2), tile entries only):
  1  F64 arithmetic: |got - twin| <= ulp32(twin) / 2 + 2^-40 A.  One rounding, nothing else.
  2  F32 / split arithmetic, any summation order: |got - twin| <= ulp32(max(|got|, |twin|)) / 2 + 1.01 (2 np + 2) u A
     (split: 12 np in place of 2 np, + 2^-23 A).  Catches lost, doubled or misplaced contributions.
  3  against the reference arithmetic: max q and mean q of the kernel at most MARGIN = 2 x those of the NumPy emulation of the stated
     arithmetic (slot order) on the same pairs.  The margin and both of its sides are measured in tests/test_float_pass_arith_cpu.py:
     another summation order costs at most 1.05 x the slot-order emulation, the cheapest mutant (the (3,1) partial product dropped, 64
     pairs) 3.76 x (max q) and 3.87 x (mean q).  For the split kernel also the project's claim: its max q and mean q
     are not above MARGIN x those of the fmaf-chain KERNEL on the same state and pairs.
Every case asserts which kernel ran and with how many pairs, and prints the kernel, np, max q, mean q and max |err| / ulp32.

Where the plan of this file did not hold by design.  The pair ring of an asynchronous handle has 2 x batch slots (host/passes.h
create_passes: pcap), but a pass's pairs never start off a batch boundary nor wrap the ring's end: pstart only moves in
retire_inflight, by the nfrozen = batch pairs of the pass that retires, and a synchronous flush sets it back to 0 -- it only ever is 0
or batch.  The ring leg below therefore covers what a handle can reach: full passes from slot 0 and from slot batch (up to the ring's
last slot), and an odd partial flush that starts at slot batch.  At 1 100 landmarks the split sum's own emulation would take a
quarter of a minute: those two cases are held to bar 2 and, for bar 3, to the fmaf chain's emulation and kernel (the sharper side).

MEASURED (one run on an MI355X; max q / mean q; the same table is in DESIGN.md section 5):
  bar 1, max |err| / ulp32 (max q):
    k_flush_mfma<float,256,4|8>        N 300 / 256, np 1 .. 64            0.4999864 .. 0.4999998   (0.626 .. 0.999)
    the same under f32_mixed / f32_split, np 1, 2                        0.4999938, 0.4999995
    k_downdate_w<float,128,8,false> np 1; <..,64,true> np 2 .. 64        0.4999837 .. 0.4999974   (0.637 .. 1.000)
    k_downdate<float,16|32|64,..>      N 40, np 1 / 5 / 20               0.4999123 / 0.4997247 / 0.499943 (the three edges alike)
    k_gather<float,fused downdate>     N 20, np 1                        0.499945
    k_merge_pass<float,256>, 8 merges  0.4999956;  the joint update's k_flush_mfma<float,256,4>, 8 pairings  0.4999957
  bars 2 and 3, kernel | NumPy emulation of its arithmetic | bar 2 used to:
    k_flush_mfma32<256,4,2,3>          N 300, np 3    4.02 / 0.463 | the same to every printed digit | 0.976      np 4    3.47 / 0.441 | same | 0.968
    k_flush_mfma32<256,4,2,3,early>    N 300, np 5    3.98 / 0.443 | same | 0.950     np 9   4.54 / 0.448 | same | 0.826     np 56   8.86 / 0.779 | same | 0.113
                                       N 256, np 5    4.04 / 0.450 | same | 0.940     np 55 10.8  / 0.723 | same | 0.109
    k_flush_strip32<8>                 N 300, np 57   8.94 / 0.784 | same | 0.111     np 64 10.1  / 0.861 | same | 0.097
                                       N 256, np 57  10.7  / 0.744 | same | 0.116     np 64 10.5  / 0.817 | same | 0.090
                                       N 1 100, np 57 9.56 / 0.760 | same | 0.125     np 64 11.0  / 0.831 | same | 0.112
    k_flush_split3<2>  N 300, np 28    5.23 / 0.438 | naive split sum 14.2 / 0.933 | 0.026 | the fmaf-chain kernel 6.74 / 0.567
                              np 32    5.75 / 0.457 | 14.8 / 0.996 | 0.023 | 7.16 / 0.601       np 33   5.70 / 0.494 | 14.2 / 1.01 | 0.025 | 7.29 / 0.612
                              np 48    6.22 / 0.539 | 14.9 / 1.23  | 0.016 | 8.31 / 0.712       np 64   7.57 / 0.657 | 16.6 / 1.51 | 0.013 | 10.1 / 0.861
                       N 1 100, np 28  5.32 / 0.427 | --           | 0.039 | 8.12 / 0.537       np 64   7.34 / 0.635 | --          | 0.014 | 11.0 / 0.831
    f32_split at 27 pairs: k_flush_mfma32<256,4,2,3,early>, 6.57 / 0.558, the f32_mixed handle's bits
    asynchronous, passes 1 .. 4:  f32_mixed, batch 24 (24, 7, 24, 24 pairs)  5.45 / 0.495, 3.90 / 0.431, 5.83 / 0.460, 4.30 / 0.470 (= emulation)
                                  f32_split, batch 32 (32, 29, 32, 32)      4.86 / 0.425, 4.74 / 0.410, 4.42 / 0.409, 3.51 / 0.397
                                                       (naive split sum 12.2 / 0.890, 11.4 / 0.750, 12.6 / 0.802, 9.33 / 0.729)
  The split kernel is closer to the F64 sum than the fmaf-chain kernel at every count tried: 0.65 .. 0.90 of its max q, 0.76 .. 0.81 of its
  mean q.  The whole module takes 10 s.
  Scratch builds of mutant kernels (not committed): the F64-arithmetic matrix-core kernel rounding through float after
  every chunk of pairs fails 26 bar-1 cases here and one incidental bit-for-bit comparison among 177 older float-tile tests; the split
  kernel without its third plane's products, or without the (3,1) product alone, fails all 15 split cases here (np 28: 111 / 8.0 and
  83.0 / 5.6) -- and the root-mean-square line of tests/test_f32_split_gpu.py as well."""
import functools

import numpy as np
import pytest

import float_pass_cases as F
from helpers import RPOS

pytestmark = pytest.mark.gpu
SEED, STEP_SEED = 61, 14
MFMA64, MFMA32, MFMA32_EARLY, STRIP32, SPLIT3 = ("k_flush_mfma<float,256,", "k_flush_mfma32<256,4,2,3>", "k_flush_mfma32<256,4,2,3,early>",
                                                 "k_flush_strip32<8>", "k_flush_split3<2>")


# ------------------------------------------------------------------------------------------------------------------
# shared, computed once, never written to
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _state(N):
    return F.representable_state(N, SEED)


@functools.lru_cache(maxsize=None)
def _steps(N):
    return F.correction_steps(N, 64, STEP_SEED)


@functools.lru_cache(maxsize=None)
def _pairs(N):
    x, P, _ = _state(N)
    return F.dense_batch(x, P, _steps(N))


def _A(N, npairs):
    return _pairs(N).first(npairs).A()


# the pair counts the emulations are asked for per map size: one walk over the 64 pairs serves them all
CHAIN_COUNTS = {300: (3, 4, 5, 7, 8, 9, 27, 55, 56, 57, 60, 63, 64, 28, 31, 32, 33, 47, 48, 49), 256: (3, 4, 5, 7, 8, 9, 55, 56, 57, 60, 63, 64),
                1100: (28, 57, 64)}
SPLIT_COUNTS = {300: (28, 31, 32, 33, 47, 48, 49, 63, 64)}


@functools.lru_cache(maxsize=None)
def _chain_emulations(N):
    return F.chain_prefixes(_state(N)[1], _pairs(N), set(CHAIN_COUNTS[N]))


@functools.lru_cache(maxsize=None)
def _split_emulations(N):
    return F.split_prefixes(_state(N)[1], _pairs(N), set(SPLIT_COUNTS[N]))


def _premise(e, twin):
    """the two handles formed the same pairs: everything kept in F64 is equal bit for bit"""
    assert e.N == twin.N
    np.testing.assert_array_equal(e.get_x(), twin.get_x())
    Pe, Pt = e.get_P(), twin.get_P()
    np.testing.assert_array_equal(Pe, Pe.T)
    np.testing.assert_array_equal(Pe[:3, :], Pt[:3, :])
    np.testing.assert_array_equal(e.get_P_diag_blocks(), twin.get_P_diag_blocks())
    m = F.tile_mask(Pe.shape[0])
    np.testing.assert_array_equal(Pe[m], Pe[m].astype(np.float32).astype(np.float64))      # tile entries are floats
    return Pe, Pt


def _twin_tile(tile):
    return tile if tile in (16, 32, 64, 128) else 0          # F64 tiles have no edge 256: the default (128)


def _one_pass(storage, tile, N, npairs, partial, state=None, steps=None, e=None, asy=False, batch=None):
    """One pass of exactly npairs pairs: the steps in one batch on a float handle (a fresh one, or `e` going on) and on a fresh F64 twin
    loaded with the same state; partial: a flush() in front of the batch's end.  Returns (kernel name, pairs, P, the twin's P, e)."""
    from ekf_slam_amd import Engine
    x, P, s = _state(N) if state is None else state
    steps = _steps(N)[:npairs] if steps is None else steps
    batch = batch or (64 if partial else npairs)
    if e is None:
        e = Engine(capacity=N + 8, storage=storage, tile=tile, batch=batch, async_flush=asy)
        e.set_state(x, P, s)
    twin = Engine(capacity=N + 8, storage="f64", tile=_twin_tile(tile), batch=batch)
    twin.set_state(x, P, s)
    for q in (e, twin):
        for z, R, idx0 in steps:
            q.predict(F.U_STEP); q.correct(z, R, idx0)
    if partial:
        assert e.pending() == twin.pending() == npairs
        e.flush(); twin.flush()
    name, pairs = e.downdate_kernel_name()
    Pe, Pt = _premise(e, twin)
    twin.close()
    return name, pairs, Pe, Pt, e


def _kernel_pass(storage, tile, N, npairs, partial):
    name, pairs, Pe, Pt, e = _one_pass(storage, tile, N, npairs, partial)
    e.close()
    return name, pairs, Pe, Pt


def _report(label, name, pairs, got, twin, A):
    mq, aq, ul = F.figures(got, twin, A)
    print("%s: %s, np = %d: max q %.3f mean q %.4f, max |err| / ulp32 %.7g" % (label, name, pairs, mq, aq, ul))
    return mq, aq, ul


def _hold_bar1(label, name, pairs, got, twin, A):
    _, _, ul = _report(label, name, pairs, got, twin, A)
    assert float(F.bar1(got, twin, A).max()) <= 1.0
    assert ul <= 0.5


def _hold_bars23(label, name, pairs, got, twin, A, split, emulation, chain_kernel=None):
    """bar 2 in the arithmetic the kernel states (split: k_flush_split3 only), bar 3 against `emulation` (the NumPy result in that
    arithmetic on the same pairs) and, where given, against the fmaf-chain kernel's result"""
    mq, aq, _ = _report(label, name, pairs, got, twin, A)
    b2 = float((F.bar2_split if split else F.bar2_f32)(got, twin, A, pairs).max())
    eq, ea, _ = F.figures(emulation, twin, A)
    print("    bar 2 used to %.3f; the emulation: max q %.3f mean q %.4f" % (b2, eq, ea))
    assert b2 <= 1.0
    assert mq <= F.MARGIN * eq and aq <= F.MARGIN * ea
    if chain_kernel is not None:
        cq, ca, _ = F.figures(chain_kernel, twin, A)
        print("    the fmaf-chain kernel on the same state and pairs: max q %.3f mean q %.4f" % (cq, ca))
        assert mq <= F.MARGIN * cq and aq <= F.MARGIN * ca


def _route(npairs_marked):
    """(np, partial) cases of a leg: every np by cfg.batch = np, the marked ones also as a partial flush of a batch of 64"""
    out = []
    for v in npairs_marked:
        npairs, marked = (v[0], True) if isinstance(v, tuple) else (v, False)
        out.append(pytest.param(npairs, False, id="np%d" % npairs))
        if marked:
            out.append(pytest.param(npairs, True, id="np%d-partial" % npairs))
    return out


# ------------------------------------------------------------------------------------------------------------------
# bar 1: F64 arithmetic
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [300, 256])
@pytest.mark.parametrize("npairs,partial", _route([1, 2, 3, 4, (5,), 8, 9, 30, (31,), 32, 33, (63,), 64]))
def test_f64_arithmetic_on_the_matrix_cores_rounds_once(N, npairs, partial):
    name, pairs, got, twin = _kernel_pass("f32", 256, N, npairs, partial)
    assert (name, pairs) == (MFMA64 + ("4>" if npairs <= 30 else "8>"), npairs)
    _hold_bar1("f32, T = 256, N = %d" % N, name, pairs, got, twin, _A(N, npairs))


@pytest.mark.parametrize("storage", ["f32_mixed", "f32_split"])
@pytest.mark.parametrize("npairs", [1, 2])
def test_one_and_two_pairs_take_the_f64_kernel_under_the_other_arithmetics(storage, npairs):
    name, pairs, got, twin = _kernel_pass(storage, 256, 300, npairs, False)
    assert (name, pairs) == (MFMA64 + "4>", npairs)
    _hold_bar1("%s, T = 256, N = 300" % storage, name, pairs, got, twin, _A(300, npairs))


@pytest.mark.parametrize("npairs,partial", _route([1, 2, 5, (20,), 64]))
def test_f64_arithmetic_on_the_valu_tile_128_rounds_once(npairs, partial):
    name, pairs, got, twin = _kernel_pass("f32", 128, 150, npairs, partial)
    assert name.startswith("k_downdate_w<float,128,") and pairs == npairs, (name, pairs)
    _hold_bar1("f32, T = 128, N = 150", name, pairs, got, twin, _A(150, npairs))


@pytest.mark.parametrize("tile", [16, 32, 64])
@pytest.mark.parametrize("N,npairs", [(40, 1), (40, 5), (40, 20), (20, 1)])
def test_f64_arithmetic_on_small_tiles_rounds_once(tile, N, npairs):
    """N = 20, one pair: the one-pair form fused into the gather (at most 24 landmarks, batch 1); N = 40: the generic kernel."""
    name, pairs, got, twin = _kernel_pass("f32", tile, N, npairs, False)
    want = "k_gather<float,fused downdate>" if N == 20 else "k_downdate<float,%d," % tile
    assert name.startswith(want) and pairs == npairs, (name, pairs)
    _hold_bar1("f32, T = %d, N = %d" % (tile, N), name, pairs, got, twin, _A(N, npairs))


# ------------------------------------------------------------------------------------------------------------------
# bars 2 and 3: F32 and split arithmetic
# ------------------------------------------------------------------------------------------------------------------
def _mixed_kernel(npairs):
    return STRIP32 if npairs > 56 else MFMA32_EARLY if npairs > 4 else MFMA32


@pytest.mark.parametrize("N", [300, 256])
@pytest.mark.parametrize("npairs,partial", _route([3, 4, (5,), 7, 8, 9, (55,), 56, (57,), 60, (63,), 64]))
def test_f32_arithmetic_entry_by_entry(N, npairs, partial):
    name, pairs, got, twin = _kernel_pass("f32_mixed", 256, N, npairs, partial)
    assert (name, pairs) == (_mixed_kernel(npairs), npairs)
    _hold_bars23("f32_mixed, N = %d" % N, name, pairs, got, twin, _A(N, npairs), False, _chain_emulations(N)[npairs])


@pytest.mark.parametrize("npairs,partial", _route([27, (28,), 31, 32, 33, 47, (48,), 49, (63,), 64]))
def test_split_arithmetic_entry_by_entry(npairs, partial):
    N = 300
    name, pairs, got, twin = _kernel_pass("f32_split", 256, N, npairs, partial)
    split = npairs >= 28                                     # 27 pairs: still the F32-arithmetic kernel, held to ITS arithmetic
    assert (name, pairs) == (SPLIT3 if split else MFMA32_EARLY, npairs)
    cname, cpairs, chain, ctwin = _kernel_pass("f32_mixed", 256, N, npairs, partial)
    assert cname == _mixed_kernel(npairs) and cpairs == npairs
    np.testing.assert_array_equal(ctwin, twin)
    emulation = (_split_emulations(N) if split else _chain_emulations(N))[npairs]
    _hold_bars23("f32_split, N = %d" % N, name, pairs, got, twin, _A(N, npairs), split, emulation, chain)
    if not split:
        np.testing.assert_array_equal(got, chain)            # the same kernel on the same pairs


@pytest.mark.parametrize("storage,npairs", [("f32_mixed", 64), ("f32_mixed", 57), ("f32_split", 64), ("f32_split", 28)])
def test_the_strip_work_list_with_two_column_ranges(storage, npairs):
    """1 100 landmarks: nine tile rows, the last one ragged -- the smallest map whose strip work list has two column ranges and full
    16-item segments."""
    N = 1100
    name, pairs, got, twin = _kernel_pass(storage, 256, N, npairs, False)
    split = storage == "f32_split"
    assert (name, pairs) == (SPLIT3 if split else STRIP32, npairs)
    chain = None
    if split:
        cname, _, chain, ctwin = _kernel_pass("f32_mixed", 256, N, npairs, False)
        assert cname == _mixed_kernel(npairs)
        np.testing.assert_array_equal(ctwin, twin)
    _hold_bars23("%s, N = %d" % (storage, N), name, pairs, got, twin, _A(N, npairs), split, _chain_emulations(N)[npairs], chain)


@pytest.mark.parametrize("storage,batch,odd", [("f32_mixed", 24, 7), ("f32_split", 32, 29)])
def test_pass_after_pass_on_one_asynchronous_handle(storage, batch, odd):
    """Four consecutive passes on ONE float handle with cfg.async_flush, a fresh twin per pass.  The ring has 2 x batch slots
    (host/passes.h: pcap); pstart moves by the retiring pass's batch pairs (retire_inflight) and returns to 0 behind a synchronous
    flush (flush_pending).  Pass 1: a full batch in slots [0, batch), launched beside the main stream into the second tile store; reading
    the state retires it: pstart = batch.  Pass 2: `odd` steps in slots [batch, batch + odd), then flush(): a ragged last chunk read from
    the ring's second half, in place; pstart = 0.  Pass 3: a full batch from slot 0 again, asynchronous; retired: pstart = batch.  Pass 4:
    a full batch in slots [batch, 2 batch), up to the ring's last slot, into the other store."""
    N = 300
    split = storage == "f32_split"
    state, e = _state(N), None
    steps = F.correction_steps(N, 3 * batch + odd, STEP_SEED + 1)
    at = 0
    for k, count in enumerate((batch, odd, batch, batch)):
        mine = steps[at:at + count]
        at += count
        name, pairs, got, twin, e = _one_pass(storage, 256, N, count, count != batch, state=state, steps=mine, e=e, asy=True, batch=batch)
        want = SPLIT3 if split and count >= 28 else _mixed_kernel(count)
        assert (name, pairs) == (want, count)
        host = F.dense_batch(state[0], state[1], mine)
        in_split = want == SPLIT3
        emulation = (F.emulate_split if in_split else F.emulate_chain)(state[1], host)
        _hold_bars23("%s, asynchronous, batch %d, pass %d" % (storage, batch, k + 1), name, pairs, got, twin, host.A(), in_split, emulation)
        state = (e.get_x(), got, e.get_s())
    e.close()


# ------------------------------------------------------------------------------------------------------------------
# bar 1 again: the passes of the map edits and of the joint update
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["f32", "f32_mixed"])
def test_the_merge_pass_rounds_a_surviving_entry_once(storage):
    from ekf_slam_amd import Engine
    from merge_batch_cases import dense_of, planted
    N = 300
    x, s, d, U, pairs = planted(N, 7)
    pairs = pairs[:8]
    P = F.representable(dense_of(d, U))
    e = Engine(capacity=N + 8, storage=storage, tile=256, batch=8)
    twin = Engine(capacity=N + 8, storage="f64", batch=8)
    for q in (e, twin):
        q.set_state(x, P, s)
    d2 = e.merge_landmarks_batch(pairs, RPOS)
    np.testing.assert_array_equal(d2, twin.merge_landmarks_batch(pairs, RPOS))
    name, npairs = e.downdate_kernel_name()
    assert name.startswith("k_merge_pass") and npairs == 8, (name, npairs)
    assert e.N == N - 8
    got, exact = _premise(e, twin)
    gone = [3 + 2 * dr + r for _, dr in pairs for r in range(2)]
    A = np.delete(np.delete(F.merge_pairs(x, P, pairs, RPOS).A(), gone, axis=0), gone, axis=1)
    _hold_bar1("%s, a batch of 8 merges" % storage, name, npairs, got, exact, A)
    e.close(); twin.close()


@pytest.mark.parametrize("storage", ["f32", "f32_mixed"])
def test_the_joint_updates_pass_rounds_once(storage):
    from ekf_slam_amd import Engine
    import joint_cases as J
    import observe_joint_cases as C
    from removal_cases import lowrank_data
    N = 300
    x, P0 = J.dense_state(N, 5)
    P, s = F.representable(P0), lowrank_data(N, 5)[1]
    ents, lms = C.scan_of(x, 8, N)
    e = Engine(capacity=N + 8, storage=storage, tile=256, batch=8)
    twin = Engine(capacity=N + 8, storage="f64", batch=8)
    for q in (e, twin):
        q.set_state(x, P, s)
    rec, rec_twin = e.observe_model_joint(ents, lms), twin.observe_model_joint(ents, lms)
    assert rec["outcome"] == C.APPLIED and rec["pairings"] == 8 and rec["d2"] == rec_twin["d2"]
    name, npairs = e.downdate_kernel_name()
    assert (name, npairs) == (MFMA64 + "4>", 8)
    got, exact = _premise(e, twin)
    _hold_bar1("%s, a joint update of 8 pairings" % storage, name, npairs, got, exact, F.joint_pairs(x, P, ents, lms).A())
    e.close(); twin.close()
