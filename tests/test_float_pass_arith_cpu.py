"""CPU: the three arithmetics a pass over float tiles is stated in (DESIGN.md sections 3 and 5), emulated in NumPy on the pairs of a batch
of update-steps (tests/float_pass_cases.py) and measured PER ENTRY against P0 - sum K_i G_i in extended precision, at 300 landmarks and
3, 28 and 64 pairs.  What tests/test_float_pass_entries_gpu.py asks of the kernels is asked here of the emulations first:

  bar 1  F64 arithmetic: one rounding.  |err| <= ulp32 / 2 (+ 2^-40 A for the F64 chain itself); max |err| / ulp32 <= 0.5.
  bar 2  F32 and split arithmetic in any summation order (slot order, reversed, pairwise by chunks of four): the derived bound of
         float_pass_cases.bar2_f32 / bar2_split.
  bar 3  against the reference arithmetic: max q and mean q (float_pass_cases.unit) at most MARGIN x those of the slot-order emulation.
         MARGIN has to lie ABOVE what another summation order can cost against the slot-order reference and BELOW what the cheapest
         mutant costs; both sides are printed and asserted here.

Measured (N = 300, seed 61, steps of seed 14), max q / mean q:
  np    chain, slots   reversed      chunks of 4   split, slots    reversed       chunks of 4   cheapest mutant of the split sum
   3    4.02 / 0.46    2.48 / 0.45   4.02 / 0.46    5.99 / 0.50    6.28 / 0.47    5.99 / 0.50   102 / 3.79  ((3,1) dropped)
  28    6.74 / 0.57    6.57 / 0.47   2.71 / 0.37   14.2  / 0.93    8.52 / 0.74    4.62 / 0.43    80.8 / 5.71
  64   10.1  / 0.86    7.37 / 0.72   3.53 / 0.39   16.6  / 1.51   13.4  / 1.25    3.84 / 0.44    62.4 / 5.85
Another order against the slot-order reference: at most 1.05 (split, reversed, np = 3; every other one is BELOW the reference: a sum by
chunks is the better sum).  Cheapest mutant against the healthy slot-order sum: 3.76 (max q) and 3.87 (mean q), at np = 64; 5.7 at 28; 17
and 7.6 at 3.  A pair lost in every 16th row: 1e5 and more.  MARGIN = 2 lies a factor 1.9 from either side.
F64 arithmetic: max |err| / ulp32 = 0.4999993, 0.4999969, 0.4999991."""
import numpy as np
import pytest

import float_pass_cases as F

N, SEED, STEP_SEED = 300, 61, 14
ORDERS = (("slot order", F.order_slots), ("reversed", F.order_reversed), ("chunks of 4", F.order_chunks4))


@pytest.fixture(scope="module")
def batch():
    x, P, _ = F.representable_state(N, SEED)
    return P, F.dense_batch(x, P, F.correction_steps(N, 64, STEP_SEED))


def test_the_state_is_representable_and_the_pairs_are_the_dense_update(batch):
    P, full = batch
    np.testing.assert_array_equal(P, P.T)
    m = F.tile_mask(P.shape[0])
    np.testing.assert_array_equal(P[m], P[m].astype(np.float32).astype(np.float64))
    assert m.sum() == N * (N - 1) * 2                        # 2 x 2 cross blocks below the diagonal, nothing of the kept set
    # P0 - sum K_i G_i IS the dense restatement's landmark block after the batch (predict touches the robot rows and columns only)
    got = np.asarray(F.exact_pass(P, full), dtype=np.float64)
    assert np.abs(got - full.P)[m].max() <= 1e-14 * np.abs(P).max()
    # the prefix walks are the slot-order emulations
    pr = full.first(3)
    np.testing.assert_array_equal(F.chain_prefixes(P, full, {3})[3], F.emulate_chain(P, pr))
    np.testing.assert_array_equal(F.split_prefixes(P, full, {3})[3], F.emulate_split(P, pr))


@pytest.mark.parametrize("npairs", [3, 28, 64])
def test_the_emulations_meet_the_bars_and_the_mutants_do_not(batch, npairs):
    P, full = batch
    pr = full.first(npairs)
    A, exact = pr.A(), F.exact_pass(P, pr)
    # bar 1
    got = F.emulate_f64_once(P, pr)
    mq, aq, ul = F.figures(got, exact, A)
    print("np = %2d  F64 arithmetic, rounded once: max q %.3f mean q %.3f, max |err| / ulp32 %.7f" % (npairs, mq, aq, ul))
    assert ul <= 0.5 and F.bar1(got, exact, A).max() <= 1.0
    # bars 2 and 3
    for kind, emulate, bar2, mutants in (("fmaf chain", F.emulate_chain, F.bar2_f32, F.chain_mutants),
                                         ("split sum", F.emulate_split, F.bar2_split, F.split_mutants)):
        ref = None
        for oname, order in ORDERS:
            got = emulate(P, pr, order)
            mq, aq, ul = F.figures(got, exact, A)
            b2 = float(bar2(got, exact, A, npairs).max())
            ref = (mq, aq) if ref is None else ref
            print("np = %2d  %s, %-11s: max q %6.2f mean q %.3f (x %.2f / %.2f of slot order), max |err| / ulp32 %.3g, bar 2 used to %.3f"
                  % (npairs, kind, oname, mq, aq, mq / ref[0], aq / ref[1], ul, b2))
            assert b2 <= 1.0
            assert mq <= F.MARGIN * ref[0] and aq <= F.MARGIN * ref[1]       # the spread between summation orders is inside the margin
        for mname, got in mutants(P, pr).items():
            mq, aq, ul = F.figures(got, exact, A)
            print("np = %2d  %s MUTANT, %s: max q %.4g mean q %.4g (x %.2f / %.2f of the healthy sum)"
                  % (npairs, kind, mname, mq, aq, mq / ref[0], aq / ref[1]))
            assert mq > F.MARGIN * ref[0] and aq > F.MARGIN * ref[1]         # every mutant is outside it
