"""Pure-NumPy side of the per-entry tests of the passes over float tiles (tests/test_float_pass_arith_cpu.py,
tests/test_float_pass_entries_gpu.py).  No GPU, no library.

One pass over float tiles leaves, in every tile entry, fl32(P0 - sum_i K_i G_i): np pairs (K_i: n x 2, G_i: 2 x n), the update summed
in one of three stated arithmetics and added to the float tile value once.  This module holds
  * the state those tests start from (representable_state: every tile entry IS a float, so an F64-tile handle loaded with it holds the
    same numbers as a float handle);
  * the pairs of a batch of update-steps, restated with oracle/ekf_dense.py's own functions (dense_batch), and of a batch of merges and
    of a joint update (merge_pairs, joint_pairs), each with A = sum_i |K_i| |G_i| per entry: the scale every rounding of the pass is
    proportional to;
  * the unit the tests measure in (unit): q = |got - exact| / (u A + ulp32(exact) / 2), u = 2^-24, on tile entries only;
  * NumPy emulations of the three stated arithmetics on those pairs, in several summation orders, and MUTANTS of them (a dropped third
    piece, a dropped partial product, a pair lost in every 16th row) that the bars must catch;
  * the bars themselves (bar1, bar2_f32, bar2_split), derived where they are defined.

Tile entries: P is symmetric and the tiles hold its lower block triangle; entry (r, c), r > c, is updated with K_i(r, :) G_i(:, c).  The
robot rows and columns and the landmarks' own 2 x 2 blocks are kept in F64 by a float handle: they are masked out
(tile_mask)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

U24 = 2.0 ** -24                 # the unit roundoff of a float
MARGIN = 2.0                     # bar 3 (chosen on the CPU: tests/test_float_pass_arith_cpu.py prints both sides and asserts them)
U_STEP = (0.1, 3.0)              # the motion input of every update-step here, as in tests/test_f32_mixed_gpu.py
SPLIT_KEPT = ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0))      # the six partial products (piece of -K, piece of G), smallest class first


# ------------------------------------------------------------------------------------------------------------------
# bfloat16 pieces (flush32_split.h: k_split_pairs)
# ------------------------------------------------------------------------------------------------------------------
def bf16_rn(v):
    """float32 array -> the float32 value of its round-to-nearest-even bfloat16 (integer arithmetic on the bits, as bf16_rn_bits)."""
    u = np.asarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return (r & 0xFFFFFFFF).astype(np.uint32).view(np.float32)


bf16 = bf16_rn


def split3(v):
    v = np.asarray(v, dtype=np.float32)
    b1 = bf16_rn(v)
    r1 = (v - b1).astype(np.float32)
    b2 = bf16_rn(r1)
    r2 = (r1 - b2).astype(np.float32)
    b3 = bf16_rn(r2)
    return b1, b2, b3, r1, r2


# ------------------------------------------------------------------------------------------------------------------
# states
# ------------------------------------------------------------------------------------------------------------------
def kept_mask(n):
    """what a float handle keeps in F64: the robot rows and columns and the landmarks' own 2 x 2 blocks"""
    kept = np.zeros((n, n), dtype=bool)
    kept[:3, :] = kept[:, :3] = True
    for a in range(3, n, 2):
        kept[a:a + 2, a:a + 2] = True
    return kept


def tile_mask(n):
    """the canonical tile entries: strictly below the diagonal, outside the kept set"""
    return np.tril(~kept_mask(n), -1)


def representable(P):
    """P made symmetric (the lower triangle mirrored) with every entry outside the kept set rounded to float"""
    P = np.asarray(P, dtype=np.float64)
    P = np.tril(P) + np.tril(P, -1).T
    kept = kept_mask(P.shape[0])
    return np.where(kept, P, P.astype(np.float32).astype(np.float64))


def representable_state(N, seed):
    """(x, P, s): the state of tests/test_f32_mixed_gpu._state(N, seed), P symmetric and its tile entries floats."""
    rng = np.random.default_rng(seed)
    n = 3 + 2 * N
    x = np.concatenate([[0.3, -0.2, 40.0], rng.uniform(-20, 20, size=2 * N)])
    U = rng.normal(0, 0.05, size=(n, 6))
    P = np.diag(rng.uniform(0.01, 0.1, size=n)) + U @ U.T
    return x, representable(P), np.arange(1, N + 1.0)


def correction_steps(N, count, seed):
    """[(z, R, idx0)] as tests/test_f32_mixed_gpu._run draws them; every step is predict(U_STEP), then correct(z, R, idx0)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        idx0 = int(rng.integers(0, N))
        z = [float(rng.uniform(1, 30)), float(rng.uniform(1, 359))]
        out.append((z, np.diag([z[0] * .01, z[1] * 5.0]), idx0))
    return out


# ------------------------------------------------------------------------------------------------------------------
# the pairs, restated densely
# ------------------------------------------------------------------------------------------------------------------
class Pairs:
    """K: n x 2np (columns 2i, 2i+1: K_i), G: 2np x n (rows 2i, 2i+1: G_i), in slot order; x, P: the dense state after the batch."""

    def __init__(self, K, G, x=None, P=None):
        self.K, self.G, self.x, self.P = np.asarray(K, dtype=np.float64), np.asarray(G, dtype=np.float64), x, P
        self.np = self.G.shape[0] // 2

    def first(self, count):
        return Pairs(self.K[:, :2 * count], self.G[:2 * count])

    def A(self):
        """sum_i |K_i| |G_i| per entry (r, c)"""
        return np.abs(self.K) @ np.abs(self.G)


def dense_batch(x, P, steps, C=0.2):
    """The pairs of a batch of update-steps, each predict(U_STEP) then correct(z, R, idx0), from (x, P): oracle/ekf_dense.py's motion
    model (f), innovation terms and 2 x 2 inverse, with its dense expressions K = P H' inv(phi), P <- (I - K H) P written as the pair
    (K, G = H P) and P <- P - K G, and its F P F' + Q applied to the rows and columns it changes (F is the identity but for F(1,3) and
    F(2,3): the same expression without the n^3 products, so that 1 100 landmarks take seconds)."""
    from oracle import ekf_dense as D
    from oracle.matlab_compat import cosd, inv2, sind, wrapTo360
    x, P = np.array(x, dtype=np.float64), np.array(P, dtype=np.float64)
    Ks, Gs = [], []
    for z, R, idx0 in steps:
        u = U_STEP
        W = np.array([[u[0] * cosd(x[2])], [u[0] * sind(x[2])], [u[1]]])
        x, F = D.f(x, u)
        f02, f12 = F[0, 2], F[1, 2]
        P[0, :] += f02 * P[2, :]; P[1, :] += f12 * P[2, :]
        P[:, 0] += f02 * P[:, 2]; P[:, 1] += f12 * P[:, 2]
        P[0:3, 0:3] += (W * C) @ W.T
        x[2] = wrapTo360(x[2])
        z_k, H_k = D._innovation_terms(x, idx0 + 1)
        G = H_k @ P
        phi = G @ H_k.T + np.asarray(R, dtype=np.float64)
        K = G.T @ inv2(phi)                                  # P symmetric: P H' = (H P)'
        x = x + (K @ (np.array([[z[0]], [z[1]]]) - z_k)).T[0]
        P = P - K @ G
        Ks.append(K); Gs.append(G)
    return Pairs(np.hstack(Ks), np.vstack(Gs), x, P)


def merge_pairs(x, P, pairs, R=None):
    """The pairs of the constraints 'l_keep - l_drop = 0 with noise R' in list order, as tests/merge_cases.constrain_dense writes them
    (G = H P, S = G H' + R, K = G' S^-1, P -= K G), in the numbering before the removal."""
    x, P = np.array(x, dtype=np.float64), np.array(P, dtype=np.float64)
    R = np.zeros((2, 2)) if R is None else np.asarray(R, dtype=np.float64)
    Ks, Gs = [], []
    for keep, drop in pairs:
        ai, aj = 3 + 2 * int(keep), 3 + 2 * int(drop)
        G = P[ai:ai + 2, :] - P[aj:aj + 2, :]
        S = G[:, ai:ai + 2] - G[:, aj:aj + 2] + R
        K = G.T @ np.linalg.inv(S)
        nu = -(x[ai:ai + 2] - x[aj:aj + 2])
        x, P = x + K @ nu, P - K @ G
        Ks.append(K); Gs.append(G)
    return Pairs(np.hstack(Ks), np.vstack(Gs), x, P)


def joint_pairs(x, P, entries, landmarks):
    """The joint update in the form the device runs (tests/observe_joint_cases.joint_update_cholesky): L L' = S, W = L^-1 H P,
    P' = P - W' W: pair i is (W' (:, 2i:2i+2), W(2i:2i+2, :))."""
    import joint_cases as J
    import observe_joint_cases as C
    rec = J.joint_dense(x, P, entries, landmarks)
    rows = C.paired_rows(landmarks)
    H, S = rec["H"][rows], rec["S"][np.ix_(rows, rows)]
    W = np.linalg.solve(np.linalg.cholesky(S), H @ np.asarray(P, dtype=np.float64))
    return Pairs(W.T, W, None, P - W.T @ W)


# ------------------------------------------------------------------------------------------------------------------
# the unit and the bars
# ------------------------------------------------------------------------------------------------------------------
def ulp32(v):
    """the spacing of the floats at |v| (v exact, F64 or wider): 2^(e - 24) for |v| = m 2^e, 0.5 <= m < 1; subnormal spacing at and near 0"""
    _, e = np.frexp(np.abs(np.asarray(v, dtype=np.float64)))
    return np.ldexp(1.0, np.maximum(e - 24, -149))


def _err(got, exact):
    return np.abs(np.asarray(got).astype(np.longdouble) - np.asarray(exact, dtype=np.longdouble)).astype(np.float64)


def unit(got, exact, A):
    """q per tile entry (a vector over tile_mask, row-major): |got - exact| / (u A + ulp32(exact) / 2)"""
    m = tile_mask(np.asarray(exact).shape[0])
    ex = np.asarray(exact)[m]
    return _err(np.asarray(got)[m], ex) / (U24 * A[m] + 0.5 * ulp32(ex))


def ulps(got, exact):
    """|got - exact| / ulp32(exact) per tile entry"""
    m = tile_mask(np.asarray(exact).shape[0])
    ex = np.asarray(exact)[m]
    return _err(np.asarray(got)[m], ex) / ulp32(ex)


def bar1(got, exact, A):
    """Bar 1, F64 arithmetic: excess of |got - exact| over ulp32(exact) / 2 + 2^-40 A, per tile entry, as a ratio (<= 1 passes).  One
    rounding of the exact value to float; the second term covers the F64 chain's own roundings (at most 2 np 2^-53 A) and ties."""
    m = tile_mask(np.asarray(exact).shape[0])
    ex = np.asarray(exact)[m]
    return _err(np.asarray(got)[m], ex) / (0.5 * ulp32(ex) + 2.0 ** -40 * A[m])


def _bar2(got, exact, A, terms, extra):
    m = tile_mask(np.asarray(exact).shape[0])
    g, ex = np.asarray(got)[m], np.asarray(exact)[m]
    top = np.maximum(np.abs(np.asarray(g, dtype=np.float64)), np.abs(np.asarray(ex, dtype=np.float64)))
    return _err(g, ex) / (0.5 * ulp32(top) + (1.01 * terms * U24 + extra) * A[m])


def bar2_f32(got, exact, A, npairs):
    """Bar 2, F32 arithmetic in ANY summation order, as a ratio (<= 1 passes): -K and G rounded to float (2 u per product), the 2 np
    products accumulated in float (each partial sum is at most A (1 + small), one u each: 2 np u A; 1.01 covers the second-order terms),
    one final add of the float tile (u of the update + half an ulp of the result)."""
    return _bar2(got, exact, A, 2 * npairs + 2, 0.0)


def bar2_split(got, exact, A, npairs):
    """Bar 2, split arithmetic: six partial products per product (12 np accumulations), and 2^-23 A for the three dropped ones
    (tests/test_split3_arith_cpu.py)."""
    return _bar2(got, exact, A, 12 * npairs + 2, 2.0 ** -23)


# ------------------------------------------------------------------------------------------------------------------
# the stated arithmetics, emulated on the pairs
# ------------------------------------------------------------------------------------------------------------------
def exact_pass(P0, pairs):
    """P0 - sum_i K_i G_i in extended precision (np.longdouble: 64 significant bits on x86-64), the reference of the CPU test"""
    return np.asarray(P0, dtype=np.longdouble) - pairs.K.astype(np.longdouble) @ pairs.G.astype(np.longdouble)


def emulate_f64_once(P0, pairs):
    """F64 arithmetic (k_flush_mfma<float,...>, k_downdate*<float,...>): the tile value widened, the pairs applied as an F64 chain in slot
    order, rounded to float once."""
    acc = np.array(P0, dtype=np.float64)
    for t in range(pairs.G.shape[0]):
        acc -= np.outer(pairs.K[:, t], pairs.G[t])
    return acc.astype(np.float32)


def order_slots(npairs):
    return [list(range(npairs))]


def order_reversed(npairs):
    return [list(range(npairs))[::-1]]


def order_chunks4(npairs):
    """chunks of four pairs summed each from zero, the chunk sums then added in order"""
    return [list(range(c, min(c + 4, npairs))) for c in range(0, npairs, 4)]


def _f32_operands(pairs):
    return (-pairs.K).astype(np.float32), pairs.G.astype(np.float32)


def _fma_terms(Kn, G, group, lost=None):
    """the float sum, from zero, of the products of the pairs of `group`, as a chain of fmaf (the product exact, one rounding per term:
    formed in F64, where a product of two floats is exact, and rounded to float with the partial sum -- the F64 add's own rounding is
    2^-29 of a float ulp)"""
    acc = np.zeros((Kn.shape[0], G.shape[1]), dtype=np.float32)
    for i in group:
        for t in (2 * i, 2 * i + 1):
            term = np.outer(Kn[:, t].astype(np.float64), G[t].astype(np.float64))
            if lost is not None and i == lost[1]:
                term[lost[0]] = 0.0
            acc = (acc.astype(np.float64) + term).astype(np.float32)
    return acc


def _combine(parts):
    acc = parts[0]
    for p in parts[1:]:
        acc = acc + p                                        # float32 + float32: one correctly rounded float add
    return acc


def emulate_chain(P0, pairs, order=order_slots, lost=None):
    """F32 arithmetic (k_flush_mfma32, k_flush_strip32): -K and G rounded to float, the update summed from zero by fmaf in the given
    order, the float tile value added once.  lost = (rows, pair): that pair's products are left out in those rows (a mutant)."""
    Kn, G = _f32_operands(pairs)
    upd = _combine([_fma_terms(Kn, G, g, lost) for g in order(pairs.np)])
    return np.asarray(P0, dtype=np.float32) + upd


def emulate_split(P0, pairs, order=order_slots, kept=SPLIT_KEPT, pieces=3, lost=None):
    """Split arithmetic (k_flush_split3): the float operands cut into three bf16 pieces by split3's rule, the partial products `kept`
    (each exact in float), summed in float from zero -- pair after pair in the given order, within a pair both columns' products in
    `kept`'s order -- and the float tile value added once.  pieces = 2 drops the third piece altogether (a mutant), as does leaving
    a product out of `kept`."""
    Kn, G = _f32_operands(pairs)
    Kp, Gp = split3(Kn)[:3], split3(G)[:3]
    use = [(p, q) for p, q in kept if p < pieces and q < pieces]
    parts = []
    for group in order(pairs.np):
        acc = np.zeros((Kn.shape[0], G.shape[1]), dtype=np.float32)
        for i in group:
            for t in (2 * i, 2 * i + 1):
                for p, q in use:
                    term = np.outer(Kp[p][:, t], Gp[q][t])   # 8 x 8 significant bits: exact in float32
                    if lost is not None and i == lost[1]:
                        term[lost[0]] = 0.0
                    acc = acc + term
        parts.append(acc)
    return np.asarray(P0, dtype=np.float32) + _combine(parts)


def chain_prefixes(P0, pairs, counts):
    """{count: emulate_chain(P0, pairs.first(count))} for every count of `counts`, from ONE walk over the pairs: in slot order the sum of
    the first count pairs is a prefix of the sum of all of them."""
    Kn, G = _f32_operands(pairs)
    tile = np.asarray(P0, dtype=np.float32)
    acc, out = np.zeros((Kn.shape[0], G.shape[1]), dtype=np.float32), {}
    for i in range(max(counts)):
        acc = _fma_onto(acc, Kn, G, i)
        if i + 1 in counts:
            out[i + 1] = tile + acc
    return out


def _fma_onto(acc, Kn, G, i):
    for t in (2 * i, 2 * i + 1):
        acc = (acc.astype(np.float64) + np.outer(Kn[:, t].astype(np.float64), G[t].astype(np.float64))).astype(np.float32)
    return acc


def split_prefixes(P0, pairs, counts):
    """the same for emulate_split in slot order"""
    Kn, G = _f32_operands(pairs)
    Kp, Gp = split3(Kn)[:3], split3(G)[:3]
    tile = np.asarray(P0, dtype=np.float32)
    acc, out = np.zeros((Kn.shape[0], G.shape[1]), dtype=np.float32), {}
    for i in range(max(counts)):
        for t in (2 * i, 2 * i + 1):
            for p, q in SPLIT_KEPT:
                acc = acc + np.outer(Kp[p][:, t], Gp[q][t])
        if i + 1 in counts:
            out[i + 1] = tile + acc
    return out


def lost_rows(n, npairs):
    """the 'one pair lost in every 16th row' mutant: the last pair, rows 15, 31, ..."""
    return (np.arange(15, n, 16), npairs - 1)


def split_mutants(P0, pairs):
    """{name: result} of the four mutants of the split arithmetic"""
    n = pairs.K.shape[0]
    return {"third piece dropped": emulate_split(P0, pairs, pieces=2),
            "(2,2) dropped": emulate_split(P0, pairs, kept=[pq for pq in SPLIT_KEPT if pq != (1, 1)]),
            "(3,1) dropped": emulate_split(P0, pairs, kept=[pq for pq in SPLIT_KEPT if pq != (2, 0)]),
            "a pair lost in every 16th row": emulate_split(P0, pairs, lost=lost_rows(n, pairs.np))}


def chain_mutants(P0, pairs):
    return {"a pair lost in every 16th row": emulate_chain(P0, pairs, lost=lost_rows(pairs.K.shape[0], pairs.np))}


def figures(got, exact, A):
    """(max q, mean q, max |err| / ulp32)"""
    q = unit(got, exact, A)
    return float(q.max()), float(q.mean()), float(ulps(got, exact).max())
