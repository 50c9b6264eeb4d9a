// Fragment of kernels.hip (included there, inside its anonymous namespace, after solve_map.h; it uses factor_map.h's d4_t, kFactorBlock
// and factor_source and map_blocks.h's chunk_k, segment_of and chunk_tree_sums): the plain product P B on the handle's own tile store (ekf_multiply_map) -- k_multiply_tiles, k_multiply_sum, k_multiply_robot.
#pragma once
#include "map_blocks.h"         // (kernels.hip has it in front already; a host build that names this fragment alone gets it here)

// ---------------------------------------------------------------------------------------------------
// THE PRODUCT (ekf_multiply_map).  P = [Prr Prm; Pmr Pmm] of a flushed handle is exactly what ekf_get_P reports: the landmark block
// Pmm(r, c) = factor_source(r, c) -- float tiles widened, a landmark's own 2 x 2 block from diag[dcur], everything else the CANONICAL
// lower-triangle entry of the handle's tile store (within a diagonal tile too) --, the strip, Prr.  With b = (b_r, b_m):
//     (P b)_m = Pmm b_m + strip' b_r,      (P b)_r = Prr b_r + strip b_m.
// kFactorChunk vectors at a time, one a COLUMN of the chunk (MultiplyMapArgs: the landmark entries first, zero from 2 N on, the
// robot's three behind them), three launches over the handle's own TileMap (edge T = 16 .. 256, nT = tiles_for(2 N) tile rows):
//     k_multiply_tiles  one workgroup per SEGMENT of S tiles (I, J0 .. J1 - 1) of tile row I, four wavefronts.  Per tile, on
//                       v_mfma_f64_16x16x4_f64: the DIRECT part T_IJ B_J, accumulated over the segment into ONE partial block of tile row
//                       I (dpart), and for J < I the TRANSPOSED part T_IJ' B_I, one partial block of tile row J per tile (tpart).  A
//                       diagonal tile is taken as the whole symmetric block in the direct part and has no transposed part.  A
//                       workgroup asks memory for its tile TWICE: the direct part reads it row by row, the transposed part reads the
//                       same lines again (a quarter-wavefront then reads 16 contiguous entries of one tile row: whole lines, as
//                       k_solve_backward).  The second read is MEANT to be served by L2; whether it is has not been measured (a tile
//                       is 128 or 256 KB and several workgroups a CU are in flight: DESIGN.md section 3z).  B_I (once a workgroup) and B_J (once a tile) go through LDS for all
//                       four wavefronts.  The first segment of a tile row also leaves the row's 3 x 16 part of strip B_m (wpart).
//     k_multiply_sum    a lane per entry of the landmark rows, T * 16 / 256 workgroups a tile row
//     k_multiply_robot  one workgroup: the robot rows (queued with the sums; it reads what k_multiply_tiles left, nothing of theirs)
// SELECTION, NOT MULTIPLICATION BY ZERO: an entry of P in a row or column at or beyond 2 N is the constant 0 whatever the store holds
// there (in-place passes skip those rows, removals leave rows behind), the strip likewise; rows at or beyond 2 N are never written.
// ARITHMETIC OF ONE ENTRY, row i = T R + u of the landmark block, vector v.  chunk_k(s, t) is the k order of a tile (map_blocks.h: steps
// s = 0 .. T / 4 - 1, the matrix instruction and its plain-FMA twin); k_multiply_tiles' two loops are tile_mac's form for a run-time
// edge T, float tiles and the multiply_entry path.  (Folded into one function the tile pass measured 1 to 3 % slower: DESIGN.md section 3z.)
//   direct, per segment g of tile row R: d_g = 0, then fma(P(i, T J + k), b_v[T J + k], d_g) over the segment's tiles J ascending and
//     in a tile over k in chunk_k's order;
//   transposed, per tile (I, R), I > R: t_I = 0, then fma(P(T I + k, i), b_v[T I + k], t_I) over k in chunk_k's order;
//   the entry: ((((d_0 + d_1) + ..) + t_{R+1}) + t_{R+2} + ..), then fma(strip[2][i], b_r[2], fma(strip[1][i], b_r[1], fma(strip[0][i],
//     b_r[0], .))).
// Robot row q: per tile row I a chain w_I = fma(strip[q][T I + u], b_v[T I + u], .) over u ascending (rows at or beyond 2 N: the constant
// 0); lane t of k_multiply_robot adds w_I for I = t, t + 256, .. ascending to 0, the 256 sums meet in chunk_tree_sums' pairwise
// tree (map_blocks.h), and the entry is fma(Prr[q][2], b_r[2], fma(Prr[q][1], b_r[1], fma(Prr[q][0], b_r[0], that sum))).
// Nothing depends on v, on what the other columns hold or on how many chunks a call has: a vector's product is the same bits wherever
// it stands.  No atomics, no data-dependent order.  b = 0 gives 0 in every chain; b = e_j leaves one product p * 1 in every chain, so
// the result is column j of P entry for entry (the sign of a zero aside).
// ---------------------------------------------------------------------------------------------------

constexpr int kMultiplyBlock = 256;        // four wavefronts; a wavefront owns the 16-row blocks wave, wave + 4, .. of a tile
constexpr int kMultiplyWaveBlocks = 4;     // at most: T <= 256

// Pmm(r, c) as the product takes it: the constant 0 at or beyond 2 N (n2), else what ekf_get_P reports
template <typename TS>
__device__ __forceinline__ double multiply_entry(const DevState &st, int64_t n2, int64_t r, int64_t c) {
    if (r >= n2 || c >= n2) return 0.0;
    return factor_source<TS>(st, r, c);
}

// TMAX: the largest tile edge this instance stages (its LDS); T itself is the handle's.
template <typename TS, int TMAX>
__global__ __launch_bounds__(kMultiplyBlock) void k_multiply_tiles(DevState st, MultiplyMapArgs a) {
    static_assert(kFactorChunk == 16 && TMAX % 16 == 0 && TMAX <= 16 * 4 * kMultiplyWaveBlocks, "one block of vectors, whole 16 x 16 blocks, four wavefronts");
    // a row of kPitch = TMAX + 2 doubles keeps every pair 16-byte aligned and spreads a quarter-wavefront's 16-byte reads over the banks
    constexpr int kPitch = TMAX + 2;
    __shared__ double BI[kFactorChunk][kPitch];
    __shared__ double BJ[kFactorChunk][kPitch];
    const int T = st.tm.T, S = a.S, nb = T >> 4, kPairs = T >> 3;
    const int64_t n2 = 2 * a.N;
    int I, seg, J0, J1;
    segment_of(blockIdx.x, S, I, seg, J0, J1);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane >> 4, lc = lane & 15;
    const TS *__restrict__ tiles = (const TS *)st.tiles;
    const int64_t rowI = (int64_t)I * T;
    const int64_t blk = (int64_t)T * kFactorChunk;                  // doubles of a partial block
    const bool partial = rowI + T > n2;                             // the last tile row, where rows at or beyond 2 N are selected away
    for (int e = tid; e < kFactorChunk * T; e += kMultiplyBlock) BI[e / T][e % T] = a.b[(int64_t)(e / T) * a.ld + rowI + e % T];
    d4_t dacc[kMultiplyWaveBlocks];
#pragma unroll
    for (int b = 0; b < kMultiplyWaveBlocks; ++b) dacc[b] = d4_t{0.0, 0.0, 0.0, 0.0};
    for (int J = J0; J < J1; ++J) {
        const int64_t colJ = (int64_t)J * T;
        __syncthreads();                                            // the tile before is done with BJ
        for (int e = tid; e < kFactorChunk * T; e += kMultiplyBlock) BJ[e / T][e % T] = a.b[(int64_t)(e / T) * a.ld + colJ + e % T];
        __syncthreads();
        const TS *__restrict__ tp = tiles + st.tm.tile_offset(I, J);
        const bool slow = partial || J == I;                        // entry by entry through multiply_entry (workgroup-uniform)
        // the direct part: block rb of T_IJ B_J
#pragma unroll
        for (int b = 0; b < kMultiplyWaveBlocks; ++b) {
            const int rb = wave + 4 * b;
            if (rb >= nb) continue;
            d4_t acc = dacc[b];
#if defined(EKF_FACTOR_FMA_TWIN)
            for (int r = 0; r < 4; ++r)
                for (int s = 0; s < 2 * kPairs; ++s)
                    for (int t = 0; t < 4; ++t) {
                        const int row = 16 * rb + lr + 4 * r, k = chunk_k(s, t);
                        const double p = slow ? multiply_entry<TS>(st, n2, rowI + row, colJ + k) : (double)tp[row * T + k];
                        acc[r] = fma(p, BJ[lc][k], acc[r]);
                    }
#else
            const int row = 16 * rb + lc;
#pragma unroll 4
            for (int p = 0; p < kPairs; ++p) {
                const int k = 8 * p + 2 * lr;
                double a0, a1;
                if (slow) { a0 = multiply_entry<TS>(st, n2, rowI + row, colJ + k); a1 = multiply_entry<TS>(st, n2, rowI + row, colJ + k + 1); }
                else { a0 = (double)tp[row * T + k]; a1 = (double)tp[row * T + k + 1]; }
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, BJ[lc][k], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, BJ[lc][k + 1], acc, 0, 0, 0);
            }
#endif
            dacc[b] = acc;
        }
        if (J == I) continue;
        // the transposed part: block cb of T_IJ' B_I, a partial block of tile row J of its own
        double *__restrict__ tout = a.tpart + st.tm.slot(I, J) * blk;
#pragma unroll
        for (int b = 0; b < kMultiplyWaveBlocks; ++b) {
            const int cb = wave + 4 * b;
            if (cb >= nb) continue;
            d4_t acc = {0.0, 0.0, 0.0, 0.0};
#if defined(EKF_FACTOR_FMA_TWIN)
            for (int r = 0; r < 4; ++r)
                for (int s = 0; s < 2 * kPairs; ++s)
                    for (int t = 0; t < 4; ++t) {
                        const int col = 16 * cb + lr + 4 * r, k = chunk_k(s, t);
                        const double p = slow ? multiply_entry<TS>(st, n2, rowI + k, colJ + col) : (double)tp[k * T + col];
                        acc[r] = fma(p, BI[lc][k], acc[r]);
                    }
#else
            const int col = 16 * cb + lc;
#pragma unroll 4
            for (int p = 0; p < kPairs; ++p) {
                const int k = 8 * p + 2 * lr;
                double a0, a1;
                if (slow) { a0 = multiply_entry<TS>(st, n2, rowI + k, colJ + col); a1 = multiply_entry<TS>(st, n2, rowI + k + 1, colJ + col); }
                else { a0 = (double)tp[k * T + col]; a1 = (double)tp[(k + 1) * T + col]; }
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, BI[lc][k], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, BI[lc][k + 1], acc, 0, 0, 0);
            }
#endif
#pragma unroll
            for (int r = 0; r < 4; ++r) tout[(16 * cb + lr + 4 * r) * kFactorChunk + lc] = acc[r];
        }
    }
    double *__restrict__ dout = a.dpart + (factor_segment_base(I, S) + seg) * blk;
#pragma unroll
    for (int b = 0; b < kMultiplyWaveBlocks; ++b) {
        const int rb = wave + 4 * b;
        if (rb >= nb) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) dout[(16 * rb + lr + 4 * r) * kFactorChunk + lc] = dacc[b][r];
    }
    // the first segment of a tile row also takes the row's part of strip B_m: lane (q, c) chains its T rows in ascending order
    if (seg != 0 || tid >= 3 * kFactorChunk) return;
    const int q = tid / kFactorChunk, c = tid % kFactorChunk;
    const double *__restrict__ sq = st.strip[a.cur] + (int64_t)q * st.ldm + rowI;
    double wsum = 0.0;
    for (int r = 0; r < T; ++r) wsum = fma(rowI + r < n2 ? sq[r] : 0.0, BI[c][r], wsum);
    a.wpart[(int64_t)I * (3 * kFactorChunk) + tid] = wsum;
}

// Grid nT * per, per = T * 16 / 256 workgroups a tile row (one at edge 16): a lane owns ONE entry e = (row e / 16, vector e % 16) of
// tile row R (the partial blocks' own order: a wavefront's reads are contiguous) and walks its chain of partial blocks alone, eight loads
// in flight; rows at and beyond 2 N are not written.  No LDS and a handful of registers: the robot rows are k_multiply_robot's.
__global__ __launch_bounds__(kFactorBlock) void k_multiply_sum(DevState st, MultiplyMapArgs a) {
    const int tid = threadIdx.x;
    const int T = st.tm.T, S = a.S;
    const int64_t n2 = 2 * a.N, nT = st.tm.tiles_for(n2);
    const int64_t blk = (int64_t)T * kFactorChunk;
    const int64_t per = (blk + kFactorBlock - 1) / kFactorBlock;
    const int64_t R = blockIdx.x / per;
    const int e = (int)(blockIdx.x % per) * kFactorBlock + tid;
    const int64_t r = R * T + e / kFactorChunk;
    if (R >= nT || e >= (int)blk || r >= n2) return;
    const int nseg = (int)(R / S) + 1;
    const double *__restrict__ dp = a.dpart + factor_segment_base(R, S) * blk + e;
    const double *__restrict__ tp = a.tpart + e;
    const double *__restrict__ s0 = st.strip[a.cur], *__restrict__ s1 = s0 + st.ldm, *__restrict__ s2 = s1 + st.ldm;
    double acc = dp[0];
    for (int s = 1; s < nseg; ++s) acc = acc + dp[(int64_t)s * blk];
#pragma unroll 8
    for (int64_t I = R + 1; I < nT; ++I) acc = acc + tp[st.tm.slot(I, R) * blk];
    const double *__restrict__ br = a.b + (int64_t)(e % kFactorChunk) * a.ld + a.rows;
    a.y[(int64_t)(e % kFactorChunk) * a.ld + r] = fma(s2[r], br[2], fma(s1[r], br[1], fma(s0[r], br[0], acc)));
}

// ONE workgroup, as k_factor_finish: the robot rows of the chunk, from the nT parts of strip B_m that k_multiply_tiles left and Prr.
__global__ __launch_bounds__(kFactorBlock) void k_multiply_robot(DevState st, MultiplyMapArgs a) {
    __shared__ double red[kFactorChunk][kFactorBlock];
    __shared__ double sums[3 * kFactorChunk];
    const int tid = threadIdx.x;
    const int64_t nT = st.tm.tiles_for(2 * a.N);
    double acc[3 * kFactorChunk];
#pragma unroll
    for (int s = 0; s < 3 * kFactorChunk; ++s) acc[s] = 0.0;
    for (int64_t I = tid; I < nT; I += kFactorBlock) {
#pragma unroll
        for (int s = 0; s < 3 * kFactorChunk; ++s) acc[s] = acc[s] + a.wpart[I * (3 * kFactorChunk) + s];
    }
    chunk_tree_sums(acc, red, sums);
    if (tid >= kFactorChunk) return;
    const double *__restrict__ prr = st.prr[a.cur];
    const double *__restrict__ br = a.b + (int64_t)tid * a.ld + a.rows;
    double *__restrict__ y = a.y + (int64_t)tid * a.ld + a.rows;
#pragma unroll
    for (int q = 0; q < 3; ++q) y[q] = fma(prr[3 * q + 2], br[2], fma(prr[3 * q + 1], br[1], fma(prr[3 * q], br[0], sums[q * kFactorChunk + tid])));
}
