// Fragment of kernels.hip (included there, inside its anonymous namespace, after map_blocks.h, whose tile_mac, segment_of and
// chunk_tree_sums it uses): the draws x + C xi behind the factorisation of P (ekf_sample_map) -- k_factor_apply, k_factor_sample.
#pragma once
#include "map_blocks.h"         // (kernels.hip has it in front already; a host build that names this fragment alone gets it here)

// ---------------------------------------------------------------------------------------------------
// THE DRAWS (ekf_sample_map).  After a factorisation that succeeded the factor store holds L (diagonal tiles lower-triangular with zeros
// above, rows at and beyond 2 N an identity tail), columns 0..2 of the right-hand sides W = L^-1 Pmr, and res[3..5] with lr_off[0..2] the
// tail L_r: the whole factor in elimination order is C = [L 0; W' L_r], and a sample of draw xi = (xi_m, xi_r) is
//     x_m + L xi_m,     x_r + W' xi_m + L_r xi_r.
// kFactorChunk draws at a time, one a COLUMN of the chunk (FactorSampleArgs), two launches:
//     k_factor_apply   one workgroup per SEGMENT of S tiles of a tile row: its TF x 16 block of L Xi over its tiles in ascending tile
//                      column, on v_mfma_f64_16x16x4_f64, every tile read from HBM once per chunk -- the hot path; one partial block out
//                      (and, from the first segment of each tile row, that row's 3 x 16 part of W' Xi)
//     k_factor_sample  workgroup I < rows / TF: tile row I's partial blocks summed in ascending segment order, x_m added, written;
//                      the last workgroup: the parts of W' Xi summed by chunk_tree_sums' fixed tree, the 3 x 3 tail, the robot
//                      rows written
// ARITHMETIC OF ONE ENTRY (row i of tile row I, draw c): per segment p = 0 starts a chain fma(L[i][k], xi_c[k], p) over the segment's
// tiles J ascending and inside a tile over k in chunk_k's order (tile_mac, map_blocks.h: the matrix instruction and its plain-FMA twin);
// the entry is x[3 + 64 I + i] + (((p_0 + p_1) + p_2) + ..), or x's entry itself where that sum is zero (sample_add).  Robot row q: per tile row I a chain w_I = fma(W[r][q], xi_c[r], .) over its
// TF rows ascending (a lane of the row's first segment in k_factor_apply; kept behind the partial blocks); lane t of the last workgroup
// of k_factor_sample adds w_I for I = t, t + 256, .. ascending to 0, the 256 sums meet in chunk_tree_sums' pairwise tree (map_blocks.h), then t_q =
// that sum with fma(L_r[q][j], xi_r[j], .) for j = 0 .. q in turn, and the entry is x[q] + t_q (sample_add).  Nothing depends on c, on what the other columns hold or
// on how many chunks a call has: a draw's sample is the same bits wherever it stands.  No atomics.  xi = 0 gives +0 in every chain: x, signed zeros included.  xi = e_j leaves one term in every chain, so the sample is fl(x + C[:, j]).
// In k_factor_apply a lane's A operands come straight from one tile row; the B operands, the same for all four wavefronts, are staged
// through LDS once per tile (which is why a draw is a column: its TF entries are contiguous).
// ---------------------------------------------------------------------------------------------------

// x + d, and x itself where the deviation is zero: x + (+0) would turn an entry -0.0 of x into +0.0, and xi = 0 is to return x bit for bit
__device__ __forceinline__ double sample_add(double x, double d) { return d == 0.0 ? x : x + d; }

template <int TF, int S>
__global__ __launch_bounds__(4 * TF) void k_factor_apply(FactorMapArgs a, FactorSampleArgs sa) {
    static_assert(TF % 16 == 0 && TF <= 64 && kFactorChunk == 16 && S >= 1, "whole 16 x 16 blocks (an even number of steps), at most four wavefronts, one block of draws");
    if (a.res[0] != 0.0) return;
    int I, seg, J0, J1;
    segment_of(blockIdx.x, S, I, seg, J0, J1);
    const int tid = threadIdx.x, lane = tid & 63, lr = lane >> 4, lc = lane & 15;
    const int row0 = 16 * (tid >> 6);
    // Xi_J, TF entries of each of the 16 draws, goes through LDS once per tile for all four wavefronts (read straight from the L2 it was
    // as many bytes again as the tile itself).  Lane t stages four contiguous doubles; two buffers, one barrier a tile.  A row of kPitch
    // = TF + 2 doubles keeps every pair 16-byte aligned and puts the 16 draws of a quarter-wavefront's 16-byte reads on 64 different banks.
    constexpr int kPitch = TF + 2, kPer = TF / 4;
    __shared__ double Xs[2][kFactorChunk][kPitch];
    const double *__restrict__ Xg = sa.xi + (int64_t)(tid / kPer) * sa.ld + 4 * (tid % kPer);
    double *const xs0 = &Xs[0][tid / kPer][4 * (tid % kPer)], *const xs1 = &Xs[1][tid / kPer][4 * (tid % kPer)];
    {
        const double *__restrict__ g4 = Xg + (int64_t)J0 * TF;
        xs0[0] = g4[0]; xs0[1] = g4[1]; xs0[2] = g4[2]; xs0[3] = g4[3];
    }
    __syncthreads();
    d4_t acc = {0.0, 0.0, 0.0, 0.0};
    for (int J = J0; J < J1; ++J) {
        const int buf = (J - J0) & 1;
        const double *__restrict__ L = a.tiles + a.tm.tile_offset(I, J);
        const double *__restrict__ XJ = &Xs[buf][lc][0];
        if (J + 1 < J1) {
            const double *__restrict__ g4 = Xg + (int64_t)(J + 1) * TF;
            double *const xn = buf ? xs0 : xs1;
            xn[0] = g4[0]; xn[1] = g4[1]; xn[2] = g4[2]; xn[3] = g4[3];
        }
        tile_mac<TF, false, false>(acc, L, XJ, row0, lr, lc);
        __syncthreads();
    }
    double *__restrict__ out = sa.part + (factor_segment_base(I, S) + seg) * (int64_t)(TF * kFactorChunk);
#pragma unroll
    for (int r = 0; r < 4; ++r) out[(row0 + lr + 4 * r) * kFactorChunk + lc] = acc[r];
    // the first segment of a tile row also takes the row's part of W' Xi: lane (q, c) chains its TF rows in ascending order
    if (seg != 0 || tid >= 3 * kFactorChunk) return;
    const int q = tid / kFactorChunk, c = tid % kFactorChunk;
    const double *__restrict__ wq = a.rhs + (int64_t)I * TF * kFactorRhs + q;
    const double *__restrict__ xc = sa.xi + (int64_t)c * sa.ld + (int64_t)I * TF;
    double wsum = 0.0;
#pragma unroll 8
    for (int r = 0; r < TF; ++r) wsum = fma(wq[r * kFactorRhs], xc[r], wsum);
    sa.part[factor_segment_base(a.rows / TF, S) * (int64_t)(TF * kFactorChunk) + (int64_t)I * (3 * kFactorChunk) + tid] = wsum;
}

// Grid rows / TF + 1.  Workgroup I < rows / TF: entry e = (row e / 16, draw e % 16) of tile row I (the partial blocks' own order: the
// reads are contiguous); rows at and beyond 2 N, the identity tail, are not written.  The last workgroup: the robot rows, from the
// rows / TF parts of W' Xi that k_factor_apply left behind the partial blocks.
template <int TF, int S>
__global__ __launch_bounds__(kFactorBlock) void k_factor_sample(DevState st, FactorMapArgs a, FactorSampleArgs sa) {
    __shared__ double red[kFactorChunk][kFactorBlock];
    __shared__ double sums[3 * kFactorChunk];
    if (a.res[0] != 0.0) return;
    const int tid = threadIdx.x;
    const int64_t nF = a.rows / TF;
    const double *__restrict__ x = st.x[a.cur];
    if ((int64_t)blockIdx.x < nF) {
        const int64_t I = blockIdx.x;
        const int nseg = (int)(I / S) + 1;
        const double *__restrict__ p = sa.part + factor_segment_base(I, S) * (int64_t)(TF * kFactorChunk);
        for (int e = tid; e < TF * kFactorChunk; e += kFactorBlock) {
            const int64_t r = I * TF + e / kFactorChunk;
            double acc = p[e];
            for (int s = 1; s < nseg; ++s) acc = acc + p[(int64_t)s * (TF * kFactorChunk) + e];
            if (r < 2 * a.N) sa.y[(int64_t)(e % kFactorChunk) * sa.ld + r] = sample_add(x[3 + r], acc);
        }
        return;
    }
    double acc[3 * kFactorChunk];
#pragma unroll
    for (int s = 0; s < 3 * kFactorChunk; ++s) acc[s] = 0.0;
    const double *__restrict__ wp = sa.part + factor_segment_base(nF, S) * (int64_t)(TF * kFactorChunk);
    for (int64_t I = tid; I < nF; I += kFactorBlock) {
#pragma unroll
        for (int s = 0; s < 3 * kFactorChunk; ++s) acc[s] = acc[s] + wp[I * (3 * kFactorChunk) + s];
    }
    chunk_tree_sums(acc, red, sums);
    if (tid >= kFactorChunk) return;
    const double *__restrict__ e = sa.xi + (int64_t)tid * sa.ld + a.rows;
    double *__restrict__ y = sa.y + (int64_t)tid * sa.ld + a.rows;
    const double l00 = a.res[3], l11 = a.res[4], l22 = a.res[5], l10 = a.lr_off[0], l20 = a.lr_off[1], l21 = a.lr_off[2];
    const double t0 = fma(l00, e[0], sums[tid]);
    const double t1 = fma(l11, e[1], fma(l10, e[0], sums[kFactorChunk + tid]));
    const double t2 = fma(l22, e[2], fma(l21, e[1], fma(l20, e[0], sums[2 * kFactorChunk + tid])));
    y[0] = sample_add(x[0], t0); y[1] = sample_add(x[1], t1); y[2] = sample_add(x[2], t2);
}
