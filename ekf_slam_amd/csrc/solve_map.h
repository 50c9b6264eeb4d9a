// Fragment of kernels.hip (included there, inside its anonymous namespace, after sample_map.h, whose chunk layout it shares, and
// map_blocks.h, whose tile_mac and chunk_tree_sums it uses): the solves C^-1 B and P^-1 B behind the factorisation of P (ekf_solve_map) -- k_solve_invert, k_solve_forward, k_solve_tail,
// k_solve_backward.
#pragma once
#include "map_blocks.h"         // (kernels.hip has it in front already; a host build that names this fragment alone gets it here)

// ---------------------------------------------------------------------------------------------------
// THE SOLVES (ekf_solve_map).  The factor in elimination order is C = [L 0; W' L_r] (sample_map.h), and for b = (b_m, b_r)
//     u_m = L^-1 b_m,   u_r = L_r^-1 (b_r - W' u_m)            u = C^-1 b          (form 1, EKF_SOLVE_HALF)
//     z_r = L_r^-T u_r, z_m = L^-T (u_m - W z_r)               z = P^-1 b          (form 0, EKF_SOLVE_FULL)
// kFactorChunk right-hand sides at a time, one a COLUMN of the chunk (FactorSolveArgs), in stream order and nothing else:
//     k_solve_invert    once a call, one wavefront per diagonal tile: X_cc = L_cc^-1 into sv.inv, a lane per column
//     k_solve_forward   one launch per tile column c ascending, one workgroup per tile row I >= c: every workgroup forms u_c = X_cc b_c
//                       for itself (a TF x TF x 16 product); workgroup 0 writes it to y, workgroup I - c > 0 goes on to
//                       b_I -= L_Ic u_c.  b_c is only read in launch c, b_I only by its own workgroup: no workgroup reads what another writes.
//     k_solve_tail      one workgroup: W' u by chunk_tree_sums' fixed tree, then the 3 x 3 solves, a lane per column: u_r into y
//                       (form 1) or z_r into b (form 0)
//     k_solve_backward  form 0 only, one launch per tile row c DESCENDING, one workgroup per tile column J <= c: every workgroup forms
//                       z_c = X_cc' (v_c - W_c z_r) for itself, v the contents of y; workgroup 0 writes it to b, workgroup c - J > 0
//                       goes on to v_J -= L_cJ' z_c in y.
// Both sweeps run on v_mfma_f64_16x16x4_f64; the right-hand sides go through LDS once per product for all four wavefronts.  THE
// TRANSPOSED OPERANDS (X_cc', L_cJ') DO NOT GO THROUGH LDS: operand A of the instruction is (row lc, term lr) per lane, and with the tile
// read as A(i, k) = tile[k][i] the 16 lanes of a quarter-wavefront read 16 ADJACENT doubles of tile row k, a whole 128-byte line -- the
// transposed read is the better coalesced of the two, so there is nothing for a staging pass to gain.
// ARITHMETIC OF ONE ENTRY, right-hand side q (nothing depends on the other columns or on how many chunks a call has: a row of the result
// is the same bits wherever its right-hand side stands).  X_cc: column j by forward substitution, x_i = (delta_ij - sum_{p < i} L_ip x_p)
// / L_ii as a chain fma(-L_ip, x_p, .) over p ascending, exact zeros above the diagonal.  Every product is a chain fma(A_ik, x_k, acc)
// over k in chunk_k's order (tile_mac, map_blocks.h: the matrix instruction and its plain-FMA twin), started from 0 for u_c and z_c and
// from the entry itself for the updates, with A = -L (negation is exact).  So entry i of tile row I of u is the chain over X_II's row
// applied to b_I less the updates of tile columns 0 .. I - 1 in that order; the backward sweep mirrors it with tile rows nF - 1 .. c + 1
// descending and, LAST, the fold fma(-W_i2, z_r2, fma(-W_i1, z_r1, fma(-W_i0, z_r0, v_i))) on the way into LDS.  W' u: lane t chains
// fma(W[r][q], u[r], .) over its rows r = t, t + 256, .. ascending, the 256 sums meet in chunk_tree_sums' pairwise tree (map_blocks.h); then
// t_q = b_r[q] - that sum, u_r by forward and z_r by backward substitution on L_r (res[3..5], lr_off) with the products as FMAs.
// No atomics, no flags between workgroups, no data-dependent order.  b = 0 gives zeros throughout.  Every launch returns at once where
// a pivot failed (res[0] != 0).
// ---------------------------------------------------------------------------------------------------

// Grid rows / TF, one wavefront each.  Lane j < TF owns column j of X = L_cc^-1 in registers (every index static: the loops unroll, as
// in k_factor_panel); every lane reads the same entry of L_cc from LDS.  A lane's entries above its diagonal are chains of zeros.
template <int TF>
__global__ __launch_bounds__(64) void k_solve_invert(FactorMapArgs a, FactorSolveArgs sv) {
    static_assert(TF <= 64, "a lane per column of the tile");
    __shared__ double Ls[TF][TF + 1];
    if (a.res[0] != 0.0) return;
    const int tid = threadIdx.x, c = (int)blockIdx.x;
    const double *__restrict__ lp = a.tiles + a.tm.tile_offset(c, c);
    for (int e = tid; e < TF * TF; e += 64) Ls[e / TF][e % TF] = lp[e];
    __syncthreads();
    if (tid >= TF) return;
    double x[TF];
#pragma unroll
    for (int i = 0; i < TF; ++i) {
        double acc = i == tid ? 1.0 : 0.0;
#pragma unroll
        for (int p = 0; p < i; ++p) acc = fma(-Ls[i][p], x[p], acc);
        x[i] = acc / Ls[i][i];
    }
    double *__restrict__ xp = sv.inv + (int64_t)c * (TF * TF);
#pragma unroll
    for (int i = 0; i < TF; ++i) xp[i * TF + tid] = i < tid ? 0.0 : x[i];
}

// Grid rows / TF - c.  Lane t stages four contiguous doubles of one right-hand side (a row of kPitch = TF + 2 doubles: sample_map.h).
template <int TF>
__global__ __launch_bounds__(4 * TF) void k_solve_forward(FactorMapArgs a, FactorSolveArgs sv, int c) {
    static_assert(TF % 16 == 0 && TF <= 64 && kFactorChunk == 16, "whole 16 x 16 blocks (an even number of steps), at most four wavefronts, one block of right-hand sides");
    constexpr int kPitch = TF + 2, kPer = TF / 4;
    __shared__ double Bs[kFactorChunk][kPitch], Us[kFactorChunk][kPitch];
    if (a.res[0] != 0.0) return;
    const int tid = threadIdx.x, lane = tid & 63, lr = lane >> 4, lc = lane & 15;
    const int row0 = 16 * (tid >> 6);
    {
        const double *__restrict__ g4 = sv.b + (int64_t)(tid / kPer) * sv.ld + (int64_t)c * TF + 4 * (tid % kPer);
        double *const bs = &Bs[tid / kPer][4 * (tid % kPer)];
        bs[0] = g4[0]; bs[1] = g4[1]; bs[2] = g4[2]; bs[3] = g4[3];
    }
    __syncthreads();
    d4_t acc = {0.0, 0.0, 0.0, 0.0};
    tile_mac<TF, false, false>(acc, sv.inv + (int64_t)c * (TF * TF), &Bs[lc][0], row0, lr, lc);
    if (blockIdx.x == 0) {
        double *__restrict__ yc = sv.y + (int64_t)lc * sv.ld + (int64_t)c * TF + row0 + lr;
#pragma unroll
        for (int r = 0; r < 4; ++r) yc[4 * r] = acc[r];
        return;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) Us[lc][row0 + lr + 4 * r] = acc[r];
    __syncthreads();
    const int I = c + (int)blockIdx.x;
    double *__restrict__ bI = sv.b + (int64_t)lc * sv.ld + (int64_t)I * TF + row0 + lr;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = bI[4 * r];
    tile_mac<TF, false, true>(acc, a.tiles + a.tm.tile_offset(I, c), &Us[lc][0], row0, lr, lc);
#pragma unroll
    for (int r = 0; r < 4; ++r) bI[4 * r] = acc[r];
}

// One workgroup.  u_m is what the forward sweep left in y; b_r is still in b (no launch of the sweep touches entries rows .. rows + 2).
__global__ __launch_bounds__(kFactorBlock) void k_solve_tail(FactorMapArgs a, FactorSolveArgs sv) {
    __shared__ double red[kFactorChunk][kFactorBlock];
    __shared__ double sums[3 * kFactorChunk];
    if (a.res[0] != 0.0) return;
    const int tid = threadIdx.x;
    double acc[3 * kFactorChunk];
#pragma unroll
    for (int s = 0; s < 3 * kFactorChunk; ++s) acc[s] = 0.0;
    for (int64_t r = tid; r < a.rows; r += kFactorBlock) {
        const double *__restrict__ w = a.rhs + r * kFactorRhs;
        const double w0 = w[0], w1 = w[1], w2 = w[2];
#pragma unroll
        for (int c = 0; c < kFactorChunk; ++c) {
            const double u = sv.y[(int64_t)c * sv.ld + r];
            acc[c] = fma(w0, u, acc[c]);
            acc[kFactorChunk + c] = fma(w1, u, acc[kFactorChunk + c]);
            acc[2 * kFactorChunk + c] = fma(w2, u, acc[2 * kFactorChunk + c]);
        }
    }
    chunk_tree_sums(acc, red, sums);
    if (tid >= kFactorChunk) return;
    double *__restrict__ br = sv.b + (int64_t)tid * sv.ld + a.rows;
    const double l00 = a.res[3], l11 = a.res[4], l22 = a.res[5], l10 = a.lr_off[0], l20 = a.lr_off[1], l21 = a.lr_off[2];
    const double t0 = br[0] - sums[tid], t1 = br[1] - sums[kFactorChunk + tid], t2 = br[2] - sums[2 * kFactorChunk + tid];
    const double u0 = t0 / l00, u1 = fma(-l10, u0, t1) / l11, u2 = fma(-l21, u1, fma(-l20, u0, t2)) / l22;
    if (sv.form != 0) {
        double *__restrict__ yr = sv.y + (int64_t)tid * sv.ld + a.rows;
        yr[0] = u0; yr[1] = u1; yr[2] = u2;
        return;
    }
    const double z2 = u2 / l22, z1 = fma(-l21, z2, u1) / l11, z0 = fma(-l10, z1, fma(-l20, z2, u0)) / l00;
    br[0] = z0; br[1] = z1; br[2] = z2;
}

// Grid c + 1.  z_r is what k_solve_tail left in b's robot entries.
template <int TF>
__global__ __launch_bounds__(4 * TF) void k_solve_backward(FactorMapArgs a, FactorSolveArgs sv, int c) {
    static_assert(TF % 16 == 0 && TF <= 64 && kFactorChunk == 16, "whole 16 x 16 blocks (an even number of steps), at most four wavefronts, one block of right-hand sides");
    constexpr int kPitch = TF + 2, kPer = TF / 4;
    __shared__ double Vs[kFactorChunk][kPitch], Zs[kFactorChunk][kPitch];
    if (a.res[0] != 0.0) return;
    const int tid = threadIdx.x, lane = tid & 63, lr = lane >> 4, lc = lane & 15;
    const int row0 = 16 * (tid >> 6);
    {
        const int q = tid / kPer, r4 = 4 * (tid % kPer);
        const double *__restrict__ g4 = sv.y + (int64_t)q * sv.ld + (int64_t)c * TF + r4;
        const double *__restrict__ zr = sv.b + (int64_t)q * sv.ld + a.rows;
        const double *__restrict__ w = a.rhs + ((int64_t)c * TF + r4) * kFactorRhs;
        const double z0 = zr[0], z1 = zr[1], z2 = zr[2];
#pragma unroll
        for (int i = 0; i < 4; ++i) Vs[q][r4 + i] = fma(-w[i * kFactorRhs + 2], z2, fma(-w[i * kFactorRhs + 1], z1, fma(-w[i * kFactorRhs], z0, g4[i])));
    }
    __syncthreads();
    d4_t acc = {0.0, 0.0, 0.0, 0.0};
    tile_mac<TF, true, false>(acc, sv.inv + (int64_t)c * (TF * TF), &Vs[lc][0], row0, lr, lc);
    if (blockIdx.x == 0) {
        double *__restrict__ zc = sv.b + (int64_t)lc * sv.ld + (int64_t)c * TF + row0 + lr;
#pragma unroll
        for (int r = 0; r < 4; ++r) zc[4 * r] = acc[r];
        return;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) Zs[lc][row0 + lr + 4 * r] = acc[r];
    __syncthreads();
    const int J = c - (int)blockIdx.x;
    double *__restrict__ vJ = sv.y + (int64_t)lc * sv.ld + (int64_t)J * TF + row0 + lr;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = vJ[4 * r];
    tile_mac<TF, true, true>(acc, a.tiles + a.tm.tile_offset(c, J), &Zs[lc][0], row0, lr, lc);
#pragma unroll
    for (int r = 0; r < 4; ++r) vJ[4 * r] = acc[r];
}
