// Fragment of kernels.hip (included there, inside its anonymous namespace, after nearest.h): the Cholesky factorisation of P on the device
// (ekf_factor_map) -- k_factor_load, k_factor_rhs, k_factor_diag, k_factor_panel, k_factor_trail, k_factor_finish.
#pragma once

// ---------------------------------------------------------------------------------------------------
// P = [Prr Prm; Pmr Pmm] of a flushed handle, n = 3 + 2 N.  ELIMINATION ORDER: the landmark block first -- tile rows ascending, then the
// rows inside each tile -- and the robot last, so Pmm = L L' is a factorisation of the tile store alone and the robot is a 3 x 3 tail:
//     W = L^-1 Pmr (the strip as three right-hand sides),  S_r = Prr - W' W,  S_r = L_r L_r' on one lane.
// With nu = x - ref_q (its heading entry wrapped into (-180, 180]), w_q = L^-1 nu_m rides the same forward substitution as W, and
//     d2_q = |w_q|^2 + |L_r^-1 (nu_r - W' w_q)|^2.
// The FACTOR STORE (FactorMapArgs: tiles) is F64 lower-triangle tiles of edge TF under a TileMap of its own (world = 1), `rows` = 2 N
// rounded up to whole tile rows; its edge is independent of the handle's T.  k_factor_load fills it with exactly what ekf_get_P reports:
// float tiles widened, every landmark's own 2 x 2 block from the live F64 copies diag[dcur], rows at and beyond 2 N an IDENTITY tail (pivot
// 1, log 0: no kernel below has a partial-tile case).  The right-hand sides are a rows x kFactorRhs block, row-major: columns 0..2 the
// strip, column 3 + q the landmark part of x - ref_q.
// A right-looking blocked Cholesky, stream-ordered, per tile column k:
//     k_factor_diag   ONE workgroup: tile (k, k) factored in LDS, its pivots written, block k of the right-hand sides forward-solved in
//                     the same sweep (they are extra columns of the elimination)
//     k_factor_panel  one wavefront per tile I > k: L_Ik = A_Ik L_kk^-T with L_kk in LDS, a lane per row; then b_I -= L_Ik w_k
//     k_factor_trail  one workgroup per tile (I, J), k < J <= I: A_IJ -= L_Ik L_Jk' on v_mfma_f64_16x16x4_f64 -- the hot path
// then k_factor_finish: W' W, W' w_q and |w_q|^2 by a fixed reduction tree, the 3 x 3 tail and d2 on one lane.
// STATUS: res[0] is 0 until a pivot fails (<= 0 or not finite): then the ONE workgroup that met it (k_factor_diag's, or k_factor_finish's
// lane 0) stores 1 (a landmark row) or 2 (the robot tail), the index into x and the pivot's value with plain vector stores; every later
// launch reads res[0] first and returns at once.  No atomics, no data-dependent order.
// ---------------------------------------------------------------------------------------------------

constexpr int kFactorBlock = 256;          // k_factor_load, k_factor_rhs, k_factor_diag, k_factor_finish
constexpr int kFactorSums = 6 + 4 * kFactorRefMax;

// the tile (i, j), j <= i, of position w in a row-major lower triangle
__device__ __forceinline__ void factor_tile_of(int64_t w, int &i, int &j) {
    int64_t r = (int64_t)((sqrt(8.0 * (double)w + 1.0) - 1.0) * 0.5);
    while (r * (r + 1) / 2 > w) --r;
    while ((r + 1) * (r + 2) / 2 <= w) ++r;
    i = (int)r;
    j = (int)(w - r * (r + 1) / 2);
}

// P(3 + r, 3 + c) of the landmark block as ekf_get_P reports it, r and c below 2 N: the own block from the live F64 copy, everything else
// from the lower triangle of the handle's tile store (an unsharded tile map: every tile is held here)
template <typename TS>
__device__ __forceinline__ double factor_source(const DevState &st, int64_t r, int64_t c) {
    if ((r >> 1) == (c >> 1)) return st.diag[st.dcur][3 * (r >> 1) + (r & 1) + (c & 1)];
    if (c > r) { const int64_t t = r; r = c; c = t; }
    const TileMap &tm = st.tm;
    return (double)((const TS *)st.tiles)[tm.tile_offset(r >> tm.shift, c >> tm.shift) + ((r & (tm.T - 1)) << tm.shift) + (c & (tm.T - 1))];
}

// One workgroup per tile of the factor store (grid = row_base(rows / TF)); diagonal tiles are written whole.
template <typename TS, int TF>
__global__ __launch_bounds__(kFactorBlock) void k_factor_load(DevState st, FactorMapArgs a) {
    int I, J;
    factor_tile_of(blockIdx.x, I, J);
    double *__restrict__ tp = a.tiles + a.tm.tile_offset(I, J);
    const int64_t n2 = 2 * a.N;
    for (int e = threadIdx.x; e < TF * TF; e += kFactorBlock) {
        const int64_t r = (int64_t)I * TF + e / TF, c = (int64_t)J * TF + e % TF;
        tp[e] = r < n2 && c < n2 ? factor_source<TS>(st, r, c) : (r == c ? 1.0 : 0.0);
    }
}

// One lane per row of the right-hand sides (grid = rows / kFactorBlock rounded up): the strip's three rows and x_m - ref_m, zero from
// row 2 N on and in the columns no reference uses.
__global__ __launch_bounds__(kFactorBlock) void k_factor_rhs(DevState st, FactorMapArgs a) {
    const int64_t r = (int64_t)blockIdx.x * kFactorBlock + threadIdx.x;
    if (r >= a.rows) return;
    double *__restrict__ b = a.rhs + r * kFactorRhs;
    const bool live = r < 2 * a.N;
    for (int q = 0; q < 3; ++q) b[q] = live ? st.strip[a.cur][q * st.ldm + r] : 0.0;
    for (int q = 0; q < kFactorRhs - 3; ++q) b[3 + q] = live && q < a.nref ? st.x[a.cur][3 + r] - a.ref[q * a.ref_stride + 3 + r] : 0.0;
}

// a pivot that ends the factorisation: zero, negative, NaN or infinite
__device__ __forceinline__ bool factor_pivot_bad(double d) { return !(d > 0.0 && d <= 1.7976931348623157e308); }

// Tile (k, k) in LDS, unblocked and right-looking: per column j every lane reads the pivot (a uniform decision, no flag), the lanes of
// column j scale it into `col` while lanes TF .. TF + 3 + nref scale row j of the right-hand sides into `wc`, and after one barrier every
// lane applies col col' to the rows below and col wc' to the right-hand sides below.  Two barriers a column.
template <int TF>
__global__ __launch_bounds__(kFactorBlock) void k_factor_diag(FactorMapArgs a, int k) {
    static_assert(TF + kFactorRhs <= kFactorBlock, "the lanes of a column and of a right-hand-side row are distinct");
    __shared__ double As[TF][TF + 1];
    __shared__ double bs[TF][kFactorRhs];
    __shared__ double col[TF], pv[TF], wc[kFactorRhs];
    if (a.res[0] != 0.0) return;
    const int tid = threadIdx.x;
    const int nr = 3 + a.nref;
    double *__restrict__ tp = a.tiles + a.tm.tile_offset(k, k);
    double *__restrict__ bp = a.rhs + (int64_t)k * TF * kFactorRhs;
    for (int e = tid; e < TF * TF; e += kFactorBlock) As[e / TF][e % TF] = tp[e];
    for (int e = tid; e < TF * kFactorRhs; e += kFactorBlock) bs[e / kFactorRhs][e % kFactorRhs] = bp[e];
    __syncthreads();
    int bad = -1;
    double bad_pivot = 0.0;
    for (int j = 0; j < TF; ++j) {
        const double d = As[j][j];
        if (factor_pivot_bad(d)) { bad = j; bad_pivot = d; break; }        // (every lane reads the same value)
        const double l = sqrt(d);
        if (tid == j) { col[j] = l; pv[j] = l; }
        else if (tid > j && tid < TF) { const double v = As[tid][j] / l; col[tid] = v; As[tid][j] = v; }
        else if (tid >= TF && tid < TF + nr) { const double v = bs[j][tid - TF] / l; wc[tid - TF] = v; bs[j][tid - TF] = v; }
        __syncthreads();
        for (int e = (j + 1) * TF + tid; e < TF * TF; e += kFactorBlock) {
            const int i = e / TF, c = e % TF;
            if (c > j && c <= i) As[i][c] = fma(-col[i], col[c], As[i][c]);
        }
        for (int e = (j + 1) * kFactorRhs + tid; e < TF * kFactorRhs; e += kFactorBlock) {
            const int i = e / kFactorRhs, q = e % kFactorRhs;
            if (q < nr) bs[i][q] = fma(-col[i], wc[q], bs[i][q]);
        }
        __syncthreads();
    }
    double *__restrict__ piv = a.res + kFactorRes + (int64_t)k * TF;
    if (tid < (bad < 0 ? TF : bad)) piv[tid] = pv[tid];
    if (bad >= 0) {
        if (tid == 0) { a.res[1] = (double)(3 + (int64_t)k * TF + bad); a.res[2] = bad_pivot; a.res[0] = 1.0; }
        return;
    }
    for (int e = tid; e < TF * TF; e += kFactorBlock) {
        const int i = e / TF, c = e % TF;
        tp[e] = c < i ? As[i][c] : (c == i ? pv[i] : 0.0);
    }
    for (int e = tid; e < TF * kFactorRhs; e += kFactorBlock) bp[e] = bs[e / kFactorRhs][e % kFactorRhs];
}

// One wavefront per tile I = k + 1 + blockIdx.x; lane i < TF owns row i of A_Ik in registers (every index static: the loops unroll) and
// solves x L_kk' = a_i, every lane reading the same entry of L_kk from LDS; then its row of the right-hand sides: b_i -= x w_k.
template <int TF>
__global__ __launch_bounds__(64) void k_factor_panel(FactorMapArgs a, int k) {
    static_assert(TF <= 64, "a lane per row of the tile");
    __shared__ double Ls[TF][TF + 1];
    __shared__ double ws[TF][kFactorRhs];
    if (a.res[0] != 0.0) return;
    const int tid = threadIdx.x;
    const int I = k + 1 + (int)blockIdx.x;
    const double *__restrict__ lp = a.tiles + a.tm.tile_offset(k, k);
    const double *__restrict__ wp = a.rhs + (int64_t)k * TF * kFactorRhs;
    for (int e = tid; e < TF * TF; e += 64) Ls[e / TF][e % TF] = lp[e];
    for (int e = tid; e < TF * kFactorRhs; e += 64) ws[e / kFactorRhs][e % kFactorRhs] = wp[e];
    __syncthreads();
    if (tid >= TF) return;
    double *__restrict__ rp = a.tiles + a.tm.tile_offset(I, k) + (int64_t)tid * TF;
    double x[TF];
#pragma unroll
    for (int c = 0; c < TF; ++c) x[c] = rp[c];
#pragma unroll
    for (int j = 0; j < TF; ++j) {
        double acc = x[j];
#pragma unroll
        for (int p = 0; p < j; ++p) acc = fma(-x[p], Ls[j][p], acc);
        x[j] = acc / Ls[j][j];
    }
#pragma unroll
    for (int c = 0; c < TF; ++c) rp[c] = x[c];
    double *__restrict__ bp = a.rhs + ((int64_t)I * TF + tid) * kFactorRhs;
    const int nr = 3 + a.nref;
    for (int q = 0; q < nr; ++q) {
        double acc = bp[q];
#pragma unroll
        for (int p = 0; p < TF; ++p) acc = fma(-x[p], ws[p][q], acc);
        bp[q] = acc;
    }
}

// The k index of the trailing update: step s of TF / 4, term t of the four one matrix instruction chains, in that order.  A lane's operands
// of all steps are then TF / 4 CONTIGUOUS doubles of one tile row, and no operand goes through LDS.
template <int TF> __device__ __forceinline__ constexpr int factor_k(int s, int t) { return (TF / 4) * t + s; }

// One workgroup per tile (I, J), k < J <= I, of the trailing matrix (grid = m (m + 1) / 2, m = rows / TF - 1 - k); a wavefront owns 16
// rows x TF columns = TF / 16 accumulator blocks.  v_mfma_f64_16x16x4_f64 is a k-ordered chain of correctly rounded FMAs
// (flush64_mfma.h), so with A = -L_Ik (negation is exact) every entry is fma(-L_I[i][k], L_J[j][k], .) over k in factor_k's order: the
// host twin below (EKF_FACTOR_FMA_TWIN, the builds of tests/support) is that chain, entry by entry.  Lane (lr, lc) = (lane / 16, lane % 16)
// supplies A(row lc, term lr) and B(term lr, column lc) and holds the entries (row lr + 4 r, column lc) of a block.
template <int TF>
__global__ __launch_bounds__(4 * TF) void k_factor_trail(FactorMapArgs a, int k) {
    static_assert(TF % 16 == 0 && TF <= 64, "whole 16 x 16 blocks, at most four wavefronts");
    constexpr int kBlocks = TF / 16, kSteps = TF / 4;
    if (a.res[0] != 0.0) return;
    int i, j;
    factor_tile_of(blockIdx.x, i, j);
    const int I = k + 1 + i, J = k + 1 + j;
    const double *__restrict__ LI = a.tiles + a.tm.tile_offset(I, k);
    const double *__restrict__ LJ = a.tiles + a.tm.tile_offset(J, k);
    double *__restrict__ C = a.tiles + a.tm.tile_offset(I, J);
    const int tid = threadIdx.x, lane = tid & 63, lr = lane >> 4, lc = lane & 15;
    const int row0 = 16 * (tid >> 6);
    d4_t acc[kBlocks];
#pragma unroll
    for (int b = 0; b < kBlocks; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[b][r] = C[(row0 + lr + 4 * r) * TF + 16 * b + lc];
#if defined(EKF_FACTOR_FMA_TWIN)
#pragma unroll
    for (int b = 0; b < kBlocks; ++b)
        for (int r = 0; r < 4; ++r)
            for (int s = 0; s < kSteps; ++s)
                for (int t = 0; t < 4; ++t)
                    acc[b][r] = fma(-LI[(row0 + lr + 4 * r) * TF + factor_k<TF>(s, t)], LJ[(16 * b + lc) * TF + factor_k<TF>(s, t)], acc[b][r]);
#else
    double av[kSteps];
#pragma unroll
    for (int s = 0; s < kSteps; ++s) av[s] = -LI[(row0 + lc) * TF + factor_k<TF>(s, lr)];
#pragma unroll
    for (int b = 0; b < kBlocks; ++b) {
        double bv[kSteps];
#pragma unroll
        for (int s = 0; s < kSteps; ++s) bv[s] = LJ[(16 * b + lc) * TF + factor_k<TF>(s, lr)];
#pragma unroll
        for (int s = 0; s < kSteps; ++s) acc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], bv[s], acc[b], 0, 0, 0);
    }
#endif
#pragma unroll
    for (int b = 0; b < kBlocks; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) C[(row0 + lr + 4 * r) * TF + 16 * b + lc] = acc[b][r];
}

// One workgroup.  Every lane sums its rows (tid, tid + 256, ..) in ascending order, the 256 partial sums of each quantity go through one
// pairwise tree in LDS: a fixed order for a given `rows`.  sums: W'W as (00, 10, 11, 20, 21, 22), then per reference (W'w)_0..2, |w|^2.
// Lane 0 then takes the 3 x 3 tail in the order robot 0, 1, 2 and writes the result block:
//   res[0] status, res[1] index into x and res[2] value of the pivot that failed, res[3..5] the tail's diagonal of L_r, res[6] how many
//   of them were taken, res[8 + q] d2 of reference q.  Where a.lr_off is given and the tail was taken whole, L_r's entries below the
//   diagonal go there, (1,0), (2,0), (2,1): the result block has no room for them, and nothing in it moves.
__global__ __launch_bounds__(kFactorBlock) void k_factor_finish(DevState st, FactorMapArgs a) {
    __shared__ double red[kFactorBlock];
    __shared__ double sums[kFactorSums];
    if (a.res[0] != 0.0) return;
    const int tid = threadIdx.x;
    double acc[kFactorSums];
#pragma unroll
    for (int s = 0; s < kFactorSums; ++s) acc[s] = 0.0;
    for (int64_t r = tid; r < a.rows; r += kFactorBlock) {
        const double *__restrict__ b = a.rhs + r * kFactorRhs;
        double v[kFactorRhs];
#pragma unroll
        for (int q = 0; q < kFactorRhs; ++q) v[q] = b[q];
        acc[0] = fma(v[0], v[0], acc[0]); acc[1] = fma(v[1], v[0], acc[1]); acc[2] = fma(v[1], v[1], acc[2]);
        acc[3] = fma(v[2], v[0], acc[3]); acc[4] = fma(v[2], v[1], acc[4]); acc[5] = fma(v[2], v[2], acc[5]);
#pragma unroll
        for (int q = 0; q < kFactorRefMax; ++q) {
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[6 + 4 * q + c] = fma(v[c], v[3 + q], acc[6 + 4 * q + c]);
            acc[6 + 4 * q + 3] = fma(v[3 + q], v[3 + q], acc[6 + 4 * q + 3]);
        }
    }
#pragma unroll
    for (int s = 0; s < kFactorSums; ++s) {
        red[tid] = acc[s];
        __syncthreads();
        for (int off = kFactorBlock / 2; off > 0; off >>= 1) {
            if (tid < off) red[tid] = red[tid] + red[tid + off];
            __syncthreads();
        }
        if (tid == 0) sums[s] = red[0];
        __syncthreads();
    }
    if (tid != 0) return;
    const double *__restrict__ prr = st.prr[a.cur];
    const double S00 = prr[0] - sums[0], S10 = prr[3] - sums[1], S11 = prr[4] - sums[2];
    const double S20 = prr[6] - sums[3], S21 = prr[7] - sums[4], S22 = prr[8] - sums[5];
    double l00 = 0.0, l10 = 0.0, l11 = 0.0, l20 = 0.0, l21 = 0.0, l22 = 0.0, d = S00;
    int taken = 0;
    if (!factor_pivot_bad(d)) {
        l00 = sqrt(d); l10 = S10 / l00; l20 = S20 / l00; taken = 1;
        d = fma(-l10, l10, S11);
        if (!factor_pivot_bad(d)) {
            l11 = sqrt(d); l21 = fma(-l20, l10, S21) / l11; taken = 2;
            d = fma(-l21, l21, fma(-l20, l20, S22));
            if (!factor_pivot_bad(d)) { l22 = sqrt(d); taken = 3; }
        }
    }
    a.res[3] = l00; a.res[4] = l11; a.res[5] = l22; a.res[6] = (double)taken;
    if (taken < 3) { a.res[1] = (double)taken; a.res[2] = d; a.res[0] = 2.0; return; }
    if (a.lr_off) { a.lr_off[0] = l10; a.lr_off[1] = l20; a.lr_off[2] = l21; }      // (ekf_sample_map: the rest of L_r)
    for (int q = 0; q < a.nref; ++q) {
        const double *__restrict__ x = st.x[a.cur], *__restrict__ ref = a.ref + q * a.ref_stride;
        const double t0 = (x[0] - ref[0]) - sums[6 + 4 * q], t1 = (x[1] - ref[1]) - sums[7 + 4 * q];
        const double t2 = ekfm::wrap180(x[2] - ref[2]) - sums[8 + 4 * q];
        const double y0 = t0 / l00, y1 = fma(-l10, y0, t1) / l11, y2 = fma(-l21, y1, fma(-l20, y0, t2)) / l22;
        a.res[8 + q] = fma(y2, y2, fma(y1, y1, fma(y0, y0, sums[9 + 4 * q])));
    }
}
