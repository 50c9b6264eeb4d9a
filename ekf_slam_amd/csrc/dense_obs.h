// Fragment of kernels.hip (included there, inside its anonymous namespace, after multiply_map.h): a linear observation whose k x n H is
// DENSE (ekf_observe_dense): k_dense_gram, k_dense_factor, k_gather_dense.
#pragma once

// ---------------------------------------------------------------------------------------------------
// "H x = z +- R", exact, no linearisation.  The rows of H are the vectors of one chunk of the plain product (multiply_map.h), so
// G = P H' is what k_multiply_tiles / k_multiply_sum / k_multiply_robot left in the chunk y: column i at i * ld, the landmark rows first,
// the robot's three at `rows`; rows 2 N .. rows - 1 of y were never written and are never read here (a lane without a live row works
// on zeros).  With S = H G + R, nu = z - H x, L L' = S, W = L^-1 G' and y = L^-1 nu:
//     d2 = |y|^2        x' = x + W' y        P' = P - W' W
// the symmetric form of joint_update.h, whose rank-2 pairs are rows 2 p, 2 p + 1 of W, twice.  The stacked system has kk = k rounded up to
// even rows; the host pads an odd k with the exactly empty row (H = 0, R = e e', z = 0), whose pivot is 1 and whose w is 0.
//
// k_dense_gram: one workgroup per segment of kDenseSegment landmark rows.  H and G of the segment go through LDS (coalesced loads, a
// pitch of kDenseSegment + 1 doubles: lanes of different rows read different banks, lanes of one row the same word); lane q owns ONE
// sum -- entry (i, j), j <= i, of H G, or row i of H x -- and adds its segment's products in ASCENDING ROW ORDER.  No atomics; a
// segment's block depends on nothing but its rows.
// ---------------------------------------------------------------------------------------------------
constexpr int kDenseBlock = 256;
#ifndef EKF_DENSE_LANES
#define EKF_DENSE_LANES 256
#endif
constexpr int kDenseFactorBlock = EKF_DENSE_LANES;      // (a host emulation runs k_dense_factor with ONE lane: every phase is a loop strided by it)
constexpr int kDensePitch = kDenseSegment + 1;

// q -> (i, j), j <= i, with q = i (i + 1) / 2 + j
__device__ __forceinline__ void dense_tri(int q, int &i, int &j) {
    i = 0;
    while ((i + 1) * (i + 2) / 2 <= q) ++i;
    j = q - i * (i + 1) / 2;
}

__global__ __launch_bounds__(kDenseBlock) void k_dense_gram(DevState st, DenseArgs a) {
    static_assert(kDensePartial <= kDenseBlock, "a lane per sum");
    __shared__ double Hs[kDenseMax][kDensePitch];
    __shared__ double Gs[kDenseMax][kDensePitch];
    __shared__ double xs[kDenseSegment];
    const int tid = threadIdx.x, n = a.kk, tri = n * (n + 1) / 2;
    const int64_t row0 = (int64_t)blockIdx.x * kDenseSegment;
    for (int e = tid; e < n * kDenseSegment; e += kDenseBlock) {
        const int r = e / kDenseSegment, c = e % kDenseSegment;
        const bool live = row0 + c < a.n_mm;
        Hs[r][c] = live ? a.b[(int64_t)r * a.ld + row0 + c] : 0.0;
        Gs[r][c] = live ? a.y[(int64_t)r * a.ld + row0 + c] : 0.0;
    }
    for (int c = tid; c < kDenseSegment; c += kDenseBlock) xs[c] = row0 + c < a.n_mm ? buffer_of(st.x, a.cur)[3 + row0 + c] : 0.0;
    __syncthreads();
    double *__restrict__ out = a.part + (int64_t)blockIdx.x * kDensePartial;
    if (tid < tri) {
        int i, j;
        dense_tri(tid, i, j);
        double acc = 0.0;
        for (int c = 0; c < kDenseSegment; ++c) acc = acc + Hs[i][c] * Gs[j][c];
        out[tid] = acc;
    } else if (tid >= kDenseBlock - kDenseMax && tid - (kDenseBlock - kDenseMax) < n) {       // (the last wavefront: it has no triangle lane)
        const int i = tid - (kDenseBlock - kDenseMax);
        double acc = 0.0;
        for (int c = 0; c < kDenseSegment; ++c) acc = acc + Hs[i][c] * xs[c];
        out[kDenseMax * (kDenseMax + 1) / 2 + i] = acc;
    }
}

// ---------------------------------------------------------------------------------------------------
// k_dense_factor: ONE workgroup.  Entry (i, j) of S is the segments' partials added in ascending segment order, then the robot's three
// products in ascending order, then R(i, j); the lower triangle is formed and mirrored.  nu(i) = z(i) - (H x)(i), summed the same way,
// wrapped into (-180, 180] where wrap says so.  nu and S are copied out, then the right-looking Cholesky of joint.h (ekfm::joint_pivot /
// joint_factor_scale / joint_factor_update, two barriers a step) with y = L^-1 nu riding along; it stops at the first row whose pivot is
// not finite and positive.  A regular S: d2 = sum y^2 in ascending row order, W_r = L^-1 G_r by k_joint_factor's chain, and L, y, W_r into
// the block.  Nothing of the state is written; an irregular S leaves a block that is not read: the host decides from the record.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kDenseFactorBlock) void k_dense_factor(DevState st, DenseArgs a, DenseSmall sm, DenseOut *__restrict__ out,
                                                              DenseBlock *__restrict__ blk) {
    __shared__ double A[kDenseMax * kDenseMax];
    __shared__ double y[kDenseMax];
    __shared__ double Wr[kDenseMax][3];
    constexpr int ld = kDenseMax, kTri = kDenseMax * (kDenseMax + 1) / 2;
    const int tid = threadIdx.x, n = a.kk, tri = n * (n + 1) / 2;
    const int64_t nseg = (a.n_mm + kDenseSegment - 1) / kDenseSegment;
    for (int e = tid; e < tri + n; e += kDenseFactorBlock) {
        double acc = 0.0;
        if (e < tri) {
            int i, j;
            dense_tri(e, i, j);
            for (int64_t s = 0; s < nseg; ++s) acc = acc + a.part[s * kDensePartial + e];
            for (int t = 0; t < 3; ++t) acc = acc + a.b[(int64_t)i * a.ld + a.rows + t] * a.y[(int64_t)j * a.ld + a.rows + t];
            acc = acc + sm.R[i * ld + j];
            A[i * ld + j] = acc;
            A[j * ld + i] = acc;
        } else {
            const int i = e - tri;
            for (int64_t s = 0; s < nseg; ++s) acc = acc + a.part[s * kDensePartial + kTri + i];
            for (int t = 0; t < 3; ++t) acc = acc + a.b[(int64_t)i * a.ld + a.rows + t] * buffer_of(st.x, a.cur)[t];
            double nu = sm.z[i] - acc;
            if (sm.wrap[i]) nu = ekfm::wrap180(nu);
            y[i] = nu;
        }
    }
    __syncthreads();
    for (int e = tid; e < kDenseMax * kDenseMax; e += kDenseFactorBlock) {
        const int i = e / ld, j = e - i * ld;
        out->S[e] = i < n && j < n ? A[e] : 0.0;
    }
    for (int i = tid; i < kDenseMax; i += kDenseFactorBlock) out->nu[i] = i < n ? y[i] : 0.0;
    __syncthreads();

    int bad = n;                                     // the first row whose pivot is not finite and positive; n: none
    for (int k = 0; k < n; ++k) {
        double lkk;
        if (!ekfm::joint_pivot(A[k * ld + k], lkk)) { bad = k; break; }       // every lane reads the same pivot: a uniform exit
        ekfm::joint_factor_scale(A, ld, y, n, k, lkk, tid, kDenseFactorBlock);
        __syncthreads();
        ekfm::joint_factor_update(A, ld, y, n, k, tid, kDenseFactorBlock);
        __syncthreads();
    }
    const bool regular = bad == n;
    if (regular) {
        for (int e = tid; e < 3 * n; e += kDenseFactorBlock) Wr[e / 3][e % 3] = a.y[(int64_t)(e / 3) * a.ld + a.rows + e % 3];
        __syncthreads();
        // W_r = L^-1 G_r, column by column of L: entry (i, t) loses L(i, k) W_r(k, t) in ascending k and is divided last -- the chain
        // k_gather_dense's lanes run for their own columns
        for (int k = 0; k < n; ++k) {
            const double lkk = sqrt(A[k * ld + k]);             // (the factorisation leaves the pivot on the diagonal: L_kk is its root, joint_pivot's)
            for (int t = tid; t < 3; t += kDenseFactorBlock) Wr[k][t] = Wr[k][t] / lkk;
            __syncthreads();
            for (int e = tid; e < 3 * (n - k - 1); e += kDenseFactorBlock) {
                const int i = k + 1 + e / 3, t = e % 3;
                Wr[i][t] = Wr[i][t] - A[i * ld + k] * Wr[k][t];
            }
            __syncthreads();
        }
        for (int e = tid; e < n * n; e += kDenseFactorBlock) {
            const int i = e / n, j = e - i * n;
            if (j <= i) blk->L[i * ld + j] = j < i ? A[i * ld + j] : sqrt(A[i * ld + i]);
        }
        for (int i = tid; i < n; i += kDenseFactorBlock) {
            blk->y[i] = y[i];
            for (int t = 0; t < 3; ++t) blk->Wr[i][t] = Wr[i][t];
        }
    }
    if (tid == 0) {
        double acc = regular ? 0.0 : NAN;
        for (int p = 0; regular && 2 * p < n; ++p) acc = ekfm::joint_prefix_add(acc, y[2 * p], y[2 * p + 1]);
        DenseRecord r;
        r.d2 = acc; r.rows = n; r.outcome = regular ? 1 : 0; r.bad_row = regular ? -1 : bad;
        out->rec = r;
    }
}

// ---------------------------------------------------------------------------------------------------
// k_gather_dense<kP>: one lane per landmark-block column c, 256 columns per workgroup, a.kk <= 2 kP rows.  L (packed by rows), y and W_r
// wait in LDS.  For i = 0 .. kk - 1 in order the lane loads g_i(c) = G[i ld + c] (coalesced: the chunk is column-major) and forms at once
// w_i = (g_i - sum_{j < i} L_ij w_j) / L_ii, ascending j: only w stays live, a fully unrolled register array.  From w alone it does what
// k_gather_joint (joint_update.h) does after its own w -- pair slot p (G and K both rows 2 p, 2 p + 1 of W, zeros over the padded tail),
// x'(c) = x(c) + sum w_i y_i, strip'(t, c) = strip(t, c) - sum W_r(i, t) w_i, the landmark's live diagonal block (lane_xor1 hands over
// the partner column's w), every sum in ascending i; workgroup 0 adds x_r' = x_r + W_r' y and Prr' = Prr - W_r' W_r under
// store_robot_part's mirror rule.  That tail is a TWIN of k_gather_joint's, kept as text of its own.  No tile is
// read, so there is no storage type among the template arguments.  N = 0: one workgroup, no live lane, the robot part alone.
// Reads state buffer a.cur / diagonal buffer st.dcur, writes the other ones whole; the pairs go to ring slots 0 .. kk / 2 - 1 of
// st.Gp / st.Kp (the caller's private F64 ring: no float copies).
// ---------------------------------------------------------------------------------------------------
template <int kP>
__global__ __launch_bounds__(kBlock) void k_gather_dense(DevState st, DenseArgs a, const DenseBlock *__restrict__ blk) {
    constexpr int kN = 2 * kP;
    static_assert(kN <= kDenseMax, "the rows of one chunk");
    __shared__ double Lp[kN * (kN + 1) / 2];
    __shared__ double ys[kN], Wr[kN][3];
    const int tid = threadIdx.x;
    const int cur = a.cur, n = a.kk, np = n >> 1;
    const int64_t c = (int64_t)blockIdx.x * kBlock + tid;
    const bool live = c < a.n_mm;

    for (int e = tid; e < n * n; e += kBlock) {
        const int i = e / n, j = e - i * n;
        if (j <= i) Lp[i * (i + 1) / 2 + j] = blk->L[i * kDenseMax + j];
    }
    for (int i = tid; i < n; i += kBlock) {
        ys[i] = blk->y[i];
        for (int t = 0; t < 3; ++t) Wr[i][t] = blk->Wr[i][t];
    }
    const ColumnOperands o = load_column_operands(st, cur, c, live);
    // G(:, c): every load issued before the chain needs the first
    double w[kN];
#pragma unroll
    for (int i = 0; i < kN; ++i) w[i] = live && i < n ? a.y[(int64_t)i * a.ld + c] : 0.0;
    __syncthreads();

    // w(:, c), row by row; a lane without a column works on zeros and ends with zeros
#pragma unroll
    for (int i = 0; i < kN; ++i) {
        if (i < n) {
            double acc = w[i];
#pragma unroll
            for (int j = 0; j < i; ++j) acc = acc - Lp[i * (i + 1) / 2 + j] * w[j];
            w[i] = acc / Lp[i * (i + 1) / 2 + i];
        }
    }

    // the pairs, x', strip' and the live diagonal block from w alone
    const int64_t pad_end = st.tm.padded(a.n_mm), ldm = st.ldm;
    double xs = 0.0, d0 = 0.0, d1 = 0.0, d2 = 0.0;
    double dgc = o.dgc, dgl = o.dgl;
#pragma unroll
    for (int p = 0; p < kP; ++p) {
        if (p < np) {
            const double2 wp = make_double2(w[2 * p], w[2 * p + 1]);
            if (c < pad_end) {
                const int64_t off = (int64_t)p * st.pair_stride;
                reinterpret_cast<double2 *>(st.Gp + off)[c] = wp;
                reinterpret_cast<double2 *>(st.Kp + off)[c] = wp;
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int i = 2 * p + s;
                xs = xs + w[i] * ys[i];
                d0 = d0 + Wr[i][0] * w[i];
                d1 = d1 + Wr[i][1] * w[i];
                d2 = d2 + Wr[i][2] * w[i];
            }
            const double2 wl = make_double2(lane_xor1(wp.x), lane_xor1(wp.y));      // the partner column's w (odd lanes: column 2k)
            dgc = rank2_apply(dgc, wp, wp);
            dgl = rank2_apply(dgl, wp, wl);
        }
    }
    if (live) {
        buffer_of(st.x, cur ^ 1)[3 + c] = o.xc + xs;
        double *__restrict__ strip = buffer_of(st.strip, cur ^ 1);
        strip[c] = o.s0 - d0;
        strip[ldm + c] = o.s1 - d1;
        strip[2 * ldm + c] = o.s2 - d2;
        store_diag_column(buffer_of(st.diag, st.dcur ^ 1), c, dgc, dgl);
    }

    // workgroup 0: x_r' and Prr', entry (r, b) and its mirror both the lower-triangle entry's value
    if (blockIdx.x == 0) {
        if (tid < 3) {
            double v = 0.0;
            for (int i = 0; i < n; ++i) v = v + Wr[i][tid] * ys[i];
            buffer_of(st.x, cur ^ 1)[tid] = buffer_of(st.x, cur)[tid] + v;
        }
        if (tid >= 64 && tid < 73) {
            const int q = tid - 64, r = q / 3, b = q - 3 * r;
            const int rr = r > b ? r : b, bb = r > b ? b : r;
            double v = 0.0;
            for (int i = 0; i < n; ++i) v = v + Wr[i][rr] * Wr[i][bb];
            buffer_of(st.prr, cur ^ 1)[3 * r + b] = buffer_of(st.prr, cur)[3 * rr + bb] - v;
        }
    }
}
