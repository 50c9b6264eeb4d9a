// Fragment of kernels.hip (included there, inside its anonymous namespace, after joint.h): a scan's pairings applied as ONE joint update
// (ekf_observe_model_joint): k_joint_factor, k_gather_joint.
#pragma once

// ---------------------------------------------------------------------------------------------------
// All np pairings of one hypothesis are linearised once, at the live state, and stacked (joint.h): S = H P H' + blockdiag(R_k), nu.  With
// L L' = S, W = L^-1 H P (2 np rows) and y = L^-1 nu the Kalman update is symmetric and needs no back substitution:
//     x' = x + W' y        P' = P - W' W
// so its rank-2 pairs are (K_p, G_p) = (rows 2 p, 2 p + 1 of W, twice) and ONE pass applies all np of them to the tiles (rank2_apply in
// slot order, as for every other pair).  The host flushes first: nothing is pending, the tiles hold the live P and no operand is patched.
//
// k_joint_factor: one workgroup, joint.h's phases (1)-(4) for the one hypothesis -- the same text k_joint_innovation runs, so S, nu, d2 and
// the record are its bits -- then G_r and the forward substitution of its three columns, and everything into the JointBlock.  Nothing of
// the state is written.  An irregular hypothesis leaves a block that is not read: the host decides from the record.
// ---------------------------------------------------------------------------------------------------
template <typename TS>
__global__ __launch_bounds__(kJointBlock) void k_joint_factor(DevState st, JointArgs a, const int64_t *__restrict__ hyp,
                                                              JointBlock *__restrict__ blk, JointRecord *__restrict__ out,
                                                              double *__restrict__ nu_out, double *__restrict__ S_out) {
    __shared__ JointLds sh;
    __shared__ double Wr[kJointRows][3];
    const int tid = threadIdx.x;
    constexpr int ld = kJointRows;
    const JointCounts cnt = joint_phases<TS>(st, a, hyp, sh, tid, nu_out, S_out);
    const int np = cnt.np, n = 2 * np;
    const bool regular = cnt.bad == np;
    if (regular) {
        // G_r, every sum in ascending index order, the robot's terms before the landmark's; Prr read from its lower triangle
        for (int e = tid; e < 3 * n; e += kJointBlock) {
            const int i = e / 3, t = e - 3 * i, p = i >> 1, s = i & 1;
            double v = 0.0;
            for (int u = 0; u < 3; ++u) v += sh.Hr[p][3 * s + u] * (t >= u ? sh.prr[3 * t + u] : sh.prr[3 * u + t]);
            for (int c = 0; c < 2; ++c) v += sh.Ht[p][2 * s + c] * sh.strips[p][2 * t + c];
            Wr[i][t] = v;
        }
        __syncthreads();
        // W_r = L^-1 G_r, column by column of L: entry (i, t) loses L(i, k) W_r(k, t) in ascending k and is divided last -- the chain
        // k_gather_joint's lanes run for their own columns
        for (int k = 0; k < n; ++k) {
            const double lkk = sqrt(sh.A[k * ld + k]);          // (the factorisation leaves the pivot on the diagonal: L_kk is its root, joint_pivot's)
            for (int t = tid; t < 3; t += kJointBlock) Wr[k][t] = Wr[k][t] / lkk;
            __syncthreads();
            for (int e = tid; e < 3 * (n - k - 1); e += kJointBlock) {
                const int i = k + 1 + e / 3, t = e % 3;
                Wr[i][t] = Wr[i][t] - sh.A[i * ld + k] * Wr[k][t];
            }
            __syncthreads();
        }
        for (int e = tid; e < n * n; e += kJointBlock) {
            const int i = e / n, j = e - i * n;
            if (j <= i) blk->L[i * ld + j] = j < i ? sh.A[i * ld + j] : sqrt(sh.A[i * ld + i]);
        }
        for (int i = tid; i < n; i += kJointBlock) {
            blk->y[i] = sh.y[i];
            for (int t = 0; t < 3; ++t) blk->Wr[i][t] = Wr[i][t];
        }
        for (int p = tid; p < np; p += kJointBlock) {
            for (int q = 0; q < 6; ++q) blk->Hr[p][q] = sh.Hr[p][q];
            for (int q = 0; q < 4; ++q) blk->Ht[p][q] = sh.Ht[p][q];
            blk->lm[p] = sh.lm[sh.scan_of[p]];
        }
    }
    if (tid == 0) {
        const JointRecord r = joint_record(sh, cnt, a.m, nullptr);
        blk->np = regular ? np : 0; blk->pad = 0;
        blk->rec = r;
        out[0] = r;
    }
}

// ---------------------------------------------------------------------------------------------------
// k_gather_joint<TS, kP>: one lane per landmark-block column c, 256 columns per workgroup, a.np <= kP pairings.  L (packed by rows), y, W_r and the
// Jacobian blocks wait in LDS.  For i = 0 .. 2 np - 1 in order the lane forms
//     g_i(c) = H_p^r(s, :) strip(:, c) + H_p^t(s, :) P(2 l_p .. 2 l_p + 1, c)            i = 2 p + s
// (constrain_row_pair: the canonical lower-triangle tile entry, transposed right of the landmark, the landmark's own columns from the live
// F64 diagonal copy) and at once w_i = (g_i - sum_{j < i} L_ij w_j) / L_ii, ascending j: only w stays live, a fully unrolled register array.
// From w alone: pair slot p (G and K both rows 2 p, 2 p + 1 of W, zeros over the padded tail), x'(c) = x(c) + sum w_i y_i,
// strip'(t, c) = strip(t, c) - sum W_r(i, t) w_i, the landmark's live diagonal block (lane_xor1 hands over the partner column's w) --
// every sum in ascending i.  Workgroup 0 adds x_r' = x_r + W_r' y and Prr' = Prr - W_r' W_r under store_robot_part's mirror rule.
// Reads state buffer a.cur / diagonal buffer st.dcur, writes the other ones whole; the pairs go to ring slots 0 .. np - 1 of st.Gp / st.Kp
// (the caller's private F64 ring: no float copies).
// ---------------------------------------------------------------------------------------------------
template <typename TS, int kP>
__global__ __launch_bounds__(kBlock) void k_gather_joint(DevState st, JointUpdateArgs a, const JointBlock *__restrict__ blk) {
    constexpr int kN = 2 * kP;
    __shared__ double Lp[kN * (kN + 1) / 2];
    __shared__ double ys[kN], Wr[kN][3], Hr[kP][6], Ht[kP][4];
    __shared__ int64_t lms[kP];
    const int tid = threadIdx.x;
    const int cur = a.cur, np = a.np, n = 2 * np;
    const int64_t c = (int64_t)blockIdx.x * kBlock + tid;
    const bool live = c < a.n_mm;

    for (int e = tid; e < n * n; e += kBlock) {
        const int i = e / n, j = e - i * n;
        if (j <= i) Lp[i * (i + 1) / 2 + j] = blk->L[i * kJointRows + j];
    }
    for (int i = tid; i < n; i += kBlock) {
        ys[i] = blk->y[i];
        for (int t = 0; t < 3; ++t) Wr[i][t] = blk->Wr[i][t];
    }
    for (int p = tid; p < np; p += kBlock) {
        for (int q = 0; q < 6; ++q) Hr[p][q] = blk->Hr[p][q];
        for (int q = 0; q < 4; ++q) Ht[p][q] = blk->Ht[p][q];
        lms[p] = blk->lm[p];
    }
    const ColumnOperands o = load_column_operands(st, cur, c, live);
    __syncthreads();

    // w(:, c), pairing by pairing; a lane without a column works on zeros and ends with zeros
    double w[kN];
#pragma unroll
    for (int p = 0; p < kP; ++p) {
        w[2 * p] = 0.0; w[2 * p + 1] = 0.0;
        if (p < np) {
            double m0 = 0.0, m1 = 0.0;
            if (live) constrain_row_pair<TS>(st, 2 * lms[p], c, m0, m1);
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int i = 2 * p + s;
                double acc = Hr[p][3 * s] * o.s0;
                acc += Hr[p][3 * s + 1] * o.s1;
                acc += Hr[p][3 * s + 2] * o.s2;
                acc += Ht[p][2 * s] * m0;
                acc += Ht[p][2 * s + 1] * m1;
#pragma unroll
                for (int j = 0; j < i; ++j) acc = acc - Lp[i * (i + 1) / 2 + j] * w[j];
                w[i] = acc / Lp[i * (i + 1) / 2 + i];
            }
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
