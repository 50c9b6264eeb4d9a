// Fragment of kernels.hip (included there, inside its anonymous namespace, after joint_update.h): a scan's pairings applied as ONE joint
// update, RELINEARISED (ekf_observe_model_joint_iterated): k_joint_factor_iter.
#pragma once

// ---------------------------------------------------------------------------------------------------
// Gauss-Newton on the MAP cost over the sub-state xi = (x_r, l_0 .. l_{np-1}) of the paired landmarks (device_math.h, "The ITERATED joint
// update"): linearisation 0 is joint_phases itself -- so S, nu, d2 and the first record are ekf_joint_innovation's bits -- and every further
// one runs the same per-pairing and cross-block texts at xi_i with the PRIOR covariance operands, which stay on-die: prr and the strips in
// JointLds as joint_phases left them, the landmarks' own blocks and the cross blocks P(l_a, l_b) read ONCE here (pmm_low_chain on the flushed
// state: no pending pair) because joint_phases discards them.  The residual r_i = nu_i - H_i (x0 - xi_i) takes nu's place in y, so the
// factorisation leaves y_i = L_i^-1 r_i; the move is v = L_i^-T y_i, xi_{i+1} = x0 + P_sub (H_i' v).
// What leaves is the LAST linearisation's: L, y, H and W_r = L^-1 G_r in the JointBlock (k_joint_factor's text for G_r and its substitution),
// from which k_gather_joint forms x' = x0 + W' y and P' = P - W' W unchanged.  With iterations == 1 the block is k_joint_factor's bit for
// bit.  Nothing of the state is written.  One workgroup; phases are separated by barriers and every loop exit is uniform: each lane reads
// the same pivots, posed flags and moves from LDS.
// LDS: JointLds 36 KiB, the cross blocks 15.5 KiB, the sub-state vectors and W_r 6 KiB.
// ---------------------------------------------------------------------------------------------------
struct JointIterLds {
    double pab[4 * (kJointMax * (kJointMax - 1) / 2)];     // by (a, b), a > b: row-major 2 x 2
    double diag3[kJointMax][3];                             // by pairing: the landmark's own block
    double x0[kJointSubMax], xi[kJointSubMax], xn[kJointSubMax], u[kJointSubMax], dstep[kJointSubMax];
    double t[kJointRows], v[kJointRows];
    JointRecord rec0;
};

template <typename TS>
__global__ __launch_bounds__(kJointBlock) void k_joint_factor_iter(DevState st, JointArgs a, JointIterArgs ia, const int64_t *__restrict__ hyp,
                                                                   JointBlock *__restrict__ blk, JointRecord *__restrict__ out,
                                                                   double *__restrict__ itrec, double *__restrict__ nu_out,
                                                                   double *__restrict__ S_out) {
    __shared__ JointLds sh;
    __shared__ double Wr[kJointRows][3];
    __shared__ JointIterLds it;
    const int tid = threadIdx.x;
    constexpr int ld = kJointRows;
    const JointCounts cnt = joint_phases<TS>(st, a, hyp, sh, tid, nu_out, S_out);
    const int np = cnt.np, n = 2 * np, ns = 3 + n;
    const bool regular = cnt.bad == np;

    // the first record, before y is overwritten; the prior operands joint_phases does not keep; xi_0 = x0
    if (tid == 0) it.rec0 = joint_record(sh, cnt, a.m, nullptr);
    for (int q = tid; q < 3; q += kJointBlock) { it.x0[q] = st.x[a.cur][q]; it.xi[q] = it.x0[q]; }
    for (int p = tid; p < np; p += kJointBlock) {
        const int64_t i = sh.lm[sh.scan_of[p]];
        const double *__restrict__ dg = st.diag[st.dcur] + 3 * i;
        for (int q = 0; q < 3; ++q) it.diag3[p][q] = dg[q];
        for (int c = 0; c < 2; ++c) { it.x0[3 + 2 * p + c] = st.x[a.cur][3 + 2 * i + c]; it.xi[3 + 2 * p + c] = it.x0[3 + 2 * p + c]; }
    }
    for (int idx = tid; idx < np * (np - 1) / 2; idx += kJointBlock) {
        int pa = 1;
        while (pa * (pa + 1) / 2 <= idx) ++pa;
        const int pb = idx - pa * (pa - 1) / 2;
        const int64_t ra = 2 * sh.lm[sh.scan_of[pa]], rb = 2 * sh.lm[sh.scan_of[pb]];
        for (int q = 0; q < 4; ++q) it.pab[4 * idx + q] = pmm_low_chain<TS>(st, a.pstart, 0, ra + (q >> 1), rb + (q & 1));
    }
    __syncthreads();

    int used = 0, converged = 0, irr_at = -1, irr_obs = -1;
    double step = 0.0, d2_last = it.rec0.d2;
    const double *xs = it.xi;                           // xi_used
    if (regular && it.rec0.d2 <= ia.gate)
        for (int i = 0;; ++i) {
            if (i > 0) {
                // (1) per pairing at xi_i, the residual in nu's place
                for (int p = tid; p < np; p += kJointBlock) {
                    const AssocModelEntry &e = a.e[sh.scan_of[p]];
                    double S[4], r[2], hr[6], ht[4];
                    sh.posed[p] = ekfm::joint_iter_pairing(e.model, e.z, e.R, sh.prr, sh.strips[p], it.diag3[p], it.x0, it.x0 + 3 + 2 * p, it.xi,
                                                           it.xi + 3 + 2 * p, hr, ht, S, r) ? 1 : 0;
                    for (int q = 0; q < 6; ++q) sh.Hr[p][q] = hr[q];
                    for (int q = 0; q < 4; ++q) sh.Ht[p][q] = ht[q];
                    sh.y[2 * p] = r[0]; sh.y[2 * p + 1] = r[1];
                    sh.A[(2 * p) * ld + 2 * p] = S[0]; sh.A[(2 * p) * ld + 2 * p + 1] = S[1];
                    sh.A[(2 * p + 1) * ld + 2 * p] = S[2]; sh.A[(2 * p + 1) * ld + 2 * p + 1] = S[3];
                }
                __syncthreads();
                // (2) the off-diagonal blocks, a > b, from the kept P(l_a, l_b)
                for (int idx = tid; idx < np * (np - 1) / 2; idx += kJointBlock) {
                    int pa = 1;
                    while (pa * (pa + 1) / 2 <= idx) ++pa;
                    const int pb = idx - pa * (pa - 1) / 2;
                    double Sab[4];
                    ekfm::joint_cross_block(sh.Hr[pa], sh.Ht[pa], sh.Hr[pb], sh.Ht[pb], sh.prr, sh.strips[pa], sh.strips[pb], it.pab + 4 * idx, Sab);
                    for (int q = 0; q < 4; ++q) sh.A[(2 * pa + (q >> 1)) * ld + 2 * pb + (q & 1)] = Sab[q];
                }
                __syncthreads();
                // (4) the factorisation, joint_phases' loop
                int bad = np;
                for (int p = np - 1; p >= 0; --p)
                    if (!sh.posed[p]) bad = p;
                for (int k = 0; k < 2 * bad; ++k) {
                    double lkk;
                    if (!ekfm::joint_pivot(sh.A[k * ld + k], lkk)) { bad = k >> 1; break; }
                    ekfm::joint_factor_scale(sh.A, ld, sh.y, n, k, lkk, tid, kJointBlock);
                    __syncthreads();
                    ekfm::joint_factor_update(sh.A, ld, sh.y, n, k, tid, kJointBlock);
                    __syncthreads();
                }
                if (bad < np) { irr_at = i; irr_obs = sh.scan_of[bad]; break; }
                d2_last = 0.0;
                for (int p = 0; p < np; ++p) d2_last = ekfm::joint_prefix_add(d2_last, sh.y[2 * p], sh.y[2 * p + 1]);
            }
            // the move: v = L^-T y, u = H' v, xi_{i+1} = x0 + P_sub u
            for (int k = tid; k < n; k += kJointBlock) it.t[k] = sh.y[k];
            __syncthreads();
            for (int k = n - 1; k >= 0; --k) {
                ekfm::joint_back_step(sh.A, ld, it.t, it.v, k, tid, kJointBlock);
                __syncthreads();
            }
            ekfm::joint_iter_Htv(&sh.Hr[0][0], &sh.Ht[0][0], it.v, np, it.u, tid, kJointBlock);
            __syncthreads();
            ekfm::joint_iter_move(sh.prr, &sh.strips[0][0], &it.diag3[0][0], it.pab, np, it.x0, it.u, it.xi, it.xn, it.dstep, tid, kJointBlock);
            __syncthreads();
            step = ekfm::joint_iter_step(it.dstep, ns);
            used = i + 1;
            converged = step <= ia.tol;
            xs = it.xn;
            if (converged || used == ia.iterations) break;
            for (int k = tid; k < ns; k += kJointBlock) it.xi[k] = it.xn[k];
            xs = it.xi;
            __syncthreads();
        }

    const bool whole = regular && irr_at < 0;           // sh holds a factored linearisation: the last one
    if (whole) {
        // k_joint_factor's text from here to the block: G_r, every sum in ascending index order, the robot's terms before the landmark's
        for (int e = tid; e < 3 * n; e += kJointBlock) {
            const int i = e / 3, t = e - 3 * i, p = i >> 1, s = i & 1;
            double v = 0.0;
            for (int u = 0; u < 3; ++u) v += sh.Hr[p][3 * s + u] * (t >= u ? sh.prr[3 * t + u] : sh.prr[3 * u + t]);
            for (int c = 0; c < 2; ++c) v += sh.Ht[p][2 * s + c] * sh.strips[p][2 * t + c];
            Wr[i][t] = v;
        }
        __syncthreads();
        // W_r = L^-1 G_r, column by column of L
        for (int k = 0; k < n; ++k) {
            const double lkk = sqrt(sh.A[k * ld + k]);
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
    for (int k = tid; k < kJointSubMax + 1; k += kJointBlock) itrec[8 + k] = k < ns ? xs[k] : 0.0;
    if (tid == 0) {
        blk->np = whole ? np : 0; blk->pad = 0;
        blk->rec = it.rec0;
        out[0] = it.rec0;
        itrec[0] = (double)used; itrec[1] = (double)converged; itrec[2] = step; itrec[3] = d2_last;
        itrec[4] = (double)irr_at; itrec[5] = (double)irr_obs; itrec[6] = (double)ns; itrec[7] = 0.0;
    }
}
