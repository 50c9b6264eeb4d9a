// Fragment of kernels.hip (included there, inside its anonymous namespace, after associate_model.h): the joint compatibility of a scan's
// pairings (ekf_joint_innovation): k_joint_innovation.
#pragma once

// ---------------------------------------------------------------------------------------------------
// A hypothesis pairs observation k of a scan with landmark hyp[k] (or leaves it out: -1).  Its paired rows, stacked, have
//     S = H P H' + blockdiag(R_k)      nu = (z_k - h_k(x))_k      d2 = nu' S^-1 nu
// and d2 is what a joint-compatibility search tests against chi2(dof): unlike the m individual d2 it sees that all innovations share the
// robot's error.  One 256-lane workgroup per hypothesis; nothing of the state is written, no atomics, no workgroup reads what another
// writes; every phase ends with a barrier.  Pairing p (the p-th paired entry in scan order) owns rows 2 p, 2 p + 1 of the stacked system.
//   (1) lane k < m, per pairing: assoc_model_d2's operands (live F64 copies: they carry every pending pair) through ekfm::joint_pairing --
//       S_pp and nu_p are ekf_model_innovation's bit for bit -- and H_p, the strip columns and the posed flag left in LDS.
//   (2) one lane per off-diagonal block (a > b, <= 496 of them): P(l_a, l_b) through pmm_low_chain (the canonical lower-triangle entry,
//       swapped where l_a < l_b, patched with the pending pairs in slot order), then ekfm::joint_cross_block.
//   (3) nu and S copied out by scan index where asked (an unpaired entry: zero rows of nu, the identity on S's diagonal) -- before
//   (4) the right-looking Cholesky with the forward substitution riding along (ekfm::joint_factor_*), two barriers a step.  It stops at
//       the first row whose pivot is not finite and positive, or at the first pairing that is not posed: that pairing is the
//       hypothesis's first irregular one, and everything before it is what it would be without it (L's leading block depends on S's
//       leading block alone).
//   (5) lane 0: the prefixes, summed over y^2 in ascending row order, and the record.
// LDS: S dense, 64 x 64 doubles = 32 KiB, and 3.6 KiB of per-pairing operands.
// ---------------------------------------------------------------------------------------------------
constexpr int kJointBlock = 256;

template <typename TS>
__global__ __launch_bounds__(kJointBlock) void k_joint_innovation(DevState st, JointArgs a, const int64_t *__restrict__ hyp,
                                                                  JointRecord *__restrict__ out, double *__restrict__ d2_prefix,
                                                                  double *__restrict__ nu_out, double *__restrict__ S_out) {
    __shared__ double A[kJointRows * kJointRows];
    __shared__ double y[kJointRows];
    __shared__ double Hr[kJointMax][6], Ht[kJointMax][4], strips[kJointMax][6], prr[9];
    __shared__ int64_t lm[kJointMax];               // by scan index: the hypothesis
    __shared__ int pair_of[kJointMax];              // by scan index: the pairing, -1 = left out
    __shared__ int scan_of[kJointMax];              // by pairing: the scan index
    __shared__ int posed[kJointMax];                // by pairing
    const int tid = threadIdx.x;
    const int m = a.m, cur = a.cur;
    const int64_t hi = blockIdx.x;
    constexpr int ld = kJointRows;

    if (tid < m) lm[tid] = hyp[hi * m + tid];
    if (tid >= 64 && tid < 73) prr[tid - 64] = st.prr[cur][tid - 64];
    __syncthreads();
    int np = 0, dof = 0;                            // pairings, real rows: every lane counts them alike
    for (int k = 0; k < m; ++k)
        if (lm[k] >= 0) { ++np; dof += (a.e[k].model == 1 || a.e[k].model == 4) ? 2 : 1; }
    const int n = 2 * np;

    // (1) per pairing
    if (tid < m) {
        int p = -1;
        if (lm[tid] >= 0) {
            p = 0;
            for (int k = 0; k < tid; ++k) p += lm[k] >= 0;
        }
        pair_of[tid] = p;
        if (p >= 0) {
            const AssocModelEntry &e = a.e[tid];
            const int64_t i = lm[tid];
            const double *__restrict__ x = st.x[cur];
            const double *__restrict__ strip = st.strip[cur] + 2 * i;
            const double *__restrict__ dg = st.diag[st.dcur] + 3 * i;
            const int64_t ldm = st.ldm;
            double p9[9];
            for (int q = 0; q < 9; ++q) p9[q] = st.prr[cur][q];
            const double xr[3] = { x[0], x[1], x[2] };
            const double l[2] = { x[3 + 2 * i], x[4 + 2 * i] };
            const double strip6[6] = { strip[0], strip[1], strip[ldm], strip[ldm + 1], strip[2 * ldm], strip[2 * ldm + 1] };
            const double diag3[3] = { dg[0], dg[1], dg[2] };
            double S[4], nu[2], hr[6], ht[4];
            posed[p] = ekfm::joint_pairing(e.model, e.z, e.R, p9, strip6, diag3, xr, l, hr, ht, S, nu) ? 1 : 0;
            scan_of[p] = tid;
            for (int q = 0; q < 6; ++q) { Hr[p][q] = hr[q]; strips[p][q] = strip6[q]; }
            for (int q = 0; q < 4; ++q) Ht[p][q] = ht[q];
            y[2 * p] = nu[0]; y[2 * p + 1] = nu[1];
            A[(2 * p) * ld + 2 * p] = S[0]; A[(2 * p) * ld + 2 * p + 1] = S[1];       // the block whole: S[1] is what the record reports
            A[(2 * p + 1) * ld + 2 * p] = S[2]; A[(2 * p + 1) * ld + 2 * p + 1] = S[3];
        }
    }
    __syncthreads();

    // (2) the off-diagonal blocks, a > b
    for (int idx = tid; idx < np * (np - 1) / 2; idx += kJointBlock) {
        int pa = 1;
        while (pa * (pa + 1) / 2 <= idx) ++pa;
        const int pb = idx - pa * (pa - 1) / 2;
        const int64_t ra = 2 * lm[scan_of[pa]], rb = 2 * lm[scan_of[pb]];
        double pab[4], Sab[4];
        for (int q = 0; q < 4; ++q) pab[q] = pmm_low_chain<TS>(st, a.pstart, a.npend, ra + (q >> 1), rb + (q & 1));
        ekfm::joint_cross_block(Hr[pa], Ht[pa], Hr[pb], Ht[pb], prr, strips[pa], strips[pb], pab, Sab);
        for (int q = 0; q < 4; ++q) A[(2 * pa + (q >> 1)) * ld + 2 * pb + (q & 1)] = Sab[q];
    }
    __syncthreads();

    // (3) nu and S by scan index, before the factorisation overwrites them
    if (nu_out)
        for (int i = tid; i < 2 * m; i += kJointBlock) {
            const int p = pair_of[i >> 1];
            nu_out[hi * 2 * m + i] = p >= 0 ? y[2 * p + (i & 1)] : 0.0;
        }
    if (S_out)
        for (int e = tid; e < 4 * m * m; e += kJointBlock) {
            const int i = e % (2 * m), j = e / (2 * m);             // column-major
            const int pi = pair_of[i >> 1], pj = pair_of[j >> 1];
            double v = i == j ? 1.0 : 0.0;
            if (pi >= 0 && pj >= 0) {
                const int ri = 2 * pi + (i & 1), rj = 2 * pj + (j & 1);
                v = (ri >= rj || pi == pj) ? A[ri * ld + rj] : A[rj * ld + ri];
            }
            S_out[hi * 4 * m * m + e] = v;
        }
    __syncthreads();

    // (4) the factorisation, up to the first pairing that has no d2
    int bad = np;                                   // the first irregular pairing; np: none
    for (int p = np - 1; p >= 0; --p)
        if (!posed[p]) bad = p;
    for (int k = 0; k < 2 * bad; ++k) {
        double lkk;
        if (!ekfm::joint_pivot(A[k * ld + k], lkk)) { bad = k >> 1; break; }       // every lane reads the same pivot: a uniform exit
        ekfm::joint_factor_scale(A, ld, y, n, k, lkk, tid, kJointBlock);
        __syncthreads();
        ekfm::joint_factor_update(A, ld, y, n, k, tid, kJointBlock);
        __syncthreads();
    }

    // (5) the prefixes and the record
    if (tid == 0) {
        double acc = 0.0;
        for (int k = 0; k < m; ++k) {
            const int p = pair_of[k];
            if (p >= 0) acc = p < bad ? ekfm::joint_prefix_add(acc, y[2 * p], y[2 * p + 1]) : NAN;
            if (d2_prefix) d2_prefix[hi * m + k] = acc;
        }
        JointRecord r;
        r.d2 = acc; r.dof = dof; r.pairings = np;
        r.outcome = bad < np ? 0 : 1;
        r.first_irregular = bad < np ? scan_of[bad] : -1;
        out[hi] = r;
    }
}
