// Fragment of kernels.hip (included there, inside its anonymous namespace, after associate_model.h): the joint compatibility of a scan's
// pairings (ekf_joint_innovation): k_joint_innovation, and its phases as functions that k_joint_factor (joint_update.h) calls too.
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
#ifndef EKF_JOINT_LANES
#define EKF_JOINT_LANES 256
#endif
constexpr int kJointBlock = EKF_JOINT_LANES;     // (a host emulation runs the phases with ONE lane: every phase is a loop strided by it)

// The LDS of one hypothesis and phases (1)-(4) as ONE text: k_joint_innovation below and k_joint_factor (joint_update.h) both call
// joint_phases, so S, nu, L and y = L^-1 nu are the same bits in both by construction.
struct JointLds {
    double A[kJointRows * kJointRows];
    double y[kJointRows];
    double Hr[kJointMax][6], Ht[kJointMax][4], strips[kJointMax][6], prr[9];
    int64_t lm[kJointMax];                          // by scan index: the hypothesis
    int pair_of[kJointMax];                         // by scan index: the pairing, -1 = left out
    int scan_of[kJointMax];                         // by pairing: the scan index
    int posed[kJointMax];                           // by pairing
};
struct JointCounts { int np, dof, bad; };           // pairings, real rows, the first irregular pairing (np: none)

// hyp: the hypothesis's m entries; nu_out / S_out: this hypothesis's 2m / 4m^2 entries, or nullptr.  Called by all kJointBlock lanes.
template <typename TS>
__device__ __forceinline__ JointCounts joint_phases(const DevState &st, const JointArgs &a, const int64_t *__restrict__ hyp, JointLds &sh,
                                                    int tid, double *__restrict__ nu_out, double *__restrict__ S_out) {
    double *A = sh.A, *y = sh.y;
    const int m = a.m, cur = a.cur;
    constexpr int ld = kJointRows;

    for (int k = tid; k < m; k += kJointBlock) sh.lm[k] = hyp[k];
    for (int q = tid; q < 9; q += kJointBlock) sh.prr[q] = st.prr[cur][q];
    __syncthreads();
    int np = 0, dof = 0;                            // pairings, real rows: every lane counts them alike
    for (int k = 0; k < m; ++k)
        if (sh.lm[k] >= 0) { ++np; dof += (a.e[k].model == 1 || a.e[k].model == 4) ? 2 : 1; }
    const int n = 2 * np;

    // (1) per pairing
    for (int ks = tid; ks < m; ks += kJointBlock) {       // (on the device one trip at most, m <= kJointMax <= kJointBlock: the break below says so)
        int p = -1;
        if (sh.lm[ks] >= 0) {
            p = 0;
            for (int k = 0; k < ks; ++k) p += sh.lm[k] >= 0;
        }
        sh.pair_of[ks] = p;
        if (p >= 0) {
            const AssocModelEntry &e = a.e[ks];
            const int64_t i = sh.lm[ks];
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
            sh.posed[p] = ekfm::joint_pairing(e.model, e.z, e.R, p9, strip6, diag3, xr, l, hr, ht, S, nu) ? 1 : 0;
            sh.scan_of[p] = ks;
            for (int q = 0; q < 6; ++q) { sh.Hr[p][q] = hr[q]; sh.strips[p][q] = strip6[q]; }
            for (int q = 0; q < 4; ++q) sh.Ht[p][q] = ht[q];
            y[2 * p] = nu[0]; y[2 * p + 1] = nu[1];
            A[(2 * p) * ld + 2 * p] = S[0]; A[(2 * p) * ld + 2 * p + 1] = S[1];       // the block whole: S[1] is what the record reports
            A[(2 * p + 1) * ld + 2 * p] = S[2]; A[(2 * p + 1) * ld + 2 * p + 1] = S[3];
        }
        if (kJointBlock >= kJointMax) break;
    }
    __syncthreads();

    // (2) the off-diagonal blocks, a > b
    for (int idx = tid; idx < np * (np - 1) / 2; idx += kJointBlock) {
        int pa = 1;
        while (pa * (pa + 1) / 2 <= idx) ++pa;
        const int pb = idx - pa * (pa - 1) / 2;
        const int64_t ra = 2 * sh.lm[sh.scan_of[pa]], rb = 2 * sh.lm[sh.scan_of[pb]];
        double pab[4], Sab[4];
        for (int q = 0; q < 4; ++q) pab[q] = pmm_low_chain<TS>(st, a.pstart, a.npend, ra + (q >> 1), rb + (q & 1));
        ekfm::joint_cross_block(sh.Hr[pa], sh.Ht[pa], sh.Hr[pb], sh.Ht[pb], sh.prr, sh.strips[pa], sh.strips[pb], pab, Sab);
        for (int q = 0; q < 4; ++q) A[(2 * pa + (q >> 1)) * ld + 2 * pb + (q & 1)] = Sab[q];
    }
    __syncthreads();

    // (3) nu and S by scan index, before the factorisation overwrites them
    if (nu_out)
        for (int i = tid; i < 2 * m; i += kJointBlock) {
            const int p = sh.pair_of[i >> 1];
            nu_out[i] = p >= 0 ? y[2 * p + (i & 1)] : 0.0;
        }
    if (S_out)
        for (int e = tid; e < 4 * m * m; e += kJointBlock) {
            const int i = e % (2 * m), j = e / (2 * m);             // column-major
            const int pi = sh.pair_of[i >> 1], pj = sh.pair_of[j >> 1];
            double v = i == j ? 1.0 : 0.0;
            if (pi >= 0 && pj >= 0) {
                const int ri = 2 * pi + (i & 1), rj = 2 * pj + (j & 1);
                v = (ri >= rj || pi == pj) ? A[ri * ld + rj] : A[rj * ld + ri];
            }
            S_out[e] = v;
        }
    __syncthreads();

    // (4) the factorisation, up to the first pairing that has no d2
    int bad = np;                                   // the first irregular pairing; np: none
    for (int p = np - 1; p >= 0; --p)
        if (!sh.posed[p]) bad = p;
    for (int k = 0; k < 2 * bad; ++k) {
        double lkk;
        if (!ekfm::joint_pivot(A[k * ld + k], lkk)) { bad = k >> 1; break; }       // every lane reads the same pivot: a uniform exit
        ekfm::joint_factor_scale(A, ld, y, n, k, lkk, tid, kJointBlock);
        __syncthreads();
        ekfm::joint_factor_update(A, ld, y, n, k, tid, kJointBlock);
        __syncthreads();
    }
    const JointCounts cnt = { np, dof, bad };
    return cnt;
}

// (5) by ONE lane: the prefixes (d2_prefix: this hypothesis's m entries, or nullptr), summed over y^2 in ascending row order, and the record
__device__ __forceinline__ JointRecord joint_record(const JointLds &sh, const JointCounts &cnt, int m, double *__restrict__ d2_prefix) {
    double acc = 0.0;
    for (int k = 0; k < m; ++k) {
        const int p = sh.pair_of[k];
        if (p >= 0) acc = p < cnt.bad ? ekfm::joint_prefix_add(acc, sh.y[2 * p], sh.y[2 * p + 1]) : NAN;
        if (d2_prefix) d2_prefix[k] = acc;
    }
    JointRecord r;
    r.d2 = acc; r.dof = cnt.dof; r.pairings = cnt.np;
    r.outcome = cnt.bad < cnt.np ? 0 : 1;
    r.first_irregular = cnt.bad < cnt.np ? sh.scan_of[cnt.bad] : -1;
    return r;
}

template <typename TS>
__global__ __launch_bounds__(kJointBlock) void k_joint_innovation(DevState st, JointArgs a, const int64_t *__restrict__ hyp,
                                                                  JointRecord *__restrict__ out, double *__restrict__ d2_prefix,
                                                                  double *__restrict__ nu_out, double *__restrict__ S_out) {
    __shared__ JointLds sh;
    const int tid = threadIdx.x;
    const int m = a.m;
    const int64_t hi = blockIdx.x;
    const JointCounts cnt = joint_phases<TS>(st, a, hyp + hi * m, sh, tid, nu_out ? nu_out + hi * 2 * m : nullptr,
                                             S_out ? S_out + hi * 4 * m * m : nullptr);
    if (tid == 0) out[hi] = joint_record(sh, cnt, m, d2_prefix ? d2_prefix + hi * m : nullptr);
}
