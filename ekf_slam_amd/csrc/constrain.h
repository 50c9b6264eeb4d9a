// Fragment of kernels.hip (included there, inside its anonymous namespace, after tile_access.h / gather.h): the rank-2 pair of a
// constraint BETWEEN TWO LANDMARKS (ekf_constrain_landmarks / ekf_merge_landmarks / ekf_landmark_distance): k_constrain_probe,
// k_gather_constrain.
#pragma once

// ---------------------------------------------------------------------------------------------------
// "l_i - l_j was observed as delta, with noise covariance R" has the constant Jacobian H = [.. +I2 (columns a_i) .. -I2 (columns a_j) ..],
// a_k = 2k in landmark-block numbering.  The model is linear, so the Kalman update is exact and has no angles:
//     G = H P = P(a_i:a_i+1, :) - P(a_j:a_j+1, :)      S = G H' + R      nu = delta - (l_i - l_j)
//     K = G' S^-1      x += K nu      P -= K G          (the reference's P = (I - K H) P, EKF_SLAM.m:145, for this H)
// (K, G) is a pair like every correction's: it goes to the pending ring and a pass applies it to the tiles (rank2_apply).
//
// The small operands -- both landmarks' own 2x2 blocks (LIVE F64 copies, DevState::diag), their cross block (tiles), the four entries
// of x -- are 14 doubles.  k_constrain_probe copies them out for the host, which forms S and nu from them BEFORE anything changes
// (a singular S is refused; ekf_landmark_distance stops there); k_gather_constrain forms them again with the same function
// (ekfm::constrain_S, device_math.h), so both sides see the same bits.
// ---------------------------------------------------------------------------------------------------
constexpr int kConstrainSmall = 14;       // Pii (0,0) (1,0) (1,1) | Pjj likewise | Pij row-major: P(a_i + r, a_j + b) at 6 + 2r + b | l_i | l_j

template <typename TS>
__device__ __forceinline__ double constrain_small_entry(const DevState &st, int cur, int64_t ai, int64_t aj, int e) {
    if (e < 3) return st.diag[st.dcur][3 * (ai >> 1) + e];
    if (e < 6) return st.diag[st.dcur][3 * (aj >> 1) + (e - 3)];
    if (e < 10) return pmm_low<TS>((const TS *)st.tiles, st.tm, ai + ((e - 6) >> 1), aj + ((e - 6) & 1));
    if (e < 12) return st.x[cur][3 + ai + (e - 10)];
    return st.x[cur][3 + aj + (e - 12)];
}

template <typename TS>
__global__ __launch_bounds__(64) void k_constrain_probe(DevState st, int cur, int64_t ai, int64_t aj, double *__restrict__ out) {
    const int e = threadIdx.x;
    if (e < kConstrainSmall) out[e] = constrain_small_entry<TS>(st, cur, ai, aj, e);
}

// rows j, j+1 of the landmark block at column c as canonical lower-triangle entries: the row part left of the landmark, the column
// part right of it, the landmark's own columns from its live F64 block (with float tiles: the unrounded values, as in k_gather)
template <typename TS>
__device__ __forceinline__ void constrain_row_pair(const DevState &st, int64_t j, int64_t c, double &m0, double &m1) {
    const TS *__restrict__ tiles = (const TS *)st.tiles;
    if ((c >> 1) == (j >> 1)) {
        const double *__restrict__ d = st.diag[st.dcur] + 3 * (j >> 1);
        const int b = (int)(c & 1);
        m0 = d[b]; m1 = d[1 + b];                               // P(j, j+b), P(j+1, j+b)
    } else if (c < j) {                                         // one tile (j is even), rows T apart
        const int64_t m = st.tm.T - 1;
        const TS *__restrict__ tp = tiles + st.tm.tile_offset(j >> st.tm.shift, c >> st.tm.shift) + ((j & m) << st.tm.shift) + (c & m);
        m0 = (double)tp[0]; m1 = (double)tp[st.tm.T];
    } else pmm_low_pair<TS>(tiles, st.tm, c, j, m0, m1);
}

struct ConstrainSolve {
    double Si[4];          // S^-1, row-major
    double nu[2];
    double Gr[2][3];       // G over the robot columns
    double Kr[3][2];
    double prr[9];         // Prr before the update
};

// One lane per landmark-block column c; 256 columns per workgroup.  The ring is empty when this runs (the host flushes first), so
// the tiles hold the live P and nothing is patched.  Reads state buffer a.cur / diagonal buffer st.dcur, writes the other ones
// whole; the small part is formed by one lane of EVERY workgroup (no workgroup reads what another one of the launch writes).
template <typename TS>
__global__ __launch_bounds__(kBlock) void k_gather_constrain(DevState st, ConstrainArgs a) {
    __shared__ ConstrainSolve sol;
    const int tid = threadIdx.x;
    const int cur = a.cur;
    const double *__restrict__ x = st.x[cur];
    const double *__restrict__ strip = st.strip[cur];
    double *__restrict__ x_nxt = st.x[cur ^ 1];
    double *__restrict__ strip_nxt = st.strip[cur ^ 1];
    const int64_t ldm = st.ldm, ai = a.ai, aj = a.aj;
    const int64_t c = (int64_t)blockIdx.x * kBlock + tid;
    const bool live = c < a.n_mm;

    // (1) the column's loads, requested before the small part is waited for
    double mi0 = 0.0, mi1 = 0.0, mj0 = 0.0, mj1 = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0, xc = 0.0, dgc = 0.0, dgl = 0.0;
    if (live) {
        constrain_row_pair<TS>(st, ai, c, mi0, mi1);
        constrain_row_pair<TS>(st, aj, c, mj0, mj1);
        s0 = strip[c]; s1 = strip[ldm + c]; s2 = strip[2 * ldm + c];
        xc = x[3 + c];
        const double *__restrict__ dg = st.diag[st.dcur] + 3 * (c >> 1);
        if (c & 1) { dgl = dg[1]; dgc = dg[2]; } else dgc = dg[0];
    }

    // (2) the small part, once per workgroup
    if (tid == 0) {
        double sm[kConstrainSmall];
#pragma unroll
        for (int e = 0; e < kConstrainSmall; ++e) sm[e] = constrain_small_entry<TS>(st, cur, ai, aj, e);
        const double R[4] = { a.R00, a.R01, a.R10, a.R11 };
        double S[4];
        ekfm::constrain_S(sm, sm + 3, sm + 6, R, S);
        ekfm::inv2(S, sol.Si);
        sol.nu[0] = a.d0 - (sm[10] - sm[12]);
        sol.nu[1] = a.d1 - (sm[11] - sm[13]);
        for (int r = 0; r < 2; ++r)
            for (int t = 0; t < 3; ++t) sol.Gr[r][t] = strip[t * ldm + ai + r] - strip[t * ldm + aj + r];
        for (int t = 0; t < 3; ++t)
            for (int cc = 0; cc < 2; ++cc) sol.Kr[t][cc] = sol.Gr[0][t] * sol.Si[cc] + sol.Gr[1][t] * sol.Si[2 + cc];
        for (int q = 0; q < 9; ++q) sol.prr[q] = st.prr[cur][q];
    }
    __syncthreads();

    // (3) the column's share of G, K, x and the strip
    const int64_t pad_end = st.tm.padded(a.n_mm);
    const int64_t out_off = (int64_t)ring_slot(a.pstart, a.npend, st.pcap) * st.pair_stride;
    double2 *__restrict__ Gout = reinterpret_cast<double2 *>(st.Gp + out_off);
    double2 *__restrict__ Kout = reinterpret_cast<double2 *>(st.Kp + out_off);
    double g0 = 0.0, g1 = 0.0, k0 = 0.0, k1 = 0.0;
    if (live) {
        g0 = mi0 - mj0; g1 = mi1 - mj1;
        k0 = g0 * sol.Si[0] + g1 * sol.Si[2];
        k1 = g0 * sol.Si[1] + g1 * sol.Si[3];
        Gout[c] = make_double2(g0, g1);
        Kout[c] = make_double2(k0, k1);
        if (st.Gp32) {                                          // the float copies, as k_gather writes them (planar, K negated)
            st.Gp32[out_off + c] = (float)g0; st.Gp32[out_off + ldm + c] = (float)g1;
            st.Kp32[out_off + c] = -(float)k0; st.Kp32[out_off + ldm + c] = -(float)k1;
        }
        x_nxt[3 + c] = xc + (k0 * sol.nu[0] + k1 * sol.nu[1]);
        strip_nxt[c] = s0 - (sol.Kr[0][0] * g0 + sol.Kr[0][1] * g1);
        strip_nxt[ldm + c] = s1 - (sol.Kr[1][0] * g0 + sol.Kr[1][1] * g1);
        strip_nxt[2 * ldm + c] = s2 - (sol.Kr[2][0] * g0 + sol.Kr[2][1] * g1);
    } else if (c < pad_end) {                                   // zeros up to the padded width: the pass reads whole tile-wide slices
        Gout[c] = make_double2(0.0, 0.0);
        Kout[c] = make_double2(0.0, 0.0);
        if (st.Gp32) {
            st.Gp32[out_off + c] = 0.0f; st.Gp32[out_off + ldm + c] = 0.0f;
            st.Kp32[out_off + c] = -0.0f; st.Kp32[out_off + ldm + c] = -0.0f;
        }
    }
    // (3b) this pair on every landmark's own 2x2 block, as k_gather step (4b): the live copies never carry a pending pair
    {
        const double2 kn = make_double2(k0, k1), gn = make_double2(g0, g1);
        const double2 gl = make_double2(lane_xor1(gn.x), lane_xor1(gn.y));       // the partner column's G (odd lanes: G(:, 2k))
        const double ndc = rank2_apply(dgc, kn, gn), ndl = rank2_apply(dgl, kn, gl);
        if (live) {
            double *__restrict__ dn = st.diag[st.dcur ^ 1] + 3 * (c >> 1);
            if (c & 1) { dn[1] = ndl; dn[2] = ndc; } else dn[0] = ndc;
        }
    }
    // (4) workgroup 0: x_r and Prr' = Prr - K_r G_r, kept EXACTLY symmetric as k_gather keeps it (both mirrors take the
    //     lower-triangle entry's value; see the comment there)
    if (blockIdx.x == 0) {
        if (tid < 3) x_nxt[tid] = x[tid] + (sol.Kr[tid][0] * sol.nu[0] + sol.Kr[tid][1] * sol.nu[1]);
        if (tid >= 64 && tid < 73) {
            const int q = tid - 64, r = q / 3, b = q - 3 * r;
            const int rr = r > b ? r : b, bb = r > b ? b : r;
            st.prr[cur ^ 1][3 * r + b] = sol.prr[3 * rr + bb] - (sol.Kr[rr][0] * sol.Gr[0][bb] + sol.Kr[rr][1] * sol.Gr[1][bb]);
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// The CHAINED form (ekf_merge_landmarks_batch): constraint number a.npend of a batch runs while the a.npend earlier pairs of the batch
// are still PENDING in the ring st.Gp / st.Kp (the batch's private F64 ring, handed over in a by-value copy of DevState: slots
// a.pstart + l, no float copies) -- the tiles still hold the P the batch started from.  Every tile operand is read PATCHED: base entry
// minus sum_l K_l G_l, rank2_apply in slot order on the canonical entry (r >= c: K_l(r,:) . G_l(:,c)), which is the chain the one-pair
// passes of a constraint-by-constraint run would have applied -- with F64 tiles the same bits, with float tiles the unrounded values.
// x, the strip, Prr and the live diagonal blocks carry every earlier pair already (each launch writes them whole) and are read as they are.
// ---------------------------------------------------------------------------------------------------
// the record of a launch (kernels.h: kConstrainRecordDoubles): S row-major (0..3) | nu (4, 5) | d2 (6) | 1.0 = S regular, 0.0 = not (7)

// canonical entry (r, c) of the landmark block, r >= c, in different landmarks, with the npend pending pairs applied
template <typename TS>
__device__ __forceinline__ double pmm_low_chain(const DevState &st, int pstart, int npend, int64_t r, int64_t c) {
    if (r < c) { const int64_t t = r; r = c; c = t; }
    double v = pmm_low<TS>((const TS *)st.tiles, st.tm, r, c);
    for (int l = 0; l < npend; ++l) {
        const int64_t so = (int64_t)ring_slot(pstart, l, st.pcap) * st.pair_stride;
        v = rank2_apply(v, reinterpret_cast<const double2 *>(st.Kp + so)[r], reinterpret_cast<const double2 *>(st.Gp + so)[c]);
    }
    return v;
}

// constrain_row_pair with the pending pairs applied: left of the landmark K_l at the landmark's rows and G_l at the lane's column, right
// of it K_l at the lane's row and G_l at the landmark's columns (k_gather's rule); the own block is live and carries them already
template <typename TS>
__device__ __forceinline__ void constrain_row_pair_chain(const DevState &st, int pstart, int npend, int64_t j, int64_t c, double &m0, double &m1) {
    constrain_row_pair<TS>(st, j, c, m0, m1);
    if ((c >> 1) == (j >> 1)) return;
    const bool left = c < j;
    for (int l = 0; l < npend; ++l) {
        const int64_t so = (int64_t)ring_slot(pstart, l, st.pcap) * st.pair_stride;
        const double2 *__restrict__ G2 = reinterpret_cast<const double2 *>(st.Gp + so);
        const double2 *__restrict__ K2 = reinterpret_cast<const double2 *>(st.Kp + so);
        if (left) {
            const double2 g = G2[c];
            m0 = rank2_apply(m0, K2[j], g); m1 = rank2_apply(m1, K2[j + 1], g);
        } else {
            const double2 k = K2[c];
            m0 = rank2_apply(m0, k, G2[j]); m1 = rank2_apply(m1, k, G2[j + 1]);
        }
    }
}

// k_gather_constrain with a.npend earlier pairs pending, and a record of what it saw (rec: kConstrainRecordDoubles doubles, written by workgroup 0).
// An S that is not regular (ekfm::constrain_d2) makes the launch a no-op that stays finite: a zero pair in its slot, x / strip / Prr / the
// diagonal blocks copied -- the host reads the record afterwards and puts the batch's snapshot back.
template <typename TS>
__global__ __launch_bounds__(kBlock) void k_gather_constrain_chain(DevState st, ConstrainArgs a, double *__restrict__ rec) {
    __shared__ ConstrainSolve sol;
    __shared__ int regular;
    const int tid = threadIdx.x;
    const int cur = a.cur;
    const double *__restrict__ x = st.x[cur];
    const double *__restrict__ strip = st.strip[cur];
    double *__restrict__ x_nxt = st.x[cur ^ 1];
    double *__restrict__ strip_nxt = st.strip[cur ^ 1];
    const int64_t ldm = st.ldm, ai = a.ai, aj = a.aj;
    const int64_t c = (int64_t)blockIdx.x * kBlock + tid;
    const bool live = c < a.n_mm;

    // (1) the column's loads and patches
    double mi0 = 0.0, mi1 = 0.0, mj0 = 0.0, mj1 = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0, xc = 0.0, dgc = 0.0, dgl = 0.0;
    if (live) {
        constrain_row_pair_chain<TS>(st, a.pstart, a.npend, ai, c, mi0, mi1);
        constrain_row_pair_chain<TS>(st, a.pstart, a.npend, aj, c, mj0, mj1);
        s0 = strip[c]; s1 = strip[ldm + c]; s2 = strip[2 * ldm + c];
        xc = x[3 + c];
        const double *__restrict__ dg = st.diag[st.dcur] + 3 * (c >> 1);
        if (c & 1) { dgl = dg[1]; dgc = dg[2]; } else dgc = dg[0];
    }

    // (2) the small part, once per workgroup: the cross block comes from the tiles and needs the chain, the own blocks are live
    if (tid == 0) {
        double sm[kConstrainSmall];
#pragma unroll
        for (int e = 0; e < kConstrainSmall; ++e)
            sm[e] = (e >= 6 && e < 10) ? pmm_low_chain<TS>(st, a.pstart, a.npend, ai + ((e - 6) >> 1), aj + ((e - 6) & 1))
                                       : constrain_small_entry<TS>(st, cur, ai, aj, e);
        const double R[4] = { a.R00, a.R01, a.R10, a.R11 };
        double S[4], d2;
        ekfm::constrain_S(sm, sm + 3, sm + 6, R, S);
        const double nu0 = a.d0 - (sm[10] - sm[12]), nu1 = a.d1 - (sm[11] - sm[13]);
        const bool ok = ekfm::constrain_d2(S, nu0, nu1, d2);
        regular = ok ? 1 : 0;
        if (blockIdx.x == 0) {
            for (int q = 0; q < 4; ++q) rec[q] = S[q];
            rec[4] = nu0; rec[5] = nu1; rec[6] = d2; rec[7] = ok ? 1.0 : 0.0;
        }
        ekfm::inv2(S, sol.Si);
        sol.nu[0] = nu0;
        sol.nu[1] = nu1;
        for (int r = 0; r < 2; ++r)
            for (int t = 0; t < 3; ++t) sol.Gr[r][t] = strip[t * ldm + ai + r] - strip[t * ldm + aj + r];
        for (int t = 0; t < 3; ++t)
            for (int cc = 0; cc < 2; ++cc) sol.Kr[t][cc] = sol.Gr[0][t] * sol.Si[cc] + sol.Gr[1][t] * sol.Si[2 + cc];
        for (int q = 0; q < 9; ++q) sol.prr[q] = st.prr[cur][q];
        if (!ok) {
            sol.nu[0] = sol.nu[1] = 0.0;
            for (int q = 0; q < 4; ++q) sol.Si[q] = 0.0;
            for (int q = 0; q < 6; ++q) { (&sol.Gr[0][0])[q] = 0.0; (&sol.Kr[0][0])[q] = 0.0; }
        }
    }
    __syncthreads();
    const bool ok = regular != 0;

    // (3) the column's share of G, K, x and the strip
    const int64_t pad_end = st.tm.padded(a.n_mm);
    const int64_t out_off = (int64_t)ring_slot(a.pstart, a.npend, st.pcap) * st.pair_stride;
    double2 *__restrict__ Gout = reinterpret_cast<double2 *>(st.Gp + out_off);
    double2 *__restrict__ Kout = reinterpret_cast<double2 *>(st.Kp + out_off);
    double g0 = 0.0, g1 = 0.0, k0 = 0.0, k1 = 0.0;
    if (live) {
        if (ok) {
            g0 = mi0 - mj0; g1 = mi1 - mj1;
            k0 = g0 * sol.Si[0] + g1 * sol.Si[2];
            k1 = g0 * sol.Si[1] + g1 * sol.Si[3];
        }
        Gout[c] = make_double2(g0, g1);
        Kout[c] = make_double2(k0, k1);
        x_nxt[3 + c] = xc + (k0 * sol.nu[0] + k1 * sol.nu[1]);
        strip_nxt[c] = s0 - (sol.Kr[0][0] * g0 + sol.Kr[0][1] * g1);
        strip_nxt[ldm + c] = s1 - (sol.Kr[1][0] * g0 + sol.Kr[1][1] * g1);
        strip_nxt[2 * ldm + c] = s2 - (sol.Kr[2][0] * g0 + sol.Kr[2][1] * g1);
    } else if (c < pad_end) {
        Gout[c] = make_double2(0.0, 0.0);
        Kout[c] = make_double2(0.0, 0.0);
    }
    // (3b) this pair on every landmark's own 2x2 block
    {
        const double2 kn = make_double2(k0, k1), gn = make_double2(g0, g1);
        const double2 gl = make_double2(lane_xor1(gn.x), lane_xor1(gn.y));
        const double ndc = rank2_apply(dgc, kn, gn), ndl = rank2_apply(dgl, kn, gl);
        if (live) {
            double *__restrict__ dn = st.diag[st.dcur ^ 1] + 3 * (c >> 1);
            if (c & 1) { dn[1] = ndl; dn[2] = ndc; } else dn[0] = ndc;
        }
    }
    // (4) workgroup 0: x_r and Prr' = Prr - K_r G_r, mirrored from the lower triangle
    if (blockIdx.x == 0) {
        if (tid < 3) x_nxt[tid] = x[tid] + (sol.Kr[tid][0] * sol.nu[0] + sol.Kr[tid][1] * sol.nu[1]);
        if (tid >= 64 && tid < 73) {
            const int q = tid - 64, r = q / 3, b = q - 3 * r;
            const int rr = r > b ? r : b, bb = r > b ? b : r;
            st.prr[cur ^ 1][3 * r + b] = sol.prr[3 * rr + bb] - (sol.Kr[rr][0] * sol.Gr[0][bb] + sol.Kr[rr][1] * sol.Gr[1][bb]);
        }
    }
}
