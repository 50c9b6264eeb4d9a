// Fragment of kernels.hip (included there, inside its anonymous namespace, after pair_column.h / gather.h): the rank-2 pair of a
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


// ---------------------------------------------------------------------------------------------------
// Pending pairs.  Constraint number a.npend of a batch (ekf_merge_landmarks_batch) runs while the a.npend earlier pairs of the batch are
// still PENDING in the ring st.Gp / st.Kp (the batch's private F64 ring, handed over in a by-value copy of DevState: slots a.pstart + l,
// no float copies) -- the tiles still hold the P the batch started from.  Every tile operand is read PATCHED: base entry minus
// sum_l K_l G_l, rank2_apply in slot order on the canonical entry (r >= c: K_l(r,:) . G_l(:,c)), which is the chain the one-pair passes
// of a constraint-by-constraint run would have applied -- with F64 tiles the same bits, with float tiles the unrounded values.
// x, the strip, Prr and the live diagonal blocks carry every earlier pair already (each launch writes them whole) and are read as they are.
// A single constraint (ekf_constrain_landmarks / ekf_merge_landmarks) is the case a.npend == 0: the host flushes first, the loops below
// are zero-trip and the tiles hold the live P.
// ---------------------------------------------------------------------------------------------------
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

// One lane per landmark-block column c; 256 columns per workgroup.  Reads state buffer a.cur / diagonal buffer st.dcur, writes the other
// ones whole; the small part is formed by one lane of EVERY workgroup (no workgroup reads what another one of the launch writes).
// Everything after G(:, c) is pair_column.h's.  rec (device, kConstrainRecordDoubles doubles, written by workgroup 0; nullptr: no record):
// S row-major, nu, d2, 1.0 = S regular, 0.0 = not.  An S that is not regular (ekfm::constrain_d2) makes the launch a no-op that stays
// finite: a zero pair in its slot, x / strip / Prr / the diagonal blocks copied -- a batch's host reads the record afterwards and puts
// its snapshot back; a single constraint's host has refused such an S before it launches.
template <typename TS>
__global__ __launch_bounds__(kBlock) void k_gather_constrain(DevState st, ConstrainArgs a, double *__restrict__ rec) {
    __shared__ PairSolve sol;
    const int tid = threadIdx.x;
    const int cur = a.cur;
    const int64_t ai = a.ai, aj = a.aj;
    const int64_t c = (int64_t)blockIdx.x * kBlock + tid;
    const bool live = c < a.n_mm;

    // (1) the column's loads and patches, requested before the small part is waited for
    double mi0 = 0.0, mi1 = 0.0, mj0 = 0.0, mj1 = 0.0;
    if (live) {
        constrain_row_pair_chain<TS>(st, a.pstart, a.npend, ai, c, mi0, mi1);
        constrain_row_pair_chain<TS>(st, a.pstart, a.npend, aj, c, mj0, mj1);
    }
    const ColumnOperands o = load_column_operands(st, cur, c, live);

    // (2) the small part, once per workgroup: the cross block comes from the tiles and needs the chain, the own blocks are live
    if (tid == 0) {
        const double *__restrict__ strip = st.strip[cur];
        double sm[kConstrainSmall];
#pragma unroll
        for (int e = 0; e < kConstrainSmall; ++e)
            sm[e] = (e >= 6 && e < 10) ? pmm_low_chain<TS>(st, a.pstart, a.npend, ai + ((e - 6) >> 1), aj + ((e - 6) & 1))
                                       : constrain_small_entry<TS>(st, cur, ai, aj, e);
        const double R[4] = { a.R00, a.R01, a.R10, a.R11 };
        double S[4], d2, Gr[2][3];
        ekfm::constrain_S(sm, sm + 3, sm + 6, R, S);
        const double nu0 = a.d0 - (sm[10] - sm[12]), nu1 = a.d1 - (sm[11] - sm[13]);
        const bool ok = ekfm::constrain_d2(S, nu0, nu1, d2);
        if (rec && blockIdx.x == 0) store_pair_record(rec, S, nu0, nu1, d2, ok ? 1.0 : 0.0);
        for (int r = 0; r < 2; ++r)
            for (int t = 0; t < 3; ++t) Gr[r][t] = strip[t * st.ldm + ai + r] - strip[t * st.ldm + aj + r];
        pair_solve(sol, S, nu0, nu1, Gr[0], Gr[1], st.prr[cur], ok);
    }
    __syncthreads();

    // (3) G(:, c) = P(rows of l_i, c) - P(rows of l_j, c), and the column's share of K, x, the strip and the diagonal blocks
    const PairDest d = pair_dest(st, cur, a.pstart, a.npend, a.n_mm);
    double g0 = 0.0, g1 = 0.0;
    if (live && sol.ok) { g0 = mi0 - mj0; g1 = mi1 - mj1; }
    finish_pair_column(d, sol, o, c, g0, g1);
    // (4) workgroup 0: x_r and Prr'
    if (blockIdx.x == 0) store_robot_part(st, cur, d, sol, tid);
}
