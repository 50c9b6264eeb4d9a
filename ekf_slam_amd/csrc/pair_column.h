// Fragment of kernels.hip (included there, inside its anonymous namespace, after tile_access.h / lane_ops.h): what every kernel that
// produces a rank-2 pair (K, G) does per landmark-block column once G(:, c) is known.  k_gather_constrain (constrain.h) is built from
// it; gather_step_body (linear_obs.h: k_gather_linear, and model_obs.h's k_gather_model) takes the small part's solve, the record and the
// robot part; the branch of k_gather that corrects nothing (gather.h: gather_decided_other) the zero pair slot and the diagonal-block copy.
// Compiles for the host too (behind tests/support/kernel_host_shim.h): DevState, double2, ring_slot, rank2_apply, lane_xor1 and
// ekfm:: functions only.
//
// TWINS.  Steps (4), (4b) of k_gather (gather.h) and the column steps of k_gather_linear hold the same steps as text of their own:
// (4b) alone as a function costs k_gather<.., predict, dev> a VGPR (216 -> 217), and k_gather_linear lost 0.1-0.4 us of its 8-17 when it
// called load_column_operands / finish_pair_column.  A change to a rule below is made there as well.  The robot block's rule is ONE
// text: robot_block_entry, which k_gather's helper wavefronts and its kDev epilogue call too (no register, no byte).
#pragma once

// ---------------------------------------------------------------------------------------------------
// the column's operands: strip(0..2, c), x(c) and its entries of the landmark's live 2x2 diagonal block (DevState::diag: even columns
// hold (2k, 2k) in dgc; odd ones (2k+1, 2k) in dgl and (2k+1, 2k+1) in dgc)
// ---------------------------------------------------------------------------------------------------
struct ColumnOperands { double s0, s1, s2, xc, dgc, dgl; };

// One buffer of a double-buffered pair of DevState.  Both pointers arrive with the first kernel-argument fetch and are SELECTED: indexing
// the by-value struct with a run-time index makes the compiler fetch the pointer with a second, dependent scalar load, which in the
// middle of a kernel stands in front of everything its first wavefront does next (k_gather's rule; measured on k_gather_linear: 0.3 us
// of 8-17 for the two pointers of load_column_operands).
__device__ __forceinline__ double *buffer_of(double *const (&pair)[2], int i) { return i ? pair[1] : pair[0]; }

__device__ __forceinline__ void load_diag_column(const DevState &st, int64_t c, double &dgc, double &dgl) {
    const double *__restrict__ dg = buffer_of(st.diag, st.dcur) + 3 * (c >> 1);
    if (c & 1) { dgl = dg[1]; dgc = dg[2]; } else dgc = dg[0];
}
__device__ __forceinline__ void store_diag_column(double *diag_nxt, int64_t c, double dgc, double dgl) {      // diag_nxt: st.diag[st.dcur ^ 1]
    double *__restrict__ dn = diag_nxt + 3 * (c >> 1);
    if (c & 1) { dn[1] = dgl; dn[2] = dgc; } else dn[0] = dgc;
}
// column c of state buffer `cur` / diagonal buffer st.dcur; zeros for a lane without a column
__device__ __forceinline__ ColumnOperands load_column_operands(const DevState &st, int cur, int64_t c, bool live) {
    ColumnOperands o = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    if (live) {
        const double *__restrict__ strip = buffer_of(st.strip, cur);
        o.s0 = strip[c]; o.s1 = strip[st.ldm + c]; o.s2 = strip[2 * st.ldm + c];
        o.xc = buffer_of(st.x, cur)[3 + c];
        load_diag_column(st, c, o.dgc, o.dgl);
    }
    return o;
}

// ---------------------------------------------------------------------------------------------------
// the small part of a launch, formed once per workgroup and read by its column lanes
// ---------------------------------------------------------------------------------------------------
struct PairSolve {
    double Si[4];          // S^-1, row-major
    double nu[2];
    double Gr[2][3];       // G over the robot columns
    double Kr[3][2];
    double prr[9];         // Prr before the update
    int ok;                // 0: the launch does not apply (S irregular, d2 beyond a gate) and everything above but prr is zero
};

// S^-1, K_r and the rest of `sol` from S, nu, the two rows of G_r and Prr.  A launch that does not apply gets zeros: every column then
// writes a zero pair and copies the state, and nothing that is not finite reaches memory.
__device__ __forceinline__ void pair_solve(PairSolve &sol, const double S[4], double nu0, double nu1, const double *Gr0, const double *Gr1,
                                           const double *prr, bool ok) {
    ekfm::inv2(S, sol.Si);
    sol.nu[0] = nu0;
    sol.nu[1] = nu1;
    for (int t = 0; t < 3; ++t) { sol.Gr[0][t] = Gr0[t]; sol.Gr[1][t] = Gr1[t]; }
    for (int t = 0; t < 3; ++t)
        for (int cc = 0; cc < 2; ++cc) sol.Kr[t][cc] = sol.Gr[0][t] * sol.Si[cc] + sol.Gr[1][t] * sol.Si[2 + cc];
    if (!ok) {
        sol.nu[0] = sol.nu[1] = 0.0;
        for (int q = 0; q < 4; ++q) sol.Si[q] = 0.0;
        for (int q = 0; q < 6; ++q) { (&sol.Gr[0][0])[q] = 0.0; (&sol.Kr[0][0])[q] = 0.0; }
    }
    for (int q = 0; q < 9; ++q) sol.prr[q] = prr[q];
    sol.ok = ok ? 1 : 0;
}

// the record of a launch (kernels.h: kConstrainRecordDoubles, kLinearRecordDoubles): S row-major (0..3) | nu (4, 5) | d2 (6) | the
// outcome (7)
__device__ __forceinline__ void store_pair_record(double *rec, const double S[4], double nu0, double nu1, double d2, double outcome) {
    for (int q = 0; q < 4; ++q) rec[q] = S[q];
    rec[4] = nu0; rec[5] = nu1; rec[6] = d2; rec[7] = outcome;
}

// ---------------------------------------------------------------------------------------------------
// the column's share of the pair and of the state
// ---------------------------------------------------------------------------------------------------
// Where a launch's results go: ring position npend (counted from slot pstart) of the pair rings -- the F64 pair and, where the handle
// keeps them (st.Gp32: the F32-arithmetic pass reads them), the planar float copies -- and the state buffers that are not `cur`.
// Resolved ONCE per lane, straight behind the small part's barrier and in front of the lane's G: each field is a scalar load from the
// argument block, and met one by one inside the branches below they queue up on the launch's critical path (measured on
// k_gather_linear: 0.3-0.4 us of 8-17).
struct PairDest {
    double2 *G, *K;
    float *G32, *K32;
    double *x, *strip, *diag;
    int64_t ldm, n_mm, pad_end;
};
__device__ __forceinline__ PairDest pair_dest(const DevState &st, int cur, int pstart, int npend, int64_t n_mm) {
    const int64_t out_off = (int64_t)ring_slot(pstart, npend, st.pcap) * st.pair_stride;
    PairDest d;
    d.G = reinterpret_cast<double2 *>(st.Gp + out_off);
    d.K = reinterpret_cast<double2 *>(st.Kp + out_off);
    d.G32 = st.Gp32 ? st.Gp32 + out_off : nullptr;
    d.K32 = st.Gp32 ? st.Kp32 + out_off : nullptr;
    d.x = buffer_of(st.x, cur ^ 1); d.strip = buffer_of(st.strip, cur ^ 1); d.diag = buffer_of(st.diag, st.dcur ^ 1);
    d.ldm = st.ldm; d.n_mm = n_mm; d.pad_end = st.tm.padded(n_mm);
    return d;
}

// Column c of the pair: F64, and the float copies planar with K negated.  Called with zeros over the padded tail, which the pass reads
// as whole tile-wide slices: 0.0f / -0.0f there.  (k_gather's twin: its step (4).)
__device__ __forceinline__ void store_pair_column(const PairDest &d, int64_t c, double g0, double g1, double k0, double k1) {
    d.G[c] = make_double2(g0, g1);
    d.K[c] = make_double2(k0, k1);
    if (d.G32) {
        d.G32[c] = (float)g0; d.G32[d.ldm + c] = (float)g1;
        d.K32[c] = -(float)k0; d.K32[d.ldm + c] = -(float)k1;
    }
}

// Everything after G(:, c) = (g0, g1) (zeros where the lane has no column or the launch does not apply): K(c, :) = G(:, c)' S^-1, the
// pair into its slot, x'(c) = x(c) + K nu, strip'(:, c) = strip(:, c) - K_r G(:, c), and the pair applied to the landmark's live 2x2
// block -- the live copies never carry a pending pair.  Called by every lane of the workgroup (lane_xor1: odd columns take the partner
// column's G for their (2k+1, 2k)).  (k_gather's twin: its steps (4) and (4b).)
__device__ __forceinline__ void finish_pair_column(const PairDest &d, const PairSolve &sol, const ColumnOperands &o, int64_t c, double g0, double g1) {
    const bool live = c < d.n_mm;
    double k0 = 0.0, k1 = 0.0;
    if (live) {
        k0 = g0 * sol.Si[0] + g1 * sol.Si[2];
        k1 = g0 * sol.Si[1] + g1 * sol.Si[3];
        store_pair_column(d, c, g0, g1, k0, k1);
        d.x[3 + c] = o.xc + (k0 * sol.nu[0] + k1 * sol.nu[1]);
        d.strip[c] = o.s0 - (sol.Kr[0][0] * g0 + sol.Kr[0][1] * g1);
        d.strip[d.ldm + c] = o.s1 - (sol.Kr[1][0] * g0 + sol.Kr[1][1] * g1);
        d.strip[2 * d.ldm + c] = o.s2 - (sol.Kr[2][0] * g0 + sol.Kr[2][1] * g1);
    } else if (c < d.pad_end) store_pair_column(d, c, 0.0, 0.0, 0.0, 0.0);
    const double2 kn = make_double2(k0, k1), gn = make_double2(g0, g1);
    const double2 gl = make_double2(lane_xor1(gn.x), lane_xor1(gn.y));       // the partner column's G (odd lanes: G(:, 2k))
    const double ndc = rank2_apply(o.dgc, kn, gn), ndl = rank2_apply(o.dgl, kn, gl);
    if (live) store_diag_column(d.diag, c, ndc, ndl);
}

// Prr'(r, b) = Prr(r, b) - K_r(r, :) G_r(:, b), kept EXACTLY symmetric: entry (r, b) and its mirror both take the lower-triangle entry's value.  Evaluated entry by entry,
// K_r(r,:) G_r(:,b) and K_r(b,:) G_r(:,r) differ in the last bit; with the strip stored once (symmetry enforced there) the antisymmetric
// part this leaves in the 3x3 block is not damped but AMPLIFIED by the corrections that follow -- measured: 2e-15 after 250 SLAM
// iterations, 1.3e-7 after 3 000, the heading drifting from the dense restatement with it (scripts/soak_config2.py), where the
// reference's dense P stays symmetric to 1e-16.  (Also called by k_gather: its helper wavefronts' tail, and the Prr' its kDev epilogue forms.)
template <typename Sol>
__device__ __forceinline__ double robot_block_entry(const double *prr, const Sol &sol, int r, int b) {
    const int rr = r > b ? r : b, bb = r > b ? b : r;
    return prr[3 * rr + bb] - (sol.Kr[rr][0] * sol.Gr[0][bb] + sol.Kr[rr][1] * sol.Gr[1][bb]);
}
// Workgroup 0 (tid: the lane's index in it): x_r' = x_r + K_r nu and Prr' = Prr - K_r G_r.
__device__ __forceinline__ void store_robot_part(const DevState &st, int cur, const PairDest &d, const PairSolve &sol, int tid) {
    if (tid < 3) d.x[tid] = buffer_of(st.x, cur)[tid] + (sol.Kr[tid][0] * sol.nu[0] + sol.Kr[tid][1] * sol.nu[1]);
    if (tid >= 64 && tid < 73) {
        const int q = tid - 64, r = q / 3, b = q - 3 * r;
        buffer_of(st.prr, cur ^ 1)[3 * r + b] = robot_block_entry(sol.prr, sol, r, b);
    }
}
