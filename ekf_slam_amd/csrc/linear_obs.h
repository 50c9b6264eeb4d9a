// Fragment of kernels.hip (included there, inside its anonymous namespace, after constrain.h): the rank-2 pair of a LINEAR observation
// with a constant Jacobian (ekf_observe_linear / ekf_linear_innovation): k_gather_linear, k_linear_probe.
#pragma once

// ---------------------------------------------------------------------------------------------------
// "H x was observed as z, with noise covariance R", H = [Hr (2x3, robot) .. Hl_0 (2x2, columns a_0) .. Hl_1 (2x2, columns a_1) ..]:
//     G = H P      S = G H' + R      nu = z - H x (rows wrapped where asked)      K = G' S^-1      x += K nu      P -= K G
// -- the update of constrain.h for a general H (there: Hr = 0, Hl = +I2, -I2).  Unlike a constraint this is an UPDATE-STEP: the
// launch runs on the handle's own ring while the a.npend earlier pairs are still pending, reads every tile operand patched with
// them (constrain_row_pair_chain, pmm_low_chain) and leaves its pair in the next slot, float copies included, as k_gather does.
// ONE BODY, two kernels.  step_small_part and gather_step_body are templates over the argument block and the workgroup's solve; what
// differs between a step with a constant H and one through a model (model_obs.h) is two overloads found by their argument types:
//     small_solve(a, sm, sol)   lane 0's work on the loaded operands: S, nu, the outcome, the record, the solve (a model: h(x) and H first)
//     step_H(a, sol)            where the column lanes read H: the argument block, or the LDS copy a model's lane 0 left
//     step_counted(a, sol)      whether a launch that did not apply is counted: always, but for model_assigned.h's skipped step
// Both kernels compile to the code they had as two texts (profiles/observe_step/README.md), and to the same code with the third
// overload in the body (profiles/observe_assigned/README.md).
// The small part's solve, the record and workgroup 0's robot part are pair_column.h's.  The column's own share (steps (1), (3), (3b)) is
// the twin of its load_column_operands / finish_pair_column, kept as text of its own: called from here those two cost k_gather_linear
// 0.1-0.4 us of its 8-17 (measured against the parent commit, profiles/pair_column/README.md), although they are the same statements.
// x, the strip, Prr and the live diagonal blocks carry every pending pair already and are read as they are.
// ---------------------------------------------------------------------------------------------------
// the record of a launch (kernels.h: kLinearRecordDoubles): S row-major (0..3) | nu (4, 5) | d2 (6) | the outcome (7): 1.0 applied, 0.0 S
// irregular, 2.0 gated

// operand e of ekfm::linear_small (device_math.h names the layout); the cross block comes from the tiles and needs the chain
// (A: LinearArgs, or model_obs.h's ModelArgs -- its fields a, cur, pstart and npend)
template <typename TS, typename A>
__device__ __forceinline__ double linear_small_entry(const DevState &st, const A &a, int e) {
    const int cur = a.cur;
    const int64_t a0 = a.a[0], a1 = a.a[1];
    if (e < 9) return st.prr[cur][e];
    if (e < 21) {
        const int q = e - 9, b = q / 6, t = (q - 6 * b) >> 1, r = q & 1;
        const int64_t ab = b ? a1 : a0;
        return ab >= 0 ? st.strip[cur][t * st.ldm + ab + r] : 0.0;
    }
    if (e < 27) {
        const int q = e - 21, b = q / 3;
        const int64_t ab = b ? a1 : a0;
        return ab >= 0 ? st.diag[st.dcur][3 * (ab >> 1) + (q - 3 * b)] : 0.0;
    }
    if (e < 31) return (a0 >= 0 && a1 >= 0) ? pmm_low_chain<TS>(st, a.pstart, a.npend, a0 + ((e - 27) >> 1), a1 + ((e - 27) & 1)) : 0.0;
    if (e < 34) return st.x[cur][e - 31];
    const int64_t ab = ((e - 34) >> 1) ? a1 : a0;
    return ab >= 0 ? st.x[cur][3 + ab + ((e - 34) & 1)] : 0.0;
}

struct LinearSolve : PairSolve {
    double rec[kLinearRecordDoubles];
};

// Lane 0's share of the small part: S, nu, d2, the decision, S^-1, Gr and Kr from the operands in sm.  A launch that does not apply (S
// irregular, d2 beyond the gate) gets zeros for S^-1, nu, Gr and Kr: every column then writes a zero pair and copies the state.
__device__ __forceinline__ void small_solve(const LinearArgs &a, double *sm, LinearSolve &sol) {
    double Gs[14], S[4], nu[2], d2;
    ekfm::linear_small(sm, a.H, a.z, a.R, a.wrap, Gs, S, nu);
    const int outcome = ekfm::linear_outcome(S, nu, a.gate, d2);
    store_pair_record(sol.rec, S, nu[0], nu[1], d2, (double)outcome);
    pair_solve(sol, S, nu[0], nu[1], Gs, Gs + 7, sm, outcome == 1);
}
__device__ __forceinline__ const double *step_H(const LinearArgs &a, const LinearSolve &) { return a.H; }
// whether a launch that did not apply goes into one of the two counters: every step's does, but for a step that was never meant to
// apply (model_assigned.h's overload: an observation its scan's assignment left out)
template <typename A, typename Solve>
__device__ __forceinline__ bool step_counted(const A &, const Solve &) { return true; }

// The small part, by the first wavefront of a workgroup: the kLinearSmall operands one per lane (each patched entry walks the ring
// once, on a lane of its own), then lane 0's small_solve.  Called by every lane of the workgroup; ends with a barrier.
template <typename TS, typename A, typename Solve>
__device__ __forceinline__ void step_small_part(const DevState &st, const A &a, double *sm, Solve &sol) {
    const int tid = threadIdx.x;
    if (tid < ekfm::kLinearSmall) sm[tid] = linear_small_entry<TS>(st, a, tid);
    __syncthreads();
    if (tid == 0) small_solve(a, sm, sol);
    __syncthreads();
}

// ekf_linear_innovation: the small part alone, and nothing written but the record
template <typename TS>
__global__ __launch_bounds__(64) void k_linear_probe(DevState st, LinearArgs a, double *__restrict__ rec) {
    __shared__ double sm[ekfm::kLinearSmall];
    __shared__ LinearSolve sol;
    step_small_part<TS>(st, a, sm, sol);
    if (threadIdx.x < kLinearRecordDoubles) rec[threadIdx.x] = sol.rec[threadIdx.x];
}

// One lane per landmark-block column c; 256 columns per workgroup (k_gather_constrain's shape).  Reads state buffer a.cur / diagonal
// buffer st.dcur, writes the other ones whole; the small part is formed by EVERY workgroup (no workgroup reads what another one of
// the launch writes).  rec: kLinearRecordDoubles doubles, cnt: the two counters of launches that did not apply (irregular, gated) --
// both written by workgroup 0 (launches on one stream are ordered: a plain load, add and store).
template <typename TS, typename A, typename Solve>
__device__ __forceinline__ void gather_step_body(const DevState &st, const A &a, double *sm, Solve &sol, double *__restrict__ rec, int64_t *__restrict__ cnt) {
    const int tid = threadIdx.x;
    const int cur = a.cur;
    const double *__restrict__ x = st.x[cur];
    const double *__restrict__ strip = st.strip[cur];
    double *__restrict__ x_nxt = st.x[cur ^ 1];
    double *__restrict__ strip_nxt = st.strip[cur ^ 1];
    const int64_t ldm = st.ldm;
    const int64_t c = (int64_t)blockIdx.x * kBlock + tid;
    const bool live = c < a.n_mm;

    // (1) the column's loads and patches; a landmark that carries no block is skipped by the whole launch
    double m[2][2] = { { 0.0, 0.0 }, { 0.0, 0.0 } }, s0 = 0.0, s1 = 0.0, s2 = 0.0, xc = 0.0, dgc = 0.0, dgl = 0.0;
    if (live) {
        if (a.a[0] >= 0) constrain_row_pair_chain<TS>(st, a.pstart, a.npend, a.a[0], c, m[0][0], m[0][1]);
        if (a.a[1] >= 0) constrain_row_pair_chain<TS>(st, a.pstart, a.npend, a.a[1], c, m[1][0], m[1][1]);
        s0 = strip[c]; s1 = strip[ldm + c]; s2 = strip[2 * ldm + c];
        xc = x[3 + c];
        const double *__restrict__ dg = st.diag[st.dcur] + 3 * (c >> 1);
        if (c & 1) { dgl = dg[1]; dgc = dg[2]; } else dgc = dg[0];
    }

    // (2) the small part, once per workgroup (a model: and H)
    step_small_part<TS>(st, a, sm, sol);
    const bool ok = sol.ok != 0;
    const double *H = step_H(a, sol);

    // (3) the column's share of G, K, x and the strip (the twin of pair_column.h's finish_pair_column / store_pair_column)
    const int64_t pad_end = st.tm.padded(a.n_mm);
    const int64_t out_off = (int64_t)ring_slot(a.pstart, a.npend, st.pcap) * st.pair_stride;
    double2 *__restrict__ Gout = reinterpret_cast<double2 *>(st.Gp + out_off);
    double2 *__restrict__ Kout = reinterpret_cast<double2 *>(st.Kp + out_off);
    double g0 = 0.0, g1 = 0.0, k0 = 0.0, k1 = 0.0;
    if (live) {
        if (ok) {
            // G(:, c) = Hr strip(:, c) + sum_b Hl_b P(rows of l_b, c), in this order
            g0 = (H[0] * s0 + H[1] * s1) + H[2] * s2;
            g1 = (H[7] * s0 + H[8] * s1) + H[9] * s2;
            if (a.a[0] >= 0) { g0 += H[3] * m[0][0] + H[4] * m[0][1]; g1 += H[10] * m[0][0] + H[11] * m[0][1]; }
            if (a.a[1] >= 0) { g0 += H[5] * m[1][0] + H[6] * m[1][1]; g1 += H[12] * m[1][0] + H[13] * m[1][1]; }
            k0 = g0 * sol.Si[0] + g1 * sol.Si[2];
            k1 = g0 * sol.Si[1] + g1 * sol.Si[3];
        }
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
    // (4) workgroup 0: x_r and Prr', the record and the counters
    if (blockIdx.x == 0) {
        store_robot_part(st, cur, pair_dest(st, cur, a.pstart, a.npend, a.n_mm), sol, tid);
        if (tid >= 128 && tid < 128 + kLinearRecordDoubles) rec[tid - 128] = sol.rec[tid - 128];
        if (tid == 0 && !ok && step_counted(a, sol)) {
            const int which = sol.rec[7] == 0.0 ? 0 : 1;
            cnt[which] = cnt[which] + 1;
        }
    }
}

// the step with H in the argument block (model_obs.h: k_gather_model, the same body with H formed on the device)
template <typename TS>
__global__ __launch_bounds__(kBlock) void k_gather_linear(DevState st, LinearArgs a, double *__restrict__ rec, int64_t *__restrict__ cnt) {
    __shared__ double sm[ekfm::kLinearSmall];
    __shared__ LinearSolve sol;
    gather_step_body<TS>(st, a, sm, sol, rec, cnt);
}
