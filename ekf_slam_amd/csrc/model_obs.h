// Fragment of kernels.hip (included there, inside its anonymous namespace, after linear_obs.h): the rank-2 pair of an observation through
// one of the MODELS of ekf_observe_model / ekf_model_innovation (range and bearing, range, bearing, relative position, landmark range):
// k_gather_model, k_model_probe.
#pragma once

// ---------------------------------------------------------------------------------------------------
// "h(x) was observed as z, with noise covariance R", linearised at the live x:
//     H = dh/dx at x      G = H P      S = G H' + R      nu = z - h(x) (angles wrapped)      K = G' S^-1      x += K nu      P -= K G
// -- the update-step of linear_obs.h with one difference: H is no kernel argument.  x carries every pending pair and the host does not
// have it without a wait, so lane 0 of every workgroup evaluates ekfm::model_eval on the seven entries of x the small part has loaded
// anyway and leaves H in the workgroup's LDS beside S^-1, K_r and nu; the column lanes read it from there, all from one address (a
// broadcast).  Everything else -- the operands one per lane through linear_small_entry, the outcome, the record, the solve, the column
// steps (1), (3), (3b), (4) -- is linear_obs.h's, statement by statement and in its order of operations, kept as a named twin:
// k_gather_linear's registers are pinned, and with the H this kernel forms handed to it as an argument it writes the
// same P bit for bit (tests/test_model_obs_gpu.py).
// A target on the robot (q = 0) or a non-finite q has no Jacobian: H = 0, and the launch is reported and counted as an irregular S.
// ---------------------------------------------------------------------------------------------------

struct ModelSolve : LinearSolve {
    double H[14];
};

// linear_small_part for a model.  Called by every lane of the workgroup; ends with a barrier.
template <typename TS>
__device__ __forceinline__ void model_small_part(const DevState &st, const ModelArgs &a, double *sm, ModelSolve &sol) {
    const int tid = threadIdx.x;
    if (tid < ekfm::kLinearSmall) sm[tid] = linear_small_entry<TS>(st, a, tid);
    __syncthreads();
    if (tid == 0) {
        double H[14], hx[2], Gs[14], S[4], nu[2], d2;
        int wrap[2];
        const bool posed = ekfm::model_eval(a.model, sm + 31, a.anchor, a.a[0] >= 0, hx, H);
        ekfm::model_wrap(a.model, wrap);
        ekfm::model_small(sm, H, hx, a.z, a.R, wrap, Gs, S, nu);
        int outcome = ekfm::linear_outcome(S, nu, a.gate, d2);
        if (!posed) { outcome = 0; d2 = NAN; }
        store_pair_record(sol.rec, S, nu[0], nu[1], d2, (double)outcome);
        pair_solve(sol, S, nu[0], nu[1], Gs, Gs + 7, sm, outcome == 1);
        for (int q = 0; q < 14; ++q) sol.H[q] = H[q];
    }
    __syncthreads();
}

// ekf_model_innovation: the small part alone, and nothing written but the record
template <typename TS>
__global__ __launch_bounds__(64) void k_model_probe(DevState st, ModelArgs a, double *__restrict__ rec) {
    __shared__ double sm[ekfm::kLinearSmall];
    __shared__ ModelSolve sol;
    model_small_part<TS>(st, a, sm, sol);
    if (threadIdx.x < kLinearRecordDoubles) rec[threadIdx.x] = sol.rec[threadIdx.x];
}

// k_gather_linear's shape, arguments and outputs (one lane per landmark-block column, 256 per workgroup, the small part by EVERY
// workgroup); rec and cnt are the handle's linear record and counters.
template <typename TS>
__global__ __launch_bounds__(kBlock) void k_gather_model(DevState st, ModelArgs a, double *__restrict__ rec, int64_t *__restrict__ cnt) {
    __shared__ double sm[ekfm::kLinearSmall];
    __shared__ ModelSolve sol;
    const int tid = threadIdx.x;
    const int cur = a.cur;
    const double *__restrict__ x = st.x[cur];
    const double *__restrict__ strip = st.strip[cur];
    double *__restrict__ x_nxt = st.x[cur ^ 1];
    double *__restrict__ strip_nxt = st.strip[cur ^ 1];
    const int64_t ldm = st.ldm;
    const int64_t c = (int64_t)blockIdx.x * kBlock + tid;
    const bool live = c < a.n_mm;

    // (1) the column's loads and patches
    double m[2][2] = { { 0.0, 0.0 }, { 0.0, 0.0 } }, s0 = 0.0, s1 = 0.0, s2 = 0.0, xc = 0.0, dgc = 0.0, dgl = 0.0;
    if (live) {
        if (a.a[0] >= 0) constrain_row_pair_chain<TS>(st, a.pstart, a.npend, a.a[0], c, m[0][0], m[0][1]);
        if (a.a[1] >= 0) constrain_row_pair_chain<TS>(st, a.pstart, a.npend, a.a[1], c, m[1][0], m[1][1]);
        s0 = strip[c]; s1 = strip[ldm + c]; s2 = strip[2 * ldm + c];
        xc = x[3 + c];
        const double *__restrict__ dg = st.diag[st.dcur] + 3 * (c >> 1);
        if (c & 1) { dgl = dg[1]; dgc = dg[2]; } else dgc = dg[0];
    }

    // (2) the small part and H, once per workgroup
    model_small_part<TS>(st, a, sm, sol);
    const bool ok = sol.ok != 0;
    const double *H = sol.H;

    // (3) the column's share of G, K, x and the strip
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
    // (3b) this pair on every landmark's own 2x2 block: the live copies never carry a pending pair
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
        if (tid == 0 && !ok) {
            const int which = sol.rec[7] == 0.0 ? 0 : 1;
            cnt[which] = cnt[which] + 1;
        }
    }
}
