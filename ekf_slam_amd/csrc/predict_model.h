// Fragment of kernels.hip (included there, inside its anonymous namespace, after predict.h): k_predict_model, a chain of motion steps through
// the models of ekfm::motion_eval (ekf_predict_model).
#pragma once

// ---------------------------------------------------------------------------------------------------
// step s = 0 .. m-1, in order:   x_r <- f_s(x_r, u_s)     P <- F_s P F_s' + V_s M_s V_s'  (the noise on the robot block alone)
// F_s = I + N_s with N_s = [fa_s; fb_s] in the heading column of rows 0 and 1: N_s N_t = 0, so over the whole chain row 2 of the strip never
// changes and rows 0 and 1 pick up fa_s * row 2 and fb_s * row 2, one FMA each per step -- predict_strip m times on registers, one read and
// one write of the strip.  fa_s, fb_s depend on the heading BEFORE step s and on u_s alone, and the headings are a serial wrapped sum of the
// turns: every workgroup forms them itself (lane s < m, no exchange between workgroups), workgroup 0 also runs the robot block step by step.
// Nothing of a step's arithmetic depends on m or on the step's position in the chain, so ONE launch of m steps leaves bit for bit what m
// launches of one step leave.  Reads buffer cur, writes a complete buffer cur ^ 1, as k_predict; no tile is touched.
// ---------------------------------------------------------------------------------------------------

// the kernels' one machine-code body of sincosd, as predict_small takes it
struct MotionSinCosNi {
    __device__ __forceinline__ void operator()(double a, double &sn, double &cs) const {
        const double2 r = sincosd_ni(a);
        sn = r.x; cs = r.y;
    }
};

// the robot block under one step: F Prr F' entry by entry as predict_prr_entry forms it (the products through predict_fp), plus
// Q = V M V' (ekfm::motion_noise_entry: one summation order per entry); lower triangle formed, both mirrors take its value, as predict_finish
__device__ __forceinline__ void predict_model_prr(const double prr_in[9], double fa, double fb, const double V[9], const double m6[6],
                                                  double prr[9], double Q[9]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            const double m1 = predict_fp(i, prr_in[j], prr_in[3 + j], prr_in[6 + j], fa, fb);
            const double p2 = predict_fp(i, prr_in[2], prr_in[5], prr_in[8], fa, fb);
            const double c0 = m1 + fa * p2, c1 = m1 + fb * p2;
            const double m2 = j == 0 ? c0 : (j == 1 ? c1 : m1);                           // (F*P)*F'
            const double q = ekfm::motion_noise_entry(V, m6, i, j);
            Q[3 * i + j] = Q[3 * j + i] = q;
            prr[3 * i + j] = prr[3 * j + i] = m2 + q;
        }
}

// One lane per strip column, 256 per workgroup (k_predict's shape); the headings and (fa, fb) of every step by EVERY workgroup, on its first
// m lanes; the pose, Prr and Q by lane 0 of workgroup 0.
__global__ __launch_bounds__(kBlock) void k_predict_model(DevState st, PredictModelArgs a) {
    __shared__ double fab[2 * kPredictModelMax];
    const int tid = threadIdx.x;
    const int cur = a.cur, nxt = cur ^ 1;
    const double *__restrict__ x = st.x[cur];
    double *__restrict__ xn = st.x[nxt];
    if (tid < a.m) {
        // the heading before step tid: the serial wrapped sum of the turns before it, formed as the steps themselves form it
        double th = x[2];
        for (int j = 0; j + 1 < a.m; ++j) {
            const double t2 = ekfm::wrapTo360(th + ekfm::motion_turn(a.e[j].model, a.e[j].u));
            th = j < tid ? t2 : th;
        }
        const PredictModelStep &e = a.e[tid];
        const double xr[3] = { 0.0, 0.0, th }, u[3] = { e.u[0], e.u[1], e.u[2] };
        double xo[3], V[9], fa = 0.0, fb = 0.0;
        ekfm::motion_eval_with(MotionSinCosNi(), e.model, xr, u, xo, fa, fb, V);
        fab[2 * tid] = fa;
        fab[2 * tid + 1] = fb;
    }
    __syncthreads();
    if (blockIdx.x == 0 && tid == 0) {
        double pose[3] = { x[0], x[1], x[2] }, prr[9], Q[9];
        for (int i = 0; i < 9; ++i) { prr[i] = st.prr[cur][i]; Q[i] = 0.0; }
        for (int s = 0; s < a.m; ++s) {
            const PredictModelStep &e = a.e[s];
            const double u[3] = { e.u[0], e.u[1], e.u[2] }, m6[6] = { e.m6[0], e.m6[1], e.m6[2], e.m6[3], e.m6[4], e.m6[5] };
            double pn[3], V[9], fa, fb, pr2[9];
            ekfm::motion_eval_with(MotionSinCosNi(), e.model, pose, u, pn, fa, fb, V);
            predict_model_prr(prr, fab[2 * s], fab[2 * s + 1], V, m6, pr2, Q);           // F's entries: the ones the columns take
            for (int i = 0; i < 9; ++i) prr[i] = pr2[i];
            for (int i = 0; i < 3; ++i) pose[i] = pn[i];
        }
        for (int i = 0; i < 9; ++i) { st.prr[nxt][i] = prr[i]; st.small[12 + i] = Q[i]; }
        for (int i = 0; i < 3; ++i) xn[i] = pose[i];
    }
    const int64_t c = (int64_t)blockIdx.x * kBlock + tid;
    if (c < a.n_mm) {
        const double *__restrict__ s = st.strip[cur];
        double *__restrict__ sn = st.strip[nxt];
        double s0 = s[c], s1 = s[st.ldm + c];
        const double s2 = s[2 * st.ldm + c];
        for (int q = 0; q < a.m; ++q) predict_strip(s0, s1, s2, fab[2 * q], fab[2 * q + 1]);
        sn[c] = s0;
        sn[st.ldm + c] = s1;
        sn[2 * st.ldm + c] = s2;
        xn[3 + c] = x[3 + c];
    }
}
