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
// broadcast).  That difference is this file: ModelSolve, and the overloads of small_solve and step_H for it.  Everything else -- the
// operands one per lane, the barriers, the column steps (1), (3), (3b), (4) -- is linear_obs.h's step_small_part and gather_step_body,
// instantiated for ModelArgs: with the H this kernel forms handed to k_gather_linear as an argument, that one writes the same P bit for
// bit (tests/test_model_obs_gpu.py).
// A target on the robot (q = 0) or a non-finite q has no Jacobian: H = 0, and the launch is reported and counted as an irregular S.
// ---------------------------------------------------------------------------------------------------

struct ModelSolve : LinearSolve {
    double H[14];
};

// small_solve for a model: h(x) and H at the x in sm first, and H left for the column lanes
__device__ __forceinline__ void small_solve(const ModelArgs &a, double *sm, ModelSolve &sol) {
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
__device__ __forceinline__ const double *step_H(const ModelArgs &, const ModelSolve &sol) { return sol.H; }

// ekf_model_innovation: the small part alone, and nothing written but the record
template <typename TS>
__global__ __launch_bounds__(64) void k_model_probe(DevState st, ModelArgs a, double *__restrict__ rec) {
    __shared__ double sm[ekfm::kLinearSmall];
    __shared__ ModelSolve sol;
    step_small_part<TS>(st, a, sm, sol);
    if (threadIdx.x < kLinearRecordDoubles) rec[threadIdx.x] = sol.rec[threadIdx.x];
}

// k_gather_linear for a model: its shape, arguments and outputs; rec and cnt are the handle's linear record and counters
template <typename TS>
__global__ __launch_bounds__(kBlock) void k_gather_model(DevState st, ModelArgs a, double *__restrict__ rec, int64_t *__restrict__ cnt) {
    __shared__ double sm[ekfm::kLinearSmall];
    __shared__ ModelSolve sol;
    gather_step_body<TS>(st, a, sm, sol, rec, cnt);
}
