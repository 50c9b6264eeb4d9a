// Fragment of kernels.hip (included there, inside its anonymous namespace, after model_obs.h): the rank-2 pair of a model observation
// RELINEARISED on lane 0 (ekf_observe_model_iterated / ekf_model_innovation_iterated, the iterated EKF update): k_gather_model_iter,
// k_model_iter_probe.
#pragma once

// ---------------------------------------------------------------------------------------------------
// model_obs.h linearises h once, at the prior x.  Here lane 0 runs ekfm::model_iterate (device_math.h: Gauss-Newton on the MAP cost over
// the seven entries and the 7 x 7 covariance the small part has in LDS anyway) and hands the column lanes the LAST linearisation's H, S^-1
// and effective residual r = wrap(z - h(xi)) - H (x0 - xi): one pair, one ring slot, the traffic of k_gather_model.  That is this file:
// IterSolve, and the overloads of small_solve and step_H for IterModelArgs; the column steps are linear_obs.h's gather_step_body as it
// stands.  Every workgroup repeats the loop (no workgroup reads what another one of the launch writes), serially on one lane: spread
// over lanes the sums would change their order.
// The 8-double record keeps the FIRST linearisation's S, nu and d2 -- the gate is read there, as ekf_model_innovation reports it -- and
// the overall outcome; a later iterate that is not posed or has an irregular S makes the launch the irregular no-op, all or nothing.
// With iterations = 1 the launch writes k_gather_model's bits (tests/test_model_iter_gpu.py).
// ---------------------------------------------------------------------------------------------------

struct IterSolve : ModelSolve {
    double it[kIterRecordDoubles];
};

__device__ __forceinline__ void small_solve(const IterModelArgs &a, double *sm, IterSolve &sol) {
    double H[14], Gs[14], S[4], r[2];
    ekfm::ModelIterate it;
    const int outcome = ekfm::model_iterate(a.model, sm, a.anchor, a.a[0] >= 0, a.z, a.R, a.gate, a.iterations, a.tol, H, Gs, S, r, it);
    store_pair_record(sol.rec, it.S0, it.nu0[0], it.nu0[1], it.d2, (double)outcome);
    pair_solve(sol, S, r[0], r[1], Gs, Gs + 7, sm, outcome == 1);
    for (int q = 0; q < 14; ++q) sol.H[q] = H[q];
    for (int q = 0; q < 4; ++q) sol.it[q] = S[q];
    sol.it[4] = r[0]; sol.it[5] = r[1];
    sol.it[6] = (double)it.used; sol.it[7] = (double)it.converged; sol.it[8] = it.last_step;
    for (int q = 0; q < 7; ++q) sol.it[9 + q] = it.xi[q];
}
__device__ __forceinline__ const double *step_H(const IterModelArgs &, const IterSolve &sol) { return sol.H; }

// ekf_model_innovation_iterated: the small part alone, and nothing written but the two records
template <typename TS>
__global__ __launch_bounds__(64) void k_model_iter_probe(DevState st, IterModelArgs a, double *__restrict__ rec, double *__restrict__ itrec) {
    __shared__ double sm[ekfm::kLinearSmall];
    __shared__ IterSolve sol;
    step_small_part<TS>(st, a, sm, sol);
    if (threadIdx.x < kLinearRecordDoubles) rec[threadIdx.x] = sol.rec[threadIdx.x];
    if (threadIdx.x >= 16 && threadIdx.x < 16 + kIterRecordDoubles) itrec[threadIdx.x - 16] = sol.it[threadIdx.x - 16];
}

// k_gather_model with the loop in its small part: its shape, arguments and outputs, and workgroup 0's second record
template <typename TS>
__global__ __launch_bounds__(kBlock) void k_gather_model_iter(DevState st, IterModelArgs a, double *__restrict__ rec, int64_t *__restrict__ cnt,
                                                              double *__restrict__ itrec) {
    __shared__ double sm[ekfm::kLinearSmall];
    __shared__ IterSolve sol;
    gather_step_body<TS>(st, a, sm, sol, rec, cnt);
    if (blockIdx.x == 0 && threadIdx.x >= 192 && threadIdx.x < 192 + kIterRecordDoubles) itrec[threadIdx.x - 192] = sol.it[threadIdx.x - 192];
}
