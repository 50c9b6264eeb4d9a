// Fragment of kernels.hip (included there, inside its anonymous namespace, after model_obs.h): the update-step of k_gather_model whose
// LANDMARK is read on the device, from the record an earlier launch of the same stream left (k_assign_solve's AssignResult::out[k]):
// k_gather_model_assigned.
#pragma once

// ---------------------------------------------------------------------------------------------------
// ekf_observe_model_assigned queues the assignment of a scan and then one of these launches per observation, with no host wait between
// them: the host cannot fill ModelArgs::a[0], so every lane loads slot->landmark at entry (one uniform 8-byte load; launches of one
// stream are ordered, so the value is the solver's) and the launch goes on as k_gather_model's for that landmark -- the same body, the
// same grid (it depends on n_mm alone), the same operands and outputs.
// An observation the assignment LEFT OUT (-1; defensively, a landmark whose columns do not lie below n_mm) runs as a SKIPPED step: a finite
// no-op like a gated one -- a zero pair takes the ring slot, the state is copied, the host's bookkeeping (finish_step) needs no answer --
// whose record says outcome 3.0 (EKF_LINEAR_UNASSIGNED), d2 NaN, S and nu zero, and which is counted by neither counter.  The model is
// not evaluated for it: a[0] = -1 would read as "anchored at `anchor`".
// What differs from a model step is, again, overloads found by type: small_solve, and step_counted (linear_obs.h).
// ---------------------------------------------------------------------------------------------------

__device__ __forceinline__ void small_solve(const AssignedModelArgs &a, double *sm, ModelSolve &sol) {
    if (!a.skipped) {
        small_solve(static_cast<const ModelArgs &>(a), sm, sol);
        return;
    }
    const double none[7] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    store_pair_record(sol.rec, none, 0.0, 0.0, NAN, 3.0);
    pair_solve(sol, none, 0.0, 0.0, none, none, sm, false);
    for (int q = 0; q < 14; ++q) sol.H[q] = 0.0;
}
__device__ __forceinline__ bool step_counted(const AssignedModelArgs &a, const ModelSolve &) { return !a.skipped; }

// k_gather_model with the landmark in device memory: its grid, block, LDS and outputs; rec is the scan's record of this observation
template <typename TS>
__global__ __launch_bounds__(kBlock) void k_gather_model_assigned(DevState st, AssignedModelArgs a, const AssignedRecord *__restrict__ slot,
                                                                   double *__restrict__ rec, int64_t *__restrict__ cnt) {
    __shared__ double sm[ekfm::kLinearSmall];
    __shared__ ModelSolve sol;
    const int64_t lm = slot->landmark;
    const bool named = lm >= 0 && lm < (a.n_mm >> 1);
    a.a[0] = named ? 2 * lm : -1;
    a.a[1] = -1;
    a.skipped = named ? 0 : 1;
    gather_step_body<TS>(st, a, sm, sol, rec, cnt);
}
