// Fragment of abi.hip, a scan assigned and then applied with no host wait between the two (ekf_observe_model_assigned /
// ekf_assigned_scan_result): assign_model.h's launches into d_asres, then one update-step per observation whose landmark the DEVICE reads
// there (k_gather_model_assigned) -- model.h's rungs, linear.h's counters and finish_step's bookkeeping, and a result block of its own.
#pragma once
namespace {
// What one copy brings back of a scan, in the order it lies on the device: the step records (the array in front of d_asres, one allocation
// with it: create_assign_model), then the head of AssignResult.
struct AssignedScanBlock {
    double rec[kAssocModelMax * kLinearRecordDoubles];
    AssignedRecord out[kAssocModelMax];
    double total, pad;
};
static_assert(offsetof(AssignedScanBlock, out) == sizeof(double) * kAssocModelMax * kLinearRecordDoubles && offsetof(AssignResult, out) == 0 &&
              offsetof(AssignResult, total) == sizeof(AssignedRecord) * kAssocModelMax, "the records, then the head of AssignResult, contiguous");

// the handle's part: the pinned block and the event behind its copy (the device side is create_assign_model's)
int32_t create_model_assigned(ekf_handle *h) {
    return stage_alloc(h, &h->h_scan, sizeof(AssignedScanBlock), &h->ev_scan);
}
}  // namespace

extern "C" {
int32_t ekf_observe_model_assigned(ekf_handle *h, const ekf_model_obs *obs, int64_t m) {
    if (!h) return EKF_ERR_INVALID_ARG;
    const std::string who = "observe_model_assigned: ";
    REQUIRE(h, obs != nullptr, EKF_ERR_INVALID_ARG, (who + "null argument").c_str());
    REQUIRE(h, m >= 1 && m <= EKF_ASSIGN_MODEL_MAX, EKF_ERR_INVALID_ARG, (who + "between 1 and EKF_ASSIGN_MODEL_MAX observations").c_str());
    AssocModelArgs scan;
    TRY(associate_model_parse(h, who, obs, m, scan));
    for (int64_t k = 0; k < m; ++k)
        REQUIRE(h, std::isfinite(scan.e[k].gate), EKF_ERR_INVALID_ARG, (who + "the gate is the price of leaving an observation out: it is finite").c_str());
    TRY(use_device(h));
    TRY(settle(h));
    REQUIRE(h, !h->pending, EKF_ERR_STATE, (who + "a sharded correction is between begin and finish").c_str());
    // ... then ekf_observe_model's rungs, all of them in front of the first launch
    TRY(edit_unsharded(h, who, "a landmark block needs that landmark's row-panel exchanged between the shards"));
    TRY(edit_settled(h, who));
    TRY(materialize_predict(h));
    AssignedScanBlock *blk = reinterpret_cast<AssignedScanBlock *>(h->h_scan);
    if (h->N == 0) {                       // every observation left out: no launch, nothing changes, the result is made here
        if (h->scan_m > 0 && !h->scan_host) HIPCHK(h, hipEventSynchronize(h->ev_scan));       // (an earlier scan's copy into the block has landed)
        double J = 0.0;
        for (int64_t k = 0; k < m; ++k) {
            blk->out[k].landmark = -1; blk->out[k].d2 = INFINITY; blk->out[k].ncand = 0; blk->out[k].reserved = 0;
            double *rec = blk->rec + k * kLinearRecordDoubles;
            for (int q = 0; q < kLinearRecordDoubles; ++q) rec[q] = 0.0;
            rec[6] = NAN; rec[7] = (double)EKF_LINEAR_UNASSIGNED;
            J += scan.e[k].gate;
        }
        blk->total = J;
        h->scan_m = m; h->scan_host = true;
        return EKF_OK;
    }
    TRY(refresh_work(h));
    scan.N = h->N; scan.cur = h->cur;
    {
        TimedLaunch tl(h, EKF_KERNEL_ASSOCIATE);
        HIPCHK(h, launch_assign_model(h->st, scan, h->d_amparts, h->d_aslists, h->d_assel, h->d_asres, h->stream));
    }
    // One step per observation, in scan order: its landmark, or "left out", is read by the launch; the grid and the host's bookkeeping
    // depend on neither.  finish_step may end a batch and start a pass between two steps: every step reads the handle anew.
    for (int64_t k = 0; k < m; ++k) {
        TRY(refresh_work(h));
        const AssocModelEntry &e = scan.e[k];
        AssignedModelArgs a = AssignedModelArgs();
        a.model = e.model;
        a.z[0] = e.z[0]; a.z[1] = e.z[1];
        for (int q = 0; q < 4; ++q) a.R[q] = e.R[q];
        a.gate = e.gate;
        a.a[0] = a.a[1] = -1;
        a.n_mm = n_mm(h); a.cur = h->cur; a.npend = h->npend; a.pstart = h->pstart;
        TIMED(h, EKF_KERNEL_GATHER, launch_gather_model_assigned(h->st, a, &h->d_asres->out[k], h->d_scanrec + k * kLinearRecordDoubles, h->d_lincnt,
                                                                 h->storage, h->stream));
        TRY(finish_step(h));
    }
    HIPCHK(h, hipMemcpyAsync(blk, h->d_scanrec, sizeof(AssignedScanBlock), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipEventRecord(h->ev_scan, h->stream));
    h->scan_m = m; h->scan_host = false;
    return EKF_OK;
}

int32_t ekf_assigned_scan_result(ekf_handle *h, int64_t *m, ekf_model_assigned *out, ekf_linear_result *res, double *total) {
    if (!h) return EKF_ERR_INVALID_ARG;
    REQUIRE(h, h->scan_m > 0, EKF_ERR_STATE, "assigned_scan_result: no scan has been queued (ekf_observe_model_assigned)");
    TRY(use_device(h));
    if (!h->scan_host) HIPCHK(h, hipEventSynchronize(h->ev_scan));      // the latest scan's copy alone: a pass on the pass stream is not waited for
    const AssignedScanBlock *blk = reinterpret_cast<const AssignedScanBlock *>(h->h_scan);
    if (m) *m = h->scan_m;
    if (out) memcpy(out, blk->out, (size_t)h->scan_m * sizeof(ekf_model_assigned));
    for (int64_t k = 0; res && k < h->scan_m; ++k) linear_fill(blk->rec + k * kLinearRecordDoubles, &res[k]);
    if (total) *total = blk->total;
    return EKF_OK;
}
}  // extern "C"
