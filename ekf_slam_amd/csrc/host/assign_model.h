// Fragment of abi.hip, a scan assigned to the map one-to-one (ekf_assign_model): ekf_associate_model's place in the order of a handle --
// settled, no flush, beside a pass in flight, sharded handles without an exchange -- and nothing written but its own buffers.
#pragma once
namespace {
static_assert(sizeof(AssignedRecord) == sizeof(ekf_model_assigned) && sizeof(ekf_model_assigned) == 32, "AssignedRecord is ekf_model_assigned, field by field");
static_assert(kAssignCandidates == EKF_ASSIGN_CANDIDATES && ekfm::kAssignCand == EKF_ASSIGN_CANDIDATES, "one width of the candidate lists");
static_assert(kAssocModelMax == EKF_ASSIGN_MODEL_MAX && ekfm::kAssignMax == EKF_ASSIGN_MODEL_MAX, "one scan size");
static_assert(sizeof(ekfm::CandList) == 16 + 16 * EKF_ASSIGN_CANDIDATES, "CandList: n, pad, the indices, the d2");

// the handle's part: one list per workgroup at capacity and per observation, the selected lists, the result block on the device and in
// pinned memory with the event behind its readback.  (The Match2 record per workgroup is ekf_associate_model's d_amparts: the two calls
// are ordered by the handle's stream.)
int32_t create_assign_model(ekf_handle *h) {
    HIPCHK(h, dalloc(h, &h->d_aslists, (size_t)kAssocModelMax * h->am_nblk_cap));
    HIPCHK(h, dalloc(h, &h->d_assel, (size_t)kAssocModelMax));
    // the result block, with the step records of ekf_observe_model_assigned in front of it in the same allocation: one copy then brings back
    // the records and the block's head (host/model_assigned.h)
    constexpr size_t recs = (size_t)kAssocModelMax * kLinearRecordDoubles;
    HIPCHK(h, dalloc(h, &h->d_scanrec, recs + sizeof(AssignResult) / sizeof(double)));
    h->d_asres = reinterpret_cast<AssignResult *>(h->d_scanrec + recs);
    static_assert(sizeof(AssignResult) % sizeof(double) == 0, "the result block is whole doubles");
    return stage_alloc(h, &h->h_asres, sizeof(AssignResult), &h->ev_assign);
}
}  // namespace

extern "C" {
int32_t ekf_assign_model(ekf_handle *h, const ekf_model_obs *obs, int64_t m, ekf_model_assigned *out, ekf_model_match *match, int64_t *cand,
                         double *cand_d2, double *total) {
    if (!h) return EKF_ERR_INVALID_ARG;
    const std::string who = "assign_model: ";
    REQUIRE(h, obs != nullptr && out != nullptr, EKF_ERR_INVALID_ARG, (who + "null argument").c_str());
    REQUIRE(h, m >= 1 && m <= EKF_ASSIGN_MODEL_MAX, EKF_ERR_INVALID_ARG, (who + "between 1 and EKF_ASSIGN_MODEL_MAX observations").c_str());
    AssocModelArgs a;
    TRY(associate_model_parse(h, who, obs, m, a));
    REQUIRE(h, (cand == nullptr) == (cand_d2 == nullptr), EKF_ERR_INVALID_ARG, (who + "cand and cand_d2 are given together or not at all").c_str());
    for (int64_t k = 0; k < m; ++k)
        REQUIRE(h, std::isfinite(a.e[k].gate), EKF_ERR_INVALID_ARG, (who + "the gate is the price of leaving an observation out: it is finite").c_str());
    TRY(use_device(h));
    TRY(settle(h));
    REQUIRE(h, !h->pending, EKF_ERR_STATE, (who + "a sharded correction is between begin and finish").c_str());
    TRY(materialize_predict(h));
    const int64_t N = h->N;
    const size_t lists = (size_t)m * EKF_ASSIGN_CANDIDATES;
    if (N == 0) {                          // every observation left out, the lists empty, no launch
        ekfm::Match2 none;
        ekfm::match2_init(none);
        double J = 0.0;
        for (int64_t k = 0; k < m; ++k) {
            out[k].landmark = -1; out[k].d2 = INFINITY; out[k].ncand = 0; out[k].reserved = 0;
            if (match) memcpy(&match[k], &none, sizeof none);
            J += a.e[k].gate;
        }
        for (size_t f = 0; cand && f < lists; ++f) { cand[f] = -1; cand_d2[f] = INFINITY; }
        if (total) *total = J;
        return EKF_OK;
    }
    a.N = N; a.cur = h->cur;
    {
        TimedLaunch tl(h, EKF_KERNEL_ASSOCIATE);
        HIPCHK(h, launch_assign_model(h->st, a, h->d_amparts, h->d_aslists, h->d_assel, h->d_asres, h->stream));
    }
    // the head of the block always; the lists, which lie behind it, where they are asked for
    const size_t bytes = cand ? sizeof(AssignResult) : offsetof(AssignResult, cand);
    HIPCHK(h, hipMemcpyAsync(h->h_asres, h->d_asres, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipEventRecord(h->ev_assign, h->stream));
    HIPCHK(h, hipEventSynchronize(h->ev_assign));      // this readback alone: a pass on the pass stream is not waited for
    const AssignResult &r = *h->h_asres;
    memcpy(out, r.out, (size_t)m * sizeof(ekf_model_assigned));
    if (match) memcpy(match, r.match, (size_t)m * sizeof(ekf_model_match));
    if (cand) {
        memcpy(cand, r.cand, lists * sizeof(int64_t));
        memcpy(cand_d2, r.cand_d2, lists * sizeof(double));
    }
    if (total) *total = r.total;
    return EKF_OK;
}
}  // extern "C"
