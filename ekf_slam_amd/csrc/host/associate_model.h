// Fragment of abi.hip, a scan matched to the map under the models' conventions (ekf_associate_model): ekf_append_model's place in the order
// of a handle -- settled, no flush, beside a pass in flight, sharded handles without an exchange -- and nothing written but its own buffers.
#pragma once
namespace {
static_assert(sizeof(ekfm::Match2) == sizeof(ekf_model_match) && sizeof(ekf_model_match) == 48, "Match2 is ekf_model_match, field by field");

// the handle's part: one record per workgroup at capacity and per observation, the m results on the device and in pinned memory with the
// event behind their readback.  (The m x N block of d2_all is allocated when it is first asked for: associate_model_block.)
int32_t create_assoc_model(ekf_handle *h) {
    h->am_nblk_cap = (h->cap + kAssocBlock - 1) / kAssocBlock;
    HIPCHK(h, dalloc(h, &h->d_amparts, (size_t)kAssocModelMax * h->am_nblk_cap));
    HIPCHK(h, dalloc(h, &h->d_amout, (size_t)kAssocModelMax));
    return stage_alloc(h, &h->h_amout, kAssocModelMax * sizeof(ekfm::Match2), &h->ev_amodel);
}

// The results followed by the m x N block, on the device and in pinned memory, so that ONE copy brings both back: kAssocModelMax records,
// then kAssocModelMax x cap doubles.  Not cleared (dalloc's clear runs on the null stream, which this call must not wait for): the
// launches write every entry that is read.  Registered like every other buffer, kept until ekf_destroy.
int32_t associate_model_block(ekf_handle *h) {
    if (h->d_amall) return EKF_OK;
    const size_t bytes = kAssocModelMax * (sizeof(ekfm::Match2) + (size_t)h->cap * sizeof(double));
    void *d = nullptr;
    HIPCHK(h, hipMalloc(&d, bytes));
    h->allocs.push_back(d);
    h->bytes += (int64_t)bytes;
    HIPCHK(h, halloc(h, &h->h_amall, bytes, hipHostMallocDefault));
    h->d_amall = (char *)d;
    return EKF_OK;
}

// the entries into the kernel's form: this call's own refusals, then model_parse's checks of model, z, R and gate (the anchor is ignored)
int32_t associate_model_parse(ekf_handle *h, const std::string &who, const ekf_model_obs *obs, int64_t m, AssocModelArgs &a) {
    a = AssocModelArgs();
    a.m = (int32_t)m;
    for (int64_t k = 0; k < m; ++k) {
        ekf_model_obs o = obs[k];
        REQUIRE(h, o.model != EKF_MODEL_LANDMARK_RANGE, EKF_ERR_INVALID_ARG,
                (who + "EKF_MODEL_LANDMARK_RANGE has no robot block and no single target").c_str());
        REQUIRE(h, o.lm[0] == -1 && o.lm[1] == -1, EKF_ERR_INVALID_ARG, (who + "lm is {-1, -1}: the target is what is searched for").c_str());
        o.anchor[0] = o.anchor[1] = 0.0;
        ModelArgs ma;
        TRY(model_parse(h, who, &o, ma));
        AssocModelEntry &e = a.e[k];
        e.z[0] = ma.z[0]; e.z[1] = ma.z[1];
        for (int q = 0; q < 4; ++q) e.R[q] = ma.R[q];
        e.gate = ma.gate;
        e.model = ma.model;
    }
    return EKF_OK;
}
}  // namespace

extern "C" {
int32_t ekf_associate_model(ekf_handle *h, const ekf_model_obs *obs, int64_t m, ekf_model_match *out, double *d2_all) {
    if (!h) return EKF_ERR_INVALID_ARG;
    const std::string who = "associate_model: ";
    REQUIRE(h, obs != nullptr && out != nullptr, EKF_ERR_INVALID_ARG, (who + "null argument").c_str());
    REQUIRE(h, m >= 1 && m <= EKF_ASSOCIATE_MODEL_MAX, EKF_ERR_INVALID_ARG, (who + "between 1 and EKF_ASSOCIATE_MODEL_MAX observations").c_str());
    AssocModelArgs a;
    TRY(associate_model_parse(h, who, obs, m, a));
    TRY(use_device(h));
    TRY(settle(h));
    REQUIRE(h, !h->pending, EKF_ERR_STATE, (who + "a sharded correction is between begin and finish").c_str());
    TRY(materialize_predict(h));           // (folding a recorded predict into this launch is not built)
    const int64_t N = h->N;
    if (N == 0) {
        ekfm::Match2 none;
        ekfm::match2_init(none);
        for (int64_t k = 0; k < m; ++k) memcpy(&out[k], &none, sizeof none);
        return EKF_OK;
    }
    if (d2_all) TRY(associate_model_block(h));
    // with d2_all the results go to the head of the block, so that one copy brings back both
    char *d_res = d2_all ? h->d_amall : (char *)h->d_amout, *h_res = d2_all ? h->h_amall : (char *)h->h_amout;
    double *d_all = d2_all ? (double *)(d_res + kAssocModelMax * sizeof(ekfm::Match2)) : nullptr;
    const size_t bytes = d2_all ? kAssocModelMax * sizeof(ekfm::Match2) + (size_t)m * N * sizeof(double) : (size_t)m * sizeof(ekfm::Match2);
    a.N = N; a.cur = h->cur;
    {
        TimedLaunch tl(h, EKF_KERNEL_ASSOCIATE);
        HIPCHK(h, launch_assoc_model(h->st, a, h->d_amparts, (ekfm::Match2 *)d_res, d_all, h->stream));
    }
    HIPCHK(h, hipMemcpyAsync(h_res, d_res, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipEventRecord(h->ev_amodel, h->stream));
    HIPCHK(h, hipEventSynchronize(h->ev_amodel));      // this readback alone: a pass on the pass stream is not waited for
    memcpy(out, h_res, (size_t)m * sizeof(ekf_model_match));
    if (d2_all) memcpy(d2_all, h_res + kAssocModelMax * sizeof(ekfm::Match2), (size_t)m * N * sizeof(double));
    return EKF_OK;
}
}  // extern "C"
