// Fragment of abi.hip, the joint compatibility of a scan's pairings (ekf_joint_innovation): ekf_linear_innovation's place in the order of a
// handle -- the rungs of linear_rungs, no flush, the tiles read patched with the pending pairs, beside a pass in flight -- with
// ekf_associate_model's scan in front and a readback waited for through an event of its own.
#pragma once
namespace {
static_assert(sizeof(JointRecord) == sizeof(ekf_joint_result) && sizeof(ekf_joint_result) == 24, "JointRecord is ekf_joint_result, field by field");
static_assert(kJointMax == EKF_JOINT_MAX && kJointHypMax == EKF_JOINT_HYP_MAX, "the kernel's limits are the header's");

// one call's answers without S, on the device and in pinned memory: nh records, then the prefixes (nh x m), then nu (nh x 2m)
constexpr size_t joint_out_bytes(int64_t nh, int64_t m) { return (size_t)nh * (sizeof(JointRecord) + (size_t)m * 8 + (size_t)2 * m * 8); }

int32_t create_joint(ekf_handle *h) {
    HIPCHK(h, dalloc(h, &h->d_jhyp, (size_t)kJointHypMax * kJointMax));
    HIPCHK(h, dalloc(h, &h->d_jout, joint_out_bytes(kJointHypMax, kJointMax)));
    HIPCHK(h, halloc(h, &h->h_jhyp, (size_t)kJointHypMax * kJointMax * sizeof(int64_t), hipHostMallocDefault));
    return stage_alloc(h, &h->h_jout, joint_out_bytes(kJointHypMax, kJointMax), &h->ev_joint);
}

// the stacked S of kJointHypMax hypotheses at kJointMax observations, on both sides; not cleared (as associate_model_block: the launch
// writes every entry that is read), registered like every other buffer, kept until ekf_destroy
int32_t joint_S_block(ekf_handle *h) {
    if (h->d_jS) return EKF_OK;
    const size_t bytes = (size_t)kJointHypMax * kJointRows * kJointRows * sizeof(double);
    void *d = nullptr;
    HIPCHK(h, hipMalloc(&d, bytes));
    h->allocs.push_back(d);
    h->bytes += (int64_t)bytes;
    HIPCHK(h, halloc(h, &h->h_jS, bytes, hipHostMallocDefault));
    h->d_jS = (double *)d;
    return EKF_OK;
}
}  // namespace

extern "C" {
int32_t ekf_joint_innovation(ekf_handle *h, const ekf_model_obs *obs, int64_t m, const int64_t *hyp, int64_t nh, ekf_joint_result *out,
                             double *d2_prefix, double *nu, double *S) {
    if (!h) return EKF_ERR_INVALID_ARG;
    const std::string who = "joint_innovation: ";
    REQUIRE(h, obs != nullptr && hyp != nullptr && out != nullptr, EKF_ERR_INVALID_ARG, (who + "null argument").c_str());
    REQUIRE(h, m >= 1 && m <= EKF_JOINT_MAX, EKF_ERR_INVALID_ARG, (who + "between 1 and EKF_JOINT_MAX observations").c_str());
    REQUIRE(h, nh >= 1 && nh <= EKF_JOINT_HYP_MAX, EKF_ERR_INVALID_ARG, (who + "between 1 and EKF_JOINT_HYP_MAX hypotheses").c_str());
    AssocModelArgs scan;
    TRY(associate_model_parse(h, who, obs, m, scan));
    int64_t top = -1;
    for (int64_t i = 0; i < nh; ++i)
        for (int64_t k = 0; k < m; ++k) {
            const int64_t l = hyp[i * m + k];
            REQUIRE(h, l >= -1, EKF_ERR_INVALID_ARG, (who + "a hypothesis entry is a 0-based landmark, or -1 for an observation left out").c_str());
            for (int64_t q = 0; q < k && l >= 0; ++q)
                REQUIRE(h, hyp[i * m + q] != l, EKF_ERR_INVALID_ARG, (who + "a landmark occurs twice in one hypothesis").c_str());
            top = std::max(top, l);
        }
    // ekf_observe_linear's rungs (the cross blocks P(l_a, l_b) live in other shards' tiles), with no landmark of their own to check ...
    ModelArgs rung;
    const int64_t none[2] = { -1, -1 };
    TRY(linear_rungs(h, who, none, rung));
    // ... then the hypotheses' landmarks, now that N is exact
    REQUIRE(h, top < h->N, EKF_ERR_INDEX, (who + "landmark index outside the state").c_str());

    JointArgs a = JointArgs();
    a.N = h->N; a.m = (int32_t)m; a.cur = rung.cur; a.npend = rung.npend; a.pstart = rung.pstart;
    for (int64_t k = 0; k < m; ++k) a.e[k] = scan.e[k];
    if (S) TRY(joint_S_block(h));
    JointRecord *d_rec = (JointRecord *)h->d_jout;
    double *d_prefix = (double *)(h->d_jout + (size_t)nh * sizeof(JointRecord)), *d_nu = d_prefix + nh * m;
    const size_t bytes = joint_out_bytes(nh, m), s_bytes = (size_t)nh * 4 * m * m * sizeof(double);
    memcpy(h->h_jhyp, hyp, (size_t)nh * m * sizeof(int64_t));      // (the area is free: every call waits for its own readback)
    HIPCHK(h, hipMemcpyAsync(h->d_jhyp, h->h_jhyp, (size_t)nh * m * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    {
        TimedLaunch tl(h, EKF_KERNEL_ASSOCIATE);
        HIPCHK(h, launch_joint_innovation(h->st, a, h->d_jhyp, (int)nh, d_rec, d_prefix, d_nu, S ? h->d_jS : nullptr, h->storage, h->stream));
    }
    HIPCHK(h, hipMemcpyAsync(h->h_jout, h->d_jout, bytes, hipMemcpyDeviceToHost, h->stream));
    if (S) HIPCHK(h, hipMemcpyAsync(h->h_jS, h->d_jS, s_bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipEventRecord(h->ev_joint, h->stream));
    HIPCHK(h, hipEventSynchronize(h->ev_joint));       // this readback alone: a pass on the pass stream is not waited for
    memcpy(out, h->h_jout, (size_t)nh * sizeof(ekf_joint_result));
    const double *h_prefix = (const double *)(h->h_jout + (size_t)nh * sizeof(JointRecord));
    if (d2_prefix) memcpy(d2_prefix, h_prefix, (size_t)nh * m * sizeof(double));
    if (nu) memcpy(nu, h_prefix + nh * m, (size_t)nh * 2 * m * sizeof(double));
    if (S) memcpy(S, h->h_jS, s_bytes);
    return EKF_OK;
}
}  // extern "C"
