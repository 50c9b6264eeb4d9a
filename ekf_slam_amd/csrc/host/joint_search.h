// Fragment of abi.hip, the joint-compatibility search over a scan (ekf_joint_search): ekf_joint_innovation's place in the order of a
// handle -- the rungs of linear_rungs, no flush, the tiles read patched with the pending pairs, beside a pass in flight -- with
// ekf_assign_model's first two launches in front, a prepare launch and two launches per scan index queued behind them with no wait, and
// ONE readback waited for through ev_joint.
#pragma once
namespace {
static_assert(sizeof(JointSearchResult) == sizeof(ekf_joint_search_result) && offsetof(JointSearchResult, tested) == offsetof(ekf_joint_search_result, tested),
              "JointSearchResult is ekf_joint_search_result, field by field");
static_assert(kJointSearchCand == EKF_JOINT_SEARCH_CAND && kJointSearchBeam == EKF_JOINT_SEARCH_BEAM_MAX, "the kernels' limits are the header's");

// the store and the block that comes back, at the first call; not cleared (as joint_S_block: the launches write every entry that is
// read), registered like every other buffer, kept until ekf_destroy
int32_t joint_search_alloc(ekf_handle *h) {
    if (h->d_jsearch) return EKF_OK;
    void *d = nullptr, *o = nullptr;
    HIPCHK(h, hipMalloc(&d, sizeof(JointSearchStore)));
    h->allocs.push_back(d);
    h->bytes += (int64_t)sizeof(JointSearchStore);
    HIPCHK(h, hipMalloc(&o, sizeof(JointSearchOut)));
    h->allocs.push_back(o);
    h->bytes += (int64_t)sizeof(JointSearchOut);
    HIPCHK(h, halloc(h, &h->h_jsout, sizeof(JointSearchOut), hipHostMallocDefault));
    h->d_jsout = (JointSearchOut *)o;
    h->d_jsearch = (JointSearchStore *)d;
    return EKF_OK;
}
}  // namespace

extern "C" {
int32_t ekf_joint_search(ekf_handle *h, const ekf_model_obs *obs, int64_t m, const double *threshold, int32_t beam, ekf_joint_search_result *res,
                         ekf_model_match *match, int64_t *cand, double *cand_d2, int64_t *alive_hyp, double *alive_d2) {
    if (!h) return EKF_ERR_INVALID_ARG;
    const std::string who = "joint_search: ";
    REQUIRE(h, obs != nullptr && res != nullptr, EKF_ERR_INVALID_ARG, (who + "null argument").c_str());
    REQUIRE(h, m >= 1 && m <= EKF_JOINT_MAX, EKF_ERR_INVALID_ARG, (who + "between 1 and EKF_JOINT_MAX observations").c_str());
    AssocModelArgs scan;
    TRY(associate_model_parse(h, who, obs, m, scan));
    REQUIRE(h, (cand == nullptr) == (cand_d2 == nullptr), EKF_ERR_INVALID_ARG, (who + "cand and cand_d2 are given together or not at all").c_str());
    for (int64_t k = 0; k < m; ++k)
        REQUIRE(h, std::isfinite(scan.e[k].gate), EKF_ERR_INVALID_ARG, (who + "the gate decides what a candidate is: it is finite").c_str());
    REQUIRE(h, threshold != nullptr, EKF_ERR_INVALID_ARG, (who + "null threshold").c_str());
    for (int64_t d = 0; d <= 2 * m; ++d)
        REQUIRE(h, std::isfinite(threshold[d]) && threshold[d] >= 0.0, EKF_ERR_INVALID_ARG, (who + "a threshold is finite and not negative").c_str());
    REQUIRE(h, beam >= 1 && beam <= EKF_JOINT_SEARCH_BEAM_MAX, EKF_ERR_INVALID_ARG, (who + "beam between 1 and EKF_JOINT_SEARCH_BEAM_MAX").c_str());
    REQUIRE(h, (alive_hyp == nullptr) == (alive_d2 == nullptr), EKF_ERR_INVALID_ARG,
            (who + "alive_hyp and alive_d2 are given together or not at all").c_str());
    // ekf_observe_linear's rungs, with no landmark of their own to check (ekf_joint_innovation's)
    ModelArgs rung;
    const int64_t none[2] = { -1, -1 };
    TRY(linear_rungs(h, who, none, rung));

    const int64_t N = h->N;
    const size_t lists = (size_t)m * EKF_ASSIGN_CANDIDATES;
    if (N == 0) {                          // every entry left out, the lists empty, no launch
        ekfm::Match2 nobody;
        ekfm::match2_init(nobody);
        memset(res, 0, sizeof *res);
        for (int64_t k = 0; k < EKF_JOINT_MAX; ++k) res->lm[k] = -1;
        res->nalive = 1;
        for (int64_t k = 0; match && k < m; ++k) memcpy(&match[k], &nobody, sizeof nobody);
        for (size_t f = 0; cand && f < lists; ++f) { cand[f] = -1; cand_d2[f] = INFINITY; }
        for (int64_t f = 0; alive_hyp && f < (int64_t)EKF_JOINT_SEARCH_BEAM_MAX * m; ++f) alive_hyp[f] = -1;
        for (int64_t s = 0; alive_d2 && s < EKF_JOINT_SEARCH_BEAM_MAX; ++s) alive_d2[s] = s == 0 ? 0.0 : NAN;
        return EKF_OK;
    }
    TRY(joint_search_alloc(h));

    scan.N = N; scan.cur = rung.cur;
    JointArgs a = JointArgs();
    a.N = N; a.m = (int32_t)m; a.cur = rung.cur; a.npend = rung.npend; a.pstart = rung.pstart;
    JointSearchLevelArgs la = JointSearchLevelArgs();
    la.m = (int32_t)m; la.beam = beam;
    for (int64_t d = 0; d <= 2 * m; ++d) la.threshold[d] = threshold[d];
    for (int64_t k = 0; k < m; ++k) {
        a.e[k] = scan.e[k];
        la.rows[k] = (scan.e[k].model == 1 || scan.e[k].model == 4) ? 2 : 1;
    }
    JointSearchArgs sa = JointSearchArgs();
    sa.N = N; sa.m = (int32_t)m; sa.cur = rung.cur; sa.npend = rung.npend; sa.pstart = rung.pstart;
    {
        TimedLaunch tl(h, EKF_KERNEL_ASSOCIATE);
        HIPCHK(h, launch_assign_lists(h->st, scan, h->d_amparts, h->d_aslists, h->d_assel, h->d_asres, h->stream));
    }
    TIMED(h, EKF_KERNEL_ASSOCIATE,
          launch_joint_search_prepare(h->st, a, h->d_assel, (const int64_t *)h->d_asres->match, h->d_jsearch, h->d_jsout, h->stream));
    for (int32_t k = 0; k < (int32_t)m; ++k) {
        sa.level = la.level = k;
        TIMED(h, EKF_KERNEL_ASSOCIATE, launch_joint_search_level(h->st, sa, la, h->d_assel, h->d_jsearch, h->d_jsout, 1, h->storage, h->stream));
        TIMED(h, EKF_KERNEL_ASSOCIATE, launch_joint_search_level(h->st, sa, la, h->d_assel, h->d_jsearch, h->d_jsout, 2, h->storage, h->stream));
    }
    // the head always; the final beam and the lists, which lie behind it in that order, where they are asked for
    const size_t bytes = cand ? sizeof(JointSearchOut) : alive_hyp ? offsetof(JointSearchOut, cand) : offsetof(JointSearchOut, alive_d2);
    HIPCHK(h, hipMemcpyAsync(h->h_jsout, h->d_jsout, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipEventRecord(h->ev_joint, h->stream));
    HIPCHK(h, hipEventSynchronize(h->ev_joint));       // this readback alone: a pass on the pass stream is not waited for
    const JointSearchOut &r = *h->h_jsout;
    memcpy(res, &r.res, sizeof *res);
    if (match) memcpy(match, r.match, (size_t)m * sizeof(ekf_model_match));
    if (cand) {
        memcpy(cand, r.cand, lists * sizeof(int64_t));
        memcpy(cand_d2, r.cand_d2, lists * sizeof(double));
    }
    if (alive_hyp) {
        memcpy(alive_hyp, r.alive_hyp, (size_t)EKF_JOINT_SEARCH_BEAM_MAX * m * sizeof(int64_t));
        memcpy(alive_d2, r.alive_d2, (size_t)EKF_JOINT_SEARCH_BEAM_MAX * sizeof(double));
    }
    return EKF_OK;
}
}  // extern "C"
