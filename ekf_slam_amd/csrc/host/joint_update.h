// Fragment of abi.hip, a scan's pairings applied as ONE joint update (ekf_observe_model_joint, and ekf_observe_model_joint_iterated through it): ekf_joint_innovation's arguments and rungs for one
// hypothesis, then ekf_merge_landmarks_batch's route -- flush first, the pairs into the batch's private F64 ring, one F64-arithmetic pass
// through launch_downdate -- so the handle's own ring, cfg.batch and cfg.pass_arith are not involved.
#pragma once
namespace {
static_assert(EKF_MERGE_BATCH_MAX >= EKF_JOINT_MAX, "the joint update's pairs share ekf_merge_landmarks_batch's private ring");

// everything that can fail for lack of memory, before anything changes: the private ring (merge_batch_alloc's, by its formula) and the block
int32_t joint_update_alloc(ekf_handle *h) {
    const bool first = !h->d_mring || !h->d_jblock;
    if (!h->d_mring) HIPCHK(h, dalloc(h, &h->d_mring, (size_t)h->st.pair_stride * EKF_MERGE_BATCH_MAX * 2));
    if (!h->d_jblock) HIPCHK(h, dalloc(h, &h->d_jblock, 1));
    if (first) HIPCHK(h, hipDeviceSynchronize());          // dalloc clears on the null stream (see removal_alloc)
    return EKF_OK;
}

// The loop's controls of ekf_observe_model_joint_iterated (host/joint_iter.h); nullptr: the plain call, linearised once by k_joint_factor.
struct JointIterCtl { int32_t iterations; double tol; ekf_joint_iter_result *it; };
int32_t joint_iter_alloc(ekf_handle *h);
void joint_iter_fill(const double *rec, ekf_joint_iter_result *it);

// ekf_observe_model_joint and ekf_observe_model_joint_iterated: ONE text for the arguments and the order of a call.
// Order: arguments -> the rungs, with the landmarks checked once N is exact -> allocations -> flush -> factor launch, readback, wait, decision
// -> gather launch -> the pass, in place on the main stream.
int32_t observe_joint(ekf_handle *h, const std::string &who, const ekf_model_obs *obs, int64_t m, const int64_t *lm, double gate,
                      const JointIterCtl *ctl, ekf_joint_result *res, double *nu, double *S) {
    REQUIRE(h, obs != nullptr && lm != nullptr && res != nullptr, EKF_ERR_INVALID_ARG, (who + "null argument").c_str());
    REQUIRE(h, m >= 1 && m <= EKF_JOINT_MAX, EKF_ERR_INVALID_ARG, (who + "between 1 and EKF_JOINT_MAX observations").c_str());
    AssocModelArgs scan;
    TRY(associate_model_parse(h, who, obs, m, scan));
    int64_t top = -1, np = 0;
    for (int64_t k = 0; k < m; ++k) {
        const int64_t l = lm[k];
        REQUIRE(h, l >= -1, EKF_ERR_INVALID_ARG, (who + "a pairing is a 0-based landmark, or -1 for an observation left out").c_str());
        for (int64_t q = 0; q < k && l >= 0; ++q)
            REQUIRE(h, lm[q] != l, EKF_ERR_INVALID_ARG, (who + "a landmark occurs twice").c_str());
        top = std::max(top, l);
        if (l >= 0) ++np;
    }
    double g;
    TRY(parse_gate(h, who, gate, g));
    if (ctl) {
        REQUIRE(h, ctl->iterations >= 1 && ctl->iterations <= EKF_JOINT_ITER_MAX, EKF_ERR_INVALID_ARG, (who + "iterations is 1 .. EKF_JOINT_ITER_MAX").c_str());
        REQUIRE(h, ctl->tol >= 0.0, EKF_ERR_INVALID_ARG, (who + "tol is a number >= 0").c_str());          // (a NaN fails the comparison)
    }
    ModelArgs rung;
    const int64_t none[2] = { -1, -1 };
    TRY(linear_rungs(h, who, none, rung));
    REQUIRE(h, top < h->N, EKF_ERR_INDEX, (who + "landmark index outside the state").c_str());
    if (np == 0) {
        // nothing is paired: the empty update, applied -- what ekf_joint_innovation reports for it, formed here
        res->d2 = 0.0; res->dof = 0; res->pairings = 0; res->outcome = EKF_LINEAR_APPLIED; res->first_irregular = -1;
        if (nu) for (int64_t i = 0; i < 2 * m; ++i) nu[i] = 0.0;
        if (S) for (int64_t e = 0; e < 4 * m * m; ++e) S[e] = e % (2 * m) == e / (2 * m) ? 1.0 : 0.0;
        if (ctl && ctl->it) {
            ekf_joint_iter_result empty = ekf_joint_iter_result();
            empty.converged = 1; empty.irregular_at = empty.irregular_obs = -1;
            *ctl->it = empty;
        }
        return EKF_OK;
    }
    TRY(joint_update_alloc(h));
    if (ctl) TRY(joint_iter_alloc(h));
    if (S) TRY(joint_S_block(h));
    TRY(flush_pending(h));                 // retires a pass in flight; from here on the tiles hold the live P and the ring is empty

    JointArgs a = JointArgs();
    a.N = h->N; a.m = (int32_t)m; a.cur = h->cur; a.npend = 0; a.pstart = 0;
    for (int64_t k = 0; k < m; ++k) a.e[k] = scan.e[k];
    JointRecord *d_rec = (JointRecord *)h->d_jout;
    double *d_nu = (double *)(h->d_jout + sizeof(JointRecord) + (size_t)m * 8);       // joint_out_bytes(1, m)'s layout: record, prefixes, nu
    const size_t bytes = joint_out_bytes(1, m), s_bytes = (size_t)4 * m * m * sizeof(double);
    memcpy(h->h_jhyp, lm, (size_t)m * sizeof(int64_t));        // (the area is free: every call waits for its own readback)
    HIPCHK(h, hipMemcpyAsync(h->d_jhyp, h->h_jhyp, (size_t)m * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    {
        TimedLaunch tl(h, EKF_KERNEL_ASSOCIATE);
        if (ctl) {
            JointIterArgs ia = JointIterArgs();
            ia.gate = g; ia.tol = ctl->tol; ia.iterations = ctl->iterations;
            HIPCHK(h, launch_joint_factor_iter(h->st, a, ia, h->d_jhyp, h->d_jblock, d_rec, h->d_jiter, d_nu, S ? h->d_jS : nullptr, h->storage, h->stream));
        } else {
            HIPCHK(h, launch_joint_factor(h->st, a, h->d_jhyp, h->d_jblock, d_rec, d_nu, S ? h->d_jS : nullptr, h->storage, h->stream));
        }
    }
    if (ctl) HIPCHK(h, hipMemcpyAsync(h->h_jiter, h->d_jiter, kJointIterRecordDoubles * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->h_jout, h->d_jout, bytes, hipMemcpyDeviceToHost, h->stream));
    if (S) HIPCHK(h, hipMemcpyAsync(h->h_jS, h->d_jS, s_bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipEventRecord(h->ev_joint, h->stream));
    HIPCHK(h, hipEventSynchronize(h->ev_joint));
    memcpy(res, h->h_jout, sizeof(ekf_joint_result));
    if (nu) memcpy(nu, h->h_jout + sizeof(JointRecord) + (size_t)m * 8, (size_t)2 * m * sizeof(double));
    if (S) memcpy(S, h->h_jS, s_bytes);
    if (ctl && ctl->it) joint_iter_fill(h->h_jiter, ctl->it);
    // the decision, on the host, before anything is written
    if (res->outcome != EKF_LINEAR_APPLIED) {
        res->outcome = EKF_LINEAR_IRREGULAR;
        return fail(h, EKF_ERR_STATE, (who + "observation " + std::to_string(res->first_irregular) + ": the pairing has no d2 (its target on the "
                    "robot, a state that is not finite, or a stacked S that is not positive definite); nothing was changed").c_str());
    }
    if (!(res->d2 <= g)) { res->outcome = EKF_LINEAR_GATED; return EKF_OK; }
    if (ctl && h->h_jiter[4] >= 0.0) {
        res->outcome = EKF_LINEAR_IRREGULAR;
        return fail(h, EKF_ERR_STATE, (who + "observation " + std::to_string((int)h->h_jiter[5]) + " at linearisation " + std::to_string((int)h->h_jiter[4]) +
                    ": the pairing is not posed at that iterate (its target on the robot, an iterate that is not finite), or the stacked S is not "
                    "positive definite there; nothing was changed").c_str());
    }

    // the gather, on a view of the state whose pair ring is the private one
    DevState st = h->st;
    st.Gp = h->d_mring; st.Kp = h->d_mring + (size_t)h->st.pair_stride * EKF_MERGE_BATCH_MAX; st.pcap = EKF_MERGE_BATCH_MAX;
    st.Gp32 = nullptr; st.Kp32 = nullptr;
    JointUpdateArgs u;
    u.n_mm = n_mm(h); u.cur = h->cur; u.np = (int32_t)np;
    TIMED(h, EKF_KERNEL_GATHER, launch_gather_joint(st, u, h->d_jblock, h->storage, h->stream));
    h->cur ^= 1;
    h->st.dcur ^= 1;
    h->hint_idx = -1;
    {
        // ONE pass for the np pairs, F64 arithmetic whatever cfg.pass_arith says: a float tile entry is rounded once
        next_pass_direction(h);
        st.dcur = h->st.dcur; st.tm = h->st.tm;
        TimedLaunch tl(h, EKF_KERNEL_DOWNDATE);
        const ekf_handle::WorkSet &ws = h->ws[h->ws_cur];
        PassJob job = {};
        job.dst = h->st.tiles;
        job.work = ws.work; job.nwork = ws.nwork; job.work_xcd = ws.xcd; job.xcd_len = ws.xcd_len;
        job.pstart = 0; job.npairs = (int)np;
        job.grid_cap = h->grid_cap; job.arith = EKF_ARITH_F64;
        job.aux = nullptr; job.nx = nullptr;
        HIPCHK(h, launch_downdate(st, job, h->storage, h->stream, h->dd_kernel));
        h->dd_pairs = (int32_t)np;
    }
    tiles_changed(h);
    return EKF_OK;
}
}  // namespace

extern "C" {
int32_t ekf_observe_model_joint(ekf_handle *h, const ekf_model_obs *obs, int64_t m, const int64_t *lm, double gate, ekf_joint_result *res,
                                double *nu, double *S) {
    if (!h) return EKF_ERR_INVALID_ARG;
    return observe_joint(h, "observe_model_joint: ", obs, m, lm, gate, nullptr, res, nu, S);
}
}  // extern "C"
