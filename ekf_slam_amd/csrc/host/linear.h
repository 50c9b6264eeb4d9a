// Fragment of abi.hip, linear observations (ekf_observe_linear / ekf_linear_innovation / ekf_linear_rejections): an UPDATE-STEP with the
// rungs of a map edit in front of it -- unsharded, settled -- but no flush: the pair goes to the pending ring through finish_step.
#pragma once
namespace {
// the handle's part: one record per entry point on the device and in pinned memory, the two counters, the event behind a record's readback
int32_t create_linear(ekf_handle *h) {
    HIPCHK(h, dalloc(h, &h->d_linrec, (size_t)2 * kLinearRecordDoubles));
    HIPCHK(h, dalloc(h, &h->d_lincnt, 2));
    HIPCHK(h, halloc(h, &h->h_linrec, (2 * kLinearRecordDoubles + 2) * sizeof(double), hipHostMallocDefault));
    return new_event(h, &h->ev_linrec) == hipSuccess ? EKF_OK : fail(h, EKF_ERR_HIP, "create: the linear observation's event");
}

// The noise covariance of `rows` observed rows, row-major into out: two rows through parse_R; one row as the pair with the exactly empty
// second row (R01 = R10 = 0, R11 = 1).  Then the gate.  (model.h's model_parse uses both.)
int32_t parse_R_rows(ekf_handle *h, const std::string &who, int rows, const double *R, double out[4]) {
    if (rows == 2) {
        if (const char *bad = parse_R(R, out[0], out[1], out[2], out[3])) return fail(h, EKF_ERR_INVALID_ARG, (who + bad).c_str());
        return EKF_OK;
    }
    out[0] = R[0]; out[1] = out[2] = 0.0; out[3] = 1.0;
    REQUIRE(h, std::isfinite(out[0]), EKF_ERR_INVALID_ARG, (who + "R is not finite").c_str());
    REQUIRE(h, out[0] >= 0.0, EKF_ERR_INVALID_ARG, (who + "R must be symmetric with non-negative diagonal and determinant").c_str());
    return EKF_OK;
}
int32_t parse_gate(ekf_handle *h, const std::string &who, double gate, double &out) {
    REQUIRE(h, !std::isnan(gate), EKF_ERR_INVALID_ARG, (who + "the gate is NaN").c_str());
    out = gate;
    return EKF_OK;
}

// Arguments of both entry points, in the header's order, into the kernel's form (row-major H over robot | lm[0] | lm[1], R row-major;
// rows == 1: the exactly empty second row).  The landmark rows are filled in once N is exact (linear_rungs).
int32_t linear_parse(ekf_handle *h, const std::string &who, const ekf_linear_obs *obs, LinearArgs &a) {
    REQUIRE(h, obs != nullptr, EKF_ERR_INVALID_ARG, (who + "null observation").c_str());
    REQUIRE(h, obs->rows == 1 || obs->rows == 2, EKF_ERR_INVALID_ARG, (who + "rows is 1 or 2").c_str());
    const int rows = obs->rows;
    a = LinearArgs();
    bool finite = true;
    for (int r = 0; r < rows; ++r) {
        finite = finite && std::isfinite(obs->z[r]);
        a.z[r] = obs->z[r];
        for (int t = 0; t < 3; ++t) { a.H[7 * r + t] = obs->Hr[2 * t + r]; finite = finite && std::isfinite(obs->Hr[2 * t + r]); }
        for (int b = 0; b < 2; ++b) {
            if (obs->lm[b] == -1) continue;
            for (int c = 0; c < 2; ++c) { a.H[7 * r + 3 + 2 * b + c] = obs->Hl[b][2 * c + r]; finite = finite && std::isfinite(obs->Hl[b][2 * c + r]); }
        }
        a.wrap[r] = obs->wrap_deg[r] != 0;
    }
    REQUIRE(h, finite, EKF_ERR_INVALID_ARG, (who + "z or H is not finite").c_str());
    TRY(parse_R_rows(h, who, rows, obs->R, a.R));
    TRY(parse_gate(h, who, obs->gate, a.gate));
    REQUIRE(h, !(obs->lm[0] >= 0 && obs->lm[0] == obs->lm[1]), EKF_ERR_INVALID_ARG, (who + "the two landmarks must differ").c_str());
    REQUIRE(h, obs->lm[0] >= -1 && obs->lm[1] >= -1, EKF_ERR_INVALID_ARG, (who + "a landmark is -1 (none) or a 0-based index").c_str());
    return EKF_OK;
}

// ... then the rungs: unsharded, settled (N exact), the indices, a recorded predict carried out, the work lists of the current map
// (A: LinearArgs, or model.h's ModelArgs; lm: the observation's two landmarks, -1 = none)
template <typename A>
int32_t linear_rungs(ekf_handle *h, const std::string &who, const int64_t lm[2], A &a) {
    TRY(edit_unsharded(h, who, "a landmark block needs that landmark's row-panel exchanged between the shards (a fix of the robot state "
                       "alone would not: its operands are replicated)"));
    TRY(edit_settled(h, who));
    for (int b = 0; b < 2; ++b) {
        REQUIRE(h, lm[b] < h->N, EKF_ERR_INDEX, (who + "landmark index outside the state").c_str());
        a.a[b] = lm[b] >= 0 ? 2 * lm[b] : -1;
    }
    TRY(materialize_predict(h));
    TRY(refresh_work(h));
    a.n_mm = n_mm(h); a.cur = h->cur; a.npend = h->npend; a.pstart = h->pstart;
    return EKF_OK;
}

void linear_fill(const double *rec, ekf_linear_result *res) {
    res->S[0] = rec[0]; res->S[1] = rec[2]; res->S[2] = rec[1]; res->S[3] = rec[3];       // column-major
    res->nu[0] = rec[4]; res->nu[1] = rec[5];
    res->d2 = rec[6];
    res->outcome = (int32_t)rec[7];
}

// The update-step behind ekf_observe_linear and ekf_observe_model, after the rungs.  gather_launch(rec, cnt) is the launch on h->stream.
// No flush: the launch reads its tile operands patched with the pending pairs and writes its own into the next ring slot.
template <typename Launch>
int32_t observe_step(ekf_handle *h, const std::string &who, ekf_linear_result *res, const char *irregular_message, Launch gather_launch) {
    TIMED(h, EKF_KERNEL_GATHER, gather_launch(h->d_linrec, h->d_lincnt));
    if (res) {
        HIPCHK(h, hipMemcpyAsync(h->h_linrec, h->d_linrec, kLinearRecordDoubles * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipEventRecord(h->ev_linrec, h->stream));
    }
    TRY(finish_step(h));
    if (!res) return EKF_OK;
    HIPCHK(h, hipEventSynchronize(h->ev_linrec));      // the launch's record alone: a pass that finish_step started is not waited for
    linear_fill(h->h_linrec, res);
    REQUIRE(h, res->outcome != EKF_LINEAR_IRREGULAR, EKF_ERR_STATE, (who + irregular_message).c_str());
    return EKF_OK;
}

// ... and the probe behind the two *_innovation entry points: probe_launch(rec) into the record's second slot, read back and waited for
template <typename Launch>
int32_t probe_step(ekf_handle *h, ekf_linear_result *res, Launch probe_launch) {
    double *d_rec = h->d_linrec + kLinearRecordDoubles, *h_rec = h->h_linrec + kLinearRecordDoubles;
    HIPCHK(h, probe_launch(d_rec));
    HIPCHK(h, hipMemcpyAsync(h_rec, d_rec, kLinearRecordDoubles * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    linear_fill(h_rec, res);
    return EKF_OK;
}
}  // namespace

extern "C" {
int32_t ekf_observe_linear(ekf_handle *h, const ekf_linear_obs *obs, ekf_linear_result *res) {
    if (!h) return EKF_ERR_INVALID_ARG;
    const std::string who = "observe_linear: ";
    LinearArgs a;
    TRY(linear_parse(h, who, obs, a));
    TRY(linear_rungs(h, who, obs->lm, a));
    return observe_step(h, who, res, "S = H P H' + R is not positive definite (an observation of something already known exactly, with R = 0?); "
                        "nothing was changed",
                        [&](double *rec, int64_t *cnt) { return launch_gather_linear(h->st, a, rec, cnt, h->storage, h->stream); });
}

int32_t ekf_linear_innovation(ekf_handle *h, const ekf_linear_obs *obs, ekf_linear_result *res) {
    if (!h) return EKF_ERR_INVALID_ARG;
    const std::string who = "linear_innovation: ";
    LinearArgs a;
    TRY(linear_parse(h, who, obs, a));
    REQUIRE(h, res != nullptr, EKF_ERR_INVALID_ARG, (who + "null result").c_str());
    TRY(linear_rungs(h, who, obs->lm, a));
    return probe_step(h, res, [&](double *rec) { return launch_linear_probe(h->st, a, rec, h->storage, h->stream); });
}

int32_t ekf_linear_rejections(ekf_handle *h, int64_t *irregular, int64_t *gated) {
    if (!h) return EKF_ERR_INVALID_ARG;
    TRY(use_device(h));
    int64_t *cnt = reinterpret_cast<int64_t *>(h->h_linrec + 2 * kLinearRecordDoubles);
    HIPCHK(h, hipMemcpyAsync(cnt, h->d_lincnt, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemsetAsync(h->d_lincnt, 0, 2 * sizeof(int64_t), h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (irregular) *irregular = cnt[0];
    if (gated) *gated = cnt[1];
    return EKF_OK;
}
}  // extern "C"
