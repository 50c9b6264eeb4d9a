// Fragment of abi.hip, landmarks that start from a model's inverse (ekf_append_model / ekf_model_invert): ekf_append's place in the order
// of a handle -- settled, no flush, beside a pass in flight -- with the position and the Jacobians left to the device, which has the live x_r,
// and a whole scan per launch.  Sharded handles run it as they run ekf_append: everything the launch reads is replicated.
#pragma once
namespace {
// the entries, in the header's order, into the kernel's form; nothing of the handle is touched but its error text
int32_t append_model_parse(ekf_handle *h, const std::string &who, const ekf_model_init *obs, int64_t m, AppendModelArgs &a) {
    a = AppendModelArgs();
    a.m = (int32_t)m;
    for (int64_t b = 0; b < m; ++b) {
        const ekf_model_init &o = obs[b];
        AppendModelEntry &e = a.e[b];
        REQUIRE(h, o.model == EKF_MODEL_RANGE_BEARING || o.model == EKF_MODEL_RELATIVE_XY, EKF_ERR_INVALID_ARG,
                (who + "a landmark starts from EKF_MODEL_RANGE_BEARING or EKF_MODEL_RELATIVE_XY (a one-row model does not determine a point)").c_str());
        REQUIRE(h, std::isfinite(o.z[0]) && std::isfinite(o.z[1]), EKF_ERR_INVALID_ARG, (who + "z is not finite").c_str());
        REQUIRE(h, o.model != EKF_MODEL_RANGE_BEARING || o.z[0] > 0.0, EKF_ERR_INVALID_ARG, (who + "a range must be positive").c_str());
        if (const char *bad = parse_R(o.R, e.R00, e.R01, e.R10, e.R11)) return fail(h, EKF_ERR_INVALID_ARG, (who + bad).c_str());
        e.z0 = o.z[0]; e.z1 = o.z[1]; e.signature = o.signature; e.model = o.model;
    }
    return EKF_OK;
}
}  // namespace

extern "C" {
int32_t ekf_append_model(ekf_handle *h, const ekf_model_init *obs, int64_t m, int64_t *first_idx) {
    if (!h) return EKF_ERR_INVALID_ARG;
    const std::string who = "append_model: ";
    REQUIRE(h, obs != nullptr, EKF_ERR_INVALID_ARG, (who + "null entries").c_str());
    REQUIRE(h, m >= 1 && m <= EKF_APPEND_MODEL_MAX, EKF_ERR_INVALID_ARG, (who + "between 1 and EKF_APPEND_MODEL_MAX entries").c_str());
    AppendModelArgs a;
    TRY(append_model_parse(h, who, obs, m, a));
    TRY(use_device(h));
    TRY(settle(h));
    REQUIRE(h, !h->pending, EKF_ERR_STATE, (who + "a sharded correction is between begin and finish").c_str());
    REQUIRE(h, h->N + m <= h->cap, EKF_ERR_CAPACITY, (who + "capacity_landmarks cannot take the whole batch; nothing was appended").c_str());
    TRY(materialize_predict(h));           // (folding a recorded predict into this launch is not built)
    // beside a pass in flight, as do_append: the new rows go to the store the main stream reads and are copied when the pass retires
    if (h->inflight) h->appended_inflight = true;
    a.N = h->N; a.cur = h->cur;
    TIMED(h, EKF_KERNEL_APPEND, launch_append_model(h->st, a, h->storage, h->stream));
    for (int64_t b = 0; b < m; ++b) note_append(h, obs[b].signature);
    if (first_idx) *first_idx = a.N;
    return EKF_OK;
}

int32_t ekf_model_invert(int32_t model, const double xr[3], const double z[2], double t[2], double Gx[6], double Gz[4]) {
    if (!xr || !z || !t || !Gx || !Gz) return EKF_ERR_INVALID_ARG;
    double gth[2];
    if (!ekfm::model_invert(model, xr, z, t, gth, Gz)) return EKF_ERR_INVALID_ARG;
    Gx[0] = 1.0; Gx[1] = 0.0; Gx[2] = gth[0];
    Gx[3] = 0.0; Gx[4] = 1.0; Gx[5] = gth[1];
    return EKF_OK;
}
}  // extern "C"
