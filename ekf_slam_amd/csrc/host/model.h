// Fragment of abi.hip, observations through a model (ekf_observe_model / ekf_model_innovation / ekf_model_evaluate): linear.h's
// update-step -- its rungs, its record, its counters, its event -- with the Jacobian left to the device, which has the live x.
#pragma once
namespace {
// Arguments of both entry points, in the header's order, into the kernel's form; the landmark rows are filled in once N is exact
// (linear_rungs).  A one-row model runs as the pair with the exactly empty second row (z1 = 0, R01 = R10 = 0, R11 = 1).
int32_t model_parse(ekf_handle *h, const std::string &who, const ekf_model_obs *obs, ModelArgs &a) {
    REQUIRE(h, obs != nullptr, EKF_ERR_INVALID_ARG, (who + "null observation").c_str());
    REQUIRE(h, obs->model >= EKF_MODEL_RANGE_BEARING && obs->model <= EKF_MODEL_LANDMARK_RANGE, EKF_ERR_INVALID_ARG,
            (who + "model is one of EKF_MODEL_*").c_str());
    const int rows = (obs->model == EKF_MODEL_RANGE_BEARING || obs->model == EKF_MODEL_RELATIVE_XY) ? 2 : 1;
    const bool pair = obs->model == EKF_MODEL_LANDMARK_RANGE;
    const bool anchored = !pair && obs->lm[0] == -1;
    a = ModelArgs();
    a.model = obs->model;
    bool finite = true;
    for (int r = 0; r < rows; ++r) { finite = finite && std::isfinite(obs->z[r]); a.z[r] = obs->z[r]; }
    if (anchored)
        for (int c = 0; c < 2; ++c) { finite = finite && std::isfinite(obs->anchor[c]); a.anchor[c] = obs->anchor[c]; }
    REQUIRE(h, finite, EKF_ERR_INVALID_ARG, (who + "z or the anchor is not finite").c_str());
    double r00, r01, r10, r11;
    if (rows == 2) {
        if (const char *bad = parse_R(obs->R, r00, r01, r10, r11)) return fail(h, EKF_ERR_INVALID_ARG, (who + bad).c_str());
    } else {
        r00 = obs->R[0]; r01 = r10 = 0.0; r11 = 1.0;
        REQUIRE(h, std::isfinite(r00), EKF_ERR_INVALID_ARG, (who + "R is not finite").c_str());
        REQUIRE(h, r00 >= 0.0, EKF_ERR_INVALID_ARG, (who + "R must be symmetric with non-negative diagonal and determinant").c_str());
    }
    a.R[0] = r00; a.R[1] = r01; a.R[2] = r10; a.R[3] = r11;
    REQUIRE(h, !std::isnan(obs->gate), EKF_ERR_INVALID_ARG, (who + "the gate is NaN").c_str());
    a.gate = obs->gate;
    if (pair) {
        REQUIRE(h, obs->lm[0] >= 0 && obs->lm[1] >= 0, EKF_ERR_INVALID_ARG, (who + "the landmark range names two landmarks (0-based)").c_str());
        REQUIRE(h, obs->lm[0] != obs->lm[1], EKF_ERR_INVALID_ARG, (who + "the two landmarks must differ").c_str());
    } else {
        REQUIRE(h, obs->lm[0] >= -1, EKF_ERR_INVALID_ARG, (who + "the target is a 0-based landmark, or -1 for the anchor").c_str());
        REQUIRE(h, obs->lm[1] == -1, EKF_ERR_INVALID_ARG, (who + "this model has one target: lm[1] is -1").c_str());
    }
    return EKF_OK;
}
}  // namespace

extern "C" {
int32_t ekf_observe_model(ekf_handle *h, const ekf_model_obs *obs, ekf_linear_result *res) {
    if (!h) return EKF_ERR_INVALID_ARG;
    const std::string who = "observe_model: ";
    ModelArgs a;
    TRY(model_parse(h, who, obs, a));
    TRY(linear_rungs(h, who, obs->lm, a));
    // no flush, as ekf_observe_linear; h(x) and H are formed by the launch, at the x that carries every pending pair
    TIMED(h, EKF_KERNEL_GATHER, launch_gather_model(h->st, a, h->d_linrec, h->d_lincnt, h->storage, h->stream));
    if (res) {
        HIPCHK(h, hipMemcpyAsync(h->h_linrec, h->d_linrec, kLinearRecordDoubles * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipEventRecord(h->ev_linrec, h->stream));
    }
    TRY(finish_step(h));
    if (!res) return EKF_OK;
    HIPCHK(h, hipEventSynchronize(h->ev_linrec));
    linear_fill(h->h_linrec, res);
    REQUIRE(h, res->outcome != EKF_LINEAR_IRREGULAR, EKF_ERR_STATE, (who + "the target lies on the point it is observed from (or the state is "
            "not finite), or S = H P H' + R is not positive definite; nothing was changed").c_str());
    return EKF_OK;
}

int32_t ekf_model_innovation(ekf_handle *h, const ekf_model_obs *obs, ekf_linear_result *res) {
    if (!h) return EKF_ERR_INVALID_ARG;
    const std::string who = "model_innovation: ";
    ModelArgs a;
    TRY(model_parse(h, who, obs, a));
    REQUIRE(h, res != nullptr, EKF_ERR_INVALID_ARG, (who + "null result").c_str());
    TRY(linear_rungs(h, who, obs->lm, a));
    double *d_rec = h->d_linrec + kLinearRecordDoubles, *h_rec = h->h_linrec + kLinearRecordDoubles;
    HIPCHK(h, launch_model_probe(h->st, a, d_rec, h->storage, h->stream));
    HIPCHK(h, hipMemcpyAsync(h_rec, d_rec, kLinearRecordDoubles * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    linear_fill(h_rec, res);
    return EKF_OK;
}

int32_t ekf_model_evaluate(int32_t model, const double xr[3], const double t0[2], const double t1[2], double hx[2], double H[14]) {
    if (model < EKF_MODEL_RANGE_BEARING || model > EKF_MODEL_LANDMARK_RANGE || !xr || !t0 || !hx || !H) return EKF_ERR_INVALID_ARG;
    if (model == EKF_MODEL_LANDMARK_RANGE && !t1) return EKF_ERR_INVALID_ARG;
    const double xs[7] = { xr[0], xr[1], xr[2], t0[0], t0[1], t1 ? t1[0] : 0.0, t1 ? t1[1] : 0.0 };
    return ekfm::model_eval(model, xs, t0, true, hx, H) ? EKF_OK : EKF_ERR_STATE;
}
}  // extern "C"
