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
    TRY(parse_R_rows(h, who, rows, obs->R, a.R));
    TRY(parse_gate(h, who, obs->gate, a.gate));
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
    // h(x) and H are formed by the launch, at the x that carries every pending pair
    return observe_step(h, who, res, "the target lies on the point it is observed from (or the state is not finite), or S = H P H' + R is not "
                        "positive definite; nothing was changed",
                        [&](double *rec, int64_t *cnt) { return launch_gather_model(h->st, a, rec, cnt, h->storage, h->stream); });
}

int32_t ekf_model_innovation(ekf_handle *h, const ekf_model_obs *obs, ekf_linear_result *res) {
    if (!h) return EKF_ERR_INVALID_ARG;
    const std::string who = "model_innovation: ";
    ModelArgs a;
    TRY(model_parse(h, who, obs, a));
    REQUIRE(h, res != nullptr, EKF_ERR_INVALID_ARG, (who + "null result").c_str());
    TRY(linear_rungs(h, who, obs->lm, a));
    return probe_step(h, res, [&](double *rec) { return launch_model_probe(h->st, a, rec, h->storage, h->stream); });
}

int32_t ekf_model_evaluate(int32_t model, const double xr[3], const double t0[2], const double t1[2], double hx[2], double H[14]) {
    if (model < EKF_MODEL_RANGE_BEARING || model > EKF_MODEL_LANDMARK_RANGE || !xr || !t0 || !hx || !H) return EKF_ERR_INVALID_ARG;
    if (model == EKF_MODEL_LANDMARK_RANGE && !t1) return EKF_ERR_INVALID_ARG;
    const double xs[7] = { xr[0], xr[1], xr[2], t0[0], t0[1], t1 ? t1[0] : 0.0, t1 ? t1[1] : 0.0 };
    return ekfm::model_eval(model, xs, t0, true, hx, H) ? EKF_OK : EKF_ERR_STATE;
}
}  // extern "C"
