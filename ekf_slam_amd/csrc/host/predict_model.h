// Fragment of abi.hip, motion steps through a model with its true Jacobians (ekf_predict_model / ekf_motion_evaluate): an EAGER predict --
// a recorded ekf_predict is carried out first, then one launch for the whole chain at h->cur and the buffers flip.  Not an update-step: no
// wait, no flush, nothing of the pair ring; beside a pass in flight, since no tile is touched.  Sharded handles run it as they run
// ekf_predict: everything the launch reads and writes is replicated.
#pragma once
namespace {
// the steps, in the header's order, into the kernel's form; nothing of the handle is touched but its error text
int32_t predict_model_parse(ekf_handle *h, const std::string &who, const ekf_motion *steps, int64_t m, PredictModelArgs &a) {
    a = PredictModelArgs();
    a.m = (int32_t)m;
    for (int64_t b = 0; b < m; ++b) {
        const ekf_motion &o = steps[b];
        PredictModelStep &e = a.e[b];
        REQUIRE(h, o.model == EKF_MOTION_TURN_DRIVE || o.model == EKF_MOTION_ARC || o.model == EKF_MOTION_POSE_DELTA, EKF_ERR_INVALID_ARG,
                (who + "the model is EKF_MOTION_TURN_DRIVE, EKF_MOTION_ARC or EKF_MOTION_POSE_DELTA").c_str());
        REQUIRE(h, o.reserved == 0, EKF_ERR_INVALID_ARG, (who + "reserved must be 0").c_str());
        const int nu = o.model == EKF_MOTION_POSE_DELTA ? 3 : 2;
        for (int q = 0; q < nu; ++q) REQUIRE(h, std::isfinite(o.u[q]), EKF_ERR_INVALID_ARG, (who + "u is not finite").c_str());
        e.model = o.model;
        for (int q = 0; q < nu; ++q) e.u[q] = o.u[q];
        // M, column-major 3 x 3: the leading 2 x 2 block under ekf_observe_linear's rules for R ...
        const double M2[4] = { o.M[0], o.M[1], o.M[3], o.M[4] };
        double m00, m01, m10, m11;
        if (const char *bad = parse_R(M2, m00, m01, m10, m11)) return fail(h, EKF_ERR_INVALID_ARG, (who + "M: " + bad).c_str());
        e.m6[0] = m00; e.m6[1] = m10; e.m6[2] = m11;
        if (nu == 3) {
            // ... and, where the model has three inputs, the rest of positive semi-definiteness that can be tested exactly
            const double m20 = o.M[2], m21 = o.M[5], m22 = o.M[8];
            REQUIRE(h, std::isfinite(m20) && std::isfinite(m21) && std::isfinite(m22) && std::isfinite(o.M[6]) && std::isfinite(o.M[7]),
                    EKF_ERR_INVALID_ARG, (who + "M is not finite").c_str());
            const double det = m00 * (m11 * m22 - m21 * m21) - m10 * (m10 * m22 - m21 * m20) + m20 * (m10 * m21 - m11 * m20);
            REQUIRE(h, m20 == o.M[6] && m21 == o.M[7] && m22 >= 0.0 && m00 * m22 - m20 * m20 >= 0.0 && m11 * m22 - m21 * m21 >= 0.0 && det >= 0.0,
                    EKF_ERR_INVALID_ARG, (who + "M must be symmetric with non-negative diagonal, principal minors and determinant").c_str());
            e.m6[3] = m20; e.m6[4] = m21; e.m6[5] = m22;
        }
    }
    return EKF_OK;
}
}  // namespace

extern "C" {
int32_t ekf_predict_model(ekf_handle *h, const ekf_motion *steps, int64_t m) {
    if (!h) return EKF_ERR_INVALID_ARG;
    const std::string who = "predict_model: ";
    REQUIRE(h, steps != nullptr, EKF_ERR_INVALID_ARG, (who + "null steps").c_str());
    REQUIRE(h, m >= 1 && m <= EKF_PREDICT_MODEL_MAX, EKF_ERR_INVALID_ARG, (who + "between 1 and EKF_PREDICT_MODEL_MAX steps").c_str());
    PredictModelArgs a;
    TRY(predict_model_parse(h, who, steps, m, a));
    TRY(use_device(h));
    TRY(settle(h));
    REQUIRE(h, !h->pending, EKF_ERR_STATE, (who + "a sharded correction is between begin and finish").c_str());
    TRY(materialize_predict(h));           // a recorded ekf_predict came before this call: it happens before it
    a.n_mm = 2 * n_hi(h); a.cur = h->cur;
    TIMED(h, EKF_KERNEL_PREDICT, launch_predict_model(h->st, a, h->stream));
    h->cur ^= 1;
    return EKF_OK;
}

int32_t ekf_motion_evaluate(int32_t model, const double xr[3], const double u[3], double x_new[3], double F[9], double V[9]) {
    if (!xr || !u || !x_new || !F || !V) return EKF_ERR_INVALID_ARG;
    const double uu[3] = { u[0], u[1], model == EKF_MOTION_POSE_DELTA ? u[2] : 0.0 };
    double fa, fb, Vr[9];
    if (!ekfm::motion_eval(model, xr, uu, x_new, fa, fb, Vr)) return EKF_ERR_INVALID_ARG;
    for (int i = 0; i < 9; ++i) F[i] = (i % 4 == 0) ? 1.0 : 0.0;
    F[6] = fa; F[7] = fb;                                       // F(0,2), F(1,2), column-major
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) V[3 * c + r] = Vr[3 * r + c];
    return EKF_OK;
}
}  // extern "C"
