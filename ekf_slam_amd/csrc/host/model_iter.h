// Fragment of abi.hip, model observations relinearised on the device (ekf_observe_model_iterated / ekf_model_innovation_iterated /
// ekf_model_iterate): model.h's update-step and probe -- their parse, rungs, record, counters and event -- with the loop's two controls and
// a second record beside the first.
#pragma once
namespace {
// the handle's part: the iteration record of the update-step, then the probe's, on the device and in pinned memory
int32_t create_model_iter(ekf_handle *h) {
    HIPCHK(h, dalloc(h, &h->d_itrec, (size_t)2 * kIterRecordDoubles));
    HIPCHK(h, halloc(h, &h->h_itrec, 2 * kIterRecordDoubles * sizeof(double), hipHostMallocDefault));
    return EKF_OK;
}

int32_t iter_parse(ekf_handle *h, const std::string &who, const ekf_model_obs *obs, int32_t iterations, double tol, IterModelArgs &a) {
    ModelArgs m;
    TRY(model_parse(h, who, obs, m));
    REQUIRE(h, iterations >= 1 && iterations <= EKF_MODEL_ITER_MAX, EKF_ERR_INVALID_ARG, (who + "iterations is 1 .. EKF_MODEL_ITER_MAX").c_str());
    REQUIRE(h, tol >= 0.0, EKF_ERR_INVALID_ARG, (who + "tol is a number >= 0").c_str());          // (a NaN fails the comparison)
    a = IterModelArgs();
    static_cast<ModelArgs &>(a) = m;
    a.iterations = iterations;
    a.tol = tol;
    return EKF_OK;
}

void iter_fill(const double *rec, ekf_iterated_result *it) {
    it->S[0] = rec[0]; it->S[1] = rec[2]; it->S[2] = rec[1]; it->S[3] = rec[3];               // column-major, as ekf_linear_result's
    it->nu[0] = rec[4]; it->nu[1] = rec[5];
    it->used = (int32_t)rec[6];
    it->converged = (int32_t)rec[7];
    it->last_step = rec[8];
    for (int k = 0; k < 7; ++k) it->x_local[k] = rec[9 + k];
}
}  // namespace

extern "C" {
int32_t ekf_observe_model_iterated(ekf_handle *h, const ekf_model_obs *obs, int32_t iterations, double tol, ekf_linear_result *first,
                                   ekf_iterated_result *it) {
    if (!h) return EKF_ERR_INVALID_ARG;
    const std::string who = "observe_model_iterated: ";
    IterModelArgs a;
    TRY(iter_parse(h, who, obs, iterations, tol, a));
    REQUIRE(h, first != nullptr || it == nullptr, EKF_ERR_INVALID_ARG, (who + "the iteration record is read back only with the first one (it without first)").c_str());
    TRY(linear_rungs(h, who, obs->lm, a));
    // the second record's copy is queued behind the launch and in front of the event observe_step waits for
    const int32_t rc = observe_step(h, who, first, "the target lies on the point it is observed from at one of the iterates (or the state is not "
                                    "finite), or S = H P H' + R is not positive definite there; nothing was changed",
                                    [&](double *rec, int64_t *cnt) {
                                        hipError_t e = launch_gather_model_iter(h->st, a, rec, cnt, h->d_itrec, h->storage, h->stream);
                                        if (e == hipSuccess && it)
                                            e = hipMemcpyAsync(h->h_itrec, h->d_itrec, kIterRecordDoubles * 8, hipMemcpyDeviceToHost, h->stream);
                                        return e;
                                    });
    if (it && first && (rc == EKF_OK || (rc == EKF_ERR_STATE && first->outcome == EKF_LINEAR_IRREGULAR))) iter_fill(h->h_itrec, it);
    return rc;
}

int32_t ekf_model_innovation_iterated(ekf_handle *h, const ekf_model_obs *obs, int32_t iterations, double tol, ekf_linear_result *first,
                                      ekf_iterated_result *it) {
    if (!h) return EKF_ERR_INVALID_ARG;
    const std::string who = "model_innovation_iterated: ";
    IterModelArgs a;
    TRY(iter_parse(h, who, obs, iterations, tol, a));
    REQUIRE(h, first != nullptr, EKF_ERR_INVALID_ARG, (who + "null result").c_str());
    TRY(linear_rungs(h, who, obs->lm, a));
    double *d_it = h->d_itrec + kIterRecordDoubles, *h_it = h->h_itrec + kIterRecordDoubles;
    TRY(probe_step(h, first, [&](double *rec) {
        hipError_t e = launch_model_iter_probe(h->st, a, rec, d_it, h->storage, h->stream);
        if (e == hipSuccess && it) e = hipMemcpyAsync(h_it, d_it, kIterRecordDoubles * 8, hipMemcpyDeviceToHost, h->stream);
        return e;
    }));
    if (it) iter_fill(h_it, it);
    return EKF_OK;
}

int32_t ekf_model_iterate(int32_t model, const double sm[38], const double anchor[2], int32_t has_landmark, const double z[2], const double R[4],
                          double gate, int32_t iterations, double tol, ekf_linear_result *first, ekf_iterated_result *it) {
    if (model < EKF_MODEL_RANGE_BEARING || model > EKF_MODEL_LANDMARK_RANGE || !sm || !anchor || !z || !R || !first) return EKF_ERR_INVALID_ARG;
    if (iterations < 1 || iterations > EKF_MODEL_ITER_MAX || !(tol >= 0.0) || std::isnan(gate)) return EKF_ERR_INVALID_ARG;
    double H[14], Gs[14], S[4], r[2], rec[kLinearRecordDoubles], itrec[kIterRecordDoubles];
    ekfm::ModelIterate mi;
    const double Rr[4] = { R[0], R[2], R[1], R[3] };                                              // column-major in, row-major inside
    const int outcome = ekfm::model_iterate(model, sm, anchor, has_landmark != 0, z, Rr, gate, iterations, tol, H, Gs, S, r, mi);
    for (int q = 0; q < 4; ++q) { rec[q] = mi.S0[q]; itrec[q] = S[q]; }
    rec[4] = mi.nu0[0]; rec[5] = mi.nu0[1]; rec[6] = mi.d2; rec[7] = (double)outcome;
    itrec[4] = r[0]; itrec[5] = r[1]; itrec[6] = (double)mi.used; itrec[7] = (double)mi.converged; itrec[8] = mi.last_step;
    for (int k = 0; k < 7; ++k) itrec[9 + k] = mi.xi[k];
    linear_fill(rec, first);
    if (it) iter_fill(itrec, it);
    return EKF_OK;
}
}  // extern "C"
