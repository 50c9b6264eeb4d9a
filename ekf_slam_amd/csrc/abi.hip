// C ABI of libekfslam (include/ekfslam.h): handle, HBM buffers, launch sequencing, measure() dispatch.
// No torch types, no exceptions across the boundary.  There is NO CPU fallback: without a HIP device
// ekf_create fails with EKF_ERR_NO_DEVICE.
// ONE host translation unit, split by family into host/*.h; below them the entry points that belong to no family.
#include "host/handle.h"       // ekf_handle, errors, the registries of device memory / pinned memory / events, TimedLaunch
#include "host/invalidate.h"   // one function per event that makes derived state stale
#include "host/exchange.h"     // the RCCL binding, the all-gather, ekf_exchange_* / ekf_comm_* / ekf_shard_*
#include "host/passes.h"       // refresh_work, retire_inflight, flush_pending, batch_complete
#include "host/steps.h"        // predict, append, correct, finish_step; correct / prefetch _begin / _finish
#include "host/assoc.h"        // verify_loop, the waited and the speculated association, the lookups
#include "host/measure.h"      // ekf_measure
#include "host/edits.h"        // remove, constrain / merge / distance, nearest
#include "host/linear.h"       // linear observations as update-steps: observe_linear, linear_innovation, linear_rejections
#include "host/model.h"        // ... through a model linearised on the device: observe_model, model_innovation, model_evaluate
#include "host/model_iter.h"   // ... relinearised on the device, the iterated EKF update: observe_model_iterated, model_innovation_iterated, model_iterate
#include "host/append_model.h" // landmarks that start from such a model's inverse, a scan per launch: append_model, model_invert
#include "host/join_map.h"     // a local submap joined into the map, its own cross-covariances kept: join_map
#include "host/extract_map.h"  // part of the map taken out into another handle, in the map frame or the robot frame: extract_map
#include "host/transform_map.h" // the whole map moved into another frame, in place: transform_map
#include "host/factor_map.h"   // the Cholesky factorisation of P in a scratch store -- definiteness, log det, NEES: factor_map
#include "host/multiply_map.h" // the plain product P B on the handle's own tile store, no factorisation: multiply_map
#include "host/associate_model.h" // which landmark a sighting belongs to, a scan per call: associate_model
#include "host/assign_model.h" // ... and the scan assigned to the map one-to-one: assign_model
#include "host/model_assigned.h" // ... and assigned, then applied step by step with no wait between: observe_model_assigned, assigned_scan_result
#include "host/joint.h"        // ... and a whole scan's pairings judged jointly, nh hypotheses per call: joint_innovation
#include "host/joint_search.h" // ... and searched on the device for the jointly compatible hypothesis, one readback: joint_search
#include "host/joint_update.h" // ... and applied as ONE joint update behind a flush: observe_model_joint
#include "host/joint_iter.h"   // ... relinearised: observe_model_joint_iterated, joint_iterate
#include "host/dense_obs.h"    // a linear observation with a dense H: multiply_map's product, then joint_update's route: observe_dense, observe_dense_innovation
#include "host/predict_model.h"// motion steps with true Jacobians, a chain per launch: predict_model, motion_evaluate
#include "host/state.h"        // get / set, low-rank load, checkpoint, digest
#include "host/lifecycle.h"    // ekf_create, ekf_destroy, the kernel timers

extern "C" {
int32_t ekf_abi_version(void) { return EKF_ABI_VERSION; }

const char *ekf_status_string(int32_t s) {
    switch (s) {
        case EKF_OK: return "ok";
        case EKF_ERR_INVALID_ARG: return "invalid argument";
        case EKF_ERR_NO_DEVICE: return "no HIP device";
        case EKF_ERR_HIP: return "HIP runtime error";
        case EKF_ERR_CAPACITY: return "landmark capacity exhausted";
        case EKF_ERR_INDEX: return "landmark index outside the state";
        case EKF_ERR_LOOKUP: return "landmark table lookup did not match exactly one entry";
        case EKF_ERR_STATE: return "call not valid in the current state";
        case EKF_ERR_COMM: return "multi-GPU exchange failed";
        default: return "unknown status";
    }
}

int32_t ekf_config_default(ekf_config *cfg, int32_t mode) {
    if (!cfg || (mode != EKF_MODE_KNOWN && mode != EKF_MODE_UC)) return EKF_ERR_INVALID_ARG;
    memset(cfg, 0, sizeof *cfg);
    cfg->C = 0.2;                                     // EKF_SLAM.m:12
    cfg->Rc[0] = mode == EKF_MODE_KNOWN ? .01 : .1;   // EKF_SLAM.m:13 / EKF_SLAM_UC.m:13
    cfg->Rc[1] = 5;
    cfg->s_cost = .00000000001;                       // EKF_SLAM.m:14 / EKF_SLAM_UC.m:16
    cfg->s_thresh = 1000000000;                       // EKF_SLAM.m:16 / EKF_SLAM_UC.m:16
    cfg->w_pos = 0.0;                                 // Correspondence.m:75 is the live line
    cfg->capacity_landmarks = 1024;
    cfg->mode = mode;
    cfg->storage = EKF_STORE_F64;
    cfg->device = 0;
    cfg->tile = 0;
    cfg->rank = 0;
    cfg->world = 1;
    cfg->batch = 1;
    cfg->async_flush = 0;
    cfg->device_assoc = mode == EKF_MODE_UC ? 3 : 0;   // unknown correspondence: the association runs, and is consumed, on the device
    return EKF_OK;
}

const char *ekf_last_error(const ekf_handle *h) { return h ? h->err.c_str() : "null handle"; }

int32_t ekf_set_stream(ekf_handle *h, void *hip_stream) {
    if (!h) return EKF_ERR_INVALID_ARG;
    TRY(enter(h));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->stream = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
    return EKF_OK;
}

int32_t ekf_sync(ekf_handle *h) {
    if (!h) return EKF_ERR_INVALID_ARG;
    TRY(enter(h));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (h->flush_stream) HIPCHK(h, hipStreamSynchronize(h->flush_stream));
    return EKF_OK;
}

int32_t ekf_flush(ekf_handle *h) {
    if (!h) return EKF_ERR_INVALID_ARG;
    REQUIRE(h, !h->pending, EKF_ERR_STATE, "flush: a sharded correction is between begin and finish");
    int32_t rc = use_device(h);
    if (!rc) rc = settle(h);
    return rc ? rc : flush_pending(h);
}

int32_t ekf_pending(ekf_handle *h, int32_t *npending) {
    if (!h || !npending) return EKF_ERR_INVALID_ARG;
    *npending = h->npend;
    return EKF_OK;
}

int32_t ekf_set_params(ekf_handle *h, double C, const double Rc[2], double s_cost, double s_thresh, double w_pos) {
    if (!h || !Rc) return fail(h, EKF_ERR_INVALID_ARG, "set_params: null argument");
    h->cfg.C = C; h->cfg.Rc[0] = Rc[0]; h->cfg.Rc[1] = Rc[1];
    h->cfg.s_cost = s_cost; h->cfg.s_thresh = s_thresh; h->cfg.w_pos = w_pos;
    return EKF_OK;
}

int32_t ekf_predict(ekf_handle *h, const double u[2]) {
    if (!h || !u) return fail(h, EKF_ERR_INVALID_ARG, "predict: null argument");
    int32_t rc = use_device(h);
    return rc ? rc : do_predict(h, u);
}

int32_t ekf_motion_model(const double *x, int64_t n, const double u[2], double *x_new, double *F) {
    if (!x || !u || !x_new || n < 3) return EKF_ERR_INVALID_ARG;
    const double th = x[2];
    for (int64_t i = 0; i < n; ++i) x_new[i] = x[i];
    x_new[0] = x[0] + u[0] * ekfm::cosd(th + u[1]);           // EKF_SLAM.m:58-60
    x_new[1] = x[1] + u[0] * ekfm::sind(th + u[1]);
    x_new[2] = th + u[1];
    if (F) {
        for (int64_t i = 0; i < n * n; ++i) F[i] = 0.0;
        for (int64_t i = 0; i < n; ++i) F[i * n + i] = 1.0;  // eye(n)
        F[2 * n + 0] = -1 * u[0] * ekfm::sind(th);           // F(1,3), column-major
        F[2 * n + 1] = u[0] * ekfm::cosd(th);                // F(2,3)
    }
    return EKF_OK;
}

int32_t ekf_append(ekf_handle *h, const double u[2], const double R[4], const double pos[2], double signature) {
    if (!h || !u || !R || !pos) return fail(h, EKF_ERR_INVALID_ARG, "append: null argument");
    int32_t rc = use_device(h);
    if (!rc) rc = settle(h);
    return rc ? rc : do_append(h, u, R, pos, signature);
}

int32_t ekf_correct(ekf_handle *h, const double z[2], const double R[4], int64_t idx) {
    if (!h || !z || !R) return fail(h, EKF_ERR_INVALID_ARG, "correct: null argument");
    int32_t rc = use_device(h);
    if (!rc) rc = settle(h);
    return rc ? rc : do_correct(h, z, R, idx);
}

int32_t ekf_associate(ekf_handle *h, const double z[3], const double R[4], int32_t *is_new, int64_t *idx,
                      double *pos_cost, double *sig_cost) {
    if (!h || !z || !R || !is_new || !idx) return fail(h, EKF_ERR_INVALID_ARG, "associate: null argument");
    int32_t rc = use_device(h);
    if (!rc) rc = settle(h);
    return rc ? rc : do_associate(h, z, R, is_new, idx, pos_cost, sig_cost);
}

int32_t ekf_hint_next(ekf_handle *h, int64_t idx) {
    if (!h) return EKF_ERR_INVALID_ARG;
    h->hint_idx = (idx >= 0 && idx < h->N) ? idx : -1;
    return EKF_OK;
}

int32_t ekf_num_landmarks(ekf_handle *h, int64_t *N) {
    if (!h || !N) return fail(h, EKF_ERR_INVALID_ARG, "num_landmarks: null argument");
    if (unsettled(h) > 0) TRY(settle(h));
    *N = h->N;
    return EKF_OK;
}

int32_t ekf_device_bytes(ekf_handle *h, int64_t *bytes) {
    if (!h || !bytes) return fail(h, EKF_ERR_INVALID_ARG, "device_bytes: null argument");
    *bytes = h->bytes;
    return EKF_OK;
}

const char *ekf_downdate_kernel_name(const ekf_handle *h, int32_t *pairs) {
    if (!h) return "";
    if (pairs) *pairs = h->dd_pairs;
    return h->dd_kernel;
}

int32_t ekf_downdate_algorithmic_bytes(ekf_handle *h, int64_t *bytes) {
    if (!h || !bytes) return fail(h, EKF_ERR_INVALID_ARG, "downdate_algorithmic_bytes: null argument");
    if (unsettled(h) > 0) TRY(settle(h));
    const int64_t n = 3 + n_mm(h);
    *bytes = (int64_t)elt_size(h) * n * (n + 1);
    return EKF_OK;
}
}  // extern "C"
