/*
 * MEX gateway: MATLAB -> C ABI (include/ekfslam.h) -> HIP.   NOT COMPILED AGAINST MATLAB IN THIS REPOSITORY'S IMAGE
 * (no MATLAB / MathWorks mex.h there); build on a MATLAB host with
 *     mex -I../include ekfslam_mex.c -L../ekf_slam_amd -lekfslam
 * What IS run here: tests/test_mex_gateway_cpu.py compiles this file against a small mock of the documented MEX C API and a
 * recording stand-in for libekfslam, and drives every command with the argument shapes the .m classes pass.
 *
 * One entry point, string command first:   out = ekfslam_mex('command', handle, args...)
 * The handle travels as a uint64 scalar.  MATLAB's 1-based landmark indices are converted to the ABI's
 * 0-based ones here.  Any non-zero status becomes mexErrMsgIdAndTxt('ekfslam:status', ...), so the .m classes
 * see MATLAB errors exactly where the reference's own code would raise them.
 *
 * Commands that take NO single handle ('create', 'f', and 'exchange_local', whose second argument is a uint64 VECTOR of handles
 * that it validates itself) are dispatched before anything looks at prhs[1] as a handle; every other command goes through
 * handle_of(), which rejects an empty / non-uint64 / null handle with a MATLAB error instead of dereferencing it.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "ekfslam.h"
#include "mex.h"

/* The map-editing entry points (ekf_remove_landmarks; ekf_constrain_landmarks, ekf_merge_landmarks, ekf_landmark_distance;
 * ekf_nearest_landmarks; ekf_merge_landmarks_batch) the linear observation (ekf_observe_linear), the model observation
 * (ekf_observe_model), the append through a model (ekf_append_model), the association of a scan under the models' conventions
 * (ekf_associate_model) and its one-to-one assignment (ekf_assign_model), the joint compatibility of a scan's pairings (ekf_joint_innovation) and their joint update
 * (ekf_observe_model_joint, relinearised: ekf_observe_model_joint_iterated), the relinearised model observation
 * (ekf_observe_model_iterated), the motion steps under them (ekf_predict_model), the join of a local map (ekf_join_map), the extraction of part of the map (ekf_extract_map), the map's change of frame (ekf_transform_map), the factorisation of P (ekf_factor_map), the draws from the posterior behind it (ekf_sample_map), the solves with the factor (ekf_solve_map) and the plain product P B (ekf_multiply_map) are the ones this gateway can live without: bound weakly, so that the gateway still links against a libekfslam (or a stand-in) that
 * predates them; their commands then raise a MATLAB error instead. */
#if defined(__GNUC__)
#pragma weak ekf_remove_landmarks
#pragma weak ekf_constrain_landmarks
#pragma weak ekf_merge_landmarks
#pragma weak ekf_landmark_distance
#pragma weak ekf_nearest_landmarks
#pragma weak ekf_merge_landmarks_batch
#pragma weak ekf_observe_linear
#pragma weak ekf_observe_model
#pragma weak ekf_append_model
#pragma weak ekf_associate_model
#pragma weak ekf_assign_model
#pragma weak ekf_predict_model
#pragma weak ekf_joint_innovation
#pragma weak ekf_joint_search
#pragma weak ekf_observe_model_iterated
#pragma weak ekf_observe_model_joint
#pragma weak ekf_observe_model_joint_iterated
#pragma weak ekf_join_map
#pragma weak ekf_extract_map
#pragma weak ekf_transform_map
#pragma weak ekf_factor_map
#pragma weak ekf_sample_map
#pragma weak ekf_solve_map
#pragma weak ekf_multiply_map
#pragma weak ekf_observe_dense
#define HAVE_REMOVE_LANDMARKS (ekf_remove_landmarks != 0)
#define HAVE_CONSTRAIN_LANDMARKS (ekf_constrain_landmarks != 0)
#define HAVE_MERGE_LANDMARKS (ekf_merge_landmarks != 0)
#define HAVE_LANDMARK_DISTANCE (ekf_landmark_distance != 0)
#define HAVE_NEAREST_LANDMARKS (ekf_nearest_landmarks != 0)
#define HAVE_MERGE_LANDMARKS_BATCH (ekf_merge_landmarks_batch != 0)
#define HAVE_OBSERVE_LINEAR (ekf_observe_linear != 0)
#define HAVE_OBSERVE_MODEL (ekf_observe_model != 0)
#define HAVE_APPEND_MODEL (ekf_append_model != 0)
#define HAVE_ASSOCIATE_MODEL (ekf_associate_model != 0)
#define HAVE_ASSIGN_MODEL (ekf_assign_model != 0)
#define HAVE_PREDICT_MODEL (ekf_predict_model != 0)
#define HAVE_JOINT_INNOVATION (ekf_joint_innovation != 0)
#define HAVE_JOINT_SEARCH (ekf_joint_search != 0)
#define HAVE_OBSERVE_MODEL_ITERATED (ekf_observe_model_iterated != 0)
#define HAVE_OBSERVE_MODEL_JOINT (ekf_observe_model_joint != 0)
#define HAVE_OBSERVE_MODEL_JOINT_ITERATED (ekf_observe_model_joint_iterated != 0)
#define HAVE_JOIN_MAP (ekf_join_map != 0)
#define HAVE_EXTRACT_MAP (ekf_extract_map != 0)
#define HAVE_TRANSFORM_MAP (ekf_transform_map != 0)
#define HAVE_FACTOR_MAP (ekf_factor_map != 0)
#define HAVE_SAMPLE_MAP (ekf_sample_map != 0)
#define HAVE_SOLVE_MAP (ekf_solve_map != 0)
#define HAVE_MULTIPLY_MAP (ekf_multiply_map != 0)
#define HAVE_OBSERVE_DENSE (ekf_observe_dense != 0)
#else
#define HAVE_REMOVE_LANDMARKS 1
#define HAVE_CONSTRAIN_LANDMARKS 1
#define HAVE_MERGE_LANDMARKS 1
#define HAVE_LANDMARK_DISTANCE 1
#define HAVE_NEAREST_LANDMARKS 1
#define HAVE_MERGE_LANDMARKS_BATCH 1
#define HAVE_OBSERVE_LINEAR 1
#define HAVE_OBSERVE_MODEL 1
#define HAVE_APPEND_MODEL 1
#define HAVE_ASSOCIATE_MODEL 1
#define HAVE_ASSIGN_MODEL 1
#define HAVE_PREDICT_MODEL 1
#define HAVE_JOINT_INNOVATION 1
#define HAVE_OBSERVE_MODEL_ITERATED 1
#define HAVE_OBSERVE_MODEL_JOINT 1
#define HAVE_OBSERVE_MODEL_JOINT_ITERATED 1
#define HAVE_JOIN_MAP 1
#define HAVE_EXTRACT_MAP 1
#define HAVE_TRANSFORM_MAP 1
#define HAVE_FACTOR_MAP 1
#define HAVE_SAMPLE_MAP 1
#define HAVE_SOLVE_MAP 1
#define HAVE_MULTIPLY_MAP 1
#define HAVE_OBSERVE_DENSE 1
#endif

static void need(int nrhs, int want, const char *cmd) {
    if (nrhs < want) mexErrMsgIdAndTxt("ekfslam:usage", "'%s' needs %d arguments, got %d", cmd, want, nrhs);
}

static ekf_handle *handle_of(int nrhs, const mxArray *prhs[]) {
    if (nrhs < 2 || !prhs[1] || mxGetClassID(prhs[1]) != mxUINT64_CLASS || mxGetNumberOfElements(prhs[1]) != 1 ||
        !mxGetData(prhs[1]))
        mexErrMsgIdAndTxt("ekfslam:handle", "second argument must be the uint64 handle returned by 'create'");
    ekf_handle *h = (ekf_handle *)(uintptr_t)(*(const uint64_t *)mxGetData(prhs[1]));
    if (!h) mexErrMsgIdAndTxt("ekfslam:handle", "null handle (already destroyed?)");
    return h;
}

static void check(ekf_handle *h, int32_t rc) {
    if (rc != EKF_OK)
        mexErrMsgIdAndTxt("ekfslam:status", "%s: %s", ekf_status_string(rc), h ? ekf_last_error(h) : "");
}

/* delta (2 elements) and R (2 x 2, column-major as MATLAB holds it) of the landmark-landmark commands */
static const double *two_of(const mxArray *a, const char *cmd, const char *what) {
    if (!a || mxGetNumberOfElements(a) != 2 || !mxGetPr(a)) mexErrMsgIdAndTxt("ekfslam:usage", "%s: %s needs 2 elements", cmd, what);
    return mxGetPr(a);
}
static const double *r2x2_of(const mxArray *a, const char *cmd) {
    if (!a || mxGetNumberOfElements(a) != 4 || !mxGetPr(a)) mexErrMsgIdAndTxt("ekfslam:usage", "%s: R needs 2 x 2 elements", cmd);
    return mxGetPr(a);
}

static int64_t nstate(ekf_handle *h) { int64_t N; check(h, ekf_num_landmarks(h, &N)); return 3 + 2 * N; }

/* The scan and its pairings of observe_model_joint and observe_model_joint_iterated, checked and unpacked ONCE: prhs[2..6] = model m x 1,
 * z m x 2, R 2 x 2 x m, lm m x 1 (1-based, 0 = left out), gate.  Returns m. */
static mwSize joint_scan(const char *cmd, const mxArray *prhs[], ekf_model_obs o[EKF_JOINT_MAX], int64_t lm[EKF_JOINT_MAX]) {
    const mwSize m = prhs[2] ? mxGetNumberOfElements(prhs[2]) : 0;
    if (m < 1 || m > EKF_JOINT_MAX) mexErrMsgIdAndTxt("ekfslam:usage", "%s: between 1 and %d observations in one call", cmd, EKF_JOINT_MAX);
    if (!mxGetPr(prhs[2]) || !prhs[3] || mxGetM(prhs[3]) != m || mxGetNumberOfElements(prhs[3]) != 2 * m || !mxGetPr(prhs[3]))
        mexErrMsgIdAndTxt("ekfslam:usage", "%s: z needs m x 2 elements, one row per entry of model", cmd);
    if (!prhs[4] || mxGetNumberOfElements(prhs[4]) != 4 * m || !mxGetPr(prhs[4]))
        mexErrMsgIdAndTxt("ekfslam:usage", "%s: R needs 2 x 2 x m elements", cmd);
    if (!prhs[5] || mxGetNumberOfElements(prhs[5]) != m || !mxGetPr(prhs[5]))
        mexErrMsgIdAndTxt("ekfslam:usage", "%s: lm needs m elements, one per entry of model", cmd);
    if (!prhs[6] || mxGetNumberOfElements(prhs[6]) != 1 || !mxGetPr(prhs[6]))
        mexErrMsgIdAndTxt("ekfslam:usage", "%s: gate is one number (Inf: no gate)", cmd);
    for (mwSize k = 0; k < m; ++k) {
        o[k].model = (int32_t)mxGetPr(prhs[2])[k]; o[k].reserved = 0;
        o[k].z[0] = mxGetPr(prhs[3])[k]; o[k].z[1] = mxGetPr(prhs[3])[m + k];       /* column-major m x 2 */
        for (int q = 0; q < 4; ++q) o[k].R[q] = mxGetPr(prhs[4])[4 * k + q];
        o[k].lm[0] = o[k].lm[1] = -1;
        o[k].anchor[0] = o[k].anchor[1] = 0.0;
        o[k].gate = HUGE_VAL;
        const double v = mxGetPr(prhs[5])[k];                                       /* 1-based -> 0-based, 0 (left out) -> -1 */
        if (!(v >= 0.0 && v < 9.0e15 && (double)(int64_t)v == v))                   /* (no libm call: the gateway links without it) */
            mexErrMsgIdAndTxt("ekfslam:usage", "%s: lm holds landmark numbers (1-based), 0 = left out", cmd);
        lm[k] = (int64_t)v - 1;
    }
    return m;
}

void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[]) {
    char cmd[32];
    if (nrhs < 1 || mxGetString(prhs[0], cmd, sizeof cmd)) mexErrMsgIdAndTxt("ekfslam:usage", "command string expected");

    /* ---- commands without a handle ---- */
    if (!strcmp(cmd, "create")) {                 /* h = ekfslam_mex('create', mode, capacity [, tile [, batch [, device, rank, world [, storage [, pass_arith [, device_assoc]]]]]]) */
        ekf_config cfg;
        ekf_handle *h = NULL;
        need(nrhs, 3, cmd);
        check(NULL, ekf_config_default(&cfg, (int32_t)mxGetScalar(prhs[1])));
        cfg.capacity_landmarks = (int64_t)mxGetScalar(prhs[2]);
        if (nrhs > 3) cfg.tile = (int32_t)mxGetScalar(prhs[3]);
        if (nrhs > 4) cfg.batch = (int32_t)mxGetScalar(prhs[4]);      /* deferred downdate, same results */
        if (nrhs > 5) {                                               /* one shard of a filter split over several GPUs */
            need(nrhs, 8, cmd);
            cfg.device = (int32_t)mxGetScalar(prhs[5]);
            cfg.rank = (int32_t)mxGetScalar(prhs[6]);
            cfg.world = (int32_t)mxGetScalar(prhs[7]);
        }
        if (nrhs > 8) cfg.storage = (int32_t)mxGetScalar(prhs[8]);    /* EKF_STORE_*: 1 = float tiles (BASELINE configs[4]) */
        if (nrhs > 9) cfg.pass_arith = (int32_t)mxGetScalar(prhs[9]); /* EKF_ARITH_*: 1 = the pass over float tiles in F32 arithmetic, 2 = in split arithmetic */
        if (nrhs > 10) cfg.device_assoc = (int32_t)mxGetScalar(prhs[10]); /* include/ekfslam.h: 4 = the device-decided branch (any w_pos) */
        int32_t rc = ekf_create(&cfg, &h);
        if (rc != EKF_OK) {
            char msg[256];
            strncpy(msg, h ? ekf_last_error(h) : "", sizeof msg - 1); msg[sizeof msg - 1] = 0;
            if (h) ekf_destroy(h);
            mexErrMsgIdAndTxt("ekfslam:status", "%s: %s", ekf_status_string(rc), msg);
        }
        plhs[0] = mxCreateNumericMatrix(1, 1, mxUINT64_CLASS, mxREAL);
        *(uint64_t *)mxGetData(plhs[0]) = (uint64_t)(uintptr_t)h;
        mexLock();
        return;
    }
    if (!strcmp(cmd, "f")) {                      /* [x_new, F] = ekfslam_mex('f', [], x, u): pure host function, prhs[1] unused */
        need(nrhs, 4, cmd);
        mwSize n = mxGetNumberOfElements(prhs[2]);
        if (n < 3 || mxGetNumberOfElements(prhs[3]) < 2) mexErrMsgIdAndTxt("ekfslam:usage", "f: x needs >= 3 and u 2 elements");
        plhs[0] = mxCreateDoubleMatrix(1, n, mxREAL);
        mxArray *F = mxCreateDoubleMatrix(n, n, mxREAL);
        check(NULL, ekf_motion_model(mxGetPr(prhs[2]), (int64_t)n, mxGetPr(prhs[3]), mxGetPr(plhs[0]), mxGetPr(F)));
        if (nlhs > 1) plhs[1] = F; else mxDestroyArray(F);
        return;
    }

    if (!strcmp(cmd, "exchange_local")) {         /* ekfslam_mex('exchange_local', handles): all shards of ONE filter, uint64 vector,
                                                     each between the same *_begin and *_finish (include/ekfslam.h, transport (c)) */
        ekf_handle *hs[64];
        need(nrhs, 2, cmd);
        if (!prhs[1] || mxGetClassID(prhs[1]) != mxUINT64_CLASS || !mxGetData(prhs[1]))
            mexErrMsgIdAndTxt("ekfslam:handle", "exchange_local: a uint64 vector of handles expected");
        const mwSize w = mxGetNumberOfElements(prhs[1]);
        if (w < 1 || w > 64) mexErrMsgIdAndTxt("ekfslam:usage", "exchange_local: between 1 and 64 handles");
        for (mwSize r = 0; r < w; ++r) {
            hs[r] = (ekf_handle *)(uintptr_t)((const uint64_t *)mxGetData(prhs[1]))[r];
            if (!hs[r]) mexErrMsgIdAndTxt("ekfslam:handle", "exchange_local: null handle in the vector");
        }
        check(hs[0], ekf_exchange_local(hs, (int32_t)w));
        return;
    }

    /* ---- everything below operates on a live handle ---- */
    ekf_handle *h = handle_of(nrhs, prhs);
    if (!strcmp(cmd, "destroy")) { ekf_destroy(h); mexUnlock(); return; }
    if (!strcmp(cmd, "set_params")) {             /* (h, C, Rc, s_cost, s_thresh, w_pos) */
        need(nrhs, 7, cmd);
        check(h, ekf_set_params(h, mxGetScalar(prhs[2]), mxGetPr(prhs[3]), mxGetScalar(prhs[4]), mxGetScalar(prhs[5]), mxGetScalar(prhs[6])));
        return;
    }
    if (!strcmp(cmd, "predict")) { need(nrhs, 3, cmd); check(h, ekf_predict(h, mxGetPr(prhs[2]))); return; }
    if (!strcmp(cmd, "append"))  { need(nrhs, 6, cmd); check(h, ekf_append(h, mxGetPr(prhs[2]), mxGetPr(prhs[3]), mxGetPr(prhs[4]), mxGetScalar(prhs[5]))); return; }
    if (!strcmp(cmd, "correct")) { need(nrhs, 5, cmd); check(h, ekf_correct(h, mxGetPr(prhs[2]), mxGetPr(prhs[3]), (int64_t)mxGetScalar(prhs[4]) - 1)); return; }
    if (!strcmp(cmd, "associate")) {              /* [newLL, index] = ... (z 1x3, R 2x2) ; index 1-based */
        int32_t is_new; int64_t idx;
        need(nrhs, 4, cmd);
        check(h, ekf_associate(h, mxGetPr(prhs[2]), mxGetPr(prhs[3]), &is_new, &idx, NULL, NULL));
        plhs[0] = mxCreateLogicalScalar(is_new != 0);
        if (nlhs > 1) plhs[1] = mxCreateDoubleScalar((double)(idx + 1));
        return;
    }
    /* sharded handles driven by one host thread: begin on every shard, 'exchange_local', finish on every shard */
    if (!strcmp(cmd, "correct_begin")) { need(nrhs, 5, cmd); check(h, ekf_correct_begin(h, mxGetPr(prhs[2]), mxGetPr(prhs[3]), (int64_t)mxGetScalar(prhs[4]) - 1)); return; }
    if (!strcmp(cmd, "correct_finish")) { check(h, ekf_correct_finish(h)); return; }
    if (!strcmp(cmd, "hint_next")) { need(nrhs, 3, cmd); check(h, ekf_hint_next(h, (int64_t)mxGetScalar(prhs[2]) - 1)); return; }   /* idx 1-based */
    if (!strcmp(cmd, "associate_begin")) {        /* (h, z 1x3, R 2x2): candidates of this shard into its send area */
        need(nrhs, 4, cmd);
        check(h, ekf_associate_begin(h, mxGetPr(prhs[2]), mxGetPr(prhs[3]), 0));
        return;
    }
    if (!strcmp(cmd, "associate_finish")) {       /* [newLL, index] = ...; index 1-based */
        int32_t is_new; int64_t idx;
        check(h, ekf_associate_finish(h, &is_new, &idx, NULL, NULL));
        plhs[0] = mxCreateLogicalScalar(is_new != 0);
        if (nlhs > 1) plhs[1] = mxCreateDoubleScalar((double)(idx + 1));
        return;
    }
    if (!strcmp(cmd, "flush")) { check(h, ekf_flush(h)); return; }
    if (!strcmp(cmd, "remove_landmarks")) {       /* (h, idx): landmark numbers, 1-based like 'correct', any order, any shape */
        need(nrhs, 3, cmd);
        if (!HAVE_REMOVE_LANDMARKS) mexErrMsgIdAndTxt("ekfslam:usage", "remove_landmarks: this libekfslam has no ekf_remove_landmarks");
        const mwSize m = mxGetNumberOfElements(prhs[2]);
        int64_t *idx0 = (int64_t *)malloc((m ? m : 1) * sizeof(int64_t));       /* freed before any MATLAB error can unwind */
        if (!idx0) mexErrMsgIdAndTxt("ekfslam:usage", "remove_landmarks: out of memory");
        for (mwSize i = 0; i < m; ++i) idx0[i] = (int64_t)mxGetPr(prhs[2])[i] - 1;
        const int32_t rc = ekf_remove_landmarks(h, idx0, (int64_t)m);
        free(idx0);
        check(h, rc);
        return;
    }
    if (!strcmp(cmd, "constrain_landmarks")) {    /* (h, i, j, delta 2x1, R 2x2): landmark numbers 1-based like 'correct' */
        need(nrhs, 6, cmd);
        if (!HAVE_CONSTRAIN_LANDMARKS) mexErrMsgIdAndTxt("ekfslam:usage", "constrain_landmarks: this libekfslam has no ekf_constrain_landmarks");
        check(h, ekf_constrain_landmarks(h, (int64_t)mxGetScalar(prhs[2]) - 1, (int64_t)mxGetScalar(prhs[3]) - 1, two_of(prhs[4], cmd, "delta"),
                                         r2x2_of(prhs[5], cmd)));
        return;
    }
    if (!strcmp(cmd, "merge_landmarks")) {        /* (h, keep, drop, R 2x2) */
        need(nrhs, 5, cmd);
        if (!HAVE_MERGE_LANDMARKS) mexErrMsgIdAndTxt("ekfslam:usage", "merge_landmarks: this libekfslam has no ekf_merge_landmarks");
        check(h, ekf_merge_landmarks(h, (int64_t)mxGetScalar(prhs[2]) - 1, (int64_t)mxGetScalar(prhs[3]) - 1, r2x2_of(prhs[4], cmd)));
        return;
    }
    if (!strcmp(cmd, "landmark_distance")) {      /* [d2, S] = (h, i, j, delta 2x1, R 2x2) */
        double d2 = 0.0;
        need(nrhs, 6, cmd);
        if (!HAVE_LANDMARK_DISTANCE) mexErrMsgIdAndTxt("ekfslam:usage", "landmark_distance: this libekfslam has no ekf_landmark_distance");
        const double *delta = two_of(prhs[4], cmd, "delta"), *R = r2x2_of(prhs[5], cmd);
        mxArray *S = mxCreateDoubleMatrix(2, 2, mxREAL);
        const int32_t rc = ekf_landmark_distance(h, (int64_t)mxGetScalar(prhs[2]) - 1, (int64_t)mxGetScalar(prhs[3]) - 1, delta, R, &d2, mxGetPr(S));
        if (rc != EKF_OK) { mxDestroyArray(S); check(h, rc); }
        plhs[0] = mxCreateDoubleScalar(d2);
        if (nlhs > 1) plhs[1] = S; else mxDestroyArray(S);
        return;
    }
    if (!strcmp(cmd, "nearest_landmarks")) {      /* [d2, partner] = (h, R 2x2): N x 1 each; partner 1-based, 0 = none */
        need(nrhs, 3, cmd);
        if (!HAVE_NEAREST_LANDMARKS) mexErrMsgIdAndTxt("ekfslam:usage", "nearest_landmarks: this libekfslam has no ekf_nearest_landmarks");
        const double *R = r2x2_of(prhs[2], cmd);
        const int64_t N = (nstate(h) - 3) / 2;
        int64_t *p0 = (int64_t *)malloc((size_t)(N ? N : 1) * sizeof(int64_t));  /* freed before any MATLAB error can unwind */
        if (!p0) mexErrMsgIdAndTxt("ekfslam:usage", "nearest_landmarks: out of memory");
        mxArray *d2 = mxCreateDoubleMatrix((mwSize)N, 1, mxREAL), *partner = mxCreateDoubleMatrix((mwSize)N, 1, mxREAL);
        const int32_t rc = ekf_nearest_landmarks(h, R, mxGetPr(d2), p0);
        if (rc == EKF_OK)
            for (int64_t i = 0; i < N; ++i) mxGetPr(partner)[i] = (double)(p0[i] + 1);       /* -1 (none) -> 0 */
        free(p0);
        if (rc != EKF_OK) { mxDestroyArray(d2); mxDestroyArray(partner); check(h, rc); }
        plhs[0] = d2;
        if (nlhs > 1) plhs[1] = partner; else mxDestroyArray(partner);
        return;
    }
    if (!strcmp(cmd, "observe_linear")) {         /* res = (h, z 2, R 2x2, Hr 2x3, lm 0..2 numbers (1-based), Hl 2x2xk, gate, wrap 2, rows, wait):
                                                     wait ~= 0: res = [nu(1) nu(2) S(1,1) S(2,1) S(1,2) S(2,2) d2 outcome]; else [] and nothing waits */
        ekf_linear_obs o;
        ekf_linear_result res;
        need(nrhs, 11, cmd);
        if (!HAVE_OBSERVE_LINEAR) mexErrMsgIdAndTxt("ekfslam:usage", "observe_linear: this libekfslam has no ekf_observe_linear");
        const double *z = two_of(prhs[2], cmd, "z"), *R = r2x2_of(prhs[3], cmd), *wrap = two_of(prhs[8], cmd, "wrap");
        if (!prhs[4] || mxGetNumberOfElements(prhs[4]) != 6 || !mxGetPr(prhs[4])) mexErrMsgIdAndTxt("ekfslam:usage", "observe_linear: Hr needs 2 x 3 elements");
        const mwSize k = prhs[5] ? mxGetNumberOfElements(prhs[5]) : 0;
        if (k > 2 || (k && (mxGetClassID(prhs[5]) != mxDOUBLE_CLASS || !mxGetPr(prhs[5]))))
            mexErrMsgIdAndTxt("ekfslam:usage", "observe_linear: lm names at most two landmarks, class double");
        if ((prhs[6] ? mxGetNumberOfElements(prhs[6]) : 0) != 4 * k || (k && !mxGetPr(prhs[6])))
            mexErrMsgIdAndTxt("ekfslam:usage", "observe_linear: Hl needs one 2 x 2 block per landmark");
        for (int r = 0; r < 2; ++r) { o.z[r] = z[r]; o.lm[r] = -1; o.wrap_deg[r] = wrap[r] != 0.0; }
        for (int q = 0; q < 8; ++q) o.Hl[q >> 2][q & 3] = 0.0;
        for (int q = 0; q < 4; ++q) o.R[q] = R[q];
        for (int q = 0; q < 6; ++q) o.Hr[q] = mxGetPr(prhs[4])[q];
        for (mwSize b = 0; b < k; ++b) {                       /* whole numbers a landmark could carry; 1-based -> 0-based, once */
            const double v = mxGetPr(prhs[5])[b];
            if (!(v >= -9.0e15 && v <= 9.0e15) || v != (double)(int64_t)v) mexErrMsgIdAndTxt("ekfslam:usage", "observe_linear: landmark numbers are whole numbers");
            o.lm[b] = (int64_t)v - 1;
            for (int q = 0; q < 4; ++q) o.Hl[b][q] = mxGetPr(prhs[6])[4 * b + q];
        }
        o.gate = mxGetScalar(prhs[7]);
        o.rows = (int32_t)mxGetScalar(prhs[9]);
        const int wait = mxGetScalar(prhs[10]) != 0.0;
        check(h, ekf_observe_linear(h, &o, wait ? &res : NULL));
        plhs[0] = mxCreateDoubleMatrix(wait ? 1 : 0, wait ? 8 : 0, mxREAL);
        if (wait) {
            double *out = mxGetPr(plhs[0]);
            out[0] = res.nu[0]; out[1] = res.nu[1];
            for (int q = 0; q < 4; ++q) out[2 + q] = res.S[q];
            out[6] = res.d2; out[7] = (double)res.outcome;
        }
        return;
    }
    if (!strcmp(cmd, "observe_model")) {          /* res = (h, model 1..5, z 2, R 2x2, lm 0..2 numbers (1-based), anchor [] or 2, gate, wait): the target is
                                                     lm(1) or, with lm empty, the fixed point anchor; res as observe_linear's */
        ekf_model_obs o;
        ekf_linear_result res;
        need(nrhs, 9, cmd);
        if (!HAVE_OBSERVE_MODEL) mexErrMsgIdAndTxt("ekfslam:usage", "observe_model: this libekfslam has no ekf_observe_model");
        const double *z = two_of(prhs[3], cmd, "z"), *R = r2x2_of(prhs[4], cmd);
        const mwSize k = prhs[5] ? mxGetNumberOfElements(prhs[5]) : 0, na = prhs[6] ? mxGetNumberOfElements(prhs[6]) : 0;
        if (k > 2 || (k && (mxGetClassID(prhs[5]) != mxDOUBLE_CLASS || !mxGetPr(prhs[5]))))
            mexErrMsgIdAndTxt("ekfslam:usage", "observe_model: lm names at most two landmarks, class double");
        if (!((na == 2 && k == 0 && mxGetPr(prhs[6])) || (na == 0 && k > 0)))
            mexErrMsgIdAndTxt("ekfslam:usage", "observe_model: the target is a landmark (anchor empty) or an anchor of 2 elements (lm empty)");
        o.model = (int32_t)mxGetScalar(prhs[2]); o.reserved = 0;
        for (int r = 0; r < 2; ++r) { o.z[r] = z[r]; o.lm[r] = -1; o.anchor[r] = na ? mxGetPr(prhs[6])[r] : 0.0; }
        for (int q = 0; q < 4; ++q) o.R[q] = R[q];
        for (mwSize b = 0; b < k; ++b) {                       /* whole numbers a landmark could carry; 1-based -> 0-based, once */
            const double v = mxGetPr(prhs[5])[b];
            if (!(v >= -9.0e15 && v <= 9.0e15) || v != (double)(int64_t)v) mexErrMsgIdAndTxt("ekfslam:usage", "observe_model: landmark numbers are whole numbers");
            o.lm[b] = (int64_t)v - 1;
        }
        o.gate = mxGetScalar(prhs[7]);
        const int wait = mxGetScalar(prhs[8]) != 0.0;
        check(h, ekf_observe_model(h, &o, wait ? &res : NULL));
        plhs[0] = mxCreateDoubleMatrix(wait ? 1 : 0, wait ? 8 : 0, mxREAL);
        if (wait) {
            double *out = mxGetPr(plhs[0]);
            out[0] = res.nu[0]; out[1] = res.nu[1];
            for (int q = 0; q < 4; ++q) out[2 + q] = res.S[q];
            out[6] = res.d2; out[7] = (double)res.outcome;
        }
        return;
    }
    if (!strcmp(cmd, "observe_model_iterated")) { /* res = (h, model 1..5, z 2, R 2x2, lm 0..2 numbers (1-based), anchor [] or 2, gate, iterations 1..16, tol, wait):
                                                     observe_model relinearised on the device; res (wait): observe_model's 8 values of the FIRST linearisation,
                                                     then S(:)' nu(1) nu(2) used converged lastStep xLocal(1:7) of the one that made the pair */
        ekf_model_obs o;
        ekf_linear_result res;
        ekf_iterated_result it;
        need(nrhs, 11, cmd);
        if (!HAVE_OBSERVE_MODEL_ITERATED) mexErrMsgIdAndTxt("ekfslam:usage", "observe_model_iterated: this libekfslam has no ekf_observe_model_iterated");
        const double *z = two_of(prhs[3], cmd, "z"), *R = r2x2_of(prhs[4], cmd);
        const mwSize k = prhs[5] ? mxGetNumberOfElements(prhs[5]) : 0, na = prhs[6] ? mxGetNumberOfElements(prhs[6]) : 0;
        if (k > 2 || (k && (mxGetClassID(prhs[5]) != mxDOUBLE_CLASS || !mxGetPr(prhs[5]))))
            mexErrMsgIdAndTxt("ekfslam:usage", "observe_model_iterated: lm names at most two landmarks, class double");
        if (!((na == 2 && k == 0 && mxGetPr(prhs[6])) || (na == 0 && k > 0)))
            mexErrMsgIdAndTxt("ekfslam:usage", "observe_model_iterated: the target is a landmark (anchor empty) or an anchor of 2 elements (lm empty)");
        o.model = (int32_t)mxGetScalar(prhs[2]); o.reserved = 0;
        for (int r = 0; r < 2; ++r) { o.z[r] = z[r]; o.lm[r] = -1; o.anchor[r] = na ? mxGetPr(prhs[6])[r] : 0.0; }
        for (int q = 0; q < 4; ++q) o.R[q] = R[q];
        for (mwSize b = 0; b < k; ++b) {                       /* whole numbers a landmark could carry; 1-based -> 0-based, once */
            const double v = mxGetPr(prhs[5])[b];
            if (!(v >= -9.0e15 && v <= 9.0e15) || v != (double)(int64_t)v) mexErrMsgIdAndTxt("ekfslam:usage", "observe_model_iterated: landmark numbers are whole numbers");
            o.lm[b] = (int64_t)v - 1;
        }
        o.gate = mxGetScalar(prhs[7]);
        const double n = mxGetScalar(prhs[8]);
        if (!(n >= 1.0 && n <= (double)EKF_MODEL_ITER_MAX) || n != (double)(int32_t)n)
            mexErrMsgIdAndTxt("ekfslam:usage", "observe_model_iterated: iterations is a whole number, 1 .. %d", EKF_MODEL_ITER_MAX);
        const double tol = mxGetScalar(prhs[9]);
        const int wait = mxGetScalar(prhs[10]) != 0.0;
        check(h, ekf_observe_model_iterated(h, &o, (int32_t)n, tol, wait ? &res : NULL, wait ? &it : NULL));
        plhs[0] = mxCreateDoubleMatrix(wait ? 1 : 0, wait ? 24 : 0, mxREAL);
        if (wait) {
            double *out = mxGetPr(plhs[0]);
            out[0] = res.nu[0]; out[1] = res.nu[1];
            for (int q = 0; q < 4; ++q) { out[2 + q] = res.S[q]; out[8 + q] = it.S[q]; }
            out[6] = res.d2; out[7] = (double)res.outcome;
            out[12] = it.nu[0]; out[13] = it.nu[1];
            out[14] = (double)it.used; out[15] = (double)it.converged; out[16] = it.last_step;
            for (int q = 0; q < 7; ++q) out[17 + q] = it.x_local[q];
        }
        return;
    }
    if (!strcmp(cmd, "append_model")) {           /* idx = (h, model m x 1 (1 or 4), z m x 2, R 2 x 2 x m, signature m x 1): one scan of new landmarks,
                                                     each from its own observation; idx m x 1, their 1-based numbers */
        need(nrhs, 6, cmd);
        if (!HAVE_APPEND_MODEL) mexErrMsgIdAndTxt("ekfslam:usage", "append_model: this libekfslam has no ekf_append_model");
        const mwSize m = prhs[2] ? mxGetNumberOfElements(prhs[2]) : 0;
        if (m < 1 || m > EKF_APPEND_MODEL_MAX) mexErrMsgIdAndTxt("ekfslam:usage", "append_model: between 1 and %d entries in one call", EKF_APPEND_MODEL_MAX);
        if (!mxGetPr(prhs[2]) || !prhs[3] || mxGetM(prhs[3]) != m || mxGetNumberOfElements(prhs[3]) != 2 * m || !mxGetPr(prhs[3]))
            mexErrMsgIdAndTxt("ekfslam:usage", "append_model: z needs m x 2 elements, one row per entry of model");
        if (!prhs[4] || mxGetNumberOfElements(prhs[4]) != 4 * m || !mxGetPr(prhs[4]))
            mexErrMsgIdAndTxt("ekfslam:usage", "append_model: R needs 2 x 2 x m elements");
        if (!prhs[5] || mxGetNumberOfElements(prhs[5]) != m || !mxGetPr(prhs[5]))
            mexErrMsgIdAndTxt("ekfslam:usage", "append_model: signature needs m elements");
        ekf_model_init o[EKF_APPEND_MODEL_MAX];
        for (mwSize b = 0; b < m; ++b) {
            o[b].model = (int32_t)mxGetPr(prhs[2])[b]; o[b].reserved = 0;
            o[b].z[0] = mxGetPr(prhs[3])[b]; o[b].z[1] = mxGetPr(prhs[3])[m + b];       /* column-major m x 2 */
            for (int q = 0; q < 4; ++q) o[b].R[q] = mxGetPr(prhs[4])[4 * b + q];
            o[b].signature = mxGetPr(prhs[5])[b];
        }
        int64_t first = 0;
        check(h, ekf_append_model(h, o, (int64_t)m, &first));
        plhs[0] = mxCreateDoubleMatrix(m, 1, mxREAL);
        for (mwSize b = 0; b < m; ++b) mxGetPr(plhs[0])[b] = (double)(first + (int64_t)b + 1);
        return;
    }
    if (!strcmp(cmd, "join_map")) {               /* idx = (h, hlocal, signature_offset): the map of the handle hlocal joined into h on the device; idx M x 1,
                                                     the 1-based numbers of the new landmarks (0 x 1 for a local map without landmarks) */
        need(nrhs, 4, cmd);
        if (!HAVE_JOIN_MAP) mexErrMsgIdAndTxt("ekfslam:usage", "join_map: this libekfslam has no ekf_join_map");
        if (!prhs[2] || mxGetClassID(prhs[2]) != mxUINT64_CLASS || mxGetNumberOfElements(prhs[2]) != 1 || !mxGetData(prhs[2]))
            mexErrMsgIdAndTxt("ekfslam:handle", "join_map: the third argument must be the uint64 handle of the local map");
        ekf_handle *local = (ekf_handle *)(uintptr_t)(*(const uint64_t *)mxGetData(prhs[2]));
        if (!local) mexErrMsgIdAndTxt("ekfslam:handle", "join_map: null local handle (already destroyed?)");
        if (!prhs[3] || mxGetNumberOfElements(prhs[3]) != 1 || !mxGetPr(prhs[3]))
            mexErrMsgIdAndTxt("ekfslam:usage", "join_map: signature_offset is one number");
        int64_t first = 0, after = 0;
        check(h, ekf_join_map(h, local, mxGetPr(prhs[3])[0], &first));
        check(h, ekf_num_landmarks(h, &after));
        const mwSize m = after > first ? (mwSize)(after - first) : 0;
        plhs[0] = mxCreateDoubleMatrix(m, 1, mxREAL);
        for (mwSize b = 0; b < m; ++b) mxGetPr(plhs[0])[b] = (double)(first + (int64_t)b + 1);
        return;
    }
    if (!strcmp(cmd, "extract_map")) {            /* (h, idx, frame, hdst): landmarks idx (1-based, distinct, any order, any shape) and the robot taken out into
                                                     the handle hdst, whose whole state is replaced; frame 0: the map frame, 1: the robot frame; no output */
        need(nrhs, 5, cmd);
        if (!HAVE_EXTRACT_MAP) mexErrMsgIdAndTxt("ekfslam:usage", "extract_map: this libekfslam has no ekf_extract_map");
        if (!prhs[4] || mxGetClassID(prhs[4]) != mxUINT64_CLASS || mxGetNumberOfElements(prhs[4]) != 1 || !mxGetData(prhs[4]))
            mexErrMsgIdAndTxt("ekfslam:handle", "extract_map: the fifth argument must be the uint64 handle of the destination");
        ekf_handle *dst = (ekf_handle *)(uintptr_t)(*(const uint64_t *)mxGetData(prhs[4]));
        if (!dst) mexErrMsgIdAndTxt("ekfslam:handle", "extract_map: null destination handle (already destroyed?)");
        if (!prhs[3] || mxGetNumberOfElements(prhs[3]) != 1 || !mxGetPr(prhs[3]) || (mxGetPr(prhs[3])[0] != 0.0 && mxGetPr(prhs[3])[0] != 1.0))
            mexErrMsgIdAndTxt("ekfslam:usage", "extract_map: frame is 0 (map) or 1 (robot)");
        const int32_t frame = (int32_t)mxGetPr(prhs[3])[0];
        const mwSize m = prhs[2] ? mxGetNumberOfElements(prhs[2]) : 0;
        if (m && !mxGetPr(prhs[2])) mexErrMsgIdAndTxt("ekfslam:usage", "extract_map: idx holds landmark numbers");
        int64_t *idx0 = (int64_t *)malloc((m ? m : 1) * sizeof(int64_t));       /* freed before any MATLAB error can unwind */
        if (!idx0) mexErrMsgIdAndTxt("ekfslam:usage", "extract_map: out of memory");
        for (mwSize i = 0; i < m; ++i) idx0[i] = (int64_t)mxGetPr(prhs[2])[i] - 1;
        const int32_t rc = ekf_extract_map(h, idx0, (int64_t)m, frame, dst);
        free(idx0);
        check(h, rc);
        return;
    }
    if (!strcmp(cmd, "transform_map")) {          /* (h, frame, t, Sigma): the whole map moved into another frame, in place.  frame 0: by the rigid transform
                                                     t (3 values: tx, ty, phi in degrees) with covariance Sigma (3 x 3, or empty: exact); frame 1: into the
                                                     robot's own frame, t and Sigma both empty; no output */
        need(nrhs, 5, cmd);
        if (!HAVE_TRANSFORM_MAP) mexErrMsgIdAndTxt("ekfslam:usage", "transform_map: this libekfslam has no ekf_transform_map");
        if (!prhs[2] || mxGetNumberOfElements(prhs[2]) != 1 || !mxGetPr(prhs[2]) || (mxGetPr(prhs[2])[0] != 0.0 && mxGetPr(prhs[2])[0] != 1.0))
            mexErrMsgIdAndTxt("ekfslam:usage", "transform_map: frame is 0 (map) or 1 (robot)");
        const int32_t frame = (int32_t)mxGetPr(prhs[2])[0];
        const mwSize nt = prhs[3] ? mxGetNumberOfElements(prhs[3]) : 0, ns = prhs[4] ? mxGetNumberOfElements(prhs[4]) : 0;
        if (frame == 1 ? (nt != 0 || ns != 0) : (nt != 3 || !mxGetPr(prhs[3]) || (ns != 0 && (ns != 9 || !mxGetPr(prhs[4])))))
            mexErrMsgIdAndTxt("ekfslam:usage", "transform_map: frame 0 takes t (3 values) and Sigma (3 x 3 or empty), frame 1 takes both empty");
        check(h, ekf_transform_map(h, frame, nt ? mxGetPr(prhs[3]) : NULL, ns ? mxGetPr(prhs[4]) : NULL));      /* (MATLAB arrays are column-major) */
        return;
    }
    if (!strcmp(cmd, "factor_map")) {             /* [info, d2] = (h, ref): the Cholesky factorisation of P on the device.  ref: empty, or n x q (q = 1 .. 8)
                                                     reference states as columns, n = 3 + 2 N.  info = [n definite bad_index bad_pivot logdet logdet_map
                                                     min_pivot max_pivot], bad_index 1-based into x and 0 = none; d2: q x 1 (0 x 1 without ref) */
        ekf_factor_info info;
        need(nrhs, 3, cmd);
        if (!HAVE_FACTOR_MAP) mexErrMsgIdAndTxt("ekfslam:usage", "factor_map: this libekfslam has no ekf_factor_map");
        const int64_t n = nstate(h);
        const mwSize nel = prhs[2] ? mxGetNumberOfElements(prhs[2]) : 0;
        const mwSize q = nel / (mwSize)n;
        if (nel != 0 && (!mxGetPr(prhs[2]) || q * (mwSize)n != nel || q < 1 || q > 8))
            mexErrMsgIdAndTxt("ekfslam:usage", "factor_map: ref is empty or n x q, n = 3 + 2 N entries a column and q = 1 .. 8 columns");
        mxArray *d2 = mxCreateDoubleMatrix(q, 1, mxREAL);
        const int32_t rc = ekf_factor_map(h, nel ? mxGetPr(prhs[2]) : NULL, (int32_t)q, &info, nel ? mxGetPr(d2) : NULL);
        if (rc != EKF_OK) { mxDestroyArray(d2); check(h, rc); }
        plhs[0] = mxCreateDoubleMatrix(1, 8, mxREAL);
        double *o = mxGetPr(plhs[0]);
        o[0] = (double)info.n; o[1] = (double)info.definite; o[2] = (double)(info.bad_index + 1); o[3] = info.bad_pivot;
        o[4] = info.logdet; o[5] = info.logdet_map; o[6] = info.min_pivot; o[7] = info.max_pivot;
        if (nlhs > 1) plhs[1] = d2; else mxDestroyArray(d2);
        return;
    }
    if (!strcmp(cmd, "sample_map")) {             /* [samples, info] = (h, xi): draws of the posterior from one factorisation.  xi: n x k, one draw a column
                                                     (n = 3 + 2 N, k >= 1); samples: n x k, column q = x + C xi(:, q), all NaN where P is not positive
                                                     definite; info as factor_map's */
        ekf_factor_info info;
        need(nrhs, 3, cmd);
        if (!HAVE_SAMPLE_MAP) mexErrMsgIdAndTxt("ekfslam:usage", "sample_map: this libekfslam has no ekf_sample_map");
        const int64_t n = nstate(h);
        const mwSize nel = prhs[2] ? mxGetNumberOfElements(prhs[2]) : 0;
        const mwSize k = nel / (mwSize)n;
        if (nel == 0 || !mxGetPr(prhs[2]) || k * (mwSize)n != nel)
            mexErrMsgIdAndTxt("ekfslam:usage", "sample_map: xi is n x k, n = 3 + 2 N entries a column and k >= 1 columns");
        mxArray *out = mxCreateDoubleMatrix((mwSize)n, k, mxREAL);
        const int32_t rc = ekf_sample_map(h, mxGetPr(prhs[2]), (int64_t)k, mxGetPr(out), &info);       /* (MATLAB arrays are column-major) */
        if (rc != EKF_OK) { mxDestroyArray(out); check(h, rc); }
        plhs[0] = out;
        if (nlhs > 1) {
            plhs[1] = mxCreateDoubleMatrix(1, 8, mxREAL);
            double *o = mxGetPr(plhs[1]);
            o[0] = (double)info.n; o[1] = (double)info.definite; o[2] = (double)(info.bad_index + 1); o[3] = info.bad_pivot;
            o[4] = info.logdet; o[5] = info.logdet_map; o[6] = info.min_pivot; o[7] = info.max_pivot;
        }
        return;
    }
    if (!strcmp(cmd, "solve_map")) {              /* [out, info] = (h, B, form): P^-1 B (form 0) or C^-1 B (form 1) from one factorisation.  B: n x k, one
                                                     right-hand side a column (n = 3 + 2 N, k >= 1); out: n x k, all NaN where P is not positive
                                                     definite; info as factor_map's */
        ekf_factor_info info;
        need(nrhs, 4, cmd);
        if (!HAVE_SOLVE_MAP) mexErrMsgIdAndTxt("ekfslam:usage", "solve_map: this libekfslam has no ekf_solve_map");
        const int64_t n = nstate(h);
        const mwSize nel = prhs[2] ? mxGetNumberOfElements(prhs[2]) : 0;
        const mwSize k = nel / (mwSize)n;
        if (nel == 0 || !mxGetPr(prhs[2]) || k * (mwSize)n != nel)
            mexErrMsgIdAndTxt("ekfslam:usage", "solve_map: B is n x k, n = 3 + 2 N entries a column and k >= 1 columns");
        mxArray *out = mxCreateDoubleMatrix((mwSize)n, k, mxREAL);
        const int32_t rc = ekf_solve_map(h, (int32_t)mxGetScalar(prhs[3]), mxGetPr(prhs[2]), (int64_t)k, mxGetPr(out), &info);   /* (MATLAB arrays are column-major) */
        if (rc != EKF_OK) { mxDestroyArray(out); check(h, rc); }
        plhs[0] = out;
        if (nlhs > 1) {
            plhs[1] = mxCreateDoubleMatrix(1, 8, mxREAL);
            double *o = mxGetPr(plhs[1]);
            o[0] = (double)info.n; o[1] = (double)info.definite; o[2] = (double)(info.bad_index + 1); o[3] = info.bad_pivot;
            o[4] = info.logdet; o[5] = info.logdet_map; o[6] = info.min_pivot; o[7] = info.max_pivot;
        }
        return;
    }
    if (!strcmp(cmd, "multiply_map")) {           /* out = (h, B): P B with no factorisation, one read-only pass over the tile store per 16 columns.  B: n x k, one
                                                     vector a column (n = 3 + 2 N, k >= 1); out: n x k */
        need(nrhs, 3, cmd);
        if (!HAVE_MULTIPLY_MAP) mexErrMsgIdAndTxt("ekfslam:usage", "multiply_map: this libekfslam has no ekf_multiply_map");
        const int64_t n = nstate(h);
        const mwSize nel = prhs[2] ? mxGetNumberOfElements(prhs[2]) : 0;
        const mwSize k = nel / (mwSize)n;
        if (nel == 0 || !mxGetPr(prhs[2]) || k * (mwSize)n != nel)
            mexErrMsgIdAndTxt("ekfslam:usage", "multiply_map: B is n x k, n = 3 + 2 N entries a column and k >= 1 columns");
        mxArray *out = mxCreateDoubleMatrix((mwSize)n, k, mxREAL);
        const int32_t rc = ekf_multiply_map(h, mxGetPr(prhs[2]), (int64_t)k, mxGetPr(out));   /* (MATLAB arrays are column-major) */
        if (rc != EKF_OK) { mxDestroyArray(out); check(h, rc); }
        plhs[0] = out;
        return;
    }
    if (!strcmp(cmd, "observe_dense")) {          /* [res, nu, S] = (h, H, z, R, gate, wrap): "H x = z +- R" for k <= 16 rows that may touch every landmark.  H: n x k,
                                                     one ROW of the observation a column (n = 3 + 2 N); z: k; R: k x k; gate: scalar (Inf: none); wrap: k
                                                     flags or empty; res = [d2 rows outcome bad_row], bad_row 1-based and 0 = none; nu: k x 1; S: k x k */
        need(nrhs, 7, cmd);
        if (!HAVE_OBSERVE_DENSE) mexErrMsgIdAndTxt("ekfslam:usage", "observe_dense: this libekfslam has no ekf_observe_dense");
        const int64_t n = nstate(h);
        const mwSize nel = prhs[2] ? mxGetNumberOfElements(prhs[2]) : 0;
        const mwSize k = nel / (mwSize)n;
        if (nel == 0 || !mxGetPr(prhs[2]) || k * (mwSize)n != nel || k > EKF_DENSE_MAX)
            mexErrMsgIdAndTxt("ekfslam:usage", "observe_dense: H is n x k, n = 3 + 2 N entries a column and 1 <= k <= %d columns", EKF_DENSE_MAX);
        if (!prhs[3] || mxGetNumberOfElements(prhs[3]) != k || !mxGetPr(prhs[3])) mexErrMsgIdAndTxt("ekfslam:usage", "observe_dense: z needs k elements");
        if (!prhs[4] || mxGetNumberOfElements(prhs[4]) != k * k || !mxGetPr(prhs[4])) mexErrMsgIdAndTxt("ekfslam:usage", "observe_dense: R needs k x k elements");
        const mwSize nw = prhs[6] ? mxGetNumberOfElements(prhs[6]) : 0;
        if (nw != 0 && (nw != k || !mxGetPr(prhs[6]))) mexErrMsgIdAndTxt("ekfslam:usage", "observe_dense: wrap needs k elements, or none");
        int32_t wrap[EKF_DENSE_MAX];
        for (mwSize i = 0; i < nw; ++i) wrap[i] = mxGetPr(prhs[6])[i] != 0.0;
        ekf_observe_dense_result res;
        mxArray *nu = mxCreateDoubleMatrix(k, 1, mxREAL), *S = mxCreateDoubleMatrix(k, k, mxREAL);
        const int32_t rc = ekf_observe_dense(h, mxGetPr(prhs[2]), (int64_t)k, mxGetPr(prhs[3]), mxGetPr(prhs[4]), nw ? wrap : NULL, mxGetScalar(prhs[5]),
                                             &res, mxGetPr(nu), mxGetPr(S));        /* (MATLAB arrays are column-major: a column of H is a row of the ABI's) */
        if (rc != EKF_OK) { mxDestroyArray(nu); mxDestroyArray(S); check(h, rc); }
        plhs[0] = mxCreateDoubleMatrix(1, 4, mxREAL);
        double *o = mxGetPr(plhs[0]);
        o[0] = res.d2; o[1] = (double)res.rows; o[2] = (double)res.outcome; o[3] = (double)(res.bad_row + 1);
        if (nlhs > 1) plhs[1] = nu; else mxDestroyArray(nu);
        if (nlhs > 2) plhs[2] = S; else mxDestroyArray(S);
        return;
    }
    if (!strcmp(cmd, "associate_model")) {        /* [match, d2] = (h, model m x 1 (1..4), z m x 2, R 2 x 2 x m, gate m x 1): which landmark each sighting of a
                                                     scan belongs to; match m x 6 = [best second d2_best d2_second within_gate irregular], landmarks
                                                     1-based and 0 = none; d2 (second output, optional): N x m, column k = observation k against every landmark */
        need(nrhs, 6, cmd);
        if (!HAVE_ASSOCIATE_MODEL) mexErrMsgIdAndTxt("ekfslam:usage", "associate_model: this libekfslam has no ekf_associate_model");
        const mwSize m = prhs[2] ? mxGetNumberOfElements(prhs[2]) : 0;
        if (m < 1 || m > EKF_ASSOCIATE_MODEL_MAX) mexErrMsgIdAndTxt("ekfslam:usage", "associate_model: between 1 and %d observations in one call", EKF_ASSOCIATE_MODEL_MAX);
        if (!mxGetPr(prhs[2]) || !prhs[3] || mxGetM(prhs[3]) != m || mxGetNumberOfElements(prhs[3]) != 2 * m || !mxGetPr(prhs[3]))
            mexErrMsgIdAndTxt("ekfslam:usage", "associate_model: z needs m x 2 elements, one row per entry of model");
        if (!prhs[4] || mxGetNumberOfElements(prhs[4]) != 4 * m || !mxGetPr(prhs[4]))
            mexErrMsgIdAndTxt("ekfslam:usage", "associate_model: R needs 2 x 2 x m elements");
        if (!prhs[5] || mxGetNumberOfElements(prhs[5]) != m || !mxGetPr(prhs[5]))
            mexErrMsgIdAndTxt("ekfslam:usage", "associate_model: gate needs m elements");
        ekf_model_obs o[EKF_ASSOCIATE_MODEL_MAX];
        ekf_model_match match[EKF_ASSOCIATE_MODEL_MAX];
        for (mwSize k = 0; k < m; ++k) {
            o[k].model = (int32_t)mxGetPr(prhs[2])[k]; o[k].reserved = 0;
            o[k].z[0] = mxGetPr(prhs[3])[k]; o[k].z[1] = mxGetPr(prhs[3])[m + k];       /* column-major m x 2 */
            for (int q = 0; q < 4; ++q) o[k].R[q] = mxGetPr(prhs[4])[4 * k + q];
            o[k].lm[0] = o[k].lm[1] = -1;
            o[k].anchor[0] = o[k].anchor[1] = 0.0;
            o[k].gate = mxGetPr(prhs[5])[k];
        }
        mxArray *all = NULL;
        if (nlhs > 1) all = mxCreateDoubleMatrix((mwSize)((nstate(h) - 3) / 2), m, mxREAL);     /* N x m column-major is m x N row-major */
        const bool want = all && mxGetNumberOfElements(all) > 0;
        check(h, ekf_associate_model(h, o, (int64_t)m, match, want ? mxGetPr(all) : NULL));
        plhs[0] = mxCreateDoubleMatrix(m, 6, mxREAL);
        double *out = mxGetPr(plhs[0]);
        for (mwSize k = 0; k < m; ++k) {
            out[k] = (double)(match[k].best + 1); out[m + k] = (double)(match[k].second + 1);
            out[2 * m + k] = match[k].d2_best; out[3 * m + k] = match[k].d2_second;
            out[4 * m + k] = (double)match[k].within_gate; out[5 * m + k] = (double)match[k].irregular;
        }
        if (all) plhs[1] = all;
        return;
    }
    if (!strcmp(cmd, "assign_model")) {           /* [res, total, cand, candD2] = (h, model m x 1 (1..4), z m x 2, R 2 x 2 x m, gate m x 1, all finite): which
                                                     observation of a scan gets which landmark when they compete; res m x 9 = [landmark d2 ncand best second
                                                     d2_best d2_second within_gate irregular], landmarks 1-based and 0 = left out / none; total: the minimised
                                                     sum; cand, candD2 (third and fourth output, optional): m x 32, row k = the candidates kept for observation k
                                                     by (d2, landmark), 0 / Inf behind them */
        need(nrhs, 6, cmd);
        if (!HAVE_ASSIGN_MODEL) mexErrMsgIdAndTxt("ekfslam:usage", "assign_model: this libekfslam has no ekf_assign_model");
        const mwSize m = prhs[2] ? mxGetNumberOfElements(prhs[2]) : 0;
        if (m < 1 || m > EKF_ASSIGN_MODEL_MAX) mexErrMsgIdAndTxt("ekfslam:usage", "assign_model: between 1 and %d observations in one call", EKF_ASSIGN_MODEL_MAX);
        if (!mxGetPr(prhs[2]) || !prhs[3] || mxGetM(prhs[3]) != m || mxGetNumberOfElements(prhs[3]) != 2 * m || !mxGetPr(prhs[3]))
            mexErrMsgIdAndTxt("ekfslam:usage", "assign_model: z needs m x 2 elements, one row per entry of model");
        if (!prhs[4] || mxGetNumberOfElements(prhs[4]) != 4 * m || !mxGetPr(prhs[4]))
            mexErrMsgIdAndTxt("ekfslam:usage", "assign_model: R needs 2 x 2 x m elements");
        if (!prhs[5] || mxGetNumberOfElements(prhs[5]) != m || !mxGetPr(prhs[5]))
            mexErrMsgIdAndTxt("ekfslam:usage", "assign_model: gate needs m elements");
        ekf_model_obs o[EKF_ASSIGN_MODEL_MAX];
        ekf_model_assigned as[EKF_ASSIGN_MODEL_MAX];
        ekf_model_match match[EKF_ASSIGN_MODEL_MAX];
        static int64_t cand[EKF_ASSIGN_MODEL_MAX * EKF_ASSIGN_CANDIDATES];
        static double cand_d2[EKF_ASSIGN_MODEL_MAX * EKF_ASSIGN_CANDIDATES];
        for (mwSize k = 0; k < m; ++k) {
            o[k].model = (int32_t)mxGetPr(prhs[2])[k]; o[k].reserved = 0;
            o[k].z[0] = mxGetPr(prhs[3])[k]; o[k].z[1] = mxGetPr(prhs[3])[m + k];       /* column-major m x 2 */
            for (int q = 0; q < 4; ++q) o[k].R[q] = mxGetPr(prhs[4])[4 * k + q];
            o[k].lm[0] = o[k].lm[1] = -1;
            o[k].anchor[0] = o[k].anchor[1] = 0.0;
            o[k].gate = mxGetPr(prhs[5])[k];
        }
        const bool lists = nlhs > 2;
        double total = 0.0;
        check(h, ekf_assign_model(h, o, (int64_t)m, as, match, lists ? cand : NULL, lists ? cand_d2 : NULL, &total));
        plhs[0] = mxCreateDoubleMatrix(m, 9, mxREAL);
        double *out = mxGetPr(plhs[0]);
        for (mwSize k = 0; k < m; ++k) {
            out[k] = (double)(as[k].landmark + 1); out[m + k] = as[k].d2; out[2 * m + k] = (double)as[k].ncand;
            out[3 * m + k] = (double)(match[k].best + 1); out[4 * m + k] = (double)(match[k].second + 1);
            out[5 * m + k] = match[k].d2_best; out[6 * m + k] = match[k].d2_second;
            out[7 * m + k] = (double)match[k].within_gate; out[8 * m + k] = (double)match[k].irregular;
        }
        if (nlhs > 1) plhs[1] = mxCreateDoubleScalar(total);
        if (lists) {
            plhs[2] = mxCreateDoubleMatrix(m, EKF_ASSIGN_CANDIDATES, mxREAL);
            mxArray *d2 = nlhs > 3 ? mxCreateDoubleMatrix(m, EKF_ASSIGN_CANDIDATES, mxREAL) : NULL;
            for (mwSize k = 0; k < m; ++k)
                for (mwSize s = 0; s < EKF_ASSIGN_CANDIDATES; ++s) {                  /* row-major m x 32 -> column-major */
                    mxGetPr(plhs[2])[s * m + k] = (double)(cand[k * EKF_ASSIGN_CANDIDATES + s] + 1);
                    if (d2) mxGetPr(d2)[s * m + k] = cand_d2[k * EKF_ASSIGN_CANDIDATES + s];
                }
            if (d2) plhs[3] = d2;
        }
        return;
    }
    if (!strcmp(cmd, "joint_innovation")) {       /* [res, prefix] = (h, model m x 1 (1..4), z m x 2, R 2 x 2 x m, hyp nh x m): the joint compatibility of a scan's
                                                     pairings; hyp(i, k) = the landmark (1-based) observation k is paired with in hypothesis i, 0 = left out;
                                                     res nh x 5 = [d2 dof pairings outcome firstIrregular] (the entry of the scan, 1-based, 0 = none);
                                                     prefix (second output, optional): nh x m, the joint d2 of the pairings among observations 1..k */
        need(nrhs, 6, cmd);
        if (!HAVE_JOINT_INNOVATION) mexErrMsgIdAndTxt("ekfslam:usage", "joint_innovation: this libekfslam has no ekf_joint_innovation");
        const mwSize m = prhs[2] ? mxGetNumberOfElements(prhs[2]) : 0;
        if (m < 1 || m > EKF_JOINT_MAX) mexErrMsgIdAndTxt("ekfslam:usage", "joint_innovation: between 1 and %d observations in one call", EKF_JOINT_MAX);
        if (!mxGetPr(prhs[2]) || !prhs[3] || mxGetM(prhs[3]) != m || mxGetNumberOfElements(prhs[3]) != 2 * m || !mxGetPr(prhs[3]))
            mexErrMsgIdAndTxt("ekfslam:usage", "joint_innovation: z needs m x 2 elements, one row per entry of model");
        if (!prhs[4] || mxGetNumberOfElements(prhs[4]) != 4 * m || !mxGetPr(prhs[4]))
            mexErrMsgIdAndTxt("ekfslam:usage", "joint_innovation: R needs 2 x 2 x m elements");
        const mwSize nh = prhs[5] ? mxGetM(prhs[5]) : 0;
        if (nh < 1 || nh > EKF_JOINT_HYP_MAX) mexErrMsgIdAndTxt("ekfslam:usage", "joint_innovation: between 1 and %d hypotheses in one call", EKF_JOINT_HYP_MAX);
        if (mxGetN(prhs[5]) != m || mxGetNumberOfElements(prhs[5]) != nh * m || !mxGetPr(prhs[5]))
            mexErrMsgIdAndTxt("ekfslam:usage", "joint_innovation: hyp needs nh x m elements, one column per entry of model");
        ekf_model_obs o[EKF_JOINT_MAX];
        for (mwSize k = 0; k < m; ++k) {
            o[k].model = (int32_t)mxGetPr(prhs[2])[k]; o[k].reserved = 0;
            o[k].z[0] = mxGetPr(prhs[3])[k]; o[k].z[1] = mxGetPr(prhs[3])[m + k];       /* column-major m x 2 */
            for (int q = 0; q < 4; ++q) o[k].R[q] = mxGetPr(prhs[4])[4 * k + q];
            o[k].lm[0] = o[k].lm[1] = -1;
            o[k].anchor[0] = o[k].anchor[1] = 0.0;
            o[k].gate = HUGE_VAL;
        }
        int64_t *hyp = (int64_t *)malloc((size_t)(nh * m) * sizeof(int64_t));           /* freed before any MATLAB error can unwind */
        ekf_joint_result *res = (ekf_joint_result *)malloc((size_t)nh * sizeof(ekf_joint_result));
        if (!hyp || !res) { free(hyp); free(res); mexErrMsgIdAndTxt("ekfslam:usage", "joint_innovation: out of memory"); }
        bool whole = true;
        for (mwSize i = 0; i < nh; ++i)
            for (mwSize k = 0; k < m; ++k) {
                const double v = mxGetPr(prhs[5])[k * nh + i];                            /* column-major nh x m -> row-major, 1-based -> 0-based */
                whole = whole && v >= 0.0 && v < 9.0e15 && (double)(int64_t)v == v;      /* (no libm call: the gateway links without it) */
                hyp[i * m + k] = whole ? (int64_t)v - 1 : -1;
            }
        if (!whole) { free(hyp); free(res); mexErrMsgIdAndTxt("ekfslam:usage", "joint_innovation: hyp holds landmark numbers (1-based), 0 = left out"); }
        mxArray *rowmajor = nlhs > 1 ? mxCreateDoubleMatrix(m, nh, mxREAL) : NULL;       /* m x nh column-major is nh x m row-major */
        const int32_t rc = ekf_joint_innovation(h, o, (int64_t)m, hyp, (int64_t)nh, res, rowmajor ? mxGetPr(rowmajor) : NULL, NULL, NULL);
        mxArray *out = NULL, *prefix = NULL;
        if (rc == EKF_OK) {
            out = mxCreateDoubleMatrix(nh, 5, mxREAL);
            for (mwSize i = 0; i < nh; ++i) {
                mxGetPr(out)[i] = res[i].d2; mxGetPr(out)[nh + i] = (double)res[i].dof; mxGetPr(out)[2 * nh + i] = (double)res[i].pairings;
                mxGetPr(out)[3 * nh + i] = (double)res[i].outcome; mxGetPr(out)[4 * nh + i] = (double)(res[i].first_irregular + 1);
            }
            if (rowmajor) {
                prefix = mxCreateDoubleMatrix(nh, m, mxREAL);
                for (mwSize i = 0; i < nh; ++i)
                    for (mwSize k = 0; k < m; ++k) mxGetPr(prefix)[k * nh + i] = mxGetPr(rowmajor)[i * m + k];
            }
        }
        free(hyp); free(res);
        if (rowmajor) mxDestroyArray(rowmajor);
        check(h, rc);
        plhs[0] = out;
        if (prefix) plhs[1] = prefix;
        return;
    }
    if (!strcmp(cmd, "joint_search")) {           /* [res, lm, match] = (h, model m x 1 (1..4), z m x 2, R 2 x 2 x m, gate, threshold (2m + 1), beam): the
                                                     joint-compatibility search on the device, one wait; gate: the candidate gate of every entry (finite);
                                                     threshold(dof + 1) for dof 0 .. 2m; res 1 x 6 = [d2 dof pairings truncated nalive irregular];
                                                     lm m x 1: the winner (1-based, 0 = left out); match (optional) m x 3 = [withinGate best d2Best] per
                                                     entry (best 1-based, 0 = none): withinGate == 0 says the entry had no candidate */
        need(nrhs, 8, cmd);
        if (!HAVE_JOINT_SEARCH) mexErrMsgIdAndTxt("ekfslam:usage", "joint_search: this libekfslam has no ekf_joint_search");
        const mwSize m = prhs[2] ? mxGetNumberOfElements(prhs[2]) : 0;
        if (m < 1 || m > EKF_JOINT_MAX) mexErrMsgIdAndTxt("ekfslam:usage", "joint_search: between 1 and %d observations in one call", EKF_JOINT_MAX);
        if (!mxGetPr(prhs[2]) || !prhs[3] || mxGetM(prhs[3]) != m || mxGetNumberOfElements(prhs[3]) != 2 * m || !mxGetPr(prhs[3]))
            mexErrMsgIdAndTxt("ekfslam:usage", "joint_search: z needs m x 2 elements, one row per entry of model");
        if (!prhs[4] || mxGetNumberOfElements(prhs[4]) != 4 * m || !mxGetPr(prhs[4]))
            mexErrMsgIdAndTxt("ekfslam:usage", "joint_search: R needs 2 x 2 x m elements");
        if (!prhs[5] || mxGetNumberOfElements(prhs[5]) != 1 || !mxGetPr(prhs[5]))
            mexErrMsgIdAndTxt("ekfslam:usage", "joint_search: gate is one number");
        if (!prhs[6] || mxGetNumberOfElements(prhs[6]) != 2 * m + 1 || !mxGetPr(prhs[6]))
            mexErrMsgIdAndTxt("ekfslam:usage", "joint_search: threshold needs 2 m + 1 elements, one per dof 0 .. 2 m");
        if (!prhs[7] || mxGetNumberOfElements(prhs[7]) != 1 || !mxGetPr(prhs[7]))
            mexErrMsgIdAndTxt("ekfslam:usage", "joint_search: beam is one number");
        const double beam = mxGetScalar(prhs[7]);
        if (!(beam >= 1.0 && beam <= (double)EKF_JOINT_SEARCH_BEAM_MAX) || (double)(int32_t)beam != beam)
            mexErrMsgIdAndTxt("ekfslam:usage", "joint_search: beam is a whole number between 1 and %d", EKF_JOINT_SEARCH_BEAM_MAX);
        ekf_model_obs o[EKF_JOINT_MAX];
        for (mwSize k = 0; k < m; ++k) {
            o[k].model = (int32_t)mxGetPr(prhs[2])[k]; o[k].reserved = 0;
            o[k].z[0] = mxGetPr(prhs[3])[k]; o[k].z[1] = mxGetPr(prhs[3])[m + k];       /* column-major m x 2 */
            for (int q = 0; q < 4; ++q) o[k].R[q] = mxGetPr(prhs[4])[4 * k + q];
            o[k].lm[0] = o[k].lm[1] = -1;
            o[k].anchor[0] = o[k].anchor[1] = 0.0;
            o[k].gate = mxGetScalar(prhs[5]);
        }
        ekf_joint_search_result res;
        ekf_model_match match[EKF_JOINT_MAX];
        check(h, ekf_joint_search(h, o, (int64_t)m, mxGetPr(prhs[6]), (int32_t)beam, &res, match, NULL, NULL, NULL, NULL));
        plhs[0] = mxCreateDoubleMatrix(1, 6, mxREAL);
        const double head[6] = { res.d2, (double)res.dof, (double)res.pairings, (double)res.truncated, (double)res.nalive, (double)res.irregular };
        for (int q = 0; q < 6; ++q) mxGetPr(plhs[0])[q] = head[q];
        if (nlhs > 1) {
            plhs[1] = mxCreateDoubleMatrix(m, 1, mxREAL);
            for (mwSize k = 0; k < m; ++k) mxGetPr(plhs[1])[k] = (double)(res.lm[k] + 1);
        }
        if (nlhs > 2) {
            plhs[2] = mxCreateDoubleMatrix(m, 3, mxREAL);
            for (mwSize k = 0; k < m; ++k) {
                mxGetPr(plhs[2])[k] = (double)match[k].within_gate; mxGetPr(plhs[2])[m + k] = (double)(match[k].best + 1);
                mxGetPr(plhs[2])[2 * m + k] = match[k].d2_best;
            }
        }
        return;
    }
    if (!strcmp(cmd, "observe_model_joint")) {    /* res = (h, model m x 1 (1..4), z m x 2, R 2 x 2 x m, lm m x 1, gate): the scan's pairings applied as ONE joint
                                                     update; lm(k) = the landmark (1-based) observation k is paired with, 0 = left out; applied only if the
                                                     joint d2 <= gate; res 1 x 5 = [d2 dof pairings outcome firstIrregular] (outcome 1 applied, 2 gated) */
        need(nrhs, 7, cmd);
        if (!HAVE_OBSERVE_MODEL_JOINT) mexErrMsgIdAndTxt("ekfslam:usage", "observe_model_joint: this libekfslam has no ekf_observe_model_joint");
        ekf_model_obs o[EKF_JOINT_MAX];
        int64_t lm[EKF_JOINT_MAX];
        const mwSize m = joint_scan(cmd, prhs, o, lm);
        ekf_joint_result res;
        check(h, ekf_observe_model_joint(h, o, (int64_t)m, lm, mxGetPr(prhs[6])[0], &res, NULL, NULL));
        plhs[0] = mxCreateDoubleMatrix(1, 5, mxREAL);
        mxGetPr(plhs[0])[0] = res.d2; mxGetPr(plhs[0])[1] = (double)res.dof; mxGetPr(plhs[0])[2] = (double)res.pairings;
        mxGetPr(plhs[0])[3] = (double)res.outcome; mxGetPr(plhs[0])[4] = (double)(res.first_irregular + 1);
        return;
    }
    if (!strcmp(cmd, "observe_model_joint_iterated")) {   /* res = (h, model, z, R, lm, gate, iterations, tol): observe_model_joint relinearised up to
                                                     `iterations` times (1..16), stopping where no entry moves by more than tol; the gate and res(1:5) are the
                                                     first linearisation's; res 1 x 8 = [d2 dof pairings outcome firstIrregular used converged step] */
        need(nrhs, 9, cmd);
        if (!HAVE_OBSERVE_MODEL_JOINT_ITERATED)
            mexErrMsgIdAndTxt("ekfslam:usage", "observe_model_joint_iterated: this libekfslam has no ekf_observe_model_joint_iterated");
        ekf_model_obs o[EKF_JOINT_MAX];
        int64_t lm[EKF_JOINT_MAX];
        const mwSize m = joint_scan(cmd, prhs, o, lm);
        if (!prhs[7] || mxGetNumberOfElements(prhs[7]) != 1 || !mxGetPr(prhs[7]) || !prhs[8] || mxGetNumberOfElements(prhs[8]) != 1 || !mxGetPr(prhs[8]))
            mexErrMsgIdAndTxt("ekfslam:usage", "observe_model_joint_iterated: iterations and tol are one number each");
        const double n = mxGetPr(prhs[7])[0];
        if (!(n >= 1.0 && n <= (double)EKF_JOINT_ITER_MAX && (double)(int32_t)n == n))
            mexErrMsgIdAndTxt("ekfslam:usage", "observe_model_joint_iterated: iterations is a whole number, 1 .. %d", EKF_JOINT_ITER_MAX);
        ekf_joint_result res;
        ekf_joint_iter_result it;
        check(h, ekf_observe_model_joint_iterated(h, o, (int64_t)m, lm, mxGetPr(prhs[6])[0], (int32_t)n, mxGetPr(prhs[8])[0], &res, &it, NULL, NULL));
        plhs[0] = mxCreateDoubleMatrix(1, 8, mxREAL);
        mxGetPr(plhs[0])[0] = res.d2; mxGetPr(plhs[0])[1] = (double)res.dof; mxGetPr(plhs[0])[2] = (double)res.pairings;
        mxGetPr(plhs[0])[3] = (double)res.outcome; mxGetPr(plhs[0])[4] = (double)(res.first_irregular + 1);
        mxGetPr(plhs[0])[5] = (double)it.used; mxGetPr(plhs[0])[6] = (double)it.converged; mxGetPr(plhs[0])[7] = it.last_step;
        return;
    }
    if (!strcmp(cmd, "predict_model")) {          /* (h, model m x 1 (1..3), u m x 3, M 3 x 3 x m): a chain of motion steps with their true Jacobians, in order,
                                                     one launch; a model with two inputs reads u(:, 1:2) and M(1:2, 1:2, k) */
        need(nrhs, 5, cmd);
        if (!HAVE_PREDICT_MODEL) mexErrMsgIdAndTxt("ekfslam:usage", "predict_model: this libekfslam has no ekf_predict_model");
        const mwSize m = prhs[2] ? mxGetNumberOfElements(prhs[2]) : 0;
        if (m < 1 || m > EKF_PREDICT_MODEL_MAX) mexErrMsgIdAndTxt("ekfslam:usage", "predict_model: between 1 and %d steps in one call", EKF_PREDICT_MODEL_MAX);
        if (!mxGetPr(prhs[2]) || !prhs[3] || mxGetM(prhs[3]) != m || mxGetNumberOfElements(prhs[3]) != 3 * m || !mxGetPr(prhs[3]))
            mexErrMsgIdAndTxt("ekfslam:usage", "predict_model: u needs m x 3 elements, one row per entry of model");
        if (!prhs[4] || mxGetNumberOfElements(prhs[4]) != 9 * m || !mxGetPr(prhs[4]))
            mexErrMsgIdAndTxt("ekfslam:usage", "predict_model: M needs 3 x 3 x m elements");
        ekf_motion o[EKF_PREDICT_MODEL_MAX];
        for (mwSize b = 0; b < m; ++b) {
            o[b].model = (int32_t)mxGetPr(prhs[2])[b]; o[b].reserved = 0;
            for (int q = 0; q < 3; ++q) o[b].u[q] = mxGetPr(prhs[3])[q * m + b];        /* column-major m x 3 */
            for (int q = 0; q < 9; ++q) o[b].M[q] = mxGetPr(prhs[4])[9 * b + q];
        }
        check(h, ekf_predict_model(h, o, (int64_t)m));
        return;
    }
    if (!strcmp(cmd, "merge_landmarks_batch")) {  /* d2 = (h, pairs k x 2 [keep drop], R 2x2): k x 1; landmark numbers 1-based, as they are before the call */
        need(nrhs, 4, cmd);
        if (!HAVE_MERGE_LANDMARKS_BATCH) mexErrMsgIdAndTxt("ekfslam:usage", "merge_landmarks_batch: this libekfslam has no ekf_merge_landmarks_batch");
        if (!prhs[2] || mxGetN(prhs[2]) != 2 || mxGetNumberOfElements(prhs[2]) != 2 * mxGetM(prhs[2]) || (mxGetM(prhs[2]) && !mxGetPr(prhs[2])))
            mexErrMsgIdAndTxt("ekfslam:usage", "merge_landmarks_batch: pairs needs k x 2 elements [keep drop]");
        const mwSize k = mxGetM(prhs[2]);
        if (k > EKF_MERGE_BATCH_MAX) mexErrMsgIdAndTxt("ekfslam:usage", "merge_landmarks_batch: at most %d pairs in one call", EKF_MERGE_BATCH_MAX);
        const double *R = r2x2_of(prhs[3], cmd);
        int64_t keep0[EKF_MERGE_BATCH_MAX], drop0[EKF_MERGE_BATCH_MAX];
        if (mxGetClassID(prhs[2]) != mxDOUBLE_CLASS) mexErrMsgIdAndTxt("ekfslam:usage", "merge_landmarks_batch: pairs must be of class double");
        for (mwSize i = 0; i < 2 * k; ++i) {                   /* whole numbers a landmark could carry: the cast below is then exact */
            const double v = mxGetPr(prhs[2])[i];
            if (!(v >= -9.0e15 && v <= 9.0e15) || v != (double)(int64_t)v)
                mexErrMsgIdAndTxt("ekfslam:usage", "merge_landmarks_batch: landmark numbers are whole numbers");
        }
        for (mwSize i = 0; i < k; ++i) {                       /* column-major: keeps, then drops; 1-based -> 0-based, once */
            keep0[i] = (int64_t)mxGetPr(prhs[2])[i] - 1;
            drop0[i] = (int64_t)mxGetPr(prhs[2])[k + i] - 1;
        }
        mxArray *d2 = mxCreateDoubleMatrix(k, 1, mxREAL);
        const int32_t rc = ekf_merge_landmarks_batch(h, keep0, drop0, (int64_t)k, R, mxGetPr(d2));
        if (rc != EKF_OK) { mxDestroyArray(d2); check(h, rc); }
        plhs[0] = d2;
        return;
    }
    if (!strcmp(cmd, "measure")) {                /* (h, observed_LL m x 3, u, lm_index L x 1, lm_loc L x 2) */
        need(nrhs, 6, cmd);
        check(h, ekf_measure(h, mxGetPr(prhs[2]), (int64_t)mxGetM(prhs[2]), mxGetPr(prhs[3]), mxGetPr(prhs[4]),
                             mxGetPr(prhs[5]), (int64_t)mxGetNumberOfElements(prhs[4])));
        return;
    }
    if (!strcmp(cmd, "get_x")) { int64_t n = nstate(h); plhs[0] = mxCreateDoubleMatrix(1, (mwSize)n, mxREAL); check(h, ekf_get_x(h, mxGetPr(plhs[0]))); return; }
    if (!strcmp(cmd, "get_P")) { int64_t n = nstate(h); plhs[0] = mxCreateDoubleMatrix((mwSize)n, (mwSize)n, mxREAL); check(h, ekf_get_P(h, mxGetPr(plhs[0]))); return; }
    if (!strcmp(cmd, "get_s")) { int64_t n = (nstate(h) - 3) / 2; plhs[0] = mxCreateDoubleMatrix((mwSize)n, 1, mxREAL); check(h, ekf_get_s(h, mxGetPr(plhs[0]))); return; }
    if (!strcmp(cmd, "get_Q")) { int64_t n = nstate(h); double q[9]; check(h, ekf_get_Q(h, q));
        plhs[0] = mxCreateDoubleMatrix((mwSize)n, (mwSize)n, mxREAL);      /* zeros(size(P)) with the 3x3 block */
        for (int c = 0; c < 3; ++c) for (int r = 0; r < 3; ++r) mxGetPr(plhs[0])[c * n + r] = q[3 * c + r];
        return; }
    if (!strcmp(cmd, "get_P_block")) {            /* (h, r0, c0, nr, nc), 1-based corner */
        need(nrhs, 6, cmd);
        mwSize nr = (mwSize)mxGetScalar(prhs[4]), nc = (mwSize)mxGetScalar(prhs[5]);
        plhs[0] = mxCreateDoubleMatrix(nr, nc, mxREAL);
        check(h, ekf_get_P_block(h, (int64_t)mxGetScalar(prhs[2]) - 1, (int64_t)mxGetScalar(prhs[3]) - 1, nr, nc, mxGetPr(plhs[0])));
        return;
    }
    if (!strcmp(cmd, "get_P_diag_blocks")) {      /* 2 x 2 x (N+1): P(1:2,1:2), then every landmark's block -- what plot() reads */
        int64_t nb = (nstate(h) - 3) / 2 + 1;
        plhs[0] = mxCreateDoubleMatrix(4, (mwSize)nb, mxREAL);             /* the .m side reshapes to 2 x 2 x nb */
        check(h, ekf_get_P_diag_blocks(h, mxGetPr(plhs[0])));
        return;
    }
    if (!strcmp(cmd, "set_state")) {              /* (h, x, P, s) */
        need(nrhs, 5, cmd);
        check(h, ekf_set_x(h, mxGetPr(prhs[2]), (int64_t)mxGetNumberOfElements(prhs[2])));
        check(h, ekf_set_s(h, mxGetPr(prhs[4]), (int64_t)mxGetNumberOfElements(prhs[4])));
        check(h, ekf_set_P(h, mxGetPr(prhs[3]), (int64_t)mxGetM(prhs[3])));
        return;
    }
    /* the reference's x, P, s are plain assignable properties (EKF_SLAM.m:6-9) */
    if (!strcmp(cmd, "set_x")) { need(nrhs, 3, cmd); check(h, ekf_set_x(h, mxGetPr(prhs[2]), (int64_t)mxGetNumberOfElements(prhs[2]))); return; }
    if (!strcmp(cmd, "set_P")) { need(nrhs, 3, cmd); check(h, ekf_set_P(h, mxGetPr(prhs[2]), (int64_t)mxGetM(prhs[2]))); return; }
    if (!strcmp(cmd, "set_s")) { need(nrhs, 3, cmd); check(h, ekf_set_s(h, mxGetPr(prhs[2]), (int64_t)mxGetNumberOfElements(prhs[2]))); return; }
    mexErrMsgIdAndTxt("ekfslam:usage", "unknown command '%s'", cmd);
}
