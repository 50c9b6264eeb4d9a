// Fragment of abi.hip, the frame of a map (ekf_transform_map): the WHOLE state of this handle moved by a rigid transform with its own
// covariance (EKF_FRAME_MAP) or into the frame of its robot's pose (EKF_FRAME_ROBOT), in place -- no second handle.  A SYNCHRONISING call
// on the rungs of host/edits.h: a recorded predict carried out, the pending pairs applied, an asynchronous pass retired, the stream drained
// before the call returns.  N, s and the numbering stay; x, the strip and every tile change: map_replaced and covariance_replaced.
// Unsharded only: the tile kernel walks the unsharded work list.
#pragma once
namespace {
// Sigma of a rigid transform (column-major, nullptr: zero) into row-major entries; nullptr, or what is wrong with it.  *zero: every entry is 0
const char *parse_Sigma(const double Sigma[9], double S[9], bool *zero) {
    for (int i = 0; i < 9; ++i) S[i] = 0.0;
    *zero = true;
    if (!Sigma) return nullptr;
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) S[3 * r + c] = Sigma[3 * c + r];
    for (int i = 0; i < 9; ++i) {
        if (!std::isfinite(S[i])) return "Sigma is not finite";
        if (S[i] != 0.0) *zero = false;
    }
    if (!(S[1] == S[3] && S[2] == S[6] && S[5] == S[7])) return "Sigma must be symmetric";
    const double m2 = S[0] * S[4] - S[1] * S[3];
    const double m3 = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6]);
    if (!(S[0] >= 0.0 && S[4] >= 0.0 && S[8] >= 0.0 && m2 >= 0.0 && m3 >= 0.0))
        return "Sigma must have a non-negative diagonal and non-negative leading principal minors";
    return nullptr;
}
}  // namespace

extern "C" {
// Order as in constrain_impl: arguments -> the rungs -> the two launches (neither reads what the other writes) -> the flips, what the new
// state makes stale -> the stream drained.
int32_t ekf_transform_map(ekf_handle *h, int32_t frame, const double t[3], const double Sigma[9]) {
    if (!h) return EKF_ERR_INVALID_ARG;
    const std::string who = "transform_map: ";
    REQUIRE(h, frame == EKF_FRAME_MAP || frame == EKF_FRAME_ROBOT, EKF_ERR_INVALID_ARG, (who + "frame is EKF_FRAME_MAP or EKF_FRAME_ROBOT").c_str());
    TransformMapArgs a = {};
    if (frame == EKF_FRAME_MAP) {
        REQUIRE(h, t != nullptr, EKF_ERR_INVALID_ARG, (who + "EKF_FRAME_MAP needs the transform t").c_str());
        REQUIRE(h, std::isfinite(t[0]) && std::isfinite(t[1]) && std::isfinite(t[2]), EKF_ERR_INVALID_ARG, (who + "t is not finite").c_str());
        bool zero;
        if (const char *bad = parse_Sigma(Sigma, a.Sigma, &zero)) return fail(h, EKF_ERR_INVALID_ARG, (who + bad).c_str());
        for (int i = 0; i < 3; ++i) a.t[i] = t[i];
        a.form = zero ? 0 : 1;
    } else {
        REQUIRE(h, t == nullptr && Sigma == nullptr, EKF_ERR_INVALID_ARG, (who + "EKF_FRAME_ROBOT takes neither t nor Sigma").c_str());
        a.form = 2;
    }
    TRY(edit_unsharded(h, who, "the tile kernel walks the unsharded work list (the exact rigid form would need no exchange: every block "
                       "depends on itself and on replicated data alone)"));
    TRY(edit_settled(h, who));
    TRY(edit_flushed(h));
    TRY(refresh_work(h));
    const ekf_handle::WorkSet &ws = h->ws[h->ws_cur];
    const int64_t N = h->N, nt = ekf_tiles_for(2 * N, h->T);
    REQUIRE(h, ws.rows == nt && ws.nwork == h->st.tm.row_base(nt) && ws.nwork <= h->work_cap, EKF_ERR_STATE, (who + "work list out of step").c_str());
    a.N = N; a.cols = h->st.tm.padded(2 * N); a.cur = h->cur;
    TIMED(h, EKF_KERNEL_COMPACT, launch_transform_state(h->st, a, h->stream));
    if (N > 0) TIMED(h, EKF_KERNEL_COMPACT, launch_transform_tiles(h->st, a, ws.work, ws.nwork, h->storage, h->stream));
    h->cur ^= 1;
    h->st.dcur ^= 1;
    covariance_replaced(h);
    map_replaced(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return EKF_OK;
}
}  // extern "C"
