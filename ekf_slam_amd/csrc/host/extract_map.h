// Fragment of abi.hip, map extraction (ekf_extract_map): m landmarks of this handle and its robot taken out into ANOTHER handle on the same
// device, whose whole state is replaced -- the marginal as it is (EKF_FRAME_MAP) or relative to the robot (EKF_FRAME_ROBOT).  A SYNCHRONISING
// call on both handles, as ekf_join_map: the rungs of host/edits.h on the source, its stream drained before the destination's stream reads its
// buffers, the destination's stream drained before the call returns.  The source is only flushed.  The destination goes through what every
// replaced state goes through (ekf_checkpoint_load, ekf_load_lowrank_state): its loop settled, its asynchronous pass retired, a recorded
// predict dropped, the pair rings cleared, covariance_replaced, map_replaced, numbering_changed.  Unsharded only: the rows kernel writes
// every tile of the destination rows and reads tiles anywhere in the source store.
#pragma once
namespace {
// a step on the destination that failed: reported on the source handle, the destination's own message quoted
int32_t extract_dst_failed(ekf_handle *h, ekf_handle *dst, int32_t rc, const std::string &who) {
    return fail(h, rc, (who + "the destination handle: " + dst->err).c_str());
}
#define DST_HIPCHK(h, dst, who, call)                                                            \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess) { fail((dst), EKF_ERR_HIP, #call, e_); return extract_dst_failed((h), (dst), EKF_ERR_HIP, (who)); } \
    } while (0)
}  // namespace

extern "C" {
int32_t ekf_extract_map(ekf_handle *h, const int64_t *idx, int64_t m, int32_t frame, ekf_handle *dst) {
    if (!h) return EKF_ERR_INVALID_ARG;
    const std::string who = "extract_map: ";
    REQUIRE(h, dst != nullptr, EKF_ERR_INVALID_ARG, (who + "null destination handle").c_str());
    REQUIRE(h, dst != h, EKF_ERR_INVALID_ARG, (who + "a map cannot be extracted into itself").c_str());
    REQUIRE(h, m >= 0, EKF_ERR_INVALID_ARG, (who + "negative count").c_str());
    REQUIRE(h, m == 0 || idx != nullptr, EKF_ERR_INVALID_ARG, (who + "null index list").c_str());
    REQUIRE(h, frame == EKF_FRAME_MAP || frame == EKF_FRAME_ROBOT, EKF_ERR_INVALID_ARG, (who + "frame is EKF_FRAME_MAP or EKF_FRAME_ROBOT").c_str());
    {
        std::vector<int64_t> sorted(idx, idx + m);
        std::sort(sorted.begin(), sorted.end());
        REQUIRE(h, std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end(), EKF_ERR_INVALID_ARG, (who + "a landmark is named twice").c_str());
    }
    const char *why = "the extraction reads tiles anywhere in the source store and writes whole tile rows, and a shard holds only its own tiles";
    TRY(pair_unsharded(h, h, who, "the handle", why));
    TRY(pair_unsharded(h, dst, who, "the destination handle", why));
    REQUIRE(h, h->cfg.device == dst->cfg.device, EKF_ERR_INVALID_ARG, (who + "both handles must live on the same device").c_str());
    // both settled (N exact), then the indices and the capacity: all or nothing, before anything is flushed or replaced
    TRY(edit_settled(h, who));
    if (const int32_t rc = edit_settled(dst, who)) return extract_dst_failed(h, dst, rc, who);
    const int64_t N = h->N;
    for (int64_t k = 0; k < m; ++k)
        REQUIRE(h, idx[k] >= 0 && idx[k] < N, EKF_ERR_INDEX, (who + "landmark index outside the state; nothing was extracted").c_str());
    REQUIRE(h, m <= dst->cap, EKF_ERR_CAPACITY, (who + "capacity_landmarks of the destination cannot take the landmarks; nothing was extracted").c_str());
    if (!dst->d_xidx) {
        DST_HIPCHK(h, dst, who, dalloc(dst, &dst->d_xidx, (size_t)dst->cap));
        DST_HIPCHK(h, dst, who, hipDeviceSynchronize());   // dalloc clears on the null stream (see removal_alloc)
    }
    TRY(edit_flushed(h));
    // the destination: whatever speaks of its old state goes
    if (const int32_t rc = retire_inflight(dst)) return extract_dst_failed(h, dst, rc, who);       // (before clear_pairs: the pass reads the pair ring)
    dst->have_pp = false;
    DST_HIPCHK(h, dst, who, clear_pairs(dst));
    covariance_replaced(dst);
    HIPCHK(h, hipStreamSynchronize(h->stream));            // what the launches below read of the source has landed
    std::vector<int32_t> idx32((size_t)m);
    for (int64_t k = 0; k < m; ++k) idx32[(size_t)k] = (int32_t)idx[k];
    if (m > 0) DST_HIPCHK(h, dst, who, hipMemcpyAsync(dst->d_xidx, idx32.data(), (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, dst->stream));
    ExtractMapArgs a;
    a.m = m; a.cols = dst->st.tm.padded(2 * m); a.frame = frame; a.scur = h->cur; a.dcur = dst->cur;      // (written in place: dst's stream orders it)
    {
        TimedLaunch tl(h, EKF_KERNEL_COMPACT, dst->stream);
        DST_HIPCHK(h, dst, who, launch_extract_state(dst->st, h->st, a, dst->d_xidx, dst->stream));
    }
    if (m > 0) {
        TimedLaunch tl(h, EKF_KERNEL_COMPACT, dst->stream);
        DST_HIPCHK(h, dst, who, launch_extract_rows(dst->st, h->st, a, dst->d_xidx, dst->storage, h->storage, dst->stream));
    }
    // the destination's host side: N, the mirror of s from this handle's mirror (a mirror shorter than an index reads as zero, as
    // ekf_join_map takes it), what the new map makes stale, the work lists of the new tile-row count
    dst->N = m;
    dst->s_host.resize((size_t)m);
    for (int64_t k = 0; k < m; ++k) dst->s_host[(size_t)k] = idx[k] < (int64_t)h->s_host.size() ? h->s_host[(size_t)idx[k]] : 0.0;
    map_replaced(dst);
    numbering_changed(dst);
    int32_t rc = refresh_work(dst);
    // `idx32` is this call's stack, and the source may be edited or destroyed as soon as the call returns
    const hipError_t e = hipStreamSynchronize(dst->stream);
    if (rc) return extract_dst_failed(h, dst, rc, who);
    if (e != hipSuccess) { fail(dst, EKF_ERR_HIP, "hipStreamSynchronize(dst->stream)", e); return extract_dst_failed(h, dst, EKF_ERR_HIP, who); }
    return EKF_OK;
}
}  // extern "C"
