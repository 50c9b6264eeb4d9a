// Fragment of abi.hip, map joining (ekf_join_map): a local handle's map joined behind this handle's, both on one device.  A SYNCHRONISING
// call on both handles -- the rungs of host/edits.h on each, the local stream drained before this handle's stream reads its buffers, this
// handle's stream drained before the call returns -- so the caller may destroy or edit the local handle at once.  Unsharded only: the rows
// kernel writes every tile of the new rows and reads every tile of the local store.
#pragma once
extern "C" {
int32_t ekf_join_map(ekf_handle *h, ekf_handle *local, double signature_offset, int64_t *first_idx) {
    if (!h) return EKF_ERR_INVALID_ARG;
    const std::string who = "join_map: ";
    REQUIRE(h, local != nullptr, EKF_ERR_INVALID_ARG, (who + "null local handle").c_str());
    REQUIRE(h, local != h, EKF_ERR_INVALID_ARG, (who + "a map cannot be joined into itself").c_str());
    REQUIRE(h, std::isfinite(signature_offset), EKF_ERR_INVALID_ARG, (who + "signature_offset is not finite").c_str());
    const char *why = "the join writes and reads whole tile rows, and a shard holds only its own tiles";
    TRY(pair_unsharded(h, h, who, "the handle", why));
    TRY(pair_unsharded(h, local, who, "the local handle", why));
    REQUIRE(h, h->cfg.device == local->cfg.device, EKF_ERR_INVALID_ARG, (who + "both handles must live on the same device").c_str());
    // both settled (N and M exact), then the capacity: all or nothing, before anything is flushed
    TRY(edit_settled(h, who));
    if (const int32_t rc = edit_settled(local, who)) return fail(h, rc, (who + "the local handle: " + local->err).c_str());
    const int64_t N = h->N, M = local->N;
    REQUIRE(h, N + M <= h->cap, EKF_ERR_CAPACITY, (who + "capacity_landmarks cannot take the whole local map; nothing was joined").c_str());
    if (const int32_t rc = edit_flushed(local)) return fail(h, rc, (who + "the local handle: " + local->err).c_str());
    TRY(edit_flushed(h));
    HIPCHK(h, hipStreamSynchronize(local->stream));        // what the launches below read of it has landed
    JoinMapArgs a;
    a.N = N; a.M = M; a.signature_offset = signature_offset; a.cur = h->cur; a.lcur = local->cur;
    TIMED(h, EKF_KERNEL_APPEND, launch_join_state(h->st, local->st, a, h->stream));
    if (M > 0) TIMED(h, EKF_KERNEL_APPEND, launch_join_rows(h->st, local->st, a, h->storage, local->storage, h->stream));
    h->cur ^= 1;
    // the host's mirror of s takes what the kernel wrote (a local mirror shorter than M reads as zeros, as removal_finish takes it)
    for (int64_t i = 0; i < M; ++i) note_append(h, (i < (int64_t)local->s_host.size() ? local->s_host[(size_t)i] : 0.0) + signature_offset);
    if (first_idx) *first_idx = N;
    HIPCHK(h, hipStreamSynchronize(h->stream));            // the local handle may be edited or destroyed as soon as the call returns
    return EKF_OK;
}
}  // extern "C"
