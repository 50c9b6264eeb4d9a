// Fragment of abi.hip, map edits (remove, constrain / merge / distance, a batch of merges, nearest): unsharded only, on a settled and flushed state -- the rungs below.
#pragma once
namespace {
// rung 1: the edit is not built for sharded handles (`why`: what its sharded form would need)
int32_t edit_unsharded(ekf_handle *h, const std::string &who, const char *why) {
    if (h->cfg.world == 1) return EKF_OK;
    return fail(h, EKF_ERR_INVALID_ARG, (who + "not built for sharded handles (world > 1): " + why).c_str());
}

// rung 1 of a call on TWO handles (join_map.h, extract_map.h), reported on `h`: `who_of` -- `which` names it -- runs no sharded code path in
// either sense (`why`: what the call would need of a shard)
int32_t pair_unsharded(ekf_handle *h, ekf_handle *who_of, const std::string &who, const char *which, const char *why) {
    if (who_of->cfg.world == 1 && !who_of->sharded) return EKF_OK;
    return fail(h, EKF_ERR_INVALID_ARG, (who + which + " is sharded (world > 1 or cfg.force_sharded): " + why).c_str());
}

// rung 2: no exchange pending, the device current, every queued row of the device loops settled (cfg.device_assoc == 4: N exact)
int32_t edit_settled(ekf_handle *h, const std::string &who) {
    if (h->pending) return fail(h, EKF_ERR_STATE, (who + "a sharded correction is between begin and finish").c_str());
    const int32_t rc = use_device(h);
    return rc ? rc : verify_loop(h, /*block*/ true);
}

// rung 3, as for every reader of P: a recorded predict carried out, the pending pairs applied, an asynchronous pass retired
int32_t edit_flushed(ekf_handle *h) { TRY(materialize_predict(h)); return flush_pending(h); }

// R of a constraint (column-major, nullptr: zero) into its entries; nullptr, or what is wrong with it (the caller's name goes in front)
const char *parse_R(const double R[4], double &r00, double &r01, double &r10, double &r11) {
    r00 = r01 = r10 = r11 = 0.0;
    if (R) colmajor2(R, r00, r01, r10, r11);
    if (!(std::isfinite(r00) && std::isfinite(r01) && std::isfinite(r10) && std::isfinite(r11))) return "R is not finite";
    if (!(r01 == r10 && r00 >= 0.0 && r11 >= 0.0 && r00 * r11 - r01 * r10 >= 0.0)) return "R must be symmetric with non-negative diagonal and determinant";
    return nullptr;
}

// A removal's buffers, everything that can fail for lack of memory, before anything changes: the second tile store (kept, as a handle with
// cfg.async_flush has it from the start), the map new landmark -> old landmark on both sides, the scratch the signatures are compacted into.
int32_t removal_alloc(ekf_handle *h) {
    const int64_t nmap = h->st.ldm / 2;
    const bool first_removal = !h->tilebuf[1] || !h->d_cmap || !h->d_s_tmp;
    if (!h->tilebuf[1]) {
        char *tiles2 = nullptr;
        HIPCHK(h, dalloc(h, &tiles2, (size_t)h->work_cap * h->T * h->T * elt_size(h)));
        h->tilebuf[1] = tiles2;
    }
    if (!h->d_cmap) HIPCHK(h, dalloc(h, &h->d_cmap, (size_t)nmap));
    if (!h->d_s_tmp) HIPCHK(h, dalloc(h, &h->d_s_tmp, (size_t)h->cap));
    // dalloc clears on the null stream, which the handle's (non-blocking) stream does not wait for: the clears must have landed
    // before anything below writes these buffers (ekf_create ends the same way)
    if (first_removal) HIPCHK(h, hipDeviceSynchronize());
    return stage_alloc(h, &h->h_cmap, (size_t)nmap * sizeof(int32_t), &h->ev_cmap);
}

// the map new landmark -> old landmark of the removal of rm (sorted, m entries) from N_old landmarks, uploaded in stream order
int32_t removal_upload_map(ekf_handle *h, const std::vector<int64_t> &rm, int64_t N_old) {
    const int64_t nmap = h->st.ldm / 2, m = (int64_t)rm.size();
    TRY(stage_wait(h, h->ev_cmap, h->cmap_busy));
    {
        int64_t q = 0, k = 0;
        for (int64_t l = 0; l < N_old; ++l) {
            if (q < m && rm[(size_t)q] == l) { ++q; continue; }
            h->h_cmap[k++] = (int32_t)l;
        }
        for (; k < nmap; ++k) h->h_cmap[k] = -1;
    }
    HIPCHK(h, hipMemcpyAsync(h->d_cmap, h->h_cmap, (size_t)nmap * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    return stage_uploaded(h, h->ev_cmap, h->cmap_busy);
}

// behind the tiles of a removal: x, the strip, the diagonal blocks and s compacted on the device, the host's mirror of s and N, what the
// new numbering makes stale, the work lists of the new tile-row count
int32_t removal_finish(ekf_handle *h, const std::vector<int64_t> &rm, int64_t N_old) {
    const size_t m = rm.size();
    HIPCHK(h, launch_compact_state(h->st, h->cur, h->d_cmap, N_old, h->d_s_tmp, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->st.s, h->d_s_tmp, (size_t)N_old * 8, hipMemcpyDeviceToDevice, h->stream));
    h->cur ^= 1;
    h->st.dcur ^= 1;
    // the host's side: the mirror of s (its sorted index is rebuilt at the next query) and N
    h->s_host.resize((size_t)N_old, 0.0);
    {
        size_t k = 0, q = 0;
        for (int64_t l = 0; l < N_old; ++l) {
            if (q < m && rm[q] == l) { ++q; continue; }
            h->s_host[k++] = h->s_host[(size_t)l];
        }
        h->s_host.resize(k);
    }
    h->N = N_old - (int64_t)m;
    map_replaced(h);
    numbering_changed(h);
    return refresh_work(h);                // the lists of the new tile-row count (both sets respected; no pass is in flight)
}
}  // namespace

extern "C" {
int32_t ekf_remove_landmarks(ekf_handle *h, const int64_t *idx, int64_t m) {
    if (!h) return EKF_ERR_INVALID_ARG;
    REQUIRE(h, m >= 0, EKF_ERR_INVALID_ARG, "remove_landmarks: negative count");
    if (m == 0) return EKF_OK;
    const std::string who = "remove_landmarks: ";
    TRY(edit_unsharded(h, who, "the tile owner is (I + J) mod world, so a compaction would move tiles between shards"));
    REQUIRE(h, idx != nullptr, EKF_ERR_INVALID_ARG, "remove_landmarks: null index list");
    TRY(edit_settled(h, who));
    const int64_t N_old = h->N;
    for (int64_t i = 0; i < m; ++i)
        REQUIRE(h, idx[i] >= 0 && idx[i] < N_old, EKF_ERR_INDEX, "remove_landmarks: landmark index outside the state");
    std::vector<int64_t> rm(idx, idx + m);
    std::sort(rm.begin(), rm.end());
    REQUIRE(h, std::adjacent_find(rm.begin(), rm.end()) == rm.end(), EKF_ERR_INVALID_ARG, "remove_landmarks: a landmark is named twice");
    TRY(removal_alloc(h));                 // everything that can fail for lack of memory, before anything changes
    TRY(edit_flushed(h));                  // the pending pairs speak of the old rows
    HIPCHK(h, clear_pairs(h));
    TRY(refresh_work(h));                  // the tiles of the OLD map, row by row: the destination tiles are a suffix of that list
    TRY(removal_upload_map(h, rm, N_old));
    {
        // Tile rows above the first removed landmark's do not change, and in tile-row-major order they are a prefix of the store; the
        // rest is compacted from the current store into the other one.  Then whichever is SMALLER moves: the prefix follows
        // (device to device) and the stores swap, or the compacted suffix is copied back and they do not -- at most 1.5 stores of
        // traffic either way instead of 2.
        const ekf_handle::WorkSet &ws = h->ws[h->ws_cur];
        const int64_t nt_old = ekf_tiles_for(2 * N_old, h->T);
        const int64_t slot0 = h->st.tm.row_base((2 * rm[0]) >> h->st.tm.shift), slot1 = h->st.tm.row_base(nt_old);
        REQUIRE(h, ws.rows == nt_old && ws.nwork == slot1 && slot1 <= h->work_cap, EKF_ERR_STATE, "remove_landmarks: work list out of step");
        const size_t tile_bytes = (size_t)h->T * h->T * elt_size(h);
        char *src = (char *)h->tilebuf[h->base], *dst = (char *)h->tilebuf[h->base ^ 1];
        TIMED(h, EKF_KERNEL_COMPACT, launch_compact_tiles(h->st.tm, src, dst, ws.work + slot0, slot1 - slot0, h->d_cmap, h->storage, h->stream));
        if (slot0 <= slot1 - slot0) {
            if (slot0 > 0) HIPCHK(h, hipMemcpyAsync(dst, src, (size_t)slot0 * tile_bytes, hipMemcpyDeviceToDevice, h->stream));
            h->base ^= 1;
            h->st.tiles = h->tilebuf[h->base];
        } else
            HIPCHK(h, hipMemcpyAsync(src + (size_t)slot0 * tile_bytes, dst + (size_t)slot0 * tile_bytes, (size_t)(slot1 - slot0) * tile_bytes,
                                     hipMemcpyDeviceToDevice, h->stream));
    }
    return removal_finish(h, rm, N_old);
}
}  // extern "C"

namespace {
// The three entry points of a constraint between two landmarks (kernels.h: ConstrainArgs) share everything up to
// the point where S = G H' + R and nu are on the host: `apply == false` (ekf_landmark_distance) stops there.
// Order: arguments -> the rungs, with the indices checked once N is exact -> S, nu -> the kernel, the one-pair pass.
int32_t constrain_impl(ekf_handle *h, const char *name, int64_t i, int64_t j, const double delta[2], const double R[4], bool apply,
                       double *d2_out, double S_out[4]) {
    const std::string who = std::string(name) + ": ";
    REQUIRE(h, i != j, EKF_ERR_INVALID_ARG, (who + "the two landmarks must differ").c_str());
    double d0 = 0.0, d1 = 0.0, r00, r01, r10, r11;
    if (delta) { d0 = delta[0]; d1 = delta[1]; }
    REQUIRE(h, std::isfinite(d0) && std::isfinite(d1), EKF_ERR_INVALID_ARG, (who + "delta is not finite").c_str());
    if (const char *bad = parse_R(R, r00, r01, r10, r11)) return fail(h, EKF_ERR_INVALID_ARG, (who + bad).c_str());
    TRY(edit_unsharded(h, who, "the pair needs the row-panels of two landmarks exchanged, and a merge ends in a compaction that would move "
                       "tiles between shards"));
    TRY(edit_settled(h, who));
    REQUIRE(h, i >= 0 && i < h->N && j >= 0 && j < h->N, EKF_ERR_INDEX, (who + "landmark index outside the state").c_str());
    TRY(edit_flushed(h));
    // S and nu on the host: both landmarks' own blocks (live F64 copies), their cross block (tiles), four entries of x
    HIPCHK(h, launch_constrain_probe(h->st, h->cur, 2 * i, 2 * j, h->d_csmall, h->storage, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->h_small, h->d_csmall, 14 * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const double *sm = h->h_small;
    const double Rr[4] = { r00, r01, r10, r11 };
    double S[4], d2;
    ekfm::constrain_S(sm, sm + 3, sm + 6, Rr, S);
    const double nu0 = d0 - (sm[10] - sm[12]), nu1 = d1 - (sm[11] - sm[13]);
    const bool regular = ekfm::constrain_d2(S, nu0, nu1, d2);       // the function k_nearest runs for every pair it reports
    if (S_out) { S_out[0] = S[0]; S_out[1] = S[2]; S_out[2] = S[1]; S_out[3] = S[3]; }       // column-major
    if (d2_out) *d2_out = d2;
    if (!apply) return EKF_OK;
    REQUIRE(h, regular, EKF_ERR_STATE, (who + "S = H P H' + R is not positive definite (two perfectly correlated identical landmarks and "
            "R = 0?); nothing was changed").c_str());
    TRY(refresh_work(h));
    ConstrainArgs a;
    a.d0 = d0; a.d1 = d1; a.R00 = r00; a.R01 = r01; a.R10 = r10; a.R11 = r11;
    a.ai = 2 * i; a.aj = 2 * j; a.n_mm = n_mm(h); a.cur = h->cur; a.npend = h->npend; a.pstart = h->pstart;     // (the ring is empty: 0, 0)
    TIMED(h, EKF_KERNEL_GATHER, launch_gather_constrain(h->st, a, h->storage, h->stream));
    h->cur ^= 1;
    h->st.dcur ^= 1;
    h->npend += 1;
    numbering_changed(h);                              // (the pass below drops the prefetched and the extracted row-panels)
    TRY(flush_pending(h));                             // the existing one-pair pass, before the call returns -- whatever cfg.batch says
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return EKF_OK;
}
}  // namespace

extern "C" {
int32_t ekf_constrain_landmarks(ekf_handle *h, int64_t i, int64_t j, const double delta[2], const double R[4]) {
    if (!h) return EKF_ERR_INVALID_ARG;
    return constrain_impl(h, "constrain_landmarks", i, j, delta, R, /*apply*/ true, nullptr, nullptr);
}

int32_t ekf_merge_landmarks(ekf_handle *h, int64_t keep, int64_t drop, const double R[4]) {
    if (!h) return EKF_ERR_INVALID_ARG;
    TRY(constrain_impl(h, "merge_landmarks", keep, drop, nullptr, R, /*apply*/ true, nullptr, nullptr));
    return ekf_remove_landmarks(h, &drop, 1);
}

int32_t ekf_landmark_distance(ekf_handle *h, int64_t i, int64_t j, const double delta[2], const double R[4], double *d2, double S[4]) {
    if (!h) return EKF_ERR_INVALID_ARG;
    if (!d2) return fail(h, EKF_ERR_INVALID_ARG, "landmark_distance: null d2");
    return constrain_impl(h, "landmark_distance", i, j, delta, R, /*apply*/ false, d2, S);
}

}  // extern "C"

namespace {
// ekf_merge_landmarks_batch, its own buffers (allocated at the first batch call and kept, as the second tile store is): the PRIVATE pair
// ring of EKF_MERGE_BATCH_MAX F64 slots (G ring, then K ring, as the handle's) -- the handle's ring has cfg.batch slots and an owner --,
// one record per constraint on both sides, and the snapshot of x / strip / Prr / the diagonal blocks behind the all-or-nothing rule
constexpr size_t kSnapPrr = 16;
size_t merge_snap_doubles(const ekf_handle *h) { return (size_t)(3 + h->st.ldm) + (size_t)(3 * h->st.ldm) + kSnapPrr + (size_t)(3 * h->cap); }
int32_t merge_batch_alloc(ekf_handle *h) {
    const bool first = !h->d_mring || !h->d_mrec || !h->d_msnap;
    if (!h->d_mring) HIPCHK(h, dalloc(h, &h->d_mring, (size_t)h->st.pair_stride * EKF_MERGE_BATCH_MAX * 2));
    if (!h->d_mrec) HIPCHK(h, dalloc(h, &h->d_mrec, (size_t)EKF_MERGE_BATCH_MAX * kConstrainRecordDoubles));
    if (!h->d_msnap) HIPCHK(h, dalloc(h, &h->d_msnap, merge_snap_doubles(h)));
    if (first) HIPCHK(h, hipDeviceSynchronize());          // dalloc clears on the null stream (see removal_alloc)
    if (!h->h_mrec) HIPCHK(h, halloc(h, &h->h_mrec, (size_t)EKF_MERGE_BATCH_MAX * kConstrainRecordDoubles * sizeof(double), hipHostMallocDefault));
    return EKF_OK;
}
// x, the strip, Prr and the diagonal blocks of the buffers (cur, dcur) into the snapshot, or back
hipError_t merge_snapshot(ekf_handle *h, int cur, int dcur, bool restore) {
    const size_t nx = (size_t)(3 + h->st.ldm), ns = (size_t)(3 * h->st.ldm), nd = (size_t)(3 * h->cap);
    double *snap = h->d_msnap;
    double *live[4] = { h->st.x[cur], h->st.strip[cur], h->st.prr[cur], h->st.diag[dcur] };
    const size_t cnt[4] = { nx, ns, kSnapPrr, nd };
    for (int q = 0; q < 4; ++q) {
        const hipError_t e = restore ? hipMemcpyAsync(live[q], snap, cnt[q] * 8, hipMemcpyDeviceToDevice, h->stream)
                                     : hipMemcpyAsync(snap, live[q], cnt[q] * 8, hipMemcpyDeviceToDevice, h->stream);
        if (e != hipSuccess) return e;
        snap += cnt[q];
    }
    return hipSuccess;
}
// the m chained constraints, queued back to back with no host wait, then ONE readback of their records; cur / st: where the chain
// leaves x / strip / Prr and the diagonal blocks (the handle's own indices are not touched)
int32_t merge_chain(ekf_handle *h, DevState &st, int &cur, const int64_t *keep, const int64_t *drop, int64_t m, const double Rr[4]) {
    for (int64_t k = 0; k < m; ++k) {
        ConstrainArgs a;
        a.d0 = 0.0; a.d1 = 0.0; a.R00 = Rr[0]; a.R01 = Rr[1]; a.R10 = Rr[2]; a.R11 = Rr[3];
        a.ai = 2 * keep[k]; a.aj = 2 * drop[k]; a.n_mm = n_mm(h); a.cur = cur; a.npend = (int32_t)k; a.pstart = 0;
        TIMED(h, EKF_KERNEL_GATHER, launch_gather_constrain_chain(st, a, h->d_mrec + k * kConstrainRecordDoubles, h->storage, h->stream));
        cur ^= 1;
        st.dcur ^= 1;
    }
    HIPCHK(h, hipMemcpyAsync(h->h_mrec, h->d_mrec, (size_t)m * kConstrainRecordDoubles * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return EKF_OK;
}
}  // namespace

extern "C" {
// Order as in constrain_impl: arguments -> the rungs, with the indices checked once N is exact -> every allocation -> the chain of m
// constraint gathers (nothing waits in between) -> their records -> the fused downdate-and-compact pass -> the rest of a removal.
int32_t ekf_merge_landmarks_batch(ekf_handle *h, const int64_t *keep, const int64_t *drop, int64_t m, const double R[4], double *d2) {
    if (!h) return EKF_ERR_INVALID_ARG;
    const std::string who = "merge_landmarks_batch: ";
    REQUIRE(h, m >= 0, EKF_ERR_INVALID_ARG, (who + "negative count").c_str());
    REQUIRE(h, m <= EKF_MERGE_BATCH_MAX, EKF_ERR_INVALID_ARG, (who + "more than EKF_MERGE_BATCH_MAX pairs").c_str());
    if (m == 0) return EKF_OK;
    REQUIRE(h, keep != nullptr && drop != nullptr, EKF_ERR_INVALID_ARG, (who + "null index list").c_str());
    for (int64_t k = 0; k < m; ++k) REQUIRE(h, keep[k] != drop[k], EKF_ERR_INVALID_ARG, (who + "the two landmarks of a pair must differ").c_str());
    std::vector<int64_t> rm(drop, drop + m);
    std::sort(rm.begin(), rm.end());
    REQUIRE(h, std::adjacent_find(rm.begin(), rm.end()) == rm.end(), EKF_ERR_INVALID_ARG, (who + "a landmark is dropped twice").c_str());
    for (int64_t k = 0; k < m; ++k)
        REQUIRE(h, !std::binary_search(rm.begin(), rm.end(), keep[k]), EKF_ERR_INVALID_ARG,
                (who + "a landmark is both kept and dropped (every keep survives: order a chain yourself)").c_str());
    double r00, r01, r10, r11;
    if (const char *bad = parse_R(R, r00, r01, r10, r11)) return fail(h, EKF_ERR_INVALID_ARG, (who + bad).c_str());
    TRY(edit_unsharded(h, who, "the pairs need the row-panels of their landmarks exchanged, and the batch ends in a compaction that would move "
                       "tiles between shards"));
    TRY(edit_settled(h, who));
    const int64_t N_old = h->N;
    for (int64_t k = 0; k < m; ++k)
        REQUIRE(h, keep[k] >= 0 && keep[k] < N_old && drop[k] >= 0 && drop[k] < N_old, EKF_ERR_INDEX, (who + "landmark index outside the state").c_str());
    // everything that can fail for lack of memory, before anything changes
    TRY(merge_batch_alloc(h));
    TRY(removal_alloc(h));
    TRY(edit_flushed(h));
    HIPCHK(h, clear_pairs(h));             // (the handle's own ring: the map is about to shrink)
    TRY(refresh_work(h));                  // the tiles of the OLD map: the fused pass writes every one of them
    TRY(removal_upload_map(h, rm, N_old));
    const ekf_handle::WorkSet &ws = h->ws[h->ws_cur];
    const int64_t nt_old = ekf_tiles_for(2 * N_old, h->T), slot1 = h->st.tm.row_base(nt_old);
    REQUIRE(h, ws.rows == nt_old && ws.nwork == slot1 && slot1 <= h->work_cap, EKF_ERR_STATE, (who + "work list out of step").c_str());
    // the chain, on a view of the state whose pair ring is the batch's own: the handle's ring bookkeeping is not involved
    DevState st = h->st;
    st.Gp = h->d_mring; st.Kp = h->d_mring + (size_t)h->st.pair_stride * EKF_MERGE_BATCH_MAX; st.pcap = EKF_MERGE_BATCH_MAX;
    st.Gp32 = nullptr; st.Kp32 = nullptr;
    int cur = h->cur;
    const double Rr[4] = { r00, r01, r10, r11 };
    HIPCHK(h, merge_snapshot(h, h->cur, h->st.dcur, /*restore*/ false));
    int32_t rc = merge_chain(h, st, cur, keep, drop, m, Rr);
    int64_t bad = -1;
    if (!rc)
        for (int64_t k = 0; k < m && bad < 0; ++k)
            if (h->h_mrec[k * kConstrainRecordDoubles + 7] != 1.0) bad = k;
    if (rc || bad >= 0) {
        // all or nothing: the tiles were not written; x, the strip, Prr and the diagonal blocks go back into the buffers they came from
        const std::string err = h->err;
        if (merge_snapshot(h, h->cur, h->st.dcur, /*restore*/ true) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess)
            return fail(h, EKF_ERR_HIP, (who + "the state could not be restored after a failed batch").c_str());
        if (rc) { h->err = err; return rc; }
        return fail(h, EKF_ERR_STATE, (who + "pair " + std::to_string(bad) + ": S = H P H' + R is not positive definite (two perfectly correlated "
                    "identical landmarks and R = 0?); nothing was changed").c_str());
    }
    {
        // ONE pass: the m pairs applied while the store is compacted into the other one, over every tile of the old map; then the stores swap.
        // A launch that fails leaves the current store as it was: the snapshot goes back, as for an irregular pair.
        TimedLaunch tl(h, EKF_KERNEL_DOWNDATE);
        const hipError_t e = launch_merge_pass(st, h->tilebuf[h->base ^ 1], ws.work, slot1, h->d_cmap, (int)m, h->storage, h->stream, h->dd_kernel);
        if (e != hipSuccess) {
            if (merge_snapshot(h, h->cur, h->st.dcur, /*restore*/ true) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess)
                return fail(h, EKF_ERR_HIP, (who + "the state could not be restored after a failed batch").c_str());
            return fail(h, EKF_ERR_HIP, (who + "the fused pass could not be launched; nothing was changed").c_str(), e);
        }
        h->dd_pairs = (int32_t)m;
    }
    // From here on the batch is committed: x / strip / Prr / diag carry the m pairs and so does the new store.  (An EKF_ERR_HIP out of the
    // removal's tail below -- queued copies and one small kernel -- would leave the handle between two maps: reload the state then.)
    h->cur = cur;
    h->st.dcur = st.dcur;
    h->base ^= 1;
    h->st.tiles = h->tilebuf[h->base];
    TRY(removal_finish(h, rm, N_old));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (d2) for (int64_t k = 0; k < m; ++k) d2[k] = h->h_mrec[k * kConstrainRecordDoubles + 6];
    return EKF_OK;
}

// Order as in constrain_impl: arguments -> the rungs -> the one read-only pass (k_nearest) -> the N entries through the pinned area.
int32_t ekf_nearest_landmarks(ekf_handle *h, const double R[4], double *d2, int64_t *partner) {
    if (!h) return EKF_ERR_INVALID_ARG;
    REQUIRE(h, h->N == 0 || (d2 && partner), EKF_ERR_INVALID_ARG, "nearest_landmarks: null argument");
    const std::string who = "nearest_landmarks: ";
    double r00, r01, r10, r11;
    if (const char *bad = parse_R(R, r00, r01, r10, r11)) return fail(h, EKF_ERR_INVALID_ARG, (who + bad).c_str());
    TRY(edit_unsharded(h, who, "the search reads every tile of the lower triangle, and a shard holds only its own"));
    TRY(edit_settled(h, who));
    REQUIRE(h, h->N == 0 || (d2 && partner), EKF_ERR_INVALID_ARG, "nearest_landmarks: null argument");      // (N is exact only now)
    TRY(edit_flushed(h));
    const int64_t N = h->N;
    if (N == 0) return EKF_OK;
    if (!h->d_nearest) {
        HIPCHK(h, dalloc(h, &h->d_nearest, (size_t)h->cap));
        HIPCHK(h, hipDeviceSynchronize());             // dalloc clears on the null stream (see ekf_remove_landmarks)
    }
    if (!h->h_nearest) HIPCHK(h, halloc(h, &h->h_nearest, (size_t)h->cap * sizeof(NearestEntry), hipHostMallocDefault));
    const double Rr[4] = { r00, r01, r10, r11 };
    TIMED(h, EKF_KERNEL_ASSOCIATE, launch_nearest(h->st, h->cur, N, Rr, h->d_nearest, h->storage, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->h_nearest, h->d_nearest, (size_t)N * sizeof(NearestEntry), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int64_t i = 0; i < N; ++i) { d2[i] = h->h_nearest[i].d2; partner[i] = h->h_nearest[i].partner; }
    return EKF_OK;
}
}  // extern "C"
