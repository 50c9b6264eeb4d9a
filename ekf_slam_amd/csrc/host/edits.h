// Fragment of abi.hip, map edits (remove, constrain / merge / distance, nearest): unsharded only, on a settled and flushed state -- the rungs below.
#pragma once
namespace {
// rung 1: the edit is not built for sharded handles (`why`: what its sharded form would need)
int32_t edit_unsharded(ekf_handle *h, const std::string &who, const char *why) {
    if (h->cfg.world == 1) return EKF_OK;
    return fail(h, EKF_ERR_INVALID_ARG, (who + "not built for sharded handles (world > 1): " + why).c_str());
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
    // everything that can fail for lack of memory, before anything changes
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
    TRY(stage_alloc(h, &h->h_cmap, (size_t)nmap * sizeof(int32_t), &h->ev_cmap));
    TRY(edit_flushed(h));                  // the pending pairs speak of the old rows
    HIPCHK(h, clear_pairs(h));
    TRY(refresh_work(h));                  // the tiles of the OLD map, row by row: the destination tiles are a suffix of that list
    const int64_t N_new = N_old - m;
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
    TRY(stage_uploaded(h, h->ev_cmap, h->cmap_busy));
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
    HIPCHK(h, launch_compact_state(h->st, h->cur, h->d_cmap, N_old, h->d_s_tmp, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->st.s, h->d_s_tmp, (size_t)N_old * 8, hipMemcpyDeviceToDevice, h->stream));
    h->cur ^= 1;
    h->st.dcur ^= 1;
    // the host's side: the mirror of s (its sorted index is rebuilt at the next query) and N
    h->s_host.resize((size_t)N_old, 0.0);
    {
        size_t k = 0, q = 0;
        for (int64_t l = 0; l < N_old; ++l) {
            if (q < (size_t)m && rm[q] == l) { ++q; continue; }
            h->s_host[k++] = h->s_host[(size_t)l];
        }
        h->s_host.resize(k);
    }
    h->N = N_new;
    map_replaced(h);
    numbering_changed(h);
    return refresh_work(h);                // the lists of the new tile-row count (both sets respected; no pass is in flight)
}
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
