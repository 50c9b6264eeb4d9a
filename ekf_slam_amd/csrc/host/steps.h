// Fragment of abi.hip, the steps: predict (recorded, carried out lazily), append, correct, the end of an update-step; a shard's _begin / _finish halves.
#pragma once
namespace {
int32_t verify_loop(ekf_handle *h, bool block);                          // assoc.h
void note_append(ekf_handle *h, double signature);

int32_t materialize_predict(ekf_handle *h) {
    if (!h->have_pp) return EKF_OK;
    h->have_pp = false;
    PredictArgs a = h->pp;
    a.n_mm = 2 * n_hi(h); a.cur = h->cur;         // (cfg.device_assoc == 4: columns beyond the device's count are never read)
    TIMED(h, EKF_KERNEL_PREDICT, launch_predict(h->st, a, h->storage, h->stream));
    h->cur ^= 1;
    return EKF_OK;
}

int32_t do_predict(ekf_handle *h, const double u[2]) {
    TRY(materialize_predict(h));           // an earlier predict that nothing consumed yet
    h->pp.u0 = u[0]; h->pp.u1 = u[1]; h->pp.C = h->cfg.C; h->pp.n_mm = 0; h->pp.cur = 0;
    h->have_pp = true;
    static const bool lazy = ekf_tune_int("EKF_LAZY_PREDICT", 1) != 0;
    return lazy ? EKF_OK : materialize_predict(h);
}

// device + every deferred host-side decision that the caller's next read depends on
int32_t enter(ekf_handle *h) {
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int32_t rc = verify_loop(h, /*block*/ true);
    return rc ? rc : materialize_predict(h);
}

// ... and every pending pair applied: what a reader of the tiles needs
int32_t enter_flushed(ekf_handle *h) { TRY(enter(h)); return flush_pending(h); }

int32_t do_append(ekf_handle *h, const double u[2], const double R[4], const double pos[2], double signature,
                  const DevLoopArgs *dl = nullptr) {
    REQUIRE(h, h->N < h->cap, EKF_ERR_CAPACITY, "append: capacity_landmarks exhausted");
    // A pass in flight (cfg.async_flush) is not waited for: the new rows are written to the store the main stream reads (the one the pass
    // reads too) and copied to the pass's output when it retires -- the pass leaves rows that did not exist at its launch as they are (its
    // pairs have K = 0 there), and k_append writes nothing but the new landmark's own two rows of the tiles.
    if (h->inflight) h->appended_inflight = true;
    AppendArgs a;
    a.u0 = u[0]; a.u1 = u[1];
    colmajor2(R, a.R00, a.R01, a.R10, a.R11);
    a.pos0 = pos[0]; a.pos1 = pos[1]; a.signature = signature; a.N = h->N; a.cur = h->cur;
    {
        // a recorded predict is carried out by the append launch itself (k_append<.., kPredict>): the state moves to the other buffer
        PredictArgs pa = h->pp;
        pa.n_mm = n_mm(h); pa.cur = h->cur;
        const PredictArgs *fuse = h->have_pp ? &pa : nullptr;
        TIMED(h, EKF_KERNEL_APPEND, launch_append(h->st, a, h->storage, h->stream, dl, fuse));
        if (fuse) { h->have_pp = false; h->cur ^= 1; }
    }
    note_append(h, signature);
    return EKF_OK;
}

// the host's side of an append: the mirror of s, N, what the map's growth invalidates
void note_append(ekf_handle *h, double signature) {
    if ((int64_t)h->s_host.size() > h->N) { h->s_host.resize((size_t)h->N); h->s_sorted_ok = false; }
    h->s_host.push_back(signature);
    if (h->s_sorted_ok && signature == signature)         // the index learns of it through its unsorted tail; NaN never matches anything
        h->s_tail.emplace_back(signature, h->N);
    h->N += 1;
    map_grew(h);
}

constexpr int kThrottle = 48;

// run-ahead throttle (see ekf_handle::throttle_ev): called once per update-step
int32_t throttle_step(ekf_handle *h) {
    if (++h->since_mark >= kThrottle) {
        h->since_mark = 0;
        const int k = h->throttle_k;
        if (!h->throttle_ev[k]) HIPCHK(h, new_event(h, &h->throttle_ev[k]));
        HIPCHK(h, hipEventRecord(h->throttle_ev[k], h->stream));
        h->throttle_set[k] = true;
        if (h->throttle_set[k ^ 1]) HIPCHK(h, hipEventSynchronize(h->throttle_ev[k ^ 1]));   // the mark before this one
        h->throttle_k = k ^ 1;
    }
    return EKF_OK;
}

int32_t finish_step(ekf_handle *h) {
    h->cur ^= 1;
    h->st.dcur ^= 1;           // the gather wrote the diagonal blocks' live copies, with its pair applied, to the other buffer
    h->npend += 1;
    const int32_t rc = (h->npend - h->nfrozen) >= h->batch ? batch_complete(h) : EKF_OK;
    h->hint_idx = -1;          // a hint speaks of the correction that follows THIS one only
    return rc ? rc : throttle_step(h);
}

void fill_correct_args(ekf_handle *h, CorrectArgs &a, const double z[2], const double R[4], int64_t idx) {
    a.z0 = z[0]; a.z1 = z[1];
    colmajor2(R, a.R00, a.R01, a.R10, a.R11);
    a.j = 2 * idx; a.n_mm = n_mm(h); a.cur = h->cur; a.npend = h->npend; a.pstart = h->pstart;
}

// the sharded gather on `panels` (the receive area after an exchange, or the prefetched panels), a recorded predict folded in
int32_t gather_sharded(ekf_handle *h, const CorrectArgs &a, const double *panels, int64_t stride, int64_t off, bool patched,
                       const DevLoopArgs *dl = nullptr) {
    const PredictArgs *fuse = h->have_pp ? &h->pp : nullptr;
    TIMED(h, EKF_KERNEL_GATHER, launch_gather_sharded(h->st, a, fuse, panels, stride, off, patched, h->storage, h->stream, dl));
    h->have_pp = false;
    return EKF_OK;
}

// slot of landmark idx among the prefetched base row-panels, or -1
int prefetch_slot(const ekf_handle *h, int64_t idx) {
    if (!h->pf_valid || h->pf_N != h->N) return -1;
    for (int q = 0; q < h->pf_m; ++q) if (h->pf_idx[(size_t)q] == idx) return q;
    return -1;
}

int32_t correct_begin(ekf_handle *h, const double z[2], const double R[4], int64_t idx) {
    REQUIRE(h, idx >= 0 && idx < h->N, EKF_ERR_INDEX, "correct: landmark index outside the state");
    REQUIRE(h, !h->pending, EKF_ERR_STATE, "correct_begin: an exchange is already pending");
    TRY(refresh_work(h));
    fill_correct_args(h, h->pending_args, z, R, idx);
    h->slab = slab_for(h, h->pending_args.n_mm);
    // unless the last pass over P left this row-panel in the send area (ekf_hint_next): nothing to extract then
    if (!(h->nx_valid && h->nx_idx == idx && h->nx_N == h->N && h->npend == 0))
        TIMED(h, EKF_KERNEL_ROWPANEL, launch_rowpanel(h->st, h->pending_args.j, h->pending_args.n_mm, h->pstart, h->npend, corr_send(h, h->slab),
              h->storage, h->stream));
    exchange_changed(h);       // (consumed, or overwritten by this correction's own extraction and all-gather)
    h->pending = true; h->pending_kind = 1; h->x_count = h->slab;
    return EKF_OK;
}

int32_t correct_finish(ekf_handle *h) {
    REQUIRE(h, h->pending && h->pending_kind == 1, EKF_ERR_STATE, "correct_finish: no correction pending");
    h->pending = false; h->pending_kind = 0;
    const int32_t rc = gather_sharded(h, h->pending_args, h->recv, h->slab, 0, /*patched*/ true);
    return rc ? rc : finish_step(h);
}

// copy the BASE row-panels (no pending pairs applied: they are applied at correction time) of m landmarks into
// the send buffer; after the all-gather the corrections on these landmarks need no exchange of their own
int32_t prefetch_begin(ekf_handle *h, const int64_t *idx, int32_t m) {
    REQUIRE(h, !h->pending, EKF_ERR_STATE, "prefetch_begin: an exchange is already pending");
    REQUIRE(h, m >= 1 && m <= h->batch, EKF_ERR_INVALID_ARG, "prefetch: between 1 and cfg.batch landmarks");
    for (int32_t q = 0; q < m; ++q)
        REQUIRE(h, idx[q] >= 0 && idx[q] < h->N, EKF_ERR_INDEX, "prefetch: landmark index outside the state");
    const int64_t slab = slab_for(h, n_mm(h));
    TIMED(h, EKF_KERNEL_ROWPANEL, launch_rowpanel_base(h->st, idx, m, n_mm(h), h->send, slab, h->storage, h->stream));
    tiles_changed(h);       // (a new prefetch starts)
    h->pf_idx.assign(idx, idx + m);
    h->pf_m = m; h->pf_slab = slab; h->pf_N = h->N;
    h->pending = true; h->pending_kind = 2; h->x_count = (int64_t)m * slab;
    return EKF_OK;
}

int32_t prefetch_finish(ekf_handle *h) {
    REQUIRE(h, h->pending && h->pending_kind == 2, EKF_ERR_STATE, "prefetch_finish: no prefetch pending");
    h->pending = false; h->pending_kind = 0;
    HIPCHK(h, store_panels(h, h->stream));
    h->pf_valid = true;
    return EKF_OK;
}

int32_t do_correct(ekf_handle *h, const double z[2], const double R[4], int64_t idx) {
    REQUIRE(h, idx >= 0 && idx < h->N, EKF_ERR_INDEX, "correct: landmark index outside the state");
    if (h->sharded) {
        const int q = prefetch_slot(h, idx);
        if (q >= 0 && slab_for(h, n_mm(h)) == h->pf_slab) {
            // base row-panel already on every shard: no exchange, pending pairs applied inside the gather
            REQUIRE(h, !h->pending, EKF_ERR_STATE, "correct: an exchange is pending");
            CorrectArgs a;
            fill_correct_args(h, a, z, R, idx);
            const int32_t rc = gather_sharded(h, a, h->pf_store, (int64_t)h->pf_m * h->pf_slab, (int64_t)q * h->pf_slab, /*patched*/ false);
            return rc ? rc : finish_step(h);
        }
        int32_t rc = correct_begin(h, z, R, idx);
        if (!rc) rc = run_exchange(h);
        return rc ? rc : correct_finish(h);
    }
    TRY(refresh_work(h));
    CorrectArgs a;
    fill_correct_args(h, a, z, R, idx);
    // small maps (one workgroup covers every column), every correction rewriting P at once: the downdate runs inside the gather
    // kernel -- one launch per update-step instead of two
    static const bool fuse_small = ekf_tune_int("EKF_FUSE_SMALL", 1) != 0;
    const bool fused = fuse_small && h->batch == 1 && !h->async_flush && h->npend == 0 && a.n_mm <= gather_fuse_max_rows() &&
                       ekf_tiles_for(a.n_mm, h->T) * h->T <= 256;
    const PredictArgs *fuse = h->have_pp ? &h->pp : nullptr;
    TIMED(h, EKF_KERNEL_GATHER, launch_gather(h->st, a, fuse, h->storage, h->stream, fused));
    h->have_pp = false;
    if (fused) {                     // the pair never became pending: nothing to flush, only the double buffers flip
        h->cur ^= 1;
        h->st.dcur ^= 1;
        snprintf(h->dd_kernel, sizeof h->dd_kernel, "k_gather<%s,fused downdate>", h->storage == EKF_STORE_F64 ? "double" : "float");
        h->dd_pairs = 1;
        return throttle_step(h);
    }
    return finish_step(h);
}

// device-resident measure loop: the correction of the landmark the DEVICE's association names (dl.parts_in); idx, the host
// mirror's prediction, only keeps a launch whose winners name nothing inside the state.  Never the small-map fused form.
int32_t do_correct_dev(ekf_handle *h, const double z[2], const double R[4], int64_t idx, const DevLoopArgs &dl) {
    REQUIRE(h, idx >= 0 && idx < h->N, EKF_ERR_INDEX, "correct: landmark index outside the state");
    TRY(refresh_work(h));
    CorrectArgs a;
    fill_correct_args(h, a, z, R, idx);
    if (h->sharded) {
        // a shard: extraction of the row-panel of the landmark the DEVICE names (every shard holds the same winners: the association
        // runs on replicated data -- x, s, the strip, the live diagonal blocks), the all-gather, the gather on the exchanged panel
        REQUIRE(h, !h->pending, EKF_ERR_STATE, "correct: an exchange is pending");
        h->slab = slab_for(h, a.n_mm);
        TIMED(h, EKF_KERNEL_ROWPANEL, launch_rowpanel_dev(h->st, a.j, a.n_mm, h->pstart, h->npend, corr_send(h, h->slab), h->storage, h->stream, dl));
        exchange_changed(h);
        h->x_count = h->slab;
        TRY(exchange_bracket(h, 1));
        TRY(gather_sharded(h, a, h->recv, h->slab, 0, /*patched*/ true, &dl));
        return finish_step(h);
    }
    const PredictArgs *fuse = h->have_pp ? &h->pp : nullptr;
    TIMED(h, EKF_KERNEL_GATHER, launch_gather_devloop(h->st, a, fuse, dl, h->storage, h->stream));
    h->have_pp = false;
    return finish_step(h);
}
}  // namespace

extern "C" {
int32_t ekf_correct_begin(ekf_handle *h, const double z[2], const double R[4], int64_t idx) {
    if (!h || !z || !R) return fail(h, EKF_ERR_INVALID_ARG, "correct_begin: null argument");
    REQUIRE(h, h->sharded, EKF_ERR_STATE, "correct_begin: handle is not sharded (use ekf_correct)");
    int32_t rc = use_device(h);
    return rc ? rc : correct_begin(h, z, R, idx);
}

int32_t ekf_correct_finish(ekf_handle *h) {
    if (!h) return EKF_ERR_INVALID_ARG;
    int32_t rc = use_device(h);
    return rc ? rc : correct_finish(h);
}

int32_t ekf_prefetch_begin(ekf_handle *h, const int64_t *idx, int32_t m) {
    if (!h || !idx) return fail(h, EKF_ERR_INVALID_ARG, "prefetch_begin: null argument");
    REQUIRE(h, h->sharded, EKF_ERR_STATE, "prefetch_begin: handle is not sharded");
    int32_t rc = use_device(h);
    return rc ? rc : prefetch_begin(h, idx, m);
}

int32_t ekf_prefetch_finish(ekf_handle *h) {
    if (!h) return EKF_ERR_INVALID_ARG;
    int32_t rc = use_device(h);
    return rc ? rc : prefetch_finish(h);
}

int32_t ekf_prefetch_rows(ekf_handle *h, const int64_t *idx, int32_t m) {
    if (!h || !idx) return fail(h, EKF_ERR_INVALID_ARG, "prefetch_rows: null argument");
    if (!h->sharded) return EKF_OK;                  // nothing to exchange on an unsharded handle
    TRY(use_device(h));
    TRY(prefetch_begin(h, idx, m));
    TRY(run_exchange(h));
    return prefetch_finish(h);
}

int32_t ekf_prefetch_next(ekf_handle *h, const int64_t *idx, int32_t m) {
    if (!h || (m > 0 && !idx) || m < 0) return fail(h, EKF_ERR_INVALID_ARG, "prefetch_next: bad argument");
    if (!h->sharded) return EKF_OK;                  // nothing to exchange on an unsharded handle
    drop_announced(h);
    if (m == 0) return EKF_OK;
    REQUIRE(h, h->batch > 1 && !h->async_flush, EKF_ERR_STATE, "prefetch_next: needs cfg.batch > 1 and a synchronous flush");
    REQUIRE(h, h->cfg.pass_arith == EKF_ARITH_F64, EKF_ERR_STATE,
            "prefetch_next: with cfg.pass_arith = EKF_ARITH_F32 the pass's result is not what an extraction in front of it can compute");
    REQUIRE(h, h->comm != nullptr || h->xhook != nullptr, EKF_ERR_STATE,
            "prefetch_next: needs the library-owned communicator (ekf_comm_init) or an exchange hook (ekf_exchange_set_hook)");
    REQUIRE(h, m <= h->batch && m <= 64, EKF_ERR_INVALID_ARG, "prefetch_next: between 1 and min(cfg.batch, 64) landmarks");
    for (int32_t q = 0; q < m; ++q)
        REQUIRE(h, idx[q] >= 0 && idx[q] < h->N, EKF_ERR_INDEX, "prefetch_next: landmark index outside the state");
    h->pn_idx.assign(idx, idx + m);
    h->pn_N = h->N;
    return EKF_OK;
}
}  // extern "C"
