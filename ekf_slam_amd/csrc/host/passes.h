// Fragment of abi.hip, the passes over P: the work lists they walk, retiring the asynchronous pass, the in-place pass, the end of a batch.
#pragma once
namespace {
// (re)build the list of owned tiles for the active tile rows.  The lists are built in pinned memory and uploaded by asynchronous
// copies in stream order (the kernels that read them follow on the same stream); the staging area is reused only after the event
// behind the previous upload has passed.  The upload goes to the set no in-flight pass holds: the newest set itself when the pass
// holds the other one (or none is in flight -- the main stream is ordered after every retired pass), else the other set.
int32_t refresh_work(ekf_handle *h) {
    const int64_t nt = ekf_tiles_for(2 * n_hi(h), h->T);          // (tiles beyond the device's count only ever see zero pairs)
    if (nt == h->ws[h->ws_cur].rows) return EKF_OK;
    const int32_t to = h->ws_pass == h->ws_cur ? h->ws_cur ^ 1 : h->ws_cur;
    ekf_handle::WorkSet &ws = h->ws[to];
    const size_t b_work = (size_t)h->work_cap * sizeof(int2), b_xcd = 8 * b_work, b_segs = (size_t)h->segs_cap * sizeof(int4);
    if (!h->wl_stage) h->wl_stage_bytes = b_work + b_xcd + b_segs;
    int32_t rc = stage_alloc(h, &h->wl_stage, h->wl_stage_bytes, &h->ev_wl);
    if (!rc) rc = stage_wait(h, h->ev_wl, h->wl_busy);
    if (rc) return rc;
    int2 *w = reinterpret_cast<int2 *>(h->wl_stage);
    int2 *flat = reinterpret_cast<int2 *>(h->wl_stage + b_work);
    int4 *segs = reinterpret_cast<int4 *>(h->wl_stage + b_work + b_xcd);
    size_t nw = 0;
    REQUIRE(h, h->st.tm.slots_for_rows(nt) <= h->work_cap, EKF_ERR_STATE, "work list overflow");
    size_t nw_head = 0;
    for (int64_t I = 0; I < nt; ++I) {
        if (I == nt - 1) nw_head = nw;
        for (int64_t J = 0; J <= I; ++J)
            if (h->st.tm.mine(I, J)) w[nw++] = make_int2((int)I, (int)J);
    }
    if (nw) HIPCHK(h, hipMemcpyAsync(ws.work, w, nw * sizeof(int2), hipMemcpyHostToDevice, h->stream));
    ws.nwork = (int64_t)nw;
    ws.nwork_head = (int64_t)nw_head;
    ws.rows = nt;

    // per-XCD streams: super-tiles of S x S tiles, largest first onto the least loaded stream
    static const int S = std::max(1, ekf_tune_int("EKF_SUPERTILE", 8));
    struct Super { int64_t si, sj; std::vector<int2> tiles; };
    std::vector<Super> supers;
    const int64_t ns = (nt + S - 1) / S;
    for (int64_t si = 0; si < ns; ++si)
        for (int64_t sj = 0; sj <= si; ++sj) {
            Super sp; sp.si = si; sp.sj = sj;
            for (int64_t I = si * S; I < nt && I < (si + 1) * S; ++I)
                for (int64_t J = sj * S; J <= I && J < (sj + 1) * S; ++J)
                    if (h->st.tm.mine(I, J)) sp.tiles.push_back(make_int2((int)I, (int)J));
            if (!sp.tiles.empty()) supers.push_back(std::move(sp));
        }
    // Order of the streams.  1 (default): the super-tiles in row-major order (si, then sj), flattened tile by tile and cut into 8
    // equal contiguous runs -- an XCD walks along a band of S tile rows, so the band's K slice (S x 64 KiB at 32 pairs) stays in
    // its L2 for the whole band and only the G slice changes from one super-tile to the next; runs are equal to within one tile.
    // 0: round 1's schedule (largest super-tile first onto the least loaded stream): every super-tile fetched both slices anew
    // and the streams differed by up to a super-tile (profiles/round2_tuning.md).
    static const int order = ekf_tune_int("EKF_XCD_ORDER", 1);
    std::vector<int2> stream[8];
    if (order == 0) {
        std::stable_sort(supers.begin(), supers.end(), [](const Super &a, const Super &b) { return a.tiles.size() > b.tiles.size(); });
        for (const Super &sp : supers) {
            int best = 0;
            for (int x = 1; x < 8; ++x) if (stream[x].size() < stream[best].size()) best = x;
            stream[best].insert(stream[best].end(), sp.tiles.begin(), sp.tiles.end());
        }
    } else {
        std::vector<int2> flat_order;
        flat_order.reserve(nw);
        for (const Super &sp : supers) flat_order.insert(flat_order.end(), sp.tiles.begin(), sp.tiles.end());
        const size_t tot = flat_order.size();
        for (int x = 0; x < 8; ++x)
            stream[x].assign(flat_order.begin() + (tot * x) / 8, flat_order.begin() + (tot * (x + 1)) / 8);
    }
    size_t len = 0;
    for (int x = 0; x < 8; ++x) len = std::max(len, stream[x].size());
    REQUIRE(h, (int64_t)(8 * len) <= 8 * h->work_cap, EKF_ERR_STATE, "XCD work list overflow");
    std::fill(flat, flat + 8 * len, make_int2(-1, -1));
    for (int x = 0; x < 8; ++x) std::copy(stream[x].begin(), stream[x].end(), flat + x * len);
    if (len) HIPCHK(h, hipMemcpyAsync(ws.xcd, flat, 8 * len * sizeof(int2), hipMemcpyHostToDevice, h->stream));
    ws.xcd_len = (int64_t)len;
    if (ws.segs) {                                    // the strip work list of the same tiles
        std::vector<int4> sg;
        const int64_t nsegs = ekf_pipe32::build_strip_segments(h->st.tm, nt, sg);
        REQUIRE(h, (int64_t)sg.size() <= h->segs_cap, EKF_ERR_STATE, "strip work list overflow");
        if (!sg.empty()) {
            std::copy(sg.begin(), sg.end(), segs);
            HIPCHK(h, hipMemcpyAsync(ws.segs, segs, sg.size() * sizeof(int4), hipMemcpyHostToDevice, h->stream));
        }
        ws.nsegs = nsegs;
        ws.cols = nt * h->T;
    }
    TRY(stage_uploaded(h, h->ev_wl, h->wl_busy));
    h->ws_cur = to;
    h->ws_unordered = true;
    return EKF_OK;
}

// the strip form's arguments for a pass over the work set `ws` (nullptr: the handle has no strip form)
const PassAux *pass_aux(const ekf_handle *h, const ekf_handle::WorkSet &ws, PassAux &out) {
    if (!ws.segs) return nullptr;
    out = h->aux;
    out.segs = ws.segs; out.nsegs = ws.nsegs; out.cols = ws.cols;
    return &out;
}

// the pass that applies ALL pending pairs over the work set `ws` into the tile store `dst` (ax: storage for the strip form's arguments)
PassJob pass_job(const ekf_handle *h, const ekf_handle::WorkSet &ws, void *dst, PassAux &ax) {
    PassJob job = {};
    job.dst = dst;
    job.work = ws.work; job.nwork = ws.nwork; job.nwork_head = ws.nwork; job.work_xcd = ws.xcd; job.xcd_len = ws.xcd_len;
    job.pstart = h->pstart; job.npairs = h->npend;
    job.grid_cap = h->grid_cap; job.arith = h->cfg.pass_arith;
    job.aux = pass_aux(h, ws, ax);
    return job;
}

// ekf_create, the work lists' part: both sets at capacity (after create_passes: the strip form's lists only where it exists)
int32_t create_worklists(ekf_handle *h) {
    for (auto &ws : h->ws) {
        if (h->cfg.pass_arith != EKF_ARITH_F64) HIPCHK(h, dalloc(h, &ws.segs, (size_t)h->segs_cap));
        HIPCHK(h, dalloc(h, &ws.work, (size_t)h->work_cap));
        HIPCHK(h, dalloc(h, &ws.xcd, (size_t)h->work_cap * 8));
    }
    return EKF_OK;
}

// The in-flight asynchronous flush becomes visible: later kernels on the main stream wait for it, the stores swap,
// its pairs leave the pending list.
int32_t retire_inflight(ekf_handle *h) {
    if (!h->inflight) return EKF_OK;
    if (h->appended_inflight) {
        // Landmarks appended beside the pass (do_append) sit in the old store only: their rows go to the new one behind the pass, ON THE PASS'S
        // STREAM -- the next pass follows in that stream's order (it does not wait for the main stream beyond ev_pairs) and must find them.
        // The copy waits for the appends (main stream, all issued by now); the main stream then waits for the copy instead of the pass.
        if (!h->ev_rows) HIPCHK(h, new_event(h, &h->ev_rows));
        HIPCHK(h, hipEventRecord(h->ev_rows, h->stream));
        HIPCHK(h, hipStreamWaitEvent(h->flush_stream, h->ev_rows, 0));
        if (decided_mode(h)) {
            // cfg.device_assoc == 4: from the count at the pass's ev_pairs to the count now, both the device's unless the host knows them
            const int64_t *hi = unsettled(h) > 0 ? h->d_nring + h->nrow % ekf_handle::kNRing : nullptr;
            HIPCHK(h, launch_copy_rows_dev(h->st.tm, h->tilebuf[h->base], h->tilebuf[h->base ^ 1], 2 * h->inflight_N, 2 * n_hi(h), h->inflight_dn,
                                           hi, h->storage, h->flush_stream));
        } else
            HIPCHK(h, launch_copy_rows(h->st.tm, h->tilebuf[h->base], h->tilebuf[h->base ^ 1], 2 * h->inflight_N, 2 * h->N, h->storage, h->flush_stream));
        HIPCHK(h, hipEventRecord(h->ev_flushed, h->flush_stream));
        h->appended_inflight = false;
    }
    HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_flushed, 0));
    h->ws_pass = -1;           // (later uploads on the main stream are ordered after the pass: its work set is free)
    h->base ^= 1;
    h->st.tiles = h->tilebuf[h->base];
    h->pstart = (h->pstart + h->nfrozen) % h->st.pcap;
    h->npend -= h->nfrozen;
    h->nfrozen = 0;
    h->inflight = false;
    tiles_changed(h);          // prefetched row-panels were base values of the old store
    return EKF_OK;
}

// Every other pass over P walks its work list backwards (TileMap::reverse, read by the pass kernels only): what one pass wrote
// last the next one reads first, out of the Infinity Cache -- 4 % off the pass at 10 k landmarks (1.6 GB of tiles), 10 % at
// 5 k (400 MB).  A store that fits the cache whole is resident either way and measured 1.5 % faster walked forwards, so the
// direction only alternates above kCacheBytes.  cfg.pass_direction = 1 / 2 forces never / always.
void next_pass_direction(ekf_handle *h) {
    const int force = h->cfg.pass_direction == 1 ? 0 : h->cfg.pass_direction == 2 ? 1 : -1;
    constexpr int64_t kCacheBytes = 256ll << 20;
    const int64_t nt = ekf_tiles_for(2 * n_hi(h), h->T);
    const int64_t store = nt * (nt + 1) / 2 / std::max(1, h->cfg.world) * (int64_t)h->T * h->T * (h->storage == EKF_STORE_F64 ? 8 : 4);
    const bool alternate = force >= 0 ? force != 0 : store > kCacheBytes;
    h->st.tm.reverse = alternate ? (h->st.tm.reverse ^ 1) : 0;
}

// apply ALL pending pairs to the tiles now, in place on the main stream: ONE pass over P for npend update-steps
int32_t flush_pending(ekf_handle *h, bool batch_done = false) {
    TRY(retire_inflight(h));
    if (h->npend == 0) return EKF_OK;
    TRY(refresh_work(h));
    next_pass_direction(h);
    bool extracted = false;
    const int64_t hint = h->hint_idx;
    // ekf_prefetch_next: the next batch's row-panels, as THIS pass will leave them, are extracted now; their all-gather runs beside the pass
    bool pn = false, pn_side = false;
    if (batch_done && !h->pn_idx.empty()) {
        if (h->sharded && !h->pending && h->pn_N == h->N && (h->comm || h->xhook)) {
            const int32_t m = (int32_t)h->pn_idx.size();
            const int64_t slab = slab_for(h, n_mm(h));
            TIMED(h, EKF_KERNEL_ROWPANEL, launch_rowpanel_next(h->st, h->pn_idx.data(), m, n_mm(h), h->pstart, h->npend, h->send, slab, h->storage,
                  h->stream));
            tiles_changed(h);   // (a new prefetch starts)
            h->pf_idx = h->pn_idx; h->pf_m = m; h->pf_slab = slab; h->pf_N = h->N;
            h->x_count = (int64_t)m * slab;
            // Where the all-gather runs.  On the handle's stream, in front of the pass: what ships.  On a stream of its own BESIDE the
            // pass (tuning builds, EKF_PN_SIDE_STREAM=1): built, bit-identical, and on one GPU twice as slow per update-step -- with a
            // second stream in use every dispatch of the main stream costs ~50 us more on this runtime (the same finding as
            // cfg.async_flush, profiles/round2_tuning.md 21-22; round4_tuning.md 49).  To be measured again where the all-gather
            // crosses xGMI and is long enough to be worth hiding.
            static const int pn_side_stream = ekf_tune_int("EKF_PN_SIDE_STREAM", 0);
            if (h->comm) {
                pn_side = pn_side_stream != 0;
                if (pn_side && !h->xchg_stream) {
                    HIPCHK(h, hipStreamCreateWithFlags(&h->xchg_stream, hipStreamNonBlocking));
                    HIPCHK(h, new_event(h, &h->ev_pn_ready));
                    HIPCHK(h, new_event(h, &h->ev_pn_done));
                }
                if (pn_side) {
                    HIPCHK(h, hipEventRecord(h->ev_pn_ready, h->stream));
                    HIPCHK(h, hipStreamWaitEvent(h->xchg_stream, h->ev_pn_ready, 0));
                }
                const hipStream_t xs = pn_side ? h->xchg_stream : h->stream;
                const int r = g_rccl.AllGather(h->send, h->recv, (size_t)h->x_count, /*ncclDouble*/ 8, h->comm, xs);
                if (r != 0) return fail(h, EKF_ERR_COMM, g_rccl.GetErrorString(r));
                HIPCHK(h, store_panels(h, xs));
                if (pn_side) HIPCHK(h, hipEventRecord(h->ev_pn_done, h->xchg_stream));
            } else {
                // transport (d): the caller's all-gather runs on the host's schedule, i.e. in front of the pass
                TRY(exchange_bracket(h, 2));
                HIPCHK(h, store_panels(h, h->stream));
            }
            pn = true;
        }
        drop_announced(h);
    }
    {
        // a sharded handle that was told which landmark the next correction names lets this pass extract that row-panel
        NextRow nx = { -1, nullptr };
        if (h->sharded && h->npend == 1 && !h->pending && hint >= 0 && hint < h->N) {
            nx.j = 2 * hint;
            nx.send = corr_send(h, slab_for(h, n_mm(h)));
        }
        TimedLaunch tl(h, EKF_KERNEL_DOWNDATE);
        const ekf_handle::WorkSet &ws = h->ws[h->ws_cur];     // (in place, on the main stream: ordered after its upload)
        PassAux ax;
        PassJob job = pass_job(h, ws, h->st.tiles, ax);
        job.nx = nx.j >= 0 ? &nx : nullptr;
        // In place: rows beyond the map hold no state and see zero K, so the pass leaves them out.  Read here, per launch, like the
        // work set's own row count (refresh_work) -- an append between two passes moves it.
        job.live_rows = 2 * n_hi(h);
        if (ekf_tiles_for(job.live_rows, h->T) == ws.rows) job.nwork_head = ws.nwork_head;     // (else: no tail, every tile is dispatched whole)
        HIPCHK(h, launch_downdate(h->st, job, h->storage, h->stream, h->dd_kernel, &extracted));
        h->dd_pairs = h->npend;
    }
    h->npend = 0;
    h->pstart = 0;
    h->pf_valid = pn;          // prefetched row-panels were base values of the old tiles -- unless they were extracted as this pass leaves them
    if (pn_side) HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_pn_done, 0));      // whatever follows the pass may read them (and reuse the exchange areas)
    h->nx_valid = extracted && !pn;
    if (extracted) { h->nx_idx = hint; h->nx_N = h->N; }
    return EKF_OK;
}

// a batch is complete: start its pass over P.  Synchronous engines do it in place; asynchronous ones launch it on the
// flush stream into the other tile store and keep going.
int32_t batch_complete(ekf_handle *h) {
    if (!h->async_flush) return flush_pending(h, /*batch_done*/ true);
    // Recorded BEFORE the main stream is made to wait for the previous pass (retire_inflight): every pair of this batch has been
    // written and every reader of the store this pass overwrites is queued in front of it -- that is all the new pass depends on
    // (the previous pass precedes it in the flush stream's own order).  Recording it after that wait would chain the passes
    // through two cross-stream hand-overs per batch (previous pass -> main stream -> this pass): ~30 us per update-step at batch 1.
    HIPCHK(h, hipEventRecord(h->ev_pairs, h->stream));
    h->ws_unordered = false;                      // every work-list upload so far precedes ev_pairs
    TRY(retire_inflight(h));              // at most one flush in flight; later main-stream kernels read its output
    TRY(refresh_work(h));
    HIPCHK(h, hipStreamWaitEvent(h->flush_stream, h->ev_pairs, 0));
    // a work set uploaded just now (behind ev_pairs) is ordered before the pass by its own event
    if (h->ws_unordered) HIPCHK(h, hipStreamWaitEvent(h->flush_stream, h->ev_wl, 0));
    {
        TimedLaunch tl(h, EKF_KERNEL_DOWNDATE, h->flush_stream);
        next_pass_direction(h);
        const ekf_handle::WorkSet &ws = h->ws[h->ws_cur];
        PassAux ax;
        HIPCHK(h, launch_downdate(h->st, pass_job(h, ws, h->tilebuf[h->base ^ 1], ax), h->storage, h->flush_stream, h->dd_kernel));
        h->dd_pairs = h->npend;
    }
    HIPCHK(h, hipEventRecord(h->ev_flushed, h->flush_stream));
    h->nfrozen = h->npend;
    h->inflight = true;
    h->ws_pass = h->ws_cur;                       // refresh_work leaves this set alone until the pass retires
    h->inflight_N = h->N;
    h->inflight_dn = unsettled(h) > 0 ? h->d_nring + h->nrow % ekf_handle::kNRing : nullptr;
    h->appended_inflight = false;
    return EKF_OK;
}

// ekf_create, the passes' part: the tile store (two and a pass stream of their own with cfg.async_flush), the pair rings, the areas of
// the strip form.  (ldm, the tile map and work_cap are set.)
int32_t create_passes(ekf_handle *h, const hipDeviceProp_t &prop) {
    const ekf_config &cfg = h->cfg;
    const int32_t T = h->T;
    const int64_t ldm = h->st.ldm, slots = h->work_cap, nt_cap = ldm / T;
    char *tiles = nullptr;
    HIPCHK(h, dalloc(h, &tiles, (size_t)slots * T * T * elt_size(h)));
    h->st.tiles = tiles;
    h->tilebuf[0] = tiles;
    h->async_flush = cfg.async_flush != 0;      // batch 1 too: the pass of update-step i then runs beside the gather of i + 1
    if (h->async_flush) {
        char *tiles2 = nullptr;
        HIPCHK(h, dalloc(h, &tiles2, (size_t)slots * T * T * elt_size(h)));
        h->tilebuf[1] = tiles2;
        // The pass over P fills every CU (3 wavefronts x 146 VGPRs per SIMD); a gather launched meanwhile then waits for
        // workgroup slots -- measured 20 us per gather, stream priorities do not help (profiles/round1_tuning.md, sweep
        // 12).  So the flush stream is confined to a CU mask that leaves `reserve` CUs (default 32 = 4 per XCD) to the
        // gather chain.  Reserved set {32a + 8b + a}: 4 CUs on every XCD whether mask bits map to XCDs round-robin
        // (bit % 8) or in blocks of 32.  (Tuning builds: EKF_ASYNC_RESERVE_CUS=0 gives a plain lowest-priority stream.)
        // (Split arithmetic: 64 -- its pass is not bound by the matrix pipe and loses less to fewer CUs than the corrections gain from more:
        // configs[4] at 40 000 landmarks 9.6 k update-steps/s against 8.8 k with 32 and 9.0 k synchronous; F32 arithmetic: 7.3 k with 32, 6.6 k
        // with 64; counts that are not a multiple of 32 leave the persistent pass kernels two workgroups on some CU: round4_tuning.md 59.)
        int reserve = ekf_tune_int("EKF_ASYNC_RESERVE_CUS", cfg.pass_arith == EKF_ARITH_SPLIT3 ? 64 : 32);
        const int ncu = prop.multiProcessorCount;
        if (reserve > 0 && ncu == 256) {
            if (reserve > 128) reserve = 128;
            uint32_t mask[8];
            for (int w = 0; w < 8; ++w) mask[w] = 0xffffffffu;
            int taken = 0;
            for (int b = 0; b < 16 && taken < reserve; ++b)           // b < 4: the balanced set above; then its shifts
                for (int a = 0; a < 8 && taken < reserve; ++a) {
                    const int bit = 32 * a + 8 * (b & 3) + ((a + (b >> 2)) & 7);
                    if (mask[bit >> 5] & (1u << (bit & 31))) { mask[bit >> 5] &= ~(1u << (bit & 31)); ++taken; }
                }
            HIPCHK(h, hipExtStreamCreateWithCUMask(&h->flush_stream, 8, mask));
            h->flush_cus = ncu - taken;                                // what a persistent pass kernel on that stream can occupy
        } else {
            int lo = 0, hi = 0;
            HIPCHK(h, hipDeviceGetStreamPriorityRange(&lo, &hi));
            HIPCHK(h, hipStreamCreateWithPriority(&h->flush_stream, hipStreamNonBlocking, lo));
        }
        HIPCHK(h, new_event(h, &h->ev_pairs));
        HIPCHK(h, new_event(h, &h->ev_flushed));
    }
    h->batch = cfg.batch < 1 ? 1 : cfg.batch;
    h->cfg.batch = h->batch;
    h->st.pair_stride = 2 * ldm;
    h->st.pcap = h->async_flush ? 2 * h->batch : h->batch;      // in-flight batch + the batch being recorded
    // ONE allocation, G pairs then K pairs: k_gather addresses both from one uniform base with 32-bit lane offsets
    HIPCHK(h, dalloc(h, &h->st.Gp, (size_t)(2 * ldm) * h->st.pcap * 2));
    h->st.Kp = h->st.Gp + (size_t)(2 * ldm) * h->st.pcap;
    h->st.Gp32 = nullptr; h->st.Kp32 = nullptr;
    if (cfg.pass_arith != EKF_ARITH_F64) {
        HIPCHK(h, dalloc(h, &h->st.Gp32, (size_t)(2 * ldm) * h->st.pcap * 2));
        h->st.Kp32 = h->st.Gp32 + (size_t)(2 * ldm) * h->st.pcap;
        // the strip form of the pass: work list (every item once + one padded segment per 128-row slab and column range at most), dump
        h->aux.grid = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        if (h->flush_cus > 0) h->aux.grid = h->flush_cus;                 // cfg.async_flush: one persistent workgroup per CU of the pass stream's mask
        h->aux.grid -= h->aux.grid % 8;                                   // (block b walks XCD stream b & 7)
        if (h->aux.grid < 8) h->aux.grid = 8;
        const int64_t ranges = (2 * nt_cap + ekf_pipe32::kSeg * cfg.world - 1) / (ekf_pipe32::kSeg * cfg.world);
        h->segs_cap = 4 * slots + (2 * nt_cap * ranges + 8) * ekf_pipe32::kSeg;      // (create_worklists allocates the lists)
        float *dump = nullptr;
        HIPCHK(h, dalloc(h, &dump, (size_t)h->aux.grid * ekf_pipe32::kDumpFloats));
        h->aux.dump = dump;
        if (cfg.pass_arith == EKF_ARITH_SPLIT3) {
            // the bf16 planes of the pending pairs (flush32_split.h), cut from the float copies in front of every pass of 28-64 pairs
            HIPCHK(h, dalloc(h, &h->aux.Kb3, pass_split_plane_elems(ldm)));
            HIPCHK(h, dalloc(h, &h->aux.Gb3, pass_split_plane_elems(ldm)));
        }
    }
    h->grid_cap = ekf_tune_int("EKF_DOWNDATE_GRID", 0);
    return EKF_OK;
}
}  // namespace
