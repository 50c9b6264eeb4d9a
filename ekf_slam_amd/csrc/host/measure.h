// Fragment of abi.hip, ekf_measure: the scan-level prefetch, one function per kind of row, and the device-decided scan (cfg.device_assoc == 4).
#pragma once
namespace {
// one scan as ekf_measure received it
struct Scan { const double *obs; int64_t m; const double *u, *lm_index, *lm_loc; int64_t L; };
// winners of a row's association that a previous launch has already left on the device
struct Winners { bool have; int set; int32_t seq, nblk; };

// The next row's association rides in this row's launch: its observation, where its winners go (set_out; the launch has one
// workgroup per 256 padded columns of the n_mm_after rows it covers), and the same in `nxt` for the row that consumes them.
void ride_next(ekf_handle *h, const Scan &sc, int64_t row, int set_out, int64_t n_mm_after, DevLoopArgs &dl, Winners &nxt) {
    dl.parts_out = h->d_lparts + (int64_t)set_out * h->lparts_stride;
    dl.seq_out = next_assoc_seq(h);
    dl.z0 = sc.obs[row]; dl.z1 = sc.obs[sc.m + row]; dl.z2 = sc.obs[2 * sc.m + row];
    dl.R00 = dl.z0 * h->cfg.Rc[0]; dl.R01 = 0.0; dl.R10 = 0.0; dl.R11 = dl.z1 * h->cfg.Rc[1];   // EKF_SLAM.m:108 / EKF_SLAM_UC.m:110
    dl.s_cost = h->cfg.s_cost; dl.s_thresh = h->cfg.s_thresh; dl.w_pos = h->cfg.w_pos;
    nxt.have = true; nxt.set = set_out; nxt.seq = dl.seq_out; nxt.nblk = (int32_t)gather_workgroups(h->st, n_mm_after);
}

// EKF_SLAM.m:110-111 / EKF_SLAM_UC.m:110-111, length(x) < 4: a row that meets an empty map appends under the first non-zero landmark
// index, signature 1
int32_t measure_row_empty(ekf_handle *h, const Scan &sc, const double R[4]) {
    double loc[2];
    const int32_t rc = lookup_loc(h, sc.lm_index, sc.lm_loc, sc.L, true, 0.0, loc);
    return rc ? rc : do_append(h, sc.u, R, loc, 1.0);
}

// cfg.device_assoc == 4, the device-decided branch: the rows [first, m) of a scan, queued without a single wait.  Per row ONE launch,
// k_gather<.., kDecide>: it takes the decision the previous launch's epilogue (or, for the scan's first row, k_associate<.., kDevN>, which
// also carries out a recorded predict) left on the device, carries it out -- correction, append, or nothing for stale winners -- and
// evaluates the next row's association on the state it leaves.  Its record comes back through the ring of ekf_handle::h_lrec and is
// settled later (verify_loop).  The caller has checked that capacity and the landmark list hold for every row (per-scan fallbacks).
int32_t measure_decided_rows(ekf_handle *h, const Scan &sc, int64_t first, int tab_set, int64_t kbase) {
    const double *obs = sc.obs, *u = sc.u;
    const int64_t m = sc.m;
    Winners nxt = { false, 0, 0, 0 };
    for (int64_t ii = first; ii < m; ++ii) {
        const double z[3] = { obs[ii], obs[m + ii], obs[2 * m + ii] };
        const double R[4] = { z[0] * h->cfg.Rc[0], 0.0, 0.0, z[1] * h->cfg.Rc[1] };   // EKF_SLAM_UC.m:110
        if (!nxt.have) {                                               // EKF_SLAM_UC.m:119 for the scan's first row, a launch of its own
            nxt.set = h->loop_set ^ 1; nxt.seq = next_assoc_seq(h);
            AssocArgs a = {};
            a.z0 = z[0]; a.z1 = z[1]; a.z2 = z[2];
            colmajor2(R, a.R00, a.R01, a.R10, a.R11);
            a.s_cost = h->cfg.s_cost; a.s_thresh = h->cfg.s_thresh; a.w_pos = h->cfg.w_pos;
            a.N = n_hi(h); a.cur = h->cur; a.npend = h->npend; a.pstart = h->pstart; a.own_only = 0;
            a.dN = unsettled(h) > 0 ? h->d_nring + h->nrow % ekf_handle::kNRing : nullptr;
            nxt.nblk = assoc_blocks(a.N);
            TIMED(h, EKF_KERNEL_ASSOCIATE, launch_associate_devn(h->st, a, h->d_lparts + (int64_t)nxt.set * h->lparts_stride, nxt.seq, h->storage,
                  h->stream, h->have_pp ? &h->pp : nullptr));
            if (h->have_pp) { h->have_pp = false; h->cur ^= 1; }      // the launch wrote the predicted state to the other buffer
            h->loop_set = nxt.set;
        }
        if (h->lrec_head - h->lrec_tail >= (uint64_t)ekf_handle::kLoopRing) TRY(verify_loop(h, /*block*/ true));
        TRY(refresh_work(h));
        const int64_t nh = n_hi(h);                                    // before this row
        DevLoopArgs dl = {};
        dl.parts_in = h->d_lparts + (int64_t)nxt.set * h->lparts_stride; dl.nblk_in = nxt.nblk; dl.seq_in = nxt.seq;
        dl.rec = h->h_lrec_dev + h->lrec_head % ekf_handle::kLoopRing;
        dl.seq_rec = next_assoc_seq(h);
        dl.n_known = unsettled(h) > 0 ? -1 : h->N;
        dl.dn_in = h->d_nring + h->nrow % ekf_handle::kNRing;
        dl.dn_out = h->d_nring + (h->nrow + 1) % ekf_handle::kNRing;
        dl.loc = h->h_loctab_dev + (int64_t)tab_set * ekf_handle::kTabCap * 3;
        dl.abort = h->d_abort; dl.scan_id = h->scan_id;
        dl.loc_base = kbase;
        dl.u0 = u[0]; dl.u1 = u[1];
        const int set_in = nxt.set;
        nxt.have = false;
        if (ii + 1 < m) ride_next(h, sc, ii + 1, set_in ^ 1, 2 * (nh + 1), dl, nxt);
        CorrectArgs a;
        fill_correct_args(h, a, z, R, 0);
        a.n_mm = 2 * (nh + 1);                                         // the bound after this row: sizes the grid only
        if (h->inflight) h->appended_inflight = true;                  // (the row may append beside the pass)
        TIMED(h, EKF_KERNEL_GATHER, launch_gather_decided(h->st, a, dl, h->storage, h->stream));
        if (nxt.have) h->loop_set = nxt.set;
        h->lspec.push_back({ dl.seq_rec, 0, -1 });
        ++h->lrec_head;
        ++h->nrow;
        TRY(finish_step(h));                                           // every row takes a pair slot: npend stays exact
    }
    return EKF_OK;
}

// cfg.device_assoc == 4: the per-scan checks that keep the error semantics of the waited path exact, then the decided rows.  *waited:
// the scan (from row *first on) must take the waited path instead (N is exact then).
int32_t measure_decided(ekf_handle *h, const Scan &sc, bool *waited, int64_t *first) {
    const double *obs = sc.obs, *lm_index = sc.lm_index, *lm_loc = sc.lm_loc;
    const int64_t m = sc.m, L = sc.L;
    *waited = false; *first = 0;
    TRY(verify_loop(h, /*block*/ false));                      // what earlier scans' launches have reported by now
    if (h->N == 0 && unsettled(h) > 0) TRY(settle(h));      // the empty-map rule needs an exact N
    if (h->N == 0) {
        const double R[4] = { obs[0] * h->cfg.Rc[0], 0.0, 0.0, obs[m] * h->cfg.Rc[1] };
        TRY(measure_row_empty(h, sc, R));
        *first = 1;
        if (m == 1) return EKF_OK;
    }
    const int64_t mr = m - *first;
    if (n_hi(h) + mr > h->cap) {                                       // capacity: a row could append beyond it
        TRY(settle(h));
        if (h->N + mr > h->cap) { *waited = true; return EKF_OK; }
    }
    if (n_hi(h) + mr - h->N > ekf_handle::kTabCap) {
        TRY(settle(h));
        if (mr > ekf_handle::kTabCap) { *waited = true; return EKF_OK; }
    }
    const int set = h->tab_next;
    if (h->tab_used[set] && h->lrec_tail <= h->tab_until[set]) {
        TRY(settle(h));
        if (h->lrec_tail <= h->tab_until[set]) HIPCHK(h, hipStreamSynchronize(h->stream));   // no later launch: wait for the scan's kernels
    }
    h->tab_used[set] = false;
    double *tab = h->h_loctab + (int64_t)set * ekf_handle::kTabCap * 3;
    // every key a row could append under: N + 1 .. n_hi + the scan's rows (lookup_loc's rule, EKF_SLAM_UC.m:122).  A key that does
    // not resolve is an error only for a row that appends under it: the rows are queued all the same -- such a row applies nothing and
    // stops the scan on the device -- and the scan is settled before ekf_measure returns, which then reports that row's error as the
    // waited loop does (one wait per scan instead of one per row).
    bool all_keys = resolve_keys(lm_index, lm_loc, L, h->N, n_hi(h) + mr - h->N, tab);
    if (!all_keys && unsettled(h) > 0) {
        TRY(settle(h));
        all_keys = resolve_keys(lm_index, lm_loc, L, h->N, mr, tab);
    }
    const int64_t kbase = h->N;
    h->tab_next = (set + 1) % ekf_handle::kTabSets;
    h->scan_id = h->scan_id == INT32_MAX ? 1 : h->scan_id + 1;
    h->lookup_fail_hits = -1;
    const int32_t rc = measure_decided_rows(h, sc, *first, set, kbase);
    h->tab_used[set] = true;
    h->tab_until[set] = h->lrec_head;
    if (rc || all_keys) return rc;
    TRY(settle(h));
    if (h->lookup_fail_hits >= 0) {
        const int64_t q = h->lookup_fail_hits - kbase;
        h->lookup_fail_hits = -1;
        return lookup_failed(h, (int64_t)tab[3 * q + 2]);
    }
    return EKF_OK;
}

// The scan's corrections are known before the loop runs: a shard that batches fetches their base row-panels in ONE exchange (rows
// that turn out to append drop the prefetch again; the per-row exchange then takes over).  Not for the device loop, which names its
// landmarks on the device.
int32_t measure_prefetch(ekf_handle *h, const Scan &sc, bool dev_loop) {
    const int64_t m = sc.m;
    if (!(h->sharded && (h->comm || h->xhook) && h->batch > 1 && m > 1 && h->N > 0 && !dev_loop)) return EKF_OK;
    std::vector<int64_t> want;
    for (int64_t ii = 0; ii < m && (int64_t)want.size() < h->batch; ++ii) {
        int64_t idx = -1;
        if (h->cfg.mode == EKF_MODE_KNOWN) { if (!(sc.obs[2 * m + ii] > (double)h->N) && ii < h->N) idx = ii; }
        else if (h->cfg.w_pos == 0.0) { int32_t nw = 0; associate_signature_only(h, sc.obs[2 * m + ii], &nw, &idx); if (nw) idx = -1; }
        if (idx >= 0 && std::find(want.begin(), want.end(), idx) == want.end()) want.push_back(idx);
    }
    if (want.size() <= 1) return EKF_OK;
    int32_t rc = prefetch_begin(h, want.data(), (int32_t)want.size());     // reads tiles only: a lazy predict stays lazy
    if (!rc) rc = run_exchange(h);
    return rc ? rc : prefetch_finish(h);
}

// known correspondence: row ii is landmark ii, or a new landmark under the key z(3)
int32_t measure_row_known(ekf_handle *h, const Scan &sc, int64_t ii, const double z[3], const double R[4]) {
    if (z[2] > (double)h->N) {                                         // EKF_SLAM.m:118-120
        double loc[2];
        const int32_t rc = lookup_loc(h, sc.lm_index, sc.lm_loc, sc.L, false, z[2], loc);
        return rc ? rc : do_append(h, sc.u, R, loc, z[2]);
    }
    // a shard that rewrites P per correction lets this row's pass extract the next row's panel (ekf_hint_next)
    if (h->sharded && h->batch == 1 && ii + 1 < sc.m && !(sc.obs[2 * sc.m + ii + 1] > (double)h->N) && ii + 1 < h->N) h->hint_idx = ii + 1;
    return do_correct(h, z, R, ii);                                    // :123  idx = ii
}

// cfg.device_assoc == 3 (the default of EKF_MODE_UC): the device-resident loop.  Per observation the host queues
//   [k_associate, only if the previous launch did not already evaluate this observation's association]  ->
//   k_gather (takes the landmark from the device's decision; its epilogue evaluates the NEXT observation's association)
//   or k_append (checks the device found nothing below the threshold)  ->  the pass over P when a batch is complete
// with no wait anywhere: which of the two it queues is the host mirror's prediction (exact when w_pos == 0: the reference's
// live likelihood is a function of z(3) and s alone, Correspondence.m:71,75), what the device decided comes back in records
// that are checked later (verify_loop).  With w_pos != 0 the host cannot predict the branch: the waited path below.
// On a shard the same loop runs on every rank (the association reads replicated data only, so every rank's device names the same
// landmark); a correction is k_rowpanel<kDev> (the panel of the landmark the device names) -> all-gather -> k_gather<sharded, kDev>.
int32_t measure_row_devloop(ekf_handle *h, const Scan &sc, int64_t ii, const double z[3], const double R[4], Winners &nxt) {
    int32_t is_new = 0, rc = EKF_OK;
    int64_t idx = 0;
    associate_signature_only(h, z[2], &is_new, &idx);              // the prediction that shapes the queue
    DevLoopArgs dl = {};
    if (!nxt.have) {                                               // EKF_SLAM_UC.m:119, as a launch of its own
        nxt.set = h->loop_set ^ 1; nxt.seq = next_assoc_seq(h); nxt.nblk = assoc_blocks(h->N);
        rc = launch_assoc(h, z, R, h->d_lparts + (int64_t)nxt.set * h->lparts_stride, nxt.seq, false, false,
                          /*fold_predict*/ !is_new);       // an append materialises the predict anyway
        if (rc) return rc;
        h->loop_set = nxt.set;
    }
    dl.parts_in = h->d_lparts + (int64_t)nxt.set * h->lparts_stride; dl.nblk_in = nxt.nblk; dl.seq_in = nxt.seq;
    if (h->lrec_head - h->lrec_tail >= (uint64_t)ekf_handle::kLoopRing) TRY(verify_loop(h, /*block*/ true));
    dl.rec = h->h_lrec_dev + h->lrec_head % ekf_handle::kLoopRing;
    dl.seq_rec = next_assoc_seq(h);
    const int set_in = nxt.set;
    nxt.have = false;
    if (is_new) {                                                  // EKF_SLAM_UC.m:121-123
        double loc[2];
        TRY(lookup_loc(h, sc.lm_index, sc.lm_loc, sc.L, false, (double)(idx + 1), loc));
        rc = do_append(h, sc.u, R, loc, (double)(idx + 1), &dl);
    } else {
        if (ii + 1 < sc.m) ride_next(h, sc, ii + 1, set_in ^ 1, n_mm(h), dl, nxt);
        rc = do_correct_dev(h, z, R, idx, dl);
        if (!rc && nxt.have) h->loop_set = nxt.set;
    }
    if (rc) return rc;
    h->lspec.push_back({ dl.seq_rec, is_new, idx });
    ++h->lrec_head;
    return EKF_OK;
}

// the waited path (cfg.device_assoc 0 / 1, or w_pos != 0) and the speculated one (cfg.device_assoc == 2)
int32_t measure_row_waited(ekf_handle *h, const Scan &sc, const double z[3], const double R[4]) {
    int32_t is_new = 0, rc = EKF_OK;
    int64_t idx = 0;
    if (h->cfg.w_pos == 0.0 && h->cfg.device_assoc != 1) {
        // The reference's decision is a pure function of z(3) and s: the Mahalanobis position cost it also
        // evaluates is discarded (Correspondence.m:74-75).  With w_pos == 0 measure() therefore decides from
        // the host mirror of s -- same arithmetic as k_associate, no launch, no device->host sync.
        // ekf_associate() always runs the full device computation.
        associate_signature_only(h, z[2], &is_new, &idx);
        if (h->cfg.device_assoc == 2) {
            // ... and with device_assoc == 2 the device evaluates the association all the same (per-landmark phi_k,
            // Mahalanobis and signature cost, arg-min), queued behind the previous row's kernels; the host does not wait
            // for it but checks every decision against its own before measure() returns
            if ((int)h->spec.size() == ekf_handle::kSpecRing) TRY(verify_speculated(h));
            const int32_t seq = next_assoc_seq(h);
            TRY(launch_assoc(h, z, R, h->h_parts_dev + (int64_t)(h->spec.size() % ekf_handle::kSpecRing) * h->parts_stride, seq));
            h->spec.push_back({ seq, is_new, assoc_blocks(h->N), idx, h->N });
        }
    } else {
        TRY(do_associate(h, z, R, &is_new, &idx, nullptr, nullptr));   // EKF_SLAM_UC.m:119
    }
    if (!is_new) return do_correct(h, z, R, idx);
    double loc[2];                                                 // EKF_SLAM_UC.m:121-123
    rc = lookup_loc(h, sc.lm_index, sc.lm_loc, sc.L, false, (double)(idx + 1), loc);
    return rc ? rc : do_append(h, sc.u, R, loc, (double)(idx + 1));
}

// ekf_create, the device-decided branch's part: the ring of landmark counts, the landmark-list sets the append branch reads
int32_t create_decided(ekf_handle *h) {
    if (!decided_mode(h)) return EKF_OK;
    HIPCHK(h, dalloc(h, &h->d_nring, ekf_handle::kNRing));
    HIPCHK(h, dalloc(h, &h->d_abort, 1));
    const size_t bytes = 3 * sizeof(double) * ekf_handle::kTabSets * ekf_handle::kTabCap;
    HIPCHK(h, halloc(h, &h->h_loctab, bytes, hipHostMallocMapped));
    memset(h->h_loctab, 0, bytes);
    void *dp = nullptr;
    HIPCHK(h, hipHostGetDevicePointer(&dp, h->h_loctab, 0));
    h->h_loctab_dev = (double *)dp;
    return EKF_OK;
}
}  // namespace

extern "C" {
int32_t ekf_measure(ekf_handle *h, const double *obs, int64_t m, const double u[2], const double *lm_index,
                    const double *lm_loc, int64_t L) {
    if (!h || !u || m < 0 || L < 0 || (m > 0 && !obs) || (L > 0 && (!lm_index || !lm_loc)))
        return fail(h, EKF_ERR_INVALID_ARG, "measure: bad argument");
    TRY(use_device(h));
    // The loop below decides row by row whether to append or correct, and a correction on a shard needs an exchange in the
    // middle of it: only the library-owned communicator can run that.  A host that runs the all-gather itself (transport (b)
    // / (c) of ekfslam.h) drives append / correct_begin / its exchange / correct_finish per row -- refused here, up front,
    // before any row has changed the state.
    REQUIRE(h, !(h->sharded && h->comm == nullptr && h->xhook == nullptr && m > 0), EKF_ERR_STATE,
            "measure: a sharded handle needs the library-owned communicator (ekf_comm_init) or an exchange hook "
            "(ekf_exchange_set_hook); with a host-run exchange call ekf_append / ekf_correct_begin / ekf_correct_finish per observation");
    const bool dev_loop = h->cfg.mode == EKF_MODE_UC && h->cfg.device_assoc == 3 && h->cfg.w_pos == 0.0;
    const Scan sc = { obs, m, u, lm_index, lm_loc, L };
    int64_t first = 0;
    if (decided_mode(h) && m > 0) {
        // cfg.device_assoc == 4: the device-decided branch, any w_pos -- unless a per-scan check sends the scan down the waited path
        bool waited = false;
        const int32_t rc = measure_decided(h, sc, &waited, &first);
        if (rc || !waited) return rc;
    }
    TRY(measure_prefetch(h, sc, dev_loop));
    if (dev_loop) TRY(verify_loop(h, /*block*/ false));                    // what earlier scans' launches have reported by now
    Winners nxt = { false, 0, 0, 0 };
    for (int64_t ii = first; ii < m; ++ii) {                               // EKF_SLAM.m:107
        const double z[3] = { obs[ii], obs[m + ii], obs[2 * m + ii] };
        const double R[4] = { z[0] * h->cfg.Rc[0], 0.0, 0.0, z[1] * h->cfg.Rc[1] };   // :108
        const int32_t rc = h->N == 0 ? measure_row_empty(h, sc, R)
           : h->cfg.mode == EKF_MODE_KNOWN ? measure_row_known(h, sc, ii, z, R)
           : dev_loop ? measure_row_devloop(h, sc, ii, z, R, nxt) : measure_row_waited(h, sc, z, R);
        if (rc) { verify_speculated(h); return rc; }                       // (what the device has decided so far is still checked)
    }
    return verify_speculated(h);
}
}  // extern "C"
