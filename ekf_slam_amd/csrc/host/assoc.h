// Fragment of abi.hip, association: the device loops' records and their verification, the waited / speculated / mirror decisions, the lookups.
#pragma once
namespace {
// one snapshot of a self-validating 16-byte entry (kernels.h: AssocHostPartial): payload, and the launch number its tag stands
// for GIVEN that payload
struct PartView { double ll; int32_t index; int32_t seq; };
inline PartView read_part(const volatile AssocHostPartial *e) {
    const volatile uint64_t *w = reinterpret_cast<const volatile uint64_t *>(e);
    const uint64_t lo = w[0], hi = w[1];
    PartView v;
    memcpy(&v.ll, &lo, 8);
    v.index = (int32_t)(uint32_t)(hi & 0xffffffffu);
    v.seq = (int32_t)((uint32_t)(hi >> 32) - assoc_part_mix((uint32_t)(lo & 0xffffffffu), (uint32_t)(lo >> 32), (uint32_t)v.index));
    return v;
}

// Device-resident measure loop: compare what the device decided (records in mapped memory) with what the host predicted when it
// queued the launches.  block == false: only the records that have landed; block == true: all of them (the stream is synchronised
// if the newest has not landed within the polling bound).
int32_t verify_loop(ekf_handle *h, bool block) {
    if (h->lrec_tail == h->lrec_head) return EKF_OK;
    if (block) {
        const volatile AssocHostPartial *newest = h->h_lrec + (h->lrec_head - 1) % ekf_handle::kLoopRing;
        const int32_t want = h->lspec.back().seq;
        bool landed = false;
        for (int spin = 0; spin < 200000 && !landed; ++spin) { landed = read_part(newest).seq == want; if (!landed) __builtin_ia32_pause(); }
        if (!landed) HIPCHK(h, hipStreamSynchronize(h->stream));
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
    }
    size_t done = 0;
    int32_t rc = EKF_OK;
    for (; h->lrec_tail < h->lrec_head; ++h->lrec_tail, ++done) {
        const ekf_handle::LoopSpec &sp = h->lspec[done];
        const PartView v = read_part(h->h_lrec + h->lrec_tail % ekf_handle::kLoopRing);
        if (v.seq != sp.seq) {
            if (!block) break;                                          // not there yet (records land in stream order)
            rc = fail(h, EKF_ERR_STATE, "measure: a decision record of the device-resident loop is missing");
            continue;
        }
        if (decided_mode(h)) {
            // cfg.device_assoc == 4: the record is the decision the device took AND carried out
            if (v.index == -1) note_append(h, (double)(h->N + 1));     // EKF_SLAM_UC.m:122: append(.., idx) with idx = N + 1
            else if (v.index == -4) h->lookup_fail_hits = h->N;          // (the row's key is N + 1; measure_decided reports it)
            else if (v.index == -2)
                rc = fail(h, EKF_ERR_STATE, "measure: the device-decided loop found stale winner entries; nothing was applied for that "
                          "observation and the state is no longer the reference's");
            continue;
        }
        const bool same = sp.is_new ? v.index == -1 : (int64_t)v.index == sp.idx;
        if (!same) {
            char buf[200];
            snprintf(buf, sizeof buf, "measure: the device association decided %s %d where the host mirror of the signatures "
                     "predicted %s %lld; the state is no longer the reference's", v.index == -1 ? "new landmark" : v.index == -2 ?
                     "(stale winner entries)" : "landmark", (int)v.index, sp.is_new ? "new landmark" : "landmark", (long long)sp.idx);
            rc = fail(h, EKF_ERR_STATE, buf);
        }
    }
    h->lspec.erase(h->lspec.begin(), h->lspec.begin() + (ptrdiff_t)done);
    return rc;
}

// cfg.device_assoc == 4: every row queued so far settled (N exact), for the entry points that read N or the state
int32_t settle(ekf_handle *h) {
    return unsettled(h) > 0 ? verify_loop(h, /*block*/ true) : EKF_OK;
}

// queue k_associate for observation z on the handle's stream; the decision goes to the device copy and, if host_slot != nullptr,
// to that mapped host slot (sequence number `seq` written last)
inline int32_t next_assoc_seq(ekf_handle *h) { return ++h->assoc_seq == 0 ? ++h->assoc_seq : h->assoc_seq; }   // never 0: a slot's initial value

// wait (bounded poll, then stream synchronisation) until the mapped slot carries sequence number seq
bool wait_mapped_seq(volatile AssocDecision *slot, int32_t seq) {
    for (int spin = 0; spin < 2000000; ++spin) {
        if (slot->seq == seq) { __atomic_thread_fence(__ATOMIC_ACQUIRE); return true; }
        __builtin_ia32_pause();
    }
    return false;
}

inline int32_t assoc_blocks(int64_t N) { return (int32_t)((N + kAssocBlock - 1) / kAssocBlock); }

// all nblk workgroups of launch `seq` have stored their winner (self-validating entries: kernels.h)
bool wait_parts(volatile AssocHostPartial *set, int32_t nblk, int32_t seq) {
    int32_t b = 0;
    for (int spin = 0; spin < 2000000; ++spin) {
        while (b < nblk && read_part(set + b).seq == seq) ++b;
        if (b == nblk) { __atomic_thread_fence(__ATOMIC_ACQUIRE); return true; }
        __builtin_ia32_pause();
    }
    return false;
}

// Correspondence.m:78-85 over the workgroups' winners: lowest likelihood, lowest index on ties (the order of the kernel's own
// reductions); nothing below the threshold anywhere -> new landmark, index N (0-based)
int32_t reduce_parts(ekf_handle *h, volatile AssocHostPartial *set, int32_t nblk, int32_t seq, int64_t N, int32_t *is_new, int64_t *idx) {
    double best = INFINITY;
    int64_t at = -1;
    for (int32_t b = 0; b < nblk; ++b) {
        const PartView v = read_part(set + b);
        REQUIRE(h, v.seq == seq, EKF_ERR_STATE, "associate: a workgroup's result is missing from the mapped buffer");
        const double ll = v.ll;
        const int64_t ix = v.index;
        if (ix >= 0 && (at < 0 || ll < best || (ll == best && ix < at))) { best = ll; at = ix; }
    }
    *is_new = at < 0 ? 1 : 0;
    *idx = at < 0 ? N : at;
    return EKF_OK;
}

// the decision of launch `seq` (nblk workgroups, entries in `set`): poll, or synchronise the stream, then reduce
int32_t collect_decision(ekf_handle *h, AssocHostPartial *set, int32_t nblk, int32_t seq, int64_t N, bool may_poll, int32_t *is_new,
                         int64_t *idx) {
    if (!(may_poll && h->assoc_poll && wait_parts(set, nblk, seq))) {
        HIPCHK(h, hipStreamSynchronize(h->stream));            // the kernel has retired: its stores to mapped memory are complete
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
    }
    return reduce_parts(h, set, nblk, seq, N, is_new, idx);
}

// exchange == false: the decision of this launch is final (unsharded, or sharded with the signature-only likelihood, which every
// shard evaluates identically from replicated data); exchange == true (sharded): this shard nominates among the landmarks whose
// diagonal block it holds and leaves its candidate -- and, want_costs, their position costs -- in the send area
// fold_predict (device-resident measure loop): a recorded predict(u) is carried out BY the association launch (it is k_predict and
// k_associate in one), so the scan's first row costs no k_predict launch and its correction folds nothing
int32_t launch_assoc(ekf_handle *h, const double z[3], const double R[4], AssocHostPartial *host_set_dev, int32_t seq,
                     bool exchange = false, bool want_costs = false, bool fold_predict = false) {
    REQUIRE(h, h->N >= 1, EKF_ERR_STATE, "associate: the state holds no landmark (Correspondence.m:29)");
    if (!fold_predict) {
        const int32_t rcp = materialize_predict(h);
        if (rcp) return rcp;
    }
    AssocArgs a;
    a.z0 = z[0]; a.z1 = z[1]; a.z2 = z[2];
    colmajor2(R, a.R00, a.R01, a.R10, a.R11);
    a.s_cost = h->cfg.s_cost; a.s_thresh = h->cfg.s_thresh; a.w_pos = h->cfg.w_pos;
    a.N = h->N; a.cur = h->cur; a.npend = h->npend; a.pstart = h->pstart;
    a.own_only = exchange ? 1 : 0;
    TimedLaunch tl(h, EKF_KERNEL_ASSOCIATE);
    HIPCHK(h, launch_associate(h->st, a, exchange ? (want_costs ? h->send + 4 : nullptr) : h->d_pos_cost, h->d_sig_cost,
                               h->d_partial, h->d_ticket, h->d_decision, exchange ? nullptr : host_set_dev, seq,
                               exchange ? h->send : nullptr, h->storage, h->stream, (fold_predict && h->have_pp) ? &h->pp : nullptr));
    if (fold_predict && h->have_pp) { h->have_pp = false; h->cur ^= 1; }       // the launch wrote the predicted state to the other buffer
    return EKF_OK;
}

// sharded association, first half: candidates (+ position costs) into the send area; the exchange moves x_count doubles
int32_t assoc_begin(ekf_handle *h, const double z[3], const double R[4], bool want_costs) {
    REQUIRE(h, !h->pending, EKF_ERR_STATE, "associate_begin: an exchange is already pending");
    TRY(launch_assoc(h, z, R, nullptr, 0, /*exchange*/ true, want_costs));
    h->pending = true; h->pending_kind = 3; h->x_count = 4 + (want_costs ? h->N : 0);
    exchange_changed(h);       // (the candidates' all-gather overwrites the receive area)
    h->assoc_costs = want_costs;
    return EKF_OK;
}

// second half: every shard takes the same arg-min over the gathered candidates; then as do_associate
int32_t assoc_finish(ekf_handle *h, int32_t *is_new, int64_t *idx, double *pos_cost, double *sig_cost) {
    REQUIRE(h, h->pending && h->pending_kind == 3, EKF_ERR_STATE, "associate_finish: no association pending");
    REQUIRE(h, !pos_cost || h->assoc_costs, EKF_ERR_STATE, "associate_finish: position costs were not requested at begin");
    h->pending = false; h->pending_kind = 0;
    const int32_t seq = next_assoc_seq(h);
    HIPCHK(h, launch_assoc_merge(h->st, h->recv, h->cfg.world, h->x_count, h->N, h->assoc_costs, h->d_pos_cost, h->d_decision,
                                 h->h_decision_dev, seq, h->stream));
    if (pos_cost) HIPCHK(h, hipMemcpyAsync(pos_cost, h->d_pos_cost, (size_t)h->N * 8, hipMemcpyDeviceToHost, h->stream));
    if (sig_cost) HIPCHK(h, hipMemcpyAsync(sig_cost, h->d_sig_cost, (size_t)h->N * 8, hipMemcpyDeviceToHost, h->stream));
    const bool have = h->h_decision_dev && !pos_cost && !sig_cost && wait_mapped_seq(h->h_decision, seq);
    if (!have) {
        HIPCHK(h, hipMemcpyAsync(h->h_decision, h->d_decision, sizeof(AssocDecision), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    *is_new = h->h_decision->is_new;
    *idx = h->h_decision->index;
    return EKF_OK;
}

// cfg.device_assoc == 2: every decision the device has produced since the last call must equal the host mirror's
int32_t verify_speculated(ekf_handle *h) {
    if (h->spec.empty()) return EKF_OK;
    const size_t n = h->spec.size();
    // wait for the NEWEST launch only: once its workgroups have reported, the launches queued before it on the same stream have
    // retired and their stores (posted in order) have landed
    {
        const ekf_handle::Spec &sp = h->spec[n - 1];
        AssocHostPartial *set = h->h_parts + (int64_t)((n - 1) % ekf_handle::kSpecRing) * h->parts_stride;
        if (!(h->assoc_poll && wait_parts(set, sp.nblk, sp.seq))) {
            HIPCHK(h, hipStreamSynchronize(h->stream));
            __atomic_thread_fence(__ATOMIC_ACQUIRE);
        }
    }
    int32_t rc = EKF_OK;
    for (size_t q = 0; q < n && !rc; ++q) {
        const ekf_handle::Spec &sp = h->spec[q];
        int32_t is_new = 0; int64_t idx = 0;
        rc = reduce_parts(h, h->h_parts + (int64_t)(q % ekf_handle::kSpecRing) * h->parts_stride, sp.nblk, sp.seq, sp.idx_N, &is_new, &idx);
        if (!rc && (is_new != sp.is_new || idx != sp.idx))
            rc = fail(h, EKF_ERR_STATE, "measure: the device association disagrees with the host mirror of the signatures");
    }
    h->spec.clear();
    return rc;
}

int32_t do_associate(ekf_handle *h, const double z[3], const double R[4], int32_t *is_new, int64_t *idx,
                     double *pos_cost, double *sig_cost) {
    // Sharded handles need NO exchange here (they did until round 3): the position cost needs each landmark's own 2x2 block,
    // and those blocks are replicated, live, on every shard (DevState::diag) -- every shard evaluates every landmark and takes the same
    // decision from the same bits.  (ekf_associate_begin / _finish remain for hosts that were written around the exchange.)
    const int32_t seq = next_assoc_seq(h);
    const int64_t N = h->N;
    AssocHostPartial *set = h->h_parts + (int64_t)ekf_handle::kSpecRing * h->parts_stride;
    TRY(launch_assoc(h, z, R, h->h_parts_dev + (int64_t)ekf_handle::kSpecRing * h->parts_stride, seq));
    if (pos_cost) HIPCHK(h, hipMemcpyAsync(pos_cost, h->d_pos_cost, (size_t)N * 8, hipMemcpyDeviceToHost, h->stream));
    if (sig_cost) HIPCHK(h, hipMemcpyAsync(sig_cost, h->d_sig_cost, (size_t)N * 8, hipMemcpyDeviceToHost, h->stream));
    // measure()'s path: every workgroup stores its winner into mapped host memory (one 16-byte store: payload + sequence number)
    // and the host takes the arg-min as soon as all of them carry this launch's number -- ~2 us after the kernel's last store,
    // against ~15 us for a device->host copy + stream synchronisation.  Bounded: after ~2 ms the stream is synchronised instead.
    // With cost vectors asked for the copies above need the synchronisation anyway.
    return collect_decision(h, set, assoc_blocks(N), seq, N, !pos_cost && !sig_cost, is_new, idx);
}

// Correspondence.m:40-43,71,75,78-85 with the live likelihood (signature cost only): the landmark of lowest likelihood among those
// at or below the threshold, the lowest index on ties (strict '<' in index order, :81); nothing below the threshold -> (new, N).
void associate_signature_only(const ekf_handle *h, double z3, int32_t *is_new, int64_t *idx) {
    const int64_t N = h->N;
    *is_new = 1; *idx = N;
    double best = INFINITY;
    const double inv_cost = 1.0 / h->cfg.s_cost, thresh = h->cfg.s_thresh;
    // ll = (d c) d <= thresh only if |d| <= sqrt(thresh / c) (up to rounding: the window below is a strict superset); on a
    // large map only the landmarks inside that window of the sorted index are evaluated -- with the very same expression
    const double w = (inv_cost > 0.0 && thresh >= 0.0) ? sqrt(thresh / inv_cost) * (1.0 + 1e-9) + 1e-300 : INFINITY;
    if (N >= 256 && w < INFINITY && z3 == z3) {
        if (!h->s_sorted_ok || (int64_t)(h->s_sorted.size() + h->s_tail.size()) > N) {
            h->s_sorted.clear();
            h->s_tail.clear();
            h->s_sorted.reserve((size_t)N);
            for (int64_t k = 0; k < N; ++k) if (h->s_host[(size_t)k] == h->s_host[(size_t)k]) h->s_sorted.emplace_back(h->s_host[(size_t)k], k);
            std::sort(h->s_sorted.begin(), h->s_sorted.end());
            h->s_sorted_ok = true;
        } else if (h->s_tail.size() >= ekf_handle::kSortedTail) {
            const size_t mid = h->s_sorted.size();
            std::sort(h->s_tail.begin(), h->s_tail.end());
            h->s_sorted.insert(h->s_sorted.end(), h->s_tail.begin(), h->s_tail.end());
            std::inplace_merge(h->s_sorted.begin(), h->s_sorted.begin() + (ptrdiff_t)mid, h->s_sorted.end());
            h->s_tail.clear();
        }
        const auto lo = std::lower_bound(h->s_sorted.begin(), h->s_sorted.end(), std::pair<double, int64_t>(z3 - w, -1));
        const auto hi = std::upper_bound(lo, h->s_sorted.end(), std::pair<double, int64_t>(z3 + w, INT64_MAX));
        if (hi - lo < N / 2) {
            auto consider = [&](double sk, int64_t k) {
                const double d = z3 - sk;
                const double ll = d * inv_cost * d;
                if (ll <= thresh && (ll < best || (ll == best && k < *idx))) { *is_new = 0; best = ll; *idx = k; }
            };
            for (auto it = lo; it != hi; ++it) consider(it->first, it->second);
            for (const auto &e : h->s_tail) consider(e.first, e.second);     // landmarks appended since the last merge
            return;
        }
    }
    for (int64_t k = 0; k < N; ++k) {
        const double d = z3 - h->s_host[(size_t)k];
        const double ll = d * inv_cost * d;
        if (ll <= thresh && ll < best) { *is_new = 0; best = ll; *idx = k; }
    }
}

int32_t lookup_failed(ekf_handle *h, int64_t hits) {
    char buf[160];
    snprintf(buf, sizeof buf, "measure: landmark lookup matched %lld entries (the reference's append() call is "
             "only well-formed for exactly one)", (long long)hits);
    return fail(h, EKF_ERR_LOOKUP, buf);
}

// landmark(find([landmark.index] == key)).loc  (key < 0: find([landmark.index]), i.e. all non-zero indices)
int32_t lookup_loc(ekf_handle *h, const double *lm_index, const double *lm_loc, int64_t L, bool any_nonzero, double key,
                   double loc[2]) {
    int64_t hits = 0, at = -1;
    for (int64_t i = 0; i < L; ++i) {
        const bool m = any_nonzero ? (lm_index[i] != 0.0) : (lm_index[i] == key);
        if (m) { ++hits; at = i; }
    }
    if (hits != 1) return lookup_failed(h, hits);
    loc[0] = lm_loc[at];
    loc[1] = lm_loc[L + at];
    return EKF_OK;
}

// lookup_loc's rule for the E keys kbase+1 .. kbase+E at once (one pass over the list): out[3q .. 3q+2] = loc of key kbase+1+q and
// the number of entries that carry it (the append branch applies an append only when that is 1); false if any key is not matched
// exactly once
bool resolve_keys(const double *lm_index, const double *lm_loc, int64_t L, int64_t kbase, int64_t E, double *out) {
    for (int64_t q = 0; q < E; ++q) { out[3 * q] = 0.0; out[3 * q + 1] = 0.0; out[3 * q + 2] = 0.0; }
    for (int64_t i = 0; i < L; ++i) {
        const double v = lm_index[i];
        if (!(v >= (double)(kbase + 1) && v <= (double)(kbase + E))) continue;
        const int64_t q = (int64_t)v - kbase - 1;
        if ((double)(kbase + 1 + q) != v) continue;                     // not an integer key
        if ((out[3 * q + 2] += 1.0) == 1.0) { out[3 * q] = lm_loc[i]; out[3 * q + 1] = lm_loc[L + i]; }
    }
    bool all = true;
    for (int64_t q = 0; q < E; ++q) all = all && out[3 * q + 2] == 1.0;
    return all;
}

// a mapped area of `count` self-validating entries that read as launch 0 (sequence numbers start at 1), and its device-side address
int32_t mapped_parts(ekf_handle *h, AssocHostPartial **host, AssocHostPartial **dev, size_t count) {
    HIPCHK(h, halloc(h, host, sizeof(AssocHostPartial) * count, hipHostMallocMapped));
    memset(*host, 0, sizeof(AssocHostPartial) * count);
    for (size_t e = 0; e < count; ++e) (*host)[e].tag = (int32_t)assoc_part_mix(0, 0, 0);
    void *dp = nullptr;
    HIPCHK(h, hipHostGetDevicePointer(&dp, *host, 0));
    *dev = (AssocHostPartial *)dp;
    return EKF_OK;
}

// ekf_create, the association's part: k_associate's outputs on the device, the mapped decision and winners, the device loop's ring
int32_t create_assoc(ekf_handle *h) {
    HIPCHK(h, dalloc(h, &h->d_partial, (size_t)((h->cap + kAssocBlock - 1) / kAssocBlock)));
    HIPCHK(h, dalloc(h, &h->d_decision, 1));
    HIPCHK(h, dalloc(h, &h->d_ticket, 1));
    HIPCHK(h, dalloc(h, &h->d_pos_cost, (size_t)h->cap));
    HIPCHK(h, dalloc(h, &h->d_sig_cost, (size_t)h->cap));
    HIPCHK(h, halloc(h, &h->h_decision, sizeof(AssocDecision), hipHostMallocMapped));
    memset(h->h_decision, 0, sizeof(AssocDecision));
    static const bool poll = ekf_tune_int("EKF_ASSOC_POLL", 1) != 0;
    h->assoc_poll = poll;
    void *dp = nullptr;
    if (poll && hipHostGetDevicePointer(&dp, h->h_decision, 0) == hipSuccess) h->h_decision_dev = (AssocDecision *)dp;
    // k_associate's per-workgroup winners (see ekf_handle::h_parts): kSpecRing sets for cfg.device_assoc == 2, one more for
    // the calls that wait; 16 bytes per workgroup at capacity
    h->parts_stride = assoc_blocks(h->cap > 0 ? h->cap : 1);
    TRY(mapped_parts(h, &h->h_parts, &h->h_parts_dev, (size_t)h->parts_stride * (ekf_handle::kSpecRing + 1)));
    // device-resident measure loop: two sets of per-workgroup winners (a k_associate launch has ceil(N / 256) workgroups, a
    // k_gather launch one per 256 padded columns) and the ring of decision records
    h->lparts_stride = std::max<int64_t>(assoc_blocks(h->cap), gather_workgroups(h->st, 2 * h->cap));
    HIPCHK(h, dalloc(h, &h->d_lparts, (size_t)(2 * h->lparts_stride)));
    return mapped_parts(h, &h->h_lrec, &h->h_lrec_dev, ekf_handle::kLoopRing);
}
}  // namespace

extern "C" {
int32_t ekf_associate_begin(ekf_handle *h, const double z[3], const double R[4], int32_t want_costs) {
    if (!h || !z || !R) return fail(h, EKF_ERR_INVALID_ARG, "associate_begin: null argument");
    REQUIRE(h, h->sharded, EKF_ERR_STATE, "associate_begin: handle is not sharded (use ekf_associate)");
    int32_t rc = use_device(h);
    return rc ? rc : assoc_begin(h, z, R, want_costs != 0);
}

int32_t ekf_associate_finish(ekf_handle *h, int32_t *is_new, int64_t *idx, double *pos_cost, double *sig_cost) {
    if (!h || !is_new || !idx) return fail(h, EKF_ERR_INVALID_ARG, "associate_finish: null argument");
    int32_t rc = use_device(h);
    return rc ? rc : assoc_finish(h, is_new, idx, pos_cost, sig_cost);
}
}  // extern "C"
