// Fragment of abi.hip, derived state (the prefetched base panels pf_*, the panel the last pass extracted nx_*, the announced prefetch pn_idx, the
// hint, the pending ring, the sorted signature index): ONE function per event that makes some of it stale.  No other code clears
// pf_valid, nx_valid or pn_idx; flush_pending alone SETS the first two, from what its own pass extracted.  
#pragma once
namespace {
// Pair slots must read as zero beyond the active columns (the pass kernels read whole tile-wide slices of K and G): whenever the
// map shrinks or the state is replaced, every ring is cleared -- the F64 pairs AND their float copies (cfg.pass_arith = EKF_ARITH_F32).
hipError_t clear_pairs(ekf_handle *h) {
    const size_t elems = (size_t)h->st.pair_stride * h->st.pcap * 2;       // G ring, then K ring: one allocation each
    hipError_t e = hipMemsetAsync(h->st.Gp, 0, elems * 8, h->stream);
    if (e == hipSuccess && h->st.Gp32) e = hipMemsetAsync(h->st.Gp32, 0, elems * 4, h->stream);
    return e;
}

// The exchange areas or the transport changed (other buffers, a hook, a communicator), or an exchange is about to overwrite them:
// the panel the last pass left in the send / receive area is gone.  The prefetched panels sit in pf_store and stay.
void exchange_changed(ekf_handle *h) { h->nx_valid = false; }

// The tile store changed (a pass retired; flush_pending, which runs its pass in place, sets both flags from what that pass extracted
// instead): the prefetched panels were base values of the old tiles, the extracted panel a row of them.  Also when a new prefetch
// starts: pf_idx / pf_store are about to be rewritten, and its all-gather overwrites the receive area.
void tiles_changed(ekf_handle *h) { h->pf_valid = false; exchange_changed(h); }

// The announced prefetch (ekf_prefetch_next) was consumed by the pass it waited for, or replaced by a new announcement.
void drop_announced(ekf_handle *h) { h->pn_idx.clear(); }

// The map grew: the panels are too short by one landmark, and an announced prefetch spoke of the map before it grew.  (The hint
// stays: finish_step drops it after every correction, and its use is guarded by hint < N.)
void map_grew(ekf_handle *h) { tiles_changed(h); drop_announced(h); }

// The landmarks behind the indices changed (removal renumbers them, a constraint rewrites both): whatever NAMES landmarks of the
// old state goes -- the announced prefetch and the hint.  The panels are the business of the pass or the edit that follows.
void numbering_changed(ekf_handle *h) { drop_announced(h); h->hint_idx = -1; }

// x / s were replaced or the map compacted: the panels and the sorted signature index (a caller whose map SHRANK clears the pair rings
// first, clear_pairs, in stream order).  ekf_remove_landmarks adds numbering_changed; ekf_set_x and the low-rank load keep the
// announcement and the hint, whose uses are guarded by pn_N == N and hint < N.
void map_replaced(ekf_handle *h) { tiles_changed(h); h->s_sorted_ok = false; }

// The covariance was replaced as a whole (ekf_set_P, the low-rank load, the checkpoint load; an in-flight pass is retired first):
// no pair is pending any more and the panels were rows of the old P.  ekf_set_P keeps N, s and therefore everything else.
void covariance_replaced(ekf_handle *h) { h->npend = 0; h->pstart = 0; tiles_changed(h); }
}  // namespace
