// Fragment of abi.hip, the handle: ekf_handle (fields grouped by family), error reporting, the registries ekf_destroy releases, small helpers.
#pragma once
#include "../../../include/ekfslam.h"
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../device_math.h"
#include "../flush32_pipe.h"
#include "../kernels.h"
#include "../layout.h"

struct KernelTimer {
    bool enabled = false;
    std::vector<hipEvent_t> ev;   // start/stop pairs
    size_t used = 0;              // events used since the last read
};

struct ekf_handle {
    // ---- the state and what every family reads ----
    ekf_config cfg;
    int64_t N = 0;         // landmarks in the state (host mirror; appends are host-initiated)
    int64_t cap = 0;
    int32_t T = 64;
    int32_t storage = 0;
    int32_t cur = 0;       // which of the double buffers holds the live x / Prr / strip
    DevState st;
    hipStream_t own_stream = nullptr, stream = nullptr;
    double *h_small = nullptr;   // pinned 32 doubles
    double *d_digest = nullptr;
    // ---- steps: the recorded predict, the host mirror of the signatures, the run-ahead throttle ----
    // lazy predict: ekf_predict only records u; the next correction folds it into its gather kernel (one launch
    // instead of two, identical arithmetic); any other consumer of x / P launches k_predict first
    bool have_pp = false;
    PredictArgs pp;
    std::vector<double> s_host;   // host mirror of the signatures (they only change through host calls)
    // (signature, landmark) sorted by signature: the signature-only decision of a large map looks at the few landmarks whose
    // signature lies within the threshold of z(3) instead of all N (the mirror's O(N) scan per observation would pace the host
    // at ~10 us per row from 10 k landmarks on).  Rebuilt lazily after bulk changes, kept up to date by appends.
    // Appends go to an unsorted TAIL that every query scans linearly and that is merged into the sorted part once it holds
    // kSortedTail entries (an insertion into the sorted vector moved ~0.8 MB per append at 50 k landmarks, on the host's
    // critical path of a streaming-append step).
    mutable std::vector<std::pair<double, int64_t>> s_sorted, s_tail;
    mutable bool s_sorted_ok = false;
    static constexpr size_t kSortedTail = 2048;
    // run-ahead throttle: the host may queue at most ~2*kThrottle update-steps ahead of the device.  Measured: the
    // first time ~150-190 launches are outstanding on a stream, one launch call blocks for 35-45 ms (the runtime
    // grows a per-queue pool); with the run-ahead bounded below that the stall never happens.
    hipEvent_t throttle_ev[2] = { nullptr, nullptr };
    bool throttle_set[2] = { false, false };
    int throttle_k = 0, since_mark = 0;
    // ---- passes over P: the pending pairs, the two tile stores, the asynchronous pass ----
    int32_t batch = 1;     // corrections per pass over P
    int32_t npend = 0;     // pending pairs a reader must apply (tiles hold P_base; live P = P_base - sum of pending K_i G_i)
    int32_t pstart = 0;    // ring slot of the oldest pending pair
    // Asynchronous flush (cfg.batch > 1, f64/f32 alike): the pass over P runs on a second stream from the current
    // tile store into the OTHER one while the next corrections keep reading the current store plus all pending
    // pairs (those being flushed, `nfrozen`, and the ones recorded since).  At the next batch boundary the stores
    // swap.  Readers of P, appends and state loads first retire the in-flight flush.
    bool async_flush = false;
    void *tilebuf[2] = { nullptr, nullptr };
    int32_t base = 0;          // tilebuf[base] == st.tiles: the store kernels read
    int32_t nfrozen = 0;       // pending pairs that belong to the in-flight flush (the oldest ones)
    bool inflight = false;
    int64_t inflight_N = 0;      // landmarks when the in-flight pass was launched (it writes rows < 2 * inflight_N) ...
    bool appended_inflight = false;   // ... and whether landmarks were appended since (their rows are copied to the new store when it retires)
    const int64_t *inflight_dn = nullptr;      // the ring slot holding the count at the in-flight pass's ev_pairs (nullptr: inflight_N is exact)
    int flush_cus = 0;           // a CU-masked pass stream: the CUs that stream may use (0: the whole device)
    hipStream_t flush_stream = nullptr;
    hipEvent_t ev_pairs = nullptr, ev_flushed = nullptr, ev_rows = nullptr;
    // cfg.pass_arith = EKF_ARITH_F32: the strip form of the pass (flush32_pipe.h) -- the dump area, the split planes (the work list
    // fields are filled from the pass's WorkSet at each launch)
    PassAux aux = { nullptr, 0, nullptr, 0, 0, nullptr, nullptr };
    int grid_cap = 0;
    char dd_kernel[64] = "";       // kernel instance of the last downdate / flush launch (ekf_downdate_kernel_name)
    int32_t dd_pairs = 0;          // pairs it applied
    // ---- work lists ----
    // Work lists of the owned lower-triangle tiles of the active tile rows, in two sets.  The pass kernels fetch their entries for their
    // whole lifetime, so refresh_work never rewrites the set an in-flight pass (cfg.async_flush) holds: it builds the other one.
    struct WorkSet {
        int2 *work = nullptr;          // the tiles, row by row
        int64_t nwork = 0;
        int64_t nwork_head = 0;        // ... of them in front of the LAST tile row's (which are the trailing entries)
        // the same tiles arranged as 8 per-XCD streams of super-tiles (batched flush: keeps each XCD's K/G working set
        // inside its own 4 MiB L2); stream x is xcd[x * xcd_len .. ), padded with (-1,-1)
        int2 *xcd = nullptr;
        int64_t xcd_len = 0;
        int4 *segs = nullptr;          // cfg.pass_arith != EKF_ARITH_F64: the strip form's work list (PassAux::segs, nsegs, cols)
        int64_t nsegs = 0, cols = 0;
        int64_t rows = -1;             // tile rows it was built for (-1: none)
    };
    WorkSet ws[2];
    int32_t ws_cur = 0;                // the newest set: what the next pass, digest or low-rank load reads
    int32_t ws_pass = -1;              // the set the in-flight pass holds (-1: no pass in flight)
    bool ws_unordered = false;         // ws[ws_cur] was uploaded after the last ev_pairs: a pass that only waits for ev_pairs must wait for ev_wl too
    int64_t work_cap = 0, segs_cap = 0;
    // pinned staging of the work lists (refresh_work): uploads are queued on the stream with no host wait -- a stream
    // synchronisation here drains a queue that may hold a whole batch and its pass (configs[4]: a 2.4 ms bubble per new tile row)
    char *wl_stage = nullptr;
    size_t wl_stage_bytes = 0;
    hipEvent_t ev_wl = nullptr;
    bool wl_busy = false;
    // ---- association ----
    AssocDecision *d_partial = nullptr, *d_decision = nullptr, *h_decision = nullptr;
    AssocDecision *h_decision_dev = nullptr;   // device-side address of the mapped h_decision (k_assoc_merge, the sharded path, writes it)
    int *d_ticket = nullptr;                   // k_associate's last-workgroup ticket (device-side consumers only)
    double *d_pos_cost = nullptr, *d_sig_cost = nullptr;
    int32_t assoc_seq = 0;
    // k_associate's workgroups store their winners into MAPPED host memory and the host takes the arg-min: kSpecRing + 1 sets of
    // parts_stride entries (one per workgroup at capacity).  Sets 0..kSpecRing-1 form the ring of cfg.device_assoc == 2 (measure()
    // dispatches on the host mirror's decision while k_associate runs for every observation in the stream; the device's decisions
    // are VERIFIED against the host's before measure() returns); set kSpecRing serves the calls that wait for their decision.
    static constexpr int kSpecRing = 64;
    AssocHostPartial *h_parts = nullptr, *h_parts_dev = nullptr;
    int64_t parts_stride = 0;
    bool assoc_poll = true;                    // false (tuning builds, EKF_ASSOC_POLL=0): wait by stream synchronisation instead of polling the mapped entries
    struct Spec { int32_t seq, is_new, nblk; int64_t idx, idx_N; };   // idx_N: landmarks at launch (the default index of a new one)
    std::vector<Spec> spec;
    // ---- the measure loops on the device ----
    // Device-resident measure loop (cfg.device_assoc == 3, the default of EKF_MODE_UC): an observation's association decision is
    // produced AND consumed on the device (kernels.h: DevLoopArgs); the host queues the launches from its mirror's prediction of
    // the control flow (append or correct: a function of z(3) and s alone when w_pos == 0) and reads what the device decided
    // afterwards, from a ring of records in mapped memory -- verified lazily (the next ekf_measure sweeps what has landed;
    // every call that synchronises or reads state checks the rest first).
    static constexpr int kLoopRing = 256;
    AssocHostPartial *d_lparts = nullptr;      // DEVICE: 2 sets of lparts_stride per-workgroup winners
    int64_t lparts_stride = 0;
    int32_t loop_set = 0;                      // set written last
    AssocHostPartial *h_lrec = nullptr, *h_lrec_dev = nullptr;     // MAPPED: kLoopRing decision records
    struct LoopSpec { int32_t seq, is_new; int64_t idx; };   // (cfg.device_assoc == 4: nothing predicted, the record IS the decision)
    std::vector<LoopSpec> lspec;               // predictions of records lrec_tail .. lrec_head-1 (ring positions mod kLoopRing)
    uint64_t lrec_head = 0, lrec_tail = 0;
    // The device-decided branch (cfg.device_assoc == 4): the device also takes the branch of every row, so the host no longer knows N
    // until the records of the rows it queued have landed ("settled").  N above is the settled count, N + the unsettled rows an upper
    // bound (n_hi) that sizes grids and work lists.  The count itself lives on the device, in a ring with one slot per launch.
    static constexpr int kNRing = 1024;
    int64_t *d_nring = nullptr;                // DEVICE: kNRing landmark counts
    uint64_t nrow = 0;                         // decided launches so far: slot nrow % kNRing holds the count the next one starts from
    // Landmark-list entries of every key a queued row could append under (EKF_SLAM_UC.m:122; x, y and how many entries carry the key),
    // one set per scan, in MAPPED memory the append branch reads; a set is reused once a record of a launch queued after its scan has
    // landed (that scan's kernels are done).
    static constexpr int kTabSets = 64, kTabCap = 512;
    double *h_loctab = nullptr, *h_loctab_dev = nullptr;
    int32_t *d_abort = nullptr;                // DEVICE: the scan whose rows stopped at a failed lookup (DevLoopArgs::abort)
    int32_t scan_id = 0;
    int64_t lookup_fail_hits = -1;             // settled: a row's append matched this many list entries (-1: none failed)
    uint64_t tab_until[kTabSets] = {};
    bool tab_used[kTabSets] = {};
    int tab_next = 0;
    // ---- exchange / sharding ----
    // sharded correction: exchange slabs (own allocations, or caller-provided device buffers)
    bool sharded = false;          // world > 1, or cfg.force_sharded (the sharded code path with one rank, on one GPU)
    double *own_send = nullptr, *own_recv = nullptr, *send = nullptr, *recv = nullptr;
    int64_t slab_cap = 0;          // doubles per shard slab at capacity
    int64_t xchg_cap = 0;          // doubles of the send area (the receive area holds world times as many)
    int64_t slab = 0;              // doubles per shard slab of the pending correction
    bool pending = false;          // an exchange is between begin and finish ...
    bool assoc_costs = false;      // the pending association's exchange carries the position costs too
    int pending_kind = 0;          // ... 1: one correction's row-panel, 2: a prefetch of several base row-panels, 3: association candidates
    int64_t x_count = 0;           // doubles per shard of the pending exchange
    CorrectArgs pending_args;
    void *comm = nullptr;          // ncclComm_t
    int32_t (*xhook)(void *) = nullptr;   // ekf_exchange_set_hook: the caller's all-gather, called where the library-owned one would run
    void *xhook_ctx = nullptr;
    hipEvent_t ev_xchg = nullptr;    // ekf_exchange_local: this shard's copies of one exchange are done
    // prefetched BASE row-panels (ekf_prefetch_rows): valid until the tiles change (flush) or the map grows
    bool pf_valid = false;
    int32_t pf_m = 0;
    int64_t pf_slab = 0, pf_N = 0;
    std::vector<int64_t> pf_idx;
    double *pf_store = nullptr;    // world x batch x slab_cap
    // the row-panel of landmark nx_idx, extracted by the last pass over P itself (ekf_hint_next + k_downdate_w<.., kNext>): valid while
    // the tiles, the map size and the send area stay as that pass left them and nothing is pending
    int64_t hint_idx = -1;         // ekf_hint_next: the landmark the NEXT ekf_correct will name
    bool nx_valid = false;
    int64_t nx_idx = -1, nx_N = 0;
    // ekf_prefetch_next: the landmarks of the batch AFTER the current one.  When the current batch completes, their row-panels are
    // extracted as the pass will leave them (k_rowpanel_next) in front of the pass, and the all-gather runs on xchg_stream beside it.
    std::vector<int64_t> pn_idx;
    int64_t pn_N = -1;
    hipStream_t xchg_stream = nullptr;
    hipEvent_t ev_pn_ready = nullptr, ev_pn_done = nullptr;
    // ---- map edits ----
    double *d_csmall = nullptr;  // 16 doubles: the small operands of a landmark-landmark constraint (k_constrain_probe)
    // ekf_remove_landmarks: the map new landmark -> old landmark (ldm / 2 entries, built in pinned memory, uploaded in stream order; the
    // staging area is reused only after the event behind the previous upload has passed) and the scratch the signatures are compacted into.
    // Allocated at the first removal -- like the second tile store of a handle without cfg.async_flush (tilebuf[1]), which is kept.
    int32_t *h_cmap = nullptr, *d_cmap = nullptr;
    double *d_s_tmp = nullptr;
    hipEvent_t ev_cmap = nullptr;
    bool cmap_busy = false;
    // ekf_extract_map, on the DESTINATION handle: the list destination landmark -> source landmark (cap entries, allocated at the first
    // extraction into this handle and kept; every extraction ends with a stream synchronisation, so the list is never busy)
    int32_t *d_xidx = nullptr;
    // ekf_nearest_landmarks: the N (d2, partner) entries k_nearest writes and the pinned area they are read back through (cap entries
    // each, allocated at the first search and kept; every search ends with a stream synchronisation, so the area is never busy)
    NearestEntry *d_nearest = nullptr, *h_nearest = nullptr;
    // ekf_merge_landmarks_batch: its private pair ring (EKF_MERGE_BATCH_MAX F64 slots: G ring, then K ring), one record per constraint on
    // the device and in pinned memory, the snapshot of x / strip / Prr / the diagonal blocks it restores when a pair is irregular
    // (allocated at the first batch call and kept); ekf_observe_model_joint puts its pairs into the same ring (host/joint_update.h)
    double *d_mring = nullptr, *d_mrec = nullptr, *h_mrec = nullptr, *d_msnap = nullptr;
    // ekf_factor_map: the factor store (F64 lower-triangle tiles of edge factor_tile_edge() for f_rows rows), and in ONE second allocation
    // the right-hand sides, the result block with the pivots behind it and the reference states; the pinned images of the last two.
    // Allocated at the first call for the N of that call, grown (freed and allocated anew) when N has outgrown them, released by
    // ekf_destroy itself -- they are not in the registries below, which only ever grow.  f_bytes of them are counted in `bytes`.
    double *d_ftiles = nullptr, *d_fsmall = nullptr, *h_fres = nullptr, *h_fref = nullptr;
    int64_t f_rows = -1, f_bytes = 0;
    // ekf_sample_map, part of the same scratch (released with it): in ONE device allocation a chunk of draws, a chunk of samples and the
    // partial blocks of one apply pass, for fs_rows rows; kSampleSlots chunks of pinned staging per direction, and the event behind each
    // slot's readback (made once, destroyed with the handle's other events).  fs_bytes of the device part are counted in `bytes`.
    double *d_fsample = nullptr, *h_fxi = nullptr, *h_fy = nullptr;
    hipEvent_t ev_fslot[4] = { nullptr, nullptr, nullptr, nullptr };
    int64_t fs_rows = -1, fs_bytes = 0;
    // ekf_solve_map, part of the same scratch (released with it): the inverses of the factor's diagonal tiles, for fv_rows rows; the
    // chunks and the pinned slots are ekf_sample_map's.  fv_bytes are counted in `bytes`.
    double *d_fsolve = nullptr;
    int64_t fv_rows = -1, fv_bytes = 0;
    // ekf_multiply_map (host/multiply_map.h), a scratch of its own (the factor store is NOT part of it): in ONE device allocation a chunk of
    // vectors, a chunk of products and the partial blocks of one tile pass, for pm_rows rows; kSampleSlots chunks of pinned staging per
    // direction and the event behind each slot's readback.  Allocated at the first call, grown when N has outgrown it, released by
    // ekf_destroy itself.  pm_bytes of the device part are counted in `bytes`.
    double *d_pmul = nullptr, *h_pmb = nullptr, *h_pmy = nullptr;
    hipEvent_t ev_pmslot[4] = { nullptr, nullptr, nullptr, nullptr };
    int64_t pm_rows = -1, pm_bytes = 0;
    // ---- linear observations (ekf_observe_linear / ekf_linear_innovation) ----
    // two records on the device and in pinned memory (the update-step's, then the probe's; behind them in the pinned area the two counters
    // ekf_linear_rejections reads), the device counters of launches that did not apply, the event behind a waited step's readback
    double *d_linrec = nullptr, *h_linrec = nullptr;
    int64_t *d_lincnt = nullptr;
    hipEvent_t ev_linrec = nullptr;
    // ---- model observations relinearised on the device (ekf_observe_model_iterated / ekf_model_innovation_iterated) ----
    // the iteration record of the update-step, then the probe's, on the device and in pinned memory; read back behind ev_linrec
    double *d_itrec = nullptr, *h_itrec = nullptr;
    // ---- a scan matched to the map under the models' conventions (ekf_associate_model) ----
    // one record per workgroup (am_nblk_cap per observation) and the m results on the device, the results' pinned copy and the event behind
    // a call's readback; the results followed by the m x N block of d2_all on the device and in pinned memory (allocated when first asked for)
    ekfm::Match2 *d_amparts = nullptr, *d_amout = nullptr, *h_amout = nullptr;
    int64_t am_nblk_cap = 0;
    char *d_amall = nullptr, *h_amall = nullptr;
    hipEvent_t ev_amodel = nullptr;
    // ---- the scan assigned to the map one-to-one (ekf_assign_model) ----
    // one candidate list per workgroup (am_nblk_cap per observation) and the selected list per observation on the device; the result block
    // on the device and in pinned memory, and the event behind a call's readback (the Match2 records per workgroup are d_amparts above)
    ekfm::CandList *d_aslists = nullptr, *d_assel = nullptr;
    AssignResult *d_asres = nullptr, *h_asres = nullptr;
    hipEvent_t ev_assign = nullptr;
    // ---- ... and applied with no wait between the two (ekf_observe_model_assigned) ----
    // one record per step of the scan on the device (in front of d_asres, in its allocation); the pinned block of the LATEST scan -- the
    // records, then the head of the result block -- and the event behind its copy; scan_m: that scan's size (0: none yet); scan_host: the
    // block was filled by the host (an empty map: no launch, no event)
    double *d_scanrec = nullptr;
    char *h_scan = nullptr;
    hipEvent_t ev_scan = nullptr;
    int64_t scan_m = 0;
    bool scan_host = false;
    // ---- the joint compatibility of a scan's pairings (ekf_joint_innovation) ----
    // the hypotheses on the device and in pinned memory; the records, prefixes and nu of a call (joint_out_bytes) likewise, and the event behind
    // a call's readback; the stacked S of every hypothesis, 8 MiB on either side, allocated when first asked for
    int64_t *d_jhyp = nullptr, *h_jhyp = nullptr;
    char *d_jout = nullptr, *h_jout = nullptr;
    double *d_jS = nullptr, *h_jS = nullptr;
    hipEvent_t ev_joint = nullptr;
    // ---- ... searched on the device (ekf_joint_search) ----
    // the store of operands, extensions and nodes, and the block a call brings back on the device and in pinned memory (allocated at the
    // first call and kept); read back behind ev_joint
    JointSearchStore *d_jsearch = nullptr;
    JointSearchOut *d_jsout = nullptr, *h_jsout = nullptr;
    // ---- a scan's pairings applied as one joint update (ekf_observe_model_joint) ----
    // what k_joint_factor hands k_gather_joint (allocated at the first call and kept); its pairs go to d_mring above
    JointBlock *d_jblock = nullptr;
    // ... relinearised (ekf_observe_model_joint_iterated): k_joint_factor_iter's iteration record on the device and in pinned memory (allocated at
    // the first call and kept); read back behind ev_joint
    double *d_jiter = nullptr, *h_jiter = nullptr;
    // ---- a linear observation with a dense H (ekf_observe_dense; host/dense_obs.h) ----
    // the chunk of H's rows and of G = P H' are ekf_multiply_map's scratch above, its pairs go to d_mring; its own: the segments' partial
    // sums (for dn_rows landmark rows; grown when N has outgrown them, released by ekf_destroy itself, dn_bytes counted in `bytes`), what
    // k_dense_factor hands k_gather_dense, and the answer on the device and in pinned memory behind an event (allocated at the first call
    // and kept)
    double *d_dpart = nullptr;
    int64_t dn_rows = -1, dn_bytes = 0;
    DenseBlock *d_dblock = nullptr;
    DenseOut *d_dout = nullptr, *h_dout = nullptr;
    hipEvent_t ev_dense = nullptr;
    // ---- timers, what ekf_destroy releases, the error text ----
    KernelTimer timers[EKF_KERNEL_COUNT];
    std::vector<void *> allocs;       // device memory (dalloc), pinned memory (halloc) and events (new_event): what ekf_destroy releases
    std::vector<void *> pinned;
    std::vector<hipEvent_t> events;
    int64_t bytes = 0;
    std::string err;
};

namespace {
int32_t fail(ekf_handle *h, int32_t status, const char *what, hipError_t e = hipSuccess) {
    if (h) {
        h->err = what ? what : "";
        if (e != hipSuccess) { h->err += ": "; h->err += hipGetErrorString(e); }
    }
    return status;
}

#define HIPCHK(h, call)                                                      \
    do {                                                                     \
        hipError_t e_ = (call);                                              \
        if (e_ != hipSuccess) return fail((h), EKF_ERR_HIP, #call, e_);      \
    } while (0)

#define REQUIRE(h, cond, status, msg)                                        \
    do { if (!(cond)) return fail((h), (status), (msg)); } while (0)

// a step that reports its own failure: pass the status on
#define TRY(call)                                                            \
    do { const int32_t rc_ = (call); if (rc_) return rc_; } while (0)

// device memory, cleared (on the null stream), released by ekf_destroy
template <typename Tp>
hipError_t dalloc(ekf_handle *h, Tp **p, size_t count) {
    void *q = nullptr;
    const size_t bytes = (count ? count : 1) * sizeof(Tp);
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) return e;
    e = hipMemset(q, 0, bytes);
    if (e != hipSuccess) return e;
    h->allocs.push_back(q);
    h->bytes += (int64_t)bytes;
    *p = (Tp *)q;
    return hipSuccess;
}

// its siblings: pinned host memory (not cleared) and an event without timing, both released by ekf_destroy
template <typename Tp>
hipError_t halloc(ekf_handle *h, Tp **p, size_t bytes, unsigned flags) {
    const hipError_t e = hipHostMalloc((void **)p, bytes, flags);
    if (e == hipSuccess) h->pinned.push_back(*p);
    return e;
}
hipError_t new_event(ekf_handle *h, hipEvent_t *ev) {
    const hipError_t e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
    if (e == hipSuccess) h->events.push_back(*ev);
    return e;
}

// a temporary device buffer of one entry point: the pointer it guards is released on every exit of the scope
struct DevTemp {
    void **p;
    template <typename Tp> explicit DevTemp(Tp **q) : p((void **)q) {}
    ~DevTemp() { if (*p) hipFree(*p); }
};

// Pinned staging of an upload queued with no host wait: the area and the event behind its last upload are made at first use; the
// area is refilled only after that event has passed (stage_wait); every upload ends with stage_uploaded.
template <typename Tp>
int32_t stage_alloc(ekf_handle *h, Tp **area, size_t bytes, hipEvent_t *ev) {
    if (!*area) HIPCHK(h, halloc(h, area, bytes ? bytes : 16, hipHostMallocDefault));
    if (!*ev) HIPCHK(h, new_event(h, ev));
    return EKF_OK;
}
int32_t stage_wait(ekf_handle *h, hipEvent_t ev, bool &busy) { if (busy) { HIPCHK(h, hipEventSynchronize(ev)); busy = false; } return EKF_OK; }
int32_t stage_uploaded(ekf_handle *h, hipEvent_t ev, bool &busy) { HIPCHK(h, hipEventRecord(ev, h->stream)); busy = true; return EKF_OK; }

inline int64_t n_mm(const ekf_handle *h) { return 2 * h->N; }
// cfg.device_assoc == 4: rows queued whose records have not been settled yet (each may have appended one landmark), and the upper
// bound of N they leave; both exact (0, N) on every other handle
inline bool decided_mode(const ekf_handle *h) { return h->cfg.mode == EKF_MODE_UC && h->cfg.device_assoc == 4; }
inline int64_t unsettled(const ekf_handle *h) { return decided_mode(h) ? (int64_t)(h->lrec_head - h->lrec_tail) : 0; }
inline int64_t n_hi(const ekf_handle *h) { return h->N + unsettled(h); }
inline size_t elt_size(const ekf_handle *h) { return h->storage == EKF_STORE_F64 ? 8 : 4; }

int32_t use_device(ekf_handle *h) {
    HIPCHK(h, hipSetDevice(h->cfg.device));
    return EKF_OK;
}

// start / stop events around the launches of its scope, on the stream they go to (only while the kernel's timer is enabled)
struct TimedLaunch {
    hipStream_t s;
    KernelTimer *t;
    hipEvent_t stop = nullptr;
    TimedLaunch(ekf_handle *h, int which) : TimedLaunch(h, which, h->stream) {}
    TimedLaunch(ekf_handle *h, int which, hipStream_t on) : s(on), t(&h->timers[which]) {
        if (!t->enabled) { t = nullptr; return; }
        if (t->used + 2 > t->ev.size()) {
            hipEvent_t a, b;
            if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { t = nullptr; return; }
            t->ev.push_back(a); t->ev.push_back(b);
        }
        hipEventRecord(t->ev[t->used], s);
        stop = t->ev[t->used + 1];
        t->used += 2;
    }
    ~TimedLaunch() { if (t) hipEventRecord(stop, s); }
};

// one launch under its kernel's timer
#define TIMED(h, which, call) do { TimedLaunch tl_((h), (which)); HIPCHK((h), call); } while (0)

void colmajor2(const double R[4], double &r00, double &r01, double &r10, double &r11) {
    r00 = R[0]; r10 = R[1]; r01 = R[2]; r11 = R[3];
}
}  // namespace
