// Host-side launch interface of the gfx950 kernels: one section per family, implemented by the fragment of kernels.hip the section names.
// The state and the argument blocks the launchers take are plain data and live in kernel_args.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_math.h"
#include "assign_math.h"
#include "kernel_args.h"
#include "layout.h"

// Tuning switches.  The PRODUCT library compiles every one of them to its default constant: no environment variable changes
// which kernel a handle runs.  Only a -DEKF_TUNING build (make -C ekf_slam_amd/csrc tuning -> libekfslam_tuning.so, used by
// scripts/ab_*.sh and scripts/tune_*.py through EKF_LIB_PATH) reads them from the environment.
#ifdef EKF_TUNING
#include <stdlib.h>
inline int ekf_tune_int(const char *name, int dflt) { const char *v = getenv(name); return v ? atoi(v) : dflt; }
#else
constexpr int ekf_tune_int(const char *, int dflt) { return dflt; }
#endif

// ---- the steps: predict, append, the gather of a correction, a shard's row-panels, association (launch/steps.h) ----
hipError_t launch_predict(const DevState &st, const PredictArgs &a, int storage, hipStream_t s);

// k_predict_model (predict_model.h): a.m <= kPredictModelMax motion steps carried out in order by ONE launch; buffer a.cur -> a.cur ^ 1
hipError_t launch_predict_model(const DevState &st, const PredictModelArgs &a, hipStream_t s);

// dl != nullptr (device-resident measure loop): the kernel also reduces dl->parts_in and records the decision in dl->rec
hipError_t launch_append(const DevState &st, const AppendArgs &a, int storage, hipStream_t s, const DevLoopArgs *dl = nullptr,
                         const PredictArgs *fused_predict = nullptr);

// k_append_model (append_model.h): a.m <= kAppendModelMax landmarks appended by ONE launch at the live robot state
hipError_t launch_append_model(const DevState &st, const AppendModelArgs &a, int storage, hipStream_t s);

// k_join_state / k_join_rows (join_map.h): the M landmarks of the flushed local state `lo` (same device, read only) joined behind the N of
// `st`.  launch_join_state: x, Prr and the strip from buffer a.cur into a complete buffer a.cur ^ 1, s and the live diagonal copies of the
// new landmarks; the caller flips cur.  launch_join_rows (a.M >= 1, both stores unsharded): tile rows 2 N .. 2 (N + M) - 1, columns <= row,
// from buffer a.cur of `st` and the tiles (local_storage) and live diagonal copies of `lo`.  Neither reads what the other writes.
hipError_t launch_join_state(const DevState &st, const DevState &lo, const JoinMapArgs &a, hipStream_t s);
hipError_t launch_join_rows(const DevState &st, const DevState &lo, const JoinMapArgs &a, int storage, int local_storage, hipStream_t s);

// k_extract_state / k_extract_rows (extract_map.h): the a.m landmarks idx[0 .. m) (device list, distinct, each inside the map of `src`) of the
// flushed source state `src` (same device, read only) into `dst`, every value of which is replaced.  launch_extract_state: x, Prr, the strip
// (buffer a.dcur, whole), s and the live diagonal copies.  launch_extract_rows (a.m >= 1, both stores unsharded): tile rows
// 0 .. padded(2 m) - 1 of dst, diagonal tiles whole, zero beyond 2 m.  Neither reads what the other writes.
hipError_t launch_extract_state(const DevState &dst, const DevState &src, const ExtractMapArgs &a, const int32_t *idx, hipStream_t s);
hipError_t launch_extract_rows(const DevState &dst, const DevState &src, const ExtractMapArgs &a, const int32_t *idx, int storage, int src_storage,
                               hipStream_t s);

// k_transform_state / k_transform_tiles (transform_map.h): the whole map of the flushed state `st` moved into another frame.
// launch_transform_state: x, Prr and the strip from buffer a.cur into a complete buffer a.cur ^ 1, the live diagonal copies from st.dcur
// into st.dcur ^ 1; the caller flips both.  launch_transform_tiles (unsharded): the `ntiles` tiles of `work` -- the list of the active tile
// rows, padded(2 N) / T of them -- IN PLACE in st.tiles, from buffer a.cur / st.dcur.  Neither reads what the other writes.
hipError_t launch_transform_state(const DevState &st, const TransformMapArgs &a, hipStream_t s);
hipError_t launch_transform_tiles(const DevState &st, const TransformMapArgs &a, const int2 *work, int64_t ntiles, int storage, hipStream_t s);

// fused_predict != nullptr folds predict(u) into the correction (one launch instead of two, identical arithmetic)
// fuse_downdate: the kernel also applies its pair to the landmark block (small maps: a.n_mm <= gather_fuse_max_rows(), one
// workgroup); the pair is then NOT written to the pending ring and no downdate launch must follow
hipError_t launch_gather(const DevState &st, const CorrectArgs &a, const PredictArgs *fused_predict, int storage,
                         hipStream_t s, bool fuse_downdate);
int gather_fuse_max_rows();
// device-resident measure loop: the corrected landmark is the arg-min over dl.parts_in (a.j is the fallback that keeps a launch
// whose winners name no landmark inside the state); dl.parts_out != nullptr adds the next observation's association
hipError_t launch_gather_devloop(const DevState &st, const CorrectArgs &a, const PredictArgs *fused_predict, const DevLoopArgs &dl,
                                 int storage, hipStream_t s);
int64_t gather_workgroups(const DevState &st, int64_t n_mm);      // of a gather over n_mm rows: one winner entry each (dl.parts_out)
// cfg.device_assoc == 4: the device-decided branch (k_gather<.., kDecide>).  The winners of dl.parts_in name a landmark -> the
// correction of launch_gather_devloop; nothing below the threshold -> the append of that observation; stale winners -> nothing is
// applied.  Either way the state is left in buffer a.cur ^ 1 (diagonal blocks: dcur ^ 1), the pair slot of ring position a.npend is
// written (zeros when nothing was corrected) and the next observation's association is evaluated on the state the launch leaves.
// a.n_mm: the host's upper bound of the landmark-block size AFTER this launch (sizes the grid only).
hipError_t launch_gather_decided(const DevState &st, const CorrectArgs &a, const DevLoopArgs &dl, int storage, hipStream_t s);

// sharded correction: (1) every shard copies the chunks of the landmark row-panel P(j:j+1,:) it owns into `send`
// (slab layout: local chunk kl of T columns, interleaved pairs), (2) the slabs are all-gathered into `recv`
// (world slabs of `slab` doubles), (3) the gather/solve kernel reads the panel from `recv` instead of the tiles.
hipError_t launch_rowpanel(const DevState &st, int64_t j, int64_t n_mm, int pstart, int npend, double *send, int storage,
                           hipStream_t s);
// device-resident measure loop on a shard: the row-panel of the landmark the DEVICE's association names (dl.parts_in); j, the host
// mirror's prediction, only when the winners name nothing inside the state
hipError_t launch_rowpanel_dev(const DevState &st, int64_t j, int64_t n_mm, int pstart, int npend, double *send, int storage,
                               hipStream_t s, const DevLoopArgs &dl);
struct RowList { int32_t m; int32_t j[64]; };      // landmark-block rows (2 * landmark index) of one prefetch
// base row-panels of m <= 64 landmarks (0-based indices idx) into send + q * slab, one launch
hipError_t launch_rowpanel_base(const DevState &st, const int64_t *idx, int m, int64_t n_mm, double *send, int64_t slab,
                                int storage, hipStream_t s);
// the row-panels of m <= 64 landmarks as the tiles will hold them after the pass that applies the npend pending pairs, into send + q * slab
hipError_t launch_rowpanel_next(const DevState &st, const int64_t *idx, int m, int64_t n_mm, int pstart, int npend, double *send,
                                int64_t slab, int storage, hipStream_t s);
// recv: `world` contributions `rank_stride` doubles apart; this correction's row-panel starts `offset` doubles into
// each; patched: the pending pairs are already applied to it (k_rowpanel) -- otherwise the gather applies them
// dl != nullptr (device-resident measure loop on a shard): as launch_gather_devloop, on the exchanged row-panel
hipError_t launch_gather_sharded(const DevState &st, const CorrectArgs &a, const PredictArgs *fused_predict, const double *recv,
                                 int64_t rank_stride, int64_t offset, bool patched, int storage, hipStream_t s,
                                 const DevLoopArgs *dl = nullptr);

struct AssocDecision {        // written by the device, read back by the host
    int64_t index;            // 0-based; == N for a new landmark
    int32_t is_new;
    int32_t seq;              // launch sequence number, written LAST (the host may poll a mapped copy for it)
    double  min_ll;
};

// One workgroup's winner, as it lands in MAPPED HOST memory: 16 bytes written by ONE store instruction of one lane (payload and
// sequence number arrive together; the host reads `seq` first, then the payload).  index: 0-based, -1 = nothing passed the threshold.
struct alignas(16) AssocHostPartial {
    double  min_ll;
    int32_t index;
    int32_t tag;       // launch sequence number + assoc_part_mix(payload): see below
};
// The 16 bytes leave the GPU in one store instruction and have been observed to land whole, but that is not an architectural
// promise -- so the entry validates itself: tag = seq + mix(payload).  A reader that sees a torn entry (new tag, old payload or
// the reverse) computes a sequence number that is not the one it waits for (up to a 2^-32 coincidence) and simply polls again.
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t assoc_part_mix(uint32_t ll_lo, uint32_t ll_hi, uint32_t index) {
    uint32_t m = ll_lo * 0x9E3779B1u ^ (ll_hi + 0x7F4A7C15u) * 0x85EBCA6Bu ^ (index + 0x165667B1u) * 0xC2B2AE35u;
    m ^= m >> 15; m *= 0x2C1B3C6Du; m ^= m >> 13;
    return m;
}

constexpr int kAssocBlock = 256;       // 4 wavefronts = one per SIMD: the per-landmark solve is a dependent f64 chain (1024 measured slower: 16 wavefronts share one CU's f64 issue)

// pos_cost / sig_cost: device arrays of N or nullptr; partial: device scratch of >= ceil(N/kAssocBlock) entries; ticket: a
// device int, zero between launches (the last workgroup to finish reduces the partials and resets it: one launch, no
// finishing kernel); decision: device copy.  host_partials != nullptr (mapped host memory, one entry per workgroup): NO cross-workgroup
// step on the device at all -- every workgroup stores its winner there and the HOST takes the arg-min over the ceil(N / kAssocBlock)
// entries once each carries `seq` (the ticket + release / acquire hand-over it replaces was ~4 of the kernel's 9 us)
// fused_predict != nullptr: the launch is ALSO k_predict -- the recorded predict(u) is applied to what the kernel reads and the
// predicted pose / Prr / strip / Q are written to state buffer a.cur ^ 1 (the caller flips its buffer index afterwards)
hipError_t launch_associate(const DevState &st, const AssocArgs &a, double *pos_cost, double *sig_cost,
                            AssocDecision *partial, int *ticket, AssocDecision *decision, AssocHostPartial *host_partials, int seq,
                            double *cand, int storage, hipStream_t s, const PredictArgs *fused_predict = nullptr);
// the same with the landmark count taken from a.dN when that is not nullptr (k_associate<.., kDevN>: workgroups beyond it store
// "no winner"); the grid is sized from a.N, the host's upper bound
hipError_t launch_associate_devn(const DevState &st, const AssocArgs &a, AssocHostPartial *host_partials, int seq, int storage,
                                 hipStream_t s, const PredictArgs *fused_predict);
// cand (nullptr or 4 device doubles): this shard's candidate {likelihood, index or -1, 0, 0} for the all-gather of a sharded
// association; launch_assoc_merge takes the arg-min over the `world` gathered contributions of `count` doubles each (candidate,
// then -- want_costs -- N position costs) and writes the decision like launch_associate does
hipError_t launch_assoc_merge(const DevState &st, const double *recv, int world, int64_t count, int64_t N, bool want_costs,
                              double *pos_cost, AssocDecision *decision, AssocDecision *host_decision, int seq, hipStream_t s);

// k_assoc_model / k_assoc_model_reduce (associate_model.h): a scan of a.m <= kAssocModelMax observations scored against all N landmarks, read-only.
// partials (device): m * ceil(N / kAssocBlock) records, one per workgroup of the first launch; out (device): m records, the second launch's;
// d2_all (device): nullptr, or m x N row-major, NaN where a pair has no d2.  Two launches ordered by the stream.
hipError_t launch_assoc_model(const DevState &st, const AssocModelArgs &a, ekfm::Match2 *partials, ekfm::Match2 *out, double *d2_all,
                              hipStream_t s);

// k_assign_candidates / k_assign_select / k_assign_solve (assign_model.h): the same scan assigned one-to-one, read-only.  partials as above;
// lists (device): m * ceil(N / kAssocBlock) candidate lists, one per workgroup of the first launch; sel (device): kAssocModelMax lists, the
// second launch's; res (device): the block everything a call returns is left in.  Three launches ordered by the stream.
hipError_t launch_assign_model(const DevState &st, const AssocModelArgs &a, ekfm::Match2 *partials, ekfm::CandList *lists, ekfm::CandList *sel,
                               AssignResult *res, hipStream_t s);
// ... its first two launches alone: the lists in sel and the match records in res->match, no solve (ekf_joint_search reads sel on the device)
hipError_t launch_assign_lists(const DevState &st, const AssocModelArgs &a, ekfm::Match2 *partials, ekfm::CandList *lists, ekfm::CandList *sel,
                               AssignResult *res, hipStream_t s);

// ---- the passes over P (launch/passes.h; launch/pass_select.h decides which kernel instance runs) ----
// nx (sharded handles): ALSO extract the row-panel of landmark-block rows j, j + 1 into send (layout of launch_rowpanel) from the updated
// entries; j < 0: none
struct NextRow { int64_t j; double *send; };
// what the strip form of the F32-arithmetic pass needs besides the tiles and the pairs (flush32_pipe.h; nullptr: that form is not used)
struct PassAux {
    const int4 *segs;      // strip work list: nsegs segments of ekf_pipe32::kSeg entries (strip_entry), 8 interleaved per-XCD streams
    int64_t nsegs;         // a multiple of 8
    float *dump;           // kDumpFloats floats per workgroup of the pass's grid
    int grid;              // workgroups the dump area was sized for (one per CU)
    int64_t cols;          // rows / columns of the landmark block the active tile rows cover (a multiple of 256): what k_split_pairs cuts
    uint16_t *Kb3, *Gb3;   // cfg.pass_arith = EKF_ARITH_SPLIT3 only (nullptr otherwise): the bf16 planes of the pending pairs, cut in front
                           // of each pass (flush32_split.h: split_plane_elems(ldm) elements each)
};
size_t pass_split_plane_elems(int64_t ldm);     // uint16_t elements of PassAux::Kb3 (and of Gb3) for a landmark block of leading dimension ldm
// One pass: tiles -= sum_{i < npairs} K_i G_i (in slot order) over the owned lower-triangle tiles of a work set -- ONE pass over P for
// npairs update-steps
struct PassJob {
    void *dst;                 // tile store the result is written to (== st.tiles for an in-place flush; a second buffer for the asynchronous
                               // flush, which must not disturb kernels still reading st.tiles)
    const int2 *work;          // the work list: (I, J) of the `nwork` owned tiles (device array)
    int64_t nwork;
    const int2 *work_xcd;      // the same tiles as 8 per-XCD streams (stream x = work_xcd[x * xcd_len ..), padded with (-1, -1)), used when
    int64_t xcd_len;           // several pairs are applied so that each XCD's K/G working set stays inside its own L2
    int pstart, npairs;        // the ring window: slot of the oldest pair, pairs to apply
    int grid_cap;              // EKF_DOWNDATE_GRID of a tuning build; 0: none
    int arith;                 // cfg.pass_arith
    const PassAux *aux;        // nullptr: the handle has no strip form
    const NextRow *nx;         // nullptr: no row-panel wanted
    int64_t live_rows;         // in-place passes only: landmark-block rows that hold state (2 * the landmark count, or an upper bound of it).
                               // K is zero from there to the padded width, so the update of those rows is an identity: k_downdate,
                               // k_downdate_w and k_flush_mfma neither load nor store a work item that starts at or beyond it.  0: no bound --
                               // a pass into a second store has to carry every row across
    int64_t nwork_head;        // with live_rows: the entries of `work` in front of the last tile row's, which are its trailing ones.  Of THOSE tiles
                               // k_downdate_w is dispatched for the slabs up to the bound only (rounded up to a power of two), not for all of
                               // them.  nwork (or anything with live_rows == 0): every tile is dispatched whole
};
// kname: nullptr, or 64 bytes that receive the name of the kernel instance that was launched ("k_flush_mfma<double,128,8>");
// *extracted tells whether that instance extracted job.nx (one pair per launch, wavefront-per-row tile shapes only)
hipError_t launch_downdate(const DevState &st, const PassJob &job, int storage, hipStream_t s, char *kname, bool *extracted = nullptr);
// cfg.async_flush: rows [r0, r1) of the landmark block (every local tile of the tile rows they lie in) copied from one tile store to the other
hipError_t launch_copy_rows(const TileMap &tm, const void *src, void *dst, int64_t r0, int64_t r1, int storage, hipStream_t s);
// the same with bounds known on the device only (cfg.device_assoc == 4): rows [2 * *n_lo, 2 * *n_hi) of the range [r0, r1) the host
// can bound them by (a pointer that is nullptr leaves the host's bound as it is)
hipError_t launch_copy_rows_dev(const TileMap &tm, const void *src, void *dst, int64_t r0, int64_t r1, const int64_t *n_lo,
                                const int64_t *n_hi, int storage, hipStream_t s);

// ---- map edits: removal, a constraint and its chained form, the fused pass of a batch of merges, the candidate search, and the linear
// observation that shares the constraint's device code (launch/edits.h) ----
// Landmark removal (compact.h).  src_of (device, ldm / 2 entries): the old landmark of every landmark of the new map, strictly
// increasing, -1 from the new count on.  launch_compact_tiles writes the `ntiles` destination tiles work[0 ..) = (I, J) of the
// store `dst` from the store `src` (never the same store): element (r', c') = old element (src(r'), src(c')), zero beyond the new map.
hipError_t launch_compact_tiles(const TileMap &tm, const void *src, void *dst, const int2 *work, int64_t ntiles, const int32_t *src_of,
                                int storage, hipStream_t s);
// ... and x, the strip and the live diagonal blocks from buffer cur / st.dcur into the other one (Prr and the pose copied), the
// signatures into s_out (N_old doubles): N_old = landmarks before the removal
hipError_t launch_compact_state(const DevState &st, int cur, const int32_t *src_of, int64_t N_old, double *s_out, hipStream_t s);
// out (device, 14 doubles): both landmarks' own 2x2 blocks (live F64 copies), their cross block (tiles), their entries of x -- what the
// host forms S and nu from before anything changes
hipError_t launch_constrain_probe(const DevState &st, int cur, int64_t ai, int64_t aj, double *out, int storage, hipStream_t s);
// k_gather_constrain: the constraint's pair into the ring slot, x / Prr / strip into buffer a.cur ^ 1, every landmark's live diagonal
// block (with the pair applied) into buffer dcur ^ 1; the caller flips both and lets a pass apply the pair to the tiles.  The ring is
// empty when it runs (a.npend == 0) and no record is written: the host has formed S from launch_constrain_probe's operands before.
hipError_t launch_gather_constrain(const DevState &st, const ConstrainArgs &a, int storage, hipStream_t s);
// A batch of merges (ekf_merge_landmarks_batch).  `st` is a by-value copy of the handle's DevState whose Gp / Kp / pcap name the batch's
// PRIVATE F64 pair ring (Gp32 == nullptr); world == 1.
// launch_gather_constrain_chain: the SAME kernel as constraint number a.npend of the batch while the a.npend earlier pairs (slots
// a.pstart ..) are still pending -- every tile operand is read patched with them -- and a record of it into rec (device,
// kConstrainRecordDoubles doubles: S row-major, nu, d2 as ekfm::constrain_d2 gives it, 1.0 / 0.0 = S regular or not); an irregular S
// leaves a zero pair and copies the state.
hipError_t launch_gather_constrain_chain(const DevState &st, const ConstrainArgs &a, double *rec, int storage, hipStream_t s);
// launch_merge_pass (merge_pass.h): the `ntiles` destination tiles work[0 ..) of the store `dst` (never st.tiles) = the compaction of
// launch_compact_tiles applied to st.tiles - sum_{i < npairs} K_i G_i (ring slots 0 .. npairs-1, in slot order), each element loaded once,
// rounded once and stored once; kname as for launch_downdate
hipError_t launch_merge_pass(const DevState &st, void *dst, const int2 *work, int64_t ntiles, const int32_t *src_of, int npairs,
                             int storage, hipStream_t s, char *kname);
// The candidate search in front of a merge (nearest.h): out[i] = (min over j < i of d2(i, j), that j; (+inf, -1) where no pair is
// admissible) for the N landmarks of an UNSHARDED tile store (tm.world == 1: the search needs every tile), d2 as ekf_landmark_distance
// defines it for delta = 0 and the noise covariance R (row-major).  Reads state buffer cur / diagonal buffer st.dcur, writes `out` only.
hipError_t launch_nearest(const DevState &st, int cur, int64_t N, const double R[4], NearestEntry *out, int storage, hipStream_t s);

// A linear observation with a constant Jacobian (linear_obs.h), an UPDATE-STEP on the handle's own ring, like a correction.
// k_gather_linear: the observation's pair into ring position a.npend (float copies included) with every tile operand read patched with
// the a.npend pending pairs, x / Prr / strip into buffer a.cur ^ 1, every landmark's live diagonal block into buffer dcur ^ 1, the record
// into rec, and cnt[0] / cnt[1] (device) incremented where S was irregular / d2 beyond the gate: such a launch leaves a zero pair and
// copies the state.  The caller ends the step as a correction's (finish_step).
hipError_t launch_gather_linear(const DevState &st, const LinearArgs &a, double *rec, int64_t *cnt, int storage, hipStream_t s);
// k_linear_probe: the record that launch would write under the current state, and nothing else
hipError_t launch_linear_probe(const DevState &st, const LinearArgs &a, double *rec, int storage, hipStream_t s);

// An observation through one of the MODELS of ekf_observe_model (model_obs.h): the same step with H formed on the device.
// k_gather_model / k_model_probe: launch_gather_linear / launch_linear_probe for a model, the record and the counters shared with them;
// a target on the robot (q = 0) or a non-finite q counts and reports as an irregular S
hipError_t launch_gather_model(const DevState &st, const ModelArgs &a, double *rec, int64_t *cnt, int storage, hipStream_t s);
hipError_t launch_model_probe(const DevState &st, const ModelArgs &a, double *rec, int storage, hipStream_t s);
// ... with the landmark read on the device (model_assigned.h).  k_gather_model_assigned: launch_gather_model for the landmark slot->landmark
// (device: AssignResult::out[k] of an earlier launch_assign_model on the same stream), a.a left {-1, -1} and a.skipped 0 by the caller; a
// slot that names no landmark below a.n_mm / 2 makes the launch a finite no-op -- a zero pair, the state copied, outcome 3.0 and d2 NaN in
// rec, neither counter touched.  rec: the scan's record of this observation, kLinearRecordDoubles doubles
hipError_t launch_gather_model_assigned(const DevState &st, const AssignedModelArgs &a, const AssignedRecord *slot, double *rec, int64_t *cnt,
                                        int storage, hipStream_t s);
// ... relinearised (model_iter.h).  k_gather_model_iter / k_model_iter_probe: the two launches above with ekfm::model_iterate on lane 0 and the
// last linearisation's pair; rec keeps the FIRST linearisation's S, nu and d2 and the overall outcome, so the counters and the gate mean
// what they mean above, and itrec (device, kIterRecordDoubles doubles) takes the iteration record
hipError_t launch_gather_model_iter(const DevState &st, const IterModelArgs &a, double *rec, int64_t *cnt, double *itrec, int storage, hipStream_t s);
hipError_t launch_model_iter_probe(const DevState &st, const IterModelArgs &a, double *rec, double *itrec, int storage, hipStream_t s);

// The joint compatibility of a scan's pairings (joint.h): k_joint_innovation, one workgroup per hypothesis, read-only.  hyp (device): nh x a.m
// landmarks, 0-based or -1, every one below a.N and none twice in a row; out (device): nh records; d2_prefix (nh x m), nu (nh x 2m) and S
// (nh x (2m x 2m column-major)), device or nullptr, laid out by scan index.  Tile operands are read patched with the a.npend pending pairs.
hipError_t launch_joint_innovation(const DevState &st, const JointArgs &a, const int64_t *hyp, int nh, JointRecord *out, double *d2_prefix,
                                   double *nu, double *S, int storage, hipStream_t s);

// The joint-compatibility search over a scan (joint_search.h), read-only, behind launch_assign_lists on the same stream: sel (device) its
// lists, match (device) its records.  launch_joint_search_prepare: one launch -- the operands of every (entry, candidate), the lists and
// records copied into out, the empty hypothesis.  launch_joint_search_level: scan index `level`'s two launches, k_joint_search_extend over the
// fixed grid of kJointSearchExt and k_joint_search_select; `which`: 0 both, 1 the extend alone, 2 the select alone (a caller that times
// each).  Neither reads anything on the host.
hipError_t launch_joint_search_prepare(const DevState &st, const JointArgs &a, const ekfm::CandList *sel, const int64_t *match,
                                       JointSearchStore *store, JointSearchOut *out, hipStream_t s);
hipError_t launch_joint_search_level(const DevState &st, const JointSearchArgs &a, const JointSearchLevelArgs &la, const ekfm::CandList *sel,
                                     JointSearchStore *store, JointSearchOut *out, int which, int storage, hipStream_t s);

// The joint UPDATE of one hypothesis (joint_update.h, ekf_observe_model_joint), on a flushed state (a.npend == 0).
// launch_joint_factor: k_joint_factor, one workgroup, read-only -- k_joint_innovation's phases for the one hypothesis hyp (device, a.m entries),
// so out / nu / S are what launch_joint_innovation reports for it bit for bit, and blk (device) takes what the gather needs.
hipError_t launch_joint_factor(const DevState &st, const JointArgs &a, const int64_t *hyp, JointBlock *blk, JointRecord *out, double *nu, double *S,
                               int storage, hipStream_t s);
// launch_joint_factor_iter (joint_iter.h): k_joint_factor_iter, launch_joint_factor relinearised up to ia.iterations times -- out / nu / S are
// the FIRST linearisation's (the same bits), blk the LAST one's, itrec (device, kJointIterRecordDoubles doubles) the iteration record.
hipError_t launch_joint_factor_iter(const DevState &st, const JointArgs &a, const JointIterArgs &ia, const int64_t *hyp, JointBlock *blk,
                                    JointRecord *out, double *itrec, double *nu, double *S, int storage, hipStream_t s);
// launch_gather_joint: k_gather_joint over the padded landmark block.  `st` is a by-value copy of the handle's DevState whose Gp / Kp / pcap
// name a PRIVATE F64 pair ring (Gp32 == nullptr): the a.np pairs go to its slots 0 .. a.np - 1, x / Prr / strip into buffer a.cur ^ 1, every
// landmark's live diagonal block into buffer dcur ^ 1; the caller flips both and lets ONE pass apply the pairs to the tiles.
hipError_t launch_gather_joint(const DevState &st, const JointUpdateArgs &a, const JointBlock *blk, int storage, hipStream_t s);

// ---- the calls that treat P as a matrix: the factorisation, the draws and the solves behind it, the plain product, the dense
// observation behind that (launch/map_algebra.h; what sizes their grids and scratch: launch/map_sizes.h, host code without HIP) ----
// k_factor_* (factor_map.h): P of the flushed state `st` factored in the scratch store `a` names -- read-only on st.  The caller queues the
// whole right-looking blocked Cholesky with no host wait: launch_factor_load (the tiles and the right-hand sides; unsharded tile maps only),
// then per tile column k = 0 .. a.rows / a.tm.T - 1 launch_factor_column's three parts in order (the last column has parts 1 and 2 empty),
// then launch_factor_finish (the reductions and the 3 x 3 tail).  a.res must be cleared in front of them (stream order); every launch
// returns at once when a.res[0] says that a pivot failed.  factor_tile_edge(): the edge of the factor store's tiles (the one that is built).
int factor_tile_edge();
hipError_t launch_factor_load(const DevState &st, const FactorMapArgs &a, int storage, hipStream_t s);
hipError_t launch_factor_column(const FactorMapArgs &a, int k, int part, hipStream_t s);      // part 0: diagonal, 1: panel, 2: trailing update
hipError_t launch_factor_finish(const DevState &st, const FactorMapArgs &a, hipStream_t s);
// k_factor_apply / k_factor_sample (sample_map.h): x + C xi for one chunk of factor_chunk() draws, queued behind launch_factor_finish of
// the same `a` (a.lr_off given: the finish stores all of L_r).  part 0: the apply pass, one partial block per segment into sa.part
// (factor_partial_doubles(a.rows) doubles); part 1: the sums, x and the robot rows into sa.y.  Both return at once where a pivot failed.
int factor_chunk();
int64_t factor_partial_doubles(int64_t rows);
hipError_t launch_factor_sample(const DevState &st, const FactorMapArgs &a, const FactorSampleArgs &sa, int part, hipStream_t s);
// k_solve_* (solve_map.h): C^-1 B or P^-1 B for one chunk of factor_chunk() right-hand sides, queued behind launch_factor_finish of the
// same `a` (a.lr_off given).  part 0: the inverses of the diagonal tiles into sv.inv (solve_inverse_doubles(a.rows) doubles), once a
// call; part 1: step c of the forward sweep, c = 0 .. rows / T - 1 ascending; part 2: the robot tail; part 3: step c of the backward
// sweep, c descending (sv.form 0 only).  All return at once where a pivot failed.
int64_t solve_inverse_doubles(int64_t rows);
hipError_t launch_solve_map(const FactorMapArgs &a, const FactorSolveArgs &sv, int part, int c, hipStream_t s);
// k_multiply_tiles / k_multiply_sum / k_multiply_robot (multiply_map.h): P B for one chunk of factor_chunk() vectors on the handle's own tile store, no
// factorisation in front.  multiply_segment(T): the tiles per segment for tile edge T (MultiplyMapArgs::S); multiply_partial_doubles:
// the doubles behind dpart, tpart and wpart together, in that order (multiply_partial_offsets: where the last two begin).  part 0: the
// tile pass (not launched for N = 0); part 1: the sums and, in a one-workgroup launch of its own, the robot rows into a.y.
int multiply_segment(int T);
int64_t multiply_partial_doubles(const TileMap &tm, int64_t rows);
void multiply_partial_offsets(const TileMap &tm, int64_t rows, int64_t *tpart, int64_t *wpart);
hipError_t launch_multiply_map(const DevState &st, const MultiplyMapArgs &a, int part, int storage, hipStream_t s);

// A linear observation with a DENSE H (dense_obs.h, ekf_observe_dense), on a flushed state, behind launch_multiply_map's two stages on the
// chunk that a.b / a.y name (the rows of H in, G = P H' out).  launch_dense_gram: k_dense_gram, a workgroup per segment of landmark rows,
// the partial sums of H G and H x into a.part (dense_partial_doubles(2 N) doubles; no launch at N = 0).  launch_dense_factor: k_dense_factor,
// one workgroup, read-only -- S, nu, the factorisation, d2 and the record into out, what the gather needs into blk.  launch_gather_dense:
// k_gather_dense over the padded landmark block (one workgroup at N = 0), under launch_gather_joint's rules for `st`: the a.kk / 2 pairs go
// to slots 0 .. a.kk / 2 - 1 of the PRIVATE F64 ring, x / Prr / strip into buffer a.cur ^ 1, the diagonal blocks into buffer dcur ^ 1.
int64_t dense_partial_doubles(int64_t n_mm);
hipError_t launch_dense_gram(const DevState &st, const DenseArgs &a, hipStream_t s);
hipError_t launch_dense_factor(const DevState &st, const DenseArgs &a, const DenseSmall &sm, DenseOut *out, DenseBlock *blk, hipStream_t s);
hipError_t launch_gather_dense(const DevState &st, const DenseArgs &a, const DenseBlock *blk, hipStream_t s);

// ---- state I/O (launch/state_io.h) ----
// dense (column-major, n x n, device) <-> tiled
hipError_t launch_unpack_dense(const DevState &st, int cur, int64_t n_mm, double *dense, int storage, hipStream_t s);
hipError_t launch_pack_dense(const DevState &st, int cur, int64_t n_mm, const double *dense, int storage, hipStream_t s);
hipError_t launch_get_block(const DevState &st, int cur, int64_t r0, int64_t c0, int64_t nr, int64_t nc,
                            double *out, int storage, hipStream_t s);
// out (device, 4 * (N+1) doubles): P(1:2,1:2), then the 2x2 diagonal block of every landmark, each column-major
hipError_t launch_get_diag_blocks(const DevState &st, int cur, int64_t N, double *out, int storage, hipStream_t s);
// P = diag(d) + U U' (d: n, U: n x k column-major, device)
hipError_t launch_lowrank(const DevState &st, int cur, int64_t n_mm, const int2 *work, int64_t nwork, const double *d,
                          const double *U, int64_t k, int storage, hipStream_t s);
// out (device, kDigestDoubles doubles; [0..2] = trace, sum and sum of squares over the lower triangle, then a ticket and one
// slot of partial sums per workgroup, added in a fixed order: equal states give bit-equal digests)
constexpr int kDigestGrid = 2048;
constexpr int kDigestDoubles = 4 + 3 * kDigestGrid;
hipError_t launch_digest(const DevState &st, int cur, int64_t n_mm, const int2 *work, int64_t nwork, double *out,
                         int storage, hipStream_t s);
