// The plain data the kernels take by value: the device-resident state, the argument block of every launch, the sizes of the records a launch
// writes.  No HIP type and no HIP header: kernels.h includes this file for the launchers, and the host emulations of tests/support compile the
// kernel sources against the SAME structs (tests/support/kernel_host_shim.h).  The launchers that take them are declared in kernels.h.
#pragma once
#include <stdint.h>

#include "layout.h"

// Device-resident filter state.  Passed BY VALUE to every kernel.
//   x / prr / strip are double-buffered: every kernel reads buffer `cur` and writes a complete buffer
//   `cur ^ 1`, so no workgroup ever reads a value another workgroup of the same launch overwrites.
struct DevState {
    double *x[2];      // state vector, 3 + ldm
    double *prr[2];    // P(1:3,1:3), row-major 3x3
    double *strip[2];  // P(1:3, 4:end): 3 rows of ldm
    void   *tiles;     // local tile store of the landmark block (double or float)
    double *s;         // signatures, cap
    // Pending rank-2 pairs: slot i holds G_i = H_s P(S,:) over landmark columns, interleaved (G(1,c), G(2,c)),
    // and K_i over landmark rows, interleaved (K(r,1), K(r,2)); slots are pair_stride doubles apart.  The tiles
    // hold P_base; the live landmark block is P_base - sum_i K_i G_i (applied in slot order).
    // The slots form a ring of `pcap` entries: a kernel that is told (pstart, npend) sees the pairs in slots
    // (pstart + i) mod pcap, i = 0 .. npend-1, oldest first.
    double *Gp;           // pending G pairs, then (same allocation) ...
    double *Kp;           // ... the pending K pairs: Kp = Gp + pcap * pair_stride (k_gather relies on a 32-bit offset between them)
    float  *Gp32;         // cfg.pass_arith = EKF_ARITH_F32 only (nullptr otherwise): float copies of the same pairs in the same slots, written by the
    float  *Kp32;         // gather beside the F64 ones for the F32-arithmetic pass (half the operand bytes) -- PLANAR (slot s: plane x = ldm floats, then
                          // plane y) and, for K, NEGATED (-(float)K, exact): the pass's LDS-DMA pieces are plain copies (flush32_pipe.h)
    int64_t pair_stride;   // 2 * ldm
    int32_t pcap;          // slots in the ring
    double *small;     // 32: Gr[2][3] (0..5), Kr[3][2] (6..11), Q[9] (12..20)
    int64_t ldm;       // strip leading dimension = landmark-block capacity rounded up to T
    TileMap tm;
    // The 2x2 DIAGONAL blocks of the landmark block, kept LIVE in F64 beside the tiles: landmark k's (P(2k,2k), P(2k+1,2k), P(2k+1,2k+1))
    // at diag[dcur][3k .. 3k+2].  Every correction's gather kernel applies its own pair to them at once (each column lane holds K(c,:)
    // and G(:,c)) -- the chain base - sum_i K_i G_i in slot order that a reader of the tiles would have to re-run over the pending pairs,
    // so in F64 the values equal the patched tile entries bit for bit -- reading buffer dcur, writing dcur ^ 1 (flipped per correction,
    // independently of `cur`: a predict does not touch them).  Why: (1) whoever needs a diagonal block (the correction's own solve, the
    // association of every landmark) reads three doubles instead of patching a chain of pending pairs; (2) with F32 tiles these are the
    // LARGE entries of P (an appended, not yet re-observed landmark: ~17 against a bulk of 0.1) whose sub-ulp updates a float store loses
    // -- in F64 they lose nothing.  Replicated on every shard (the gather is).  The tiles' own copies of these entries keep being
    // maintained by the passes but are no longer read.
    double *diag[2];
    int32_t dcur;
};

// ---- the steps: predict, append, the gather of a correction, association ----
struct PredictArgs {
    double u0, u1, C;
    int64_t n_mm;
    int32_t cur;
};

struct AssocHostPartial;      // (kernels.h, with the association)

// Device-resident measure() loop (EKF_SLAM_UC.m:107-151 without a host round trip per observation): the association decision of
// an observation is PRODUCED on the device (k_associate, or the epilogue of the previous observation's k_gather) as one winner per
// workgroup, and CONSUMED on the device by the next launch (k_gather takes its landmark from the arg-min over those winners;
// k_append checks that nothing passed the threshold).  The host only learns the decisions afterwards, from `rec`.
struct DevLoopArgs {
    const AssocHostPartial *parts_in;   // DEVICE: per-workgroup winners of THIS observation's association; nullptr: not in use
    AssocHostPartial *rec;              // MAPPED HOST: the decision this launch consumed, one self-validating 16-byte store
                                        //   (index: landmark 0-based, -1 = new landmark, -2 = a winner entry did not carry seq_in)
    AssocHostPartial *parts_out;        // DEVICE: winners of the NEXT observation's association, evaluated in k_gather's epilogue
                                        //   on the state this correction leaves (one entry per k_gather workgroup); nullptr: none
    int32_t nblk_in, seq_in;            // entries of parts_in and the launch number they must carry
    int32_t seq_rec, seq_out;           // launch numbers stamped on rec / parts_out
    double z0, z1, z2;                  // the next observation [range, bearing_deg, signature] and its R
    double R00, R01, R10, R11;
    double s_cost, s_thresh, w_pos;
    // cfg.device_assoc == 4 (k_gather<.., kDecide>): the device also takes the branch.  The landmark count lives on the device, in a
    // ring the host advances by one slot per launch: the launch reads *dn_in (n_known >= 0: the host knows it exactly, *dn_in is not
    // read) and writes the count it leaves to *dn_out.  An append (winners: -1) reads the landmark-list entry of key N + 1
    // (EKF_SLAM_UC.m:122) from loc + 3 (N - loc_base) (MAPPED host memory: x, y, number of entries that carry the key) and carries out
    // append(u, R, loc, N + 1) -- unless the key matched no entry or several: then nothing is applied, the record says -4 and every
    // later launch of the same scan (*abort == scan_id) applies nothing either (record -3), as the waited loop stops at that row.
    const int64_t *dn_in;
    int64_t *dn_out;
    int64_t n_known;
    const double *loc;
    int64_t loc_base;
    double u0, u1;
    int32_t *abort;
    int32_t scan_id;
};

struct AppendArgs {
    double u0, u1;
    double R00, R01, R10, R11;
    double pos0, pos1, signature;
    int64_t N;                // landmarks before the append
    int32_t cur;
};

// k_append_model (append_model.h): m <= kAppendModelMax landmarks that start from a range-and-bearing or a relative-position fix, appended
// by ONE launch at the live robot state -- entry b becomes landmark N + b.  Nothing but new slots is written, in place on buffer cur (the
// live diagonal copies: st.dcur); no predict is folded in.  The entries travel in the argument block.
constexpr int kAppendModelMax = 32;
struct AppendModelEntry {
    double z0, z1;            // RANGE_BEARING: range, bearing in degrees; RELATIVE_XY: the landmark in the robot frame
    double R00, R01, R10, R11;
    double signature;
    int32_t model, pad;       // EKF_MODEL_RANGE_BEARING (1) or EKF_MODEL_RELATIVE_XY (4)
};
struct AppendModelArgs {
    int64_t N;                // landmarks before the append
    int32_t m;                // entries in use
    int32_t cur;
    AppendModelEntry e[kAppendModelMax];
};

// k_join_state / k_join_rows (join_map.h): the M landmarks of a LOCAL handle, expressed in the frame of this handle's robot pose and
// independent of its P, joined into the map behind its N landmarks -- local landmark i becomes landmark N + i, the robot composes with the
// local one.  The local handle's DevState travels beside the global one; both are flushed and live on the same device.
struct JoinMapArgs {
    int64_t N;                // landmarks of the global map before the join
    int64_t M;                // landmarks of the local map
    double signature_offset;  // added to every local signature
    int32_t cur;              // the global handle's live buffer: read; cur ^ 1 is written whole
    int32_t lcur;             // the local handle's live buffer: read only
};

// k_extract_state / k_extract_rows (extract_map.h): m landmarks of a flushed SOURCE handle, named by a device list idx (distinct, any order),
// taken out into another handle on the same device, whose whole state is replaced -- destination landmark k is source landmark idx[k].
// The source's DevState travels beside the destination's; the source is read only.
struct ExtractMapArgs {
    int64_t m;                // landmarks taken out
    int64_t cols;             // padded(2 m) of the destination's tile map: the columns k_extract_state writes (zero from 2 m on)
    int32_t frame;            // 0: EKF_FRAME_MAP, the marginal as it is; 1: EKF_FRAME_ROBOT, relative to the robot
    int32_t scur;             // the source's live buffer: read only
    int32_t dcur;             // the destination buffer that is written whole (its diagonal copies: diag[dcur of its DevState])
};

// k_transform_state / k_transform_tiles (transform_map.h): the WHOLE map of a flushed handle moved into another frame, in place -- by the
// rigid transform t = (tx, ty, phi) whose covariance is Sigma (form 0: Sigma = 0, the rotation alone; form 1: the Sigma terms added), or
// into the frame of the robot's own pose (form 2: t and Sigma are not read).  N and s stay.
struct TransformMapArgs {
    int64_t N;                // landmarks
    int64_t cols;             // padded(2 N): the columns k_transform_state writes (zero from 2 N on)
    int32_t form;             // 0: rigid, exact; 1: rigid, uncertain; 2: robot frame
    int32_t cur;              // the live buffer: read; k_transform_state writes cur ^ 1 whole (the diagonal copies: dcur -> dcur ^ 1)
    double t[3];              // the transform, phi in degrees
    double Sigma[9];          // its covariance, row-major (symmetric)
};

// k_factor_* (factor_map.h): the Cholesky factorisation of P of a flushed handle in a scratch store of its own -- F64 lower-triangle tiles
// of edge tm.T under their own tile map (world = 1), whatever the handle's tile edge and storage kind are.  Nothing of the state is written.
constexpr int kFactorRefMax = 8;                  // reference states of one call
constexpr int kFactorRhs = 3 + kFactorRefMax + 1; // doubles per row of the right-hand sides: the strip's three, one per reference, one of padding
constexpr int kFactorRes = 16;                    // doubles of the result block (factor_map.h: k_factor_finish); the pivots follow it
struct FactorMapArgs {
    double *tiles;            // the factor store: row_base(rows / tm.T) tiles
    double *rhs;              // rows x kFactorRhs, row-major
    double *res;              // kFactorRes doubles of status and results (cleared before the first launch), then `rows` pivots (the diagonal of L)
    const double *ref;        // nref reference states on the device, ref_stride doubles apart (nullptr with nref == 0)
    TileMap tm;               // of the factor store
    int64_t N;                // landmarks
    int64_t rows;             // 2 N rounded up to whole tile rows of the factor store
    int64_t ref_stride;
    int32_t nref;             // 0 .. kFactorRefMax
    int32_t cur;              // the live buffer of x, Prr and the strip (the diagonal copies: dcur of the DevState)
    double *lr_off;           // where k_factor_finish stores L_r(1,0), L_r(2,0), L_r(2,1) once the tail is taken whole; nullptr: not stored
};

// k_factor_apply / k_factor_sample (sample_map.h): x + C xi for one chunk of kFactorChunk draws behind a factorisation that FactorMapArgs
// describes.  A chunk is kFactorChunk COLUMNS ld doubles apart, one draw a column in elimination order: entries [0, rows) the landmark
// part (zero from 2 N on), entries rows .. rows + 2 the robot's.  Tile row I of the factor store is cut into segments of S tiles
// (I / S + 1 of them); every segment leaves one partial block of tm.T x kFactorChunk doubles, row-major.
constexpr int kFactorChunk = 16;                  // one v_mfma_f64_16x16x4_f64 N-width
struct FactorSampleArgs {
    const double *xi;         // the draws of the chunk
    double *y;                // the samples of the chunk, in the same layout (entries 2 N .. rows - 1 are not written)
    double *part;             // factor_segment_base(rows / tm.T, S) partial blocks, then rows / tm.T parts of W' Xi, 3 x kFactorChunk doubles each
    int64_t ld;               // >= rows + 3
};
// the partial blocks in front of tile row I's: rows g S .. g S + S - 1 have g + 1 segments each
EKF_HD int64_t factor_segment_base(int64_t I, int64_t S) {
    const int64_t g = I / S;
    return S * g * (g + 1) / 2 + (I - g * S) * (g + 1);
}

// k_solve_* (solve_map.h): C^-1 B or P^-1 B for one chunk of kFactorChunk right-hand sides behind the same factorisation.  The chunks
// have FactorSampleArgs' layout: a right-hand side is a column in elimination order, ld doubles apart.
struct FactorSolveArgs {
    double *b;                // in: the right-hand sides of the chunk; the forward sweep updates it in place; form 0: P^-1 b is left here
    double *y;                // the forward sweep's result u = C^-1 b (form 1's result); the backward sweep updates it in place
    double *inv;              // rows / tm.T tiles of edge tm.T, row-major: the inverses of the factor's diagonal tiles
    int64_t ld;               // >= rows + 3
    int32_t form;             // 0: P^-1 b (EKF_SOLVE_FULL), 1: C^-1 b (EKF_SOLVE_HALF)
};

// k_multiply_tiles / k_multiply_sum (multiply_map.h): P B for one chunk of kFactorChunk vectors on the handle's OWN tile store (the DevState's
// tile map: any edge, either storage kind).  A chunk has FactorSampleArgs' layout under the handle's tile edge: a vector is a column, ld
// doubles apart -- entries [0, rows) the landmark part in x's order (zero from 2 N on), entries rows .. rows + 2 the robot's.  Tile row I
// is cut into segments of S tiles (I / S + 1 of them).
struct MultiplyMapArgs {
    const double *b;          // the vectors of the chunk
    double *y;                // their products, in the same layout (entries 2 N .. rows - 1 are not written)
    double *dpart;            // factor_segment_base(rows / T, S) direct partial blocks of T x kFactorChunk doubles, row-major
    double *tpart;            // row_base(rows / T) blocks of the same shape: the transposed partial of tile (I, J), J < I, at slot(I, J) (the diagonal slots stay unused)
    double *wpart;            // rows / T parts of strip B_m, 3 x kFactorChunk doubles each
    int64_t ld;               // >= rows + 3
    int64_t N;                // landmarks
    int64_t rows;             // 2 N rounded up to whole tile rows of the handle's store
    int32_t S;                // tiles per segment, >= 1
    int32_t cur;              // the live buffer of Prr and the strip (the diagonal copies: dcur of the DevState)
};

// k_predict_model (predict_model.h): a chain of m <= kPredictModelMax motion steps through the models of ekfm::motion_eval, carried out in
// order by ONE launch that reads buffer cur and writes buffer cur ^ 1, as k_predict.  No tile is read: the storage type does not matter.
// The steps travel in the argument block, M as its six unique entries -- 80 bytes a step, 2.5 KiB at 32 (nine entries a step would not fit
// the 4 KiB argument block beside DevState).
constexpr int kPredictModelMax = 32;
struct PredictModelStep {
    int32_t model, pad;       // EKF_MOTION_TURN_DRIVE (1), _ARC (2) or _POSE_DELTA (3)
    double u[3];              // (d, turn, -), (arc length, turn, -) or (dx, dy, turn); angles in degrees
    double m6[6];             // the inputs' covariance, lower triangle (0,0) (1,0) (1,1) (2,0) (2,1) (2,2); a two-input model: row 2 zero
};
struct PredictModelArgs {
    int64_t n_mm;             // strip columns carried along (2 * landmarks)
    int32_t m;                // steps in use
    int32_t cur;
    PredictModelStep e[kPredictModelMax];
};

struct CorrectArgs {
    double z0, z1;            // [range, bearing_deg]
    double R00, R01, R10, R11;
    int64_t j;                // landmark-block row of the corrected landmark (2*idx)
    int64_t n_mm;             // active landmark-block size (2N)
    int32_t cur;
    int32_t npend;            // pending pairs before this correction; its own pair goes to ring position npend
    int32_t pstart;           // ring slot of the oldest pending pair
};

struct AssocArgs {
    double z0, z1, z2;
    double R00, R01, R10, R11;
    double s_cost, s_thresh, w_pos;
    int64_t N;
    int32_t cur;
    int32_t npend;
    int32_t pstart;
    int32_t own_only;         // sharded association with an exchange: nominate only landmarks whose diagonal block this shard holds
    const int64_t *dN;        // k_associate<.., kDevN> (cfg.device_assoc == 4): the landmark count on the device (nullptr: N is exact);
                              //   N is then the host's upper bound, which only sizes the grid
};

// k_assoc_model / k_assoc_model_reduce (associate_model.h): a scan of m <= kAssocModelMax observations under ekf_observe_model's conventions
// scored against all N landmarks, read-only, from the live F64 copies alone (x, Prr, the strip, the diagonal blocks of buffer cur / st.dcur):
// no tile is touched, so the storage type does not matter.  The entries travel in the argument block.
constexpr int kAssocModelMax = 32;
struct AssocModelEntry {
    double z[2];
    double R[4];              // row-major; a one-row model: [r, 0, 0, 1] and z[1] = 0 (model_parse)
    double gate;              // feeds the count `within` alone
    int32_t model, pad;       // EKF_MODEL_* 1-4
};
struct AssocModelArgs {
    int64_t N;                // landmarks, >= 1
    int32_t m;                // entries in use
    int32_t cur;
    AssocModelEntry e[kAssocModelMax];
};

// k_assign_candidates / k_assign_select / k_assign_solve (assign_model.h): the scan of k_assoc_model assigned to the map one-to-one.  The
// first launch takes AssocModelArgs as k_assoc_model does; the solver needs only the gates.  Everything a call returns lies in ONE block,
// so that one copy brings it back: the head (out, total, match) always, the lists behind it where they are asked for.
constexpr int kAssignCandidates = 32;
struct AssignSolveArgs {
    int32_t m, pad;
    double gate[kAssocModelMax];
};
struct AssignedRecord {        // ekf_model_assigned, field by field
    int64_t landmark;
    double d2;
    int64_t ncand, reserved;
};
struct AssignResult {
    AssignedRecord out[kAssocModelMax];
    double total, pad;
    int64_t match[kAssocModelMax * 6];                        // kAssocModelMax records of ekfm::Match2 (= ekf_model_match)
    int64_t cand[kAssocModelMax * kAssignCandidates];         // row-major, -1 behind a row's ncand entries
    double cand_d2[kAssocModelMax * kAssignCandidates];       // ... +inf there
};

// k_joint_innovation (joint.h): nh <= kJointHypMax hypotheses over one scan of m <= kJointMax observations, each pairing observation k
// with landmark hyp[i * m + k] (or -1: left out), judged JOINTLY -- one workgroup per hypothesis, read-only.  The scan travels in the
// argument block as k_assoc_model's does (the gate is not read); the hypotheses are a device array.  The cross blocks P(l_a, l_b) come
// from the tiles patched with the npend pending pairs from ring slot pstart.
constexpr int kJointMax = kAssocModelMax;
constexpr int kJointHypMax = 256;
constexpr int kJointRows = 2 * kJointMax;   // rows of the largest stacked S
struct JointArgs {
    int64_t N;                // landmarks; every hypothesis entry is -1 or below N
    int32_t m;                // entries in use
    int32_t cur;
    int32_t npend;
    int32_t pstart;
    AssocModelEntry e[kJointMax];
};
// one hypothesis's answer: ekf_joint_result, field by field (outcome: 1 regular, 0 irregular)
struct JointRecord {
    double d2;
    int32_t dof, pairings, outcome, first_irregular;
};

// The joint-compatibility SEARCH over a scan (joint_search.h, ekf_joint_search): a level per scan index, at most kJointSearchBeam
// hypotheses alive between two levels, each extended by the first kJointSearchCand candidates of the level's entry and by "left out".
// Everything lives in ONE device store: the operands of the (entry, candidate) pairs, the extensions of the level in flight, and per
// level and alive slot a NODE -- the two factor rows its pairing appended (ekfm::joint_append_*: L's entries, the pivot's root, then y),
// the hypothesis so far, and per earlier level the slot of its ancestor and the candidate it took, which is how a workgroup finds its
// parent's factor rows without copying them.  Node level k holds what is alive BEFORE scan index k; level 0 is the empty hypothesis.
constexpr int kJointSearchCand = 4;
constexpr int kJointSearchBeam = 64;
constexpr int kJointSearchExt = kJointSearchBeam * kJointSearchCand;        // extensions that append rows: (parent, candidate)
constexpr int kJointSearchSlots = kJointSearchBeam * (kJointSearchCand + 1);   // ... and "left out" behind each parent's candidates
constexpr int kJointSearchRow = kJointRows + 2;                             // a row's entries, its diagonal, its y (row 63: 65 entries)
struct JointSearchResult {        // ekf_joint_search_result, field by field
    int64_t lm[kJointMax];
    double d2;
    int32_t dof, pairings, truncated, nalive, irregular;
    int32_t tested[kJointMax], survived[kJointMax];
};
struct JointSearchOperand {       // ekfm::joint_pairing's outputs for one (entry, candidate)
    double Hr[6], Ht[4], strip[6], S[4], nu[2];
    int64_t lm;
    int32_t posed, pad;
};
struct JointSearchExt {
    double row[2][kJointSearchRow];
    double d2;                    // NaN: irregular
};
struct JointSearchNode {
    double row[2][kJointSearchRow];
    double d2;
    int64_t hyp[kJointMax];       // by scan index: the 0-based landmark, -1 = left out
    int32_t anc[kJointMax];       // by scan index k: its ancestor's slot at node level k + 1
    int32_t slot[kJointMax];      // by scan index: the candidate taken, -1 = left out
    int32_t dof, pairings;
};
struct JointSearchStore {
    JointSearchOperand op[kJointMax * kJointSearchCand];
    int32_t nalive[kJointMax + 2];                // by node level: hypotheses alive
    int32_t nirregular[kJointMax + 2];            // by node level: extensions without a d2 so far
    JointSearchExt ext[kJointSearchExt];
    JointSearchNode node[(kJointMax + 1) * kJointSearchBeam];
};
// what one call brings back, in the order of what is asked for: the head always, the final beam, the candidate lists
struct JointSearchOut {
    JointSearchResult res;
    int64_t match[kJointMax * 6];                             // ekfm::Match2 (= ekf_model_match) per entry
    double alive_d2[kJointSearchBeam];                        // NaN behind nalive
    int64_t alive_hyp[kJointSearchBeam * kJointMax];          // row-major nalive x m, -1 behind
    int64_t cand[kJointMax * kAssignCandidates];              // k_assign_select's lists
    double cand_d2[kJointMax * kAssignCandidates];
};
struct JointSearchArgs {          // k_joint_search_extend
    int64_t N;
    int32_t m, level, cur, npend, pstart, pad;
};
struct JointSearchLevelArgs {     // k_joint_search_select
    double threshold[kJointRows + 1];     // by dof
    int32_t rows[kJointMax];              // by scan index: 2 for a two-row model, 1 for a one-row model
    int32_t m, level, beam, pad;
};

// The joint UPDATE of one hypothesis (joint_update.h, ekf_observe_model_joint): k_joint_factor leaves what k_gather_joint needs in one device
// block -- with L L' = S the factor of the stacked S, y = L^-1 nu, the Jacobian blocks of every pairing and the robot part
// W_r = L^-1 G_r, G_r(2p + r, t) = H_p^r(r, :) Prr(:, t) + H_p^t(r, :) strip(t, l_p)' -- and k_gather_joint forms W = L^-1 H P column by column.
struct JointBlock {
    double L[kJointRows * kJointRows];      // the lower triangle, leading dimension kJointRows; rows below 2 np
    double y[kJointRows];
    double Wr[kJointRows][3];
    double Hr[kJointMax][6], Ht[kJointMax][4];   // by pairing, row-major 2 x 3 and 2 x 2
    int64_t lm[kJointMax];                  // by pairing: the landmark
    int32_t np, pad;                        // pairings (rows: 2 np)
    JointRecord rec;
};
struct JointUpdateArgs {
    int64_t n_mm;             // active landmark-block size (2N)
    int32_t cur;
    int32_t np;               // pairings, as the host read them back in the record: the pairs go to ring slots 0 .. np - 1
};
// ... relinearised up to `iterations` times (joint_iter.h, ekf_observe_model_joint_iterated): the loop's controls beside JointArgs.  The
// JointBlock is the LAST linearisation's; the gate is read at the first.
struct JointIterArgs {
    double gate;              // d2 of the first linearisation above it: no step is taken (used = 0)
    double tol;               // the loop stops where the largest move of an entry is <= tol
    int32_t iterations;       // 1 .. kJointIterMax
    int32_t pad_;
};
constexpr int kJointIterMax = 16;
constexpr int kJointSubMax = 3 + 2 * kJointMax;       // entries of the largest sub-state (x_r and the paired landmarks)
// the second record of such a launch: used (0) | converged (1) | the last step (2) | d2 of the last linearisation (3) | the linearisation
// that was irregular, or -1 (4) | the scan index of its first irregular pairing, or -1 (5) | ns (6) | 0 (7) | x'_sub = xi_used (8 .. 8 + ns)
constexpr int kJointIterRecordDoubles = 8 + kJointSubMax + 1;

// A linear observation with a DENSE k x n H (dense_obs.h, ekf_observe_dense): the rows of H are the vectors of ONE chunk of
// k_multiply_tiles (MultiplyMapArgs' layout: row i is column i of the chunk b, its product G_i = P H_i' column i of y), kk = k rounded up
// to even rows, the last one exactly empty where k is odd.  k_dense_gram cuts the landmark rows [0, 2 N) into segments of kDenseSegment
// rows and leaves one block of kDensePartial sums per segment: the lower triangle of H G by rows ((i, j), j <= i, at i (i + 1) / 2 + j),
// then the kDenseMax sums of H x.  k_dense_factor adds them in ascending segment order, then the robot's three terms, then R.
constexpr int kDenseMax = kFactorChunk;
constexpr int kDenseSegment = 128;
constexpr int kDensePartial = kDenseMax * (kDenseMax + 1) / 2 + kDenseMax;
struct DenseArgs {
    const double *b;          // the chunk of H's rows (device)
    const double *y;          // the chunk of G = P H' (device); rows 2 N .. rows - 1 are never read
    double *part;             // cdiv(2 N, kDenseSegment) blocks of kDensePartial doubles
    int64_t ld, rows;         // the chunk's leading dimension and the robot entries' offset (MultiplyMapArgs::ld, ::rows)
    int64_t n_mm;             // 2 N
    int32_t kk;               // rows of the stacked system, even, 2 .. kDenseMax
    int32_t cur;
};
struct DenseSmall {           // what k_dense_factor alone reads: z, R (row-major, leading dimension kDenseMax) and the wrap flags, padded by the host
    double z[kDenseMax];
    double R[kDenseMax * kDenseMax];
    int32_t wrap[kDenseMax];
};
// the answer of a call: ekf_observe_dense_result field by field (outcome: 1 regular, 0 irregular), then nu and S (leading dimension kDenseMax)
struct DenseRecord {
    double d2;
    int32_t rows, outcome, bad_row;
};
struct DenseOut {
    DenseRecord rec;
    double nu[kDenseMax];
    double S[kDenseMax * kDenseMax];
};
// what k_dense_factor hands k_gather_dense: L (the pivot's root on the diagonal), y = L^-1 nu, W_r = L^-1 G_r
struct DenseBlock {
    double L[kDenseMax * kDenseMax];
    double y[kDenseMax];
    double Wr[kDenseMax][3];
};

// ---- map edits, and the observations that share the constraint's device code ----
// A constraint between two landmarks (constrain.h): "l_i - l_j was observed as (d0, d1) with noise covariance R".
struct ConstrainArgs {
    double d0, d1;
    double R00, R01, R10, R11;
    int64_t ai, aj;           // landmark-block rows of the two landmarks (2 * index), ai != aj
    int64_t n_mm;             // active landmark-block size (2N)
    int32_t cur;
    int32_t npend;            // ring position the pair goes to (the ring is empty when the kernel runs: 0) ...
    int32_t pstart;           // ... counted from this slot
};
// the record of launch_gather_constrain_chain: S row-major, nu, d2 as ekfm::constrain_d2 gives it, 1.0 / 0.0 = S regular or not
constexpr int kConstrainRecordDoubles = 8;

// one landmark's answer of the candidate search (nearest.h): the smallest d2 to an earlier landmark and that landmark; (+inf, -1): none admissible
struct alignas(16) NearestEntry { double d2; int64_t partner; };

// A linear observation with a constant Jacobian (linear_obs.h): "H x was observed as z with noise covariance R", H = a 2x3 block on
// the robot state and 2x2 blocks on up to two landmarks.  An UPDATE-STEP on the handle's own ring, like a correction.
struct LinearArgs {
    double z[2];
    double R[4];              // row-major
    double H[14];             // row-major 2 x 7: the robot block (columns 0..2), landmark a[0]'s (3, 4), landmark a[1]'s (5, 6); zeros where absent
    double gate;              // applied only if d2 <= gate (+inf: always)
    int64_t a[2];             // landmark-block rows of the landmarks that carry a block (2 * index), -1 = none; different when both >= 0
    int64_t n_mm;             // active landmark-block size (2N)
    int32_t wrap[2];          // row r of nu is an angle in degrees: wrapped into (-180, 180]
    int32_t cur;
    int32_t npend;            // pending pairs before this step; its own pair goes to ring position npend
    int32_t pstart;           // ring slot of the oldest pending pair
};
// the record of a launch: S row-major, nu, d2 as ekfm::constrain_d2 gives it, the outcome (1.0 applied, 0.0 S irregular, 2.0 gated)
constexpr int kLinearRecordDoubles = 8;

// An observation through one of the MODELS of ekf_observe_model (model_obs.h): the update-step above with h(x) and its Jacobian H
// evaluated on the device at the live x (ekfm::model_eval), nu = z - h(x).  H is no argument: lane 0 of every workgroup forms it.
struct ModelArgs {
    double z[2];
    double R[4];              // row-major
    double anchor[2];         // the target of models 1-4 where a[0] == -1
    double gate;
    int64_t a[2];             // as LinearArgs::a; models 1-4: a[1] == -1, model 5: both >= 0
    int64_t n_mm;
    int32_t model;            // EKF_MODEL_*
    int32_t cur;
    int32_t npend;
    int32_t pstart;
};

// ... with the landmark read on the device from an AssignedRecord an earlier launch left (model_assigned.h): ModelArgs with a[0], a[1] and
// `skipped` set by the KERNEL at entry -- the host leaves them -1, -1, 0.  skipped: the record names no landmark below n_mm / 2, the step is a
// finite no-op with outcome 3.0 (EKF_LINEAR_UNASSIGNED) that no counter counts.
struct AssignedModelArgs : ModelArgs {
    int32_t skipped;
    int32_t pad_;
};

// ... relinearised up to `iterations` times on lane 0 (model_iter.h, ekfm::model_iterate): ModelArgs and the loop's two controls.  The pair
// of the LAST linearisation goes to the ring; the launch's shape, its operands and its outputs are k_gather_model's.
struct IterModelArgs : ModelArgs {
    int32_t iterations;       // 1 .. ekfm::kModelIterMax
    int32_t pad_;
    double tol;               // the loop stops where the largest move of an entry is <= tol (0: all of them, but for a move of exactly 0)
};
// the second record of such a launch: the last linearisation's S row-major (0..3) | its residual r (4, 5) | used (6) | converged (7) |
// the last step (8) | xi_used (9..15)
constexpr int kIterRecordDoubles = 16;
