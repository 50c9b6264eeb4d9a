/*
 * libekfslam -- C ABI of the MI355X-native EKF-SLAM update engine.
 *
 * The reference (SamShue/EKF_SLAM) is pure MATLAB and has NO plugin / operator / FFI interface; its
 * boundary is the class-method surface of EKF_SLAM.m / EKF_SLAM_UC.m / Correspondence.m / append.m.  Each
 * entry point below names the reference method it replaces (file:line in the reference tree).  A MEX
 * gateway (matlab/ekfslam_mex.c) and a ctypes binding (ekf_slam_amd/_lib.py) bind exactly these symbols.
 *
 * Conventions
 *   - every call returns an int32 status (EKF_OK == 0) and never throws across the ABI;
 *     ekf_last_error(h) gives the message of the last failure on that handle;
 *   - arrays are caller-owned HOST buffers of IEEE doubles; matrices are COLUMN-MAJOR (MATLAB native);
 *   - landmark indices are 0-BASED here (the MEX / Python layers convert from the reference's 1-based);
 *   - angles are degrees, exactly as in the reference;
 *   - a handle is not thread-safe; all work is queued on the handle's HIP stream and calls that return
 *     data synchronise that stream, the others are asynchronous;
 *   - state lives in HBM: x (3+2N), s (N) and P in a tiled symmetric block layout (3x3 robot block,
 *     3 x 2N robot/landmark strip, T x T tiles of the lower block triangle of the landmark block).
 */
#ifndef EKFSLAM_H
#define EKFSLAM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EKF_ABI_VERSION 1

enum {
    EKF_OK = 0,
    EKF_ERR_INVALID_ARG = 1,
    EKF_ERR_NO_DEVICE = 2,   /* no HIP device / HIP runtime failure at create */
    EKF_ERR_HIP = 3,         /* a HIP call failed; see ekf_last_error         */
    EKF_ERR_CAPACITY = 4,    /* append beyond capacity_landmarks              */
    EKF_ERR_INDEX = 5,       /* landmark index outside the state              */
    EKF_ERR_LOOKUP = 6,      /* landmark-table lookup did not match exactly one entry (MATLAB would error) */
    EKF_ERR_STATE = 7,       /* call not valid in the handle's current state  */
    EKF_ERR_COMM = 8         /* multi-GPU exchange failed                     */
};

enum { EKF_MODE_KNOWN = 0,   /* EKF_SLAM.m    : known correspondence   */
       EKF_MODE_UC = 1 };    /* EKF_SLAM_UC.m : unknown correspondence */

enum { EKF_STORE_F64 = 0,    /* P tiles stored as double                               */
       EKF_STORE_F32 = 1 };  /* P tiles stored as float, every solve still in double   */
enum { EKF_ARITH_F64 = 0,    /* the pass over P forms P - sum K_i G_i in double (one rounding per pass when the tiles are float) */
       EKF_ARITH_F32 = 1,    /* F32 tiles with tile = 256 only: the pass runs on the f32 matrix pipe (cfg.pass_arith below)      */
       EKF_ARITH_SPLIT3 = 2 };/* as EKF_ARITH_F32, every float operand cut exactly into three bfloat16 pieces: bf16 matrix pipe  */

/* Hard-coded property defaults of the reference collected in one struct
 * (EKF_SLAM.m:12-16, EKF_SLAM_UC.m:13,16). */
typedef struct ekf_config {
    double  C;                   /* process-noise constant              EKF_SLAM.m:12               */
    double  Rc[2];               /* measurement-noise constants         EKF_SLAM.m:13 / _UC.m:13    */
    double  s_cost;              /* signature cost                      EKF_SLAM.m:14 / _UC.m:16    */
    double  s_thresh;            /* new-landmark threshold              EKF_SLAM.m:16 / _UC.m:16    */
    double  w_pos;               /* weight of the Mahalanobis position cost in the association
                                    likelihood; 0 reproduces the live line Correspondence.m:75,
                                    1 the commented-out line Correspondence.m:74                    */
    int64_t capacity_landmarks;  /* HBM is sized for this many landmarks (streaming append never reallocates) */
    int32_t mode;                /* EKF_MODE_*  (selects the ekf_measure dispatch)                  */
    int32_t storage;             /* EKF_STORE_*                                                     */
    int32_t device;              /* HIP device ordinal                                              */
    int32_t tile;                /* tile edge T in elements: 16, 32, 64, 128 (256 for F32 storage);
                                    0 = default (128 for F64 storage, 256 for F32 storage)           */
    int32_t rank;                /* shard rank  (0 when world == 1)                                 */
    int32_t world;               /* number of shards P is split over; 0 or 1 = unsharded            */
    int32_t batch;               /* deferred downdate: up to `batch` corrections are kept as pending rank-2
                                    pairs (the rows later corrections need are patched on the fly) and applied
                                    to P in ONE pass; with F64 tiles results are bit-identical to batch = 1 (F32 tiles round once
                                    per pass, so the batch moves the roundings: equal within the F32 tolerance).  0 or 1 = every
                                    correction rewrites P immediately (EKF_SLAM.m:145 as written); max 64  */
    int32_t async_flush;         /* run each pass over P on a second stream, from the current tile store into a
                                    second one (2x tile memory), while the next corrections go on reading the current
                                    store plus all pending pairs; stores swap at the next batch boundary.  With
                                    batch = 1 that is the as-written update-step software-pipelined: the pass of step i
                                    beside the gather (and, sharded, the exchange) of step i + 1.  Same bits as
                                    async_flush = 0 with F64 tiles (with F32 tiles the corrections beside a pass read its pairs
                                    unrounded where the synchronous engine reads the rounded tiles: equal within the F32 tolerance).  The second stream is confined to a CU mask that leaves 32 CUs
                                    (64 with EKF_ARITH_SPLIT3) to the main stream.  ekf_append beside a pass does not wait for it
                                    (the new rows reach the second store when the pass retires).  Pays when a batch's steps take
                                    about as long as its pass; with batch = 1 it has measured slower than the in-place
                                    pass at every map size on one GPU (two stores defeat the cache). */
    int32_t device_assoc;        /* EKF_MODE_UC, ekf_measure (EKF_SLAM_UC.m:107-151), when w_pos == 0 (the reference's live likelihood is
                                    signature-only, Correspondence.m:75, so WHETHER a row appends or corrects is a function of z(3) and
                                    s alone and the host's mirror of s can predict it):
                                    3 (default of EKF_MODE_UC): the device-resident loop.  Every observation's association runs on
                                       the device (per-landmark phi_k, Mahalanobis and signature cost, thresholded arg-min:
                                       Correspondence.m:49-87 as the reference evaluates it) and its decision is CONSUMED on the
                                       device: the correction's gather kernel takes its landmark from the association's winners, and
                                       evaluates the next observation's association in its own epilogue (one launch per
                                       observation); an append checks that nothing passed the threshold.  The host queues all m rows
                                       without a single wait -- which branch it queues is its mirror's prediction -- and the decisions
                                       the device took come back as records that are checked against the prediction later: the
                                       next ekf_measure checks what has landed, every call that synchronises or reads or loads state
                                       (ekf_sync, ekf_get_*, ekf_set_*, ...) checks the rest first and returns EKF_ERR_STATE on a
                                       mismatch (it cannot happen unless s was changed behind the library's back).  On a sharded
                                       handle the same loop runs on every shard (the association reads replicated data only): a
                                       correction extracts the row-panel of the landmark the device names, exchanges it (the library's
                                       communicator or the hook of transport (d)) and gathers on the exchanged panel.
                                    0: the decision is taken from the host mirror of s -- no association launch at all;
                                    1: the association kernel runs for every observation and the host WAITS for its decision;
                                    2: the kernel runs for every observation, the host dispatches on its mirror's decision (passed
                                       to the gather kernel as an argument) and VERIFIES every device decision before ekf_measure
                                       returns (EKF_ERR_STATE on a mismatch).
                                    With w_pos != 0 the branch cannot be predicted: under 0-3 the device decides and is waited for (as 1)
                                    whatever this says; ekf_associate() always runs on the device and waits.
                                    4 (opt-in, unsharded handles only -- EKF_ERR_INVALID_ARG at create with world > 1 or force_sharded):
                                       the device-decided branch, for ANY w_pos.  The device evaluates every row's association, takes
                                       the branch (append, or correct landmark k) and carries it out; the host queues the whole scan
                                       without a wait.  The landmark count is then the device's until the rows' records have come back
                                       ("settled"): the next ekf_measure settles what has landed, every other call settles all of them
                                       first and sees the state the waited mode (1) would show.  Every row takes a pending-pair slot (an
                                       append or a stale row writes zeros): with F64 tiles the results are bit-identical to 1; with float
                                       tiles the batch boundaries move (equal within the float tolerance).  To keep the waited mode's
                                       errors exact a scan that could append beyond capacity_landmarks takes the waited path, and a scan
                                       whose possible append keys do not all resolve in the landmark list is settled before ekf_measure
                                       returns (a row whose append key fails applies nothing and stops the scan: EKF_ERR_LOOKUP, as 1).
                                       Stale winner entries apply nothing and make the next settling call return EKF_ERR_STATE. */
    int32_t pass_direction;      /* the pass over P: 0 (default) = every other pass walks its work list backwards when the shard's
                                    tile store exceeds the 256 MiB Infinity Cache (what one pass wrote last the next reads first,
                                    on-die), forwards otherwise; 1 = always forwards; 2 = always alternate.  Same bits. */
    int32_t force_sharded;       /* 1: run the sharded code path (row-panel extraction, exchange, sharded gather) although
                                    world == 1 -- how that path is exercised and timed on a single GPU */
    int32_t pass_arith;          /* EKF_ARITH_*: arithmetic of the pass over P.  EKF_ARITH_F32 ("F32 mixed precision with F64 innovation
                                    solve", BASELINE.json configs[4]) needs storage = EKF_STORE_F32 and tile = 256 (EKF_ERR_INVALID_ARG
                                    otherwise): the pass's update -sum K_i G_i is formed from float copies of the pending pairs and
                                    summed in float on the f32 matrix pipe (three times the f64 pipe's measured rate), then added to the
                                    float tile value ONCE -- an entry still sees one rounding at its own magnitude per pass, as with
                                    EKF_ARITH_F64.  Passes of one or two pairs are purely HBM-bound and keep the F64-arithmetic kernel.
                                    The innovation, S, K, x, the robot block, the strip and the landmarks' 2x2 diagonal blocks are F64 as
                                    always.  Costs pcap x 4 N floats for the copies.  Measured against the F64 engine: DESIGN.md section 5
                                    (the whole configs[4] workload, 40 000 -> 50 000 landmarks: 2e-8).
                                    EKF_ARITH_SPLIT3 (same preconditions): the same float copies, each cut EXACTLY into three bfloat16
                                    pieces (3 x 8 significant bits) in front of the pass; a product is the sum of the six partial
                                    products that matter (what is dropped is at most 2^-23 of it, 0.09 x 2^-24 in the root mean square),
                                    each exact in float, summed in float on the bf16 matrix pipe from zero, then added to the tile
                                    value once.  Same error class as EKF_ARITH_F32 (a float sum of 2m terms; measured against an F64
                                    sum beside the fmaf chain: DESIGN.md section 5), NOT the same bits; at 28-64 pending pairs the
                                    pass is then bound by HBM instead of the f32 matrix pipe.  Up to 27 pairs: EKF_ARITH_F32's kernels
                                    (faster there).
                                    Costs 2 x 768 bytes per row of P for the planes. */
    int32_t reserved[2];
} ekf_config;

typedef struct ekf_handle ekf_handle;

/* ---- library ---- */
int32_t     ekf_abi_version(void);
const char *ekf_status_string(int32_t status);
/* Fill *cfg with the reference's property defaults for `mode` (Rc = [.01,5] known, [.1,5] UC). */
int32_t     ekf_config_default(ekf_config *cfg, int32_t mode);

/* ---- lifecycle: EKF_SLAM() / EKF_SLAM_UC() constructors (EKF_SLAM.m:26-34, EKF_SLAM_UC.m:27-36):
 *      x = [0 0 0], P = 0.1*eye(3), s = [] ---- */
int32_t     ekf_create(const ekf_config *cfg, ekf_handle **out);
int32_t     ekf_destroy(ekf_handle *h);
const char *ekf_last_error(const ekf_handle *h);
/* Use an existing hipStream_t (e.g. torch's current stream) for all subsequent work; NULL restores the
 * handle's own stream. */
int32_t     ekf_set_stream(ekf_handle *h, void *hip_stream);
int32_t     ekf_sync(ekf_handle *h);
/* Apply all pending rank-2 pairs to P now (no-op when nothing is pending).  Every call that reads P
 * (ekf_get_P, ekf_get_P_block, ekf_P_digest) does this itself. */
int32_t     ekf_flush(ekf_handle *h);
int32_t     ekf_pending(ekf_handle *h, int32_t *npending);
/* The reference's tunables are public properties that may be reassigned at any time (EKF_SLAM.m:12-16):
 * update C, Rc, s_cost, s_thresh, w_pos of a live handle. */
int32_t     ekf_set_params(ekf_handle *h, double C, const double Rc[2], double s_cost, double s_thresh, double w_pos);

/* ---- hot path ---- */
/* predict(h,u)  EKF_SLAM.m:40-51 (EKF_SLAM_UC.m:42-53): u = [dD, dTheta_deg]. */
int32_t ekf_predict(ekf_handle *h, const double u[2]);

/* [x_new,F] = f(h,x,u)  EKF_SLAM.m:56-65: pure host function on caller arrays (public method of the
 * reference).  x, x_new: n doubles; F: n x n column-major or NULL. */
int32_t ekf_motion_model(const double *x, int64_t n, const double u[2], double *x_new, double *F);

/* append(h,u,R,landmarkPos,signature)  EKF_SLAM.m:67-98 (EKF_SLAM_UC.m:69-100).  R: 2x2 column-major. */
int32_t ekf_append(ekf_handle *h, const double u[2], const double R[4], const double pos[2], double signature);

/* Correction body of measure()  EKF_SLAM.m:124-145 (EKF_SLAM_UC.m:125-146) for landmark `idx` (0-based):
 * innovation, H_k, phi_k, K, x += K nu, P = (I - K H_k) P.  z = [range, bearing_deg]. */
int32_t ekf_correct(ekf_handle *h, const double z[2], const double R[4], int64_t idx);

/* [newLL,index] = estimateCorrespondence(h,z,R,x,P,s)  Correspondence.m:28-88 on the handle's x, P, s.
 * z = [range, bearing_deg, signature].  *idx is 0-based (== N for a new landmark).  pos_cost / sig_cost:
 * optional N-element outputs (Correspondence.m:69,71), may be NULL. */
int32_t ekf_associate(ekf_handle *h, const double z[3], const double R[4], int32_t *is_new, int64_t *idx,
                      double *pos_cost, double *sig_cost);
/* On a sharded handle (cfg.world > 1) ekf_associate / ekf_measure need NO exchange, whatever w_pos: signatures, x, the robot block and
 * the strip are replicated, and so are the landmarks' own 2x2 diagonal blocks (live F64 copies that every correction's gather kernel
 * updates on every shard) -- every shard scores every landmark and takes the same decision, the unsharded handle's bit for bit.
 * A second protocol exists for hosts that exchange candidates instead: every shard scores the landmarks whose diagonal TILE it
 * holds, the candidates {likelihood, index} -- and the position costs, if asked for -- travel in one all-gather of 4 (+ N) doubles per
 * shard run by the caller between _begin and _finish (ekf_exchange_info, ekf_exchange_local), and every shard takes the same strict
 * arg-min (lowest likelihood, lowest index on ties). */
int32_t ekf_associate_begin(ekf_handle *h, const double z[3], const double R[4], int32_t want_costs);
int32_t ekf_associate_finish(ekf_handle *h, int32_t *is_new, int64_t *idx, double *pos_cost, double *sig_cost);

/* measure(h,laserData,u,landmark_list) AFTER the landmark front-end has run, i.e. the loop
 * EKF_SLAM.m:105-150 / EKF_SLAM_UC.m:107-151 over observed_LL (m x 3 column-major [range, bearing_deg, index]).
 * The landmark struct array the loop looks `loc` up in (landmark_list.landmarkObj.landmark(k).index/.loc,
 * EKF_SLAM.m:111,120) is passed as lm_index (L) and lm_loc (L x 2 column-major).  Dispatch follows
 * cfg.mode, including the reference's quirks: the empty-map row only appends (signature 1), the
 * known-correspondence branch corrects landmark ii (the row number, EKF_SLAM.m:123), R = diag(z1*Rc1, z2*Rc2). */
int32_t ekf_measure(ekf_handle *h, const double *observed_LL, int64_t m, const double u[2],
                    const double *lm_index, const double *lm_loc, int64_t L);

/* Sharded handles, cfg.batch = 1 (every correction rewrites P at once): tell the handle which
 * landmark (0-based) the NEXT ekf_correct will name.  The pass over P that ends the current correction then also extracts that
 * landmark's row-panel into the exchange area (its entries are in registers anyway), so the next update-step starts with its
 * all-gather instead of an extraction launch (with the library's own communicator and buffers that all-gather runs in place).  A hint holds for one correction; a wrong or
 * missing one only costs the extraction launch back.  Results are bit-identical either way.  No-op on other handles. */
int32_t ekf_hint_next(ekf_handle *h, int64_t idx);

/* ---- multi-GPU: P split over `world` shards (cfg.rank / cfg.world), tile (I,J) on shard (I+J) mod world ----
 * x, s, the robot block and the robot/landmark strip are replicated; predict, append and associate need no
 * exchange.  A correction needs the 2 x 2N landmark row-panel P(j:j+1,:), whose T-wide chunk k lives on shard
 * (tile_row(j) + k) mod world: one equal-count all-gather per update-step.  Three ways to run it:
 *   (a) ekf_comm_init: the library owns an RCCL communicator (one process per GPU); ekf_correct / ekf_measure
 *       then run extract -> ncclAllGather -> solve -> downdate on the handle's stream;
 *   (b) ekf_correct_begin, the caller's own all-gather over the device buffers of ekf_exchange_info (e.g.
 *       torch.distributed on buffers given through ekf_exchange_set_buffers), ekf_correct_finish;
 *   (c) ekf_exchange_local: one host thread driving every shard of the filter in ONE process (the way a
 *       MATLAB host would): begin on all handles, ekf_exchange_local, finish on all handles;
 *   (d) ekf_exchange_set_hook: the caller's all-gather as a callback, run wherever (a) would run ncclAllGather -- inside
 *       ekf_correct, ekf_prefetch_rows and, which (b) and (c) cannot do, in the middle of ekf_measure's loop.  The
 *       hook finds the handle between begin and finish (ekf_exchange_info names buffers and count) and returns 0 or
 *       an error; with one host thread per shard it is a barrier, ekf_exchange_local on one thread, a barrier
 *       (ekf_slam_amd/sharding.py: ShardGroup.measure). */
typedef struct ekf_comm_id { char internal[128]; } ekf_comm_id;   /* == ncclUniqueId */
int32_t ekf_comm_unique_id(ekf_comm_id *id);                      /* rank 0 creates it, the host broadcasts it */
int32_t ekf_comm_init(ekf_handle *h, const ekf_comm_id *id);      /* collective over all shards */
int32_t ekf_exchange_set_hook(ekf_handle *h, int32_t (*hook)(void *ctx), void *ctx);   /* hook == NULL removes it */
int32_t ekf_correct_begin(ekf_handle *h, const double z[2], const double R[4], int64_t idx);
int32_t ekf_correct_finish(ekf_handle *h);
/* Latency hiding for hosts that know which landmarks the next corrections touch (a scan's observation list):
 * all-gather the BASE row-panels of up to cfg.batch landmarks in ONE exchange; later corrections on them run with no
 * exchange of their own (the pending pairs are applied inside the gather kernel).  The prefetch is dropped when P is
 * rewritten (a flush) or the map grows.  ekf_prefetch_rows = begin + ncclAllGather + finish (transport (a)); begin /
 * finish bracket the caller's all-gather for transports (b) and (c).  No-op on an unsharded handle. */
int32_t ekf_prefetch_rows(ekf_handle *h, const int64_t *idx, int32_t m);
/* The same for the batch AFTER the current one, announced while the current one is still being recorded: when the current batch
 * completes, the row-panels of these landmarks are extracted AS THE BATCH'S PASS WILL LEAVE THEM (pending pairs applied in slot
 * order, rounded through the storage type -- bit for bit what a prefetch after the pass would read) and exchanged in front of the
 * pass: the next batch starts with its prefetch in place, and the exchange no longer depends on the pass (a build that runs it on a
 * stream of its own beside the pass exists behind a tuning switch; on one GPU it is slower, csrc/host/passes.h: flush_pending).  Dropped if the map grows before the batch completes.  Needs cfg.batch > 1, a synchronous
 * flush and cfg.pass_arith = EKF_ARITH_F64 (EKF_ERR_STATE otherwise); m = 0 withdraws an announcement; no-op on an unsharded handle. */
int32_t ekf_prefetch_next(ekf_handle *h, const int64_t *idx, int32_t m);
int32_t ekf_prefetch_begin(ekf_handle *h, const int64_t *idx, int32_t m);
int32_t ekf_prefetch_finish(ekf_handle *h);
/* Device pointers of the exchange: send area (*count doubles valid for the pending begin) and receive area (world
 * contributions of *count doubles, contribution r from shard r); *count_capacity = largest count at capacity
 * (cfg.batch row-panels, or an association's candidate + one position cost per landmark, whichever is larger). */
int32_t ekf_exchange_info(ekf_handle *h, void **send, void **recv, int64_t *count, int64_t *count_capacity);
/* Use caller-owned device buffers (>= count_capacity and world * count_capacity doubles); NULL restores the own ones. */
int32_t ekf_exchange_set_buffers(ekf_handle *h, void *send, void *recv);
int32_t ekf_exchange_local(ekf_handle **shards, int32_t world);
/* Host-only descriptions of the shard plan (no GPU needed): owner of tile (I,J); its slot in the owner's tile
 * store; which shard / local chunk supplies chunk `chunk` of the row-panel of a landmark in tile row tile_row_j. */
int32_t ekf_shard_owner(int32_t world, int64_t I, int64_t J);
int64_t ekf_shard_slot(int32_t world, int64_t I, int64_t J);
int32_t ekf_shard_panel_source(int32_t world, int64_t tile_row_j, int64_t chunk, int32_t *owner, int64_t *local_chunk);

/* ---- state access (the reference's public properties x, P, Q, s; EKF_SLAM.m:6-9) ---- */
int32_t ekf_num_landmarks(ekf_handle *h, int64_t *N);
int32_t ekf_get_x(ekf_handle *h, double *x /* 3+2N */);
int32_t ekf_set_x(ekf_handle *h, const double *x, int64_t n);
int32_t ekf_get_s(ekf_handle *h, double *s /* N */);
int32_t ekf_set_s(ekf_handle *h, const double *s, int64_t N);
/* Remove the m landmarks idx[0 .. m-1] (0-based, any order) from the map: marginalisation in covariance form -- their entries of x,
 * their signatures and their rows and columns of P are dropped, on the device, with no arithmetic.  Afterwards N is N - m; the surviving
 * landmarks keep their relative order (landmark k becomes k - #{removed < k}: ties of the association still go to the lowest index, and
 * known correspondence corrects landmark `ii`), and every surviving value of x, s and P keeps its BITS in every storage kind.
 * Signatures are NOT renumbered: the reference's convention "a new landmark gets signature N + 1" (EKF_SLAM_UC.m:122-123) can therefore
 * hand out a signature a surviving landmark already carries -- ekf_set_s is the caller's tool for that.
 * Pending corrections are applied first (as for every reader of P), a recorded predict(u) is carried out, and with cfg.device_assoc = 4
 * every queued row is settled.  The tile store is compacted OUT OF PLACE into a second store: a handle without cfg.async_flush allocates
 * it at its first removal and keeps it (ekf_device_bytes reports it; EKF_ERR_HIP with the state untouched if that allocation fails).
 * m == 0: EKF_OK, nothing happens.  Removing all N landmarks leaves the empty map.
 * Refused before anything changes: idx == NULL with m > 0, m < 0, a duplicate (EKF_ERR_INVALID_ARG); an index outside [0, N)
 * (EKF_ERR_INDEX); a handle with world > 1 (EKF_ERR_INVALID_ARG: a compaction moves tiles between shards, which is not built). */
int32_t ekf_remove_landmarks(ekf_handle *h, const int64_t *idx, int64_t m);
/* Tell the filter that landmarks i and j (0-based, i != j) are related: "l_i - l_j was observed as delta, with noise covariance R" -- a
 * LINEAR correction between two landmarks (H = +I2 at landmark i's entries, -I2 at landmark j's), hence the exact Kalman update with no
 * angles:  G = H P,  S = G H' + R,  nu = delta - (l_i - l_j),  K = G' S^-1,  x += K nu,  P -= K G  (P = (I - K H) P, EKF_SLAM.m:145, for
 * this H).  delta == NULL means (0, 0): "the same point"; R (2 x 2, column-major) == NULL means the zero matrix.
 * A synchronising call: the device-resident measure loop is settled, a recorded predict(u) is carried out, pending corrections are
 * applied and an asynchronous pass is retired (as for every reader of P); then the pair (K, G) is formed on the device and applied by one
 * pass over P BEFORE the call returns: ekf_pending reports 0 afterwards, whatever cfg.batch says.
 * Refused before anything changes: i == j, a non-finite delta or R, an R that is not symmetric or has a negative diagonal entry or
 * determinant (EKF_ERR_INVALID_ARG); a handle with world > 1 (EKF_ERR_INVALID_ARG: the pair needs two exchanged row-panels, which is not
 * built for sharded handles); a sharded correction between begin and finish (EKF_ERR_STATE); an index outside [0, N) (EKF_ERR_INDEX).
 * An S that is not finite or not positive definite (two perfectly correlated identical landmarks with R = 0 give S = 0) is refused
 * with EKF_ERR_STATE: x, s and P are then what the getters reported before the call. */
int32_t ekf_constrain_landmarks(ekf_handle *h, int64_t i, int64_t j, const double delta[2], const double R[4]);
/* Fuse two landmarks that are the same point: ekf_constrain_landmarks(h, keep, drop, NULL, R) followed by
 * ekf_remove_landmarks(h, &drop, 1) -- bit for bit what those two calls leave, with their refusals.  `keep` retains its signature, the
 * survivors keep their order, and keep's index afterwards is keep - (drop < keep).  WHICH pairs to merge is the caller's policy
 * (ekf_landmark_distance is the gate). */
int32_t ekf_merge_landmarks(ekf_handle *h, int64_t keep, int64_t drop, const double R[4]);
/* Fuse the m pairs ONE search yields (ekf_nearest_landmarks) in one call: the state is left as
 *   ekf_constrain_landmarks(h, keep[k], drop[k], NULL, R) for k = 0 .. m-1, in list order, followed by ONE ekf_remove_landmarks(h, drop, m)
 * would leave it -- all indices 0-based in the numbering BEFORE the call, R (2 x 2, column-major, NULL = zero) shared by all pairs.
 * d2[k] (d2 may be NULL) is what ekf_landmark_distance(h, keep[k], drop[k], NULL, R, ..) would report immediately before constraint k,
 * i.e. under the state after constraints 0 .. k-1.  Afterwards N is N - m, the survivors keep their order and signatures, and keep[k]
 * has become keep[k] - #{drop < keep[k]}.  A keep may be shared by several pairs (a triple fuses in one call).
 * With F64 tiles ekf_get_x / _s / _P / _P_diag_blocks, ekf_P_digest and d2 return the SAME BITS as that sequence of calls; with float
 * tiles every float-stored entry is rounded ONCE where the sequence rounds it m times: equal within the float tolerance and closer to
 * the F64 result (what cfg.batch says of corrections).  The unread upper halves of diagonal tiles mirror the canonical entries.
 * On the device: m constraint gathers queued back to back, each reading its operands patched with the earlier pairs of the batch (a
 * private F64 pair ring of EKF_MERGE_BATCH_MAX slots, allocated at the first batch call and kept: cfg.batch and ekf_pending are not
 * involved), one readback of their m records, then ONE pass that applies the m pairs while it compacts the tile store out of place
 * (one read and one write of P) -- counted under EKF_KERNEL_GATHER (m launches) and EKF_KERNEL_DOWNDATE (one), none under
 * EKF_KERNEL_COMPACT.  A synchronising call like ekf_constrain_landmarks; ekf_pending reports 0 afterwards.
 * Refused before anything changes, in ekf_constrain_landmarks' order: m < 0, m > EKF_MERGE_BATCH_MAX, keep or drop NULL with m > 0,
 * keep[k] == drop[k], a landmark named twice in drop, a keep that is also a drop (every keep survives: chains are the caller's to order),
 * an R that ekf_constrain_landmarks would refuse, a handle with world > 1 (EKF_ERR_INVALID_ARG; sharding is not built, a lone shard with
 * cfg.force_sharded works); a sharded correction between begin and finish (EKF_ERR_STATE); an index outside [0, N) (EKF_ERR_INDEX);
 * a failed allocation (EKF_ERR_HIP).  m == 0: EKF_OK, nothing happens.
 * ALL OR NOTHING: if constraint k meets an S that ekf_constrain_landmarks would refuse (not finite, S00 <= 0 or det S <= 0) the call
 * returns EKF_ERR_STATE, ekf_last_error names the pair number k, and x, s, P, the diagonal blocks and the digest are bit for bit what the
 * getters reported before the call (d2 is not written); the handle goes on working. */
#define EKF_MERGE_BATCH_MAX 32
int32_t ekf_merge_landmarks_batch(ekf_handle *h, const int64_t *keep, const int64_t *drop, int64_t m,
                                  const double R[4] /* 2x2 column-major, NULL = zero, shared by all pairs */,
                                  double *d2 /* m, may be NULL */);
/* What a caller gates a merge on: *d2 = nu' S^-1 nu, the squared Mahalanobis distance of "l_i - l_j = delta" under the current state
 * (arguments, synchronisation and refusals as for ekf_constrain_landmarks), and S (2 x 2, column-major; may be NULL).  Changes nothing:
 * x, s, P and ekf_P_digest are afterwards what they were.  A singular S is no error here: it is returned, and *d2 is NaN. */
int32_t ekf_landmark_distance(ekf_handle *h, int64_t i, int64_t j, const double delta[2], const double R[4],
                              double *d2, double S[4] /* column-major, may be NULL */);
/* WHICH pairs to merge -- the candidate search in front of ekf_merge_landmarks: for every landmark i (0-based), partner[i] is the j in
 * [0, i) that minimises d2(i, j), and d2[i] is that minimum.  d2(i, j) is BY DEFINITION the value
 * ekf_landmark_distance(h, i, j, NULL, R, &d2, NULL) yields -- nu' S^-1 nu of "l_i - l_j = 0" under the current state, i the first
 * argument and j < i the second (the rounding of S is not symmetric in the two, so the order is part of the definition) -- bit for bit.
 * A pair for which ekf_landmark_distance yields NaN (S not finite, S00 <= 0 or det S <= 0) never wins: it is skipped.  The comparison
 * is a strict < in ascending j: the lowest index wins ties, as everywhere (Correspondence.m).  Landmark 0 and any row whose pairs are
 * all irregular get partner = -1 and d2 = +inf.  Only j < i is searched, on purpose: a duplicate is the LATER append, so a row reads as
 * ekf_merge_landmarks(h, keep = partner[i], drop = i, R), and the output has the fixed size N.  Gating is the caller's: compare d2[i]
 * with a chi-square value (2 degrees of freedom), as with ekf_landmark_distance.
 * One read-only pass over the tiled P on the device.  Refusals and synchronisation in ekf_constrain_landmarks' order: h, d2 or partner
 * NULL with N > 0, an R that ekf_constrain_landmarks would refuse (EKF_ERR_INVALID_ARG); a handle with world > 1 (EKF_ERR_INVALID_ARG:
 * sharding -- the search needs every tile; a lone shard with cfg.force_sharded owns every tile and works); a sharded correction between
 * begin and finish (EKF_ERR_STATE); then the device-resident measure loop is settled (N exact), a recorded predict(u) is carried out,
 * pending corrections are applied and an asynchronous pass is retired.  N == 0: EKF_OK, nothing written.
 * Changes nothing: x, s, P and ekf_P_digest are afterwards what they were; ekf_pending reports 0, as after ekf_landmark_distance. */
int32_t ekf_nearest_landmarks(ekf_handle *h, const double R[4] /* 2x2 column-major, NULL = zero */,
                              double *d2 /* N */, int64_t *partner /* N */);
/* A LINEAR observation with a constant Jacobian: "H x was observed as z, with noise covariance R" -- a surveyed landmark position, a GPS
 * fix of the robot, a compass reading, a relation between two landmarks.  H has a 2 x 3 block on the robot state and 2 x 2 blocks on up
 * to two landmarks, so the Kalman update is exact, with no linearisation:
 *     G = H P,  S = G H' + R,  nu = z - H x (rows named in wrap_deg wrapped into (-180, 180]),  K = G' S^-1,  x += K nu,  P -= K G,
 *     d2 = nu' S^-1 nu
 * (ekf_constrain_landmarks is the case Hr = 0, Hl = (+I2, -I2)).  rows == 1 is a scalar observation: row 1 of z, H and R is ignored and
 * runs as the exactly empty second row (H(1,:) = 0, R01 = R10 = 0, R11 = 1, z1 = 0), so S = [[s, 0], [0, 1]], nu1 = 0 and d2 = nu0^2 / s.
 * x(3), the heading, is NOT re-wrapped afterwards (as after ekf_correct).
 *
 * ekf_observe_linear is an UPDATE-STEP like ekf_correct, not a synchronising edit: a recorded predict(u) is carried out, then ONE launch
 * (counted under EKF_KERNEL_GATHER) reads its operands patched with the pairs still pending, writes its pair (K, G) into the next slot
 * of the pending ring and updates x; ekf_pending grows by one and the pass over P runs at the batch boundary cfg.batch sets (beside
 * the next steps with cfg.async_flush).  Nothing is flushed and, with res == NULL, nothing is waited for.  With res != NULL the call
 * waits for that launch's record (one small readback) and reports nu, S, d2 and the outcome.
 * An S that is not finite or not positive definite (EKF_LINEAR_IRREGULAR: a landmark fixed twice with R = 0) or a d2 above `gate`
 * (EKF_LINEAR_GATED) turns the launch into a no-op: a zero pair takes the slot (ekf_pending still grows by one) and every value the
 * getters report stays bit for bit what it was.  With res != NULL an irregular S returns EKF_ERR_STATE and a gated observation EKF_OK
 * with res->outcome == EKF_LINEAR_GATED; with res == NULL the call returns EKF_OK either way and ekf_linear_rejections counts them.
 * Refused before anything changes, in this order: obs NULL, rows not 1 or 2, a non-finite entry of z, H or R (of the rows in use), a
 * NaN gate, an R that ekf_constrain_landmarks would refuse (rows == 1: only R00 >= 0 matters), lm[0] == lm[1] >= 0, an lm below -1
 * (EKF_ERR_INVALID_ARG); a handle with world > 1 (EKF_ERR_INVALID_ARG: sharding -- a landmark block needs that landmark's exchanged
 * row-panel, which is not built; a lone shard with cfg.force_sharded works); a sharded correction between begin and finish
 * (EKF_ERR_STATE); then the device-resident measure loop is settled (N exact) and an lm outside [0, N) is EKF_ERR_INDEX.
 *
 * ekf_linear_innovation is the gate a host asks for: nu, S, d2 and the outcome ekf_observe_linear WOULD report under the current
 * state, bit for bit, read patched with the pending pairs -- no flush, and x, s, P, ekf_P_digest and ekf_pending stay what they were
 * (a recorded predict(u) is carried out first, as by every reader).  Arguments and refusals as above; an irregular S is no error here.
 * ekf_linear_rejections synchronises, reports how many ekf_observe_linear launches since the last call did not apply (S irregular;
 * gated) and resets both counts; either pointer may be NULL. */
enum { EKF_LINEAR_APPLIED = 1, EKF_LINEAR_IRREGULAR = 0, EKF_LINEAR_GATED = 2,
       EKF_LINEAR_UNASSIGNED = 3 /* a step of ekf_observe_model_assigned whose observation the assignment left out; nothing else reports it */ };
typedef struct ekf_linear_obs {
    double  z[2];         /* the observed value of H x                                                    */
    double  R[4];         /* 2x2 column-major noise covariance (rules of ekf_constrain_landmarks' R)      */
    double  Hr[6];        /* 2x3 column-major block on the robot state (x, y, theta in DEGREES); zeros = none */
    int64_t lm[2];        /* 0-based landmarks carrying a block, -1 = none; if both >= 0 they differ      */
    double  Hl[2][4];     /* 2x2 column-major block on landmark lm[b]; ignored where lm[b] == -1          */
    double  gate;         /* apply only if d2 <= gate; +inf = no gate                                     */
    int32_t wrap_deg[2];  /* row r is an angle in degrees: nu_r is wrapped into (-180, 180]               */
    int32_t rows;         /* 2, or 1: a scalar observation -- row 1 of z, H, R is ignored                 */
} ekf_linear_obs;
typedef struct ekf_linear_result { double nu[2]; double S[4] /* column-major */; double d2; int32_t outcome; } ekf_linear_result;
int32_t ekf_observe_linear(ekf_handle *h, const ekf_linear_obs *obs, ekf_linear_result *res /* NULL: do not wait */);
int32_t ekf_linear_innovation(ekf_handle *h, const ekf_linear_obs *obs, ekf_linear_result *res /* required */);
int32_t ekf_linear_rejections(ekf_handle *h, int64_t *irregular, int64_t *gated);   /* synchronises, reads and resets */
/* An observation through a MODEL h(x) whose Jacobian depends on the state: "h(x) was observed as z, with noise covariance R" -- a UWB
 * beacon (range only), a camera (bearing only), a lidar or stereo front end (the landmark's position in the robot frame), a tape measure
 * between two beacons.  The update of ekf_observe_linear with H = dh/dx evaluated ON THE DEVICE at the live x (which carries every
 * pending pair) and nu = z - h(x), not z - H x:
 *     G = H P,  S = G H' + R,  nu = z - h(x) (bearings wrapped into (-180, 180]),  K = G' S^-1,  x += K nu,  P -= K G,  d2 = nu' S^-1 nu
 * Unlike ekf_correct, which keeps the reference's conventions, the bearing innovation IS wrapped, the Jacobian carries 180/pi (theta
 * is in degrees), R is the caller's own covariance (no range scaling) and the step can be gated.
 * The target t of models 1-4 is landmark lm[0] (0-based) when lm[0] >= 0; with lm[0] == -1 it is the fixed point `anchor`, a known
 * point that is not in the map: H has no landmark block then and only the robot is corrected through it.  lm[1] is -1 in both cases.
 * EKF_MODEL_LANDMARK_RANGE takes landmarks lm[0] != lm[1], both >= 0, and has no robot block.
 * With p = x(0:2), theta = x(2), d = t - p, q = d'd, r = sqrt(q), k = 180/pi, c = cosd(theta), s = sind(theta):
 *   RANGE_BEARING   h = [r; atan2d(d_y, d_x) - theta]    H(x,y,theta) = [-d_x/r, -d_y/r, 0; k d_y/q, -k d_x/q, -1]
 *                                                         H(t) = [d_x/r, d_y/r; -k d_y/q, k d_x/q]             row 1 wrapped
 *   RANGE           its row 0 alone                       BEARING  its row 1 alone (row 0 wrapped)
 *   RELATIVE_XY     h = [c d_x + s d_y; -s d_x + c d_y]   H(x,y,theta) = [-c, -s, h_1/k; s, -c, -h_0/k]         H(t) = [c, s; -s, c]
 *   LANDMARK_RANGE  h = |l_0 - l_1|                       H = +e' on l_0, -e' on l_1, e = (l_0 - l_1) / |l_0 - l_1|
 * R: 2x2 column-major with ekf_observe_linear's rules; a one-row model reads R[0] >= 0 alone and runs as the pair with the exactly
 * empty second row (S = [[s, 0], [0, 1]], nu1 = 0), as rows == 1 does there.
 * An UPDATE-STEP exactly as ekf_observe_linear: one launch counted under EKF_KERNEL_GATHER, no flush, ekf_pending grows by one, with
 * res == NULL nothing is waited for; gate, res and the outcomes are its.  Where q is 0 or not finite (the target on the robot, the two
 * landmarks of a range on one point) there is no Jacobian: the outcome is EKF_LINEAR_IRREGULAR, the launch is a finite no-op, and with
 * res != NULL the call returns EKF_ERR_STATE.  Launches that do not apply are counted in the SAME two counters ekf_linear_rejections
 * reads and resets: it reports linear and model observations together.
 * Refused before anything changes, in this order: obs NULL, an unknown model, a non-finite entry of z (of the rows in use) or of the
 * anchor (where it is the target), a bad R, a NaN gate, an lm pattern the model does not allow (EKF_ERR_INVALID_ARG); then
 * ekf_observe_linear's rungs: world > 1 (EKF_ERR_INVALID_ARG: sharding, the anchor forms included), a sharded correction in flight
 * (EKF_ERR_STATE), the measure loop settled, an lm outside [0, N) (EKF_ERR_INDEX).
 * ekf_model_innovation is ekf_linear_innovation for a model: what ekf_observe_model WOULD report, bit for bit, nothing changed.
 * ekf_model_evaluate is the function the kernel runs, on the host (pure, like ekf_motion_model): h(x) and H (row-major 2 x 7 over
 * x, y, theta | t0 | t1; rows and blocks a model does not have are zero) at the robot state xr and the targets t0 (models 1-4: the
 * target, landmark or anchor -- an anchor's block of H is not used) and t1 (model 5 alone: the second landmark; else may be NULL).
 * EKF_ERR_STATE (H and hx zero) where q is 0 or not finite. */
enum { EKF_MODEL_RANGE_BEARING = 1, EKF_MODEL_RANGE = 2, EKF_MODEL_BEARING = 3, EKF_MODEL_RELATIVE_XY = 4, EKF_MODEL_LANDMARK_RANGE = 5 };
typedef struct ekf_model_obs {
    int32_t model, reserved;   /* EKF_MODEL_*; reserved: 0                                                    */
    double  z[2];              /* the observed value of h(x); a one-row model reads z[0]                      */
    double  R[4];              /* 2x2 column-major noise covariance; a one-row model reads R[0]               */
    int64_t lm[2];             /* 0-based landmarks, -1 = none (see above)                                    */
    double  anchor[2];         /* the target where lm[0] == -1                                                */
    double  gate;              /* apply only if d2 <= gate; +inf = no gate                                    */
} ekf_model_obs;
int32_t ekf_observe_model(ekf_handle *h, const ekf_model_obs *obs, ekf_linear_result *res /* NULL: do not wait */);
int32_t ekf_model_innovation(ekf_handle *h, const ekf_model_obs *obs, ekf_linear_result *res /* required */);
int32_t ekf_model_evaluate(int32_t model, const double xr[3], const double t0[2], const double t1[2], double hx[2], double H[14]);
/* The same observation RELINEARISED: the iterated EKF update (IEKF), Gauss-Newton on the MAP cost
 *     J(x) = (x - x0)' P^-1 (x - x0) + nu(x)' R^-1 nu(x),  nu(x) = z - h(x) (bearings wrapped).
 * ekf_observe_model linearises h once, at the prior x0; where the prior is wide against the sensor (a new landmark, a heading known to
 * ten degrees, a precise fix) that step lands off the mode.  Here the device repeats, over the seven entries xs = (robot, lm[0], lm[1])
 * and their 7 x 7 covariance, up to `iterations` times (1 .. EKF_MODEL_ITER_MAX):
 *     xi_0 = xs;  (h_i, H_i) at xi_i;  S_i = H_i P H_i' + R;  r_i = wrap(z - h_i) - H_i (xs - xi_i);  xi_{i+1} = xs + P H_i' S_i^-1 r_i
 * and stops after the last one or where step = max_k |xi_{i+1}[k] - xi_i[k]| <= tol (tol = 0: all of them -- but a step of exactly 0,
 * a model that is linear in effect, counts as converged and stops).  The LAST linearisation's H, S and r then make the one rank-2 pair of
 * the step: K = P H' S^-1, x += K r, P -= K H P.  One launch counted under EKF_KERNEL_GATHER with the traffic of ekf_observe_model's, no
 * flush, ekf_pending grows by one.  With iterations = 1 it writes ekf_observe_model's bits.
 * The GATE is read at the first linearisation only: `first` is what ekf_model_innovation reports (its S, nu, d2), and a call is accepted
 * or rejected exactly as it says; first->outcome is the call's.  A later iterate with no Jacobian (q = 0 or not finite) or an irregular S
 * makes the whole call EKF_LINEAR_IRREGULAR: all or nothing, a finite no-op, counted once by ekf_linear_rejections, EKF_ERR_STATE with
 * first != NULL.  With first == NULL nothing is waited for (and `it` must be NULL).
 * it (may be NULL): S (column-major) and nu = r of the linearisation that made the pair; used = the linearisations whose step was taken
 * (0: the first one did not apply; on a later irregular iterate, the ones before it, and S / nu are that iterate's); converged = the
 * last step was <= tol; last_step; x_local = xi_used, the seven entries the pair leaves in x (absent landmarks: 0).
 * Refusals: ekf_observe_model's, in its order, then iterations outside 1 .. EKF_MODEL_ITER_MAX or a NaN or negative tol
 * (EKF_ERR_INVALID_ARG), then its rungs (unsharded, settled).
 * ekf_model_innovation_iterated: the two records ekf_observe_model_iterated WOULD report, bit for bit, nothing changed.
 * ekf_model_iterate is the loop the kernel runs, on the host (pure): sm = the 38 operands (Prr row-major 0..8 | the strip at lm[b]'s
 * columns 9 + 6b + 2t + r | lm[b]'s own block (0,0) (1,0) (1,1) at 21 + 3b | the cross block 27 + 2r + c | the seven entries 31..37), R
 * column-major 2 x 2 as the kernel sees it (a one-row model: [r, 0, 0, 1]), first required, it may be NULL. */
#define EKF_MODEL_ITER_MAX 16
typedef struct ekf_iterated_result { double S[4] /* column-major */; double nu[2]; int32_t used; int32_t converged; double last_step; double x_local[7]; } ekf_iterated_result;
int32_t ekf_observe_model_iterated(ekf_handle *h, const ekf_model_obs *obs, int32_t iterations, double tol,
                                   ekf_linear_result *first /* NULL: do not wait */, ekf_iterated_result *it /* may be NULL */);
int32_t ekf_model_innovation_iterated(ekf_handle *h, const ekf_model_obs *obs, int32_t iterations, double tol,
                                      ekf_linear_result *first /* required */, ekf_iterated_result *it /* may be NULL */);
int32_t ekf_model_iterate(int32_t model, const double sm[38], const double anchor[2], int32_t has_landmark, const double z[2], const double R[4],
                          double gate, int32_t iterations, double tol, ekf_linear_result *first, ekf_iterated_result *it);
/* New landmarks under the SAME conventions: "a landmark that is not in the map yet was seen as z through the model, with noise covariance
 * R".  ekf_append keeps the reference's append (the position from the caller's table, Jacobians built from the motion input, no pi/180)
 * and is the inverse of none of the models above; a filter driven through ekf_observe_model starts its landmarks here.  Only the models
 * that determine a point are accepted, EKF_MODEL_RANGE_BEARING and EKF_MODEL_RELATIVE_XY.  With p = x(0:2), theta = x(2) in degrees,
 * k = 180/pi, the landmark t = g(x_r, z), Gx = dg/dx_r = [1 0 g0; 0 1 g1] and Gz = dg/dz are
 *   RANGE_BEARING  z = (r, b):  (s, c) = sincosd(theta + b)   t = p + r (c, s)   (g0, g1) = (-r s / k, r c / k)   Gz = [c g0; s g1]
 *   RELATIVE_XY    z = (a, b):  (s, c) = sincosd(theta)       w = (c a - s b, s a + c b)   t = p + w
 *                                                              (g0, g1) = (-w_1 / k, w_0 / k)                       Gz = [c -s; s c]
 * evaluated ON THE DEVICE at the live x_r (which carries every pending pair), so that h(g(x, z)) = z, H_t Gz = I and H_r + H_t Gx = 0
 * with ekf_model_evaluate's blocks: right after the call ekf_model_innovation of the same z on the new landmark reports nu = 0, S = 2 R.
 * A batch is one scan: all m entries are inverted at the same x_r, entry b becomes landmark N + b (0-based; *first_idx = N) with
 *     x <- t_b     s <- signature_b     P(new_b, new_b) = Gx_b Prr Gx_b' + Gz_b R_b Gz_b'     P(1:3, new_b) = Prr Gx_b'
 *     P(new_b, old) = Gx_b P(1:3, old)                  P(new_b, new_a) = Gx_b Prr Gx_a'  (a < b)
 * by ONE launch (counted under EKF_KERNEL_APPEND) that writes new slots only -- bit for bit what m calls with one entry leave.  The call
 * returns without waiting for the device, does not flush and leaves ekf_pending as it found it; beside a pass in flight
 * (cfg.async_flush) it does not wait for the pass, as ekf_append.  A recorded predict is carried out first, by a launch of its own.
 * SHARDED handles are supported: everything the launch reads is replicated, so the same call on every shard needs no exchange.
 * Refused with nothing changed, in this order: h or obs NULL, m < 1 or m > EKF_APPEND_MODEL_MAX (EKF_ERR_INVALID_ARG); per entry, an
 * unknown or one-row model, a non-finite z, r <= 0 for RANGE_BEARING, an R that ekf_observe_linear's rules refuse
 * (EKF_ERR_INVALID_ARG); then, with the measure loop settled (cfg.device_assoc = 4: N exact), a sharded correction between begin and
 * finish (EKF_ERR_STATE); N + m > cfg.capacity_landmarks (EKF_ERR_CAPACITY: all or nothing).
 * ekf_model_invert is the function the kernel runs, on the host (pure, like ekf_model_evaluate): t, Gx (row-major 2 x 3) and Gz
 * (row-major 2 x 2) at the robot state xr; EKF_ERR_INVALID_ARG for a NULL argument or any other model. */
#define EKF_APPEND_MODEL_MAX 32
typedef struct ekf_model_init {
    int32_t model, reserved;   /* EKF_MODEL_RANGE_BEARING or EKF_MODEL_RELATIVE_XY; reserved: 0                */
    double  z[2];              /* the observed value                                                          */
    double  R[4];              /* 2x2 column-major noise covariance of z                                      */
    double  signature;
} ekf_model_init;
int32_t ekf_append_model(ekf_handle *h, const ekf_model_init *obs, int64_t m, int64_t *first_idx /* may be NULL */);
int32_t ekf_model_invert(int32_t model, const double xr[3], const double z[2], double t[2], double Gx[6], double Gz[4]);
/* MAP JOINING: a LOCAL map joined into this one on the device.  `local` holds y = [q; m_1 .. m_M] with covariance PL: a filter of its own
 * (any tile edge, any storage kind, same cfg.device) that was started at the pose r = x(0:2) of `h` -- typically ekf_set_x(0), ekf_set_P(0)
 * at the moment `h` stops moving -- so y is expressed in the frame of r and is independent of P.  With theta = r(2) in degrees, k = 180/pi,
 * Rot = Rot(theta) and w(v) = Rot v:
 *     r'  = r (+) q      p' = p + w(q(0:1)), theta' = wrapTo360(theta + q(2)): ekf_motion_evaluate's EKF_MOTION_POSE_DELTA at (r, q),
 *                        J1 = its F, J2 = its V = blockdiag(Rot, 1)
 *     g_i = p + w(m_i)   ekf_model_invert's EKF_MODEL_RELATIVE_XY at (r, m_i), Gx_i = [1 0 -w_1(m_i)/k; 0 1 w_0(m_i)/k], Gz = Rot
 * The old landmarks stay; local landmark i becomes landmark N + i (0-based; *first_idx = N) with signature s_local[i] + signature_offset, and
 * P' = J blockdiag(P, PL) J', block by block (strip = P(1:3, landmarks)):
 *     P'(1:3,1:3)     = J1 P(1:3,1:3) J1' + J2 PL_qq J2'           strip'(old c) = J1 strip(:, c)
 *     strip'(new i)   = J1 (P(1:3,1:3) Gx_i') + J2 PL(q, m_i) Rot'
 *     P'(new i, old c) = Gx_i strip(:, c)  (the OLD strip)         P'(new i, new a) = Gx_i (P(1:3,1:3) Gx_a') + Rot PL(m_i, m_a) Rot'
 * and nothing of P(old, old) read or written.  Two launches, counted under EKF_KERNEL_APPEND: the small part and the strip (one lane per
 * column), and the new tile rows (one lane per 2 x 2 block, the local tile store read once, the new rows written once).  M has no limit but
 * the capacity; M = 0 is a pure pose composition -- bit for bit ekf_predict_model's POSE_DELTA step with u = q, M = PL_qq -- and N = 0 is
 * allowed.  A local map with q = 0, PL_qq = 0, PL(q, .) = 0 and a block-diagonal PL_mm leaves bit for bit what ekf_append_model leaves for
 * EKF_MODEL_RELATIVE_XY entries (z = m_i, R = PL(m_i, m_i)).  What makes it a join: the local map's internal geometry does not depend on
 * where it is attached -- a RELATIVE_XY innovation of new landmark N + i on `h` reports the nu and S it reports for landmark i on `local`.
 * A SYNCHRONISING call on BOTH handles, like ekf_constrain_landmarks: both are settled, recorded predicts carried out, pending pairs applied,
 * an asynchronous pass retired (ekf_pending is 0 on both afterwards); `local`'s stream is drained before `h`'s stream reads its buffers and
 * `h`'s stream is drained before the call returns, so ekf_destroy(local) or any edit of it right afterwards is safe.  Apart from that flush
 * `local` is left bit for bit as it was.  The usual next steps are ekf_nearest_landmarks and ekf_merge_landmarks_batch, which fuse the
 * landmarks both maps saw.
 * Refused with nothing changed: h or local NULL, h == local, a non-finite signature_offset, either handle sharded (world > 1 or
 * cfg.force_sharded), different cfg.device (EKF_ERR_INVALID_ARG); then, with both measure loops settled, N + M > cfg.capacity_landmarks
 * of `h` (EKF_ERR_CAPACITY: all or nothing).  A step that fails on `local` (settling or flushing it) is reported on `h`, its message
 * quoting `local`'s, which `local`'s own ekf_last_error holds as well.  The host's mirror of the new signatures is taken from `local`'s
 * mirror (what ekf_set_s / the appends gave it), as ekf_remove_landmarks takes its own: a signature written to the device behind the
 * library's back (ekf_diag_poke_device_signature) reaches the device copy of `h` but not its mirror. */
int32_t ekf_join_map(ekf_handle *h, ekf_handle *local, double signature_offset, int64_t *first_idx /* may be NULL */);
/* MAP EXTRACTION, the other direction: part of this map taken out into a handle of its own, on the device.  idx[0 .. m-1] are 0-based
 * landmarks of `h`, distinct, in ANY order; destination landmark k is source landmark idx[k] and keeps its signature.  `dst` is an existing
 * handle on the same cfg.device with any tile edge and storage kind and capacity_landmarks >= m; its WHOLE state (x, s, P) is replaced --
 * what it held, pending pairs and a recorded predict included, is dropped, as by ekf_load_lowrank_state.  Afterwards ekf_num_landmarks(dst)
 * is m and ekf_pending(dst) is 0.  Marginalisation in covariance form is a selection, so the call costs O(m^2) bytes whatever N is.
 * With strip = P(1:3, landmarks), theta = x(2) in degrees, k = 180/pi, c / s the cosine / sine of theta:
 *   EKF_FRAME_MAP    the joint Gaussian of the robot and the chosen landmarks as it is: x' = [r; l_idx[0]; ..], P' = P(sel, sel) with
 *                    sel = rows (robot, l_idx[0], .., l_idx[m-1]).  Nothing is computed: every value keeps its bits between stores of
 *                    one kind, a float store widens exactly into an F64 store, an F64 store is rounded once per tile entry into a float
 *                    store (x, P(1:3,1:3), the strip and the landmarks' own 2 x 2 blocks are F64 on every handle and stay exact).
 *   EKF_FRAME_ROBOT  the same landmarks relative to the robot, the robot's own uncertainty folded in to first order: the robot of dst is
 *                    (0, 0, 0) with P'(1:3, :) = 0; landmark k is m_k = (c dx + s dy, c dy - s dx), d = l_idx[k] - r(0:1): bit for bit
 *                    ekf_model_evaluate's EKF_MODEL_RELATIVE_XY hx at (r, l_idx[k]); and with that model's blocks
 *                    Hr_k = [-c -s m_k(1)/k; s -c -m_k(0)/k] on the robot and Hl = [c s; -s c] on the landmark
 *                      P'(k, a) = Hr_k P(1:3,1:3) Hr_a' + Hr_k strip(:, idx[a]) Hl' + Hl strip(:, idx[k])' Hr_a' + Hl P(l_idx[k], l_idx[a]) Hl'
 *                    (the four terms formed in this order and added left to right).  That is exactly the shape ekf_join_map expects of
 *                    a `local`: q = 0, PL_qq = 0, PL(q, .) = 0.  A landmark exactly on the robot is regular here (m_k = 0, a zero
 *                    heading column in Hr_k) and is not refused.
 * A landmark's own 2 x 2 block is taken from the live F64 diagonal copy in either frame.  m == 0 is allowed: a robot-only dst (in the
 * robot frame the zero pose with P = 0).  Two launches on dst's stream, counted on `h` under EKF_KERNEL_COMPACT; the index list is uploaded
 * once into a device buffer dst keeps (ekf_device_bytes of dst reports it).
 * A SYNCHRONISING call on BOTH handles, like ekf_join_map: `h` is settled and flushed as for every reader of P (a recorded predict carried
 * out, pending pairs applied, an asynchronous pass retired) and otherwise keeps every bit; `h`'s stream is drained before dst's stream
 * reads its buffers, and dst's stream is drained before the call returns.
 * Refused with nothing changed on either handle: h or dst NULL, h == dst, idx NULL with m > 0, m < 0, a landmark named twice, a frame that
 * is neither constant, either handle sharded (world > 1 or cfg.force_sharded), different cfg.device (EKF_ERR_INVALID_ARG); then, with both
 * measure loops settled, an index outside [0, N) (EKF_ERR_INDEX) and m > capacity_landmarks of dst (EKF_ERR_CAPACITY).  The message is in
 * ekf_last_error(h); a step that fails on dst is reported on `h`, quoting dst's own message.  The host's mirror of dst's signatures is taken
 * from `h`'s mirror, as ekf_join_map takes it. */
enum { EKF_FRAME_MAP = 0, EKF_FRAME_ROBOT = 1 };
int32_t ekf_extract_map(ekf_handle *h, const int64_t *idx, int64_t m, int32_t frame, ekf_handle *dst);
/* THE FRAME OF A MAP: the whole state of `h` moved into another frame, IN PLACE -- no second handle, the handle keeps its log and its
 * configuration.  N, s and the numbering stay.  k = 180/pi.
 *   EKF_FRAME_MAP    the map stays a map, moved by the rigid transform t = (tx, ty, phi), phi in degrees; Sigma is the column-major 3 x 3
 *                    covariance of t, independent of the state (NULL or all zeros: an exact transform).  With (s, c) the degree sine and
 *                    cosine of phi, Rot = [c -s; s c] and w(v) = Rot v:
 *                      r'   = t (+) r         bit for bit ekf_motion_evaluate's EKF_MOTION_POSE_DELTA at (xr = t, u = r): p' = t_xy + w(p),
 *                                             theta' = wrapTo360(phi + theta); F is that call's F, V = blockdiag(Rot, 1) its V
 *                      l_i' = t_xy + w(l_i)   bit for bit ekf_model_invert's EKF_MODEL_RELATIVE_XY at (t, l_i);
 *                                             A_i = its Gx = [1 0 -w_1(l_i)/k; 0 1 w_0(l_i)/k]
 *                    and P' = T P T' + A Sigma A', T = blockdiag(V, Rot, .., Rot), A = (F; A_1; ..; A_N), block by block, every sum left to
 *                    right and the rotation term first (strip = P(1:3, landmarks)):
 *                      P'(1:3,1:3) = V P(1:3,1:3) V' + F Sigma F'       strip'(:, i) = V strip(:, i) Rot' + F Sigma A_i'
 *                      P'(i, j)    = Rot P(i, j) Rot' + A_i Sigma A_j'
 *                    With Sigma NULL or zero the Sigma terms are not formed: the rotation alone, so t = 0 leaves every value equal as a
 *                    number and phi = 90 is a signed permutation of P's entries (the degree sine and cosine are exact there).  This is
 *                    ekf_join_map's J with the roles swapped: the transform plays the global robot, the whole map the local one.
 *   EKF_FRAME_ROBOT  the robot's own pose becomes the origin; t and Sigma must be NULL.  The result is bit for bit what
 *                    ekf_extract_map(h, [0 .. N-1], EKF_FRAME_ROBOT, dst) writes into a dst of the same tile edge and storage kind (x, s,
 *                    P, the diagonal copies; a float tile is widened to F64 and the result rounded once): the robot at (0, 0, 0) with
 *                    P'(1:3, :) = 0 -- the shape ekf_join_map expects of a `local`.  A landmark exactly on the robot is regular.
 * A landmark's own 2 x 2 block is formed from the live F64 diagonal copy and written to the copy and to the tile.  Two launches, counted
 * under EKF_KERNEL_COMPACT: the small part and the strip (one lane per column, into the other buffer set), and ONE IN-PLACE PASS over the
 * current tile store (a lane owns whole 2 x 2 blocks, 16-byte accesses; diagonal tiles stored whole, their halves equal bit for bit;
 * entries beyond 2 N stay zero; a second store of cfg.async_flush or of a removal is untouched).  N = 0 is allowed and launches no pass.
 * A SYNCHRONISING call, like ekf_constrain_landmarks: the measure loop settled, a recorded predict carried out, pending pairs applied, an
 * asynchronous pass retired; the stream is drained before the call returns and ekf_pending is 0.  Prefetched row-panels are dropped as for
 * a replaced covariance; an announced prefetch and the hint stay (the numbering did not change).
 * Refused with nothing changed and nothing flushed: h NULL, a frame that is neither constant, EKF_FRAME_MAP with t NULL or not finite, Sigma
 * not finite, not symmetric, or with a negative diagonal entry or a negative leading principal minor, EKF_FRAME_ROBOT with t or Sigma given,
 * a sharded handle (world > 1) (EKF_ERR_INVALID_ARG); a sharded correction between begin and finish (EKF_ERR_STATE). */
int32_t ekf_transform_map(ekf_handle *h, int32_t frame, const double t[3] /* EKF_FRAME_ROBOT: NULL */, const double Sigma[9] /* may be NULL */);
/* THE FACTORISATION OF P: is the matrix `h` carries still a covariance (float tiles, split arithmetic and thousands of downdates can leave
 * it indefinite), what is its log determinant (the entropy of the map), and what is the normalised estimation error squared (NEES) of x
 * against a reference state -- all three from ONE Cholesky factorisation P = L L' on the device, of exactly the matrix ekf_get_P would
 * report at that moment: the tiles (float tiles widened to F64), every landmark's own 2 x 2 block from the live F64 copy, rows at and
 * beyond 2 N left out.  All arithmetic and the factor are F64 for every storage kind.
 *   ELIMINATION ORDER: THE LANDMARK BLOCK FIRST, in ascending row order (index 3, 4, .. of x), THE ROBOT LAST (index 0, 1, 2).  So
 *   P(4:end, 4:end) = L L' is a factorisation of the landmark block alone, and the robot is a 3 x 3 tail: W = L^-1 P(4:end, 1:3),
 *   S_r = P(1:3, 1:3) - W' W, S_r = L_r L_r'.  A pivot is the value under the square root: it fails when it is <= 0 or not finite.
 *   Determinant, definiteness and d2 do not depend on the order; bad_index does: it is the FIRST pivot that fails IN THIS ORDER.
 * info (always written on EKF_OK):
 *   n           3 + 2 N
 *   definite    1: every pivot was > 0 and finite; 0: the factorisation stopped at bad_index
 *   bad_index   -1, or the index into x of the pivot that failed: 3 + r for row r of the landmark block, 0 .. 2 for the robot
 *   bad_pivot   that pivot's value (0.0, negative, NaN or infinite); 0.0 where definite
 *   logdet      log det P = 2 sum log L_ii, summed on the host in elimination order; NaN where not definite
 *   logdet_map  log det of the landmark block alone (0 for N = 0); NaN only where a LANDMARK pivot failed
 *   min_pivot, max_pivot   the smallest and the largest L_ii^2 over the pivots taken (NaN when none was taken)
 * A filter that starts at a known pose has P(1:3, 1:3) = 0: the call reports definite = 0, bad_index = 0, bad_pivot = 0.0 and a valid
 * logdet_map.  That is a result (EKF_OK), not an error.
 * ref: NULL, or nref (1 .. 8) reference states of 3 + 2 N finite entries each, one after another; then d2[q] = nu' P^-1 nu with
 * nu = x - ref_q, its heading entry (degrees) wrapped into (-180, 180]; NaN where P is not definite.  The solve rides the factorisation:
 * the strip and the nu's are right-hand sides of its forward substitution.
 * A right-looking blocked Cholesky in a scratch store the handle owns: F64 lower-triangle tiles of edge 64 whatever the handle's tile edge
 * is, 8 (n^2 / 2 + 12 n) bytes, allocated at the first call for the N of that call, grown when N has outgrown it, counted by
 * ekf_device_bytes and released by ekf_destroy.  Per tile column: the diagonal tile in LDS by one workgroup, the panel below it, the
 * trailing update on the F64 matrix cores; nothing waits in between and one readback ends the call.  A pivot that fails makes every later
 * launch return at once.  Launches count under EKF_KERNEL_COMPACT (load, right-hand sides, tail), EKF_KERNEL_GATHER (diagonal tiles and
 * panels, one count per column) and EKF_KERNEL_DOWNDATE (trailing updates).
 * A SYNCHRONISING, READ-ONLY call like ekf_nearest_landmarks: the measure loop settled, a recorded predict carried out, pending pairs
 * applied, an asynchronous pass retired; ekf_pending is 0 afterwards, and x, s, P, the diagonal blocks and ekf_P_digest are bit for bit
 * those of a handle that only flushed.  Nothing is kept between calls: every call factors.
 * Refused with nothing changed and nothing flushed: h or info NULL, ref given with nref outside 1 .. 8 or without d2, a handle with
 * world > 1 (sharding: every shard holds only its own tiles; a lone shard with cfg.force_sharded works) (EKF_ERR_INVALID_ARG); a sharded
 * correction between begin and finish (EKF_ERR_STATE); then, once N is exact, a ref entry that is not finite (EKF_ERR_INVALID_ARG);
 * EKF_ERR_HIP if the scratch store cannot be allocated, before anything is queued. */
typedef struct ekf_factor_info {
    int64_t n;
    int32_t definite;
    int64_t bad_index;
    double bad_pivot;
    double logdet;
    double logdet_map;
    double min_pivot, max_pivot;
} ekf_factor_info;
int32_t ekf_factor_map(ekf_handle *h, const double *ref /* nref x (3 + 2N), may be NULL */, int32_t nref, ekf_factor_info *info, double *d2 /* nref */);
/* DRAWS FROM THE POSTERIOR: k joint samples x + C xi of the Gaussian N(x, P) the handle carries, from ONE factorisation -- ekf_factor_map's,
 * with the factor applied to the caller's draws before it is forgotten.  xi is k rows of 3 + 2 N finite entries in x's order (robot
 * first), standard normal where samples of the posterior are wanted; THE LIBRARY GENERATES NO RANDOM NUMBERS.  Row q of out is x + C xi_q.
 *   C IS THE LOWER-TRIANGULAR CHOLESKY FACTOR OF P IN ekf_factor_map's ELIMINATION ORDER -- the landmark block first, rows ascending, the
 *   robot last -- mapped back to x's order, so C C' = P in x's order.  Unlike P, C depends on that order: in elimination order it is
 *   [L 0; W' L_r] with P(4:end, 4:end) = L L', W = L^-1 P(4:end, 1:3) and L_r L_r' = P(1:3, 1:3) - W' W, and a sample is
 *       out(4:end) = x(4:end) + L xi(4:end),      out(1:3) = x(1:3) + W' xi(4:end) + L_r xi(1:3).
 *   The unit vectors as draws return the columns of C.  The heading entry is x[2] plus its deviation, NOT wrapped.
 * info is filled as by ekf_factor_map(h, NULL, 0, ..), bit for bit, and may not be NULL.  A P THAT IS NOT DEFINITE IS A RESULT: EKF_OK,
 * info says where the factorisation stopped, and every entry of out is NaN.
 * Promised: (1) xi = 0 gives out = x, bit for bit, an entry -0.0 included (a deviation of zero is not added); (2) row q of out depends on xi_q alone -- the same draw gives the same bits alone, first, last or
 * in the middle of a batch of any k, and from call to call; (3) no atomics and no data-dependent order of summation.
 * The draws are taken 16 at a time (one chunk: the N-width of the F64 matrix instruction), a partial last chunk padded with zeros.  Per
 * chunk one streaming pass over the factor store forms L Xi on the F64 matrix cores, every tile read once, each tile row cut into
 * segments of 16 tiles with one workgroup and one partial block each; a second launch sums the partial blocks in ascending order, adds
 * x and forms the robot rows.  Chunks go up and come down through pinned staging of four chunks a direction, whatever k is; the host
 * waits only for a slot's own readback four chunks later.  There is one chunk of draws and one of samples on the device and one stream:
 * the copies and launches of successive chunks run one after another, the pinned slots only take the host's packing out of that line.  The chunks and the partial blocks (8 (N^2 / 32 + 80 N) bytes or so:
 * 31 MB at 10 000 landmarks beside the 1.6 GB factor store) are part of ekf_factor_map's scratch: allocated before anything is
 * flushed, counted by ekf_device_bytes, released with it.
 * The apply passes count under EKF_KERNEL_ASSOCIATE, the second launches under EKF_KERNEL_COMPACT, the factorisation as in ekf_factor_map.
 * Nothing is kept between calls: every call factors, so ask for all the draws of one state in one call.
 * SYNCHRONISING and READ-ONLY exactly as ekf_factor_map.  Refused with nothing changed and nothing flushed: h, xi, out or info NULL,
 * k < 1, a handle with world > 1 (a lone shard with cfg.force_sharded works) (EKF_ERR_INVALID_ARG); a sharded correction between begin
 * and finish (EKF_ERR_STATE); then, once N is exact, an xi entry that is not finite (EKF_ERR_INVALID_ARG); EKF_ERR_HIP if the scratch
 * cannot be allocated, before anything is queued.  A refusal leaves out untouched; an EKF_ERR_HIP once the launches have begun leaves
 * every entry of out NaN.  For a SUBSET of the landmarks: ekf_extract_map, then this call on the small handle. */
int32_t ekf_sample_map(ekf_handle *h, const double *xi /* k x (3 + 2N), one row per draw */, int64_t k /* >= 1 */, double *out /* k x (3 + 2N) */,
                       ekf_factor_info *info);
/* THE OTHER DIRECTION: C^-1 B AND P^-1 B for k right-hand sides the caller chooses, from ONE factorisation -- ekf_factor_map's again,
 * with the two triangular solves queued behind it before the factor is forgotten.  B is k rows of 3 + 2 N finite entries in x's order.
 * In ekf_factor_map's ELIMINATION ORDER (the landmark block m first, the robot r last) the factor is C = [L 0; W' L_r] and b = (b_m, b_r):
 *       u_m = L^-1 b_m,      u_r = L_r^-1 (b_r - W' u_m),      z_r = L_r^-T u_r,      z_m = L^-T (u_m - W z_r).
 *   EKF_SOLVE_HALF: row q of out is u = C^-1 b_q mapped back to x's order, out[0:3] = u_r and out[3:] = u_m: the WHITENED right-hand
 *     side.  |out_q|^2 = b_q' P^-1 b_q (a Mahalanobis distance where b is a difference of states), and C^-1 (sample_q - x) returns
 *     the draw xi_q of ekf_sample_map.  Like C, it depends on the elimination order.
 *   EKF_SOLVE_FULL: row q of out is z = P^-1 b_q in x's order: the information vector with b = x, columns of the information matrix
 *     with unit vectors.
 * Plain linear algebra: NO entry is wrapped; wrap the heading entry of a state difference before the call.
 * info is filled as by ekf_factor_map(h, NULL, 0, ..), bit for bit, and may not be NULL.  A P THAT IS NOT DEFINITE IS A RESULT: EKF_OK,
 * info says where the factorisation stopped, and every entry of out is NaN.
 * Promised: (1) row q of out depends on b_q alone -- the same right-hand side gives the same bits alone, first, last or in the middle
 * of a batch of any k, across chunk boundaries; (2) B = 0 gives out = 0 in every entry; (3) two calls on the same state give the same
 * bits: no atomics, no data-dependent order of summation.  Everything else is arithmetic in F64 with a forward error of a small
 * multiple of cond(P) 2^-53.
 * The right-hand sides are taken 16 at a time (ekf_sample_map's chunks, slots and events; the pinned staging does not grow with k).
 * Once a call the diagonal tiles of L are inverted in parallel (rows / 64 tiles of scratch, 10 MB at 10 000 landmarks); per chunk the
 * forward sweep is one launch per tile column, ascending -- every workgroup forms u_c = L_cc^-1 b_c for itself and then updates its
 * own tile row, b_I -= L_Ic u_c, on the F64 matrix cores --, one small launch takes the robot tail, and for EKF_SOLVE_FULL the backward
 * sweep mirrors the forward one over the tile rows, descending, with the transposed tiles.  STREAM ORDER IS THE ONLY ORDER between
 * workgroups: 2 rows / 64 + 1 launches a chunk (half of that for EKF_SOLVE_HALF), no flags in memory, no atomics.
 * The forward sweeps count under EKF_KERNEL_ASSOCIATE and the backward sweeps under EKF_KERNEL_APPEND (one bracket per chunk each),
 * the inverses and the tails under EKF_KERNEL_COMPACT, the factorisation as in ekf_factor_map.
 * Nothing is kept between calls: every call factors, so ask for all the right-hand sides of one state in one call.
 * SYNCHRONISING and READ-ONLY exactly as ekf_factor_map.  Refused with nothing changed and nothing flushed: h, B, out or info NULL,
 * k < 1, a form that is neither constant, a handle with world > 1 (a lone shard with cfg.force_sharded works) (EKF_ERR_INVALID_ARG);
 * a sharded correction between begin and finish (EKF_ERR_STATE); then, once N is exact, a B entry that is not finite
 * (EKF_ERR_INVALID_ARG); EKF_ERR_HIP if the scratch cannot be allocated, before anything is queued.  A refusal leaves out untouched;
 * an EKF_ERR_HIP once the launches have begun leaves every entry of out NaN. */
enum { EKF_SOLVE_FULL = 0, EKF_SOLVE_HALF = 1 };
int32_t ekf_solve_map(ekf_handle *h, int32_t form, const double *B /* k x (3 + 2N), one row per right-hand side, x's order */,
                      int64_t k /* >= 1 */, double *out /* k x (3 + 2N) */, ekf_factor_info *info);
/* THE PLAIN PRODUCT P B for k vectors the caller chooses, with NO factorisation: one read-only pass over the handle's own tile store per
 * 16 vectors.  B is k rows of 3 + 2 N finite entries in x's order; row q of out is P b_q in x's order.  What it is for: the covariance
 * A P A' of linear functions of the map (a centroid, the vector between two landmarks, a path length), cross-covariance blocks between
 * arbitrary landmark sets (unit vectors), the residual P z - b of an ekf_solve_map answer, P H' for an observation row that touches many
 * landmarks.
 * WHICH P: exactly what ekf_get_P reports at that moment -- float tiles widened to F64, every landmark's own 2 x 2 block from the live F64
 * copies, every other entry of the landmark block the canonical lower-triangle entry (within diagonal tiles too), the robot block from
 * Prr and the strip.  Plain linear algebra: NO entry is wrapped, and all arithmetic is F64 for every storage kind.  Rows and columns at
 * or beyond 2 N never contribute, whatever the store holds below the map (they are masked by selection, not multiplied by zero).
 * Promised: (1) row q of out depends on b_q alone -- the same vector gives the same bits alone, first, last or in the middle of a batch
 * of any k, across chunk boundaries and from call to call; (2) B = 0 gives 0 in every entry; (3) the unit vector e_j returns column j
 * of ekf_get_P, equal entry for entry as numbers (the sign of a zero is not promised); (4) no atomics and no data-dependent order of
 * summation.  Each entry is a sum of 3 + 2 N products in a fixed order: |out - P b|_i <= 2 n 2^-53 (|P| |b|)_i.
 * The vectors are taken 16 at a time; per chunk k_multiply_tiles makes one pass over the tile store on the F64 matrix cores -- every
 * stored tile T_IJ is used twice by the workgroup that holds it, as T_IJ B_J and as T_IJ' B_I --, k_multiply_sum adds the partial blocks
 * and the strip's part in a fixed order, and k_multiply_robot forms the robot rows.  The tile passes count under EKF_KERNEL_ASSOCIATE, the sums under EKF_KERNEL_COMPACT.
 * The scratch is the call's own (a chunk in, a chunk out, the partial blocks -- about an eighth of the tile store's F64 bytes at edge
 * 128 -- and four pinned chunks a direction whatever k is): allocated at the first call, grown when N has outgrown it, counted by
 * ekf_device_bytes, released by ekf_destroy.  ekf_factor_map's factor store is not allocated.  N = 0: out = Prr b.
 * SYNCHRONISING and READ-ONLY exactly as ekf_nearest_landmarks and ekf_factor_map: a recorded predict is carried out, pending pairs
 * are applied, an asynchronous pass is retired (ekf_pending is 0 afterwards); x, s, P and ekf_P_digest are bit for bit those of a
 * handle that only flushed; nothing is logged.  Refused with nothing changed and nothing flushed, in ekf_solve_map's order: h, B or out
 * NULL, k < 1, a handle with world > 1 (a lone shard with cfg.force_sharded works) (EKF_ERR_INVALID_ARG); a sharded correction between
 * begin and finish (EKF_ERR_STATE); then, once N is exact, a B entry that is not finite (EKF_ERR_INVALID_ARG); EKF_ERR_HIP if the
 * scratch cannot be allocated, before anything is queued.  A refusal leaves out untouched; an EKF_ERR_HIP once the launches have begun
 * leaves every entry of out NaN. */
int32_t ekf_multiply_map(ekf_handle *h, const double *B /* k x (3 + 2N), one row per vector, x's order */,
                         int64_t k /* >= 1 */, double *out /* k x (3 + 2N) */);
/* A LINEAR OBSERVATION WITH A DENSE H: "H x = z +- R" for k <= EKF_DENSE_MAX rows of 3 + 2 N finite entries in x's order, every row free to
 * touch every landmark -- the fix of a group's centroid, displacement constraints between several landmarks applied jointly, conditioning
 * on landmarks whose positions became known (R = 0), a loop closure delivered as a linear factor.  Exact, no linearisation:
 *     G = P H'      S = H G + R      nu = z - H x  (a row flagged in wrap_deg wrapped into (-180, 180], as ekf_observe_linear's)
 * and, with L L' = S, W = L^-1 G' and y = L^-1 nu, the symmetric form of ekf_observe_model_joint, with no back substitution:
 *     d2 = |y|^2        x' = x + W' y        P' = P - W' W.
 * The heading is not re-wrapped afterwards.  res (required; rows = k), nu (k) and S (k x k, column-major, symmetric as read):
 *   EKF_LINEAR_APPLIED    d2 <= gate (+inf: no gate): the update above ran.
 *   EKF_LINEAR_GATED      d2 > gate: EKF_OK, nothing changed beyond the flush.
 *   EKF_LINEAR_IRREGULAR  a pivot of S is not finite and positive (bad_row: the first such row, -1 otherwise): EKF_ERR_STATE, nothing
 *                         changed beyond the flush -- the record is read back and waited for before anything is written -- and the
 *                         handle goes on working.  Whether a singular S (R = 0 and two rows that say the same) is found so depends on
 *                         the rounding of that pivot: it is exactly what the device computed.
 * Neither refusal is counted by ekf_linear_rejections.  An odd k runs as k + 1 rows whose last is exactly empty (H = 0, R's row and
 * column 0 but a 1 on the diagonal, z = 0) -- ekf_observe_linear's convention for rows == 1 --, and leaves the bits of the call with that
 * row written out.
 * G is ONE chunk of ekf_multiply_map (its tile pass and its sums, unchanged, in its scratch; no download); k_dense_gram forms the lower
 * triangle of H G and H x over fixed segments of 128 rows, each in ascending row order, k_dense_factor adds them in ascending segment
 * order, factors S and forms d2; after the decision k_gather_dense forms W column by column and the pairs (rows 2 p, 2 p + 1 of W, twice)
 * go to ekf_merge_landmarks_batch's private F64 ring, slots 0 .. ceil(k / 2) - 1, and ONE F64-arithmetic pass applies them in place on
 * the main stream (float tiles are rounded once per entry, whatever cfg.pass_arith).  No atomics, no data-dependent order.  Afterwards
 * ekf_pending is 0 and ekf_downdate_kernel_name reports that pass with pairs = ceil(k / 2) (N = 0: no pass, the robot part alone).  The
 * call does not wait at its end and does not enter the pending ring.  The tile pass, k_dense_gram and k_dense_factor count under
 * EKF_KERNEL_ASSOCIATE, the sums under _COMPACT, the gather under _GATHER, the pass under _DOWNDATE.
 * A SYNCHRONISING EDIT on ekf_multiply_map's rungs.  Order of a call: h, H, z, R or res NULL, k outside 1 .. EKF_DENSE_MAX, an entry of z
 * or R that is not finite, R not exactly symmetric or with a negative diagonal entry, a NaN gate, an entry of H that is not finite
 * (EKF_ERR_INVALID_ARG; on a handle with cfg.device_assoc == 4 and rows still unsettled H is read once N is exact, behind the rungs);
 * world > 1 (EKF_ERR_INVALID_ARG; a lone cfg.force_sharded shard works); a sharded correction between begin and finish (EKF_ERR_STATE);
 * every allocation; the flush (a recorded predict carried out, the pending pairs applied, a pass in flight retired); the chunk, the
 * product, the two small launches, ONE readback and the decision; the gather; the pass.  R = 0 is allowed.
 * ekf_observe_dense_innovation is the same body stopped after the decision (no gate): res, nu and S bit for bit what ekf_observe_dense
 * would report; x, s, P and ekf_P_digest afterwards those of a handle that only flushed. */
#define EKF_DENSE_MAX 16          /* rows per call = one chunk of ekf_multiply_map */
typedef struct ekf_observe_dense_result {
    double  d2;
    int32_t rows;                  /* k */
    int32_t outcome;               /* EKF_LINEAR_APPLIED, _GATED or _IRREGULAR                 */
    int32_t bad_row;               /* the first row whose pivot is not finite and positive, or -1 */
} ekf_observe_dense_result;
int32_t ekf_observe_dense(ekf_handle *h, const double *H /* k x (3 + 2N), one row per observation row, x's order */,
                          int64_t k, const double *z /* k */, const double *R /* k x k column-major */,
                          const int32_t *wrap_deg /* k, may be NULL */, double gate,
                          ekf_observe_dense_result *res /* required */, double *nu /* k, may be NULL */, double *S /* k x k, may be NULL */);
int32_t ekf_observe_dense_innovation(ekf_handle *h, const double *H, int64_t k, const double *z, const double *R, const int32_t *wrap_deg,
                                     ekf_observe_dense_result *res, double *nu, double *S);
/* The step between the two: "WHICH landmark does this sighting belong to?", for a whole scan, under the conventions of ekf_observe_model.
 * ekf_associate keeps the reference's (signature-only by default, an unwrapped bearing, a range-scaled R) and cannot serve a filter
 * driven through the model calls.  For each of the m observations, d2(k, i) is, BIT FOR BIT, the d2 that ekf_model_innovation reports for
 * obs[k] with lm[0] = i on the same handle in the same state -- pending pairs, a recorded predict (carried out first) and every storage
 * kind included -- for EVERY landmark i, by two small launches: a one-landmark model's innovation reads nothing but the live F64 copies
 * (x, P(1:3,1:3), P(1:3, landmark), the landmark's own 2x2 block), which carry every pending pair and are replicated on every shard.
 *   best, second   the landmarks with the smallest and the second-smallest d2 (0-based; smaller d2 first, the lower index on equal d2);
 *                  -1 and d2 = +inf where there is none
 *   within_gate    landmarks with d2 <= obs[k].gate -- the gate feeds this count alone: a landmark ekf_model_innovation would call
 *                  EKF_LINEAR_GATED still has a d2 and is a candidate; gating is the caller's job (+inf counts every regular landmark)
 *   irregular      landmarks with no d2 (the target on the robot, a non-finite state, S not positive definite): never a candidate,
 *                  NaN in d2_all
 * d2_all, where not NULL, receives the whole m x N matrix, row-major: the hook for joint-compatibility or assignment solvers.
 * Each entry of obs: the model is EKF_MODEL_RANGE_BEARING, _RANGE, _BEARING or _RELATIVE_XY (EKF_MODEL_LANDMARK_RANGE has no robot block
 * and no single target); lm is {-1, -1}: the target is what is being searched for; anchor is ignored; z, R and gate as for
 * ekf_observe_model.  Mixed models in one scan are allowed.
 * The call changes nothing: no flush, ekf_pending and every bit of the state stay as found, a pass in flight (cfg.async_flush) is neither
 * waited for nor retired; it waits for the event behind its own readback alone.  A recorded predict is carried out first, by a launch
 * of its own.  The two launches are counted as one under EKF_KERNEL_ASSOCIATE.  SHARDED handles are supported: every shard computes the
 * same answer from replicated data, no exchange.  N = 0: best = second = -1, d2 = +inf, counts 0, no launch.
 * Refused in this order: h, obs or out NULL, m < 1 or m > EKF_ASSOCIATE_MODEL_MAX; per entry EKF_MODEL_LANDMARK_RANGE, lm != {-1, -1},
 * then what ekf_observe_model refuses of model, z, R and gate (EKF_ERR_INVALID_ARG); then, with the measure loop settled
 * (cfg.device_assoc = 4: N exact), a sharded correction between begin and finish (EKF_ERR_STATE). */
#define EKF_ASSOCIATE_MODEL_MAX 32
typedef struct ekf_model_match {
    int64_t best, second;        /* 0-based landmarks with the smallest and second-smallest d2; -1 = none          */
    double  d2_best, d2_second;  /* +inf where none                                                               */
    int64_t within_gate;         /* landmarks with d2 <= obs.gate                                                 */
    int64_t irregular;           /* landmarks with no d2: target on the robot, non-finite state, S not pos. def.  */
} ekf_model_match;
int32_t ekf_associate_model(ekf_handle *h, const ekf_model_obs *obs, int64_t m,
                            ekf_model_match *out /* m, required */, double *d2_all /* m x N row-major, may be NULL */);
/* The step between "score" and "apply": WHICH observation gets WHICH landmark when they compete -- the global-nearest-neighbour assignment
 * of a scan, decided on the device without the m x N matrix leaving it.
 *   d2            d2(k, i) is ekf_associate_model's, and so ekf_model_innovation's, bit for bit (the same function on the same operands):
 *                 pending pairs, a recorded predict (carried out first) and every storage kind included.
 *   match[k]      where not NULL: the record ekf_associate_model returns for the same scan, bit for bit.
 *   candidates    of observation k: the landmarks that have a d2 with d2 <= obs[k].gate, ordered by (d2, index) -- smaller d2 first, the
 *                 lower index on equal d2 -- of which the first EKF_ASSIGN_CANDIDATES are KEPT.  out[k].ncand is how many were kept
 *                 (match[k].within_gate still counts all of them); cand / cand_d2, where not NULL (both or neither), receive the kept
 *                 lists, m x EKF_ASSIGN_CANDIDATES row-major, with -1 / +inf in the slots behind ncand.
 *   assignment    among all injective partial maps a: observation -> landmark whose every pair (k, a_k) is a candidate of k -- over the
 *                 WHOLE map, not only the kept lists -- one that minimises  J = sum over the assigned d2(k, a_k) + sum over the left-out
 *                 obs[k].gate:  the gate is the price of leaving an observation out.  out[k].landmark is a_k (0-based) or -1 = left
 *                 out; out[k].d2 is that pair's d2, the same bits as in cand_d2, or +inf; *total, where not NULL, is J summed in scan
 *                 order.  Keeping EKF_ASSIGN_CANDIDATES >= m candidates per observation loses nothing: an observation assigned outside
 *                 its m cheapest landmarks can move to one of them that the other m - 1 leave free, at no higher cost.
 *   ties          which of several optimal assignments is returned is fixed by the implementation (deterministic: no atomics, nothing that
 *                 depends on the order in which lanes arrive); beyond that it is contract only as: the host build of the same source
 *                 (csrc/assign_math.h) returns the same one for the same lists.
 * Each entry of obs as for ekf_associate_model, except that the gate must be finite.  The call's place in a handle's order is
 * ekf_associate_model's: it changes and flushes nothing, ekf_pending and every bit of the state stay as found, it runs beside a pass in
 * flight and waits for the event behind its own readback alone; a recorded predict is carried out first.  Three launches, counted as one
 * under EKF_KERNEL_ASSOCIATE.  SHARDED handles are supported: every shard computes the same answer from replicated data, no exchange.
 * N = 0: every observation left out, ncand 0, the lists empty, total = sum of the gates, no launch.
 * Refused in this order: h, obs or out NULL, m < 1 or m > EKF_ASSIGN_MODEL_MAX; per entry what ekf_associate_model refuses; cand without
 * cand_d2 or the reverse; a gate that is not finite (EKF_ERR_INVALID_ARG); then a sharded correction between begin and finish
 * (EKF_ERR_STATE). */
#define EKF_ASSIGN_MODEL_MAX   32   /* observations per scan (= EKF_ASSOCIATE_MODEL_MAX) */
#define EKF_ASSIGN_CANDIDATES  32   /* candidates kept per observation                    */
typedef struct ekf_model_assigned {
    int64_t landmark;            /* 0-based landmark the observation is assigned to; -1 = left out */
    double  d2;                  /* that pair's d2; +inf where left out                            */
    int64_t ncand;               /* candidates kept: min(within_gate, EKF_ASSIGN_CANDIDATES)       */
    int64_t reserved;            /* 0                                                              */
} ekf_model_assigned;
int32_t ekf_assign_model(ekf_handle *h, const ekf_model_obs *obs, int64_t m,
                         ekf_model_assigned *out        /* m */,
                         ekf_model_match    *match      /* m, or NULL */,
                         int64_t            *cand       /* m x EKF_ASSIGN_CANDIDATES row-major, or NULL */,
                         double             *cand_d2    /* same shape, or NULL (both or neither) */,
                         double             *total      /* or NULL */);
/* "Decide" and "apply" with NO host wait between them.  After ekf_assign_model the host reads out[k].landmark and only then can it name the
 * target of each ekf_observe_model: the device idles for that round trip once per scan.  ekf_observe_model_assigned queues both: the three
 * launches of the assignment, then, for k = 0 .. m - 1 in scan order, ONE update-step whose launch reads out[k].landmark ON THE DEVICE:
 *   assigned    ekf_observe_model's update-step for obs[k] at that landmark: relinearised at the then-live state (which carries the steps
 *               before it), gated by obs[k].gate, the same launch shape, one pair into the pending ring.
 *   left out    (-1) a finite no-op as a gated step is: a zero pair takes the ring slot and the state is copied.  Its record says outcome
 *               EKF_LINEAR_UNASSIGNED, d2 NaN, S and nu zero, and ekf_linear_rejections does NOT count it.  Irregular and gated steps of
 *               assigned observations are counted as ekf_observe_model counts them.
 * THE REFERENCE SEQUENCE.  On the same state the call leaves, bit for bit, the x, s, P (ekf_get_P) and ekf_pending that this leaves:
 *     ekf_assign_model(obs, m, out, ...);  then for k in scan order
 *         out[k].landmark >= 0:  ekf_observe_model(obs[k] with lm[0] = out[k].landmark, NULL)
 *         otherwise:             ekf_observe_model(obs[k] with lm[0] = 0 and gate = -1, NULL)       (a step that cannot apply)
 * on every storage kind and batch size; on F64 tiles it also equals, after ekf_flush, the sequence with the left-out entries omitted.
 * obs and m as for ekf_assign_model: 1 <= m <= EKF_ASSIGN_MODEL_MAX, models 1-4, lm = {-1, -1}, every gate finite -- it is both the price
 * of leaving the observation out and the gate of its step.
 * The call's place in a handle's order is ekf_observe_model's: unsharded, the measure loop settled, a recorded predict carried out first; it
 * waits for nothing and flushes nothing.  ekf_pending grows by m; the batch and cfg.async_flush bookkeeping runs after every step as after
 * every update-step, so a scan may cross a batch boundary and a pass over P may start in the middle of it.  The assignment counts as one
 * launch under EKF_KERNEL_ASSOCIATE, the steps as m under EKF_KERNEL_GATHER.  Behind the last step ONE asynchronous copy brings the scan's
 * result into pinned memory of the handle's own, with an event behind it.  N = 0: no launch, nothing changes (ekf_pending too), and the
 * result says every observation is left out, ncand 0, total = the sum of the gates.
 * Refused with every bit of the state and ekf_pending as found, in this order: ekf_assign_model's refusals (h or obs NULL, m out of range,
 * per entry what ekf_associate_model refuses, a gate that is not finite: EKF_ERR_INVALID_ARG; a sharded correction between begin and
 * finish: EKF_ERR_STATE), then ekf_observe_model's for a handle with world > 1 (EKF_ERR_INVALID_ARG).
 * ekf_assigned_scan_result waits for the event of the LATEST scan alone -- a pass in flight is not waited for -- and reports it: *m its size,
 * out[k] and *total what ekf_assign_model would have returned for that scan at the state it saw, bit for bit; res[k] the nu, S, d2 and
 * outcome of step k, for an assigned k what ekf_observe_model(..., res) reports.  Every pointer may be NULL.  A later scan replaces an
 * earlier scan's result.  Outcomes are data: an irregular step does not make this call fail.  Before any scan: EKF_ERR_STATE. */
int32_t ekf_observe_model_assigned(ekf_handle *h, const ekf_model_obs *obs, int64_t m);
int32_t ekf_assigned_scan_result(ekf_handle *h, int64_t *m /* or NULL */, ekf_model_assigned *out /* m, or NULL */,
                                 ekf_linear_result *res /* m, or NULL */, double *total /* or NULL */);
/* A scan judged AS A WHOLE: the joint compatibility of its pairings.  ekf_associate_model scores every observation against every landmark
 * one at a time; where the pose is uncertain and the map locally tight several landmarks pass an observation's gate, and only a JOINT test
 * uses that all innovations of a scan share the robot's error.  A hypothesis pairs observation k with landmark hyp[i * m + k] (0-based) or
 * leaves it out (-1); with H_k and nu_k exactly as ekf_observe_model forms them for obs[k] at that landmark -- on the device, at the live x,
 * bearings wrapped -- the paired rows are stacked:
 *     S = H P H' + blockdiag(R_k),   d2 = nu' S^-1 nu   (Cholesky and a forward substitution in F64)
 * A one-row model enters as the pair with the exactly empty second row (S_kk = [[s, 0], [0, 1]], nu_1 = 0): it adds nothing to d2 and 1 to
 * dof.  Entries left out occupy no rows.  Each diagonal block S_kk and nu_k are ekf_model_innovation's for that pair, bit for bit.
 *   d2_prefix[i * m + k]   the joint d2 of the pairings among observations 0 .. k: 0 before the first pairing, repeated over entries left
 *                          out -- what a branch and bound needs at depth k.  It depends on those pairings alone, with the same bits
 *                          whatever follows them.
 *   nu, S                  by SCAN index: an entry left out has zero rows in nu, the identity on S's diagonal and zeros elsewhere.
 * A pairing is IRREGULAR where its target lies on the robot or its state is not finite, or where the Cholesky pivot of one of its rows is
 * not finite and positive.  For the first such pairing of a hypothesis: outcome = EKF_LINEAR_IRREGULAR, first_irregular = its scan index, d2
 * and every prefix from there on are NaN, the prefixes before it are what they would be without it.  Irregular hypotheses do not fail the
 * call.  A hypothesis with no pairing is legal: d2 = 0, dof = 0, regular.
 * obs: entries as ekf_associate_model takes them (models 1-4, lm = {-1, -1}, the anchor ignored); the gate is ignored: testing d2 against
 * chi2(dof) is the caller's job.
 * The call changes nothing: no flush, ekf_pending and every bit of the state stay as found; the cross blocks P(l_a, l_b) are read from the
 * current tile store patched with the pending pairs, beside a pass in flight (cfg.async_flush), as ekf_linear_innovation reads; it waits
 * for the event behind its own readback alone.  A recorded predict is carried out first.  One launch, one workgroup per hypothesis,
 * counted under EKF_KERNEL_ASSOCIATE.
 * Refused in this order, with nothing done: h, obs, hyp or out NULL, m outside 1 .. EKF_JOINT_MAX, nh outside 1 .. EKF_JOINT_HYP_MAX, an
 * entry ekf_associate_model refuses, a hypothesis entry below -1, a landmark twice in one hypothesis (EKF_ERR_INVALID_ARG); then
 * ekf_observe_linear's rungs: world > 1 (EKF_ERR_INVALID_ARG: sharding -- the cross blocks live in other shards' tiles; a lone
 * cfg.force_sharded shard works), a sharded correction between begin and finish (EKF_ERR_STATE); then a landmark >= N (EKF_ERR_INDEX). */
#define EKF_JOINT_MAX      32      /* observations per scan (= EKF_ASSOCIATE_MODEL_MAX)        */
#define EKF_JOINT_HYP_MAX  256     /* hypotheses per call                                      */
typedef struct ekf_joint_result {
    double  d2;                    /* joint nu' S^-1 nu over all pairings; NaN where irregular */
    int32_t dof;                   /* real rows: 2 per two-row model, 1 per one-row model      */
    int32_t pairings;              /* entries of the hypothesis that are >= 0                  */
    int32_t outcome;               /* EKF_LINEAR_APPLIED (= regular) or EKF_LINEAR_IRREGULAR   */
    int32_t first_irregular;       /* scan index of the first pairing with no d2, else -1      */
} ekf_joint_result;
int32_t ekf_joint_innovation(ekf_handle *h, const ekf_model_obs *obs, int64_t m,
                             const int64_t *hyp /* nh x m row-major: 0-based landmark or -1 */, int64_t nh,
                             ekf_joint_result *out   /* nh, required */,
                             double *d2_prefix       /* nh x m, may be NULL */,
                             double *nu              /* nh x 2m, may be NULL */,
                             double *S               /* nh x (2m x 2m column-major), may be NULL */);
/* ... and SEARCHED: the joint-compatibility search that a caller otherwise walks with one ekf_assign_model call and one ekf_joint_innovation
 * call per scan entry, as launches queued on the device with no host wait between them and ONE readback at the end.
 *   candidates  entry k's are the first min(EKF_JOINT_SEARCH_CAND, ncand_k) landmarks of its ekf_assign_model candidate list (inside the
 *               entry's gate, ordered by (d2, index)), read on the device from the buffer ekf_assign_model's second launch leaves.
 *   levels      the scan indices 0 .. m-1 in order, from the empty hypothesis (d2 = 0, dof = 0).  At level k every alive hypothesis is
 *               extended by each candidate of entry k it has not used yet, in list order, then by "left out".  An entry without
 *               candidates extends every hypothesis by "left out" alone: nothing is tested (tested[k] = survived[k] = 0).
 *   test        an extension survives where d2 <= threshold[dof], d2 its joint d2 and dof its real row count (ekf_joint_result.dof's
 *               rule); NaN never survives.  "Left out" keeps its parent's d2 and dof and is tested like the rest.
 *   order       survivors by (pairings descending, d2 ascending, hypothesis ascending: entry by entry in scan order on the 0-based
 *               landmark, -1 for left out).  Where more than `beam` survive the first `beam` are kept and truncated is set; exactly
 *               `beam` survivors is no cut.
 *   winner      the first hypothesis in that order after the last level: there is always one, all entries left out.
 * Every d2 the search forms is, BIT FOR BIT, the d2_prefix ekf_joint_innovation reports for that hypothesis at that scan index on the same
 * state: a hypothesis's factor is its parent's with two rows appended, every entry seeing the right-looking factorisation's operations
 * in their order.  An extension whose new pairing is irregular (ekf_joint_innovation's rule) has no d2, does not survive and is counted in
 * `irregular`.
 * match / cand / cand_d2 are ekf_assign_model's for the same scan, the same bits (ekf_model_match.within_gate == 0 says an entry has no
 * candidate).  N == 0: no launch, the winner all -1, d2 = 0, nalive = 1, the lists empty as ekf_assign_model returns them.
 * The call's place in a handle's order is ekf_joint_innovation's: settled, a recorded predict carried out first, no flush, ekf_pending and
 * every bit of x, s and P as found, the cross blocks read patched with the pending pairs beside a pass in flight, and it waits for the
 * event behind its own readback alone.  Launches count under EKF_KERNEL_ASSOCIATE: the candidate part once, as ekf_assign_model's; then
 * the prepare launch and each level's two launches once each.  The search's scratch is allocated at the first call, kept, and reported by
 * ekf_device_bytes.
 * Refused in this order, with nothing done: ekf_assign_model's argument refusals in its order (res required where it requires out);
 * threshold NULL or an entry of threshold[0 .. 2m] NaN, infinite or negative; beam outside 1 .. EKF_JOINT_SEARCH_BEAM_MAX; alive_hyp
 * and alive_d2 not both given or both NULL (EKF_ERR_INVALID_ARG); then ekf_observe_linear's rungs as ekf_joint_innovation has them. */
#define EKF_JOINT_SEARCH_CAND      4
#define EKF_JOINT_SEARCH_BEAM_MAX  64
typedef struct ekf_joint_search_result {
    int64_t lm[EKF_JOINT_MAX];        /* the winner by scan index: 0-based landmark, -1 = left out (entries >= m: -1) */
    double  d2;  int32_t dof, pairings;
    int32_t truncated;                /* 1 where a level had more than `beam` survivors               */
    int32_t nalive;                   /* hypotheses alive after the last level (after the cut)        */
    int32_t irregular;                /* extensions that had no d2, over all levels                   */
    int32_t tested[EKF_JOINT_MAX];    /* by scan index: extensions formed at that level               */
    int32_t survived[EKF_JOINT_MAX];  /* ... that passed their threshold, before the cut              */
} ekf_joint_search_result;
int32_t ekf_joint_search(ekf_handle *h, const ekf_model_obs *obs, int64_t m,
                         const double *threshold /* 2m + 1, by dof; finite, >= 0 */, int32_t beam,
                         ekf_joint_search_result *res     /* required */,
                         ekf_model_match *match           /* m, or NULL: ekf_assign_model's records, the same bits */,
                         int64_t *cand, double *cand_d2   /* m x EKF_ASSIGN_CANDIDATES, both or neither: ekf_assign_model's lists */,
                         int64_t *alive_hyp               /* EKF_JOINT_SEARCH_BEAM_MAX x m, or NULL: the final beam in order, -1 behind nalive rows */,
                         double  *alive_d2                /* EKF_JOINT_SEARCH_BEAM_MAX, or NULL (NaN behind nalive) */);
/* ... and APPLIED as a whole: one hypothesis of ekf_joint_innovation as ONE joint update.  All np paired observations are linearised once, at
 * the live state, and stacked; with L L' = S (the Cholesky factor of the stacked S), W = L^-1 H P (2 np rows) and y = L^-1 nu
 *     x' = x + W' y        P' = P - W' W
 * the symmetric form, with no back substitution: its pairs are (K_p, G_p) = (rows 2p, 2p + 1 of W, twice).  Unlike np sequential
 * ekf_observe_model steps, which relinearise at the state the previous one left, the update that runs is the one whose d2 was tested, and it
 * does not depend on scan order; it costs two small launches and ONE pass over P whatever np is.
 * obs, m, lm: exactly one hypothesis of ekf_joint_innovation -- m in 1 .. EKF_JOINT_MAX, models 1-4, a one-row model as the pair with the
 * exactly empty second row, the per-entry gate and the anchor ignored, no landmark twice.  res (required), nu and S are bit for bit what
 * ekf_joint_innovation reports for that hypothesis on the flushed state (with F64 tiles also against a call made before the flush, which is
 * bit-exact there).  res->outcome:
 *   EKF_LINEAR_APPLIED    joint d2 <= gate (+inf: no gate): the update above ran.
 *   EKF_LINEAR_GATED      d2 > gate: EKF_OK, nothing changed beyond the flush.
 *   EKF_LINEAR_IRREGULAR  a pairing has no d2: EKF_ERR_STATE naming its scan index (res->first_irregular), nothing changed beyond the flush --
 *                         the record is read back and waited for before anything is written -- and the handle goes on working.
 * Neither is counted by ekf_linear_rejections: the decision is taken on the host.  No pairing at all (every lm[k] == -1): EKF_OK, applied,
 * d2 = 0, no launch of its own and no flush (the rungs below come first: a recorded predict is carried out).
 * The call does not enter the handle's pending ring.  It takes ekf_merge_landmarks_batch's route: the pending pairs are applied first (a
 * flush, which retires a pass in flight), its own np pairs go to that call's private F64 ring (EKF_MERGE_BATCH_MAX >= EKF_JOINT_MAX slots,
 * allocated at first use, counted by ekf_device_bytes), and one F64-arithmetic pass applies them in place on the main stream -- float tiles
 * are rounded once per entry, whatever cfg.pass_arith.  Afterwards ekf_pending is 0 and ekf_downdate_kernel_name reports that pass with
 * pairs = np.  The call does not wait at its end.  Launches count under EKF_KERNEL_ASSOCIATE, _GATHER and _DOWNDATE.
 * Order of a call: ekf_joint_innovation's argument refusals in its order (nh = 1), a NaN gate (EKF_ERR_INVALID_ARG); ekf_observe_linear's
 * rungs (world > 1: EKF_ERR_INVALID_ARG, a lone cfg.force_sharded shard works; a sharded correction between begin and finish:
 * EKF_ERR_STATE; a recorded predict carried out); a landmark >= N (EKF_ERR_INDEX); allocations; the flush; the factor launch, its readback
 * and the decision; the gather launch; the pass. */
int32_t ekf_observe_model_joint(ekf_handle *h, const ekf_model_obs *obs, int64_t m,
                                const int64_t *lm       /* m: 0-based landmark, or -1 = left out */,
                                double gate             /* apply only if joint d2 <= gate; +inf = none */,
                                ekf_joint_result *res   /* required */,
                                double *nu              /* 2m, may be NULL */,
                                double *S               /* 2m x 2m column-major, may be NULL */);
/* ... and RELINEARISED: the iterated joint update, Gauss-Newton on the MAP cost of the whole scan over the sub-state
 * xi = (x_r, l_0 .. l_{np-1}) (pairing p = the p-th paired entry in scan order; ns = 3 + 2 np <= EKF_JOINT_SUB_MAX entries) under its prior
 * covariance P_sub, up to `iterations` times (1 .. EKF_JOINT_ITER_MAX):
 *     xi_0 = x0;   H_i, nu_i = wrap(z - h(xi_i)) per pairing, S_i = H_i P_sub H_i' + blockdiag(R) from the PRIOR covariance;
 *     r_i = nu_i - H_i (x0 - xi_i)   (i = 0: nu_0 alone);   L_i L_i' = S_i, y_i = L_i^-1 r_i;
 *     xi_{i+1} = x0 + P_sub H_i' L_i^-T y_i;   step = max_k |xi_{i+1}[k] - xi_i[k]|;   stop after i = iterations - 1 or where step <= tol
 * (tol = 0: a step of exactly 0 counts as converged).  The update that is applied is the LAST linearisation's, over the whole state and by
 * ekf_observe_model_joint's two launches unchanged: x' = x0 + W' y_last, P' = P - W' W, W = L_last^-1 H_last P.  With iterations = 1 the state is
 * ekf_observe_model_joint's bit for bit.  Plain Gauss-Newton: no damping, no line search.
 * The GATE is read at the first linearisation; res, nu and S are the first linearisation's: ekf_joint_innovation's bits.  A first linearisation
 * that is irregular or gated behaves as in ekf_observe_model_joint (it->used = 0).  A LATER iterate with a pairing that is not posed or a
 * pivot that is not finite and positive makes the whole call EKF_LINEAR_IRREGULAR: EKF_ERR_STATE naming the scan index and the
 * linearisation (it->irregular_obs, it->irregular_at), nothing changed beyond the flush, and the handle goes on working.
 * it (may be NULL): used = the linearisations whose step was taken, converged = step <= tol, the last step, d2 of the last linearisation,
 * and x_sub = xi_used (ns entries, zeros behind them).  No pairing at all: the empty update, used = 0, converged = 1.
 * Order of a call: ekf_observe_model_joint's, with iterations outside 1 .. EKF_JOINT_ITER_MAX or a NaN or negative tol refused
 * (EKF_ERR_INVALID_ARG) after its argument refusals and before the rungs.  The iteration record's device buffer is allocated at first use
 * and counted by ekf_device_bytes.
 * ekf_joint_iterate is the loop the kernel runs, on the host (pure, no handle): x_sub (ns), P_sub (ns x ns column-major, its lower triangle
 * read), the np entries of obs (models 1-4; lm, anchor and gate ignored), all paired.  x_out / P_out receive x' and P' over the sub-state;
 * an irregular linearisation (it->irregular_at >= 0, the first included; irregular_obs = the entry) leaves them equal to the inputs. */
#define EKF_JOINT_ITER_MAX EKF_MODEL_ITER_MAX
#define EKF_JOINT_SUB_MAX  (3 + 2 * EKF_JOINT_MAX)
typedef struct ekf_joint_iter_result {
    int32_t used, converged;
    double  last_step;
    double  d2_last;
    int32_t irregular_at;          /* the linearisation that was irregular, or -1              */
    int32_t irregular_obs;         /* the scan index of its first irregular pairing, or -1     */
    int32_t ns, reserved;
    double  x_sub[EKF_JOINT_SUB_MAX];
} ekf_joint_iter_result;
int32_t ekf_observe_model_joint_iterated(ekf_handle *h, const ekf_model_obs *obs, int64_t m, const int64_t *lm, double gate,
                                         int32_t iterations, double tol, ekf_joint_result *res /* required */,
                                         ekf_joint_iter_result *it /* may be NULL */, double *nu /* 2m, may be NULL */,
                                         double *S /* 2m x 2m column-major, may be NULL */);
int32_t ekf_joint_iterate(const double *x_sub, const double *P_sub, const ekf_model_obs *obs, int64_t np, int32_t iterations, double tol,
                          ekf_joint_iter_result *it, double *x_out, double *P_out);
/* The MOTION step under the same conventions: "the robot moved by u through the model, and u has the covariance M".  ekf_predict keeps the
 * reference's step (F(1,3), F(2,3) at the pre-motion heading and without pi/180, Q = (W C) W' of rank one) and is consistent with none of
 * the calls above: a filter driven through ekf_observe_model / ekf_append_model moves here.  With p = x(0:2), theta = x(2) in degrees,
 * k = 180/pi, the step is x_r' = f(x_r, u), P' = F P F' + V M V' with F = df/dx_r = I + [0 0 F02; 0 0 F12; 0 0 0] (the identity over the map)
 * and V = df/du:
 *   TURN_DRIVE  u = (d, t): turn by t degrees, then drive d.    (s, c) = sincosd(theta + t)       p' = p + d (c, s)
 *               (F02, F12) = (-d s / k, d c / k)                V = [c F02; s F12; 0 1]            -- the reference's f: the same pose, bit for bit
 *   ARC         u = (d, t): an arc of length d that turns by t. a = t / (2k), g = sin a / a, g' = (a cos a - sin a) / a^2 (both from their
 *               series for |a| < 1/2: finite at t = 0, where the arc is the straight line), (s, c) = sincosd(theta + t / 2)
 *               p' = p + d g (c, s)      (F02, F12) = (-d g s / k, d g c / k)      V = [g c, d (g' c - g s) / (2k); g s, d (g' s + g c) / (2k); 0 1]
 *   POSE_DELTA  u = (dx, dy, t) in the robot frame.             (s, c) = sincosd(theta)            w = (c dx - s dy, s dx + c dy)   p' = p + w
 *               (F02, F12) = (-w_1 / k, w_0 / k)                V = [c -s 0; s c 0; 0 0 1]         -- with u = 0: additive noise M in the robot frame
 * and theta' = wrapTo360(theta + t) in all three, as ekf_predict forms it (so a sum of exactly 360 stays 360).  M is column-major 3 x 3; a
 * model with two inputs reads its leading 2 x 2 block, M[0], M[1], M[3], M[4], and u[0], u[1] alone.
 * A chain of m steps is carried out in order by ONE launch (counted under EKF_KERNEL_PREDICT) that reads and writes x, P(1:3,1:3) and
 * P(1:3, map) once -- bit for bit what m calls with one step leave.  The landmarks, the landmark block of P, its pending pairs and s are
 * not touched.  The call is EAGER (ekf_predict is recorded and carried out by whatever comes next; a recorded one is carried out first, by
 * a launch of its own), returns without waiting for the device, does not flush and leaves ekf_pending as it found it; beside a pass in
 * flight (cfg.async_flush) it does not wait for the pass.  ekf_get_Q reports the LAST step's V M V' afterwards.
 * SHARDED handles are supported: everything the launch reads and writes is replicated, so the same call on every shard needs no exchange.
 * Refused with nothing changed, in this order: h or steps NULL, m < 1 or m > EKF_PREDICT_MODEL_MAX; per step an unknown model,
 * reserved != 0, a non-finite entry of u in use, then an M (the part in use) that is not finite, not exactly symmetric, or has a negative
 * diagonal entry, a negative 2 x 2 principal minor or, with three inputs, a negative determinant (all EKF_ERR_INVALID_ARG); then, with the
 * measure loop settled, a sharded correction between begin and finish (EKF_ERR_STATE).
 * ekf_motion_evaluate is the function the kernel runs, on the host (pure, like ekf_model_evaluate): x_new, F and V (both column-major
 * 3 x 3) at the robot state xr; EKF_ERR_INVALID_ARG for a NULL argument or an unknown model. */
enum { EKF_MOTION_TURN_DRIVE = 1, EKF_MOTION_ARC = 2, EKF_MOTION_POSE_DELTA = 3 };
#define EKF_PREDICT_MODEL_MAX 32
typedef struct ekf_motion {
    int32_t model, reserved;   /* EKF_MOTION_*; reserved: 0                                                    */
    double  u[3];              /* the inputs; angles in degrees                                               */
    double  M[9];              /* column-major covariance of u                                                */
} ekf_motion;
int32_t ekf_predict_model(ekf_handle *h, const ekf_motion *steps, int64_t m);
int32_t ekf_motion_evaluate(int32_t model, const double xr[3], const double u[3], double x_new[3], double F[9], double V[9]);
/* Diagnostic -- a fault injector for tests of the device-resident measure loop's verification, of no use to a host: overwrites the DEVICE copy
 * of signature idx (0-based) and leaves the host mirror alone.  The next ekf_measure whose association involves that landmark then queues its
 * launches from a prediction the device contradicts; every launch stays inside the state (a correction falls back to the predicted landmark,
 * a predicted append appends), ekf_measure itself returns EKF_OK (it waits for nothing),
 * and the FIRST synchronising call afterwards (ekf_sync, any getter, ekf_flush ...) returns EKF_ERR_STATE once, with the decision and the
 * prediction in ekf_last_error: from there on the state is no longer the reference's -- reload it (ekf_set_x / _P / _s, a checkpoint). */
int32_t ekf_diag_poke_device_signature(ekf_handle *h, int64_t idx, double value);
/* Dense n x n column-major P.  set_P stores the lower triangle (P is a covariance: symmetric).  On a shard
 * (world > 1) get_P / get_P_block return NaN for landmark-block entries held by another shard. */
int32_t ekf_get_P(ekf_handle *h, double *P);
int32_t ekf_set_P(ekf_handle *h, const double *P, int64_t n);
/* P(r0:r0+nr-1, c0:c0+nc-1) into out (nr x nc column-major): what plot() reads (EKF_SLAM.m:180,205). */
int32_t ekf_get_P_block(ekf_handle *h, int64_t r0, int64_t c0, int64_t nr, int64_t nc, double *out);
/* Everything plot() reads of P in ONE call (EKF_SLAM.m:180 robotSigma, :205 landmarkSigma): out holds 4 * (N+1) doubles --
 * P(1:2,1:2), then the 2x2 diagonal block of landmark 1..N, each column-major.  NaN for blocks held by another shard. */
int32_t ekf_get_P_diag_blocks(ekf_handle *h, double *out /* 4*(N+1) */);
/* The 3x3 non-zero block of the last predict's Q (EKF_SLAM.m:43-44), column-major. */
int32_t ekf_get_Q(ekf_handle *h, double Q[9]);
/* Bulk state load used to start large benchmarks: sets N landmarks, x (3+2N), s (N) and
 * P = diag(d) + U U' with d (3+2N) > 0 and U ((3+2N) x k column-major), built tile by tile on the device. */
int32_t ekf_load_lowrank_state(ekf_handle *h, int64_t N, const double *x, const double *s,
                               const double *d, const double *U, int64_t k);
/* Order-independent digests of P computed on the device over the unique (lower-triangle) entries:
 * out[0] = trace, out[1] = sum of the lower triangle incl. diagonal, out[2] = sum of squares of it. */
int32_t ekf_P_digest(ekf_handle *h, double out[3]);
/* Bytes of HBM held by the handle (all buffers). */
int32_t ekf_device_bytes(ekf_handle *h, int64_t *bytes);

/* ---- checkpoint (the reference has none; its whole state is the four properties x, P, Q, s, EKF_SLAM.m:6-9) ----
 * Binary file: 64-byte header (magic "EKFSLAM2", N, tile, storage, world, rank), then x, s, the robot block, the
 * robot/landmark strip, the landmarks' live F64 diagonal blocks (3 doubles each) and this handle's tiles of the active
 * tile rows, bit for bit (pending pairs are flushed first).  Loading needs a handle with the same tile edge, storage type
 * and shard (rank/world) and capacity >= N; a sharded filter is one file per shard.  Files with the magic "EKFSLAM1"
 * (no diagonal-block section) are rejected with EKF_ERR_STATE and a message that says so: there is no migration. */
int32_t ekf_checkpoint_save(ekf_handle *h, const char *path);
int32_t ekf_checkpoint_load(ekf_handle *h, const char *path);

/* ---- measurement hooks ---- */
enum { EKF_KERNEL_DOWNDATE = 0, EKF_KERNEL_GATHER = 1, EKF_KERNEL_PREDICT = 2, EKF_KERNEL_ASSOCIATE = 3,
       EKF_KERNEL_APPEND = 4,
       EKF_KERNEL_ROWPANEL = 5,   /* sharded handles: the extraction of a correction's (or a prefetch's) row-panels into the send area */
       EKF_KERNEL_EXCHANGE = 6,   /* sharded handles with ekf_comm_init: the all-gather on the library's communicator */
       EKF_KERNEL_COMPACT = 7,    /* ekf_remove_landmarks: the compaction of the tile store (k_compact_tiles alone, not its device-to-device copy) */
       EKF_KERNEL_COUNT = 8 };
/* Bracket every launch of kernel `which` with HIP events on the handle's stream (on != 0; on > 512 also reserves
 * event pairs for that many launches between two reads, so that none is created inside a timed region) and read the
 * accumulated launch count and device time; reading synchronises the stream and resets the counters. */
int32_t ekf_kernel_timing_enable(ekf_handle *h, int32_t which, int32_t on);
int32_t ekf_kernel_timing_read(ekf_handle *h, int32_t which, int64_t *launches, double *total_ms);
/* Name of the kernel instance the LAST downdate / flush launch of this handle used, as the launcher chose it
 * (e.g. "k_downdate_w<double,128,4,false>", "k_flush_mfma<double,128,8>"), and the number of pending pairs it applied
 * (*pairs, may be NULL); "" before the first launch.  The string is owned by the handle. */
const char *ekf_downdate_kernel_name(const ekf_handle *h, int32_t *pairs);
/* Algorithmic bytes one launch of the downdate kernel moves at the current N: every unique entry of the
 * symmetric P read once and written once = w * n * (n+1), n = 3+2N. */
int32_t ekf_downdate_algorithmic_bytes(ekf_handle *h, int64_t *bytes);

#ifdef __cplusplus
}
#endif
#endif /* EKFSLAM_H */
