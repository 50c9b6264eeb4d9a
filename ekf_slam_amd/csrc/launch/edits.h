// Fragment of kernels.hip, the launchers of the map edits: landmark removal (compact.h), part of a map taken out into another handle (extract_map.h), a constraint between two landmarks and its
// chained form (constrain.h), a linear observation (linear_obs.h) and one through a model (model_obs.h), the joint innovation of a scan's pairings (joint.h) and their joint update (joint_update.h, joint_iter.h), the fused pass of a batch of merges (merge_pass.h), the candidate search (nearest.h).
#pragma once

namespace {
// A pass that writes `ntiles` whole destination tiles out of place, kBlock * kCompactRows 16-byte pieces per work item: the items per
// tile and the grid; false: the grid does not fit 31 bits
bool compact_grid(const TileMap &tm, int64_t ntiles, int storage, int &items, int64_t &grid) {
    const int64_t pieces = (int64_t)tm.T * tm.T / (storage == 0 ? 2 : 4);
    items = (int)cdiv(pieces, (int64_t)kBlock * kCompactRows);
    grid = ntiles * items;
    return grid <= 0x7fffffff;
}
}  // namespace

hipError_t launch_compact_tiles(const TileMap &tm, const void *src, void *dst, const int2 *work, int64_t ntiles, const int32_t *src_of,
                                int storage, hipStream_t s) {
    if (ntiles <= 0) return hipSuccess;
    if (src == dst) return hipErrorInvalidValue;                        // out of place only
    int items;
    int64_t grid;
    if (!compact_grid(tm, ntiles, storage, items, grid)) return hipErrorInvalidValue;
    return with_storage(storage, [&](auto ts) {
        using TS = decltype(ts);
        hipLaunchKernelGGL(k_compact_tiles<TS>, dim3((unsigned)grid), dim3(kBlock), 0, s, (const TS *)src, (TS *)dst, work, items, src_of, tm);
    });
}

hipError_t launch_compact_state(const DevState &st, int cur, const int32_t *src_of, int64_t N_old, double *s_out, hipStream_t s) {
    const int64_t grid = cdiv(N_old > 0 ? N_old : 1, kBlock);
    hipLaunchKernelGGL(k_compact_state, dim3((unsigned)grid), dim3(kBlock), 0, s, st, cur, src_of, N_old, s_out);
    return hipGetLastError();
}

hipError_t launch_extract_state(const DevState &dst, const DevState &src, const ExtractMapArgs &a, const int32_t *idx, hipStream_t s) {
    // the columns written inside the destination's strip (whole tiles: zero from 2 m on), the list there where a landmark is read
    if (a.m < 0 || a.cols != dst.tm.padded(2 * a.m) || a.cols > dst.ldm || (a.m > 0 && !idx) || (a.frame != 0 && a.frame != 1)) return hipErrorInvalidValue;
    const int64_t grid = cdiv(a.cols > 0 ? a.cols : 1, kBlock);
    hipLaunchKernelGGL(k_extract_state, dim3((unsigned)grid), dim3(kBlock), 0, s, dst, src, a, idx);
    return hipGetLastError();
}

hipError_t launch_extract_rows(const DevState &dst, const DevState &src, const ExtractMapArgs &a, const int32_t *idx, int storage, int src_storage,
                               hipStream_t s) {
    if (a.m < 1 || a.cols != dst.tm.padded(2 * a.m) || a.cols > dst.ldm || !idx || (a.frame != 0 && a.frame != 1) || dst.tm.world != 1 ||
        src.tm.world != 1 || dst.tiles == src.tiles)
        return hipErrorInvalidValue;
    const int64_t rows = a.cols / 2;                        // destination landmarks, the zero ones of the last tile row included
    const int64_t per_row = cdiv(rows, kBlock);             // workgroups per destination landmark: 256 column landmarks each
    const int64_t grid = rows * per_row;
    if (grid > 0x7fffffffll) return hipErrorInvalidValue;
    return with_storage(storage, [&](auto td) { with_storage(src_storage, [&](auto tsrc) {
        hipLaunchKernelGGL((k_extract_rows<decltype(td), decltype(tsrc)>), dim3((unsigned)grid), dim3(kBlock), 0, s, dst, src, a, idx, (int32_t)per_row);
    }); });
}

namespace {
bool transform_args_ok(const DevState &st, const TransformMapArgs &a) {
    return a.N >= 0 && a.cols == st.tm.padded(2 * a.N) && a.cols <= st.ldm && a.form >= 0 && a.form <= 2 && (a.cur == 0 || a.cur == 1);
}
}  // namespace

hipError_t launch_transform_state(const DevState &st, const TransformMapArgs &a, hipStream_t s) {
    if (!transform_args_ok(st, a)) return hipErrorInvalidValue;
    const int64_t grid = cdiv(a.cols > 0 ? a.cols : 1, kBlock);
    if (a.form == 0) hipLaunchKernelGGL(k_transform_state<0>, dim3((unsigned)grid), dim3(kBlock), 0, s, st, a);
    else if (a.form == 1) hipLaunchKernelGGL(k_transform_state<1>, dim3((unsigned)grid), dim3(kBlock), 0, s, st, a);
    else hipLaunchKernelGGL(k_transform_state<2>, dim3((unsigned)grid), dim3(kBlock), 0, s, st, a);
    return hipGetLastError();
}

hipError_t launch_transform_tiles(const DevState &st, const TransformMapArgs &a, const int2 *work, int64_t ntiles, int storage, hipStream_t s) {
    if (ntiles <= 0 || a.N <= 0) return hipSuccess;
    // the list is that of the active tile rows (every tile it names lies inside the store), every tile held here; a tile row holds whole
    // 16-byte pieces and a workgroup whole tile rows of them
    const int pieces_per_row = st.tm.T / (storage == 0 ? 2 : 4);
    if (!transform_args_ok(st, a) || !work || st.tm.world != 1 || ntiles != st.tm.row_base(a.cols >> st.tm.shift) || pieces_per_row < 1 ||
        kBlock % pieces_per_row != 0)
        return hipErrorInvalidValue;
    const int64_t units = (int64_t)(st.tm.T / 2) * pieces_per_row;
    const int items = (int)cdiv(units, (int64_t)kBlock * kTransformUnits);
    const int64_t grid = ntiles * items;
    if (grid > 0x7fffffffll) return hipErrorInvalidValue;
    return with_storage(storage, [&](auto ts) {
        using TS = decltype(ts);
        if (a.form == 0) hipLaunchKernelGGL((k_transform_tiles<TS, 0>), dim3((unsigned)grid), dim3(kBlock), 0, s, st, a, work, items);
        else if (a.form == 1) hipLaunchKernelGGL((k_transform_tiles<TS, 1>), dim3((unsigned)grid), dim3(kBlock), 0, s, st, a, work, items);
        else hipLaunchKernelGGL((k_transform_tiles<TS, 2>), dim3((unsigned)grid), dim3(kBlock), 0, s, st, a, work, items);
    });
}

hipError_t launch_merge_pass(const DevState &st, void *dst, const int2 *work, int64_t ntiles, const int32_t *src_of, int npairs,
                             int storage, hipStream_t s, char *kname) {
    if (ntiles <= 0) return hipSuccess;
    if (st.tiles == dst || !dst || !src_of || npairs < 0 || npairs > st.pcap || st.tm.world != 1) return hipErrorInvalidValue;      // out of place only
    int items;
    int64_t grid;
    if (!compact_grid(st.tm, ntiles, storage, items, grid)) return hipErrorInvalidValue;
    if (kname) snprintf(kname, 64, "k_merge_pass<%s,%d>", storage == 0 ? "double" : "float", st.tm.T);
    return with_storage(storage, [&](auto ts) {
        using TS = decltype(ts);
        hipLaunchKernelGGL(k_merge_pass<TS>, dim3((unsigned)grid), dim3(kBlock), 0, s, (const TS *)st.tiles, (TS *)dst, work, items, src_of,
                           (const double *)st.Kp, (const double *)st.Gp, st.pair_stride, npairs, st.tm);
    });
}

hipError_t launch_constrain_probe(const DevState &st, int cur, int64_t ai, int64_t aj, double *out, int storage, hipStream_t s) {
    if (!out || ai < 0 || aj < 0 || ((ai | aj) & 1) || ai == aj) return hipErrorInvalidValue;
    return with_storage(storage, [&](auto ts) {
        hipLaunchKernelGGL(k_constrain_probe<decltype(ts)>, dim3(1), dim3(64), 0, s, st, cur, ai, aj, out);
    });
}

namespace {
// two different landmarks inside the map, the padded block inside the strip, the pair's ring position inside the ring
bool constrain_args_ok(const DevState &st, const ConstrainArgs &a) {
    const bool rows_ok = a.ai >= 0 && a.aj >= 0 && a.ai + 1 < a.n_mm && a.aj + 1 < a.n_mm && (a.ai & 1) == 0 && (a.aj & 1) == 0 && a.ai != a.aj;
    return rows_ok && st.tm.padded(a.n_mm) <= st.ldm && a.npend >= 0 && a.npend < st.pcap;
}
unsigned constrain_grid(const DevState &st, const ConstrainArgs &a) { return (unsigned)cdiv(st.tm.padded(a.n_mm), kBlock); }
}  // namespace

hipError_t launch_gather_constrain(const DevState &st, const ConstrainArgs &a, int storage, hipStream_t s) {
    if (!constrain_args_ok(st, a)) return hipErrorInvalidValue;
    return with_storage(storage, [&](auto ts) {
        hipLaunchKernelGGL(k_gather_constrain<decltype(ts)>, dim3(constrain_grid(st, a)), dim3(kBlock), 0, s, st, a, (double *)nullptr);
    });
}

hipError_t launch_gather_constrain_chain(const DevState &st, const ConstrainArgs &a, double *rec, int storage, hipStream_t s) {
    if (!constrain_args_ok(st, a) || a.pstart < 0 || a.pstart >= st.pcap || !rec || st.Gp32 || st.tm.world != 1) return hipErrorInvalidValue;
    return with_storage(storage, [&](auto ts) {
        hipLaunchKernelGGL(k_gather_constrain<decltype(ts)>, dim3(constrain_grid(st, a)), dim3(kBlock), 0, s, st, a, rec);
    });
}

namespace {
// the landmarks that carry a block inside the map and different, the padded block inside the strip, the ring positions inside the ring
template <typename A>
bool linear_args_ok(const DevState &st, const A &a) {
    for (int b = 0; b < 2; ++b)
        if (a.a[b] != -1 && !(a.a[b] >= 0 && a.a[b] + 1 < a.n_mm && (a.a[b] & 1) == 0)) return false;
    if (a.a[0] >= 0 && a.a[0] == a.a[1]) return false;
    return a.n_mm >= 0 && st.tm.padded(a.n_mm) <= st.ldm && a.npend >= 0 && a.npend <= st.pcap && a.pstart >= 0 && a.pstart < st.pcap &&
           st.tm.world == 1;
}
// the landmark pattern of the model: the pair of model 5, at most the first one otherwise
bool model_args_ok(const ModelArgs &a) {
    if (a.model < 1 || a.model > 5) return false;
    return a.model == 5 ? (a.a[0] >= 0 && a.a[1] >= 0) : a.a[1] == -1;
}
// One launch of an update-step over the padded landmark block, 256 columns per workgroup (an empty map: workgroup 0 alone, for x_r and
// Prr), and of its probe (one wavefront).  kernel: a generic lambda that names the instance for a storage tag, `[](auto ts) { return
// k_gather_linear<decltype(ts)>; }`; ok: the caller's argument check.
template <typename K, typename A>
hipError_t launch_step(bool ok, K kernel, const DevState &st, const A &a, double *rec, int64_t *cnt, int storage, hipStream_t s) {
    if (!ok) return hipErrorInvalidValue;
    const int64_t grid = std::max<int64_t>(1, cdiv(st.tm.padded(a.n_mm), kBlock));
    return with_storage(storage, [&](auto ts) { hipLaunchKernelGGL(kernel(ts), dim3((unsigned)grid), dim3(kBlock), 0, s, st, a, rec, cnt); });
}
template <typename K, typename A>
hipError_t launch_step_probe(bool ok, K kernel, const DevState &st, const A &a, double *rec, int storage, hipStream_t s) {
    if (!ok) return hipErrorInvalidValue;
    return with_storage(storage, [&](auto ts) { hipLaunchKernelGGL(kernel(ts), dim3(1), dim3(64), 0, s, st, a, rec); });
}
}  // namespace

hipError_t launch_gather_linear(const DevState &st, const LinearArgs &a, double *rec, int64_t *cnt, int storage, hipStream_t s) {
    return launch_step(linear_args_ok(st, a) && a.npend < st.pcap && rec && cnt, [](auto ts) { return k_gather_linear<decltype(ts)>; }, st, a, rec, cnt, storage, s);
}

hipError_t launch_linear_probe(const DevState &st, const LinearArgs &a, double *rec, int storage, hipStream_t s) {
    return launch_step_probe(linear_args_ok(st, a) && rec, [](auto ts) { return k_linear_probe<decltype(ts)>; }, st, a, rec, storage, s);
}

hipError_t launch_gather_model(const DevState &st, const ModelArgs &a, double *rec, int64_t *cnt, int storage, hipStream_t s) {
    return launch_step(linear_args_ok(st, a) && model_args_ok(a) && a.npend < st.pcap && rec && cnt, [](auto ts) { return k_gather_model<decltype(ts)>; }, st, a, rec, cnt,
                       storage, s);
}

hipError_t launch_model_probe(const DevState &st, const ModelArgs &a, double *rec, int storage, hipStream_t s) {
    return launch_step_probe(linear_args_ok(st, a) && model_args_ok(a) && rec, [](auto ts) { return k_model_probe<decltype(ts)>; }, st, a, rec, storage, s);
}

// the step whose landmark the device reads: launch_step's grid (it depends on n_mm alone), with the slot as one more argument; the host
// names no landmark (the kernel checks the one it reads against n_mm) and a model that takes one target
hipError_t launch_gather_model_assigned(const DevState &st, const AssignedModelArgs &a, const AssignedRecord *slot, double *rec, int64_t *cnt,
                                        int storage, hipStream_t s) {
    if (!(linear_args_ok(st, a) && a.model >= 1 && a.model <= 4 && a.a[0] == -1 && a.a[1] == -1 && a.skipped == 0 && a.npend < st.pcap && slot &&
          rec && cnt))
        return hipErrorInvalidValue;
    const int64_t grid = std::max<int64_t>(1, cdiv(st.tm.padded(a.n_mm), kBlock));
    return with_storage(storage, [&](auto ts) {
        hipLaunchKernelGGL(k_gather_model_assigned<decltype(ts)>, dim3((unsigned)grid), dim3(kBlock), 0, s, st, a, slot, rec, cnt);
    });
}

// the relinearised step: launch_step's grid and launch_step_probe's wavefront, with the iteration record as one more argument
hipError_t launch_gather_model_iter(const DevState &st, const IterModelArgs &a, double *rec, int64_t *cnt, double *itrec, int storage, hipStream_t s) {
    if (!(linear_args_ok(st, a) && model_args_ok(a) && a.npend < st.pcap && rec && cnt && itrec) || a.iterations < 1 ||
        a.iterations > ekfm::kModelIterMax || !(a.tol >= 0.0))
        return hipErrorInvalidValue;
    const int64_t grid = std::max<int64_t>(1, cdiv(st.tm.padded(a.n_mm), kBlock));
    return with_storage(storage, [&](auto ts) {
        hipLaunchKernelGGL(k_gather_model_iter<decltype(ts)>, dim3((unsigned)grid), dim3(kBlock), 0, s, st, a, rec, cnt, itrec);
    });
}

hipError_t launch_model_iter_probe(const DevState &st, const IterModelArgs &a, double *rec, double *itrec, int storage, hipStream_t s) {
    if (!(linear_args_ok(st, a) && model_args_ok(a) && rec && itrec) || a.iterations < 1 || a.iterations > ekfm::kModelIterMax || !(a.tol >= 0.0))
        return hipErrorInvalidValue;
    return with_storage(storage, [&](auto ts) { hipLaunchKernelGGL(k_model_iter_probe<decltype(ts)>, dim3(1), dim3(64), 0, s, st, a, rec, itrec); });
}

hipError_t launch_joint_innovation(const DevState &st, const JointArgs &a, const int64_t *hyp, int nh, JointRecord *out, double *d2_prefix,
                                   double *nu, double *S, int storage, hipStream_t s) {
    // the scan and the hypotheses inside their limits, the map inside the strip, the ring window inside the ring, every tile held here
    if (a.m < 1 || a.m > kJointMax || nh < 1 || nh > kJointHypMax || !hyp || !out || a.N < 0 || 2 * a.N > st.ldm || a.npend < 0 ||
        a.npend > st.pcap || a.pstart < 0 || a.pstart >= st.pcap || st.tm.world != 1)
        return hipErrorInvalidValue;
    return with_storage(storage, [&](auto ts) {
        hipLaunchKernelGGL(k_joint_innovation<decltype(ts)>, dim3((unsigned)nh), dim3(kJointBlock), 0, s, st, a, hyp, out, d2_prefix, nu, S);
    });
}

hipError_t launch_joint_search_prepare(const DevState &st, const JointArgs &a, const ekfm::CandList *sel, const int64_t *match,
                                       JointSearchStore *store, JointSearchOut *out, hipStream_t s) {
    if (a.m < 1 || a.m > kJointMax || !sel || !match || !store || !out || a.N < 1 || 2 * a.N > st.ldm) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_joint_search_prepare, dim3((unsigned)a.m), dim3(kJointSearchBlock), 0, s, st, a, sel, match, store, out);
    return hipGetLastError();
}

hipError_t launch_joint_search_level(const DevState &st, const JointSearchArgs &a, const JointSearchLevelArgs &la, const ekfm::CandList *sel,
                                     JointSearchStore *store, JointSearchOut *out, int which, int storage, hipStream_t s) {
    // launch_joint_innovation's checks, the level inside the scan, the beam inside the store
    if (a.m < 1 || a.m > kJointMax || a.level < 0 || a.level >= a.m || la.m != a.m || la.level != a.level || la.beam < 1 ||
        la.beam > kJointSearchBeam || !sel || !store || !out || a.N < 1 || 2 * a.N > st.ldm || a.npend < 0 || a.npend > st.pcap || a.pstart < 0 ||
        a.pstart >= st.pcap || st.tm.world != 1)
        return hipErrorInvalidValue;
    return with_storage(storage, [&](auto ts) {
        if (which != 2)
            hipLaunchKernelGGL(k_joint_search_extend<decltype(ts)>, dim3(kJointSearchExt), dim3(kJointSearchBlock), 0, s, st, a, sel, store);
        if (which != 1)
            hipLaunchKernelGGL(k_joint_search_select, dim3(1), dim3(kJointSearchSelectBlock), 0, s, la, sel, store, out);
    });
}

hipError_t launch_joint_factor(const DevState &st, const JointArgs &a, const int64_t *hyp, JointBlock *blk, JointRecord *out, double *nu, double *S,
                               int storage, hipStream_t s) {
    // launch_joint_innovation's checks for one hypothesis on a flushed state
    if (a.m < 1 || a.m > kJointMax || !hyp || !blk || !out || a.N < 0 || 2 * a.N > st.ldm || a.npend != 0 || a.pstart < 0 || a.pstart >= st.pcap ||
        st.tm.world != 1)
        return hipErrorInvalidValue;
    return with_storage(storage, [&](auto ts) {
        hipLaunchKernelGGL(k_joint_factor<decltype(ts)>, dim3(1), dim3(kJointBlock), 0, s, st, a, hyp, blk, out, nu, S);
    });
}

hipError_t launch_joint_factor_iter(const DevState &st, const JointArgs &a, const JointIterArgs &ia, const int64_t *hyp, JointBlock *blk,
                                    JointRecord *out, double *itrec, double *nu, double *S, int storage, hipStream_t s) {
    // launch_joint_factor's checks, and the loop's controls inside their limits
    if (a.m < 1 || a.m > kJointMax || !hyp || !blk || !out || !itrec || a.N < 0 || 2 * a.N > st.ldm || a.npend != 0 || a.pstart < 0 ||
        a.pstart >= st.pcap || st.tm.world != 1 || ia.iterations < 1 || ia.iterations > kJointIterMax || !(ia.tol >= 0.0) || ia.gate != ia.gate)
        return hipErrorInvalidValue;
    return with_storage(storage, [&](auto ts) {
        hipLaunchKernelGGL(k_joint_factor_iter<decltype(ts)>, dim3(1), dim3(kJointBlock), 0, s, st, a, ia, hyp, blk, out, itrec, nu, S);
    });
}

hipError_t launch_gather_joint(const DevState &st, const JointUpdateArgs &a, const JointBlock *blk, int storage, hipStream_t s) {
    // the pairs inside the private F64 ring, the padded block inside the strip, every tile held here
    if (!blk || a.np < 1 || a.np > kJointMax || a.np > st.pcap || a.n_mm < 2 || (a.n_mm & 1) || st.tm.padded(a.n_mm) > st.ldm || st.Gp32 || st.Kp32 ||
        !st.Gp || !st.Kp || st.tm.world != 1)
        return hipErrorInvalidValue;
    const unsigned grid = (unsigned)cdiv(st.tm.padded(a.n_mm), kBlock);
    return with_storage(storage, [&](auto ts) {
        using TS = decltype(ts);
        if (a.np <= 8) hipLaunchKernelGGL((k_gather_joint<TS, 8>), dim3(grid), dim3(kBlock), 0, s, st, a, blk);
        else hipLaunchKernelGGL((k_gather_joint<TS, 32>), dim3(grid), dim3(kBlock), 0, s, st, a, blk);
    });
}

// ---- a linear observation with a dense H (dense_obs.h), behind launch_multiply_map's two stages on the same chunk ----
namespace {
bool dense_args_ok(const DevState &st, const DenseArgs &a) {
    // every row the kernels read lies inside the chunks (ld) and inside the strip; the robot's three entries lie behind the landmark rows
    return a.b && a.y && a.part && a.kk >= 2 && a.kk <= kDenseMax && !(a.kk & 1) && a.n_mm >= 0 && !(a.n_mm & 1) && a.n_mm <= st.ldm &&
           a.rows == st.tm.padded(a.n_mm) && a.ld >= a.rows + 3 && (a.cur == 0 || a.cur == 1) && st.tm.world == 1;
}
}  // namespace
int64_t dense_partial_doubles(int64_t n_mm) { return cdiv(n_mm, (int64_t)kDenseSegment) * kDensePartial; }

hipError_t launch_dense_gram(const DevState &st, const DenseArgs &a, hipStream_t s) {
    if (!dense_args_ok(st, a)) return hipErrorInvalidValue;
    const int64_t grid = cdiv(a.n_mm, (int64_t)kDenseSegment);
    if (grid > 0x7fffffffll) return hipErrorInvalidValue;
    if (grid == 0) return hipSuccess;
    hipLaunchKernelGGL(k_dense_gram, dim3((unsigned)grid), dim3(kDenseBlock), 0, s, st, a);
    return hipGetLastError();
}

hipError_t launch_dense_factor(const DevState &st, const DenseArgs &a, const DenseSmall &sm, DenseOut *out, DenseBlock *blk, hipStream_t s) {
    if (!dense_args_ok(st, a) || !out || !blk) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_dense_factor, dim3(1), dim3(kDenseFactorBlock), 0, s, st, a, sm, out, blk);
    return hipGetLastError();
}

hipError_t launch_gather_dense(const DevState &st, const DenseArgs &a, const DenseBlock *blk, hipStream_t s) {
    // launch_gather_joint's checks: the pairs inside the private F64 ring, the padded block inside the strip.  N = 0 is one workgroup
    // without a live lane: the robot part alone
    if (!dense_args_ok(st, a) || !blk || a.kk / 2 > st.pcap || st.tm.padded(a.n_mm) > st.ldm || st.Gp32 || st.Kp32 || !st.Gp || !st.Kp)
        return hipErrorInvalidValue;
    const int64_t cols = st.tm.padded(a.n_mm);
    const unsigned grid = (unsigned)(cols > 0 ? cdiv(cols, (int64_t)kBlock) : 1);
    if (a.kk <= 4) hipLaunchKernelGGL(k_gather_dense<2>, dim3(grid), dim3(kBlock), 0, s, st, a, blk);
    else hipLaunchKernelGGL(k_gather_dense<8>, dim3(grid), dim3(kBlock), 0, s, st, a, blk);
    return hipGetLastError();
}

hipError_t launch_nearest(const DevState &st, int cur, int64_t N, const double R[4], NearestEntry *out, int storage, hipStream_t s) {
    if (N <= 0) return hipSuccess;
    // a group of landmarks (and a float lane's two) must lie inside one tile row / one tile; landmark indices are 32-bit in the kernel
    if (!out || !R || st.tm.world != 1 || st.tm.T < 4 || (st.tm.T / 2) % kNearestGroup != 0 || 2 * N > st.ldm || N > 0x7fffffff) return hipErrorInvalidValue;
    const int64_t grid = cdiv(cdiv(N, (int64_t)kNearestGroup), kBlock / 64);
    return with_storage(storage, [&](auto ts) {
        hipLaunchKernelGGL(k_nearest<decltype(ts)>, dim3((unsigned)grid), dim3(kBlock), 0, s, st, cur, N, R[0], R[1], R[2], R[3], out);
    });
}

// ---- the factorisation of P (factor_map.h) ----
// The factor store's tile edge.  64: a diagonal tile and the right-hand sides take 40 KiB of LDS, a lane of k_factor_panel holds a whole
// row in registers, a workgroup of k_factor_trail is four wavefronts with no LDS at all.  Edge 128 (a 128 KiB diagonal tile) is not built.
constexpr int kFactorTile = 64;
int factor_tile_edge() { return kFactorTile; }

namespace {
bool factor_args_ok(const FactorMapArgs &a) {
    return a.tiles && a.rhs && a.res && a.N >= 0 && a.tm.T == kFactorTile && a.tm.world == 1 && a.rows == a.tm.padded(2 * a.N) &&
           a.nref >= 0 && a.nref <= kFactorRefMax && (a.nref == 0 || (a.ref && a.ref_stride >= 3 + 2 * a.N)) && (a.cur == 0 || a.cur == 1);
}
}  // namespace

hipError_t launch_factor_load(const DevState &st, const FactorMapArgs &a, int storage, hipStream_t s) {
    // every tile of the source is read from this handle's store (an unsharded tile map), every landmark below 2 N lies inside it
    if (!factor_args_ok(a) || st.tm.world != 1 || 2 * a.N > st.ldm) return hipErrorInvalidValue;
    if (a.rows == 0) return hipSuccess;
    const int64_t ntiles = a.tm.row_base(a.rows / kFactorTile);
    if (ntiles > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_factor_rhs, dim3((unsigned)cdiv(a.rows, (int64_t)kFactorBlock)), dim3(kFactorBlock), 0, s, st, a);
    return with_storage(storage, [&](auto ts) {
        hipLaunchKernelGGL((k_factor_load<decltype(ts), kFactorTile>), dim3((unsigned)ntiles), dim3(kFactorBlock), 0, s, st, a);
    });
}

hipError_t launch_factor_column(const FactorMapArgs &a, int k, int part, hipStream_t s) {
    const int64_t nF = a.rows / kFactorTile, m = nF - 1 - k;
    if (!factor_args_ok(a) || k < 0 || k >= nF || part < 0 || part > 2) return hipErrorInvalidValue;
    if (part == 0) hipLaunchKernelGGL(k_factor_diag<kFactorTile>, dim3(1), dim3(kFactorBlock), 0, s, a, k);
    else if (m == 0) return hipSuccess;
    else if (part == 1) hipLaunchKernelGGL(k_factor_panel<kFactorTile>, dim3((unsigned)m), dim3(64), 0, s, a, k);
    else {
        const int64_t grid = m * (m + 1) / 2;
        if (grid > 0x7fffffffll) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_factor_trail<kFactorTile>, dim3((unsigned)grid), dim3(4 * kFactorTile), 0, s, a, k);
    }
    return hipGetLastError();
}

hipError_t launch_factor_finish(const DevState &st, const FactorMapArgs &a, hipStream_t s) {
    if (!factor_args_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_factor_finish, dim3(1), dim3(kFactorBlock), 0, s, st, a);
    return hipGetLastError();
}

// ---- the draws behind it (sample_map.h: k_factor_apply, k_factor_sample) ----
// Tiles per segment of a tile row.  16: a workgroup streams 512 KiB of the factor for one 8 KiB partial block (3 % of the store's bytes
// written and read again), and 10 000 landmarks (313 tile rows) still make 3 220 workgroups, all of the same length but the last of each tile row.
constexpr int kFactorSegment = 16;
int factor_chunk() { return kFactorChunk; }
// one partial block per segment, then per tile row its 3 x kFactorChunk part of W' Xi
int64_t factor_partial_doubles(int64_t rows) {
    const int64_t nF = rows / kFactorTile;
    return factor_segment_base(nF, kFactorSegment) * (int64_t)(kFactorTile * kFactorChunk) + nF * (3 * kFactorChunk);
}

hipError_t launch_factor_sample(const DevState &st, const FactorMapArgs &a, const FactorSampleArgs &sa, int part, hipStream_t s) {
    // every index the two kernels form lies inside the chunk (ld), the partial blocks (one per segment of the grid) and the store
    if (!factor_args_ok(a) || !a.lr_off || !sa.xi || !sa.y || !sa.part || sa.ld < a.rows + 3 || part < 0 || part > 1) return hipErrorInvalidValue;
    const int64_t nF = a.rows / kFactorTile, segments = factor_segment_base(nF, kFactorSegment);
    if (segments > 0x7fffffffll) return hipErrorInvalidValue;
    if (part == 0) {
        if (segments == 0) return hipSuccess;
        hipLaunchKernelGGL((k_factor_apply<kFactorTile, kFactorSegment>), dim3((unsigned)segments), dim3(4 * kFactorTile), 0, s, a, sa);
    } else
        hipLaunchKernelGGL((k_factor_sample<kFactorTile, kFactorSegment>), dim3((unsigned)(nF + 1)), dim3(kFactorBlock), 0, s, st, a, sa);
    return hipGetLastError();
}

// ---- the solves behind it (solve_map.h: k_solve_invert, k_solve_forward, k_solve_tail, k_solve_backward) ----
int64_t solve_inverse_doubles(int64_t rows) { return rows * (int64_t)kFactorTile; }

hipError_t launch_solve_map(const FactorMapArgs &a, const FactorSolveArgs &sv, int part, int c, hipStream_t s) {
    // every index the kernels form lies inside the chunks (ld), the inverse tiles (one per tile row) and the store (c inside the grid)
    if (!factor_args_ok(a) || !a.lr_off || !sv.b || !sv.y || !sv.inv || sv.ld < a.rows + 3 || (sv.form != 0 && sv.form != 1)) return hipErrorInvalidValue;
    const int64_t nF = a.rows / kFactorTile;
    if (part == 0) {
        if (nF == 0) return hipSuccess;
        hipLaunchKernelGGL(k_solve_invert<kFactorTile>, dim3((unsigned)nF), dim3(64), 0, s, a, sv);
    } else if (part == 1 || part == 3) {
        if (c < 0 || c >= nF || (part == 3 && sv.form != 0)) return hipErrorInvalidValue;
        if (part == 1) hipLaunchKernelGGL(k_solve_forward<kFactorTile>, dim3((unsigned)(nF - c)), dim3(4 * kFactorTile), 0, s, a, sv, c);
        else hipLaunchKernelGGL(k_solve_backward<kFactorTile>, dim3((unsigned)(c + 1)), dim3(4 * kFactorTile), 0, s, a, sv, c);
    } else if (part == 2)
        hipLaunchKernelGGL(k_solve_tail, dim3(1), dim3(kFactorBlock), 0, s, a, sv);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

// ---- the plain product P B on the handle's own store (multiply_map.h: k_multiply_tiles, k_multiply_sum) ----
// Tiles per segment of a tile row: 256 columns' worth.  A workgroup then streams 2 tiles at the F64 production edge 128 and one at 256
// for one direct partial block, and a map of 140 landmarks at edge 16 still has tile rows of two segments.
int multiply_segment(int T) { return T >= 256 ? 1 : 256 / T; }
void multiply_partial_offsets(const TileMap &tm, int64_t rows, int64_t *tpart, int64_t *wpart) {
    const int64_t nT = rows / tm.T, blk = (int64_t)tm.T * kFactorChunk;
    *tpart = factor_segment_base(nT, multiply_segment(tm.T)) * blk;
    *wpart = *tpart + tm.row_base(nT) * blk;
}
int64_t multiply_partial_doubles(const TileMap &tm, int64_t rows) {
    int64_t t, w;
    multiply_partial_offsets(tm, rows, &t, &w);
    return w + (rows / tm.T) * (3 * kFactorChunk);
}

hipError_t launch_multiply_map(const DevState &st, const MultiplyMapArgs &a, int part, int storage, hipStream_t s) {
    // every index the kernels form lies inside the chunks (ld), the partial blocks (one per segment, one slot per tile, one part per tile
    // row) and the handle's own store (an unsharded tile map, every landmark below 2 N inside the strip)
    const int T = st.tm.T;
    if (!a.b || !a.y || !a.dpart || !a.tpart || !a.wpart || a.N < 0 || st.tm.world != 1 || T < 16 || T > 16 * 4 * kMultiplyWaveBlocks || (T & (T - 1)) ||
        2 * a.N > st.ldm || a.rows != st.tm.padded(2 * a.N) || a.ld < a.rows + 3 || a.S != multiply_segment(T) || (a.cur != 0 && a.cur != 1) || part < 0 || part > 1)
        return hipErrorInvalidValue;
    const int64_t nT = a.rows / T, segments = factor_segment_base(nT, a.S);
    if (segments > 0x7fffffffll) return hipErrorInvalidValue;
    if (part == 1) {
        const int64_t grid = nT * cdiv((int64_t)T * kFactorChunk, (int64_t)kFactorBlock);
        if (grid > 0x7fffffffll) return hipErrorInvalidValue;
        if (grid > 0) hipLaunchKernelGGL(k_multiply_sum, dim3((unsigned)grid), dim3(kFactorBlock), 0, s, st, a);
        hipLaunchKernelGGL(k_multiply_robot, dim3(1), dim3(kFactorBlock), 0, s, st, a);
        return hipGetLastError();
    }
    if (segments == 0) return hipSuccess;
    return with_storage(storage, [&](auto ts) {
        using TS = decltype(ts);
        if (T <= 128) hipLaunchKernelGGL((k_multiply_tiles<TS, 128>), dim3((unsigned)segments), dim3(kMultiplyBlock), 0, s, st, a);
        else hipLaunchKernelGGL((k_multiply_tiles<TS, 256>), dim3((unsigned)segments), dim3(kMultiplyBlock), 0, s, st, a);
    });
}
