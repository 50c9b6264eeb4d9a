// Fragment of kernels.hip, the launchers of the map edits: landmark removal (compact.h), part of a map taken out into another handle
// (extract_map.h), the whole map moved into another frame (transform_map.h), the fused pass of a batch of merges (merge_pass.h), a
// constraint between two landmarks and its chained form (constrain.h), a linear observation (linear_obs.h), one through a model
// (model_obs.h), with the landmark read on the device (model_assigned.h) and relinearised (model_iter.h), the joint innovation of a scan's
// pairings (joint.h), the search over them (joint_search.h) and their joint update (joint_update.h, joint_iter.h), the candidate search
// (nearest.h).  The calls that treat P as a matrix have launch/map_algebra.h.
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

hipError_t launch_nearest(const DevState &st, int cur, int64_t N, const double R[4], NearestEntry *out, int storage, hipStream_t s) {
    if (N <= 0) return hipSuccess;
    // a group of landmarks (and a float lane's two) must lie inside one tile row / one tile; landmark indices are 32-bit in the kernel
    if (!out || !R || st.tm.world != 1 || st.tm.T < 4 || (st.tm.T / 2) % kNearestGroup != 0 || 2 * N > st.ldm || N > 0x7fffffff) return hipErrorInvalidValue;
    const int64_t grid = cdiv(cdiv(N, (int64_t)kNearestGroup), kBlock / 64);
    return with_storage(storage, [&](auto ts) {
        hipLaunchKernelGGL(k_nearest<decltype(ts)>, dim3((unsigned)grid), dim3(kBlock), 0, s, st, cur, N, R[0], R[1], R[2], R[3], out);
    });
}
