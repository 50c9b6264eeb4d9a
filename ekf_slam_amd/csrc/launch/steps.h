// Fragment of kernels.hip, the launchers of the steps: predict, a chain of model predicts, append, the join of a local map, the gather of a correction in its five forms, a shard's
// row-panels, the association and the model-convention association of a scan (declared in kernels.h, in this order).
#pragma once

hipError_t launch_predict(const DevState &st, const PredictArgs &a, int, hipStream_t s) {
    // MFMA panel product at large landmark counts (EKF_PREDICT_MFMA=0/1 forces the VALU / MFMA kernel)
    static const int force = ekf_tune_int("EKF_PREDICT_MFMA", -1);
    const bool mfma = force >= 0 ? force != 0 : a.n_mm >= 2048;
    if (mfma) {
        const int64_t nslices = (a.n_mm + 15) / 16;
        int64_t grid = cdiv(nslices > 0 ? nslices : 1, 4);
        if (grid > 1024) grid = 1024;
        hipLaunchKernelGGL(k_predict_mfma, dim3((unsigned)grid), dim3(kBlock), 0, s, st, a);
        return hipGetLastError();
    }
    const int64_t grid = cdiv(a.n_mm > 0 ? a.n_mm : 1, kBlock);
    hipLaunchKernelGGL(k_predict, dim3((unsigned)grid), dim3(kBlock), 0, s, st, a);
    return hipGetLastError();
}

hipError_t launch_predict_model(const DevState &st, const PredictModelArgs &a, hipStream_t s) {
    if (a.n_mm < 0 || a.n_mm > st.ldm || a.m < 1 || a.m > kPredictModelMax) return hipErrorInvalidValue;
    for (int b = 0; b < a.m; ++b) if (a.e[b].model < 1 || a.e[b].model > 3) return hipErrorInvalidValue;
    const int64_t grid = cdiv(a.n_mm > 0 ? a.n_mm : 1, kBlock);
    hipLaunchKernelGGL(k_predict_model, dim3((unsigned)grid), dim3(kBlock), 0, s, st, a);
    return hipGetLastError();
}

hipError_t launch_append(const DevState &st, const AppendArgs &a, int storage, hipStream_t s, const DevLoopArgs *dlp,
                         const PredictArgs *fused_predict) {
    const int64_t n_mm = 2 * a.N;
    const int64_t grid = cdiv(n_mm > 0 ? n_mm : 1, kBlock);
    const DevLoopArgs dl = dlp ? *dlp : DevLoopArgs{};
    const PredictArgs pa = predict_or_none(fused_predict);
    return with_storage(storage, [&](auto ts) { with_bool(fused_predict != nullptr, [&](auto pred) {
        hipLaunchKernelGGL((k_append<decltype(ts), decltype(pred)::value>), dim3((unsigned)grid), dim3(kBlock), 0, s, st, a, dl, pa);
    }); });
}

hipError_t launch_append_model(const DevState &st, const AppendModelArgs &a, int storage, hipStream_t s) {
    if (a.N < 0 || a.m < 1 || a.m > kAppendModelMax || 2 * (a.N + a.m) > st.ldm) return hipErrorInvalidValue;
    for (int b = 0; b < a.m; ++b) if (a.e[b].model != 1 && a.e[b].model != 4) return hipErrorInvalidValue;
    const int64_t grid = cdiv(2 * (a.N + a.m), kBlock);
    return with_storage(storage, [&](auto ts) {
        hipLaunchKernelGGL(k_append_model<decltype(ts)>, dim3((unsigned)grid), dim3(kBlock), 0, s, st, a);
    });
}

hipError_t launch_join_state(const DevState &st, const DevState &lo, const JoinMapArgs &a, hipStream_t s) {
    if (a.N < 0 || a.M < 0 || 2 * (a.N + a.M) > st.ldm || 2 * a.M > lo.ldm) return hipErrorInvalidValue;
    const int64_t cols = 2 * (a.N + a.M);
    const int64_t grid = cdiv(cols > 0 ? cols : 1, kBlock);
    hipLaunchKernelGGL(k_join_state, dim3((unsigned)grid), dim3(kBlock), 0, s, st, lo, a);
    return hipGetLastError();
}

hipError_t launch_join_rows(const DevState &st, const DevState &lo, const JoinMapArgs &a, int storage, int local_storage, hipStream_t s) {
    if (a.N < 0 || a.M < 1 || 2 * (a.N + a.M) > st.ldm || 2 * a.M > lo.ldm || st.tm.world != 1 || lo.tm.world != 1) return hipErrorInvalidValue;
    const int64_t per_row = cdiv(a.N + a.M, kBlock);          // workgroups per new landmark: 256 column landmarks each
    const int64_t grid = a.M * per_row;
    if (grid > 0x7fffffffll) return hipErrorInvalidValue;
    return with_storage(storage, [&](auto td) { with_storage(local_storage, [&](auto tsrc) {
        hipLaunchKernelGGL((k_join_rows<decltype(td), decltype(tsrc)>), dim3((unsigned)grid), dim3(kBlock), 0, s, st, lo, a, (int32_t)per_row);
    }); });
}

// k_gather.  The kernel is 216 VGPRs wide and every flag doubles its instantiations, so only the forms a handle can ask for exist:
// per storage type  {plain, fused downdate, device loop} x {predict folded in or not},  the device-decided form (never with a predict),
// sharded {plain, device loop} x {predict}  -- 11, each named by one of the launchers below.
int64_t gather_workgroups(const DevState &st, int64_t n_mm) { return cdiv(ekf_tiles_for(n_mm, st.tm.T) * st.tm.T, kGatherCols); }
int gather_fuse_max_rows() { return kFuseMaxRows; }

namespace {
// pv: all zeros for an unsharded gather, which reads the row-panel from its own tiles; dl: read when kDev
template <bool kSharded, bool kFused, bool kDev, bool kDecide>
hipError_t gather_form(const DevState &st, const CorrectArgs &a, const PredictArgs *fused_predict, const PanelView &pv,
                       const DevLoopArgs *dl, int storage, hipStream_t s) {
    typename DevLoopParam<kDev>::type dla{};
    if constexpr (kDev) {
        if (!dl->parts_in || !dl->rec || dl->nblk_in < 1 || a.n_mm < 2) return hipErrorInvalidValue;
        dla = *dl;
    }
    const int64_t grid = gather_workgroups(st, a.n_mm);
    const PredictArgs pa = predict_or_none(fused_predict);
    return with_storage(storage, [&](auto ts) {
        auto launch = [&](auto pred) {
            hipLaunchKernelGGL((k_gather<decltype(ts), kSharded, decltype(pred)::value, kFused, kDev, kDecide>), dim3((unsigned)grid),
                               dim3(kGatherBlock), 0, s, st, a, pv, pa, dla);
        };
        if constexpr (kDecide) launch(std::false_type{});
        else with_bool(fused_predict != nullptr, launch);
    });
}
}  // namespace

hipError_t launch_gather(const DevState &st, const CorrectArgs &a, const PredictArgs *fused_predict, int storage,
                         hipStream_t s, bool fuse_downdate) {
    if (!fuse_downdate) return gather_form<false, false, false, false>(st, a, fused_predict, PanelView{}, nullptr, storage, s);
    if (a.n_mm > kFuseMaxRows || gather_workgroups(st, a.n_mm) != 1) return hipErrorInvalidValue;
    return gather_form<false, true, false, false>(st, a, fused_predict, PanelView{}, nullptr, storage, s);
}

hipError_t launch_gather_devloop(const DevState &st, const CorrectArgs &a, const PredictArgs *fused_predict, const DevLoopArgs &dl,
                                 int storage, hipStream_t s) {
    return gather_form<false, false, true, false>(st, a, fused_predict, PanelView{}, &dl, storage, s);
}

hipError_t launch_gather_decided(const DevState &st, const CorrectArgs &a, const DevLoopArgs &dl, int storage, hipStream_t s) {
    if (!dl.dn_out || !dl.loc || !dl.abort || (dl.n_known < 0 && !dl.dn_in)) return hipErrorInvalidValue;
    return gather_form<false, false, true, true>(st, a, nullptr, PanelView{}, &dl, storage, s);
}

hipError_t launch_gather_sharded(const DevState &st, const CorrectArgs &a, const PredictArgs *fused_predict, const double *recv,
                                 int64_t rank_stride, int64_t offset, bool patched, int storage, hipStream_t s, const DevLoopArgs *dl) {
    const PanelView pv = { recv, rank_stride, offset, /*Ij*/ a.j >> st.tm.shift, patched ? 1 : 0 };
    return dl ? gather_form<true, false, true, false>(st, a, fused_predict, pv, dl, storage, s)
              : gather_form<true, false, false, false>(st, a, fused_predict, pv, nullptr, storage, s);
}

// ---- a shard's row-panels ----
hipError_t launch_rowpanel(const DevState &st, int64_t j, int64_t n_mm, int pstart, int npend, double *send, int storage,
                           hipStream_t s) {
    const int64_t nloc = rowpanel_local_chunks(st.tm, j, n_mm);
    if (nloc == 0) return hipSuccess;
    const int64_t grid = cdiv(nloc * st.tm.T, kBlock);
    return with_storage(storage, [&](auto ts) {
        hipLaunchKernelGGL(k_rowpanel<decltype(ts)>, dim3((unsigned)grid), dim3(kBlock), 0, s, st, j, n_mm, pstart, npend, send, nloc, NoDevLoop{});
    });
}

hipError_t launch_rowpanel_dev(const DevState &st, int64_t j, int64_t n_mm, int pstart, int npend, double *send, int storage,
                               hipStream_t s, const DevLoopArgs &dl) {
    if (!dl.parts_in || dl.nblk_in < 1) return hipErrorInvalidValue;
    const int64_t nt = ekf_tiles_for(n_mm, st.tm.T);
    const int64_t most = (nt + st.tm.world - 1) / st.tm.world;           // what the tile row with this shard's first chunk at k = 0 gives
    const int64_t grid = cdiv(most * st.tm.T, kBlock);
    return with_storage(storage, [&](auto ts) {
        hipLaunchKernelGGL((k_rowpanel<decltype(ts), true>), dim3((unsigned)grid), dim3(kBlock), 0, s, st, j, n_mm, pstart, npend, send, (int64_t)0, dl);
    });
}

namespace {
// the row list and the grid of a prefetch of m landmarks (one grid row per landmark), then launch(rows, grid)
template <typename Launch>
hipError_t rowpanel_prefetch(const DevState &st, const int64_t *idx, int m, int64_t n_mm, bool args_ok, Launch &&launch) {
    if (m <= 0) return hipSuccess;
    if (m > 64 || !args_ok) return hipErrorInvalidValue;
    RowList rows;
    rows.m = m;
    for (int q = 0; q < m; ++q) rows.j[q] = (int32_t)(2 * idx[q]);
    const int64_t nt = st.tm.tiles_for(n_mm);
    const int64_t max_chunks = (nt + st.tm.world - 1) / st.tm.world;
    if (max_chunks == 0) return hipSuccess;
    return launch(rows, dim3((unsigned)cdiv(max_chunks * st.tm.T, kBlock), (unsigned)m));
}
}  // namespace

hipError_t launch_rowpanel_base(const DevState &st, const int64_t *idx, int m, int64_t n_mm, double *send, int64_t slab,
                                int storage, hipStream_t s) {
    return rowpanel_prefetch(st, idx, m, n_mm, true, [&](const RowList &rows, dim3 grid) { return with_storage(storage, [&](auto ts) {
        hipLaunchKernelGGL(k_rowpanel_base<decltype(ts)>, grid, dim3(kBlock), 0, s, st, rows, n_mm, send, slab);
    }); });
}

hipError_t launch_rowpanel_next(const DevState &st, const int64_t *idx, int m, int64_t n_mm, int pstart, int npend, double *send,
                                int64_t slab, int storage, hipStream_t s) {
    const bool ring_ok = npend >= 0 && npend <= kMaxPending;
    return rowpanel_prefetch(st, idx, m, n_mm, ring_ok, [&](const RowList &rows, dim3 grid) { return with_storage(storage, [&](auto ts) {
        hipLaunchKernelGGL(k_rowpanel_next<decltype(ts)>, grid, dim3(kBlock), 0, s, st, rows, n_mm, pstart, npend, send, slab);
    }); });
}

// ---- association ----
namespace {
template <bool kDevN>
hipError_t associate_form(const DevState &st, const AssocArgs &a, double *pos_cost, double *sig_cost, AssocDecision *partial, int *ticket,
                          AssocDecision *decision, AssocHostPartial *host_partials, int seq, double *cand, int storage, hipStream_t s,
                          const PredictArgs *fused_predict) {
    const int64_t grid = cdiv(a.N > 0 ? a.N : 1, kAssocBlock);
    const PredictArgs pa = predict_or_none(fused_predict);
    return with_storage(storage, [&](auto ts) { with_bool(fused_predict != nullptr, [&](auto pred) {
        hipLaunchKernelGGL((k_associate<decltype(ts), decltype(pred)::value, kDevN>), dim3((unsigned)grid), dim3(kAssocBlock), 0, s, st, a, pos_cost,
                           sig_cost, partial, ticket, decision, host_partials, seq, cand, pa);
    }); });
}
}  // namespace

hipError_t launch_associate(const DevState &st, const AssocArgs &a, double *pos_cost, double *sig_cost,
                            AssocDecision *partial, int *ticket, AssocDecision *decision, AssocHostPartial *host_partials, int seq,
                            double *cand, int storage, hipStream_t s, const PredictArgs *fused_predict) {
    return associate_form<false>(st, a, pos_cost, sig_cost, partial, ticket, decision, host_partials, seq, cand, storage, s, fused_predict);
}

hipError_t launch_associate_devn(const DevState &st, const AssocArgs &a, AssocHostPartial *host_partials, int seq, int storage,
                                 hipStream_t s, const PredictArgs *fused_predict) {
    if (!host_partials) return hipErrorInvalidValue;
    return associate_form<true>(st, a, nullptr, nullptr, nullptr, nullptr, nullptr, host_partials, seq, nullptr, storage, s, fused_predict);
}

hipError_t launch_assoc_merge(const DevState &st, const double *recv, int world, int64_t count, int64_t N, bool want_costs,
                              double *pos_cost, AssocDecision *decision, AssocDecision *host_decision, int seq, hipStream_t s) {
    int64_t grid = want_costs ? cdiv(N > 0 ? N : 1, kBlock) : 1;
    if (grid > 1024) grid = 1024;
    hipLaunchKernelGGL(k_assoc_merge, dim3((unsigned)grid), dim3(kBlock), 0, s, st.tm, recv, world, count, N, want_costs ? 1 : 0,
                       pos_cost, decision, host_decision, seq);
    return hipGetLastError();
}

hipError_t launch_assoc_model(const DevState &st, const AssocModelArgs &a, ekfm::Match2 *partials, ekfm::Match2 *out, double *d2_all,
                              hipStream_t s) {
    if (a.N < 1 || 2 * a.N > st.ldm || a.m < 1 || a.m > kAssocModelMax || !partials || !out) return hipErrorInvalidValue;
    for (int k = 0; k < a.m; ++k) if (a.e[k].model < 1 || a.e[k].model > 4) return hipErrorInvalidValue;
    const int64_t nblk = cdiv(a.N, kAssocBlock);
    hipLaunchKernelGGL(k_assoc_model, dim3((unsigned)nblk, (unsigned)a.m), dim3(kAssocBlock), 0, s, st, a, partials, d2_all);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_assoc_model_reduce, dim3((unsigned)a.m), dim3(64), 0, s, partials, (int)nblk, out);
    return hipGetLastError();
}

hipError_t launch_assign_lists(const DevState &st, const AssocModelArgs &a, ekfm::Match2 *partials, ekfm::CandList *lists, ekfm::CandList *sel,
                               AssignResult *res, hipStream_t s) {
    if (a.N < 1 || 2 * a.N > st.ldm || a.m < 1 || a.m > kAssocModelMax || !partials || !lists || !sel || !res) return hipErrorInvalidValue;
    for (int k = 0; k < a.m; ++k)
        if (a.e[k].model < 1 || a.e[k].model > 4 || !std::isfinite(a.e[k].gate)) return hipErrorInvalidValue;
    const int64_t nblk = cdiv(a.N, kAssocBlock);
    hipLaunchKernelGGL(k_assign_candidates, dim3((unsigned)nblk, (unsigned)a.m), dim3(kAssocBlock), 0, s, st, a, partials, lists);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_assign_select, dim3((unsigned)a.m), dim3(kAssocBlock), 0, s, partials, lists, (int)nblk, (ekfm::Match2 *)res->match, sel);
    return hipGetLastError();
}

hipError_t launch_assign_model(const DevState &st, const AssocModelArgs &a, ekfm::Match2 *partials, ekfm::CandList *lists, ekfm::CandList *sel,
                               AssignResult *res, hipStream_t s) {
    if (a.N < 1 || 2 * a.N > st.ldm || a.m < 1 || a.m > kAssocModelMax || !partials || !lists || !sel || !res) return hipErrorInvalidValue;
    AssignSolveArgs sa = {};
    sa.m = a.m;
    for (int k = 0; k < a.m; ++k) {
        if (a.e[k].model < 1 || a.e[k].model > 4 || !std::isfinite(a.e[k].gate)) return hipErrorInvalidValue;
        sa.gate[k] = a.e[k].gate;
    }
    const int64_t nblk = cdiv(a.N, kAssocBlock);
    hipLaunchKernelGGL(k_assign_candidates, dim3((unsigned)nblk, (unsigned)a.m), dim3(kAssocBlock), 0, s, st, a, partials, lists);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_assign_select, dim3((unsigned)a.m), dim3(kAssocBlock), 0, s, partials, lists, (int)nblk, (ekfm::Match2 *)res->match, sel);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_assign_solve, dim3(1), dim3(64), 0, s, sa, sel, res);
    return hipGetLastError();
}
