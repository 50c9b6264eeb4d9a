// Fragment of abi.hip, a linear observation with a dense k x n H (ekf_observe_dense, ekf_observe_dense_innovation): ekf_multiply_map's rungs and
// ONE chunk of its product for G = P H' (host/multiply_map.h: its scratch, its two launches, no download), two small launches for S, nu and
// the factorisation, one readback and the decision on the host, then ekf_observe_model_joint's route (host/joint_update.h): the pairs into
// ekf_merge_landmarks_batch's private F64 ring, one F64-arithmetic pass through launch_downdate -- so the handle's own ring, cfg.batch and
// cfg.pass_arith are not involved.  A SYNCHRONISING EDIT, not an update-step.
#pragma once
namespace {
static_assert(EKF_DENSE_MAX == kFactorChunk && EKF_DENSE_MAX == kDenseMax, "the rows of a call are one chunk of ekf_multiply_map");
static_assert(EKF_DENSE_MAX <= 2 * EKF_MERGE_BATCH_MAX, "the pairs share ekf_merge_landmarks_batch's private ring");
static_assert(sizeof(DenseRecord) == sizeof(ekf_observe_dense_result) && sizeof(ekf_observe_dense_result) == 24, "DenseRecord is ekf_observe_dense_result, field by field");

// everything that can fail for lack of memory, before anything is queued: the product's scratch, the private ring (merge_batch_alloc's, by
// its formula), the partial sums for n2 landmark rows, the block, the answer on both sides and its event
int32_t dense_alloc(ekf_handle *h, int64_t rows, int64_t n2) {
    TRY(multiply_alloc(h, rows));
    const bool first = !h->d_mring || !h->d_dblock || !h->d_dout;
    if (!h->d_mring) HIPCHK(h, dalloc(h, &h->d_mring, (size_t)h->st.pair_stride * EKF_MERGE_BATCH_MAX * 2));
    if (!h->d_dblock) HIPCHK(h, dalloc(h, &h->d_dblock, 1));
    if (!h->d_dout) HIPCHK(h, dalloc(h, &h->d_dout, 1));
    if (first) HIPCHK(h, hipDeviceSynchronize());          // dalloc clears on the null stream (see removal_alloc)
    TRY(stage_alloc(h, &h->h_dout, sizeof(DenseOut), &h->ev_dense));
    if (h->dn_rows < n2) {
        // not cleared: k_dense_gram writes every sum that k_dense_factor reads.  Nothing of it is in use: every call waits for its readback
        if (h->d_dpart) hipFree(h->d_dpart);
        h->d_dpart = nullptr;
        h->bytes -= h->dn_bytes;
        h->dn_bytes = 0;
        h->dn_rows = -1;
        const size_t bytes = (size_t)std::max<int64_t>(dense_partial_doubles(n2), 1) * sizeof(double);
        const hipError_t e = hipMalloc((void **)&h->d_dpart, bytes);
        if (e != hipSuccess) return fail(h, EKF_ERR_HIP, "observe_dense: the partial sums could not be allocated; nothing was changed", e);
        h->dn_rows = n2;
        h->dn_bytes = (int64_t)bytes;
        h->bytes += h->dn_bytes;
    }
    return EKF_OK;
}

// ekf_observe_dense (apply) and ekf_observe_dense_innovation: ONE text.
// Order: arguments -> the rungs -> every allocation -> the flush -> the chunk, the product, gram and factor, the readback, the wait, the
// decision -> the gather -> the pass, in place on the main stream.
int32_t dense_body(ekf_handle *h, const std::string &who, const double *H, int64_t k, const double *z, const double *R, const int32_t *wrap_deg,
                   double gate, bool apply, ekf_observe_dense_result *res, double *nu, double *S) {
    REQUIRE(h, H != nullptr && z != nullptr && R != nullptr && res != nullptr, EKF_ERR_INVALID_ARG, (who + "null argument").c_str());
    REQUIRE(h, k >= 1 && k <= EKF_DENSE_MAX, EKF_ERR_INVALID_ARG, (who + "between 1 and EKF_DENSE_MAX rows").c_str());
    for (int64_t i = 0; i < k; ++i) REQUIRE(h, std::isfinite(z[i]), EKF_ERR_INVALID_ARG, (who + "z is not finite").c_str());
    for (int64_t i = 0; i < k * k; ++i) REQUIRE(h, std::isfinite(R[i]), EKF_ERR_INVALID_ARG, (who + "R is not finite").c_str());
    for (int64_t i = 0; i < k; ++i)
        for (int64_t j = 0; j < i; ++j) REQUIRE(h, R[i + j * k] == R[j + i * k], EKF_ERR_INVALID_ARG, (who + "R is not symmetric").c_str());
    for (int64_t i = 0; i < k; ++i) REQUIRE(h, R[i + i * k] >= 0.0, EKF_ERR_INVALID_ARG, (who + "R has a negative diagonal entry").c_str());
    double g;
    TRY(parse_gate(h, who, gate, g));
    auto finite_H = [&]() {
        const int64_t n = 3 + 2 * h->N;
        for (int64_t i = 0; i < k * n; ++i)
            if (!std::isfinite(H[i])) return false;
        return true;
    };
    const bool exact = unsettled(h) == 0;                   // (cfg.device_assoc == 4 with rows queued: N, and with it H's size, is exact only behind the rungs)
    if (exact) REQUIRE(h, finite_H(), EKF_ERR_INVALID_ARG, (who + "H is not finite").c_str());
    TRY(edit_unsharded(h, who, "G = P H' reads every tile of the lower triangle, and every shard holds only its own tiles"));
    TRY(edit_settled(h, who));
    if (!exact) REQUIRE(h, finite_H(), EKF_ERR_INVALID_ARG, (who + "H is not finite").c_str());
    const int64_t N = h->N, n = 3 + 2 * N, n2 = 2 * N;
    const int64_t rows = h->st.tm.padded(n2);
    TRY(dense_alloc(h, rows, n2));
    TRY(edit_flushed(h));                  // retires a pass in flight; from here on the tiles hold the live P and the ring is empty

    // the stacked system: k rounded up to even, the last row exactly empty where k is odd
    const int kk = (int)((k + 1) & ~(int64_t)1);
    DenseSmall sm = DenseSmall();
    for (int64_t i = 0; i < k; ++i) {
        sm.z[i] = z[i];
        sm.wrap[i] = wrap_deg && wrap_deg[i] ? 1 : 0;
        for (int64_t j = 0; j < k; ++j) sm.R[i * kDenseMax + j] = R[i + j * k];
    }
    if (kk > k) sm.R[k * kDenseMax + k] = 1.0;
    // H as one chunk of the product, in multiply_body's layout (the slot is free: every call that uses it waits for a readback behind its upload)
    const MultiplyMapArgs ma = multiply_chunk_args(h, rows);
    const size_t chunk = sample_chunk_doubles(rows);
    double *u = h->h_pmb;
    std::memset(u, 0, chunk * sizeof(double));
    for (int64_t c = 0; c < k; ++c) {
        const double *row = H + c * n;
        std::memcpy(u + c * ma.ld, row + 3, (size_t)n2 * sizeof(double));
        std::memcpy(u + c * ma.ld + rows, row, 3 * sizeof(double));
    }
    HIPCHK(h, hipMemcpyAsync(h->d_pmul, u, chunk * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (N > 0) TIMED(h, EKF_KERNEL_ASSOCIATE, launch_multiply_map(h->st, ma, 0, h->storage, h->stream));
    TIMED(h, EKF_KERNEL_COMPACT, launch_multiply_map(h->st, ma, 1, h->storage, h->stream));
    DenseArgs a = DenseArgs();
    a.b = ma.b; a.y = ma.y; a.part = h->d_dpart; a.ld = ma.ld; a.rows = rows; a.n_mm = n2; a.kk = kk; a.cur = h->cur;
    if (N > 0) TIMED(h, EKF_KERNEL_ASSOCIATE, launch_dense_gram(h->st, a, h->stream));
    TIMED(h, EKF_KERNEL_ASSOCIATE, launch_dense_factor(h->st, a, sm, h->d_dout, h->d_dblock, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->h_dout, h->d_dout, sizeof(DenseOut), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipEventRecord(h->ev_dense, h->stream));
    HIPCHK(h, hipEventSynchronize(h->ev_dense));
    const DenseOut &o = *h->h_dout;
    res->d2 = o.rec.d2; res->rows = (int32_t)k; res->outcome = o.rec.outcome; res->bad_row = o.rec.bad_row;
    if (nu) for (int64_t i = 0; i < k; ++i) nu[i] = o.nu[i];
    if (S) for (int64_t j = 0; j < k; ++j) for (int64_t i = 0; i < k; ++i) S[i + j * k] = o.S[i * kDenseMax + j];
    // the decision, on the host, before anything is written
    if (res->outcome != EKF_LINEAR_APPLIED) {
        res->outcome = EKF_LINEAR_IRREGULAR;
        if (!apply) return EKF_OK;
        return fail(h, EKF_ERR_STATE, (who + "row " + std::to_string(res->bad_row) + ": the pivot of S = H P H' + R is not finite and positive (rows that "
                    "say the same under R = 0, a state that is not finite); nothing was changed").c_str());
    }
    if (!apply) return EKF_OK;
    if (!(res->d2 <= g)) { res->outcome = EKF_LINEAR_GATED; return EKF_OK; }

    // the gather, on a view of the state whose pair ring is the private one
    DevState st = h->st;
    st.Gp = h->d_mring; st.Kp = h->d_mring + (size_t)h->st.pair_stride * EKF_MERGE_BATCH_MAX; st.pcap = EKF_MERGE_BATCH_MAX;
    st.Gp32 = nullptr; st.Kp32 = nullptr;
    if (N > 0) TRY(refresh_work(h));       // (before the gather: nothing may fail between it and the pass)
    TIMED(h, EKF_KERNEL_GATHER, launch_gather_dense(st, a, h->d_dblock, h->stream));
    h->cur ^= 1;
    h->st.dcur ^= 1;
    h->hint_idx = -1;
    if (N > 0) {
        // ONE pass for the kk / 2 pairs, F64 arithmetic whatever cfg.pass_arith says: a float tile entry is rounded once
        next_pass_direction(h);
        st.dcur = h->st.dcur; st.tm = h->st.tm;
        TimedLaunch tl(h, EKF_KERNEL_DOWNDATE);
        const ekf_handle::WorkSet &ws = h->ws[h->ws_cur];
        PassJob job = {};
        job.dst = h->st.tiles;
        job.work = ws.work; job.nwork = ws.nwork; job.work_xcd = ws.xcd; job.xcd_len = ws.xcd_len;
        job.pstart = 0; job.npairs = kk / 2;
        job.grid_cap = h->grid_cap; job.arith = EKF_ARITH_F64;
        job.aux = nullptr; job.nx = nullptr;
        HIPCHK(h, launch_downdate(st, job, h->storage, h->stream, h->dd_kernel));
        h->dd_pairs = kk / 2;
    }
    tiles_changed(h);
    return EKF_OK;
}
}  // namespace

extern "C" {
int32_t ekf_observe_dense(ekf_handle *h, const double *H, int64_t k, const double *z, const double *R, const int32_t *wrap_deg, double gate,
                          ekf_observe_dense_result *res, double *nu, double *S) {
    if (!h) return EKF_ERR_INVALID_ARG;
    return dense_body(h, "observe_dense: ", H, k, z, R, wrap_deg, gate, /*apply*/ true, res, nu, S);
}

int32_t ekf_observe_dense_innovation(ekf_handle *h, const double *H, int64_t k, const double *z, const double *R, const int32_t *wrap_deg,
                                     ekf_observe_dense_result *res, double *nu, double *S) {
    if (!h) return EKF_ERR_INVALID_ARG;
    return dense_body(h, "observe_dense_innovation: ", H, k, z, R, wrap_deg, INFINITY, /*apply*/ false, res, nu, S);
}
}  // extern "C"
