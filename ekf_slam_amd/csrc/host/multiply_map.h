// Fragment of abi.hip, the plain product P B (ekf_multiply_map): k vectors through exactly what ekf_get_P would report, in one read-only
// pass over the handle's OWN tile store per chunk of factor_chunk() vectors -- no factorisation, no factor store.  A SYNCHRONISING,
// READ-ONLY call on the rungs of host/edits.h, as ekf_nearest_landmarks and ekf_factor_map: a recorded predict carried out, the pending
// pairs applied, an asynchronous pass retired; x, s, P, the diagonal copies and the digest are afterwards those of a handle that only
// flushed.  No invalidation function is called and nothing is kept between calls but the scratch.  Unsharded only: the pass reads every
// tile, and a shard holds only its own.  The chunks travel as ekf_sample_map's do, through the same chunk_stream (host/factor_map.h:
// kSampleSlots pinned slots a direction, the host waits only where it takes a slot again), in a scratch and with events of this call's own, so that the byte counts
// of the factor, sample and solve calls stay what they were.
#pragma once
namespace {
void multiply_release(ekf_handle *h) {
    if (h->d_pmul) hipFree(h->d_pmul);
    if (h->h_pmb) hipHostFree(h->h_pmb);
    if (h->h_pmy) hipHostFree(h->h_pmy);
    h->d_pmul = h->h_pmb = h->h_pmy = nullptr;
    h->bytes -= h->pm_bytes;
    h->pm_bytes = 0;
    h->pm_rows = -1;
}

// The scratch for `rows` rows (a multiple of the handle's tile edge): a chunk of vectors, a chunk of products, the partial blocks; the
// pinned slots; their events -- everything that can fail for lack of memory, before anything is queued.  Its size depends on the rows
// alone, not on k.  Nothing is cleared: the launches write every byte that is read.  Nothing of it is in use here: every call ends drained.
int32_t multiply_alloc(ekf_handle *h, int64_t rows) {
    for (hipEvent_t &ev : h->ev_pmslot) if (!ev) HIPCHK(h, new_event(h, &ev));
    if (h->pm_rows >= rows) return EKF_OK;
    multiply_release(h);
    const size_t chunk = sample_chunk_doubles(rows), part = (size_t)multiply_partial_doubles(h->st.tm, rows);
    const size_t dev_bytes = (2 * chunk + (part ? part : 1)) * sizeof(double);
    hipError_t e = hipMalloc((void **)&h->d_pmul, dev_bytes);
    if (e == hipSuccess) e = hipHostMalloc((void **)&h->h_pmb, kSampleSlots * chunk * sizeof(double), hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostMalloc((void **)&h->h_pmy, kSampleSlots * chunk * sizeof(double), hipHostMallocDefault);
    if (e != hipSuccess) {
        multiply_release(h);
        return fail(h, EKF_ERR_HIP, "multiply_map: the chunks and the partial blocks could not be allocated; nothing was changed", e);
    }
    h->pm_rows = rows;
    h->pm_bytes = (int64_t)dev_bytes;
    h->bytes += h->pm_bytes;
    return EKF_OK;
}

// One chunk of the scratch as the launches take it (after multiply_alloc for `rows` and the flush: N and h->cur are final): the vectors at the
// front, their products behind them, then the partial blocks.  ekf_observe_dense (host/dense_obs.h) runs the same two launches on it.
MultiplyMapArgs multiply_chunk_args(const ekf_handle *h, int64_t rows) {
    const TileMap &tm = h->st.tm;
    MultiplyMapArgs a = {};
    double *d_b = h->d_pmul, *d_y = d_b + sample_chunk_doubles(h->pm_rows), *d_part = d_y + sample_chunk_doubles(h->pm_rows);
    int64_t toff = 0, woff = 0;
    multiply_partial_offsets(tm, rows, &toff, &woff);
    a.b = d_b; a.y = d_y; a.dpart = d_part; a.tpart = d_part + toff; a.wpart = d_part + woff;
    a.ld = sample_ld(rows); a.N = h->N; a.rows = rows; a.S = multiply_segment(tm.T); a.cur = h->cur;
    return a;
}

// Order as in factor_body: the rungs, with what depends on N checked once N is exact -> every allocation -> the flush -> the launches,
// queued back to back by chunk_stream (host/factor_map.h): per chunk the upload of a pinned slot, the two launches and the download into
// a pinned slot.  `queued` is set once the launches begin: out is written only from there on.
int32_t multiply_body(ekf_handle *h, const std::string &who, const double *B, int64_t k, double *out, bool &queued) {
    TRY(edit_unsharded(h, who, "the product reads every tile of the lower triangle, and every shard holds only its own tiles"));
    TRY(edit_settled(h, who));
    const int64_t N = h->N, n = 3 + 2 * N;                 // (N is exact only now)
    for (int64_t i = 0; i < k * n; ++i) REQUIRE(h, std::isfinite(B[i]), EKF_ERR_INVALID_ARG, (who + "B is not finite").c_str());
    const TileMap &tm = h->st.tm;
    const int64_t rows = tm.padded(2 * N);
    TRY(multiply_alloc(h, rows));
    TRY(edit_flushed(h));
    const MultiplyMapArgs a = multiply_chunk_args(h, rows);
    queued = true;
    // timed by family: the tile pass under EKF_KERNEL_ASSOCIATE, the sums under EKF_KERNEL_COMPACT (both free in this call)
    TRY(chunk_stream(h, h->h_pmb, h->h_pmy, h->ev_pmslot, h->d_pmul, a.y, rows, N, B, k, out, [&]() -> int32_t {
        if (N > 0) TIMED(h, EKF_KERNEL_ASSOCIATE, launch_multiply_map(h->st, a, 0, h->storage, h->stream));
        TIMED(h, EKF_KERNEL_COMPACT, launch_multiply_map(h->st, a, 1, h->storage, h->stream));
        return EKF_OK;
    }));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    chunk_stream_tail(h->h_pmy, rows, N, k, out);
    return EKF_OK;
}
}  // namespace

extern "C" {
int32_t ekf_multiply_map(ekf_handle *h, const double *B, int64_t k, double *out) {
    if (!h) return EKF_ERR_INVALID_ARG;
    const std::string who = "multiply_map: ";
    REQUIRE(h, B != nullptr, EKF_ERR_INVALID_ARG, (who + "null B").c_str());
    REQUIRE(h, out != nullptr, EKF_ERR_INVALID_ARG, (who + "null out").c_str());
    REQUIRE(h, k >= 1, EKF_ERR_INVALID_ARG, (who + "k is at least 1 vector").c_str());
    // no half-written products: a call that fails once its launches have begun (EKF_ERR_HIP) leaves every entry of out NaN; a refusal
    // before that leaves out untouched
    bool queued = false;
    const int32_t rc = multiply_body(h, who, B, k, out, queued);
    if (rc != EKF_OK && queued)
        for (int64_t i = 0; i < k * (3 + 2 * h->N); ++i) out[i] = NAN;
    return rc;
}
}  // extern "C"
