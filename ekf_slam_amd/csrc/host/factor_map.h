// Fragment of abi.hip, the factorisation of P (ekf_factor_map): is the matrix this handle carries still a covariance, what is its log
// determinant, and what is the normalised estimation error squared of x against up to eight reference states -- one Cholesky factorisation
// of exactly what ekf_get_P would report, in a scratch store of its own.  A SYNCHRONISING, READ-ONLY call on the rungs of host/edits.h, as
// ekf_nearest_landmarks: a recorded predict carried out, the pending pairs applied, an asynchronous pass retired; x, s, P, the diagonal
// copies and the digest are afterwards those of a handle that only flushed.  No invalidation function is called and nothing is kept
// between calls: every call factors.  Unsharded only: the load reads every tile, and a shard holds only its own.
// ekf_sample_map is the same factorisation (factor_run below is the body of both) with the draws x + C xi queued behind it, a chunk of
// factor_chunk() draws at a time through pinned staging that does not grow with the number of draws.
// ekf_solve_map is the same body again with the other direction queued behind the factorisation: C^-1 B or P^-1 B for the caller's k
// right-hand sides, through the same chunks, slots and events.
#pragma once
namespace {
constexpr int kSampleSlots = 4;            // chunks of pinned staging per direction (ekf_handle::ev_fslot)

void factor_release(ekf_handle *h) {
    if (h->d_ftiles) hipFree(h->d_ftiles);
    if (h->d_fsmall) hipFree(h->d_fsmall);
    if (h->h_fres) hipHostFree(h->h_fres);
    if (h->h_fref) hipHostFree(h->h_fref);
    h->d_ftiles = h->d_fsmall = h->h_fres = h->h_fref = nullptr;
    h->bytes -= h->f_bytes;
    h->f_bytes = 0;
    h->f_rows = -1;
    // the draws' part
    if (h->d_fsample) hipFree(h->d_fsample);
    if (h->h_fxi) hipHostFree(h->h_fxi);
    if (h->h_fy) hipHostFree(h->h_fy);
    h->d_fsample = h->h_fxi = h->h_fy = nullptr;
    h->bytes -= h->fs_bytes;
    h->fs_bytes = 0;
    h->fs_rows = -1;
    // the solves' part
    if (h->d_fsolve) hipFree(h->d_fsolve);
    h->d_fsolve = nullptr;
    h->bytes -= h->fv_bytes;
    h->fv_bytes = 0;
    h->fv_rows = -1;
}

// doubles of the second allocation for `rows` rows: the right-hand sides, the result block and the pivots, the reference states, L_r's
// entries below the diagonal (three, and one of padding)
size_t factor_rhs_doubles(int64_t rows) { return (size_t)rows * kFactorRhs; }
size_t factor_res_doubles(int64_t rows) { return (size_t)kFactorRes + (size_t)rows; }
size_t factor_ref_doubles(int64_t rows) { return (size_t)kFactorRefMax * (size_t)(3 + rows); }
constexpr size_t kFactorTailDoubles = 4;
// a chunk of draws or of samples: factor_chunk() columns of rows + 3 entries and one of padding
int64_t sample_ld(int64_t rows) { return rows + 4; }
size_t sample_chunk_doubles(int64_t rows) { return (size_t)sample_ld(rows) * (size_t)factor_chunk(); }

// THE CHUNK PIPELINE of ekf_sample_map, ekf_solve_map (factor_body below) and ekf_multiply_map (host/multiply_map.h): the k vectors of
// `src`, rows of n = 3 + 2 N entries in x's order, a chunk of factor_chunk() at a time.  A vector is a COLUMN of its chunk with the
// landmark part first (`rows` entries, zero from 2 N on) and the robot's three behind it; a partial last chunk is zero-padded.  Per chunk:
// a pinned slot of in_slots zeroed, packed and uploaded to d_in, launch_chunk() -- the caller's launches for one chunk, which returns a
// status --, d_out downloaded into the slot of out_slots, that slot's event recorded.  The host waits only where it takes a slot again,
// kSampleSlots chunks later, for that slot's own download, and unpacks it into the rows of `out` then; the last kSampleSlots slots are
// left to chunk_stream_tail, after the caller's final synchronise.
void chunk_unpack(const double *out_slots, int64_t rows, int64_t N, int64_t k, double *out, int64_t j) {
    const int64_t C = factor_chunk(), ld = sample_ld(rows), n = 3 + 2 * N;
    const double *y = out_slots + (size_t)(j % kSampleSlots) * sample_chunk_doubles(rows);
    for (int64_t c = 0; c < C && j * C + c < k; ++c) {
        double *o = out + (j * C + c) * n;
        std::memcpy(o, y + c * ld + rows, 3 * sizeof(double));
        std::memcpy(o + 3, y + c * ld, (size_t)(2 * N) * sizeof(double));
    }
}

template <typename F>
int32_t chunk_stream(ekf_handle *h, double *in_slots, double *out_slots, hipEvent_t *events, double *d_in, const double *d_out, int64_t rows,
                     int64_t N, const double *src, int64_t k, double *out, F launch_chunk) {
    const int64_t C = factor_chunk(), ld = sample_ld(rows), n = 3 + 2 * N, nchunks = (k + C - 1) / C;
    const size_t chunk = sample_chunk_doubles(rows);
    for (int64_t j = 0; j < nchunks; ++j) {
        const int slot = (int)(j % kSampleSlots);
        if (j >= kSampleSlots) {
            HIPCHK(h, hipEventSynchronize(events[slot]));
            chunk_unpack(out_slots, rows, N, k, out, j - kSampleSlots);
        }
        double *u = in_slots + (size_t)slot * chunk;
        std::memset(u, 0, chunk * sizeof(double));
        for (int64_t c = 0; c < C && j * C + c < k; ++c) {
            const double *row = src + (j * C + c) * n;
            std::memcpy(u + c * ld, row + 3, (size_t)(2 * N) * sizeof(double));
            std::memcpy(u + c * ld + rows, row, 3 * sizeof(double));
        }
        HIPCHK(h, hipMemcpyAsync(d_in, u, chunk * sizeof(double), hipMemcpyHostToDevice, h->stream));
        TRY(launch_chunk());
        HIPCHK(h, hipMemcpyAsync(out_slots + (size_t)slot * chunk, d_out, chunk * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipEventRecord(events[slot], h->stream));
    }
    return EKF_OK;
}

void chunk_stream_tail(const double *out_slots, int64_t rows, int64_t N, int64_t k, double *out) {
    const int64_t C = factor_chunk(), nchunks = (k + C - 1) / C;
    for (int64_t j = nchunks > kSampleSlots ? nchunks - kSampleSlots : 0; j < nchunks; ++j) chunk_unpack(out_slots, rows, N, k, out, j);
}

// The scratch for `rows` rows (a multiple of the factor store's tile edge), everything that can fail for lack of memory, before anything
// is queued.  Nothing is cleared (dalloc would clear on the null stream, which the handle's streams do not wait for): the launches write
// every byte that is read, and the result block is cleared in stream order.  Nothing of it is in use here: every call ends drained.
int32_t factor_alloc(ekf_handle *h, int64_t rows) {
    if (h->f_rows >= rows) return EKF_OK;
    factor_release(h);
    const int TF = factor_tile_edge();
    const TileMap tm = ekf_make_tilemap(TF, 1, 0);
    const int64_t slots = tm.row_base(rows / TF);
    const size_t tile_bytes = (size_t)(slots > 0 ? slots : 1) * TF * TF * sizeof(double);
    const size_t small_bytes = (factor_rhs_doubles(rows) + factor_res_doubles(rows) + factor_ref_doubles(rows) + kFactorTailDoubles) * sizeof(double);
    hipError_t e = hipMalloc((void **)&h->d_ftiles, tile_bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_fsmall, small_bytes);
    if (e == hipSuccess) e = hipHostMalloc((void **)&h->h_fres, factor_res_doubles(rows) * sizeof(double), hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostMalloc((void **)&h->h_fref, factor_ref_doubles(rows) * sizeof(double), hipHostMallocDefault);
    if (e != hipSuccess) {
        factor_release(h);
        return fail(h, EKF_ERR_HIP, "factor_map: the factor store could not be allocated; nothing was changed", e);
    }
    h->f_rows = rows;
    h->f_bytes = (int64_t)(tile_bytes + small_bytes);
    h->bytes += h->f_bytes;
    return EKF_OK;
}

// ... and what the draws need on top (after factor_alloc of the same call, which releases this part too when it grows): a chunk of
// draws, a chunk of samples, the partial blocks; the pinned slots; their events.  Its size depends on the rows alone, not on k.
int32_t sample_alloc(ekf_handle *h, int64_t rows) {
    for (hipEvent_t &ev : h->ev_fslot) if (!ev) HIPCHK(h, new_event(h, &ev));
    if (h->fs_rows >= rows) return EKF_OK;
    if (h->d_fsample) hipFree(h->d_fsample);
    if (h->h_fxi) hipHostFree(h->h_fxi);
    if (h->h_fy) hipHostFree(h->h_fy);
    h->d_fsample = h->h_fxi = h->h_fy = nullptr;
    h->bytes -= h->fs_bytes;
    h->fs_bytes = 0;
    h->fs_rows = -1;
    const size_t chunk = sample_chunk_doubles(rows), part = (size_t)factor_partial_doubles(rows);
    const size_t dev_bytes = (2 * chunk + (part ? part : 1)) * sizeof(double);
    hipError_t e = hipMalloc((void **)&h->d_fsample, dev_bytes);
    if (e == hipSuccess) e = hipHostMalloc((void **)&h->h_fxi, kSampleSlots * chunk * sizeof(double), hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostMalloc((void **)&h->h_fy, kSampleSlots * chunk * sizeof(double), hipHostMallocDefault);
    if (e != hipSuccess) {
        factor_release(h);
        return fail(h, EKF_ERR_HIP, "sample_map: the chunks of draws and samples could not be allocated; nothing was changed", e);
    }
    h->fs_rows = rows;
    h->fs_bytes = (int64_t)dev_bytes;
    h->bytes += h->fs_bytes;
    return EKF_OK;
}

// ... and what the solves need on top of both (after sample_alloc of the same call): the inverses of the diagonal tiles.
int32_t solve_alloc(ekf_handle *h, int64_t rows) {
    if (h->fv_rows >= rows) return EKF_OK;
    if (h->d_fsolve) hipFree(h->d_fsolve);
    h->d_fsolve = nullptr;
    h->bytes -= h->fv_bytes;
    h->fv_bytes = 0;
    h->fv_rows = -1;
    const size_t inv = (size_t)solve_inverse_doubles(rows);
    const size_t dev_bytes = (inv ? inv : 1) * sizeof(double);
    const hipError_t e = hipMalloc((void **)&h->d_fsolve, dev_bytes);
    if (e != hipSuccess) {
        factor_release(h);
        return fail(h, EKF_ERR_HIP, "solve_map: the inverses of the diagonal tiles could not be allocated; nothing was changed", e);
    }
    h->fv_rows = rows;
    h->fv_bytes = (int64_t)dev_bytes;
    h->bytes += h->fv_bytes;
    return EKF_OK;
}

// The body of ekf_factor_map, of ekf_sample_map and of ekf_solve_map (form < 0: the draws; form 0 / 1: xi is B, the right-hand sides,
// and out is P^-1 B / C^-1 B).  What follows speaks of ekf_sample_map (xi given: k draws, out their samples; ref is then NULL).  Order as in
// ekf_nearest_landmarks: the rungs, with what depends on N checked once N is exact -> every allocation -> the flush -> the launches, none
// waited for -> ONE readback (the result block and the pivots) -> the sums, on the host, in index order.  The draws go between the finish
// and the readback: per chunk the upload of a pinned slot, the two launches and the download into a pinned slot, queued back to back; the
// host waits only where it takes a slot again, kSampleSlots chunks later, for that slot's own download.  There is ONE chunk of draws and
// one of samples on the device and one stream, so the copies and the launches of successive chunks run one after another; the pinned
// slots take the host's packing and unpacking out of that line, nothing more.  `queued` is set once the launches begin: out is written
// only from there on (slots are unpacked into it before the status is known).
int32_t factor_body(ekf_handle *h, const std::string &who, const double *ref, int32_t nref, ekf_factor_info *info, double *d2, const double *xi,
                    int64_t k, double *out, int form, bool &queued) {
    TRY(edit_unsharded(h, who, "the factorisation reads and updates every tile of the lower triangle, and every shard holds only its own tiles"));
    TRY(edit_settled(h, who));
    const int64_t N = h->N, n = 3 + 2 * N;                 // (N is exact only now)
    for (int64_t i = 0; i < (int64_t)nref * n; ++i)
        REQUIRE(h, std::isfinite(ref[i]), EKF_ERR_INVALID_ARG, (who + "ref is not finite").c_str());
    if (xi)
        for (int64_t i = 0; i < k * n; ++i) REQUIRE(h, std::isfinite(xi[i]), EKF_ERR_INVALID_ARG, (who + (form < 0 ? "xi is not finite" : "B is not finite")).c_str());
    const int TF = factor_tile_edge();
    FactorMapArgs a = {};
    a.tm = ekf_make_tilemap(TF, 1, 0);
    a.N = N; a.rows = a.tm.padded(2 * N); a.nref = nref; a.ref_stride = n;
    TRY(factor_alloc(h, a.rows));
    if (xi) TRY(sample_alloc(h, a.rows));
    if (xi && form >= 0) TRY(solve_alloc(h, a.rows));
    TRY(edit_flushed(h));
    TRY(refresh_work(h));
    a.tiles = h->d_ftiles;
    a.rhs = h->d_fsmall;
    a.res = a.rhs + factor_rhs_doubles(h->f_rows);
    double *d_ref = a.res + factor_res_doubles(h->f_rows);
    a.ref = nref ? d_ref : nullptr;
    a.lr_off = xi ? d_ref + factor_ref_doubles(h->f_rows) : nullptr;
    a.cur = h->cur;
    queued = true;
    HIPCHK(h, hipMemsetAsync(a.res, 0, kFactorRes * sizeof(double), h->stream));
    if (nref) {
        std::memcpy(h->h_fref, ref, (size_t)nref * n * sizeof(double));
        HIPCHK(h, hipMemcpyAsync(d_ref, h->h_fref, (size_t)nref * n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    // timed by family: the load, the right-hand sides and the tail under EKF_KERNEL_COMPACT, the diagonal tiles and the panels under
    // EKF_KERNEL_GATHER, the trailing updates under EKF_KERNEL_DOWNDATE; the draws' apply pass under EKF_KERNEL_ASSOCIATE (free in this
    // call) and their sums under EKF_KERNEL_COMPACT; the solves' forward sweep of a chunk as ONE bracket under EKF_KERNEL_ASSOCIATE, its
    // backward sweep as one under EKF_KERNEL_APPEND (both free in this call), the inverses and the robot tail under EKF_KERNEL_COMPACT
    if (N > 0) TIMED(h, EKF_KERNEL_COMPACT, launch_factor_load(h->st, a, h->storage, h->stream));
    const int64_t nF = a.rows / TF;
    for (int64_t c = 0; c < nF; ++c) {
        {
            TimedLaunch tl(h, EKF_KERNEL_GATHER);
            HIPCHK(h, launch_factor_column(a, (int)c, 0, h->stream));
            HIPCHK(h, launch_factor_column(a, (int)c, 1, h->stream));
        }
        if (c + 1 < nF) TIMED(h, EKF_KERNEL_DOWNDATE, launch_factor_column(a, (int)c, 2, h->stream));
    }
    TIMED(h, EKF_KERNEL_COMPACT, launch_factor_finish(h->st, a, h->stream));
    // the draws: xi's rows permuted into elimination order as columns of a chunk on the way in, the samples permuted back into rows of
    // `out` on the way out (chunk_stream)
    if (xi) {
        const int64_t ld = sample_ld(a.rows);
        FactorSampleArgs sa = {};
        double *d_xi = h->d_fsample, *d_y = d_xi + sample_chunk_doubles(h->fs_rows);
        sa.xi = d_xi; sa.y = d_y; sa.part = d_y + sample_chunk_doubles(h->fs_rows); sa.ld = ld;
        FactorSolveArgs sv = {};
        sv.b = d_xi; sv.y = d_y; sv.inv = h->d_fsolve; sv.ld = ld; sv.form = form;
        if (form >= 0) TIMED(h, EKF_KERNEL_COMPACT, launch_solve_map(a, sv, 0, 0, h->stream));
        // P^-1 B is left in the chunk of right-hand sides, everything else in the chunk behind it
        TRY(chunk_stream(h, h->h_fxi, h->h_fy, h->ev_fslot, d_xi, form == 0 ? d_xi : d_y, a.rows, N, xi, k, out, [&]() -> int32_t {
            if (form < 0) {
                TIMED(h, EKF_KERNEL_ASSOCIATE, launch_factor_sample(h->st, a, sa, 0, h->stream));
                TIMED(h, EKF_KERNEL_COMPACT, launch_factor_sample(h->st, a, sa, 1, h->stream));
                return EKF_OK;
            }
            // the sweeps, sequential in the tile index: stream order is the only order between their workgroups
            {
                TimedLaunch tl(h, EKF_KERNEL_ASSOCIATE);
                for (int64_t c = 0; c < nF; ++c) HIPCHK(h, launch_solve_map(a, sv, 1, (int)c, h->stream));
            }
            TIMED(h, EKF_KERNEL_COMPACT, launch_solve_map(a, sv, 2, 0, h->stream));
            if (form == 0) {
                TimedLaunch tl(h, EKF_KERNEL_APPEND);
                for (int64_t c = nF - 1; c >= 0; --c) HIPCHK(h, launch_solve_map(a, sv, 3, (int)c, h->stream));
            }
            return EKF_OK;
        }));
    }
    HIPCHK(h, hipMemcpyAsync(h->h_fres, a.res, (kFactorRes + (size_t)(2 * N)) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    // the host's part: 2 sum log L_ii in index order (the landmark rows, then the robot), the smallest and largest pivot taken
    const double *res = h->h_fres, *piv = res + kFactorRes;
    const int status = (int)res[0];
    const int64_t taken_m = status == 1 ? (int64_t)res[1] - 3 : 2 * N;
    double sum = 0.0, lo = NAN, hi = NAN;
    auto take = [&](double l) {
        sum += std::log(l);
        const double p = l * l;
        if (!(lo <= p)) lo = p;
        if (!(hi >= p)) hi = p;
    };
    for (int64_t i = 0; i < taken_m; ++i) take(piv[i]);
    *info = ekf_factor_info();
    info->n = n;
    info->logdet_map = status == 1 ? NAN : 2.0 * sum;
    if (status != 1) for (int i = 0; i < (int)res[6]; ++i) take(res[3 + i]);
    info->definite = status == 0;
    info->bad_index = status == 0 ? -1 : (int64_t)res[1];
    info->bad_pivot = status == 0 ? 0.0 : res[2];
    info->logdet = status == 0 ? 2.0 * sum : NAN;
    info->min_pivot = lo;
    info->max_pivot = hi;
    for (int q = 0; q < nref; ++q) d2[q] = status == 0 ? res[8 + q] : NAN;
    // the samples of the last slots; where a pivot failed the launches returned at once and every entry is NaN
    if (xi && status == 0)
        chunk_stream_tail(h->h_fy, a.rows, N, k, out);
    else if (xi)
        for (int64_t i = 0; i < k * n; ++i) out[i] = NAN;
    return EKF_OK;
}

// ... and no half-written samples: a call that fails once its launches have begun (EKF_ERR_HIP) leaves every entry of out NaN, as a
// pivot that failed does; a refusal before that leaves out untouched.
int32_t factor_run(ekf_handle *h, const std::string &who, const double *ref, int32_t nref, ekf_factor_info *info, double *d2, const double *xi,
                   int64_t k, double *out, int form = -1) {
    bool queued = false;
    const int32_t rc = factor_body(h, who, ref, nref, info, d2, xi, k, out, form, queued);
    if (rc != EKF_OK && xi && queued)
        for (int64_t i = 0; i < k * (3 + 2 * h->N); ++i) out[i] = NAN;
    return rc;
}
}  // namespace

extern "C" {
int32_t ekf_factor_map(ekf_handle *h, const double *ref, int32_t nref, ekf_factor_info *info, double *d2) {
    if (!h) return EKF_ERR_INVALID_ARG;
    const std::string who = "factor_map: ";
    REQUIRE(h, info != nullptr, EKF_ERR_INVALID_ARG, (who + "null info").c_str());
    if (ref) {
        REQUIRE(h, nref >= 1 && nref <= kFactorRefMax, EKF_ERR_INVALID_ARG, (who + "nref is 1 to 8 reference states").c_str());
        REQUIRE(h, d2 != nullptr, EKF_ERR_INVALID_ARG, (who + "ref given without d2").c_str());
    } else
        nref = 0;
    return factor_run(h, who, ref, nref, info, d2, nullptr, 0, nullptr);
}

int32_t ekf_sample_map(ekf_handle *h, const double *xi, int64_t k, double *out, ekf_factor_info *info) {
    if (!h) return EKF_ERR_INVALID_ARG;
    const std::string who = "sample_map: ";
    REQUIRE(h, xi != nullptr, EKF_ERR_INVALID_ARG, (who + "null xi").c_str());
    REQUIRE(h, out != nullptr, EKF_ERR_INVALID_ARG, (who + "null out").c_str());
    REQUIRE(h, info != nullptr, EKF_ERR_INVALID_ARG, (who + "null info").c_str());
    REQUIRE(h, k >= 1, EKF_ERR_INVALID_ARG, (who + "k is at least 1 draw").c_str());
    return factor_run(h, who, nullptr, 0, info, nullptr, xi, k, out);
}

int32_t ekf_solve_map(ekf_handle *h, int32_t form, const double *B, int64_t k, double *out, ekf_factor_info *info) {
    if (!h) return EKF_ERR_INVALID_ARG;
    const std::string who = "solve_map: ";
    REQUIRE(h, B != nullptr, EKF_ERR_INVALID_ARG, (who + "null B").c_str());
    REQUIRE(h, out != nullptr, EKF_ERR_INVALID_ARG, (who + "null out").c_str());
    REQUIRE(h, info != nullptr, EKF_ERR_INVALID_ARG, (who + "null info").c_str());
    REQUIRE(h, k >= 1, EKF_ERR_INVALID_ARG, (who + "k is at least 1 right-hand side").c_str());
    REQUIRE(h, form == EKF_SOLVE_FULL || form == EKF_SOLVE_HALF, EKF_ERR_INVALID_ARG, (who + "form is EKF_SOLVE_FULL or EKF_SOLVE_HALF").c_str());
    return factor_run(h, who, nullptr, 0, info, nullptr, B, k, out, form);
}
}  // extern "C"
