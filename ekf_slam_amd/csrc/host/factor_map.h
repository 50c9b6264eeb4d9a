// Fragment of abi.hip, the factorisation of P (ekf_factor_map): is the matrix this handle carries still a covariance, what is its log
// determinant, and what is the normalised estimation error squared of x against up to eight reference states -- one Cholesky factorisation
// of exactly what ekf_get_P would report, in a scratch store of its own.  A SYNCHRONISING, READ-ONLY call on the rungs of host/edits.h, as
// ekf_nearest_landmarks: a recorded predict carried out, the pending pairs applied, an asynchronous pass retired; x, s, P, the diagonal
// copies and the digest are afterwards those of a handle that only flushed.  No invalidation function is called and nothing is kept
// between calls: every call factors.  Unsharded only: the load reads every tile, and a shard holds only its own.
#pragma once
namespace {
void factor_release(ekf_handle *h) {
    if (h->d_ftiles) hipFree(h->d_ftiles);
    if (h->d_fsmall) hipFree(h->d_fsmall);
    if (h->h_fres) hipHostFree(h->h_fres);
    if (h->h_fref) hipHostFree(h->h_fref);
    h->d_ftiles = h->d_fsmall = h->h_fres = h->h_fref = nullptr;
    h->bytes -= h->f_bytes;
    h->f_bytes = 0;
    h->f_rows = -1;
}

// doubles of the second allocation for `rows` rows: the right-hand sides, the result block and the pivots, the reference states
size_t factor_rhs_doubles(int64_t rows) { return (size_t)rows * kFactorRhs; }
size_t factor_res_doubles(int64_t rows) { return (size_t)kFactorRes + (size_t)rows; }
size_t factor_ref_doubles(int64_t rows) { return (size_t)kFactorRefMax * (size_t)(3 + rows); }

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
    const size_t small_bytes = (factor_rhs_doubles(rows) + factor_res_doubles(rows) + factor_ref_doubles(rows)) * sizeof(double);
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
}  // namespace

extern "C" {
// Order as in ekf_nearest_landmarks: arguments -> the rungs, with what depends on N checked once N is exact -> every allocation -> the
// flush -> the launches, none waited for -> ONE readback (the result block and the pivots) -> the sums, on the host, in index order.
int32_t ekf_factor_map(ekf_handle *h, const double *ref, int32_t nref, ekf_factor_info *info, double *d2) {
    if (!h) return EKF_ERR_INVALID_ARG;
    const std::string who = "factor_map: ";
    REQUIRE(h, info != nullptr, EKF_ERR_INVALID_ARG, (who + "null info").c_str());
    if (ref) {
        REQUIRE(h, nref >= 1 && nref <= kFactorRefMax, EKF_ERR_INVALID_ARG, (who + "nref is 1 to 8 reference states").c_str());
        REQUIRE(h, d2 != nullptr, EKF_ERR_INVALID_ARG, (who + "ref given without d2").c_str());
    } else
        nref = 0;
    TRY(edit_unsharded(h, who, "the factorisation reads and updates every tile of the lower triangle, and every shard holds only its own tiles"));
    TRY(edit_settled(h, who));
    const int64_t N = h->N, n = 3 + 2 * N;                 // (N is exact only now)
    for (int64_t i = 0; i < (int64_t)nref * n; ++i)
        REQUIRE(h, std::isfinite(ref[i]), EKF_ERR_INVALID_ARG, (who + "ref is not finite").c_str());
    const int TF = factor_tile_edge();
    FactorMapArgs a = {};
    a.tm = ekf_make_tilemap(TF, 1, 0);
    a.N = N; a.rows = a.tm.padded(2 * N); a.nref = nref; a.ref_stride = n;
    TRY(factor_alloc(h, a.rows));
    TRY(edit_flushed(h));
    TRY(refresh_work(h));
    a.tiles = h->d_ftiles;
    a.rhs = h->d_fsmall;
    a.res = a.rhs + factor_rhs_doubles(h->f_rows);
    double *d_ref = a.res + factor_res_doubles(h->f_rows);
    a.ref = nref ? d_ref : nullptr;
    a.cur = h->cur;
    HIPCHK(h, hipMemsetAsync(a.res, 0, kFactorRes * sizeof(double), h->stream));
    if (nref) {
        std::memcpy(h->h_fref, ref, (size_t)nref * n * sizeof(double));
        HIPCHK(h, hipMemcpyAsync(d_ref, h->h_fref, (size_t)nref * n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    // timed by family: the load, the right-hand sides and the tail under EKF_KERNEL_COMPACT, the diagonal tiles and the panels under
    // EKF_KERNEL_GATHER, the trailing updates under EKF_KERNEL_DOWNDATE
    if (N > 0) TIMED(h, EKF_KERNEL_COMPACT, launch_factor_load(h->st, a, h->storage, h->stream));
    const int64_t nF = a.rows / TF;
    for (int64_t k = 0; k < nF; ++k) {
        {
            TimedLaunch tl(h, EKF_KERNEL_GATHER);
            HIPCHK(h, launch_factor_column(a, (int)k, 0, h->stream));
            HIPCHK(h, launch_factor_column(a, (int)k, 1, h->stream));
        }
        if (k + 1 < nF) TIMED(h, EKF_KERNEL_DOWNDATE, launch_factor_column(a, (int)k, 2, h->stream));
    }
    TIMED(h, EKF_KERNEL_COMPACT, launch_factor_finish(h->st, a, h->stream));
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
    return EKF_OK;
}
}  // extern "C"
