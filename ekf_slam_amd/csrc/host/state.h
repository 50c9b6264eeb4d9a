// Fragment of abi.hip, state I/O: reading and replacing x, s and P, the low-rank load, checkpoints, the digest.
#pragma once
namespace {
// the tail of the getters / setters that run on a temporary device buffer: wait for the stream, report the first failure as `what`
int32_t synced(ekf_handle *h, hipError_t e, const char *what) {
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    return e == hipSuccess ? EKF_OK : fail(h, EKF_ERR_HIP, what, e);
}
}  // namespace

extern "C" {
int32_t ekf_get_x(ekf_handle *h, double *x) {
    if (!h || !x) return fail(h, EKF_ERR_INVALID_ARG, "get_x: null argument");
    TRY(enter(h));
    HIPCHK(h, hipMemcpyAsync(x, h->st.x[h->cur], (size_t)(3 + n_mm(h)) * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return EKF_OK;
}

int32_t ekf_set_x(ekf_handle *h, const double *x, int64_t n) {
    if (!h || !x) return fail(h, EKF_ERR_INVALID_ARG, "set_x: null argument");
    REQUIRE(h, n >= 3 && (n - 3) % 2 == 0 && (n - 3) / 2 <= h->cap, EKF_ERR_INVALID_ARG, "set_x: bad length");
    TRY(enter_flushed(h));     // pending pairs belong to the old state
    if ((n - 3) / 2 < h->N) HIPCHK(h, clear_pairs(h));      // shrinking the map
    map_replaced(h);           // a prefetch belongs to the state it was taken from
    h->N = (n - 3) / 2;
    h->s_host.resize((size_t)h->N, 0.0);
    HIPCHK(h, hipMemcpyAsync(h->st.x[h->cur], x, (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return EKF_OK;
}

int32_t ekf_get_s(ekf_handle *h, double *s) {
    if (!h || (!s && h->N > 0)) return fail(h, EKF_ERR_INVALID_ARG, "get_s: null argument");
    TRY(enter(h));
    if (h->N > 0) HIPCHK(h, hipMemcpyAsync(s, h->st.s, (size_t)h->N * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return EKF_OK;
}

int32_t ekf_set_s(ekf_handle *h, const double *s, int64_t N) {
    if (!h || (!s && N > 0)) return fail(h, EKF_ERR_INVALID_ARG, "set_s: null argument");
    REQUIRE(h, N == h->N, EKF_ERR_INVALID_ARG, "set_s: length must equal the number of landmarks (set x first)");
    TRY(enter(h));
    if (N > 0) HIPCHK(h, hipMemcpyAsync(h->st.s, s, (size_t)N * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->s_host.assign(s, s + N);
    h->s_sorted_ok = false;
    return EKF_OK;
}

int32_t ekf_diag_poke_device_signature(ekf_handle *h, int64_t idx, double value) {
    if (!h) return EKF_ERR_INVALID_ARG;
    REQUIRE(h, idx >= 0 && idx < h->N, EKF_ERR_INVALID_ARG, "diag_poke_device_signature: no such landmark");
    TRY(enter(h));
    HIPCHK(h, hipMemcpyAsync(h->st.s + idx, &value, 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));      // (`value` is this call's stack)
    return EKF_OK;
}

int32_t ekf_get_P(ekf_handle *h, double *P) {
    if (!h || !P) return fail(h, EKF_ERR_INVALID_ARG, "get_P: null argument");
    TRY(enter_flushed(h));
    const int64_t n = 3 + n_mm(h);
    double *dense = nullptr;  DevTemp tmp(&dense);
    HIPCHK(h, hipMalloc((void **)&dense, (size_t)(n * n) * 8));
    hipError_t e = launch_unpack_dense(h->st, h->cur, n_mm(h), dense, h->storage, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(P, dense, (size_t)(n * n) * 8, hipMemcpyDeviceToHost, h->stream);
    return synced(h, e, "get_P");
}

int32_t ekf_set_P(ekf_handle *h, const double *P, int64_t n) {
    if (!h || !P) return fail(h, EKF_ERR_INVALID_ARG, "set_P: null argument");
    REQUIRE(h, n == 3 + n_mm(h), EKF_ERR_INVALID_ARG, "set_P: n must equal length(x) (set x first)");
    TRY(enter(h));
    TRY(retire_inflight(h));
    covariance_replaced(h);
    double *dense = nullptr;  DevTemp tmp(&dense);
    HIPCHK(h, hipMalloc((void **)&dense, (size_t)(n * n) * 8));
    hipError_t e = hipMemcpyAsync(dense, P, (size_t)(n * n) * 8, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = launch_pack_dense(h->st, h->cur, n_mm(h), dense, h->storage, h->stream);
    return synced(h, e, "set_P");
}

int32_t ekf_get_P_block(ekf_handle *h, int64_t r0, int64_t c0, int64_t nr, int64_t nc, double *out) {
    if (!h || !out) return fail(h, EKF_ERR_INVALID_ARG, "get_P_block: null argument");
    const int64_t n = 3 + n_mm(h);
    REQUIRE(h, r0 >= 0 && c0 >= 0 && nr >= 1 && nc >= 1 && r0 + nr <= n && c0 + nc <= n, EKF_ERR_INVALID_ARG,
            "get_P_block: block outside P");
    TRY(enter_flushed(h));
    double *d = nullptr;  DevTemp tmp(&d);
    HIPCHK(h, hipMalloc((void **)&d, (size_t)(nr * nc) * 8));
    hipError_t e = launch_get_block(h->st, h->cur, r0, c0, nr, nc, d, h->storage, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d, (size_t)(nr * nc) * 8, hipMemcpyDeviceToHost, h->stream);
    return synced(h, e, "get_P_block");
}

int32_t ekf_get_P_diag_blocks(ekf_handle *h, double *out) {
    if (!h || !out) return fail(h, EKF_ERR_INVALID_ARG, "get_P_diag_blocks: null argument");
    TRY(enter(h));
    // no pass over P: what plot() reads (EKF_SLAM.m:180,205) is the robot block and the landmarks' own 2x2 blocks, and both are live
    // (DevState::prr, DevState::diag carry every correction so far, pending or not)
    const size_t bytes = (size_t)(4 * (h->N + 1)) * 8;
    double *d = nullptr;  DevTemp tmp(&d);
    HIPCHK(h, hipMalloc((void **)&d, bytes));
    hipError_t e = launch_get_diag_blocks(h->st, h->cur, h->N, d, h->storage, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d, bytes, hipMemcpyDeviceToHost, h->stream);
    return synced(h, e, "get_P_diag_blocks");
}

int32_t ekf_get_Q(ekf_handle *h, double Q[9]) {
    if (!h || !Q) return fail(h, EKF_ERR_INVALID_ARG, "get_Q: null argument");
    TRY(enter(h));
    HIPCHK(h, hipMemcpyAsync(h->h_small, h->st.small, 32 * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) Q[c * 3 + r] = h->h_small[12 + 3 * r + c];
    return EKF_OK;
}

int32_t ekf_load_lowrank_state(ekf_handle *h, int64_t N, const double *x, const double *s, const double *d,
                               const double *U, int64_t k) {
    if (!h || !x || !s || !d || !U) return fail(h, EKF_ERR_INVALID_ARG, "load_lowrank_state: null argument");
    REQUIRE(h, N >= 0 && N <= h->cap && k >= 1, EKF_ERR_INVALID_ARG, "load_lowrank_state: bad N or k");
    TRY(enter(h));
    const int64_t n = 3 + 2 * N;
    TRY(retire_inflight(h));      // (before clear_pairs: the pass reads the pair ring)
    if (N < h->N) HIPCHK(h, clear_pairs(h));
    map_replaced(h);
    covariance_replaced(h);
    h->N = N;
    h->s_host.assign(s, s + N);
    TRY(refresh_work(h));
    double *dd = nullptr, *dU = nullptr;  DevTemp tmp_d(&dd), tmp_U(&dU);
    HIPCHK(h, hipMalloc((void **)&dd, (size_t)n * 8));
    hipError_t e = hipMalloc((void **)&dU, (size_t)(n * k) * 8);
    if (e == hipSuccess) e = hipMemcpyAsync(dd, d, (size_t)n * 8, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dU, U, (size_t)(n * k) * 8, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(h->st.x[h->cur], x, (size_t)n * 8, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess && N > 0) e = hipMemcpyAsync(h->st.s, s, (size_t)N * 8, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = launch_lowrank(h->st, h->cur, 2 * N, h->ws[h->ws_cur].work, h->ws[h->ws_cur].nwork, dd, dU, k, h->storage, h->stream);
    return synced(h, e, "load_lowrank_state");
}
}  // extern "C"

namespace {
struct CkptHeader {
    char magic[8];
    int64_t N;
    int32_t tile, storage, world, rank;
    int64_t tile_bytes;      // bytes of the tile section
    int64_t reserved[3];
};
static_assert(sizeof(CkptHeader) == 64, "checkpoint header is 64 bytes");

// device -> file / file -> device through a bounded pinned staging buffer
int32_t stream_out(ekf_handle *h, FILE *f, const void *dev, size_t bytes, void *stage, size_t stage_bytes) {
    const char *p = (const char *)dev;
    while (bytes) {
        const size_t n = bytes < stage_bytes ? bytes : stage_bytes;
        HIPCHK(h, hipMemcpyAsync(stage, p, n, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (fwrite(stage, 1, n, f) != n) return fail(h, EKF_ERR_STATE, "checkpoint: short write");
        p += n; bytes -= n;
    }
    return EKF_OK;
}
int32_t stream_in(ekf_handle *h, FILE *f, void *dev, size_t bytes, void *stage, size_t stage_bytes) {
    char *p = (char *)dev;
    while (bytes) {
        const size_t n = bytes < stage_bytes ? bytes : stage_bytes;
        if (fread(stage, 1, n, f) != n) return fail(h, EKF_ERR_STATE, "checkpoint: short read");
        HIPCHK(h, hipMemcpyAsync(p, stage, n, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        p += n; bytes -= n;
    }
    return EKF_OK;
}
}  // namespace

extern "C" {
int32_t ekf_checkpoint_save(ekf_handle *h, const char *path) {
    if (!h || !path) return fail(h, EKF_ERR_INVALID_ARG, "checkpoint_save: null argument");
    TRY(enter_flushed(h));
    FILE *f = fopen(path, "wb");
    REQUIRE(h, f != nullptr, EKF_ERR_STATE, "checkpoint_save: cannot open the file for writing");
    const size_t stage_bytes = (size_t)32 << 20;
    void *stage = nullptr;
    if (hipHostMalloc(&stage, stage_bytes, hipHostMallocDefault) != hipSuccess) { fclose(f); return fail(h, EKF_ERR_HIP, "checkpoint: staging buffer"); }
    const int64_t nmm = n_mm(h), nt = ekf_tiles_for(nmm, h->T);
    CkptHeader hd;
    memset(&hd, 0, sizeof hd);
    memcpy(hd.magic, "EKFSLAM2", 8);
    hd.N = h->N; hd.tile = h->T; hd.storage = h->storage; hd.world = h->cfg.world; hd.rank = h->cfg.rank;
    hd.tile_bytes = h->st.tm.slots_for_rows(nt) * (int64_t)h->T * h->T * (int64_t)elt_size(h);
    int32_t rc = fwrite(&hd, sizeof hd, 1, f) == 1 ? EKF_OK : fail(h, EKF_ERR_STATE, "checkpoint: short write");
    if (!rc) rc = stream_out(h, f, h->st.x[h->cur], (size_t)(3 + nmm) * 8, stage, stage_bytes);
    if (!rc && h->N > 0) rc = stream_out(h, f, h->st.s, (size_t)h->N * 8, stage, stage_bytes);
    if (!rc) rc = stream_out(h, f, h->st.prr[h->cur], 9 * 8, stage, stage_bytes);
    for (int r = 0; r < 3 && !rc && nmm > 0; ++r)
        rc = stream_out(h, f, h->st.strip[h->cur] + (size_t)r * h->st.ldm, (size_t)nmm * 8, stage, stage_bytes);
    if (!rc && h->N > 0) rc = stream_out(h, f, h->st.diag[h->st.dcur], (size_t)(3 * h->N) * 8, stage, stage_bytes);
    if (!rc && hd.tile_bytes > 0) rc = stream_out(h, f, h->st.tiles, (size_t)hd.tile_bytes, stage, stage_bytes);
    hipHostFree(stage);
    if (fclose(f) != 0 && !rc) rc = fail(h, EKF_ERR_STATE, "checkpoint: close failed");
    return rc;
}

int32_t ekf_checkpoint_load(ekf_handle *h, const char *path) {
    if (!h || !path) return fail(h, EKF_ERR_INVALID_ARG, "checkpoint_load: null argument");
    TRY(enter(h));
    FILE *f = fopen(path, "rb");
    REQUIRE(h, f != nullptr, EKF_ERR_STATE, "checkpoint_load: cannot open the file");
    void *stage = nullptr;
    // every exit below goes through here: the file is closed and the staging buffer released whatever happened
    auto done = [&](int32_t status) { if (stage) hipHostFree(stage); fclose(f); return status; };
    CkptHeader hd;
    if (fread(&hd, sizeof hd, 1, f) != 1) return done(fail(h, EKF_ERR_STATE, "checkpoint_load: not an EKFSLAM2 file"));
    if (memcmp(hd.magic, "EKFSLAM1", 8) == 0)
        return done(fail(h, EKF_ERR_STATE, "checkpoint_load: EKFSLAM1 file -- that format (no section for the landmarks' live diagonal "
                                           "blocks) is no longer read; re-save the state with this library (INTEGRATION.md, checkpoints)"));
    if (memcmp(hd.magic, "EKFSLAM2", 8) != 0) return done(fail(h, EKF_ERR_STATE, "checkpoint_load: not an EKFSLAM2 file"));
    if (hd.tile != h->T || hd.storage != h->storage || hd.world != h->cfg.world || hd.rank != h->cfg.rank || hd.N < 0 || hd.N > h->cap)
        return done(fail(h, EKF_ERR_STATE, "checkpoint_load: tile edge, storage, shard or capacity do not match this handle"));
    const int64_t nmm = 2 * hd.N, nt = ekf_tiles_for(nmm, h->T);
    if (hd.tile_bytes != h->st.tm.slots_for_rows(nt) * (int64_t)h->T * h->T * (int64_t)elt_size(h))
        return done(fail(h, EKF_ERR_STATE, "checkpoint_load: tile section size mismatch"));
    // the whole payload must be there BEFORE any device state is overwritten: a truncated file leaves the handle as it was
    const int64_t payload = (3 + nmm) * 8 + hd.N * 8 + 9 * 8 + 3 * nmm * 8 + 3 * hd.N * 8 + hd.tile_bytes;
    if (fseek(f, 0, SEEK_END) != 0) return done(fail(h, EKF_ERR_STATE, "checkpoint_load: cannot seek"));
    const long fsize = ftell(f);
    if (fsize < 0 || (int64_t)fsize != (int64_t)sizeof hd + payload)
        return done(fail(h, EKF_ERR_STATE, "checkpoint_load: file length does not match its header (truncated?)"));
    if (fseek(f, (long)sizeof hd, SEEK_SET) != 0) return done(fail(h, EKF_ERR_STATE, "checkpoint_load: cannot seek"));
    const size_t stage_bytes = (size_t)32 << 20;
    if (hipHostMalloc(&stage, stage_bytes, hipHostMallocDefault) != hipSuccess) { stage = nullptr; return done(fail(h, EKF_ERR_HIP, "checkpoint: staging buffer")); }
    int32_t rc = retire_inflight(h);
    if (rc) return done(rc);
    covariance_replaced(h);
    h->have_pp = false;          // (only here, and a no-op: enter() above has carried a recorded predict out)
    hipError_t e = clear_pairs(h);
    if (e != hipSuccess) return done(fail(h, EKF_ERR_HIP, "checkpoint_load: clearing the pending pairs", e));
    std::vector<double> shost((size_t)hd.N);
    rc = stream_in(h, f, h->st.x[h->cur], (size_t)(3 + nmm) * 8, stage, stage_bytes);
    if (!rc && hd.N > 0) {
        const long at = ftell(f);
        rc = stream_in(h, f, h->st.s, (size_t)hd.N * 8, stage, stage_bytes);
        if (!rc) { fseek(f, at, SEEK_SET); if (fread(shost.data(), 8, (size_t)hd.N, f) != (size_t)hd.N) rc = fail(h, EKF_ERR_STATE, "checkpoint: short read"); }
    }
    if (!rc) rc = stream_in(h, f, h->st.prr[h->cur], 9 * 8, stage, stage_bytes);
    for (int r = 0; r < 3 && !rc && nmm > 0; ++r)
        rc = stream_in(h, f, h->st.strip[h->cur] + (size_t)r * h->st.ldm, (size_t)nmm * 8, stage, stage_bytes);
    if (!rc && hd.N > 0) rc = stream_in(h, f, h->st.diag[h->st.dcur], (size_t)(3 * hd.N) * 8, stage, stage_bytes);
    if (!rc && hd.tile_bytes > 0) rc = stream_in(h, f, h->st.tiles, (size_t)hd.tile_bytes, stage, stage_bytes);
    // N follows x even when a later section failed (an I/O error mid-way): x and N must never disagree
    h->N = hd.N;
    h->s_host = shost;
    map_replaced(h);
    h->ws[h->ws_cur].rows = -1;  // (no pass is in flight: the newest set is rebuilt in place)
    return done(rc);
}

int32_t ekf_P_digest(ekf_handle *h, double out[3]) {
    if (!h || !out) return fail(h, EKF_ERR_INVALID_ARG, "P_digest: null argument");
    TRY(enter_flushed(h));
    TRY(refresh_work(h));
    HIPCHK(h, launch_digest(h->st, h->cur, n_mm(h), h->ws[h->ws_cur].work, h->ws[h->ws_cur].nwork, h->d_digest, h->storage, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->h_small, h->d_digest, 3 * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    out[0] = h->h_small[0]; out[1] = h->h_small[1]; out[2] = h->h_small[2];
    return EKF_OK;
}
}  // extern "C"
