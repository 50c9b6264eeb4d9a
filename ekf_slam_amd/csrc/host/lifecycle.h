// Fragment of abi.hip, the life of a handle: ekf_create (checks, stream, geometry, then one step per family), ekf_destroy, the kernel timers.
#pragma once
namespace {
// ekf_create, the state's part: x / Prr / strip / diag in two buffers, s, the small outputs; x = [0 0 0], P = 0.1*eye(3)
// (EKF_SLAM.m:28-31, EKF_SLAM_UC.m:29-32)
int32_t create_state(ekf_handle *h) {
    const int64_t ldm = h->st.ldm;
    for (int b = 0; b < 2; ++b) {
        HIPCHK(h, dalloc(h, &h->st.x[b], (size_t)(3 + ldm)));
        HIPCHK(h, dalloc(h, &h->st.prr[b], 16));
        HIPCHK(h, dalloc(h, &h->st.strip[b], (size_t)(3 * ldm)));
        HIPCHK(h, dalloc(h, &h->st.diag[b], (size_t)(3 * h->cap)));       // live F64 copies of the 2x2 diagonal blocks (kernels.h)
    }
    h->st.dcur = 0;
    HIPCHK(h, dalloc(h, &h->st.s, (size_t)h->cap));
    HIPCHK(h, dalloc(h, &h->st.small, 32));
    HIPCHK(h, dalloc(h, &h->d_digest, kDigestDoubles));
    HIPCHK(h, dalloc(h, &h->d_csmall, 16));
    HIPCHK(h, halloc(h, &h->h_small, 32 * sizeof(double), hipHostMallocDefault));
    const double prr0[9] = { 0.1, 0, 0, 0, 0.1, 0, 0, 0, 0.1 };
    HIPCHK(h, hipMemcpy(h->st.prr[0], prr0, sizeof prr0, hipMemcpyHostToDevice));
    h->cur = 0;
    h->N = 0;
    return EKF_OK;
}
}  // namespace

extern "C" {
int32_t ekf_create(const ekf_config *cfg, ekf_handle **out) {
    if (!cfg || !out) return EKF_ERR_INVALID_ARG;
    *out = nullptr;
    const int32_t T = cfg->tile == 0 ? (cfg->storage == EKF_STORE_F32 ? 256 : 128) : cfg->tile;
    const int32_t world = cfg->world <= 0 ? 1 : cfg->world;
    if (!(T == 16 || T == 32 || T == 64 || T == 128 || (T == 256 && cfg->storage == EKF_STORE_F32))) return EKF_ERR_INVALID_ARG;
    if (cfg->capacity_landmarks < 1 || cfg->rank < 0 || cfg->rank >= world) return EKF_ERR_INVALID_ARG;
    if (cfg->storage != EKF_STORE_F64 && cfg->storage != EKF_STORE_F32) return EKF_ERR_INVALID_ARG;
    if (cfg->mode != EKF_MODE_KNOWN && cfg->mode != EKF_MODE_UC) return EKF_ERR_INVALID_ARG;
    if (cfg->batch < 0 || cfg->batch > 64) return EKF_ERR_INVALID_ARG;
    // the device-decided branch runs unsharded only (its sharded form is not built)
    if (cfg->mode == EKF_MODE_UC && cfg->device_assoc == 4 && (world > 1 || cfg->force_sharded)) return EKF_ERR_INVALID_ARG;
    if (cfg->pass_arith != EKF_ARITH_F64 &&
        !((cfg->pass_arith == EKF_ARITH_F32 || cfg->pass_arith == EKF_ARITH_SPLIT3) && cfg->storage == EKF_STORE_F32 && T == 256))
        return EKF_ERR_INVALID_ARG;                   // the f32-arithmetic passes exist for float tiles of edge 256 only
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device < 0 || cfg->device >= ndev)
        return EKF_ERR_NO_DEVICE;

    ekf_handle *h = new (std::nothrow) ekf_handle();
    if (!h) return EKF_ERR_INVALID_ARG;
    h->cfg = *cfg;
    h->cfg.world = world;
    h->cfg.tile = T;
    h->T = T;
    h->cap = cfg->capacity_landmarks;
    h->storage = cfg->storage;
    *out = h;   // returned even on failure so the caller can read ekf_last_error, then ekf_destroy

    HIPCHK(h, hipSetDevice(cfg->device));
    hipDeviceProp_t prop = {};                    // the one query, for the two consumers in create_passes
    if (cfg->async_flush != 0 || cfg->pass_arith != EKF_ARITH_F64) HIPCHK(h, hipGetDeviceProperties(&prop, cfg->device));
    {
        // the main stream carries the latency-bound step kernels: highest priority, so that their few workgroups are
        // dispatched ahead of the tens of thousands a concurrent flush (own stream, lowest priority) has queued
        int lo = 0, hi = 0;
        HIPCHK(h, hipDeviceGetStreamPriorityRange(&lo, &hi));
        HIPCHK(h, hipStreamCreateWithPriority(&h->own_stream, hipStreamNonBlocking, hi));
    }
    h->stream = h->own_stream;
    const int64_t nt_cap = ekf_tiles_for(2 * h->cap, T);
    h->st.ldm = nt_cap * T;
    h->st.tm = ekf_make_tilemap(T, world, cfg->rank);
    h->work_cap = h->st.tm.slots_for_rows(nt_cap);

    TRY(create_state(h));
    TRY(create_passes(h, prop));
    TRY(create_worklists(h));
    TRY(create_assoc(h));
    TRY(create_exchange(h));
    TRY(create_decided(h));
    TRY(create_linear(h));
    TRY(create_model_iter(h));
    TRY(create_assoc_model(h));
    TRY(create_assign_model(h));
    TRY(create_model_assigned(h));
    TRY(create_joint(h));
    HIPCHK(h, hipDeviceSynchronize());      // dalloc clears on the null stream, which the handle's (non-blocking) streams do not wait for
    return EKF_OK;
}

int32_t ekf_destroy(ekf_handle *h) {
    if (!h) return EKF_OK;
    hipSetDevice(h->cfg.device);
    if (h->stream) hipStreamSynchronize(h->stream);
    if (h->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(h->comm);
    for (hipStream_t s : { h->flush_stream, h->xchg_stream }) if (s) { hipStreamSynchronize(s); hipStreamDestroy(s); }
    for (hipEvent_t e : h->events) hipEventDestroy(e);
    for (auto &t : h->timers) for (hipEvent_t e : t.ev) hipEventDestroy(e);
    for (void *p : h->allocs) hipFree(p);
    for (void *p : { (void *)h->d_ftiles, (void *)h->d_fsmall, (void *)h->d_fsample, (void *)h->d_fsolve, (void *)h->d_pmul, (void *)h->d_dpart }) if (p) hipFree(p);   // ekf_factor_map's, ekf_sample_map's and ekf_solve_map's scratch (host/factor_map.h), ekf_multiply_map's (host/multiply_map.h), ekf_observe_dense's partial sums (host/dense_obs.h)
    for (void *p : { (void *)h->h_fres, (void *)h->h_fref, (void *)h->h_fxi, (void *)h->h_fy, (void *)h->h_pmb, (void *)h->h_pmy }) if (p) hipHostFree(p);
    for (void *p : h->pinned) hipHostFree(p);
    if (h->own_stream) hipStreamDestroy(h->own_stream);
    delete h;
    return EKF_OK;
}

int32_t ekf_kernel_timing_enable(ekf_handle *h, int32_t which, int32_t on) {
    if (!h || which < 0 || which >= EKF_KERNEL_COUNT) return fail(h, EKF_ERR_INVALID_ARG, "kernel_timing_enable: bad kernel id");
    TRY(use_device(h));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    KernelTimer &t = h->timers[which];
    if (on) {
        // create the event pool now: hipEventCreate inside a timed region costs tens of microseconds per launch
        const size_t reserve = on > 512 ? (size_t)on : 512;
        while (t.ev.size() < 2 * reserve) {
            hipEvent_t e;
            HIPCHK(h, hipEventCreate(&e));
            t.ev.push_back(e);
        }
    }
    t.enabled = on != 0;
    t.used = 0;
    return EKF_OK;
}

int32_t ekf_kernel_timing_read(ekf_handle *h, int32_t which, int64_t *launches, double *total_ms) {
    if (!h || which < 0 || which >= EKF_KERNEL_COUNT || !launches || !total_ms)
        return fail(h, EKF_ERR_INVALID_ARG, "kernel_timing_read: bad argument");
    TRY(use_device(h));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (h->flush_stream) HIPCHK(h, hipStreamSynchronize(h->flush_stream));
    KernelTimer &t = h->timers[which];
    double tot = 0.0;
    for (size_t i = 0; i + 1 < t.used; i += 2) {
        float ms = 0.f;
        HIPCHK(h, hipEventElapsedTime(&ms, t.ev[i], t.ev[i + 1]));
        tot += ms;
    }
    *launches = (int64_t)(t.used / 2);
    *total_ms = tot;
    t.used = 0;
    return EKF_OK;
}
}  // extern "C"
