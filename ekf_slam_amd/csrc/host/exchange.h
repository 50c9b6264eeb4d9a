// Fragment of abi.hip, a shard's exchange: the RCCL binding, where a contribution is sent from, the all-gather, ekf_exchange_* / ekf_comm_* / ekf_shard_*.
#pragma once
// RCCL is bound at run time (dlopen) so that single-GPU users never load it.
struct RcclApi {
    void *dl = nullptr;
    int (*GetUniqueId)(void *) = nullptr;
    int (*CommInitRank)(void **, int, ekf_comm_id, int) = nullptr;      // ncclUniqueId is 128 opaque bytes by value
    int (*AllGather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
};

static RcclApi g_rccl;

static bool rccl_load(std::string &err) {
    if (g_rccl.dl) return true;
    const char *names[] = { "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1" };
    void *dl = nullptr;
    for (const char *n : names) { dl = dlopen(n, RTLD_NOW | RTLD_GLOBAL); if (dl) break; }
    if (!dl) { err = std::string("dlopen(librccl): ") + dlerror(); return false; }
    RcclApi a;
    a.dl = dl;
    a.GetUniqueId = (int (*)(void *))dlsym(dl, "ncclGetUniqueId");
    a.CommInitRank = (int (*)(void **, int, ekf_comm_id, int))dlsym(dl, "ncclCommInitRank");
    a.AllGather = (int (*)(const void *, void *, size_t, int, void *, hipStream_t))dlsym(dl, "ncclAllGather");
    a.CommDestroy = (int (*)(void *))dlsym(dl, "ncclCommDestroy");
    a.GetErrorString = (const char *(*)(int))dlsym(dl, "ncclGetErrorString");
    if (!a.GetUniqueId || !a.CommInitRank || !a.AllGather || !a.CommDestroy || !a.GetErrorString) {
        err = "librccl lacks a required symbol";
        return false;
    }
    g_rccl = a;
    return true;
}

namespace {
int64_t slab_for(const ekf_handle *h, int64_t mm_rows) {
    const int64_t nt = ekf_tiles_for(mm_rows, h->T);
    const int64_t cmax = (nt + h->cfg.world - 1) / h->cfg.world;
    return cmax * h->T * 2;
}

// Where a correction's row-panel is extracted to.  With the library's own communicator and its own buffers: straight into this
// rank's segment of the receive area -- the all-gather is then IN PLACE (sendbuff == recvbuff + rank * count): no local copy inside
// the collective, and with one rank nothing at all.  Caller-provided buffers / a host-run exchange keep the separate send area.
double *corr_send(const ekf_handle *h, int64_t slab) {
    return (h->comm && h->send == h->own_send && h->recv == h->own_recv) ? h->recv + (size_t)h->cfg.rank * (size_t)slab : h->send;
}

// the buffer the PENDING exchange's contribution sits in (what a caller-run all-gather must send)
double *pending_send(const ekf_handle *h) {
    return (h->pending && h->pending_kind == 1) ? corr_send(h, h->x_count) : h->send;
}

int32_t exchange_rccl(ekf_handle *h) {
    if (h->comm == nullptr && h->xhook != nullptr) {
        // transport (d): the caller moves the pending contribution (ekf_exchange_info), between begin and finish as for (b) / (c)
        const int32_t rc = h->xhook(h->xhook_ctx);
        return rc == EKF_OK ? EKF_OK : fail(h, EKF_ERR_COMM, "the exchange hook reported a failure");
    }
    REQUIRE(h, h->comm != nullptr, EKF_ERR_STATE,
            "sharded handle without a communicator: call ekf_comm_init, or drive the begin / your own all-gather / "
            "finish calls");
    const double *src = pending_send(h);
    TimedLaunch tl(h, EKF_KERNEL_EXCHANGE);
    const int r = g_rccl.AllGather(src, h->recv, (size_t)h->x_count, /*ncclDouble*/ 8, h->comm, h->stream);
    if (r != 0) { h->pending = false; return fail(h, EKF_ERR_COMM, g_rccl.GetErrorString(r)); }
    return EKF_OK;
}

// the exchange of what a _begin call left pending; a failed exchange leaves nothing pending
int32_t run_exchange(ekf_handle *h) { const int32_t rc = exchange_rccl(h); if (rc) h->pending = false; return rc; }

// a whole exchange of kind k (x_count doubles per shard, already in place), for the paths that have no finish call of their own
int32_t exchange_bracket(ekf_handle *h, int kind) {
    h->pending = true; h->pending_kind = kind;
    const int32_t rc = run_exchange(h);
    h->pending = false; h->pending_kind = 0;
    return rc;
}

// the panels every shard received become the prefetched base panels, on stream s
hipError_t store_panels(ekf_handle *h, hipStream_t s) {
    return hipMemcpyAsync(h->pf_store, h->recv, (size_t)h->x_count * h->cfg.world * sizeof(double), hipMemcpyDeviceToDevice, s);
}

// ekf_create, the exchange's part: the handle's own send / receive areas and the store of prefetched panels
int32_t create_exchange(ekf_handle *h) {
    h->sharded = h->cfg.world > 1 || h->cfg.force_sharded != 0;
    if (!h->sharded) return EKF_OK;
    h->slab_cap = slab_for(h, 2 * h->cap);
    const size_t rows = (size_t)h->batch;                                  // a prefetch carries up to `batch` row-panels
    // ... and an association's exchange a candidate + one position cost per landmark
    h->xchg_cap = std::max<int64_t>(h->slab_cap * (int64_t)rows, 4 + h->cap);
    HIPCHK(h, dalloc(h, &h->own_send, (size_t)h->xchg_cap));
    HIPCHK(h, dalloc(h, &h->own_recv, (size_t)h->xchg_cap * h->cfg.world));
    HIPCHK(h, dalloc(h, &h->pf_store, (size_t)h->slab_cap * rows * h->cfg.world));
    h->send = h->own_send;
    h->recv = h->own_recv;
    return EKF_OK;
}
}  // namespace

extern "C" {
int32_t ekf_exchange_info(ekf_handle *h, void **send, void **recv, int64_t *count, int64_t *count_capacity) {
    if (!h) return EKF_ERR_INVALID_ARG;
    REQUIRE(h, h->sharded, EKF_ERR_STATE, "exchange_info: handle is not sharded");
    if (send) *send = pending_send(h);
    if (recv) *recv = h->recv;
    if (count) *count = h->pending ? h->x_count : h->slab;
    if (count_capacity) *count_capacity = h->xchg_cap;
    return EKF_OK;
}

int32_t ekf_exchange_set_buffers(ekf_handle *h, void *send, void *recv) {
    if (!h) return EKF_ERR_INVALID_ARG;
    REQUIRE(h, h->sharded && !h->pending, EKF_ERR_STATE, "exchange_set_buffers: not sharded, or a correction is pending");
    h->send = send ? (double *)send : h->own_send;
    h->recv = recv ? (double *)recv : h->own_recv;
    exchange_changed(h);       // corr_send() may point elsewhere now: a hinted extraction sits in the old area
    return EKF_OK;
}

int32_t ekf_exchange_set_hook(ekf_handle *h, int32_t (*hook)(void *), void *ctx) {
    if (!h) return EKF_ERR_INVALID_ARG;
    REQUIRE(h, h->sharded && !h->pending, EKF_ERR_STATE, "exchange_set_hook: not sharded, or an exchange is pending");
    REQUIRE(h, h->comm == nullptr || hook == nullptr, EKF_ERR_STATE, "exchange_set_hook: the handle has a communicator of its own");
    h->xhook = hook;
    h->xhook_ctx = ctx;
    exchange_changed(h);
    return EKF_OK;
}

int32_t ekf_exchange_local(ekf_handle **hs, int32_t world) {
    if (!hs || world < 1) return EKF_ERR_INVALID_ARG;
    for (int r = 0; r < world; ++r) {
        if (!hs[r]) return EKF_ERR_INVALID_ARG;
        REQUIRE(hs[r], hs[r]->sharded && hs[r]->cfg.world == world && hs[r]->cfg.rank == r && hs[r]->pending &&
                           hs[r]->x_count == hs[0]->x_count && hs[r]->pending_kind == hs[0]->pending_kind,
                EKF_ERR_STATE, "exchange_local: handles must be the shards 0..world-1 of one filter, each between the same begin and finish");
    }
    // producers first: every shard's send slab must be complete before anyone copies it
    for (int r = 0; r < world; ++r) {
        HIPCHK(hs[r], hipSetDevice(hs[r]->cfg.device));
        HIPCHK(hs[r], hipStreamSynchronize(hs[r]->stream));
    }
    const size_t bytes = (size_t)hs[0]->x_count * sizeof(double);
    for (int dst = 0; dst < world; ++dst) {
        ekf_handle *d = hs[dst];
        HIPCHK(d, hipSetDevice(d->cfg.device));
        for (int src = 0; src < world; ++src) {
            const double *from = pending_send(hs[src]);
            double *to = d->recv + (size_t)src * d->x_count;
            if (from == to) continue;                                  // already in place (own segment of the own receive area)
            HIPCHK(d, hipMemcpyPeerAsync(to, d->cfg.device, from, hs[src]->cfg.device, bytes, d->stream));
        }
        if (!d->ev_xchg) HIPCHK(d, new_event(d, &d->ev_xchg));
        HIPCHK(d, hipEventRecord(d->ev_xchg, d->stream));
    }
    // consumers before the next producers: a shard's stream may run ahead into its next extract (k_rowpanel overwrites its
    // send slab) while another shard's stream has not yet copied that slab -- every stream waits for every shard's copies.
    // (Found as an intermittent divergence of the replicated state across a 4-shard group on one GPU.)
    for (int r = 0; r < world; ++r) {
        HIPCHK(hs[r], hipSetDevice(hs[r]->cfg.device));
        for (int dst = 0; dst < world; ++dst)
            if (dst != r) HIPCHK(hs[r], hipStreamWaitEvent(hs[r]->stream, hs[dst]->ev_xchg, 0));
    }
    return EKF_OK;
}

int32_t ekf_comm_unique_id(ekf_comm_id *id) {
    if (!id) return EKF_ERR_INVALID_ARG;
    std::string err;
    if (!rccl_load(err)) return EKF_ERR_COMM;
    return g_rccl.GetUniqueId(id) == 0 ? EKF_OK : EKF_ERR_COMM;
}

int32_t ekf_comm_init(ekf_handle *h, const ekf_comm_id *id) {
    if (!h || !id) return fail(h, EKF_ERR_INVALID_ARG, "comm_init: null argument");
    REQUIRE(h, h->sharded, EKF_ERR_STATE, "comm_init: handle is not sharded");
    REQUIRE(h, h->comm == nullptr, EKF_ERR_STATE, "comm_init: communicator already attached");
    TRY(use_device(h));
    std::string err;
    if (!rccl_load(err)) return fail(h, EKF_ERR_COMM, err.c_str());
    void *comm = nullptr;
    const int r = g_rccl.CommInitRank(&comm, h->cfg.world, *id, h->cfg.rank);
    if (r != 0) return fail(h, EKF_ERR_COMM, g_rccl.GetErrorString(r));
    h->comm = comm;
    exchange_changed(h);       // with a communicator the row-panel goes straight into the receive area (corr_send)
    return EKF_OK;
}

int32_t ekf_shard_owner(int32_t world, int64_t I, int64_t J) {
    if (world < 1 || I < 0 || J < 0) return -1;
    return ekf_make_tilemap(64, world, 0).owner(I, J);
}

int64_t ekf_shard_slot(int32_t world, int64_t I, int64_t J) {
    if (world < 1 || I < 0 || J < 0 || J > I) return -1;
    return ekf_make_tilemap(64, world, 0).slot(I, J);
}

int32_t ekf_shard_panel_source(int32_t world, int64_t tile_row_j, int64_t chunk, int32_t *owner, int64_t *local_chunk) {
    if (world < 1 || tile_row_j < 0 || chunk < 0 || !owner || !local_chunk) return EKF_ERR_INVALID_ARG;
    *owner = (int32_t)((tile_row_j + chunk) % world);
    *local_chunk = chunk / world;
    return EKF_OK;
}
}  // extern "C"
