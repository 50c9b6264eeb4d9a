// Fragment of kernels.hip, the launchers of the passes over P: launch_downdate -- launch/pass_select.h decides, this file launches --
// and the row copies that follow an asynchronous pass.
#pragma once

size_t pass_split_plane_elems(int64_t ldm) { return ekf_pipe32::split_plane_elems(ldm); }

namespace {
// Dynamic LDS beyond 64 KiB has to be allowed per kernel AND per device (a ShardGroup drives several devices from one process): set once for
// the device that is current at the launch, remembered in a bit mask.
hipError_t allow_dynamic_lds(const void *fn, size_t bytes, std::atomic<uint64_t> &done) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const uint64_t bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) done.fetch_or(bit, std::memory_order_release);
    return e;
}

// every (storage type, tile edge, rows per workgroup) the VALU kernels are built for: the slabs of ekf_pass::kSlabRules
template <typename TS_, int kT, int kSlab> struct PassShape { using TS = TS_; static constexpr int T = kT, slab = kSlab; };
template <typename... S> struct PassShapes {};
using ValuShapes = PassShapes<
    PassShape<double, 16, 16>, PassShape<double, 32, 16>, PassShape<double, 32, 32>,
    PassShape<double, 64, 8>, PassShape<double, 64, 16>, PassShape<double, 64, 32>, PassShape<double, 64, 64>,
    PassShape<double, 128, 4>, PassShape<double, 128, 8>, PassShape<double, 128, 16>, PassShape<double, 128, 32>,
    PassShape<float, 16, 16>, PassShape<float, 32, 32>, PassShape<float, 64, 64>, PassShape<float, 128, 8>, PassShape<float, 128, 64>,
    PassShape<float, 256, 4>, PassShape<float, 256, 8>, PassShape<float, 256, 16>, PassShape<float, 256, 32>>;

// f(shape) for the shape the instance names; false: it is not in the list
template <typename F, typename... S> bool with_shape(PassShapes<S...>, const ekf_pass::PassInstance &p, F &&f) {
    return (((int)sizeof(typename S::TS) == p.elt && S::T == p.T && S::slab == p.slab ? (f(S{}), true) : false) || ...);
}
}  // namespace

// pstart / npairs: the ring window, oldest pair first; nx: see NextRow
hipError_t launch_downdate(const DevState &st, const PassJob &job, int storage, hipStream_t s, char *kname, bool *extracted) {
    using namespace ekf_pass;
    if (extracted) *extracted = false;
    if (job.nwork <= 0 || job.npairs <= 0) return hipSuccess;
    static const int slab1 = ekf_tune_int("EKF_DOWNDATE_SLAB", 0);
    static const int slabm = ekf_tune_int("EKF_DOWNDATE_SLAB_BATCH", 0);
    static const PassKnobs knobs = { ekf_tune_int("EKF_FLUSH_MFMA", 1) != 0, ekf_tune_int("EKF_FLUSH_MFMA_SWITCH", 30), ekf_tune_int("EKF_FLUSH_HALF_MAX", 12),
                                     ekf_tune_int("EKF_PASS_STRIP", 1) != 0, ekf_tune_int("EKF_FLUSH_XCD", 1) != 0 };
    const PassAux *aux = job.aux;
    const int T = st.tm.T, pstart = job.pstart, npairs = job.npairs;
    // rows that hold state (in-place passes: PassJob::live_rows); the kernels that take it skip the work items of padding rows
    const int live = job.live_rows > 0 && job.live_rows < INT_MAX ? (int)job.live_rows : INT_MAX;
    PassQuery q = { storage == 0 ? 8 : 4, T, npairs, job.arith, /*xcd_list*/ job.work_xcd && job.xcd_len > 0,
                    /*strip_list*/ aux && aux->segs && aux->nsegs > 0, /*planes*/ aux && aux->Kb3 && aux->Gb3, /*next_row*/ job.nx && job.nx->j >= 0,
                    /*slab_override*/ npairs > 1 ? slabm : slab1 };
    PassInstance p = select_pass(q, knobs);
    // the split and the strip kernel need more dynamic LDS than a kernel gets unasked; a device that refuses it takes the next candidate
    static std::atomic<uint64_t> split_ok{0}, strip_ok{0};
    if (p.family == kSplit3 && allow_dynamic_lds((const void *)ekf_pipe32::k_flush_split3<2>, ekf_pipe32::lds_bytes_split(), split_ok) != hipSuccess) {
        q.planes = false;
        p = select_pass(q, knobs);
    }
    if (p.family == kStrip32 && allow_dynamic_lds((const void *)ekf_pipe32::k_flush_strip32<8>, ekf_pipe32::lds_bytes_strip<8>(), strip_ok) != hipSuccess) {
        q.strip_list = false;
        p = select_pass(q, knobs);
    }

    // the matrix-core kernels share one argument list; a work item is rows x cols of a tile, counted per XCD stream
    auto flush = [&](auto kernel, auto ts, auto *Kp, auto *Gp, int rows, int cols, auto... more) {
        using TS = decltype(ts);
        hipLaunchKernelGGL(kernel, dim3(clamp_grid(8 * job.xcd_len * (T / rows) * (T / cols), job.grid_cap)), dim3(kBlock), 0, s,
                           (const TS *)st.tiles, (TS *)job.dst, job.work_xcd, job.xcd_len, Kp, Gp, st.pair_stride, pstart, st.pcap, npairs, st.tm, more...);
    };
    switch (p.family) {
        case kInvalid: return hipErrorInvalidValue;
        case kSplit3:
            hipLaunchKernelGGL(ekf_pipe32::k_split_pairs, dim3((unsigned)(aux->cols / 256), ekf_pipe32::kKB, 2), dim3(256), 0, s, (const float *)st.Kp32,
                               (const float *)st.Gp32, aux->Kb3, aux->Gb3, st.pair_stride, st.ldm, aux->cols, pstart, st.pcap, npairs);
            hipLaunchKernelGGL((ekf_pipe32::k_flush_split3<2>), dim3((unsigned)aux->grid), dim3(512), ekf_pipe32::lds_bytes_split(), s,
                               (const float *)st.tiles, (float *)job.dst, aux->segs, aux->nsegs, (const uint16_t *)aux->Kb3, (const uint16_t *)aux->Gb3, st.ldm,
                               st.tm, aux->dump);
            break;
        case kStrip32:
            hipLaunchKernelGGL((ekf_pipe32::k_flush_strip32<8>), dim3((unsigned)aux->grid), dim3(512), ekf_pipe32::lds_bytes_strip<8>(), s,
                               (const float *)st.tiles, (float *)job.dst, aux->segs, aux->nsegs, (const float *)st.Kp32, (const float *)st.Gp32, st.pair_stride,
                               st.ldm, pstart, st.pcap, npairs, st.tm, aux->dump, (unsigned long long *)nullptr);
            break;
        case kMfma32:                                   // (float tiles of edge 256 only: select_pass)
            if (p.early) flush(k_flush_mfma32<256, 4, 2, 3, true>, float{}, st.Kp32, st.Gp32, 128, 128);
            else flush(k_flush_mfma32<256, 4, 2, 3>, float{}, st.Kp32, st.Gp32, 128, 128);
            break;
        case kMfma64:                                   // (f64 tiles of edge 128, float tiles of edge 256)
            if (p.elt == 4) {
                if (p.chunk == 4) flush(k_flush_mfma<float, 256, 4>, float{}, st.Kp, st.Gp, 64, 128, live);
                else flush(k_flush_mfma<float, 256, 8>, float{}, st.Kp, st.Gp, 64, 128, live);
            } else if (p.cols == 64) flush(k_flush_mfma<double, 128, 4, 64, 5>, double{}, st.Kp, st.Gp, 64, 64, live);
            else if (p.chunk == 4) flush(k_flush_mfma<double, 128, 4>, double{}, st.Kp, st.Gp, 64, 128, live);
            else flush(k_flush_mfma<double, 128, 8>, double{}, st.Kp, st.Gp, 64, 128, live);
            break;
        case kDowndateW:
        case kDowndate: {
            bool oversize = false;
            const bool built = with_shape(ValuShapes{}, p, [&](auto shape) {
                using TS = typename decltype(shape)::TS;
                constexpr int kT = decltype(shape)::T, kSlab = decltype(shape)::slab, kLanes = kT / Lane16<TS>::kCols;
                const TS *src = (const TS *)st.tiles;
                TS *dst = (TS *)job.dst;
                const dim3 grid(clamp_grid(job.nwork * (kT / kSlab), job.grid_cap)), grid_xcd(clamp_grid(8 * job.xcd_len * (kT / kSlab), job.grid_cap));
                if constexpr (kLanes != 64 && kLanes != 32) {
                    hipLaunchKernelGGL((k_downdate<TS, kT, kSlab>), grid, dim3(kBlock), 0, s, src, dst, job.work, job.nwork, st.Kp, st.Gp,
                                       st.pair_stride, pstart, st.pcap, npairs, st.tm, live);
                } else {
                    // the one list's item space (k_downdate_w: head, tail_shift): every tile whole -- or, under a bound, the tiles of the
                    // last tile row (the entries from job.nwork_head on) only up to the slab that holds the bound, rounded up to a power of two
                    constexpr int kSlabs = kT / kSlab;
                    int64_t head = job.nwork * kSlabs, items = head;
                    int tail_shift = 0;
                    if (live != INT_MAX && job.nwork_head >= 0 && job.nwork_head < job.nwork) {
                        const int in_last = live - (live - 1) / kT * kT, slabs = (in_last + kSlab - 1) / kSlab;
                        while ((1 << tail_shift) < slabs) ++tail_shift;
                        head = job.nwork_head * kSlabs;
                        items = head + ((job.nwork - job.nwork_head) << tail_shift);
                    }
                    if (!p.xcd && items > INT_MAX) { oversize = true; return; }      // (k_downdate_w counts the one list's items in 32 bits)
                    const dim3 grid_list(clamp_grid(items, job.grid_cap));
                    auto per_row = [&](auto kernel, dim3 g, const int2 *list, int64_t n, auto next) {
                        hipLaunchKernelGGL(kernel, g, dim3(kBlock), 0, s, src, dst, list, n, st.Kp, st.Gp, st.pair_stride, pstart, st.pcap, npairs, st.tm, next, live,
                                           (int)head, tail_shift);
                    };
                    if (p.xcd) per_row(k_downdate_w<TS, kT, kSlab, true>, grid_xcd, job.work_xcd, job.xcd_len, NoNextRow{});
                    else if (p.rowpanel) per_row(k_downdate_w<TS, kT, kSlab, false, true>, grid_list, job.work, job.nwork, *job.nx);
                    else per_row(k_downdate_w<TS, kT, kSlab, false>, grid_list, job.work, job.nwork, NoNextRow{});
                }
            });
            if (!built || oversize) return hipErrorInvalidValue;
            if (extracted) *extracted = p.rowpanel;
            break;
        }
    }
    if (kname) snprintf(kname, 64, "%s", p.name);
    return hipGetLastError();
}

namespace {
// the tile rows that hold landmark-block rows [r0, r1): launch(grid, slot0, nslots, lo, n, I) once per tile row, for its local rows
// [lo, lo + n) in every local tile slot0 .. slot0 + nslots - 1; returns the last error a launch reported
template <typename Launch>
hipError_t copy_tile_rows(const TileMap &tm, int64_t r0, int64_t r1, int storage, Launch &&launch) {
    if (r1 <= r0) return hipSuccess;
    const int T = tm.T;
    if (T > kBlock * (storage == 0 ? 2 : 4)) return hipErrorInvalidValue;                    // a tile row must fit one workgroup's lanes
    hipError_t e = hipSuccess;
    for (int64_t I = r0 >> tm.shift; I <= (r1 - 1) >> tm.shift; ++I) {
        const int64_t lo = std::max<int64_t>(r0, I * T) - I * T, hi = std::min<int64_t>(r1, (I + 1) * T) - I * T;
        const int64_t slot0 = tm.row_base(I), nslots = tm.row_base(I + 1) - slot0;
        if (nslots <= 0 || hi <= lo) continue;
        const int lanes = T / (storage == 0 ? 2 : 4), per_wg = kBlock / lanes > 0 ? kBlock / lanes : 1;
        const hipError_t ei = launch(dim3((unsigned)cdiv(nslots * (hi - lo), per_wg)), slot0, nslots, (int)lo, (int)(hi - lo), I);
        if (ei != hipSuccess) e = ei;
    }
    return e;
}
}  // namespace

hipError_t launch_copy_rows(const TileMap &tm, const void *src, void *dst, int64_t r0, int64_t r1, int storage, hipStream_t s) {
    return copy_tile_rows(tm, r0, r1, storage, [&](dim3 grid, int64_t slot0, int64_t nslots, int lo, int n, int64_t) {
        return with_storage(storage, [&](auto ts) {
            using TS = decltype(ts);
            hipLaunchKernelGGL(k_copy_tile_rows<TS>, grid, dim3(kBlock), 0, s, (const TS *)src, (TS *)dst, slot0, nslots, lo, n, tm.T);
        });
    });
}

hipError_t launch_copy_rows_dev(const TileMap &tm, const void *src, void *dst, int64_t r0, int64_t r1, const int64_t *n_lo,
                                const int64_t *n_hi, int storage, hipStream_t s) {
    return copy_tile_rows(tm, r0, r1, storage, [&](dim3 grid, int64_t slot0, int64_t nslots, int lo, int n, int64_t I) {
        return with_storage(storage, [&](auto ts) {
            using TS = decltype(ts);
            hipLaunchKernelGGL(k_copy_tile_rows_dev<TS>, grid, dim3(kBlock), 0, s, (const TS *)src, (TS *)dst, slot0, nslots, lo, n, tm.T,
                               I * tm.T, r0, r1, n_lo, n_hi);
        });
    });
}
