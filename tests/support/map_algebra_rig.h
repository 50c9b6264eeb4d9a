// The rig of the four emulations of the calls that treat P as a matrix (factor_map, sample_map, solve_map and multiply_map
// _host_emulation.cpp; no GPU, no HIP runtime).  Their kernels work through barriers (a diagonal tile is factored in LDS, the chunks are
// staged through LDS), so a workgroup's lanes cannot run one after another as launch_wg of emulated_state.h runs them: each lane of a
// workgroup with barriers is a THREAD here, threadIdx / blockIdx are per thread, __syncthreads is a real barrier and __shared__ storage is
// the function's static storage, one workgroup at a time.  The matrix-core loops compile as their plain-FMA twins in the same k order
// (EKF_FACTOR_FMA_TWIN).  The rig brings in the shim, the Store, factor_map.h and map_blocks.h; a program includes the kernel sources it
// runs beyond those after it.  It holds, once:
//   launch_threads / launch_lanes   workgroups first .. last - 1 of a grid, the lanes of each as the threads of one pool / one after another
//   pack_chunk / unpack_chunk       vectors in x's order <-> the columns of a chunk, as host/factor_map.h's chunk_stream does it
//   FactoredCase                    a case read, the Store filled, the scratch poisoned, the factorisation run launch after launch
#pragma once
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include <pthread.h>
#include "kernel_host_shim.h"
#include "emulated_state.h"

static thread_local Idx lane_idx, group_idx;
static pthread_barrier_t group_barrier;
#define threadIdx lane_idx
#define blockIdx group_idx
#define __syncthreads() pthread_barrier_wait(&group_barrier)
#define EKF_FACTOR_FMA_TWIN 1
typedef double d4_t __attribute__((vector_size(32)));
#include "factor_map.h"
#include "map_blocks.h"

// The sweeps of a solve are hundreds of small launches a case, so the threads are made once: lane t of every workgroup is worker t of a
// pool that sleeps between workgroups.
struct LanePool {
    std::vector<std::thread> workers;
    std::mutex m;
    std::condition_variable go, done;
    std::function<void()> body;
    long gen = 0;
    int lanes = 0, group = 0, left = 0;
    bool stop = false;
    void work(int t) {
        long seen = 0;
        for (;;) {
            std::function<void()> f;
            {
                std::unique_lock<std::mutex> lk(m);
                go.wait(lk, [&] { return stop || (gen != seen && t < lanes); });
                if (stop) return;
                seen = gen;
                f = body;
                lane_idx.x = (unsigned)t; group_idx.x = (unsigned)group;
            }
            f();
            std::lock_guard<std::mutex> lk(m);
            if (--left == 0) done.notify_one();
        }
    }
    void run(int b, int n, const std::function<void()> &f) {
        std::unique_lock<std::mutex> lk(m);
        while ((int)workers.size() < n) { const int t = (int)workers.size(); workers.emplace_back([this, t] { work(t); }); }
        body = f; group = b; lanes = n; left = n; ++gen;
        go.notify_all();
        done.wait(lk, [&] { return left == 0; });
        lanes = 0;
    }
    ~LanePool() {
        { std::lock_guard<std::mutex> lk(m); stop = true; }
        go.notify_all();
        for (auto &th : workers) th.join();
    }
};
static LanePool pool;
template <typename F> static void launch_threads(int first, int last, int lanes, F body) {
    for (int b = first; b < last; ++b) {
        pthread_barrier_init(&group_barrier, nullptr, (unsigned)lanes);
        pool.run(b, lanes, body);
        pthread_barrier_destroy(&group_barrier);
    }
}
// ... and one after another (no barrier on the way)
template <typename F> static void launch_lanes(int first, int last, int lanes, F body) {
    for (int b = first; b < last; ++b) for (int t = 0; t < lanes; ++t) { lane_idx.x = (unsigned)t; group_idx.x = (unsigned)b; body(); }
}

constexpr double kPoison = -7.0;

// Chunk j of the k vectors of src (n = 3 + 2 N entries each, x's order) as columns ld doubles apart: the landmark part first, the robot's
// three from entry `rows` on; and the columns of a chunk back into the rows of out
static void pack_chunk(double *chunk, const double *src, int64_t j, int64_t k, int N, int64_t rows, int64_t ld) {
    const int n = 3 + 2 * N;
    for (int64_t q = 0; q < kFactorChunk && j * kFactorChunk + q < k; ++q) {
        const double *row = src + (j * kFactorChunk + q) * n;
        memcpy(chunk + q * ld, row + 3, (size_t)(2 * N) * 8);
        memcpy(chunk + q * ld + rows, row, 24);
    }
}
static void unpack_chunk(double *out, const double *chunk, int64_t j, int64_t k, int N, int64_t rows, int64_t ld) {
    const int n = 3 + 2 * N;
    for (int64_t q = 0; q < kFactorChunk && j * kFactorChunk + q < k; ++q) {
        double *o = out + (j * kFactorChunk + q) * n;
        memcpy(o, chunk + q * ld + rows, 24);
        memcpy(o + 3, chunk + q * ld, (size_t)(2 * N) * 8);
    }
}

// how many entries of the state the launches changed: they are to leave it bit for bit as it was
template <typename TS> static int state_differs(const Store<TS> &S, const Store<TS> &S0) {
    return differ(S.x[0], S0.x[0], "x") + differ(S.x[1], S0.x[1], "x other") + differ(S.prr[0], S0.prr[0], "prr") + differ(S.strip[0], S0.strip[0], "strip") +
           differ(S.diag[0], S0.diag[0], "diag") + differ(S.diag[1], S0.diag[1], "diag other") + differ(S.s, S0.s, "s") +
           differ(S.ring, S0.ring, "pair ring") + differ(S.tiles, S0.tiles, "tiles") + differ(S.small, S0.small, "small");
}

// A case of the factor, sample or solve program: dir/name.in holds x, the dense P column by column as the test wants the handle to hold
// it, then `extra` doubles of the program's own (reference states, draws, right-hand sides).  The Store (source tile edge Tsrc) is
// filled, the factor store of edge TF, the right-hand sides and the pivots poisoned, and run() is the factorisation in the order
// host/factor_map.h's factor_body queues it.  nref reference states are the front of `extra`; with_tail: k_factor_finish stores all of
// L_r (a.lr_off), as the draws and the solves need it.
template <typename TS, int TF> struct FactoredCase {
    int N, n, nF = 0, unloaded = 0;
    bool ok = false, with_tail;
    std::vector<double> in, tiles, rhs, res, ref, tail;
    const double *extra = nullptr;
    Store<TS> S, S0;
    FactorMapArgs a = {};
    DevState st;
    FactoredCase(const std::string &dir, const std::string &name, int Tsrc, int N_, size_t extra_doubles, int nref, bool with_tail_)
        : N(N_), n(3 + 2 * N_), with_tail(with_tail_), in((size_t)n + (size_t)n * n + extra_doubles), tail(4, kPoison), S(Tsrc, N_, N_ + 3), S0(S) {
        FILE *f = fopen((dir + "/" + name + ".in").c_str(), "rb");
        ok = f && fread(in.data(), 8, in.size(), f) == in.size();
        if (f) fclose(f);
        if (!ok) return;
        const double *x = in.data(), *P = x + n;
        extra = P + (size_t)n * n;
        for (int i = 0; i < n; ++i) S.x[0][i] = x[i];
        for (int q = 0; q < N; ++q) S.s[q] = q + 1.0;
        scatter(S, [&](int r, int col) { return P[(size_t)col * n + r]; });
        for (auto &v : S.ring) v = 0.25;
        S0 = S;
        a.tm = ekf_make_tilemap(TF, 1, 0);
        a.N = N; a.rows = a.tm.padded(2 * N); a.nref = nref; a.ref_stride = n; a.cur = S.cur;
        nF = (int)(a.rows / TF);
        tiles.assign((size_t)(a.tm.row_base(nF) > 0 ? a.tm.row_base(nF) : 1) * TF * TF, kPoison);
        rhs.assign((size_t)a.rows * kFactorRhs + 1, kPoison);
        res.assign((size_t)kFactorRes + a.rows, 0.0);
        for (int64_t i = 0; i < a.rows; ++i) res[kFactorRes + i] = kPoison;
        ref.assign(extra, extra + (size_t)nref * n);
        a.tiles = tiles.data(); a.rhs = rhs.data(); a.res = res.data(); a.ref = nref ? ref.data() : nullptr; a.lr_off = with_tail ? tail.data() : nullptr;
        st = S.st;
    }
    void run() {
        if (N > 0) {
            launch_lanes(0, (int)((a.rows + kFactorBlock - 1) / kFactorBlock), kFactorBlock, [&] { k_factor_rhs(st, a); });
            launch_lanes(0, (int)a.tm.row_base(nF), kFactorBlock, [&] { k_factor_load<TS, TF>(st, a); });
            for (double v : tiles) if (v == kPoison) ++unloaded;                      // (the load writes every tile whole)
        }
        for (int col = 0; col < nF; ++col) {
            launch_threads(0, 1, kFactorBlock, [&] { k_factor_diag<TF>(a, col); });
            const int m = nF - 1 - col;
            if (m == 0) continue;
            launch_threads(0, m, 64, [&] { k_factor_panel<TF>(a, col); });
            launch_lanes(0, m * (m + 1) / 2, 4 * TF, [&] { k_factor_trail<TF>(a, col); });
        }
        launch_threads(0, 1, kFactorBlock, [&] { k_factor_finish(st, a); });
    }
    // nothing of the state was written, nothing behind the right-hand sides or L_r's three entries
    int untouched() const { return state_differs(S, S0) + (rhs.back() != kPoison) + (with_tail && tail[3] != kPoison); }
    // THE FACTOR THE LAUNCHES WORKED WITH, read out of what the factorisation left: C = [L 0; W' L_r] in elimination order, n x n
    // row-major -- L from the factor store (above the diagonal as stored: the apply pass reads those entries too), W from columns 0..2 of
    // the right-hand sides, L_r from res[3..5] and lr_off; NaN throughout where a pivot failed
    void put_factor(FILE *f) const {
        std::vector<double> C((size_t)n * n, res[0] == 0.0 ? 0.0 : NAN);
        if (res[0] == 0.0) {
            for (int r = 0; r < 2 * N; ++r)
                for (int col = 0; col < 2 * N; ++col)
                    if (col / TF <= r / TF) C[(size_t)r * n + col] = tiles[a.tm.tile_offset(r / TF, col / TF) + (size_t)(r % TF) * TF + col % TF];
            for (int q = 0; q < 3; ++q)
                for (int col = 0; col < 2 * N; ++col) C[(size_t)(2 * N + q) * n + col] = rhs[(size_t)col * kFactorRhs + q];
            double *Lr = C.data() + (size_t)(2 * N) * n + 2 * N;
            Lr[0] = res[3]; Lr[n] = tail[0]; Lr[n + 1] = res[4]; Lr[2 * n] = tail[1]; Lr[2 * n + 1] = tail[2]; Lr[2 * n + 2] = res[5];
        }
        put(f, C.data(), C.size());
    }
};
