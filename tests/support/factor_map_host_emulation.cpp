// Host emulation of the kernels of ekf_factor_map (tests/test_factor_map_cpu.py compiles and runs it; no GPU, no HIP runtime).  The kernel
// SOURCE ekf_slam_amd/csrc/factor_map.h is compiled for the host behind kernel_host_shim.h.  Unlike the kernels of the other emulations
// these work through barriers (a diagonal tile is factored in LDS, two barriers a column), so a workgroup's lanes cannot run one after
// another: each lane of a workgroup with barriers is a THREAD here, threadIdx / blockIdx are per thread, __syncthreads is a real barrier
// and __shared__ storage is the function's static storage, one workgroup at a time.  The kernels without a barrier (k_factor_load,
// k_factor_rhs, k_factor_trail) run their lanes one after another.  k_factor_trail's matrix-core loop is replaced by its plain-FMA twin
// in the same k order (EKF_FACTOR_FMA_TWIN).  Factor tile edges 16 and 32; the source store is F64 or float with its own tile edge.
// The cases -- one line "name TF Tsrc float N nref" each -- are read from argv[1]/cases.txt; case `name` reads argv[1]/name.in (x, the
// dense P column by column as the test wants the handle to hold it, nref reference states) and writes argv[1]/name.out: the result
// block, then the pivots.  Each case checks here that the launches left the state (x, Prr, the strip, the tiles, the diagonal copies, s,
// the pair ring) bit for bit as it was.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
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

// every workgroup of the grid, its lanes as threads
template <typename F> static void launch_threads(int grid, int lanes, F body) {
    for (int b = 0; b < grid; ++b) {
        pthread_barrier_init(&group_barrier, nullptr, (unsigned)lanes);
        std::vector<std::thread> pool;
        for (int t = 0; t < lanes; ++t) pool.emplace_back([&body, b, t] { lane_idx.x = (unsigned)t; group_idx.x = (unsigned)b; body(); });
        for (auto &th : pool) th.join();
        pthread_barrier_destroy(&group_barrier);
    }
}
// ... and one after another (no barrier in the kernel)
template <typename F> static void launch_lanes(int grid, int lanes, F body) {
    for (int b = 0; b < grid; ++b) for (int t = 0; t < lanes; ++t) { lane_idx.x = (unsigned)t; group_idx.x = (unsigned)b; body(); }
}

struct Case { std::string name; int TF, Tsrc, isfloat, N, nref; };

template <typename TS, int TF> static int run_case(const Case &c, const std::string &dir) {
    const int N = c.N, n = 3 + 2 * N;
    std::vector<double> in((size_t)n + (size_t)n * n + (size_t)c.nref * n);
    FILE *f = fopen((dir + "/" + c.name + ".in").c_str(), "rb");
    if (!f || fread(in.data(), 8, in.size(), f) != in.size()) return 1000;
    fclose(f);
    const double *x = in.data(), *P = x + n, *refs = P + (size_t)n * n;
    Store<TS> S(c.Tsrc, N, N + 3);
    for (int i = 0; i < n; ++i) S.x[0][i] = x[i];
    for (int k = 0; k < N; ++k) S.s[k] = k + 1.0;
    scatter(S, [&](int r, int col) { return P[(size_t)col * n + r]; });
    for (auto &v : S.ring) v = 0.25;
    const Store<TS> S0(S);
    FactorMapArgs a = {};
    a.tm = ekf_make_tilemap(TF, 1, 0);
    a.N = N; a.rows = a.tm.padded(2 * N); a.nref = c.nref; a.ref_stride = n; a.cur = S.cur;
    const int nF = (int)(a.rows / TF);
    const double kPoison = -7.0;
    std::vector<double> tiles((size_t)(a.tm.row_base(nF) > 0 ? a.tm.row_base(nF) : 1) * TF * TF, kPoison), rhs((size_t)a.rows * kFactorRhs + 1, kPoison);
    std::vector<double> res((size_t)kFactorRes + a.rows, 0.0), ref(refs, refs + (size_t)c.nref * n);
    for (int64_t i = 0; i < a.rows; ++i) res[kFactorRes + i] = kPoison;
    a.tiles = tiles.data(); a.rhs = rhs.data(); a.res = res.data(); a.ref = c.nref ? ref.data() : nullptr;
    const DevState st = S.st;
    if (N > 0) {
        launch_lanes((int)((a.rows + kFactorBlock - 1) / kFactorBlock), kFactorBlock, [&] { k_factor_rhs(st, a); });
        launch_lanes((int)a.tm.row_base(nF), kFactorBlock, [&] { k_factor_load<TS, TF>(st, a); });
    }
    int bad = 0;
    for (double v : tiles) if (N > 0 && v == kPoison) ++bad;                      // the load writes every tile whole
    for (int k = 0; k < nF; ++k) {
        launch_threads(1, kFactorBlock, [&] { k_factor_diag<TF>(a, k); });
        const int m = nF - 1 - k;
        if (m == 0) continue;
        launch_threads(m, 64, [&] { k_factor_panel<TF>(a, k); });
        launch_lanes(m * (m + 1) / 2, 4 * TF, [&] { k_factor_trail<TF>(a, k); });
    }
    launch_threads(1, kFactorBlock, [&] { k_factor_finish(st, a); });
    // nothing of the state was written
    bad += differ(S.x[0], S0.x[0], "x") + differ(S.x[1], S0.x[1], "x other") + differ(S.prr[0], S0.prr[0], "prr") + differ(S.strip[0], S0.strip[0], "strip") +
           differ(S.diag[0], S0.diag[0], "diag") + differ(S.diag[1], S0.diag[1], "diag other") + differ(S.s, S0.s, "s") +
           differ(S.ring, S0.ring, "pair ring") + differ(S.tiles, S0.tiles, "tiles") + differ(S.small, S0.small, "small");
    if (rhs.back() != kPoison) ++bad;
    f = fopen((dir + "/" + c.name + ".out").c_str(), "wb");
    if (!f) return 1000;
    put(f, res.data(), res.size());
    fclose(f);
    printf("%s: %d differences\n", c.name.c_str(), bad);
    return bad;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    FILE *f = fopen((dir + "/cases.txt").c_str(), "r");
    if (!f) return 3;
    int bad = 0, n = 0;
    char name[128];
    Case c;
    while (fscanf(f, "%127s %d %d %d %d %d", name, &c.TF, &c.Tsrc, &c.isfloat, &c.N, &c.nref) == 6) {
        if ((c.TF != 16 && c.TF != 32) || (c.Tsrc != 16 && c.Tsrc != 32) || c.N < 0 || c.N > 64 || c.nref < 0 || c.nref > kFactorRefMax) { fclose(f); return 4; }
        c.name = name;
        if (c.TF == 16) bad += c.isfloat ? run_case<float, 16>(c, dir) : run_case<double, 16>(c, dir);
        else bad += c.isfloat ? run_case<float, 32>(c, dir) : run_case<double, 32>(c, dir);
        ++n;
    }
    fclose(f);
    if (n == 0) return 5;
    return bad != 0;
}
