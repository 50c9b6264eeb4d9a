// Host emulation of the iterated model-observation kernels (tests/test_model_iter_cpu.py compiles and runs it; no GPU, no HIP runtime).
// The kernel SOURCES of ekf_slam_amd/csrc (tile_access.h, pair_column.h, constrain.h, linear_obs.h, model_obs.h, model_iter.h) are compiled
// for the host behind kernel_host_shim.h, as model_obs_host_emulation.cpp does.  argv[1]/cases.bin (doubles; tests/model_iter_cases.py's
// scenes, written by the test) holds N, x (3 + 2N), the dense P (row-major) and the cases: model, l0, l1 (-1: none), anchored, anchor (2),
// z (2), R (4, row-major), gate, iterations, tol.  For every case, on that state with an empty ring:
//   k_gather_model_iter, and k_model_iter_probe, whose two records must be the launch's BIT FOR BIT;
//   with iterations == 1 also k_gather_model: x, Prr, the strip, the diagonal blocks, the pair (G, K) and the record BIT FOR BIT.
// What the iterated launch left goes to argv[1]/case_<k>.bin for the dense restatement: x', Prr', strip' (3 rows of 2N), the diagonal
// blocks (3N), G and K (2N x 2 each), the record (8), the iteration record (16), the two counters.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "kernel_host_shim.h"
#include "emulated_state.h"
#include "model_obs.h"
#include "model_iter.h"

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    std::vector<double> raw;
    {
        FILE *f = fopen((dir + "/cases.bin").c_str(), "rb");
        if (!f) return 2;
        double v;
        while (fread(&v, 8, 1, f) == 1) raw.push_back(v);
        fclose(f);
    }
    size_t at = 0;
    const int N = (int)raw[at++], n = 3 + 2 * N, T = 16;
    const double *x0 = &raw[at]; at += n;
    const double *Pd = &raw[at]; at += (size_t)n * n;
    auto P = [&](int r, int c) { return Pd[(size_t)r * n + c]; };
    Store base(T, N, N + 2);
    for (int i = 0; i < n; ++i) base.x[0][i] = x0[i];
    scatter(base, P);
    const int ncases = (int)raw[at++];
    int total_bad = 0;
    for (int k = 0; k < ncases; ++k) {
        const double *c = &raw[at]; at += 16;
        IterModelArgs m = {};
        m.model = (int)c[0]; m.a[0] = c[1] >= 0 ? 2 * (int64_t)c[1] : -1; m.a[1] = c[2] >= 0 ? 2 * (int64_t)c[2] : -1;
        m.anchor[0] = c[4]; m.anchor[1] = c[5]; m.z[0] = c[6]; m.z[1] = c[7];
        for (int q = 0; q < 4; ++q) m.R[q] = c[8 + q];
        m.gate = c[12]; m.iterations = (int)c[13]; m.tol = c[14];
        m.n_mm = 2 * N; m.cur = base.cur; m.npend = 0; m.pstart = 0;
        Store A(base), B(base);
        A.sync(); B.sync();
        double recA[8], itA[16], recP[8], itP[16], recB[8];
        int64_t cntA[2] = { 0, 0 }, cntB[2] = { 0, 0 };
        DevState stA = A.st, stB = B.st;
        // the probe: one workgroup of 64 lanes twice (pass 0: the operands), no lane exchange; the launches: run_linear's three passes
        launch_wg(1, { 2, -1, nullptr, 64 }, [&] { k_model_iter_probe<double>(stA, m, recP, itP); });
        launch_wg(A.grid(), { 3, 2, cntA }, [&] { k_gather_model_iter<double>(stA, m, recA, cntA, itA); });
        A.flip();
        int bad = 0;
        if (memcmp(recA, recP, sizeof recA) || memcmp(itA, itP, sizeof itA)) { printf("  the probe's records differ from the launch's\n"); ++bad; }
        if (m.iterations == 1) {
            const ModelArgs &plain = m;
            launch_wg(B.grid(), { 3, 2, cntB }, [&] { k_gather_model<double>(stB, plain, recB, cntB); });
            B.flip();
            if (memcmp(recA, recB, sizeof recA)) { printf("  the record differs from k_gather_model's\n"); ++bad; }
            if (cntA[0] != cntB[0] || cntA[1] != cntB[1]) { printf("  the counters differ\n"); ++bad; }
            bad += differ(A.x[A.cur], B.x[B.cur], "x") + differ(A.strip[A.cur], B.strip[B.cur], "strip") + differ(A.prr[A.cur], B.prr[B.cur], "prr") +
                   differ(A.diag[A.dcur], B.diag[B.dcur], "diag") + differ(A.ring, B.ring, "pair ring");
        }
        bad += differ(A.tiles, base.tiles, "tiles") + differ(A.x[base.cur], base.x[base.cur], "the x read") + differ(A.strip[base.cur], base.strip[base.cur], "the strip read");
        FILE *f = fopen((dir + "/case_" + std::to_string(k) + ".bin").c_str(), "wb");
        if (!f) return 2;
        put(f, A.x[A.cur].data(), n); put(f, A.prr[A.cur].data(), 9);
        for (int r = 0; r < 3; ++r) put(f, A.strip[A.cur].data() + r * A.ldm, 2 * N);
        put(f, A.diag[A.dcur].data(), 3 * N);
        put(f, A.st.Gp, 4 * N); put(f, A.st.Kp, 4 * N);
        put(f, recA, 8); put(f, itA, 16);
        const double cnt[2] = { (double)cntA[0], (double)cntA[1] };
        put(f, cnt, 2);
        fclose(f);
        printf("case %d (model %d, %d linearisations): %d differences\n", k, m.model, m.iterations, bad);
        total_bad += bad;
    }
    return total_bad != 0;
}
