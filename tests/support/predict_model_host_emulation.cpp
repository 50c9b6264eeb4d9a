// Host emulation of k_predict_model (tests/test_predict_model_cpu.py compiles and runs it; no GPU, no HIP runtime).
// The kernel SOURCES of ekf_slam_amd/csrc (predict.h, predict_model.h) are compiled for the host behind kernel_host_shim.h -- thread indices
// as globals, __shared__ as static storage, every workgroup run twice, so that what its first lanes leave in the shared storage is there.
// predict.h comes in whole: what k_predict_mfma names of the matrix cores is a stand-in here, and that kernel is never run.
// For N = 0, 1 and 150 landmarks (300 columns: two workgroups, the second partly idle) and the first m = 1, 2, 9, 32 steps of the chain in
// argv[1]/chain.bin (32 steps of 13 doubles: model, u[3], M row-major 3 x 3; tests/predict_model_cases.py builds it):
//   the batch:   one launch with m steps
//   the singles: m launches of one step each
// must leave x, Prr, the strip and Q BIT FOR BIT the same, the buffer the launch read untouched, row 2 of the strip and the landmarks'
// entries of x as they were.  Each state before and each case's state after are written to argv[1] for the dense restatement.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "kernel_host_shim.h"
static Idx gridDim;
#define ext_vector_type(n) vector_size(8 * n)
#define __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, x, y, z) (c)
#include "emulated_state.h"
#include "predict.h"
#include "predict_model.h"

// k_predict_model: every workgroup twice -- the first run leaves fa and fb of every step in the shared storage; no lane exchange
static void run_predict(Store<> &S, const PredictModelStep *e, int m) {
    PredictModelArgs a = {};
    a.n_mm = 2 * S.N; a.m = m; a.cur = S.cur;
    for (int b = 0; b < m; ++b) a.e[b] = e[b];
    DevState st = S.st;
    const int cols = 2 * S.N > 0 ? 2 * S.N : 1;
    launch_wg((cols + kBlock - 1) / kBlock, { 2, -1 }, [&] { k_predict_model(st, a); });
    S.cur ^= 1;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    std::vector<double> raw(32 * 13);
    {
        FILE *f = fopen((dir + "/chain.bin").c_str(), "rb");
        if (!f || fread(raw.data(), 8, raw.size(), f) != raw.size()) return 2;
        fclose(f);
    }
    PredictModelStep e[kPredictModelMax] = {};
    for (int b = 0; b < 32; ++b) {
        const double *r = raw.data() + 13 * b, *M = r + 4;
        e[b].model = (int)r[0];
        for (int q = 0; q < 3; ++q) e[b].u[q] = r[1 + q];
        const double m6[6] = { M[0], M[3], M[4], M[6], M[7], M[8] };
        for (int q = 0; q < 6; ++q) e[b].m6[q] = m6[q];
    }
    int total_bad = 0;
    for (int N : { 0, 1, 150 }) {
        Store<> base(16, N, N + 8);                           // (ldm: the 2 N columns and at least one more, rounded up to 16)
        base.poison(-7.0);
        fill(base, 13, true);
        const int n0 = 3 + 2 * N;
        {
            FILE *f = fopen((dir + "/before_" + std::to_string(N) + ".bin").c_str(), "wb");
            if (!f) return 2;
            put(f, base.x[0].data(), n0); put(f, base.prr[0].data(), 9);
            for (int r = 0; r < 3; ++r) put(f, base.strip[0].data() + r * base.ldm, 2 * N);
            fclose(f);
        }
        for (int m : { 1, 2, 9, 32 }) {
            Store A(base), B(base);
            A.sync(); B.sync();
            run_predict(A, e, m);
            for (int b = 0; b < m; ++b) run_predict(B, e + b, 1);
            int bad = 0;
            // (the singles end in buffer m & 1; what lies beyond the live columns is never written: compare the live part)
            const std::vector<double> &ax = A.x[A.cur], &bx = B.x[B.cur], &as = A.strip[A.cur], &bs = B.strip[B.cur];
            for (int i = 0; i < n0; ++i) if (memcmp(&ax[i], &bx[i], 8)) { ++bad; printf("  x[%d] differs\n", i); }
            for (int r = 0; r < 3; ++r) for (int c = 0; c < 2 * N; ++c) if (memcmp(&as[r * A.ldm + c], &bs[r * B.ldm + c], 8)) ++bad;
            bad += differ(A.prr[A.cur], B.prr[B.cur], "prr") + differ(A.small, B.small, "small");
            // the buffer the batch read is as it was; row 2 of the strip and the landmarks did not move; nothing beyond the live columns
            bad += differ(A.x[0], base.x[0], "the x read") + differ(A.prr[0], base.prr[0], "the prr read") + differ(A.strip[0], base.strip[0], "the strip read");
            for (int i = 3; i < n0; ++i) if (ax[i] != base.x[0][i]) ++bad;
            for (int c = 0; c < 2 * N; ++c) if (as[2 * A.ldm + c] != base.strip[0][2 * base.ldm + c]) ++bad;
            for (int i = n0; i < 3 + A.ldm; ++i) if (ax[i] != -7.0) ++bad;
            for (int r = 0; r < 3; ++r) for (int c = 2 * N; c < A.ldm; ++c) if (as[r * A.ldm + c] != -7.0) ++bad;
            for (int i = 0; i < 32; ++i) if ((i < 12 || i >= 21) && A.small[i] != -7.0) ++bad;
            for (int r = 0; r < 3; ++r) for (int c = 0; c < r; ++c) if (A.prr[A.cur][3 * r + c] != A.prr[A.cur][3 * c + r]) ++bad;
            FILE *f = fopen((dir + "/after_" + std::to_string(N) + "_" + std::to_string(m) + ".bin").c_str(), "wb");
            if (!f) return 2;
            put(f, ax.data(), n0); put(f, A.prr[A.cur].data(), 9);
            for (int r = 0; r < 3; ++r) put(f, as.data() + r * A.ldm, 2 * N);
            put(f, A.small.data() + 12, 9);
            fclose(f);
            printf("N=%d m=%d: %d differences\n", N, m, bad);
            total_bad += bad;
        }
    }
    return total_bad != 0;
}
