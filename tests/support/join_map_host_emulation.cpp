// Host emulation of k_join_state and k_join_rows (tests/test_join_map_cpu.py compiles and runs it; no GPU, no HIP runtime).
// The kernel SOURCES of ekf_slam_amd/csrc (predict.h, predict_model.h, append.h, append_model.h, join_map.h) are compiled for the host behind
// kernel_host_shim.h -- thread indices as globals, __shared__ as static storage, every workgroup run twice, so that what its lane 0 leaves in
// the shared storage is there.  Two Stores of emulated_state.h hold the two states: the global one with tiles of edge 16, the local one with
// tiles of edge 32, each with double or float tiles (the four instances of k_join_rows).  For (N, M) = (0, 3), (5, 1), (8, 8), (13, 21) --
// a tile row of edge 16 holds 8 landmarks, so the new rows start inside a tile row, on its edge and span several -- each case checks here
// that the launches wrote nothing they do not own (the buffer they read, every tile row below 2 N, the whole local state) and that both
// kernels leave the same bits in the new landmarks' live diagonal copies, and writes both states before and the joined state after to
// argv[1] for the dense restatement of tests/join_map_cases.py.
// What append.h's k_append and predict.h's k_predict_mfma name besides the argument blocks is a stand-in: neither is run here.
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
void reduce_partials_wave(const AssocHostPartial *parts, int nblk, int seq, int lane, double &ll, int &ix);
void store_partial(AssocHostPartial *dst, double ll, int index, int seq);
#include "emulated_state.h"
#include "predict.h"
#include "predict_model.h"
#include "append.h"
#include "append_model.h"
#include "join_map.h"

// the live dense P of a flushed Store (row-major, both triangles)
template <typename TS> static std::vector<double> dense(Store<TS> &S) {
    const int n = 3 + 2 * S.N;
    std::vector<double> P((size_t)n * n);
    for (int r = 0; r < n; ++r) for (int c = 0; c <= r; ++c) {
        double v;
        if (r < 3) v = S.prr[S.cur][3 * r + c];
        else if (c < 3) v = S.strip[S.cur][c * S.ldm + (r - 3)];
        else v = S.live(r - 3, c - 3, 0);
        P[(size_t)r * n + c] = P[(size_t)c * n + r] = v;
    }
    return P;
}
template <typename TS> static void put_state(FILE *f, Store<TS> &S) {
    const int n = 3 + 2 * S.N;
    put(f, S.x[S.cur].data(), n);
    put(f, S.s.data(), S.N);
    const std::vector<double> P = dense(S);
    put(f, P.data(), P.size());
}

template <typename TD, typename TSRC> static int run_case(const char *name, const std::string &dir, int N, int M) {
    const int cap = N + M + 3;
    Store<TD> G(16, N, cap);
    fill(G, 21 + N, true);
    Store<TSRC> Lo(32, M, M + 5);
    fill(Lo, 77 + M, false);
    // a local robot pose near the origin of its frame, as a submap's is
    Lo.x[0][0] = 0.8; Lo.x[0][1] = -0.45; Lo.x[0][2] = 11.5;
    const double offset = 1000.0;
    FILE *f = fopen((dir + "/" + name + "_" + std::to_string(N) + "_" + std::to_string(M) + ".bin").c_str(), "wb");
    if (!f) return 1000;
    const double hdr[3] = { (double)N, (double)M, offset };
    put(f, hdr, 3);
    put_state(f, G);
    put_state(f, Lo);
    const Store<TD> G0(G);
    const Store<TSRC> L0(Lo);
    JoinMapArgs a = {};
    a.N = N; a.M = M; a.signature_offset = offset; a.cur = G.cur; a.lcur = Lo.cur;
    const DevState st = G.st, lo = Lo.st;
    launch_wg((2 * (N + M) + kBlock - 1) / kBlock > 0 ? (2 * (N + M) + kBlock - 1) / kBlock : 1, { 2, -1 }, [&] { k_join_state(st, lo, a); });
    int bad = 0;
    const std::vector<double> diag_state = G.diag[G.dcur];
    // poison what the first launch left of the new diagonal copies: the second launch must write the same bits on its own
    for (int k = 3 * N; k < 3 * (N + M); ++k) G.diag[G.dcur][k] = -7.0;
    const int per_row = (N + M + kBlock - 1) / kBlock;
    if (M > 0) launch_wg(M * per_row, { 2, -1 }, [&] { k_join_rows<TD, TSRC>(st, lo, a, per_row); });
    if (M > 0) bad += differ(G.diag[G.dcur], diag_state, "the diagonal copies of the two launches");
    else G.diag[G.dcur] = diag_state;
    // what the launches do not own: the buffer they read, the other diagonal buffer, every tile row below 2 N, the ring, the local state
    bad += differ(G.x[G.cur], G0.x[G0.cur], "the x read") + differ(G.prr[G.cur], G0.prr[G0.cur], "the prr read") +
           differ(G.strip[G.cur], G0.strip[G0.cur], "the strip read") + differ(G.diag[G.dcur ^ 1], G0.diag[G0.dcur ^ 1], "the other diag") +
           differ(G.ring, G0.ring, "pair ring") + differ(G.small, G0.small, "small");
    for (int k = 0; k < 3 * N; ++k) if (G.diag[G.dcur][k] != G0.diag[G0.dcur][k]) ++bad;
    for (int k = 0; k < N; ++k) if (G.s[k] != G0.s[k]) ++bad;
    {
        const int64_t below = G.tm.tile_offset((2 * N) >> G.tm.shift, 0);          // whole tile rows below the first new row
        for (int64_t e = 0; e < below; ++e) if (memcmp(&G.tiles[e], &G0.tiles[e], sizeof(TD))) ++bad;
        for (int r = 0; r < 2 * N; ++r) for (int c = 0; c <= r; ++c) {
            Store<TD> &g0 = const_cast<Store<TD> &>(G0);
            if (memcmp(&G.tile(r, c), &g0.tile(r, c), sizeof(TD))) ++bad;
        }
        // beyond the new map nothing was written: columns above the row's own landmark within the new rows stay zero
        for (int r = 2 * N; r < 2 * (N + M); ++r) for (int c = (r | 1) + 1; c < (int)G.tm.padded(r + 1); ++c) if ((double)G.tile(r, c) != 0.0) ++bad;
    }
    bad += differ(Lo.tiles, L0.tiles, "local tiles") + differ(Lo.s, L0.s, "local s");
    for (int q = 0; q < 2; ++q)
        bad += differ(Lo.x[q], L0.x[q], "local x") + differ(Lo.strip[q], L0.strip[q], "local strip") + differ(Lo.diag[q], L0.diag[q], "local diag") +
               differ(Lo.prr[q], L0.prr[q], "local prr");
    // the robot block is left exactly symmetric
    for (int r = 0; r < 3; ++r) for (int c = 0; c < r; ++c) if (G.prr[G.cur ^ 1][3 * r + c] != G.prr[G.cur ^ 1][3 * c + r]) ++bad;
    G.cur ^= 1; G.N += M; G.sync();
    put_state(f, G);
    fclose(f);
    printf("%s N=%d M=%d: %d differences\n", name, N, M, bad);
    return bad;
}

template <typename TD, typename TSRC> static int run_cases(const char *name, const std::string &dir) {
    int bad = 0;
    const int cases[4][2] = { { 0, 3 }, { 5, 1 }, { 8, 8 }, { 13, 21 } };
    for (const auto &c : cases) bad += run_case<TD, TSRC>(name, dir, c[0], c[1]);
    return bad;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    const int bad = run_cases<double, double>("dd", dir) + run_cases<double, float>("df", dir) + run_cases<float, double>("fd", dir) +
                    run_cases<float, float>("ff", dir);
    return bad != 0;
}
