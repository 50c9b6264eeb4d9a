// Host emulation of k_transform_state and k_transform_tiles (tests/test_transform_map_cpu.py compiles and runs it; no GPU, no HIP runtime).
// The kernel SOURCES of ekf_slam_amd/csrc (predict.h, predict_model.h, append.h, append_model.h, join_map.h, extract_map.h, transform_map.h)
// are compiled for the host behind kernel_host_shim.h -- thread indices as globals, __shared__ as static storage.  k_transform_tiles works IN
// PLACE, so each of its workgroups runs ONCE: its lane 0 comes first and leaves the shared storage for the others.  The cases -- one line
// "name T float N form tx ty phi S00 .. S22" each -- are read from argv[1]/cases.txt, so that the transforms are those of the test.
// The buffers k_transform_state writes start out POISONED; each case checks here that the launches wrote nothing they do not own (the
// buffers they read, s, the pair ring, every tile behind the last active tile row, x and the strip behind the last column), that nothing
// they own keeps the poison, that everything from landmark N on is still zero, that both halves of every diagonal tile agree bit for bit
// and that the tile's own copy of a landmark's block is its diagonal copy rounded to the store.  The robot form is also compared, bit for
// bit, with k_extract_state / k_extract_rows over all landmarks into a store of the same tile edge and kind.  The state before and after
// goes to argv[1] for the dense restatement.
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
#include "extract_map.h"
#include "transform_map.h"

constexpr double kPoison = -7.0;

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

template <int kForm, typename TS> static void launch(Store<TS> &S, const TransformMapArgs &a) {
    const DevState st = S.st;
    const int cols = (int)a.cols;
    launch_wg(cols > 0 ? (cols + kBlock - 1) / kBlock : 1, { 2, -1 }, [&] { k_transform_state<kForm>(st, a); });
    if (S.N == 0) return;
    std::vector<int2> work;
    const int nt = cols / S.T;
    for (int I = 0; I < nt; ++I) for (int J = 0; J <= I; ++J) work.push_back({ I, J });
    const int per_row = S.T / Lane16<TS>::kCols, units = (S.T / 2) * per_row;
    const int items = (units + kBlock * kTransformUnits - 1) / (kBlock * kTransformUnits);
    const int2 *w = work.data();
    launch_wg((int)work.size() * items, { 1, -1 }, [&] { k_transform_tiles<TS, kForm>(st, a, w, items); });
}

struct Case { std::string name; int T, isfloat, N, form; double t[3], Sg[9]; };

template <typename TS> static int run_case(const Case &c, const std::string &dir) {
    const int N = c.N, T = c.T;
    Store<TS> S(T, N, N + 3);
    fill(S, 41 + N, true);
    if (N > 1) { S.x[0][3 + 2 * 1] = S.x[0][0]; S.x[0][4 + 2 * 1] = S.x[0][1]; }      // landmark 1 exactly on the robot: regular here
    for (int b : { 1 }) {
        S.x[b].assign(S.x[b].size(), kPoison); S.prr[b].assign(S.prr[b].size(), kPoison); S.strip[b].assign(S.strip[b].size(), kPoison);
        S.diag[b].assign(S.diag[b].size(), kPoison);
    }
    const Store<TS> S0(S);
    FILE *f = fopen((dir + "/" + c.name + ".bin").c_str(), "wb");
    if (!f) return 1000;
    const double hdr[2] = { (double)N, (double)c.form };
    put(f, hdr, 2);
    put_state(f, S);
    TransformMapArgs a = {};
    a.N = N; a.cols = S.tm.padded(2 * N); a.form = c.form; a.cur = S.cur;
    for (int i = 0; i < 3; ++i) a.t[i] = c.t[i];
    for (int i = 0; i < 9; ++i) a.Sigma[i] = c.Sg[i];
    if (c.form == 0) launch<0>(S, a); else if (c.form == 1) launch<1>(S, a); else launch<2>(S, a);
    int bad = 0;
    const int cols = (int)a.cols;
    // what the launches read stays: the old buffers, s, the ring
    bad += differ(S.x[0], S0.x[0], "old x") + differ(S.prr[0], S0.prr[0], "old prr") + differ(S.strip[0], S0.strip[0], "old strip") +
           differ(S.diag[0], S0.diag[0], "old diag") + differ(S.s, S0.s, "s") + differ(S.ring, S0.ring, "pair ring");
    // behind what they own
    for (int col = cols; col < S.ldm; ++col) {
        if (S.x[1][3 + col] != kPoison) ++bad;
        for (int r = 0; r < 3; ++r) if (S.strip[1][r * S.ldm + col] != kPoison) ++bad;
    }
    for (int k = N; k < S.cap; ++k) for (int q = 0; q < 3; ++q) if (S.diag[1][3 * k + q] != kPoison) ++bad;
    const int64_t owned = S.tm.tile_offset(cols >> S.tm.shift, 0);
    for (int64_t e = owned; e < (int64_t)S.tiles.size(); ++e) if (memcmp(&S.tiles[e], &S0.tiles[e], sizeof(TS))) ++bad;
    // what they own: no poison left, zero from landmark N on
    for (int col = 0; col < cols; ++col) {
        const bool live = col < 2 * N;
        if (S.x[1][3 + col] == kPoison || (!live && S.x[1][3 + col] != 0.0)) ++bad;
        for (int r = 0; r < 3; ++r) { const double v = S.strip[1][r * S.ldm + col]; if (v == kPoison || (!live && v != 0.0)) ++bad; }
    }
    for (int i = 0; i < 3; ++i) if (S.x[1][i] == kPoison) ++bad;
    for (int i = 0; i < 9; ++i) if (S.prr[1][i] == kPoison) ++bad;
    for (int k = 0; k < N; ++k) for (int q = 0; q < 3; ++q) if (S.diag[1][3 * k + q] == kPoison) ++bad;
    S.flip();
    for (int r = 0; r < cols; ++r) {
        const int tile_end = ((r >> S.tm.shift) + 1) << S.tm.shift;
        for (int col = 0; col < tile_end; ++col) {
            if (col > r && (col >> S.tm.shift) != (r >> S.tm.shift)) continue;
            const TS v = S.tile(r, col);
            if ((r >= 2 * N || col >= 2 * N) && (double)v != 0.0) ++bad;
            if ((col >> S.tm.shift) == (r >> S.tm.shift)) { const TS w = S.tile(col, r); if (memcmp(&v, &w, sizeof(TS))) ++bad; }
        }
    }
    for (int k = 0; k < N; ++k) {
        const double *dg = &S.diag[S.dcur][3 * k];
        const TS want[4] = { (TS)dg[0], (TS)dg[1], (TS)dg[1], (TS)dg[2] };
        const TS got[4] = { S.tile(2 * k, 2 * k), S.tile(2 * k, 2 * k + 1), S.tile(2 * k + 1, 2 * k), S.tile(2 * k + 1, 2 * k + 1) };
        if (memcmp(want, got, sizeof want)) ++bad;
    }
    int bad_extract = 0;
    if (c.form == 2) {
        // the same state through k_extract_state / k_extract_rows over all landmarks, into a store of the same tile edge and kind
        Store<TS> Src(S0);
        Src.sync();
        Store<TS> D(T, 0, N + 3);
        std::vector<int32_t> idx(N > 0 ? N : 1);
        for (int k = 0; k < N; ++k) idx[k] = k;
        ExtractMapArgs ea = {};
        ea.m = N; ea.cols = D.tm.padded(2 * N); ea.frame = 1; ea.scur = Src.cur; ea.dcur = D.cur;
        const DevState dst = D.st, src = Src.st;
        const int32_t *ix = idx.data();
        launch_wg(cols > 0 ? (cols + kBlock - 1) / kBlock : 1, { 2, -1 }, [&] { k_extract_state(dst, src, ea, ix); });
        const int rows = cols / 2, per_row = (rows + kBlock - 1) / kBlock;
        if (N > 0) launch_wg(rows * per_row, { 2, -1 }, [&] { k_extract_rows<TS, TS>(dst, src, ea, ix, per_row); });
        for (int i = 0; i < 3 + cols; ++i) if (memcmp(&S.x[S.cur][i], &D.x[D.cur][i], 8)) ++bad_extract;
        for (int i = 0; i < 9; ++i) if (memcmp(&S.prr[S.cur][i], &D.prr[D.cur][i], 8)) ++bad_extract;
        for (int r = 0; r < 3; ++r) for (int col = 0; col < cols; ++col) if (memcmp(&S.strip[S.cur][r * S.ldm + col], &D.strip[D.cur][r * D.ldm + col], 8)) ++bad_extract;
        for (int i = 0; i < 3 * N; ++i) if (memcmp(&S.diag[S.dcur][i], &D.diag[D.dcur][i], 8)) ++bad_extract;
        for (int i = 0; i < N; ++i) if (memcmp(&S.s[i], &D.s[i], 8)) ++bad_extract;
        for (int64_t e = 0; e < owned; ++e) if (memcmp(&S.tiles[e], &D.tiles[e], sizeof(TS))) ++bad_extract;
    } else {
        // x' against the library's own functions, bit for bit: POSE_DELTA at (xr = t, u = r), RELATIVE_XY's inverse at (t, l_i)
        double xn[3], fa, fb, V[9];
        const double r[3] = { S0.x[0][0], S0.x[0][1], S0.x[0][2] };
        ekfm::motion_eval(3, c.t, r, xn, fa, fb, V);
        for (int i = 0; i < 3; ++i) if (memcmp(&xn[i], &S.x[S.cur][i], 8)) ++bad_extract;
        for (int k = 0; k < N; ++k) {
            const double z[2] = { S0.x[0][3 + 2 * k], S0.x[0][4 + 2 * k] };
            double tp[2], gth[2], Gz[4];
            ekfm::model_invert(4, c.t, z, tp, gth, Gz);
            for (int j = 0; j < 2; ++j) if (memcmp(&tp[j], &S.x[S.cur][3 + 2 * k + j], 8)) ++bad_extract;
        }
    }
    put_state(f, S);
    fclose(f);
    printf("%s: %d differences, %d against the library's own\n", c.name.c_str(), bad, bad_extract);
    return bad + bad_extract;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    FILE *f = fopen((dir + "/cases.txt").c_str(), "r");
    if (!f) return 3;
    int bad = 0, n = 0;
    char name[128];
    Case c;
    while (fscanf(f, "%127s %d %d %d %d", name, &c.T, &c.isfloat, &c.N, &c.form) == 5) {
        for (int i = 0; i < 3; ++i) if (fscanf(f, "%lf", &c.t[i]) != 1) { fclose(f); return 4; }
        for (int i = 0; i < 9; ++i) if (fscanf(f, "%lf", &c.Sg[i]) != 1) { fclose(f); return 4; }
        if ((c.T != 16 && c.T != 32) || c.N < 0 || c.N > 64 || c.form < 0 || c.form > 2) { fclose(f); return 4; }
        c.name = name;
        bad += c.isfloat ? run_case<float>(c, dir) : run_case<double>(c, dir);
        ++n;
    }
    fclose(f);
    if (n == 0) return 5;
    return bad != 0;
}
