// Host emulation of k_extract_state and k_extract_rows (tests/test_extract_map_cpu.py compiles and runs it; no GPU, no HIP runtime).
// The kernel SOURCES of ekf_slam_amd/csrc (predict.h, predict_model.h, append.h, append_model.h, join_map.h, extract_map.h) are compiled for
// the host behind kernel_host_shim.h -- thread indices as globals, __shared__ as static storage, every workgroup run twice, so that what its
// lane 0 leaves in the shared storage is there.  Two Stores of emulated_state.h hold the two states: the source with tiles of edge 32, the
// destination with tiles of edge 16, each with double or float tiles (the four instances of k_extract_rows), both frames.  The cases -- one
// line "N m idx[0] .. idx[m-1]" each -- are read from argv[1]/cases.txt, so that the index plans are those of tests/extract_map_cases.py.
// The destination starts out POISONED everywhere; each case checks here that the launches wrote nothing they do not own (the whole source
// state, the destination's other buffers, every tile behind the last active tile row, x and the strip behind its last column), that nothing
// they own keeps the poison, that everything from landmark m on is zero and that both halves of every diagonal tile agree, and writes the
// source state and the extracted state to argv[1] for the dense restatement.
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

constexpr double kPoison = -7.0;

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

template <typename TD, typename TSRC>
static int run_case(const char *name, const std::string &dir, int N, const std::vector<int32_t> &idx, int frame) {
    const int m = (int)idx.size();
    Store<TSRC> Src(32, N, N + 3);
    fill(Src, 41 + N, true);
    Src.x[0][3 + 2 * 1] = Src.x[0][0]; Src.x[0][4 + 2 * 1] = Src.x[0][1];      // landmark 1 exactly on the robot: regular here
    Store<TD> D(16, 0, (m > 0 ? m : 1) + 2);
    D.poison(kPoison);
    for (int b = 0; b < 2; ++b) D.diag[b].assign(D.diag[b].size(), kPoison);
    D.tiles.assign(D.tiles.size(), (TD)kPoison);
    D.s.assign(D.s.size(), kPoison);
    const Store<TSRC> S0(Src);
    const Store<TD> D0(D);
    FILE *f = fopen((dir + "/" + name + "_" + std::to_string(frame) + "_" + std::to_string(N) + "_" + std::to_string(m) + ".bin").c_str(), "wb");
    if (!f) return 1000;
    const double hdr[3] = { (double)N, (double)m, (double)frame };
    put(f, hdr, 3);
    for (int k = 0; k < m; ++k) { const double v = idx[k]; put(f, &v, 1); }
    put_state(f, Src);
    ExtractMapArgs a = {};
    a.m = m; a.cols = D.tm.padded(2 * m); a.frame = frame; a.scur = Src.cur; a.dcur = D.cur;
    const DevState dst = D.st, src = Src.st;
    const int32_t *ix = idx.data();
    const int cols = (int)a.cols;
    launch_wg(cols > 0 ? (cols + kBlock - 1) / kBlock : 1, { 2, -1 }, [&] { k_extract_state(dst, src, a, ix); });
    const int rows = cols / 2, per_row = (rows + kBlock - 1) / kBlock;
    if (m > 0) launch_wg(rows * per_row, { 2, -1 }, [&] { k_extract_rows<TD, TSRC>(dst, src, a, ix, per_row); });
    int bad = 0;
    // the source: every buffer as it was
    bad += differ(Src.tiles, S0.tiles, "source tiles") + differ(Src.s, S0.s, "source s") + differ(Src.ring, S0.ring, "source ring");
    for (int q = 0; q < 2; ++q)
        bad += differ(Src.x[q], S0.x[q], "source x") + differ(Src.strip[q], S0.strip[q], "source strip") + differ(Src.diag[q], S0.diag[q], "source diag") +
               differ(Src.prr[q], S0.prr[q], "source prr");
    // the destination's other buffers, its ring, and what lies behind the columns and the tile rows the launches own
    bad += differ(D.x[D.cur ^ 1], D0.x[D0.cur ^ 1], "the other x") + differ(D.strip[D.cur ^ 1], D0.strip[D0.cur ^ 1], "the other strip") +
           differ(D.prr[D.cur ^ 1], D0.prr[D0.cur ^ 1], "the other prr") + differ(D.diag[D.dcur ^ 1], D0.diag[D0.dcur ^ 1], "the other diag") +
           differ(D.ring, D0.ring, "pair ring");
    for (int c = cols; c < D.ldm; ++c) {
        if (D.x[D.cur][3 + c] != kPoison) ++bad;
        for (int r = 0; r < 3; ++r) if (D.strip[D.cur][r * D.ldm + c] != kPoison) ++bad;
    }
    for (int k = m; k < D.cap; ++k) {
        if (D.s[k] != kPoison) ++bad;
        for (int q = 0; q < 3; ++q) if (D.diag[D.dcur][3 * k + q] != kPoison) ++bad;
    }
    const int64_t owned = D.tm.tile_offset(cols >> D.tm.shift, 0);               // whole tile rows 0 .. padded(2 m) / T - 1
    for (int64_t e = owned; e < (int64_t)D.tiles.size(); ++e) if ((double)D.tiles[e] != kPoison) ++bad;
    // what they own: no poison left, zero from landmark m on, diagonal tiles whole and symmetric bit for bit
    for (int64_t e = 0; e < owned; ++e) if ((double)D.tiles[e] == kPoison) ++bad;
    for (int c = 0; c < cols; ++c) {
        const bool live = c < 2 * m;
        if (D.x[D.cur][3 + c] == kPoison || (!live && D.x[D.cur][3 + c] != 0.0)) ++bad;
        for (int r = 0; r < 3; ++r) { const double v = D.strip[D.cur][r * D.ldm + c]; if (v == kPoison || (!live && v != 0.0)) ++bad; }
    }
    for (int i = 0; i < 3; ++i) if (D.x[D.cur][i] == kPoison) ++bad;
    for (int i = 0; i < 9; ++i) if (D.prr[D.cur][i] == kPoison) ++bad;
    for (int r = 0; r < cols; ++r) {
        const int tile_end = ((r >> D.tm.shift) + 1) << D.tm.shift;
        for (int c = 0; c < tile_end; ++c) {
            if (c > r && (c >> D.tm.shift) != (r >> D.tm.shift)) continue;
            const TD v = D.tile(r, c);
            if ((r >= 2 * m || c >= 2 * m) && (double)v != 0.0) ++bad;
            if ((c >> D.tm.shift) == (r >> D.tm.shift)) { const TD w = D.tile(c, r); if (memcmp(&v, &w, sizeof(TD))) ++bad; }
        }
    }
    // the tile's own copy of a landmark's block is the live diagonal copy, rounded to the store
    for (int k = 0; k < m; ++k) {
        const double *dg = &D.diag[D.dcur][3 * k];
        const TD want[4] = { (TD)dg[0], (TD)dg[1], (TD)dg[1], (TD)dg[2] };
        const TD got[4] = { D.tile(2 * k, 2 * k), D.tile(2 * k, 2 * k + 1), D.tile(2 * k + 1, 2 * k), D.tile(2 * k + 1, 2 * k + 1) };
        if (memcmp(want, got, sizeof want)) ++bad;
    }
    D.N = m;
    put_state(f, D);
    fclose(f);
    printf("%s frame=%d N=%d m=%d: %d differences\n", name, frame, N, m, bad);
    return bad;
}

struct Case { int N; std::vector<int32_t> idx; };

template <typename TD, typename TSRC> static int run_cases(const char *name, const std::string &dir, const std::vector<Case> &cases) {
    int bad = 0;
    for (const Case &c : cases) for (int frame = 0; frame < 2; ++frame) bad += run_case<TD, TSRC>(name, dir, c.N, c.idx, frame);
    return bad;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    std::vector<Case> cases;
    FILE *f = fopen((dir + "/cases.txt").c_str(), "r");
    if (!f) return 3;
    int N, m;
    while (fscanf(f, "%d %d", &N, &m) == 2) {
        Case c; c.N = N;
        for (int k = 0; k < m; ++k) { int v; if (fscanf(f, "%d", &v) != 1 || v < 0 || v >= N) { fclose(f); return 4; } c.idx.push_back(v); }
        cases.push_back(c);
    }
    fclose(f);
    if (cases.empty()) return 5;
    const int bad = run_cases<double, double>("dd", dir, cases) + run_cases<double, float>("df", dir, cases) +
                    run_cases<float, double>("fd", dir, cases) + run_cases<float, float>("ff", dir, cases);
    return bad != 0;
}
