// What the host emulations of tests/support share beyond the shim (include it after kernel_host_shim.h; it brings in tile_access.h,
// pair_column.h, constrain.h and linear_obs.h, the kernel sources it names itself): Store, the host image of DevState; scatter and fill, a
// dense symmetric P laid out as the kernels read it; launch_wg, the one workgroup runner; run_linear, differ, put and rnd.
// One Store serves all five programs.  The ring capacity is a constructor argument.  s and small are always there, because no kernel
// emulated here asks whether either pointer is set; k_predict_model reads no tile, diagonal block or pair, so its program uses the same
// Store with tiles of edge 16 and fills the buffers its kernel writes with a poison value (poison()).  The second tile store that a
// compaction writes is the caller's own vector, swapped in afterwards (merge_batch_host_emulation.cpp).
#pragma once
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>
#include "tile_access.h"
#include "pair_column.h"
#include "constrain.h"
#include "linear_obs.h"

// Every workgroup of the grid `passes` times over its `lanes` lanes, one lane after another: a pass leaves in the shared storage what the
// next one's first statements read, and the last pass is the launch.  Pass `replay` (none: -1) is the one in which lane_xor1 returns what
// the partner lane recorded in the pass before; every pass in front of it records, on cleared recordings, so that only the last of them
// is replayed.  What the earlier passes counted in cnt (the kernel's two counters, if given) is dropped: cnt is put back before each pass.
struct Passes { int passes, replay; int64_t *cnt = nullptr; int lanes = kBlock; };
template <typename F> static void launch_wg(int grid, Passes p, F body) {
    for (int b = 0; b < grid; ++b) {
        const int64_t c0 = p.cnt ? p.cnt[0] : 0, c1 = p.cnt ? p.cnt[1] : 0;
        for (int pass = 0; pass < p.passes; ++pass) {
            xor_pass = pass == p.replay;
            if (pass < p.replay) for (int t = 0; t < kBlock; ++t) { xor_rec[t].clear(); xor_pos[t] = 0; }
            if (p.cnt) { p.cnt[0] = c0; p.cnt[1] = c1; }
            for (int t = 0; t < p.lanes; ++t) { blockIdx.x = b; threadIdx.x = t; body(); }
        }
    }
}

// The host image of DevState: two copies each of x, Prr, the strip and the diagonal blocks, the tiles (TS: double or float), the ring of
// pcap pairs behind Gp / Kp, s and small.  A copy of a Store still points into the original: sync() it first.
template <typename TS = double> struct Store {
    int T, N, ldm, nt_cap, cap, pcap; TileMap tm; int64_t slots;
    std::vector<double> x[2], prr[2], strip[2], diag[2], ring, s, small; std::vector<TS> tiles; int cur = 0, dcur = 0;
    DevState st;
    Store(int T_, int N_, int cap_, int pcap_ = 8) : T(T_), N(N_), cap(cap_), pcap(pcap_) {
        tm = ekf_make_tilemap(T, 1, 0); nt_cap = (int)ekf_tiles_for(2 * cap, T); ldm = nt_cap * T; slots = tm.row_base(nt_cap);
        for (int b = 0; b < 2; ++b) { x[b].assign(3 + ldm, 0); prr[b].assign(16, 0); strip[b].assign(3 * ldm, 0); diag[b].assign(3 * cap, 0); }
        tiles.assign(slots * T * T, 0); ring.assign((size_t)2 * ldm * pcap * 2, 0); s.assign(cap, 0); small.assign(32, 0);
        sync();
    }
    void sync() {
        st = DevState();
        for (int b = 0; b < 2; ++b) { st.x[b] = x[b].data(); st.prr[b] = prr[b].data(); st.strip[b] = strip[b].data(); st.diag[b] = diag[b].data(); }
        st.tiles = tiles.data(); st.s = s.data(); st.Gp = ring.data(); st.Kp = ring.data() + (size_t)2 * ldm * pcap; st.Gp32 = st.Kp32 = nullptr;
        st.pair_stride = 2 * ldm; st.pcap = pcap; st.small = small.data(); st.ldm = ldm; st.tm = tm; st.dcur = dcur;
    }
    // v in every entry of x, Prr, the strip and small, so that a write beyond the live columns shows
    void poison(double v) {
        for (int b = 0; b < 2; ++b) { x[b].assign(x[b].size(), v); prr[b].assign(prr[b].size(), v); strip[b].assign(strip[b].size(), v); }
        small.assign(small.size(), v);
    }
    TS &tile(int64_t r, int64_t c) { return tiles[tm.tile_offset(r >> tm.shift, c >> tm.shift) + ((r & (T - 1)) << tm.shift) + (c & (T - 1))]; }
    void flip() { cur ^= 1; dcur ^= 1; sync(); }
    int grid() const { const int g = (int)((tm.padded(2 * N) + kBlock - 1) / kBlock); return g > 0 ? g : 1; }
    // live P(3 + r, 3 + c), r >= c, of the landmark block: the own blocks from the F64 copies, everything else the tile with the
    // `pending` pairs of ring slots 0 .. applied in slot order (rows that did not exist when a pair was formed have K = 0)
    double live(int64_t r, int64_t c, int pending) {
        if ((r >> 1) == (c >> 1)) return diag[dcur][3 * (r >> 1) + (r & 1) + (c & 1)];
        double v = (double)tile(r, c);
        for (int i = 0; i < pending; ++i) {
            const double *G = st.Gp + (size_t)i * st.pair_stride, *K = st.Kp + (size_t)i * st.pair_stride;
            v = rank2_apply(v, make_double2(K[2 * r], K[2 * r + 1]), make_double2(G[2 * c], G[2 * c + 1]));
        }
        return v;
    }
};

// A dense symmetric P, asked for as P(r, c) with r >= c, into buffer 0 of Prr, the strip and the diagonal blocks and into the tiles (the
// lower triangle, diagonal tiles whole)
template <typename TS, typename F> static void scatter(Store<TS> &S, F P) {
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) S.prr[0][3 * r + c] = P(r > c ? r : c, r > c ? c : r);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 2 * S.N; ++c) S.strip[0][r * S.ldm + c] = P(3 + c, r);
    for (int r = 0; r < 2 * S.N; ++r) for (int c = 0; c < 2 * S.N; ++c) {
        const bool diag = (r / S.T) == (c / S.T);
        if (c > r && !diag) continue;
        S.tile(r, c) = (TS)P(3 + (r > c ? r : c), 3 + (r > c ? c : r));
    }
    for (int k = 0; k < S.N; ++k) { S.diag[0][3 * k] = P(3 + 2 * k, 3 + 2 * k); S.diag[0][3 * k + 1] = P(4 + 2 * k, 3 + 2 * k); S.diag[0][3 * k + 2] = P(4 + 2 * k, 4 + 2 * k); }
}
static double rnd() { return (rand() % 20001 - 10000) / 10000.0; }
// P = D + U U' (k = 3), x random, s = 1 .. N; tiles, strip, prr, diag consistent.  The draws after srand(seed), in this order: U, D, x and,
// if asked for, a heading of 137 +- 40 degrees in place of x[2] -- a program's later rnd() calls go on from there.
template <typename TS> static void fill(Store<TS> &S, unsigned seed, bool heading) {
    srand(seed);
    const int n = 3 + 2 * S.N;
    std::vector<double> U(n * 3), d(n);
    for (auto &v : U) v = 0.3 * rnd();
    for (auto &v : d) v = 0.1 + 0.05 * (rnd() + 1);
    for (int i = 0; i < n; ++i) S.x[0][i] = 20 * rnd();
    if (heading) S.x[0][2] = 137.0 + 40 * rnd();
    for (int k = 0; k < S.N; ++k) S.s[k] = k + 1.0;
    scatter(S, [&](int r, int c) { double v = r == c ? d[r] : 0; for (int k = 0; k < 3; ++k) v += U[r * 3 + k] * U[c * 3 + k]; return v; });
}

// k_gather_linear, and k_gather_model / k_gather_model_iter where their programs launch them: every workgroup three times -- the first pass
// leaves the small part's operands in the shared storage, the second one has lane 0 form the shared solve (and a model's H) from them and
// records what lane_xor1 hands over, the third one is the launch
template <typename TS> static void run_linear(Store<TS> &S, LinearArgs a, double *rec, int64_t *cnt) {
    a.n_mm = 2 * S.N; a.cur = S.cur; a.pstart = 0;
    DevState st = S.st;
    launch_wg(S.grid(), { 3, 2, cnt }, [&] { k_gather_linear<TS>(st, a, rec, cnt); });
    S.flip();
}
template <typename V> static int differ(const std::vector<V> &u, const std::vector<V> &v, const char *what) {
    int b = 0;
    for (size_t i = 0; i < u.size(); ++i) if (memcmp(&u[i], &v[i], sizeof(V))) ++b;
    if (b) printf("  %s: %d differ\n", what, b);
    return b;
}
static void put(FILE *f, const double *v, size_t n) { fwrite(v, 8, n, f); }
