// Host emulation of the batch-fusion kernels (tests/test_merge_batch_cpu.py compiles and runs it; no GPU, no HIP runtime).
// The kernel SOURCES of ekf_slam_amd/csrc (pair_column.h, constrain.h, compact.h, merge_pass.h, tile_access.h) are compiled for the host behind
// kernel_host_shim.h -- thread indices as globals, __shared__ as static storage with thread 0 of a workgroup run first, lane_xor1 in two
// passes -- and two routes are compared BIT FOR BIT on the same state:
//   the batch:    m x k_gather_constrain with a record (earlier pairs pending in the ring), then k_merge_pass
//   the sequence: m x (k_gather_constrain with npend = 0 and no record, the one-pair pass as a plain rank2_apply loop), then k_compact_tiles
// both followed by k_compact_state.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "kernel_host_shim.h"
#include "tile_access.h"
#include "compact.h"
#include "pair_column.h"
#include "constrain.h"
#include "merge_pass.h"

// FNV-1a over the bytes of a route's final state: printed in each line's parentheses, so that two builds of this file can be compared
static uint64_t fnv(uint64_t h, const double *p, size_t n) {
    const unsigned char *b = (const unsigned char *)p;
    for (size_t i = 0; i < 8 * n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}
template <typename F> static void launch_wg(int grid, F body) {      // thread 0 first (it fills the shared solve), two lane_xor1 passes
    for (int b = 0; b < grid; ++b) {
        for (int t = 0; t < kBlock; ++t) { xor_rec[t].clear(); xor_pos[t] = 0; }
        for (xor_pass = 0; xor_pass < 2; ++xor_pass)
            for (int t = 0; t < kBlock; ++t) { blockIdx.x = b; threadIdx.x = t; body(); }
    }
}
struct Store {
    int T, N, ldm, nt_cap; TileMap tm; int64_t slots;
    std::vector<double> x[2], prr[2], strip[2], diag[2], s, ring, tiles[2]; int cur = 0, dcur = 0, base = 0;
    DevState st;
    Store(int T_, int N_, int cap) : T(T_), N(N_) {
        tm = ekf_make_tilemap(T, 1, 0); nt_cap = (int)ekf_tiles_for(2 * cap, T); ldm = nt_cap * T; slots = tm.row_base(nt_cap);
        for (int b = 0; b < 2; ++b) { x[b].assign(3 + ldm, 0); prr[b].assign(16, 0); strip[b].assign(3 * ldm, 0); diag[b].assign(3 * cap, 0); tiles[b].assign(slots * T * T, 0); }
        s.assign(cap, 0); ring.assign((size_t)2 * ldm * 32 * 2, 0);
        sync();
    }
    void sync() {
        for (int b = 0; b < 2; ++b) { st.x[b] = x[b].data(); st.prr[b] = prr[b].data(); st.strip[b] = strip[b].data(); st.diag[b] = diag[b].data(); }
        st.tiles = tiles[base].data(); st.s = s.data(); st.Gp = ring.data(); st.Kp = ring.data() + (size_t)2 * ldm * 32; st.Gp32 = st.Kp32 = nullptr;
        st.pair_stride = 2 * ldm; st.pcap = 32; st.small = nullptr; st.ldm = ldm; st.tm = tm; st.dcur = dcur;
    }
    double &tile(int64_t r, int64_t c) { return tiles[base][tm.tile_offset(r >> tm.shift, c >> tm.shift) + ((r & (T - 1)) << tm.shift) + (c & (T - 1))]; }
};
static void fill(Store &S) {            // P = D + U U' (k = 3), x random; tiles, strip, prr, diag consistent
    srand(11);
    auto rnd = [] { return (rand() % 20001 - 10000) / 10000.0; };
    const int n = 3 + 2 * S.N;
    std::vector<double> U(n * 3), d(n);
    for (auto &v : U) v = 0.3 * rnd();
    for (auto &v : d) v = 0.1 + 0.05 * (rnd() + 1);
    auto P = [&](int r, int c) { double v = r == c ? d[r] : 0; for (int k = 0; k < 3; ++k) v += U[r * 3 + k] * U[c * 3 + k]; return v; };
    for (int i = 0; i < n; ++i) S.x[0][i] = 20 * rnd();
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) S.prr[0][3 * r + c] = P(r > c ? r : c, r > c ? c : r);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 2 * S.N; ++c) S.strip[0][r * S.ldm + c] = P(3 + c, r);
    for (int r = 0; r < 2 * S.N; ++r) for (int c = 0; c < 2 * S.N; ++c) {
        const bool diag = (r / S.T) == (c / S.T);
        if (c > r && !diag) continue;
        S.tile(r, c) = P(3 + (r > c ? r : c), 3 + (r > c ? c : r));
    }
    for (int k = 0; k < S.N; ++k) { S.diag[0][3 * k] = P(3 + 2 * k, 3 + 2 * k); S.diag[0][3 * k + 1] = P(4 + 2 * k, 3 + 2 * k); S.diag[0][3 * k + 2] = P(4 + 2 * k, 4 + 2 * k); S.s[k] = k + 1; }
}
static ConstrainArgs args(const Store &S, int keep, int drop, int npend, const double R[4]) {
    ConstrainArgs a; a.d0 = a.d1 = 0; a.R00 = R[0]; a.R01 = R[1]; a.R10 = R[2]; a.R11 = R[3]; a.ai = 2 * keep; a.aj = 2 * drop; a.n_mm = 2 * S.N;
    a.cur = S.cur; a.npend = npend; a.pstart = 0; return a;
}
static void compact(Store &S, const std::vector<int32_t> &src_of, int npairs, bool fused) {
    const int nt = (int)ekf_tiles_for(2 * S.N, S.T);
    std::vector<int2> work;
    for (int I = 0; I < nt; ++I) for (int J = 0; J <= I; ++J) work.push_back({I, J});
    const int items = (S.T * S.T / 2 + kBlock * kCompactRows - 1) / (kBlock * kCompactRows);
    S.sync();
    double *src = S.tiles[S.base].data(), *dst = S.tiles[S.base ^ 1].data();
    for (unsigned b = 0; b < work.size() * items; ++b)
        for (unsigned t = 0; t < kBlock; ++t) {
            blockIdx.x = b; threadIdx.x = t;
            if (fused) k_merge_pass<double>(src, dst, work.data(), items, src_of.data(), S.st.Kp, S.st.Gp, S.st.pair_stride, npairs, S.tm);
            else k_compact_tiles<double>(src, dst, work.data(), items, src_of.data(), S.tm);
        }
    S.base ^= 1; S.sync();
    std::vector<double> s_tmp(S.N);
    for (int b = 0; b < (S.N + kBlock - 1) / kBlock; ++b) for (int t = 0; t < kBlock; ++t) { blockIdx.x = b; threadIdx.x = t; k_compact_state(S.st, S.cur, src_of.data(), S.N, s_tmp.data()); }
    for (int k = 0; k < S.N; ++k) S.s[k] = s_tmp[k];
    S.cur ^= 1; S.dcur ^= 1; S.sync();
}
int main() {
    const double RP[4] = { 0.02, 0.005, 0.005, 0.03 }, R0[4] = { 0, 0, 0, 0 };
    int total_bad = 0;
    for (int T : { 16, 64 }) for (int rcase = 0; rcase < 2; ++rcase) {
        const double *R = rcase ? RP : R0;
        const int N = 90, cap = 96;
        std::vector<std::pair<int, int>> pairs = { { 3, 40 }, { 50, 7 }, { 3, 88 }, { 31, 32 }, { 89, 0 }, { 10, 60 }, { 61, 12 } };
        if (T == 16) pairs.push_back({ 8, 9 });          // adjacent
        const int m = (int)pairs.size();
        Store A(T, N, cap), B(T, N, cap);
        fill(A); fill(B);
        std::vector<int32_t> src_of(A.ldm / 2, -1);
        { int k = 0; for (int l = 0; l < N; ++l) { bool d = false; for (auto &p : pairs) d |= p.second == l; if (!d) src_of[k++] = l; } }
        const int grid = (int)(A.tm.padded(2 * N) / kBlock) + (A.tm.padded(2 * N) % kBlock ? 1 : 0);
        // A: the batch
        std::vector<double> rec(8 * m);
        for (int k = 0; k < m; ++k) {
            A.sync();
            ConstrainArgs a = args(A, pairs[k].first, pairs[k].second, k, R);
            DevState st = A.st;
            launch_wg(grid, [&] { k_gather_constrain<double>(st, a, rec.data() + 8 * k); });
            A.cur ^= 1; A.dcur ^= 1;
        }
        compact(A, src_of, m, true);
        // B: the sequence
        std::vector<double> d2(m);
        for (int k = 0; k < m; ++k) {
            B.sync();
            ConstrainArgs a = args(B, pairs[k].first, pairs[k].second, 0, R);
            DevState st = B.st;
            double sm[14];
            for (int e = 0; e < 14; ++e) sm[e] = constrain_small_entry<double>(st, B.cur, a.ai, a.aj, e);
            double Sm[4];
            ekfm::constrain_S(sm, sm + 3, sm + 6, R, Sm);
            if (!ekfm::constrain_d2(Sm, -(sm[10] - sm[12]), -(sm[11] - sm[13]), d2[k])) printf("irregular pair %d\n", k);
            launch_wg(grid, [&] { k_gather_constrain<double>(st, a, (double *)nullptr); });
            B.cur ^= 1; B.dcur ^= 1;
            // the one-pair pass, in place, over every stored entry (diagonal tiles whole)
            const double2 *G2 = (const double2 *)B.st.Gp, *K2 = (const double2 *)B.st.Kp;
            for (int r = 0; r < 2 * N; ++r) for (int c = 0; c < 2 * N; ++c) {
                if (c > r && (r / T) != (c / T)) continue;
                B.tile(r, c) = rank2_apply(B.tile(r, c), K2[r], G2[c]);
            }
        }
        compact(B, src_of, 0, false);
        int bad = 0;
        auto cmp = [&](const std::vector<double> &u, const std::vector<double> &v, const char *what) {
            int b = 0; for (size_t i = 0; i < u.size(); ++i) if (memcmp(&u[i], &v[i], 8)) ++b;
            if (b) printf("  %s: %d differ\n", what, b); bad += b; };
        cmp(A.x[A.cur], B.x[B.cur], "x"); cmp(A.strip[A.cur], B.strip[B.cur], "strip"); cmp(A.prr[A.cur], B.prr[B.cur], "prr");
        cmp(A.diag[A.dcur], B.diag[B.dcur], "diag"); cmp(A.s, B.s, "s");
        const int nt = (int)ekf_tiles_for(2 * N, T);
        int tb = 0;
        for (int r = 0; r < nt * T; ++r) for (int c = 0; c <= r; ++c) { double u = A.tile(r, c), v = B.tile(r, c); if (memcmp(&u, &v, 8)) ++tb; }
        if (tb) printf("  tiles (lower triangle): %d differ\n", tb);
        bad += tb;
        int db = 0;
        for (int k = 0; k < m; ++k) { if (memcmp(&rec[8 * k + 6], &d2[k], 8) || rec[8 * k + 7] != 1.0) ++db; }
        if (db) printf("  d2 records: %d differ\n", db);
        bad += db;
        uint64_t hs = 14695981039346656037ull;                  // route A: x, strip, prr, diag, s, lower-triangle tiles, records
        hs = fnv(hs, A.x[A.cur].data(), A.x[A.cur].size()); hs = fnv(hs, A.strip[A.cur].data(), A.strip[A.cur].size());
        hs = fnv(hs, A.prr[A.cur].data(), A.prr[A.cur].size()); hs = fnv(hs, A.diag[A.dcur].data(), A.diag[A.dcur].size());
        hs = fnv(hs, A.s.data(), A.s.size());
        for (int r = 0; r < nt * T; ++r) for (int c = 0; c <= r; ++c) { const double u = A.tile(r, c); hs = fnv(hs, &u, 1); }
        hs = fnv(hs, rec.data(), rec.size());
        printf("T=%d R%s m=%d: %d differences (d2[0]=%g d2[%d]=%g state %016llx)\n", T, rcase ? "pos" : "0", m, bad, rec[6], m - 1, rec[8 * (m - 1) + 6],
               (unsigned long long)hs);
        total_bad += bad;
    }
    return total_bad != 0;
}
