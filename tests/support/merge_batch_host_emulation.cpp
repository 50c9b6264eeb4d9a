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
#include "emulated_state.h"
#include "compact.h"
#include "merge_pass.h"

// FNV-1a over the bytes of a route's final state: printed in each line's parentheses, so that two builds of this file can be compared
static uint64_t fnv(uint64_t h, const double *p, size_t n) {
    const unsigned char *b = (const unsigned char *)p;
    for (size_t i = 0; i < 8 * n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}
static ConstrainArgs args(const Store<> &S, int keep, int drop, int npend, const double R[4]) {
    ConstrainArgs a; a.d0 = a.d1 = 0; a.R00 = R[0]; a.R01 = R[1]; a.R10 = R[2]; a.R11 = R[3]; a.ai = 2 * keep; a.aj = 2 * drop; a.n_mm = 2 * S.N;
    a.cur = S.cur; a.npend = npend; a.pstart = 0; return a;
}
static void compact(Store<> &S, const std::vector<int32_t> &src_of, int npairs, bool fused) {
    const int nt = (int)ekf_tiles_for(2 * S.N, S.T);
    std::vector<int2> work;
    for (int I = 0; I < nt; ++I) for (int J = 0; J <= I; ++J) work.push_back({I, J});
    const int items = (S.T * S.T / 2 + kBlock * kCompactRows - 1) / (kBlock * kCompactRows);
    S.sync();
    std::vector<double> other(S.tiles.size(), 0);          // the second tile store: the pass writes it, then it is the live one
    double *src = S.tiles.data(), *dst = other.data();
    for (unsigned b = 0; b < work.size() * items; ++b)
        for (unsigned t = 0; t < kBlock; ++t) {
            blockIdx.x = b; threadIdx.x = t;
            if (fused) k_merge_pass<double>(src, dst, work.data(), items, src_of.data(), S.st.Kp, S.st.Gp, S.st.pair_stride, npairs, S.tm);
            else k_compact_tiles<double>(src, dst, work.data(), items, src_of.data(), S.tm);
        }
    S.tiles.swap(other); S.sync();
    std::vector<double> s_tmp(S.N);
    for (int b = 0; b < (S.N + kBlock - 1) / kBlock; ++b) for (int t = 0; t < kBlock; ++t) { blockIdx.x = b; threadIdx.x = t; k_compact_state(S.st, S.cur, src_of.data(), S.N, s_tmp.data()); }
    for (int k = 0; k < S.N; ++k) S.s[k] = s_tmp[k];
    S.flip();
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
        Store<> A(T, N, cap, 32), B(T, N, cap, 32);
        fill(A, 11, false); fill(B, 11, false);
        std::vector<int32_t> src_of(A.ldm / 2, -1);
        { int k = 0; for (int l = 0; l < N; ++l) { bool d = false; for (auto &p : pairs) d |= p.second == l; if (!d) src_of[k++] = l; } }
        // A: the batch.  k_gather_constrain: every workgroup twice -- lane 0 fills the shared solve first of all, so the recording pass already
        // computes with it, and the second pass, the launch, takes the partners from what the first one recorded
        std::vector<double> rec(8 * m);
        for (int k = 0; k < m; ++k) {
            ConstrainArgs a = args(A, pairs[k].first, pairs[k].second, k, R);
            DevState st = A.st;
            launch_wg(A.grid(), { 2, 1 }, [&] { k_gather_constrain<double>(st, a, rec.data() + 8 * k); });
            A.flip();
        }
        compact(A, src_of, m, true);
        // B: the sequence
        std::vector<double> d2(m);
        for (int k = 0; k < m; ++k) {
            ConstrainArgs a = args(B, pairs[k].first, pairs[k].second, 0, R);
            DevState st = B.st;
            double sm[14];
            for (int e = 0; e < 14; ++e) sm[e] = constrain_small_entry<double>(st, B.cur, a.ai, a.aj, e);
            double Sm[4];
            ekfm::constrain_S(sm, sm + 3, sm + 6, R, Sm);
            if (!ekfm::constrain_d2(Sm, -(sm[10] - sm[12]), -(sm[11] - sm[13]), d2[k])) printf("irregular pair %d\n", k);
            launch_wg(B.grid(), { 2, 1 }, [&] { k_gather_constrain<double>(st, a, (double *)nullptr); });
            B.flip();
            // the one-pair pass, in place, over every stored entry (diagonal tiles whole)
            const double2 *G2 = (const double2 *)B.st.Gp, *K2 = (const double2 *)B.st.Kp;
            for (int r = 0; r < 2 * N; ++r) for (int c = 0; c < 2 * N; ++c) {
                if (c > r && (r / T) != (c / T)) continue;
                B.tile(r, c) = rank2_apply(B.tile(r, c), K2[r], G2[c]);
            }
        }
        compact(B, src_of, 0, false);
        int bad = differ(A.x[A.cur], B.x[B.cur], "x") + differ(A.strip[A.cur], B.strip[B.cur], "strip") + differ(A.prr[A.cur], B.prr[B.cur], "prr") +
                  differ(A.diag[A.dcur], B.diag[B.dcur], "diag") + differ(A.s, B.s, "s");
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
