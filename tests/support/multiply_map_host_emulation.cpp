// Host emulation of the kernels of ekf_multiply_map (tests/test_multiply_map_cpu.py compiles and runs it; no GPU, no HIP runtime): the
// kernel SOURCE ekf_slam_amd/csrc/multiply_map.h (with factor_map.h, whose factor_source it reads P through) behind map_algebra_rig.h,
// a workgroup with barriers as threads, the matrix-core loops as their plain-FMA twins in the same k order (EKF_FACTOR_FMA_TWIN) -- per
// chunk of kFactorChunk vectors k_multiply_tiles and k_multiply_sum, launch after launch as host/multiply_map.h queues them, on the
// store's own tile map: tile edges 16 .. 256, F64 or float tiles.
// The cases -- one line "name T float N k" each -- are read from argv[1]/cases.txt (or argv[1]/argv[2]); case `name` reads
// argv[1]/name.in (the dense P column by column as the test wants the handle to hold it, k vectors of 3 + 2 N entries in x's order) and
// writes argv[1]/name.out: the k products in x's order.
// WHAT THE STORE HOLDS BESIDE P, so that only the stated read gives the right answer: every tile entry in a row or column at or beyond
// 2 N is NaN, the strip's columns from 2 N on are NaN, the tile entries of every landmark's own 2 x 2 block hold a wrong value (the
// diag copies hold the right one), the upper triangle of every diagonal tile holds garbage, the other buffer of Prr / strip / diag is
// NaN.  The chunks are packed and unpacked as host/multiply_map.h does it, the result chunk and the partial blocks poisoned first, so
// that an entry no launch wrote (or one written that must not be) shows.  Each case checks here that the launches left the state bit
// for bit as it was.
#include "map_algebra_rig.h"
#include "multiply_map.h"
#include "launch/map_sizes.h"      // multiply_segment, multiply_partial_offsets, multiply_partial_doubles: the launchers' own arithmetic

struct Case { std::string name; int T, isfloat, N, k; };

template <typename TS, int TMAX> static int run_case(const Case &c, const std::string &dir) {
    const int N = c.N, n = 3 + 2 * N, k = c.k, T = c.T;
    std::vector<double> in((size_t)n * n + (size_t)k * n);
    FILE *f = fopen((dir + "/" + c.name + ".in").c_str(), "rb");
    if (!f || fread(in.data(), 8, in.size(), f) != in.size()) return 1000;
    fclose(f);
    const double *P = in.data(), *B = P + (size_t)n * n;
    Store<TS> S(T, N, N + 3);
    // everything NaN first, then P where the kernels may read it
    for (auto &v : S.tiles) v = (TS)NAN;
    for (int b = 0; b < 2; ++b) { S.strip[b].assign(S.strip[b].size(), NAN); S.prr[b].assign(S.prr[b].size(), NAN); S.diag[b].assign(S.diag[b].size(), NAN); S.x[b].assign(S.x[b].size(), NAN); }
    scatter(S, [&](int r, int col) { return P[(size_t)col * n + r]; });
    for (int r = 0; r < 2 * N; ++r)
        for (int col = 0; col < 2 * N; ++col) {
            if (r / T != col / T) continue;
            if (r / 2 == col / 2) S.tile(r, col) = (TS)(1000.0 + r);          // the own blocks' tile entries: wrong
            else if (col > r) S.tile(r, col) = (TS)(-500.0 - col);            // above the diagonal of a diagonal tile: garbage
        }
    for (auto &v : S.ring) v = 0.25;
    const Store<TS> S0(S);
    const DevState st = S.st;
    const int64_t rows = S.tm.padded(2 * N), nT = rows / T, ld = rows + 4, blk = (int64_t)T * kFactorChunk;
    const int Sg = multiply_segment(T);
    const int64_t segments = factor_segment_base(nT, Sg);
    int64_t toff, woff;
    multiply_partial_offsets(S.tm, rows, &toff, &woff);
    const size_t chunk = (size_t)ld * kFactorChunk;
    std::vector<double> cb(chunk + 1), cy(chunk + 1), part((size_t)multiply_partial_doubles(S.tm, rows) + 1), out((size_t)k * n, kPoison);
    MultiplyMapArgs a = {};
    a.b = cb.data(); a.y = cy.data(); a.dpart = part.data(); a.tpart = part.data() + toff; a.wpart = part.data() + woff;
    a.ld = ld; a.N = N; a.rows = rows; a.S = Sg; a.cur = S.cur;
    int bad = 0;
    for (int64_t j = 0; j * kFactorChunk < k; ++j) {
        cb.assign(cb.size(), 0.0);
        cy.assign(cy.size(), kPoison);
        part.assign(part.size(), kPoison);
        cb.back() = kPoison;
        pack_chunk(cb.data(), B, j, k, N, rows, ld);
        if (N > 0) launch_threads(0, (int)segments, kMultiplyBlock, [&] { k_multiply_tiles<TS, TMAX>(st, a); });
        const int sum_grid = (int)(nT * ((blk + kFactorBlock - 1) / kFactorBlock));
        launch_lanes(0, sum_grid, kFactorBlock, [&] { k_multiply_sum(st, a); });
        launch_threads(0, 1, kFactorBlock, [&] { k_multiply_robot(st, a); });
        for (int64_t q = 0; q < kFactorChunk; ++q)
            for (int64_t i = 0; i < rows + 4; ++i) {
                const bool written = i < 2 * N || (i >= rows && i < rows + 3);
                if ((cy[q * ld + i] == kPoison) == written) ++bad;              // every live entry written, nothing else
            }
        if (cy.back() != kPoison || cb.back() != kPoison || part.back() != kPoison) ++bad;
        unpack_chunk(out.data(), cy.data(), j, k, N, rows, ld);
    }
    // nothing of the state was written
    bad += state_differs(S, S0);
    f = fopen((dir + "/" + c.name + ".out").c_str(), "wb");
    if (!f) return 1000;
    put(f, out.data(), out.size());
    fclose(f);
    printf("%s: %d differences\n", c.name.c_str(), bad);
    return bad;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    FILE *f = fopen((dir + "/" + (argc > 2 ? argv[2] : "cases.txt")).c_str(), "r");
    if (!f) return 3;
    int bad = 0, n = 0;
    char name[128];
    Case c;
    while (fscanf(f, "%127s %d %d %d %d", name, &c.T, &c.isfloat, &c.N, &c.k) == 5) {
        if ((c.T != 16 && c.T != 32 && c.T != 64 && c.T != 128 && c.T != 256) || c.N < 0 || c.N > 400 || c.k < 1 || c.k > 1024) { fclose(f); return 4; }
        c.name = name;
        if (c.T <= 128) bad += c.isfloat ? run_case<float, 128>(c, dir) : run_case<double, 128>(c, dir);
        else bad += c.isfloat ? run_case<float, 256>(c, dir) : run_case<double, 256>(c, dir);
        ++n;
    }
    fclose(f);
    if (n == 0) return 5;
    return bad != 0;
}
