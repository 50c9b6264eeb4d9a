// Host emulation of the one-pair pass kernels with a live-row bound (PassJob::live_rows): the kernel SOURCE of ekf_slam_amd/csrc/downdate.h
// compiled with g++ behind tests/support/kernel_host_shim.h, every workgroup's lanes one after another.
//
// The scene: a store of 3 x 3 tile rows of edge 64 (the lower block triangle: 6 tiles, 192 rows), 138 rows of which hold state.  Rows
// 138 .. 191 of every tile of the last tile row hold a SENTINEL pattern.  K is zero on rows 138 .. up to the end of the slab that straddles
// the bound (as the gather leaves it) and POISON beyond, G is zero from column 138 on.  For every kernel instance, both walking directions
// and a grid smaller than the item count:
// (k_downdate_w on the one list runs over the two-range item space launch_downdate gives it under a bound: the tiles of the last tile row
// only up to the slab that holds the bound, rounded up to a power of two; the unbounded twin over every tile whole)
//   * the bounded run leaves every sentinel as it was, bit for bit -- a work item of padding rows that was loaded and stored would have
//     taken the poisoned K along;
//   * the rows that hold state equal, bit for bit, those of the unbounded run over the same store with K zero from row 138 on.
// Prints one line per case and "ok" at the end; the exit status counts the failures.
#include <climits>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include "kernel_host_shim.h"
#include "tile_access.h"

static Idx gridDim;
static inline int2 make_int2(int a, int b) { return {a, b}; }
#define __builtin_amdgcn_readfirstlane(v) (v)
#if !defined(__clang__)
#define __builtin_assume(c) ((void)0)
#endif
struct NextRow { int64_t j; double *send; };
// (downdate.h brings its own Lane16 and lane16_pack, which the shim also has for the kernels that take them from pair_column.h)
#define Lane16 PassLane16
#define lane16_pack pass_lane16_pack
#define lane16_unpack pass_lane16_unpack
#define lane16_get pass_lane16_get
#include "downdate.h"

constexpr int T = 64, NT = 3, ROWS = NT * T, LIVE = 138;
static const TileMap tm0 = ekf_make_tilemap(T, 1, 0);

struct Scene {
    std::vector<double> tiles, K, G;
    std::vector<int2> work, xcd; int64_t nwork = 0, xcd_len = 0;
    Scene(int first_dead) {
        srand(17);
        auto rnd = [] { return (rand() % 20001 - 10000) / 10000.0; };
        tiles.assign((size_t)tm0.row_base(NT) * T * T, 0.0);
        for (int I = 0; I < NT; ++I) for (int J = 0; J <= I; ++J) {
            work.push_back(make_int2(I, J));
            double *t = tiles.data() + tm0.tile_offset(I, J);
            for (int r = 0; r < T; ++r) for (int c = 0; c < T; ++c)
                t[r * T + c] = I * T + r < LIVE ? rnd() : -(1e6 * (I * T + r) + J * T + c + 0.5);        // the sentinels
        }
        nwork = (int64_t)work.size();
        // 8 streams, the tiles dealt out in order, padded with (-1, -1) -- as refresh_work lays them out
        xcd_len = 1;
        xcd.assign(8 * xcd_len, make_int2(-1, -1));
        for (size_t i = 0; i < work.size(); ++i) xcd[i * xcd_len] = work[i];
        K.assign(2 * ROWS, 0.0); G.assign(2 * ROWS, 0.0);
        for (int r = 0; r < ROWS; ++r)
            for (int a = 0; a < 2; ++a) {
                K[2 * r + a] = r < LIVE ? rnd() : r < first_dead ? 0.0 : 1e30;       // poison where a bounded pass must not come
                G[2 * r + a] = r < LIVE ? rnd() : 0.0;
            }
    }
};

// the item space of the one list as launch_downdate cuts it (k_downdate_w: head, tail_shift); two_ranges = false: every tile whole
struct Items { int live, head, tail_shift; int64_t n; };
static Items items_for(const Scene &s, int slab, bool xcd, int live, bool two_ranges) {
    const int slabs_per_tile = T / slab;
    Items it = { live, (int)s.nwork * slabs_per_tile, 0, (xcd ? 8 * s.xcd_len : s.nwork) * slabs_per_tile };
    if (!two_ranges || live == INT_MAX) return it;
    const int64_t nwork_head = tm0.row_base(NT - 1);                       // the tiles in front of the last tile row's
    const int in_last = live - (live - 1) / T * T, slabs = (in_last + slab - 1) / slab;
    while ((1 << it.tail_shift) < slabs) ++it.tail_shift;
    it.head = (int)nwork_head * slabs_per_tile;
    it.n = it.head + ((s.nwork - nwork_head) << it.tail_shift);
    return it;
}

template <typename Launch> static int run_case(const char *name, int slab, bool xcd, bool two_ranges, Launch launch) {
    const int first_dead = (LIVE + slab - 1) / slab * slab;
    int bad = 0;
    for (int reverse = 0; reverse < 2; ++reverse)
        for (int pass = 0; pass < 2; ++pass) {
            Scene bounded(first_dead), plain(first_dead);
            for (int r = LIVE; r < ROWS; ++r) plain.K[2 * r] = plain.K[2 * r + 1] = 0.0;     // the unbounded twin: identity beyond the map
            const std::vector<double> before = bounded.tiles;
            TileMap tm = tm0; tm.reverse = reverse;
            const Items ib = items_for(bounded, slab, xcd, LIVE, two_ranges), ip = items_for(plain, slab, xcd, INT_MAX, false);
            const int grid = pass == 0 ? (int)ib.n : 5;                                      // one item per workgroup; a grid-stride walk
            launch(bounded, tm, grid, ib);
            launch(plain, tm, pass == 0 ? (int)ip.n : 5, ip);
            int sentinels = 0, moved = 0, differ = 0, untouched = 0;
            for (int I = 0; I < NT; ++I) for (int J = 0; J <= I; ++J)
                for (int r = 0; r < T; ++r) for (int c = 0; c < T; ++c) {
                    const size_t o = (size_t)tm0.tile_offset(I, J) + r * T + c;
                    if (I * T + r >= LIVE) { ++sentinels; moved += memcmp(&bounded.tiles[o], &before[o], 8) != 0; }
                    else {
                        differ += memcmp(&bounded.tiles[o], &plain.tiles[o], 8) != 0;
                        untouched += J * T + c < LIVE && memcmp(&bounded.tiles[o], &before[o], 8) == 0;
                    }
                }
            // (a live entry keeps its bits only where K G rounds away: with these operands never)
            const bool ok = moved == 0 && differ == 0 && untouched == 0 && sentinels == (ROWS - LIVE) * T * NT;
            printf("%s reverse %d grid %d: sentinels %d moved %d, live entries differing from the unbounded run %d, left alone %d: %s\n", name,
                   reverse, grid, sentinels, moved, differ, untouched, ok ? "pass" : "FAIL");
            bad += !ok;
        }
    return bad;
}

template <typename Kernel> static void wg(int grid, Kernel k) {
    gridDim.x = (unsigned)grid;
    for (int b = 0; b < grid; ++b) for (int t = 0; t < kBlock; ++t) { blockIdx.x = (unsigned)b; threadIdx.x = (unsigned)t; k(); }
}

template <int kSlab, bool kXcd> static int case_w(const char *name) {
    return run_case(name, kSlab, kXcd, !kXcd, [](Scene &s, TileMap tm, int grid, Items it) {
        wg(grid, [&] {
            k_downdate_w<double, T, kSlab, kXcd>(s.tiles.data(), s.tiles.data(), kXcd ? s.xcd.data() : s.work.data(), kXcd ? s.xcd_len : s.nwork,
                                                 s.K.data(), s.G.data(), 2 * ROWS, 0, 1, 1, tm, NoNextRow{}, it.live, it.head, it.tail_shift);
        });
    });
}

int main() {
    int bad = 0;
    bad += case_w<8, false>("k_downdate_w<double,64,8,false>");
    bad += case_w<16, false>("k_downdate_w<double,64,16,false>");
    bad += case_w<64, false>("k_downdate_w<double,64,64,false>");        // a slab is a whole tile: nothing is ever left out
    bad += case_w<8, true>("k_downdate_w<double,64,8,true>");
    bad += case_w<32, true>("k_downdate_w<double,64,32,true>");
    bad += run_case("k_downdate_w<double,64,8,false,+rowpanel>", 8, false, true, [](Scene &s, TileMap tm, int grid, Items it) {
        std::vector<double> send(2 * ROWS + 2, 0.0);
        const NextRow nx = { 70, send.data() };                            // the row-panel of landmark-block rows 70, 71 rides along
        wg(grid, [&] {
            k_downdate_w<double, T, 8, false, true>(s.tiles.data(), s.tiles.data(), s.work.data(), s.nwork, s.K.data(), s.G.data(), 2 * ROWS, 0, 1, 1,
                                                    tm, nx, it.live, it.head, it.tail_shift);
        });
    });
    bad += run_case("k_downdate<double,64,16>", 16, false, false, [](Scene &s, TileMap tm, int grid, Items it) {
        wg(grid, [&] {
            k_downdate<double, T, 16>(s.tiles.data(), s.tiles.data(), s.work.data(), s.nwork, s.K.data(), s.G.data(), 2 * ROWS, 0, 1, 1, tm, it.live);
        });
    });
    bad += run_case("k_downdate<double,64,8>", 8, false, false, [](Scene &s, TileMap tm, int grid, Items it) {
        wg(grid, [&] {
            k_downdate<double, T, 8>(s.tiles.data(), s.tiles.data(), s.work.data(), s.nwork, s.K.data(), s.G.data(), 2 * ROWS, 0, 1, 1, tm, it.live);
        });
    });
    puts(bad ? "FAILED" : "ok");
    return bad;
}
