// Host emulation of the kernels of ekf_solve_map (tests/test_solve_map_cpu.py compiles and runs it; no GPU, no HIP runtime): the
// factorisation exactly as sample_map_host_emulation.cpp runs it (FactoredCase of map_algebra_rig.h), then from the kernel SOURCE
// ekf_slam_amd/csrc/solve_map.h k_solve_invert once and per chunk of kFactorChunk right-hand sides the forward sweep, the robot
// tail and, for form 0, the backward sweep, launch after launch in the order host/factor_map.h queues them.  Factor tile edges 16 and
// 32; the source store is F64 or float with its own tile edge.
// The cases -- one line "name TF Tsrc float N k form" each -- are read from argv[1]/cases.txt (or argv[1]/argv[2], so that several
// processes can share one directory); case `name` reads argv[1]/name.in (x, the
// dense P column by column as the test wants the handle to hold it, k right-hand sides of 3 + 2 N entries in x's order) and writes
// argv[1]/name.out: the result block, the pivots, the k results in x's order (NaN where a pivot failed, as the host layer fills them),
// then the factor C in elimination order as the factorisation left it in the store.  The chunks are packed and unpacked as
// host/factor_map.h does it, the result chunk and the inverse tiles poisoned first, so that an entry no launch wrote shows.  Each case
// checks here that the launches left the state bit for bit as it was.
#include "map_algebra_rig.h"
#include "sample_map.h"
#include "solve_map.h"

struct Case { std::string name; int TF, Tsrc, isfloat, N, k, form; };

template <typename TS, int TF> static int run_case(const Case &c, const std::string &dir) {
    const int N = c.N, n = 3 + 2 * N, k = c.k;
    FactoredCase<TS, TF> fc(dir, c.name, c.Tsrc, N, (size_t)k * n, 0, true);
    if (!fc.ok) return 1000;
    fc.run();
    const FactorMapArgs &a = fc.a;
    const std::vector<double> &res = fc.res;
    const int nF = fc.nF;
    // the right-hand sides, a chunk at a time
    const int64_t ld = a.rows + 4;
    const size_t chunk = (size_t)ld * kFactorChunk;
    std::vector<double> cb(chunk + 1), cy(chunk + 1), inv((size_t)a.rows * TF + 1, kPoison), out((size_t)k * n, kPoison);
    FactorSolveArgs sv = {};
    sv.b = cb.data(); sv.y = cy.data(); sv.inv = inv.data(); sv.ld = ld; sv.form = c.form;
    int bad = 0;
    launch_threads(0, nF, 64, [&] { k_solve_invert<TF>(a, sv); });
    if (res[0] == 0.0)
        for (size_t i = 0; i + 1 < inv.size(); ++i) if (inv[i] == kPoison) ++bad;                 // every inverse written whole
    for (int64_t j = 0; j * kFactorChunk < k; ++j) {
        cb.assign(cb.size(), 0.0);
        cy.assign(cy.size(), kPoison);
        cb.back() = kPoison;
        pack_chunk(cb.data(), fc.extra, j, k, N, a.rows, ld);
        for (int col = 0; col < nF; ++col) launch_threads(0, nF - col, 4 * TF, [&] { k_solve_forward<TF>(a, sv, col); });
        launch_threads(0, 1, kFactorBlock, [&] { k_solve_tail(a, sv); });
        if (c.form == 0)
            for (int col = nF - 1; col >= 0; --col) launch_threads(0, col + 1, 4 * TF, [&] { k_solve_backward<TF>(a, sv, col); });
        const std::vector<double> &cr = c.form == 0 ? cb : cy;
        if (res[0] == 0.0)
            for (int64_t q = 0; q < kFactorChunk; ++q)
                for (int64_t i = 0; i < a.rows + 3; ++i) if (cr[q * ld + i] == kPoison) ++bad;     // every entry of the result written
        if (cy.back() != kPoison || cb.back() != kPoison || inv.back() != kPoison) ++bad;
        unpack_chunk(out.data(), cr.data(), j, k, N, a.rows, ld);
    }
    if (res[0] != 0.0) out.assign(out.size(), NAN);
    bad += fc.untouched();
    FILE *f = fopen((dir + "/" + c.name + ".out").c_str(), "wb");
    if (!f) return 1000;
    put(f, res.data(), res.size());
    put(f, out.data(), out.size());
    fc.put_factor(f);
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
    while (fscanf(f, "%127s %d %d %d %d %d %d", name, &c.TF, &c.Tsrc, &c.isfloat, &c.N, &c.k, &c.form) == 7) {
        if ((c.form != 0 && c.form != 1) || (c.TF != 16 && c.TF != 32) || (c.Tsrc != 16 && c.Tsrc != 32) || c.N < 0 || c.N > 64 || c.k < 1 || c.k > 1024) { fclose(f); return 4; }
        c.name = name;
        if (c.TF == 16) bad += c.isfloat ? run_case<float, 16>(c, dir) : run_case<double, 16>(c, dir);
        else bad += c.isfloat ? run_case<float, 32>(c, dir) : run_case<double, 32>(c, dir);
        ++n;
    }
    fclose(f);
    if (n == 0) return 5;
    return bad != 0;
}
