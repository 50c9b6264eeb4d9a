// Host emulation of the kernels of ekf_factor_map (tests/test_factor_map_cpu.py compiles and runs it; no GPU, no HIP runtime).  The kernel
// SOURCE ekf_slam_amd/csrc/factor_map.h is compiled for the host behind map_algebra_rig.h: the kernels with barriers (a diagonal tile is
// factored in LDS, two barriers a column) run their lanes as threads, the kernels without one (k_factor_load, k_factor_rhs,
// k_factor_trail) one after another, k_factor_trail's matrix-core loop as its plain-FMA twin in the same k order.  Factor tile edges 16
// and 32; the source store is F64 or float with its own tile edge.
// The cases -- one line "name TF Tsrc float N nref" each -- are read from argv[1]/cases.txt; case `name` reads argv[1]/name.in (x, the
// dense P column by column as the test wants the handle to hold it, nref reference states) and writes argv[1]/name.out: the result
// block, then the pivots.  Each case checks here that the launches left the state (x, Prr, the strip, the tiles, the diagonal copies, s,
// the pair ring) bit for bit as it was.
#include "map_algebra_rig.h"

struct Case { std::string name; int TF, Tsrc, isfloat, N, nref; };

template <typename TS, int TF> static int run_case(const Case &c, const std::string &dir) {
    FactoredCase<TS, TF> fc(dir, c.name, c.Tsrc, c.N, (size_t)c.nref * (3 + 2 * c.N), c.nref, false);
    if (!fc.ok) return 1000;
    fc.run();
    const int bad = fc.unloaded + fc.untouched();
    FILE *f = fopen((dir + "/" + c.name + ".out").c_str(), "wb");
    if (!f) return 1000;
    put(f, fc.res.data(), fc.res.size());
    fclose(f);
    printf("%s: %d differences\n", c.name.c_str(), bad);
    return bad;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    FILE *f = fopen((dir + "/cases.txt").c_str(), "r");
    if (!f) return 3;
    int bad = 0, n = 0;
    char name[128];
    Case c;
    while (fscanf(f, "%127s %d %d %d %d %d", name, &c.TF, &c.Tsrc, &c.isfloat, &c.N, &c.nref) == 6) {
        if ((c.TF != 16 && c.TF != 32) || (c.Tsrc != 16 && c.Tsrc != 32) || c.N < 0 || c.N > 64 || c.nref < 0 || c.nref > kFactorRefMax) { fclose(f); return 4; }
        c.name = name;
        if (c.TF == 16) bad += c.isfloat ? run_case<float, 16>(c, dir) : run_case<double, 16>(c, dir);
        else bad += c.isfloat ? run_case<float, 32>(c, dir) : run_case<double, 32>(c, dir);
        ++n;
    }
    fclose(f);
    if (n == 0) return 5;
    return bad != 0;
}
