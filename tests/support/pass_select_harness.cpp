// Prints what ekf_slam_amd/csrc/launch/pass_select.h selects for every combination tests/test_pass_select_cpu.py asks about, one line each:
//   elt T npairs arith xcd strip next | family slab chunk cols early xcd rowpanel name          (argv[1]: the slab override, default 0)
#include <stdlib.h>

#include <initializer_list>

#include "launch/pass_select.h"

int main(int argc, char **argv) {
    const int slab_override = argc > 1 ? atoi(argv[1]) : 0;
    for (int elt : { 8, 4 })
        for (int T : { 16, 32, 64, 128, 256 })
            for (int np = 1; np <= 64; ++np)
                for (int arith = 0; arith <= (elt == 4 && T == 256 ? 2 : 0); ++arith)
                    for (int flags = 0; flags < 8 && !(elt == 8 && T == 256); ++flags) {
                        const bool xcd = flags & 1, strip = flags & 2, next = flags & 4;
                        const ekf_pass::PassInstance p = ekf_pass::select_pass({ elt, T, np, arith, xcd, strip, /*planes*/ strip, next, slab_override });
                        printf("%d %d %d %d %d %d %d | %d %d %d %d %d %d %d %s\n", elt, T, np, arith, xcd, strip, next, (int)p.family, p.slab, p.chunk,
                               p.cols, p.early, p.xcd, p.rowpanel, p.name);
                    }
    return 0;
}
