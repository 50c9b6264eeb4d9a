// segment_of of ekf_slam_amd/csrc/map_blocks.h, the decode of a grid index into (tile row, segment, first tile, one past the last tile)
// that k_factor_apply and k_multiply_tiles share, compiled for the host behind map_algebra_rig.h (tests/test_sample_map_cpu.py runs it).
// argv: the largest tile-row count, then the segment lengths S.  For every S and every nF = 1 .. that count, one line "S nF I seg J0 J1"
// per grid index w = 0 .. factor_segment_base(nF, S) - 1, in w's order.
#include <cstdlib>
#include "map_algebra_rig.h"

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const int most = atoi(argv[1]);
    for (int i = 2; i < argc; ++i) {
        const int S = atoi(argv[i]);
        if (S < 1) return 3;
        for (int nF = 1; nF <= most; ++nF)
            for (int64_t w = 0; w < factor_segment_base(nF, S); ++w) {
                int I, seg, J0, J1;
                segment_of(w, S, I, seg, J0, J1);
                printf("%d %d %d %d %d %d\n", S, nF, I, seg, J0, J1);
            }
    }
    return 0;
}
