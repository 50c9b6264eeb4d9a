// The sizing arithmetic of the calls that treat P as a matrix (launch/map_algebra.h launches what it sizes; kernels.h declares it for
// the host layer): the factor store's tile edge, the tiles per segment, and how many doubles the partial blocks, the inverse tiles and
// the dense observation's partial sums take.  Host code, nothing from HIP: it needs layout.h and kernel_args.h alone, so the emulations
// of tests/support compile it with g++ and size their scratch by it.
#pragma once
#include <stdint.h>

#include "../kernel_args.h"
#include "../layout.h"

// ---- the factorisation of P (factor_map.h) ----
// The factor store's tile edge.  64: a diagonal tile and the right-hand sides take 40 KiB of LDS, a lane of k_factor_panel holds a whole
// row in registers, a workgroup of k_factor_trail is four wavefronts with no LDS at all.  Edge 128 (a 128 KiB diagonal tile) is not built.
constexpr int kFactorTile = 64;
int factor_tile_edge() { return kFactorTile; }

// ---- the draws behind it (sample_map.h: k_factor_apply, k_factor_sample) ----
// Tiles per segment of a tile row.  16: a workgroup streams 512 KiB of the factor for one 8 KiB partial block (3 % of the store's bytes
// written and read again), and 10 000 landmarks (313 tile rows) still make 3 220 workgroups, all of the same length but the last of each tile row.
constexpr int kFactorSegment = 16;
int factor_chunk() { return kFactorChunk; }
// one partial block per segment, then per tile row its 3 x kFactorChunk part of W' Xi
int64_t factor_partial_doubles(int64_t rows) {
    const int64_t nF = rows / kFactorTile;
    return factor_segment_base(nF, kFactorSegment) * (int64_t)(kFactorTile * kFactorChunk) + nF * (3 * kFactorChunk);
}

// ---- the solves behind it (solve_map.h): one inverse tile per tile row ----
int64_t solve_inverse_doubles(int64_t rows) { return rows * (int64_t)kFactorTile; }

// ---- the plain product P B on the handle's own store (multiply_map.h) ----
// Tiles per segment of a tile row: 256 columns' worth.  A workgroup then streams 2 tiles at the F64 production edge 128 and one at 256
// for one direct partial block, and a map of 140 landmarks at edge 16 still has tile rows of two segments.
int multiply_segment(int T) { return T >= 256 ? 1 : 256 / T; }
void multiply_partial_offsets(const TileMap &tm, int64_t rows, int64_t *tpart, int64_t *wpart) {
    const int64_t nT = rows / tm.T, blk = (int64_t)tm.T * kFactorChunk;
    *tpart = factor_segment_base(nT, multiply_segment(tm.T)) * blk;
    *wpart = *tpart + tm.row_base(nT) * blk;
}
int64_t multiply_partial_doubles(const TileMap &tm, int64_t rows) {
    int64_t t, w;
    multiply_partial_offsets(tm, rows, &t, &w);
    return w + (rows / tm.T) * (3 * kFactorChunk);
}

// ---- a linear observation with a dense H (dense_obs.h): one block of sums per segment of landmark rows ----
int64_t dense_partial_doubles(int64_t n_mm) { return (n_mm + kDenseSegment - 1) / kDenseSegment * kDensePartial; }
