// Fragment of kernels.hip (included there, inside its anonymous namespace, after downdate.h / constrain.h): the candidate search in
// front of a merge (ekf_nearest_landmarks): k_nearest.
#pragma once

// ---------------------------------------------------------------------------------------------------
// For every landmark i: the j < i that minimises d2(i, j) = nu' S^-1 nu of "l_i - l_j = 0", with
//     S = P(l_i, l_i) + P(l_j, l_j) - P(l_i, l_j) - P(l_i, l_j)' + R        nu = -(l_i - l_j)
// -- by definition the value ekf_landmark_distance(h, i, j, NULL, R) yields, so every pair goes through the SAME two functions the
// host runs there (ekfm::constrain_S, ekfm::constrain_d2) on the same operands: the cross block from the tiles (a canonical
// lower-triangle entry for j < i, taken as constrain_small_entry takes it), both own blocks from the live F64 copies, the positions
// from x.  Nothing is written but the N results: ONE READ-ONLY pass over the stored lower triangle, w * n_mm (n_mm + 1) / 2 bytes.
//
// A wavefront owns kNearestGroup consecutive landmarks (2 * kNearestGroup rows of one tile row: T / 2 is a multiple of the group, so
// a group never straddles a tile edge) and walks their rows from column 0 to the diagonal, 64 lanes x 16 bytes at a time: one
// landmark's column pair per lane with F64 tiles, two landmarks' with float tiles.  With the production tile edges (128 for F64, 256
// for float) one wave instruction loads one whole 1 KiB tile row, the unit k_downdate_w and k_compact_tiles stream.  The column
// operands (x_j, the own block of j: 40 bytes per landmark, arrays that stay in L2) are loaded once per step and serve the whole
// group; the row operands are wave-uniform.  Every lane keeps a running (min d2, j) per row; its columns come in ascending order and
// the comparison is a strict <, so the lowest index wins ties inside a lane, and the wave reduction at the end orders by (d2, j).
// No atomics, no cross-workgroup step, no LDS: the results are deterministic.
//
// Only lanes with j < i take part (on the diagonal tile too), and i < N: nothing at or beyond landmark N is ever a candidate -- the
// zero rows a removal leaves cannot win.  An irregular pair (S not finite, S00 <= 0, det S <= 0: where ekf_landmark_distance yields
// NaN) is skipped, and so is a NaN d2 (a strict < against it is false).  A row without an admissible partner reports (+inf, -1).
//
// Rows cost in proportion to their index: the groups are handed out from the LAST landmark down, so the heavy rows start first.
// ---------------------------------------------------------------------------------------------------
constexpr int kNearestGroup = 2;

template <typename TS>
__global__ __launch_bounds__(kBlock) void k_nearest(DevState st, int cur, int64_t N, double R00, double R01, double R10, double R11,
                                                    NearestEntry *__restrict__ out) {
    using VL = typename Lane16<TS>::type;
    constexpr int kCols = Lane16<TS>::kCols;              // columns per lane: 2 (one landmark) or 4 (two)
    constexpr int kLm = kCols / 2;
    constexpr int G = kNearestGroup;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t ngroups = (N + G - 1) / G;
    const int64_t gi = (int64_t)blockIdx.x * (kBlock / 64) + wave;
    if (gi >= ngroups) return;
    const int64_t i0 = (ngroups - 1 - gi) * G;            // first landmark of the group (wave-uniform)
    const int ni = (int)(N - i0 < G ? N - i0 : G);        // landmarks of the group inside the map
    const int T = st.tm.T;
    const int64_t m = T - 1;
    const int64_t I = (2 * i0) >> st.tm.shift;
    const TS *__restrict__ tiles = (const TS *)st.tiles;
    const int64_t rowoff = ((2 * i0) & m) << st.tm.shift; // row a_i0 inside its tiles
    const double *__restrict__ x = st.x[cur] + 3;
    const double *__restrict__ dg = st.diag[st.dcur];
    const double R[4] = { R00, R01, R10, R11 };

    // the row operands: wave-uniform
    double xi[G][2], di[G][3], best[G];
    int bj[G];
#pragma unroll
    for (int u = 0; u < G; ++u) {
        const int64_t i = u < ni ? i0 + u : i0;
        xi[u][0] = x[2 * i]; xi[u][1] = x[2 * i + 1];
        di[u][0] = dg[3 * i]; di[u][1] = dg[3 * i + 1]; di[u][2] = dg[3 * i + 2];
        best[u] = INFINITY; bj[u] = -1;
    }

    const int64_t jend = i0 + ni - 1;                     // columns j < jend are a candidate of at least one row of the group
    for (int64_t c0 = 0; c0 < jend; c0 += 64 * kLm) {
        const int64_t jl = c0 + (int64_t)lane * kLm;      // the lane's first column landmark
        if (jl >= jend) continue;
        const int64_t col = 2 * jl;
        // (float tiles: the 16 bytes may reach one landmark beyond jend -- still inside the tile, T is a multiple of 4 -- which is
        // loaded and never used)
        const TS *__restrict__ tp = tiles + st.tm.tile_offset(I, col >> st.tm.shift) + rowoff + (col & m);
        VL v[2 * G];
#pragma unroll
        for (int u = 0; u < G; ++u)
            if (u < ni) {
                v[2 * u] = *reinterpret_cast<const VL *>(tp + (int64_t)(2 * u) * T);
                v[2 * u + 1] = *reinterpret_cast<const VL *>(tp + (int64_t)(2 * u + 1) * T);
            }
        double xj[kLm][2], dj[kLm][3];
#pragma unroll
        for (int q = 0; q < kLm; ++q) {
            const int64_t j = jl + q < jend ? jl + q : jl;
            xj[q][0] = x[2 * j]; xj[q][1] = x[2 * j + 1];
            dj[q][0] = dg[3 * j]; dj[q][1] = dg[3 * j + 1]; dj[q][2] = dg[3 * j + 2];
        }
#pragma unroll
        for (int q = 0; q < kLm; ++q) {                   // ascending j inside the lane
            const int64_t j = jl + q;
#pragma unroll
            for (int u = 0; u < G; ++u) {
                if (u < ni && j < i0 + u) {
                    // P(a_i + r, a_j + b) at 2 r + b
                    const double pij[4] = { lane16_get(v[2 * u], 2 * q), lane16_get(v[2 * u], 2 * q + 1),
                                            lane16_get(v[2 * u + 1], 2 * q), lane16_get(v[2 * u + 1], 2 * q + 1) };
                    double S[4], d2;
                    ekfm::constrain_S(di[u], dj[q], pij, R, S);
                    const double nu0 = 0.0 - (xi[u][0] - xj[q][0]), nu1 = 0.0 - (xi[u][1] - xj[q][1]);      // delta = (0, 0)
                    if (ekfm::constrain_d2(S, nu0, nu1, d2) && d2 < best[u]) { best[u] = d2; bj[u] = (int)j; }
                }
            }
        }
    }

    // the wave's winner per row: smaller d2, then smaller j (a lane without a candidate holds (+inf, -1) and never beats one with)
#pragma unroll
    for (int u = 0; u < G; ++u) {
        double b = best[u];
        int j = bj[u];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double ob = __shfl_xor(b, off, 64);
            const int oj = __shfl_xor(j, off, 64);
            const bool take = oj >= 0 && (j < 0 || ob < b || (ob == b && oj < j));
            if (take) { b = ob; j = oj; }
        }
        if (lane == 0 && u < ni) {
            NearestEntry e;
            e.d2 = b; e.partner = j;
            out[i0 + u] = e;
        }
    }
}
