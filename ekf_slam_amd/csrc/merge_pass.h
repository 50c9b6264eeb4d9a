// Fragment of kernels.hip (included there, inside its anonymous namespace, after compact.h / constrain.h): the fused pass of
// ekf_merge_landmarks_batch: k_merge_pass.
#pragma once

// ---------------------------------------------------------------------------------------------------
// m constraints between landmarks followed by the removal of m landmarks, as ONE pass over P: the downdate of k_downdate's pair loop
// carried out WHILE the tile store is compacted the way k_compact_tiles compacts it.  Element (r', c') of the new landmark block is
//     old(src(r'), src(c')) - sum_l K_l(src(r'), :) . G_l(:, src(c'))          (rank2_apply, slot order l = 0 .. npairs-1)
// with src(2k' + a) = 2 src_of[k'] + a: every element is loaded once, takes the npairs pairs in registers, is converted to the
// storage type once and stored once -- one read of the old triangle and one write of the new one, where a merge-by-merge run reads
// and writes P twice per merge (the one-pair pass, then the compaction) and rounds a float entry once per merge.
//
// OUT OF PLACE, over ALL tile rows of the old map (every entry changes: there is no unchanged prefix): src_of holds -1 from the new
// landmark count on, so the rows and columns beyond the new map -- and the tile rows it no longer reaches -- are written as zero.
// The work item and the addressing are k_compact_tiles' (16-byte pieces per lane, consecutive lanes on consecutive pieces of a tile
// row: with the production tile edges one wave instruction stores one whole 1 KiB tile row, whose K is then one wave-uniform
// address; the lane's G values are L2 hits).  K and G are indexed by the SOURCE row and column, so nothing is read at or beyond
// 2 N_old.  On a diagonal tile the upper half takes the canonical entry mirrored, with the canonical entry's row and column in the chain.
// ---------------------------------------------------------------------------------------------------
template <typename TS, bool kDiag>
__device__ __forceinline__ void merge_rows(const TS *__restrict__ src, const TileMap &tm, const double *__restrict__ Kp, const double *__restrict__ Gp,
                                           int64_t pair_stride, int npairs, const int (&lr)[kCompactRows], const int (&rr)[kCompactRows],
                                           const int (&lc)[Lane16<TS>::kCols / 2], double (&v)[kCompactRows][Lane16<TS>::kCols]) {
    constexpr int kL = Lane16<TS>::kCols / 2;             // landmarks per lane
#pragma unroll
    for (int u = 0; u < kCompactRows; ++u)
#pragma unroll
        for (int t = 0; t < kL; ++t) {
            const typename Vec2<TS>::type p = compact_pair<TS, kDiag>(src, tm, lr[u], rr[u] & 1, lc[t]);      // zero beyond the new map
            v[u][2 * t] = (double)p.x; v[u][2 * t + 1] = (double)p.y;
        }
    // source indices, clamped into the state where the piece lies beyond the new map (its value is put back to zero below)
    int64_t krow[kCompactRows], gcol[kL];
#pragma unroll
    for (int u = 0; u < kCompactRows; ++u) krow[u] = lr[u] < 0 ? 0 : 2 * (int64_t)lr[u] + (rr[u] & 1);
#pragma unroll
    for (int t = 0; t < kL; ++t) gcol[t] = lc[t] < 0 ? 0 : 2 * (int64_t)lc[t];
    for (int i = 0; i < npairs; ++i) {
        const double2 *__restrict__ G2 = reinterpret_cast<const double2 *>(Gp + (int64_t)i * pair_stride);
        const double2 *__restrict__ K2 = reinterpret_cast<const double2 *>(Kp + (int64_t)i * pair_stride);
        if constexpr (!kDiag) {
            double2 g[2 * kL];
#pragma unroll
            for (int t = 0; t < kL; ++t) { g[2 * t] = G2[gcol[t]]; g[2 * t + 1] = G2[gcol[t] + 1]; }
#pragma unroll
            for (int u = 0; u < kCompactRows; ++u) {
                const double2 k = K2[krow[u]];
#pragma unroll
                for (int q = 0; q < 2 * kL; ++q) v[u][q] = rank2_apply(v[u][q], k, g[q]);
            }
        } else {
#pragma unroll
            for (int u = 0; u < kCompactRows; ++u)
#pragma unroll
                for (int t = 0; t < kL; ++t) {
                    // lr < lc: the piece mirrors the canonical entries (c, r) and (c + 1, r)
                    const bool mir = lr[u] < lc[t];
                    const int64_t r = krow[u], c = gcol[t];
                    const double2 ka = K2[mir ? c : r], kb = K2[mir ? c + 1 : r];
                    const double2 ga = G2[mir ? r : c], gb = G2[mir ? r : c + 1];
                    v[u][2 * t] = rank2_apply(v[u][2 * t], ka, ga);
                    v[u][2 * t + 1] = rank2_apply(v[u][2 * t + 1], kb, gb);
                }
        }
    }
#pragma unroll
    for (int u = 0; u < kCompactRows; ++u)
#pragma unroll
        for (int t = 0; t < kL; ++t)
            if (lr[u] < 0 || lc[t] < 0) { v[u][2 * t] = 0.0; v[u][2 * t + 1] = 0.0; }
}

// work: the destination tiles (I, J) -- every tile of the OLD map's tile rows -- `items_per_tile` work items each; Kp / Gp: slot 0 of
// the batch's pair ring, slots pair_stride doubles apart, applied in slot order
template <typename TS>
__global__ __launch_bounds__(kBlock) void k_merge_pass(const TS *__restrict__ src, TS *__restrict__ dst, const int2 *__restrict__ work,
                                                       int items_per_tile, const int32_t *__restrict__ src_of,
                                                       const double *__restrict__ Kp, const double *__restrict__ Gp, int64_t pair_stride,
                                                       int npairs, TileMap tm) {
    using VL = typename Lane16<TS>::type;
    constexpr int kCols = Lane16<TS>::kCols;
    constexpr int kColShift = kCols == 2 ? 1 : 2;
    const int T = tm.T;
    const int lshift = tm.shift - kColShift;
    const int pieces = T << lshift;
    const int64_t w = blockIdx.x / (unsigned)items_per_tile;
    const int chunk = (int)(blockIdx.x - w * items_per_tile);
    const int2 ij = work[w];
    const int tid = threadIdx.x;
    const int cl = tid & ((1 << lshift) - 1);
    const int64_t lcol = (((int64_t)ij.y * T) >> 1) + (cl << (kColShift - 1));
    int lc[kCols / 2];
    lc[0] = src_of[lcol];
    if constexpr (kCols == 4) lc[1] = src_of[lcol + 1];
    TS *__restrict__ td = dst + tm.tile_offset(ij.x, ij.y);
    int rr[kCompactRows], lr[kCompactRows];
#pragma unroll
    for (int u = 0; u < kCompactRows; ++u) {
        const int p = (chunk * kCompactRows + u) * kBlock + tid;
        rr[u] = p < pieces ? p >> lshift : -1;
        lr[u] = rr[u] >= 0 ? src_of[((int64_t)ij.x * T + rr[u]) >> 1] : -1;
    }
    double v[kCompactRows][kCols];
    if (ij.x != ij.y) merge_rows<TS, false>(src, tm, Kp, Gp, pair_stride, npairs, lr, rr, lc, v);
    else merge_rows<TS, true>(src, tm, Kp, Gp, pair_stride, npairs, lr, rr, lc, v);
#pragma unroll
    for (int u = 0; u < kCompactRows; ++u)
        if (rr[u] >= 0) {
            VL o;
            lane16_pack(v[u], o);
            *reinterpret_cast<VL *>(td + ((int64_t)rr[u] << tm.shift) + kCols * cl) = o;
        }
}
