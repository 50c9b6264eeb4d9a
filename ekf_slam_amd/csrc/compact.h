// Fragment of kernels.hip (included there, inside its anonymous namespace, after tile_access.h / downdate.h): landmark removal as an
// order-preserving compaction of the state (ekf_remove_landmarks): k_compact_tiles, k_compact_state.
#pragma once

// ---------------------------------------------------------------------------------------------------
// Marginalising landmarks out of the Gaussian = dropping their entries of x, s and their rows and columns of P.  In the tiled
// layout that is a copy: element (r', c') of the new landmark block is element (src(r'), src(c')) of the old one, with
// src(2k' + a) = 2 src_of[k'] + a and src_of (new landmark -> old landmark) strictly increasing -- so the lower triangle maps to
// the lower triangle, a landmark's 2 x 2 block stays a 2 x 2 block, and a destination tile row reads a few contiguous runs of at
// most two source tile rows.  Nothing is computed: every surviving value keeps its bits, in either storage type.
//
// OUT OF PLACE (the project's rule: no workgroup reads what another workgroup of the same launch writes): `src` and `dst` are
// different tile stores.  src_of holds -1 from the new landmark count on, up to the padded capacity: rows and columns beyond
// the new map are written as zero, which is what a fresh store and k_lowrank_tiles leave there.
//
// A work item is 16 KiB of one destination tile (kCompactRows 16-byte pieces per lane); consecutive lanes own consecutive
// 16-byte pieces of a tile row, so with the production tile edges (128 for F64, 256 for float) one wave instruction stores one
// whole 1 KiB tile row and loads it from a 1 KiB run that every removed landmark before it shifts by 16 (F64) or 8 bytes (float):
// F64 loads stay 16-byte aligned, float loads are issued as two 8-byte halves (one per landmark).
// ---------------------------------------------------------------------------------------------------
constexpr int kCompactRows = 4;

// elements (2 lr + rbit, 2 lc) and (2 lr + rbit, 2 lc + 1) of the old landmark block; lr < 0 or lc < 0: beyond the new map.
// kDiag: the destination is a diagonal tile, whose upper half (lr < lc) takes the canonical entries transposed -- a diagonal tile is
// stored whole, only its lower half is ever read.
template <typename TS, bool kDiag>
__device__ __forceinline__ typename Vec2<TS>::type compact_pair(const TS *__restrict__ tiles, const TileMap &tm, int lr, int rbit, int lc) {
    typename Vec2<TS>::type v;
    v.x = (TS)0; v.y = (TS)0;
    if (lr < 0 || lc < 0) return v;
    const int64_t m = tm.T - 1;
    const int64_t r = 2 * (int64_t)lr + rbit, c = 2 * (int64_t)lc;
    if (!kDiag || lr >= lc) {
        // (lr == lc: the landmark's own block, inside one diagonal tile and stored whole)
        v = *reinterpret_cast<const typename Vec2<TS>::type *>(tiles + tm.tile_offset(r >> tm.shift, c >> tm.shift) + ((r & m) << tm.shift) + (c & m));
    } else {
        const TS *__restrict__ p = tiles + tm.tile_offset(c >> tm.shift, r >> tm.shift) + ((c & m) << tm.shift) + (r & m);
        v.x = p[0]; v.y = p[tm.T];              // rows c, c + 1 of one tile (T is even)
    }
    return v;
}

// one lane's 16-byte piece of a destination row: one landmark's column pair (F64) or two landmarks' (float)
template <typename TS, bool kDiag>
__device__ __forceinline__ typename Lane16<TS>::type compact_piece(const TS *__restrict__ tiles, const TileMap &tm, int lr, int rbit, int lc0, int lc1) {
    if constexpr (Lane16<TS>::kCols == 2) {
        return compact_pair<TS, kDiag>(tiles, tm, lr, rbit, lc0);
    } else {
        const float2 a = compact_pair<TS, kDiag>(tiles, tm, lr, rbit, lc0), b = compact_pair<TS, kDiag>(tiles, tm, lr, rbit, lc1);
        return make_float4(a.x, a.y, b.x, b.y);
    }
}

// work: the destination tiles (I, J), `items_per_tile` work items each; grid = ntiles * items_per_tile workgroups
template <typename TS>
__global__ __launch_bounds__(kBlock) void k_compact_tiles(const TS *__restrict__ src, TS *__restrict__ dst, const int2 *__restrict__ work,
                                                          int items_per_tile, const int32_t *__restrict__ src_of, TileMap tm) {
    using VL = typename Lane16<TS>::type;
    constexpr int kCols = Lane16<TS>::kCols;              // columns per lane: 2 (one landmark) or 4 (two)
    constexpr int kColShift = kCols == 2 ? 1 : 2;
    const int T = tm.T;
    const int lshift = tm.shift - kColShift;              // log2 of the 16-byte pieces of a tile row
    const int pieces = T << lshift;                       // ... and of a tile
    const int64_t w = blockIdx.x / (unsigned)items_per_tile;
    const int chunk = (int)(blockIdx.x - w * items_per_tile);
    const int2 ij = work[w];
    const int tid = threadIdx.x;
    // kBlock is a multiple of the pieces of a row: a lane stays on one column group for all its rows
    const int cl = tid & ((1 << lshift) - 1);
    const int64_t lcol = (((int64_t)ij.y * T) >> 1) + (cl << (kColShift - 1));       // destination landmark of the lane's first column
    const int lc0 = src_of[lcol], lc1 = kCols == 4 ? src_of[lcol + 1] : -1;
    TS *__restrict__ td = dst + tm.tile_offset(ij.x, ij.y);
    int rr[kCompactRows], lr[kCompactRows];
#pragma unroll
    for (int u = 0; u < kCompactRows; ++u) {
        const int p = (chunk * kCompactRows + u) * kBlock + tid;
        rr[u] = p < pieces ? p >> lshift : -1;            // tile row; -1: beyond the tile (tiles smaller than a work item)
        lr[u] = rr[u] >= 0 ? src_of[((int64_t)ij.x * T + rr[u]) >> 1] : -1;
    }
    VL v[kCompactRows];
    if (ij.x != ij.y) {
#pragma unroll
        for (int u = 0; u < kCompactRows; ++u) v[u] = compact_piece<TS, false>(src, tm, lr[u], rr[u] & 1, lc0, lc1);
    } else {
#pragma unroll
        for (int u = 0; u < kCompactRows; ++u) v[u] = compact_piece<TS, true>(src, tm, lr[u], rr[u] & 1, lc0, lc1);
    }
#pragma unroll
    for (int u = 0; u < kCompactRows; ++u)
        if (rr[u] >= 0) *reinterpret_cast<VL *>(td + ((int64_t)rr[u] << tm.shift) + kCols * cl) = v[u];
}

// The replicated state of the same removal: x, the three strip rows and the landmarks' live diagonal blocks from buffer cur / dcur
// into cur ^ 1 / dcur ^ 1 (one lane per landmark of the OLD map; zero from the new count on), the pose and Prr copied, the
// signatures compacted into s_out (s itself is single-buffered: the caller copies s_out back in stream order).
__global__ __launch_bounds__(kBlock) void k_compact_state(DevState st, int cur, const int32_t *__restrict__ src_of, int64_t N_old,
                                                          double *__restrict__ s_out) {
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k == 0) {
        for (int i = 0; i < 3; ++i) st.x[cur ^ 1][i] = st.x[cur][i];
        for (int i = 0; i < 9; ++i) st.prr[cur ^ 1][i] = st.prr[cur][i];
    }
    if (k >= N_old) return;
    const int l = src_of[k];
    const bool live = l >= 0;
    const double2 zero = make_double2(0.0, 0.0);
    // (x + 3 is 8-byte aligned only: plain loads)
    for (int a = 0; a < 2; ++a) st.x[cur ^ 1][3 + 2 * k + a] = live ? st.x[cur][3 + 2 * (int64_t)l + a] : 0.0;
    for (int r = 0; r < 3; ++r) {
        const double2 t = live ? *reinterpret_cast<const double2 *>(st.strip[cur] + r * st.ldm + 2 * (int64_t)l) : zero;
        *reinterpret_cast<double2 *>(st.strip[cur ^ 1] + r * st.ldm + 2 * k) = t;
    }
    for (int q = 0; q < 3; ++q) st.diag[st.dcur ^ 1][3 * k + q] = live ? st.diag[st.dcur][3 * (int64_t)l + q] : 0.0;
    s_out[k] = live ? st.s[l] : 0.0;
}
