// Fragment of kernels.hip (included there, inside its anonymous namespace, after join_map.h): k_extract_state and k_extract_rows, part of
// a map taken out into ANOTHER handle (ekf_extract_map).
#pragma once

// ---------------------------------------------------------------------------------------------------
// Source state x = [r; l_1 .. l_N] with covariance P (`src`, read only); destination state of m landmarks (`dst`, every value replaced).
// Destination landmark k is source landmark idx[k]; idx holds distinct landmarks in ANY order (compact.h's src_of is strictly increasing
// and maps a store onto itself; here the two stores have their own tile maps and storage kinds, as in join_map.h).
// strip = P(1:3, landmarks), sel = (robot, l_idx[0], .., l_idx[m-1]).
//   EKF_FRAME_MAP     the marginal of sel, a selection: x' = x(sel), P' = P(sel, sel), nothing computed, every value keeps its bits
//                     (one rounding where an F64 store is read into a float store).
//   EKF_FRAME_ROBOT   the chosen landmarks relative to the robot, the robot's uncertainty folded in to first order: r' = 0,
//                     m_k = RELATIVE_XY's h at (r, l_idx[k]) (ekfm::model_eval model 4: its expressions, extract_relative_xy below),
//                     Prr' = 0, strip' = 0 and, with Hr_k / Hl that model's blocks on the robot and on the landmark,
//                       P'(k, a) = Hr_k Prr Hr_a' + Hr_k strip(:, idx[a]) Hl' + Hl strip(:, idx[k])' Hr_a' + Hl P(l_idx[k], l_idx[a]) Hl'
//                     the four terms formed in this order and added left to right (extract_robot_block: one text for the tiles and the
//                     diagonal copies).  A landmark exactly on the robot is regular here: m_k = 0, Hr_k's heading column 0.
// Source block (idx[k], idx[a]): the canonical lower entry where idx[k] > idx[a], block (idx[a], idx[k]) transposed where idx[k] < idx[a],
// the live F64 diagonal copy where a = k (never the tile's own copy of it).
// k_extract_state writes a COMPLETE buffer a.dcur of dst (x, Prr, strip: zero from column 2 m to the end of the last tile row), s and the
// diagonal copies diag[dst.dcur]; k_extract_rows writes tile rows 0 .. padded(2 m) - 1, diagonal tiles whole, zero beyond 2 m.  Neither
// reads a slot either writes (the source is another handle), so the two launches and their workgroups need no order among themselves.
// ---------------------------------------------------------------------------------------------------

// RELATIVE_XY's h at (xr, l) and its block on the robot from the sine and cosine model_eval takes of the heading: its expressions, without
// the q > 0 guard that belongs to the range models
__device__ __forceinline__ void extract_relative_xy(const double xr[3], double s, double c, double lx, double ly, double mk[2], double Hr[2][3]) {
    const double dx = lx - xr[0], dy = ly - xr[1];
    mk[0] = c * dx + s * dy;
    mk[1] = c * dy - s * dx;
    Hr[0][0] = -c; Hr[0][1] = -s; Hr[0][2] = mk[1] / ekfm::kR2D;
    Hr[1][0] = s; Hr[1][1] = -c; Hr[1][2] = -mk[0] / ekfm::kR2D;
}

// P'(k, a) of the robot frame.  sk / sa: the strip columns of the two source landmarks (sk[r][j] = strip(r, 2 idx[k] + j)); B: the source
// block P(l_idx[k], l_idx[a]) row-major; Hl = [c s; -s c].  Each term's sums run left to right, the terms are added in the order written.
__device__ __forceinline__ void extract_robot_block(const double Hrk[2][3], const double Hra[2][3], double s, double c, const double *prr,
                                                    const double sk[3][2], const double sa[3][2], const double B[4], double o[4]) {
    const double Hl[2][2] = { { c, s }, { -s, c } };
    double U[2][3], V[2][2], W[2][3], X[2][2];
    for (int i = 0; i < 2; ++i) for (int j = 0; j < 3; ++j) {
        double acc = 0; for (int r = 0; r < 3; ++r) acc += Hrk[i][r] * prr[3 * r + j]; U[i][j] = acc; }
    for (int i = 0; i < 2; ++i) for (int j = 0; j < 2; ++j) {
        double acc = 0; for (int r = 0; r < 3; ++r) acc += Hrk[i][r] * sa[r][j]; V[i][j] = acc; }
    for (int i = 0; i < 2; ++i) for (int r = 0; r < 3; ++r) {
        double acc = 0; for (int q = 0; q < 2; ++q) acc += Hl[i][q] * sk[r][q]; W[i][r] = acc; }
    for (int i = 0; i < 2; ++i) for (int j = 0; j < 2; ++j) {
        double acc = 0; for (int q = 0; q < 2; ++q) acc += Hl[i][q] * B[2 * q + j]; X[i][j] = acc; }
    for (int i = 0; i < 2; ++i) for (int j = 0; j < 2; ++j) {
        double t1 = 0, t2 = 0, t3 = 0, t4 = 0;
        for (int r = 0; r < 3; ++r) t1 += U[i][r] * Hra[j][r];
        for (int q = 0; q < 2; ++q) t2 += V[i][q] * Hl[j][q];
        for (int r = 0; r < 3; ++r) t3 += W[i][r] * Hra[j][r];
        for (int q = 0; q < 2; ++q) t4 += X[i][q] * Hl[j][q];
        o[2 * i + j] = ((t1 + t2) + t3) + t4;
    }
}

// the strip column pair of source landmark l
__device__ __forceinline__ void extract_strip_cols(const DevState &src, int cur, int64_t l, double sc[3][2]) {
    const double *__restrict__ s = src.strip[cur];
    for (int r = 0; r < 3; ++r) {
        const double2 t = *reinterpret_cast<const double2 *>(s + r * src.ldm + 2 * l);
        sc[r][0] = t.x; sc[r][1] = t.y;
    }
}

// The own block of destination landmark k = source landmark l as (P'(0,0), P'(1,0), P'(1,1)): the live F64 diagonal copy, in the robot
// frame through extract_robot_block with a = k -- its off-diagonal entry is computed once, as entry (1, 0), and serves both places.
__device__ __forceinline__ void extract_own_block(const DevState &src, int cur, int frame, const double *xr, double s, double c, const double *prr,
                                                  int64_t l, double o[3]) {
    const double *__restrict__ d = src.diag[src.dcur] + 3 * l;
    o[0] = d[0]; o[1] = d[1]; o[2] = d[2];
    if (frame == 0) return;
    double mk[2], Hr[2][3], sk[3][2], blk[4];
    const double *__restrict__ x = src.x[cur];
    extract_relative_xy(xr, s, c, x[3 + 2 * l], x[3 + 2 * l + 1], mk, Hr);
    extract_strip_cols(src, cur, l, sk);
    const double B[4] = { o[0], o[1], o[1], o[2] };
    extract_robot_block(Hr, Hr, s, c, prr, sk, sk, B, blk);
    o[0] = blk[0]; o[1] = blk[2]; o[2] = blk[3];
}

// what lane 0 of a workgroup leaves in LDS: the source pose, the sine and cosine of its heading, Prr
struct ExtractSmall { double xr[3], s, c, prr[9]; };
__device__ __forceinline__ void extract_small(const DevState &src, int cur, ExtractSmall &o) {
    for (int i = 0; i < 3; ++i) o.xr[i] = src.x[cur][i];
    for (int i = 0; i < 9; ++i) o.prr[i] = src.prr[cur][i];
    const double2 sc = sincosd_ni(o.xr[2]);
    o.s = sc.x; o.c = sc.y;
}

// One lane per destination column c < a.cols = padded(2 m) of dst's tile map (at least 1 workgroup), 256 per workgroup; the small part by
// every workgroup on lane 0, the pose and Prr' by workgroup 0.
__global__ __launch_bounds__(kBlock) void k_extract_state(DevState dst, DevState src, ExtractMapArgs a, const int32_t *__restrict__ idx) {
    __shared__ ExtractSmall sm;
    const int tid = threadIdx.x;
    const int scur = a.scur, dcur = a.dcur;
    if (tid == 0) extract_small(src, scur, sm);
    __syncthreads();
    const bool robot = a.frame != 0;
    if (blockIdx.x == 0 && tid == 0) {
        for (int i = 0; i < 3; ++i) dst.x[dcur][i] = robot ? 0.0 : sm.xr[i];
        for (int i = 0; i < 9; ++i) dst.prr[dcur][i] = robot ? 0.0 : sm.prr[i];
    }
    const int64_t c = (int64_t)blockIdx.x * kBlock + tid;
    if (c >= a.cols) return;
    double *__restrict__ xn = dst.x[dcur];
    double *__restrict__ sn = dst.strip[dcur];
    if (c >= 2 * a.m) {
        xn[3 + c] = 0.0;
        for (int r = 0; r < 3; ++r) sn[r * dst.ldm + c] = 0.0;
        return;
    }
    const int64_t k = c >> 1, l = idx[k];
    const int j = (int)(c & 1);
    const double *__restrict__ x = src.x[scur];
    if (robot) {
        double mk[2], Hr[2][3];
        extract_relative_xy(sm.xr, sm.s, sm.c, x[3 + 2 * l], x[3 + 2 * l + 1], mk, Hr);
        xn[3 + c] = mk[j];
        for (int r = 0; r < 3; ++r) sn[r * dst.ldm + c] = 0.0;
    } else {
        xn[3 + c] = x[3 + 2 * l + j];
        for (int r = 0; r < 3; ++r) sn[r * dst.ldm + c] = src.strip[scur][r * src.ldm + 2 * l + j];
    }
    if (j == 0) {
        dst.s[k] = src.s[l];
        double own[3];
        extract_own_block(src, scur, a.frame, sm.xr, sm.s, sm.c, sm.prr, l, own);
        double *__restrict__ dg = dst.diag[dst.dcur] + 3 * k;
        dg[0] = own[0]; dg[1] = own[1]; dg[2] = own[2];
    }
}

// The tile rows.  Workgroup b serves ONE destination landmark k = b / blocks_per_row (rows 2 k, 2 k + 1) and 256 consecutive column
// landmarks of it: a lane owns one 2 x 2 block, two rows times two adjacent columns, so a wavefront writes contiguous runs of a tile row.
// The columns of a row end with its diagonal tile (stored whole: an upper block there is the lower one of the same pair, transposed, so the
// two halves of a diagonal tile agree bit for bit in either frame); rows and columns from landmark m on are zero.  The store is addressed
// through dst's tile map, the loads through src's; both tile edges are even, so no block straddles a tile edge on either side.
template <typename TSdst, typename TSsrc>
__global__ __launch_bounds__(kBlock) void k_extract_rows(DevState dst, DevState src, ExtractMapArgs a, const int32_t *__restrict__ idx,
                                                         int32_t blocks_per_row) {
    __shared__ ExtractSmall sm;
    const int tid = threadIdx.x;
    const int64_t k = blockIdx.x / (uint32_t)blocks_per_row;
    const int64_t cl0 = (int64_t)(blockIdx.x - (uint32_t)k * (uint32_t)blocks_per_row) * kBlock;
    const int64_t cend = (((2 * k) >> dst.tm.shift) + 1) << (dst.tm.shift - 1);       // the first column landmark behind the row's diagonal tile
    if (cl0 >= cend) return;                                // (the whole workgroup)
    const bool robot = a.frame != 0;
    if (tid == 0 && robot) extract_small(src, a.scur, sm);
    __syncthreads();
    const int64_t cl = cl0 + tid;
    if (cl >= cend) return;
    TSdst *__restrict__ tiles = (TSdst *)dst.tiles;
    const int64_t r0 = 2 * k, c0 = 2 * cl;
    if (k >= a.m || cl >= a.m) {
        pmm_low_store_pair<TSdst>(tiles, dst.tm, r0, c0, 0.0, 0.0);
        pmm_low_store_pair<TSdst>(tiles, dst.tm, r0 + 1, c0, 0.0, 0.0);
        return;
    }
    if (cl == k) {
        double own[3];
        extract_own_block(src, a.scur, a.frame, sm.xr, sm.s, sm.c, sm.prr, idx[k], own);
        pmm_low_store_pair<TSdst>(tiles, dst.tm, r0, c0, own[0], own[1]);
        pmm_low_store_pair<TSdst>(tiles, dst.tm, r0 + 1, c0, own[1], own[2]);
        return;
    }
    // the pair (hi, lo) of destination landmarks whose LOWER block this lane forms; an upper block of the diagonal tile stores it transposed
    const bool upper = cl > k;
    const int64_t lh = idx[upper ? cl : k], ll = idx[upper ? k : cl];
    double B[4];                                            // P(l_lh, l_ll), row-major
    if (lh > ll) {
        pmm_low_pair<TSsrc>((const TSsrc *)src.tiles, src.tm, 2 * lh, 2 * ll, B[0], B[1]);
        pmm_low_pair<TSsrc>((const TSsrc *)src.tiles, src.tm, 2 * lh + 1, 2 * ll, B[2], B[3]);
    } else {
        pmm_low_pair<TSsrc>((const TSsrc *)src.tiles, src.tm, 2 * ll, 2 * lh, B[0], B[2]);
        pmm_low_pair<TSsrc>((const TSsrc *)src.tiles, src.tm, 2 * ll + 1, 2 * lh, B[1], B[3]);
    }
    double o[4] = { B[0], B[1], B[2], B[3] };
    if (robot) {
        const double *__restrict__ x = src.x[a.scur];
        double mh[2], ml[2], Hrh[2][3], Hrl[2][3], sh[3][2], sl[3][2];
        extract_relative_xy(sm.xr, sm.s, sm.c, x[3 + 2 * lh], x[3 + 2 * lh + 1], mh, Hrh);
        extract_relative_xy(sm.xr, sm.s, sm.c, x[3 + 2 * ll], x[3 + 2 * ll + 1], ml, Hrl);
        extract_strip_cols(src, a.scur, lh, sh);
        extract_strip_cols(src, a.scur, ll, sl);
        extract_robot_block(Hrh, Hrl, sm.s, sm.c, sm.prr, sh, sl, B, o);
    }
    if (upper) { const double t = o[1]; o[1] = o[2]; o[2] = t; }
    pmm_low_store_pair<TSdst>(tiles, dst.tm, r0, c0, o[0], o[1]);
    pmm_low_store_pair<TSdst>(tiles, dst.tm, r0 + 1, c0, o[2], o[3]);
}
