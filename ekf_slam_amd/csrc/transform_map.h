// Fragment of kernels.hip (included there, inside its anonymous namespace, after extract_map.h): k_transform_state and k_transform_tiles,
// the WHOLE map moved into another frame, in place (ekf_transform_map).
#pragma once

// ---------------------------------------------------------------------------------------------------
// State x = [r; l_1 .. l_N] with covariance P, strip = P(1:3, landmarks), k = 180 / pi.  N and s stay.
//   rigid (forms 0, 1)  the map stays a map, moved by t = (tx, ty, phi) with covariance Sigma, independent of the state.  With (s, c) the
//                       degree sine and cosine of phi, Rot = [c -s; s c] and w(v) = Rot v:
//                         r'   = t (+) r            ekfm::motion_eval POSE_DELTA at (xr = t, u = r): F = I + [fa; fb] in the heading column,
//                                                   V = blockdiag(Rot, 1)
//                         l_i' = t_xy + w(l_i)      ekfm::model_invert RELATIVE_XY at (t, l_i) (join_invert_xy: its expressions),
//                                                   A_i = its Gx = [1 0 g0_i; 0 1 g1_i]
//                       and P' = T P T' + A Sigma A', T = blockdiag(V, Rot, .., Rot), A = (F; A_1; ..; A_N), block by block, every sum left
//                       to right, the rotation term first:
//                         Prr'         = V Prr V' + F Sigma F'
//                         strip'(:, i) = V strip(:, i) Rot' + F Sigma A_i'
//                         P'(i, j)     = Rot P(i, j) Rot' + A_i Sigma A_j'
//                       Form 0 (Sigma = 0) does not form the Sigma terms: the rotation alone, exact where (s, c) is (0, 1) or (1, 0).
//   robot (form 2)      the robot's own pose becomes the origin: what k_extract_state / k_extract_rows leave for idx = (0 .. N - 1) in
//                       EKF_FRAME_ROBOT, through their text (extract_relative_xy, extract_robot_block, extract_own_block): r' = 0,
//                       Prr' = 0, strip' = 0, the four-term block of extract_map.h's header.
// Every 2 x 2 block of P' depends on its own old block and on replicated data of the OLD buffers (x, Prr, the strip, the diagonal copies of
// buffer cur / dcur) alone, so the tiles are transformed IN PLACE: a lane reads and writes only blocks it owns.  k_transform_state reads the
// old buffers and writes a COMPLETE buffer cur ^ 1 (x, Prr, the strip: zero from column 2 N to the end of the last tile row) and the
// diagonal copies diag[dcur ^ 1]; the caller flips both.  Neither kernel reads what either writes, so the two launches and their
// workgroups need no order among themselves.  A landmark's own block comes from the live F64 diagonal copy and goes to both places.
// ---------------------------------------------------------------------------------------------------

// what lane 0 of a workgroup leaves in LDS
struct TransformSmall {
    double s, c;                    // rigid: of phi; robot: of the robot's heading
    double xr[3], prr[9];           // the old pose and Prr
    double xn[3], fa, fb, V[9];     // k_transform_state, rigid: the robot's composition
    double FS[9];                   // ... form 1: F Sigma, row-major
};
__device__ __forceinline__ void transform_small(const DevState &st, const TransformMapArgs &a, bool state, TransformSmall &o) {
    for (int i = 0; i < 3; ++i) o.xr[i] = st.x[a.cur][i];
    for (int i = 0; i < 9; ++i) o.prr[i] = st.prr[a.cur][i];
    const double2 sc = sincosd_ni(a.form == 2 ? o.xr[2] : a.t[2]);
    o.s = sc.x; o.c = sc.y;
    if (!state || a.form == 2) return;
    ekfm::motion_eval_with(MotionSinCosNi(), 3, a.t, o.xr, o.xn, o.fa, o.fb, o.V);
    if (a.form != 1) return;
    const double F[3][3] = { { 1.0, 0.0, o.fa }, { 0.0, 1.0, o.fb }, { 0.0, 0.0, 1.0 } };
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) {
        double acc = 0; for (int q = 0; q < 3; ++q) acc += F[i][q] * a.Sigma[3 * q + j]; o.FS[3 * i + j] = acc; }
}

// What a block needs of ONE of its two landmarks.  Rigid, form 1: g = dl'/dphi (join_invert_xy's gth); form 0: nothing.  Robot: RELATIVE_XY's
// block on the robot and the landmark's strip columns.
template <int kForm> struct TransformOp;
template <> struct TransformOp<0> {};
template <> struct TransformOp<1> { double g[2]; };
template <> struct TransformOp<2> { double Hr[2][3], sk[3][2]; };
template <int kForm>
__device__ __forceinline__ void transform_op(const DevState &st, const TransformMapArgs &a, const TransformSmall &sm, int64_t l, TransformOp<kForm> &o) {
    if constexpr (kForm == 1) {
        const double *__restrict__ x = st.x[a.cur];
        double tp[2];
        join_invert_xy(a.t, sm.s, sm.c, x[3 + 2 * l], x[3 + 2 * l + 1], tp, o.g);
    } else if constexpr (kForm == 2) {
        const double *__restrict__ x = st.x[a.cur];
        double mk[2];
        extract_relative_xy(sm.xr, sm.s, sm.c, x[3 + 2 * l], x[3 + 2 * l + 1], mk, o.Hr);
        extract_strip_cols(st, a.cur, l, o.sk);
    }
}

// A_i Sigma A_j' (row-major 2 x 2) from the heading columns g of the two landmarks: every product of the sums is formed, left to right
__device__ __forceinline__ void transform_sigma_block(const double gi[2], const double gj[2], const double *Sg, double o[4]) {
    const double Ai[2][3] = { { 1.0, 0.0, gi[0] }, { 0.0, 1.0, gi[1] } }, Aj[2][3] = { { 1.0, 0.0, gj[0] }, { 0.0, 1.0, gj[1] } };
    double M[2][3];
    for (int i = 0; i < 2; ++i) for (int q = 0; q < 3; ++q) {
        double acc = 0; for (int r = 0; r < 3; ++r) acc += Ai[i][r] * Sg[3 * r + q]; M[i][q] = acc; }
    for (int i = 0; i < 2; ++i) for (int j = 0; j < 2; ++j) {
        double acc = 0; for (int q = 0; q < 3; ++q) acc += M[i][q] * Aj[j][q]; o[2 * i + j] = acc; }
}

// P'(i, j) from B = P(i, j), row-major
template <int kForm>
__device__ __forceinline__ void transform_block(const TransformMapArgs &a, const TransformSmall &sm, const TransformOp<kForm> &ri,
                                                const TransformOp<kForm> &cj, const double B[4], double o[4]) {
    if constexpr (kForm == 2) {
        extract_robot_block(ri.Hr, cj.Hr, sm.s, sm.c, sm.prr, ri.sk, cj.sk, B, o);
    } else {
        const double Gz[4] = { sm.c, -sm.s, sm.s, sm.c };
        join_rotate_block(Gz, B[0], B[1], B[2], B[3], o);
        if constexpr (kForm == 1) {
            double e[4];
            transform_sigma_block(ri.g, cj.g, a.Sigma, e);
            for (int q = 0; q < 4; ++q) o[q] = o[q] + e[q];
        }
    }
}

// The own block of landmark l as (P'(0,0), P'(1,0), P'(1,1)) from the live F64 diagonal copy: its off-diagonal entry is computed once, as
// entry (1, 0), and serves both places (extract_own_block: the same rule, and the robot form IS that function)
template <int kForm>
__device__ __forceinline__ void transform_own_block(const DevState &st, const TransformMapArgs &a, const TransformSmall &sm, int64_t l, double o[3]) {
    if constexpr (kForm == 2) {
        extract_own_block(st, a.cur, 1, sm.xr, sm.s, sm.c, sm.prr, l, o);
    } else {
        const double *__restrict__ d = st.diag[st.dcur] + 3 * l;
        const double B[4] = { d[0], d[1], d[1], d[2] };
        TransformOp<kForm> op;
        transform_op<kForm>(st, a, sm, l, op);
        double blk[4];
        transform_block<kForm>(a, sm, op, op, B, blk);
        o[0] = blk[0]; o[1] = blk[2]; o[2] = blk[3];
    }
}

// One lane per column c < a.cols = padded(2 N) (at least 1 workgroup), 256 per workgroup; the small part by every workgroup on lane 0, the
// pose and Prr' by workgroup 0.
template <int kForm>
__global__ __launch_bounds__(kBlock) void k_transform_state(DevState st, TransformMapArgs a) {
    __shared__ TransformSmall sm;
    const int tid = threadIdx.x;
    const int cur = a.cur, nxt = cur ^ 1;
    if (tid == 0) transform_small(st, a, /*state*/ true, sm);
    __syncthreads();
    if (blockIdx.x == 0 && tid == 0) {
        if constexpr (kForm == 2) {
            for (int i = 0; i < 3; ++i) st.x[nxt][i] = 0.0;
            for (int i = 0; i < 9; ++i) st.prr[nxt][i] = 0.0;
        } else {
            double T1[9];
            for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) {
                double acc = 0; for (int q = 0; q < 3; ++q) acc += sm.V[3 * i + q] * sm.prr[3 * q + j]; T1[3 * i + j] = acc; }
            const double F[3][3] = { { 1.0, 0.0, sm.fa }, { 0.0, 1.0, sm.fb }, { 0.0, 0.0, 1.0 } };
            // the lower triangle, mirrored: Prr' is symmetric bit for bit
            for (int i = 0; i < 3; ++i) for (int j = 0; j <= i; ++j) {
                double acc = 0; for (int q = 0; q < 3; ++q) acc += T1[3 * i + q] * sm.V[3 * j + q];
                if constexpr (kForm == 1) {
                    double e = 0; for (int q = 0; q < 3; ++q) e += sm.FS[3 * i + q] * F[j][q];
                    acc = acc + e;
                }
                st.prr[nxt][3 * i + j] = acc;
                st.prr[nxt][3 * j + i] = acc;
            }
            for (int i = 0; i < 3; ++i) st.x[nxt][i] = sm.xn[i];
        }
    }
    const int64_t c = (int64_t)blockIdx.x * kBlock + tid;
    if (c >= a.cols) return;
    double *__restrict__ xn = st.x[nxt];
    double *__restrict__ sn = st.strip[nxt];
    if (c >= 2 * a.N) {
        xn[3 + c] = 0.0;
        for (int r = 0; r < 3; ++r) sn[r * st.ldm + c] = 0.0;
        return;
    }
    const int64_t l = c >> 1;
    const int j = (int)(c & 1);
    const double *__restrict__ x = st.x[cur];
    if constexpr (kForm == 2) {
        double mk[2], Hr[2][3];
        extract_relative_xy(sm.xr, sm.s, sm.c, x[3 + 2 * l], x[3 + 2 * l + 1], mk, Hr);
        xn[3 + c] = mk[j];
        for (int r = 0; r < 3; ++r) sn[r * st.ldm + c] = 0.0;
    } else {
        double tp[2], g[2], sk[3][2], W[3][2];
        join_invert_xy(a.t, sm.s, sm.c, x[3 + 2 * l], x[3 + 2 * l + 1], tp, g);
        xn[3 + c] = tp[j];
        extract_strip_cols(st, cur, l, sk);
        for (int r = 0; r < 3; ++r) for (int q = 0; q < 2; ++q) {
            double acc = 0; for (int p = 0; p < 3; ++p) acc += sm.V[3 * r + p] * sk[p][q]; W[r][q] = acc; }
        const double rot[2][2] = { { sm.c, -sm.s }, { sm.s, sm.c } };
        const double Aj[3] = { j ? 0.0 : 1.0, j ? 1.0 : 0.0, g[j] };
        for (int r = 0; r < 3; ++r) {
            double acc = 0; for (int q = 0; q < 2; ++q) acc += W[r][q] * rot[j][q];
            if constexpr (kForm == 1) {
                double e = 0; for (int q = 0; q < 3; ++q) e += sm.FS[3 * r + q] * Aj[q];
                acc = acc + e;
            }
            sn[r * st.ldm + c] = acc;
        }
    }
    if (j == 0) {
        double own[3];
        transform_own_block<kForm>(st, a, sm, l, own);
        double *__restrict__ dg = st.diag[st.dcur ^ 1] + 3 * l;
        dg[0] = own[0]; dg[1] = own[1]; dg[2] = own[2];
    }
}

__device__ __forceinline__ void transform_unpack(const double2 &t, double *v) { v[0] = t.x; v[1] = t.y; }
__device__ __forceinline__ void transform_unpack(const float4 &t, double *v) { v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }

// The tiles, in place.  work: the tiles (I, J) of the active tile rows, `items_per_tile` work items each; grid = ntiles * items_per_tile.
// A work item is kBlock * kTransformUnits UNITS of one tile; a unit is two rows (one landmark's) times one 16-byte piece: one 2 x 2 block
// with F64 tiles, two with float tiles.  Consecutive lanes own consecutive pieces of a tile row, so with the production tile edges (128 for
// F64, 256 for float) one wave instruction loads or stores one whole 1 KiB tile row, and a lane stays on one column group for all its units:
// its column operands are formed once.  A block with a landmark at or beyond N keeps what it holds (zero).
//   off-diagonal tiles  a lane loads its units' two pieces, forms the blocks and stores the pieces where they came from
//   diagonal tiles      stored whole, block by block (8- or 16-byte accesses): the lane of a lower block loads it and writes it and its
//                       transposed mirror, the lane of a landmark's own block forms it from the diagonal copy, the lane of an upper block
//                       does nothing -- no lane reads an upper block, and the two halves agree bit for bit
constexpr int kTransformUnits = 2;
template <typename TS, int kForm>
__global__ __launch_bounds__(kBlock) void k_transform_tiles(DevState st, TransformMapArgs a, const int2 *__restrict__ work, int items_per_tile) {
    using VL = typename Lane16<TS>::type;
    constexpr int kCols = Lane16<TS>::kCols;              // columns per lane: 2 (one landmark) or 4 (two)
    constexpr int kLm = kCols / 2;
    constexpr int kColShift = kCols == 2 ? 1 : 2;
    __shared__ TransformSmall sm;
    const int tid = threadIdx.x;
    if (tid == 0) transform_small(st, a, /*state*/ false, sm);
    __syncthreads();
    const TileMap tm = st.tm;
    const int T = tm.T;
    const int lshift = tm.shift - kColShift;              // log2 of the 16-byte pieces of a tile row
    const int units = (T >> 1) << lshift;                 // ... and the units of a tile
    const int64_t w = blockIdx.x / (unsigned)items_per_tile;
    const int chunk = (int)(blockIdx.x - w * items_per_tile);
    const int2 ij = work[w];
    // kBlock is a multiple of the pieces of a row: a lane stays on one column group for all its units
    const int cl = tid & ((1 << lshift) - 1);
    const int64_t lcol = (((int64_t)ij.y * T) >> 1) + (cl << (kColShift - 1));       // the landmark of the lane's first column pair
    const int64_t lrow0 = ((int64_t)ij.x * T) >> 1;
    TS *__restrict__ tp = (TS *)st.tiles + tm.tile_offset(ij.x, ij.y);
    int br[kTransformUnits];
#pragma unroll
    for (int u = 0; u < kTransformUnits; ++u) {
        const int p = (chunk * kTransformUnits + u) * kBlock + tid;
        br[u] = p < units && lrow0 + (p >> lshift) < a.N ? p >> lshift : -1;      // the landmark row inside the tile; -1: nothing to do
    }
    if (lcol >= a.N) return;
    TransformOp<kForm> cop[kLm];
#pragma unroll
    for (int q = 0; q < kLm; ++q) transform_op<kForm>(st, a, sm, lcol + q < a.N ? lcol + q : lcol, cop[q]);
    if (ij.x != ij.y) {
        VL v[kTransformUnits][2];
#pragma unroll
        for (int u = 0; u < kTransformUnits; ++u)
            if (br[u] >= 0) {
                const TS *__restrict__ p = tp + ((int64_t)(2 * br[u]) << tm.shift) + kCols * cl;
                v[u][0] = *reinterpret_cast<const VL *>(p);
                v[u][1] = *reinterpret_cast<const VL *>(p + T);
            }
#pragma unroll
        for (int u = 0; u < kTransformUnits; ++u) {
            if (br[u] < 0) continue;
            TransformOp<kForm> rop;
            transform_op<kForm>(st, a, sm, lrow0 + br[u], rop);
            double r0[kCols], r1[kCols];
            transform_unpack(v[u][0], r0);
            transform_unpack(v[u][1], r1);
#pragma unroll
            for (int q = 0; q < kLm; ++q) {
                if (lcol + q >= a.N) continue;
                const double B[4] = { r0[2 * q], r0[2 * q + 1], r1[2 * q], r1[2 * q + 1] };
                double o[4];
                transform_block<kForm>(a, sm, rop, cop[q], B, o);
                r0[2 * q] = o[0]; r0[2 * q + 1] = o[1]; r1[2 * q] = o[2]; r1[2 * q + 1] = o[3];
            }
            VL w0, w1;
            lane16_pack(r0, w0);
            lane16_pack(r1, w1);
            TS *__restrict__ p = tp + ((int64_t)(2 * br[u]) << tm.shift) + kCols * cl;
            *reinterpret_cast<VL *>(p) = w0;
            *reinterpret_cast<VL *>(p + T) = w1;
        }
        return;
    }
    using V2 = typename Vec2<TS>::type;
#pragma unroll
    for (int u = 0; u < kTransformUnits; ++u) {
        if (br[u] < 0) continue;
        const int64_t lr = lrow0 + br[u];
#pragma unroll
        for (int q = 0; q < kLm; ++q) {
            const int64_t lc = lcol + q;
            if (lc > lr || lc >= a.N) continue;           // an upper block: its lower partner's lane writes it
            TS *__restrict__ p = tp + ((int64_t)(2 * br[u]) << tm.shift) + kCols * cl + 2 * q;
            V2 w0, w1;
            if (lc == lr) {
                double own[3];
                transform_own_block<kForm>(st, a, sm, lr, own);
                w0.x = (TS)own[0]; w0.y = (TS)own[1]; w1.x = (TS)own[1]; w1.y = (TS)own[2];
            } else {
                const V2 b0 = *reinterpret_cast<const V2 *>(p), b1 = *reinterpret_cast<const V2 *>(p + T);
                const double B[4] = { (double)b0.x, (double)b0.y, (double)b1.x, (double)b1.y };
                TransformOp<kForm> rop;
                transform_op<kForm>(st, a, sm, lr, rop);
                double o[4];
                transform_block<kForm>(a, sm, rop, cop[q], B, o);
                w0.x = (TS)o[0]; w0.y = (TS)o[1]; w1.x = (TS)o[2]; w1.y = (TS)o[3];
                // the mirror: rows of landmark lc, columns of landmark lr
                TS *__restrict__ m = tp + ((int64_t)(2 * (lc - lrow0)) << tm.shift) + 2 * br[u];
                V2 m0, m1;
                m0.x = w0.x; m0.y = w1.x; m1.x = w0.y; m1.y = w1.y;
                *reinterpret_cast<V2 *>(m) = m0;
                *reinterpret_cast<V2 *>(m + T) = m1;
            }
            *reinterpret_cast<V2 *>(p) = w0;
            *reinterpret_cast<V2 *>(p + T) = w1;
        }
    }
}
