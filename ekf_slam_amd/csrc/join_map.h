// Fragment of kernels.hip (included there, inside its anonymous namespace, after append_model.h): k_join_state and k_join_rows, a LOCAL map
// joined into the map on the device (ekf_join_map).
#pragma once

// ---------------------------------------------------------------------------------------------------
// Global state x = [r; l_1 .. l_N] with covariance P (`st`); local state y = [q; m_1 .. m_M] with covariance PL (`lo`), expressed in the frame
// of the global robot pose r = (p, theta) and independent of P.  With Rot = Rot(theta), w(v) = Rot v and k = 180 / pi:
//     r'  = r (+) q                     ekfm::motion_eval POSE_DELTA at (r, q):  F = J1 = I + [fa; fb] in the heading column, V = J2 = blockdiag(Rot, 1)
//     g_i = p + w(m_i)                  ekfm::model_invert RELATIVE_XY at (r, m_i):  Gx_i = [1 0 gth0; 0 1 gth1], Gz = Rot
// and P' = J blockdiag(P, PL) J', block by block (strip = P(1:3, landmarks)):
//     Prr'                = J1 Prr J1' + J2 PL_qq J2'                       predict_model_prr with M = PL_qq
//     strip'(old c)       = J1 strip(:, c)                                   predict_strip
//     strip'(new i)       = J1 (Prr Gx_i') + J2 PL(q, m_i) Rot'              append_model_strip, predict_strip, then the local term
//     P'(new i, old c)    = Gx_i strip(:, c)            the OLD strip        append_row_entry
//     P'(new i, new a)    = Gx_i (Prr Gx_a') + Rot PL(m_i, m_a) Rot'  a < i  append_row_entry on append_model_strip, then the local term
//     P'(new i, new i)    = Gx_i Prr Gx_i' + Rot PL(m_i, m_i) Rot'           append_model_own with append_model_noise(Rot, PL(m_i, m_i))
//     P'(old, old)        untouched: no tile below row 2 N is read or written
// Everywhere the global term is formed first and the local term added last, so a local map with q = 0, PL_qq = 0, PL(q, .) = 0 and a
// block-diagonal PL_mm leaves what k_append_model leaves for RELATIVE_XY entries (z = m_i, R = PL(m_i, m_i)) bit for bit, and M = 0 leaves
// what k_predict_model leaves for one POSE_DELTA step (u = q, M = PL_qq).
// k_join_state reads buffer cur of the global state and writes a COMPLETE buffer cur ^ 1 (x, Prr, strip) plus s and the live diagonal copies
// of the new landmarks; k_join_rows reads buffer cur too (the OLD pose, Prr and strip) and writes the new tile rows.  Neither reads a slot
// either writes, so the two launches and their workgroups need no order among themselves.  The local state is read only.
// ---------------------------------------------------------------------------------------------------

// RELATIVE_XY's t and dg/dtheta from the sine and cosine ekfm::model_invert took of the heading: its expressions, for a workgroup that has
// them already (model_invert at z = 0 leaves them in Gz)
__device__ __forceinline__ void join_invert_xy(const double xr[3], double s, double c, double z0, double z1, double t[2], double gth[2]) {
    const double w0 = c * z0 - s * z1, w1 = s * z0 + c * z1;
    t[0] = xr[0] + w0;
    t[1] = xr[1] + w1;
    gth[0] = -w1 / ekfm::kR2D;
    gth[1] = w0 / ekfm::kR2D;
}
// Gz B Gz' for a 2 x 2 block B that need not be symmetric, all four entries row-major: append_model_noise's two products, in its order
__device__ __forceinline__ void join_rotate_block(const double Gz[4], double B00, double B01, double B10, double B11, double o[4]) {
    const double jz[2][2] = { { Gz[0], Gz[1] }, { Gz[2], Gz[3] } };
    const double B[2][2] = { { B00, B01 }, { B10, B11 } };
    double t2[2][2];
    for (int i = 0; i < 2; ++i) for (int j = 0; j < 2; ++j) {
        double acc = 0; for (int k = 0; k < 2; ++k) acc += jz[i][k] * B[k][j]; t2[i][j] = acc; }
    for (int i = 0; i < 2; ++i) for (int j = 0; j < 2; ++j) {
        double acc = 0; for (int k = 0; k < 2; ++k) acc += t2[i][k] * jz[j][k]; o[2 * i + j] = acc; }
}

// what lane 0 of a workgroup leaves in LDS: the old pose and Prr, Rot as model_invert's Gz, and the robot's composition
struct JoinSmall {
    double xr[3], prr[9], Gz[4];
    double xn[3], fa, fb, V[9];     // k_join_state only
    double mi[2], gth[2];           // k_join_rows only: the row landmark's local position and its dg/dtheta
};
__device__ __forceinline__ void join_small_common(const DevState &st, int cur, JoinSmall &o) {
    for (int i = 0; i < 3; ++i) o.xr[i] = st.x[cur][i];
    for (int i = 0; i < 9; ++i) o.prr[i] = st.prr[cur][i];
    const double z0[2] = { 0.0, 0.0 };
    double t[2], gth[2];
    ekfm::model_invert(4, o.xr, z0, t, gth, o.Gz);
}

// One lane per column c < 2 (N + M), 256 per workgroup; the small part by EVERY workgroup on lane 0, Prr' and the pose by workgroup 0.
__global__ __launch_bounds__(kBlock) void k_join_state(DevState st, DevState lo, JoinMapArgs a) {
    __shared__ JoinSmall sm;
    const int tid = threadIdx.x;
    const int cur = a.cur, nxt = cur ^ 1, lcur = a.lcur;
    if (tid == 0) {
        join_small_common(st, cur, sm);
        const double q[3] = { lo.x[lcur][0], lo.x[lcur][1], lo.x[lcur][2] };
        ekfm::motion_eval_with(MotionSinCosNi(), 3, sm.xr, q, sm.xn, sm.fa, sm.fb, sm.V);
    }
    __syncthreads();
    const double *__restrict__ prr = sm.prr;
    if (blockIdx.x == 0 && tid == 0) {
        const double *__restrict__ lp = lo.prr[lcur];
        const double m6[6] = { lp[0], lp[3], lp[4], lp[6], lp[7], lp[8] };
        double pr2[9], Q[9];
        predict_model_prr(prr, sm.fa, sm.fb, sm.V, m6, pr2, Q);
        for (int i = 0; i < 9; ++i) st.prr[nxt][i] = pr2[i];
        for (int i = 0; i < 3; ++i) st.x[nxt][i] = sm.xn[i];
    }
    const int64_t n_mm = 2 * a.N;
    const int64_t c = (int64_t)blockIdx.x * kBlock + tid;
    if (c >= n_mm + 2 * a.M) return;
    const double *__restrict__ x = st.x[cur];
    double *__restrict__ xn = st.x[nxt];
    double *__restrict__ sn = st.strip[nxt];
    if (c < n_mm) {
        // an old column: J1 on the strip column, the landmark where it was
        const double *__restrict__ s = st.strip[cur];
        double s0 = s[c], s1 = s[st.ldm + c];
        const double s2 = s[2 * st.ldm + c];
        predict_strip(s0, s1, s2, sm.fa, sm.fb);
        sn[c] = s0; sn[st.ldm + c] = s1; sn[2 * st.ldm + c] = s2;
        xn[3 + c] = x[3 + c];
        return;
    }
    // column j of new landmark i: its position, J1 (Prr Gx_i') and then the local term J2 PL(q, m_i) Rot'
    const int64_t i = (c - n_mm) >> 1;
    const int j = (int)(c & 1);
    const double *__restrict__ lx = lo.x[lcur];
    double t[2], gth[2], v[3];
    join_invert_xy(sm.xr, sm.Gz[2], sm.Gz[0], lx[3 + 2 * i], lx[3 + 2 * i + 1], t, gth);
    xn[3 + c] = t[j];
    const double gx[3] = { j ? 0.0 : 1.0, j ? 1.0 : 0.0, gth[j] };
    append_model_strip(gx, prr, v);
    predict_strip(v[0], v[1], v[2], sm.fa, sm.fb);
    const double *__restrict__ ls = lo.strip[lcur];
    double u[3];
    for (int r = 0; r < 3; ++r) u[r] = ls[r * lo.ldm + 2 * i] * sm.Gz[2 * j] + ls[r * lo.ldm + 2 * i + 1] * sm.Gz[2 * j + 1];
    for (int r = 0; r < 3; ++r) {
        double acc = 0; for (int k = 0; k < 3; ++k) acc += sm.V[3 * r + k] * u[k];
        sn[r * st.ldm + c] = v[r] + acc;
    }
    if (j == 0) {
        st.s[a.N + i] = lo.s[i] + a.signature_offset;
        const double *__restrict__ ld = lo.diag[lo.dcur] + 3 * i;
        double jxr[2][3], gzr[3], cblk[3];
        append_model_jxr(gth[0], gth[1], jxr);
        append_model_noise(sm.Gz, ld[0], ld[1], ld[1], ld[2], gzr);
        append_model_own(jxr, prr, gzr, cblk);
        double *__restrict__ dg = st.diag[st.dcur] + 3 * (a.N + i);
        dg[0] = cblk[0]; dg[1] = cblk[1]; dg[2] = cblk[2];
    }
}

// two adjacent elements of one tile row, one 16- / 8-byte store (c even)
template <typename TS>
__device__ __forceinline__ void pmm_low_store_pair(TS *__restrict__ tiles, const TileMap &tm, int64_t r, int64_t c, double v0, double v1) {
    const int64_t I = r >> tm.shift, J = c >> tm.shift;
    const int64_t m = tm.T - 1;
    typename Vec2<TS>::type t;
    t.x = (TS)v0; t.y = (TS)v1;
    *reinterpret_cast<typename Vec2<TS>::type *>(tiles + tm.tile_offset(I, J) + ((r & m) << tm.shift) + (c & m)) = t;
}

// The new tile rows.  Workgroup b serves ONE new landmark i = b / blocks_per_row (rows 2 N + 2 i, + 1) and 256 consecutive column landmarks
// of it: a lane owns one 2 x 2 block, two rows times two adjacent columns, so a wavefront writes contiguous runs of a tile row.  Column
// landmarks above N + i lie in the upper triangle: those lanes leave.  The two stores are addressed through their own tile maps; 2 N and
// both tile edges are even, so no block straddles a tile edge on either side.
template <typename TSdst, typename TSsrc>
__global__ __launch_bounds__(kBlock) void k_join_rows(DevState st, DevState lo, JoinMapArgs a, int32_t blocks_per_row) {
    __shared__ JoinSmall sm;
    const int tid = threadIdx.x;
    const int cur = a.cur, lcur = a.lcur;
    const int64_t i = blockIdx.x / (uint32_t)blocks_per_row;
    const int64_t cl = (int64_t)(blockIdx.x - (uint32_t)i * (uint32_t)blocks_per_row) * kBlock + tid;      // the column landmark
    if (tid == 0) {
        join_small_common(st, cur, sm);
        sm.mi[0] = lo.x[lcur][3 + 2 * i]; sm.mi[1] = lo.x[lcur][3 + 2 * i + 1];
        double t[2];
        join_invert_xy(sm.xr, sm.Gz[2], sm.Gz[0], sm.mi[0], sm.mi[1], t, sm.gth);
    }
    __syncthreads();
    if (cl > a.N + i) return;
    const double *__restrict__ prr = sm.prr;
    TSdst *__restrict__ tiles = (TSdst *)st.tiles;
    const int64_t r0 = 2 * (a.N + i), c0 = 2 * cl;
    double jxr[2][3];
    append_model_jxr(sm.gth[0], sm.gth[1], jxr);
    if (cl < a.N) {
        // old columns: Gx_i on the OLD strip columns
        const double *__restrict__ s = st.strip[cur];
        const double2 s0 = *reinterpret_cast<const double2 *>(s + c0), s1 = *reinterpret_cast<const double2 *>(s + st.ldm + c0),
                      s2 = *reinterpret_cast<const double2 *>(s + 2 * st.ldm + c0);
        for (int ri = 0; ri < 2; ++ri)
            pmm_low_store_pair<TSdst>(tiles, st.tm, r0 + ri, c0, append_row_entry(jxr, ri, s0.x, s1.x, s2.x), append_row_entry(jxr, ri, s0.y, s1.y, s2.y));
        return;
    }
    const int64_t al = cl - a.N;                            // the local landmark of this column, al <= i
    if (al == i) {
        // the own block: from the live F64 diagonal copy of the local map, never the tile's copy of it
        const double *__restrict__ ld = lo.diag[lo.dcur] + 3 * i;
        double gzr[3], cblk[3];
        append_model_noise(sm.Gz, ld[0], ld[1], ld[1], ld[2], gzr);
        append_model_own(jxr, prr, gzr, cblk);
        double *__restrict__ dg = st.diag[st.dcur] + 3 * (a.N + i);
        dg[0] = cblk[0]; dg[1] = cblk[1]; dg[2] = cblk[2];
        pmm_low_store<TSdst>(tiles, st.tm, r0, c0, cblk[0]);
        pmm_low_store_pair<TSdst>(tiles, st.tm, r0 + 1, c0, cblk[1], cblk[2]);
        return;
    }
    // an earlier new landmark: Gx_i (Prr Gx_a'), then the local block rotated
    const double *__restrict__ lx = lo.x[lcur];
    double t[2], gtha[2], v0[3], v1[3], B[4], rot[4];
    join_invert_xy(sm.xr, sm.Gz[2], sm.Gz[0], lx[3 + 2 * al], lx[3 + 2 * al + 1], t, gtha);
    const double gx0[3] = { 1.0, 0.0, gtha[0] }, gx1[3] = { 0.0, 1.0, gtha[1] };
    append_model_strip(gx0, prr, v0);
    append_model_strip(gx1, prr, v1);
    pmm_low_pair<TSsrc>((const TSsrc *)lo.tiles, lo.tm, 2 * i, 2 * al, B[0], B[1]);
    pmm_low_pair<TSsrc>((const TSsrc *)lo.tiles, lo.tm, 2 * i + 1, 2 * al, B[2], B[3]);
    join_rotate_block(sm.Gz, B[0], B[1], B[2], B[3], rot);
    for (int ri = 0; ri < 2; ++ri)
        pmm_low_store_pair<TSdst>(tiles, st.tm, r0 + ri, c0, append_row_entry(jxr, ri, v0[0], v0[1], v0[2]) + rot[2 * ri],
                                  append_row_entry(jxr, ri, v1[0], v1[1], v1[2]) + rot[2 * ri + 1]);
}
