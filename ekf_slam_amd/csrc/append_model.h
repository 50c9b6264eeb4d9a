// Fragment of kernels.hip (included there, inside its anonymous namespace, after append.h): k_append_model, the append of a whole scan of
// landmarks that start from a range-and-bearing or a relative-position fix (ekf_append_model).
#pragma once

// ---------------------------------------------------------------------------------------------------
// "landmark N + b was seen as z_b through model_b, with noise covariance R_b", b = 0 .. m-1, all at the live robot state:
//     t_b = g(x_r, z_b)      Gx_b = dg/dx_r = [1 0 gth0; 0 1 gth1]      Gz_b = dg/dz      (ekfm::model_invert)
//     P(new_b, old)   = Gx_b P(1:3, old)                 the strip column, as k_append's row entry
//     P(new_b, new_a) = Gx_b Prr Gx_a'    (a < b)        the same expression on v = Prr Gx_a', what a's strip columns become
//     P(new_b, new_b) = Gx_b Prr Gx_b' + Gz_b R_b Gz_b'  append_blocks' summation order, lower triangle canonical
//     P(1:3, new_b)   = Prr Gx_b'
// in place on buffer `cur`, only new slots written -- k_append's rules without its predict.  The landmarks of one scan depend on each other
// through the robot state alone, so the cross blocks have that closed form and ONE launch appends all m: a batch writes bit for bit what
// m launches of one entry write, because the strip columns a later launch would read back are Prr Gx_a' formed by this same expression.
// No lane reads a slot this launch writes (x_r, Prr and the strip below 2N are read; x, the strip, s, the diagonal copies and the tiles are
// written from 2N on), so the workgroups need no order among themselves.
// ---------------------------------------------------------------------------------------------------

// Gx of an entry from its dg/dtheta: append_jxr's shape
__device__ __forceinline__ void append_model_jxr(double gth0, double gth1, double jxr[2][3]) {
    jxr[0][0] = 1; jxr[0][1] = 0; jxr[0][2] = gth0;
    jxr[1][0] = 0; jxr[1][1] = 1; jxr[1][2] = gth1;
}
// column i of Prr Gx' = what the strip holds at the new landmark's column i: append_blocks' iblk, one column
// (gx: row i of Gx)
__device__ __forceinline__ void append_model_strip(const double gx[3], const double *prr, double v[3]) {
    for (int r = 0; r < 3; ++r) {
        double acc = 0; for (int k = 0; k < 3; ++k) acc += prr[3 * r + k] * gx[k];
        v[r] = acc; }
}
// gzr = Gz R Gz' as ((0,0), (1,0), (1,1)): append_blocks' c2 with jz = Gz (row-major)
__device__ __forceinline__ void append_model_noise(const double Gz[4], double R00, double R01, double R10, double R11, double gzr[3]) {
    const double jz[2][2] = { { Gz[0], Gz[1] }, { Gz[2], Gz[3] } };
    const double R[2][2] = { { R00, R01 }, { R10, R11 } };
    double t2[2][2], c2[2][2];
    for (int i = 0; i < 2; ++i) for (int j = 0; j < 2; ++j) {
        double acc = 0; for (int k = 0; k < 2; ++k) acc += jz[i][k] * R[k][j]; t2[i][j] = acc; }
    for (int i = 0; i < 2; ++i) for (int j = 0; j < 2; ++j) {
        double acc = 0; for (int k = 0; k < 2; ++k) acc += t2[i][k] * jz[j][k]; c2[i][j] = acc; }
    gzr[0] = c2[0][0]; gzr[1] = c2[1][0]; gzr[2] = c2[1][1];
}
// the own block C = Gx Prr Gx' + gzr (lower triangle): append_blocks' c1, then its sum
__device__ __forceinline__ void append_model_own(const double jxr[2][3], const double *prr, const double gzr[3], double cblk[3]) {
    double t[2][3], c1[2][2];
    for (int i = 0; i < 2; ++i) for (int j = 0; j < 3; ++j) {
        double acc = 0; for (int k = 0; k < 3; ++k) acc += jxr[i][k] * prr[3 * k + j]; t[i][j] = acc; }
    for (int i = 0; i < 2; ++i) for (int j = 0; j < 2; ++j) {
        double acc = 0; for (int k = 0; k < 3; ++k) acc += t[i][k] * jxr[j][k]; c1[i][j] = acc; }
    cblk[0] = c1[0][0] + gzr[0]; cblk[1] = c1[1][0] + gzr[1]; cblk[2] = c1[1][1] + gzr[2];
}

// what lane b of every workgroup leaves in LDS for entry b: t, dg/dtheta, Gz R Gz'
struct AppendModelSmall {
    double t[2], gth[2], gzr[3], pad;
};

// One lane per column of the NEW landmark block (c < 2 (N + m)), 256 per workgroup; the small part by EVERY workgroup, on its first m lanes.
template <typename TS>
__global__ __launch_bounds__(kBlock) void k_append_model(DevState st, AppendModelArgs a) {
    __shared__ AppendModelSmall sm[kAppendModelMax];
    const int tid = threadIdx.x;
    const int cur = a.cur;
    const double *__restrict__ xin = st.x[cur];
    const double *__restrict__ prr = st.prr[cur];
    if (tid < a.m) {
        const AppendModelEntry &e = a.e[tid];
        const double xr[3] = { xin[0], xin[1], xin[2] };
        const double z[2] = { e.z0, e.z1 };
        double t[2] = { 0.0, 0.0 }, gth[2] = { 0.0, 0.0 }, Gz[4] = { 0.0, 0.0, 0.0, 0.0 }, gzr[3];
        ekfm::model_invert(e.model, xr, z, t, gth, Gz);
        append_model_noise(Gz, e.R00, e.R01, e.R10, e.R11, gzr);
        AppendModelSmall &o = sm[tid];
        o.t[0] = t[0]; o.t[1] = t[1]; o.gth[0] = gth[0]; o.gth[1] = gth[1];
        o.gzr[0] = gzr[0]; o.gzr[1] = gzr[1]; o.gzr[2] = gzr[2];
    }
    __syncthreads();
    double *__restrict__ x = st.x[cur];
    double *__restrict__ s = st.strip[cur];
    TS *__restrict__ tiles = (TS *)st.tiles;
    const int64_t n_mm = 2 * a.N;                           // old landmark-block size; entry b's rows are n_mm + 2 b, n_mm + 2 b + 1
    const int64_t c = (int64_t)blockIdx.x * kBlock + tid;
    if (c >= n_mm + 2 * a.m) return;
    double jxr[2][3], v[3];
    int b0 = 0;                                             // the first entry whose rows lie below this column's own landmark
    if (c < n_mm) {
        // an old column: v is the live strip column, P(new_b, c) for every b
        v[0] = s[c]; v[1] = s[st.ldm + c]; v[2] = s[2 * st.ldm + c];
    } else {
        // a column of new landmark own: v = Prr Gx_own', formed from Prr -- never from the strip slots this launch writes
        const int own = (int)((c - n_mm) >> 1), i = (int)(c & 1);
        const double gx[3] = { i ? 0.0 : 1.0, i ? 1.0 : 0.0, sm[own].gth[i] };
        append_model_strip(gx, prr, v);
        s[c] = v[0]; s[st.ldm + c] = v[1]; s[2 * st.ldm + c] = v[2];
        x[3 + c] = sm[own].t[i];
        if (i == 0) {
            double cblk[3];
            append_model_jxr(sm[own].gth[0], sm[own].gth[1], jxr);
            append_model_own(jxr, prr, sm[own].gzr, cblk);
            st.s[a.N + own] = a.e[own].signature;
            double *__restrict__ dg = st.diag[st.dcur] + 3 * (a.N + own);      // the live F64 copy of the own block (every shard)
            dg[0] = cblk[0]; dg[1] = cblk[1]; dg[2] = cblk[2];
            if (st.tm.mine(c >> st.tm.shift, c >> st.tm.shift)) {
                pmm_low_store<TS>(tiles, st.tm, c, c, cblk[0]);
                pmm_low_store<TS>(tiles, st.tm, c + 1, c, cblk[1]);
                pmm_low_store<TS>(tiles, st.tm, c + 1, c + 1, cblk[2]);
            }
        }
        b0 = own + 1;
    }
    for (int b = b0; b < a.m; ++b) {
        append_model_jxr(sm[b].gth[0], sm[b].gth[1], jxr);
        const int64_t r0 = n_mm + 2 * b;
        for (int i = 0; i < 2; ++i) {
            const double val = append_row_entry(jxr, i, v[0], v[1], v[2]);
            if (st.tm.mine((r0 + i) >> st.tm.shift, c >> st.tm.shift))
                pmm_low_store<TS>(tiles, st.tm, r0 + i, c, val);
        }
    }
}
