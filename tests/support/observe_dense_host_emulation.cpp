// Host emulation of the dense observation's kernels (tests/test_observe_dense_cpu.py compiles and runs it; no GPU, no HIP runtime).
// The kernel SOURCES of ekf_slam_amd/csrc/dense_obs.h (and what they call: pair_column.h, tile_access.h, device_math.h) are compiled for
// the host behind kernel_host_shim.h.  k_dense_gram runs its 256 lanes one after another, every workgroup twice (the first pass fills
// the shared storage, the second is the launch); k_dense_factor runs with ONE lane (EKF_DENSE_LANES: every phase is a loop strided by
// the lane count); k_gather_dense runs every workgroup three times as observe_joint_host_emulation.cpp runs k_gather_joint; the pass is
// the plain pair loop, rank2_apply in slot order over every stored entry.
// G = P H' is formed HERE, by the plain product over the dense P of the store, in the chunk layout of multiply_map.h (column i at i * ld,
// the landmark rows first, the robot's three at `rows`, rows 2 N .. rows - 1 left NaN: nothing may read them) -- not by the multiply
// emulation, whose matrix-instruction twin is multiply_map_host_emulation.cpp's own business.
// Per case it checks here: that a gated and an irregular case leave every buffer as it was, that the pairs are zero over the padded
// tail, that the live diagonal blocks are the tiles' own bits.  And it writes to argv[1], as doubles, what the test compares with the
// NumPy restatement:  n  k  outcome  bad_row  H (k x n)  z (k)  R (k x k)  x0 (n)  P0 (n x n)  x1  P1  d2  nu (k)  S (k x k)
#define EKF_DENSE_LANES 1
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "kernel_host_shim.h"
#include "emulated_state.h"
#include "dense_obs.h"

static void dense(Store<> &S, std::vector<double> &x, std::vector<double> &P) {
    const int n = 3 + 2 * S.N;
    x.assign(S.x[S.cur].begin(), S.x[S.cur].begin() + n);
    P.assign((size_t)n * n, 0.0);
    for (int r = 0; r < n; ++r) for (int c = 0; c <= r; ++c) {
        double v;
        if (r < 3) v = S.prr[S.cur][3 * r + c];
        else if (c < 3) v = S.strip[S.cur][c * S.ldm + (r - 3)];
        else v = S.live(r - 3, c - 3, 0);
        P[(size_t)r * n + c] = P[(size_t)c * n + r] = v;
    }
}

// what: 0 dense rows, 1 two identical unit rows on state entry 3 + 2 * 5 with R = 0 (S singular), 2 rows on the robot alone
static int run_case(FILE *f, const char *name, int N, int seed, int k, int what, double gate) {
    const int T = 16, cap = 300;
    Store<> S(T, N, cap, 32);
    fill(S, seed, true);
    const int n = 3 + 2 * N, n2 = 2 * N, rows = (int)S.tm.padded(n2), ld = rows + 4, kk = (k + 1) & ~1;
    std::vector<double> x0, P0, x1, P1, H((size_t)k * n, 0.0), z(k), R((size_t)k * k, 0.0);
    dense(S, x0, P0);
    for (int i = 0; i < k; ++i) {
        if (what == 1) H[(size_t)i * n + 3 + 2 * 5] = 1.0;
        else for (int c = 0; c < (what == 2 ? 3 : n); ++c) H[(size_t)i * n + c] = rnd();
        double hx = 0.0;
        for (int c = 0; c < n; ++c) hx += H[(size_t)i * n + c] * x0[c];
        z[i] = hx + 0.3 * rnd();
        R[(size_t)i * k + i] = what == 1 ? 0.0 : 0.05 + 0.02 * i;
    }
    if (what == 0 && k > 1) R[1] = R[k] = 0.01;
    // the chunk: H's rows in, G = P H' out, NaN where nothing may be read
    std::vector<double> b((size_t)kDenseMax * ld, 0.0), g((size_t)kDenseMax * ld, NAN);
    for (int i = 0; i < kDenseMax; ++i)
        for (int r = 0; r < n; ++r) {
            double acc = 0.0;
            if (i < k) {
                for (int c = 0; c < n; ++c) acc += P0[(size_t)r * n + c] * H[(size_t)i * n + c];
                b[(size_t)i * ld + (r < 3 ? rows + r : r - 3)] = H[(size_t)i * n + r];
            }
            g[(size_t)i * ld + (r < 3 ? rows + r : r - 3)] = acc;
        }
    const int nseg = (n2 + kDenseSegment - 1) / kDenseSegment;
    std::vector<double> part((size_t)(nseg ? nseg : 1) * kDensePartial, NAN);
    DenseArgs a = DenseArgs();
    a.b = b.data(); a.y = g.data(); a.part = part.data(); a.ld = ld; a.rows = rows; a.n_mm = n2; a.kk = kk; a.cur = S.cur;
    DenseSmall sm = DenseSmall();
    for (int i = 0; i < k; ++i) { sm.z[i] = z[i]; for (int j = 0; j < k; ++j) sm.R[i * kDenseMax + j] = R[(size_t)i * k + j]; }
    if (kk > k) sm.R[k * kDenseMax + k] = 1.0;
    const Store<> before = S;
    DevState st = S.st;
    static DenseBlock blk;
    static DenseOut out;
    launch_wg(nseg, { 2, -1 }, [&] { k_dense_gram(st, a); });
    blockIdx.x = 0; threadIdx.x = 0;
    k_dense_factor(st, a, sm, &out, &blk);
    int bad = 0;
    const int outcome = out.rec.outcome != 1 ? 0 : (!(out.rec.d2 <= gate) ? 2 : 1);
    if (outcome == 1) {
        const int grid = rows > 0 ? (rows + kBlock - 1) / kBlock : 1;
        if (kk <= 4) launch_wg(grid, { 3, 2 }, [&] { k_gather_dense<2>(st, a, &blk); });
        else launch_wg(grid, { 3, 2 }, [&] { k_gather_dense<8>(st, a, &blk); });
        S.flip();
        for (int p = 0; p < kk / 2; ++p) {
            const double2 *G2 = (const double2 *)(S.st.Gp + (size_t)p * S.st.pair_stride), *K2 = (const double2 *)(S.st.Kp + (size_t)p * S.st.pair_stride);
            for (int r = 0; r < n2; ++r) for (int c = 0; c < n2; ++c) {
                if (c > r && (r / T) != (c / T)) continue;
                S.tile(r, c) = rank2_apply(S.tile(r, c), K2[r], G2[c]);
            }
            for (int c = n2; c < rows; ++c)
                if (G2[c].x != 0.0 || G2[c].y != 0.0 || K2[c].x != 0.0 || K2[c].y != 0.0) { printf("  pair %d is not zero at padded column %d\n", p, c); ++bad; }
        }
        for (int q = 0; q < N; ++q) {
            const double t3[3] = { S.tile(2 * q, 2 * q), S.tile(2 * q + 1, 2 * q), S.tile(2 * q + 1, 2 * q + 1) };
            if (memcmp(t3, &S.diag[S.dcur][3 * q], 24)) { printf("  landmark %d: the live diagonal block differs from the tile's\n", q); ++bad; }
        }
    } else {
        bad += differ(S.x[0], before.x[0], "x") + differ(S.x[1], before.x[1], "x (other buffer)") + differ(S.strip[0], before.strip[0], "strip") +
               differ(S.strip[1], before.strip[1], "strip (other buffer)") + differ(S.prr[0], before.prr[0], "prr") + differ(S.prr[1], before.prr[1], "prr (other)") +
               differ(S.diag[0], before.diag[0], "diag") + differ(S.diag[1], before.diag[1], "diag (other buffer)") + differ(S.tiles, before.tiles, "tiles") +
               differ(S.ring, before.ring, "ring");
    }
    dense(S, x1, P1);
    const double head[4] = { (double)n, (double)k, (double)outcome, (double)out.rec.bad_row };
    put(f, head, 4);
    put(f, H.data(), H.size()); put(f, z.data(), z.size()); put(f, R.data(), R.size());
    put(f, x0.data(), x0.size()); put(f, P0.data(), P0.size()); put(f, x1.data(), x1.size()); put(f, P1.data(), P1.size());
    put(f, &out.rec.d2, 1);
    put(f, out.nu, k);
    for (int i = 0; i < k; ++i) put(f, out.S + i * kDenseMax, k);
    printf("%s: N = %d, k = %d, outcome %d, bad row %d, d2 = %.6g: %d differences\n", name, N, k, outcome, out.rec.bad_row, out.rec.d2, bad);
    return bad;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "wb");
    if (!f) return 2;
    int bad = 0;
    // N = 40 fills its five tile rows of edge 16 exactly, N = 41 leaves 14 padded columns; N = 140 has three segments of 128 rows and two
    // column workgroups; N = 0 is the robot part alone
    bad += run_case(f, "a scalar row", 40, 3, 1, 0, INFINITY);
    bad += run_case(f, "one full pair", 41, 4, 2, 0, INFINITY);
    bad += run_case(f, "odd, two pairs, a padded tail", 41, 5, 3, 0, INFINITY);
    bad += run_case(f, "the full chunk, three segments", 140, 6, 16, 0, INFINITY);
    bad += run_case(f, "five rows, three segments", 140, 7, 5, 0, INFINITY);
    bad += run_case(f, "no landmark", 0, 8, 3, 2, INFINITY);
    bad += run_case(f, "gated", 41, 4, 2, 0, 0.0);
    bad += run_case(f, "irregular: the same entry twice, R = 0", 41, 9, 2, 1, INFINITY);
    fclose(f);
    return bad != 0;
}
