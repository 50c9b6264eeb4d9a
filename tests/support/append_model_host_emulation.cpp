// Host emulation of k_append_model (tests/test_append_model_cpu.py compiles and runs it; no GPU, no HIP runtime).
// The kernel SOURCES of ekf_slam_amd/csrc (tile_access.h, append.h, append_model.h, and pair_column.h / constrain.h / linear_obs.h for the
// pairs that are left pending) are compiled for the host behind kernel_host_shim.h -- thread indices as globals,
// __shared__ as static storage, every workgroup run again until what its first lanes leave in the shared storage is there.  For tiles of
// edge 16 and 64, double and float tiles, 0 and 3 pairs pending in the ring, and m = 1, 3, 9 entries from 123 landmarks (the columns of
// landmark 128 start k_append_model's second workgroup and, at T = 16, a tile row):
//   the batch:   one launch with m entries
//   the singles: m launches of one entry each
// must leave the tiles, the strip, x, s, both diagonal copies and the pair ring BIT FOR BIT the same, and everything below the old map
// untouched.  Each case's live state before (the pending pairs applied to what the tiles hold) and its new rows after are written to
// argv[1] for the dense restatement of tests/append_model_cases.py.
// What append.h's k_append names besides the argument blocks is declared and never defined -- the template is not instantiated here.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "kernel_host_shim.h"
// what k_append (append.h) names: declared, never defined
struct PredictSmall { double fa, fb; double pose[3]; double prr[9]; double Q[9]; };
void predict_small(const double pose[3], const double prr_in[9], double u0, double u1, double C, PredictSmall &o);
void predict_strip(double &s0, double &s1, double s2, double fa, double fb);
void reduce_partials_wave(const AssocHostPartial *parts, int nblk, int seq, int lane, double &ll, int &ix);
void store_partial(AssocHostPartial *dst, double ll, int index, int seq);
#include "emulated_state.h"
#include "append.h"
#include "append_model.h"

// k_append_model: every workgroup twice -- the first run leaves t, dg/dtheta and Gz R Gz' of every entry in the shared storage, the second
// one is the launch (it rewrites every slot the first one wrote; no lane reads a slot the launch writes); no lane exchange
template <typename TS> static void run_append(Store<TS> &S, const AppendModelEntry *e, int m) {
    AppendModelArgs a = {};
    a.N = S.N; a.m = m; a.cur = S.cur;
    for (int b = 0; b < m; ++b) a.e[b] = e[b];
    DevState st = S.st;
    launch_wg((2 * (S.N + m) + kBlock - 1) / kBlock, { 2, -1 }, [&] { k_append_model<TS>(st, a); });
    S.N += m;
}

template <typename TS> static int run_cases(const char *ts, const std::string &dir) {
    int total_bad = 0;
    for (int T : { 16, 64 }) for (int pending : { 0, 3 }) {
        const int N = 123, cap = 136;
        Store<TS> base(T, N, cap);
        fill(base, 11, true);
        int64_t cnt0[2] = { 0, 0 };
        double rec0[8];
        for (int k = 0; k < pending; ++k) {                   // some pairs pending in the ring (never applied to the tiles)
            LinearArgs a = {};
            for (int q = 0; q < 14; ++q) a.H[q] = 0.4 * rnd();
            a.a[0] = 2 * (5 + 40 * k); a.a[1] = 2 * (N - 1 - k);
            const double R[4] = { 0.3, 0.05, 0.05, 0.2 };
            memcpy(a.R, R, sizeof R);
            const double *x = base.x[base.cur].data();
            for (int r = 0; r < 2; ++r) {
                double hx = 0;
                for (int i = 0; i < 3; ++i) hx += a.H[7 * r + i] * x[i];
                for (int b = 0; b < 2; ++b) for (int c = 0; c < 2; ++c) hx += a.H[7 * r + 3 + 2 * b + c] * x[3 + a.a[b] + c];
                a.z[r] = hx + 0.2 * rnd();
            }
            a.gate = INFINITY; a.npend = k;
            run_linear(base, a, rec0, cnt0);
            if (rec0[7] != 1.0) { printf("a pending pair did not apply\n"); return 1000; }
        }
        // the live state before, for the dense restatement: n, x, s, P (row-major, both triangles)
        const int n0 = 3 + 2 * N;
        {
            std::vector<double> P((size_t)n0 * n0);
            for (int r = 0; r < n0; ++r) for (int c = 0; c <= r; ++c) {
                double v;
                if (r < 3) v = base.prr[base.cur][3 * r + c];
                else if (c < 3) v = base.strip[base.cur][c * base.ldm + (r - 3)];
                else v = base.live(r - 3, c - 3, pending);
                P[(size_t)r * n0 + c] = P[(size_t)c * n0 + r] = v;
            }
            FILE *f = fopen((dir + "/before_" + ts + "_" + std::to_string(T) + "_" + std::to_string(pending) + ".bin").c_str(), "wb");
            if (!f) return 1000;
            const double hdr[1] = { (double)n0 };
            fwrite(hdr, 8, 1, f);
            put(f, base.x[base.cur].data(), n0);
            put(f, base.s.data(), N);
            put(f, P.data(), P.size());
            fclose(f);
        }
        for (int m : { 1, 3, 9 }) {
            AppendModelEntry e[kAppendModelMax] = {};
            for (int b = 0; b < m; ++b) {
                e[b].model = (b + m) % 2 ? 1 : 4;
                e[b].z0 = e[b].model == 1 ? 2.0 + 11.0 * (rnd() + 1) : 15 * rnd();
                e[b].z1 = e[b].model == 1 ? 360.0 * rnd() : 15 * rnd();
                const double sc = e[b].model == 1 ? 30.0 : 1.0;
                e[b].R00 = 0.02 * (1 + 0.1 * b); e[b].R01 = e[b].R10 = 0.004 * std::sqrt(sc); e[b].R11 = 0.03 * sc;
                e[b].signature = 5000.0 + 10 * m + b;
            }
            Store<TS> A(base), B(base);
            A.sync(); B.sync();
            run_append(A, e, m);
            for (int b = 0; b < m; ++b) run_append(B, e + b, 1);
            int bad = 0;
            bad += differ(A.tiles, B.tiles, "tiles") + differ(A.s, B.s, "s") + differ(A.ring, B.ring, "pair ring") + differ(A.ring, base.ring, "pair ring against before");
            for (int q = 0; q < 2; ++q)
                bad += differ(A.x[q], B.x[q], "x") + differ(A.strip[q], B.strip[q], "strip") + differ(A.diag[q], B.diag[q], "diag") + differ(A.prr[q], B.prr[q], "prr");
            // nothing below the old map moved, and the buffers the launch does not own were not touched
            bad += differ(A.prr[A.cur], base.prr[base.cur], "prr against before") + differ(A.x[A.cur ^ 1], base.x[base.cur ^ 1], "the other x") +
                   differ(A.strip[A.cur ^ 1], base.strip[base.cur ^ 1], "the other strip") + differ(A.diag[A.dcur ^ 1], base.diag[base.dcur ^ 1], "the other diag");
            for (int i = 0; i < n0; ++i) if (A.x[A.cur][i] != base.x[base.cur][i]) ++bad;
            for (int r = 0; r < 3; ++r) for (int c = 0; c < 2 * N; ++c) if (A.strip[A.cur][r * A.ldm + c] != base.strip[base.cur][r * base.ldm + c]) ++bad;
            for (int k = 0; k < 3 * N; ++k) if (A.diag[A.dcur][k] != base.diag[base.dcur][k]) ++bad;
            for (int r = 0; r < 2 * N; ++r) for (int c = 0; c <= r; ++c) if (memcmp(&A.tile(r, c), &base.tile(r, c), sizeof(TS))) ++bad;
            if (A.N != N + m) ++bad;
            // the new part after: the entries, then x, s and the rows of P from 3 + 2 N on
            const int n1 = 3 + 2 * (N + m);
            std::vector<double> rows((size_t)2 * m * n1), ent;
            for (int b = 0; b < m; ++b) for (double v : { (double)e[b].model, e[b].z0, e[b].z1, e[b].R00, e[b].R01, e[b].R10, e[b].R11, e[b].signature }) ent.push_back(v);
            for (int r = n0; r < n1; ++r) for (int c = 0; c < n1; ++c) {
                const int hi = r > c ? r : c, lo = r > c ? c : r;
                rows[(size_t)(r - n0) * n1 + c] = lo < 3 ? A.strip[A.cur][lo * A.ldm + (hi - 3)] : A.live(hi - 3, lo - 3, pending);
            }
            FILE *f = fopen((dir + "/after_" + ts + "_" + std::to_string(T) + "_" + std::to_string(pending) + "_" + std::to_string(m) + ".bin").c_str(), "wb");
            if (!f) return 1000;
            put(f, ent.data(), ent.size());
            put(f, A.x[A.cur].data() + n0, n1 - n0);
            put(f, A.s.data() + N, m);
            put(f, rows.data(), rows.size());
            fclose(f);
            printf("%s T=%d pending=%d m=%d: %d differences\n", ts, T, pending, m, bad);
            total_bad += bad;
        }
    }
    return total_bad;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const int bad = run_cases<double>("double", argv[1]) + run_cases<float>("float", argv[1]);
    return bad != 0;
}
