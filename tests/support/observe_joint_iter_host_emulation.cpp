// Host emulation of the relinearised joint update's kernels (tests/test_observe_joint_iter_cpu.py compiles and runs it, once more under
// the address and undefined-behaviour sanitizers; no GPU, no HIP runtime).  The kernel SOURCES of ekf_slam_amd/csrc (joint.h,
// joint_update.h, joint_iter.h and what they call) are compiled for the host behind kernel_host_shim.h.  k_joint_factor_iter and
// k_joint_factor run with ONE lane (EKF_JOINT_LANES: every phase is a loop strided by the lane count); k_gather_joint and the pass's pair
// loop run as in observe_joint_host_emulation.cpp.  The scans sit well beside h(x) on a prior widened over the robot and the paired
// landmarks, so the iterates move.
// Per case it checks here, bit for bit: with iterations == 1 the JointBlock against k_joint_factor's; the first record, nu and S against
// k_joint_factor's whatever iterations is; that a gated and an irregular-later case leave every buffer as it was.  And it writes to
// argv[1], as doubles, what the test compares with the NumPy restatement:
//   n  m  outcome  iterations  (model z0 z1 R00 R01 R10 R11 landmark) x m  x0 (n)  P0 (n x n)  x1  P1  d2  used  converged  irregular_at
#define EKF_JOINT_LANES 1
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "kernel_host_shim.h"
#include "emulated_state.h"
#include "joint.h"
#include "joint_update.h"
#include "joint_iter.h"

struct Obs { int model; double z[2]; double R[4]; int lm; };        // R as the caller gives it: a one-row model's variance in R[0]

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

// an observation of landmark lm through `model`, a little beside h(x)
static Obs sight(Store<> &S, int model, int lm) {
    Obs o; o.model = model; o.lm = lm;
    const double *x = S.x[S.cur].data();
    const double xs[7] = { x[0], x[1], x[2], x[3 + 2 * lm], x[4 + 2 * lm], 0, 0 }, anchor[2] = { 0, 0 };
    double hx[2], H[14];
    ekfm::model_eval(model, xs, anchor, true, hx, H);
    const bool two = model == 1 || model == 4;
    o.z[0] = hx[0] + (model == 3 ? 3.0 : 0.4) * rnd(); o.z[1] = two ? hx[1] + (model == 1 ? 3.0 : 0.4) * rnd() : 0.0;
    if (two) { o.R[0] = 0.02; o.R[1] = o.R[2] = 0.005; o.R[3] = model == 1 ? 0.5 : 0.03; }
    else { o.R[0] = model == 2 ? 0.05 : 0.3; o.R[1] = o.R[2] = o.R[3] = 0.0; }
    return o;
}

// N = 40 fills its five tile rows of edge 16 exactly; N = 41 leaves landmark N - 1 alone in an edge-padded tile row with 14 padded columns
static int run_case(FILE *f, const char *name, int N, int seed, const std::vector<std::pair<int, int>> &scan, double gate, int iterations,
                    bool far_range) {
    const int T = 16, cap = 44, m = (int)scan.size();
    Store<> S(T, N, cap, 32);
    fill(S, seed, true);
    // a wide prior where the scan looks: the heading and the paired landmarks' own blocks
    S.prr[0][8] += 25.0;
    for (auto &e : scan)
        if (e.second >= 0) {
            S.diag[0][3 * e.second] += 1.0; S.diag[0][3 * e.second + 2] += 1.0;
            S.tile(2 * e.second, 2 * e.second) += 1.0; S.tile(2 * e.second + 1, 2 * e.second + 1) += 1.0;
        }
    std::vector<Obs> obs;
    for (auto &e : scan) obs.push_back(sight(S, e.first, e.second < 0 ? 0 : e.second));
    if (far_range) obs[0].z[0] = 1e200;            // (a range-bearing entry: xi_1 lies where q = |d|^2 overflows)
    JointArgs a = JointArgs();
    a.N = N; a.m = m; a.cur = S.cur; a.npend = 0; a.pstart = 0;
    std::vector<int64_t> hyp(m);
    int np = 0;
    for (int k = 0; k < m; ++k) {
        const Obs &o = obs[k];
        const bool two = o.model == 1 || o.model == 4;
        a.e[k].model = o.model; a.e[k].z[0] = o.z[0]; a.e[k].z[1] = o.z[1]; a.e[k].gate = INFINITY;
        a.e[k].R[0] = o.R[0]; a.e[k].R[1] = two ? o.R[1] : 0.0; a.e[k].R[2] = two ? o.R[2] : 0.0; a.e[k].R[3] = two ? o.R[3] : 1.0;
        hyp[k] = scan[k].second;
        np += hyp[k] >= 0;
    }
    std::vector<double> x0, P0, x1, P1;
    dense(S, x0, P0);
    const Store<> before = S;

    // the relinearised factor launch, and k_joint_factor on the same state: the first record, nu and S must be the same bits, and with one
    // linearisation the whole block
    static JointBlock blk, blk_1;
    memset(&blk, 0, sizeof blk); memset(&blk_1, 0, sizeof blk_1);
    JointRecord rec, rec_i;
    std::vector<double> nu(2 * m), Sm(4 * m * m), nu_i(2 * m), Sm_i(4 * m * m), itrec(kJointIterRecordDoubles);
    DevState st = S.st;
    JointIterArgs ia = JointIterArgs();
    ia.gate = gate; ia.tol = 0.0; ia.iterations = iterations;
    blockIdx.x = 0; threadIdx.x = 0;
    k_joint_factor_iter<double>(st, a, ia, hyp.data(), &blk, &rec, itrec.data(), nu.data(), Sm.data());
    k_joint_factor<double>(st, a, hyp.data(), &blk_1, &rec_i, nu_i.data(), Sm_i.data());
    int bad = memcmp(&rec, &rec_i, sizeof rec) != 0;
    bad += differ(nu, nu_i, "nu against k_joint_factor") + differ(Sm, Sm_i, "S against k_joint_factor");
    if (iterations == 1 && memcmp(&blk, &blk_1, sizeof blk)) { printf("  one linearisation: the block is not k_joint_factor's\n"); ++bad; }
    const int used = (int)itrec[0], irr_at = (int)itrec[4];
    if (iterations == 1 && rec.outcome == 1 && rec.d2 <= gate && used != 1) { printf("  one linearisation: used = %d\n", used); ++bad; }
    if (!(rec.d2 <= gate) && used != 0) { printf("  gated at the first linearisation: used = %d\n", used); ++bad; }
    if (far_range && !(rec.outcome == 1 && irr_at == 1 && (int)itrec[5] == 0 && used == 1 && blk.np == 0)) {
        printf("  the far range: outcome %d, irregular at %d (observation %d), used %d, block np %d\n", rec.outcome, irr_at, (int)itrec[5], used, blk.np);
        ++bad;
    }

    // the host's decision
    int outcome = rec.outcome != 1 ? 0 : (!(rec.d2 <= gate) ? 2 : (irr_at >= 0 ? 0 : 1));
    if (outcome == 1 && np > 0) {
        JointUpdateArgs u;
        u.n_mm = 2 * N; u.cur = S.cur; u.np = np;
        if (np <= 8) launch_wg(S.grid(), { 3, 2 }, [&] { k_gather_joint<double, 8>(st, u, &blk); });
        else launch_wg(S.grid(), { 3, 2 }, [&] { k_gather_joint<double, 32>(st, u, &blk); });
        S.flip();
        // the pass: the np pairs in slot order over every stored entry (diagonal tiles whole)
        for (int p = 0; p < np; ++p) {
            const double2 *G2 = (const double2 *)(S.st.Gp + (size_t)p * S.st.pair_stride), *K2 = (const double2 *)(S.st.Kp + (size_t)p * S.st.pair_stride);
            for (int r = 0; r < 2 * N; ++r) for (int c = 0; c < 2 * N; ++c) {
                if (c > r && (r / T) != (c / T)) continue;
                S.tile(r, c) = rank2_apply(S.tile(r, c), K2[r], G2[c]);
            }
            // the pair is zero over the padded tail (N = 41: columns 82 .. 95)
            if (N == 41 && S.tm.padded(2 * N) - 2 * N != 14) { printf("  N = 41 has no padded tail\n"); ++bad; }
            for (int c = 2 * N; c < (int)S.tm.padded(2 * N); ++c)
                if (G2[c].x != 0.0 || G2[c].y != 0.0 || K2[c].x != 0.0 || K2[c].y != 0.0) { printf("  pair %d is not zero at padded column %d\n", p, c); ++bad; }
        }
        // the tiles' own copies of the diagonal blocks went through the same chain as the live ones: the same bits
        for (int k = 0; k < N; ++k) {
            const double t3[3] = { S.tile(2 * k, 2 * k), S.tile(2 * k + 1, 2 * k), S.tile(2 * k + 1, 2 * k + 1) };
            if (memcmp(t3, &S.diag[S.dcur][3 * k], 24)) { printf("  landmark %d: the live diagonal block differs from the tile's\n", k); ++bad; }
        }
    } else {
        // gated, irregular or empty: nothing was written
        bad += differ(S.x[0], before.x[0], "x") + differ(S.x[1], before.x[1], "x (other buffer)") + differ(S.strip[0], before.strip[0], "strip") +
               differ(S.strip[1], before.strip[1], "strip (other buffer)") + differ(S.prr[0], before.prr[0], "prr") + differ(S.prr[1], before.prr[1], "prr (other)") +
               differ(S.diag[0], before.diag[0], "diag") + differ(S.diag[1], before.diag[1], "diag (other buffer)") + differ(S.tiles, before.tiles, "tiles") +
               differ(S.ring, before.ring, "ring");
    }
    dense(S, x1, P1);
    const double n = 3 + 2 * N, head[4] = { n, (double)m, (double)outcome, (double)iterations };
    put(f, head, 4);
    for (int k = 0; k < m; ++k) {
        const Obs &o = obs[k];
        const double row[8] = { (double)o.model, o.z[0], o.z[1], o.R[0], o.R[1], o.R[2], o.R[3], (double)hyp[k] };
        put(f, row, 8);
    }
    put(f, x0.data(), x0.size()); put(f, P0.data(), P0.size()); put(f, x1.data(), x1.size()); put(f, P1.data(), P1.size());
    const double tail[4] = { rec.d2, itrec[0], itrec[1], itrec[4] };
    put(f, tail, 4);
    printf("%s, %d linearisations: np = %d, outcome %d, used %d, last step %.3g, d2 = %.6g -> %.6g: %d differences\n", name, iterations, np, outcome,
           used, itrec[2], rec.d2, itrec[3], bad);
    return bad;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "wb");
    if (!f) return 2;
    int bad = 0;
    const std::vector<std::pair<int, int>> one = { { 1, 17 } }, two = { { 4, 8 }, { 2, 9 } },                       // neighbours: adjacent lane pairs, one tile
        five = { { 1, 0 }, { 2, 40 }, { 3, 20 }, { 4, -1 }, { 1, 21 }, { 4, 5 } };                              // landmark 0, landmark N - 1 of N = 41, one entry left out
    std::vector<std::pair<int, int>> all;
    for (int q = 0; q < 32; ++q) all.push_back({ 1 + q % 4, (7 * q + 3) % 40 });
    for (int iterations : { 1, 3, 8 }) {
        bad += run_case(f, "one pairing", 40, 3, one, INFINITY, iterations, false);
        bad += run_case(f, "neighbours", 40, 4, two, INFINITY, iterations, false);
        bad += run_case(f, "mixed models, an entry left out, a padded tail", 41, 5, five, INFINITY, iterations, false);
        bad += run_case(f, "a full scan", 40, 6, all, INFINITY, iterations, false);
        bad += run_case(f, "a full scan, a padded tail", 41, 7, all, INFINITY, iterations, false);
    }
    bad += run_case(f, "gated", 40, 4, two, 0.0, 3, false);
    bad += run_case(f, "irregular at the second linearisation", 41, 5, five, INFINITY, 3, true);
    fclose(f);
    return bad != 0;
}
