// Host build of the ekfm:: functions ekf_joint_search adds (ekf_slam_amd/csrc/device_math.h): the row-append joint_append_step /
// joint_append_close against the right-looking joint_pivot / joint_factor_scale / joint_factor_update run on the whole matrix, and the
// order joint_search_before with the cut joint_search_cut.  Reads one case per line from stdin and answers each with one line of %.17g
// numbers (tests/test_joint_search_cpu.py):
//   append n lanes  S[0 .. n*n-1] (row-major, the lower triangle is read)  nu[0 .. n-1]          n even, <= 64
//     -> mismatches bad_right_looking bad_append  prefix_right_looking[0 .. n/2-1]  prefix_append[0 .. n/2-1]
//        mismatches: entries of L, roots of the pivots, entries of y and prefixes in front of the first irregular pairing whose BITS differ
//        bad_*: the first pairing with a failing pivot (n/2: none); a prefix from there on is NaN
//   before n  pa da ha[0 .. n-1] ta  pb db hb[0 .. n-1] tb      -> 1 where a stands before b, else 0
//   cut survived beam                                            -> alive truncated
//   passes d2 threshold                                          -> 1 or 0
#include "device_math.h"
#include <cstdio>
#include <cstring>
#include <vector>

static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }

static int run_append() {
    int n, lanes;
    if (scanf("%d %d", &n, &lanes) != 2 || n < 2 || n > 64 || (n & 1) || lanes < 1) return 2;
    std::vector<double> S((size_t)n * n), nu(n);
    for (double &v : S) if (scanf("%lf", &v) != 1) return 2;
    for (double &v : nu) if (scanf("%lf", &v) != 1) return 2;
    const int np = n / 2, ld = n;
    // the right-looking factorisation of the whole matrix, one lane, as k_joint_innovation stops it
    std::vector<double> A(S), y(nu);
    int bad = np;
    for (int k = 0; k < 2 * bad; ++k) {
        double lkk;
        if (!ekfm::joint_pivot(A[k * ld + k], lkk)) { bad = k >> 1; break; }
        ekfm::joint_factor_scale(A.data(), ld, y.data(), n, k, lkk, 0, 1);
        ekfm::joint_factor_update(A.data(), ld, y.data(), n, k, 0, 1);
    }
    std::vector<double> pre(np), pre2(np);
    double acc = 0.0;
    for (int p = 0; p < np; ++p) { acc = p < bad ? ekfm::joint_prefix_add(acc, y[2 * p], y[2 * p + 1]) : NAN; pre[p] = acc; }
    // the same matrix two rows at a time: L with the pivots' roots on its diagonal, as the node store keeps it
    std::vector<double> L((size_t)n * n, 0.0), y2(n, 0.0), a0(n + 2), a1(n + 2), l0(n + 2), l1(n + 2);
    int bad2 = np;
    acc = 0.0;
    for (int p = 0; p < np; ++p) {
        const int i0 = 2 * p;
        if (bad2 == np) {
            for (int j = 0; j <= i0; ++j) { a0[j] = S[i0 * ld + j]; a1[j] = S[(i0 + 1) * ld + j]; }
            a0[i0 + 1] = nu[i0];
            a1[i0 + 1] = S[(i0 + 1) * ld + i0 + 1]; a1[i0 + 2] = nu[i0 + 1];
            for (int k = 0; k < i0; ++k)
                for (int lane = lanes - 1; lane >= 0; --lane)          // (any order: within a step no lane reads what another writes)
                    ekfm::joint_append_step(L.data(), ld, y2.data(), a0.data(), a1.data(), l0.data(), l1.data(), i0, k, lane, lanes);
            if (ekfm::joint_append_close(a0.data(), a1.data(), l0.data(), l1.data(), i0)) {
                for (int j = 0; j <= i0; ++j) L[i0 * ld + j] = l0[j];
                for (int j = 0; j <= i0 + 1; ++j) L[(i0 + 1) * ld + j] = l1[j];
                y2[i0] = l0[i0 + 1]; y2[i0 + 1] = l1[i0 + 2];
                acc = ekfm::joint_prefix_add(acc, y2[i0], y2[i0 + 1]);
            } else {
                bad2 = p;
            }
        }
        pre2[p] = bad2 == np ? acc : NAN;
    }
    int mism = 0;
    const int lim = 2 * (bad < bad2 ? bad : bad2);
    for (int i = 0; i < lim; ++i) {
        for (int j = 0; j < i; ++j) mism += !same_bits(A[i * ld + j], L[i * ld + j]);
        mism += !same_bits(sqrt(A[i * ld + i]), L[i * ld + i]);
        mism += !same_bits(y[i], y2[i]);
    }
    for (int p = 0; p < np; ++p) mism += !(same_bits(pre[p], pre2[p]) || (pre[p] != pre[p] && pre2[p] != pre2[p]));
    printf("%d %d %d", mism, bad, bad2);
    for (double v : pre) printf(" %.17g", v);
    for (double v : pre2) printf(" %.17g", v);
    printf("\n");
    return 0;
}

static int run_before() {
    int n;
    if (scanf("%d", &n) != 1 || n < 0 || n > 32) return 2;
    int p[2];
    double d[2];
    long long t[2];
    std::vector<long long> h[2];
    for (int s = 0; s < 2; ++s) {
        h[s].resize(n + 1);
        if (scanf("%d %lf", &p[s], &d[s]) != 2) return 2;
        for (int k = 0; k < n; ++k) if (scanf("%lld", &h[s][k]) != 1) return 2;
        if (scanf("%lld", &t[s]) != 1) return 2;
    }
    printf("%d\n", ekfm::joint_search_before(p[0], d[0], h[0].data(), t[0], p[1], d[1], h[1].data(), t[1], n) ? 1 : 0);
    return 0;
}

int main() {
    char what[16];
    while (scanf("%15s", what) == 1) {
        int rc = 2;
        if (!strcmp(what, "append")) rc = run_append();
        else if (!strcmp(what, "before")) rc = run_before();
        else if (!strcmp(what, "cut")) {
            int survived, beam;
            bool truncated;
            if (scanf("%d %d", &survived, &beam) == 2) {
                const int alive = ekfm::joint_search_cut(survived, beam, truncated);
                printf("%d %d\n", alive, truncated ? 1 : 0);
                rc = 0;
            }
        } else if (!strcmp(what, "passes")) {
            double d2, thr;
            if (scanf("%lf %lf", &d2, &thr) == 2) { printf("%d\n", ekfm::joint_search_passes(d2, thr) ? 1 : 0); rc = 0; }
        }
        if (rc) return rc;
    }
    return 0;
}
