// Host build of the ekfm:: functions k_joint_innovation runs (ekf_slam_amd/csrc/device_math.h): joint_pairing, joint_cross_block,
// joint_pivot / joint_factor_scale / joint_factor_update with one lane, joint_prefix_add -- put together in the kernel's phases.
// Reads one hypothesis per line from stdin and answers each with one line of %.17g numbers (tests/test_joint_cpu.py):
//   joint m  (model z0 z1 R00 R01 R10 R11 landmark) x m   prr[0..8] xr[0..2]
//         then for every paired entry (landmark >= 0) in scan order: strip6[0..5] diag3[0..2] l0 l1
//         then for every two pairings a > b (a = 1 .., b = 0 .. a-1): P(l_a + r, l_b + c) as pab[2 r + c]
//   -> outcome first_irregular dof pairings d2  prefix[0..m-1]  nu[0..2m-1]  S[0..4m^2-1] (column-major, by scan index)
#include "device_math.h"
#include <cstdio>
#include <cstring>
#include <vector>

int main() {
    char what[16];
    while (scanf("%15s", what) == 1) {
        if (strcmp(what, "joint")) return 2;
        int m;
        if (scanf("%d", &m) != 1 || m < 1 || m > 32) return 2;
        std::vector<int> model(m), pair_of(m, -1), scan_of;
        std::vector<long long> lm(m);
        std::vector<double> z(2 * m), R(4 * m);
        for (int k = 0; k < m; ++k) {
            if (scanf("%d", &model[k]) != 1) return 2;
            for (int q = 0; q < 2; ++q) if (scanf("%lf", &z[2 * k + q]) != 1) return 2;
            for (int q = 0; q < 4; ++q) if (scanf("%lf", &R[4 * k + q]) != 1) return 2;
            if (scanf("%lld", &lm[k]) != 1) return 2;
            if (lm[k] >= 0) { pair_of[k] = (int)scan_of.size(); scan_of.push_back(k); }
        }
        double prr[9], xr[3];
        for (double &v : prr) if (scanf("%lf", &v) != 1) return 2;
        for (double &v : xr) if (scanf("%lf", &v) != 1) return 2;
        const int np = (int)scan_of.size(), n = 2 * np, ld = n > 0 ? n : 1;
        std::vector<double> A((size_t)ld * ld, 0.0), y(ld, 0.0), Hr(6 * np + 1), Ht(4 * np + 1), strips(6 * np + 1);
        std::vector<int> posed(np);
        int dof = 0;
        // (1) per pairing
        for (int p = 0; p < np; ++p) {
            const int k = scan_of[p];
            double diag3[3], l[2], S[4], nu[2];
            for (int q = 0; q < 6; ++q) if (scanf("%lf", &strips[6 * p + q]) != 1) return 2;
            for (double &v : diag3) if (scanf("%lf", &v) != 1) return 2;
            for (double &v : l) if (scanf("%lf", &v) != 1) return 2;
            posed[p] = ekfm::joint_pairing(model[k], &z[2 * k], &R[4 * k], prr, &strips[6 * p], diag3, xr, l, &Hr[6 * p], &Ht[4 * p], S, nu);
            y[2 * p] = nu[0]; y[2 * p + 1] = nu[1];
            A[(2 * p) * ld + 2 * p] = S[0]; A[(2 * p) * ld + 2 * p + 1] = S[1];
            A[(2 * p + 1) * ld + 2 * p] = S[2]; A[(2 * p + 1) * ld + 2 * p + 1] = S[3];
            dof += (model[k] == 1 || model[k] == 4) ? 2 : 1;
        }
        // (2) the off-diagonal blocks
        for (int pa = 1; pa < np; ++pa)
            for (int pb = 0; pb < pa; ++pb) {
                double pab[4], Sab[4];
                for (double &v : pab) if (scanf("%lf", &v) != 1) return 2;
                ekfm::joint_cross_block(&Hr[6 * pa], &Ht[4 * pa], &Hr[6 * pb], &Ht[4 * pb], prr, &strips[6 * pa], &strips[6 * pb], pab, Sab);
                for (int q = 0; q < 4; ++q) A[(2 * pa + (q >> 1)) * ld + 2 * pb + (q & 1)] = Sab[q];
            }
        // (3) nu and S by scan index
        std::vector<double> nu_out(2 * m), S_out((size_t)4 * m * m);
        for (int i = 0; i < 2 * m; ++i) nu_out[i] = pair_of[i >> 1] >= 0 ? y[2 * pair_of[i >> 1] + (i & 1)] : 0.0;
        for (int e = 0; e < 4 * m * m; ++e) {
            const int i = e % (2 * m), j = e / (2 * m);
            const int pi = pair_of[i >> 1], pj = pair_of[j >> 1];
            double v = i == j ? 1.0 : 0.0;
            if (pi >= 0 && pj >= 0) {
                const int ri = 2 * pi + (i & 1), rj = 2 * pj + (j & 1);
                v = (ri >= rj || pi == pj) ? A[ri * ld + rj] : A[rj * ld + ri];
            }
            S_out[e] = v;
        }
        // (4) the factorisation with one lane
        int bad = np;
        for (int p = np - 1; p >= 0; --p) if (!posed[p]) bad = p;
        for (int k = 0; k < 2 * bad; ++k) {
            double lkk;
            if (!ekfm::joint_pivot(A[k * ld + k], lkk)) { bad = k >> 1; break; }
            ekfm::joint_factor_scale(A.data(), ld, y.data(), n, k, lkk, 0, 1);
            ekfm::joint_factor_update(A.data(), ld, y.data(), n, k, 0, 1);
        }
        // (5) the prefixes and the record
        std::vector<double> prefix(m);
        double acc = 0.0;
        for (int k = 0; k < m; ++k) {
            const int p = pair_of[k];
            if (p >= 0) acc = p < bad ? ekfm::joint_prefix_add(acc, y[2 * p], y[2 * p + 1]) : NAN;
            prefix[k] = acc;
        }
        printf("%d %d %d %d %.17g", bad < np ? 0 : 1, bad < np ? scan_of[bad] : -1, dof, np, acc);
        for (double v : prefix) printf(" %.17g", v);
        for (double v : nu_out) printf(" %.17g", v);
        for (double v : S_out) printf(" %.17g", v);
        printf("\n");
    }
    return 0;
}
