// Host build of ekfm::assoc_model_d2 and ekfm::Match2 (ekf_slam_amd/csrc/device_math.h): the functions k_assoc_model's lanes run.
// Reads cases from stdin and answers each with one line of %.17g numbers (tests/test_associate_model_cpu.py):
//   d2     model z0 z1 R00 R01 R10 R11 prr[0..8] strip6[0..5] diag3[0..2] xr[0..2] l0 l1      ->  regular d2
//   match  gate n  (d2 regular) x n  nparts  cut_1 .. cut_(nparts-1)  reversed
//          -> two records of  best second d2_best d2_second within irregular : the list offered in order to ONE record, then the list cut
//          at the given positions, each part offered to a record of its own, and the parts merged (in reverse order where asked)
#include "device_math.h"
#include <cstdio>
#include <cstring>
#include <vector>

static void print_record(const ekfm::Match2 &m) {
    printf("%lld %lld %.17g %.17g %lld %lld", m.best, m.second, m.d2_best, m.d2_second, m.within, m.irregular);
}

int main() {
    char what[16];
    while (scanf("%15s", what) == 1) {
        if (!strcmp(what, "d2")) {
            int model;
            double z[2], R[4], prr[9], strip6[6], diag3[3], xr[3], l[2], d2;
            if (scanf("%d", &model) != 1) return 2;
            for (double &v : z) if (scanf("%lf", &v) != 1) return 2;
            for (double &v : R) if (scanf("%lf", &v) != 1) return 2;
            for (double &v : prr) if (scanf("%lf", &v) != 1) return 2;
            for (double &v : strip6) if (scanf("%lf", &v) != 1) return 2;
            for (double &v : diag3) if (scanf("%lf", &v) != 1) return 2;
            for (double &v : xr) if (scanf("%lf", &v) != 1) return 2;
            for (double &v : l) if (scanf("%lf", &v) != 1) return 2;
            const bool regular = ekfm::assoc_model_d2(model, z, R, prr, strip6, diag3, xr, l, d2);
            printf("%d %.17g\n", regular ? 1 : 0, d2);
        } else if (!strcmp(what, "match")) {
            double gate;
            int n, nparts, reversed;
            if (scanf("%lf %d", &gate, &n) != 2 || n < 0) return 2;
            std::vector<double> d2(n);
            std::vector<int> regular(n);
            for (int i = 0; i < n; ++i) if (scanf("%lf %d", &d2[i], &regular[i]) != 2) return 2;
            if (scanf("%d", &nparts) != 1 || nparts < 1) return 2;
            std::vector<int> cut(nparts + 1, 0);
            cut[nparts] = n;
            for (int p = 1; p < nparts; ++p) if (scanf("%d", &cut[p]) != 1 || cut[p] < cut[p - 1] || cut[p] > n) return 2;
            if (scanf("%d", &reversed) != 1) return 2;
            ekfm::Match2 whole;
            ekfm::match2_init(whole);
            for (int i = 0; i < n; ++i) ekfm::match2_offer(whole, d2[i], i, regular[i] != 0, gate);
            std::vector<ekfm::Match2> part(nparts);
            for (int p = 0; p < nparts; ++p) {
                ekfm::match2_init(part[p]);
                for (int i = cut[p]; i < cut[p + 1]; ++i) ekfm::match2_offer(part[p], d2[i], i, regular[i] != 0, gate);
            }
            ekfm::Match2 merged;
            ekfm::match2_init(merged);
            for (int p = 0; p < nparts; ++p) merged = ekfm::match2_merge(merged, part[reversed ? nparts - 1 - p : p]);
            print_record(whole);
            printf(" ");
            print_record(merged);
            printf("\n");
        } else return 2;
    }
    return 0;
}
