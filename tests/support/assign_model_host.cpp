// Host build of ekfm::CandList and ekfm::assign_solve (ekf_slam_amd/csrc/assign_math.h): the list k_assign_candidates / k_assign_select keep
// and the solver k_assign_solve runs.  Reads cases from stdin and answers each with one line of %.17g numbers
// (tests/test_assign_model_cpu.py):
//   merge  gate n  (d2 regular) x n  nparts  cut_1 .. cut_(nparts-1)  reversed
//          -> two lists of  n idx[0..31] d2[0..31]  (-1 / inf behind n): the keys offered in order to ONE list, then the keys cut at the
//          given positions, each part offered to a list of its own, and the parts merged (in reverse order where asked)
//   solve  nlanes m  then per row: gate n (idx d2) x n
//          -> landmark[0..m-1] d2[0..m-1] total : ekfm::assign_solve with a team of nlanes emulated lanes
#include "assign_math.h"
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

static void print_list(const ekfm::CandList &c) {
    printf("%lld", c.n);
    for (int s = 0; s < ekfm::kAssignCand; ++s) printf(" %lld", s < c.n ? c.idx[s] : -1LL);
    for (int s = 0; s < ekfm::kAssignCand; ++s) printf(" %.17g", s < c.n ? c.d2[s] : INFINITY);
}

int main() {
    char what[16];
    while (scanf("%15s", what) == 1) {
        if (!strcmp(what, "merge")) {
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
            ekfm::CandList whole;
            ekfm::cand_init(whole);
            for (int i = 0; i < n; ++i) ekfm::cand_offer(whole, d2[i], i, regular[i] != 0, gate);
            std::vector<ekfm::CandList> part(nparts);
            for (int p = 0; p < nparts; ++p) {
                ekfm::cand_init(part[p]);
                for (int i = cut[p]; i < cut[p + 1]; ++i) ekfm::cand_offer(part[p], d2[i], i, regular[i] != 0, gate);
            }
            ekfm::CandList merged;
            ekfm::cand_init(merged);
            for (int p = 0; p < nparts; ++p) merged = ekfm::cand_merge(merged, part[reversed ? nparts - 1 - p : p]);
            print_list(whole);
            printf(" ");
            print_list(merged);
            printf("\n");
        } else if (!strcmp(what, "solve")) {
            int nlanes, m;
            if (scanf("%d %d", &nlanes, &m) != 2 || nlanes < 1 || m < 1 || m > ekfm::kAssignMax) return 2;
            std::unique_ptr<ekfm::AssignProblem> p(new ekfm::AssignProblem());
            p->m = m;
            for (int k = 0; k < m; ++k) {
                int n;
                if (scanf("%lf %d", &p->gate[k], &n) != 2 || n < 0 || n > ekfm::kAssignCand) return 2;
                p->n[k] = n;
                for (int s = 0; s < ekfm::kAssignCand; ++s) { p->idx[k * ekfm::kAssignCand + s] = -1; p->d2[k * ekfm::kAssignCand + s] = INFINITY; }
                for (int s = 0; s < n; ++s)
                    if (scanf("%lld %lf", &p->idx[k * ekfm::kAssignCand + s], &p->d2[k * ekfm::kAssignCand + s]) != 2) return 2;
            }
            ekfm::AssignHostTeam team = { nlanes };
            ekfm::assign_solve(*p, team);
            for (int k = 0; k < m; ++k) printf("%lld ", ekfm::assign_landmark(*p, k));
            for (int k = 0; k < m; ++k) printf("%.17g ", ekfm::assign_d2(*p, k));
            printf("%.17g\n", ekfm::assign_total(*p));
        } else return 2;
    }
    return 0;
}
