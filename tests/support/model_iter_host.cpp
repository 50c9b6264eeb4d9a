// Host build of ekfm::model_iterate (ekf_slam_amd/csrc/device_math.h): the loop k_gather_model_iter's lane 0 runs.
// Reads cases from stdin, one per line, and answers each with one line of %.17g numbers (tests/test_model_iter_cpu.py):
//   iter  model has_landmark z0 z1 R00 R01 R10 R11 gate ax ay sm[0..37] iterations tol
//           ->  outcome d2 nu0[2] S0[4] | S[4] r[2] used converged last_step xi[7] | H[14] Gs[14]
//   small model has_landmark z0 z1 R00 R01 R10 R11 gate ax ay sm[0..37]
//           ->  outcome d2 nu[2] S[4] | H[14] Gs[14]        model_eval, model_wrap, model_small, linear_outcome in model_obs.h's order
// (sm: linear_small's 38 operands; the seven entries of x are sm[31..37]; R, S row-major).
#include "device_math.h"
#include <cstdio>
#include <cstring>

int main() {
    char what[16];
    while (scanf("%15s", what) == 1) {
        int model, has_landmark;
        if (scanf("%d %d", &model, &has_landmark) != 2) return 2;
        double z[2], R[4], gate, anchor[2], sm[ekfm::kLinearSmall];
        for (double &v : z) if (scanf("%lf", &v) != 1) return 2;
        for (double &v : R) if (scanf("%lf", &v) != 1) return 2;
        if (scanf("%lf", &gate) != 1) return 2;
        for (double &v : anchor) if (scanf("%lf", &v) != 1) return 2;
        for (double &v : sm) if (scanf("%lf", &v) != 1) return 2;
        double H[14], Gs[14], S[4], r[2];
        if (!strcmp(what, "iter")) {
            int iterations;
            double tol;
            if (scanf("%d %lf", &iterations, &tol) != 2) return 2;
            ekfm::ModelIterate it;
            const int outcome = ekfm::model_iterate(model, sm, anchor, has_landmark != 0, z, R, gate, iterations, tol, H, Gs, S, r, it);
            printf("%d %.17g %.17g %.17g", outcome, it.d2, it.nu0[0], it.nu0[1]);
            for (double v : it.S0) printf(" %.17g", v);
            for (double v : S) printf(" %.17g", v);
            printf(" %.17g %.17g %d %d %.17g", r[0], r[1], it.used, it.converged, it.last_step);
            for (double v : it.xi) printf(" %.17g", v);
        } else if (!strcmp(what, "small")) {
            double hx[2], d2;
            int wrap[2];
            const bool ok = ekfm::model_eval(model, sm + 31, anchor, has_landmark != 0, hx, H);
            ekfm::model_wrap(model, wrap);
            ekfm::model_small(sm, H, hx, z, R, wrap, Gs, S, r);
            int outcome = ekfm::linear_outcome(S, r, gate, d2);
            if (!ok) { outcome = 0; d2 = NAN; }
            printf("%d %.17g %.17g %.17g", outcome, d2, r[0], r[1]);
            for (double v : S) printf(" %.17g", v);
        } else return 2;
        for (double v : H) printf(" %.17g", v);
        for (double v : Gs) printf(" %.17g", v);
        printf("\n");
    }
    return 0;
}
