// Host build of ekfm::model_eval / model_small (ekf_slam_amd/csrc/device_math.h): the function k_gather_model's lane 0 runs.
// Reads cases from stdin, one per line, and answers each with one line of %.17g numbers (tests/test_model_obs_cpu.py):
//   eval  model has_landmark x y theta t0x t0y t1x t1y ax ay      ->  ok hx0 hx1 H[0..13]
//   small model has_landmark z0 z1 R00 R01 R10 R11 gate ax ay sm[0..37]   ->  ok outcome d2 nu0 nu1 S[0..3] Gs[0..13]
// (sm: linear_small's 38 operands; the seven entries of x are sm[31..37]).
#include "device_math.h"
#include <cstdio>
#include <cstring>

int main() {
    char what[16];
    while (scanf("%15s", what) == 1) {
        int model, has_landmark;
        if (scanf("%d %d", &model, &has_landmark) != 2) return 2;
        double hx[2], H[14];
        if (!strcmp(what, "eval")) {
            double xs[7], anchor[2];
            for (double &v : xs) if (scanf("%lf", &v) != 1) return 2;
            for (double &v : anchor) if (scanf("%lf", &v) != 1) return 2;
            const bool ok = ekfm::model_eval(model, xs, anchor, has_landmark != 0, hx, H);
            printf("%d %.17g %.17g", ok ? 1 : 0, hx[0], hx[1]);
            for (double v : H) printf(" %.17g", v);
            printf("\n");
        } else if (!strcmp(what, "small")) {
            double z[2], R[4], gate, anchor[2], sm[ekfm::kLinearSmall];
            for (double &v : z) if (scanf("%lf", &v) != 1) return 2;
            for (double &v : R) if (scanf("%lf", &v) != 1) return 2;
            if (scanf("%lf", &gate) != 1) return 2;
            for (double &v : anchor) if (scanf("%lf", &v) != 1) return 2;
            for (double &v : sm) if (scanf("%lf", &v) != 1) return 2;
            double Gs[14], S[4], nu[2], d2;
            int wrap[2];
            const bool ok = ekfm::model_eval(model, sm + 31, anchor, has_landmark != 0, hx, H);
            ekfm::model_wrap(model, wrap);
            ekfm::model_small(sm, H, hx, z, R, wrap, Gs, S, nu);
            int outcome = ekfm::linear_outcome(S, nu, gate, d2);
            if (!ok) { outcome = 0; d2 = NAN; }
            printf("%d %d %.17g %.17g %.17g", ok ? 1 : 0, outcome, d2, nu[0], nu[1]);
            for (double v : S) printf(" %.17g", v);
            for (double v : Gs) printf(" %.17g", v);
            printf("\n");
        } else return 2;
    }
    return 0;
}
