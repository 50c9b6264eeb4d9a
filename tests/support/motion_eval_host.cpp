// Host build of ekfm::motion_eval, ekfm::motion_chord and ekfm::motion_noise_entry (ekf_slam_amd/csrc/device_math.h): the functions
// k_predict_model's lanes run.  Reads cases from stdin, one per line, and answers each with one line of %.17g numbers
// (tests/test_predict_model_cpu.py):
//   eval model x y theta u0 u1 u2   ->  ok xn[0..2] fa fb V[0..8] (row-major)
//   chord turn                      ->  a g g'  for the arc that turns by `turn` degrees, formed as motion_eval forms them
//   noise V[0..8] m6[0..5]          ->  Q[0..8] (row-major), entry by entry
#include "device_math.h"
#include <cstdio>
#include <cstring>

int main() {
    char what[16];
    while (scanf("%15s", what) == 1) {
        if (!strcmp(what, "eval")) {
            int model;
            double xr[3], u[3];
            if (scanf("%d", &model) != 1) return 2;
            for (double &v : xr) if (scanf("%lf", &v) != 1) return 2;
            for (double &v : u) if (scanf("%lf", &v) != 1) return 2;
            double xn[3] = { 0, 0, 0 }, fa = 0, fb = 0, V[9] = { 0 };
            const bool ok = ekfm::motion_eval(model, xr, u, xn, fa, fb, V);
            printf("%d %.17g %.17g %.17g %.17g %.17g", ok ? 1 : 0, xn[0], xn[1], xn[2], fa, fb);
            for (double v : V) printf(" %.17g", v);
            printf("\n");
        } else if (!strcmp(what, "chord")) {
            double turn;
            if (scanf("%lf", &turn) != 1) return 2;
            const double half = 0.5 * turn, a = half / ekfm::kR2D;
            double sa, ca, g, gp;
            ekfm::sincosd(half, sa, ca);
            ekfm::motion_chord(a, sa, ca, g, gp);
            printf("%.17g %.17g %.17g\n", a, g, gp);
        } else if (!strcmp(what, "noise")) {
            double V[9], m6[6];
            for (double &v : V) if (scanf("%lf", &v) != 1) return 2;
            for (double &v : m6) if (scanf("%lf", &v) != 1) return 2;
            for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) printf(i + j ? " %.17g" : "%.17g", ekfm::motion_noise_entry(V, m6, i, j));
            printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
