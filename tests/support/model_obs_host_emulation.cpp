// Host emulation of the model-observation kernels (tests/test_model_obs_cpu.py compiles and runs it; no GPU, no HIP runtime).
// The kernel SOURCES of ekf_slam_amd/csrc (tile_access.h, pair_column.h, constrain.h, linear_obs.h, model_obs.h) are compiled for the host
// behind kernel_host_shim.h -- thread indices as globals, __shared__ as static storage, every workgroup run
// again until the small part's operands and lane_xor1's partners are there -- and two routes are compared BIT FOR BIT on
// the same state, with 0 and with 3 pairs pending in the ring:
//   the model:   k_gather_model, which forms H on its lane 0
//   the twin:    k_gather_linear handed the H that ekfm::model_eval gives the host at the same x, and a z that yields the same nu
// in the pair (G, K), the strip, Prr and the diagonal blocks; x to rounding; the record's S and outcome; k_model_probe's record against
// the launch's.  A target on the robot must leave a zero pair, the state copied and one count.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "kernel_host_shim.h"
#include "emulated_state.h"
#include "model_obs.h"

int main() {
    const double RP[4] = { 0.02, 0.005, 0.005, 0.03 };
    struct Case { const char *name; int model, l0, l1; bool anchored; };
    int total_bad = 0;
    for (int T : { 16, 64 }) for (int pending : { 0, 3 }) {
        const int N = 150, cap = 158, e = T == 16 ? 72 : 64;
        Store base(T, N, cap);
        fill(base, 11, true);
        int64_t cnt0[2] = { 0, 0 };
        double rec0[8];
        for (int k = 0; k < pending; ++k) {                   // some pairs pending in the ring (never applied to the tiles)
            LinearArgs a = {};
            for (int q = 0; q < 14; ++q) a.H[q] = 0.4 * rnd();
            a.a[0] = 2 * (k ? 5 + 40 * k : e); a.a[1] = 2 * (N - 1 - k);
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
            if (rec0[7] != 1.0) { printf("a pending pair did not apply\n"); return 2; }
        }
        const Case cases[] = { { "range and bearing, edge", 1, e, -1, false }, { "range, last", 2, N - 1, -1, false }, { "bearing, first", 3, 0, -1, false },
                               { "relative xy, edge", 4, e, -1, false }, { "landmark range over a tile edge", 5, e, e - 1, false },
                               { "landmark range, first and last", 5, 0, N - 1, false }, { "range and bearing, anchor", 1, -1, -1, true },
                               { "bearing, anchor", 3, -1, -1, true }, { "range, anchor on the robot", 2, -1, -1, true } };
        for (const Case &c : cases) {
            Store A(base), B(base);
            A.sync(); B.sync();
            const double *x = A.x[A.cur].data();
            const bool on_robot = !strcmp(c.name, "range, anchor on the robot");
            ModelArgs m = {};
            m.model = c.model; m.a[0] = c.l0 >= 0 ? 2 * c.l0 : -1; m.a[1] = c.l1 >= 0 ? 2 * c.l1 : -1;
            m.anchor[0] = on_robot ? x[0] : x[0] + 9.0; m.anchor[1] = on_robot ? x[1] : x[1] - 5.0;
            m.gate = INFINITY; m.n_mm = 2 * N; m.cur = A.cur; m.npend = pending; m.pstart = 0;
            const bool two = c.model == 1 || c.model == 4;
            const double R1[4] = { 0.05, 0, 0, 1.0 };
            memcpy(m.R, two ? RP : R1, sizeof m.R);
            double xs[7] = { x[0], x[1], x[2], 0, 0, 0, 0 }, hx[2], H[14];
            if (c.l0 >= 0) { xs[3] = x[3 + 2 * c.l0]; xs[4] = x[4 + 2 * c.l0]; }
            if (c.l1 >= 0) { xs[5] = x[3 + 2 * c.l1]; xs[6] = x[4 + 2 * c.l1]; }
            const bool posed = ekfm::model_eval(c.model, xs, m.anchor, c.l0 >= 0, hx, H);
            m.z[0] = hx[0] + 0.3; m.z[1] = two ? hx[1] - 0.4 : 0.0;
            if (c.model == 3) m.z[0] += 360.0;                                  // (a bearing a whole turn away: the wrap brings it back)
            double recA[8], recP[8], recB[8];
            int64_t cntA[2] = { 0, 0 }, cntB[2] = { 0, 0 };
            DevState stA = A.st;
            // the probe: one workgroup of 64 lanes twice (pass 0: the operands), no lane exchange; the launch: run_linear's three passes
            launch_wg(1, { 2, -1, nullptr, 64 }, [&] { k_model_probe<double>(stA, m, recP); });
            launch_wg(A.grid(), { 3, 2, cntA }, [&] { k_gather_model<double>(stA, m, recA, cntA); });
            A.flip();
            int bad = 0;
            if (memcmp(recA, recP, sizeof recA)) { printf("  the probe's record differs from the launch's\n"); ++bad; }
            if (on_robot) {
                // a finite no-op: outcome 0, d2 NaN, a zero pair, the state copied, one count
                if (posed || recA[7] != 0.0 || !std::isnan(recA[6]) || cntA[0] != 1 || cntA[1] != 0) { printf("  on the robot: not reported as irregular\n"); ++bad; }
                for (int q = 0; q < 6; ++q) if (!std::isfinite(recA[q])) ++bad;
                bad += differ(A.x[A.cur], base.x[base.cur], "x") + differ(A.strip[A.cur], base.strip[base.cur], "strip") +
                       differ(A.diag[A.dcur], base.diag[base.dcur], "diag");
                for (int q = 0; q < 9; ++q) if (A.prr[A.cur][q] != base.prr[base.cur][q]) ++bad;
                const size_t off = (size_t)pending * A.st.pair_stride;
                for (int64_t q = 0; q < 2 * A.tm.padded(2 * N); ++q) if (A.st.Gp[off + q] != 0.0 || A.st.Kp[off + q] != 0.0) ++bad;
            } else {
                LinearArgs l = {};
                memcpy(l.R, m.R, sizeof l.R); memcpy(l.H, H, sizeof H);
                if (c.l0 < 0) for (int r = 0; r < 2; ++r) for (int q = 3; q < 7; ++q) l.H[7 * r + q] = 0.0;
                l.a[0] = m.a[0]; l.a[1] = m.a[1]; l.gate = INFINITY; l.npend = pending;
                for (int r = 0; r < 2; ++r) {
                    double Hx = 0;
                    for (int i = 0; i < 7; ++i) Hx += l.H[7 * r + i] * xs[i];
                    l.z[r] = Hx + recA[4 + r];
                }
                run_linear(B, l, recB, cntB);
                if (recA[7] != 1.0 || recB[7] != 1.0 || cntA[0] || cntA[1]) { printf("  not applied\n"); ++bad; }
                if (memcmp(recA, recB, 4 * sizeof(double))) { printf("  S differs\n"); ++bad; }
                const double want0 = 0.3, want1 = two ? -0.4 : 0.0;
                if (std::fabs(recA[4] - want0) > 1e-11 || std::fabs(recA[5] - want1) > 1e-11) { printf("  nu = %.17g, %.17g\n", recA[4], recA[5]); ++bad; }
                if (!two && (recA[1] != 0.0 || recA[2] != 0.0 || recA[3] != 1.0 || recA[5] != 0.0)) { printf("  the second row is not empty\n"); ++bad; }
                bad += differ(A.strip[A.cur], B.strip[B.cur], "strip") + differ(A.prr[A.cur], B.prr[B.cur], "prr") + differ(A.diag[A.dcur], B.diag[B.dcur], "diag") +
                       differ(A.ring, B.ring, "pair ring");
                double dx = 0, moved = 0;
                for (size_t i = 0; i < A.x[A.cur].size(); ++i) {
                    dx = std::fmax(dx, std::fabs(A.x[A.cur][i] - B.x[B.cur][i]));
                    moved = std::fmax(moved, std::fabs(A.x[A.cur][i] - base.x[base.cur][i]));
                }
                if (!(dx < 1e-10) || !(moved > 1e-6)) { printf("  x: differs from the twin by %g, moved by %g\n", dx, moved); ++bad; }
            }
            printf("T=%d pending=%d %s: %d differences\n", T, pending, c.name, bad);
            total_bad += bad;
        }
    }
    return total_bad != 0;
}
