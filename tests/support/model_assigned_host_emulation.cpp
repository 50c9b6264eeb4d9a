// Host emulation of k_gather_model_assigned (tests/test_observe_assigned_cpu.py compiles and runs it; no GPU, no HIP runtime).
// The kernel SOURCES of ekf_slam_amd/csrc (tile_access.h, pair_column.h, constrain.h, linear_obs.h, model_obs.h, model_assigned.h) are
// compiled for the host behind kernel_host_shim.h, in model_obs_host_emulation.cpp's manner, and on the same state, with 0 and with 3
// pairs pending in the ring:
//   a slot that names a landmark    k_gather_model_assigned must write, BIT FOR BIT, what k_gather_model writes with a.a[0] set on the host:
//                                   the pair ring, the strip, Prr, the diagonal blocks, x, the record and the counters
//   a slot of -1, and one of N      a zero pair in the slot, the state copied, outcome 3.0 with d2 NaN, S and nu zero, BOTH counters untouched
//   a landmark behind a tight gate  outcome 2.0 and one count in the gated counter, as k_gather_model counts it
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "kernel_host_shim.h"
#include "emulated_state.h"
#include "model_obs.h"
#include "model_assigned.h"

int main() {
    const double RP[4] = { 0.02, 0.005, 0.005, 0.03 }, R1[4] = { 0.05, 0, 0, 1.0 };
    int total_bad = 0;
    for (int T : { 16, 64 }) for (int pending : { 0, 3 }) {
        const int N = 150, cap = 158;
        Store base(T, N, cap);
        fill(base, 11, true);
        int64_t cnt0[2] = { 0, 0 };
        double rec0[8];
        for (int k = 0; k < pending; ++k) {                   // some pairs pending in the ring (never applied to the tiles)
            LinearArgs a = {};
            for (int q = 0; q < 14; ++q) a.H[q] = 0.4 * rnd();
            a.a[0] = 2 * (k ? 5 + 40 * k : 72); a.a[1] = 2 * (N - 1 - k);
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
        // the observation of `model` that lies 0.3 (and -0.4) off what the model predicts for landmark lm at the base state
        auto observation = [&](int model, int64_t lm, double gate) {
            const double *x = base.x[base.cur].data();
            AssignedModelArgs m = {};
            m.model = model; m.a[0] = m.a[1] = -1;
            m.gate = gate; m.n_mm = 2 * N; m.cur = base.cur; m.npend = pending; m.pstart = 0;
            const bool two = model == 1 || model == 4;
            memcpy(m.R, two ? RP : R1, sizeof m.R);
            const double xs[7] = { x[0], x[1], x[2], x[3 + 2 * lm], x[4 + 2 * lm], 0, 0 };
            double hx[2], H[14];
            ekfm::model_eval(model, xs, m.anchor, true, hx, H);
            m.z[0] = hx[0] + 0.3; m.z[1] = two ? hx[1] - 0.4 : 0.0;
            return m;
        };
        // the launch, by run_linear's three passes; the counters start at (5, 7) so that "untouched" shows
        auto launch_assigned = [&](Store<double> &S, const AssignedModelArgs &m, int64_t slot_landmark, double *rec, int64_t *cnt) {
            AssignedRecord slot = { slot_landmark, 0.0, 0, 0 };
            DevState st = S.st;
            launch_wg(S.grid(), { 3, 2, cnt }, [&] { k_gather_model_assigned<double>(st, m, &slot, rec, cnt); });
            S.flip();
        };
        for (int64_t lm : { (int64_t)72, (int64_t)0, (int64_t)N - 1 }) for (int model = 1; model <= 4; ++model) {
            Store A(base), B(base);
            A.sync(); B.sync();
            const AssignedModelArgs m = observation(model, lm, INFINITY);
            double recA[8], recB[8];
            int64_t cntA[2] = { 5, 7 }, cntB[2] = { 5, 7 };
            launch_assigned(A, m, lm, recA, cntA);
            ModelArgs host = m;                               // the twin: the landmark named by the host
            host.a[0] = 2 * lm;
            DevState stB = B.st;
            launch_wg(B.grid(), { 3, 2, cntB }, [&] { k_gather_model<double>(stB, host, recB, cntB); });
            B.flip();
            int bad = 0;
            if (recA[7] != 1.0) { printf("  not applied\n"); ++bad; }
            if (memcmp(recA, recB, sizeof recA)) { printf("  the record differs\n"); ++bad; }
            if (memcmp(cntA, cntB, sizeof cntA) || cntA[0] != 5 || cntA[1] != 7) { printf("  the counters differ\n"); ++bad; }
            bad += differ(A.ring, B.ring, "pair ring") + differ(A.strip[A.cur], B.strip[B.cur], "strip") + differ(A.prr[A.cur], B.prr[B.cur], "prr") +
                   differ(A.diag[A.dcur], B.diag[B.dcur], "diag") + differ(A.x[A.cur], B.x[B.cur], "x");
            double moved = 0;
            for (size_t i = 0; i < A.x[A.cur].size(); ++i) moved = std::fmax(moved, std::fabs(A.x[A.cur][i] - base.x[base.cur][i]));
            if (!(moved > 1e-6)) { printf("  x did not move\n"); ++bad; }
            printf("T=%d pending=%d landmark %d model %d against the host-named step: %d differences\n", T, pending, (int)lm, model, bad);
            total_bad += bad;
        }
        for (int64_t slot : { (int64_t)-1, (int64_t)N }) {
            Store A(base);
            A.sync();
            const AssignedModelArgs m = observation(1, 72, INFINITY);
            double recA[8];
            int64_t cntA[2] = { 5, 7 };
            launch_assigned(A, m, slot, recA, cntA);
            int bad = 0;
            if (recA[7] != 3.0 || !std::isnan(recA[6])) { printf("  outcome %g, d2 %g\n", recA[7], recA[6]); ++bad; }
            for (int q = 0; q < 6; ++q) if (recA[q] != 0.0) ++bad;
            if (cntA[0] != 5 || cntA[1] != 7) { printf("  a counter moved\n"); ++bad; }
            bad += differ(A.x[A.cur], base.x[base.cur], "x") + differ(A.strip[A.cur], base.strip[base.cur], "strip") +
                   differ(A.diag[A.dcur], base.diag[base.dcur], "diag");
            for (int q = 0; q < 9; ++q) if (A.prr[A.cur][q] != base.prr[base.cur][q]) ++bad;
            const size_t off = (size_t)pending * A.st.pair_stride;
            for (int64_t q = 0; q < 2 * A.tm.padded(2 * N); ++q) if (A.st.Gp[off + q] != 0.0 || A.st.Kp[off + q] != 0.0) ++bad;
            printf("T=%d pending=%d slot %d is a skipped step: %d differences\n", T, pending, (int)slot, bad);
            total_bad += bad;
        }
        {
            Store A(base);
            A.sync();
            const AssignedModelArgs m = observation(1, 72, 1e-9);
            double recA[8];
            int64_t cntA[2] = { 5, 7 };
            launch_assigned(A, m, 72, recA, cntA);
            int bad = 0;
            if (recA[7] != 2.0 || !(recA[6] > 1e-9)) { printf("  outcome %g, d2 %g\n", recA[7], recA[6]); ++bad; }
            if (cntA[0] != 5 || cntA[1] != 8) { printf("  counters %d %d\n", (int)cntA[0], (int)cntA[1]); ++bad; }
            bad += differ(A.x[A.cur], base.x[base.cur], "x") + differ(A.strip[A.cur], base.strip[base.cur], "strip");
            printf("T=%d pending=%d a landmark behind a tight gate: %d differences\n", T, pending, bad);
            total_bad += bad;
        }
    }
    return total_bad != 0;
}
