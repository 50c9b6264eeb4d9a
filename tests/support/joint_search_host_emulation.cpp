// Host emulation of the joint-compatibility search's kernels (tests/test_joint_search_emulation_cpu.py compiles and runs it; no GPU, no HIP
// runtime).  The kernel SOURCES of ekf_slam_amd/csrc (joint.h, joint_search.h and what they call: constrain.h, tile_access.h) are compiled
// for the host behind kernel_host_shim.h.  k_joint_search_prepare / _extend / _select and k_joint_innovation run with ONE lane
// (EKF_JOINT_SEARCH_LANES, EKF_JOINT_LANES: every phase is a loop strided by the lane count, so one lane carries out the phases in order),
// every workgroup of the fixed grids in turn.  The candidate lists and match records that k_assign_candidates / k_assign_select leave are
// formed by their own host functions (ekfm::assoc_model_d2, cand_offer, match2_offer: the list is the same whatever the shape of the reduction).
// argv[1]: the cases, as doubles:  ncases, then per case  N m beam pending float_store  x (n)  P (n x n)  (model z0 z1 R00 R01 R10 R11 gate) x m
//          (R as the library parses it: row-major, a one-row model [r, 0, 0, 1])  threshold (2m + 1)
// Per case it checks here, bit for bit: every alive hypothesis's d2 against k_joint_innovation's prefix at the last scan index on the same
// state, the winner against the first alive row, and that every buffer of the state is as it was.  And it writes to argv[2], as doubles,
// what the test compares with the NumPy search:  n m  x (n)  P (n x n, the pending pairs applied)  lm (m)  d2 dof pairings truncated
// nalive irregular  tested (m)  survived (m)  alive_d2 (64)  differences
#define EKF_JOINT_LANES 1
#define EKF_JOINT_SEARCH_LANES 1
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "kernel_host_shim.h"
#include "emulated_state.h"
#include "assign_math.h"
#include "joint.h"
#include "joint_search.h"

static JointSearchStore store;
static JointSearchOut out;

template <typename TS> static int run_case(const double *&in, FILE *f, int index) {
    const int N = (int)in[0], m = (int)in[1], beam = (int)in[2], pending = (int)in[3], n = 3 + 2 * N, T = 16;
    in += 5;
    Store<TS> S(T, N, N + 3, 8);
    const double *x = in, *P = in + n;
    in += n + (size_t)n * n;
    for (int i = 0; i < n; ++i) S.x[0][i] = x[i];
    for (int k = 0; k < N; ++k) S.s[k] = k + 1.0;
    scatter(S, [&](int r, int c) { return P[(size_t)r * n + c]; });
    srand(100 + index);
    int64_t cnt0[2] = { 0, 0 };
    double rec0[8];
    for (int k = 0; k < pending; ++k) {                       // some pairs pending in the ring (never applied to the tiles)
        LinearArgs a = {};
        for (int q = 0; q < 14; ++q) a.H[q] = 0.4 * rnd();
        a.a[0] = 2 * (3 + 5 * k); a.a[1] = 2 * (N - 1 - k);
        const double R[4] = { 0.3, 0.05, 0.05, 0.2 };
        memcpy(a.R, R, sizeof R);
        const double *xs = S.x[S.cur].data();
        for (int r = 0; r < 2; ++r) {
            double hx = 0;
            for (int i = 0; i < 3; ++i) hx += a.H[7 * r + i] * xs[i];
            for (int b = 0; b < 2; ++b) for (int c = 0; c < 2; ++c) hx += a.H[7 * r + 3 + 2 * b + c] * xs[3 + a.a[b] + c];
            a.z[r] = hx + 0.02 * rnd();
        }
        a.gate = INFINITY; a.npend = k;
        run_linear(S, a, rec0, cnt0);
        if (rec0[7] != 1.0) { printf("a pending pair did not apply\n"); return 1000; }
    }
    JointArgs a = JointArgs();
    a.N = N; a.m = m; a.cur = S.cur; a.npend = pending; a.pstart = 0;
    JointSearchLevelArgs la = JointSearchLevelArgs();
    la.m = m; la.beam = beam;
    for (int k = 0; k < m; ++k, in += 8) {
        AssocModelEntry &e = a.e[k];
        e.model = (int)in[0]; e.z[0] = in[1]; e.z[1] = in[2];
        for (int q = 0; q < 4; ++q) e.R[q] = in[3 + q];
        e.gate = in[7];
        la.rows[k] = (e.model == 1 || e.model == 4) ? 2 : 1;
    }
    for (int d = 0; d <= 2 * m; ++d) la.threshold[d] = *in++;
    DevState st = S.st;
    const Store<TS> before = S;

    // what k_assign_candidates and k_assign_select leave: the lists and the match records
    std::vector<ekfm::CandList> sel(m);
    std::vector<ekfm::Match2> match(m);
    for (int k = 0; k < m; ++k) {
        ekfm::cand_init(sel[k]);
        ekfm::match2_init(match[k]);
        const double *xs = st.x[a.cur], *p9 = st.prr[a.cur];
        for (int64_t i = 0; i < N; ++i) {
            const double *strip = st.strip[a.cur] + 2 * i, *dg = st.diag[st.dcur] + 3 * i;
            const double xr[3] = { xs[0], xs[1], xs[2] }, l[2] = { xs[3 + 2 * i], xs[4 + 2 * i] };
            const double strip6[6] = { strip[0], strip[1], strip[st.ldm], strip[st.ldm + 1], strip[2 * st.ldm], strip[2 * st.ldm + 1] };
            const double diag3[3] = { dg[0], dg[1], dg[2] };
            double d2 = NAN;
            const bool regular = ekfm::assoc_model_d2(a.e[k].model, a.e[k].z, a.e[k].R, p9, strip6, diag3, xr, l, d2);
            ekfm::match2_offer(match[k], d2, i, regular, a.e[k].gate);
            ekfm::cand_offer(sel[k], d2, i, regular, a.e[k].gate);
        }
        for (int q = (int)sel[k].n; q < ekfm::kAssignCand; ++q) { sel[k].idx[q] = -1; sel[k].d2[q] = INFINITY; }
    }

    // the launches, in the stream's order
    memset(&out, 0xff, sizeof out);                           // (nothing that is read may come from an earlier case)
    threadIdx.x = 0;
    for (int b = 0; b < m; ++b) { blockIdx.x = b; k_joint_search_prepare(st, a, sel.data(), (const int64_t *)match.data(), &store, &out); }
    JointSearchArgs sa = JointSearchArgs();
    sa.N = N; sa.m = m; sa.cur = a.cur; sa.npend = pending; sa.pstart = 0;
    for (int k = 0; k < m; ++k) {
        sa.level = la.level = k;
        for (int b = 0; b < kJointSearchExt; ++b) { blockIdx.x = b; k_joint_search_extend<TS>(st, sa, sel.data(), &store); }
        blockIdx.x = 0;
        k_joint_search_select(la, sel.data(), &store, &out);
    }

    int bad = 0;
    const JointSearchResult &r = out.res;
    if (r.nalive < 1 || r.nalive > beam) { printf("  nalive %d outside 1 .. beam\n", r.nalive); return 1000; }
    // every alive hypothesis: its d2 is k_joint_innovation's prefix at the last scan index, bit for bit; behind nalive -1 and NaN
    for (int s = 0; s < kJointSearchBeam; ++s) {
        const int64_t *hyp = out.alive_hyp + (size_t)s * m;
        if (s >= r.nalive) {
            for (int k = 0; k < m; ++k) bad += hyp[k] != -1;
            bad += out.alive_d2[s] == out.alive_d2[s];
            continue;
        }
        JointRecord rec;
        std::vector<double> prefix(m);
        blockIdx.x = 0; threadIdx.x = 0;
        k_joint_innovation<TS>(st, a, hyp, &rec, prefix.data(), nullptr, nullptr);
        if (memcmp(&prefix[m - 1], &out.alive_d2[s], 8)) { printf("  alive %d: d2 %.17g against k_joint_innovation's %.17g\n", s, out.alive_d2[s], prefix[m - 1]); ++bad; }
        if (s == 0) {
            bad += memcmp(&r.d2, &prefix[m - 1], 8) != 0 || r.dof != rec.dof || r.pairings != rec.pairings;
            for (int k = 0; k < m; ++k) bad += r.lm[k] != hyp[k];
        }
    }
    for (int k = m; k < kJointMax; ++k) bad += r.lm[k] != -1 || r.tested[k] != 0 || r.survived[k] != 0;
    // the lists and the records came back as they were given
    for (int k = 0; k < m; ++k) {
        bad += memcmp(out.match + 6 * k, &match[k], sizeof(ekfm::Match2)) != 0;
        bad += memcmp(out.cand + (size_t)k * kAssignCandidates, sel[k].idx, sizeof sel[k].idx) != 0;
        bad += memcmp(out.cand_d2 + (size_t)k * kAssignCandidates, sel[k].d2, sizeof sel[k].d2) != 0;
    }
    // nothing of the state was written
    bad += differ(S.x[0], before.x[0], "x") + differ(S.x[1], before.x[1], "x (other buffer)") + differ(S.strip[0], before.strip[0], "strip") +
           differ(S.strip[1], before.strip[1], "strip (other buffer)") + differ(S.prr[0], before.prr[0], "prr") + differ(S.prr[1], before.prr[1], "prr (other)") +
           differ(S.diag[0], before.diag[0], "diag") + differ(S.diag[1], before.diag[1], "diag (other buffer)") + differ(S.tiles, before.tiles, "tiles") +
           differ(S.ring, before.ring, "ring") + differ(S.s, before.s, "s") + differ(S.small, before.small, "small");

    // the dense state the search saw, and what it found
    std::vector<double> xd(S.x[S.cur].begin(), S.x[S.cur].begin() + n), Pd((size_t)n * n, 0.0);
    for (int rr = 0; rr < n; ++rr) for (int c = 0; c <= rr; ++c) {
        double v;
        if (rr < 3) v = S.prr[S.cur][3 * rr + c];
        else if (c < 3) v = S.strip[S.cur][c * S.ldm + (rr - 3)];
        else v = S.live(rr - 3, c - 3, pending);
        Pd[(size_t)rr * n + c] = Pd[(size_t)c * n + rr] = v;
    }
    const double head[2] = { (double)n, (double)m };
    put(f, head, 2); put(f, xd.data(), xd.size()); put(f, Pd.data(), Pd.size());
    std::vector<double> res;
    for (int k = 0; k < m; ++k) res.push_back((double)r.lm[k]);
    for (double v : { r.d2, (double)r.dof, (double)r.pairings, (double)r.truncated, (double)r.nalive, (double)r.irregular }) res.push_back(v);
    for (int k = 0; k < m; ++k) res.push_back((double)r.tested[k]);
    for (int k = 0; k < m; ++k) res.push_back((double)r.survived[k]);
    for (int s = 0; s < kJointSearchBeam; ++s) res.push_back(out.alive_d2[s]);
    res.push_back((double)bad);
    put(f, res.data(), res.size());
    printf("case %d: N = %d, m = %d, beam %d, %d pending, %s tiles: d2 = %.6g, %d pairings, nalive %d, truncated %d, irregular %d: %d differences\n", index, N, m,
           beam, pending, sizeof(TS) == 4 ? "float" : "F64", r.d2, r.pairings, r.nalive, r.truncated, r.irregular, bad);
    return bad;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    FILE *g = fopen(argv[1], "rb");
    if (!g) return 2;
    fseek(g, 0, SEEK_END);
    const long bytes = ftell(g);
    fseek(g, 0, SEEK_SET);
    std::vector<double> raw(bytes / 8);
    if (fread(raw.data(), 8, raw.size(), g) != raw.size()) return 2;
    fclose(g);
    FILE *f = fopen(argv[2], "wb");
    if (!f) return 2;
    const double *in = raw.data();
    const int ncases = (int)*in++;
    int bad = 0;
    for (int c = 0; c < ncases; ++c) bad += in[4] != 0.0 ? run_case<float>(in, f, c) : run_case<double>(in, f, c);
    fclose(f);
    return bad != 0;
}
