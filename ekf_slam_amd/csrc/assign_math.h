// The arithmetic of ekf_assign_model that host and device share (included beside device_math.h; tests/support/assign_model_host.cpp builds it
// for the host): a bounded candidate list under the total order (d2, index), and the assignment solver over m such lists.
#pragma once
#include "device_math.h"

// a lambda handed to a Team is part of the loop it stands in: inlined, so that what it captures stays in registers
#define EKF_TEAM_STEP __attribute__((always_inline))

namespace ekfm {

constexpr int kAssignMax = 32;                              // observations per scan (EKF_ASSIGN_MODEL_MAX)
constexpr int kAssignCand = 32;                             // candidates kept per observation (EKF_ASSIGN_CANDIDATES)
constexpr int kAssignEdges = kAssignMax * kAssignCand;      // kept pairs, and so the most distinct landmarks among them
constexpr int kAssignCols = kAssignEdges + kAssignMax;      // ... and one private "left out" column per observation behind them

// ---------------------------------------------------------------------------------------------------
// The candidate list: the first kAssignCand of a set of (d2, index) keys in match2_before's order -- smaller d2 first, the lower index on
// equal d2 -- kept sorted.  The order is total and no index occurs twice, so the first kAssignCand of a union are the first kAssignCand of
// the union of the parts' first kAssignCand: cand_merge is associative and commutative, and a lane, a workgroup, the grid and the host
// reach the same list whatever the shape of the reduction.  Both operations place a key by cand_rank, the number of keys in front of it:
// that count is all a parallel merge needs (a key's place in the union is the sum of its ranks in the parts).
// ---------------------------------------------------------------------------------------------------
struct CandList {
    long long n, pad;                 // entries in use
    long long idx[kAssignCand];
    double d2[kAssignCand];
};
EKF_MHD void cand_init(CandList &c) { c.n = 0; c.pad = 0; }
// how many of the n keys (kd2, kidx) come before (d2, i); a key with a negative index is no key
EKF_MHD int cand_rank(const double *kd2, const long long *kidx, int n, double d2, long long i) {
    int r = 0;
    for (int j = 0; j < n; ++j) r += match2_before(kd2[j], kidx[j], d2, i) ? 1 : 0;
    return r;
}
// landmark i with its d2, as match2_offer takes it: a candidate where it has a d2 and d2 <= gate
EKF_MHD void cand_offer(CandList &c, double d2, long long i, bool regular, double gate) {
    if (!regular || !(d2 <= gate)) return;
    const int n = (int)c.n, at = cand_rank(c.d2, c.idx, n, d2, i);
    if (at >= kAssignCand) return;
    const int last = n < kAssignCand ? n : kAssignCand - 1;
    for (int s = last; s > at; --s) { c.d2[s] = c.d2[s - 1]; c.idx[s] = c.idx[s - 1]; }
    c.d2[at] = d2; c.idx[at] = i;
    c.n = n < kAssignCand ? n + 1 : kAssignCand;
}
// the first kAssignCand of the union: every entry goes to (its place in its own list) + (its rank in the other)
EKF_MHD CandList cand_merge(const CandList &a, const CandList &b) {
    CandList r;
    cand_init(r);
    const int na = (int)a.n, nb = (int)b.n;
    for (int s = 0; s < na; ++s) {
        const int at = s + cand_rank(b.d2, b.idx, nb, a.d2[s], a.idx[s]);
        if (at < kAssignCand) { r.d2[at] = a.d2[s]; r.idx[at] = a.idx[s]; }
    }
    for (int s = 0; s < nb; ++s) {
        const int at = s + cand_rank(a.d2, a.idx, na, b.d2[s], b.idx[s]);
        if (at < kAssignCand) { r.d2[at] = b.d2[s]; r.idx[at] = b.idx[s]; }
    }
    r.n = na + nb < kAssignCand ? na + nb : kAssignCand;
    return r;
}

// ---------------------------------------------------------------------------------------------------
// The solver.  Rows are the m observations; row k's edges are its n[k] kept candidates (landmark idx[k * kAssignCand + s], cost d2[..]) and
// one private column kAssignEdges + k at cost gate[k]: "left out".  Landmarks shared between rows are one column: the column of an edge is
// the flat number of the FIRST edge (in row-major order) that names its landmark, so column numbers need no compaction; the columns in use are
// listed once (act), and the searches scan that list alone.
//
// Shortest augmenting paths with column prices v (Jonker-Volgenant's augmentation, no initialisation phases), rows in scan order, all in
// F64.  For row i: a Dijkstra search over the columns from i to the nearest free column -- dist[j] the reduced length of the best path
// found so far, pred[j] the edge it ends with -- in which every step relaxes the <= kAssignCand + 1 edges of ONE row and then takes the
// arg-min of dist over the columns in use that are not yet scanned, under the total order (dist, column).  Then v[j] += dist[j] - dist[last] over the
// scanned columns and the path is flipped.  The private column of row i is free until i itself takes it, so the search always ends.
//
// Every loop over edges or columns is strided over (lane, nlanes) and no two lanes of a step write one address (the edges of a row lie in
// distinct columns); the one cross-lane step is the arg-min, whose order is total.  So the result does not depend on nlanes: the host runs
// this text with a team of 1 (or an emulated 64), k_assign_solve with the 64 lanes of one wavefront.  A Team supplies
//   each(f)    f(lane, nlanes) on every lane, then all lanes' writes visible to all
//   argmin(f)  assign_min_merge over every lane's f(lane, nlanes), the same value returned to all
// ---------------------------------------------------------------------------------------------------
struct AssignProblem {
    long long idx[kAssignEdges];      // in: the kept lists, row k at k * kAssignCand
    double d2[kAssignEdges];
    long long n[kAssignMax];          // in: entries in use per row
    double gate[kAssignMax];          // in: the price of leaving row k out (finite)
    int m, pad;                       // in: rows
    int col[kAssignEdges];            // an edge's column
    double v[kAssignCols], dist[kAssignCols];
    int pred[kAssignCols];            // the edge a column was reached by (private columns: not used, their one edge is known)
    int own[kAssignCols];             // the edge a column is assigned by, -1: free; a private column: its row or -1
    unsigned char done[kAssignCols];
    int act[kAssignCols];             // the columns in use: one per distinct landmark (in row-major order of their first edge), then the
    int nact;                         //   private ones -- the searches scan these and no others
    int rowcnt[kAssignMax];           // columns that row k's edges are the first to name
    int rowcol[kAssignMax];           // out: the column row k is assigned to
};
struct AssignMin { double d; int j; };
EKF_MHD AssignMin assign_min_merge(const AssignMin &a, const AssignMin &b) {
    const bool a_first = a.j >= 0 && (b.j < 0 || a.d < b.d || (a.d == b.d && a.j < b.j));
    AssignMin r;                      // (field by field: a select between the two objects would go through their addresses)
    r.d = a_first ? a.d : b.d;
    r.j = a_first ? a.j : b.j;
    return r;
}
// edge s of row k (s == n[k]: the private one): its column and its cost
EKF_MHD int assign_edge_col(const AssignProblem &p, int k, int s) { return s < (int)p.n[k] ? p.col[k * kAssignCand + s] : kAssignEdges + k; }
EKF_MHD double assign_edge_cost(const AssignProblem &p, int k, int s) { return s < (int)p.n[k] ? p.d2[k * kAssignCand + s] : p.gate[k]; }
// ... and of the edge a column is owned by
EKF_MHD int assign_owner_row(const AssignProblem &p, int j) { return j < kAssignEdges ? p.own[j] / kAssignCand : p.own[j]; }
EKF_MHD double assign_owner_cost(const AssignProblem &p, int j) { return j < kAssignEdges ? p.d2[p.own[j]] : p.gate[p.own[j]]; }

// the columns of the edges: the first edge that names the landmark
EKF_MHD void assign_columns(AssignProblem &p, int lane, int nlanes) {
    for (int f = lane; f < p.m * kAssignCand; f += nlanes) {
        const int k = f / kAssignCand, s = f % kAssignCand;
        if (s >= (int)p.n[k]) continue;
        int c = f;
        for (int k2 = 0; k2 < k && c == f; ++k2)
            for (int s2 = 0; s2 < (int)p.n[k2]; ++s2)
                if (p.idx[k2 * kAssignCand + s2] == p.idx[f]) { c = k2 * kAssignCand + s2; break; }
        p.col[f] = c;
    }
    for (int j = lane; j < kAssignCols; j += nlanes) { p.v[j] = 0.0; p.own[j] = -1; }
    for (int k = lane; k < p.m; k += nlanes) p.rowcol[k] = -1;
}
// ... counted per row (after assign_columns), and listed (after the counts): rows write behind the rows in front of them, so the list
// is the same for every number of lanes
EKF_MHD void assign_count_columns(AssignProblem &p, int lane, int nlanes) {
    for (int k = lane; k < p.m; k += nlanes) {
        int c = 0;
        for (int s = 0; s < (int)p.n[k]; ++s) c += p.col[k * kAssignCand + s] == k * kAssignCand + s ? 1 : 0;
        p.rowcnt[k] = c;
    }
}
EKF_MHD void assign_list_columns(AssignProblem &p, int lane, int nlanes) {
    int total = 0;
    for (int k = 0; k < p.m; ++k) total += p.rowcnt[k];
    for (int k = lane; k < p.m; k += nlanes) {
        int at = 0;
        for (int k2 = 0; k2 < k; ++k2) at += p.rowcnt[k2];
        for (int s = 0; s < (int)p.n[k]; ++s)
            if (p.col[k * kAssignCand + s] == k * kAssignCand + s) p.act[at++] = k * kAssignCand + s;
        p.act[total + k] = kAssignEdges + k;
    }
    if (lane == 0) p.nact = total + p.m;
}

template <class Team>
EKF_MHD void assign_solve(AssignProblem &p, Team &t) {
    t.each([&](int lane, int nlanes) EKF_TEAM_STEP { assign_columns(p, lane, nlanes); });
    t.each([&](int lane, int nlanes) EKF_TEAM_STEP { assign_count_columns(p, lane, nlanes); });
    t.each([&](int lane, int nlanes) EKF_TEAM_STEP { assign_list_columns(p, lane, nlanes); });
    const int nact = p.nact;
    for (int i = 0; i < p.m; ++i) {
        if (p.n[i] == 0) {
            // a row without a candidate has one edge, to its private column, which is free: what the search below would find, with no
            // price moved (dist = dmin there)
            t.each([&](int lane, int) EKF_TEAM_STEP { if (lane == 0) { p.rowcol[i] = kAssignEdges + i; p.own[kAssignEdges + i] = i; } });
            continue;
        }
        t.each([&](int lane, int nlanes) EKF_TEAM_STEP {
            for (int q = lane; q < nact; q += nlanes) { const int j = p.act[q]; p.dist[j] = INFINITY; p.done[j] = 0; }
        });
        int cur = i, last;
        double h = 0.0, dmin;
        for (;;) {
            t.each([&](int lane, int nlanes) EKF_TEAM_STEP {
                for (int s = lane; s <= (int)p.n[cur]; s += nlanes) {
                    const int j = assign_edge_col(p, cur, s);
                    if (p.done[j]) continue;
                    const double nd = (assign_edge_cost(p, cur, s) - p.v[j]) - h;
                    if (nd < p.dist[j]) { p.dist[j] = nd; p.pred[j] = cur * kAssignCand + s; }
                }
            });
            const AssignMin best = t.argmin([&](int lane, int nlanes) EKF_TEAM_STEP {
                AssignMin a = { INFINITY, -1 };
                for (int q = lane; q < nact; q += nlanes) {
                    const int j = p.act[q];
                    if (!p.done[j] && p.dist[j] < INFINITY) a = assign_min_merge(a, AssignMin{ p.dist[j], j });
                }
                return a;
            });
            last = best.j; dmin = best.d;
            if (last < 0) break;                      // (cannot happen: row i's private column is free and reached)
            const bool is_free = p.own[last] < 0;
            t.each([&](int lane, int) EKF_TEAM_STEP { if (lane == 0) p.done[last] = 1; });
            if (is_free) break;
            cur = assign_owner_row(p, last);
            h = (assign_owner_cost(p, last) - p.v[last]) - dmin;
        }
        if (last < 0) { t.each([&](int lane, int) EKF_TEAM_STEP { if (lane == 0) p.rowcol[i] = -1; }); continue; }
        t.each([&](int lane, int nlanes) EKF_TEAM_STEP {
            for (int q = lane; q < nact; q += nlanes) { const int j = p.act[q]; if (p.done[j]) p.v[j] += p.dist[j] - dmin; }
        });
        // the path flipped, from the free column back to row i: each column goes to the row it was reached from
        t.each([&](int lane, int) EKF_TEAM_STEP {
            if (lane != 0) return;
            int j = last;
            for (;;) {
                const int r = j < kAssignEdges ? p.pred[j] / kAssignCand : j - kAssignEdges;
                p.own[j] = j < kAssignEdges ? p.pred[j] : r;
                const int before = r == i ? -1 : p.rowcol[r];
                p.rowcol[r] = j;
                if (r == i) break;
                j = before;
            }
        });
    }
}

// the host's team: the lanes one after the other
struct AssignHostTeam {
    int nlanes;
    template <class F> void each(F f) { for (int l = 0; l < nlanes; ++l) f(l, nlanes); }
    template <class F> AssignMin argmin(F f) {
        AssignMin a = { INFINITY, -1 };
        for (int l = 0; l < nlanes; ++l) a = assign_min_merge(a, f(l, nlanes));
        return a;
    }
};

// What the call returns for row k once the solver has run: the landmark (or -1) and the pair's d2 (or +inf); and J summed in scan order.
EKF_MHD long long assign_landmark(const AssignProblem &p, int k) {
    const int j = p.rowcol[k];
    return j >= 0 && j < kAssignEdges ? p.idx[p.own[j]] : -1;
}
EKF_MHD double assign_d2(const AssignProblem &p, int k) {
    const int j = p.rowcol[k];
    return j >= 0 && j < kAssignEdges ? p.d2[p.own[j]] : INFINITY;
}
EKF_MHD double assign_total(const AssignProblem &p) {
    double J = 0.0;
    for (int k = 0; k < p.m; ++k) {
        const int j = p.rowcol[k];
        J += j >= 0 && j < kAssignEdges ? p.d2[p.own[j]] : p.gate[k];
    }
    return J;
}

}  // namespace ekfm
