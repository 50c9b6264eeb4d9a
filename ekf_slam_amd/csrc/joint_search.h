// Fragment of kernels.hip (included there, inside its anonymous namespace, after joint.h): the joint-compatibility search over a scan
// (ekf_joint_search): k_joint_search_prepare, k_joint_search_extend, k_joint_search_select.
#pragma once

// ---------------------------------------------------------------------------------------------------
// The level-synchronous branch and bound that measure_model_joint walks on the host -- one ekf_joint_innovation call per level, every
// hypothesis factored from scratch -- as launches ordered by the stream behind k_assign_candidates / k_assign_select, with nothing read
// by the host in between.  Nothing of the state is written; no atomics, no flags, no grid-wide barrier: within one launch no workgroup
// reads what another writes.
//
// k_joint_search_prepare, one wavefront per scan entry: ekfm::joint_pairing for the entry's first kJointSearchCand candidates, read from
// the list k_assign_select left (the operands depend on (entry, candidate) alone: once per call, never per extension); the lists and
// the match records copied into the block that goes back; workgroup 0 starts the result block and the empty hypothesis.
//
// Per scan index k, two launches.
// k_joint_search_extend<TS>, one wavefront per (alive parent b, candidate c), a fixed grid of kJointSearchExt: workgroups beyond the alive
// count the select before left on the device, beyond the entry's candidates, or naming a landmark the parent uses return at once.  The
// others gather the parent's factor rows from its ancestors' nodes into LDS, form the new pairing's S row blocks -- one lane per earlier
// pairing: pmm_low_chain and ekfm::joint_cross_block, k_joint_innovation's operands and text -- and append two rows
// (ekfm::joint_append_*), so the d2 is k_joint_innovation's prefix for that hypothesis bit for bit.  "Left out" appends nothing and needs
// no workgroup.
// k_joint_search_select, ONE workgroup, a lane per (parent, extension slot 0..4): the test against threshold[dof], the rank of every
// survivor by counting the survivors in front of it (ekfm::joint_search_before), the next level's nodes, the counters; at the last
// level the winner and the final beam.
// LDS: extend 32 KiB for the parent's factor and 2.6 KiB of rows; select 16 KiB of parents' hypotheses and 8 KiB of keys.
// ---------------------------------------------------------------------------------------------------
#ifdef EKF_JOINT_SEARCH_LANES                                   // (a host emulation runs the kernels with ONE lane: every phase is a loop strided by the lane count)
constexpr int kJointSearchBlock = EKF_JOINT_SEARCH_LANES, kJointSearchSelectBlock = EKF_JOINT_SEARCH_LANES;
#else
constexpr int kJointSearchBlock = 64;
constexpr int kJointSearchSelectBlock = kJointSearchSlots;      // 320
#endif

__global__ __launch_bounds__(kJointSearchBlock) void k_joint_search_prepare(DevState st, JointArgs a, const ekfm::CandList *__restrict__ sel,
                                                                            const int64_t *__restrict__ match,
                                                                            JointSearchStore *__restrict__ store, JointSearchOut *__restrict__ out) {
    const int tid = threadIdx.x;
    const int k = blockIdx.x;
    const ekfm::CandList &list = sel[k];
    const int nc = list.n < kJointSearchCand ? (int)list.n : kJointSearchCand;
    for (int c = tid; c < nc; c += kJointSearchBlock) {
        const AssocModelEntry &e = a.e[k];
        const int cur = a.cur;
        const int64_t i = list.idx[c];
        const double *__restrict__ x = st.x[cur];
        const double *__restrict__ strip = st.strip[cur] + 2 * i;
        const double *__restrict__ dg = st.diag[st.dcur] + 3 * i;
        const int64_t ldm = st.ldm;
        double p9[9];
        for (int q = 0; q < 9; ++q) p9[q] = st.prr[cur][q];
        const double xr[3] = { x[0], x[1], x[2] };
        const double l[2] = { x[3 + 2 * i], x[4 + 2 * i] };
        const double strip6[6] = { strip[0], strip[1], strip[ldm], strip[ldm + 1], strip[2 * ldm], strip[2 * ldm + 1] };
        const double diag3[3] = { dg[0], dg[1], dg[2] };
        double S[4], nu[2], hr[6], ht[4];
        const bool posed = ekfm::joint_pairing(e.model, e.z, e.R, p9, strip6, diag3, xr, l, hr, ht, S, nu);
        JointSearchOperand &o = store->op[k * kJointSearchCand + c];
        for (int q = 0; q < 6; ++q) { o.Hr[q] = hr[q]; o.strip[q] = strip6[q]; }
        for (int q = 0; q < 4; ++q) { o.Ht[q] = ht[q]; o.S[q] = S[q]; }
        o.nu[0] = nu[0]; o.nu[1] = nu[1];
        o.lm = i; o.posed = posed ? 1 : 0; o.pad = 0;
    }
    for (int f = tid; f < kAssignCandidates; f += kJointSearchBlock) {
        out->cand[k * kAssignCandidates + f] = list.idx[f];
        out->cand_d2[k * kAssignCandidates + f] = list.d2[f];
    }
    for (int q = tid; q < 6; q += kJointSearchBlock) out->match[k * 6 + q] = match[k * 6 + q];
    if (k == 0) {
        for (int q = tid; q < kJointMax; q += kJointSearchBlock) { out->res.lm[q] = -1; out->res.tested[q] = 0; out->res.survived[q] = 0; }
        if (tid == 0) {
            out->res.d2 = 0.0; out->res.dof = 0; out->res.pairings = 0; out->res.truncated = 0; out->res.nalive = 0; out->res.irregular = 0;
            store->nalive[0] = 1;
            JointSearchNode &root = store->node[0];
            root.d2 = 0.0; root.dof = 0; root.pairings = 0;
        }
    }
}

template <typename TS>
__global__ __launch_bounds__(kJointSearchBlock) void k_joint_search_extend(DevState st, JointSearchArgs a, const ekfm::CandList *__restrict__ sel,
                                                                           JointSearchStore *__restrict__ store) {
    __shared__ double L[kJointRows * kJointRows];
    __shared__ double y[kJointRows];
    __shared__ double a0[kJointSearchRow], a1[kJointSearchRow], l0[kJointSearchRow], l1[kJointSearchRow];
    __shared__ double prr[9];
    __shared__ int scan_of[kJointMax];
    __shared__ int used, regular;
    constexpr int ld = kJointRows;
    const int tid = threadIdx.x;
    const int k = a.level;
    const int b = blockIdx.x / kJointSearchCand, c = blockIdx.x % kJointSearchCand;
    if (b >= store->nalive[k]) return;
    const ekfm::CandList &list = sel[k];
    const int nc = list.n < kJointSearchCand ? (int)list.n : kJointSearchCand;
    if (c >= nc) return;
    const JointSearchNode &parent = store->node[k * kJointSearchBeam + b];
    const JointSearchOperand &on = store->op[k * kJointSearchCand + c];
    const int64_t lm = on.lm;
    if (tid == 0) used = 0;
    __syncthreads();
    for (int j = tid; j < k; j += kJointSearchBlock) {
        const int64_t hj = parent.hyp[j];
        if (hj == lm) used = 1;                               // (every writer stores the same value)
        if (hj >= 0) {
            int p = 0;
            for (int q = 0; q < j; ++q) p += parent.hyp[q] >= 0;
            scan_of[p] = j;
        }
    }
    for (int q = tid; q < 9; q += kJointSearchBlock) prr[q] = st.prr[a.cur][q];
    __syncthreads();
    if (used) return;                                         // uniform
    const int np = parent.pairings, i0 = 2 * np;

    // the parent's factor and y: pairing p's two rows lie in the node of its scan index's level, at the ancestor's slot
    for (int e = tid; e < np * 2 * kJointSearchBlock; e += kJointSearchBlock) {
        const int p = e / (2 * kJointSearchBlock), r = (e / kJointSearchBlock) & 1;
        const int s = scan_of[p], i = 2 * p + r;
        const double *__restrict__ src = store->node[(s + 1) * kJointSearchBeam + parent.anc[s]].row[r];
        for (int j = e % kJointSearchBlock; j <= i + 1; j += kJointSearchBlock) {
            if (j <= i) L[i * ld + j] = src[j];
            else y[i] = src[j];
        }
    }
    // the new rows' S entries: the cross blocks against the parent's pairings, then the pairing's own block and nu
    for (int pb = tid; pb < np; pb += kJointSearchBlock) {
        const int s = scan_of[pb];
        const JointSearchOperand &ob = store->op[s * kJointSearchCand + parent.slot[s]];
        const int64_t ra = 2 * lm, rb = 2 * ob.lm;
        double pab[4], Sab[4];
        for (int q = 0; q < 4; ++q) pab[q] = pmm_low_chain<TS>(st, a.pstart, a.npend, ra + (q >> 1), rb + (q & 1));
        ekfm::joint_cross_block(on.Hr, on.Ht, ob.Hr, ob.Ht, prr, on.strip, ob.strip, pab, Sab);
        a0[2 * pb] = Sab[0]; a0[2 * pb + 1] = Sab[1];
        a1[2 * pb] = Sab[2]; a1[2 * pb + 1] = Sab[3];
    }
    if (tid == 0) {
        a0[i0] = on.S[0]; a0[i0 + 1] = on.nu[0];
        a1[i0] = on.S[2]; a1[i0 + 1] = on.S[3]; a1[i0 + 2] = on.nu[1];
        regular = 0;
    }
    __syncthreads();
    // (uniform.  A pairing that is not posed has no d2 -- but it has no individual d2 either, so k_assign_candidates never lists its landmark:
    // through ekf_joint_search the branch is never false.  It is kept because the operand record carries the flag and a NaN costs nothing.)
    if (on.posed) {
        for (int q = 0; q < i0; ++q) {
            ekfm::joint_append_step(L, ld, y, a0, a1, l0, l1, i0, q, tid, kJointSearchBlock);
            __syncthreads();
        }
        if (tid == 0) regular = ekfm::joint_append_close(a0, a1, l0, l1, i0) ? 1 : 0;
        __syncthreads();
    }
    JointSearchExt &x = store->ext[blockIdx.x];
    if (regular) {
        for (int j = tid; j <= i0 + 2; j += kJointSearchBlock) {
            if (j <= i0 + 1) x.row[0][j] = l0[j];
            x.row[1][j] = l1[j];
        }
    }
    if (tid == 0) x.d2 = regular ? ekfm::joint_prefix_add(parent.d2, l0[i0 + 1], l1[i0 + 2]) : NAN;
}

__global__ __launch_bounds__(kJointSearchSelectBlock) void k_joint_search_select(JointSearchLevelArgs a, const ekfm::CandList *__restrict__ sel,
                                                                                 JointSearchStore *__restrict__ store,
                                                                                 JointSearchOut *__restrict__ out) {
    __shared__ long long ph[kJointSearchBeam * kJointMax];    // the parents' hypotheses
    __shared__ double pd2[kJointSearchBeam];
    __shared__ int pdof[kJointSearchBeam], ppair[kJointSearchBeam];
    __shared__ double ed2[kJointSearchSlots];
    __shared__ long long elm[kJointSearchSlots];
    __shared__ int epair[kJointSearchSlots], edof[kJointSearchSlots], eflag[kJointSearchSlots];     // 1 formed, 2 passed, 4 irregular
    __shared__ int taken[kJointSearchBeam];                   // by rank: the extension
    constexpr int kSlots = kJointSearchCand + 1;
    const int tid = threadIdx.x;
    const int k = a.level, m = a.m;
    const int na = store->nalive[k];
    const ekfm::CandList &list = sel[k];
    const int nc = list.n < kJointSearchCand ? (int)list.n : kJointSearchCand;
    const JointSearchNode *__restrict__ parents = store->node + k * kJointSearchBeam;
    JointSearchNode *__restrict__ next = store->node + (k + 1) * kJointSearchBeam;

    for (int s = tid; s < na; s += kJointSearchSelectBlock) { pd2[s] = parents[s].d2; pdof[s] = parents[s].dof; ppair[s] = parents[s].pairings; }
    int nn = na, tested = 0, survived = 0, irregular = 0;
    bool cut = false;
    if (nc == 0) {
        // an entry without candidates: every parent goes on, left out, in the order it stands in -- nothing tested, nothing ranked
        __syncthreads();
        for (int s = tid; s < na; s += kJointSearchSelectBlock) {
            const int t = s * kSlots + kJointSearchCand;
            ed2[t] = pd2[s]; elm[t] = -1; epair[t] = ppair[s]; edof[t] = pdof[s];
            taken[s] = t;
        }
    } else {
        for (int e = tid; e < na * kJointMax; e += kJointSearchSelectBlock) ph[e] = parents[e / kJointMax].hyp[e % kJointMax];
        __syncthreads();
        // every extension: formed, tested against its threshold
        for (int t = tid; t < kJointSearchSlots; t += kJointSearchSelectBlock) {
            const int b = t / kSlots, c = t % kSlots;
            const bool pairing = c < kJointSearchCand;
            const long long lm = pairing && c < nc ? list.idx[c] : -1;
            bool formed = b < na && (!pairing || c < nc);
            if (formed && pairing)
                for (int j = 0; j < k; ++j) formed = formed && ph[b * kJointMax + j] != lm;
            double d2 = NAN;
            int dof = 0, pairings = 0;
            if (formed) {
                d2 = pairing ? store->ext[b * kJointSearchCand + c].d2 : pd2[b];
                dof = pdof[b] + (pairing ? a.rows[k] : 0);
                pairings = ppair[b] + (pairing ? 1 : 0);
            }
            const bool passed = formed && ekfm::joint_search_passes(d2, a.threshold[dof]);
            ed2[t] = d2; elm[t] = lm; epair[t] = pairings; edof[t] = dof;
            eflag[t] = (formed ? 1 : 0) | (passed ? 2 : 0) | (formed && d2 != d2 ? 4 : 0);
        }
        __syncthreads();
        // the counters, and per survivor the survivors in front of it
        for (int j = 0; j < kJointSearchSlots; ++j) {
            const int f = eflag[j];
            tested += f & 1; survived += (f >> 1) & 1; irregular += (f >> 2) & 1;
        }
        nn = ekfm::joint_search_cut(survived, a.beam, cut);
        for (int t = tid; t < kJointSearchSlots; t += kJointSearchSelectBlock) {
            if (!(eflag[t] & 2)) continue;
            int rank = 0;
            for (int j = 0; j < kJointSearchSlots; ++j)
                if ((eflag[j] & 2) && j != t)
                    rank += ekfm::joint_search_before(epair[j], ed2[j], ph + (j / kSlots) * kJointMax, elm[j], epair[t], ed2[t],
                                                      ph + (t / kSlots) * kJointMax, elm[t], k) ? 1 : 0;
            if (rank < nn) taken[rank] = t;
        }
    }
    __syncthreads();

    // the next level's nodes
    for (int e = tid; e < nn * kJointSearchBlock; e += kJointSearchSelectBlock) {
        const int s = e / kJointSearchBlock;
        const int src = taken[s], sb = src / kSlots, sc = src % kSlots;
        JointSearchNode &n = next[s];
        for (int j = e % kJointSearchBlock; j <= k; j += kJointSearchBlock) {
            if (j < k) { n.hyp[j] = parents[sb].hyp[j]; n.anc[j] = parents[sb].anc[j]; n.slot[j] = parents[sb].slot[j]; }
            else { n.hyp[j] = elm[src]; n.anc[j] = s; n.slot[j] = sc < kJointSearchCand ? sc : -1; }
        }
        if (e % kJointSearchBlock == 0) { n.d2 = ed2[src]; n.dof = edof[src]; n.pairings = epair[src]; }
        if (sc < kJointSearchCand) {
            const JointSearchExt &x = store->ext[sb * kJointSearchCand + sc];
            const int i0 = 2 * ppair[sb];
            for (int q = e % kJointSearchBlock; q <= i0 + 2; q += kJointSearchBlock) {
                if (q <= i0 + 1) n.row[0][q] = x.row[0][q];
                n.row[1][q] = x.row[1][q];
            }
        }
    }
    if (tid == 0) {
        store->nalive[k + 1] = nn;
        store->nirregular[k + 1] = (k ? store->nirregular[k] : 0) + irregular;     // (a sum kept per level: a repeated launch leaves the same)
        out->res.tested[k] = tested;
        out->res.survived[k] = survived;
        if (cut) out->res.truncated = 1;
        out->res.irregular = store->nirregular[k + 1];
    }
    if (k + 1 < m) return;

    // the last level: the winner and the final beam
    for (int e = tid; e < kJointSearchBeam * m; e += kJointSearchSelectBlock) {
        const int s = e / m, j = e % m;
        long long v = -1;
        if (s < nn) {
            const int src = taken[s];
            v = j < k ? parents[src / kSlots].hyp[j] : elm[src];
        }
        out->alive_hyp[e] = v;
        if (s == 0) out->res.lm[j] = v;
    }
    for (int s = tid; s < kJointSearchBeam; s += kJointSearchSelectBlock) out->alive_d2[s] = s < nn ? ed2[taken[s]] : NAN;
    if (tid == 0 && nn > 0) {                                 // (there is always one: the all-left-out hypothesis passes threshold[0] >= 0)
        const int src = taken[0];
        out->res.d2 = ed2[src]; out->res.dof = edof[src]; out->res.pairings = epair[src]; out->res.nalive = nn;
    }
}
