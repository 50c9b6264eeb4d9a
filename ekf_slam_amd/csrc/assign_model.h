// Fragment of kernels.hip (included there, inside its anonymous namespace, after associate_model.h): a scan assigned to the map one-to-one
// (ekf_assign_model): k_assign_candidates, k_assign_select, k_assign_solve.
#pragma once

// ---------------------------------------------------------------------------------------------------
// Three launches ordered by the stream, no atomics, no tickets, no fences.
//
// k_assign_candidates is k_assoc_model -- the same grid, the same operand loads, assoc_model_d2, match2_offer and the Match2 reduction --
// and in addition every workgroup leaves the up to kAssignCand best (d2, index) keys of its lanes INSIDE the gate, in order, in
// lists[k * gridDim.x + blockIdx.x].  Whether any lane is inside is known to all after the reduction's own barrier (a ballot per
// wavefront, stored beside its record); a workgroup with none stores n = 0 and is done: one uniform branch more than k_assoc_model.
// Otherwise the 256 keys go to LDS and every inside lane counts the keys in front of its own (ekfm::cand_rank): that rank is its place
// in the list, exact however many are inside, with no sort network and no divergent barrier.
//
// k_assign_select, one workgroup per observation, merges the workgroups' lists into the observation's first kAssignCand -- rounds of
// (the list so far) + 7 lists = 256 keys, placed by the same rank, rounds without a key skipped -- and the Match2 records into match[k].
//
// k_assign_solve, ONE wavefront, loads the m lists into LDS and runs ekfm::assign_solve (assign_math.h) with its 64 lanes as the team;
// out, total and the lists go to one result block.
// ---------------------------------------------------------------------------------------------------

constexpr int kAssignListsPerRound = kAssocBlock / ekfm::kAssignCand - 1;     // 7

// the lane's key (idx < 0: none) ranked among the workgroup's kAssocBlock keys; how many keys there are
__device__ __forceinline__ int assign_rank_block(double *kd2, long long *kidx, double d2, long long idx, int &count) {
    const int tid = threadIdx.x;
    kd2[tid] = d2; kidx[tid] = idx;
    __syncthreads();
    int r = 0, c = 0;
    for (int j = 0; j < kAssocBlock; ++j) {
        const double dj = kd2[j];
        const long long ij = kidx[j];
        r += ekfm::match2_before(dj, ij, d2, idx) ? 1 : 0;
        c += ij >= 0 ? 1 : 0;
    }
    count = c;
    return r;
}

__global__ __launch_bounds__(kAssocBlock) void k_assign_candidates(DevState st, AssocModelArgs a, ekfm::Match2 *__restrict__ partials,
                                                                   ekfm::CandList *__restrict__ lists) {
    __shared__ ekfm::Match2 wave_rec[kAssocBlock / 64];
    __shared__ int wave_in[kAssocBlock / 64];
    __shared__ double kd2[kAssocBlock];
    __shared__ long long kidx[kAssocBlock];
    const int tid = threadIdx.x;
    const int k = blockIdx.y;
    const AssocModelEntry &e = a.e[k];
    const int cur = a.cur;
    const int64_t i = (int64_t)blockIdx.x * kAssocBlock + tid;
    ekfm::Match2 m;
    ekfm::match2_init(m);
    double d2 = NAN;
    bool inside = false;
    if (i < a.N) {
        const double *__restrict__ x = st.x[cur];
        const double *__restrict__ strip = st.strip[cur] + 2 * i;
        const double *__restrict__ dg = st.diag[st.dcur] + 3 * i;
        const int64_t ldm = st.ldm;
        double prr[9];
        for (int q = 0; q < 9; ++q) prr[q] = st.prr[cur][q];
        const double xr[3] = { x[0], x[1], x[2] };
        const double l[2] = { x[3 + 2 * i], x[4 + 2 * i] };
        const double strip6[6] = { strip[0], strip[1], strip[ldm], strip[ldm + 1], strip[2 * ldm], strip[2 * ldm + 1] };
        const double diag3[3] = { dg[0], dg[1], dg[2] };
        const bool regular = ekfm::assoc_model_d2(e.model, e.z, e.R, prr, strip6, diag3, xr, l, d2);
        ekfm::match2_offer(m, d2, i, regular, e.gate);
        inside = regular && d2 <= e.gate;
    }
    m = match2_wave(m);
    const bool wave_any = __ballot(inside) != 0;
    if ((tid & 63) == 0) { wave_rec[tid >> 6] = m; wave_in[tid >> 6] = wave_any ? 1 : 0; }
    __syncthreads();
    ekfm::CandList &list = lists[(int64_t)k * gridDim.x + blockIdx.x];
    if (tid == 0) {
        ekfm::Match2 r = wave_rec[0];
        for (int w = 1; w < kAssocBlock / 64; ++w) r = ekfm::match2_merge(r, wave_rec[w]);
        partials[(int64_t)k * gridDim.x + blockIdx.x] = r;
    }
    int any = 0;
    for (int w = 0; w < kAssocBlock / 64; ++w) any |= wave_in[w];
    if (!any) {                                               // uniform: the common case
        if (tid == 0) list.n = 0;
        return;
    }
    int count;
    const int rank = assign_rank_block(kd2, kidx, d2, inside ? (long long)i : -1, count);
    if (inside && rank < ekfm::kAssignCand) { list.idx[rank] = i; list.d2[rank] = d2; }
    if (tid == 0) list.n = count < ekfm::kAssignCand ? count : ekfm::kAssignCand;
}

// sel[k] = the first kAssignCand of the union of lists[k * nblk .. + nblk); match[k] = the merge of partials[k * nblk .. + nblk)
__global__ __launch_bounds__(kAssocBlock) void k_assign_select(const ekfm::Match2 *__restrict__ partials, const ekfm::CandList *__restrict__ lists,
                                                               int nblk, ekfm::Match2 *__restrict__ match, ekfm::CandList *__restrict__ sel) {
    __shared__ double kd2[kAssocBlock];
    __shared__ long long kidx[kAssocBlock];
    __shared__ double acc_d2[ekfm::kAssignCand];
    __shared__ long long acc_idx[ekfm::kAssignCand];
    __shared__ int acc_n;
    __shared__ int round_any;
    const int tid = threadIdx.x;
    const int k = blockIdx.x;
    const ekfm::CandList *__restrict__ mine = lists + (int64_t)k * nblk;
    if (tid < 64) {                                           // the records: k_assoc_model_reduce on the first wavefront
        ekfm::Match2 m;
        ekfm::match2_init(m);
        for (int b = tid; b < nblk; b += 64) m = ekfm::match2_merge(m, partials[(int64_t)k * nblk + b]);
        m = match2_wave(m);
        if (tid == 0) { match[k] = m; acc_n = 0; }
    }
    const int slot = tid % ekfm::kAssignCand, which = tid / ekfm::kAssignCand - 1;      // which < 0: the list so far
    for (int b0 = 0; b0 < nblk; b0 += kAssignListsPerRound) {
        __syncthreads();                                      // acc_n, acc_* of the round before; round_any read by all
        if (tid == 0) round_any = 0;
        __syncthreads();
        double d2 = INFINITY;
        long long idx = -1;
        if (which < 0) {
            if (slot < acc_n) { d2 = acc_d2[slot]; idx = acc_idx[slot]; }
        } else if (b0 + which < nblk) {
            const ekfm::CandList &l = mine[b0 + which];
            if (slot < l.n) { d2 = l.d2[slot]; idx = l.idx[slot]; round_any = 1; }      // (every writer stores the same value)
        }
        __syncthreads();
        if (!round_any) continue;                             // uniform: no list of this round holds a key
        int count;
        const int rank = assign_rank_block(kd2, kidx, d2, idx, count);
        __syncthreads();                                      // every lane has read its entry of the list so far
        if (idx >= 0 && rank < ekfm::kAssignCand) { acc_d2[rank] = d2; acc_idx[rank] = idx; }
        if (tid == 0) acc_n = count < ekfm::kAssignCand ? count : ekfm::kAssignCand;
    }
    __syncthreads();
    ekfm::CandList &o = sel[k];
    if (tid < ekfm::kAssignCand) {
        const bool used = tid < acc_n;
        o.idx[tid] = used ? acc_idx[tid] : -1;
        o.d2[tid] = used ? acc_d2[tid] : INFINITY;
    }
    if (tid == 0) { o.n = acc_n; o.pad = 0; }
}

// the 64 lanes of one wavefront as assign_solve's team
struct AssignWaveTeam {
    template <class F> __device__ __forceinline__ void each(F f) { f((int)threadIdx.x, 64); __syncthreads(); }
    template <class F> __device__ __forceinline__ ekfm::AssignMin argmin(F f) {
        ekfm::AssignMin a = f((int)threadIdx.x, 64);
        const int lane = threadIdx.x;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            ekfm::AssignMin o;
            o.d = lane_gather(a.d, lane ^ off);
            o.j = __builtin_amdgcn_ds_bpermute((lane ^ off) << 2, a.j);
            a = ekfm::assign_min_merge(a, o);
        }
        return a;
    }
};

__global__ __launch_bounds__(64) void k_assign_solve(AssignSolveArgs a, const ekfm::CandList *__restrict__ sel, AssignResult *__restrict__ res) {
    __shared__ ekfm::AssignProblem p;
    const int lane = threadIdx.x;
    const int m = a.m;
    for (int f = lane; f < m * ekfm::kAssignCand; f += 64) {
        const ekfm::CandList &l = sel[f / ekfm::kAssignCand];
        p.idx[f] = l.idx[f % ekfm::kAssignCand];
        p.d2[f] = l.d2[f % ekfm::kAssignCand];
    }
    if (lane < m) { p.n[lane] = sel[lane].n; p.gate[lane] = a.gate[lane]; }
    if (lane == 0) p.m = m;
    __syncthreads();
    AssignWaveTeam team;
    ekfm::assign_solve(p, team);
    for (int f = lane; f < m * ekfm::kAssignCand; f += 64) { res->cand[f] = p.idx[f]; res->cand_d2[f] = p.d2[f]; }
    if (lane < m) {
        res->out[lane].landmark = ekfm::assign_landmark(p, lane);
        res->out[lane].d2 = ekfm::assign_d2(p, lane);
        res->out[lane].ncand = p.n[lane];
        res->out[lane].reserved = 0;
    }
    if (lane == 0) { res->total = ekfm::assign_total(p); res->pad = 0.0; }
}
