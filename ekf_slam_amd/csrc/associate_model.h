// Fragment of kernels.hip (included there, inside its anonymous namespace, after model_obs.h): a whole scan scored against the whole map
// under the conventions of ekf_observe_model (ekf_associate_model): k_assoc_model, k_assoc_model_reduce.
#pragma once

// ---------------------------------------------------------------------------------------------------
// d2(k, i) = what k_model_probe reports for observation k with landmark i as its target.  A one-landmark model's small part needs nothing
// from the tiles: Prr, the strip at the landmark's columns, its live diagonal block and x are F64 copies that carry every pending pair and
// are replicated on every shard (linear_small_entry, entries 0-26 and 31-35).  So one lane takes one landmark, loads its 11 doubles and
// runs ekfm::assoc_model_d2 -- model_eval, model_small and constrain_d2 on the operands the probe would have loaded, the same sums in the
// same order.  Nothing of the state is written, no chain of pending pairs is walked, and the launch runs beside a pass in flight.
//
// Grid (ceil(N / kAssocBlock), m): the observation is blockIdx.y, so model, z, R and the gate are uniform over a workgroup (mixed models in
// one scan never diverge inside one), and so are Prr and the pose.  Every lane offers its landmark to a Match2 record; the records meet by
// match2_merge -- shuffles inside a wavefront, the four wavefronts through LDS behind one barrier -- and the workgroup leaves one record in
// partials[k * gridDim.x + blockIdx.x].  k_assoc_model_reduce, the next launch on the stream, merges an observation's records on one
// wavefront.  match2_merge is associative and commutative: no atomics, no tickets, no fences, and the result does not depend on the shape
// of the reduction.
// ---------------------------------------------------------------------------------------------------

__device__ __forceinline__ long long lane_gather_ll(long long v, int src) {
    return __double_as_longlong(lane_gather(__longlong_as_double(v), src));
}
// the record of lane `src`
__device__ __forceinline__ ekfm::Match2 match2_from_lane(const ekfm::Match2 &m, int src) {
    ekfm::Match2 o;
    o.best = lane_gather_ll(m.best, src); o.second = lane_gather_ll(m.second, src);
    o.d2_best = lane_gather(m.d2_best, src); o.d2_second = lane_gather(m.d2_second, src);
    o.within = lane_gather_ll(m.within, src); o.irregular = lane_gather_ll(m.irregular, src);
    return o;
}
// every lane's record merged over the wavefront (a butterfly: every lane ends with the whole)
__device__ __forceinline__ ekfm::Match2 match2_wave(ekfm::Match2 m) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = ekfm::match2_merge(m, match2_from_lane(m, lane ^ off));
    return m;
}

// d2_all: nullptr, or m x N row-major (NaN where a pair has no d2)
__global__ __launch_bounds__(kAssocBlock) void k_assoc_model(DevState st, AssocModelArgs a, ekfm::Match2 *__restrict__ partials,
                                                             double *__restrict__ d2_all) {
    __shared__ ekfm::Match2 wave_rec[kAssocBlock / 64];
    const int tid = threadIdx.x;
    const int k = blockIdx.y;
    const AssocModelEntry &e = a.e[k];
    const int cur = a.cur;
    const int64_t i = (int64_t)blockIdx.x * kAssocBlock + tid;
    ekfm::Match2 m;
    ekfm::match2_init(m);
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
        double d2;
        const bool regular = ekfm::assoc_model_d2(e.model, e.z, e.R, prr, strip6, diag3, xr, l, d2);
        ekfm::match2_offer(m, d2, i, regular, e.gate);
        if (d2_all) d2_all[(int64_t)k * a.N + i] = d2;
    }
    m = match2_wave(m);
    if ((tid & 63) == 0) wave_rec[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
        ekfm::Match2 r = wave_rec[0];
        for (int w = 1; w < kAssocBlock / 64; ++w) r = ekfm::match2_merge(r, wave_rec[w]);
        partials[(int64_t)k * gridDim.x + blockIdx.x] = r;
    }
}

// out[k] = the merge of partials[k * nblk .. + nblk): one wavefront per observation, lanes striding over the records
__global__ __launch_bounds__(64) void k_assoc_model_reduce(const ekfm::Match2 *__restrict__ partials, int nblk, ekfm::Match2 *__restrict__ out) {
    const int lane = threadIdx.x;
    const int k = blockIdx.x;
    ekfm::Match2 m;
    ekfm::match2_init(m);
    for (int b = lane; b < nblk; b += 64) m = ekfm::match2_merge(m, partials[(int64_t)k * nblk + b]);
    m = match2_wave(m);
    if (lane == 0) out[k] = m;
}
