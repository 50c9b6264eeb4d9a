// Fragment of kernels.hip, the launchers of the calls that treat P as a matrix: the factorisation (factor_map.h), the draws (sample_map.h)
// and the solves (solve_map.h) behind it, the plain product P B (multiply_map.h) and the linear observation with a dense H behind that
// (dense_obs.h).  What they size their grids and their scratch by is launch/map_sizes.h, included in front of this fragment.
#pragma once

// ---- the factorisation of P (factor_map.h) ----
namespace {
bool factor_args_ok(const FactorMapArgs &a) {
    return a.tiles && a.rhs && a.res && a.N >= 0 && a.tm.T == kFactorTile && a.tm.world == 1 && a.rows == a.tm.padded(2 * a.N) &&
           a.nref >= 0 && a.nref <= kFactorRefMax && (a.nref == 0 || (a.ref && a.ref_stride >= 3 + 2 * a.N)) && (a.cur == 0 || a.cur == 1);
}
}  // namespace

hipError_t launch_factor_load(const DevState &st, const FactorMapArgs &a, int storage, hipStream_t s) {
    // every tile of the source is read from this handle's store (an unsharded tile map), every landmark below 2 N lies inside it
    if (!factor_args_ok(a) || st.tm.world != 1 || 2 * a.N > st.ldm) return hipErrorInvalidValue;
    if (a.rows == 0) return hipSuccess;
    const int64_t ntiles = a.tm.row_base(a.rows / kFactorTile);
    if (ntiles > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_factor_rhs, dim3((unsigned)cdiv(a.rows, (int64_t)kFactorBlock)), dim3(kFactorBlock), 0, s, st, a);
    return with_storage(storage, [&](auto ts) {
        hipLaunchKernelGGL((k_factor_load<decltype(ts), kFactorTile>), dim3((unsigned)ntiles), dim3(kFactorBlock), 0, s, st, a);
    });
}

hipError_t launch_factor_column(const FactorMapArgs &a, int k, int part, hipStream_t s) {
    const int64_t nF = a.rows / kFactorTile, m = nF - 1 - k;
    if (!factor_args_ok(a) || k < 0 || k >= nF || part < 0 || part > 2) return hipErrorInvalidValue;
    if (part == 0) hipLaunchKernelGGL(k_factor_diag<kFactorTile>, dim3(1), dim3(kFactorBlock), 0, s, a, k);
    else if (m == 0) return hipSuccess;
    else if (part == 1) hipLaunchKernelGGL(k_factor_panel<kFactorTile>, dim3((unsigned)m), dim3(64), 0, s, a, k);
    else {
        const int64_t grid = m * (m + 1) / 2;
        if (grid > 0x7fffffffll) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_factor_trail<kFactorTile>, dim3((unsigned)grid), dim3(4 * kFactorTile), 0, s, a, k);
    }
    return hipGetLastError();
}

hipError_t launch_factor_finish(const DevState &st, const FactorMapArgs &a, hipStream_t s) {
    if (!factor_args_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_factor_finish, dim3(1), dim3(kFactorBlock), 0, s, st, a);
    return hipGetLastError();
}

// ---- the draws behind it (sample_map.h: k_factor_apply, k_factor_sample) ----
hipError_t launch_factor_sample(const DevState &st, const FactorMapArgs &a, const FactorSampleArgs &sa, int part, hipStream_t s) {
    // every index the two kernels form lies inside the chunk (ld), the partial blocks (one per segment of the grid) and the store
    if (!factor_args_ok(a) || !a.lr_off || !sa.xi || !sa.y || !sa.part || sa.ld < a.rows + 3 || part < 0 || part > 1) return hipErrorInvalidValue;
    const int64_t nF = a.rows / kFactorTile, segments = factor_segment_base(nF, kFactorSegment);
    if (segments > 0x7fffffffll) return hipErrorInvalidValue;
    if (part == 0) {
        if (segments == 0) return hipSuccess;
        hipLaunchKernelGGL((k_factor_apply<kFactorTile, kFactorSegment>), dim3((unsigned)segments), dim3(4 * kFactorTile), 0, s, a, sa);
    } else
        hipLaunchKernelGGL((k_factor_sample<kFactorTile, kFactorSegment>), dim3((unsigned)(nF + 1)), dim3(kFactorBlock), 0, s, st, a, sa);
    return hipGetLastError();
}

// ---- the solves behind it (solve_map.h: k_solve_invert, k_solve_forward, k_solve_tail, k_solve_backward) ----
hipError_t launch_solve_map(const FactorMapArgs &a, const FactorSolveArgs &sv, int part, int c, hipStream_t s) {
    // every index the kernels form lies inside the chunks (ld), the inverse tiles (one per tile row) and the store (c inside the grid)
    if (!factor_args_ok(a) || !a.lr_off || !sv.b || !sv.y || !sv.inv || sv.ld < a.rows + 3 || (sv.form != 0 && sv.form != 1)) return hipErrorInvalidValue;
    const int64_t nF = a.rows / kFactorTile;
    if (part == 0) {
        if (nF == 0) return hipSuccess;
        hipLaunchKernelGGL(k_solve_invert<kFactorTile>, dim3((unsigned)nF), dim3(64), 0, s, a, sv);
    } else if (part == 1 || part == 3) {
        if (c < 0 || c >= nF || (part == 3 && sv.form != 0)) return hipErrorInvalidValue;
        if (part == 1) hipLaunchKernelGGL(k_solve_forward<kFactorTile>, dim3((unsigned)(nF - c)), dim3(4 * kFactorTile), 0, s, a, sv, c);
        else hipLaunchKernelGGL(k_solve_backward<kFactorTile>, dim3((unsigned)(c + 1)), dim3(4 * kFactorTile), 0, s, a, sv, c);
    } else if (part == 2)
        hipLaunchKernelGGL(k_solve_tail, dim3(1), dim3(kFactorBlock), 0, s, a, sv);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

// ---- the plain product P B on the handle's own store (multiply_map.h: k_multiply_tiles, k_multiply_sum) ----
hipError_t launch_multiply_map(const DevState &st, const MultiplyMapArgs &a, int part, int storage, hipStream_t s) {
    // every index the kernels form lies inside the chunks (ld), the partial blocks (one per segment, one slot per tile, one part per tile
    // row) and the handle's own store (an unsharded tile map, every landmark below 2 N inside the strip)
    const int T = st.tm.T;
    if (!a.b || !a.y || !a.dpart || !a.tpart || !a.wpart || a.N < 0 || st.tm.world != 1 || T < 16 || T > 16 * 4 * kMultiplyWaveBlocks || (T & (T - 1)) ||
        2 * a.N > st.ldm || a.rows != st.tm.padded(2 * a.N) || a.ld < a.rows + 3 || a.S != multiply_segment(T) || (a.cur != 0 && a.cur != 1) || part < 0 || part > 1)
        return hipErrorInvalidValue;
    const int64_t nT = a.rows / T, segments = factor_segment_base(nT, a.S);
    if (segments > 0x7fffffffll) return hipErrorInvalidValue;
    if (part == 1) {
        const int64_t grid = nT * cdiv((int64_t)T * kFactorChunk, (int64_t)kFactorBlock);
        if (grid > 0x7fffffffll) return hipErrorInvalidValue;
        if (grid > 0) hipLaunchKernelGGL(k_multiply_sum, dim3((unsigned)grid), dim3(kFactorBlock), 0, s, st, a);
        hipLaunchKernelGGL(k_multiply_robot, dim3(1), dim3(kFactorBlock), 0, s, st, a);
        return hipGetLastError();
    }
    if (segments == 0) return hipSuccess;
    return with_storage(storage, [&](auto ts) {
        using TS = decltype(ts);
        if (T <= 128) hipLaunchKernelGGL((k_multiply_tiles<TS, 128>), dim3((unsigned)segments), dim3(kMultiplyBlock), 0, s, st, a);
        else hipLaunchKernelGGL((k_multiply_tiles<TS, 256>), dim3((unsigned)segments), dim3(kMultiplyBlock), 0, s, st, a);
    });
}

// ---- a linear observation with a dense H (dense_obs.h), behind launch_multiply_map's two stages on the same chunk ----
namespace {
bool dense_args_ok(const DevState &st, const DenseArgs &a) {
    // every row the kernels read lies inside the chunks (ld) and inside the strip; the robot's three entries lie behind the landmark rows
    return a.b && a.y && a.part && a.kk >= 2 && a.kk <= kDenseMax && !(a.kk & 1) && a.n_mm >= 0 && !(a.n_mm & 1) && a.n_mm <= st.ldm &&
           a.rows == st.tm.padded(a.n_mm) && a.ld >= a.rows + 3 && (a.cur == 0 || a.cur == 1) && st.tm.world == 1;
}
}  // namespace

hipError_t launch_dense_gram(const DevState &st, const DenseArgs &a, hipStream_t s) {
    if (!dense_args_ok(st, a)) return hipErrorInvalidValue;
    const int64_t grid = cdiv(a.n_mm, (int64_t)kDenseSegment);
    if (grid > 0x7fffffffll) return hipErrorInvalidValue;
    if (grid == 0) return hipSuccess;
    hipLaunchKernelGGL(k_dense_gram, dim3((unsigned)grid), dim3(kDenseBlock), 0, s, st, a);
    return hipGetLastError();
}

hipError_t launch_dense_factor(const DevState &st, const DenseArgs &a, const DenseSmall &sm, DenseOut *out, DenseBlock *blk, hipStream_t s) {
    if (!dense_args_ok(st, a) || !out || !blk) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_dense_factor, dim3(1), dim3(kDenseFactorBlock), 0, s, st, a, sm, out, blk);
    return hipGetLastError();
}

hipError_t launch_gather_dense(const DevState &st, const DenseArgs &a, const DenseBlock *blk, hipStream_t s) {
    // launch_gather_joint's checks: the pairs inside the private F64 ring, the padded block inside the strip.  N = 0 is one workgroup
    // without a live lane: the robot part alone
    if (!dense_args_ok(st, a) || !blk || a.kk / 2 > st.pcap || st.tm.padded(a.n_mm) > st.ldm || st.Gp32 || st.Kp32 || !st.Gp || !st.Kp)
        return hipErrorInvalidValue;
    const int64_t cols = st.tm.padded(a.n_mm);
    const unsigned grid = (unsigned)(cols > 0 ? cdiv(cols, (int64_t)kBlock) : 1);
    if (a.kk <= 4) hipLaunchKernelGGL(k_gather_dense<2>, dim3(grid), dim3(kBlock), 0, s, st, a, blk);
    else hipLaunchKernelGGL(k_gather_dense<8>, dim3(grid), dim3(kBlock), 0, s, st, a, blk);
    return hipGetLastError();
}
