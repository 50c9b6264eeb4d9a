// Fragment of kernels.hip, the launchers of state I/O (the kernels of ../state_io.h): dense <-> tiled, block reads, the low-rank load,
// the digest.
#pragma once

hipError_t launch_unpack_dense(const DevState &st, int cur, int64_t n_mm, double *dense, int storage, hipStream_t s) {
    const int64_t n = n_mm + 3;
    return with_storage(storage, [&](auto ts) {
        hipLaunchKernelGGL(k_unpack_dense<decltype(ts)>, dim3((unsigned)cdiv(n * n, kBlock)), dim3(kBlock), 0, s, st, cur, n, dense);
    });
}

hipError_t launch_pack_dense(const DevState &st, int cur, int64_t n_mm, const double *dense, int storage, hipStream_t s) {
    const int64_t n = n_mm + 3;
    return with_storage(storage, [&](auto ts) {
        hipLaunchKernelGGL(k_pack_dense<decltype(ts)>, dim3((unsigned)cdiv(n * n, kBlock)), dim3(kBlock), 0, s, st, cur, n, dense);
    });
}

hipError_t launch_get_block(const DevState &st, int cur, int64_t r0, int64_t c0, int64_t nr, int64_t nc, double *out,
                            int storage, hipStream_t s) {
    return with_storage(storage, [&](auto ts) {
        hipLaunchKernelGGL(k_get_block<decltype(ts)>, dim3((unsigned)cdiv(nr * nc, kBlock)), dim3(kBlock), 0, s, st, cur, r0, c0, nr, nc, out);
    });
}

hipError_t launch_get_diag_blocks(const DevState &st, int cur, int64_t N, double *out, int storage, hipStream_t s) {
    return with_storage(storage, [&](auto ts) {
        hipLaunchKernelGGL(k_get_diag_blocks<decltype(ts)>, dim3((unsigned)cdiv(4 * (N + 1), kBlock)), dim3(kBlock), 0, s, st, cur, N, out);
    });
}

hipError_t launch_lowrank(const DevState &st, int cur, int64_t n_mm, const int2 *work, int64_t nwork, const double *d,
                          const double *U, int64_t k, int storage, hipStream_t s) {
    if (nwork > 0) {
        const int64_t grid = nwork < 65536 ? nwork : 65536;
        const hipError_t e = with_storage(storage, [&](auto ts) {
            hipLaunchKernelGGL(k_lowrank_tiles<decltype(ts)>, dim3((unsigned)grid), dim3(kBlock), 0, s, st, n_mm, work, nwork, d, U, k);
        });
        if (e != hipSuccess) return e;
    }
    const int64_t grid = cdiv(n_mm > 0 ? n_mm : 1, kBlock);
    hipLaunchKernelGGL(k_lowrank_robot, dim3((unsigned)grid), dim3(kBlock), 0, s, st, cur, n_mm, d, U, k);
    return hipGetLastError();
}

hipError_t launch_digest(const DevState &st, int cur, int64_t n_mm, const int2 *work, int64_t nwork, double *out,
                         int storage, hipStream_t s) {
    hipError_t e = hipMemsetAsync(out, 0, 4 * sizeof(double), s);      // sums + the ticket; partial slots follow (kDigestSlots)
    if (e != hipSuccess) return e;
    int64_t grid = nwork < kDigestGrid ? nwork : kDigestGrid;
    if (grid < 1) grid = 1;
    return with_storage(storage, [&](auto ts) {
        hipLaunchKernelGGL(k_digest<decltype(ts)>, dim3((unsigned)grid), dim3(kBlock), 0, s, st, cur, n_mm, work, nwork, out);
    });
}
