// Fragment of kernels.hip (included there, inside its anonymous namespace, in front of every kernel family): values that travel between
// the lanes of one wavefront without LDS memory, and the wavefront's own LDS ordering.  (The host emulations of
// tests/support supply a lane_xor1 of their own, kernel_host_shim.h, and do not include this file.)
#pragma once

__device__ __forceinline__ double lane_bcast(double v, int src) {        // value of lane `src` (compile-time) on every lane
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src), hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double lane_gather(double v, int src) {       // value of lane `src` (per-lane index): ds_bpermute x 2
    const int lo = __builtin_amdgcn_ds_bpermute(src << 2, __double2loint(v)), hi = __builtin_amdgcn_ds_bpermute(src << 2, __double2hiint(v));
    return __hiloint2double(hi, lo);
}
// value of the neighbouring lane (lane ^ 1): a DPP quad permutation [1,0,3,2] -- two VALU moves, no LDS crossbar round trip (what
// __shfl_xor's ds_bpermute costs at the tail of k_gather's latency chain)
__device__ __forceinline__ double lane_xor1(double v) {
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), 0xB1, 0xF, 0xF, true), hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), 0xB1, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}
// LDS traffic of ONE wavefront is ordered; this only keeps the compiler from moving accesses across it and drains the queue
__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
