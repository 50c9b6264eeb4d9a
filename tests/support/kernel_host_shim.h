// The shim behind which the host emulations of tests/support compile the kernel SOURCES of ekf_slam_amd/csrc with g++ (no GPU, no HIP
// runtime): the HIP keywords as empty macros, the vector types the kernels name, thread indices as globals, __shared__ as static storage,
// lane_xor1 in two passes.  The state and the argument blocks are the kernels' own: kernel_args.h needs no HIP header.
// An emulation runs a workgroup's lanes one after another and the whole workgroup again until what its first lanes leave in the shared
// storage is there (launch_wg of emulated_state.h, which also holds the state the kernels run on), so __syncthreads is empty.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>
#include "layout.h"
#include "device_math.h"
#include "kernel_args.h"
struct double2 { double x, y; }; struct float2 { float x, y; }; struct float4 { float x, y, z, w; }; struct int2 { int x, y; };
static inline double2 make_double2(double a, double b) { return {a, b}; }
static inline float4 make_float4(float a, float b, float c, float d) { return {a, b, c, d}; }
#define __device__
#define __global__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(x)
#define __shared__ static
static inline void __syncthreads() {}
struct Idx { unsigned x; };
static Idx threadIdx, blockIdx;
constexpr int kBlock = 256;
static inline int ring_slot(int pstart, int i, int pcap) { const int s = pstart + i; return s >= pcap ? s - pcap : s; }
// lane_xor1: two passes per workgroup -- the first (xor_pass == 0) records what every lane hands over, the second returns the partner's
static int xor_pass; static std::vector<double> xor_rec[kBlock]; static size_t xor_pos[kBlock];
static inline double lane_xor1(double v) {
    const unsigned t = threadIdx.x;
    if (xor_pass == 0) { xor_rec[t].push_back(v); return 0.0; }
    return xor_rec[t ^ 1][xor_pos[t]++];
}
template <typename TS> struct Lane16;
template <> struct Lane16<double> { using type = double2; static constexpr int kCols = 2; };
template <> struct Lane16<float>  { using type = float4;  static constexpr int kCols = 4; };
static inline void lane16_pack(const double *v, double2 &t) { t.x = v[0]; t.y = v[1]; }
static inline void lane16_pack(const double *v, float4 &t) { t.x = (float)v[0]; t.y = (float)v[1]; t.z = (float)v[2]; t.w = (float)v[3]; }
