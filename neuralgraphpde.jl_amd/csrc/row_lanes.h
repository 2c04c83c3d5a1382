// row_lanes.h -- the (entry slot, column) lane layout of the row-reducing kernels (msgpass.hip, readout.hip): `dpl` lanes cover one
// chunk of a row's columns, 64 / dpl rows are processed at once, and the slots' partials are combined by a fixed xor butterfly.  Here:
// the float / float4 forms of the few operations those row loops need, so that one kernel body serves both column types.
#pragma once

#include "device_utils.h"

namespace ngpde {

__device__ __forceinline__ float vzero(float) { return 0.f; }
__device__ __forceinline__ float4 vzero(float4) { return f4_zero(); }
__device__ __forceinline__ float vadd(float a, float b) { return a + b; }
__device__ __forceinline__ float4 vadd(float4 a, float4 b) { return f4_add(a, b); }
__device__ __forceinline__ float vmul(float a, float b) { return a * b; }
__device__ __forceinline__ float4 vmul(float4 a, float4 b) { return f4_mul(a, b); }
__device__ __forceinline__ float vscale(float s, float a) { return s * a; }
__device__ __forceinline__ float4 vscale(float s, float4 a) { return f4_scale(s, a); }
__device__ __forceinline__ float vhsum(float a) { return a; }
__device__ __forceinline__ float vhsum(float4 a) { return (a.x + a.y) + (a.z + a.w); }
__device__ __forceinline__ float vxor(float a, int o) { return __shfl_xor(a, o); }
__device__ __forceinline__ float4 vxor(float4 a, int o) {
  return make_float4(__shfl_xor(a.x, o), __shfl_xor(a.y, o), __shfl_xor(a.z, o), __shfl_xor(a.w, o));
}

// lanes per entry for a row chunk of w columns: the next power of two, at most the wave
__host__ __device__ __forceinline__ int lanes_per_entry(int w) {
  int dpl = 1;
  while (dpl < w && dpl < 64) dpl <<= 1;
  return dpl;
}

}  // namespace ngpde
