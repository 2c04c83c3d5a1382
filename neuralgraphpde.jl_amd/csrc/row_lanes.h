// row_lanes.h -- the (entry slot, column) lane layout of the row-reducing kernels (msgpass.hip, readout.hip): `dpl` lanes cover one
// chunk of a row's columns, 64 / dpl rows are processed at once, and the slots' partials are combined by a fixed xor butterfly.  Here:
// the float / float4 forms of the few operations those row loops (and graph_ops.hip's group reduce) need, so that one kernel body
// serves both column types.
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
__device__ __forceinline__ float vmax(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ float4 vmax(float4 a, float4 b) { return make_float4(fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w)); }
__device__ __forceinline__ float vmin(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ float4 vmin(float4 a, float4 b) { return make_float4(fminf(a.x, b.x), fminf(a.y, b.y), fminf(a.z, b.z), fminf(a.w, b.w)); }
__device__ __forceinline__ float vsel_eq(float a, float b, float v) { return a == b ? v : 0.f; }   // v where a == b, else 0
__device__ __forceinline__ float4 vsel_eq(float4 a, float4 b, float4 v) {
  return make_float4(a.x == b.x ? v.x : 0.f, a.y == b.y ? v.y : 0.f, a.z == b.z ? v.z : 0.f, a.w == b.w ? v.w : 0.f);
}
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
