// The slab reduce of the ordered-slab fp32 weight gradients, shared by idf_wgrad_f32.hip (exact fp32 MFMA) and
// idf_wgrad_split.hip (split-bf16 MFMA).  Lives in an anonymous namespace per translation unit.
#pragma once
#include "idf_common.h"

namespace {

// dW | db = sum of the S slabs, in slab order; one float4 per thread (nW % 4 == 0: no float4 straddles dW | db)
__global__ __launch_bounds__(256) void wgrad_f32_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dW,
                                                               float* __restrict__ db, long nW, long n4, long slab, int S) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const long e = 4 * i;
  float4 v = *reinterpret_cast<const float4*>(ws + e);
  for (int s = 1; s < S; ++s) {
    const float4 u = *reinterpret_cast<const float4*>(ws + (size_t)s * slab + e);
    v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
  }
  *reinterpret_cast<float4*>(e < nW ? dW + e : db + (e - nW)) = v;
}

}  // namespace
