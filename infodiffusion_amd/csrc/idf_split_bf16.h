// The split-bf16 arithmetic of the fp32 modes bf16x3 / bf16x2, shared by idf_conv3x3_split.hip (forward, data gradient) and
// idf_wgrad_split.hip (weight gradient): the register split of 8 fp32 values into TERMS bf16 runs and the kept cross products of
// one 16x16x32 MFMA tile.  Everything lives in an anonymous namespace per translation unit.
#pragma once
#include "idf_common.h"

namespace {

// v -> TERMS bf16 terms of 8 consecutive channels, one dword pair per idf_pack_bf16
template <int TERMS>
__device__ __forceinline__ void split8(const float4& a, const float4& b, uint4* out) {
  const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  float r[8];
  uint32_t d[TERMS][4];
#pragma unroll
  for (int e = 0; e < 8; ++e) r[e] = v[e];
#pragma unroll
  for (int t = 0; t < TERMS; ++t) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t pk = idf_pack_bf16(r[2 * e], r[2 * e + 1]);
      d[t][e] = pk;
      if (t + 1 < TERMS) {        // exact: the term is the leading bits of r
        r[2 * e] -= __uint_as_float(pk << 16);
        r[2 * e + 1] -= __uint_as_float(pk & 0xffff0000u);
      }
    }
    out[t] = make_uint4(d[t][0], d[t][1], d[t][2], d[t][3]);
  }
}

__device__ __forceinline__ bf16x8_t as_bf16x8(const uint4& v) { return __builtin_bit_cast(bf16x8_t, v); }

// the cross products of one (cout 16-tile, pixel 16-tile, tap, chunk), smallest first, hh last; w = A (rows = cout), x = B
template <int TERMS>
__device__ __forceinline__ f32x4_t split_mfma(const bf16x8_t* w, const bf16x8_t* x, f32x4_t acc) {
  if constexpr (TERMS == 3) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[1], x[1], acc, 0, 0, 0);    // mm
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[2], x[0], acc, 0, 0, 0);    // w.l x.h
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[0], x[2], acc, 0, 0, 0);    // w.h x.l
  }
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[1], x[0], acc, 0, 0, 0);      // w.m x.h
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[0], x[1], acc, 0, 0, 0);      // w.h x.m
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[0], x[0], acc, 0, 0, 0);      // hh
  return acc;
}

}  // namespace
