// Fused fp32 single-head attention, forward and backward, on the exact-fp32 MFMA (v_mfma_f32_16x16x4_f32): K and V (forward,
// query half of the backward) or Q and dO (key/value half) stream through LDS in row chunks, double-buffered; scores and
// probabilities never leave the registers.  DESIGN.md 4l has the mapping and the bank arithmetic.
//
// MFMA 16x16x4 operand layout, lane = 16 g + c:  A[m = c][k = g], B[k = g][n = c], D[m = 4 g + i][n = c] in register i.
//
// Every product contracts over channels or over rows of the streamed chunk, and both contractions may visit their index in any
// order as long as A and B agree on it.  Two orders are used:
//   channel contraction (scores, dP): step (j, e) of lane group g is channel 16 j + 4 g + e -- the four steps e of one j are ONE
//     16-byte vector per lane, from LDS for the streamed rows (row c of the tile) and from global memory, once, for the strip's own rows;
//   row contraction (P V, dS K, P^T dO, dS^T Q): step i of lane group g is row 4 g + i of the 16-row tile -- which is where the
//     score MFMA left the value: register i of lane (c, g) IS the B operand, no shuffle.  The A operand V[row][channel] is read
//     as one 16-byte vector of channels 64 h + 4 c .. + 3 and feeds FOUR output tiles (h, jj): output tile (h, jj) holds channels
//     64 h + 4 m + jj, so register i of the four tiles jj = 0 .. 3 is one 16-byte vector of channels 64 h + 16 g + 4 i .. + 3 of row c.
// LDS rows have a pitch of D + 4 floats = 4 banks (mod 64): see bank arithmetic in DESIGN.md 4l.
//
// Fixed summation order, one writer per output element, no atomics: a second call is bit-identical.
#include "idf_common.h"

#include <math.h>

namespace {

constexpr float LOG2E = 1.4426950408889634f;

#define MFMA4(acc, a, b) (acc) = __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (acc), 0, 0, 0)

template <int D, int NW>
struct Cfg {
  static constexpr int NT = 64 * NW;                      // threads
  static constexpr int QB = 16 * NW;                      // strip rows per workgroup
  static constexpr int P = D + 4;                         // LDS row pitch, floats
  static constexpr int V4 = D / 4;                        // 16-byte vectors per row
  static constexpr int NJ = D / 16;                       // 16-byte vectors of its own row per lane = channel steps / 4 = output tiles
  static constexpr int KC_FWD = 64;                       // streamed rows per chunk, forward: a chunk's loads fly under 64 * D / 64 MFMAs
  static constexpr int KC_BWD = D == 128 ? 16 : 32;       // backward: two matrices per chunk
  static constexpr size_t LDS_FWD = (size_t)2 * KC_FWD * P * sizeof(float);
  static constexpr size_t LDS_BWD = ((size_t)4 * KC_BWD * P + 4 * KC_BWD) * sizeof(float);
};

__device__ __forceinline__ float q16_max(float v) {       // over the four lanes c, c + 16, c + 32, c + 48
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float q16_sum(float v) {       // same four lanes; every lane ends with the same bits
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}
__device__ __forceinline__ float dot4(const f32x4_t& a, const f32x4_t& b) { return ((a.x * b.x + a.y * b.y) + a.z * b.z) + a.w * b.w; }

// one 16 x 16 tile of a channel contraction: acc[m][n] += sum_d rows[m][d] * own[n][d]; rows = 16 LDS rows, own = the lane's vectors
template <int D>
__device__ __forceinline__ void tile_over_channels(f32x4_t& acc, const float* __restrict__ rows, const f32x4_t* own, int c, int g) {
  constexpr int P = D + 4;
#pragma unroll
  for (int j = 0; j < D / 16; ++j) {
    const f32x4_t a = *reinterpret_cast<const f32x4_t*>(rows + c * P + 16 * j + 4 * g);
    MFMA4(acc, a.x, own[j].x);
    MFMA4(acc, a.y, own[j].y);
    MFMA4(acc, a.z, own[j].z);
    MFMA4(acc, a.w, own[j].w);
  }
}

// a row contraction over one 16-row tile: out[(h, jj)][m][n] += sum_r rows[r][64 h + 4 m + jj] * w[r][n], w = the score-layout tile
template <int D>
__device__ __forceinline__ void tile_over_rows(f32x4_t* out, const float* __restrict__ rows, const f32x4_t& w, int c, int g) {
  constexpr int P = D + 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int h = 0; h < D / 64; ++h) {
      const f32x4_t a = *reinterpret_cast<const f32x4_t*>(rows + (4 * g + i) * P + 64 * h + 4 * c);
      MFMA4(out[4 * h + 0], a.x, w[i]);
      MFMA4(out[4 * h + 1], a.y, w[i]);
      MFMA4(out[4 * h + 2], a.z, w[i]);
      MFMA4(out[4 * h + 3], a.w, w[i]);
    }
  }
}

// out tiles -> row c of dst (D floats at dst), scaled
template <int D>
__device__ __forceinline__ void store_rows(float* __restrict__ dst, const f32x4_t* out, float s, int g) {
#pragma unroll
  for (int h = 0; h < D / 64; ++h) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      *reinterpret_cast<f32x4_t*>(dst + 64 * h + 16 * g + 4 * i) =
          f32x4_t{out[4 * h + 0][i] * s, out[4 * h + 1][i] * s, out[4 * h + 2][i] * s, out[4 * h + 3][i] * s};
  }
}

// ------------------------------------------------------------------------------------------------------------------ forward
// grid (N / QB, B); a wave owns 16 queries.  c2 = scale * log2(e); lse2 = log2 of the row sum of 2^(c2 * s).
template <int N, int D, int NW>
__global__ __launch_bounds__(64 * NW) void attn_f32_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ o,
                                                                float* __restrict__ lse, float c2) {
  using C = Cfg<D, NW>;
  constexpr int NT = C::NT, P = C::P, V4 = C::V4, NJ = C::NJ, KC = C::KC_FWD, LPT = KC * V4 / NT, NCH = N / KC, TPC = KC / 16;
  static_assert(LPT * NT == KC * V4 && NCH * KC == N, "chunking");
  extern __shared__ f32x4_t attn_f32_smem[];
  float* sm = reinterpret_cast<float*>(attn_f32_smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
  const int b = blockIdx.y, q0 = blockIdx.x * C::QB + wave * 16;
  const float* base = qkv + (size_t)b * N * 3 * D;

  f32x4_t qf[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) qf[j] = *reinterpret_cast<const f32x4_t*>(base + (size_t)(q0 + c) * 3 * D + 16 * j + 4 * g);

  f32x4_t stg[LPT];
  auto gload = [&](int idx) {      // chunk idx of the sequence K chunks | V chunks
    const float* src = base + (idx < NCH ? D : 2 * D) + (size_t)((idx < NCH ? idx : idx - NCH) * KC) * 3 * D;
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      const int e = tid + i * NT;
      stg[i] = *reinterpret_cast<const f32x4_t*>(src + (size_t)(e / V4) * 3 * D + (e % V4) * 4);
    }
  };
  auto sstore = [&](float* buf) {
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      const int e = tid + i * NT;
      *reinterpret_cast<f32x4_t*>(buf + (e / V4) * P + (e % V4) * 4) = stg[i];
    }
  };

  f32x4_t acc[N / 16];
#pragma unroll
  for (int t = 0; t < N / 16; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  f32x4_t out[NJ];
#pragma unroll
  for (int t = 0; t < NJ; ++t) out[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float mx = 0.f, sum = 0.f;

  gload(0);
  sstore(sm);
  __syncthreads();
#pragma unroll
  for (int idx = 0; idx < 2 * NCH; ++idx) {
    const float* cur = sm + (idx & 1) * KC * P;
    if (idx + 1 < 2 * NCH) gload(idx + 1);          // in flight under this chunk's MFMAs
    if (idx < NCH) {
#pragma unroll
      for (int tt = 0; tt < TPC; ++tt) tile_over_channels<D>(acc[idx * TPC + tt], cur + tt * 16 * P, qf, c, g);
    } else {
      if (idx == NCH) {                             // the whole score row of query c is in the four lanes c + 16 g
        mx = acc[0][0];
#pragma unroll
        for (int t = 0; t < N / 16; ++t)
#pragma unroll
          for (int i = 0; i < 4; ++i) mx = fmaxf(mx, acc[t][i]);
        mx = q16_max(mx);
#pragma unroll
        for (int t = 0; t < N / 16; ++t)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            acc[t][i] = __builtin_amdgcn_exp2f((acc[t][i] - mx) * c2);
            sum += acc[t][i];
          }
        sum = q16_sum(sum);
      }
#pragma unroll
      for (int tt = 0; tt < TPC; ++tt) tile_over_rows<D>(out, cur + tt * 16 * P, acc[(idx - NCH) * TPC + tt], c, g);
    }
    if (idx + 1 < 2 * NCH) {
      sstore(sm + ((idx + 1) & 1) * KC * P);        // last read in iteration idx - 1, before that iteration's barrier
      __syncthreads();
    }
  }
  store_rows<D>(o + ((size_t)b * N + q0 + c) * D, out, 1.0f / sum, g);
  if (g == 0) lse[(size_t)b * N + q0 + c] = mx * c2 + log2f(sum);
}

// ----------------------------------------------------------------------------------------------------------------- backward
// grid (N / QB, B, 2): z = 0 the query half (strip = 16 queries, streams K | V, writes dQ), z = 1 the key/value half (strip = 16
// keys, streams Q | dO and forms delta = rowsum(dO . O) of the streamed rows, writes dK and dV).
template <int D, int NW>
struct Bwd {
  using C = Cfg<D, NW>;
  static constexpr int NT = C::NT, P = C::P, V4 = C::V4, NJ = C::NJ, KC = C::KC_BWD, LPT = KC * V4 / NT, TPC = KC / 16;
  static_assert(LPT * NT == KC * V4, "chunking");

  static __device__ __forceinline__ void query_half(float* sm, const float* __restrict__ qkv, const float* __restrict__ dO,
                                                    const float* __restrict__ lse, const float* __restrict__ o,
                                                    float* __restrict__ dqkv, int N, float scale, float c2) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
    const int b = blockIdx.y, q0 = blockIdx.x * C::QB + wave * 16;
    const float* base = qkv + (size_t)b * N * 3 * D;
    const size_t row = (size_t)b * N + q0 + c;
    f32x4_t qf[NJ], dof[NJ];
    float delta = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      qf[j] = *reinterpret_cast<const f32x4_t*>(base + (size_t)(q0 + c) * 3 * D + 16 * j + 4 * g);
      dof[j] = *reinterpret_cast<const f32x4_t*>(dO + row * D + 16 * j + 4 * g);
      delta += dot4(dof[j], *reinterpret_cast<const f32x4_t*>(o + row * D + 16 * j + 4 * g));
    }
    delta = q16_sum(delta);
    const float l2 = lse[row];

    f32x4_t sk[LPT], sv[LPT];
    auto gload = [&](int idx) {
      const float* src = base + (size_t)(idx * KC) * 3 * D;
#pragma unroll
      for (int i = 0; i < LPT; ++i) {
        const int e = tid + i * NT;
        const float* p = src + (size_t)(e / V4) * 3 * D + (e % V4) * 4;
        sk[i] = *reinterpret_cast<const f32x4_t*>(p + D);
        sv[i] = *reinterpret_cast<const f32x4_t*>(p + 2 * D);
      }
    };
    auto sstore = [&](float* buf) {
#pragma unroll
      for (int i = 0; i < LPT; ++i) {
        const int e = tid + i * NT;
        *reinterpret_cast<f32x4_t*>(buf + (e / V4) * P + (e % V4) * 4) = sk[i];
        *reinterpret_cast<f32x4_t*>(buf + KC * P + (e / V4) * P + (e % V4) * 4) = sv[i];
      }
    };
    f32x4_t dq[NJ];
#pragma unroll
    for (int t = 0; t < NJ; ++t) dq[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    const int nch = N / KC;
    gload(0);
    sstore(sm);
    __syncthreads();
    for (int idx = 0; idx < nch; ++idx) {
      const float* cur = sm + (idx & 1) * 2 * KC * P;
      if (idx + 1 < nch) gload(idx + 1);
#pragma unroll
      for (int tt = 0; tt < TPC; ++tt) {
        f32x4_t s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f}, ds;
        tile_over_channels<D>(s, cur + tt * 16 * P, qf, c, g);                  // s[key 4g+i][query c]
        tile_over_channels<D>(dp, cur + KC * P + tt * 16 * P, dof, c, g);       // dP, same layout
#pragma unroll
        for (int i = 0; i < 4; ++i) ds[i] = __builtin_amdgcn_exp2f(fmaf(s[i], c2, -l2)) * (dp[i] - delta);
        tile_over_rows<D>(dq, cur + tt * 16 * P, ds, c, g);                     // dQ^T += K^T dS^T
      }
      if (idx + 1 < nch) {
        sstore(sm + ((idx + 1) & 1) * 2 * KC * P);
        __syncthreads();
      }
    }
    store_rows<D>(dqkv + row * 3 * D, dq, scale, g);
  }

  static __device__ __forceinline__ void kv_half(float* sm, const float* __restrict__ qkv, const float* __restrict__ dO,
                                                 const float* __restrict__ lse, const float* __restrict__ o,
                                                 float* __restrict__ dqkv, int N, float scale, float c2) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
    const int b = blockIdx.y, k0 = blockIdx.x * C::QB + wave * 16;
    const float* base = qkv + (size_t)b * N * 3 * D;
    float* ext = sm + 4 * KC * P;                 // [2 buffers][lse2 | delta][KC]
    f32x4_t kf[NJ], vf[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      kf[j] = *reinterpret_cast<const f32x4_t*>(base + (size_t)(k0 + c) * 3 * D + D + 16 * j + 4 * g);
      vf[j] = *reinterpret_cast<const f32x4_t*>(base + (size_t)(k0 + c) * 3 * D + 2 * D + 16 * j + 4 * g);
    }
    f32x4_t sq[LPT], sd[LPT], so[LPT];
    float sl = 0.f;
    auto gload = [&](int idx) {
      const size_t r0 = (size_t)b * N + idx * KC;
#pragma unroll
      for (int i = 0; i < LPT; ++i) {
        const int e = tid + i * NT;
        const size_t r = r0 + e / V4;
        sq[i] = *reinterpret_cast<const f32x4_t*>(qkv + r * 3 * D + (e % V4) * 4);
        sd[i] = *reinterpret_cast<const f32x4_t*>(dO + r * D + (e % V4) * 4);
        so[i] = *reinterpret_cast<const f32x4_t*>(o + r * D + (e % V4) * 4);
      }
      if (tid < KC) sl = lse[r0 + tid];
    };
    auto sstore = [&](int bufi) {
      float* buf = sm + bufi * 2 * KC * P;
      float* ex = ext + bufi * 2 * KC;
#pragma unroll
      for (int i = 0; i < LPT; ++i) {
        const int e = tid + i * NT;
        *reinterpret_cast<f32x4_t*>(buf + (e / V4) * P + (e % V4) * 4) = sq[i];
        *reinterpret_cast<f32x4_t*>(buf + KC * P + (e / V4) * P + (e % V4) * 4) = sd[i];
        float part = dot4(sd[i], so[i]);          // the V4 threads of a row are V4 consecutive lanes of one wave
#pragma unroll
        for (int m = 1; m < V4; m <<= 1) part += __shfl_xor(part, m, 64);
        if (e % V4 == 0) ex[KC + e / V4] = part;
      }
      if (tid < KC) ex[tid] = sl;
    };
    f32x4_t dk[NJ], dv[NJ];
#pragma unroll
    for (int t = 0; t < NJ; ++t) dk[t] = dv[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    const int nch = N / KC;
    gload(0);
    sstore(0);
    __syncthreads();
    for (int idx = 0; idx < nch; ++idx) {
      const float* cur = sm + (idx & 1) * 2 * KC * P;
      const float* ex = ext + (idx & 1) * 2 * KC;
      if (idx + 1 < nch) gload(idx + 1);
#pragma unroll
      for (int tt = 0; tt < TPC; ++tt) {
        f32x4_t s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f}, p, ds;
        tile_over_channels<D>(s, cur + tt * 16 * P, kf, c, g);                  // s[query 4g+i][key c]
        tile_over_channels<D>(dp, cur + KC * P + tt * 16 * P, vf, c, g);        // dP, same layout
        const f32x4_t l2 = *reinterpret_cast<const f32x4_t*>(ex + tt * 16 + 4 * g);
        const f32x4_t dl = *reinterpret_cast<const f32x4_t*>(ex + KC + tt * 16 + 4 * g);
        const float l2a[4] = {l2.x, l2.y, l2.z, l2.w}, dla[4] = {dl.x, dl.y, dl.z, dl.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          p[i] = __builtin_amdgcn_exp2f(fmaf(s[i], c2, -l2a[i]));
          ds[i] = p[i] * (dp[i] - dla[i]);
        }
        tile_over_rows<D>(dv, cur + KC * P + tt * 16 * P, p, c, g);             // dV^T += dO^T P
        tile_over_rows<D>(dk, cur + tt * 16 * P, ds, c, g);                     // dK^T += Q^T dS
      }
      if (idx + 1 < nch) {
        sstore((idx + 1) & 1);
        __syncthreads();
      }
    }
    float* dst = dqkv + ((size_t)b * N + k0 + c) * 3 * D;
    store_rows<D>(dst + D, dk, scale, g);
    store_rows<D>(dst + 2 * D, dv, 1.0f, g);
  }
};

template <int D, int NW>
__global__ __launch_bounds__(64 * NW) void attn_f32_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ dO,
                                                                const float* __restrict__ lse, const float* __restrict__ o,
                                                                float* __restrict__ dqkv, int N, float scale, float c2) {
  extern __shared__ f32x4_t attn_f32_smem[];
  float* sm = reinterpret_cast<float*>(attn_f32_smem);
  if (blockIdx.z == 0) Bwd<D, NW>::query_half(sm, qkv, dO, lse, o, dqkv, N, scale, c2);
  else Bwd<D, NW>::kv_half(sm, qkv, dO, lse, o, dqkv, N, scale, c2);
}

// ------------------------------------------------------------------------------------------------------------------ planner
// Strip rows per workgroup: 64 (four waves share every staged chunk) once the batch gives two rounds of 64-row workgroups on the
// 256 CUs, 32 below that -- a strip is one wave whatever the workgroup, so the smaller workgroup spreads the same waves over twice
// the CUs and halves what each CU stages.
int rows_per_wg(int B, int N) { return (long)B * N / 64 >= 512 ? 64 : 32; }

// Measured out (profiles/f32_attn.txt): N = 256, D = 128 below that threshold.  There a launch has at most one strip per SIMD, every
// wave waits out its own LDS and MFMA latencies, and the four generic batched GEMMs of the older route, which spread the same
// arithmetic over more waves, take less GPU time in the training step (B = 32: 103 us against 90 us per forward + backward).
bool covered(int B, int N, int D) {
  if (B < 0 || B > 65535 || (N != 64 && N != 256) || (D != 64 && D != 128)) return false;
  return !(N == 256 && D == 128 && B > 0 && rows_per_wg(B, N) == 32);
}

template <int N, int D, int NW>
hipError_t launch_fwd(const float* qkv, float* o, float* lse, int B, float c2, hipStream_t st) {
  using C = Cfg<D, NW>;
  static IdfLdsGrant grant;
  if (hipError_t e = idf_ensure_lds((const void*)attn_f32_fwd_kernel<N, D, NW>, C::LDS_FWD, grant); e != hipSuccess) return e;
  hipLaunchKernelGGL((attn_f32_fwd_kernel<N, D, NW>), dim3(N / C::QB, B), dim3(C::NT), C::LDS_FWD, st, qkv, o, lse, c2);
  return hipGetLastError();
}
template <int D, int NW>
void launch_bwd(const float* qkv, const float* dO, const float* lse, const float* o, float* dqkv, int B, int N, float scale,
                float c2, hipStream_t st) {
  using C = Cfg<D, NW>;
  hipLaunchKernelGGL((attn_f32_bwd_kernel<D, NW>), dim3(N / C::QB, B, 2), dim3(C::NT), C::LDS_BWD, st, qkv, dO, lse, o, dqkv, N,
                     scale, c2);
}

}  // namespace

extern "C" int idf_attn_f32_ok(int B, int N, int D) { return covered(B, N, D) ? 1 : 0; }

extern "C" int idf_attn_f32_fwd(const float* qkv, float* o, float* lse, int B, int N, int D, float scale, void* stream) {
  if (!covered(B, N, D)) IDF_FAIL(IDF_ERR_UNSUPPORTED, "idf_attn_f32_fwd: needs N in {64, 256}, D in {64, 128}, B >= 128 at N = 256 with D = 128 (B=%d N=%d D=%d)", B, N, D);
  if (!qkv || !o || !lse) IDF_FAIL(IDF_ERR_BADARG, "idf_attn_f32_fwd: null qkv, o or lse");
  if (B == 0) return IDF_OK;
  hipStream_t st = (hipStream_t)stream;
  const float c2 = scale * LOG2E;
  const bool big = rows_per_wg(B, N) == 64;
  hipError_t e;
#define IDF_ATTN_F32_FWD(N_, D_) \
  e = big ? launch_fwd<N_, D_, 4>(qkv, o, lse, B, c2, st) : launch_fwd<N_, D_, 2>(qkv, o, lse, B, c2, st)
  if (N == 256) { if (D == 128) e = launch_fwd<256, 128, 4>(qkv, o, lse, B, c2, st); else IDF_ATTN_F32_FWD(256, 64); }     // (256, 128): 64-row workgroups only, see covered()
  else { if (D == 128) IDF_ATTN_F32_FWD(64, 128); else IDF_ATTN_F32_FWD(64, 64); }
#undef IDF_ATTN_F32_FWD
  if (e != hipSuccess) IDF_FAIL(IDF_ERR_HIP, "idf_attn_f32_fwd: %s", hipGetErrorString(e));
  return IDF_OK;
}

extern "C" int idf_attn_f32_bwd(const float* qkv, const float* dO, const float* lse, const float* o, float* dqkv, int B, int N,
                                int D, float scale, void* stream) {
  if (!covered(B, N, D)) IDF_FAIL(IDF_ERR_UNSUPPORTED, "idf_attn_f32_bwd: needs N in {64, 256}, D in {64, 128}, B >= 128 at N = 256 with D = 128 (B=%d N=%d D=%d)", B, N, D);
  if (!qkv || !dO || !lse || !o || !dqkv) IDF_FAIL(IDF_ERR_BADARG, "idf_attn_f32_bwd: null qkv, dO, lse, o or dqkv");
  if (B == 0) return IDF_OK;
  hipStream_t st = (hipStream_t)stream;
  const float c2 = scale * LOG2E;
  const bool big = rows_per_wg(B, N) == 64;
  if (D == 128) { if (big) launch_bwd<128, 4>(qkv, dO, lse, o, dqkv, B, N, scale, c2, st); else launch_bwd<128, 2>(qkv, dO, lse, o, dqkv, B, N, scale, c2, st); }
  else { if (big) launch_bwd<64, 4>(qkv, dO, lse, o, dqkv, B, N, scale, c2, st); else launch_bwd<64, 2>(qkv, dO, lse, o, dqkv, B, N, scale, c2, st); }
  IDF_CHECK_LAUNCH();
  return IDF_OK;
}
