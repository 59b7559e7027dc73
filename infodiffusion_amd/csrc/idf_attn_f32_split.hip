// Fused fp32 single-head attention, forward and backward, on the bf16 MFMA of gfx950 (v_mfma_f32_16x16x32_bf16) with split
// operands -- the attention of the opt-in arithmetic modes bf16x3 / bf16x2 (idf_attn_f32.hip holds the exact-fp32 kernels whose
// work split this one keeps, idf_split_bf16.h the arithmetic).  DESIGN.md 4o has the mapping and the bank arithmetic.
//
// Work split: a wave owns a strip of 16 rows (queries; keys in the key/value half of the backward), a workgroup 4 strips.
// K and V (forward, query half) or Q and dO (key/value half) stream through LDS in chunks of 32 rows; scores and probabilities
// stay in registers; softmax (max, exp2, sum) is fp32 VALU work as in the exact kernel; only MFMA operands are split.
//
// MFMA 16x16x32 operand layout, lane = 16 g + c:  A[m = c][k = 8 g + e], B[k = 8 g + e][n = c], e = 0 .. 7 the elements of the
// lane's bf16x8; D[m = 4 g + i][n = c] in register i.
//
//   channel contraction (scores, dP): k slot 8 g + e of step j is channel 32 j + 8 g + e.  A = 16 bytes of row c of the streamed
//     chunk per term (one ds_read_b128 from the term's plane), B = the lane's own row, loaded once from global memory and split
//     once into TERMS register fragments per step.  Result: register i of lane (c, g) = score[streamed row 4 g + i][own row c].
//   row contraction (P V, dS K, P^T dO, dS^T Q): 32 streamed rows = two 16-row score tiles t = 0, 1; k slot 8 g + 4 t + i is row
//     16 t + 4 g + i -- exactly where the score MFMAs left P (or dS): the eight registers (t, i) of a lane, split in registers,
//     ARE the B operand, no shuffle.  A[m = channel][k] is the streamed matrix transposed: ds_read_b64_tr_b16 on the row-major
//     plane, lane (g, q = c / 4, pp = c % 4) reads the 8 bytes of channels 16 h + 4 pp .. + 3 of row 16 t + 4 g + q and receives
//     channel 16 h + c of rows 16 t + 4 g .. + 3 (t = 0: low half of the fragment, t = 1: high half).  Output tile h holds
//     channels 16 h + 4 g + i of own row c in register i: one 16-byte store per tile.
//
// Staging: thread = 8 channels (two 16-byte loads, held in registers across the MFMAs of the chunk before) of one streamed row;
// split8 once on the way into LDS, TERMS 16-byte stores into the row's TERMS planes.
//   LDS row r of a chunk: r * PITCH + 16 * (r / 8 % 2), PITCH = TERMS * 2 D + 32 bytes, term t at + t * 2 D.
// PITCH is an odd multiple of 32 B (mod 256): the 8 rows of a transposed-read pass fall on 8 distinct 32-byte groups; the 16-byte
// shift of rows 8 .. 15 puts the 16 rows of a ds_read_b128 pass on 16 distinct 16-byte groups.
// Forward: two buffers of 32 rows, one barrier a chunk: 51200 B at D = 128, three terms.  Backward: two matrices a chunk, ONE
// buffer, two barriers a chunk (51456 B).  Both stay under 64 KB; the launches still go through idf_ensure_lds.
//
// Fixed summation order, one writer per output element, no atomics: a second call is bit-identical.
// Non-finite inputs, and magnitudes that round to the bf16 infinity, give non-finite outputs (inf - inf in the split).
#include "idf_common.h"
#include "idf_split_bf16.h"

#include <math.h>

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr int KC = 32;      // streamed rows per chunk of the backward: one row-contraction step
// forward: the same 32 rows (64-row chunks measured 26.8 against 27.6 us at (32, 256, 128): not what bounds it, and they leave one
// workgroup per CU at D = 128 with three terms)
constexpr int kc_fwd(int NW) { return 32; }

template <int D, int NW, int TERMS, int ROWS = KC>
struct Cfg {
  static constexpr int NT = 64 * NW;                      // threads
  static constexpr int QB = 16 * NW;                      // strip rows per workgroup
  static constexpr int PLANE = 2 * D;                     // bytes of a row in one term's plane
  static constexpr int PITCH = TERMS * PLANE + 32;        // bytes per staged row
  static constexpr int V8 = D / 8;                        // staging items (8 channels) per row
  static constexpr int NJ = D / 32;                       // channel steps
  static constexpr int NH = D / 16;                       // output tiles
  static constexpr int ITEMS = ROWS * V8 / NT;            // staging items per thread, chunk and matrix
  static constexpr int MAT = ROWS * PITCH;                // bytes of one staged matrix chunk
  static constexpr size_t LDS_FWD = (size_t)2 * MAT;
  static constexpr size_t LDS_BWD = (size_t)2 * MAT + 2 * KC * sizeof(float);
  static_assert(ITEMS * NT == ROWS * V8 && ITEMS >= 1 && ROWS % 32 == 0, "staging");
};

__device__ __forceinline__ int row_off(int r, int pitch) { return r * pitch + ((r & 8) << 1); }

__device__ __forceinline__ float q16_max(float v) {       // over the four lanes c, c + 16, c + 32, c + 48
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float q16_sum(float v) {       // same four lanes; every lane ends with the same bits
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}
__device__ __forceinline__ float dot4(const f32x4_t& a, const f32x4_t& b) { return ((a.x * b.x + a.y * b.y) + a.z * b.z) + a.w * b.w; }
__device__ __forceinline__ float4 f4(const f32x4_t& v) { return make_float4(v[0], v[1], v[2], v[3]); }

__device__ __forceinline__ s16x4_t tr_read(const unsigned char* lds_ptr) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(lds_ptr));
}
__device__ __forceinline__ bf16x8_t mkfrag(s16x4_t lo, s16x4_t hi) {
  union { struct { s16x4_t a, b; } s; bf16x8_t v; } u;
  u.s.a = lo; u.s.b = hi;
  return u.v;
}

// the lane's own row (D floats at src) -> NJ x TERMS register fragments: step j = channels 32 j + 8 g .. + 7
template <int D, int TERMS>
__device__ __forceinline__ void own_frags(const float* __restrict__ src, int g, bf16x8_t (*fr)[TERMS]) {
#pragma unroll
  for (int j = 0; j < D / 32; ++j) {
    const f32x4_t a = *reinterpret_cast<const f32x4_t*>(src + 32 * j + 8 * g);
    const f32x4_t b = *reinterpret_cast<const f32x4_t*>(src + 32 * j + 8 * g + 4);
    uint4 tv[TERMS];
    split8<TERMS>(f4(a), f4(b), tv);
#pragma unroll
    for (int t = 0; t < TERMS; ++t) fr[j][t] = as_bf16x8(tv[t]);
  }
}

// one staged matrix chunk: ROWS rows of D floats (row stride ld) -> registers -> TERMS bf16 planes
template <int D, int NW, int TERMS, int ROWS = KC>
struct Stage {
  using C = Cfg<D, NW, TERMS, ROWS>;
  f32x4_t v[C::ITEMS][2];
  __device__ __forceinline__ void load(const float* __restrict__ src, size_t ld, int tid) {
#pragma unroll
    for (int i = 0; i < C::ITEMS; ++i) {
      const int e = tid + i * C::NT;
      const float* p = src + (size_t)(e / C::V8) * ld + (e % C::V8) * 8;
      v[i][0] = *reinterpret_cast<const f32x4_t*>(p);
      v[i][1] = *reinterpret_cast<const f32x4_t*>(p + 4);
    }
  }
  __device__ __forceinline__ void store(unsigned char* buf, int tid) const {
#pragma unroll
    for (int i = 0; i < C::ITEMS; ++i) {
      const int e = tid + i * C::NT;
      uint4 tv[TERMS];
      split8<TERMS>(f4(v[i][0]), f4(v[i][1]), tv);
      unsigned char* dst = buf + row_off(e / C::V8, C::PITCH) + (e % C::V8) * 16;
#pragma unroll
      for (int t = 0; t < TERMS; ++t) *reinterpret_cast<uint4*>(dst + t * C::PLANE) = tv[t];
    }
  }
};

// one 16 x 16 tile of a channel contraction: acc[m][n] += sum_d rows[m][d] * own[n][d]; rows = 16 staged rows from row r0 on
template <int D, int TERMS>
__device__ __forceinline__ f32x4_t tile_over_channels(f32x4_t acc, const unsigned char* mat, int r0, const bf16x8_t (*own)[TERMS],
                                                      int c, int g) {
  constexpr int PLANE = 2 * D, PITCH = TERMS * PLANE + 32;
  const unsigned char* row = mat + row_off(r0 + c, PITCH) + 16 * g;
#pragma unroll
  for (int j = 0; j < D / 32; ++j) {
    bf16x8_t a[TERMS];
#pragma unroll
    for (int t = 0; t < TERMS; ++t) a[t] = as_bf16x8(*reinterpret_cast<const uint4*>(row + t * PLANE + 64 * j));
    acc = split_mfma<TERMS>(a, own[j], acc);
  }
  return acc;
}

// a row contraction over 32 staged rows from row r0 on: out[h][m][n] += sum_r mat[r][16 h + m] * w[r][n], w = the two score-layout tiles
template <int D, int TERMS>
__device__ __forceinline__ void chunk_over_rows(f32x4_t* out, const unsigned char* mat, int r0, const f32x4_t& w0, const f32x4_t& w1,
                                                int c, int g) {
  constexpr int PLANE = 2 * D, PITCH = TERMS * PLANE + 32;
  uint4 tv[TERMS];
  split8<TERMS>(f4(w0), f4(w1), tv);
  bf16x8_t wf[TERMS];
#pragma unroll
  for (int t = 0; t < TERMS; ++t) wf[t] = as_bf16x8(tv[t]);
  const int r = r0 + 4 * g + (c >> 2);
  const unsigned char* lo = mat + row_off(r, PITCH) + (c & 3) * 8;
  const unsigned char* hi = mat + row_off(r + 16, PITCH) + (c & 3) * 8;
#pragma unroll
  for (int h = 0; h < D / 16; ++h) {
    bf16x8_t a[TERMS];
#pragma unroll
    for (int t = 0; t < TERMS; ++t) a[t] = mkfrag(tr_read(lo + t * PLANE + 32 * h), tr_read(hi + t * PLANE + 32 * h));
    out[h] = split_mfma<TERMS>(a, wf, out[h]);
  }
}

// out tiles -> own row c (D floats at dst), scaled
template <int D>
__device__ __forceinline__ void store_rows(float* __restrict__ dst, const f32x4_t* out, float s, int g) {
#pragma unroll
  for (int h = 0; h < D / 16; ++h) *reinterpret_cast<f32x4_t*>(dst + 16 * h + 4 * g) = out[h] * s;
}

// ------------------------------------------------------------------------------------------------------------------ forward
// grid (N / QB, B); a wave owns 16 queries.  c2 = scale * log2(e); lse2 = log2 of the row sum of 2^(c2 * s).
template <int N, int D, int NW, int TERMS>
__global__ __launch_bounds__(64 * NW) void attn_f32_split_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ o,
                                                                      float* __restrict__ lse, float c2) {
  constexpr int KC = kc_fwd(NW), NCH = N / KC, TPC = KC / 16;
  using C = Cfg<D, NW, TERMS, KC>;
  static_assert(NCH * KC == N, "chunking");
  extern __shared__ uint4 attn_split_smem[];
  unsigned char* sm = reinterpret_cast<unsigned char*>(attn_split_smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
  const int b = blockIdx.y, q0 = blockIdx.x * C::QB + wave * 16;
  const float* base = qkv + (size_t)b * N * 3 * D;

  bf16x8_t qf[C::NJ][TERMS];
  own_frags<D, TERMS>(base + (size_t)(q0 + c) * 3 * D, g, qf);

  Stage<D, NW, TERMS, KC> stg;
  auto gload = [&](int idx) {      // chunk idx of the sequence K chunks | V chunks
    stg.load(base + (idx < NCH ? D : 2 * D) + (size_t)((idx < NCH ? idx : idx - NCH) * KC) * 3 * D, 3 * D, tid);
  };

  f32x4_t acc[N / 16];
#pragma unroll
  for (int t = 0; t < N / 16; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  f32x4_t out[C::NH];
#pragma unroll
  for (int t = 0; t < C::NH; ++t) out[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float mx = 0.f, sum = 0.f;

  gload(0);
  stg.store(sm, tid);
  __syncthreads();
#pragma unroll
  for (int idx = 0; idx < 2 * NCH; ++idx) {
    const unsigned char* cur = sm + (idx & 1) * C::MAT;
    if (idx + 1 < 2 * NCH) gload(idx + 1);          // in flight under this chunk's MFMAs
    if (idx < NCH) {
#pragma unroll
      for (int tt = 0; tt < TPC; ++tt) acc[idx * TPC + tt] = tile_over_channels<D, TERMS>(acc[idx * TPC + tt], cur, 16 * tt, qf, c, g);
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
      for (int tt = 0; tt < TPC; tt += 2)
        chunk_over_rows<D, TERMS>(out, cur, 16 * tt, acc[(idx - NCH) * TPC + tt], acc[(idx - NCH) * TPC + tt + 1], c, g);
    }
    if (idx + 1 < 2 * NCH) {
      stg.store(sm + ((idx + 1) & 1) * C::MAT, tid);        // last read in iteration idx - 1, before that iteration's barrier
      __syncthreads();
    }
  }
  store_rows<D>(o + ((size_t)b * N + q0 + c) * D, out, 1.0f / sum, g);
  if (g == 0) lse[(size_t)b * N + q0 + c] = mx * c2 + log2f(sum);
}

// ----------------------------------------------------------------------------------------------------------------- backward
// grid (N / QB, B, 2): z = 0 the query half (strip = 16 queries, streams K | V, writes dQ), z = 1 the key/value half (strip = 16
// keys, streams Q | dO and forms delta = rowsum(dO . O) of the streamed rows, writes dK and dV).  One LDS buffer: the next chunk
// waits in registers under this chunk's MFMAs and is split and stored between the chunk's two barriers.
template <int D, int NW, int TERMS>
struct Bwd {
  using C = Cfg<D, NW, TERMS>;

  static __device__ __forceinline__ void query_half(unsigned char* sm, const float* __restrict__ qkv, const float* __restrict__ dO,
                                                    const float* __restrict__ lse, const float* __restrict__ o,
                                                    float* __restrict__ dqkv, int N, float scale, float c2) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
    const int b = blockIdx.y, q0 = blockIdx.x * C::QB + wave * 16;
    const float* base = qkv + (size_t)b * N * 3 * D;
    const size_t row = (size_t)b * N + q0 + c;
    bf16x8_t qf[C::NJ][TERMS], dof[C::NJ][TERMS];
    own_frags<D, TERMS>(base + (size_t)(q0 + c) * 3 * D, g, qf);
    own_frags<D, TERMS>(dO + row * D, g, dof);
    float delta = 0.f;
#pragma unroll
    for (int j = 0; j < C::NJ; ++j)
#pragma unroll
      for (int h = 0; h < 2; ++h)
        delta += dot4(*reinterpret_cast<const f32x4_t*>(dO + row * D + 32 * j + 8 * g + 4 * h),
                      *reinterpret_cast<const f32x4_t*>(o + row * D + 32 * j + 8 * g + 4 * h));
    delta = q16_sum(delta);
    const float l2 = lse[row];

    Stage<D, NW, TERMS> sk, sv;
    auto gload = [&](int idx) {
      sk.load(base + D + (size_t)(idx * KC) * 3 * D, 3 * D, tid);
      sv.load(base + 2 * D + (size_t)(idx * KC) * 3 * D, 3 * D, tid);
    };
    unsigned char* kb = sm;
    unsigned char* vb = sm + C::MAT;
    f32x4_t dq[C::NH];
#pragma unroll
    for (int t = 0; t < C::NH; ++t) dq[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    const int nch = N / KC;
    gload(0);
    for (int idx = 0; idx < nch; ++idx) {
      sk.store(kb, tid);
      sv.store(vb, tid);
      __syncthreads();
      if (idx + 1 < nch) gload(idx + 1);
      f32x4_t ds[2];
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        const f32x4_t z = {0.f, 0.f, 0.f, 0.f};
        const f32x4_t s = tile_over_channels<D, TERMS>(z, kb, 16 * tt, qf, c, g);       // s[key 4g+i][query c]
        const f32x4_t dp = tile_over_channels<D, TERMS>(z, vb, 16 * tt, dof, c, g);     // dP, same layout
#pragma unroll
        for (int i = 0; i < 4; ++i) ds[tt][i] = __builtin_amdgcn_exp2f(fmaf(s[i], c2, -l2)) * (dp[i] - delta);
      }
      chunk_over_rows<D, TERMS>(dq, kb, 0, ds[0], ds[1], c, g);                            // dQ^T += K^T dS^T
      __syncthreads();          // every fragment read of this chunk before the next chunk's stores
    }
    store_rows<D>(dqkv + row * 3 * D, dq, scale, g);
  }

  static __device__ __forceinline__ void kv_half(unsigned char* sm, const float* __restrict__ qkv, const float* __restrict__ dO,
                                                 const float* __restrict__ lse, const float* __restrict__ o,
                                                 float* __restrict__ dqkv, int N, float scale, float c2) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
    const int b = blockIdx.y, k0 = blockIdx.x * C::QB + wave * 16;
    const float* base = qkv + (size_t)b * N * 3 * D;
    unsigned char* qb = sm;
    unsigned char* db = sm + C::MAT;
    float* ex = reinterpret_cast<float*>(sm + 2 * C::MAT);       // [lse2 | delta][KC]
    bf16x8_t kf[C::NJ][TERMS], vf[C::NJ][TERMS];
    own_frags<D, TERMS>(base + (size_t)(k0 + c) * 3 * D + D, g, kf);
    own_frags<D, TERMS>(base + (size_t)(k0 + c) * 3 * D + 2 * D, g, vf);

    Stage<D, NW, TERMS> sq, sd, so;
    float sl = 0.f;
    auto gload = [&](int idx) {
      const size_t r0 = (size_t)b * N + idx * KC;
      sq.load(qkv + r0 * 3 * D, 3 * D, tid);
      sd.load(dO + r0 * D, D, tid);
      so.load(o + r0 * D, D, tid);
      if (tid < KC) sl = lse[r0 + tid];
    };
    auto sstore = [&]() {
      sq.store(qb, tid);
      sd.store(db, tid);
#pragma unroll
      for (int i = 0; i < C::ITEMS; ++i) {
        const int e = tid + i * C::NT;
        float part = dot4(sd.v[i][0], so.v[i][0]) + dot4(sd.v[i][1], so.v[i][1]);
#pragma unroll
        for (int m = 1; m < C::V8; m <<= 1) part += __shfl_xor(part, m, 64);      // the V8 threads of a row: consecutive lanes of one wave
        if (e % C::V8 == 0) ex[KC + e / C::V8] = part;
      }
      if (tid < KC) ex[tid] = sl;
    };
    f32x4_t dk[C::NH], dv[C::NH];
#pragma unroll
    for (int t = 0; t < C::NH; ++t) dk[t] = dv[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    const int nch = N / KC;
    gload(0);
    for (int idx = 0; idx < nch; ++idx) {
      sstore();
      __syncthreads();
      if (idx + 1 < nch) gload(idx + 1);
      f32x4_t p[2], ds[2];
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        const f32x4_t z = {0.f, 0.f, 0.f, 0.f};
        const f32x4_t s = tile_over_channels<D, TERMS>(z, qb, 16 * tt, kf, c, g);       // s[query 4g+i][key c]
        const f32x4_t dp = tile_over_channels<D, TERMS>(z, db, 16 * tt, vf, c, g);      // dP, same layout
        const f32x4_t l2 = *reinterpret_cast<const f32x4_t*>(ex + tt * 16 + 4 * g);
        const f32x4_t dl = *reinterpret_cast<const f32x4_t*>(ex + KC + tt * 16 + 4 * g);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          p[tt][i] = __builtin_amdgcn_exp2f(fmaf(s[i], c2, -l2[i]));
          ds[tt][i] = p[tt][i] * (dp[i] - dl[i]);
        }
      }
      chunk_over_rows<D, TERMS>(dv, db, 0, p[0], p[1], c, g);                              // dV^T += dO^T P
      chunk_over_rows<D, TERMS>(dk, qb, 0, ds[0], ds[1], c, g);                            // dK^T += Q^T dS
      __syncthreads();
    }
    float* dst = dqkv + ((size_t)b * N + k0 + c) * 3 * D;
    store_rows<D>(dst + D, dk, scale, g);
    store_rows<D>(dst + 2 * D, dv, 1.0f, g);
  }
};

template <int D, int NW, int TERMS>
__global__ __launch_bounds__(64 * NW) void attn_f32_split_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ dO,
                                                                      const float* __restrict__ lse, const float* __restrict__ o,
                                                                      float* __restrict__ dqkv, int N, float scale, float c2) {
  extern __shared__ uint4 attn_split_smem[];
  unsigned char* sm = reinterpret_cast<unsigned char*>(attn_split_smem);
  if (blockIdx.z == 0) Bwd<D, NW, TERMS>::query_half(sm, qkv, dO, lse, o, dqkv, N, scale, c2);
  else Bwd<D, NW, TERMS>::kv_half(sm, qkv, dO, lse, o, dqkv, N, scale, c2);
}

// ------------------------------------------------------------------------------------------------------------------ planner
// Strip rows per workgroup: 64 at every batch size, unlike the exact kernel.  The split of a staged chunk is VALU work of about the
// size of the chunk's MFMAs (about 90 instructions per 8 values at three terms) and every wave of the workgroup does a 1 / waves
// share of it: with 32-row workgroups the (32, 256, 128) forward measured 27.2 us in GPU time (profiles/f32_attn_split.txt).
constexpr int NWAVES = 4;

bool covered(int B, int N, int D, int terms) {
  if (terms != 2 && terms != 3) return false;
  return B >= 0 && B <= 65535 && (N == 64 || N == 256) && (D == 64 || D == 128);
}

template <int N, int D, int NW, int TERMS>
hipError_t launch_fwd(const float* qkv, float* o, float* lse, int B, float c2, hipStream_t st) {
  using C = Cfg<D, NW, TERMS, kc_fwd(NW)>;
  static IdfLdsGrant grant;
  if (hipError_t e = idf_ensure_lds((const void*)attn_f32_split_fwd_kernel<N, D, NW, TERMS>, C::LDS_FWD, grant); e != hipSuccess)
    return e;
  hipLaunchKernelGGL((attn_f32_split_fwd_kernel<N, D, NW, TERMS>), dim3(N / C::QB, B), dim3(C::NT), C::LDS_FWD, st, qkv, o, lse, c2);
  return hipGetLastError();
}
template <int TERMS>
hipError_t fwd_shape(int N, int D, const float* qkv, float* o, float* lse, int B, float c2, hipStream_t st) {
  if (N == 256)
    return D == 128 ? launch_fwd<256, 128, NWAVES, TERMS>(qkv, o, lse, B, c2, st) : launch_fwd<256, 64, NWAVES, TERMS>(qkv, o, lse, B, c2, st);
  return D == 128 ? launch_fwd<64, 128, NWAVES, TERMS>(qkv, o, lse, B, c2, st) : launch_fwd<64, 64, NWAVES, TERMS>(qkv, o, lse, B, c2, st);
}

template <int D, int NW, int TERMS>
hipError_t launch_bwd(const float* qkv, const float* dO, const float* lse, const float* o, float* dqkv, int B, int N, float scale,
                      float c2, hipStream_t st) {
  using C = Cfg<D, NW, TERMS>;
  static IdfLdsGrant grant;
  if (hipError_t e = idf_ensure_lds((const void*)attn_f32_split_bwd_kernel<D, NW, TERMS>, C::LDS_BWD, grant); e != hipSuccess) return e;
  hipLaunchKernelGGL((attn_f32_split_bwd_kernel<D, NW, TERMS>), dim3(N / C::QB, B, 2), dim3(C::NT), C::LDS_BWD, st, qkv, dO, lse, o,
                     dqkv, N, scale, c2);
  return hipGetLastError();
}
template <int TERMS>
hipError_t bwd_shape(int D, const float* qkv, const float* dO, const float* lse, const float* o, float* dqkv, int B, int N,
                     float scale, float c2, hipStream_t st) {
  return D == 128 ? launch_bwd<128, NWAVES, TERMS>(qkv, dO, lse, o, dqkv, B, N, scale, c2, st)
                  : launch_bwd<64, NWAVES, TERMS>(qkv, dO, lse, o, dqkv, B, N, scale, c2, st);
}

}  // namespace

extern "C" int idf_attn_f32_split_ok(int B, int N, int D, int terms) { return covered(B, N, D, terms) ? 1 : 0; }

extern "C" int idf_attn_f32_split_fwd(const float* qkv, float* o, float* lse, int B, int N, int D, float scale, int terms,
                                      void* stream) {
  if (!covered(B, N, D, terms))
    IDF_FAIL(IDF_ERR_UNSUPPORTED, "idf_attn_f32_split_fwd: needs terms 2 or 3, N in {64, 256}, D in {64, 128} (B=%d N=%d D=%d terms=%d)", B, N, D, terms);
  if (!qkv || !o || !lse) IDF_FAIL(IDF_ERR_BADARG, "idf_attn_f32_split_fwd: null qkv, o or lse");
  if (B == 0) return IDF_OK;
  hipStream_t st = (hipStream_t)stream;
  const float c2 = scale * LOG2E;
  const hipError_t e = terms == 3 ? fwd_shape<3>(N, D, qkv, o, lse, B, c2, st) : fwd_shape<2>(N, D, qkv, o, lse, B, c2, st);
  if (e != hipSuccess) IDF_FAIL(IDF_ERR_HIP, "idf_attn_f32_split_fwd: %s", hipGetErrorString(e));
  return IDF_OK;
}

extern "C" int idf_attn_f32_split_bwd(const float* qkv, const float* dO, const float* lse, const float* o, float* dqkv, int B, int N,
                                      int D, float scale, int terms, void* stream) {
  if (!covered(B, N, D, terms))
    IDF_FAIL(IDF_ERR_UNSUPPORTED, "idf_attn_f32_split_bwd: needs terms 2 or 3, N in {64, 256}, D in {64, 128} (B=%d N=%d D=%d terms=%d)", B, N, D, terms);
  if (!qkv || !dO || !lse || !o || !dqkv) IDF_FAIL(IDF_ERR_BADARG, "idf_attn_f32_split_bwd: null qkv, dO, lse, o or dqkv");
  if (B == 0) return IDF_OK;
  hipStream_t st = (hipStream_t)stream;
  const float c2 = scale * LOG2E;
  const hipError_t e = terms == 3 ? bwd_shape<3>(D, qkv, dO, lse, o, dqkv, B, N, scale, c2, st)
                                  : bwd_shape<2>(D, qkv, dO, lse, o, dqkv, B, N, scale, c2, st);
  if (e != hipSuccess) IDF_FAIL(IDF_ERR_HIP, "idf_attn_f32_split_bwd: %s", hipGetErrorString(e));
  return IDF_OK;
}
