// fp32 3x3 stride-1 NHWC convolution (forward, and the data gradient with the flipped weight shadow) on the bf16 MFMA of
// gfx950 with split operands -- the opt-in arithmetic modes bf16x3 / bf16x2 of the fp32 path (gfx950 has no xf32 MFMA).
//
//   y[b,oy,ox,n] = bias[n] + res[b,oy,ox,n] + sum_{ky,kx,c} x[b,oy+ky-1,ox+kx-1,c] * w[n][ky*3+kx][c]
//
// Every fp32 operand is written as a sum of bf16 terms, v = h + m (+ l): h = bf16(v), m = bf16(v - h), l = bf16(v - h - m), each
// rounding to nearest even (the subtractions are exact in fp32).  Only the significant cross products are formed, on
// v_mfma_f32_16x16x32_bf16 into ONE fp32 accumulator, smallest first:
//   TERMS 3 (bf16x3): mm, hl, lh, hm, mh, hh  -- 6 MFMAs per 32-deep K step; dropped: ml, lm, ll (< 3 * 2^-27 per product)
//   TERMS 2 (bf16x2): hm, mh, hh              -- 3 MFMAs; dropped: mm and the third terms (<= 3 * 2^-18 per product)
// against the 8 v_mfma_f32_16x16x4_f32 of the exact kernel (idf_conv3x3_f32.hip), whose work split this kernel keeps: a
// 256-thread workgroup owns R whole rows x W columns of one image (BM = 64 / 128 / 256 pixel slots, the last row tile of an
// image masks rows) times a 64-wide cout tile (Cout <= 16: one 16-wide tile).  Fixed summation order, no atomics.
//
// Activations are split ONCE per workgroup, at staging: K runs over Cin in chunks of 32 channels (one MFMA K step); per chunk
// the (R+2) x (W+2) halo slab is loaded as fp32 from global memory, split in registers and stored to LDS as TERMS bf16 planes
// per pixel (border pixels as zeros: no bounds checks in the tap loop), where it serves all 9 taps.
//
// LDS layout: slab[pixel][TERMS planes x 64 B + 16 B pad] -- pitch 208 B (13 quads of 16 B) at three terms, 144 B (9 quads) at
// two.  A lane's B operand of a (pixel 16-tile, tap, plane) is ONE ds_read_b128: pixel l%16, channels 8 * (l/16) .. +7, at byte
// pitch * pix + 64 * plane + 16 * (l/16).  The 16 lanes of a quarter read 16 consecutive slab pixels (16 | W), i.e. quads
// (13 i + const) mod 16 resp. (9 i + const) mod 16 for i = pix0 .. pix0+15: the stride is odd, so these are 16 distinct quads of
// the 64 banks -- conflict-free.  (The unpadded pitches, 12 and 8 quads, would be 4- and 8-way.)
//
// One slab buffer: at 2.6x the exact kernel's bytes per staged pixel two buffers of the 256-pixel tile (2 x 82 KB) do not fit a
// CU even once.  The fp32 global loads of chunk k+1 are issued before the MFMAs of chunk k and held in registers across
// them; after a barrier they are split and stored into the same buffer -- two barriers per chunk, covered by the second
// workgroup of the CU (slabs are capped at 80 KB: two workgroups per CU; a tile whose slab is larger takes the next smaller
// form, which is the 64-wide maps at three terms: 128-pixel tiles).
//
// Weights do not pass through LDS and are not split here: idf_split_weight_bf16 turns the fp32 shadow [rows][9][Cin] into a
// fragment-major bf16 shadow -- for each (cout 16-tile, tap, 32-channel chunk, term) the 64 lanes' 16-byte A operands
// contiguously (rows past `rows` as zeros) -- so a lane's A operand is one global_load_dwordx4 per term, issued one (tap, cout
// tile) step ahead of the MFMAs that use it.
//
// Non-finite inputs, and magnitudes that round to the bf16 infinity, give non-finite outputs (inf - inf in the split).
#include "idf_common.h"
#include "idf_split_bf16.h"

namespace {

constexpr int KC = 32;                 // channels per K chunk = one MFMA K step
constexpr int FULL_GRID = 512;         // two workgroups on each of the 256 CUs
constexpr int LDS_CAP = 80 * 1024;     // per workgroup: two per CU
constexpr int pitch_of(int terms) { return terms * 64 + 16; }      // bytes per staged pixel

struct S3P {
  const float* x;
  const uint4* w;       // fragment-major split shadow
  const float* bias;
  const float* res;
  float* y;
  int B, H, W, Cin, Cout;
  int R, tiles, n_tiles, w_tiles;      // rows per tile, row tiles per image, cout tiles, 16-row tiles of the shadow
};

struct Plan { int bm, bn, R, tiles, n_tiles, slab_px; };

// staging items (8 channels of one slab pixel, held as fp32 across a chunk's MFMAs) per thread each kernel form has room for
// (NS * 256 >= 4 * slab pixels); 6 at the three-term 256-pixel tile, whose slabs end at 80 KB / 208 B = 393 pixels anyway: the
// seventh item is the 8 registers that keep that form out of scratch
constexpr int ns_of(int bm, int terms) { return bm == 256 ? (terms == 3 ? 6 : 7) : bm == 128 ? 5 : 4; }

// Tile shape for a covered problem; false: not covered.  The rule of idf_conv3x3_f32.hip -- the largest pixel tile that still
// gives the chip two workgroups per CU, images up to 8x8 as one tile -- among the tiles whose slab fits LDS_CAP.
bool plan_of(int B, int H, int W, int Cin, int Cout, int terms, Plan* pl) {
  if (terms != 2 && terms != 3) return false;
  if (B < 1 || H < 4 || W < 4 || W > 64 || Cin < 32 || (Cin % 32) || Cout < 1) return false;
  // measured out (profiles/f32_split.txt section 1): two terms on maps of <= 64 pixels at B >= 32 did not beat the exact kernel
  if (terms == 2 && H * W <= 64 && B >= 32) return false;
  const long lim = 1L << 31;
  if ((long)H * W * Cin >= lim || (long)H * W * Cout >= lim || (long)(Cout + 15) * 9 * Cin * terms >= lim / 2) return false;
  Plan p;
  p.bn = Cout <= 16 ? 16 : 64;
  p.n_tiles = idf_cdiv(Cout, p.bn);
  const int bms[4] = {256, 128, 64, 0};
  bool found = false;
  for (int i = 0; i < 3 && !found; ++i) {
    p.bm = bms[i];
    if ((long)H * W <= 64) p.bm = 64;           // images up to 8x8: one tile
    p.R = p.bm / W < H ? p.bm / W : H;
    p.tiles = idf_cdiv(H, p.R);
    p.slab_px = (p.R + 2) * (W + 2);
    const bool fits = p.slab_px * 4 <= ns_of(p.bm, terms) * 256 && p.slab_px * pitch_of(terms) <= LDS_CAP;
    const bool smaller_ok = p.bm > 64 && (bms[i + 1] / W >= 2);
    if (!fits) {
      if (!smaller_ok) return false;
      continue;
    }
    found = !smaller_ok || (long)B * p.tiles * p.n_tiles >= FULL_GRID;
  }
  if (!found || (long)B * p.tiles * p.n_tiles >= lim) return false;
  *pl = p;
  return true;
}

// TM pixel 16-tiles x TN cout 16-tiles per wave, waves WM (pixel) x WN (cout): BM = 16 * TM * WM pixel slots, BN couts.
template <int TERMS, int TM, int WM, int WN, int NS, int BN>
__global__ __launch_bounds__(256, 2) void conv3x3_split_kernel(const S3P p) {
  constexpr int TN = BN / 16 / WN;
  constexpr int PITCH = pitch_of(TERMS);
  static_assert(WM * WN == 4 && TN >= 1, "4 waves");
  extern __shared__ __attribute__((aligned(16))) unsigned char slab[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int wm = wave % WM, wn = wave / WM;
  int bid = blockIdx.x;
  const int tn = bid % p.n_tiles;
  bid /= p.n_tiles;
  const int tr = bid % p.tiles, b = bid / p.tiles;
  const int row0 = tr * p.R, n0 = tn * BN;
  const int SW = p.W + 2, slab_px = (p.R + 2) * SW, RW = p.R * p.W;

  const float* __restrict__ X = p.x + (size_t)b * p.H * p.W * p.Cin;

  // staging: item i = tid + 256 j is channels 8 * (i & 3) .. +7 of slab pixel i >> 2; goff < 0: padding, staged as zeros
  int goff[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    const int i = tid + 256 * j, px = i >> 2;
    const int sr = px / SW, sc = px - sr * SW;
    const int iy = row0 + sr - 1, ix = sc - 1;
    const bool ok = px < slab_px && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
    goff[j] = ok ? (iy * p.W + ix) * p.Cin + (i & 3) * 8 : -1;
  }
  float4 sv[NS][2];
  // (two selects, not one branch around both loads: that form crashed the ROCm 7.2 back end in machine copy propagation)
  auto stage_load = [&](int c0) {
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      sv[j][0] = goff[j] >= 0 ? *reinterpret_cast<const float4*>(X + goff[j] + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
      sv[j][1] = goff[j] >= 0 ? *reinterpret_cast<const float4*>(X + goff[j] + c0 + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto stage_store = [&]() {
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      const int i = tid + 256 * j;
      if (i < slab_px * 4) {
        uint4 tv[TERMS];
        split8<TERMS>(sv[j][0], sv[j][1], tv);
#pragma unroll
        for (int t = 0; t < TERMS; ++t) *reinterpret_cast<uint4*>(slab + (i >> 2) * PITCH + t * 64 + (i & 3) * 16) = tv[t];
      }
    }
  };

  // fragment addresses: slab byte offset of the lane's pixel at tap (0, 0) (slots past the tile read pixel 0 and are not stored)
  int xoff[TM];
#pragma unroll
  for (int t = 0; t < TM; ++t) {
    int m = (wm * TM + t) * 16 + fr;
    if (m >= RW) m = 0;
    const int r = m / p.W, c = m - r * p.W;
    xoff[t] = (r * SW + c) * PITCH + 16 * fq;
  }
  // ... and of its cout 16-tiles in the split shadow, in uint4 (tiles past the shadow read its last tile and are not stored)
  const int nchunk = p.Cin / KC;
  int woff[TN];
#pragma unroll
  for (int a = 0; a < TN; ++a) {
    int nt = n0 / 16 + wn * TN + a;
    if (nt >= p.w_tiles) nt = p.w_tiles - 1;
    woff[a] = nt * 9 * nchunk * TERMS * 64 + lane;
  }
  const bf16x8_t* __restrict__ Wt = reinterpret_cast<const bf16x8_t*>(p.w);
  auto load_w = [&](bf16x8_t* dst, int a, int tap, int ch) {
    const bf16x8_t* src = Wt + woff[a] + (tap * nchunk + ch) * (TERMS * 64);
#pragma unroll
    for (int t = 0; t < TERMS; ++t) dst[t] = src[t * 64];
  };

  f32x4_t acc[TN][TM];
#pragma unroll
  for (int a = 0; a < TN; ++a)
#pragma unroll
    for (int t = 0; t < TM; ++t) acc[a][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // two weight registers sets, used in turn by the (tap, cout tile) steps of a chunk; a chunk's first step reads set 0
  bf16x8_t wq[2][TERMS];
  stage_load(0);
  load_w(wq[0], 0, 0, 0);
  stage_store();
  __syncthreads();

  for (int ch = 0; ch < nchunk; ++ch) {
    const bool more = ch + 1 < nchunk;
    if (more) stage_load((ch + 1) * KC);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int toff = ((tap / 3) * SW + tap % 3) * PITCH;
      bf16x8_t xf[TM][TERMS];
#pragma unroll
      for (int t = 0; t < TM; ++t)
#pragma unroll
        for (int s = 0; s < TERMS; ++s) xf[t][s] = *reinterpret_cast<const bf16x8_t*>(slab + xoff[t] + toff + s * 64);
#pragma unroll
      for (int a = 0; a < TN; ++a) {
        const int step = tap * TN + a, cur = step & 1;
        const int nxt = step + 1 == 9 * TN ? 0 : (step + 1) & 1;
        const bool late = nxt == cur;      // an odd step count (TN = 1): the chunk's last step reloads its own set, after its MFMAs
        auto prefetch = [&]() {
          if (a + 1 < TN) load_w(wq[nxt], a + 1, tap, ch);
          else if (tap < 8) load_w(wq[nxt], 0, tap + 1, ch);
          else if (more) load_w(wq[nxt], 0, 0, ch + 1);
        };
        if (!late) prefetch();
#pragma unroll
        for (int t = 0; t < TM; ++t) acc[a][t] = split_mfma<TERMS>(wq[cur], xf[t], acc[a][t]);
        if (late) prefetch();
      }
    }
    __syncthreads();          // every wave has read this chunk's slab
    if (more) {
      stage_store();
      __syncthreads();
    }
  }

  // epilogue: lane holds couts n .. n+3 of pixel m
  const bool vec_ok = (p.Cout & 3) == 0;
#pragma unroll
  for (int t = 0; t < TM; ++t) {
    const int m = (wm * TM + t) * 16 + fr;
    if (m >= RW) continue;
    const int r = m / p.W, c = m - r * p.W, oy = row0 + r;
    if (oy >= p.H) continue;
    const size_t pix = ((size_t)b * p.H + oy) * p.W + c;
#pragma unroll
    for (int a = 0; a < TN; ++a) {
      const int n = n0 + (wn * TN + a) * 16 + 4 * fq;
      if (n >= p.Cout) continue;
      const size_t e = pix * p.Cout + n;
      float o[4] = {acc[a][t][0], acc[a][t][1], acc[a][t][2], acc[a][t][3]};
      if (vec_ok) {
        if (p.bias) {
#pragma unroll
          for (int i = 0; i < 4; ++i) o[i] += p.bias[n + i];
        }
        if (p.res) {
          const float4 rv = *reinterpret_cast<const float4*>(p.res + e);
          o[0] += rv.x; o[1] += rv.y; o[2] += rv.z; o[3] += rv.w;
        }
        *reinterpret_cast<float4*>(p.y + e) = make_float4(o[0], o[1], o[2], o[3]);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (n + i < p.Cout) p.y[e + i] = o[i] + (p.bias ? p.bias[n + i] : 0.f) + (p.res ? p.res[e + i] : 0.f);
        }
      }
    }
  }
}

// fp32 shadow [rows][taps][Cin] -> fragment-major split shadow: thread = one 16-byte operand (lane l of a (row 16-tile, tap,
// chunk): row 16 * nt + l % 16, channels 32 * ck + 8 * (l / 16) .. +7), written once per term
template <int TERMS>
__global__ __launch_bounds__(256) void split_weight_kernel(const float* __restrict__ w, uint4* __restrict__ out, int rows, int taps,
                                                           int Cin, long n_frag) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_frag) return;
  const int l = (int)(i & 63);
  long f = i >> 6;
  const int nchunk = Cin / KC;
  const int ck = (int)(f % nchunk);
  f /= nchunk;
  const int tap = (int)(f % taps), nt = (int)(f / taps);
  const int row = nt * 16 + (l & 15);
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
  if (row < rows) {
    const float* src = w + ((size_t)row * taps + tap) * Cin + ck * KC + 8 * (l >> 4);
    a = *reinterpret_cast<const float4*>(src);
    b = *reinterpret_cast<const float4*>(src + 4);
  }
  uint4 tv[TERMS];
  split8<TERMS>(a, b, tv);
  uint4* dst = out + (i >> 6) * (TERMS * 64) + l;
#pragma unroll
  for (int t = 0; t < TERMS; ++t) dst[t * 64] = tv[t];
}

template <int TERMS, int TM, int WM, int WN, int BM, int BN>
int launch(const S3P& p, const Plan& pl, hipStream_t st) {
  auto kern = conv3x3_split_kernel<TERMS, TM, WM, WN, ns_of(BM, TERMS), BN>;
  const size_t lds = (size_t)pl.slab_px * pitch_of(TERMS);
  static IdfLdsGrant grant;
  if (hipError_t e = idf_ensure_lds((const void*)kern, lds, grant); e != hipSuccess)
    IDF_FAIL(IDF_ERR_HIP, "conv3x3_f32_split: LDS opt-in failed: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(kern, dim3((unsigned)(p.B * pl.tiles * pl.n_tiles)), dim3(256), lds, st, p);
  IDF_CHECK_LAUNCH();
  return IDF_OK;
}

template <int TERMS>
int launch_terms(const S3P& p, const Plan& pl, hipStream_t st) {
  if (pl.bn == 64) {
    if (pl.bm == 256) return launch<TERMS, 4, 4, 1, 256, 64>(p, pl, st);
    if (pl.bm == 128) return launch<TERMS, 2, 4, 1, 128, 64>(p, pl, st);
    return launch<TERMS, 2, 2, 2, 64, 64>(p, pl, st);
  }
  // Cout <= 16: one cout 16-tile, the waves split the pixels only
  if (pl.bm == 256) return launch<TERMS, 4, 4, 1, 256, 16>(p, pl, st);
  if (pl.bm == 128) return launch<TERMS, 2, 4, 1, 128, 16>(p, pl, st);
  return launch<TERMS, 1, 4, 1, 64, 16>(p, pl, st);
}

}  // namespace

extern "C" int idf_conv3x3_f32_split_ok(int B, int H, int W, int Cin, int Cout, int terms) {
  Plan pl;
  return plan_of(B, H, W, Cin, Cout, terms, &pl) ? 1 : 0;
}

extern "C" long idf_split_weight_bytes(int rows, int taps, int Cin, int terms) {
  if (rows < 1 || taps < 1 || Cin < 1 || terms < 1) return 0;
  return (long)((rows + 15) / 16 * 16) * taps * Cin * 2 * terms;
}

extern "C" int idf_split_weight_bf16(const float* w, void* wsplit, int rows, int taps, int Cin, int terms, void* stream) {
  if ((terms != 2 && terms != 3) || rows < 1 || taps < 1 || Cin < KC || (Cin % KC))
    IDF_FAIL(IDF_ERR_UNSUPPORTED, "split_weight_bf16: needs terms 2 or 3 and Cin %% 32 == 0 (rows=%d taps=%d Cin=%d terms=%d)",
             rows, taps, Cin, terms);
  if (!w || !wsplit) IDF_FAIL(IDF_ERR_BADARG, "split_weight_bf16: null w or wsplit");
  const long n_frag = (long)((rows + 15) / 16) * taps * (Cin / KC) * 64;
  if (n_frag >= (1L << 31)) IDF_FAIL(IDF_ERR_UNSUPPORTED, "split_weight_bf16: shadow too large");
  const dim3 g((unsigned)((n_frag + 255) / 256));
  hipStream_t st = (hipStream_t)stream;
  if (terms == 3) hipLaunchKernelGGL(split_weight_kernel<3>, g, dim3(256), 0, st, w, (uint4*)wsplit, rows, taps, Cin, n_frag);
  else hipLaunchKernelGGL(split_weight_kernel<2>, g, dim3(256), 0, st, w, (uint4*)wsplit, rows, taps, Cin, n_frag);
  IDF_CHECK_LAUNCH();
  return IDF_OK;
}

extern "C" int idf_conv3x3_f32_split(const float* x, const void* wsplit, const float* bias, const float* res, float* y,
                                     int B, int H, int W, int Cin, int Cout, int terms, void* stream) {
  Plan pl;
  if (!plan_of(B, H, W, Cin, Cout, terms, &pl))
    IDF_FAIL(IDF_ERR_UNSUPPORTED,
             "conv3x3_f32_split: needs Cin %% 32 == 0, 4 <= W <= 64, H >= 4, terms 2 or 3 (B=%d H=%d W=%d Cin=%d Cout=%d terms=%d)",
             B, H, W, Cin, Cout, terms);
  if (!x || !wsplit || !y) IDF_FAIL(IDF_ERR_BADARG, "conv3x3_f32_split: null x, wsplit or y");
  S3P p{x, (const uint4*)wsplit, bias, res, y, B, H, W, Cin, Cout, pl.R, pl.tiles, pl.n_tiles, (Cout + 15) / 16};
  hipStream_t st = (hipStream_t)stream;
  return terms == 3 ? launch_terms<3>(p, pl, st) : launch_terms<2>(p, pl, st);
}
