// fp32 3x3 stride-1 NHWC convolution (forward, and the data gradient with the flipped weight shadow) on the exact-fp32
// MFMA of gfx950 -- the halo-tile form of conv_igemm_kernel<float> (idf_conv.hip), which gathers every input pixel from
// global memory once per tap.
//
//   y[b,oy,ox,n] = bias[n] + res[b,oy,ox,n] + sum_{ky,kx,c} x[b,oy+ky-1,ox+kx-1,c] * w[n][ky*3+kx][c]
//
// Work split: a 256-thread workgroup owns R whole rows x W columns of one image (BM = 64 / 128 / 256 pixel slots, R =
// min(H, BM / W); the last row tile of an image masks rows) times a 64-wide cout tile (Cout <= 16, the 64 -> 3 tail conv:
// one 16-wide tile, the four waves split the pixels).  K runs over Cin in chunks of 16
// channels; per chunk the (R+2) x (W+2) halo slab is staged into LDS once (border pixels as zeros) and serves all 9
// taps, so the MFMA loop has no bounds checks and every input element is read from global memory once per (tile, cout
// tile).  Two slab buffers: the global loads of chunk k+1 are issued before the MFMAs of chunk k and land in the other
// buffer after them -- one barrier per chunk.
//
// Weights go straight from global memory (L2 / L1 resident: 9 * Cin * 64 floats per cout tile) into registers, one tap
// ahead of the MFMAs that use them: a lane's A operand for a (cout 16-tile, tap, chunk) is one float4, w[n0 + lane%16]
// [tap][c0 + 4 * (lane/16) ..+3].  Through LDS they would take 2 x 45 KB next to the slabs and leave one workgroup per
// CU; in registers they cost 2 x 4 float4 and LDS stays at <= 62 KB (two workgroups per CU, 2 waves per SIMD).
//
// MFMA: v_mfma_f32_16x16x4_f32, operand A = weights (rows = cout), operand B = pixels (cols = pixel): lane = (pixel or
// cout row l%16, quarter q = l/16).  One float4 per operand feeds 4 K-steps: at step j quarter q supplies channel
// c0 + 4q + j on both sides (the K order inside a chunk is free as long as A and B agree; it is fixed, so results are
// bit-identical run to run).  Each lane ends with 4 consecutive couts of one pixel.
//
// LDS layout: slab[pixel][20 floats] (16 channels + 4 pad).  A fragment read is one ds_read_b128 per lane at float
// offset 20 * pix + 4 * q.  The 16 lanes of a quarter read 16 consecutive slab pixels when 16 | W (32- and 64-wide
// maps: a 16-pixel group never wraps a row), i.e. bank quads 4 * (5 * i mod 16) for i = pix0 .. pix0+15: 5 is odd, so
// these are the 16 distinct quads of the 64 banks -- conflict-free.  (A 16-channel pitch would put pixels i and i+4 on
// the same quad: 4-way.)  Maps whose 16-pixel groups wrap a row (W = 28, 7, ...) skip 2 slab pixels at the wrap and can
// see a 2-way conflict on up to 2 lanes.
#include "idf_common.h"

namespace {

constexpr int KC = 16;       // channels per K chunk
constexpr int PITCH = 20;    // floats per staged pixel
constexpr int FULL_GRID = 512;   // two workgroups on each of the 256 CUs

struct C3P {
  const float* x;
  const float* w;
  const float* bias;
  const float* res;
  float* y;
  int B, H, W, Cin, Cout;
  int R, tiles, n_tiles;     // rows per tile, row tiles per image, cout tiles
};

struct Plan { int bm, bn, R, tiles, n_tiles, slab_px; };

// staged float4 per thread each kernel form has room for (NS * 256 >= 4 * slab pixels)
constexpr int ns_of(int bm) { return bm == 256 ? 7 : bm == 128 ? 5 : 4; }

// Tile shape for a covered problem; false: not covered.  The largest pixel tile that still gives the chip two workgroups per
// CU; below that the smallest whose tiles keep at least two rows (a one-row tile stages three rows per output row).
bool plan_of(int B, int H, int W, int Cin, int Cout, Plan* pl) {
  if (B < 1 || H < 4 || W < 4 || W > 64 || Cin < 32 || (Cin % 32) || Cout < 1) return false;
  const long lim = 1L << 31;
  if ((long)H * W * Cin >= lim || (long)H * W * Cout >= lim || (long)Cout * 9 * Cin >= lim) return false;
  Plan p;
  p.bn = Cout <= 16 ? 16 : 64;               // the 64 -> 3 tail conv: a quarter of the MFMA work of a 64-wide tile
  p.n_tiles = idf_cdiv(Cout, p.bn);
  const int bms[3] = {256, 128, 64};
  bool found = false;
  for (int i = 0; i < 3 && !found; ++i) {
    p.bm = bms[i];
    if ((long)H * W <= 64) p.bm = 64;           // images up to 8x8: one tile
    p.R = p.bm / W < H ? p.bm / W : H;
    p.tiles = idf_cdiv(H, p.R);
    const bool smaller_ok = p.bm > 64 && (bms[i + 1] / W >= 2);
    found = !smaller_ok || (long)B * p.tiles * p.n_tiles >= FULL_GRID;
  }
  if ((long)B * p.tiles * p.n_tiles >= lim) return false;
  p.slab_px = (p.R + 2) * (W + 2);
  if (p.slab_px * 4 > ns_of(p.bm) * 256 || 2 * p.slab_px * PITCH * 4 > 64 * 1024) return false;
  *pl = p;
  return true;
}

// TM pixel 16-tiles x TN cout 16-tiles per wave, waves WM (pixel) x WN (cout): BM = 16 * TM * WM pixel slots, BN couts.
template <int TM, int WM, int WN, int NS, int BN>
__global__ __launch_bounds__(256, 2) void conv3x3_f32_kernel(const C3P p) {
  constexpr int TN = BN / 16 / WN;
  static_assert(WM * WN == 4 && TN >= 1 && (BN == 16 || (TM >= 2 && TN >= 2)), "4 waves; at least 2x2 MFMA tiles each at the 64-wide cout tile");
  extern __shared__ __attribute__((aligned(16))) float slab[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int wm = wave % WM, wn = wave / WM;
  int bid = blockIdx.x;
  const int tn = bid % p.n_tiles;
  bid /= p.n_tiles;
  const int tr = bid % p.tiles, b = bid / p.tiles;
  const int row0 = tr * p.R, n0 = tn * BN;
  const int SW = p.W + 2, slab_px = (p.R + 2) * SW, RW = p.R * p.W;
  const int buf_floats = slab_px * PITCH;

  const float* __restrict__ X = p.x + (size_t)b * p.H * p.W * p.Cin;
  const float* __restrict__ Wt = p.w;

  // staging: item i = tid + 256 j is float4 (i & 3) of slab pixel i >> 2; goff < 0: padding, staged as zeros
  int goff[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    const int i = tid + 256 * j, px = i >> 2;
    const int sr = px / SW, sc = px - sr * SW;
    const int iy = row0 + sr - 1, ix = sc - 1;
    const bool ok = px < slab_px && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
    goff[j] = ok ? (iy * p.W + ix) * p.Cin + (i & 3) * 4 : -1;
  }
  float4 sv[NS];
  auto stage_load = [&](int c0) {
#pragma unroll
    for (int j = 0; j < NS; ++j)
      sv[j] = goff[j] >= 0 ? *reinterpret_cast<const float4*>(X + goff[j] + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  auto stage_store = [&](float* buf) {
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      const int i = tid + 256 * j;
      if (i < slab_px * 4) *reinterpret_cast<float4*>(buf + (i >> 2) * PITCH + (i & 3) * 4) = sv[j];
    }
  };

  // fragment addresses: slab offset of the lane's pixel at tap (0, 0) (slots past the tile read pixel 0 and are not stored)
  int xoff[TM];
#pragma unroll
  for (int t = 0; t < TM; ++t) {
    int m = (wm * TM + t) * 16 + fr;
    if (m >= RW) m = 0;
    const int r = m / p.W, c = m - r * p.W;
    xoff[t] = (r * SW + c) * PITCH + 4 * fq;
  }
  // ... and of its cout rows (rows past Cout read the last row and are not stored)
  int woff[TN];
#pragma unroll
  for (int a = 0; a < TN; ++a) {
    int n = n0 + (wn * TN + a) * 16 + fr;
    if (n >= p.Cout) n = p.Cout - 1;
    woff[a] = n * 9 * p.Cin + 4 * fq;
  }

  f32x4_t acc[TN][TM];
#pragma unroll
  for (int a = 0; a < TN; ++a)
#pragma unroll
    for (int t = 0; t < TM; ++t) acc[a][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int nchunk = p.Cin / KC;
  float4 wnx[TN];
  stage_load(0);
#pragma unroll
  for (int a = 0; a < TN; ++a) wnx[a] = *reinterpret_cast<const float4*>(Wt + woff[a]);
  stage_store(slab);
  __syncthreads();

  for (int ch = 0; ch < nchunk; ++ch) {
    const float* cur = slab + (ch & 1) * buf_floats;
    const bool more = ch + 1 < nchunk;
    if (more) stage_load((ch + 1) * KC);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      float4 wc[TN];
#pragma unroll
      for (int a = 0; a < TN; ++a) wc[a] = wnx[a];
      if (tap < 8 || more) {
        const int nxt = tap < 8 ? (tap + 1) * p.Cin + ch * KC : (ch + 1) * KC;
#pragma unroll
        for (int a = 0; a < TN; ++a) wnx[a] = *reinterpret_cast<const float4*>(Wt + woff[a] + nxt);
      }
      const int toff = ((tap / 3) * SW + tap % 3) * PITCH;
      float4 xf[TM];
#pragma unroll
      for (int t = 0; t < TM; ++t) xf[t] = *reinterpret_cast<const float4*>(cur + xoff[t] + toff);
#pragma unroll
      for (int a = 0; a < TN; ++a) {
        const float wa[4] = {wc[a].x, wc[a].y, wc[a].z, wc[a].w};
#pragma unroll
        for (int t = 0; t < TM; ++t) {
          const float xb[4] = {xf[t].x, xf[t].y, xf[t].z, xf[t].w};
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[a][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[j], xb[j], acc[a][t], 0, 0, 0);
        }
      }
    }
    // the other buffer was last read before the previous barrier
    if (more) stage_store(slab + ((ch + 1) & 1) * buf_floats);
    __syncthreads();
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

}  // namespace

extern "C" int idf_conv3x3_f32_ok(int B, int H, int W, int Cin, int Cout) {
  Plan pl;
  return plan_of(B, H, W, Cin, Cout, &pl) ? 1 : 0;
}

extern "C" int idf_conv3x3_f32(const float* x, const float* w, const float* bias, const float* res, float* y,
                               int B, int H, int W, int Cin, int Cout, void* stream) {
  Plan pl;
  if (!plan_of(B, H, W, Cin, Cout, &pl))
    IDF_FAIL(IDF_ERR_UNSUPPORTED, "conv3x3_f32: needs Cin %% 32 == 0, 4 <= W <= 64, H >= 4 (B=%d H=%d W=%d Cin=%d Cout=%d)",
             B, H, W, Cin, Cout);
  if (!x || !w || !y) IDF_FAIL(IDF_ERR_BADARG, "conv3x3_f32: null x, w or y");
  C3P p{x, w, bias, res, y, B, H, W, Cin, Cout, pl.R, pl.tiles, pl.n_tiles};
  hipStream_t st = (hipStream_t)stream;
  const dim3 g((unsigned)(B * pl.tiles * pl.n_tiles));
  const size_t lds = (size_t)2 * pl.slab_px * PITCH * sizeof(float);
  if (pl.bn == 64) {
    if (pl.bm == 256) hipLaunchKernelGGL((conv3x3_f32_kernel<4, 4, 1, ns_of(256), 64>), g, dim3(256), lds, st, p);
    else if (pl.bm == 128) hipLaunchKernelGGL((conv3x3_f32_kernel<2, 4, 1, ns_of(128), 64>), g, dim3(256), lds, st, p);
    else hipLaunchKernelGGL((conv3x3_f32_kernel<2, 2, 2, ns_of(64), 64>), g, dim3(256), lds, st, p);
  } else {      // Cout <= 16: one cout 16-tile, the waves split the pixels only
    if (pl.bm == 256) hipLaunchKernelGGL((conv3x3_f32_kernel<4, 4, 1, ns_of(256), 16>), g, dim3(256), lds, st, p);
    else if (pl.bm == 128) hipLaunchKernelGGL((conv3x3_f32_kernel<2, 4, 1, ns_of(128), 16>), g, dim3(256), lds, st, p);
    else hipLaunchKernelGGL((conv3x3_f32_kernel<1, 4, 1, ns_of(64), 16>), g, dim3(256), lds, st, p);
  }
  IDF_CHECK_LAUNCH();
  return IDF_OK;
}
