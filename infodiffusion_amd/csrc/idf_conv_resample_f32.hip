// fp32 DownSample (3x3, stride 2, pad 1) and UpSample (nearest x2 + 3x3) convs, forward and data gradient, on the exact-fp32
// MFMA of gfx950 in the halo-slab form of idf_conv3x3_f32.hip, with the algebra that does not multiply what is known:
//
//   S2 forward    y[oy][ox][n] = sum_{u,v<3,c} x[2oy-1+u][2ox-1+v][c] * w[n][3u+v][c]                  9 taps per output pixel
//   UP2 data grad dx[i][j][c]  = sum_{u,v<4,n} dy[2i-1+u][2j-1+v][n] * (sum_{ky in U[u], kx in U[v]} wd[c][3ky+kx][n])
//                 U = ({0}, {0,1}, {1,2}, {2}): the flipped 3x3 over dy followed by the 2x2 sum pool, as ONE 4x4 stride-2
//                 conv -- 16 taps per low-resolution pixel instead of 36, no intermediate, no pool launch
//   UP2 forward   y[2i+py][2j+px][n] = sum_{ty,tx<2,c} x[i+py+ty-1][j+px+tx-1][c] * (sum_{ky in S[py][ty], kx in S[px][tx]} w[n][3ky+kx][c])
//                 S = (({0}, {1,2}), ({0,1}, {2})): 4 taps per output pixel instead of 9
//   S2 data grad  dx[2i+py][2j+px][c]: per axis, parity 0 -> flipped tap 1 at dy offset 0; parity 1 -> flipped tap 0 at offset 0 and
//                 tap 2 at offset +1: 1 / 2 / 2 / 4 taps for the four parity classes (9 per four outputs instead of 36)
//
// Two kernels.  conv_s2k_f32_kernel<KU> (KU = 3: S2 forward, KU = 4: UP2 data gradient) tiles R output rows x Wo columns; the
// slab holds the 2R + KU - 2 input rows from row 2 * row0 - 1, each row de-interleaved WHILE STAGING into an odd-column plane
// (index j = column 2j - 1) followed by an even-column plane (index j = column 2j), Wo + 1 pixels each: tap v reads plane v & 1
// at index ox + (v >> 1), so consecutive output pixels are consecutive slab pixels.  conv_subpix_f32_kernel<FORM> (UP2 forward, S2
// data gradient) tiles R rows x W columns of BASE (low-resolution) pixels with a one-pixel halo, slab (R+2) x (W+2); a wave
// holds the accumulators of every parity class its workgroup owns (4, 2 or 1: the planner splits classes over workgroups where
// a launch would otherwise leave CUs idle), so the slab is staged once for all of them, and stores the classes interleaved.
//
// Everything else is idf_conv3x3_f32.hip's: 256 threads, K in 16-channel chunks, slab[pixel][20 floats] with out-of-image pixels
// as zeros (no bounds checks in the MFMA loop, a tap is a uniform offset), one ds_read_b128 per lane feeding 4 K-steps, two slab
// buffers and one barrier per chunk, weights from global memory into registers one tap ahead, bias / residual in the epilogue, a
// lane ends with 4 consecutive output channels of one pixel.  16 consecutive slab pixels at the 20-float pitch sit on the 16
// distinct bank quads (5 is odd); a 16-pixel group that wraps a tile row skips slab pixels and can see a 2-way conflict on up to 2 lanes.
//
// Weights are the two existing fp32 shadows ([rows][9][K]: forward [Cout][9][Cin], data gradient [Cin][9 flipped][Cout]).  A summed
// operand is 1, 2 or 4 float4 loads added in registers in a fixed order -- kernel rows first, then columns, as ops.upconv_pack.
#include "idf_common.h"
#include <utility>

namespace {

constexpr int KC = 16;       // channels per K chunk
constexpr int PITCH = 20;    // floats per staged pixel
constexpr int FULL_GRID = 512;   // two workgroups on each of the 256 CUs
constexpr int BN = 64, TN = 2;   // cout tile; 2 x 2 waves, TN cout 16-tiles each

enum { S2K3 = 0, S2K4 = 1, SUB_UP = 2, SUB_DN = 3 };                       // kernel forms
enum { OP_S2_FWD = 0, OP_S2_DGRAD = 1, OP_UP2_FWD = 2, OP_UP2_DGRAD = 3 };    // the C entry's `op`

struct RSP {
  const float* x;
  const float* w;
  const float* bias;
  const float* res;
  float* y;
  int B, Hi, Wi, K;          // staged map and its channels (the K side)
  int Ho, Wo, N;             // output map and its channels (the rows of w)
  int Hb, Wb;                // the map the tiles cover: output pixels (s2k), base pixels (subpix)
  int R, tiles, n_tiles;     // rows per tile, row tiles per image, cout tiles
};

// One MFMA tap: the slab pixel it reads relative to the lane's pixel (row dr, plane pl, column dc) and the 3x3 shadow taps
// ky0 .. ky0+nky-1 x kx0 .. kx0+nkx-1 whose sum is its weight.
struct Tap { int dr, pl, dc, ky0, nky, kx0, nkx; };

constexpr int cls_taps(int form, int cls) {
  return form == S2K3 ? 9 : form == S2K4 ? 16 : form == SUB_UP ? 4 : (1 + (cls >> 1)) * (1 + (cls & 1));
}
constexpr Tap tap_of(int form, int cls, int t) {
  const int py = cls >> 1, px = cls & 1;
  if (form == S2K3) return Tap{t / 3, (t % 3) & 1, (t % 3) >> 1, t / 3, 1, t % 3, 1};
  if (form == S2K4) {
    const int u = t >> 2, v = t & 3;
    return Tap{u, v & 1, v >> 1, u > 1 ? u - 1 : 0, (u == 0 || u == 3) ? 1 : 2, v > 1 ? v - 1 : 0, (v == 0 || v == 3) ? 1 : 2};
  }
  if (form == SUB_UP) {
    const int ty = t >> 1, tx = t & 1;
    return Tap{py + ty, 0, px + tx, py ? 2 * ty : ty, py != ty ? 2 : 1, px ? 2 * tx : tx, px != tx ? 2 : 1};
  }
  const int ty = t / (1 + px), tx = t % (1 + px);
  return Tap{py ? 1 + ty : 1, 0, px ? 1 + tx : 1, py ? 2 * ty : 1, 1, px ? 2 * tx : 1, 1};
}
// the (class, tap) pairs of classes cls0 .. cls0+ncls-1 as one sequence
constexpr int total_taps(int form, int cls0, int ncls) {
  int n = 0;
  for (int c = 0; c < ncls; ++c) n += cls_taps(form, cls0 + c);
  return n;
}
constexpr int flat_cls(int form, int cls0, int i) {
  int c = cls0;
  while (i >= cls_taps(form, c)) i -= cls_taps(form, c++);
  return c;
}
constexpr int flat_tap(int form, int cls0, int i) {
  int c = cls0;
  while (i >= cls_taps(form, c)) i -= cls_taps(form, c++);
  return i;
}

template <int... I, class F>
__device__ __forceinline__ void static_for_impl(std::integer_sequence<int, I...>, F&& f) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  static_for_impl(std::make_integer_sequence<int, N>{}, f);
}

__device__ __forceinline__ float4 f4add(const float4 a, const float4 b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

constexpr int ns_of(int form, int tm) { return form >= SUB_UP ? 3 : tm == 2 ? 7 : 5; }   // NS * 256 >= 4 * slab pixels

// The tile of one workgroup: classes CLS0 .. CLS0+NCLS-1 (s2k: the one class 0) of pixel slots 32 * TM x 64 couts from n0.
template <int FORM, int TM, int CLS0, int NCLS>
__device__ __forceinline__ void run_tile(const RSP& p, float* slab, int b, int row0, int n0) {
  constexpr bool S2K = FORM == S2K3 || FORM == S2K4;
  constexpr int KU = FORM == S2K4 ? 4 : 3;
  constexpr int NS = ns_of(FORM, TM);
  constexpr int NT = total_taps(FORM, CLS0, NCLS);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int wm = wave & 1, wn = wave >> 1;
  const int PW = p.Wb + 1;                                   // pixels per column plane (s2k)
  const int SW = S2K ? 2 * PW : p.Wb + 2;                    // slab pixels per staged row
  const int SR = S2K ? 2 * p.R + KU - 2 : p.R + 2;           // staged rows
  const int slab_px = SR * SW, RW = p.R * p.Wb;
  const int buf_floats = slab_px * PITCH;

  const float* __restrict__ X = p.x + (size_t)b * p.Hi * p.Wi * p.K;
  const float* __restrict__ Wt = p.w;

  // staging: item i = tid + 256 j is float4 (i & 3) of slab pixel i >> 2; goff < 0: padding, staged as zeros
  int goff[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    const int i = tid + 256 * j, px = i >> 2;
    const int sr = px / SW, sc = px - sr * SW;
    int iy, ix;
    if (S2K) {
      const int pl = sc >= PW ? 1 : 0, jj = sc - pl * PW;
      iy = 2 * row0 - 1 + sr;
      ix = 2 * jj - 1 + pl;
    } else {
      iy = row0 + sr - 1;
      ix = sc - 1;
    }
    const bool ok = px < slab_px && (unsigned)iy < (unsigned)p.Hi && (unsigned)ix < (unsigned)p.Wi;
    goff[j] = ok ? (iy * p.Wi + ix) * p.K + (i & 3) * 4 : -1;
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
    const int r = m / p.Wb, c = m - r * p.Wb;
    xoff[t] = ((S2K ? 2 * r : r) * SW + c) * PITCH + 4 * fq;
  }
  // ... and of its weight rows (rows past N read the last row and are not stored)
  int woff[TN];
#pragma unroll
  for (int a = 0; a < TN; ++a) {
    int n = n0 + (wn * TN + a) * 16 + fr;
    if (n >= p.N) n = p.N - 1;
    woff[a] = n * 9 * p.K + 4 * fq;
  }

  f32x4_t acc[NCLS][TN][TM];
#pragma unroll
  for (int c = 0; c < NCLS; ++c)
#pragma unroll
    for (int a = 0; a < TN; ++a)
#pragma unroll
      for (int t = 0; t < TM; ++t) acc[c][a][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // the raw shadow taps of the next MFMA tap: column kx of the sum outer, row ky inner
  float4 wnx[TN][4];
  auto wload = [&](auto I, int c0) {
    constexpr int i = decltype(I)::value;
    constexpr Tap tp = tap_of(FORM, flat_cls(FORM, CLS0, i), flat_tap(FORM, CLS0, i));
#pragma unroll
    for (int a = 0; a < TN; ++a)
#pragma unroll
      for (int kx = 0; kx < tp.nkx; ++kx)
#pragma unroll
        for (int ky = 0; ky < tp.nky; ++ky)
          wnx[a][kx * tp.nky + ky] =
              *reinterpret_cast<const float4*>(Wt + woff[a] + ((tp.ky0 + ky) * 3 + tp.kx0 + kx) * p.K + c0);
  };

  const int nchunk = p.K / KC;
  stage_load(0);
  wload(std::integral_constant<int, 0>{}, 0);
  stage_store(slab);
  __syncthreads();

  for (int ch = 0; ch < nchunk; ++ch) {
    const float* cur = slab + (ch & 1) * buf_floats;
    const bool more = ch + 1 < nchunk;
    if (more) stage_load((ch + 1) * KC);
    static_for<NT>([&](auto I) {
      constexpr int i = decltype(I)::value;
      constexpr int cls = flat_cls(FORM, CLS0, i);
      constexpr Tap tp = tap_of(FORM, cls, flat_tap(FORM, CLS0, i));
      constexpr int nw = tp.nky * tp.nkx;
      float4 wc[TN];
#pragma unroll
      for (int a = 0; a < TN; ++a) {
        if (nw == 1) wc[a] = wnx[a][0];
        else if (nw == 2) wc[a] = f4add(wnx[a][0], wnx[a][1]);
        else wc[a] = f4add(f4add(wnx[a][0], wnx[a][1]), f4add(wnx[a][2], wnx[a][3]));
      }
      if constexpr (i + 1 < NT) wload(std::integral_constant<int, i + 1>{}, ch * KC);
      else if (more) wload(std::integral_constant<int, 0>{}, (ch + 1) * KC);
      const int toff = (tp.dr * SW + tp.pl * PW + tp.dc) * PITCH;
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
          for (int j = 0; j < 4; ++j)
            acc[cls - CLS0][a][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[j], xb[j], acc[cls - CLS0][a][t], 0, 0, 0);
        }
      }
    });
    // the other buffer was last read before the previous barrier
    if (more) stage_store(slab + ((ch + 1) & 1) * buf_floats);
    __syncthreads();
  }

  // epilogue: lane holds rows n .. n+3 of pixel m of each class
  const bool vec_ok = (p.N & 3) == 0;
  static_for<NCLS>([&](auto C) {
    constexpr int ci = decltype(C)::value, cls = CLS0 + ci;
#pragma unroll
    for (int t = 0; t < TM; ++t) {
      const int m = (wm * TM + t) * 16 + fr;
      if (m >= RW) continue;
      const int r = m / p.Wb, c = m - r * p.Wb, i = row0 + r;
      if (i >= p.Hb) continue;
      const int oy = S2K ? i : 2 * i + (cls >> 1), ox = S2K ? c : 2 * c + (cls & 1);
      const size_t pix = ((size_t)b * p.Ho + oy) * p.Wo + ox;
#pragma unroll
      for (int a = 0; a < TN; ++a) {
        const int n = n0 + (wn * TN + a) * 16 + 4 * fq;
        if (n >= p.N) continue;
        const size_t e = pix * p.N + n;
        float o[4] = {acc[ci][a][t][0], acc[ci][a][t][1], acc[ci][a][t][2], acc[ci][a][t][3]};
        if (vec_ok) {
          if (p.bias) {
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] += p.bias[n + k];
          }
          if (p.res) {
            const float4 rv = *reinterpret_cast<const float4*>(p.res + e);
            o[0] += rv.x; o[1] += rv.y; o[2] += rv.z; o[3] += rv.w;
          }
          *reinterpret_cast<float4*>(p.y + e) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            if (n + k < p.N) p.y[e + k] = o[k] + (p.bias ? p.bias[n + k] : 0.f) + (p.res ? p.res[e + k] : 0.f);
          }
        }
      }
    }
  });
}

// KU x KU conv, stride 2, pad 1 (KU = 3: S2 forward; KU = 4: UP2 data gradient with the U-summed flipped taps); 32 * TM pixel slots
template <int KU, int TM>
__global__ __launch_bounds__(256, 2) void conv_s2k_f32_kernel(const RSP p) {
  extern __shared__ __attribute__((aligned(16))) float slab[];
  int bid = blockIdx.x;
  const int tn = bid % p.n_tiles;
  bid /= p.n_tiles;
  const int tr = bid % p.tiles, b = bid / p.tiles;
  run_tile<KU == 3 ? S2K3 : S2K4, TM, 0, 1>(p, slab, b, tr * p.R, tn * BN);
}

// Four parity-class convs over a tile of 64 base pixels; a workgroup owns NCLS of the classes (class group cg of 4 / NCLS)
template <int FORM, int NCLS>
__global__ __launch_bounds__(256, 2) void conv_subpix_f32_kernel(const RSP p) {
  extern __shared__ __attribute__((aligned(16))) float slab[];
  int bid = blockIdx.x;
  const int tn = bid % p.n_tiles;
  bid /= p.n_tiles;
  const int cg = bid % (4 / NCLS);
  bid /= 4 / NCLS;
  const int tr = bid % p.tiles, b = bid / p.tiles;
  const int row0 = tr * p.R, n0 = tn * BN;
  if constexpr (NCLS == 4) {
    run_tile<FORM, 2, 0, 4>(p, slab, b, row0, n0);
  } else if constexpr (NCLS == 2) {
    if (cg == 0) run_tile<FORM, 2, 0, 2>(p, slab, b, row0, n0);
    else run_tile<FORM, 2, 2, 2>(p, slab, b, row0, n0);
  } else {
    if (cg == 0) run_tile<FORM, 2, 0, 1>(p, slab, b, row0, n0);
    else if (cg == 1) run_tile<FORM, 2, 1, 1>(p, slab, b, row0, n0);
    else if (cg == 2) run_tile<FORM, 2, 2, 1>(p, slab, b, row0, n0);
    else run_tile<FORM, 2, 3, 1>(p, slab, b, row0, n0);
  }
}

struct Plan { int form, tm, ncls, slab_px; long grid; RSP g; };

// Geometry, tile shape and class split for a covered problem (Hs, Ws, Cin, Cout: the FORWARD conv's input map and channels);
// false: not covered.
bool plan_of(int B, int Hs, int Ws, int Cin, int Cout, int op, Plan* pl) {
  if (B < 1 || Hs < 1 || Ws < 1 || Cin < 1 || Cout < 1 || op < OP_S2_FWD || op > OP_UP2_DGRAD) return false;
  if (Hs > 4096 || Ws > 4096) return false;
  Plan P{};
  RSP& g = P.g;
  g.B = B;
  if (op == OP_S2_FWD) {
    P.form = S2K3;
    g.Hi = Hs; g.Wi = Ws; g.K = Cin; g.N = Cout;
    g.Hb = g.Ho = (Hs + 1) / 2; g.Wb = g.Wo = (Ws + 1) / 2;
  } else if (op == OP_UP2_DGRAD) {
    P.form = S2K4;
    g.Hi = 2 * Hs; g.Wi = 2 * Ws; g.K = Cout; g.N = Cin;
    g.Hb = g.Ho = Hs; g.Wb = g.Wo = Ws;
  } else if (op == OP_UP2_FWD) {
    P.form = SUB_UP;
    g.Hi = g.Hb = Hs; g.Wi = g.Wb = Ws; g.K = Cin; g.N = Cout;
    g.Ho = 2 * Hs; g.Wo = 2 * Ws;
  } else {
    if ((Hs | Ws) & 1) return false;            // odd maps keep the zero-stuffed route
    P.form = SUB_DN;
    g.Hi = g.Hb = Hs / 2; g.Wi = g.Wb = Ws / 2; g.K = Cout; g.N = Cin;
    g.Ho = Hs; g.Wo = Ws;
  }
  if (g.K < 32 || (g.K % 32) || g.Wb < 4 || g.Wb > 32 || g.Hb < 2) return false;
  const long lim = 1L << 31;
  if ((long)g.Hi * g.Wi * g.K >= lim || (long)g.Ho * g.Wo * g.N >= lim || (long)g.N * 9 * g.K >= lim) return false;
  g.n_tiles = idf_cdiv(g.N, BN);
  const bool s2k = P.form <= S2K4;
  // UP2 data gradient: 64-pixel tiles where they still give the chip two workgroups per CU, else 32 (S2 forward: always 32, it
  // serves under-filled launches only); subpix: 64 base pixels, and the four classes spread over 2 or 4 workgroups while the
  // launch is short of that
  P.tm = op == OP_S2_FWD ? 1 : 2;
  P.ncls = s2k ? 1 : 4;
  for (;;) {
    const int bm = 32 * P.tm;
    g.R = bm / g.Wb < g.Hb ? bm / g.Wb : g.Hb;
    g.tiles = idf_cdiv(g.Hb, g.R);
    P.grid = (long)B * g.tiles * g.n_tiles * (s2k ? 1 : 4 / P.ncls);
    if (P.grid >= FULL_GRID) break;
    if (s2k && P.tm == 2) P.tm = 1;
    else if (!s2k && P.ncls > 1) P.ncls /= 2;
    else break;
  }
  if (P.grid >= lim) return false;
  // measured out (profiles/f32_resample.txt): the S2 forward keeps its 9 taps, and where its launch fills the chip the generic
  // gather kernel is as fast or faster; the UP2 data gradient of a one-tile image (8 x 8) at the training batch is one chain of
  // 16 summed-weight taps per chunk on half the CUs and loses to the stride-1 kernel over dy + pool
  if (op == OP_S2_FWD && P.grid >= FULL_GRID) return false;
  if (op == OP_UP2_DGRAD && g.Hb * g.Wb <= 64 && B >= 32) return false;
  const int ku = P.form == S2K4 ? 4 : 3;
  P.slab_px = s2k ? (2 * g.R + ku - 2) * 2 * (g.Wb + 1) : (g.R + 2) * (g.Wb + 2);
  if (P.slab_px * 4 > ns_of(P.form, P.tm) * 256 || 2 * P.slab_px * PITCH * 4 > 64 * 1024) return false;
  *pl = P;
  return true;
}

}  // namespace

extern "C" int idf_conv_resample_f32_ok(int B, int Hs, int Ws, int Cin, int Cout, int op) {
  Plan pl;
  return plan_of(B, Hs, Ws, Cin, Cout, op, &pl) ? 1 : 0;
}

extern "C" int idf_conv_resample_f32(const float* x, const float* w, const float* bias, const float* res, float* y,
                                     int B, int Hs, int Ws, int Cin, int Cout, int op, void* stream) {
  Plan pl;
  if (!plan_of(B, Hs, Ws, Cin, Cout, op, &pl))
    IDF_FAIL(IDF_ERR_UNSUPPORTED,
             "conv_resample_f32: needs K-side channels %% 32 == 0, tile map width 4 .. 32 and height >= 2, even Hs / Ws for the S2 "
             "data gradient (B=%d Hs=%d Ws=%d Cin=%d Cout=%d op=%d)", B, Hs, Ws, Cin, Cout, op);
  if (!x || !w || !y) IDF_FAIL(IDF_ERR_BADARG, "conv_resample_f32: null x, w or y");
  RSP p = pl.g;
  p.x = x; p.w = w; p.bias = bias; p.res = res; p.y = y;
  hipStream_t st = (hipStream_t)stream;
  const dim3 g((unsigned)pl.grid), blk(256);
  const size_t lds = (size_t)2 * pl.slab_px * PITCH * sizeof(float);
  if (pl.form == S2K3) {
    hipLaunchKernelGGL((conv_s2k_f32_kernel<3, 1>), g, blk, lds, st, p);
  } else if (pl.form == S2K4) {
    if (pl.tm == 2) hipLaunchKernelGGL((conv_s2k_f32_kernel<4, 2>), g, blk, lds, st, p);
    else hipLaunchKernelGGL((conv_s2k_f32_kernel<4, 1>), g, blk, lds, st, p);
  } else if (pl.form == SUB_UP) {
    if (pl.ncls == 4) hipLaunchKernelGGL((conv_subpix_f32_kernel<SUB_UP, 4>), g, blk, lds, st, p);
    else if (pl.ncls == 2) hipLaunchKernelGGL((conv_subpix_f32_kernel<SUB_UP, 2>), g, blk, lds, st, p);
    else hipLaunchKernelGGL((conv_subpix_f32_kernel<SUB_UP, 1>), g, blk, lds, st, p);
  } else {
    if (pl.ncls == 4) hipLaunchKernelGGL((conv_subpix_f32_kernel<SUB_DN, 4>), g, blk, lds, st, p);
    else if (pl.ncls == 2) hipLaunchKernelGGL((conv_subpix_f32_kernel<SUB_DN, 2>), g, blk, lds, st, p);
    else hipLaunchKernelGGL((conv_subpix_f32_kernel<SUB_DN, 1>), g, blk, lds, st, p);
  }
  IDF_CHECK_LAUNCH();
  return IDF_OK;
}
