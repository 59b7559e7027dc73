// fp32 stride-1 NHWC convolution weight gradient (3x3 and 1x1) with the bias gradient fused in, on the exact-fp32 MFMA of
// gfx950: no atomics, no zero-fill, a fixed summation order -- the deterministic form of conv_wgrad_kernel<float, 3>
// (idf_conv.hip), which gathers the input from global memory once per tap and adds its partials with fp32 atomics.
//
//   dW[n][tap][c] = sum_{b,oy,ox} dy[b,oy,ox,n] * a[b,oy+ky-1,ox+kx-1,c]      (tap = ky*3+kx; 1x1: a[b,oy,ox,c])
//   db[n]         = sum_{b,oy,ox} dy[b,oy,ox,n]
//
// Work split: a 256-thread workgroup owns one (64-cin tile, 64-cout tile, kernel row ky) and a contiguous range of pixel
// tiles (one of S pixel splits).  A pixel tile is R whole rows x W columns of one image (R * W <= 64 slots; the last tile
// of an image masks rows).  Each of the 4 waves holds 32 couts x 32 cins x the row's 3 taps: 2 x 2 x 3 accumulator tiles
// of 16 x 16 = 48 registers; per 4-pixel K-step it issues 2 + 6 ds_read_b32 for 12 MFMAs (1x1: 2 + 2 for 4).  The three
// kernel rows are three workgroups that each stage their own input rows: the fp32 MFMA runs at 1/16 of the bf16 rate,
// so the kernel is bound by the MFMA pipe and small accumulators / many resident waves are worth more than input reuse.
//
// MFMA: v_mfma_f32_16x16x4_f32, operand A = dy (rows = cout), operand B = a (cols = cin), K = 4 consecutive pixel slots.
// Lane (r = lane % 16, q = lane / 16) supplies dy[slot 4s+q][n0+r] and a[slot 4s+q shifted by the tap][c0+r]: one
// ds_read_b32 each from tiles kept in their natural [pixel][channel] layout -- K is the pixel index and the instruction
// takes one scalar per lane, so there is no transpose and no scalar scatter.  A lane ends with 4 consecutive couts
// (4q .. 4q+3) of one cin (r): the 16 lanes of a quarter store 64 contiguous bytes of dW[n][tap][c0 .. c0+15].
//
// LDS: dyt[64 slots][80 floats] and at[<= 80 staged pixels][80 floats] (64 channels + 16 pad), 46080 bytes, written with
// ds_write_b128 from float4 global loads (thread = float4 tid % 16 of pixel tid / 16 + 16 j: the 16 lanes of a pixel write 64
// consecutive floats, the next pixel starts 80 floats on -- every 16-lane group covers the 64 banks once).  The input
// tile is R x (W + 2) pixels of the rows shifted by ky - 1 with out-of-image pixels (and channels past Cin / Cout) stored
// as zeros, so the MFMA loop has no bounds checks and tap kx is the uniform offset kx * 80.  Bank arithmetic of a
// fragment read: lane (r, q) reads float 80 * (p0 + q) + ch0 + r, i.e. bank (16 * (p0 + q) + ch0 + r) mod 64 with ch0 a
// multiple of 16: when the four slots of a K-step sit in one staged row (W % 4 == 0, p0 + q consecutive) the quarters
// land on banks 0 / 16 / 32 / 48 + r (rotated) -- all 64 distinct, conflict-free.  (A 64-float pitch would put all four
// quarters on the same 16 banks: 4-way.)  Maps where a K-step wraps a row (W = 7, 14, ...; not 28) skip the two halo
// pixels at the wrap, so the staged pixels of the four quarters are e.g. p, p+1, p+4, p+5: equal in pairs mod 4, a
// 2-way conflict on that one step of the 3x3 (the 1x1 stages no halo and never conflicts).  Each lane carries its own
// staged-pixel offset, advanced by 4 (+2 at a row wrap) per step.  Slots past R * W in the last K-step hold dy = 0 and
// read staged pixel 0; masked rows of an image's last tile hold dy = 0 against whatever in-image row the tap reaches.
// Both rely on 0 * a = 0: a non-finite activation (an input that is already broken) turns into NaN in every cout of its
// channel, where the exact formula would touch only the taps that reach it.
//
// Pipeline: one LDS buffer, the next tile in registers -- the 4 + 5 float4 global loads of tile t+1 are issued before
// the MFMAs of tile t and stored after them (two barriers per tile).  46 KB of LDS and 156 VGPRs (3x3; 116 at 1x1)
// leave three workgroups per CU.
//
// Accumulation: the planner picks S pixel splits so that c_tiles * n_tiles * rows * S reaches two workgroups per CU
// without cutting a split below MIN_TILES tiles (a split's partial store is 4 tiles' worth of loads).  S == 1: the
// workgroups store straight into dW / db.  S > 1: split s stores its partial dW | db into slab s of the workspace (plain
// stores, one writer per element) and wgrad_f32_reduce_kernel adds the slabs in slab order.  Splits may begin and end
// inside an image.  The bias gradient rides on the workgroups of cin tile 0 on the middle kernel row (the only row at
// 1x1): each thread sums the dy float4 it stages anyway (same 4 channels every time), the 16 per-pixel-group partials
// of a channel are combined through LDS in index order.
//
// The gather-mode variant (wgrad_f32_gather_kernel, idf_conv_wgrad_f32_gather: stride 2, x2 up-sampling, channel counts
// that are not multiples of 4) shares all of the above; its staging layouts and bank arithmetic are described above it.
#include "idf_common.h"
#include "idf_wgrad_f32_parts.h"

namespace {

constexpr int PITCH = 80;        // floats per staged pixel: 64 channels + 16 pad
constexpr int TILE_PX = 64;      // dy pixel slots per tile
constexpr int A_PX = 80;         // staged input pixels per tile at most
constexpr int NDY = TILE_PX / 16, NA = A_PX / 16;   // float4 per thread and tile
constexpr int FULL_GRID = 512;   // two workgroups on each of the 256 CUs
constexpr int MAX_CH = 65536;    // channel counts the plan admits
constexpr int MIN_TILES = 6;     // a split is at least this many pixel tiles (unless the problem has fewer)

struct WgPlan { int R, T, c_tiles, n_tiles, rows, S, per; long NT, nW, slab; };

struct WgP {
  const float* a;
  const float* dy;
  float* dW;
  float* db;
  float* ws;
  int H, W, Cin, Cout;
  int R, T, c_tiles, n_tiles, S, per;
  long NT, nW, slab;
};

bool plan_of(int B, int H, int W, int Cin, int Cout, int taps, WgPlan* pl) {
  if (taps != 9 && taps != 1) return false;
  if (B < 1 || H < 4 || W < 4 || W > 64 || Cin < 4 || (Cin % 4) || Cout < 4 || (Cout % 4)) return false;
  if (Cin > MAX_CH || Cout > MAX_CH) return false;      // the staging offsets (<= 80 pixels x channels) are ints
  const long lim = 1L << 31;
  if ((long)B * H * W * Cin >= lim || (long)B * H * W * Cout >= lim || (long)Cout * taps * Cin + Cout >= lim) return false;
  WgPlan p;
  const int halo = taps == 9 ? 1 : 0;
  p.R = TILE_PX / W < H ? TILE_PX / W : H;
  while (p.R * (W + 2 * halo) > A_PX) --p.R;
  p.T = idf_cdiv(H, p.R);
  p.NT = (long)B * p.T;
  p.c_tiles = idf_cdiv(Cin, 64);
  p.n_tiles = idf_cdiv(Cout, 64);
  p.rows = taps == 9 ? 3 : 1;
  const long base = (long)p.c_tiles * p.n_tiles * p.rows;
  long S = (FULL_GRID + base - 1) / base;
  if (S > p.NT / MIN_TILES) S = p.NT / MIN_TILES;
  if (S < 1) S = 1;
  p.per = (int)((p.NT + S - 1) / S);
  p.S = (int)((p.NT + p.per - 1) / p.per);      // no empty split
  p.nW = (long)Cout * taps * Cin;
  p.slab = p.nW + Cout;                         // Cin % 4 == 0 and Cout % 4 == 0: a multiple of 4 floats as it stands
  if (base * p.S >= lim) return false;
  *pl = p;
  return true;
}

// NKX = 3: one kernel row of the 3x3 (halo 1); NKX = 1: the 1x1
template <int NKX>
__global__ __launch_bounds__(256, 2) void wgrad_f32_kernel(const WgP p) {
  constexpr int HALO = NKX == 3 ? 1 : 0;
  __shared__ __attribute__((aligned(16))) float dyt[TILE_PX * PITCH];
  __shared__ __attribute__((aligned(16))) float at[A_PX * PITCH];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int wn = wave & 1, wc = wave >> 1;
  int bid = blockIdx.x;
  const int ky = bid % NKX;
  bid /= NKX;
  const int ct = bid % p.c_tiles;
  bid /= p.c_tiles;
  const int nt = bid % p.n_tiles, s = bid / p.n_tiles;
  const int c0 = ct * 64, n0 = nt * 64;
  const int W = p.W, H = p.H, Cin = p.Cin, Cout = p.Cout, R = p.R, T = p.T;
  const int SW = W + 2 * HALO, npx = R * W, apx = R * SW, ksteps = (npx + 3) >> 2;
  const long t0 = (long)s * p.per, t1 = t0 + p.per < p.NT ? t0 + p.per : p.NT;

  const float* __restrict__ A = p.a;
  const float* __restrict__ DY = p.dy;

  // staging: item j of a thread is float4 sf of staged pixel sp + 16 j; rel < 0: never loaded (staged as zeros),
  // row: the tile row whose image row decides at run time
  const int sf = tid & 15, sp = tid >> 4;
  int dy_rel[NDY], dy_row[NDY], a_rel[NA], a_row[NA];
#pragma unroll
  for (int j = 0; j < NDY; ++j) {
    const int px = sp + 16 * j;
    dy_row[j] = px / W;
    dy_rel[j] = (px < npx && n0 + 4 * sf < Cout) ? px * Cout + n0 + 4 * sf : -1;
  }
#pragma unroll
  for (int j = 0; j < NA; ++j) {
    const int px = sp + 16 * j;
    const int sr = px / SW, ix = px - sr * SW - HALO;
    a_row[j] = sr;
    a_rel[j] = (px < apx && (unsigned)ix < (unsigned)W && c0 + 4 * sf < Cin) ? (sr * W + ix) * Cin + c0 + 4 * sf : -1;
  }
  f32x4_t dyv[NDY], av[NA];
  const f32x4_t zero4 = {0.f, 0.f, 0.f, 0.f};
  auto stage_load = [&](long t) {
    const long b = t / T;
    const int row0 = (int)(t - b * T) * R;
    const long dy_base = ((b * H + row0) * W) * (long)Cout;
    const long a_base = ((b * H + row0 + ky - HALO) * W) * (long)Cin;      // may point above the image: masked per item
#pragma unroll
    for (int j = 0; j < NDY; ++j) {
      const bool ok = dy_rel[j] >= 0 && row0 + dy_row[j] < H;
      dyv[j] = ok ? *reinterpret_cast<const f32x4_t*>(DY + (dy_base + dy_rel[j])) : zero4;
    }
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      const bool ok = a_rel[j] >= 0 && (unsigned)(row0 + a_row[j] + ky - HALO) < (unsigned)H;
      av[j] = ok ? *reinterpret_cast<const f32x4_t*>(A + (a_base + a_rel[j])) : zero4;
    }
  };

  const bool bias_wg = p.db != nullptr && ct == 0 && ky == HALO;
  f32x4_t bsum = zero4;
  auto stage_store = [&]() {
#pragma unroll
    for (int j = 0; j < NDY; ++j) {
      *reinterpret_cast<f32x4_t*>(dyt + (sp + 16 * j) * PITCH + 4 * sf) = dyv[j];
      if (bias_wg) bsum += dyv[j];      // uniform per workgroup
    }
#pragma unroll
    for (int j = 0; j < NA; ++j) *reinterpret_cast<f32x4_t*>(at + (sp + 16 * j) * PITCH + 4 * sf) = av[j];
  };

  f32x4_t acc[2][2][NKX];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int kx = 0; kx < NKX; ++kx) acc[i][j][kx] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int dy_lane = fq * PITCH + wn * 32 + fr;      // + 4 * PITCH per K-step; + 16 for the second cout 16-tile
  const int a_lane0 = wc * 32 + fr;                   // staged pixel 0

  stage_load(t0);
  for (long t = t0; t < t1; ++t) {
    stage_store();
    __syncthreads();
    if (t + 1 < t1) stage_load(t + 1);

    int cc = fq, aoff = a_lane0 + fq * PITCH;         // the lane's slot: column in its row, staged offset at kx = 0
    for (int ks = 0; ks < ksteps; ++ks) {
      const float* dp = dyt + dy_lane + ks * 4 * PITCH;
      const float d0 = dp[0], d1 = dp[16];
      const float* ap = at + (4 * ks + fq < npx ? aoff : a_lane0);
#pragma unroll
      for (int kx = 0; kx < NKX; ++kx) {
        const float x0 = ap[kx * PITCH], x1 = ap[kx * PITCH + 16];
        acc[0][0][kx] = __builtin_amdgcn_mfma_f32_16x16x4f32(d0, x0, acc[0][0][kx], 0, 0, 0);
        acc[0][1][kx] = __builtin_amdgcn_mfma_f32_16x16x4f32(d0, x1, acc[0][1][kx], 0, 0, 0);
        acc[1][0][kx] = __builtin_amdgcn_mfma_f32_16x16x4f32(d1, x0, acc[1][0][kx], 0, 0, 0);
        acc[1][1][kx] = __builtin_amdgcn_mfma_f32_16x16x4f32(d1, x1, acc[1][1][kx], 0, 0, 0);
      }
      cc += 4;
      aoff += 4 * PITCH;
      if (cc >= W) {          // W >= 4: at most one row wrap per step; skip the two halo pixels between rows
        cc -= W;
        aoff += 2 * HALO * PITCH;
      }
    }
    __syncthreads();          // every fragment read of this tile before the next tile's stores
  }

  float* __restrict__ ow = p.S > 1 ? p.ws + (size_t)s * p.slab : p.dW;
  float* __restrict__ ob = p.S > 1 ? ow + p.nW : p.db;

  // lane holds couts n .. n+3 of cin c
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n0 + wn * 32 + i * 16 + 4 * fq, c = c0 + wc * 32 + j * 16 + fr;
      if (c >= Cin) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (n + e >= Cout) continue;
#pragma unroll
        for (int kx = 0; kx < NKX; ++kx)
          ow[((size_t)(n + e) * (NKX * NKX) + ky * NKX + kx) * Cin + c] = acc[i][j][kx][e];
      }
    }

  if (bias_wg) {              // uniform per workgroup; dyt is free since the loop's last barrier
    *reinterpret_cast<f32x4_t*>(dyt + sp * 64 + 4 * sf) = bsum;
    __syncthreads();
    if (tid < 64 && n0 + tid < Cout) {
      float v = 0.f;
#pragma unroll
      for (int g = 0; g < 16; ++g) v += dyt[g * 64 + tid];
      ob[n0 + tid] = v;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Gather-mode variant (idf_conv_wgrad_f32_gather): the same work split, MFMA loop, slab scheme and bias sum for the
// weight gradients the stride-1 plan refuses -- the stride-2 3x3 (S2), the 3x3 over the nearest-neighbour x2 up-sampled
// input (UP2), and any conv whose channel counts are not multiples of 4 (the 3-channel head and tail).
//
//   S2   dW[n][ky][kx][c] = sum dy[b,oy,ox,n] * a[b,2oy+ky-1,2ox+kx-1,c]            Ho = (Hs+1)/2, Wo = (Ws+1)/2 <= 32
//   UP2  dW[n][ky][kx][c] = sum dy[b,oy,ox,n] * a[b,(oy+ky-1)>>1,(ox+kx-1)>>1,c]    Ho = 2 Hs, Wo = 2 Ws <= 64
//
// A pixel tile is still R whole OUTPUT rows (R * Wo <= 64 dy slots), K = 4 consecutive output-pixel slots, and both
// operands are one ds_read_b32 each at the 80-float pitch; only the staged input tile and the lane's offset into it
// differ by mode.  Out-of-image pixels are staged as zeros in every mode (odd Hs / Ws at S2: the right / bottom taps).
//
// S2 staging: kernel row ky needs the R input rows 2oy+ky-1, columns ix = -1 .. 2Wo-1.  Staged as they lie in memory the
// four quarters of a K-step would read staged pixels p, p+2, p+4, p+6 = 160 floats apart = banks 0 / 32 / 0 / 32 + r:
// 2-way on every read.  So each staged row is de-interleaved while staging into an odd-column plane (Wo + 1 pixels,
// plane index j = column 2j-1) followed by an even-column plane (Wo pixels, j = column 2j): 2Wo + 1 pixels a row, at
// most 144 a tile.  Tap kx = 0 reads odd[ox], kx = 1 even[ox], kx = 2 odd[ox+1]: consecutive output pixels are
// consecutive staged pixels, so the bank argument above holds unchanged, and kx is again a uniform offset
// (0, Wo + 1, 1 pixels).  LDS (64 + 144) x 320 B = 66560 B: two workgroups per CU.
//
// UP2 staging: the LOW-RESOLUTION tile only, the <= R/2 + 1 source rows that kernel row ky reaches x (Ws + 2) columns
// (source columns -1 .. Ws), at most 48 pixels -- half the global traffic and LDS of a materialised up-sampled tile
// (LDS (64 + 48) x 320 B = 35840 B).  Each lane computes its own staged pixel per tap: row ((r + par) >> 1) with
// par = the parity of the tile's first up-sampled row, column (ox + kx + 1) >> 1.  Two neighbouring output pixels that
// share a source pixel read the same address (a broadcast); distinct source pixels of a K-step are consecutive staged
// pixels = 16 banks apart: conflict-free.
//
// Channel counts: VA / VD pick float4 staging (Cin % 4 == 0 / Cout % 4 == 0) or scalar global loads with zero fill for
// the input / dy tile at compile time.  A wave whose 16-channel sub-tile lies wholly past Cin or Cout skips that
// sub-tile's MFMAs (a wave-uniform test): Cin = 3 issues 1/8 of the MFMAs of a full tile, not all of them.
constexpr int A_PX_S2 = 144, A_PX_UP2 = 48;
enum { G_S1 = 0, G_S2 = 1, G_UP2 = 2 };

struct WgGPlan { int R, T, c_tiles, n_tiles, rows, S, per; long NT, nW, nWp, slab; bool s1; };

struct WgGP {
  const float* a;
  const float* dy;
  float* dW;
  float* db;
  float* ws;
  int Hs, Ws, Ho, Wo, Cin, Cout;
  int R, T, c_tiles, n_tiles, S, per;
  long NT, nW, nWp, slab;
};

constexpr int a_px_of(int mode) { return mode == G_S2 ? A_PX_S2 : mode == G_UP2 ? A_PX_UP2 : A_PX; }

// staged input rows and pixels a row of a tile of R output rows
inline int g_arows(int mode, int R) { return mode == G_UP2 ? (R >> 1) + 1 : R; }
inline int g_sw(int mode, int halo, int Ws, int Wo) { return mode == G_S2 ? 2 * Wo + 1 : mode == G_UP2 ? Ws + 2 : Wo + 2 * halo; }

bool gather_plan_of(int B, int Hs, int Ws, int Cin, int Ho, int Wo, int Cout, int mode, int taps, WgGPlan* pl) {
  if (taps != 9 && taps != 1) return false;
  if (mode != G_S1 && mode != G_S2 && mode != G_UP2) return false;
  if (taps == 1 && mode != G_S1) return false;
  if (B < 1 || Hs < 1 || Ws < 1 || Cin < 1 || Cout < 1 || Cin > MAX_CH || Cout > MAX_CH) return false;
  if (Hs > (1 << 20) || Ws > (1 << 20)) return false;
  const int eh = mode == G_S2 ? (Hs + 1) / 2 : mode == G_UP2 ? 2 * Hs : Hs;
  const int ew = mode == G_S2 ? (Ws + 1) / 2 : mode == G_UP2 ? 2 * Ws : Ws;
  if (Ho != eh || Wo != ew) return false;
  if (Ho < 4 || Wo < 4 || Wo > (mode == G_S2 ? 32 : 64)) return false;
  const long lim = 1L << 31;
  if ((long)B * Hs * Ws * Cin >= lim || (long)B * Ho * Wo * Cout >= lim || (long)Cout * taps * Cin + Cout + 8 >= lim) return false;
  WgGPlan p{};
  WgPlan s1;
  p.s1 = mode == G_S1 && plan_of(B, Ho, Wo, Cin, Cout, taps, &s1);
  if (p.s1) {      // the stride-1 kernel's own shapes stay its own
    p.S = s1.S;
    p.slab = s1.slab;
    *pl = p;
    return true;
  }
  const int halo = taps == 9 ? 1 : 0;
  p.R = TILE_PX / Wo < Ho ? TILE_PX / Wo : Ho;
  while (g_arows(mode, p.R) * g_sw(mode, halo, Ws, Wo) > a_px_of(mode)) --p.R;      // R = 1 always fits
  p.T = idf_cdiv(Ho, p.R);
  p.NT = (long)B * p.T;
  p.c_tiles = idf_cdiv(Cin, 64);
  p.n_tiles = idf_cdiv(Cout, 64);
  p.rows = taps == 9 ? 3 : 1;
  const long base = (long)p.c_tiles * p.n_tiles * p.rows;
  long S = (FULL_GRID + base - 1) / base;
  if (S > p.NT / MIN_TILES) S = p.NT / MIN_TILES;
  if (S < 1) S = 1;
  p.per = (int)((p.NT + S - 1) / S);
  p.S = (int)((p.NT + p.per - 1) / p.per);      // no empty split
  p.nW = (long)Cout * taps * Cin;
  p.nWp = (p.nW + 3) & ~3L;                     // the slab pads dW and db to float4s each; dW / db themselves are not padded
  p.slab = p.nWp + ((Cout + 3) & ~3);
  if (base * p.S >= lim) return false;
  *pl = p;
  return true;
}

template <int MODE, int NKX, bool VA, bool VD>
__global__ __launch_bounds__(256, 2) void wgrad_f32_gather_kernel(const WgGP p) {
  constexpr int HALO = NKX == 3 ? 1 : 0;
  constexpr int APX = a_px_of(MODE), NAJ = APX / 16;
  static_assert(MODE == G_S1 || NKX == 3, "S2 and UP2 are 3x3 only");
  __shared__ __attribute__((aligned(16))) float dyt[TILE_PX * PITCH];
  __shared__ __attribute__((aligned(16))) float at[APX * PITCH];

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int wn = wave & 1, wc = wave >> 1;
  int bid = blockIdx.x;
  const int ky = bid % NKX;
  bid /= NKX;
  const int ct = bid % p.c_tiles;
  bid /= p.c_tiles;
  const int nt = bid % p.n_tiles, s = bid / p.n_tiles;
  const int c0 = ct * 64, n0 = nt * 64;
  const int Hs = p.Hs, Ws = p.Ws, Ho = p.Ho, Wo = p.Wo, Cin = p.Cin, Cout = p.Cout, R = p.R, T = p.T;
  const int SW = MODE == G_S2 ? 2 * Wo + 1 : MODE == G_UP2 ? Ws + 2 : Wo + 2 * HALO;
  const int npx = R * Wo, apx = (MODE == G_UP2 ? (R >> 1) + 1 : R) * SW, ksteps = (npx + 3) >> 2;
  const long t0 = (long)s * p.per, t1 = t0 + p.per < p.NT ? t0 + p.per : p.NT;

  const float* __restrict__ A = p.a;
  const float* __restrict__ DY = p.dy;

  // staging: item j of a thread is channels 4 sf .. 4 sf + 3 of staged pixel sp + 16 j; rel < 0: never loaded (staged as
  // zeros), row: the source row (relative to the tile's first) that decides at run time
  const int sf = tid & 15, sp = tid >> 4;
  int dy_rel[NDY], dy_row[NDY], a_rel[NAJ], a_row[NAJ];
#pragma unroll
  for (int j = 0; j < NDY; ++j) {
    const int px = sp + 16 * j;
    dy_row[j] = px / Wo;
    dy_rel[j] = (px < npx && n0 + 4 * sf < Cout) ? px * Cout + n0 + 4 * sf : -1;
  }
#pragma unroll
  for (int j = 0; j < NAJ; ++j) {
    const int px = sp + 16 * j;
    const int sr = px / SW, col = px - sr * SW;
    int ix, dr;
    if (MODE == G_S2) {          // odd plane (columns -1, 1, .., 2Wo-1), then even plane (0, 2, .., 2Wo-2)
      ix = col <= Wo ? 2 * col - 1 : 2 * (col - Wo - 1);
      dr = 2 * sr;
    } else if (MODE == G_UP2) {
      ix = col - 1;
      dr = sr;
    } else {
      ix = col - HALO;
      dr = sr;
    }
    a_row[j] = dr;
    a_rel[j] = (px < apx && (unsigned)ix < (unsigned)Ws && c0 + 4 * sf < Cin) ? (dr * Ws + ix) * Cin + c0 + 4 * sf : -1;
  }
  f32x4_t dyv[NDY], av[NAJ];
  const f32x4_t zero4 = {0.f, 0.f, 0.f, 0.f};
  // first source row of kernel row ky for the tile whose first output row is row0 (may lie above the image)
  auto src_row0 = [&](int row0) { return MODE == G_S2 ? 2 * row0 + ky - 1 : MODE == G_UP2 ? (row0 + ky - 1) >> 1 : row0 + ky - HALO; };
  auto stage_load = [&](long t) {
    const long b = t / T;
    const int row0 = (int)(t - b * T) * R, iy0 = src_row0(row0);
    const long dy_base = ((b * Ho + row0) * Wo) * (long)Cout;
    const long a_base = ((b * Hs + iy0) * Ws) * (long)Cin;      // may point outside the image: masked per item
#pragma unroll
    for (int j = 0; j < NDY; ++j) {
      const bool ok = dy_rel[j] >= 0 && row0 + dy_row[j] < Ho;
      if (VD) {
        dyv[j] = ok ? *reinterpret_cast<const f32x4_t*>(DY + (dy_base + dy_rel[j])) : zero4;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) dyv[j][e] = (ok && n0 + 4 * sf + e < Cout) ? DY[dy_base + dy_rel[j] + e] : 0.f;
      }
    }
#pragma unroll
    for (int j = 0; j < NAJ; ++j) {
      const bool ok = a_rel[j] >= 0 && (unsigned)(iy0 + a_row[j]) < (unsigned)Hs;
      if (VA) {
        av[j] = ok ? *reinterpret_cast<const f32x4_t*>(A + (a_base + a_rel[j])) : zero4;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) av[j][e] = (ok && c0 + 4 * sf + e < Cin) ? A[a_base + a_rel[j] + e] : 0.f;
      }
    }
  };

  const bool bias_wg = p.db != nullptr && ct == 0 && ky == HALO;
  f32x4_t bsum = zero4;
  auto stage_store = [&]() {
#pragma unroll
    for (int j = 0; j < NDY; ++j) {
      *reinterpret_cast<f32x4_t*>(dyt + (sp + 16 * j) * PITCH + 4 * sf) = dyv[j];
      if (bias_wg) bsum += dyv[j];      // uniform per workgroup
    }
#pragma unroll
    for (int j = 0; j < NAJ; ++j) *reinterpret_cast<f32x4_t*>(at + (sp + 16 * j) * PITCH + 4 * sf) = av[j];
  };

  f32x4_t acc[2][2][NKX];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int kx = 0; kx < NKX; ++kx) acc[i][j][kx] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // 16-channel sub-tiles of this wave that hold any channel at all (wave-uniform)
  const bool n_live0 = n0 + wn * 32 < Cout, n_live1 = n0 + wn * 32 + 16 < Cout;
  const bool c_live0 = c0 + wc * 32 < Cin, c_live1 = c0 + wc * 32 + 16 < Cin;

  const int dy_lane = fq * PITCH + wn * 32 + fr;      // + 4 * PITCH per K-step; + 16 for the second cout 16-tile
  const int a_lane0 = wc * 32 + fr;                   // staged pixel 0
  const int wrap = (SW - Wo) * PITCH;                 // S1 / S2: staged pixels skipped between two output rows
  const int kx1 = MODE == G_S2 ? (Wo + 1) * PITCH : PITCH, kx2 = MODE == G_S2 ? PITCH : 2 * PITCH;      // S1 / S2 tap offsets

  stage_load(t0);
  for (long t = t0; t < t1; ++t) {
    stage_store();
    __syncthreads();
    if (t + 1 < t1) stage_load(t + 1);
    int par = 0;
    if (MODE == G_UP2) par = ((int)(t % T) * R + ky - 1) & 1;

    int cc = fq, rr = 0, aoff = a_lane0 + fq * PITCH;   // the lane's slot: column, row of the tile, staged offset at kx = 0
    for (int ks = 0; ks < ksteps; ++ks) {
      const float* dp = dyt + dy_lane + ks * 4 * PITCH;
      const float d0 = dp[0], d1 = dp[16];
      const bool live = 4 * ks + fq < npx;              // slots past R * Wo: dy = 0 against staged pixel 0
      int o[3];
      if (MODE == G_UP2) {
        const int rowb = ((rr + par) >> 1) * SW;
        o[0] = live ? a_lane0 + (rowb + ((cc + 1) >> 1)) * PITCH : a_lane0;
        o[1] = live ? a_lane0 + (rowb + (cc >> 1) + 1) * PITCH : a_lane0;
        o[2] = o[0] + PITCH;
      } else {
        o[0] = live ? aoff : a_lane0;
        o[1] = o[0] + kx1;
        o[2] = o[0] + kx2;
      }
#pragma unroll
      for (int kx = 0; kx < NKX; ++kx) {
        const float x0 = at[o[kx]], x1 = at[o[kx] + 16];
        if (n_live0 && c_live0) acc[0][0][kx] = __builtin_amdgcn_mfma_f32_16x16x4f32(d0, x0, acc[0][0][kx], 0, 0, 0);
        if (n_live0 && c_live1) acc[0][1][kx] = __builtin_amdgcn_mfma_f32_16x16x4f32(d0, x1, acc[0][1][kx], 0, 0, 0);
        if (n_live1 && c_live0) acc[1][0][kx] = __builtin_amdgcn_mfma_f32_16x16x4f32(d1, x0, acc[1][0][kx], 0, 0, 0);
        if (n_live1 && c_live1) acc[1][1][kx] = __builtin_amdgcn_mfma_f32_16x16x4f32(d1, x1, acc[1][1][kx], 0, 0, 0);
      }
      cc += 4;
      aoff += 4 * PITCH;
      if (cc >= Wo) {         // Wo >= 4: at most one row wrap per step
        cc -= Wo;
        ++rr;
        aoff += wrap;
      }
    }
    __syncthreads();          // every fragment read of this tile before the next tile's stores
  }

  float* __restrict__ ow = p.S > 1 ? p.ws + (size_t)s * p.slab : p.dW;
  float* __restrict__ ob = p.S > 1 ? ow + p.nWp : p.db;

  // lane holds couts n .. n+3 of cin c
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n0 + wn * 32 + i * 16 + 4 * fq, c = c0 + wc * 32 + j * 16 + fr;
      if (c >= Cin) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (n + e >= Cout) continue;
#pragma unroll
        for (int kx = 0; kx < NKX; ++kx)
          ow[((size_t)(n + e) * (NKX * NKX) + ky * NKX + kx) * Cin + c] = acc[i][j][kx][e];
      }
    }

  if (bias_wg) {              // uniform per workgroup; dyt is free since the loop's last barrier
    *reinterpret_cast<f32x4_t*>(dyt + sp * 64 + 4 * sf) = bsum;
    __syncthreads();
    if (tid < 64 && n0 + tid < Cout) {
      float v = 0.f;
#pragma unroll
      for (int g = 0; g < 16; ++g) v += dyt[g * 64 + tid];
      ob[n0 + tid] = v;
    }
  }
}

// the reduce for slabs whose dW / db parts are padded (nW or Cout not a multiple of 4): float4 loads from the padded
// slabs, scalar stores that stop at the end of dW and of db
__global__ __launch_bounds__(256) void wgrad_f32_reduce_ragged_kernel(const float* __restrict__ ws, float* __restrict__ dW,
                                                                      float* __restrict__ db, long nW, long nWp, int Cout, long n4,
                                                                      long slab, int S) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const long e = 4 * i;
  float4 v = *reinterpret_cast<const float4*>(ws + e);
  for (int s = 1; s < S; ++s) {
    const float4 u = *reinterpret_cast<const float4*>(ws + (size_t)s * slab + e);
    v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
  }
  const float r[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (e < nWp) {
      if (e + k < nW) dW[e + k] = r[k];
    } else if (e - nWp + k < Cout) {
      db[e - nWp + k] = r[k];
    }
  }
}

template <int MODE, int NKX>
void launch_gather(const WgGP& p, dim3 g, hipStream_t st) {
  const bool va = p.Cin % 4 == 0, vd = p.Cout % 4 == 0;
  if constexpr (MODE == G_S1 && NKX == 3) {       // at least one side is ragged here: the stride-1 kernel has taken the rest
    if (va) hipLaunchKernelGGL((wgrad_f32_gather_kernel<MODE, NKX, true, false>), g, dim3(256), 0, st, p);
    else if (vd) hipLaunchKernelGGL((wgrad_f32_gather_kernel<MODE, NKX, false, true>), g, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((wgrad_f32_gather_kernel<MODE, NKX, false, false>), g, dim3(256), 0, st, p);
  } else if constexpr (MODE == G_S1) {
    hipLaunchKernelGGL((wgrad_f32_gather_kernel<MODE, NKX, false, false>), g, dim3(256), 0, st, p);
  } else {
    if (va && vd) hipLaunchKernelGGL((wgrad_f32_gather_kernel<MODE, NKX, true, true>), g, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((wgrad_f32_gather_kernel<MODE, NKX, false, false>), g, dim3(256), 0, st, p);
  }
}

}  // namespace

extern "C" int idf_conv_wgrad_f32_plan(int B, int H, int W, int Cin, int Cout, int taps, int* splits_out, long* ws_floats_out) {
  WgPlan pl;
  if (!plan_of(B, H, W, Cin, Cout, taps, &pl)) return 0;
  if (splits_out) *splits_out = pl.S;
  if (ws_floats_out) *ws_floats_out = pl.S > 1 ? pl.S * pl.slab : 0;
  return 1;
}

extern "C" int idf_conv_wgrad_f32(const float* a, const float* dy, float* dW, float* db, float* ws, int B, int H, int W,
                                  int Cin, int Cout, int taps, void* stream) {
  WgPlan pl;
  if (!plan_of(B, H, W, Cin, Cout, taps, &pl))
    IDF_FAIL(IDF_ERR_UNSUPPORTED,
             "conv_wgrad_f32: needs taps 9 or 1, Cin %% 4 == 0, Cout %% 4 == 0 (<= 65536), 4 <= W <= 64, H >= 4 (B=%d H=%d W=%d Cin=%d Cout=%d taps=%d)",
             B, H, W, Cin, Cout, taps);
  if (!a || !dy || !dW) IDF_FAIL(IDF_ERR_BADARG, "conv_wgrad_f32: null a, dy or dW");
  if (pl.S > 1 && !ws) IDF_FAIL(IDF_ERR_BADARG, "conv_wgrad_f32: %d splits need a workspace of %ld floats", pl.S, pl.S * pl.slab);
  WgP p{a, dy, dW, db, ws, H, W, Cin, Cout, pl.R, pl.T, pl.c_tiles, pl.n_tiles, pl.S, pl.per, pl.NT, pl.nW, pl.slab};
  hipStream_t st = (hipStream_t)stream;
  const dim3 g((unsigned)((long)pl.c_tiles * pl.n_tiles * pl.rows * pl.S));
  if (taps == 9) hipLaunchKernelGGL(wgrad_f32_kernel<3>, g, dim3(256), 0, st, p);
  else hipLaunchKernelGGL(wgrad_f32_kernel<1>, g, dim3(256), 0, st, p);
  IDF_CHECK_LAUNCH();
  if (pl.S > 1) {
    const long n4 = (db ? pl.slab : pl.nW) / 4;
    hipLaunchKernelGGL(wgrad_f32_reduce_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, ws, dW, db, pl.nW, n4,
                       pl.slab, pl.S);
    IDF_CHECK_LAUNCH();
  }
  return IDF_OK;
}

extern "C" int idf_conv_wgrad_f32_gather_plan(int B, int Hs, int Ws, int Cin, int Ho, int Wo, int Cout, int mode, int taps,
                                              int* splits_out, long* ws_floats_out) {
  WgGPlan pl;
  if (!gather_plan_of(B, Hs, Ws, Cin, Ho, Wo, Cout, mode, taps, &pl)) return 0;
  if (splits_out) *splits_out = pl.S;
  if (ws_floats_out) *ws_floats_out = pl.S > 1 ? pl.S * pl.slab : 0;
  return 1;
}

extern "C" int idf_conv_wgrad_f32_gather(const float* a, const float* dy, float* dW, float* db, float* ws, int B, int Hs, int Ws,
                                         int Cin, int Ho, int Wo, int Cout, int mode, int taps, void* stream) {
  WgGPlan pl;
  if (!gather_plan_of(B, Hs, Ws, Cin, Ho, Wo, Cout, mode, taps, &pl))
    IDF_FAIL(IDF_ERR_UNSUPPORTED,
             "conv_wgrad_f32_gather: needs mode S1 (taps 9 or 1, Wo <= 64), S2 (taps 9, Ho = (Hs+1)/2, Wo = (Ws+1)/2 <= 32) or UP2 (taps 9, "
             "Ho = 2 Hs, Wo = 2 Ws <= 64), Ho >= 4, Wo >= 4, channels <= 65536 (B=%d Hs=%d Ws=%d Cin=%d Ho=%d Wo=%d Cout=%d mode=%d taps=%d)",
             B, Hs, Ws, Cin, Ho, Wo, Cout, mode, taps);
  if (!a || !dy || !dW) IDF_FAIL(IDF_ERR_BADARG, "conv_wgrad_f32_gather: null a, dy or dW");
  if (pl.S > 1 && !ws)
    IDF_FAIL(IDF_ERR_BADARG, "conv_wgrad_f32_gather: %d splits need a workspace of %ld floats", pl.S, pl.S * pl.slab);
  if (pl.s1) return idf_conv_wgrad_f32(a, dy, dW, db, ws, B, Ho, Wo, Cin, Cout, taps, stream);
  WgGP p{a, dy, dW, db, ws, Hs, Ws, Ho, Wo, Cin, Cout, pl.R, pl.T, pl.c_tiles, pl.n_tiles, pl.S, pl.per, pl.NT, pl.nW, pl.nWp, pl.slab};
  hipStream_t st = (hipStream_t)stream;
  const dim3 g((unsigned)((long)pl.c_tiles * pl.n_tiles * pl.rows * pl.S));
  if (mode == G_S2) launch_gather<G_S2, 3>(p, g, st);
  else if (mode == G_UP2) launch_gather<G_UP2, 3>(p, g, st);
  else if (taps == 9) launch_gather<G_S1, 3>(p, g, st);
  else launch_gather<G_S1, 1>(p, g, st);
  IDF_CHECK_LAUNCH();
  if (pl.S > 1) {
    const long n4 = (db ? pl.slab : pl.nWp) / 4;
    const dim3 rg((unsigned)((n4 + 255) / 256));
    if (pl.nW % 4 == 0 && Cout % 4 == 0)
      hipLaunchKernelGGL(wgrad_f32_reduce_kernel, rg, dim3(256), 0, st, ws, dW, db, pl.nW, n4, pl.slab, pl.S);
    else
      hipLaunchKernelGGL(wgrad_f32_reduce_ragged_kernel, rg, dim3(256), 0, st, ws, dW, db, pl.nW, pl.nWp, Cout, n4, pl.slab, pl.S);
    IDF_CHECK_LAUNCH();
  }
  return IDF_OK;
}
