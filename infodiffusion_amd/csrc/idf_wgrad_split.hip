// fp32 stride-1 NHWC convolution weight gradient (3x3 and 1x1) with the bias gradient fused in, on the bf16 MFMA of gfx950 with
// split operands -- the weight gradient of the opt-in arithmetic modes bf16x3 / bf16x2 (idf_conv3x3_split.hip holds the forward
// and data-gradient convs, idf_wgrad_f32.hip the exact-fp32 kernel whose work split and ordered-slab accumulation this one keeps).
//
//   dW[n][tap][c] = sum_{b,oy,ox} dy[b,oy,ox,n] * a[b,oy+ky-1,ox+kx-1,c]      (tap = ky*3+kx; 1x1: a[b,oy,ox,c])
//   db[n]         = sum_{b,oy,ox} dy[b,oy,ox,n]                                (exact fp32, summed before the split)
//
// Arithmetic (idf_split_bf16.h): v = h + m (+ l), each term rounded to nearest even; the kept cross products go to
// v_mfma_f32_16x16x32_bf16 into ONE fp32 accumulator, smallest first -- TERMS 3: mm, hl, lh, hm, mh, hh; TERMS 2: hm, mh, hh.
// Operand A = dy (rows = cout), operand B = a (cols = cin), K = 32 pixel slots.  BOTH operands are activations: both are split
// on the fly, once per staged tile (not once per tap).
//
// Work split (idf_wgrad_f32.hip's): a 256-thread workgroup owns one (64-cin tile, 64-cout tile, kernel row ky) and a contiguous
// range of pixel tiles (one of S pixel splits); a pixel tile is R whole rows x W columns of one image, R * W <= 64 slots = two
// K steps; each of the 4 waves holds 32 couts x 32 cins x the row's taps (48 accumulator registers at 3x3).  The three kernel rows
// are three workgroups that each stage and split their own tiles.  Per K step a wave issues (2 + 2 NKX) * TERMS * 2 transposed
// reads for 4 * NKX * (6 | 3) MFMAs.
// Not built, not measured: the 768-thread form of idf_wgrad.hip (three 4-wave groups share one (R + 2)-row tile and split each
// element a third as often) -- at three terms its tile, (64 + 6 * 18) x 416 B doubled for its one-barrier pipeline, leaves one
// workgroup per CU with nobody to cover its split phase; and 128-slot tiles in this form, (128 + 160) x 416 B = 117 KB at three
// terms: one workgroup per CU.
//
// Staging: thread = 8 channels (two float4) of staged pixel tid / 8 + 32 j -- 2 dy items and 3 input items a tile, 40 registers
// held across the MFMAs of the previous tile (one LDS buffer, two barriers per tile).  Each item is split in registers
// (idf_pack_bf16: round to nearest even) and stored as TERMS 16-byte runs into per-pixel planes:
//   LDS  dyt[64 slots] | at[80 staged pixels] | 3 zero pixels,  pixel pitch = TERMS * 128 B (64 channels bf16 a plane) + 32 B pad
// i.e. 416 B at three terms (61152 B static), 288 B at two (42336 B): two / three workgroups per CU.  Out-of-image halo pixels,
// masked rows, dy slots past R * W and channels past Cin / Cout are stored as zeros; a K-step slot past R * W reads the zero
// pixels behind `at` (three of them: the taps add up to two pixels), so the MFMA loop has no bounds checks and no 0 * a.
//
// Fragments: a lane of the 16x16x32 MFMA needs 8 consecutive K values (pixels) of one channel; the planes are pixel-major, so
// they come through ds_read_b64_tr_b16 (idf_wgrad.hip's tr_read / mkfrag): lane (g = l / 16, q = l % 16 / 4, pp = l % 4) reads
// the 8 bytes of channels 4 pp .. 4 pp + 3 of slot 32 ks + 4 g + q (and of slot + 16 for the upper half), and receives channel
// l % 16 of slots 4 g .. 4 g + 3 -- the same slot permutation on both operands, so the contraction is unchanged.  Every lane
// carries its own staged-pixel address per (K step, half), computed once per workgroup (a tile is two K steps): K steps wrap
// staged rows (the two halo pixels are skipped) or run past the tile into the zero pixels; tap kx is the uniform offset
// kx * pitch.
// Bank arithmetic of a transposed read: the LDS serves 32 lanes a pass = 8 slots (g = 0, 1 x q) x 32 B (pp x 8 B).  Slot s sits
// at pitch * s + const; pitch = 13 x 32 B resp. 9 x 32 B is an ODD multiple of 32 B, so 8 consecutive staged pixels fall on the 8
// distinct 32-byte groups of the 256-byte bank row: conflict-free (the unpadded 384 / 256 B would put all 8 on one group).
// A K step that wraps a row (W = 7, 14, 28 ...) reads pixels p, p+1, .., p+k, p+k+3, ..: two of the eight can share a group -- a
// 2-way conflict on that pass of the 3x3 only, as in idf_wgrad_f32.hip.  The staging stores (ds_write_b128, 8 lanes a pixel's
// 128-byte plane) overlap the next pixel's by 32 B a 16-lane pass; not measured separately.
//
// Accumulation: idf_wgrad_f32.hip's, unchanged -- S pixel splits that begin and end inside images; S == 1 stores straight into
// dW / db, otherwise split s stores slab s (plain stores, one writer per element) and wgrad_f32_reduce_kernel adds the slabs in
// slab order.  No atomics, no zero-fill: two calls are bit-identical.  The plan keeps the exact kernel's rule for S.
//
// Measured (profiles/f32_split_wgrad.txt section 1): every stride-1 weight-gradient shape of the B = 32 step passed the gate at
// both term counts, the 1x1 included, so the plan takes no shape out.  The staged loads must stay vector-typed: as float4
// structs they compiled to eight predicated dword loads per item and every row measured slower than the exact kernel.
//
// Non-finite inputs, and magnitudes that round to the bf16 infinity, give non-finite outputs (inf - inf in the split).
#include "idf_common.h"
#include "idf_split_bf16.h"
#include "idf_wgrad_f32_parts.h"

namespace {

constexpr int TILE_PX = 64;      // dy pixel slots per tile: two K steps
constexpr int A_PX = 80;         // staged input pixels per tile at most
constexpr int ZERO_PX = 3;       // zero pixels behind the input tile: slots past the tile, at taps 0 .. 2
constexpr int NDY = TILE_PX / 32, NA = (A_PX + 31) / 32;      // staging items (8 channels of a pixel) per thread and tile
constexpr int FULL_GRID = 512;   // two workgroups on each of the 256 CUs
constexpr int MAX_CH = 65536;    // channel counts the plan admits
constexpr int MIN_TILES = 6;     // a split is at least this many pixel tiles (unless the problem has fewer)
constexpr int pitch_of(int terms) { return terms * 128 + 32; }      // bytes per staged pixel

struct WsPlan { int R, T, c_tiles, n_tiles, rows, S, per; long NT, nW, slab; };

struct WsP {
  const float* a;
  const float* dy;
  float* dW;
  float* db;
  float* ws;
  int H, W, Cin, Cout;
  int R, T, c_tiles, n_tiles, S, per;
  long NT, nW, slab;
};

bool plan_of(int B, int H, int W, int Cin, int Cout, int taps, int terms, WsPlan* pl) {
  if (terms != 2 && terms != 3) return false;
  if (taps != 9 && taps != 1) return false;
  if (B < 1 || H < 4 || W < 4 || W > 64 || Cin < 8 || (Cin % 8) || Cout < 8 || (Cout % 8)) return false;
  if (Cin > MAX_CH || Cout > MAX_CH) return false;      // the staging offsets (<= 80 pixels x channels) are ints
  const long lim = 1L << 31;
  if ((long)B * H * W * Cin >= lim || (long)B * H * W * Cout >= lim || (long)Cout * taps * Cin + Cout >= lim) return false;
  WsPlan p;
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
  p.slab = p.nW + Cout;                         // Cin % 8 == 0 and Cout % 8 == 0: a multiple of 4 floats as it stands
  if (base * p.S >= lim) return false;
  *pl = p;
  return true;
}

__device__ __forceinline__ s16x4_t tr_read(const unsigned char* lds_ptr) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(lds_ptr));
}

__device__ __forceinline__ bf16x8_t mkfrag(s16x4_t lo, s16x4_t hi) {
  union { struct { s16x4_t a, b; } s; bf16x8_t v; } u;
  u.s.a = lo; u.s.b = hi;
  return u.v;
}

// NKX = 3: one kernel row of the 3x3 (halo 1); NKX = 1: the 1x1
template <int TERMS, int NKX>
__global__ __launch_bounds__(256, 2) void wgrad_split_kernel(const WsP p) {
  constexpr int HALO = NKX == 3 ? 1 : 0;
  constexpr int PITCH = pitch_of(TERMS);
  __shared__ __attribute__((aligned(16))) unsigned char lds[(TILE_PX + A_PX + ZERO_PX) * PITCH];
  unsigned char* const dyt = lds;
  unsigned char* const at = lds + TILE_PX * PITCH;

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
  const int W = p.W, H = p.H, Cin = p.Cin, Cout = p.Cout, R = p.R, T = p.T;
  const int SW = W + 2 * HALO, npx = R * W, apx = R * SW, ksteps = (npx + 31) >> 5;
  const long t0 = (long)s * p.per, t1 = t0 + p.per < p.NT ? t0 + p.per : p.NT;

  const float* __restrict__ A = p.a;
  const float* __restrict__ DY = p.dy;

  // staging: item j of a thread is channels 8 c8 .. + 7 of staged pixel sp + 32 j; rel < 0: never loaded (staged as zeros),
  // row: the tile row whose image row decides at run time
  const int c8 = tid & 7, sp = tid >> 3;
  int dy_rel[NDY], dy_row[NDY], a_rel[NA], a_row[NA];
#pragma unroll
  for (int j = 0; j < NDY; ++j) {
    const int px = sp + 32 * j;
    dy_row[j] = px / W;
    dy_rel[j] = (px < npx && n0 + 8 * c8 < Cout) ? px * Cout + n0 + 8 * c8 : -1;
  }
#pragma unroll
  for (int j = 0; j < NA; ++j) {
    const int px = sp + 32 * j;
    const int sr = px / SW, ix = px - sr * SW - HALO;
    a_row[j] = sr;
    a_rel[j] = (px < apx && (unsigned)ix < (unsigned)W && c0 + 8 * c8 < Cin) ? (sr * W + ix) * Cin + c0 + 8 * c8 : -1;
  }
  // (vector types, not float4: the struct's conditional load came out as eight predicated global_load_dword per item)
  f32x4_t dyv[NDY][2], av[NA][2];
  const f32x4_t zero4 = {0.f, 0.f, 0.f, 0.f};
  auto f4 = [](const f32x4_t& v) { return make_float4(v[0], v[1], v[2], v[3]); };
  auto stage_load = [&](long t) {
    const long b = t / T;
    const int row0 = (int)(t - b * T) * R;
    const long dy_base = ((b * H + row0) * W) * (long)Cout;
    const long a_base = ((b * H + row0 + ky - HALO) * W) * (long)Cin;      // may point above the image: masked per item
#pragma unroll
    for (int j = 0; j < NDY; ++j) {
      const bool ok = dy_rel[j] >= 0 && row0 + dy_row[j] < H;
      dyv[j][0] = ok ? *reinterpret_cast<const f32x4_t*>(DY + (dy_base + dy_rel[j])) : zero4;
      dyv[j][1] = ok ? *reinterpret_cast<const f32x4_t*>(DY + (dy_base + dy_rel[j] + 4)) : zero4;
    }
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      const bool ok = a_rel[j] >= 0 && (unsigned)(row0 + a_row[j] + ky - HALO) < (unsigned)H;
      av[j][0] = ok ? *reinterpret_cast<const f32x4_t*>(A + (a_base + a_rel[j])) : zero4;
      av[j][1] = ok ? *reinterpret_cast<const f32x4_t*>(A + (a_base + a_rel[j] + 4)) : zero4;
    }
  };

  const bool bias_wg = p.db != nullptr && ct == 0 && ky == HALO;
  float bsum[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) bsum[e] = 0.f;
  auto stage_store = [&]() {
#pragma unroll
    for (int j = 0; j < NDY; ++j) {          // all 64 slots, every tile: slots past R * W and masked rows as zeros
      uint4 tv[TERMS];
      split8<TERMS>(f4(dyv[j][0]), f4(dyv[j][1]), tv);
#pragma unroll
      for (int t = 0; t < TERMS; ++t) *reinterpret_cast<uint4*>(dyt + (sp + 32 * j) * PITCH + t * 128 + c8 * 16) = tv[t];
      if (bias_wg) {                         // uniform per workgroup; the fp32 values, before the split
#pragma unroll
        for (int e = 0; e < 4; ++e) { bsum[e] += dyv[j][0][e]; bsum[4 + e] += dyv[j][1][e]; }
      }
    }
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      if (sp + 32 * j < apx) {               // staged pixels past the tile are never read
        uint4 tv[TERMS];
        split8<TERMS>(f4(av[j][0]), f4(av[j][1]), tv);
#pragma unroll
        for (int t = 0; t < TERMS; ++t) *reinterpret_cast<uint4*>(at + (sp + 32 * j) * PITCH + t * 128 + c8 * 16) = tv[t];
      }
    }
  };

  f32x4_t acc[2][2][NKX];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int kx = 0; kx < NKX; ++kx) acc[i][j][kx] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // 16-channel sub-tiles of this wave that hold any channel at all (wave-uniform)
  const bool n_live[2] = {n0 + wn * 32 < Cout, n0 + wn * 32 + 16 < Cout};
  const bool c_live[2] = {c0 + wc * 32 < Cin, c0 + wc * 32 + 16 < Cin};

  // transposed-read lane geometry: the lane's slot of (K step ks, half h) is 32 ks + 16 h + 4 g + q; its byte offsets into the
  // dy tile and (at tap kx = 0) the input tile, the same for every tile of the workgroup
  const int tq = (lane & 15) >> 2, tpp = lane & 3;
  int dyo[2][2], ao[2][2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int slot = 32 * ks + 16 * h + 4 * fq + tq;
      const int sr = slot / W;
      const int apix = slot < npx ? sr * SW + (slot - sr * W) : A_PX;      // past the tile: the zero pixels
      dyo[ks][h] = slot * PITCH + (wn * 32 + 4 * tpp) * 2;
      ao[ks][h] = apix * PITCH + (wc * 32 + 4 * tpp) * 2;
    }

  if (tid < ZERO_PX * PITCH / 16) *reinterpret_cast<uint4*>(at + A_PX * PITCH + tid * 16) = make_uint4(0, 0, 0, 0);

  stage_load(t0);
  for (long t = t0; t < t1; ++t) {
    stage_store();
    __syncthreads();
    if (t + 1 < t1) stage_load(t + 1);

#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      if (ks < ksteps) {
        bf16x8_t df[2][TERMS];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int tm = 0; tm < TERMS; ++tm)
            df[i][tm] = mkfrag(tr_read(dyt + dyo[ks][0] + i * 32 + tm * 128), tr_read(dyt + dyo[ks][1] + i * 32 + tm * 128));
#pragma unroll
        for (int kx = 0; kx < NKX; ++kx) {
          bf16x8_t xf[2][TERMS];
#pragma unroll
          for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int tm = 0; tm < TERMS; ++tm)
              xf[j][tm] = mkfrag(tr_read(at + ao[ks][0] + kx * PITCH + j * 32 + tm * 128),
                                 tr_read(at + ao[ks][1] + kx * PITCH + j * 32 + tm * 128));
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
              if (n_live[i] && c_live[j]) acc[i][j][kx] = split_mfma<TERMS>(df[i], xf[j], acc[i][j][kx]);
        }
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

  if (bias_wg) {              // uniform per workgroup; the tiles are free since the loop's last barrier
    float* part = reinterpret_cast<float*>(lds);        // [32 pixel groups][64 couts]
    *reinterpret_cast<float4*>(part + sp * 64 + 8 * c8) = make_float4(bsum[0], bsum[1], bsum[2], bsum[3]);
    *reinterpret_cast<float4*>(part + sp * 64 + 8 * c8 + 4) = make_float4(bsum[4], bsum[5], bsum[6], bsum[7]);
    __syncthreads();
    if (tid < 64 && n0 + tid < Cout) {
      float v = 0.f;
#pragma unroll
      for (int g = 0; g < 32; ++g) v += part[g * 64 + tid];
      ob[n0 + tid] = v;
    }
  }
}

template <int TERMS>
void launch(const WsP& p, int taps, dim3 g, hipStream_t st) {
  if (taps == 9) hipLaunchKernelGGL((wgrad_split_kernel<TERMS, 3>), g, dim3(256), 0, st, p);
  else hipLaunchKernelGGL((wgrad_split_kernel<TERMS, 1>), g, dim3(256), 0, st, p);
}

}  // namespace

extern "C" int idf_conv_wgrad_f32_split_plan(int B, int H, int W, int Cin, int Cout, int taps, int terms, int* splits_out,
                                             long* ws_floats_out) {
  WsPlan pl;
  if (!plan_of(B, H, W, Cin, Cout, taps, terms, &pl)) return 0;
  if (splits_out) *splits_out = pl.S;
  if (ws_floats_out) *ws_floats_out = pl.S > 1 ? pl.S * pl.slab : 0;
  return 1;
}

extern "C" int idf_conv_wgrad_f32_split(const float* a, const float* dy, float* dW, float* db, float* ws, int B, int H, int W,
                                        int Cin, int Cout, int taps, int terms, void* stream) {
  WsPlan pl;
  if (!plan_of(B, H, W, Cin, Cout, taps, terms, &pl))
    IDF_FAIL(IDF_ERR_UNSUPPORTED,
             "conv_wgrad_f32_split: needs terms 2 or 3, taps 9 or 1, Cin %% 8 == 0, Cout %% 8 == 0 (<= 65536), 4 <= W <= 64, H >= 4 "
             "(B=%d H=%d W=%d Cin=%d Cout=%d taps=%d terms=%d)",
             B, H, W, Cin, Cout, taps, terms);
  if (!a || !dy || !dW) IDF_FAIL(IDF_ERR_BADARG, "conv_wgrad_f32_split: null a, dy or dW");
  if (pl.S > 1 && !ws)
    IDF_FAIL(IDF_ERR_BADARG, "conv_wgrad_f32_split: %d splits need a workspace of %ld floats", pl.S, pl.S * pl.slab);
  WsP p{a, dy, dW, db, ws, H, W, Cin, Cout, pl.R, pl.T, pl.c_tiles, pl.n_tiles, pl.S, pl.per, pl.NT, pl.nW, pl.slab};
  hipStream_t st = (hipStream_t)stream;
  const dim3 g((unsigned)((long)pl.c_tiles * pl.n_tiles * pl.rows * pl.S));
  if (terms == 3) launch<3>(p, taps, g, st);
  else launch<2>(p, taps, g, st);
  IDF_CHECK_LAUNCH();
  if (pl.S > 1) {
    const long n4 = (db ? pl.slab : pl.nW) / 4;
    hipLaunchKernelGGL(wgrad_f32_reduce_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, ws, dW, db, pl.nW, n4,
                       pl.slab, pl.S);
    IDF_CHECK_LAUNCH();
  }
  return IDF_OK;
}
