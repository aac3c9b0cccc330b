// Weight gradient of every conv of the UNet (autograd of nn.Conv2d in the reference's
// `l_pix.backward()`, model/model.py:54) as a GEMM over pixels on v_mfma_f32_32x32x2_f32:
//     dw[n][tap][c] = sum_{m = (b, oh, ow)} dy[m][n] * a[b, oh*s + r - pad, ow*s + q - pad, c]
// with a = the conv's activated input.  The training driver materialises a = dropout(silu(gn(x0|x1))) once per
// conv (k_apply_act) and passes it as a single source; the generic kernel can also apply the prologue itself and
// folds the nearest x2 upsample / stride into the address (used for the Upsample / Downsample / 1x1 convs).
// Both operands are pixel-major ([m][channels], the natural NHWC order), so a k-step reads its
// fragments with conflict-free ds_read_b32 (lanes along channels).  Workgroup tile TN x TC of one
// filter tap; pixels are walked in chunks of 32, register-prefetched and double-buffered; the pixel
// range is split over gridDim.z and the partial slabs are summed by a deterministic reduce kernel.
// Which kernel runs a layer, and over how many pixel splits, is decided in one place: wgrad_pick.
#include <algorithm>

#include <string.h>

#include "conv_prologue.h"
#include "sr3_common.h"
#include "train.h"

namespace sr3 {

// ---- what the kernels share ------------------------------------------------------------------------------------------------------------
// The frame of a one-tap workgroup: blockIdx.x = (n tile, c tile) of TC-channel tiles, blockIdx.y = the filter tap (fr, fs),
// blockIdx.z = the pixel split, chunks [ch0, ch1) of 32 output pixels.  Hi x Wi: the (upsampled) input map the tap shift is tested against.
struct WgradFrame {
  int Cin, taps, pad, HoWo, M, Hi, Wi, tile_n, tile_c, tap, fr, fs, ch0, ch1;
  __device__ __forceinline__ WgradFrame(const ConvParams& p, int TC, int chunks_per_split) {
    Cin = p.C0 + p.C1;
    taps = p.ksize * p.ksize;
    pad = p.ksize / 2;
    HoWo = p.Ho * p.Wo;
    M = p.B * HoWo;
    Hi = p.Hs << p.ups; Wi = p.Ws << p.ups;
    const int tiles_c = (Cin + TC - 1) / TC;
    tile_n = blockIdx.x / tiles_c; tile_c = blockIdx.x - tile_n * tiles_c;
    tap = blockIdx.y;
    fr = tap / p.ksize; fs = tap - fr * p.ksize;
    const int nchunks = (M + 31) / 32;
    ch0 = blockIdx.z * chunks_per_split;
    ch1 = min(nchunks, ch0 + chunks_per_split);
  }
};

// output pixel m = (b, oh, ow).  logW >= 0: power-of-two feature maps (every real config), shifts instead of divisions
struct OutPix { int b, oh, ow; };
__device__ __forceinline__ OutPix out_pixel(int m, int HoWo, int Wo, int logW, int logHW) {
  OutPix o;
  if (logW >= 0) {
    o.b = m >> logHW;
    const int rem = m & (HoWo - 1);
    o.oh = rem >> logW; o.ow = rem & (Wo - 1);
  } else {
    o.b = m / HoWo;
    const int rem = m - o.b * HoWo;
    o.oh = rem / Wo; o.ow = rem - o.oh * Wo;
  }
  return o;
}

// The activation quad that output pixel `o` meets under the frame's tap: the bounds test (`mcv`: the pixel and the channel quad `ce`
// exist), the address through the concat source with the x2 upsample folded in, and with `act` the quad's GroupNorm pairs.  A quad that
// fails the test reads element 0 and is zeroed when it is staged; returns the test.
__device__ __forceinline__ bool gather_act(const ConvParams& p, const WgradFrame& f, const ConcatQuad<const float>& src, int ce, const OutPix& o,
                                           bool mcv, bool act, f32x4& v, f32x4& sa, f32x4& sb) {
  const int ih = o.oh * p.stride + f.fr - f.pad, iw = o.ow * p.stride + f.fs - f.pad;
  const bool ok = mcv && (unsigned)ih < (unsigned)f.Hi && (unsigned)iw < (unsigned)f.Wi;
  const int pix = (o.b * p.Hs + (ih >> p.ups)) * p.Ws + (iw >> p.ups);
  v = *reinterpret_cast<const f32x4*>(src.base + (ok ? pix * src.C + src.c : 0));
  if (act) {
    const float* q = p.ss + (o.b * f.Cin + ce) * 2;
    sa = *reinterpret_cast<const f32x4*>(q);
    sb = *reinterpret_cast<const f32x4*>(q + 4);
  }
  return ok;
}

// One 32 x 32 accumulator block to the slab (or dw) `dst` [Cout][taps][Cin].  MFMA layout: lane & 31 is the block's column, register r its
// row (r & 3) + 8 (r >> 2) + 4 (lane >> 5); (n0, c0): the block's first output / input channel.
__device__ __forceinline__ void store_block(float* dst, const f32x16& acc, int Cout, int taps, int Cin, int tap, int n0, int c0) {
  const int lane = threadIdx.x & 63;
  const int c = c0 + (lane & 31);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int n = n0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    if (n < Cout && c < Cin) dst[((size_t)n * taps + tap) * Cin + c] = acc[r];
  }
}

// ---- the fp32 one-tap kernel -----------------------------------------------------------------------------------------------------------
constexpr int wgrad_stage_floats(int TN, int TC) { return 32 * (TN + 4 + TC + 4); }          // 32 pixels of dy | activations, rows padded by 4
constexpr int wgrad_lds_bytes(int TN, int TC) { return 2 * wgrad_stage_floats(TN, TC) * 4; }   // two stages

template <int TN, int TC>
__global__ __launch_bounds__(256, 2) void k_conv_wgrad(const ConvParams p, const float* __restrict__ dy,
                                                        float* __restrict__ slabs, int chunks_per_split, int logW,
                                                        int logHW) {
  constexpr int LDN = TN + 4, LDC = TC + 4;
  constexpr int WN = TN / 2, WC = TC / 2;
  constexpr int MI = WN / 32, NI = WC / 32;
  constexpr int STAGE = wgrad_stage_floats(TN, TC);
  extern __shared__ f32x4 smem_v[];
  float* smem = reinterpret_cast<float*>(smem_v);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const WgradFrame f(p, TC, chunks_per_split);

  const int lq = tid & 31, lpx = tid >> 5;        // loader: channel quad, pixel row (0..7) + 8 i
  f32x4 ry[4], ra[4], sa[4], sb[4];
  bool yok[4], aok[4];
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

  auto load = [&](int chunk) {
    const int n = f.tile_n * TN + lq * 4;
    const int c = f.tile_c * TC + lq * 4;
    const bool nv = (lq * 4 < TN) && n < p.Cout;
    const bool cv = (lq * 4 < TC) && c < f.Cin;
    const int ce = cv ? c : 0;
    const auto src = concat_quad(p.src0, p.C0, p.src1, p.C1, ce);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = chunk * 32 + lpx + 8 * i;
      const bool mv = m < f.M;
      const int me = mv ? m : 0;
      const OutPix o = out_pixel(me, f.HoWo, p.Wo, logW, logHW);
      yok[i] = mv && nv;
      ry[i] = *reinterpret_cast<const f32x4*>(dy + (yok[i] ? me * p.Cout + n : 0));
      aok[i] = gather_act(p, f, src, ce, o, mv && cv, p.act != 0, ra[i], sa[i], sb[i]);
    }
  };
  auto store = [&](int st) {
    float* Ys = smem + st * STAGE;
    float* As = Ys + 32 * LDN;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int px = lpx + 8 * i;
      if (lq * 4 < TN) *reinterpret_cast<f32x4*>(&Ys[px * LDN + lq * 4]) = yok[i] ? ry[i] : zero;
      if (lq * 4 < TC) {
        f32x4 v = ra[i];
        if (p.act != 0) {
          v = gn_affine4(v, sa[i], sb[i]);
          if (p.act == 2) v = silu4_libm(v);
        }
        *reinterpret_cast<f32x4*>(&As[px * LDC + lq * 4]) = aok[i] ? v : zero;
      }
    }
  };

  f32x16 acc[MI][NI] = {};

  const int wave_n = wave >> 1, wave_c = wave & 1;
  const int ncol = wave_n * WN + (lane & 31);
  const int ccol = wave_c * WC + (lane & 31);
  const int khalf = lane >> 5;

  if (f.ch0 < f.ch1) {
    load(f.ch0);
    store(0);
    __syncthreads();
    for (int ch = f.ch0; ch < f.ch1; ++ch) {
      const int cur = (ch - f.ch0) & 1;
      const bool more = ch + 1 < f.ch1;
      if (more) load(ch + 1);
      const float* Ys = smem + cur * STAGE;
      const float* As = Ys + 32 * LDN;
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) {
        const int row = 2 * kk + khalf;
        float a[MI], bq[NI];
#pragma unroll
        for (int i = 0; i < MI; ++i) a[i] = Ys[row * LDN + ncol + 32 * i];
#pragma unroll
        for (int j = 0; j < NI; ++j) bq[j] = As[row * LDC + ccol + 32 * j];
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int j = 0; j < NI; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], bq[j], acc[i][j], 0, 0, 0);
      }
      if (more) store(cur ^ 1);
      __syncthreads();
    }
  }

  float* dst = slabs + (size_t)blockIdx.z * p.Cout * f.taps * f.Cin;
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j)
      store_block(dst, acc[i][j], p.Cout, f.taps, f.Cin, f.tap, f.tile_n * TN + wave_n * WN + 32 * i, f.tile_c * TC + wave_c * WC + 32 * j);
}

// ---------------------------------------------------------------------------------------------------
// The same GEMM on v_mfma_f32_32x32x16_bf16 with 3-way split fp32 operands (plan option wgrad_split, default ON, used for the layers
// with more than 64 channels on both sides): six bf16 products per fp32 product, fp32 accumulation -- the arithmetic of the split conv
// kernels.  A 128 x 128 tile of one tap per workgroup (blockIdx.y), so the tap shift lives in the loader's pixel address and nothing has
// to be re-aligned; 3x3 stride-1 layers run here too under wgrad_split (the 9-tap kernel's shared halo would need funnel-shifted
// fragments).
// The contraction runs over PIXELS, which are the rows of both NHWC operands, while a bf16 MFMA operand wants 8 consecutive k per
// lane: the staging step transposes.  A unit of staging = 8 consecutive pixels (one k-half of a 16-pixel k-step) x 4 channels, one unit
// per thread: eight 16-byte loads, per channel one split3x8 of the eight pixel values, three 16-byte LDS writes into
//   plane[3][k-step 2][k-half 2][row][8 bf16]        (row = output channel n for dy, input channel c for the activations)
// so that a lane's MFMA operand is ONE conflict-free ds_read_b128 (lanes along rows).  Single LDS stage, the next chunk's loads in
// flight in registers across the MFMAs.
// ---------------------------------------------------------------------------------------------------
constexpr int SPLIT_T = 128;                              // the tile, both ways
constexpr int SPLIT_ROWS = 2 * SPLIT_T;                   // fragment rows per (k-step, k-half): dy rows then activation rows
constexpr int SPLIT_PLANE = 4 * SPLIT_ROWS * 8;           // bf16 elements per plane [ks 2][kh 2][ROWS][8]
constexpr int SPLIT_LDS_BYTES = 3 * SPLIT_PLANE * 2;      // three planes

template <bool ACT>
__global__ __launch_bounds__(256, 2) void k_conv_wgrad_split(const ConvParams p, const float* __restrict__ dy,
                                                              float* __restrict__ slabs, int chunks_per_split, int logW,
                                                              int logHW) {
  constexpr int TN = SPLIT_T, TC = SPLIT_T, ROWS = SPLIT_ROWS, PLANE = SPLIT_PLANE;
  constexpr int WN = TN / 2, WC = TC / 2;
  constexpr int MI = WN / 32, NI = WC / 32;
  constexpr int PX = 8;                                   // pixels per staging unit
  extern __shared__ f32x4 smem_v[];
  __bf16* planes = reinterpret_cast<__bf16*>(smem_v);     // [plane 3][ks 2][kh 2][ROWS][8]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const WgradFrame f(p, TC, chunks_per_split);

  // staging unit of this thread: threads 0-127 (waves 0, 1) stage dy, threads 128-255 the activations; within an operand the unit
  // is (channel quad uq, pixel group ug): 32 quads x 4 groups of 8 pixels
  const bool is_act = tid >= 128;
  const int u = tid & 127;
  constexpr int QUADS = TN / 4;
  const int uq = u % QUADS, ug = u / QUADS;
  f32x4 rv[PX], sa[ACT ? PX : 1], sb[ACT ? PX : 1];       // (ACT: the GroupNorm pairs of the unit's pixels travel with the prefetch)
  bool rok[PX];
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

  auto load = [&](int chunk) {
    const int n = f.tile_n * TN + uq * 4;
    const int c = f.tile_c * TC + uq * 4;
    const bool nv = n < p.Cout, cv = c < f.Cin;
    const int ce = cv ? c : 0;
    const auto src = concat_quad(p.src0, p.C0, p.src1, p.C1, ce);
    // power-of-two maps at least PX wide: the unit's PX pixels lie in one image row -- decode the first, step the column (the
    // per-pixel decode was a third of this kernel's 6 VALU instructions per MFMA)
    int ub = 0, uoh = 0, uow = 0;
    const bool rowunit = logW >= 3;
    if (rowunit) {
      const int m0 = min(chunk * 32 + ug * PX, f.M - PX);
      ub = m0 >> logHW;
      const int rem = m0 & (f.HoWo - 1);
      uoh = rem >> logW; uow = rem & (p.Wo - 1);
    }
#pragma unroll
    for (int i = 0; i < PX; ++i) {
      const int m = chunk * 32 + ug * PX + i;
      const bool mv = m < f.M;
      const int me = mv ? m : 0;
      int b, oh, ow;          // (three ints set in both branches: an OutPix assigned whole comes out with other registers through the loader)
      if (rowunit) {
        b = ub; oh = uoh; ow = uow + i;
      } else {
        const OutPix o = out_pixel(me, f.HoWo, p.Wo, logW, logHW);
        b = o.b; oh = o.oh; ow = o.ow;
      }
      if (!is_act) {
        rok[i] = mv && nv;
        rv[i] = *reinterpret_cast<const f32x4*>(dy + (rok[i] ? me * p.Cout + n : 0));
      } else {
        // gather_act, spelled out: behind the call both instantiations are scheduled differently and need more registers
        const int ih = oh * p.stride + f.fr - f.pad, iw = ow * p.stride + f.fs - f.pad;
        const bool ok = mv && cv && (unsigned)ih < (unsigned)f.Hi && (unsigned)iw < (unsigned)f.Wi;
        rok[i] = ok;
        const int pix = (b * p.Hs + (ih >> p.ups)) * p.Ws + (iw >> p.ups);
        rv[i] = *reinterpret_cast<const f32x4*>(src.base + (ok ? pix * src.C + src.c : 0));
        if constexpr (ACT) {
          const float* q = p.ss + (b * f.Cin + ce) * 2;
          sa[i] = *reinterpret_cast<const f32x4*>(q);
          sb[i] = *reinterpret_cast<const f32x4*>(q + 4);
        }
      }
    }
  };
  auto store = [&]() {
    f32x4 v[PX];
#pragma unroll
    for (int i = 0; i < PX; ++i) {
      v[i] = rv[i];
      if constexpr (ACT) if (is_act) {
        v[i] = gn_affine4(v[i], sa[i], sb[i]);
        if (p.act == 2) v[i] = silu4_libm(v[i]);
      }
      if (!rok[i]) v[i] = zero;
    }
    // k position of the unit's pixels inside the chunk: pixel index ug * PX + i = 16 ks + 8 kh + i
    const int p0 = ug * PX;
    const int ks = p0 >> 4, kh = (p0 >> 3) & 1;
    // fragment row of channel 4 uq + chn = chn * QUADS + uq: the lanes of a write -- consecutive uq -- hit consecutive 16-byte rows
    // (row 4 uq + chn put them 64 bytes apart: four-way bank conflicts, 60 % of the kernel's LDS cycles); the epilogue un-permutes
    const int row0 = (is_act ? TN : 0) + uq;
#pragma unroll
    for (int chn = 0; chn < 4; ++chn) {
      __bf16* dstp = planes + ((size_t)(ks * 2 + kh) * ROWS + row0 + chn * QUADS) * 8;
      const f32x4 lo = {v[0][chn], v[1][chn], v[2][chn], v[3][chn]}, hi = {v[4][chn], v[5][chn], v[6][chn], v[7][chn]};
      bf16x8 h, m, l;
      split3x8(lo, hi, h, m, l);
      *reinterpret_cast<bf16x8*>(dstp) = h;
      *reinterpret_cast<bf16x8*>(dstp + PLANE) = m;
      *reinterpret_cast<bf16x8*>(dstp + 2 * PLANE) = l;
    }
  };

  f32x16 acc[MI][NI];                        // (cleared by hand: `= {}`, as the other kernels have it, reorders this kernel's set-up code)
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int wave_n = wave >> 1, wave_c = wave & 1;
  const int nrow = wave_n * WN + (lane & 31);             // fragment row of this lane's dy operand (+ 32 i)
  const int crow = TN + wave_c * WC + (lane & 31);        // ... of its activation operand (+ 32 j)
  const int khl = lane >> 5;

  if (f.ch0 < f.ch1) {
    load(f.ch0);
    store();
    __syncthreads();
    for (int ch = f.ch0; ch < f.ch1; ++ch) {
      const bool more = ch + 1 < f.ch1;
      if (more) load(ch + 1);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        bf16x8 a[MI][3], bq[NI][3];
        const __bf16* base = planes + (size_t)(ks * 2 + khl) * ROWS * 8;
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
#pragma unroll
          for (int i = 0; i < MI; ++i) a[i][pl] = *reinterpret_cast<const bf16x8*>(base + pl * PLANE + (nrow + 32 * i) * 8);
#pragma unroll
          for (int j = 0; j < NI; ++j) bq[j][pl] = *reinterpret_cast<const bf16x8*>(base + pl * PLANE + (crow + 32 * j) * 8);
        }
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int j = 0; j < NI; ++j) mfma_split6(a[i], bq[j], acc[i][j]);
      }
      __syncthreads();                       // every fragment of this chunk is read
      if (more) store();
      __syncthreads();
    }
  }

  float* dst = slabs + (size_t)blockIdx.z * p.Cout * f.taps * f.Cin;
  // store_block with the rows un-permuted (fragment row -> channel of the tile: 4 (row % QUADS) + row / QUADS), spelled out: behind the
  // call the ACT instantiation needs more registers
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int cr = wave_c * WC + 32 * j + (lane & 31);
      const int c = f.tile_c * TC + 4 * (cr % QUADS) + cr / QUADS;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int nr = wave_n * WN + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        const int n = f.tile_n * TN + 4 * (nr % QUADS) + nr / QUADS;
        if (n < p.Cout && c < f.Cin) dst[((size_t)n * f.taps + f.tap) * f.Cin + c] = acc[i][j][r];
      }
    }
}

// ---------------------------------------------------------------------------------------------------
// 9-tap variant for the 3x3 stride-1 convs (the bulk of the weight-gradient FLOPs).  A workgroup owns a
// 64 x 64 (n, c) tile of ALL nine taps: per 32-pixel chunk (RPC rows x Wc columns, Wc the largest of 32, 16, 8
// that divides W -- a row segment of a wide map, 2-4 rows of a narrow or a non-power-of-two one) it stages
// dOut[32][64] and the (rows+2) x (cols+2) halo of the materialised activated input ONCE and
// every tap reads its B fragments from the halo at a shifted pixel -- 144 MFMAs per wave per barrier and
// 3.5x fewer staged bytes per MFMA than one tap at a time.  a: [B,H,W,Cin] single source (k_apply_act).
// ---------------------------------------------------------------------------------------------------
constexpr int W9_HPX_MAX = 102;                           // 3 x 34 halo pixels (Wc = 32); 4 x 18, 6 x 10 for Wc = 16, 8
constexpr int W9_STAGE = (32 + W9_HPX_MAX) * 68;          // floats per stage: 32 pixels of dy, the halo; rows of 64 padded by 4
constexpr int W9_LDS_BYTES = 2 * W9_STAGE * 4;            // two stages

__global__ __launch_bounds__(256, 2) void k_conv_wgrad9(const float* __restrict__ a, int Cin,
                                                         const float* __restrict__ dy, int Cout, int B, int H, int W,
                                                         int logWc, float* __restrict__ slabs, int chunks_per_split) {
  constexpr int T = 64, LD = 68;
  constexpr int HPX_MAX = W9_HPX_MAX;
  constexpr int HI = (HPX_MAX * 16 + 255) / 256;     // halo float4 items per thread (7)
  constexpr int STAGE = W9_STAGE;
  extern __shared__ f32x4 smem_v[];
  float* smem = reinterpret_cast<float*>(smem_v);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Wc = 1 << logWc;                         // chunk = RPC rows x Wc columns = 32 pixels (Wc divides W, RPC divides H: wgrad9_ok)
  const int RPC = 32 >> logWc;
  const int HWp = Wc + 2, HR = RPC + 2, HPX = HR * HWp;
  const int cpr = W / Wc;                            // chunks side by side in a band of RPC image rows (W need not be a power of two)
  const int chunks_per_img = (H * W) >> 5;
  const int nchunks = B * chunks_per_img;
  const int tiles_c = (Cin + T - 1) / T;
  const int tile_n = blockIdx.x / tiles_c, tile_c = blockIdx.x - tile_n * tiles_c;
  const int ch0 = blockIdx.z * chunks_per_split;
  const int ch1 = min(nchunks, ch0 + chunks_per_split);

  // loader items (fixed per thread): halo pixel (tid>>4) + 16 j, channel quad tid & 15
  const int lq = tid & 15, lp = tid >> 4;
  int hy[HI], hx[HI];
#pragma unroll
  for (int j = 0; j < HI; ++j) {
    const int hp = lp + 16 * j;
    hy[j] = hp < HPX ? hp / HWp : -1000;
    hx[j] = hp < HPX ? hp - (hp / HWp) * HWp : 0;
  }
  f32x4 rh[HI], ry[2];
  bool hok[HI], yok[2];
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

  auto load = [&](int chunk) {
    const int b = chunk / chunks_per_img;
    const int ci = chunk - b * chunks_per_img;
    const int band = ci / cpr;
    const int oh0 = band * RPC;
    const int ow0 = (ci - band * cpr) * Wc;
    const int c = tile_c * T + lq * 4;
    const int n = tile_n * T + lq * 4;
    const bool cv = c < Cin, nv = n < Cout;
#pragma unroll
    for (int j = 0; j < HI; ++j) {
      const int ih = oh0 + hy[j] - 1, iw = ow0 + hx[j] - 1;
      const bool ok = cv && hy[j] >= 0 && (unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W;
      hok[j] = ok;
      rh[j] = *reinterpret_cast<const f32x4*>(a + (ok ? ((b * H + ih) * W + iw) * Cin + c : 0));
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int px = lp + 16 * i;                    // 0..31
      const int oh = oh0 + (px >> logWc), ow = ow0 + (px & (Wc - 1));
      yok[i] = nv;
      ry[i] = *reinterpret_cast<const f32x4*>(dy + (nv ? ((b * H + oh) * W + ow) * Cout + n : 0));
    }
  };
  auto store = [&](int st) {
    float* Ys = smem + st * STAGE;
    float* Hs = Ys + 32 * LD;
#pragma unroll
    for (int i = 0; i < 2; ++i) *reinterpret_cast<f32x4*>(&Ys[(lp + 16 * i) * LD + lq * 4]) = yok[i] ? ry[i] : zero;
#pragma unroll
    for (int j = 0; j < HI; ++j) {
      const int hp = lp + 16 * j;
      if (hp < HPX) *reinterpret_cast<f32x4*>(&Hs[hp * LD + lq * 4]) = hok[j] ? rh[j] : zero;
    }
  };

  f32x16 acc[9] = {};
  const int wave_n = wave >> 1, wave_c = wave & 1;
  const int ncol = wave_n * 32 + (lane & 31);
  const int ccol = wave_c * 32 + (lane & 31);
  const int khalf = lane >> 5;

  if (ch0 < ch1) {
    load(ch0);
    store(0);
    __syncthreads();
    for (int ch = ch0; ch < ch1; ++ch) {
      const int cur = (ch - ch0) & 1;
      const bool more = ch + 1 < ch1;
      if (more) load(ch + 1);
      const float* Ys = smem + cur * STAGE;
      const float* Hs = Ys + 32 * LD;
#pragma unroll 4
      for (int kk = 0; kk < 16; ++kk) {
        const int px = 2 * kk + khalf;
        const float av = Ys[px * LD + ncol];
        const int hbase = (px >> logWc) * HWp + (px & (Wc - 1));      // halo pixel of tap (0,0)
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          const float bv = Hs[(hbase + (t / 3) * HWp + (t % 3)) * LD + ccol];
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[t], 0, 0, 0);
        }
      }
      if (more) store(cur ^ 1);
      __syncthreads();
    }
  }
  float* dst = slabs + (size_t)blockIdx.z * Cout * 9 * Cin;
#pragma unroll
  for (int t = 0; t < 9; ++t) store_block(dst, acc[t], Cout, 9, Cin, t, tile_n * T + wave_n * 32, tile_c * T + wave_c * 32);
}

__global__ __launch_bounds__(256) void k_wgrad_reduce(const float* __restrict__ slabs, int msplit, size_t n4,
                                                       float* __restrict__ dw) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    // double accumulation: a batch can hold samples whose gradient terms are orders of magnitude larger than the
    // others' (noise levels near 0); summing their slabs with the rest in fp32 costs the small ones their low bits
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    auto slab = [&](int s) { return *reinterpret_cast<const f32x4*>(slabs + ((size_t)s * n4 + i) * 4); };
    int s = 0;
    for (; s + 4 <= msplit; s += 4) {      // four slabs in flight (same order of additions; one load per iteration waited for each in turn)
      const f32x4 v0 = slab(s), v1 = slab(s + 1), v2 = slab(s + 2), v3 = slab(s + 3);
      a0 += (double)v0.x; a1 += (double)v0.y; a2 += (double)v0.z; a3 += (double)v0.w;
      a0 += (double)v1.x; a1 += (double)v1.y; a2 += (double)v1.z; a3 += (double)v1.w;
      a0 += (double)v2.x; a1 += (double)v2.y; a2 += (double)v2.z; a3 += (double)v2.w;
      a0 += (double)v3.x; a1 += (double)v3.y; a2 += (double)v3.z; a3 += (double)v3.w;
    }
    for (; s < msplit; ++s) {
      const f32x4 v = slab(s);
      a0 += (double)v.x; a1 += (double)v.y; a2 += (double)v.z; a3 += (double)v.w;
    }
    const f32x4 r = {(float)a0, (float)a1, (float)a2, (float)a3};
    *reinterpret_cast<f32x4*>(dw + i * 4) = r;
  }
}

namespace {
inline int cdivw(int a, int b) { return (a + b - 1) / b; }
inline int ilog2w(int v) { int l = 0; while ((1 << l) < v) ++l; return (1 << l) == v ? l : -1; }
// chunk width of the 9-tap kernel: the largest of 32, 16, 8 that divides the map width (0: none does)
int wgrad9_chunk_w(int W) { return (W % 32) == 0 ? 32 : (W % 16) == 0 ? 16 : (W % 8) == 0 ? 8 : 0; }
// the 9-tap kernel covers 3x3 stride-1 non-upsampled single-source convs on maps whose width is a multiple of 8 and whose
// height is a multiple of the chunk's rows (32 / chunk width); a power of two is not required
bool wgrad9_ok(const ConvParams& c) {
  if (c.ksize != 3 || c.stride != 1 || c.ups != 0 || c.C1 != 0 || c.act != 0) return false;
  if (c.Ho != c.Hs || c.Wo != c.Ws || c.Ho < 1) return false;
  const int Wc = wgrad9_chunk_w(c.Wo);
  if (Wc == 0) return false;
  return c.Ho % (32 / Wc) == 0;
}
// plan option wgrad_split: the one-tap-per-workgroup split kernel on its 128 x 128 tile, i.e. for every layer with more than 64
// input and output channels (3x3 layers included); the 64-channel layers keep their kernels (a 64 x 64 split tile stages as
// many operand values per MFMA as it saves: 292 VALU instructions per 12 MFMAs)
bool wgrad_use_split(const ConvParams& c) { return c.wgrad_split && c.Cout > 64 && c.C0 + c.C1 > 64; }

// THE choice: which kernel runs the layer, over how many pixel splits (msplit slabs, > 1: summed by k_wgrad_reduce) of how many
// 32-pixel chunks each (cps).  conv_wgrad launches what this says and wgrad_slab_bytes sizes from it; nothing else decides.
// The split is one rule over a row per kernel family: enough splits that `target` workgroups run, capped so that a workgroup keeps at
// least cap_div chunks (its prologue and epilogue are paid once), then evened out over the chunks.
enum WgradKernel { WG_NINE_TAP, WG_SPLIT, WG_FP32_128, WG_FP32_64 };
struct WgradPick { WgradKernel kernel; int tile, msplit, cps; };
WgradPick wgrad_pick(const ConvParams& c) {
  struct Row { int tile, grid_y, target, cap_div; };
  const int Cin = c.C0 + c.C1;
  const bool wide = c.Cout > 64 && Cin > 64;
  WgradPick k;
  k.kernel = wgrad_use_split(c) ? WG_SPLIT : wgrad9_ok(c) ? WG_NINE_TAP : wide ? WG_FP32_128 : WG_FP32_64;
  const Row row = k.kernel == WG_NINE_TAP ? Row{64, 1, 512, 2} : Row{wide ? 128 : 64, c.ksize * c.ksize, 1024, 4};
  k.tile = row.tile;
  const long wgs = (long)cdivw(c.Cout, row.tile) * cdivw(Cin, row.tile) * row.grid_y;          // workgroups per pixel split
  const int nchunks = cdivw(c.B * c.Ho * c.Wo, 32);
  const long ms = std::min((row.target + wgs - 1) / wgs, (long)std::max(nchunks / row.cap_div, 1));
  k.cps = cdivw(nchunks, (int)ms);
  k.msplit = cdivw(nchunks, k.cps);
  return k;
}

// the one-tap kernels: grid (tiles, taps, pixel splits); K's own function-local flag for its LDS attribute
typedef void (*OneTapKernel)(const ConvParams, const float*, float*, int, int, int);
template <OneTapKernel K>
int launch_one_tap(int lds_bytes, const char* name, const WgradParams& p, const WgradPick& k, hipStream_t st) {
  static std::atomic<uint64_t> attr_done{0};
  if (int rc = ensure_max_lds(reinterpret_cast<const void*>(K), lds_bytes, attr_done)) return rc;
  const int Cin = p.c.C0 + p.c.C1;
  dim3 grid(cdivw(p.c.Cout, k.tile) * cdivw(Cin, k.tile), p.c.ksize * p.c.ksize, k.msplit);
  int logW = ilog2w(p.c.Wo), logHW = ilog2w(p.c.Ho * p.c.Wo);
  if (logW < 0 || logHW < 0) logW = logHW = -1;
  hipLaunchKernelGGL(K, grid, dim3(256), lds_bytes, st, p.c, p.dy, k.msplit > 1 ? p.slabs : p.dw, k.cps, logW, logHW);
  SR3_LAUNCH_CHECK(name);
  return SR3_OK;
}
}  // namespace

size_t wgrad_slab_bytes(const ConvParams& c) {
  // the slab size covers BOTH values of wgrad_split (the plan sizes its scratch before it knows the option)
  size_t bytes = 0;
  ConvParams v = c;
  for (int mode = 0; mode < 2; ++mode) {
    v.wgrad_split = mode;
    const int ms = wgrad_pick(v).msplit;
    if (ms > 1) bytes = std::max(bytes, (size_t)ms * c.Cout * c.ksize * c.ksize * (c.C0 + c.C1) * sizeof(float));
  }
  return bytes;
}

int conv_wgrad(const WgradParams& p, hipStream_t st) {
  const ConvParams& c = p.c;
  const int Cin = c.C0 + c.C1;
  if ((c.C0 & 3) || (c.C1 & 3) || (c.Cout & 3)) { set_error("wgrad: channel counts must be multiples of 4"); return SR3_E_UNSUPPORTED; }
  if ((double)c.B * c.Ho * c.Wo * c.Cout >= 2147483647.0 || (double)c.B * c.Hs * c.Ws * (c.C0 > c.C1 ? c.C0 : c.C1) >= 2147483647.0) {
    set_error("wgrad: tensor exceeds 2^31 elements");
    return SR3_E_UNSUPPORTED;
  }
  if (c.act != 0 && !c.ss) { set_error("wgrad: act needs ss"); return SR3_E_BADARG; }
  const WgradPick k = wgrad_pick(c);
  int rc = SR3_OK;
  switch (k.kernel) {
    case WG_SPLIT:
      rc = c.act != 0 ? launch_one_tap<k_conv_wgrad_split<true>>(SPLIT_LDS_BYTES, "k_conv_wgrad_split", p, k, st)
                      : launch_one_tap<k_conv_wgrad_split<false>>(SPLIT_LDS_BYTES, "k_conv_wgrad_split", p, k, st);
      break;
    case WG_FP32_128: rc = launch_one_tap<k_conv_wgrad<128, 128>>(wgrad_lds_bytes(128, 128), "k_conv_wgrad", p, k, st); break;
    case WG_FP32_64: rc = launch_one_tap<k_conv_wgrad<64, 64>>(wgrad_lds_bytes(64, 64), "k_conv_wgrad", p, k, st); break;
    case WG_NINE_TAP: {
      static std::atomic<uint64_t> attr9_done{0};
      if (int rc9 = ensure_max_lds(reinterpret_cast<const void*>(k_conv_wgrad9), W9_LDS_BYTES, attr9_done)) return rc9;
      dim3 grid(cdivw(c.Cout, k.tile) * cdivw(Cin, k.tile), 1, k.msplit);
      hipLaunchKernelGGL(k_conv_wgrad9, grid, dim3(256), W9_LDS_BYTES, st, c.src0, Cin, p.dy, c.Cout, c.B, c.Ho, c.Wo,
                         ilog2w(wgrad9_chunk_w(c.Wo)), k.msplit > 1 ? p.slabs : p.dw, k.cps);
      SR3_LAUNCH_CHECK("k_conv_wgrad9");
      break;
    }
  }
  if (rc) return rc;
  if (k.msplit > 1) {
    const size_t n4 = (size_t)c.Cout * c.ksize * c.ksize * Cin / 4;
    size_t blocks = (n4 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_wgrad_reduce, dim3((unsigned)blocks), dim3(256), 0, st, p.slabs, k.msplit, n4, p.dw);
    SR3_LAUNCH_CHECK("k_wgrad_reduce");
  }
  return SR3_OK;
}

}  // namespace sr3

// ---- per-op entry (include/sr3_mi355x.h): the weight gradient of one convolution, for op-level tests of every kernel of this file ----
namespace {
void wgrad_fill(sr3::ConvParams& c, const float* src0, int C0, const float* src1, int C1, int B, int Hs, int Ws, int ups, int stride, int ksize,
                int Cout, const float* ss, int act, int split) {
  memset(&c, 0, sizeof(c));
  c.src0 = src0; c.src1 = src1; c.C0 = C0; c.C1 = src1 ? C1 : 0; c.B = B; c.Hs = Hs; c.Ws = Ws; c.ups = ups; c.stride = stride; c.ksize = ksize;
  const int pad = ksize / 2;
  c.Ho = ((Hs << ups) + 2 * pad - ksize) / stride + 1;
  c.Wo = ((Ws << ups) + 2 * pad - ksize) / stride + 1;
  c.Cout = Cout; c.ss = ss; c.act = act; c.ksplit = 1; c.wgrad_split = split;
}
}  // namespace
extern "C" size_t sr3_conv_wgrad_scratch_bytes(int B, int Hs, int Ws, int ups, int stride, int ksize, int C0, int C1, int Cout, int split) {
  sr3::ConvParams c;
  wgrad_fill(c, nullptr, C0, C1 ? reinterpret_cast<const float*>(1) : nullptr, C1, B, Hs, Ws, ups, stride, ksize, Cout, nullptr, 0, split);
  return sr3::wgrad_slab_bytes(c);
}
extern "C" int sr3_conv_wgrad_f32(const float* src0, int C0, const float* src1, int C1, int B, int Hs, int Ws, int ups, int stride, int ksize,
                                  int Cout, const float* ss, int act, const float* dy, float* dw_ohwi, int split, void* scratch,
                                  size_t scratch_bytes, void* stream) {
  if (!src0 || !dy || !dw_ohwi) { sr3::set_error("null argument"); return SR3_E_BADARG; }
  if ((ksize != 1 && ksize != 3) || (stride != 1 && stride != 2) || (ups != 0 && ups != 1)) { sr3::set_error("wgrad: ksize 1 | 3, stride 1 | 2, ups 0 | 1"); return SR3_E_UNSUPPORTED; }
  sr3::WgradParams wp;
  wgrad_fill(wp.c, src0, C0, src1, C1, B, Hs, Ws, ups, stride, ksize, Cout, ss, act, split);
  wp.dy = dy; wp.dw = dw_ohwi; wp.slabs = static_cast<float*>(scratch);
  const size_t need = sr3::wgrad_slab_bytes(wp.c);
  const int msplit = sr3::wgrad_pick(wp.c).msplit;
  if (msplit > 1 && scratch && ((uintptr_t)scratch & 15)) { sr3::set_error("wgrad: scratch is not 16-byte aligned"); return SR3_E_ALIGN; }
  if (msplit > 1 && (!scratch || scratch_bytes < need)) { sr3::set_error("wgrad: scratch too small (%zu < %zu)", scratch_bytes, need); return SR3_E_NOMEM; }
  return sr3::conv_wgrad(wp, static_cast<hipStream_t>(stream));
}
