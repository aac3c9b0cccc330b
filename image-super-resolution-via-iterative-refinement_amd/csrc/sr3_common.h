// Internal shared declarations for libsr3_mi355x (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include <atomic>

#include "../../include/sr3_mi355x.h"

namespace sr3 {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// x = h + m + l with three bf16 terms (8 + 8 + 8 significant bits): each residual is exact in fp32.  A pair at a time: one
// v_cvt_pk_bf16_f32 per plane; the residual x - h of either element is one v_dot2c_f32_bf16 (acc += h.lo * -1 + h.hi * 0 and
// the mirrored constant: the bf16 pair is consumed as it is, no unpack to fp32; the result is exactly representable, so the
// instruction's internal rounding does not matter) -- 7 VALU instructions per pair instead of 9 (-DSR3_SPLIT_NO_DOT2: the
// and / shift / packed-subtract form, A/B builds)
__device__ __forceinline__ void split3_pair(float x0, float x1, bf16x2& h, bf16x2& m, bf16x2& l) {
#ifdef SR3_SPLIT_NO_DOT2
  h[0] = (__bf16)x0; h[1] = (__bf16)x1;
  const float r0 = x0 - (float)h[0], r1 = x1 - (float)h[1];
  m[0] = (__bf16)r0; m[1] = (__bf16)r1;
  const float q0 = r0 - (float)m[0], q1 = r1 - (float)m[1];
  l[0] = (__bf16)q0; l[1] = (__bf16)q1;
#else
  // the selectors (-1, 0) / (0, -1) live in registers: as compile-time constants the compiler folds them into the inline
  // constant -1.0, which this instruction reads as 0xBF800000 = (0, -1) for BOTH (measured: garbage results)
  unsigned s_lo = 0x0000BF80u, s_hi = 0xBF800000u;
  asm("" : "+v"(s_lo), "+v"(s_hi));              // (not volatile: one materialisation per kernel, hoisted out of the loops)
  const bf16x2 sel_lo = __builtin_bit_cast(bf16x2, s_lo), sel_hi = __builtin_bit_cast(bf16x2, s_hi);
  h[0] = (__bf16)x0; h[1] = (__bf16)x1;
  const float r0 = __builtin_amdgcn_fdot2_f32_bf16(h, sel_lo, x0, false);
  const float r1 = __builtin_amdgcn_fdot2_f32_bf16(h, sel_hi, x1, false);
  m[0] = (__bf16)r0; m[1] = (__bf16)r1;
  const float q0 = __builtin_amdgcn_fdot2_f32_bf16(m, sel_lo, r0, false);
  const float q1 = __builtin_amdgcn_fdot2_f32_bf16(m, sel_hi, r1, false);
  l[0] = (__bf16)q0; l[1] = (__bf16)q1;
#endif
}
__device__ __forceinline__ void split3(const f32x4 v, bf16x4& h, bf16x4& m, bf16x4& l) {
#pragma unroll
  for (int e = 0; e < 4; e += 2) {
    bf16x2 hh, mm, ll;
    split3_pair(v[e], v[e + 1], hh, mm, ll);
    h[e] = hh[0]; h[e + 1] = hh[1]; m[e] = mm[0]; m[e + 1] = mm[1]; l[e] = ll[0]; l[e + 1] = ll[1];
  }
}

// ... for the eight values a lane contributes to one v_mfma_f32_32x32x16_bf16 operand (k = 0..3 from lo, 4..7 from hi)
__device__ __forceinline__ void split3x8(const f32x4& lo, const f32x4& hi, bf16x8& h, bf16x8& m, bf16x8& l) {
#pragma unroll
  for (int e = 0; e < 8; e += 2) {
    bf16x2 hh, mm, ll;
    split3_pair(e < 4 ? lo[e] : hi[e - 4], e < 4 ? lo[e + 1] : hi[e - 3], hh, mm, ll);
    h[e] = hh[0]; h[e + 1] = hh[1]; m[e] = mm[0]; m[e + 1] = mm[1]; l[e] = ll[0]; l[e + 1] = ll[1];
  }
}
// six bf16 MFMA products of the split operands (a = a_h + a_m + a_l, b likewise), smallest terms first: a.b up to terms <= 2^-24 of it
__device__ __forceinline__ void mfma_split6(const bf16x8 (&a)[3], const bf16x8 (&b)[3], f32x16& acc) {
  constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
  for (int q = 0; q < 6; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[PA[q]], b[PB[q]], acc, 0, 0, 0);
}

// ---- 16-byte stores of an epilogue, plain or written through L2 (plan option store_wt) ----
// A plain store leaves its line dirty in the XCD's L2, and the kernel boundary behind it writes those lines back before the next kernel
// starts; a write-through store (sc1) sends the bytes on while the kernel still runs and leaves nothing to flush.  Only 16-byte stores
// are written through: narrower sc1 stores cost a fabric write each.  The write-through form is a buffer store (one 32-bit byte offset
// from a wave-uniform base; the compiler counts it in vmcnt like any other store; `wt` a compile-time constant in the big kernels), so a tensor -- or a set of split-K slabs -- of 4 GiB
// or more keeps plain stores: store_wt_fits, decided on the host.  Bits of ConvParams::store_wt / plan option store_wt, one per family:
enum {
  STORE_WT_WINO2 = 1,      // k_conv3x3_wino2, every instantiation: outputs and split-K slabs
  STORE_WT_WINO = 2,       // k_conv3x3_wino, the 8-wave kernel: the four-image split-K form of the 8 x 8 maps (what the default plans run): slabs
  STORE_WT_REDUCE = 4,     // k_rows_fold<true> and k_splitk_reduce: the reduced output
  STORE_WT_ALL = 7,
};
inline bool store_wt_fits(size_t bytes) { return bytes < ((size_t)1 << 32); }
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
struct WtDst {
  __amdgpu_buffer_rsrc_t rsrc;
  float* base;
  bool wt;                 // wave-uniform
};
// base: wave-uniform; bytes < 4 GiB when wt (host: store_wt_fits)
__device__ __forceinline__ WtDst wt_dst(float* base, size_t bytes, bool wt) {
  return WtDst{__builtin_amdgcn_make_buffer_rsrc(base, 0, wt ? (int)(unsigned)bytes : 0, 0x00020000), base, wt};
}
// base[elem .. elem + 3] = v (16-byte aligned)
__device__ __forceinline__ void store16(const WtDst& d, size_t elem, const f32x4 v) {
  if (d.wt) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), d.rsrc, (int)(unsigned)(elem * sizeof(float)), 0, /*aux: sc1*/ 16);
  else *reinterpret_cast<f32x4*>(d.base + elem) = v;
}

// sigmoid / SiLU of the staging and activation-backward steps: libm expf (1 ulp) and the hardware reciprocal v_rcp_f32
// (1 ulp).  Measured against float64 autograd at batch 64 (profiles/r04_grad_probe.txt): parameter gradients are within 5e-7
// of float64 with these, the same as with an IEEE division (-DSR3_EXACT_ACT, A/B builds only) and as stock PyTorch-ROCm.
#ifdef SR3_EXACT_ACT
#define SR3_SIGMOID(v) (1.0f / (1.0f + expf(-(v))))
#define SR3_SILU(v) ((v) / (1.0f + expf(-(v))))
#else
#define SR3_SIGMOID(v) __builtin_amdgcn_rcpf(1.0f + expf(-(v)))
#define SR3_SILU(v) ((v) * __builtin_amdgcn_rcpf(1.0f + expf(-(v))))
#endif

// ---- error plumbing (thread-local message, int codes: 0 ok, >0 hipError_t, <0 engine) ----
enum { SR3_OK = 0 };   // SR3_E_* come from the public header
void set_error(const char* fmt, ...);
int hip_fail(hipError_t e, const char* what);
#define SR3_HIP(call)                                   \
  do {                                                  \
    hipError_t _e = (call);                             \
    if (_e != hipSuccess) return sr3::hip_fail(_e, #call); \
  } while (0)
#define SR3_LAUNCH_CHECK(name)                          \
  do {                                                  \
    hipError_t _e = hipGetLastError();                  \
    if (_e != hipSuccess) return sr3::hip_fail(_e, name); \
  } while (0)

// hipFuncAttributeMaxDynamicSharedMemorySize is a PER-DEVICE attribute: remember which devices a kernel instantiation has
// been prepared on (one bit per device ordinal) so a process that drives several GPUs -- the reference's single-process
// DataParallel layout -- sets it on each of them.  `done` is a function-local static of the launcher.
inline int ensure_max_lds(const void* kern, int bytes, std::atomic<uint64_t>& done) {
  int dev = 0;
  SR3_HIP(hipGetDevice(&dev));
  const uint64_t bit = 1ull << (dev & 63);
  if (done.load(std::memory_order_acquire) & bit) return SR3_OK;
  SR3_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  done.fetch_or(bit, std::memory_order_release);
  return SR3_OK;
}

// The C ABI carries fp32 hyper-parameters (lr, betas, dropout p) while the reference evaluates expressions of them as
// Python floats (double): recover the decimal the caller meant (0.2f -> 0.2, 1e-4f -> 1e-4) = the shortest decimal
// that rounds back to the same float, so derived quantities (Adam bias corrections, the dropout threshold p * 2^32)
// match the reference's double arithmetic exactly.
double meant_double(float f);
// dropout p -> (keep threshold on the 32-bit hash, 1 / (1 - p)); one definition for every entry point and the oracle
inline void dropout_consts(float p, unsigned* thresh, float* scale) {
  const double pd = meant_double(p);
  *thresh = p > 0.f ? (unsigned)(pd * 4294967296.0) : 0u;
  *scale = p > 0.f ? (float)(1.0 / (1.0 - pd)) : 1.0f;
}

// The GroupNorm fold of the op that FOLLOWS, done in the tail of the kernel that completes this tensor (round 6; plan option fold_fuse):
// k_rows_fold (small_kernels.hip) walks the tensor per (image, consumer group) -- as the split-K reduce of a conv (ConvParams::fold)
// or as the stand-alone statistics pass -- so a workgroup holds the whole-image sums of its group's channels: it writes them as this
// tensor's partials (one per image: T = 1), adds the other concat source's channels of the group from ITS partials, and writes the
// consumer's (scale, shift) pairs.  No atomics, fixed summation order; one launch instead of two (reduce / statistics + fold).
struct FoldTailPlain {
  int groups, Ctot, c_off;     // the consumer's GroupNorm: `groups` over Ctot channels; this tensor is channels [c_off, c_off + C) of them
  const double* ostat;         // the other concat source's partials [B][oT][oC][2], its channels at [o_off, o_off + oC); null: single source
  int oC, oT, o_off;
  const float* gamma;          // [Ctot]
  const float* beta;
  float eps;
  float* ss;                   // out: [B][Ctot][2]
  float* mr;                   // out: [B][groups][2] (mean, rstd) or null (training keeps them for the backward)
};
// ... with a scale-shift modulation of the consumer's GroupNorm (plan flag SR3_UNET_SCALE_SHIFT_NORM; fold_modulate, small_kernels.hip):
// image b's scales [Ctot] then shifts [Ctot] at mod + b * mod_stride; null: none.  The kernels without a modulation take the plain
// struct, so their argument layout is what it was
struct FoldTail : FoldTailPlain {
  const float* mod;
  int mod_stride;
};
bool fold_tail_fits(int C, int Ctot, int c_off, int groups);
// stand-alone form: statistics of x [B][HW][C] (partials [B][1][C][2] into `stat`) + the fold
int chan_stats_fold(const float* x, int B, int HW, int C, double* stat, const FoldTail& f, hipStream_t st);

// ---- convolution (implicit GEMM on v_mfma_f32_32x32x2_f32) --------------------------------
// Activations are NHWC fp32.  The input is the *virtual* channel concat of up to two sources,
// optionally nearest-upsampled x2 (gather in the address math), optionally strided.
// Prologue (per input element, before zero padding): none | x*scale+shift | silu(x*scale+shift)
// with (scale, shift) per (image, input channel) = GroupNorm folded with its affine; then the train-mode dropout mask.
// conv_prologue.h is its definition: the source select, the affine, the two SiLU forms and the mask index every kernel stages through.
// Epilogue: + bias[n] + film[b][n] + residual[m][n] (residual is itself a two-source concat view).
struct ConvParams {
  const float* src0;
  const float* src1;
  int C0, C1;          // channels of src0 / src1 (C1 = 0 when no concat); both % 4 == 0
  int B, Hs, Ws;       // source spatial dims
  int ups;             // 1: nearest x2 upsample of the source before the conv
  int stride;          // 1 | 2
  int ksize;           // 1 | 3  (pad = ksize / 2)
  int Ho, Wo;          // output spatial dims
  int Cout;
  const float* w;      // [Cout][ksize*ksize][Cin]   (OHWI)
  const float* bias;   // [Cout] or null
  const float* ss;     // [B][Cin][2] (scale, shift) or null
  int act;             // 0 none, 1 affine, 2 affine + SiLU
  const float* film;   // film[b * film_stride + n] or null
  int film_stride;
  const float* res0;   // residual, NHWC [B,Ho,Wo,RC0 (+RC1)] or null
  const float* res1;
  int RC0, RC1;
  float* out;          // [B,Ho,Wo,Cout]
  float* partial;      // split-K scratch [ksplit][M][Cout] (ksplit > 1)
  int ksplit;
  double* ostat;       // optional (halo kernel only): partial {sum, sumsq} of the OUTPUT, [B][T][Cout][2]
  int dbg;             // profiling ablations only (env SR3_CONV_DBG): 1 = skip MFMA + fragment reads, 2 = skip staging, 4 = skip the global loads only, 8 = skip the LDS writes (and the split) only
  // Optional second K-segment (halo kernel only): a 1x1 conv of another tensor (virtual concat
  // x2_src0|x2_src1, same spatial size as the output, no prologue) accumulated into the same
  // output tile -- ResnetBlock's `res_conv(x)` (unet.py:102-103,110) folded into block2's conv.
  const float* x2_src0;
  const float* x2_src1;
  int x2_C0, x2_C1;
  const float* x2_w;    // [Cout][x2_C0 + x2_C1]
  const float* x2_bias; // [Cout] or null
  // Train-mode dropout between the activation and the conv (nn.Dropout of Block, unet.py:86): an
  // activated input element with NHWC linear index i is kept iff hash32(i * 0x9E3779B9 + drop_seed) >=
  // drop_thresh and scaled by drop_scale = 1 / (1 - p).  drop_thresh == 0 disables it.  Only defined for
  // single-source, non-upsampled inputs (block2's input is never a concat).
  unsigned drop_seed, drop_thresh;
  float drop_scale;
  // tile_cfg 11 (Winograd): this conv's transformed filters in fragment-major order (conv3x3_wino.hip)
  const float* wino_u;
  int wino_split;      // 1: the filters are the 3 x bf16 split form and the kernel's SPLIT instantiation runs (tile_cfg 12 at the ABI);
                       // 2: the same filters on the two-workgroups-per-CU kernel of conv3x3_wino2.hip (tile_cfg 13; 8 x 16 pixel tile)
                       // 3: ... on that kernel's RAGGED instantiation (tile_cfg 23): maps that are not whole multiples of the tile
  int igemm_split;     // im2col kernel (tile_cfg 1-4; 1x1 and stride-2 convs): 1 = its 3 x bf16 split instantiation (tile_cfg 14-17 at the ABI)
  int wgrad_split;     // weight gradient (wgrad.hip): 1 = the one-tap-per-workgroup kernel's 3 x bf16 split instantiation for the layers with > 64 channels on both sides
  const FoldTail* fold; // host side only (conv_forward): split-K convs -- the reduce runs as k_rows_fold and does the next op's GroupNorm fold too;
                        // ostat then holds ONE partial per image
  const void* w_split; // igemm_split: the weights pre-split into bf16 planes by igemm_split_weights (tile_cfg 18-21 at the ABI; a plan
                       // keeps them in its derived buffer); null: the kernel splits the weights while it stages them
  int wino_full;       // wino_split 2 / 3 with ups == 1: 1 = all sixteen Winograd positions (tile_cfg 25 / 26 at the ABI; plan option wino_up = 0);
                       // 0: the UP instantiation of conv3x3_wino2.hip, which skips the seven positions whose operand is exactly zero
  int store_wt;        // STORE_WT_* bits (above): which kernels of this conv write their 16-byte stores through L2; 0: plain stores everywhere.
                       // Set per launch from the plan option; conv_forward clears the write-through bits where store_wt_fits says no
  int gemm_epi;        // the GEMM kernel's epilogue (gemm1x1.hip, template parameter EPI): 0 = the library's default form (GEMM_EPI_DEFAULT: tile_cfg
                       // 22 at the ABI), 1 + form names one: 1 = the 4-byte epilogue, 2 = 16-byte stores, 3 = 16-byte stores written through L2
                       // (tile_cfg 27 / 28 / 29; plan option gemm_epi = form).  gemm1x1_forward drops form 2 to 1 where store_wt_fits says no
};
// the form ConvParams::gemm_epi == 0 and a fresh plan run: what measured fastest (profiles/gemm_epi_ab.txt)
constexpr int GEMM_EPI_DEFAULT = 2;

__device__ __forceinline__ unsigned hash32(unsigned x) {
  x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
  return x;
}
__device__ __forceinline__ float drop_mask(unsigned seed, unsigned idx, unsigned thresh, float scale) {
  return hash32(idx * 0x9E3779B9U + seed) >= thresh ? scale : 0.f;
}

// ---- conv dispatch (conv_dispatch.hip) over the five kernel families: im2col (conv_igemm.hip), halo, Winograd 8-wave, Winograd
// two-workgroup, plain GEMM.  tile_cfg is the kernel tile itself (tile_code.h has the numbers), 0 = conv_pick chooses; ksplit 0 = auto
struct ConvPick { int tile, ksplit; };
ConvPick conv_pick(const ConvParams& p, int tile_cfg, int ksplit);
// mid (profiling): recorded between the conv kernel and the split-K reduce, when the conv splits
int conv_forward(const ConvParams& p, int tile_cfg, int ksplit, float* splitk_scratch, size_t splitk_scratch_bytes, hipStream_t st,
                 hipEvent_t mid = nullptr);
// scratch bytes the auto heuristic may ask for (upper bound) for this problem
size_t conv_splitk_bytes(const ConvParams& p, int tile_cfg, int ksplit);
int splitk_rows_per_block(const ConvParams& p, bool stats);
// the reduce behind a split-K conv (small_kernels.hip): k_rows_fold where p.fold is set, k_splitk_reduce otherwise
int splitk_reduce(const ConvParams& p, hipStream_t st);
// THE split-K rule: `units` k-steps (or chunks) over ks splits of cdiv(units, ks) each.  Below `below` workgroups, as many splits as
// fill `round` workgroup slots, at least min_units per split, at most 16, and none of them empty
inline bool split_leaves_empty(int units, int ks) { return ks > 1 && (long)(ks - 1) * ((units + ks - 1) / ks) >= units; }
inline int split_shrink(int units, int ks) { while (split_leaves_empty(units, ks)) --ks; return ks; }
inline int split_k(long tiles, long below, long round, int units, int min_units) {
  int ks = 1;
  if (tiles < below && tiles > 0) {
    ks = (int)((round + tiles - 1) / tiles);
    const int cap = units / min_units > 1 ? units / min_units : 1;
    if (ks > cap) ks = cap;
    if (ks > 16) ks = 16;
  }
  return split_shrink(units, ks);
}
// the im2col kernel on tile 1-4 (conv_igemm.hip); p.igemm_split / p.w_split select the 3 x bf16 split instantiations
int conv_igemm_forward(const ConvParams& p, int tile, hipStream_t st);
// pre-split weights of the im2col SPLIT instantiations: floats of the derived block for `numel` weights, and the transform
size_t igemm_wsplit_floats(int Cout, int taps, int Cin);
int igemm_split_weights(const float* w, int Cout, int taps, int Cin, float* out, hipStream_t st);
// 1x1 stride-1 convs as a plain GEMM on the split arithmetic (gemm1x1.hip; tile_cfg 22: 64 x 128 tile, mi = 2; needs w_split)
bool gemm1x1_fits(const ConvParams& p, int mi);
int gemm1x1_cols(const ConvParams& p);      // 128, or 64 (waves 2 x 2) where Cout % 128 != 0
int gemm1x1_forward(const ConvParams& p, int mi, hipStream_t st);
int gemm1x1_rows(const ConvParams& p);      // 64, or 32 where 64-row tiles would leave workgroup slots empty
struct HaloGeom {
  int TH, TW, NB;          // spatial tile per image, images per workgroup tile (TH*TW*NB = BM)
  int log_tw, log_thw;     // log2(TW), log2(TH*TW)
  int tiles_w, tiles_h;    // tiles per image
  int HPI, HP;             // halo pixels per image / per workgroup
};
// halo-tile configurations: 5 = 128(M) x 128(N), 6 = 256 x 64 (4 waves, two workgroups per CU); 9 = 256 x 128
// (8 waves, one workgroup per CU); 7 / 8 / 10 = the split-bf16 instantiations of 5 / 6 / 9 (8 runs its 256 x 64
// tile on 8 waves of 64 x 32)
inline bool halo_cfg_one_wg_per_cu(int cfg) { return cfg >= 8; }
inline int halo_cfg_bm(int cfg) { return (cfg == 5 || cfg == 7) ? 128 : 256; }
inline int halo_cfg_bn(int cfg) { return (cfg == 6 || cfg == 8) ? 64 : 128; }
inline bool halo_cfg_split(int cfg) { return cfg == 7 || cfg == 8 || cfg == 10; }
bool halo_geometry(const ConvParams& p, int cfg, HaloGeom* g);
int conv3x3_halo_forward(const ConvParams& p, int cfg, const HaloGeom& g, hipStream_t st);

// Winograd F(2x2, 3x3) form of the same conv (conv3x3_wino.hip): tile_cfg 11.  The transformed filters U = G g G^T live
// in a "derived" buffer in fragment-major order (wino_weight_floats floats per conv), rebuilt by wino_transform_weights
// whenever the weights change.
struct WinoGeom {
  int TH, TW, NB;        // output pixels per image in the workgroup tile, images per tile
  int twt, log_twt;      // Winograd (2x2) tiles per tile row
  int tpi, log_tpi;      // Winograd tiles per image of the workgroup tile
  int tiles_w, tiles_h;  // workgroup tiles per image
  int nbt;               // batch tiles: B (one image per tile) or B / 4 (NB = 4: four 8 x 8 images per tile)
  int HPI, HP;           // raw halo pixels per image / per workgroup
  int log_tw, log_th, pow2;   // tile decode of the persistent kernel: tiles_w / tiles_h as shifts when both are powers of two
  unsigned sp_magic;          // ceil(2^32 / (tiles_w * tiles_h * B)): tile id / tiles-per-cout-block as a multiply-high
};
bool wino_geometry(const ConvParams& p, WinoGeom* g);
int wino_stats_slices(const WinoGeom& g);
int wino_max_chunks_per_split(const WinoGeom& g);     // 64 (1024 input channels); 16 for the four-image tile
long wino_workgroups(const ConvParams& p, const WinoGeom& g);
int wino_chunks(const ConvParams& p);
size_t wino_weight_floats(int Cout, int Cin, bool split = false);
int wino_transform_weights(const float* w_ohwi, int Cout, int Cin, float* ufrag, hipStream_t st, bool split = false);
int conv3x3_wino_forward(const ConvParams& p, const float* ufrag, hipStream_t st);
// the 3 x bf16 split form as two independent four-wave workgroups per CU, 8 x 16 pixel tile (conv3x3_wino2.hip; ConvParams::wino_split == 2,
// tile_cfg 13 at the ABI; wino_geometry gives that tile's geometry when wino_split == 2)
bool wino2_fits(const ConvParams& p);
bool wino2_ragged_fits(const ConvParams& p);     // wino_split == 3: wino2_fits without the divisibility conditions
int conv3x3_wino2_forward(const ConvParams& p, const WinoGeom& g, const float* ufrag, hipStream_t st);

// ---- small kernels ------------------------------------------------------------------------
// partial per-(b, channel) {sum, sumsq} in double of an NHWC tensor [B, HW, C]:
// stat[B][T][C][2] with T = chan_stats_slices(B, HW, C); plain stores, no memset needed.
int chan_stats_slices(int B, int HW, int C);
int chan_stats(const float* x, int B, int HW, int C, double* stat, hipStream_t st);
// GroupNorm fold: partial stats of up to two concat sources + gamma/beta -> ss[B][C0+C1][2]
int gn_finalize(const double* stat0, int C0, int T0, const double* stat1, int C1, int T1, int B, int HW, int groups,
                const float* gamma, const float* beta, float eps, float* ss, hipStream_t st, float* mr = nullptr,
                const float* mod = nullptr, int mod_stride = 0);      // mod: scale-shift modulation rows (fold_modulate), null: none
// partials per image the halo conv writes into ConvParams::ostat for this geometry
int halo_stats_slices(const HaloGeom& g);
// first conv of the UNet: NCHW inputs (virtual concat of a: Ca, b: Cb channels), 3x3 pad 1,
// weights OHWI [Cout][9][Ca+Cb], output NHWC [B,H,W,Cout]
// statistics partials per image conv_in_nchw writes into `ostat` for this shape (0: no fused statistics: VALU kernel)
int conv_in_stat_slices(int Cin, int H, int W, int Cout);
int conv_in_nchw(const float* a, int Ca, const float* b, int Cb, int B, int H, int W, const float* w,
                 const float* bias, int Cout, float* out, double* ostat, hipStream_t st);
// fused reverse-step update (NCHW, elementwise): coef = {a, b, c1, c2, sigma} tables of length T
struct StepTables { const float* a; const float* b; const float* c1; const float* c2; const float* sigma; };

// ---- the tail of a reverse step (sr3 diffusion.py:141-149,162-174; ddpm :151-198), defined here once ----
//   x0 = a_t x - b_t eps ; clamp[-1,1] ; mean = c1_t x0 + c2_t x (+ c3_t hist ; hist <- x0) ; x <- mean + sigma_t z
// Every product, sum and difference is rounded on its own: the empty asm makes the value opaque, so hipcc (default
// -ffp-contract=fast) cannot fuse it into an fma.  That makes the update bit-identical to the reference's elementwise torch ops for
// the same eps -- and its three users (k_p_sample_update, the FUSE epilogue of k_conv_out_nchw, k_tiled_step) to one another.
__device__ __forceinline__ float mul_rn(float a, float b) { float r = a * b; asm volatile("" : "+v"(r)); return r; }
__device__ __forceinline__ float add_rn(float a, float b) { float r = a + b; asm volatile("" : "+v"(r)); return r; }
__device__ __forceinline__ float sub_rn(float a, float b) { float r = a - b; asm volatile("" : "+v"(r)); return r; }
struct StepCoef { float a, b, c1, c2, c3, sigma; };
// row t of the tables; HIST false: no history, the c3 table is not read
template <bool HIST>
__device__ __forceinline__ StepCoef load_step_coef(const StepTables& tb, const float* c3, int t) {
  return StepCoef{tb.a[t], tb.b[t], tb.c1[t], tb.c2[t], HIST ? c3[t] : 0.f, tb.sigma[t]};
}
// one element in two halves, so that a rule for x0 (the block-mean projection of consistency.hip) has a place between them:
//   step_x0: x0 = a x - b eps, clamped when clip (clip_denoised, sr3 diffusion.py:162-163)
//   step_mix: returns the new x = ((c1 x0 + c2 x) + c3 hist) + sigma z.  HIST (the multistep tail): + c3 hist before the noise term, then
//   hist <- x0; the caller's thread owns the element's history, loads it before and stores it after
__device__ __forceinline__ float step_x0(const StepCoef& k, bool clip, float x, float eps) {
  float x0 = sub_rn(mul_rn(k.a, x), mul_rn(k.b, eps));
  if (clip) x0 = fminf(fmaxf(x0, -1.f), 1.f);
  return x0;
}
template <bool HIST>
__device__ __forceinline__ float step_mix(const StepCoef& k, float x0, float x, float z, float& hist) {
  float mean = add_rn(mul_rn(k.c1, x0), mul_rn(k.c2, x));
  if (HIST) { mean = add_rn(mean, mul_rn(k.c3, hist)); hist = x0; }
  return add_rn(mean, mul_rn(z, k.sigma));
}
// ... and their composition: the whole tail of one element, what the three users above run
template <bool HIST>
__device__ __forceinline__ float step_tail(const StepCoef& k, bool clip, float x, float eps, float z, float& hist) {
  return step_mix<HIST>(k, step_x0(k, clip, x, eps), x, z, hist);
}
// do the byte ranges [a, a + abytes) and [b, b + bbytes) share a byte?  (host side: the argument checks of the step tails)
inline bool overlaps(const void* a, size_t abytes, const void* b, size_t bbytes) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + bbytes && b0 < a0 + abytes;
}
// host check of a step's history arguments, before anything is launched: c3 and hist both or neither; hist (`bytes` long, as x and eps
// are) overlaps neither x nor eps (eps may be null); align16: the caller's kernel needs hist 16-byte aligned
inline int check_step_history(const char* who, const float* c3, const float* hist, const float* x, const float* eps, size_t bytes,
                              bool align16 = false) {
  if ((c3 != nullptr) != (hist != nullptr)) { set_error("%s: the c3 table and the history go together (both or neither)", who); return SR3_E_BADARG; }
  if (!hist) return SR3_OK;
  const uintptr_t h0 = (uintptr_t)hist;
  if (align16 && (h0 & 15)) { set_error("misaligned pointer (hist: 16 B)"); return SR3_E_ALIGN; }
  for (const float* p : {x, eps}) {
    const uintptr_t p0 = (uintptr_t)p;
    if (p && p0 < h0 + bytes && h0 < p0 + bytes) { set_error("%s: the history overlaps x or eps", who); return SR3_E_BADARG; }
  }
  return SR3_OK;
}

// the state of a step's tail behind a kernel that produces eps (the output conv's epilogue: sr3_reverse_step; the tile blend:
// sr3_tiled_step): x <- step_tail(x, eps, z) at t = *step_cur, and *step_next = t - 1 (one thread)
struct StepFuse {
  float* x;               // [B, Cout, H, W] in / out
  const float* z;         // noise or null (= 0)
  StepTables tb;
  const int* step_cur;    // t of this step (written by the embedding kernel of the same forward)
  int* step_next;         // t of the next step
  int clip;
  // multistep tail (both set or both null; behind the older fields, whose offsets the kernels without history keep): x <- ... + c3[t] hist
  const float* c3;        // table of the previous x0's coefficient, indexed like tb
  float* hist;            // the previous step's x0, same layout as x; read, then overwritten by this step's
};
// final Block: silu(gn(x)) -> conv3x3 C->Cout(<=4), NHWC in, NCHW out (out_nchw may be null when `fuse` is given)
int conv_out_nchw(const float* x, const float* ss, int B, int H, int W, int C, const float* w,
                  const float* bias, int Cout, float* out_nchw, hipStream_t st, const StepFuse* fuse = nullptr);
// noise-level / timestep embedding + MLP + all FiLM projections
struct EmbedParams {
  int variant;            // 0 sr3 (continuous level), 1 ddpm (integer t)
  int B, inner;           // embedding dim = inner, hidden = 4*inner
  const float* level;     // [B] (sr3) or null
  const int64_t* tstep;   // [B] (ddpm) or null
  const float* level_table;  // sr3: level = level_table[step_dev[0] + 1] when step_dev != null
  const int* step_dev;    // device step counter (graph replay) or null
  const int* t_map;       // ddpm, with step_dev: timestep = t_map[step_dev[0]] (a strided walk through the schedule); null: the counter itself
  int* step_out;          // optional: block 0 copies *step_dev here (sr3_reverse_step: the slot the step's tail kernel reads)
  const float* freq;      // [inner/2] frequency table
  const float* w1; const float* b1;   // [4*inner][inner], [4*inner]
  const float* w2; const float* b2;   // [inner][4*inner], [inner]
  const float* wf; const float* bf;   // concatenated FiLM projections [F][inner], [F]
  int F;
  float* temb;            // [B][inner] scratch
  float* film;            // [B][F]
};
int embed_forward(const EmbedParams& p, hipStream_t st);
// single-head attention over NHWC qkv [B][N][3C] -> out [B][N][C]
// mode bit 0: the staging-free kernel's 3 x bf16 split instantiation where the shape takes that kernel (fp32 MFMA otherwise);
// mode bit 1: the key-blocked kernel of attention_long.hip (any N; also where the score strip would fit)
int attention_forward(const float* qkv, int B, int N, int C, float* out, hipStream_t st, int mode = 0);
// host predicate: can the strip kernels of attention_forward (mode bit 1 clear) run N tokens of C channels?  (They keep a 32-query
// score strip over all N keys in LDS.)
bool attention_fits(int N, int C);
// key-blocked (online softmax) form: any N > 0, C % 4 == 0 (attention_long.hip); split: 3 x bf16 split arithmetic where C % 128 == 0
// heads > 1: C is ONE head's width here (the rows hold heads * C channels; the multi-head layout below)
int attention_long_forward(const float* qkv, int B, int N, int C, float* out, hipStream_t st, bool split, int heads = 1);
// multi-head attention (the reference SelfAttention's n_head; attention_heads.hip): H = heads heads of d = C / heads channels over the
// same tensors -- head h owns channels [3 d h, 3 d (h + 1)) of a qkv row as q | k | v and [d h, d (h + 1)) of an out row, its scores
// are Q_h K_h^T / sqrt(C) (the FULL C) with a softmax of their own.  heads == 1 is attention_forward (same launches).  mode bits 0
// and 1 as there; bit 2 keeps 64- and 32-channel heads off k_attention_heads (the generalised kernels instead: a measurement knob).
// Needs heads >= 1, C % heads == 0, d % 4 == 0.
int attention_forward_heads(const float* qkv, int B, int N, int C, int heads, float* out, hipStream_t st, int mode = 0);
// ... its fall-back onto the MH instantiations of the single-head kernels (attention.hip, attention_long.hip), heads > 1
int attention_forward_strided(const float* qkv, int B, int N, int C, int heads, float* out, hipStream_t st, int mode);
// host check both head entries share: SR3_OK, or the refusal with its message
int attention_heads_check(const char* who, int C, int heads);
int p_sample_update(float* x, const float* eps, const float* z, StepTables tb, const int* step_dev,
                    const int64_t* t_per_sample, int step_host, int B, int per_image, hipStream_t st, bool clip = true,
                    const float* c3 = nullptr, float* hist = nullptr);
int step_decrement(int* step_dev, hipStream_t st);
// step2[0] <- step2[1] (tiled.hip): the first launch of a step whose tail is a kernel of its own (sr3_tiled_step, sr3_consistent_step)
int step_copy(int* step2, hipStream_t st);
// split3_pair self-test (small_kernels.hip): *bad_dev = number of elements whose three bf16 terms do not add back exactly
int split3_selftest(int* bad_dev, hipStream_t st);
// q_sample (sr3: per-sample gamma; ddpm: a[t], s[t]) -> x_noisy ; l1 loss sum
int q_sample(const float* x0, const float* z, const float* ca, const float* cb, int B, int per_image,
             float* out, hipStream_t st);

}  // namespace sr3
