// The prologue of a conv input, defined once: what every kernel that reads a conv input does to a channel quad (four consecutive
// channels, one f32x4) before it reaches LDS, in this order:
//   concat_quad   pick the source of the virtual concat
//   gn_affine4    x * scale + shift, the folded GroupNorm pair (ConvParams::act >= 1)
//   silu4_*       SiLU (ConvParams::act == 2)
//   drop_mask     the train-mode dropout mask, at drop_index
//   (the kernel)  zero padding, AFTER the activation, as the reference does
// The forward convs, the weight gradient and the training backward (which recomputes what the forward applied) stage through these.
#pragma once
#include "sr3_common.h"

namespace sr3 {

// channel quad `ce` of the virtual concat s0 (C0 channels) | s1 (C1): its source, that source's channel count, the channel inside it
template <typename T>
struct ConcatQuad { T* base; int C, c; bool second; };
template <typename T>
__device__ __forceinline__ ConcatQuad<T> concat_quad(T* s0, int C0, T* s1, int C1, int ce) {
  const bool second = ce >= C0;
  return ConcatQuad<T>{second ? s1 : s0, second ? C1 : C0, second ? ce - C0 : ce, second};
}

// ssa | ssb: the quad's four (scale, shift) pairs as they lie in ConvParams::ss, interleaved
__device__ __forceinline__ f32x4 gn_affine4(f32x4 v, const f32x4 ssa, const f32x4 ssb) {
  v.x = fmaf(v.x, ssa.x, ssa.y);
  v.y = fmaf(v.y, ssa.z, ssa.w);
  v.z = fmaf(v.z, ssb.x, ssb.y);
  v.w = fmaf(v.w, ssb.z, ssb.w);
  return v;
}

// x * sigmoid(x); exp is the accurate libm one, the reciprocal is v_rcp_f32 (1 ulp): SR3_SILU
__device__ __forceinline__ float silu_libm(float v) { return SR3_SILU(v); }
// x * sigmoid(x) with the hardware exp2 (v_exp_f32 on x * log2 e) and the hardware reciprocal: ~1e-7 relative error on silu,
// three instructions instead of libm expf's twelve -- every element the Winograd kernels stage pays for this once per output-channel
// block.  The other kernels use silu_libm; the difference is below what the parity tests resolve.
__device__ __forceinline__ float silu_exp2(float v) {
#ifdef SR3_EXACT_ACT
  return SR3_SILU(v);
#else
  return v * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(v * -1.44269504088896341f));
#endif
}
__device__ __forceinline__ f32x4 silu4_libm(f32x4 v) { v.x = silu_libm(v.x); v.y = silu_libm(v.y); v.z = silu_libm(v.z); v.w = silu_libm(v.w); return v; }
__device__ __forceinline__ f32x4 silu4_exp2(f32x4 v) { v.x = silu_exp2(v.x); v.y = silu_exp2(v.y); v.z = silu_exp2(v.z); v.w = silu_exp2(v.w); return v; }

// Dropout (ConvParams::drop_*): the mask index of an activated element is its NHWC linear index -- pixel `pix` of a C-channel tensor,
// channel c + e (e: the lane of the quad that starts at channel c).  Only defined for single-source, non-upsampled inputs (block2's
// input is never a concat).  An element is kept iff drop_mask(seed, index, thresh, scale) != 0 and multiplied by it; the training backward
// recomputes the forward's mask from this index.  P: the caller's pixel type (int in the convs, size_t in the training kernels).
// (The four multiplies of a quad stay at the call sites: behind a function the compiler schedules the staging loops differently.)
template <typename P>
__device__ __forceinline__ unsigned drop_index(P pix, int C, int c, int e = 0) { return (unsigned)(pix * C + c + e); }

}  // namespace sr3
