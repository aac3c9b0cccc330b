// Self-conditioning (include/sr3_mi355x.h: sr3_selfcond_x0_f32): the network's own estimate of x0 written into channels of its
// conditioning tensor (Chen et al. 2022, "Analog Bits", section 3.2).  Sampling feeds every step the previous step's estimate; training
// makes the estimate with a first, gradient-free pass for a random part of the batch and trains on it as on any other input.
//
// The arithmetic (step_x0 of sr3_common.h and nothing else, so the x0 written here is bit for bit the x0 a step tail computes):
//
//   row = step_dev ? step_dev[0] : b                         the sampling form reads the device counter, the training form is per image
//   x0  = a[row] x - b[row] out                              mul_rn, mul_rn, sub_rn
//   x0  = clamp(x0, -1, 1)   if clip
//   dst[b][dst_first_channel + c] = keep[b] ? x0 : +0.0      c < channels; keep NULL: every image kept; the other channels untouched
//
// A dropped image's x and out are not read: its channels are +0.0 whatever they hold (a NaN included).
//
// Work split: a thread owns V consecutive elements of one (b, c) plane (V = 4 as one 16-byte access where width % 4 == 0 and x, out
// and dst are 16-byte aligned, step_tail.h's vec16 -- the planes' offsets in dst are then multiples of four floats too; V = 1
// otherwise).  One thread per item, no grid-stride loop: there are fewer than 2^31 items.  Plain vector stores, no atomics.
#include "step_tail.h"

namespace sr3 {
namespace {

struct SelfCond {
  const float* x;            // [B, C, H, W]
  const float* out;          // [B, C, H, W] the network's output, whatever it predicts (a, b say what it stands for)
  const float* a;
  const float* b;
  const int* step;           // the device counter, or null: row = image
  const int* keep;           // [B] or null
  float* dst;                // [B, dst_channels, H, W]
  unsigned per_src;          // C * H * W
  unsigned per_dst;          // dst_channels * H * W
  unsigned first;            // dst_first_channel * H * W
  size_t total;              // items = B * C * H * W / V
};

template <bool CLIP, int V>
__global__ __launch_bounds__(256) void k_selfcond_x0(SelfCond s) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= s.total) return;
  const size_t e = i * V;
  const unsigned b = (unsigned)(e / s.per_src);
  const unsigned rem = (unsigned)(e - (size_t)b * s.per_src);      // (per_src % V == 0: the V elements lie in one image)
  float r[V];
#pragma unroll
  for (int k = 0; k < V; ++k) r[k] = 0.f;
  if (!s.keep || s.keep[b] != 0) {
    const int row = s.step ? s.step[0] : (int)b;
    const StepCoef cf{s.a[row], s.b[row], 0.f, 0.f, 0.f, 0.f};
    float xv[V], ov[V];
    load_v<V>(s.x + e, xv);
    load_v<V>(s.out + e, ov);
#pragma unroll
    for (int k = 0; k < V; ++k) r[k] = step_x0(cf, CLIP, xv[k], ov[k]);
  }
  store_v<V>(s.dst + (size_t)b * s.per_dst + s.first + rem, r);
}

}  // namespace
}  // namespace sr3

using namespace sr3;

extern "C" int sr3_selfcond_x0_f32(const float* x_nchw, const float* out_nchw, const float* tab_a, const float* tab_b, const int* step_dev,
                                   const int* keep_dev, int clip, int batch, int channels, int height, int width, float* dst_nchw,
                                   int dst_channels, int dst_first_channel, void* stream) {
  const char* who = "selfcond_x0";
  const Req req[] = {{x_nchw, "x_nchw"}, {out_nchw, "out_nchw"}, {tab_a, "tab_a"}, {tab_b, "tab_b"}, {dst_nchw, "dst_nchw"}};
  if (const int rc = check_required(who, req)) return rc;
  if (const int rc = check_image_dims(who, batch, channels, height, width)) return rc;
  if (dst_channels <= 0) { set_error("%s: dst_channels must be positive (got %d)", who, dst_channels); return SR3_E_BADARG; }
  if (dst_first_channel < 0) { set_error("%s: dst_first_channel must not be negative (got %d)", who, dst_first_channel); return SR3_E_BADARG; }
  if ((long)dst_first_channel + channels > dst_channels) {
    set_error("%s: dst_first_channel %d + channels %d exceeds dst_channels %d", who, dst_first_channel, channels, dst_channels);
    return SR3_E_BADARG;
  }
  const size_t HW = (size_t)height * width;
  const size_t total = (size_t)batch * channels * HW, dst_total = (size_t)batch * dst_channels * HW;
  if (const int rc = check_image_limit(who, dst_total)) return rc;      // (dst_channels >= channels: this bounds x and out too)
  // a table is `batch` rows in the per-image form; in the step-index form its length is the caller's, and one row stands for it
  const size_t tab_bytes = (step_dev ? 1 : (size_t)batch) * sizeof(float);
  const Buf bufs[] = {{dst_nchw, dst_total * sizeof(float), "dst_nchw", true}, {x_nchw, total * sizeof(float), "x_nchw", false},
      {out_nchw, total * sizeof(float), "out_nchw", false}, {tab_a, tab_bytes, "tab_a", false}, {tab_b, tab_bytes, "tab_b", false},
      {step_dev, sizeof(int), "step_dev", false}, {keep_dev, (size_t)batch * sizeof(int), "keep_dev", false}};
  if (const int rc = check_overlaps(who, bufs)) return rc;
  const bool vec = (width & 3) == 0 && vec16(x_nchw, out_nchw, dst_nchw);
  SelfCond s{x_nchw, out_nchw, tab_a, tab_b, step_dev, keep_dev, dst_nchw, (unsigned)(channels * HW), (unsigned)(dst_channels * HW),
             (unsigned)(dst_first_channel * HW), vec ? total / 4 : total};
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((s.total + 255) / 256));
  dispatch_bools([&](auto c, auto v4) {
    hipLaunchKernelGGL((k_selfcond_x0<c(), v4() ? 4 : 1>), grid, dim3(256), 0, st, s);
  }, clip != 0, vec);
  SR3_LAUNCH_CHECK("k_selfcond_x0");
  return SR3_OK;
}
