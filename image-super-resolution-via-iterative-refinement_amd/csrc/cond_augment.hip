// Noise conditioning augmentation (include/sr3_mi355x.h: sr3_cond_augment_f32): the conditioning image of a super-resolver diffused to a
// level of its own before the network reads it (Ho et al. 2021, "Cascaded Diffusion Models", section 4.2; Sahak et al. 2023, SR3+).
// Training draws the level per image, sampling applies one small fixed level; the network may be told the level as one extra input plane.
//
// The arithmetic, per image b (s = the standard deviation of the added noise, a = sqrt(1 - s^2), both from the host, fp32):
//
//   aug = s[b] == 0 ? src : a[b] src + s[b] eps                      mul_rn, mul_rn, add_rn; eps null: aug = src, and a is not read
//   dst[b][first + c]        = keep[b] ? aug  : +0.0                 c < channels
//   dst[b][first + channels] = keep[b] ? s[b] : +0.0                 with level_channel only
//
// keep null: every image kept.  Every other channel of dst is left untouched.  A dropped image's src and eps are not read: its planes
// are +0.0 whatever they hold (a NaN included) -- the level plane too, so a dropped image is the all-zero conditioning tensor a guided
// step's second forward reads.  An image at level 0 is a bit copy of src (a -0.0 included) and its eps is not read.
//
// Work split: a thread owns V consecutive elements of one written (b, c) plane (V = 4 as one 16-byte access where height * width % 4
// == 0 and src, eps and dst are 16-byte aligned, step_tail.h's vec16 -- every plane's offset is then a multiple of four floats too;
// V = 1 otherwise).  One thread per item, no grid-stride loop: there are fewer than 2^31 items.  Plain vector stores, no atomics.
#include "step_tail.h"

namespace sr3 {
namespace {

struct CondAug {
  const float* src;          // [B, C, H, W]
  const float* eps;          // [B, C, H, W] or null: nothing is added
  const float* a;            // [B] (not read where eps is null)
  const float* s;            // [B]
  const int* keep;           // [B] or null
  float* dst;                // [B, dst_channels, H, W]
  unsigned hw;               // H * W
  unsigned per_src;          // C * H * W
  unsigned per_out;          // (C + level_channel) * H * W: what is written of one image
  unsigned per_dst;          // dst_channels * H * W
  unsigned first;            // dst_first_channel * H * W
  size_t total;              // items = B * per_out / V
};

template <int V>
__global__ __launch_bounds__(256) void k_cond_augment(CondAug q) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= q.total) return;
  const size_t e = i * V;
  const unsigned b = (unsigned)(e / q.per_out);
  const unsigned rem = (unsigned)(e - (size_t)b * q.per_out);      // (hw % V == 0: the V elements lie in one plane)
  float r[V];
#pragma unroll
  for (int k = 0; k < V; ++k) r[k] = 0.f;
  if (!q.keep || q.keep[b] != 0) {
    const float s = q.s[b];
    if (rem >= q.per_src) {                    // the level plane
#pragma unroll
      for (int k = 0; k < V; ++k) r[k] = s;
    } else {
      const size_t at = (size_t)b * q.per_src + rem;
      load_v<V>(q.src + at, r);
      if (q.eps && s != 0.f) {
        const float a = q.a[b];
        float ev[V];
        load_v<V>(q.eps + at, ev);
#pragma unroll
        for (int k = 0; k < V; ++k) r[k] = add_rn(mul_rn(a, r[k]), mul_rn(s, ev[k]));
      }
    }
  }
  store_v<V>(q.dst + (size_t)b * q.per_dst + q.first + rem, r);
}

}  // namespace
}  // namespace sr3

using namespace sr3;

extern "C" int sr3_cond_augment_f32(const float* src_nchw, const float* eps_nchw, const float* a_dev, const float* s_dev, const int* keep_dev,
                                    int level_channel, float* dst_nchw, int dst_channels, int dst_first_channel, int batch, int channels,
                                    int height, int width, void* stream) {
  const char* who = "cond_augment";
  const Req req[] = {{src_nchw, "src_nchw"}, {s_dev, "s_dev"}, {dst_nchw, "dst_nchw"}};
  if (const int rc = check_required(who, req)) return rc;
  if (eps_nchw && !a_dev) { set_error("%s: a_dev is NULL (only the form without eps_nchw reads no a)", who); return SR3_E_BADARG; }
  if (const int rc = check_image_dims(who, batch, channels, height, width)) return rc;
  if (dst_channels <= 0) { set_error("%s: dst_channels must be positive (got %d)", who, dst_channels); return SR3_E_BADARG; }
  if (dst_first_channel < 0) { set_error("%s: dst_first_channel must not be negative (got %d)", who, dst_first_channel); return SR3_E_BADARG; }
  const int written = channels + (level_channel ? 1 : 0);
  if ((long)dst_first_channel + written > dst_channels) {
    set_error("%s: dst_first_channel %d + channels %d%s exceeds dst_channels %d", who, dst_first_channel, channels,
              level_channel ? " + the level channel" : "", dst_channels);
    return SR3_E_BADARG;
  }
  const size_t HW = (size_t)height * width;
  const size_t total = (size_t)batch * channels * HW, dst_total = (size_t)batch * dst_channels * HW;
  if (const int rc = check_image_limit(who, dst_total)) return rc;      // (dst_channels >= channels: this bounds src and eps too)
  const size_t per_image = (size_t)batch * sizeof(float);
  const Buf bufs[] = {{dst_nchw, dst_total * sizeof(float), "dst_nchw", true}, {src_nchw, total * sizeof(float), "src_nchw", false},
      {eps_nchw, total * sizeof(float), "eps_nchw", false}, {a_dev, per_image, "a_dev", false}, {s_dev, per_image, "s_dev", false},
      {keep_dev, (size_t)batch * sizeof(int), "keep_dev", false}};
  if (const int rc = check_overlaps(who, bufs)) return rc;
  const bool vec = (HW & 3) == 0 && vec16(src_nchw, eps_nchw, dst_nchw);
  const size_t out_total = (size_t)batch * written * HW;
  CondAug q{src_nchw, eps_nchw, a_dev, s_dev, keep_dev, dst_nchw, (unsigned)HW, (unsigned)(channels * HW), (unsigned)(written * HW),
            (unsigned)(dst_channels * HW), (unsigned)(dst_first_channel * HW), vec ? out_total / 4 : out_total};
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((q.total + 255) / 256));
  dispatch_bools([&](auto v4) {
    hipLaunchKernelGGL((k_cond_augment<v4() ? 4 : 1>), grid, dim3(256), 0, st, q);
  }, vec);
  SR3_LAUNCH_CHECK("k_cond_augment");
  return SR3_OK;
}
