// Zero-shot restoration (include/sr3_mi355x.h: sr3_restore_step, sr3_travel_back_f32, sr3_gray_f32): the range / null-space projection
// of DDNM (Wang et al. 2022) for two operators a trained diffusion model is asked for first -- a pixel mask (inpainting, outpainting,
// RePaint's known region) and a channel sum (colourisation) -- in the x0 slot of a reverse step's tail, and the forward jump of the
// resampled walk (RePaint's "jumps", DDNM's "time travel") that moves the chain -- and the device counter -- UP.
//
// The arithmetic (lambda = strength in (0, 1], j = step2_dev[1] on entry; every product, sum and difference rounded on its own, in
// exactly this order, so that a NumPy float32 restatement gives the same bits):
//
//   x0  = a[j] x - b[j] eps ; clamp(-1, 1) if clip_denoised        step_x0 of sr3_common.h; clamp first, then project
//   mask (op 0):  w   = lambda * m                                  m = mask[b, c or 0, y, x] in [0, 1], 1 = known
//                 x0' = (w * y) + ((1 - w) * x0)                    the lerp form: w = 1 gives y exactly, w = 0 gives x0 exactly
//   gray (op 1):  g   = ((a0 x0_0 + a1 x0_1) + a2 x0_2) + a3 x0_3   channel order, C <= 4
//                 r   = y - g                                       y = target[b, 0, y, x]
//                 x0'_c = x0_c + ((lambda * p[c]) * r)              p = a / sum a^2, the pseudo-inverse, made by the host
//   x   = ((c1[j] x0' + c2[j] x) + c3[j] hist) + sigma[j] z ;  hist <- x0'      step_mix of sr3_common.h
//   step2_dev[1] = j - 1 on completion (step2_dev[0] is scratch, as in sr3_consistent_step)
//
//   travel:       r = step2_dev[1] + 1 ;  x = (ra[r] * x) + (rs[r] * z) ;  step2_dev[1] = to[r]
//
// Work split: a thread owns V consecutive columns (V = 4 as one 16-byte access where W % 4 == 0 and every pointer is 16-byte aligned,
// step_tail.h's vec16; V = 1 otherwise) of ALL C planes of one image: lanes run along a plane, so every plane is read as contiguous
// segments by consecutive lanes, the channel sum of the gray operator needs no shuffle and no second pass, and a one-plane mask is read
// once for the C channels it covers.  One thread per item, no grid-stride loop: there are fewer than 2^31 items.
#include <cmath>

#include "step_tail.h"

namespace sr3 {
namespace {

constexpr int GRAY_MAX_C = 4;
struct GrayW { float a[GRAY_MAX_C], p[GRAY_MAX_C]; };      // by value: C <= 4 (p unused by sr3_gray_f32)

// item i -> image b and the first of its V pixels q (in a plane of hw pixels); element (b, c, q) sits at (b * C + c) * hw + q
template <int V>
__device__ __forceinline__ size_t pixel_of(size_t i, size_t hw, size_t& b) {
  const size_t per = hw / V;
  b = i / per;
  return (i % per) * V;
}

// g = ((a0 v0 + a1 v1) + a2 v2) + a3 v3, channel order
template <int C>
__device__ __forceinline__ float gray_of(const GrayW& w, const float (&v)[C]) {
  float g = mul_rn(w.a[0], v[0]);
#pragma unroll
  for (int c = 1; c < C; ++c) g = add_rn(g, mul_rn(w.a[c], v[c]));
  return g;
}

struct RestoreStep {
  StepFuse f;                // the step's tail on x [B, C, H, W]; step_cur: step_copy put j there
  const float* eps;          // [B, C, H, W]
  const float* y;            // mask: known [B, C, H, W]; gray: target [B, 1, H, W]
  const float* mask;         // mask: [B, Mc, H, W]; gray: null
  int C, Mc;
  size_t hw;                 // H * W
  float strength;
  GrayW w;
  size_t total;              // items = B * H * W / V
};

template <bool CLIP, bool HIST, int V>
__global__ __launch_bounds__(256) void k_restore_mask(RestoreStep s) {
  const StepFuse& f = s.f;
  const StepCoef cf = tail_begin<HIST>(f, blockIdx.x == 0 && threadIdx.x == 0);
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= s.total) return;
  size_t b;
  const size_t q = pixel_of<V>(i, s.hw, b);
  float wv[V];
  if (s.Mc == 1) {
    load_v<V>(s.mask + b * s.hw + q, wv);
#pragma unroll
    for (int k = 0; k < V; ++k) wv[k] = mul_rn(s.strength, wv[k]);
  }
  for (int c = 0; c < s.C; ++c) {
    const size_t e = (b * s.C + c) * s.hw + q;
    float xv[V], ev[V], zv[V], hv[V], yv[V], x0[V];
    if (s.Mc != 1) {
      load_v<V>(s.mask + e, wv);
#pragma unroll
      for (int k = 0; k < V; ++k) wv[k] = mul_rn(s.strength, wv[k]);
    }
    load_v<V>(s.eps + e, ev);
    load_v<V>(s.y + e, yv);
    tail_load<HIST, V>(f, e, xv, zv, hv);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float v = step_x0(cf, CLIP, xv[k], ev[k]);
      x0[k] = add_rn(mul_rn(wv[k], yv[k]), mul_rn(sub_rn(1.f, wv[k]), v));
    }
    tail_mix_store<HIST, V>(f, cf, e, x0, xv, zv, hv);
  }
}

template <bool CLIP, bool HIST, int V, int C>
__global__ __launch_bounds__(256) void k_restore_gray(RestoreStep s) {
  const StepFuse& f = s.f;
  const StepCoef cf = tail_begin<HIST>(f, blockIdx.x == 0 && threadIdx.x == 0);
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= s.total) return;
  size_t b;
  const size_t q = pixel_of<V>(i, s.hw, b);
  const size_t e0 = b * C * s.hw + q;
  float xv[C][V], zv[C][V], hv[C][V], x0[C][V], yv[V];
  load_v<V>(s.y + b * s.hw + q, yv);
#pragma unroll
  for (int c = 0; c < C; ++c) {
    float ev[V];
    load_v<V>(s.eps + e0 + c * s.hw, ev);
    tail_load<HIST, V>(f, e0 + c * s.hw, xv[c], zv[c], hv[c]);
#pragma unroll
    for (int k = 0; k < V; ++k) x0[c][k] = step_x0(cf, CLIP, xv[c][k], ev[k]);
  }
  float lp[C];
#pragma unroll
  for (int c = 0; c < C; ++c) lp[c] = mul_rn(s.strength, s.w.p[c]);
#pragma unroll
  for (int k = 0; k < V; ++k) {
    float v[C];
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = x0[c][k];
    const float r = sub_rn(yv[k], gray_of<C>(s.w, v));
#pragma unroll
    for (int c = 0; c < C; ++c) x0[c][k] = add_rn(v[c], mul_rn(lp[c], r));
  }
#pragma unroll
  for (int c = 0; c < C; ++c) tail_mix_store<HIST, V>(f, cf, e0 + c * s.hw, x0[c], xv[c], zv[c], hv[c]);
}

// dst[b, 0, q] = gray of src[b, :, q]
template <int V, int C>
__global__ __launch_bounds__(256) void k_gray(const float* __restrict__ src, float* __restrict__ dst, GrayW w, size_t hw, size_t total) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  size_t b;
  const size_t q = pixel_of<V>(i, hw, b);
  float sv[C][V], g[V];
#pragma unroll
  for (int c = 0; c < C; ++c) load_v<V>(src + (b * C + c) * hw + q, sv[c]);
#pragma unroll
  for (int k = 0; k < V; ++k) {
    float v[C];
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = sv[c][k];
    g[k] = gray_of<C>(w, v);
  }
  store_v<V>(dst + b * hw + q, g);
}

// x <- ra[r] x + rs[r] z at row r = step2[0] + 1 (step_copy put the counter there); one thread moves the counter to to[r].  A counter
// outside [-1, rows - 2] touches nothing: no table can take the kernel outside its tensors
template <int V>
__global__ __launch_bounds__(256) void k_travel_back(float* __restrict__ x, const float* __restrict__ z, const float* __restrict__ ra,
                                                      const float* __restrict__ rs, const int* __restrict__ to, int rows, int* step2,
                                                      size_t total) {
  const int r = step2[0] + 1;
  if (r < 0 || r >= rows) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) step2[1] = to[r];
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const float a = ra[r], s = rs[r];
  float xv[V], zv[V];
  load_v<V>(x + i * V, xv);
  load_v<V>(z + i * V, zv);
#pragma unroll
  for (int k = 0; k < V; ++k) xv[k] = add_rn(mul_rn(a, xv[k]), mul_rn(s, zv[k]));
  store_v<V>(x + i * V, xv);
}

// runtime C in 1..4 -> the template argument
template <class F>
void dispatch_channels(int C, F&& f) {
  switch (C) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 4>{}); break;
  }
}

int check_gray_channels(const char* who, int channels) {
  if (channels > GRAY_MAX_C) {
    set_error("%s: the gray operator takes at most %d channels: its weights travel by value (got %d)", who, GRAY_MAX_C, channels);
    return SR3_E_BADARG;
  }
  return SR3_OK;
}

// the host's weight arrays into the kernel argument; every weight finite
int load_gray_weights(const char* who, const float* a, const float* p, int channels, GrayW* w) {
  *w = GrayW{};
  for (int c = 0; c < channels; ++c) {
    w->a[c] = a[c];
    w->p[c] = p ? p[c] : 0.f;
    if (!std::isfinite(w->a[c]) || !std::isfinite(w->p[c])) { set_error("%s: gray weight %d is not finite", who, c); return SR3_E_BADARG; }
  }
  return SR3_OK;
}

}  // namespace
}  // namespace sr3

using namespace sr3;

extern "C" {

int sr3_gray_f32(const float* src_nchw, int batch, int channels, int height, int width, const float* gray_a_host, float* dst_nchw,
                 void* stream) {
  const char* who = "gray";
  const Req req[] = {{src_nchw, "src_nchw"}, {gray_a_host, "gray_a_host"}, {dst_nchw, "dst_nchw"}};
  if (const int rc = check_required(who, req)) return rc;
  if (const int rc = check_image_dims(who, batch, channels, height, width)) return rc;
  if (const int rc = check_gray_channels(who, channels)) return rc;
  const size_t hw = (size_t)height * width, total = (size_t)batch * channels * hw;
  if (const int rc = check_image_limit(who, total)) return rc;
  const Buf bufs[] = {{dst_nchw, (size_t)batch * hw * sizeof(float), "dst_nchw", true}, {src_nchw, total * sizeof(float), "src_nchw", false}};
  if (const int rc = check_overlaps(who, bufs)) return rc;
  GrayW w;
  if (const int rc = load_gray_weights(who, gray_a_host, nullptr, channels, &w)) return rc;
  const bool vec = (width & 3) == 0 && vec16(src_nchw, dst_nchw);
  const size_t items = (size_t)batch * hw / (vec ? 4 : 1);
  const dim3 grid((unsigned)((items + 255) / 256));
  hipStream_t st = static_cast<hipStream_t>(stream);
  dispatch_channels(channels, [&](auto c) {
    dispatch_bools([&](auto v4) {
      hipLaunchKernelGGL((k_gray<v4() ? 4 : 1, c()>), grid, dim3(256), 0, st, src_nchw, dst_nchw, w, hw, items);
    }, vec);
  });
  SR3_LAUNCH_CHECK("k_gray");
  return SR3_OK;
}

int sr3_restore_step(float* x_nchw, const float* eps_nchw, const float* z_nchw, int op, const float* target, const float* mask,
                     int mask_channels, const float* gray_a_host, const float* gray_p_host, int batch, int channels, int height,
                     int width, float strength, const float* tab_a, const float* tab_b, const float* tab_c1, const float* tab_c2,
                     const float* tab_sigma, int* step2_dev, int clip_denoised, const float* tab_c3, float* hist_nchw, void* stream) {
  const char* who = "restore_step";
  const Req req[] = {{x_nchw, "x_nchw"}, {eps_nchw, "eps_nchw"}, {target, "target"}, {tab_a, "tab_a"}, {tab_b, "tab_b"},
      {tab_c1, "tab_c1"}, {tab_c2, "tab_c2"}, {tab_sigma, "tab_sigma"}, {step2_dev, "step2_dev"}};
  if (const int rc = check_required(who, req)) return rc;
  if (op != 0 && op != 1) { set_error("%s: op must be 0 (mask) or 1 (gray) (got %d)", who, op); return SR3_E_BADARG; }
  if (op == 0) {
    const Req rq[] = {{mask, "mask"}};
    if (const int rc = check_required(who, rq)) return rc;
  } else {
    const Req rq[] = {{gray_a_host, "gray_a_host"}, {gray_p_host, "gray_p_host"}};
    if (const int rc = check_required(who, rq)) return rc;
  }
  if (const int rc = check_image_dims(who, batch, channels, height, width)) return rc;
  if (op == 0 && mask_channels != 1 && mask_channels != channels) {
    set_error("%s: mask_channels must be 1 or channels = %d (got %d)", who, channels, mask_channels);
    return SR3_E_BADARG;
  }
  if (op == 1) {
    if (const int rc = check_gray_channels(who, channels)) return rc;
  }
  const size_t hw = (size_t)height * width, total = (size_t)batch * channels * hw;
  if (const int rc = check_image_limit(who, total)) return rc;
  if (!(strength > 0.f && strength <= 1.f)) { set_error("%s: strength must lie in (0, 1] (got %g)", who, (double)strength); return SR3_E_BADARG; }
  const size_t fl = sizeof(float), bytes = total * fl, plane = (size_t)batch * hw * fl;
  if (const int rc = check_step_history(who, tab_c3, hist_nchw, x_nchw, eps_nchw, bytes)) return rc;
  if (op == 1) mask = nullptr;      // (the gray operator reads none: it takes no part below)
  // what the call writes (x, hist, the counter) against everything else it is given
  const Buf bufs[] = {{x_nchw, bytes, "x_nchw", true}, {eps_nchw, bytes, "eps_nchw", false}, {z_nchw, bytes, "z_nchw", false},
      {target, op == 0 ? bytes : plane, "target", false}, {mask, mask_channels == 1 ? plane : bytes, "mask", false},
      {hist_nchw, bytes, "hist_nchw", true}, {step2_dev, 2 * sizeof(int), "step2_dev", true},
      {tab_a, fl, "tab_a", false}, {tab_b, fl, "tab_b", false}, {tab_c1, fl, "tab_c1", false}, {tab_c2, fl, "tab_c2", false},
      {tab_sigma, fl, "tab_sigma", false}, {tab_c3, fl, "tab_c3", false}};
  if (const int rc = check_overlaps(who, bufs)) return rc;
  RestoreStep s;
  s.w = GrayW{};
  if (op == 1) {
    if (const int rc = load_gray_weights(who, gray_a_host, gray_p_host, channels, &s.w)) return rc;
  }
  const bool vec = (width & 3) == 0 && vec16(x_nchw, eps_nchw, z_nchw, hist_nchw, target, mask);
  s.f = StepFuse{x_nchw, z_nchw, StepTables{tab_a, tab_b, tab_c1, tab_c2, tab_sigma}, step2_dev, step2_dev + 1, clip_denoised, tab_c3, hist_nchw};
  s.eps = eps_nchw; s.y = target; s.mask = mask; s.C = channels; s.Mc = mask_channels; s.hw = hw; s.strength = strength;
  s.total = (size_t)batch * hw / (vec ? 4 : 1);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (const int rc = step_copy(step2_dev, st)) return rc;
  const dim3 grid((unsigned)((s.total + 255) / 256));
  if (op == 0) {
    dispatch_bools([&](auto clip, auto hist, auto v4) {
      hipLaunchKernelGGL((k_restore_mask<clip(), hist(), v4() ? 4 : 1>), grid, dim3(256), 0, st, s);
    }, clip_denoised != 0, hist_nchw != nullptr, vec);
    SR3_LAUNCH_CHECK("k_restore_mask");
  } else {
    dispatch_channels(channels, [&](auto c) {
      dispatch_bools([&](auto clip, auto hist, auto v4) {
        hipLaunchKernelGGL((k_restore_gray<clip(), hist(), v4() ? 4 : 1, c()>), grid, dim3(256), 0, st, s);
      }, clip_denoised != 0, hist_nchw != nullptr, vec);
    });
    SR3_LAUNCH_CHECK("k_restore_gray");
  }
  return SR3_OK;
}

int sr3_travel_back_f32(float* x, const float* z, const float* tab_ra, const float* tab_rs, const int* tab_to, int rows, int* step2_dev,
                        int batch, int elems_per_image, void* stream) {
  const char* who = "travel_back";
  const Req req[] = {{x, "x"}, {z, "z"}, {tab_ra, "tab_ra"}, {tab_rs, "tab_rs"}, {tab_to, "tab_to"}, {step2_dev, "step2_dev"}};
  if (const int rc = check_required(who, req)) return rc;
  if (rows <= 0 || batch <= 0 || elems_per_image <= 0) {
    set_error("%s: rows, batch and elems_per_image must be positive (got %d, %d, %d)", who, rows, batch, elems_per_image);
    return SR3_E_BADARG;
  }
  const size_t total = (size_t)batch * elems_per_image;
  if (const int rc = check_image_limit(who, total)) return rc;
  const size_t fl = sizeof(float), bytes = total * fl;
  const Buf bufs[] = {{x, bytes, "x", true}, {z, bytes, "z", false}, {step2_dev, 2 * sizeof(int), "step2_dev", true},
      {tab_ra, rows * fl, "tab_ra", false}, {tab_rs, rows * fl, "tab_rs", false}, {tab_to, rows * sizeof(int), "tab_to", false}};
  if (const int rc = check_overlaps(who, bufs)) return rc;
  const bool vec = (elems_per_image & 3) == 0 && vec16(x, z);
  const size_t items = vec ? total / 4 : total;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (const int rc = step_copy(step2_dev, st)) return rc;
  const dim3 grid((unsigned)((items + 255) / 256));
  dispatch_bools([&](auto v4) {
    hipLaunchKernelGGL((k_travel_back<v4() ? 4 : 1>), grid, dim3(256), 0, st, x, z, tab_ra, tab_rs, tab_to, rows, step2_dev, items);
  }, vec);
  SR3_LAUNCH_CHECK("k_travel_back");
  return SR3_OK;
}

}  // extern "C"
