// LR-consistent sampling (include/sr3_mi355x.h: sr3_block_mean_f32, sr3_consistent_step): the range / null-space projection of DDNM
// (Wang et al. 2022) for the r x r average pool, inside the tail of a reverse step.  Every step replaces the part of the predicted x0
// that the pool can see -- the mean of each r x r block -- by the target's, and keeps the rest from the network.
//
// The arithmetic (r = block, lambda = strength in (0, 1], y[b, c, by, bx] = the target block means, j = step2_dev[1] on entry):
//
//   x0  = a[j] x - b[j] eps                                  step_x0 of sr3_common.h: mul_rn, mul_rn, sub_rn
//   x0  = clamp(x0, -1, 1)   if clip_denoised                clamp first, then project: the projected value may leave [-1, 1]
//   S   = sum over the r x r block of (double) x0            fixed order, no atomics
//   d   = (float)((double) lambda * ((double) y - S / (double)(r r)))      one rounding to fp32
//   x0' = add_rn(x0, d)
//   x   = ((c1[j] x0' + c2[j] x) + c3[j] hist) + sigma[j] z ;  hist <- x0'      step_mix of sr3_common.h, same association
//                                                                               (c3 / hist both NULL: no history term)
//   step2_dev[1] = j - 1 on completion (step2_dev[0] is scratch, as in sr3_tiled_step)
//
// The block sum is a double: a sum of <= 1024 fp32 values of magnitude <= 1 is then (almost always exactly) independent of the order,
// so d, rounded once, is the value a NumPy restatement gets, and the step is bitwise reproducible run to run.
//
// Work split: a thread owns V consecutive columns (V = 4 as one 16-byte access where W % 4 == 0, r % 4 == 0 and every pointer is
// 16-byte aligned, step_tail.h's vec16; V = 1 otherwise) of one strip of r image rows of one (b, c) plane, lanes along x, so a row of
// the strip is read as one contiguous segment by consecutive lanes.  It adds its columns down the strip in row order; the n = r / V lanes of a block -- n is
// a power of two <= 32, and the lanes are consecutive and aligned to n, so they sit in one wavefront -- combine with a fixed
// __shfl_xor tree, after which every lane of the block holds the same S (a + b == b + a at every level).  x0 is not kept (r V values
// per thread: up to 128 registers): the second pass computes it again from the same operands, the same bits, and the strip's x and
// eps come out of the cache.  One thread per item, no grid-stride loop: there are fewer than 2^31 items.
#include "step_tail.h"

namespace sr3 {
namespace {

// the lanes of one block add up: afterwards all n hold the same sum
__device__ __forceinline__ double block_reduce(double S, int n) {
  for (int m = 1; m < n; m <<= 1) S += __shfl_xor(S, m);
  return S;
}

// item i -> its strip s = (b * C + c) * (H / r) + by and its lane lx along x; the strip's first row starts at s * r * W
template <int V>
__device__ __forceinline__ size_t strip_of(size_t i, int W, int& lx) {
  const int wv = W / V;
  lx = (int)(i % wv);
  return i / wv;
}

// dst[b, c, by, bx] = (float)(sum_double of the block / r^2)
template <int V>
__global__ __launch_bounds__(256) void k_block_mean(const float* __restrict__ src, float* __restrict__ dst, int W, int r, int n,
                                                     size_t total) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool act = i < total;      // (a block's lanes are all in or all out: total % n == 0; nobody leaves before the shuffles)
  int lx = 0;
  const size_t s = act ? strip_of<V>(i, W, lx) : 0;
  double S = 0.0;
  if (act) {
    const float* p = src + s * r * W + (size_t)lx * V;
    for (int y = 0; y < r; ++y, p += W) {
      float v[V];
      load_v<V>(p, v);
#pragma unroll
      for (int k = 0; k < V; ++k) S += (double)v[k];
    }
  }
  S = block_reduce(S, n);
  if (act && lx % n == 0) dst[s * (W / r) + lx / n] = (float)(S / (double)(r * r));
}

struct ConsistentStep {
  StepFuse f;                // the step's tail on x [B, C, H, W]; step_cur: step_copy put j there (clip: the kernel's template argument rules)
  const float* eps;          // [B, C, H, W]
  const float* y;            // target block means [B, C, H / r, W / r]
  int W, r, n;               // n = r / V lanes per block
  float strength;
  size_t total;              // items = B * C * (H / r) * (W / V)
};

template <bool CLIP, bool HIST, int V>
__global__ __launch_bounds__(256) void k_consistent_step(ConsistentStep s) {
  const StepFuse& f = s.f;
  const StepCoef cf = tail_begin<HIST>(f, blockIdx.x == 0 && threadIdx.x == 0);
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool act = i < s.total;
  int lx = 0;
  const size_t st = act ? strip_of<V>(i, s.W, lx) : 0;
  const size_t e0 = st * s.r * s.W + (size_t)lx * V;
  double S = 0.0;
  if (act) {
    const float* px = f.x + e0;
    const float* pe = s.eps + e0;
    for (int y = 0; y < s.r; ++y, px += s.W, pe += s.W) {
      float xv[V], ev[V];
      load_v<V>(px, xv);
      load_v<V>(pe, ev);
#pragma unroll
      for (int k = 0; k < V; ++k) S += (double)step_x0(cf, CLIP, xv[k], ev[k]);
    }
  }
  S = block_reduce(S, s.n);
  if (!act) return;
  const double yv = (double)s.y[st * (s.W / s.r) + lx / s.n];
  double mean = S / (double)(s.r * s.r);
  asm volatile("" : "+v"(mean));      // (opaque, as mul_rn's products are: the difference below is a subtraction, never one half of an fma)
  const float delta = (float)((double)s.strength * (yv - mean));
  size_t e = e0;
  for (int y = 0; y < s.r; ++y, e += s.W) {
    float xv[V], ev[V], zv[V], hv[V], x0[V];
    load_v<V>(s.eps + e, ev);
    tail_load<HIST, V>(f, e, xv, zv, hv);
#pragma unroll
    for (int k = 0; k < V; ++k) x0[k] = add_rn(step_x0(cf, CLIP, xv[k], ev[k]), delta);
    tail_mix_store<HIST, V>(f, cf, e, x0, xv, zv, hv);
  }
}

// the size arguments both entries share, before anything is launched; *total = B * C * H * W
int check_blocks(const char* who, int batch, int channels, int height, int width, int block, size_t* total) {
  if (const int rc = check_image_dims(who, batch, channels, height, width)) return rc;
  if (block != 2 && block != 4 && block != 8 && block != 16 && block != 32) { set_error("%s: block must be 2, 4, 8, 16 or 32 (got %d)", who, block); return SR3_E_BADARG; }
  if (height % block || width % block) { set_error("%s: block %d does not divide height %d and width %d", who, block, height, width); return SR3_E_BADARG; }
  *total = (size_t)batch * channels * height * width;
  return check_image_limit(who, *total);
}

}  // namespace
}  // namespace sr3

using namespace sr3;

extern "C" {

int sr3_block_mean_f32(const float* src_nchw, int batch, int channels, int height, int width, int block, float* dst_means, void* stream) {
  if (!src_nchw) { set_error("block_mean: src_nchw is NULL"); return SR3_E_BADARG; }
  if (!dst_means) { set_error("block_mean: dst_means is NULL"); return SR3_E_BADARG; }
  size_t total = 0;
  if (const int rc = check_blocks("block_mean", batch, channels, height, width, block, &total)) return rc;
  if (overlaps(src_nchw, total * sizeof(float), dst_means, total / ((size_t)block * block) * sizeof(float))) { set_error("block_mean: dst_means overlaps src_nchw"); return SR3_E_BADARG; }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool vec = (width & 3) == 0 && (block & 3) == 0 && vec16(src_nchw);
  const size_t items = vec ? total / block / 4 : total / block;
  const dim3 grid((unsigned)((items + 255) / 256));
  if (vec) hipLaunchKernelGGL(k_block_mean<4>, grid, dim3(256), 0, st, src_nchw, dst_means, width, block, block / 4, items);
  else hipLaunchKernelGGL(k_block_mean<1>, grid, dim3(256), 0, st, src_nchw, dst_means, width, block, block, items);
  SR3_LAUNCH_CHECK("k_block_mean");
  return SR3_OK;
}

int sr3_consistent_step(float* x_nchw, const float* eps_nchw, const float* z_nchw, const float* target_means, int batch, int channels,
                        int height, int width, int block, float strength, const float* tab_a, const float* tab_b, const float* tab_c1,
                        const float* tab_c2, const float* tab_sigma, int* step2_dev, int clip_denoised, const float* tab_c3,
                        float* hist_nchw, void* stream) {
  const Req req[] = {{x_nchw, "x_nchw"}, {eps_nchw, "eps_nchw"}, {target_means, "target_means"}, {tab_a, "tab_a"}, {tab_b, "tab_b"},
      {tab_c1, "tab_c1"}, {tab_c2, "tab_c2"}, {tab_sigma, "tab_sigma"}, {step2_dev, "step2_dev"}};
  if (const int rc = check_required("consistent_step", req)) return rc;
  size_t total = 0;
  if (const int rc = check_blocks("consistent_step", batch, channels, height, width, block, &total)) return rc;
  if (!(strength > 0.f && strength <= 1.f)) { set_error("consistent_step: strength must lie in (0, 1] (got %g)", (double)strength); return SR3_E_BADARG; }
  const size_t bytes = total * sizeof(float);
  if (const int rc = check_step_history("consistent_step", tab_c3, hist_nchw, x_nchw, eps_nchw, bytes)) return rc;
  if (overlaps(x_nchw, bytes, target_means, bytes / ((size_t)block * block))) { set_error("consistent_step: target_means overlaps x_nchw"); return SR3_E_BADARG; }
  const bool vec = (width & 3) == 0 && (block & 3) == 0 && vec16(x_nchw, eps_nchw, z_nchw, hist_nchw);
  ConsistentStep s;
  s.f = StepFuse{x_nchw, z_nchw, StepTables{tab_a, tab_b, tab_c1, tab_c2, tab_sigma}, step2_dev, step2_dev + 1, clip_denoised, tab_c3, hist_nchw};
  s.eps = eps_nchw; s.y = target_means; s.W = width; s.r = block; s.n = vec ? block / 4 : block; s.strength = strength;
  s.total = vec ? total / block / 4 : total / block;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (const int rc = step_copy(step2_dev, st)) return rc;
  const dim3 grid((unsigned)((s.total + 255) / 256));
  dispatch_bools([&](auto clip, auto hist, auto v4) {
    hipLaunchKernelGGL((k_consistent_step<clip(), hist(), v4() ? 4 : 1>), grid, dim3(256), 0, st, s);
  }, clip_denoised != 0, hist_nchw != nullptr, vec);
  SR3_LAUNCH_CHECK("k_consistent_step");
  return SR3_OK;
}

}  // extern "C"
