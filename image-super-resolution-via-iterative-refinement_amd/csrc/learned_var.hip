// Ancestral sampling with a learned reverse-process variance (include/sr3_mi355x.h: sr3_learned_var_step; Nichol & Dhariwal 2021,
// "Improved DDPM"): the network emits, next to its prediction, a per-pixel v that interpolates between log beta and log beta~ of the
// step, and the tail of a reverse step draws with that sigma instead of the table's.
//
// The arithmetic (out = the network's 2C channels [B, 2C, H, W]: C prediction channels, then C variance channels; j = step2_dev[1] on
// entry; lb = tab_log_beta[j], lt = tab_log_beta_tilde[j]):
//
//   x0    = a[j] x - b[j] out_c                              step_x0 of sr3_common.h: mul_rn, mul_rn, sub_rn
//   x0    = clamp(x0, -1, 1)   if clip_denoised
//   mean  = c1[j] x0 + c2[j] x                               step_mix's: mul_rn, mul_rn, add_rn -- bit-identical to k_p_sample_update's mean
//   f     = (out_{C + c} + 1) / 2 ;  sigma = exp((f lb + (1 - f) lt) / 2)      fp32; 0 where tab_sigma[j] == 0: the tables mark the
//                                                                              walk's last step that way, and it adds no noise
//   x     = mean + sigma z                                   mul_rn, add_rn (z NULL: zeros)
//   step2_dev[1] = j - 1 on completion (step2_dev[0] is scratch, as in sr3_tiled_step)
//
// Work split: a thread owns V consecutive elements of one (b, c) plane of x (V = 4 as one 16-byte access where H W % 4 == 0 and every
// pointer is 16-byte aligned, step_tail.h's vec16; V = 1 otherwise) and reads the same elements of the prediction plane and of the
// variance plane of `out`: three reads (four with z) and one write per element, one pass.  One thread per item, no grid-stride loop:
// there are fewer than 2^31 items.  No history: a multistep rule has no stochastic form here, and the entry refuses one.
#include "step_tail.h"

namespace sr3 {
namespace {

struct LearnedVarStep {
  StepFuse f;                   // the step's tail on x [B, C, H, W]; step_cur: step_copy put j there
  const float* out;             // [B, 2C, H, W]
  const float* log_beta;        // [S] tables, indexed like f.tb
  const float* log_beta_tilde;
  size_t plane;                 // C * H * W: elements of one image of x
  size_t total;                 // items = B * C * H * W / V
};

template <bool CLIP, int V>
__global__ __launch_bounds__(256) void k_learned_var_step(LearnedVarStep s) {
  const StepFuse& f = s.f;
  const StepCoef cf = tail_begin<false>(f, blockIdx.x == 0 && threadIdx.x == 0);
  const int j = f.step_cur[0];
  const float lb = s.log_beta[j], lt = s.log_beta_tilde[j];
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= s.total) return;
  const size_t e = i * V;
  const size_t po = e + (e / s.plane) * s.plane;      // the same element of the prediction plane: image b of `out` starts at 2 b plane
  float xv[V], zv[V], hv[V], ov[V], vv[V];
  load_v<V>(s.out + po, ov);
  load_v<V>(s.out + po + s.plane, vv);
  tail_load<false, V>(f, e, xv, zv, hv);
#pragma unroll
  for (int k = 0; k < V; ++k) {
    StepCoef c = cf;
    const float fr = 0.5f * (vv[k] + 1.f);
    c.sigma = cf.sigma == 0.f ? 0.f : expf(0.5f * (fr * lb + (1.f - fr) * lt));
    xv[k] = step_mix<false>(c, step_x0(cf, CLIP, xv[k], ov[k]), xv[k], zv[k], hv[k]);
  }
  store_v<V>(f.x + e, xv);
}

}  // namespace
}  // namespace sr3

using namespace sr3;

extern "C" {

int sr3_learned_var_step(float* x_nchw, const float* out_nchw, const float* z_nchw, int batch, int channels, int height, int width,
                         const float* tab_a, const float* tab_b, const float* tab_c1, const float* tab_c2, const float* tab_sigma,
                         const float* tab_log_beta, const float* tab_log_beta_tilde, int* step2_dev, int clip_denoised,
                         const float* tab_c3, float* hist_nchw, void* stream) {
  const char* who = "learned_var_step";
  const Req req[] = {{x_nchw, "x_nchw"}, {out_nchw, "out_nchw"}, {tab_a, "tab_a"}, {tab_b, "tab_b"}, {tab_c1, "tab_c1"}, {tab_c2, "tab_c2"},
      {tab_sigma, "tab_sigma"}, {tab_log_beta, "tab_log_beta"}, {tab_log_beta_tilde, "tab_log_beta_tilde"}, {step2_dev, "step2_dev"}};
  if (const int rc = check_required(who, req)) return rc;
  if (const int rc = check_image_dims(who, batch, channels, height, width)) return rc;
  const size_t total = (size_t)batch * channels * height * width;
  if (const int rc = check_image_limit(who, 2 * total)) return rc;      // (`out` is the larger buffer)
  if (tab_c3 || hist_nchw) { set_error("%s: no multistep history with a learned variance (tab_c3 and hist_nchw must be NULL)", who); return SR3_E_UNSUPPORTED; }
  const size_t bytes = total * sizeof(float);
  const Buf bufs[] = {{x_nchw, bytes, "x_nchw", true}, {out_nchw, 2 * bytes, "out_nchw", false}, {z_nchw, bytes, "z_nchw", false},
      {step2_dev, 2 * sizeof(int), "step2_dev", true}};
  if (const int rc = check_overlaps(who, bufs)) return rc;
  const size_t plane = (size_t)channels * height * width;
  const bool vec = (((size_t)height * width) & 3) == 0 && vec16(x_nchw, out_nchw, z_nchw);
  LearnedVarStep s;
  s.f = StepFuse{x_nchw, z_nchw, StepTables{tab_a, tab_b, tab_c1, tab_c2, tab_sigma}, step2_dev, step2_dev + 1, clip_denoised, nullptr, nullptr};
  s.out = out_nchw; s.log_beta = tab_log_beta; s.log_beta_tilde = tab_log_beta_tilde; s.plane = plane;
  s.total = vec ? total / 4 : total;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (const int rc = step_copy(step2_dev, st)) return rc;
  const dim3 grid((unsigned)((s.total + 255) / 256));
  dispatch_bools([&](auto clip, auto v4) {
    hipLaunchKernelGGL((k_learned_var_step<clip(), v4() ? 4 : 1>), grid, dim3(256), 0, st, s);
  }, clip_denoised != 0, vec);
  SR3_LAUNCH_CHECK("k_learned_var_step");
  return SR3_OK;
}

}  // extern "C"
