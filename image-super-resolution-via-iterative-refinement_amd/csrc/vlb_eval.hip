// Per-image terms of the variational bound (include/sr3_mi355x.h: sr3_vlb_terms_f32, sr3_q_sample_step_f32, sr3_prior_bpd_f32;
// Nichol & Dhariwal 2021, "Improved DDPM"): what the evaluation walk (calc_bpd_loop) measures per step and what the
// loss-aware timestep sampler reads back from a training step (sr3_train_step_ex3).
//
// The per-element term is the hybrid loss kernel's vlb (vlb_elem, train_kernels.hip), restated here without its gradient and with the sampler's clamp
// of x0^ -- the training kernel is left as it is.  With the row {a, b, c1, c2, lb = log beta, lt = log beta~, last} of the step, all fp32:
//
//   x0^ = a x_t - b out_c ; clamp(-1, 1) if clip_denoised
//   v   = the variance plane (var_mode 0), -1 (1: fixed small) or +1 (2: fixed large) ; f = (v + 1) / 2 ; lv = f lb + (1 - f) lt
//   not last:  vlb = (-1 + lv - lt + exp(lt - lv) + d^2 exp(-lv)) / 2 / ln 2,  d = c1 (x0 - x0^)
//   last:      vlb = -log2 max(mass, 1e-12), the mass N(c1 x0^ + c2 x_t, e^lv) puts on the bin x0 +- 1/255 (open beyond +-0.999), tanh CDF
//   mse = (x0 - x0^)^2
//
// Reduction: VLB_PARTS blocks per image, whatever its size.  A thread owns groups of four consecutive elements of the image (one 16-byte
// access each where C P % 4 == 0 and the pointers allow it, four guarded loads otherwise: the same elements in the same order, so the
// same bits either way), adds its terms in double in element order, the block folds its 256 sums in a fixed tree and stores one partial
// pair.  A second launch of one block adds an image's VLB_PARTS partials in index order and divides by C P.  No atomics, no last-block
// protocol: the same bits every run, whatever the scratch held.
#include <math.h>

#include "step_tail.h"
#include "train.h"

namespace sr3 {
namespace {

constexpr int VLB_PARTS = 16;

struct VlbScal { float a, b, c1, c2, lb, lt; bool last; };
__device__ __forceinline__ float tanh_cdf(float u) {
  constexpr float K = 0.7978845608028654f;      // sqrt(2 / pi)
  return 0.5f * (1.f + tanhf(K * (u + 0.044715f * u * u * u)));
}
// (vlb_elem of train_kernels.hip, term for term, on an x0^ the caller made)
__device__ __forceinline__ float vlb_term(const VlbScal& k, float x0, float xt, float x0h, float v) {
  constexpr float RLN2 = 1.4426950408889634f;
  const float f = 0.5f * (v + 1.f);
  const float lv = f * k.lb + (1.f - f) * k.lt;
  if (!k.last) {
    const float d = k.c1 * (x0 - x0h);
    const float r = expf(k.lt - lv), q = d * d * expf(-lv);
    return 0.5f * (-1.f + lv - k.lt + r + q) * RLN2;
  }
  const float cx = x0 - (k.c1 * x0h + k.c2 * xt), inv = expf(-0.5f * lv);
  const float up = inv * (cx + 1.f / 255.f), um = inv * (cx - 1.f / 255.f);
  const float cp = tanh_cdf(up), cm = tanh_cdf(um);
  const float arg = x0 < -0.999f ? cp : (x0 > 0.999f ? 1.f - cm : cp - cm);
  return -logf(arg >= 1e-12f ? arg : 1e-12f) * RLN2;
}

// four consecutive floats at p, the first `cnt` of them inside the image
template <int V>
__device__ __forceinline__ void load_group(const float* p, int cnt, float (&v)[4]) {
  if constexpr (V == 4) {
    load_v<4>(p, v);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = k < cnt ? p[k] : 0.f;
  }
}

// the block's two sums -> part[(image * VLB_PARTS + slice) * 2 + {0, 1}]
__device__ __forceinline__ void store_partials(double s0, double s1, double* part) {
  __shared__ double red[256];
  for (int pass = 0; pass < 2; ++pass) {
    __syncthreads();
    red[threadIdx.x] = pass ? s1 : s0;
    __syncthreads();
    for (int m = 128; m >= 1; m >>= 1) {
      if ((int)threadIdx.x < m) red[threadIdx.x] += red[threadIdx.x + m];
      __syncthreads();
    }
    if (threadIdx.x == 0) part[(size_t)blockIdx.x * 2 + pass] = red[0];
  }
}

struct VlbTerms {
  const float* x0; const float* xt;   // [B, n]
  const float* out;                   // [B, out_stride]: the prediction planes first, then (MODE 0) the variance planes
  const float* table;                 // [table_rows, HYB_STRIDE]
  const int* rows;                    // [B] or null
  const int* step2;                   // the step counter pair or null (then step2[1] is every image's row); both null: image b reads row b
  int table_rows;
  size_t n, out_stride, groups;       // C P ; OC P ; ceil(n / 4)
  double* part;
};

template <int MODE, bool CLIP, int V>
__global__ __launch_bounds__(256) void k_vlb_terms(VlbTerms s) {
  const size_t b = blockIdx.x / VLB_PARTS;
  const int slice = blockIdx.x % VLB_PARTS;
  const int row = s.rows ? s.rows[b] : (s.step2 ? s.step2[1] : (int)b);
  double sv = 0.0, sm = 0.0;
  if (row < 0 || row >= s.table_rows) {           // (uniform over the block) a row the table does not have: the image's terms are NaN
    sv = sm = __builtin_nan("");
  } else {
    const float* hs = s.table + (size_t)row * HYB_STRIDE;
    const VlbScal k = {hs[HYB_A], hs[HYB_B], hs[HYB_C1], hs[HYB_C2], hs[HYB_LOG_BETA], hs[HYB_LOG_BETA_TILDE], hs[HYB_LAST] != 0.f};
    const float* x0 = s.x0 + b * s.n;
    const float* xt = s.xt + b * s.n;
    const float* oc = s.out + b * s.out_stride;
    for (size_t g = (size_t)slice * 256 + threadIdx.x; g < s.groups; g += (size_t)VLB_PARTS * 256) {
      const size_t e = g * 4;
      const int cnt = (int)(s.n - e < 4 ? s.n - e : 4);
      float xv[4], tv[4], ov[4], vv[4];
      load_group<V>(x0 + e, cnt, xv);
      load_group<V>(xt + e, cnt, tv);
      load_group<V>(oc + e, cnt, ov);
      if (MODE == 0) load_group<V>(oc + s.n + e, cnt, vv);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (q < cnt) {
          float x0h = k.a * tv[q] - k.b * ov[q];
          if (CLIP) x0h = fminf(fmaxf(x0h, -1.f), 1.f);
          const float v = MODE == 0 ? vv[q] : (MODE == 1 ? -1.f : 1.f);
          sv += (double)vlb_term(k, xv[q], tv[q], x0h, v);
          const float dm = xv[q] - x0h;
          sm += (double)dm * (double)dm;
        }
      }
    }
  }
  store_partials(sv, sm, s.part);
}

// KL(N(sa x0, var) || N(0, 1)) in bits per element: (-1 - log var + var + (sa x0)^2) / 2 / ln 2
template <int V>
__global__ __launch_bounds__(256) void k_prior_bpd(const float* __restrict__ x0, size_t n, size_t groups, float sa, float var, float lvar,
                                                    double* __restrict__ part) {
  constexpr float RLN2 = 1.4426950408889634f;
  const size_t b = blockIdx.x / VLB_PARTS;
  const int slice = blockIdx.x % VLB_PARTS;
  double sv = 0.0;
  for (size_t g = (size_t)slice * 256 + threadIdx.x; g < groups; g += (size_t)VLB_PARTS * 256) {
    const size_t e = g * 4;
    const int cnt = (int)(n - e < 4 ? n - e : 4);
    float xv[4];
    load_group<V>(x0 + b * n + e, cnt, xv);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (q < cnt) {
        const float m = sa * xv[q];
        sv += (double)(0.5f * (-1.f - lvar + var + m * m) * RLN2);
      }
    }
  }
  store_partials(sv, 0.0, part);
}

// One block.  Image b's partials in index order, divided by n: out0 / out1 (may be null) [b * ostride], or row j = step2[1] of
// [table_rows, B] arrays -- then step2[1] = j - 1.  Every thread has read j before one writes; slot 0 (a step's scratch copy in the loops whose
// first launch is step_copy) is neither read nor written: every reader of this step -- q_sample at the counter, the forward, k_vlb_terms --
// runs before this launch and reads slot 1, which nothing else moves.
__global__ __launch_bounds__(256) void k_vlb_finish(const double* __restrict__ part, int B, double n, float* __restrict__ out0,
                                                     float* __restrict__ out1, int ostride, int* step2, int table_rows) {
  const int j = step2 ? step2[1] : 0;
  __syncthreads();
  if (j >= 0 && j < table_rows) {
    for (int b = threadIdx.x; b < B; b += 256) {
      double s0 = 0.0, s1 = 0.0;
      for (int p = 0; p < VLB_PARTS; ++p) {
        s0 += part[((size_t)b * VLB_PARTS + p) * 2];
        s1 += part[((size_t)b * VLB_PARTS + p) * 2 + 1];
      }
      const size_t o = ((size_t)j * B + b) * ostride;
      out0[o] = (float)(s0 / n);
      if (out1) out1[o] = (float)(s1 / n);
    }
  }
  if (step2 && threadIdx.x == 0) step2[1] = j - 1;
}

template <int V>
__global__ __launch_bounds__(256) void k_q_sample_step(const float* __restrict__ x0, const float* __restrict__ z,
                                                        const float* __restrict__ ca, const float* __restrict__ cb,
                                                        const int* __restrict__ step_dev, int table_rows, size_t items,
                                                        float* __restrict__ out) {
  const int j = step_dev[0];
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= items || j < 0 || j >= table_rows) return;
  const float a = ca[j], s = cb[j];
  float xv[V], zv[V], ov[V];
  load_v<V>(x0 + i * V, xv);
  load_v<V>(z + i * V, zv);
#pragma unroll
  for (int k = 0; k < V; ++k) ov[k] = add_rn(mul_rn(a, xv[k]), mul_rn(s, zv[k]));      // k_q_sample's
  store_v<V>(out + i * V, ov);
}

size_t scratch_need(int batch) { return (size_t)batch * VLB_PARTS * 2 * sizeof(double); }

}  // namespace

// the launch pair behind the public entry and behind sr3_train_step_ex3 (arguments checked by the caller)
int vlb_terms(const float* x0, const float* xt, const float* out, const float* table, int table_rows, const int* rows, int* step2,
              int var_mode, bool clip, int B, int C, int OC, int P, float* vb_out, float* mse_out, int ostride, double* part, hipStream_t st) {
  VlbTerms s;
  s.x0 = x0; s.xt = xt; s.out = out; s.table = table; s.rows = rows; s.step2 = step2; s.table_rows = table_rows;
  s.n = (size_t)C * P; s.out_stride = (size_t)OC * P; s.groups = (s.n + 3) / 4; s.part = part;
  const bool vec = (s.n & 3) == 0 && (s.out_stride & 3) == 0 && vec16(x0, xt, out);
  const dim3 grid((unsigned)((size_t)B * VLB_PARTS));
  auto launch = [&](auto mode) {
    dispatch_bools([&](auto cl, auto v4) {
      hipLaunchKernelGGL((k_vlb_terms<decltype(mode)::value, cl(), v4() ? 4 : 1>), grid, dim3(256), 0, st, s);
    }, clip, vec);
  };
  if (var_mode == 0) launch(std::integral_constant<int, 0>{});
  else if (var_mode == 1) launch(std::integral_constant<int, 1>{});
  else launch(std::integral_constant<int, 2>{});
  SR3_LAUNCH_CHECK("k_vlb_terms");
  hipLaunchKernelGGL(k_vlb_finish, dim3(1), dim3(256), 0, st, part, B, (double)s.n, vb_out, mse_out, ostride, step2, step2 ? table_rows : 1);
  SR3_LAUNCH_CHECK("k_vlb_finish");
  return SR3_OK;
}
size_t vlb_terms_scratch(int batch) { return scratch_need(batch); }

}  // namespace sr3

using namespace sr3;

extern "C" {

size_t sr3_vlb_terms_partials_bytes(int batch) { return batch > 0 ? scratch_need(batch) : 0; }

int sr3_vlb_terms_f32(const float* x0, const float* x_t, const float* out, int out_channels, const float* table, int table_rows,
                      const int* rows_per_image, int* step2_dev, int var_mode, int clip_denoised, int batch, int channels, int pixels,
                      float* vb_out, float* x0_mse_out, void* scratch, size_t scratch_bytes, void* stream) {
  const char* who = "sr3_vlb_terms_f32";
  const Req req[] = {{x0, "x0"}, {x_t, "x_t"}, {out, "out"}, {table, "table"}, {vb_out, "vb_out"}, {x0_mse_out, "x0_mse_out"},
      {scratch, "scratch"}};
  if (const int rc = check_required(who, req)) return rc;
  if ((rows_per_image != nullptr) == (step2_dev != nullptr)) {
    set_error("%s: exactly one of rows_per_image and step2_dev selects the rows (%s given)", who, rows_per_image ? "both" : "neither");
    return SR3_E_BADARG;
  }
  if (batch <= 0 || channels <= 0 || pixels <= 0 || table_rows <= 0) {
    set_error("%s: batch, channels, pixels and table_rows must be positive (got %d, %d, %d, %d)", who, batch, channels, pixels, table_rows);
    return SR3_E_BADARG;
  }
  if (var_mode < 0 || var_mode > 2) { set_error("%s: var_mode %d is outside 0..2", who, var_mode); return SR3_E_BADARG; }
  if (out_channels != (var_mode == 0 ? 2 * channels : channels)) {
    set_error("%s: out_channels %d does not go with var_mode %d (%d channels: %d)", who, out_channels, var_mode, channels,
              var_mode == 0 ? 2 * channels : channels);
    return SR3_E_BADARG;
  }
  const size_t total = (size_t)batch * out_channels * pixels;
  if (const int rc = check_image_limit(who, total)) return rc;
  if ((size_t)batch * VLB_PARTS >= ((size_t)1 << 31) || (step2_dev && (size_t)table_rows * batch >= ((size_t)1 << 31))) {
    set_error("%s: batch %d (times table_rows %d) is too large", who, batch, table_rows);
    return SR3_E_UNSUPPORTED;
  }
  const size_t need = scratch_need(batch);
  if (scratch_bytes < need) { set_error("%s: scratch too small (%zu < %zu)", who, scratch_bytes, need); return SR3_E_NOMEM; }
  const size_t img = (size_t)batch * channels * pixels * sizeof(float);
  const size_t outb = (step2_dev ? (size_t)table_rows : 1) * batch * sizeof(float);
  const Buf bufs[] = {{vb_out, outb, "vb_out", true}, {x0_mse_out, outb, "x0_mse_out", true}, {scratch, need, "scratch", true},
      {step2_dev, 2 * sizeof(int), "step2_dev", true}, {x0, img, "x0", false}, {x_t, img, "x_t", false},
      {out, total * sizeof(float), "out", false}, {table, (size_t)table_rows * HYB_STRIDE * sizeof(float), "table", false},
      {rows_per_image, (size_t)batch * sizeof(int), "rows_per_image", false}};
  if (const int rc = check_overlaps(who, bufs)) return rc;
  if ((uintptr_t)scratch & 7) { set_error("%s: scratch is not 8-byte aligned", who); return SR3_E_ALIGN; }
  return vlb_terms(x0, x_t, out, table, table_rows, rows_per_image, step2_dev, var_mode, clip_denoised != 0, batch, channels, out_channels,
                   pixels, vb_out, x0_mse_out, 1, static_cast<double*>(scratch), static_cast<hipStream_t>(stream));
}

int sr3_prior_bpd_f32(const float* x0, int batch, int elems_per_image, float sqrt_abar, float var, float log_var, float* out,
                      void* scratch, size_t scratch_bytes, void* stream) {
  const char* who = "sr3_prior_bpd_f32";
  const Req req[] = {{x0, "x0"}, {out, "out"}, {scratch, "scratch"}};
  if (const int rc = check_required(who, req)) return rc;
  if (batch <= 0 || elems_per_image <= 0) { set_error("%s: batch and elems_per_image must be positive (got %d, %d)", who, batch, elems_per_image); return SR3_E_BADARG; }
  if (!(isfinite(sqrt_abar) && isfinite(var) && isfinite(log_var))) { set_error("%s: sqrt_abar, var and log_var must be finite", who); return SR3_E_BADARG; }
  const size_t total = (size_t)batch * elems_per_image;
  if (const int rc = check_image_limit(who, total)) return rc;
  if ((size_t)batch * VLB_PARTS >= ((size_t)1 << 31)) { set_error("%s: batch %d is too large", who, batch); return SR3_E_UNSUPPORTED; }
  const size_t need = scratch_need(batch);
  if (scratch_bytes < need) { set_error("%s: scratch too small (%zu < %zu)", who, scratch_bytes, need); return SR3_E_NOMEM; }
  const Buf bufs[] = {{out, (size_t)batch * sizeof(float), "out", true}, {scratch, need, "scratch", true},
      {x0, total * sizeof(float), "x0", false}};
  if (const int rc = check_overlaps(who, bufs)) return rc;
  if ((uintptr_t)scratch & 7) { set_error("%s: scratch is not 8-byte aligned", who); return SR3_E_ALIGN; }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t n = (size_t)elems_per_image, groups = (n + 3) / 4;
  const dim3 grid((unsigned)((size_t)batch * VLB_PARTS));
  double* part = static_cast<double*>(scratch);
  if ((n & 3) == 0 && vec16(x0)) hipLaunchKernelGGL(k_prior_bpd<4>, grid, dim3(256), 0, st, x0, n, groups, sqrt_abar, var, log_var, part);
  else hipLaunchKernelGGL(k_prior_bpd<1>, grid, dim3(256), 0, st, x0, n, groups, sqrt_abar, var, log_var, part);
  SR3_LAUNCH_CHECK("k_prior_bpd");
  hipLaunchKernelGGL(k_vlb_finish, dim3(1), dim3(256), 0, st, part, batch, (double)n, out, (float*)nullptr, 1, (int*)nullptr, 1);
  SR3_LAUNCH_CHECK("k_vlb_finish");
  return SR3_OK;
}

int sr3_q_sample_step_f32(const float* x0, const float* z, const float* tab_ca, const float* tab_cb, int table_rows, const int* step_dev,
                          int batch, int elems_per_image, float* out, void* stream) {
  const char* who = "sr3_q_sample_step_f32";
  const Req req[] = {{x0, "x0"}, {z, "z"}, {tab_ca, "tab_ca"}, {tab_cb, "tab_cb"}, {step_dev, "step_dev"}, {out, "out"}};
  if (const int rc = check_required(who, req)) return rc;
  if (batch <= 0 || elems_per_image <= 0 || table_rows <= 0) {
    set_error("%s: batch, elems_per_image and table_rows must be positive (got %d, %d, %d)", who, batch, elems_per_image, table_rows);
    return SR3_E_BADARG;
  }
  const size_t total = (size_t)batch * elems_per_image;
  if (const int rc = check_image_limit(who, total)) return rc;
  const size_t bytes = total * sizeof(float);
  const Buf bufs[] = {{out, bytes, "out", true}, {x0, bytes, "x0", false}, {z, bytes, "z", false},
      {tab_ca, (size_t)table_rows * sizeof(float), "tab_ca", false}, {tab_cb, (size_t)table_rows * sizeof(float), "tab_cb", false},
      {step_dev, sizeof(int), "step_dev", false}};
  if (const int rc = check_overlaps(who, bufs)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool vec = (total & 3) == 0 && vec16(x0, z, out);
  const size_t items = vec ? total / 4 : total;
  const dim3 grid((unsigned)((items + 255) / 256));
  if (vec) hipLaunchKernelGGL(k_q_sample_step<4>, grid, dim3(256), 0, st, x0, z, tab_ca, tab_cb, step_dev, table_rows, items, out);
  else hipLaunchKernelGGL(k_q_sample_step<1>, grid, dim3(256), 0, st, x0, z, tab_ca, tab_cb, step_dev, table_rows, items, out);
  SR3_LAUNCH_CHECK("k_q_sample_step");
  return SR3_OK;
}

}  // extern "C"
