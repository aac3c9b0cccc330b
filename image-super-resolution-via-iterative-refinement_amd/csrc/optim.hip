// The optimizer's passes over the parameter arena, HBM-bound, and their ABI entries: the fused Adam(+EMA) update -- ONE kernel
// template, one launcher and one argument check behind sr3_adam_step / sr3_adam_ema_step / sr3_adam_ema_step_scaled, so that the
// three give the same bits because they run the same code -- and the global gradient norm / micro-batch accumulation that feed
// it (config train.optimizer.clip_grad_norm / accumulate).  None of them takes a plan.
#include <math.h>

#include "sr3_common.h"
#include "train.h"

namespace sr3 {

__device__ __forceinline__ f32x4 ld4(const float* p, size_t i) { return *reinterpret_cast<const f32x4*>(p + i * 4); }
__device__ __forceinline__ void st4(float* p, size_t i, const f32x4& x) { *reinterpret_cast<f32x4*>(p + i * 4) = x; }

// T12: fused Adam over the whole parameter arena (torch.optim.Adam defaults, model/model.py:39-40):
// m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2 ; p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps)
// Four elements.  The fused multiply-adds are written out: left to the compiler, which of the two products of `v b2 + w2 g g` is
// fused depends on the code around the expression, and every instantiation of k_adam_pass must give the same bits.
__device__ __forceinline__ void adam_vec4(f32x4& pv, const f32x4& gv, f32x4& mv, f32x4& vv, float w1, float b2, float w2,
                                          float eps, float step, float bc2_sqrt) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    mv[e] = fmaf(gv[e] - mv[e], w1, mv[e]);                   // torch: exp_avg.lerp_(grad, 1 - beta1)
    vv[e] = fmaf(vv[e], b2, w2 * gv[e] * gv[e]);              //        exp_avg_sq.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    const float denom = sqrtf(vv[e]) / bc2_sqrt + eps;
    pv[e] = fmaf(-step, mv[e] / denom, pv[e]);
  }
}
// T12b: the exponential moving average of the weights as one more stream over the arena: ema += (p_new - ema) * we,
// we = 1 - ema_decay -- the lerp form of exp_avg above: p_new == ema leaves ema unchanged exactly.
__device__ __forceinline__ void ema_lerp4(f32x4& ev, const f32x4& pv, float we) {
#pragma unroll
  for (int e = 0; e < 4; ++e) ev[e] = fmaf(pv[e] - ev[e], we, ev[e]);
}
// T12c: the scaled gradient is a product rounded on its own: contraction is switched off for it, since this toolchain's __fmul_rn
// is a plain `x * y` that the compiler may fold into the subtraction that follows.
__device__ __forceinline__ float fmul_rn_alone(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
// The pass.  MODE 0: Adam alone (no access to ema); 1: ema = p_new (the copy before step_start_ema); 2: the lerp.  SCALED: on
// g * scale4[1], guarded by scale4[2] (scale4 = the four floats k_grad_norm_finish writes: norm, coef, finite flag, 0; every thread
// reads the same 16 bytes).  Flag 0: nothing is written.  coef == 1: the bits of the unscaled pass.  No atomics.
template <int MODE, bool SCALED>
__global__ __launch_bounds__(256) void k_adam_pass(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, float* __restrict__ ema, size_t n4, float w1, float b2,
                                                    float w2, float eps, float step, float bc2_sqrt, float we,
                                                    const float* __restrict__ scale4) {
  float coef = 1.f;
  if (SCALED) {
    const f32x4 sc = ld4(scale4, 0);
    if (sc[2] == 0.f) return;
    coef = sc[1];
  }
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    f32x4 pv = ld4(p, i), gv = ld4(g, i), mv = ld4(m, i), vv = ld4(v, i);
    f32x4 ev = {0.f, 0.f, 0.f, 0.f};
    if (MODE == 2) ev = ld4(ema, i);
    if (SCALED) {
#pragma unroll
      for (int e = 0; e < 4; ++e) gv[e] = fmul_rn_alone(gv[e], coef);
    }
    adam_vec4(pv, gv, mv, vv, w1, b2, w2, eps, step, bc2_sqrt);
    if (MODE == 2) ema_lerp4(ev, pv, we);
    st4(p, i, pv);
    st4(m, i, mv);
    st4(v, i, vv);
    if (MODE == 1) st4(ema, i, pv);
    if (MODE == 2) st4(ema, i, ev);
  }
}

// torch.optim.Adam evaluates 1 - beta, the bias corrections and the step size as Python floats (double) and rounds
// each ONCE to fp32 when it meets the tensor (meant_double: the decimal behind the ABI's fp32 hyper-parameters).
struct AdamScalars { float w1, b2, w2, eps, step_size, bc2s; };
static AdamScalars adam_scalars(float lr, float b1, float b2, float eps, int step) {
  const double b1d = meant_double(b1), b2d = meant_double(b2), lrd = meant_double(lr);
  const double bc1 = 1.0 - pow(b1d, (double)step);
  const double bc2 = 1.0 - pow(b2d, (double)step);
  return {(float)(1.0 - b1d), (float)b2d, (float)(1.0 - b2d), (float)meant_double(eps), (float)(lrd / bc1), (float)sqrt(bc2)};
}
// ema_mode 0 none | 1 ema = p | 2 ema += (p - ema)(1 - ema_decay).  Arguments are checked by check_adam_args.
static int adam_pass(float* p, const float* g, float* m, float* v, float* ema, size_t n, float lr, float b1, float b2, float eps,
                     int step, float ema_decay, int ema_mode, const float* scale4 /* null: unscaled */, hipStream_t st) {
  const AdamScalars a = adam_scalars(lr, b1, b2, eps, step);
  const float we = (float)(1.0 - meant_double(ema_decay));      // 1 - decay in double, rounded once (as 1 - beta1 is)
  static constexpr decltype(&k_adam_pass<0, false>) kernels[3][2] = {{k_adam_pass<0, false>, k_adam_pass<0, true>},
                                                                     {k_adam_pass<1, false>, k_adam_pass<1, true>},
                                                                     {k_adam_pass<2, false>, k_adam_pass<2, true>}};
  hipLaunchKernelGGL(kernels[ema_mode][scale4 != nullptr], dim3(ew_blocks(n / 4)), dim3(256), 0, st, p, g, m, v, ema, n / 4, a.w1,
                     a.b2, a.w2, a.eps, a.step_size, a.bc2s, we, scale4);
  SR3_LAUNCH_CHECK("k_adam_pass");
  return SR3_OK;
}

// The refusals of the three Adam entries, in one order under the entry's own name (`scaled`: scale4 is one of its arguments).
// Nothing has been launched when this returns non-zero.
static int check_adam_args(const char* who, const float* params, const float* grads, const float* exp_avg, const float* exp_avg_sq,
                           const float* ema, size_t n, int step, float ema_decay, int ema_mode, bool scaled, const float* scale4) {
  if (!params || !grads || !exp_avg || !exp_avg_sq) { set_error("%s: params / grads / exp_avg / exp_avg_sq is NULL", who); return SR3_E_BADARG; }
  if (scaled && !scale4) { set_error("%s: scale4_dev is NULL", who); return SR3_E_BADARG; }
  if (ema_mode < 0 || ema_mode > 2) { set_error("%s: ema_mode %d is outside 0..2", who, ema_mode); return SR3_E_BADARG; }
  if (!ema && ema_mode != 0) { set_error("%s: ema is NULL with ema_mode %d", who, ema_mode); return SR3_E_BADARG; }
  if (!(ema_decay >= 0.f && ema_decay < 1.f)) { set_error("%s: ema_decay %g is outside [0, 1)", who, (double)ema_decay); return SR3_E_BADARG; }
  if (n & 3) { set_error("%s: n %zu is not a multiple of 4", who, n); return SR3_E_BADARG; }
  if (step < 1) { set_error("%s: step %d < 1", who, step); return SR3_E_BADARG; }
  if (((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)ema | (uintptr_t)scale4) & 15) {
    set_error("%s: misaligned pointer (16-byte vectors)", who);
    return SR3_E_ALIGN;
  }
  return SR3_OK;
}

// T13: global L2 norm of the gradient arena and accumulation of micro-batch gradients (config train.optimizer.clip_grad_norm /
// accumulate).  The grid is FIXED -- min(GRAD_NORM_BLOCKS, ceil(n4 / 256)) blocks of 256 threads, whatever the device -- and every
// sum has one order: a thread adds the squares of its vectors in stride order (elements 0..3 of each) in double, the 64 lanes of a
// wave combine by __shfl_xor (32, 16, .., 1), the block's four waves are added in wave order through LDS, and one wave adds the
// blocks' partial sums in index order.  The square of an fp32 is exact in double, so contraction cannot change a bit.  No atomics.
constexpr int GRAD_NORM_BLOCKS = 512;
static inline int grad_norm_blocks(size_t n4) { const size_t b = (n4 + 255) / 256; return (int)(b > GRAD_NORM_BLOCKS ? GRAD_NORM_BLOCKS : (b ? b : 1)); }

__device__ __forceinline__ void sqsum4(double& s, const f32x4& x) {
#pragma unroll
  for (int e = 0; e < 4; ++e) s += (double)x[e] * (double)x[e];
}
__device__ __forceinline__ void grad_sq_block_part(double s, double* __restrict__ part) {
  __shared__ double red[4];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}
__global__ __launch_bounds__(256) void k_grad_sqnorm_parts(const float* __restrict__ g, size_t n4, double* __restrict__ part) {
  double s = 0.0;
  const size_t st = (size_t)gridDim.x * 256;
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  for (; i + 3 * st < n4; i += 4 * st) {       // four loads in flight; the squares are added in the order of the plain loop
    const f32x4 a = ld4(g, i), b = ld4(g, i + st), c = ld4(g, i + 2 * st), d = ld4(g, i + 3 * st);
    sqsum4(s, a); sqsum4(s, b); sqsum4(s, c); sqsum4(s, d);
  }
  for (; i < n4; i += st) sqsum4(s, ld4(g, i));
  grad_sq_block_part(s, part);
}
// acc = g (FIRST) or acc + g: one fp32 add per element; NORM: also the partial sums of squares of the result, as k_grad_sqnorm_parts
// would give them for it
template <bool FIRST, bool NORM>
__global__ __launch_bounds__(256) void k_grad_accumulate(float* __restrict__ acc, const float* __restrict__ g, size_t n4,
                                                          double* __restrict__ part) {
  double s = 0.0;
  const size_t st = (size_t)gridDim.x * 256;
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  for (; i + 3 * st < n4; i += 4 * st) {
    f32x4 a = ld4(g, i), b = ld4(g, i + st), c = ld4(g, i + 2 * st), d = ld4(g, i + 3 * st);
    if (!FIRST) {
      const f32x4 pa = ld4(acc, i), pb = ld4(acc, i + st), pc = ld4(acc, i + 2 * st), pd = ld4(acc, i + 3 * st);
      a = pa + a; b = pb + b; c = pc + c; d = pd + d;
    }
    st4(acc, i, a); st4(acc, i + st, b); st4(acc, i + 2 * st, c); st4(acc, i + 3 * st, d);
    if (NORM) { sqsum4(s, a); sqsum4(s, b); sqsum4(s, c); sqsum4(s, d); }
  }
  for (; i < n4; i += st) {
    f32x4 r = ld4(g, i);
    if (!FIRST) r = ld4(acc, i) + r;
    st4(acc, i, r);
    if (NORM) sqsum4(s, r);
  }
  if (NORM) grad_sq_block_part(s, part);
}
// one wave: out4 = {norm, coef, finite ? 1 : 0, 0}; coef as torch.nn.utils.clip_grad_norm_ forms it in fp32, 1 when max_norm <= 0
__global__ __launch_bounds__(64) void k_grad_norm_finish(const double* __restrict__ part, int nparts, float max_norm,
                                                          float* __restrict__ out4) {
  __shared__ double sp[GRAD_NORM_BLOCKS];
  for (int i = threadIdx.x; i < nparts; i += 64) sp[i] = part[i];
  __syncthreads();
  if (threadIdx.x != 0) return;
  double s = 0.0;
  for (int i = 0; i < nparts; ++i) s += sp[i];
  const float norm = (float)sqrt(s);
  float coef = 1.0f;
  if (max_norm > 0.f) {
    const float c = max_norm / (norm + 1e-6f);
    coef = c < 1.0f ? c : 1.0f;
  }
  const f32x4 o = {norm, coef, isfinite(norm) ? 1.0f : 0.0f, 0.0f};
  *reinterpret_cast<f32x4*>(out4) = o;
}

static size_t grad_norm_scratch_bytes(size_t n) { return (size_t)grad_norm_blocks(n / 4) * sizeof(double); }
static int grad_norm_finish(const double* part, int nparts, float max_norm, float* out4, hipStream_t st) {
  hipLaunchKernelGGL(k_grad_norm_finish, dim3(1), dim3(64), 0, st, part, nparts, max_norm, out4);
  SR3_LAUNCH_CHECK("k_grad_norm_finish");
  return SR3_OK;
}
// out4 = {norm, coef, finite flag, 0} of g[0..n), coef = min(1, max_norm / (norm + 1e-6)) (1 when max_norm <= 0);
// part: grad_norm_scratch_bytes(n) of doubles
static int grad_norm(const float* g, size_t n, float max_norm, double* part, float* out4, hipStream_t st) {
  const int blocks = grad_norm_blocks(n / 4);
  hipLaunchKernelGGL(k_grad_sqnorm_parts, dim3(blocks), dim3(256), 0, st, g, n / 4, part);
  SR3_LAUNCH_CHECK("k_grad_sqnorm_parts");
  return grad_norm_finish(part, blocks, max_norm, out4, st);
}
// acc = first ? g : acc + g; out4 != nullptr: also what grad_norm(acc) would write, from the same pass (bit-equal to it)
static int grad_accumulate(float* acc, const float* g, size_t n, bool first, float max_norm, double* part, float* out4, hipStream_t st) {
  const dim3 grid(grad_norm_blocks(n / 4)), block(256);
#define SR3_GRAD_ACC(FIRST, NORM) hipLaunchKernelGGL((k_grad_accumulate<FIRST, NORM>), grid, block, 0, st, acc, g, n / 4, part)
  if (out4) { if (first) SR3_GRAD_ACC(true, true); else SR3_GRAD_ACC(false, true); }
  else { if (first) SR3_GRAD_ACC(true, false); else SR3_GRAD_ACC(false, false); }
#undef SR3_GRAD_ACC
  SR3_LAUNCH_CHECK("k_grad_accumulate");
  return out4 ? grad_norm_finish(part, (int)grid.x, max_norm, out4, st) : SR3_OK;
}

// The norm-side refusals sr3_grad_norm and sr3_grad_accumulate share (`with_norm`: the norm is asked for, so its scratch is
// needed): a NaN max_norm, the scratch size, alignment.  vec16: the entry's 16-byte pointers ORed, `names` as its message lists them.
static int check_norm_args(const char* who, size_t n, float max_norm, const void* scratch, size_t scratch_bytes, bool with_norm,
                           uintptr_t vec16, const char* names) {
  if (with_norm) {
    if (max_norm != max_norm) { set_error("%s: max_norm is NaN", who); return SR3_E_BADARG; }
    if (scratch_bytes < grad_norm_scratch_bytes(n)) {
      set_error("%s: scratch_bytes %zu < %zu", who, scratch_bytes, grad_norm_scratch_bytes(n));
      return SR3_E_BADARG;
    }
  }
  if ((vec16 & 15) || (with_norm && ((uintptr_t)scratch & 7))) {
    set_error("%s: misaligned pointer (%s: 16 bytes, scratch: 8)", who, names);
    return SR3_E_ALIGN;
  }
  return SR3_OK;
}

}  // namespace sr3

using namespace sr3;

extern "C" {

int sr3_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, size_t n, float lr, float beta1,
                  float beta2, float eps, int step, void* stream) {
  const int rc = check_adam_args("sr3_adam_step", params, grads, exp_avg, exp_avg_sq, nullptr, n, step, 0.f, 0, false, nullptr);
  return rc ? rc : adam_pass(params, grads, exp_avg, exp_avg_sq, nullptr, n, lr, beta1, beta2, eps, step, 0.f, 0, nullptr,
                             static_cast<hipStream_t>(stream));
}

int sr3_adam_ema_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, size_t n, float lr,
                      float beta1, float beta2, float eps, int step, float ema_decay, int ema_mode, void* stream) {
  const int rc = check_adam_args("sr3_adam_ema_step", params, grads, exp_avg, exp_avg_sq, ema, n, step, ema_decay, ema_mode, false, nullptr);
  return rc ? rc : adam_pass(params, grads, exp_avg, exp_avg_sq, ema, n, lr, beta1, beta2, eps, step, ema_decay, ema_mode, nullptr,
                             static_cast<hipStream_t>(stream));
}

int sr3_adam_ema_step_scaled(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, size_t n, float lr,
                             float beta1, float beta2, float eps, int step, float ema_decay, int ema_mode,
                             const float* scale4_dev, void* stream) {
  const int rc = check_adam_args("sr3_adam_ema_step_scaled", params, grads, exp_avg, exp_avg_sq, ema, n, step, ema_decay, ema_mode, true, scale4_dev);
  return rc ? rc : adam_pass(params, grads, exp_avg, exp_avg_sq, ema, n, lr, beta1, beta2, eps, step, ema_decay, ema_mode, scale4_dev,
                             static_cast<hipStream_t>(stream));
}

size_t sr3_grad_norm_scratch_bytes(size_t n) { return grad_norm_scratch_bytes(n); }

int sr3_grad_norm(const float* grads, size_t n, float max_norm, void* scratch, size_t scratch_bytes, float* out4_dev,
                  void* stream) {
  if (!grads) { set_error("sr3_grad_norm: grads is NULL"); return SR3_E_BADARG; }
  if (!scratch) { set_error("sr3_grad_norm: scratch is NULL"); return SR3_E_BADARG; }
  if (!out4_dev) { set_error("sr3_grad_norm: out4_dev is NULL"); return SR3_E_BADARG; }
  if (n & 3) { set_error("sr3_grad_norm: n %zu is not a multiple of 4", n); return SR3_E_BADARG; }
  const int rc = check_norm_args("sr3_grad_norm", n, max_norm, scratch, scratch_bytes, true, (uintptr_t)grads | (uintptr_t)out4_dev,
                                 "grads / out4_dev");
  return rc ? rc : grad_norm(grads, n, max_norm, static_cast<double*>(scratch), out4_dev, static_cast<hipStream_t>(stream));
}

int sr3_grad_accumulate(float* acc, const float* g, size_t n, int first, float max_norm, void* scratch, size_t scratch_bytes,
                        float* out4_dev, void* stream) {
  if (!acc) { set_error("sr3_grad_accumulate: acc is NULL"); return SR3_E_BADARG; }
  if (!g) { set_error("sr3_grad_accumulate: g is NULL"); return SR3_E_BADARG; }
  if (n & 3) { set_error("sr3_grad_accumulate: n %zu is not a multiple of 4", n); return SR3_E_BADARG; }
  // with out4_dev the norm of the result rides along: its scratch is needed
  if (out4_dev && !scratch) { set_error("sr3_grad_accumulate: scratch is NULL with out4_dev given"); return SR3_E_BADARG; }
  const int rc = check_norm_args("sr3_grad_accumulate", n, max_norm, scratch, scratch_bytes, out4_dev != nullptr,
                                 (uintptr_t)acc | (uintptr_t)g | (uintptr_t)out4_dev, "acc / g / out4_dev");
  return rc ? rc : grad_accumulate(acc, g, n, first != 0, max_norm, static_cast<double*>(scratch), out4_dev, static_cast<hipStream_t>(stream));
}

}  // extern "C"
