// Backward-pass helpers of the training step (DDPM.optimize_parameters, model/model.py:48-58:
// p_losses -> backward -> Adam), HBM-bound: GroupNorm+SiLU backward (reduce / fold / apply),
// gradient routing through the virtual concat / residual / nearest-upsample / stride-2 views,
// weight re-layout for the data-gradient convolutions, bias / FiLM gradient sums and the L1 loss.
// The optimizer's passes (Adam, gradient norm) are in optim.hip; the contractions (dgrad, wgrad, attention backward) live in
// conv3x3_halo.hip / conv_igemm.hip (reused with transformed weights), wgrad.hip and
// attention_bwd.hip.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "conv_prologue.h"
#include "sr3_common.h"
#include "train.h"

namespace sr3 {

double meant_double(float f) {
  char buf[40];
  for (int prec = 1; prec <= 9; ++prec) {
    snprintf(buf, sizeof(buf), "%.*g", prec, (double)f);
    const double d = strtod(buf, nullptr);
    if ((float)d == f) return d;
  }
  return (double)f;
}

// ---------------------------------------------------------------------------------------------
// T1: activation backward + partial sums.  For the virtual concat x = (x0|x1) with u = x*scale+shift,
// a = silu(u) (act 2) or a = u (act 1):  du = dA * act'(u)  is written in place of dA, and per
// (image, channel) partials {sum du, sum du*xhat} go to part[B][T][C][2] (xhat = (x-mean)*rstd).
// Same geometry as k_chan_stats.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_act_bwd_reduce(float* __restrict__ dA, const float* __restrict__ x0,
                                                         const float* __restrict__ x1, int C0, int C1, int HW,
                                                         int LQ, int pix_per_block, const float* __restrict__ ss,
                                                         const float* __restrict__ mr, int groups, int act,
                                                         unsigned drop_seed, unsigned drop_thresh, float drop_scale,
                                                         double* __restrict__ part, float* __restrict__ aout) {
  __shared__ double red[256 * 8];
  const int tid = threadIdx.x;
  const int C = C0 + C1;
  const int nq = C >> 2;
  const int ql = tid % LQ, pl = tid / LQ, PP = 256 / LQ;
  const int q = blockIdx.y * LQ + ql;
  const int b = blockIdx.z;
  const int T = gridDim.x;
  const int p0 = blockIdx.x * pix_per_block;
  const int p1 = min(HW, p0 + pix_per_block);
  const int cpg = C / groups;
  double s[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
  if (q < nq) {
    const int c = q * 4;
    const auto src = concat_quad(x0, C0, x1, C1, c);
    float sc[4], sh[4], mu[4], rs[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      sc[e] = ss[((size_t)b * C + c + e) * 2];
      sh[e] = ss[((size_t)b * C + c + e) * 2 + 1];
      const int g = (c + e) / cpg;
      mu[e] = mr[((size_t)b * groups + g) * 2];
      rs[e] = mr[((size_t)b * groups + g) * 2 + 1];
    }
    for (int p = p0 + pl; p < p1; p += PP) {
      const size_t pix = (size_t)b * HW + p;
      f32x4 g4 = *reinterpret_cast<const f32x4*>(dA + pix * C + c);
      const f32x4 xv = *reinterpret_cast<const f32x4*>(src.base + pix * src.C + src.c);
      f32x4 a4;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float du = g4[e];
        float dm = 1.0f;
        // mirrors drop_index(pix, C, c, e) of conv_prologue.h, spelled out: behind the call this loop's set-up is scheduled differently
        if (drop_thresh != 0) { dm = drop_mask(drop_seed, (unsigned)(pix * C + c + e), drop_thresh, drop_scale); du *= dm; }
        const float u = fmaf(xv[e], sc[e], sh[e]);
        float av = u;
        if (act == 2) {
          const float sg = SR3_SIGMOID(u);     // (av below: silu_libm(u), sharing the sigmoid with the derivative)
          du *= sg * (1.0f + u * (1.0f - sg));
          av = u * sg;
        }
        if (drop_thresh != 0) av *= dm;
        a4[e] = av;
        g4[e] = du;
        const double xh = ((double)xv[e] - (double)mu[e]) * (double)rs[e];
        s[e] += (double)du;
        s2[e] += (double)du * xh;
      }
      *reinterpret_cast<f32x4*>(dA + pix * C + c) = g4;
      // the activated (and dropped) conv input, for the weight gradient that follows: the values k_apply_act writes, without its pass over x
      if (aout) *reinterpret_cast<f32x4*>(aout + pix * C + c) = a4;
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) { red[tid * 8 + e] = s[e]; red[tid * 8 + 4 + e] = s2[e]; }
  __syncthreads();
  if (pl == 0 && q < nq) {
    for (int k = 1; k < PP; ++k) {
#pragma unroll
      for (int e = 0; e < 4; ++e) { s[e] += red[(k * LQ + ql) * 8 + e]; s2[e] += red[(k * LQ + ql) * 8 + 4 + e]; }
    }
    double* o = part + (((size_t)b * T + blockIdx.x) * C + q * 4) * 2;
#pragma unroll
    for (int e = 0; e < 4; ++e) { o[2 * e] = s[e]; o[2 * e + 1] = s2[e]; }
  }
}

// The factor a scale-shift modulation puts on gamma_c for image b (fold_modulate, small_kernels.hip): m = 1 + s as the forward rounded
// it.  mod_b: image b's scales [C] then shifts [C].  The MOD instantiations of the kernels below use gamma_c m where the plain ones use
// gamma_c, in double; the plain ones read neither mod nor mod_stride
__device__ __forceinline__ double mod_factor(const float* __restrict__ mod_b, int c) { return (double)add_rn(1.0f, mod_b[c]); }

// T2a: per (image, group): S1 = sum_c gamma_c * A_c, S2 = sum_c gamma_c * B_c  -> gs[B][G][2] (double)
template <bool MOD>
__global__ __launch_bounds__(64) void k_gn_bwd_group(const double* __restrict__ part, int C, int T, int groups,
                                                      const float* __restrict__ gamma, double* __restrict__ gs,
                                                      const float* __restrict__ mod, int mod_stride) {
  const int b = blockIdx.x / groups, g = blockIdx.x - b * groups;
  const int cpg = C / groups;
  const int lane = threadIdx.x;
  double a = 0.0, bb = 0.0;
  for (int idx = lane; idx < cpg * T; idx += 64) {
    const int k = idx / T, t = idx - k * T;
    const int c = g * cpg + k;
    const double* q = part + (((size_t)b * T + t) * C + c) * 2;
    double gm = (double)gamma[c];
    if constexpr (MOD) gm *= mod_factor(mod + (size_t)b * mod_stride, c);
    a += gm * q[0]; bb += gm * q[1];
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { a += __shfl_xor(a, m); bb += __shfl_xor(bb, m); }
  if (lane == 0) { gs[((size_t)b * groups + g) * 2] = a; gs[((size_t)b * groups + g) * 2 + 1] = bb; }
}

// T2b / T8: per channel: out0[c] (+)= sum_{b,t} part[..][c][0] ; out1[c] (+)= sum part[..][c][1]  (either may be null)
// MOD: image b's partials weighted by mod_factor (the gradients of gamma and beta under a scale-shift modulation); a factor of exactly
// 1 -- a zero scale row -- gives the plain sums' bits
template <bool MOD>
__global__ __launch_bounds__(64) void k_part_colsum(const double* __restrict__ part, int B, int C, int T,
                                                     float* __restrict__ out0, float* __restrict__ out1,
                                                     const float* __restrict__ mod, int mod_stride) {
  const int c = blockIdx.x;
  const int lane = threadIdx.x;
  double a = 0.0, bb = 0.0;
  for (int idx = lane; idx < B * T; idx += 64) {
    const double* q = part + ((size_t)idx * C + c) * 2;
    if constexpr (MOD) {
      const double m = mod_factor(mod + (size_t)(idx / T) * mod_stride, c);
      a += m * q[0]; bb += m * q[1];
    } else {
      a += q[0]; bb += q[1];
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { a += __shfl_xor(a, m); bb += __shfl_xor(bb, m); }
  if (lane == 0) {
    if (out0) out0[c] = (float)a;
    if (out1) out1[c] = (float)bb;
  }
}

// per (image, channel): out[b*stride + c] = sum_t part[b][t][c][0]   (FiLM gradient rows)
__global__ __launch_bounds__(256) void k_part_imgsum(const double* __restrict__ part, int B, int C, int T,
                                                      float* __restrict__ out, int stride) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= B * C) return;
  const int b = idx / C, c = idx - b * C;
  double a = 0.0;
  for (int t = 0; t < T; ++t) a += part[(((size_t)b * T + t) * C + c) * 2];
  out[(size_t)b * stride + c] = (float)a;
}

// The gradients of a scale-shift modulation's rows, from the partials {sum du, sum du xhat}: per (image, channel), in double, rounded once,
//   d shift = sum_t part[0] ;  d scale = sum du GN(x) = gamma_c sum_t part[1] + beta_c sum_t part[0]      (GN(x) = xhat gamma + beta)
// into dmod_b[c] (scales) and dmod_b[C + c] (shifts), the layout of mod
__global__ __launch_bounds__(256) void k_part_modgrad(const double* __restrict__ part, int B, int C, int T, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, float* __restrict__ dmod, int mod_stride) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= B * C) return;
  const int b = idx / C, c = idx - b * C;
  double a = 0.0, bb = 0.0;
  for (int t = 0; t < T; ++t) {
    const double* q = part + (((size_t)b * T + t) * C + c) * 2;
    a += q[0]; bb += q[1];
  }
  float* o = dmod + (size_t)b * mod_stride;
  o[c] = (float)((double)gamma[c] * bb + (double)beta[c] * a);
  o[C + c] = (float)a;
}

// T3: dx(src) += rstd * (gamma*du - (S1 + xhat*S2)/n), routed to the two concat sources.
// The two terms cancel heavily (GroupNorm's backward projects the x-hat and the constant component out of du), so the
// per-(image, group) coefficients stay in double and the expression is evaluated in double and rounded once -- what
// torch's CPU GroupNorm backward does (acc_type<float> = double for its c1 / c2 / c3 coefficients).  With fp32
// coefficients the rounding of S2 is a perturbation along x-hat that is coherent over a whole (image, group) and is
// amplified by sqrt(B H W) in the weight gradient of the conv that produced x (measured 1.2e-4 normwise at B = 64).
// GAMMA: the plain pointer, or GammaMod -- gamma_c mod_factor stands where gamma_c does, in double.  (A type in gamma's own slot, not
// arguments behind the others as in the kernels above: this kernel's grid-stride loop reads the launch dimensions, which sit behind
// the explicit arguments, so the plain instantiation keeps its argument block -- and its instruction stream -- only this way)
struct GammaMod { const float* gamma; const float* mod; int mod_stride; };
__device__ __forceinline__ double gamma_at(const float* __restrict__ gamma, int, int c) { return (double)gamma[c]; }
__device__ __forceinline__ double gamma_at(const GammaMod& g, int b, int c) { return (double)g.gamma[c] * mod_factor(g.mod + (size_t)b * g.mod_stride, c); }
template <class GAMMA>
__global__ __launch_bounds__(256) void k_gn_bwd_apply(const float* __restrict__ du, const float* __restrict__ x0,
                                                       const float* __restrict__ x1, int C0, int C1, int HW,
                                                       const float* __restrict__ mr, const double* __restrict__ gs,
                                                       int groups, const GAMMA gamma,
                                                       float* __restrict__ dx0, float* __restrict__ dx1,
                                                       size_t total4, int acc0, int acc1) {
  const int C = C0 + C1;
  const int nq = C >> 2;
  const int cpg = C / groups;
  const double inv_n = 1.0 / ((double)HW * (double)cpg);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (size_t)gridDim.x * blockDim.x) {
    const size_t pix = i / nq;
    const int c = (int)(i - pix * nq) * 4;
    const int b = (int)(pix / HW);
    const auto src = concat_quad(x0, C0, x1, C1, c);
    const auto dst = concat_quad(dx0, C0, dx1, C1, c);
    const f32x4 g4 = *reinterpret_cast<const f32x4*>(du + pix * C + c);
    const f32x4 xv = *reinterpret_cast<const f32x4*>(src.base + pix * src.C + src.c);
    // (acc == 0: this is the first contribution to that gradient tensor in the backward walk -- a plain store, the mirror is not zeroed)
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (dst.second ? acc1 : acc0) o = *reinterpret_cast<const f32x4*>(dst.base + pix * dst.C + dst.c);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int g = (c + e) / cpg;
      const double mu = (double)mr[((size_t)b * groups + g) * 2], rs = (double)mr[((size_t)b * groups + g) * 2 + 1];
      const double S1 = gs[((size_t)b * groups + g) * 2], S2 = gs[((size_t)b * groups + g) * 2 + 1];
      const double xh = ((double)xv[e] - mu) * rs;
      o[e] += (float)(rs * (gamma_at(gamma, b, c + e) * (double)g4[e] - (S1 + xh * S2) * inv_n));
    }
    *reinterpret_cast<f32x4*>(dst.base + pix * dst.C + dst.c) = o;
  }
}

// T4: route a gradient over the virtual concat to its sources: dst(src) += g[.., c]; `ups` sums the
// 2x2 children of every source pixel (backward of the nearest x2 upsample, unet.py:61).
__global__ __launch_bounds__(256) void k_grad_route(const float* __restrict__ g, int C0, int C1, int B, int Hs, int Ws,
                                                     int ups, float* __restrict__ d0, float* __restrict__ d1,
                                                     size_t total4, int acc0, int acc1) {
  const int C = C0 + C1;
  const int nq = C >> 2;
  const int Wg = Ws << ups;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (size_t)gridDim.x * blockDim.x) {
    const size_t pix = i / nq;                  // source pixel (b, y, x)
    const int c = (int)(i - pix * nq) * 4;
    const auto dst = concat_quad(d0, C0, d1, C1, c);
    f32x4 acc;
    if (ups) {
      const int x = (int)(pix % Ws);
      const size_t by = pix / Ws;               // b*Hs + y
      const int y = (int)(by % Hs);
      const size_t bb = by / Hs;
      const size_t base = ((bb * (Hs * 2) + 2 * y) * Wg + 2 * x);
      acc = *reinterpret_cast<const f32x4*>(g + base * C + c);
      acc += *reinterpret_cast<const f32x4*>(g + (base + 1) * C + c);
      acc += *reinterpret_cast<const f32x4*>(g + (base + Wg) * C + c);
      acc += *reinterpret_cast<const f32x4*>(g + (base + Wg + 1) * C + c);
    } else {
      acc = *reinterpret_cast<const f32x4*>(g + pix * C + c);
    }
    f32x4 o = acc;
    if (dst.second ? acc1 : acc0) o += *reinterpret_cast<const f32x4*>(dst.base + pix * dst.C + dst.c);
    *reinterpret_cast<f32x4*>(dst.base + pix * dst.C + dst.c) = o;
  }
}

// T5: zero insertion for the stride-2 data gradient: z[b][2oh][2ow] = g[b][oh][ow], rest 0 (z pre-zeroed)
__global__ __launch_bounds__(256) void k_zero_insert(const float* __restrict__ g, int C, int Ho, int Wo,
                                                      float* __restrict__ z, size_t total4) {
  const int nq = C >> 2;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (size_t)gridDim.x * blockDim.x) {
    const size_t pix = i / nq;
    const int c = (int)(i - pix * nq) * 4;
    const int ow = (int)(pix % Wo);
    const size_t bo = pix / Wo;
    const int oh = (int)(bo % Ho);
    const size_t b = bo / Ho;
    const size_t zp = (b * (2 * Ho) + 2 * oh) * (2 * Wo) + 2 * ow;
    *reinterpret_cast<f32x4*>(z + zp * C + c) = *reinterpret_cast<const f32x4*>(g + pix * C + c);
  }
}

// T6: weights of the data-gradient conv: wt[c][taps-1-tap][n] = w[n][tap][c]   (w: [Cout][taps][Cin])
// CoutP >= Cout pads the new K dimension with zeros (Cout = 3 -> 4 for the output Block).
__global__ __launch_bounds__(256) void k_w_flip_transpose(const float* __restrict__ w, int Cout, int taps, int Cin,
                                                           int CoutP, float* __restrict__ wt) {
  const size_t total = (size_t)Cin * taps * CoutP;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int n = (int)(i % CoutP);
    const size_t r = i / CoutP;
    const int tp = (int)(r % taps);
    const int c = (int)(r / taps);
    wt[i] = n < Cout ? w[((size_t)n * taps + (taps - 1 - tp)) * Cin + c] : 0.f;
  }
}

// T11: the loss of one step and its gradient w.r.t. the network's output, written NHWC with the channel dim padded to CP -- ONE kernel
// template, k_loss_grad<KIND, FORM> (below), over ONE lane, ONE block reduction and ONE launch (objective_loss_grad).
// THE lane: rho(d) is added to `acc` in double and g = -ws rho'(d) returned, with rho = |d| (KIND 0: nn.L1Loss(reduction='sum'), what
// define_G configures; rho' = sign, 0 at 0), d^2 (1: nn.MSELoss(reduction='sum'), loss_type 'l2'; 2d) or Huber(delta) (2: d^2 / 2 inside
// |d| <= delta, delta (|d| - delta / 2) outside, rho' = clamp(d, -delta, delta)); ws = weight * scale
template <int KIND>
__device__ __forceinline__ float loss_lane(float d, float ws, float delta, double& acc) {
  if (KIND == LOSS_L2) {
    acc += (double)d * (double)d;
    return -2.f * d * ws;
  }
  if (KIND == LOSS_HUBER) {
    const double a = (double)fabsf(d), dl = (double)delta;
    acc += a <= dl ? 0.5 * a * a : dl * (a - 0.5 * dl);
    return -fminf(fmaxf(d, -delta), delta) * ws;
  }
  acc += (double)fabsf(d);
  return d > 0.f ? -ws : (d < 0.f ? ws : 0.f);
}
// THE block reduction of the loss kernels: the 256 threads' doubles summed in a fixed tree, thread 0 stores the sum.  Ends behind a
// barrier every thread has passed, so `red` can be reused at once
__device__ __forceinline__ void block_sum_256(double* red, double v, double* out) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int k = 128; k >= 1; k >>= 1) {
    if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = red[0];
}
// The three forms of the kernel.  Behaviour is bits, so each keeps its own expression of d and its own grouping of the double sum:
//   PLAIN      sr3_train_step's objective (target z, weight 1, L1 / L2): d = z - e, every channel's rho added straight into the thread's sum
//   OBJECTIVE  T11b, v- / x0-prediction, Min-SNR weights, Huber: per image b the regression target is ta[b] z + tb[b] hr
//              and the weight w[b] (NULL tables: target z, weight 1; hr is read only with tb):  d = (ta z + tb hr) - e, a pixel's channels
//              summed first and weighted once.  With NULL tables d differs from PLAIN's in the sign of a zero (-0.f + 0.f is +0.f), which
//              for L2 reaches g; the sum differs in its rounding (tests/test_gpu_loss_bits.py pins both)
//   HYBRID     T11c, OBJECTIVE on the prediction rows plus lambda L_vlb on the variance rows
// T11c: the hybrid loss of a learned reverse-process variance (Nichol & Dhariwal 2021).  e is [B, 2 Cc, HW]: channels
// 0 .. Cc - 1 the prediction, under the OBJECTIVE form's lanes (the same d, rho, g: one piece of code); channels Cc ..
// 2 Cc - 1 the raw variance head v.  Per image the scalars of the drawn step (train.h: HYB_*).  Per element, all fp32:
//   x0^ = a x_t - b out (no clamp) ; mu_theta = c1 x0^ + c2 x_t, a constant here: no L_vlb gradient reaches the prediction lanes
//   f = (v + 1) / 2 ; lv = f log beta + (1 - f) log beta~                         log sigma_theta^2
//   not last:  vlb = KL(N(mu_q, beta~) || N(mu_theta, e^lv)) / ln 2,  mu_q - mu_theta = c1 (x0 - x0^)
//   last:      vlb = -log2 of the mass N(mu_theta, e^lv) puts on the bin x0 +- 1/255 (open below -0.999 and above 0.999), with
//              Phi(u) = (1 + tanh(sqrt(2 / pi) (u + 0.044715 u^3))) / 2 and logs of max(., 1e-12)
//   g lane Cc + c = lambda scale d vlb / d v, in closed form; lanes >= 2 Cc are 0
// loss_part[block] = sum w rho(d) + lambda sum vlb, loss_part[gridDim.x + block] = sum vlb: double partials, fixed order, no atomics.
// vw (sr3_train_step_ex3's vlb_weight; null: 1): per image, lambda vw[b] stands where lambda does -- in the variance lanes and in the
// first sum; the second sum stays the plain sum of vlb.
struct VlbScal { float a, b, c1, c2, lb, lt; bool last; };
__device__ __forceinline__ float approx_cdf(float u, float* pdf) {
  constexpr float K = 0.7978845608028654f;      // sqrt(2 / pi)
  const float th = tanhf(K * (u + 0.044715f * u * u * u));
  *pdf = 0.5f * (1.f - th * th) * K * (1.f + 3.f * 0.044715f * u * u);
  return 0.5f * (1.f + th);
}
__device__ __forceinline__ float vlb_elem(const VlbScal& k, float x0, float xt, float o, float v, float* dv) {
  constexpr float RLN2 = 1.4426950408889634f;
  const float x0h = k.a * xt - k.b * o;
  const float f = 0.5f * (v + 1.f);
  const float lv = f * k.lb + (1.f - f) * k.lt;
  const float dlv = 0.5f * (k.lb - k.lt);      // d lv / d v
  if (!k.last) {
    const float d = k.c1 * (x0 - x0h);
    const float r = expf(k.lt - lv), q = d * d * expf(-lv);
    *dv = 0.5f * (1.f - r - q) * dlv * RLN2;
    return 0.5f * (-1.f + lv - k.lt + r + q) * RLN2;
  }
  const float cx = x0 - (k.c1 * x0h + k.c2 * xt), inv = expf(-0.5f * lv);
  const float up = inv * (cx + 1.f / 255.f), um = inv * (cx - 1.f / 255.f);
  float pp, pm;
  const float cp = approx_cdf(up, &pp), cm = approx_cdf(um, &pm);
  // d u / d lv = -u / 2 for either bound; a clamped log has no gradient
  float arg, darg;
  if (x0 < -0.999f) { arg = cp; darg = pp * (-0.5f * up); }
  else if (x0 > 0.999f) { arg = 1.f - cm; darg = pm * (0.5f * um); }
  else { arg = cp - cm; darg = pp * (-0.5f * up) + pm * (0.5f * um); }
  const bool open = arg >= 1e-12f;
  *dv = open ? -(darg / arg) * dlv * RLN2 : 0.f;
  return -logf(open ? arg : 1e-12f) * RLN2;
}
enum { LOSS_PLAIN = 0, LOSS_OBJECTIVE, LOSS_HYBRID };
template <int KIND, int FORM>
__global__ __launch_bounds__(256) void k_loss_grad(const LossTensors t, const Objective o, int B, int Cc, int HW, int CP, float scale) {
  __shared__ double red[256];
  double s = 0.0, sv = 0.0;
  const int Ce = FORM == LOSS_HYBRID ? 2 * Cc : Cc;      // channels of e
  const size_t total = (size_t)B * HW;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / HW, p = i - b * HW;
    float az = 1.f, ax = 0.f, wb = 1.f, lam = 0.f;
    VlbScal k = {};
    if (FORM != LOSS_PLAIN) {
      az = o.tgt_z ? o.tgt_z[b] : 1.f; ax = o.tgt_x0 ? o.tgt_x0[b] : 0.f; wb = o.weight ? o.weight[b] : 1.f;
    }
    if (FORM == LOSS_HYBRID) {
      lam = o.vlb_w ? o.lambda * o.vlb_w[b] : o.lambda;      // (vw: a per-image weight of L_vlb; null: lambda as it is -- the same operations)
      const float* hs = o.hyb + b * HYB_STRIDE;
      k = {hs[HYB_A], hs[HYB_B], hs[HYB_C1], hs[HYB_C2], hs[HYB_LOG_BETA], hs[HYB_LOG_BETA_TILDE], hs[HYB_LAST] != 0.f};
    }
    const float ws = FORM == LOSS_PLAIN ? scale : wb * scale, ls = lam * scale;
    double sp = 0.0, vp = 0.0;                  // this pixel's sums of rho(d) and of vlb: weighted once
    for (int c = 0; c < CP; ++c) {
      float gv = 0.f;
      if (c < Cc) {
        const size_t ie = (b * Ce + c) * HW + p, ix = (b * Cc + c) * HW + p;
        if (FORM == LOSS_PLAIN) gv = loss_lane<KIND>(t.z[ix] - t.e[ie], ws, o.huber_delta, s);
        else gv = loss_lane<KIND>((az * t.z[ix] + (o.tgt_x0 ? ax * t.hr[ix] : 0.f)) - t.e[ie], ws, o.huber_delta, sp);
      } else if (FORM == LOSS_HYBRID && c < 2 * Cc) {
        const size_t ix = (b * Cc + (c - Cc)) * HW + p;
        float dv;
        vp += (double)vlb_elem(k, t.hr[ix], t.xt[ix], t.e[(b * Ce + (c - Cc)) * HW + p], t.e[(b * Ce + c) * HW + p], &dv);
        gv = ls * dv;
      }
      t.g_nhwc[i * CP + c] = gv;
    }
    if (FORM == LOSS_OBJECTIVE) s += (double)wb * sp;
    if (FORM == LOSS_HYBRID) { s += (double)wb * sp + (double)lam * vp; sv += vp; }
  }
  block_sum_256(red, s, t.loss_part + blockIdx.x);
  if (FORM == LOSS_HYBRID) block_sum_256(red, sv, t.loss_part + gridDim.x + blockIdx.x);
}
__global__ __launch_bounds__(64) void k_sum_parts(const double* __restrict__ part, int n, float* __restrict__ out) {
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 64) s += part[i];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
  if (threadIdx.x == 0) out[0] = (float)s;
}

// NCHW (C <= 4) -> NHWC with the channel dim padded to CP (input of the first conv for its wgrad)
__global__ __launch_bounds__(256) void k_nchw_to_nhwc_pad(const float* __restrict__ a, int Ca, const float* __restrict__ b2,
                                                           int Cb, int HW, int CP, float* __restrict__ out, size_t total) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t bi = i / HW, p = i - bi * HW;
    for (int c = 0; c < CP; ++c) {
      float v = 0.f;
      if (c < Ca) v = a[(bi * Ca + c) * HW + p];
      else if (c < Ca + Cb) v = b2[(bi * Cb + (c - Ca)) * HW + p];
      out[i * CP + c] = v;
    }
  }
}

// materialise the activated conv input a = dropout(act(x * scale + shift)) over the virtual concat
// (input of the weight-gradient GEMM, so that it needs no per-tap recomputation)
__global__ __launch_bounds__(256) void k_apply_act(const float* __restrict__ x0, const float* __restrict__ x1, int C0,
                                                    int C1, int HW, const float* __restrict__ ss, int act,
                                                    unsigned drop_seed, unsigned drop_thresh, float drop_scale,
                                                    float* __restrict__ out, size_t total4) {
  const int C = C0 + C1;
  const int nq = C >> 2;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (size_t)gridDim.x * blockDim.x) {
    const size_t pix = i / nq;
    const int c = (int)(i - pix * nq) * 4;
    const int b = (int)(pix / HW);
    const auto src = concat_quad(x0, C0, x1, C1, c);
    f32x4 v = *reinterpret_cast<const f32x4*>(src.base + pix * src.C + src.c);
    const f32x4 s0 = *reinterpret_cast<const f32x4*>(ss + ((size_t)b * C + c) * 2);
    const f32x4 s1 = *reinterpret_cast<const f32x4*>(ss + ((size_t)b * C + c) * 2 + 4);
    v = gn_affine4(v, s0, s1);
    if (act == 2) v = silu4_libm(v);
    if (drop_thresh != 0) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] *= drop_mask(drop_seed, drop_index(pix, C, c, e), drop_thresh, drop_scale);
    }
    *reinterpret_cast<f32x4*>(out + pix * C + c) = v;
  }
}

// ---- host wrappers --------------------------------------------------------------------------------
static void stats_geometry(int B, int HW, int C, int* LQ_, int* cblocks_, int* ppb_, int* slices_) {
  const int nq = C >> 2;
  int LQ = 1;
  while (LQ < nq && LQ < 64) LQ <<= 1;
  const int cblocks = (nq + LQ - 1) / LQ;
  const int PP = 256 / LQ;
  long base_blocks = (long)cblocks * B;
  long want = 2048 / (base_blocks > 0 ? base_blocks : 1);
  if (want < 1) want = 1;
  if (want > 64) want = 64;
  long max_slices = (HW + PP - 1) / PP;
  if (want > max_slices) want = max_slices;
  int ppb = (int)((HW + want - 1) / want);
  ppb = ((ppb + PP - 1) / PP) * PP;
  *LQ_ = LQ; *cblocks_ = cblocks; *ppb_ = ppb; *slices_ = (HW + ppb - 1) / ppb;
}

int act_bwd(float* dA, const float* x0, const float* x1, int C0, int C1, int B, int HW, const float* ss, const float* mr,
            int groups, int act, const float* gamma, double* part, double* gs, float* dgamma, float* dbeta, float* dx0,
            float* dx1, hipStream_t st, unsigned drop_seed, unsigned drop_thresh, float drop_scale, float* aout, bool acc0, bool acc1,
            const ModBwd* md) {
  const int C = C0 + C1;
  if ((C0 & 3) || (C1 & 3)) { set_error("act_bwd: channels %% 4"); return SR3_E_UNSUPPORTED; }
  int LQ, cblocks, ppb, T;
  stats_geometry(B, HW, C, &LQ, &cblocks, &ppb, &T);
  hipLaunchKernelGGL(k_act_bwd_reduce, dim3(T, cblocks, B), dim3(256), 0, st, dA, x0, x1, C0, C1, HW, LQ, ppb, ss, mr,
                     groups, act, drop_seed, drop_thresh, drop_scale, part, aout);
  SR3_LAUNCH_CHECK("k_act_bwd_reduce");
  // md: the GroupNorm was folded under a scale-shift modulation (the MOD instantiations), whose rows' gradients come out of the same partials
  const float* mod = md ? md->mod : nullptr;
  const int mstride = md ? md->stride : 0;
  hipLaunchKernelGGL(md ? k_gn_bwd_group<true> : k_gn_bwd_group<false>, dim3(B * groups), dim3(64), 0, st, part, C, T, groups, gamma, gs, mod, mstride);
  SR3_LAUNCH_CHECK("k_gn_bwd_group");
  hipLaunchKernelGGL(md ? k_part_colsum<true> : k_part_colsum<false>, dim3(C), dim3(64), 0, st, part, B, C, T, dbeta, dgamma, mod, mstride);
  SR3_LAUNCH_CHECK("k_part_colsum");
  if (md) {
    hipLaunchKernelGGL(k_part_modgrad, dim3((B * C + 255) / 256), dim3(256), 0, st, part, B, C, T, gamma, md->beta, md->dmod, mstride);
    SR3_LAUNCH_CHECK("k_part_modgrad");
  }
  const size_t total4 = (size_t)B * HW * (C >> 2);
  if (md) hipLaunchKernelGGL(k_gn_bwd_apply<GammaMod>, dim3(ew_blocks(total4)), dim3(256), 0, st, dA, x0, x1, C0, C1, HW, mr, gs, groups,
                             GammaMod{gamma, mod, mstride}, dx0, dx1, total4, acc0 ? 1 : 0, acc1 ? 1 : 0);
  else hipLaunchKernelGGL(k_gn_bwd_apply<const float* __restrict__>, dim3(ew_blocks(total4)), dim3(256), 0, st, dA, x0, x1, C0, C1, HW, mr, gs, groups,
                          gamma, dx0, dx1, total4, acc0 ? 1 : 0, acc1 ? 1 : 0);
  SR3_LAUNCH_CHECK("k_gn_bwd_apply");
  return SR3_OK;
}
size_t act_bwd_part_bytes(int B, int HW, int C) {
  int LQ, cb, ppb, T;
  stats_geometry(B, HW, C, &LQ, &cb, &ppb, &T);
  return (size_t)B * T * C * 2 * sizeof(double);
}

int apply_act(const float* x0, const float* x1, int C0, int C1, int B, int HW, const float* ss, int act, unsigned drop_seed,
              unsigned drop_thresh, float drop_scale, float* out, hipStream_t st) {
  const size_t total4 = (size_t)B * HW * ((C0 + C1) >> 2);
  hipLaunchKernelGGL(k_apply_act, dim3(ew_blocks(total4)), dim3(256), 0, st, x0, x1, C0, C1, HW, ss, act, drop_seed,
                     drop_thresh, drop_scale, out, total4);
  SR3_LAUNCH_CHECK("k_apply_act");
  return SR3_OK;
}

int grad_route(const float* g, int C0, int C1, int B, int Hs, int Ws, int ups, float* d0, float* d1, hipStream_t st, bool acc0, bool acc1) {
  const size_t total4 = (size_t)B * Hs * Ws * ((C0 + C1) >> 2);
  hipLaunchKernelGGL(k_grad_route, dim3(ew_blocks(total4)), dim3(256), 0, st, g, C0, C1, B, Hs, Ws, ups, d0, d1, total4, acc0 ? 1 : 0, acc1 ? 1 : 0);
  SR3_LAUNCH_CHECK("k_grad_route");
  return SR3_OK;
}
int zero_insert(const float* g, int B, int Ho, int Wo, int C, float* z, hipStream_t st) {
  SR3_HIP(hipMemsetAsync(z, 0, (size_t)B * 4 * Ho * Wo * C * sizeof(float), st));
  const size_t total4 = (size_t)B * Ho * Wo * (C >> 2);
  hipLaunchKernelGGL(k_zero_insert, dim3(ew_blocks(total4)), dim3(256), 0, st, g, C, Ho, Wo, z, total4);
  SR3_LAUNCH_CHECK("k_zero_insert");
  return SR3_OK;
}
int w_flip_transpose(const float* w, int Cout, int taps, int Cin, int CoutP, float* wt, hipStream_t st) {
  const size_t total = (size_t)Cin * taps * CoutP;
  hipLaunchKernelGGL(k_w_flip_transpose, dim3(ew_blocks(total)), dim3(256), 0, st, w, Cout, taps, Cin, CoutP, wt);
  SR3_LAUNCH_CHECK("k_w_flip_transpose");
  return SR3_OK;
}
// bias gradient (sum over images and pixels) and / or FiLM gradient rows (sum over pixels) of g [B,HW,C]
int colsums(const float* g, int B, int HW, int C, double* part, float* dbias, float* dfilm, int film_stride,
            hipStream_t st) {
  int rc = chan_stats(g, B, HW, C, part, st);
  if (rc) return rc;
  const int T = chan_stats_slices(B, HW, C);
  if (dbias) {
    hipLaunchKernelGGL(k_part_colsum<false>, dim3(C), dim3(64), 0, st, part, B, C, T, dbias, (float*)nullptr, (const float*)nullptr, 0);
    SR3_LAUNCH_CHECK("k_part_colsum");
  }
  if (dfilm) {
    hipLaunchKernelGGL(k_part_imgsum, dim3((B * C + 255) / 256), dim3(256), 0, st, part, B, C, T, dfilm, film_stride);
    SR3_LAUNCH_CHECK("k_part_imgsum");
  }
  return SR3_OK;
}
// The refusals of the objective arguments of sr3_train_step_ex / sr3_loss_grad_f32 under the entry's own name (min_kind: -1 where a
// plan's loss_l2 can stand in).  Nothing has been launched when this returns non-zero.
int check_objective_args(const char* who, const float* tgt_z, const float* tgt_x0, const float* weight, int loss_kind, int min_kind,
                         float huber_delta) {
  const int given = (tgt_z != nullptr) + (tgt_x0 != nullptr) + (weight != nullptr);
  if (given != 0 && given != 3) { set_error("%s: tgt_z / tgt_x0 / weight must be all NULL or all given (%d of 3 are)", who, given); return SR3_E_BADARG; }
  if (loss_kind < min_kind || loss_kind > LOSS_HUBER) { set_error("%s: loss_kind %d is outside %d..2", who, loss_kind, min_kind); return SR3_E_BADARG; }
  if (loss_kind == LOSS_HUBER && !(isfinite(huber_delta) && huber_delta > 0.f)) {
    set_error("%s: huber_delta %g must be finite and > 0", who, (double)huber_delta);
    return SR3_E_BADARG;
  }
  return SR3_OK;
}
// THE launch of the loss kernels, and THE place that picks the form.  A variance head (o.hyb): the hybrid form.  Otherwise plain against
// general: target z, weight 1 and L1 / L2 is the plain form as it always was; everything else the objective's form on the same grid.
// Then k_sum_parts over each run of block partials that has a destination (loss_out; the hybrid form's vlb_out, which may be null)
int objective_loss_grad(const LossTensors& t, const Objective& o, int B, int Cc, int HW, int CP, float scale, hipStream_t st) {
  using Kernel = void (*)(const LossTensors, const Objective, int, int, int, int, float);
  static constexpr Kernel kernels[3][3] = {
      {k_loss_grad<LOSS_L1, LOSS_PLAIN>, k_loss_grad<LOSS_L2, LOSS_PLAIN>, nullptr},      // (Huber has no plain form)
      {k_loss_grad<LOSS_L1, LOSS_OBJECTIVE>, k_loss_grad<LOSS_L2, LOSS_OBJECTIVE>, k_loss_grad<LOSS_HUBER, LOSS_OBJECTIVE>},
      {k_loss_grad<LOSS_L1, LOSS_HYBRID>, k_loss_grad<LOSS_L2, LOSS_HYBRID>, k_loss_grad<LOSS_HUBER, LOSS_HYBRID>}};
  static const char* const names[3] = {"k_l1_loss_grad", "k_loss_grad", "k_hybrid_loss_grad"};      // (a launch failure names the form as it always did)
  const int form = o.hyb ? LOSS_HYBRID : (!o.tgt_z && o.kind != LOSS_HUBER ? LOSS_PLAIN : LOSS_OBJECTIVE);
  const int blocks = LOSS_GRAD_BLOCKS;
  hipLaunchKernelGGL(kernels[form][o.kind], dim3(blocks), dim3(256), 0, st, t, o, B, Cc, HW, CP, scale);
  SR3_LAUNCH_CHECK(names[form]);
  float* const sums[2] = {t.loss_out, o.hyb ? t.vlb_out : nullptr};
  for (int k = 0; k < 2; ++k) {
    if (!sums[k]) continue;
    hipLaunchKernelGGL(k_sum_parts, dim3(1), dim3(64), 0, st, t.loss_part + k * blocks, blocks, sums[k]);
    SR3_LAUNCH_CHECK("k_sum_parts");
  }
  return SR3_OK;
}
int nchw_to_nhwc_pad(const float* a, int Ca, const float* b, int Cb, int B, int HW, int CP, float* out, hipStream_t st) {
  const size_t total = (size_t)B * HW;
  hipLaunchKernelGGL(k_nchw_to_nhwc_pad, dim3(ew_blocks(total)), dim3(256), 0, st, a, Ca, b, Cb, HW, CP, out, total);
  SR3_LAUNCH_CHECK("k_nchw_to_nhwc_pad");
  return SR3_OK;
}

}  // namespace sr3

// ---- the backward walk's own kernels on caller-owned tensors: each entry checks its arguments, then calls what run_train calls ----
namespace {
int check_gn_bwd_shape(const char* who, int C0, int C1, int B, int HW, int groups) {
  using namespace sr3;
  if (B <= 0 || HW <= 0 || C0 <= 0 || C1 < 0 || groups <= 0) { set_error("%s: batch %d, pixels %d, channels %d | %d and groups %d must be positive (C1 >= 0)", who, B, HW, C0, C1, groups); return SR3_E_BADARG; }
  if ((C0 & 3) || (C1 & 3)) { set_error("%s: channel counts must be multiples of 4 (C0 %d, C1 %d)", who, C0, C1); return SR3_E_UNSUPPORTED; }
  if ((C0 + C1) % groups) { set_error("%s: %d channels do not divide into %d groups", who, C0 + C1, groups); return SR3_E_UNSUPPORTED; }
  if ((double)B * HW * (double)(C0 + C1) >= 2147483647.0) { set_error("%s: tensor exceeds 2^31 elements", who); return SR3_E_UNSUPPORTED; }
  return SR3_OK;
}
}  // namespace

extern "C" size_t sr3_groupnorm_act_bwd_scratch_bytes(int B, int HW, int C, int groups) {
  using namespace sr3;
  if (check_gn_bwd_shape("sr3_groupnorm_act_bwd_scratch_bytes", C, 0, B, HW, groups)) return 0;
  return al256(act_bwd_part_bytes(B, HW, C)) + (size_t)B * groups * 2 * sizeof(double);
}
namespace {
// sr3_groupnorm_act_bwd_f32 (md null) and sr3_groupnorm_act_bwd_mod_f32: one list of checks, then act_bwd
int gn_act_bwd_entry(const char* who, float* dA, const float* x0, int C0, const float* x1, int C1, int B, int HW, const float* ss,
                     const float* mr, int groups, int act, const float* gamma, unsigned drop_seed, float drop_p,
                     float* dgamma, float* dbeta, float* dx0, int acc0, float* dx1, int acc1, float* aout,
                     void* scratch, size_t scratch_bytes, const sr3::ModBwd* md, void* stream) {
  using namespace sr3;
  if (md && (!md->mod || !md->dmod || !md->beta)) { set_error("%s: beta / mod / dmod is NULL", who); return SR3_E_BADARG; }
  if (!dA || !x0 || !ss || !mr || !gamma || !dgamma || !dbeta || !dx0 || !scratch || (C1 > 0 && (!x1 || !dx1))) {
    set_error("%s: dA / x0 / ss / mr / gamma / dgamma / dbeta / dx0 / scratch (or x1 / dx1 with C1 > 0) is NULL", who);
    return SR3_E_BADARG;
  }
  if (const int rc = check_gn_bwd_shape(who, C0, C1, B, HW, groups)) return rc;
  if (act != 1 && act != 2) { set_error("%s: act %d is outside 1..2", who, act); return SR3_E_BADARG; }
  if (!(drop_p >= 0.f && drop_p < 1.f)) { set_error("%s: drop_p out of range", who); return SR3_E_BADARG; }
  if ((uintptr_t)scratch & 7) { set_error("%s: scratch is not 8-byte aligned", who); return SR3_E_ALIGN; }
  const size_t part = al256(act_bwd_part_bytes(B, HW, C0 + C1)), need = part + (size_t)B * groups * 2 * sizeof(double);
  if (scratch_bytes < need) { set_error("%s: scratch too small (%zu < %zu)", who, scratch_bytes, need); return SR3_E_NOMEM; }
  unsigned thresh;
  float scale;
  dropout_consts(drop_p, &thresh, &scale);       // the step's mapping p -> (threshold, scale)
  if (md && md->stride < 2 * (C0 + C1)) { set_error("%s: mod_stride %d is below the 2 x %d values of an image", who, md->stride, C0 + C1); return SR3_E_BADARG; }
  char* s = static_cast<char*>(scratch);
  return act_bwd(dA, x0, x1, C0, C1, B, HW, ss, mr, groups, act, gamma, reinterpret_cast<double*>(s), reinterpret_cast<double*>(s + part),
                 dgamma, dbeta, dx0, dx1, static_cast<hipStream_t>(stream), drop_seed, thresh, scale, aout, acc0 != 0, acc1 != 0, md);
}
}  // namespace
extern "C" int sr3_groupnorm_act_bwd_f32(float* dA, const float* x0, int C0, const float* x1, int C1, int B, int HW, const float* ss,
                                         const float* mr, int groups, int act, const float* gamma, unsigned drop_seed, float drop_p,
                                         float* dgamma, float* dbeta, float* dx0, int acc0, float* dx1, int acc1, float* aout,
                                         void* scratch, size_t scratch_bytes, void* stream) {
  return gn_act_bwd_entry("sr3_groupnorm_act_bwd_f32", dA, x0, C0, x1, C1, B, HW, ss, mr, groups, act, gamma, drop_seed, drop_p, dgamma, dbeta, dx0,
                          acc0, dx1, acc1, aout, scratch, scratch_bytes, nullptr, stream);
}
// ... of a GroupNorm folded under a scale-shift modulation (sr3_groupnorm_fold_mod_f32): ss holds the modulated pairs; beta and the rows
// `mod` give the gradients of the rows, dmod (same layout and stride; only the 2 C entries per image are written).  The scratch is the
// plain entry's (sr3_groupnorm_act_bwd_scratch_bytes)
extern "C" int sr3_groupnorm_act_bwd_mod_f32(float* dA, const float* x0, int C0, const float* x1, int C1, int B, int HW, const float* ss,
                                             const float* mr, int groups, int act, const float* gamma, unsigned drop_seed, float drop_p,
                                             float* dgamma, float* dbeta, float* dx0, int acc0, float* dx1, int acc1, float* aout,
                                             void* scratch, size_t scratch_bytes, const float* beta, const float* mod, int mod_stride,
                                             float* dmod, void* stream) {
  const sr3::ModBwd md = {mod, mod_stride, beta, dmod};
  return gn_act_bwd_entry("sr3_groupnorm_act_bwd_mod_f32", dA, x0, C0, x1, C1, B, HW, ss, mr, groups, act, gamma, drop_seed, drop_p, dgamma, dbeta,
                          dx0, acc0, dx1, acc1, aout, scratch, scratch_bytes, &md, stream);
}

extern "C" int sr3_grad_route_f32(const float* g, int C0, int C1, int B, int Hs, int Ws, int ups, float* d0, int acc0, float* d1, int acc1,
                                  void* stream) {
  using namespace sr3;
  const char* who = "sr3_grad_route_f32";
  if (!g || !d0 || (C1 > 0 && !d1)) { set_error("%s: g / d0 (or d1 with C1 > 0) is NULL", who); return SR3_E_BADARG; }
  if (B <= 0 || Hs <= 0 || Ws <= 0 || C0 <= 0 || C1 < 0) { set_error("%s: batch %d, map %d x %d and channels %d | %d must be positive (C1 >= 0)", who, B, Hs, Ws, C0, C1); return SR3_E_BADARG; }
  if (ups != 0 && ups != 1) { set_error("%s: ups %d is outside 0..1", who, ups); return SR3_E_BADARG; }
  if ((C0 & 3) || (C1 & 3)) { set_error("%s: channel counts must be multiples of 4 (C0 %d, C1 %d)", who, C0, C1); return SR3_E_UNSUPPORTED; }
  if ((double)B * (Hs << ups) * (Ws << ups) * (double)(C0 + C1) >= 2147483647.0) { set_error("%s: tensor exceeds 2^31 elements", who); return SR3_E_UNSUPPORTED; }
  return grad_route(g, C0, C1, B, Hs, Ws, ups, d0, d1, static_cast<hipStream_t>(stream), acc0 != 0, acc1 != 0);
}

extern "C" size_t sr3_colsums_scratch_bytes(int B, int HW, int C) {
  using namespace sr3;
  if (B <= 0 || HW <= 0 || C <= 0 || (C & 3)) return 0;
  return (size_t)B * chan_stats_slices(B, HW, C) * C * 2 * sizeof(double);
}
extern "C" int sr3_colsums_f32(const float* g, int B, int HW, int C, float* dbias, float* dfilm, int film_stride, void* scratch,
                               size_t scratch_bytes, void* stream) {
  using namespace sr3;
  const char* who = "sr3_colsums_f32";
  if (!g || !scratch || (!dbias && !dfilm)) { set_error("%s: g / scratch is NULL, or both of dbias / dfilm are", who); return SR3_E_BADARG; }
  if (B <= 0 || HW <= 0 || C <= 0) { set_error("%s: batch %d, pixels %d and channels %d must be positive", who, B, HW, C); return SR3_E_BADARG; }
  if (C & 3) { set_error("%s: channel count must be a multiple of 4 (C %d)", who, C); return SR3_E_UNSUPPORTED; }
  if (dfilm && film_stride < C) { set_error("%s: film_stride %d is below the channel count %d", who, film_stride, C); return SR3_E_BADARG; }
  if ((double)B * HW * (double)C >= 2147483647.0) { set_error("%s: tensor exceeds 2^31 elements", who); return SR3_E_UNSUPPORTED; }
  if ((uintptr_t)scratch & 7) { set_error("%s: scratch is not 8-byte aligned", who); return SR3_E_ALIGN; }
  const size_t need = sr3_colsums_scratch_bytes(B, HW, C);
  if (scratch_bytes < need) { set_error("%s: scratch too small (%zu < %zu)", who, scratch_bytes, need); return SR3_E_NOMEM; }
  return colsums(g, B, HW, C, static_cast<double*>(scratch), dbias, dfilm, film_stride, static_cast<hipStream_t>(stream));
}

// ---- the loss ops.  Their argument checks are the same but for the names of the required pointers, in one order: required pointers,
// the objective, hr with tgt_x0 (the hybrid op requires hr outright), the shape, vlb_lambda (the hybrid op's; null: none), the scratch ----
namespace {
struct LossOpShape { int batch, channels, pixels; };
int check_loss_op(const char* who, bool missing, const char* required, const sr3::Objective& o, const float* hr_nchw, const LossOpShape& s,
                  const float* vlb_lambda, const void* scratch) {
  using namespace sr3;
  if (missing) { set_error("%s: %s is NULL", who, required); return SR3_E_BADARG; }
  if (const int rc = check_objective_args(who, o.tgt_z, o.tgt_x0, o.weight, o.kind, 0, o.huber_delta)) return rc;
  if (o.tgt_x0 && !hr_nchw) { set_error("%s: hr_nchw is NULL with tgt_x0 given", who); return SR3_E_BADARG; }
  if (s.batch <= 0 || s.pixels <= 0) { set_error("%s: batch %d and pixels %d must be positive", who, s.batch, s.pixels); return SR3_E_BADARG; }
  if (s.channels < 1 || s.channels > 4) { set_error("%s: channels %d is outside 1..4", who, s.channels); return SR3_E_BADARG; }
  if (vlb_lambda && !(isfinite(*vlb_lambda) && *vlb_lambda >= 0.f)) { set_error("%s: vlb_lambda %g must be finite and >= 0", who, (double)*vlb_lambda); return SR3_E_BADARG; }
  if ((uintptr_t)scratch & 7) { set_error("%s: scratch is not 8-byte aligned", who); return SR3_E_ALIGN; }
  return SR3_OK;
}
}  // namespace

extern "C" size_t sr3_loss_grad_scratch_bytes(void) { return sr3::LOSS_GRAD_BLOCKS * sizeof(double); }
extern "C" int sr3_loss_grad_f32(const float* z_nchw, const float* out_nchw, const float* hr_nchw, const float* tgt_z, const float* tgt_x0,
                                 const float* weight, int batch, int channels, int pixels, int loss_kind, float huber_delta, float scale,
                                 float* g_nhwc4, float* loss_sum_out, void* scratch, void* stream) {
  using namespace sr3;
  Objective o;
  o.tgt_z = tgt_z; o.tgt_x0 = tgt_x0; o.weight = weight; o.kind = loss_kind; o.huber_delta = huber_delta;
  if (const int rc = check_loss_op("sr3_loss_grad_f32", !z_nchw || !out_nchw || !g_nhwc4 || !loss_sum_out || !scratch,
                                   "z_nchw / out_nchw / g_nhwc4 / loss_sum_out / scratch", o, hr_nchw, {batch, channels, pixels}, nullptr, scratch))
    return rc;
  return objective_loss_grad({z_nchw, hr_nchw, nullptr, out_nchw, g_nhwc4, static_cast<double*>(scratch), loss_sum_out, nullptr}, o, batch,
                             channels, pixels, 4, scale, static_cast<hipStream_t>(stream));
}

extern "C" size_t sr3_hybrid_loss_grad_scratch_bytes(void) { return 2 * sr3::LOSS_GRAD_BLOCKS * sizeof(double); }
extern "C" int sr3_hybrid_loss_grad_f32(const float* z_nchw, const float* out_nchw, const float* hr_nchw, const float* xt_nchw,
                                        const float* tgt_z, const float* tgt_x0, const float* weight, const float* step_scalars,
                                        float vlb_lambda, int batch, int channels, int pixels, int loss_kind, float huber_delta, float scale,
                                        float* g_nhwc8, float* loss_sum_out, float* vlb_sum_out, void* scratch, void* stream) {
  using namespace sr3;
  Objective o;
  o.tgt_z = tgt_z; o.tgt_x0 = tgt_x0; o.weight = weight; o.kind = loss_kind; o.huber_delta = huber_delta;
  o.hyb = step_scalars; o.lambda = vlb_lambda;
  if (const int rc = check_loss_op("sr3_hybrid_loss_grad_f32",
                                   !z_nchw || !out_nchw || !hr_nchw || !xt_nchw || !step_scalars || !g_nhwc8 || !loss_sum_out || !scratch,
                                   "z_nchw / out_nchw / hr_nchw / xt_nchw / step_scalars / g_nhwc8 / loss_sum_out / scratch", o, hr_nchw,
                                   {batch, channels, pixels}, &vlb_lambda, scratch))
    return rc;
  return objective_loss_grad({z_nchw, hr_nchw, xt_nchw, out_nchw, g_nhwc8, static_cast<double*>(scratch), loss_sum_out, vlb_sum_out}, o, batch,
                             channels, pixels, 8, scale, static_cast<hipStream_t>(stream));
}
