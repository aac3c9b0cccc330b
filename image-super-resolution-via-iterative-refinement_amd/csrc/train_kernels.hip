// Backward-pass helpers of the training step (DDPM.optimize_parameters, model/model.py:48-58:
// p_losses -> backward -> Adam), HBM-bound: GroupNorm+SiLU backward (reduce / fold / apply),
// gradient routing through the virtual concat / residual / nearest-upsample / stride-2 views,
// weight re-layout for the data-gradient convolutions, bias / FiLM gradient sums, L1 loss and
// the fused Adam update.  The contractions (dgrad, wgrad, attention backward) live in
// conv3x3_halo.hip / conv_igemm.hip (reused with transformed weights), wgrad.hip and
// attention_bwd.hip.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

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

__device__ __forceinline__ float sigmoid_t(float v) { return SR3_SIGMOID(v); }

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
    const bool second = c >= C0;
    const float* xs = second ? x1 : x0;
    const int Cs = second ? C1 : C0, cs = second ? c - C0 : c;
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
      const f32x4 xv = *reinterpret_cast<const f32x4*>(xs + pix * Cs + cs);
      f32x4 a4;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float du = g4[e];
        float dm = 1.0f;
        if (drop_thresh != 0) { dm = drop_mask(drop_seed, (unsigned)(pix * C + c + e), drop_thresh, drop_scale); du *= dm; }
        const float u = fmaf(xv[e], sc[e], sh[e]);
        float av = u;
        if (act == 2) {
          const float sg = sigmoid_t(u);
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

// T2a: per (image, group): S1 = sum_c gamma_c * A_c, S2 = sum_c gamma_c * B_c  -> gs[B][G][2] (double)
__global__ __launch_bounds__(64) void k_gn_bwd_group(const double* __restrict__ part, int C, int T, int groups,
                                                      const float* __restrict__ gamma, double* __restrict__ gs) {
  const int b = blockIdx.x / groups, g = blockIdx.x - b * groups;
  const int cpg = C / groups;
  const int lane = threadIdx.x;
  double a = 0.0, bb = 0.0;
  for (int idx = lane; idx < cpg * T; idx += 64) {
    const int k = idx / T, t = idx - k * T;
    const int c = g * cpg + k;
    const double* q = part + (((size_t)b * T + t) * C + c) * 2;
    const double gm = (double)gamma[c];
    a += gm * q[0]; bb += gm * q[1];
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { a += __shfl_xor(a, m); bb += __shfl_xor(bb, m); }
  if (lane == 0) { gs[((size_t)b * groups + g) * 2] = a; gs[((size_t)b * groups + g) * 2 + 1] = bb; }
}

// T2b / T8: per channel: out0[c] (+)= sum_{b,t} part[..][c][0] ; out1[c] (+)= sum part[..][c][1]  (either may be null)
__global__ __launch_bounds__(64) void k_part_colsum(const double* __restrict__ part, int B, int C, int T,
                                                     float* __restrict__ out0, float* __restrict__ out1) {
  const int c = blockIdx.x;
  const int lane = threadIdx.x;
  double a = 0.0, bb = 0.0;
  for (int idx = lane; idx < B * T; idx += 64) {
    const double* q = part + ((size_t)idx * C + c) * 2;
    a += q[0]; bb += q[1];
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

// T3: dx(src) += rstd * (gamma*du - (S1 + xhat*S2)/n), routed to the two concat sources.
// The two terms cancel heavily (GroupNorm's backward projects the x-hat and the constant component out of du), so the
// per-(image, group) coefficients stay in double and the expression is evaluated in double and rounded once -- what
// torch's CPU GroupNorm backward does (acc_type<float> = double for its c1 / c2 / c3 coefficients).  With fp32
// coefficients the rounding of S2 is a perturbation along x-hat that is coherent over a whole (image, group) and is
// amplified by sqrt(B H W) in the weight gradient of the conv that produced x (measured 1.2e-4 normwise at B = 64).
__global__ __launch_bounds__(256) void k_gn_bwd_apply(const float* __restrict__ du, const float* __restrict__ x0,
                                                       const float* __restrict__ x1, int C0, int C1, int HW,
                                                       const float* __restrict__ mr, const double* __restrict__ gs,
                                                       int groups, const float* __restrict__ gamma,
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
    const bool second = c >= C0;
    const float* xs = second ? x1 : x0;
    float* ds = second ? dx1 : dx0;
    const int Cs = second ? C1 : C0, cs = second ? c - C0 : c;
    const f32x4 g4 = *reinterpret_cast<const f32x4*>(du + pix * C + c);
    const f32x4 xv = *reinterpret_cast<const f32x4*>(xs + pix * Cs + cs);
    // (acc == 0: this is the first contribution to that gradient tensor in the backward walk -- a plain store, the mirror is not zeroed)
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (second ? acc1 : acc0) o = *reinterpret_cast<const f32x4*>(ds + pix * Cs + cs);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int g = (c + e) / cpg;
      const double mu = (double)mr[((size_t)b * groups + g) * 2], rs = (double)mr[((size_t)b * groups + g) * 2 + 1];
      const double S1 = gs[((size_t)b * groups + g) * 2], S2 = gs[((size_t)b * groups + g) * 2 + 1];
      const double xh = ((double)xv[e] - mu) * rs;
      o[e] += (float)(rs * ((double)gamma[c + e] * (double)g4[e] - (S1 + xh * S2) * inv_n));
    }
    *reinterpret_cast<f32x4*>(ds + pix * Cs + cs) = o;
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
    const bool second = c >= C0;
    float* ds = second ? d1 : d0;
    const int Cs = second ? C1 : C0, cs = second ? c - C0 : c;
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
    if (second ? acc1 : acc0) o += *reinterpret_cast<const f32x4*>(ds + pix * Cs + cs);
    *reinterpret_cast<f32x4*>(ds + pix * Cs + cs) = o;
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

// T11: the pixel loss of set_loss (diffusion.py:84-90,245) and its gradient w.r.t. eps_hat, written NHWC with the
// channel dim padded to CP.  L1 (nn.L1Loss(reduction='sum'), what define_G configures): loss_part[block] = sum |z - e|,
// g = -sign(z - e) * scale.  L2 (nn.MSELoss(reduction='sum'), loss_type 'l2'): sum (z - e)^2, g = -2 (z - e) * scale.
template <bool L2>
__global__ __launch_bounds__(256) void k_l1_loss_grad(const float* __restrict__ z, const float* __restrict__ e, int B,
                                                       int Cc, int HW, int CP, float scale, float* __restrict__ g_nhwc,
                                                       double* __restrict__ loss_part) {
  __shared__ double red[256];
  double s = 0.0;
  const size_t total = (size_t)B * HW;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / HW, p = i - b * HW;
    for (int c = 0; c < CP; ++c) {
      float gv = 0.f;
      if (c < Cc) {
        const size_t idx = (b * Cc + c) * HW + p;
        const float d = z[idx] - e[idx];
        if (L2) {
          s += (double)d * (double)d;
          gv = -2.f * d * scale;
        } else {
          s += (double)fabsf(d);
          gv = d > 0.f ? -scale : (d < 0.f ? scale : 0.f);
        }
      }
      g_nhwc[i * CP + c] = gv;
    }
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int k = 128; k >= 1; k >>= 1) {
    if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss_part[blockIdx.x] = red[0];
}
__global__ __launch_bounds__(64) void k_sum_parts(const double* __restrict__ part, int n, float* __restrict__ out) {
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 64) s += part[i];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
  if (threadIdx.x == 0) out[0] = (float)s;
}

// T12: fused Adam over the whole parameter arena (torch.optim.Adam defaults, model/model.py:39-40):
// m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2 ; p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps)
// Four elements, shared by k_adam and k_adam_ema.  The fused multiply-adds are written out: left to the compiler, which of the
// two products of `v b2 + w2 g g` is fused depends on the code around the expression, and the two kernels must give the same bits.
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
__global__ __launch_bounds__(256) void k_adam(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                               float* __restrict__ v, size_t n4, float w1, float b2, float w2, float eps,
                                               float step, float bc2_sqrt) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    f32x4 pv = *reinterpret_cast<f32x4*>(p + i * 4);
    const f32x4 gv = *reinterpret_cast<const f32x4*>(g + i * 4);
    f32x4 mv = *reinterpret_cast<f32x4*>(m + i * 4);
    f32x4 vv = *reinterpret_cast<f32x4*>(v + i * 4);
    adam_vec4(pv, gv, mv, vv, w1, b2, w2, eps, step, bc2_sqrt);
    *reinterpret_cast<f32x4*>(p + i * 4) = pv;
    *reinterpret_cast<f32x4*>(m + i * 4) = mv;
    *reinterpret_cast<f32x4*>(v + i * 4) = vv;
  }
}

// T12b: the same pass with the exponential moving average of the weights as one more stream over the arena.
// MODE 0: Adam alone (no access to ema); 1: ema = p_new (the copy before step_start_ema); 2: ema += (p_new - ema) * we,
// we = 1 - ema_decay -- the lerp form of exp_avg above: p_new == ema leaves ema unchanged exactly.  No atomics.
__device__ __forceinline__ void ema_lerp4(f32x4& ev, const f32x4& pv, float we) {
#pragma unroll
  for (int e = 0; e < 4; ++e) ev[e] = fmaf(pv[e] - ev[e], we, ev[e]);
}
template <int MODE>
__global__ __launch_bounds__(256) void k_adam_ema(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, float* __restrict__ ema, size_t n4, float w1,
                                                   float b2, float w2, float eps, float step, float bc2_sqrt, float we) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    f32x4 pv = *reinterpret_cast<f32x4*>(p + i * 4);
    const f32x4 gv = *reinterpret_cast<const f32x4*>(g + i * 4);
    f32x4 mv = *reinterpret_cast<f32x4*>(m + i * 4);
    f32x4 vv = *reinterpret_cast<f32x4*>(v + i * 4);
    f32x4 ev = {0.f, 0.f, 0.f, 0.f};
    if (MODE == 2) ev = *reinterpret_cast<f32x4*>(ema + i * 4);
    adam_vec4(pv, gv, mv, vv, w1, b2, w2, eps, step, bc2_sqrt);
    if (MODE == 2) ema_lerp4(ev, pv, we);
    *reinterpret_cast<f32x4*>(p + i * 4) = pv;
    *reinterpret_cast<f32x4*>(m + i * 4) = mv;
    *reinterpret_cast<f32x4*>(v + i * 4) = vv;
    if (MODE == 1) *reinterpret_cast<f32x4*>(ema + i * 4) = pv;
    if (MODE == 2) *reinterpret_cast<f32x4*>(ema + i * 4) = ev;
  }
}

// T12c: k_adam_ema on a gradient scaled by a device-side coefficient, guarded by a device-side flag (scale4 = the four floats
// k_grad_norm_finish writes: norm, coef, finite flag, 0).  Every thread reads the same 16 bytes.  Flag 0: nothing is written.
// The scaled gradient is a product rounded on its own: contraction is switched off for it, since this toolchain's __fmul_rn is a
// plain `x * y` that the compiler may fold into the subtraction that follows.  coef == 1: the bits of k_adam_ema.
__device__ __forceinline__ float fmul_rn_alone(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
template <int MODE>
__global__ __launch_bounds__(256) void k_adam_ema_scaled(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v, float* __restrict__ ema, size_t n4, float w1,
                                                          float b2, float w2, float eps, float step, float bc2_sqrt, float we,
                                                          const float* __restrict__ scale4) {
  const f32x4 sc = *reinterpret_cast<const f32x4*>(scale4);
  if (sc[2] == 0.f) return;
  const float coef = sc[1];
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    f32x4 pv = *reinterpret_cast<f32x4*>(p + i * 4);
    f32x4 gv = *reinterpret_cast<const f32x4*>(g + i * 4);
    f32x4 mv = *reinterpret_cast<f32x4*>(m + i * 4);
    f32x4 vv = *reinterpret_cast<f32x4*>(v + i * 4);
    f32x4 ev = {0.f, 0.f, 0.f, 0.f};
    if (MODE == 2) ev = *reinterpret_cast<f32x4*>(ema + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) gv[e] = fmul_rn_alone(gv[e], coef);
    adam_vec4(pv, gv, mv, vv, w1, b2, w2, eps, step, bc2_sqrt);
    if (MODE == 2) ema_lerp4(ev, pv, we);
    *reinterpret_cast<f32x4*>(p + i * 4) = pv;
    *reinterpret_cast<f32x4*>(m + i * 4) = mv;
    *reinterpret_cast<f32x4*>(v + i * 4) = vv;
    if (MODE == 1) *reinterpret_cast<f32x4*>(ema + i * 4) = pv;
    if (MODE == 2) *reinterpret_cast<f32x4*>(ema + i * 4) = ev;
  }
}

// T13: global L2 norm of the gradient arena and accumulation of micro-batch gradients (config train.optimizer.clip_grad_norm /
// accumulate).  The grid is FIXED -- min(GRAD_NORM_BLOCKS, ceil(n4 / 256)) blocks of 256 threads, whatever the device -- and every
// sum has one order: a thread adds the squares of its vectors in stride order (elements 0..3 of each) in double, the 64 lanes of a
// wave combine by __shfl_xor (32, 16, .., 1), the block's four waves are added in wave order through LDS, and one wave adds the
// blocks' partial sums in index order.  The square of an fp32 is exact in double, so contraction cannot change a bit.  No atomics.
constexpr int GRAD_NORM_BLOCKS = 512;
static inline int grad_norm_blocks(size_t n4) { const size_t b = (n4 + 255) / 256; return (int)(b > GRAD_NORM_BLOCKS ? GRAD_NORM_BLOCKS : (b ? b : 1)); }

__device__ __forceinline__ f32x4 ld4(const float* p, size_t i) { return *reinterpret_cast<const f32x4*>(p + i * 4); }
__device__ __forceinline__ void st4(float* p, size_t i, const f32x4& x) { *reinterpret_cast<f32x4*>(p + i * 4) = x; }
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
    const bool second = c >= C0;
    const float* xs = second ? x1 : x0;
    const int Cs = second ? C1 : C0, cs = second ? c - C0 : c;
    f32x4 v = *reinterpret_cast<const f32x4*>(xs + pix * Cs + cs);
    const f32x4 s0 = *reinterpret_cast<const f32x4*>(ss + ((size_t)b * C + c) * 2);
    const f32x4 s1 = *reinterpret_cast<const f32x4*>(ss + ((size_t)b * C + c) * 2 + 4);
    v.x = fmaf(v.x, s0.x, s0.y); v.y = fmaf(v.y, s0.z, s0.w); v.z = fmaf(v.z, s1.x, s1.y); v.w = fmaf(v.w, s1.z, s1.w);
    if (act == 2) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = v[e] * sigmoid_t(v[e]);
    }
    if (drop_thresh != 0) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] *= drop_mask(drop_seed, (unsigned)(pix * C + c + e), drop_thresh, drop_scale);
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

static inline int ew_blocks(size_t n) { size_t b = (n + 255) / 256; return (int)(b > 8192 ? 8192 : (b ? b : 1)); }

int act_bwd(float* dA, const float* x0, const float* x1, int C0, int C1, int B, int HW, const float* ss, const float* mr,
            int groups, int act, const float* gamma, double* part, double* gs, float* dgamma, float* dbeta, float* dx0,
            float* dx1, hipStream_t st, unsigned drop_seed, unsigned drop_thresh, float drop_scale, float* aout, bool acc0, bool acc1) {
  const int C = C0 + C1;
  if ((C0 & 3) || (C1 & 3)) { set_error("act_bwd: channels %% 4"); return SR3_E_UNSUPPORTED; }
  int LQ, cblocks, ppb, T;
  stats_geometry(B, HW, C, &LQ, &cblocks, &ppb, &T);
  hipLaunchKernelGGL(k_act_bwd_reduce, dim3(T, cblocks, B), dim3(256), 0, st, dA, x0, x1, C0, C1, HW, LQ, ppb, ss, mr,
                     groups, act, drop_seed, drop_thresh, drop_scale, part, aout);
  SR3_LAUNCH_CHECK("k_act_bwd_reduce");
  hipLaunchKernelGGL(k_gn_bwd_group, dim3(B * groups), dim3(64), 0, st, part, C, T, groups, gamma, gs);
  SR3_LAUNCH_CHECK("k_gn_bwd_group");
  hipLaunchKernelGGL(k_part_colsum, dim3(C), dim3(64), 0, st, part, B, C, T, dbeta, dgamma);
  SR3_LAUNCH_CHECK("k_part_colsum");
  const size_t total4 = (size_t)B * HW * (C >> 2);
  hipLaunchKernelGGL(k_gn_bwd_apply, dim3(ew_blocks(total4)), dim3(256), 0, st, dA, x0, x1, C0, C1, HW, mr, gs, groups,
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
    hipLaunchKernelGGL(k_part_colsum, dim3(C), dim3(64), 0, st, part, B, C, T, dbias, (float*)nullptr);
    SR3_LAUNCH_CHECK("k_part_colsum");
  }
  if (dfilm) {
    hipLaunchKernelGGL(k_part_imgsum, dim3((B * C + 255) / 256), dim3(256), 0, st, part, B, C, T, dfilm, film_stride);
    SR3_LAUNCH_CHECK("k_part_imgsum");
  }
  return SR3_OK;
}
int l1_loss_grad(const float* z, const float* e, int B, int Cc, int HW, int CP, float scale, bool l2, float* g_nhwc,
                 double* loss_part, float* loss_out, hipStream_t st) {
  const int blocks = 256;
  if (l2) hipLaunchKernelGGL(k_l1_loss_grad<true>, dim3(blocks), dim3(256), 0, st, z, e, B, Cc, HW, CP, scale, g_nhwc, loss_part);
  else hipLaunchKernelGGL(k_l1_loss_grad<false>, dim3(blocks), dim3(256), 0, st, z, e, B, Cc, HW, CP, scale, g_nhwc, loss_part);
  SR3_LAUNCH_CHECK("k_l1_loss_grad");
  hipLaunchKernelGGL(k_sum_parts, dim3(1), dim3(64), 0, st, loss_part, blocks, loss_out);
  SR3_LAUNCH_CHECK("k_sum_parts");
  return SR3_OK;
}
namespace {
// torch.optim.Adam evaluates 1 - beta, the bias corrections and the step size as Python floats (double) and rounds
// each ONCE to fp32 when it meets the tensor (meant_double: the decimal behind the ABI's fp32 hyper-parameters).
struct AdamScalars { float w1, b2, w2, eps, step_size, bc2s; };
AdamScalars adam_scalars(float lr, float b1, float b2, float eps, int step) {
  const double b1d = meant_double(b1), b2d = meant_double(b2), lrd = meant_double(lr);
  const double bc1 = 1.0 - pow(b1d, (double)step);
  const double bc2 = 1.0 - pow(b2d, (double)step);
  return {(float)(1.0 - b1d), (float)b2d, (float)(1.0 - b2d), (float)meant_double(eps), (float)(lrd / bc1), (float)sqrt(bc2)};
}
}  // namespace
int adam_step(float* p, const float* g, float* m, float* v, size_t n, float lr, float b1, float b2, float eps, int step,
              hipStream_t st) {
  if (n & 3) { set_error("adam: n %% 4"); return SR3_E_BADARG; }
  const AdamScalars a = adam_scalars(lr, b1, b2, eps, step);
  hipLaunchKernelGGL(k_adam, dim3(ew_blocks(n / 4)), dim3(256), 0, st, p, g, m, v, n / 4, a.w1, a.b2, a.w2, a.eps, a.step_size,
                     a.bc2s);
  SR3_LAUNCH_CHECK("k_adam");
  return SR3_OK;
}
int adam_ema_step(float* p, const float* g, float* m, float* v, float* ema, size_t n, float lr, float b1, float b2, float eps,
                  int step, float ema_decay, int ema_mode, hipStream_t st) {
  const AdamScalars a = adam_scalars(lr, b1, b2, eps, step);
  const float we = (float)(1.0 - meant_double(ema_decay));      // 1 - decay in double, rounded once (as 1 - beta1 is)
  const dim3 grid(ew_blocks(n / 4)), block(256);
#define SR3_ADAM_EMA(MODE) \
  hipLaunchKernelGGL(k_adam_ema<MODE>, grid, block, 0, st, p, g, m, v, ema, n / 4, a.w1, a.b2, a.w2, a.eps, a.step_size, a.bc2s, we)
  if (ema_mode == 0) SR3_ADAM_EMA(0);
  else if (ema_mode == 1) SR3_ADAM_EMA(1);
  else SR3_ADAM_EMA(2);
#undef SR3_ADAM_EMA
  SR3_LAUNCH_CHECK("k_adam_ema");
  return SR3_OK;
}
int adam_ema_step_scaled(float* p, const float* g, float* m, float* v, float* ema, size_t n, float lr, float b1, float b2,
                         float eps, int step, float ema_decay, int ema_mode, const float* scale4, hipStream_t st) {
  const AdamScalars a = adam_scalars(lr, b1, b2, eps, step);
  const float we = (float)(1.0 - meant_double(ema_decay));
  const dim3 grid(ew_blocks(n / 4)), block(256);
#define SR3_ADAM_EMA_SCALED(MODE)                                                                                                  \
  hipLaunchKernelGGL(k_adam_ema_scaled<MODE>, grid, block, 0, st, p, g, m, v, ema, n / 4, a.w1, a.b2, a.w2, a.eps, a.step_size, \
                     a.bc2s, we, scale4)
  if (ema_mode == 0) SR3_ADAM_EMA_SCALED(0);
  else if (ema_mode == 1) SR3_ADAM_EMA_SCALED(1);
  else SR3_ADAM_EMA_SCALED(2);
#undef SR3_ADAM_EMA_SCALED
  SR3_LAUNCH_CHECK("k_adam_ema_scaled");
  return SR3_OK;
}
size_t grad_norm_scratch_bytes(size_t n) { return (size_t)grad_norm_blocks(n / 4) * sizeof(double); }
static int grad_norm_finish(const double* part, int nparts, float max_norm, float* out4, hipStream_t st) {
  hipLaunchKernelGGL(k_grad_norm_finish, dim3(1), dim3(64), 0, st, part, nparts, max_norm, out4);
  SR3_LAUNCH_CHECK("k_grad_norm_finish");
  return SR3_OK;
}
int grad_norm(const float* g, size_t n, float max_norm, double* part, float* out4, hipStream_t st) {
  const int blocks = grad_norm_blocks(n / 4);
  hipLaunchKernelGGL(k_grad_sqnorm_parts, dim3(blocks), dim3(256), 0, st, g, n / 4, part);
  SR3_LAUNCH_CHECK("k_grad_sqnorm_parts");
  return grad_norm_finish(part, blocks, max_norm, out4, st);
}
int grad_accumulate(float* acc, const float* g, size_t n, bool first, float max_norm, double* part, float* out4, hipStream_t st) {
  const dim3 grid(grad_norm_blocks(n / 4)), block(256);
#define SR3_GRAD_ACC(FIRST, NORM) hipLaunchKernelGGL((k_grad_accumulate<FIRST, NORM>), grid, block, 0, st, acc, g, n / 4, part)
  if (out4) { if (first) SR3_GRAD_ACC(true, true); else SR3_GRAD_ACC(false, true); }
  else { if (first) SR3_GRAD_ACC(true, false); else SR3_GRAD_ACC(false, false); }
#undef SR3_GRAD_ACC
  SR3_LAUNCH_CHECK("k_grad_accumulate");
  return out4 ? grad_norm_finish(part, (int)grid.x, max_norm, out4, st) : SR3_OK;
}
int nchw_to_nhwc_pad(const float* a, int Ca, const float* b, int Cb, int B, int HW, int CP, float* out, hipStream_t st) {
  const size_t total = (size_t)B * HW;
  hipLaunchKernelGGL(k_nchw_to_nhwc_pad, dim3(ew_blocks(total)), dim3(256), 0, st, a, Ca, b, Cb, HW, CP, out, total);
  SR3_LAUNCH_CHECK("k_nchw_to_nhwc_pad");
  return SR3_OK;
}

}  // namespace sr3
