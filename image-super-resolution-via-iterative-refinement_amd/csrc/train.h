// Internal declarations of the training-step kernels (train_kernels.hip, wgrad.hip, attention_bwd.hip).
#pragma once
#include "sr3_common.h"

namespace sr3 {

// grid of an element-wise pass over n items: 256 threads a block, at most 8192 blocks (grid-stride loops)
inline int ew_blocks(size_t n) { size_t b = (n + 255) / 256; return (int)(b > 8192 ? 8192 : (b ? b : 1)); }
// the regions a per-op entry cuts its caller's scratch into start on 256-byte boundaries, as the regions of the step's workspace do
inline size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }

// GroupNorm(+SiLU) backward over the virtual concat (x0|x1): dA (grad w.r.t. the activated input) is
// overwritten with du, partial sums go to `part`, group sums to gs[B][G][2], parameter gradients to
// dgamma/dbeta[C], and dx0/dx1 (+=) receive the input gradient.  mr[B][G][2] = (mean, rstd).
// ... of a GroupNorm folded under a scale-shift modulation (fold_modulate, small_kernels.hip): the rows (image b's scales [C] then shifts
// [C] at mod + b * stride), the GroupNorm's beta, and where the rows' gradients go (dmod: the layout and stride of mod)
struct ModBwd { const float* mod; int stride; const float* beta; float* dmod; };
int act_bwd(float* dA, const float* x0, const float* x1, int C0, int C1, int B, int HW, const float* ss, const float* mr,
            int groups, int act, const float* gamma, double* part, double* gs, float* dgamma, float* dbeta, float* dx0,
            float* dx1, hipStream_t st, unsigned drop_seed = 0, unsigned drop_thresh = 0, float drop_scale = 1.f,
            float* aout = nullptr, bool acc0 = true, bool acc1 = true, const ModBwd* md = nullptr);      // aout: also write a = dropout(act(x*scale+shift)) (what apply_act would, in the same pass; round 6)
// a = dropout(act(x*scale+shift)) over the virtual concat, materialised for the weight-gradient GEMM
int apply_act(const float* x0, const float* x1, int C0, int C1, int B, int HW, const float* ss, int act, unsigned drop_seed,
              unsigned drop_thresh, float drop_scale, float* out, hipStream_t st);
size_t act_bwd_part_bytes(int B, int HW, int C);
// acc0 / acc1 (here and in act_bwd): false = the first contribution to that destination in the backward walk is a plain store (round 6:
// the gradient mirror is no longer zeroed every step)
int grad_route(const float* g, int C0, int C1, int B, int Hs, int Ws, int ups, float* d0, float* d1, hipStream_t st,
               bool acc0 = true, bool acc1 = true);
int zero_insert(const float* g, int B, int Ho, int Wo, int C, float* z, hipStream_t st);
int w_flip_transpose(const float* w, int Cout, int taps, int Cin, int CoutP, float* wt, hipStream_t st);
int colsums(const float* g, int B, int HW, int C, double* part, float* dbias, float* dfilm, int film_stride,
            hipStream_t st);
// The training objective of one step (sr3_train_step_ex / sr3_loss_grad_f32): per-image target coefficients and weight (device, all
// three or none: target z, weight 1) and the pixel loss
enum { LOSS_L1 = 0, LOSS_L2 = 1, LOSS_HUBER = 2 };
constexpr int LOSS_GRAD_BLOCKS = 256;      // blocks of the loss kernels = doubles of their partial-sum scratch
struct Objective {
  const float* tgt_z = nullptr; const float* tgt_x0 = nullptr; const float* weight = nullptr;
  int kind = LOSS_L1;
  float huber_delta = 1.f;
  // learned reverse-process variance (sr3_train_step_ex2 / sr3_hybrid_loss_grad_f32): per image the HYB_STRIDE scalars of the drawn step
  // (device; null: the objective above alone) and the weight lambda of L_vlb
  const float* hyb = nullptr;
  float lambda = 0.f;
  const float* vlb_w = nullptr;      // per image, lambda * vlb_w[b] in place of lambda (sr3_train_step_ex3's vlb_weight; null: lambda)
};
// one image's row of Objective::hyb: x0 = a x_t - b out ; posterior mean c1 x0 + c2 x_t ; log beta, log beta~ (clipped) of the step ;
// last != 0: the walk's last step (the discretised log-likelihood instead of the KL term)
enum { HYB_A = 0, HYB_B, HYB_C1, HYB_C2, HYB_LOG_BETA, HYB_LOG_BETA_TILDE, HYB_LAST, HYB_STRIDE = 8 };
int check_objective_args(const char* who, const float* tgt_z, const float* tgt_x0, const float* weight, int loss_kind, int min_kind,
                         float huber_delta);
// the tensors of the loss: z, hr, e [B, Cc, HW] (hr read only with tgt_x0 or o.hyb), g [B, HW, CP], LOSS_GRAD_BLOCKS doubles of loss_part.
// With o.hyb (a variance head): e [B, 2 Cc, HW], x_t [B, Cc, HW], CP >= 2 Cc, twice the doubles, vlb_out (may be null) = sum vlb in bits
struct LossTensors { const float* z; const float* hr; const float* xt; const float* e; float* g_nhwc; double* loss_part; float* loss_out; float* vlb_out; };
// loss sum and its gradient under `o`: the plain form of k_loss_grad for target z / weight 1 / L1 or L2, else the objective's; with
// o.hyb the hybrid loss L_simple + lambda L_vlb, loss_out[0] = sum w rho(d) + lambda sum vlb
int objective_loss_grad(const LossTensors& t, const Objective& o, int B, int Cc, int HW, int CP, float scale, hipStream_t st);
int nchw_to_nhwc_pad(const float* a, int Ca, const float* b, int Cb, int B, int HW, int CP, float* out, hipStream_t st);
// Per-image terms of the variational bound (vlb_eval.hip): vb_out / mse_out [b * ostride] (rows: a row index per image;
// step2: the device step counter, one row for all images and row j of [table_rows, B] outputs; both null: image b reads row b) = the
// mean over C P of the bound's term in bits and of (x0 - x0^)^2.  Two launches; part: vlb_terms_scratch(B) bytes of block partials
int vlb_terms(const float* x0, const float* xt, const float* out, const float* table, int table_rows, const int* rows, int* step2,
              int var_mode, bool clip, int B, int C, int OC, int P, float* vb_out, float* mse_out, int ostride, double* part, hipStream_t st);
size_t vlb_terms_scratch(int batch);
// sr3_train_step_ex3: where the step's per-image terms go (out null: none are computed), and the rows' table where the objective has none
struct PerImage { float* out = nullptr; double* part = nullptr; const float* scal = nullptr; };
// Everything one training step is given (train_plan.hip): each sr3_train_step* entry fills it by name, train_step_checked refuses or
// settles it, run_train launches it.  As an entry fills it the fields hold the caller's arguments as they came (obj.kind -1: the plan's
// loss; obj.hyb: step_scalars; obj.vlb_w: vlb_weight; pi.out / pi.part: per_image_out / scratch, pi.scal unset)
struct TrainStep {
  const float* hr = nullptr; const float* cond = nullptr; int cond_channels = 0; const float* z = nullptr;
  const float* q_ca = nullptr; const float* q_cb = nullptr;      // q_sample's coefficients, per image
  const float* level = nullptr; const int64_t* tstep = nullptr;  // the SR3 variant's noise level / the DDPM variant's timestep
  const float* freq = nullptr; const float* params = nullptr; float* grads = nullptr;
  void* workspace = nullptr; size_t workspace_bytes = 0;
  float* loss_sum_out = nullptr; float grad_scale = 1.f;
  float dropout_p = 0.f; unsigned dropout_seed = 0;
  int n_marks = 0; const size_t* mark_offsets = nullptr; void* const* mark_events = nullptr;      // gradient-ready marks
  int batch = 0; hipStream_t stream = nullptr;
  Objective obj; float* vlb_sum_out = nullptr;
  PerImage pi; size_t pi_scratch_bytes = 0;
};

// Weight gradient of a conv (wgrad.hip): dw[n][tap][c] = sum_m dy[m][n] * a_tap[m][c], a = prologue(x0|x1)
// recomputed on the fly (same ConvParams geometry as the forward; p.out / p.w unused).
// `slabs` holds the per-pixel-split partial results; dw is overwritten.
struct WgradParams {
  ConvParams c;        // forward geometry + src0/src1/ss/act (+ ups/stride/ksize)
  const float* dy;     // [B,Ho,Wo,Cout]
  float* dw;           // [Cout][taps][Cin]
  float* slabs;        // [msplit][Cout][taps][Cin], wgrad_slab_bytes(c) of them (read only where the layer's pixel split is > 1)
};
size_t wgrad_slab_bytes(const ConvParams& c);
int conv_wgrad(const WgradParams& p, hipStream_t st);

// Attention backward (attention_bwd.hip): qkv [B][N][3C], dout [B][N][C] -> dqkv [B][N][3C] (overwritten)
// out_fwd (the forward attention output [B][N][C]) is only read by the key-blocked path (N too large for LDS strips)
// scratch (attention_backward_scratch_bytes): dK / dV slabs per query block, summed in order -- no atomics, no memset; null: fp32 atomics
size_t attention_backward_scratch_bytes(int B, int N, int C);
int attention_backward(const float* qkv, const float* dout, const float* out_fwd, int B, int N, int C, float* dqkv, hipStream_t st,
                       float* scratch = nullptr, size_t scratch_bytes = 0, int heads = 1);
// (heads > 1: the multi-head layout of attention_forward_heads, C the full channel count; needs the slabs -- scratch is not optional)

// Embedding / FiLM backward (small): see train_small.hip
struct EmbedBwdParams {
  int variant, B, inner, F;
  const float* level; const int64_t* tstep; const float* freq;
  const float* w1; const float* b1; const float* w2; const float* b2; const float* wf;
  const float* dfilm;     // [B][F]
  float* dw1; float* db1; float* dw2; float* db2; float* dwf; float* dbf;
  float* scratch;         // >= B * 29 * inner floats (8 per image of the recompute, 5 of the MLP backward, 16 row-chunk partials)
};
int embed_backward(const EmbedBwdParams& p, hipStream_t st);

}  // namespace sr3
