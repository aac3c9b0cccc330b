// Training step driver: q_sample -> UNet forward (train plan) -> L1 loss -> backward walk -> gradient
// arena.  Replaces the reference's autograd step `l_pix = netG(data); l_pix.backward()`
// (model/model.py:50-54 over p_losses, model/sr3_modules/diffusion.py:221-246 /
// model/ddpm_modules/diffusion.py:278-294).  The backward is a reverse walk over the records the
// train plan kept for every conv / attention of the forward:
//   data gradient  = the same MFMA conv kernels run on dOut with flipped-transposed weights
//                    (zero insertion for the stride-2 convs, 2x2 sum for the nearest upsample),
//   weight gradient = wgrad.hip (activated input recomputed on the fly),
//   GroupNorm+SiLU  = reduce / fold / apply (train_kernels.hip), routed through the concat views,
//   attention       = attention_bwd.hip,
//   bias / FiLM     = per-channel sums of dOut (partial sums, fixed order).
// Every parameter gradient is written exactly once (no accumulation across ops), activation
// gradients live in a mirror of the activation arena and are accumulated in stream order.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "plan_internal.h"
#include "tile_code.h"
#include "train.h"

namespace sr3 {

// ---------------------------------------------------------------------------------------------
// training plan: the forward walk with every activation kept and persistent GroupNorm tables, a gradient mirror of the
// activation arena, and the backward of every record resolved once -- shapes, kernels, store-or-accumulate -- so that ONE list
// sizes the scratch regions here and is launched by run_train
// ---------------------------------------------------------------------------------------------
namespace {
// the input conv's weight gradient reads the image with its channels padded to a multiple of 4 the wgrad kernels take
// (nchw_to_nhwc_pad): 8 up to 8 input channels -- every model without self-conditioning keeps its workspace bytes -- 16 above
// (the plan accepts in_channel <= 16)
inline int in_pad(int in_channel) { return in_channel <= 8 ? 8 : 16; }
// the output conv's gradients read dOut with its channels padded to a multiple of 4 (k_loss_grad): 4 up to 4 output rows -- every
// model without a variance head keeps its launches and its workspace bytes -- 8 above (6 or 8 rows: a prediction and its variance head)
inline int out_pad(const sr3_plan* P) { return P->out_ch <= 4 ? 4 : 8; }

// shape of a record's weight gradient: the forward conv's own geometry
ConvParams wgrad_shape(const sr3_plan* P, const Rec& r, int B) {
  const std::vector<Tensor>& T = P->ttens;
  if (r.kind == R_CONV_IN) return conv_shape(B, T[r.out].H, T[r.out].W, 0, 1, 3, in_pad(P->d.in_channel), 0, T[r.out].C);
  const Tensor& x0 = T[r.s.x0];
  if (r.kind == R_CONV_OUT) return conv_shape(B, x0.H, x0.W, 0, 1, 3, x0.C, 0, out_pad(P));
  ConvParams c = conv_shape(B, x0.H, x0.W, r.s.ups, r.s.stride, r.s.ksize, x0.C, r.s.x1 >= 0 ? T[r.s.x1].C : 0, T[r.out].C);
  if (r.s.act) { c.C0 += c.C1; c.C1 = 0; }      // the activated input is materialised by act_bwd: a single source
  return c;
}
// ... of the fused res_conv segment's
ConvParams wgrad_q_shape(const sr3_plan* P, const Rec& r, int B) {
  const std::vector<Tensor>& T = P->ttens;
  return conv_shape(B, T[r.out].H, T[r.out].W, 0, 1, 1, T[r.s.q0].C, r.s.q1 >= 0 ? T[r.s.q1].C : 0, T[r.out].C);
}
// shape of the data gradient of the forward conv `f`: dOut [B,H,W,f.Cout] (zero-inserted for a stride-2 conv, so H x W is the
// forward conv's input map behind its upsampling) under a stride-1 conv producing f's input channels
ConvParams dgrad_shape(const ConvParams& f) { return conv_shape(f.B, f.Hs << f.ups, f.Ws << f.ups, 0, 1, f.ksize, f.Cout, 0, f.C0 + f.C1); }

// The Winograd form of one data-gradient conv `g`, or false: the general kernels run it.  Sets g.wino_split to what the launch
// uses; *split_filters: the 3 x bf16 split form of the transformed filters.  THE Winograd rule of the backward (choose_dgrad)
bool dgrad_wino(const sr3_plan* P, ConvParams& g, WinoGeom* wg, bool* split_filters) {
  g.wino_split = 0;
  *split_filters = false;
  if (!P->opt.winograd || g.ksize != 3) return false;
  // the data gradient has neither a prologue nor dropout, so every 3x3 stride-1 / zero-inserted stride-2 layer with H, W multiples
  // of 16 qualifies (and the four-image 8 x 8 tile); the one-image tile on its 3 x bf16 split instantiation, as the forward
  if (wino_geometry(g, wg)) {
    *split_filters = P->opt.wino_split && wg->NB == 1;
    g.wino_split = *split_filters ? (P->opt.wino2 ? 2 : 1) : 0;      // (2: the 8 x 16 tile of conv3x3_wino2.hip)
    return true;
  }
  // off the native geometry (plan option train_geom): the two-workgroup kernel on the maps that rule refuses, plain where the map is a
  // whole multiple of its 8 x 16 tile, ragged where wino_ragged_wins -- wino_mode's rule for the forward
  if (!P->opt.train_geom || plan_native_geometry(P) || !P->opt.wino_split || !P->opt.wino2) return false;
  g.wino_split = wino2_fits(g) ? 2 : 3;
  if ((g.wino_split == 3 && !(P->opt.wino_ragged && wino_ragged_wins(g))) || !wino_geometry(g, wg)) { g.wino_split = 0; return false; }
  *split_filters = true;
  return true;
}

size_t wu_bytes(const Dgrad& d) {
  if (d.wu == WU_NONE) return 0;
  return (d.wu == WU_GEMM ? igemm_wsplit_floats(d.c.Cout, 1, d.c.C0) : wino_weight_floats(d.c.Cout, d.c.C0, d.wu == WU_WINO_SPLIT)) * sizeof(float);
}

// The kernel of the data-gradient conv whose shape d.c holds: THE place where the backward decides it.  A kernel that reads derived
// filters is taken where they fit `wu_cap` bytes, the 1x1 GEMM kernel where its split-K slabs fit `slab_cap` bytes too
void choose_dgrad(const sr3_plan* P, Dgrad& d, size_t wu_cap, size_t slab_cap) {
  ConvParams& c = d.c;
  d.tile = 0; d.ksplit = 0; c.igemm_split = 0;
  // 3x3: Winograd F(2x2,3x3) on the flipped-transposed filters where dgrad_wino says so
  WinoGeom wg;
  bool split_filters;
  if (dgrad_wino(P, c, &wg, &split_filters)) {
    d.tile = 11; d.wu = split_filters ? WU_WINO_SPLIT : WU_WINO;
    if (wu_bytes(d) <= wu_cap) return;
    d.tile = 0; c.wino_split = 0;
  }
  // 1x1 / 8x8 data gradients on the im2col kernel: its 3 x bf16 split instantiation by the forward's rule
  c.igemm_split = igemm_split_rule(P, c);
  // 1x1: the plain GEMM kernel where it fits (plan option gemm2; gemm1x1.hip), its pre-split weights derived from the transposed
  // filters into the region the Winograd data gradients use for theirs
  d.wu = WU_GEMM;
  if (c.igemm_split && P->opt.gemm2 && gemm1x1_fits(c, 2) && (!(c.Cout & 127) || P->opt.gemm_n64) && wu_bytes(d) <= wu_cap) {
    const int ks = conv_pick(c, 22, 0).ksplit;
    if (ks == 1 || (size_t)ks * c.B * c.Ho * c.Wo * c.Cout * sizeof(float) <= slab_cap) { d.tile = 22; d.ksplit = ks; return; }
  }
  d.wu = WU_NONE;
}

// every data gradient of the record list, under the same caps
void choose_dgrads(sr3_plan* P, size_t wu_cap, size_t slab_cap) {
  for (Rec& r : P->recs) {
    if (r.kind == R_CONV || r.kind == R_CONV_OUT) choose_dgrad(P, r.dx, wu_cap, slab_cap);
    if (r.kind == R_CONV && r.s.q0 >= 0) choose_dgrad(P, r.dq, wu_cap, slab_cap);
  }
}

// Shapes, parameter extents and the store-or-accumulate flags of every record's backward.  The activation-gradient mirror is NOT
// zeroed (round 6: 1.5 ms per step): the first contribution to a tensor's gradient in the backward walk -- the records in reverse,
// the destinations of a record in the order run_train writes them -- is a plain store, later ones accumulate in stream order
int resolve_backward(sr3_plan* P, int B) {
  const std::vector<Tensor>& T = P->ttens;
  std::vector<char> seen(T.size(), 0);
  auto acc = [&](int h) { if (h < 0) return true; const bool a = seen[h]; seen[h] = 1; return a; };
  auto pend = [](size_t off, size_t n) { return off + n; };
  for (int ri = (int)P->recs.size() - 1; ri >= 0; --ri) {
    Rec& r = P->recs[ri];
    const ConvSpec& s = r.s;
    if (r.kind == R_ATTN) {
      // attention_backward stores the qkv gradient: nothing may have written it before (with today's walk a qkv tensor has one consumer)
      if (acc(r.qkv)) { set_error("train: the qkv gradient has an earlier writer"); return SR3_E_UNSUPPORTED; }
      continue;
    }
    r.dw = wgrad_shape(P, r, B);
    if (r.kind != R_CONV_IN) r.dx.c = dgrad_shape(r.dw);
    if (r.kind == R_CONV) {
      r.acc_r0 = acc(s.r0); r.acc_r1 = acc(s.r1);
      if (s.q0 >= 0) {
        r.dqw = wgrad_q_shape(P, r, B);
        r.dq.c = dgrad_shape(r.dqw);
        r.acc_q0 = acc(s.q0); r.acc_q1 = acc(s.q1);
      }
    }
    if (r.kind != R_CONV_IN) { r.acc_x0 = acc(s.x0); r.acc_x1 = acc(s.x1); }
    // parameters: the conv's own (the arena holds the real channel counts, not the padded ones), its GroupNorm's, res_conv's
    const size_t cout = r.kind == R_CONV_OUT ? P->out_ch : r.dw.Cout, cin = r.kind == R_CONV_IN ? P->d.in_channel : r.dw.C0 + r.dw.C1;
    r.param_end = pend(s.w, cout * s.ksize * s.ksize * cin);
    if (s.bias != NO_OFF) r.param_end = std::max(r.param_end, pend(s.bias, cout));
    if (s.act) r.param_end = std::max({r.param_end, pend(r.gamma, cin), pend(r.beta, cin)});
    if (s.q0 >= 0) r.param_end = std::max({r.param_end, pend(s.qw, cout * (r.dqw.C0 + r.dqw.C1)), pend(s.qb, cout)});
  }
  return SR3_OK;
}
}  // namespace

int build_train(sr3_plan* P, int B, int cond_channels) {
  if (const int rc = check_out_rows(P)) return rc;
  if (!P->opt.train_geom && !plan_native_geometry(P)) {
    set_error("training runs at image_size x image_size only: the plan's geometry is %d x %d (sr3_plan_set_geometry(plan, 0, 0) restores %d x %d)",
              plan_height(P), plan_width(P), P->d.image_size, P->d.image_size);
    return SR3_E_UNSUPPORTED;
  }
  // (the geometry is the native one here unless train_geom; every option that changes the plan resets train_batch: sr3_plan_set_option)
  const int IH = plan_height(P), IW = plan_width(P);
  if (P->train_batch == B && P->train_cond == cond_channels && P->train_h == IH && P->train_w == IW) return SR3_OK;
  const sr3_unet_desc& d = P->d;
  if (B <= 0) { set_error("batch must be > 0"); return SR3_E_BADARG; }
  if (cond_channels < 0 || cond_channels >= d.in_channel) { set_error("cond_channels out of range"); return SR3_E_BADARG; }
  P->train_batch = -1;
  const TrainWalk fw = walk_train(P, B, cond_channels);
  // a plan is refused HERE, when it is built, never after a launch has been enqueued: a geometry no kernel can run (as build_forward) ...
  int rc = SR3_OK;
  if (!fw.refused.empty()) { set_error("training geometry %d x %d unsupported: %s", IH, IW, fw.refused.c_str()); rc = SR3_E_UNSUPPORTED; }
  else rc = resolve_backward(P, B);      // ... and a record list the backward walk cannot run
  if (rc) {
    P->tops.clear();
    P->recs.clear();
    return rc;
  }
  choose_dgrads(P, ~(size_t)0, ~(size_t)0);      // every kernel the data gradients could run on: the regions are sized by these
  const size_t S2 = (size_t)IH * IW;
  const int inner = d.inner_channel, G = d.norm_groups;
  auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
  auto raise = [](size_t& m, size_t v) { m = std::max(m, v); };
  auto fbytes = [](const ConvParams& c, size_t channels) { return (size_t)c.B * c.Ho * c.Wo * channels * sizeof(float); };
  // backward scratch: every region is the maximum over the resolved records
  size_t max_dA = 0, max_z = 0, max_dq = 0, max_wt = 0, max_wu = 0, max_slab = 0, max_part = 0, max_dwtmp = 0;
  size_t max_bscratch = 0;                    // split-K slabs of the data-gradient convs, dK / dV slabs of the attention backward
  for (const Rec& r : P->recs) {
    if (r.kind == R_ATTN) {
      raise(max_bscratch, attention_backward_scratch_bytes(B, P->ttens[r.o].H * P->ttens[r.o].W, P->ttens[r.o].C));
      continue;
    }
    const ConvParams& w = r.dw;
    raise(max_slab, wgrad_slab_bytes(w));
    raise(max_part, (size_t)B * chan_stats_slices(B, w.Ho * w.Wo, w.Cout) * w.Cout * 2 * sizeof(double));      // colsums of dOut
    if (r.kind != R_CONV) raise(max_dwtmp, (size_t)w.Cout * 9 * w.C0 * sizeof(float));       // padded filters, compacted into the arena
    if (r.kind == R_CONV_IN) continue;
    const ConvParams& g = r.dx.c;
    raise(max_part, act_bwd_part_bytes(B, w.Hs * w.Ws, w.C0 + w.C1));
    raise(max_dA, fbytes(g, g.Cout));
    raise(max_wt, (size_t)g.C0 * g.ksize * g.ksize * g.Cout * sizeof(float));
    if (w.stride == 2) raise(max_z, 4 * fbytes(w, w.Cout));
    raise(max_bscratch, conv_splitk_bytes(g, 0, 0));
    // KEPT QUIRK: only the Winograd data gradients of the R_CONV records size t_wu and the tile-11 slabs.  Neither the output conv's
    // Winograd form nor any tile-22 data gradient is sized for: they run where some other layer made the regions large enough (below)
    if (r.kind == R_CONV && r.dx.tile == 11) {
      raise(max_bscratch, conv_splitk_bytes(g, 11, 0));
      raise(max_wu, wu_bytes(r.dx));
    }
    if (r.s.q0 >= 0) {
      raise(max_slab, wgrad_slab_bytes(r.dqw));
      raise(max_dq, fbytes(r.dq.c, r.dq.c.Cout));
      raise(max_wt, (size_t)r.dq.c.C0 * r.dq.c.Cout * sizeof(float));
      raise(max_bscratch, conv_splitk_bytes(r.dq.c, 0, 0));
    }
  }
  size_t off = al(fw.act_high);
  P->t_act_bytes = off;
  off *= 2;                                   // gradients mirror the activations at +t_act_bytes
  Regions& R = P->t_regions;
  R.stats_off = off; off += al(fw.stats_bytes);
  R.ss_off = off; off += al(fw.gn_bytes);                  // per-GroupNorm scale / shift tables, kept for the backward
  R.mr_off = off; off += al(fw.mr_bytes);                  // ... and mean / rstd tables
  R.temb_off = off; off += al((size_t)B * inner * sizeof(float));
  R.film_off = off; off += al((size_t)B * P->film_rows() * sizeof(float));
  R.scratch_bytes = std::max(fw.max_scratch, max_bscratch);      // the forward's split-K region doubles as the backward's
  R.scratch_off = off; off += al(R.scratch_bytes);
  P->t_dA_off = off; off += al(max_dA);
  P->t_a_off = off; off += al(max_dA);       // materialised activated input of the weight-gradient GEMM
  P->t_z_off = off; off += al(max_z);
  P->t_dq_off = off; off += al(max_dq);
  P->t_wt_off = off; off += al(max_wt);
  P->t_wu_off = off; P->t_wu_bytes = max_wu; off += al(max_wu);
  P->t_slab_off = off; off += al(max_slab);
  P->t_part_off = off; off += al(max_part);
  P->t_gs_off = off; off += al((size_t)B * G * 2 * sizeof(double));
  P->t_dfilm_off = off; off += al((size_t)B * P->film_rows() * sizeof(float));
  P->t_xnoisy_off = off; off += al((size_t)B * (d.in_channel - cond_channels) * S2 * sizeof(float));
  P->t_eps_off = off; off += al((size_t)B * P->out_ch * S2 * sizeof(float));
  P->t_geps_off = off; off += al((size_t)B * S2 * out_pad(P) * sizeof(float));
  P->t_inpad_off = off; off += al((size_t)B * S2 * in_pad(d.in_channel) * sizeof(float));
  P->t_dwtmp_off = off; off += al(4096 * sizeof(double)) + al(max_dwtmp);      // [loss partials | dw temp]
  P->t_embscr_off = off; off += al((size_t)B * (13 + 16) * inner * sizeof(float));     // (+ the 16 row chunks of k_film_bwd_input)
  P->t_ws_bytes = off;
  // KEPT QUIRK: THIS PASS settles the kernels that read derived filters nothing above sized for -- taken exactly where the filters fit
  // t_wu and (tile 22) the slabs fit t_scratch as sized.  Sizing for them would move workspace sizes and kernel choices: a change of its own
  choose_dgrads(P, P->t_wu_bytes, R.scratch_bytes);
  // gradient-ready marks: t_unproc_max[k] = largest arena offset (exclusive end) among the parameters whose
  // gradients are still unwritten once records k .. end have been processed (records < k + the FiLM /
  // embedding block at the arena head, which is written last)
  const size_t nrec = P->recs.size();
  P->t_unproc_max.assign(nrec + 1, 0);
  size_t run = std::max(P->emb_b2 + (size_t)inner, P->film_b + (size_t)P->film_rows());
  for (size_t k = 0; k < nrec; ++k) {
    P->t_unproc_max[k] = run;
    run = std::max(run, P->recs[k].param_end);
  }
  P->t_unproc_max[nrec] = run;
  P->train_batch = B;
  P->train_cond = cond_channels;
  P->train_h = IH; P->train_w = IW;
  return SR3_OK;
}

namespace {
// the buffers of one data-gradient conv: run_train binds the regions of its workspace, sr3_conv_dgrad_f32 the caller's scratch
struct DgradBufs {
  float* wt;            // the flipped-transposed filters [Cin][taps][Cg]
  float* wu;            // the derived filters of Dgrad::wu (not read with WU_NONE)
  float* z;             // the zero-inserted dOut of a stride-2 conv [B, 2 Ho, 2 Wo, Cg] (not read at stride 1)
  float* slabs;         // split-K slabs
  size_t slab_bytes;
};
struct TrainCtx {
  sr3_plan* P;
  char* ws;
  const float* params;
  float* grads;
  int B;
  hipStream_t st;
  const float* act(int h) const { return reinterpret_cast<const float*>(ws + P->ttens[h].off); }
  float* grad(int h) const { return h >= 0 ? reinterpret_cast<float*>(ws + P->t_act_bytes + P->ttens[h].off) : nullptr; }
  template <typename T> T* at(size_t off) const { return reinterpret_cast<T*>(ws + off); }
  DgradBufs dgrad_bufs() const {
    return DgradBufs{at<float>(P->t_wt_off), at<float>(P->t_wu_off), at<float>(P->t_z_off), at<float>(P->t_regions.scratch_off),
                     P->t_regions.scratch_bytes};
  }
};

// dOut [B,H,W,Cg] --(conv with flipped-transposed weights)--> dA [B,H,W,Cin], on the kernel choose_dgrad chose; the arena holds
// `Cout_w` <= Cg of the Cg filters (the output conv's padding).  stride 2: dOut is [B,Ho,Wo,Cg] and is zero-inserted first
int dgrad_conv(const Dgrad& d, int stride, int Ho, int Wo, const float* g, const float* w, int Cout_w, float* dA, const DgradBufs& b, int gemm_epi,
               hipStream_t st) {
  ConvParams c = d.c;
  int rc;
  if (stride == 2) {
    rc = zero_insert(g, c.B, Ho, Wo, c.C0, b.z, st);
    if (rc) return rc;
    g = b.z;
  }
  rc = w_flip_transpose(w, Cout_w, c.ksize * c.ksize, c.Cout, c.C0, b.wt, st);
  if (rc) return rc;
  c.src0 = g; c.w = b.wt; c.out = dA;
  c.gemm_epi = 1 + gemm_epi;      // (plan option gemm_epi, read at launch: the data gradients on the GEMM kernel follow it; -1: not set)
  if (d.wu == WU_GEMM) { rc = igemm_split_weights(b.wt, c.Cout, 1, c.C0, b.wu, st); c.w_split = b.wu; }
  else if (d.wu != WU_NONE) { rc = wino_transform_weights(b.wt, c.Cout, c.C0, b.wu, st, d.wu == WU_WINO_SPLIT); c.wino_u = b.wu; }
  if (rc) return rc;
  return conv_forward(c, d.tile, d.ksplit, b.slabs, b.slab_bytes, st);
}

// weight gradient of the shape `c` over the sources src0 | src1.  wgrad_split is a no-rebuild option: the slabs are sized for both
// values, and conv_wgrad picks the kernel and the pixel split at launch
int wgrad_call(const TrainCtx& X, ConvParams c, const float* src0, const float* src1, const float* dy, float* dw) {
  WgradParams wp;
  c.src0 = src0; c.src1 = src1;
  c.wgrad_split = X.P->opt.wgrad_split;
  wp.c = c;
  wp.dy = dy;
  wp.dw = dw;
  wp.slabs = X.at<float>(X.P->t_slab_off);
  return conv_wgrad(wp, X.st);
}
}  // namespace

// one step as train_step_checked settled it: nothing is refused from here on
int run_train(sr3_plan* P, const TrainStep& t) {
  const sr3_unet_desc& d = P->d;
  const float* params = t.params; float* grads = t.grads; char* ws = static_cast<char*>(t.workspace);
  const int B = t.batch;
  hipStream_t st = t.stream;
  // image geometry of this step: build_train built the plan for it (the native one unless plan option train_geom)
  const int IH = P->train_h, IW = P->train_w, S2 = IH * IW, G = d.norm_groups;
  const int xc = d.in_channel - t.cond_channels;
  TrainCtx X{P, ws, params, grads, B, st};
  int rc;
  // ---- q_sample + forward ----
  float* x_noisy = X.at<float>(P->t_xnoisy_off);
  float* eps = X.at<float>(P->t_eps_off);
  rc = q_sample(t.hr, t.z, t.q_ca, t.q_cb, B, xc * S2, x_noisy, st);
  if (rc) return rc;
  DropCfg dc;
  dc.seed = t.dropout_seed;
  dropout_consts(t.dropout_p, &dc.thresh, &dc.scale);
  const ForwardCall fwd = {.x = x_noisy, .cond = t.cond, .cond_channels = t.cond_channels, .level = t.level, .tstep = t.tstep, .freq = t.freq,
                           .params = params, .workspace = ws, .eps_out = eps, .batch = B, .stream = st, .drop = &dc, .train = true};
  rc = run_forward(P, fwd);
  if (rc) return rc;
  // ---- loss and its gradient (NHWC, channel dim padded to 4) ----
  float* geps = X.at<float>(P->t_geps_off);
  double* lparts = X.at<double>(P->t_dwtmp_off);
  // (target z, weight 1 and L1 / L2 -- sr3_train_step's objective -- is the plain form of the loss kernel: objective_loss_grad)
  // (obj.hyb, a variance head: L_simple on the prediction rows + lambda L_vlb on the variance rows, the same kernel; without one
  // the image's channels are all of out_ch)
  const int OUT_PAD = out_pad(P);
  rc = objective_loss_grad({t.z, t.hr, x_noisy, eps, geps, lparts, t.loss_sum_out, t.vlb_sum_out}, t.obj, B, plan_image_channels(P), S2, OUT_PAD,
                           t.grad_scale, st);
  if (rc) return rc;
  if (t.pi.out) {     // sr3_train_step_ex3: the per-image terms of the bound on the step's own x_noisy and output, while both are live
    const int Cc = plan_image_channels(P);
    rc = vlb_terms(t.hr, x_noisy, eps, t.pi.scal, B, nullptr, nullptr, t.obj.hyb ? 0 : 1, false, B, Cc, t.obj.hyb ? 2 * Cc : Cc, S2, t.pi.out, t.pi.out + 1, 2,
                   t.pi.part, st);
    if (rc) return rc;
  }
  // ---- the backward walk: the records in reverse, each as build_train resolved it.  The activation-gradient mirror is not zeroed
  // (Rec::acc_*).  The FiLM gradient table is, as a precaution only: every row of it belongs to exactly one conv, whose colsums below
  // stores it -- or (scale_shift) to the one GroupNorm it modulates, whose act_bwd stores it -- so with today's walk no element of the
  // table is read before it is written ----
  const int FR = P->film_rows();
  float* dfilm = X.at<float>(P->t_dfilm_off);
  const float* film = X.at<float>(P->t_regions.film_off);      // the forward's FiLM table (the modulation rows of scale_shift)
  SR3_HIP(hipMemsetAsync(dfilm, 0, (size_t)B * FR * sizeof(float), st));

  float* dA = X.at<float>(P->t_dA_off);
  double* part = X.at<double>(P->t_part_off);
  double* gs = X.at<double>(P->t_gs_off);
  float* dwtmp = reinterpret_cast<float*>(ws + P->t_dwtmp_off + 4096 * sizeof(double));

  int next_mark = 0;
  for (int ri = (int)P->recs.size() - 1; ri >= 0; --ri) {
    // gradient-ready marks: every parameter at arena offset >= marks[k] has its gradient enqueued
    while (next_mark < t.n_marks && P->t_unproc_max[ri + 1] <= t.mark_offsets[next_mark]) {
      SR3_HIP(hipEventRecord(static_cast<hipEvent_t>(t.mark_events[next_mark]), st));
      ++next_mark;
    }
    const Rec& r = P->recs[ri];
    const ConvSpec& s = r.s;
    float* abuf = X.at<float>(P->t_a_off);        // the activated input of a conv, written by act_bwd's first pass
    if (r.kind == R_CONV_OUT) {
      const int C = r.dw.C0;
      // bias (3 of the 4 padded columns are real -- 6 of 8 with a variance head; arena slots are 4-float aligned)
      rc = colsums(geps, B, S2, OUT_PAD, part, grads + s.bias, nullptr, 0, st);
      if (rc) return rc;
      rc = dgrad_conv(r.dx, 1, r.dw.Ho, r.dw.Wo, geps, params + s.w, P->out_ch, dA, X.dgrad_bufs(), P->opt.launch_gemm_epi(), st);
      if (rc) return rc;
      rc = act_bwd(dA, X.act(s.x0), nullptr, C, 0, B, S2, X.at<float>(P->t_regions.ss_off + r.ss_off),
                   X.at<float>(P->t_regions.mr_off + r.mr_off), G, s.act, params + r.gamma, part, gs, grads + r.gamma,
                   grads + r.beta, X.grad(s.x0), nullptr, st, 0u, 0u, 1.f, abuf, r.acc_x0, true);
      if (rc) return rc;
      rc = wgrad_call(X, r.dw, abuf, nullptr, geps, dwtmp);
      if (rc) return rc;
      SR3_HIP(hipMemcpyAsync(grads + s.w, dwtmp, (size_t)P->out_ch * 9 * C * sizeof(float), hipMemcpyDeviceToDevice, st));
    } else if (r.kind == R_ATTN) {
      const Tensor& o = P->ttens[r.o];
      // dK / dV through per-query-block slabs in the backward's scratch region, summed in block order: no atomics (round 6)
      rc = attention_backward(X.act(r.qkv), X.grad(r.o), X.act(r.o), B, o.H * o.W, o.C, X.grad(r.qkv), st,
                              X.at<float>(P->t_regions.scratch_off), P->t_regions.scratch_bytes, r.heads);
      if (rc) return rc;
    } else if (r.kind == R_CONV_IN) {
      const int Cout = r.dw.Cout;
      float* inpad = X.at<float>(P->t_inpad_off);
      const float* a = t.cond_channels > 0 ? t.cond : x_noisy;
      const int Ca = t.cond_channels > 0 ? t.cond_channels : xc;
      const float* b2 = t.cond_channels > 0 ? x_noisy : nullptr;
      const int Cb = t.cond_channels > 0 ? xc : 0;
      const int CP = in_pad(d.in_channel);
      rc = nchw_to_nhwc_pad(a, Ca, b2, Cb, B, S2, CP, inpad, st);
      if (rc) return rc;
      rc = colsums(X.grad(r.out), B, S2, Cout, part, grads + s.bias, nullptr, 0, st);
      if (rc) return rc;
      rc = wgrad_call(X, r.dw, inpad, nullptr, X.grad(r.out), dwtmp);
      if (rc) return rc;
      // compact [Cout][9][CP] -> [Cout][9][in_channel]
      SR3_HIP(hipMemcpy2DAsync(grads + s.w, (size_t)d.in_channel * sizeof(float), dwtmp, CP * sizeof(float),
                               (size_t)d.in_channel * sizeof(float), (size_t)Cout * 9, hipMemcpyDeviceToDevice, st));
    } else {
      const Tensor& x0 = P->ttens[s.x0];
      const int C0 = x0.C, C1 = s.x1 >= 0 ? P->ttens[s.x1].C : 0;
      const int Ho = r.dw.Ho, Wo = r.dw.Wo, Cout = r.dw.Cout;
      const bool bias_grad = s.bias != NO_OFF, has_q = s.q0 >= 0;
      const float* g = X.grad(r.out);
      const float* x0p = X.act(s.x0);
      const float* x1p = s.x1 >= 0 ? X.act(s.x1) : nullptr;
      // 1. bias and FiLM gradients: column sums of dOut
      if (bias_grad || s.film_row >= 0 || has_q) {
        rc = colsums(g, B, Ho * Wo, Cout, part, bias_grad ? grads + s.bias : nullptr,
                     s.film_row >= 0 ? dfilm + s.film_row : nullptr, FR, st);
        if (rc) return rc;
        if (has_q)        // res_conv bias sees the same sums
          SR3_HIP(hipMemcpyAsync(grads + s.qb, grads + s.bias, (size_t)Cout * sizeof(float), hipMemcpyDeviceToDevice, st));
      }
      // 2. identity residual
      if (s.r0 >= 0) {
        rc = grad_route(g, P->ttens[s.r0].C, s.r1 >= 0 ? P->ttens[s.r1].C : 0, B, Ho, Wo, 0, X.grad(s.r0), X.grad(s.r1), st,
                        r.acc_r0, r.acc_r1);
        if (rc) return rc;
      }
      // 3. fused res_conv segment
      if (has_q) {
        float* dq = X.at<float>(P->t_dq_off);
        rc = dgrad_conv(r.dq, 1, Ho, Wo, g, params + s.qw, Cout, dq, X.dgrad_bufs(), P->opt.launch_gemm_epi(), st);
        if (rc) return rc;
        rc = grad_route(dq, r.dqw.C0, r.dqw.C1, B, Ho, Wo, 0, X.grad(s.q0), X.grad(s.q1), st, r.acc_q0, r.acc_q1);
        if (rc) return rc;
        rc = wgrad_call(X, r.dqw, X.act(s.q0), s.q1 >= 0 ? X.act(s.q1) : nullptr, g, grads + s.qw);
        if (rc) return rc;
      }
      // 4. main segment: data gradient
      rc = dgrad_conv(r.dx, s.stride, Ho, Wo, g, params + s.w, Cout, dA, X.dgrad_bufs(), P->opt.launch_gemm_epi(), st);
      if (rc) return rc;
      if (s.act) {
        const bool dropped = s.drop_key >= 0 && dc.thresh != 0;
        const unsigned lseed = drop_layer_seed(dc.seed, (unsigned)(s.drop_key >= 0 ? s.drop_key : 0));
        // scale_shift: this conv's GroupNorm was folded under the block's rows of the FiLM table; their gradients go to the same rows of dfilm
        const int mrow = s.gn.mod_row;
        const ModBwd md = {film + (mrow >= 0 ? mrow : 0), FR, params + r.beta, dfilm + (mrow >= 0 ? mrow : 0)};
        rc = act_bwd(dA, x0p, x1p, C0, C1, B, x0.H * x0.W, X.at<float>(P->t_regions.ss_off + r.ss_off),
                     X.at<float>(P->t_regions.mr_off + r.mr_off), G, s.act, params + r.gamma, part, gs, grads + r.gamma,
                     grads + r.beta, X.grad(s.x0), X.grad(s.x1), st, lseed, dropped ? dc.thresh : 0u, dc.scale, abuf, r.acc_x0, r.acc_x1,
                     mrow >= 0 ? &md : nullptr);
      } else {
        rc = grad_route(dA, C0, C1, B, x0.H, x0.W, s.ups, X.grad(s.x0), X.grad(s.x1), st, r.acc_x0, r.acc_x1);
      }
      if (rc) return rc;
      // 5. weight gradient.  The activated (and dropped) input is materialised once instead of being recomputed per tap: by act_bwd's
      // first pass above (round 6; it was a pass of its own over x, k_apply_act)
      rc = s.act ? wgrad_call(X, r.dw, abuf, nullptr, g, grads + s.w) : wgrad_call(X, r.dw, x0p, x1p, g, grads + s.w);
      if (rc) return rc;
    }
  }
  while (next_mark < t.n_marks && P->t_unproc_max[0] <= t.mark_offsets[next_mark]) {
    SR3_HIP(hipEventRecord(static_cast<hipEvent_t>(t.mark_events[next_mark]), st));
    ++next_mark;
  }
  // ---- embedding MLP and FiLM projections ----
  EmbedBwdParams e;
  memset(&e, 0, sizeof(e));
  e.variant = d.variant; e.B = B; e.inner = d.inner_channel; e.F = FR; e.level = t.level; e.tstep = t.tstep; e.freq = t.freq;
  e.w1 = params + P->emb_w1; e.b1 = params + P->emb_b1; e.w2 = params + P->emb_w2; e.b2 = params + P->emb_b2;
  e.wf = params + P->film_w; e.dfilm = dfilm;
  e.dw1 = grads + P->emb_w1; e.db1 = grads + P->emb_b1; e.dw2 = grads + P->emb_w2; e.db2 = grads + P->emb_b2;
  e.dwf = grads + P->film_w; e.dbf = grads + P->film_b;
  e.scratch = X.at<float>(P->t_embscr_off);
  rc = embed_backward(e, st);
  if (rc) return rc;
  while (next_mark < t.n_marks) {       // whatever is left becomes ready with the head block
    SR3_HIP(hipEventRecord(static_cast<hipEvent_t>(t.mark_events[next_mark]), st));
    ++next_mark;
  }
  return SR3_OK;
}

// ---- the data gradient of one conv on caller-owned tensors (sr3_conv_dgrad_f32): run_train's choose_dgrad and dgrad_conv ----
namespace {
// the argument checks of the two entries and the shape of the forward conv; nothing is launched
int dgrad_entry_shape(const char* who, const sr3_plan* plan, int B, int Hs, int Ws, int ups, int stride, int ksize, int Cin, int CoutP,
                      ConvParams* f) {
  if (!plan) { set_error("%s: plan is NULL", who); return SR3_E_BADARG; }
  if (B <= 0 || Hs <= 0 || Ws <= 0 || Cin <= 0 || CoutP <= 0) { set_error("%s: batch %d, map %d x %d and channels %d -> %d must be positive", who, B, Hs, Ws, Cin, CoutP); return SR3_E_BADARG; }
  if ((ups != 0 && ups != 1) || (stride != 1 && stride != 2) || (ksize != 1 && ksize != 3)) {
    set_error("%s: ups %d / stride %d / ksize %d out of range (ups 0 | 1, stride 1 | 2, ksize 1 | 3)", who, ups, stride, ksize);
    return SR3_E_BADARG;
  }
  if (ups && stride == 2) { set_error("%s: an upsampled stride-2 conv is unsupported", who); return SR3_E_UNSUPPORTED; }
  if ((Cin & 3) || (CoutP & 3)) { set_error("%s: channel counts must be multiples of 4 (Cin %d, CoutP %d)", who, Cin, CoutP); return SR3_E_UNSUPPORTED; }
  // dgrad_shape takes the data gradient's map to be the forward input's, zero_insert writes [2 Ho, 2 Wo]: they agree on even maps only
  if (stride == 2 && ((Hs & 1) || (Ws & 1))) { set_error("%s: a stride-2 conv needs an even input map (%d x %d)", who, Hs, Ws); return SR3_E_UNSUPPORTED; }
  if ((double)B * (Hs << ups) * (Ws << ups) * (double)(Cin > CoutP ? Cin : CoutP) >= 2147483647.0) { set_error("%s: tensor exceeds 2^31 elements", who); return SR3_E_UNSUPPORTED; }
  *f = conv_shape(B, Hs, Ws, ups, stride, ksize, Cin, 0, CoutP);
  return SR3_OK;
}
// THE layout of the entry's scratch: [wt | z | slabs], byte offsets; `slabs` is also the bytes in front of the split-K slabs
struct DgradScratch {
  size_t z, slabs;
  explicit DgradScratch(const ConvParams& f) {
    z = al256((size_t)f.Cout * f.ksize * f.ksize * f.C0 * sizeof(float));
    slabs = z + al256(f.stride == 2 ? (size_t)f.B * f.Hs * f.Ws * f.Cout * sizeof(float) : 0);
  }
  DgradBufs bind(void* scratch, size_t scratch_bytes, void* derived) const {
    char* s = static_cast<char*>(scratch);
    return DgradBufs{reinterpret_cast<float*>(s), static_cast<float*>(derived), reinterpret_cast<float*>(s + z),
                     reinterpret_cast<float*>(s + slabs), scratch_bytes - slabs};
  }
};
}  // namespace

}  // namespace sr3

extern "C" {

size_t sr3_conv_dgrad_scratch_bytes(sr3_plan* plan, int B, int Hs, int Ws, int ups, int stride, int ksize, int Cin, int CoutP,
                                    size_t* derived_bytes, size_t* base_bytes) {
  if (derived_bytes) *derived_bytes = 0;
  if (base_bytes) *base_bytes = 0;
  ConvParams f;
  if (dgrad_entry_shape("sr3_conv_dgrad_scratch_bytes", plan, B, Hs, Ws, ups, stride, ksize, Cin, CoutP, &f)) return 0;
  Dgrad d;
  d.c = dgrad_shape(f);
  choose_dgrad(plan, d, ~(size_t)0, ~(size_t)0);       // the kernel it runs with room for everything ...
  size_t slabs = conv_splitk_bytes(d.c, d.tile, d.ksplit);
  if (derived_bytes) *derived_bytes = wu_bytes(d);
  choose_dgrad(plan, d, 0, 0);                         // ... and the general one it falls back to without
  slabs = std::max(slabs, conv_splitk_bytes(d.c, d.tile, d.ksplit));
  const DgradScratch lay(f);
  if (base_bytes) *base_bytes = lay.slabs;
  return lay.slabs + al256(slabs);
}

int sr3_conv_dgrad_f32(sr3_plan* plan, const float* dy, const float* w_ohwi, int Cout_w, int CoutP, int B, int Hs, int Ws, int ups,
                       int stride, int ksize, int Cin, float* dA, void* scratch, size_t scratch_bytes, void* derived,
                       size_t derived_bytes, int* tile_out, int* ksplit_out, int* derived_kind_out, void* stream) {
  const char* who = "sr3_conv_dgrad_f32";
  ConvParams f;
  if (const int rc = dgrad_entry_shape(who, plan, B, Hs, Ws, ups, stride, ksize, Cin, CoutP, &f)) return rc;
  if (!dy || !w_ohwi || !dA || !scratch) { set_error("%s: dy / w_ohwi / dA / scratch is NULL", who); return SR3_E_BADARG; }
  if (Cout_w <= 0 || Cout_w > CoutP) { set_error("%s: Cout_w %d is outside 1..CoutP (%d)", who, Cout_w, CoutP); return SR3_E_BADARG; }
  if (((uintptr_t)scratch & 255) || ((uintptr_t)derived & 255)) { set_error("%s: scratch / derived is not 256-byte aligned", who); return SR3_E_ALIGN; }
  const DgradScratch lay(f);
  if (scratch_bytes < lay.slabs) { set_error("%s: scratch too small (%zu < %zu)", who, scratch_bytes, lay.slabs); return SR3_E_NOMEM; }
  const DgradBufs bufs = lay.bind(scratch, scratch_bytes, derived);
  Dgrad d;
  d.c = dgrad_shape(f);
  // choose_dgrad's caps are what the caller passed: derived filters that do not fit -- or split-K slabs of the GEMM kernel that do
  // not -- send the conv to the general kernels, whose own slabs must fit
  choose_dgrad(plan, d, derived ? derived_bytes : 0, bufs.slab_bytes);
  const size_t slabs = conv_splitk_bytes(d.c, d.tile, d.ksplit);
  // the query rounds the slabs up to 256 bytes, and so does this check: what is refused is exactly a scratch below the chosen kernel's
  // query.  (choose_dgrad above is capped by the unrounded room, so a scratch less than 256 bytes short of the rounded size is refused
  // here instead of running: such a caller is below the query either way)
  if (bufs.slab_bytes < al256(slabs)) { set_error("%s: scratch too small (%zu < %zu)", who, scratch_bytes, lay.slabs + al256(slabs)); return SR3_E_NOMEM; }
  const ConvPick pk = conv_pick(d.c, d.tile, d.ksplit);      // (what conv_forward resolves tile 0 / ksplit 0 to)
  if (tile_out) *tile_out = tile_encode(pk.tile, d.c.wino_split, d.c.igemm_split, false);
  if (ksplit_out) *ksplit_out = pk.ksplit;
  if (derived_kind_out) *derived_kind_out = d.wu;
  return dgrad_conv(d, stride, f.Ho, f.Wo, dy, w_ohwi, Cout_w, dA, bufs, plan->opt.launch_gemm_epi(), static_cast<hipStream_t>(stream));
}

size_t sr3_train_workspace_bytes(sr3_plan* plan, int batch, int cond_channels) {
  if (!plan) return 0;
  if (build_train(plan, batch, cond_channels)) return 0;
  return plan->t_ws_bytes;
}

// what an entry asks of the request it filled: sr3_train_step_ex ignores the hybrid and per-image fields (it leaves them unset),
// _ex2 needs step_scalars, _ex3 needs them too and takes the per-image terms -- on a plan without a variance head for those alone
enum TrainForm { TRAIN_EX, TRAIN_EX2, TRAIN_EX3 };

// THE checks of a training step, in the order the refusals are pinned in (tests/test_train_refusals_cpu.py); nothing has been launched
// when this returns non-zero without reaching run_train.  `who` names the entry in its refusals
static int train_step_checked(const char* who, sr3_plan* plan, TrainStep t, TrainForm form) {
  if (form != TRAIN_EX && !t.obj.hyb) { set_error("%s: step_scalars is NULL", who); return SR3_E_BADARG; }
  if (!plan || !t.hr || !t.z || !t.q_ca || !t.q_cb || !t.freq || !t.params || !t.grads || !t.workspace || !t.loss_sum_out) {
    set_error("null argument");
    return SR3_E_BADARG;
  }
  Objective& obj = t.obj;
  if (const int rc = check_objective_args(who, obj.tgt_z, obj.tgt_x0, obj.weight, obj.kind, -1, obj.huber_delta)) return rc;
  if (!t.cond) t.cond_channels = 0;
  const int rc = build_train(plan, t.batch, t.cond_channels);
  if (rc) return rc;
  if (t.workspace_bytes < plan->t_ws_bytes) { set_error("train workspace too small: %zu < %zu", t.workspace_bytes, plan->t_ws_bytes); return SR3_E_NOMEM; }
  if (((uintptr_t)t.workspace & 255) || ((uintptr_t)t.params & 15) || ((uintptr_t)t.grads & 15)) { set_error("misaligned pointer"); return SR3_E_ALIGN; }
  if (plan->d.variant == SR3_VARIANT_SR3 && !t.level) { set_error("SR3 variant needs noise_level"); return SR3_E_BADARG; }
  if (plan->d.variant == SR3_VARIANT_DDPM && !t.tstep) { set_error("DDPM variant needs timestep"); return SR3_E_BADARG; }
  if (t.dropout_p < 0.f || t.dropout_p >= 1.f) { set_error("dropout_p out of range"); return SR3_E_BADARG; }
  if (form == TRAIN_EX3 && t.pi.out) {
    const size_t out_bytes = (size_t)t.batch * 2 * sizeof(float), need = vlb_terms_scratch(t.batch);
    if (!t.pi.part) { set_error("%s: scratch is NULL with per_image_out given", who); return SR3_E_BADARG; }
    if (t.pi_scratch_bytes < need) { set_error("%s: scratch too small (%zu < %zu)", who, t.pi_scratch_bytes, need); return SR3_E_NOMEM; }
    if (overlaps(t.pi.out, out_bytes, t.pi.part, need)) { set_error("%s: per_image_out overlaps scratch", who); return SR3_E_BADARG; }
    if (overlaps(t.workspace, plan->t_ws_bytes, t.pi.out, out_bytes) || overlaps(t.workspace, plan->t_ws_bytes, t.pi.part, need)) {
      set_error("%s: per_image_out / scratch overlaps the workspace", who);
      return SR3_E_BADARG;
    }
    if ((uintptr_t)t.pi.part & 7) { set_error("%s: scratch is not 8-byte aligned", who); return SR3_E_ALIGN; }
    t.pi.scal = obj.hyb;
  } else {
    t.pi = PerImage();
  }
  if (form == TRAIN_EX3 && plan->opt.var_channels == 0) obj.hyb = nullptr;      // no variance head: sr3_train_step_ex's objective; the rows serve the terms alone
  if ((plan->opt.var_channels > 0) != (obj.hyb != nullptr)) {
    set_error("%s: the plan's variance rows (var_channels %d) and step_scalars go together (sr3_train_step_ex2 trains them)", who, plan->opt.var_channels);
    return SR3_E_BADARG;
  }
  if (obj.hyb && !(isfinite(obj.lambda) && obj.lambda >= 0.f)) { set_error("%s: vlb_lambda %g must be finite and >= 0", who, (double)obj.lambda); return SR3_E_BADARG; }
  if (!obj.hyb) obj.vlb_w = nullptr;      // (a plan without a variance head has no L_vlb to weight)
  if (obj.kind < 0) obj.kind = plan->opt.loss_l2 != 0 ? LOSS_L2 : LOSS_L1;      // -1: the plan's loss_l2
  if (!t.mark_offsets || !t.mark_events) t.n_marks = 0;
  return run_train(plan, t);
}

// the arguments all four sr3_train_step* entries have (_COMMON) and the objective's, which the three _ex entries have (_OBJECTIVE), under
// the names every prototype gives them (include/sr3_mi355x.h), into the request `t`
#define SR3_TRAIN_STEP_COMMON(t)                                                                                                      \
  t.hr = hr_nchw; t.cond = cond_nchw; t.cond_channels = cond_channels; t.z = z_nchw; t.q_ca = q_ca; t.q_cb = q_cb;                    \
  t.level = noise_level; t.tstep = timestep; t.freq = freq; t.params = params; t.grads = grads;                                       \
  t.workspace = workspace; t.workspace_bytes = workspace_bytes; t.loss_sum_out = loss_sum_out; t.grad_scale = grad_scale;             \
  t.dropout_p = dropout_p; t.dropout_seed = dropout_seed;                                                                             \
  t.n_marks = n_marks; t.mark_offsets = mark_offsets; t.mark_events = mark_events;                                                    \
  t.batch = batch; t.stream = static_cast<hipStream_t>(stream)
#define SR3_TRAIN_STEP_OBJECTIVE(t) \
  t.obj.tgt_z = tgt_z; t.obj.tgt_x0 = tgt_x0; t.obj.weight = weight; t.obj.kind = loss_kind; t.obj.huber_delta = huber_delta

int sr3_train_step_ex(sr3_plan* plan, const float* hr_nchw, const float* cond_nchw, int cond_channels, const float* z_nchw,
                      const float* q_ca, const float* q_cb, const float* noise_level, const int64_t* timestep,
                      const float* freq, const float* params, float* grads, void* workspace, size_t workspace_bytes,
                      float* loss_sum_out, float grad_scale, float dropout_p, unsigned dropout_seed, int n_marks,
                      const size_t* mark_offsets, void* const* mark_events, int batch, const float* tgt_z, const float* tgt_x0,
                      const float* weight, int loss_kind, float huber_delta, void* stream) {
  TrainStep t;
  SR3_TRAIN_STEP_COMMON(t);
  SR3_TRAIN_STEP_OBJECTIVE(t);
  return train_step_checked("sr3_train_step_ex", plan, t, TRAIN_EX);
}

// ... of a plan with a variance head (plan option var_channels): the hybrid loss (sr3_hybrid_loss_grad_f32) in place of the pixel loss
int sr3_train_step_ex2(sr3_plan* plan, const float* hr_nchw, const float* cond_nchw, int cond_channels, const float* z_nchw,
                       const float* q_ca, const float* q_cb, const float* noise_level, const int64_t* timestep,
                       const float* freq, const float* params, float* grads, void* workspace, size_t workspace_bytes,
                       float* loss_sum_out, float grad_scale, float dropout_p, unsigned dropout_seed, int n_marks,
                       const size_t* mark_offsets, void* const* mark_events, int batch, const float* tgt_z, const float* tgt_x0,
                       const float* weight, int loss_kind, float huber_delta, const float* step_scalars, float vlb_lambda,
                       float* vlb_sum_out, void* stream) {
  TrainStep t;
  SR3_TRAIN_STEP_COMMON(t);
  SR3_TRAIN_STEP_OBJECTIVE(t);
  t.obj.hyb = step_scalars; t.obj.lambda = vlb_lambda; t.vlb_sum_out = vlb_sum_out;
  return train_step_checked("sr3_train_step_ex2", plan, t, TRAIN_EX2);
}

// sr3_train_step_ex2 (a plan with a variance head) or sr3_train_step_ex (one without: fixed small variance) with the per-image terms of
// the bound behind the loss kernel: the same launches, and one pair of sr3_vlb_terms_f32's where per_image_out is given
int sr3_train_step_ex3(sr3_plan* plan, const float* hr_nchw, const float* cond_nchw, int cond_channels, const float* z_nchw,
                       const float* q_ca, const float* q_cb, const float* noise_level, const int64_t* timestep,
                       const float* freq, const float* params, float* grads, void* workspace, size_t workspace_bytes,
                       float* loss_sum_out, float grad_scale, float dropout_p, unsigned dropout_seed, int n_marks,
                       const size_t* mark_offsets, void* const* mark_events, int batch, const float* tgt_z, const float* tgt_x0,
                       const float* weight, int loss_kind, float huber_delta, const float* step_scalars, float vlb_lambda,
                       float* vlb_sum_out, float* per_image_out, void* scratch, size_t scratch_bytes, const float* vlb_weight,
                       void* stream) {
  TrainStep t;
  SR3_TRAIN_STEP_COMMON(t);
  SR3_TRAIN_STEP_OBJECTIVE(t);
  t.obj.hyb = step_scalars; t.obj.lambda = vlb_lambda; t.vlb_sum_out = vlb_sum_out;
  t.obj.vlb_w = vlb_weight;
  t.pi.out = per_image_out; t.pi.part = static_cast<double*>(scratch); t.pi_scratch_bytes = scratch_bytes;
  return train_step_checked("sr3_train_step_ex3", plan, t, TRAIN_EX3);
}
// sr3_train_step_ex with its own objective: target z, weight 1, the plan's loss (refusals under that entry's name, as ever)
int sr3_train_step(sr3_plan* plan, const float* hr_nchw, const float* cond_nchw, int cond_channels, const float* z_nchw,
                   const float* q_ca, const float* q_cb, const float* noise_level, const int64_t* timestep,
                   const float* freq, const float* params, float* grads, void* workspace, size_t workspace_bytes,
                   float* loss_sum_out, float grad_scale, float dropout_p, unsigned dropout_seed, int n_marks,
                   const size_t* mark_offsets, void* const* mark_events, int batch, void* stream) {
  TrainStep t;
  SR3_TRAIN_STEP_COMMON(t);
  t.obj.kind = -1; t.obj.huber_delta = 0.f;
  return train_step_checked("sr3_train_step_ex", plan, t, TRAIN_EX);
}
#undef SR3_TRAIN_STEP_COMMON
#undef SR3_TRAIN_STEP_OBJECTIVE

}  // extern "C"
