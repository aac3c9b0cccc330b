// UNet plan, the forward driver: binds the launch list plan_build.hip compiled to one call's pointers and replays it.
#include <string.h>

#include <vector>

#include "plan_internal.h"
#include "tile_code.h"

namespace sr3 {

// ---- binding -----------------------------------------------------------------------------------
// pointer into the arena for an optional offset (NO_OFF: null)
static const float* bind(const float* params, size_t off) { return off == NO_OFF ? nullptr : params + off; }

// What one call binds every op of its list to: the per-call pointers, and the stream / split-K mid event of the op being launched
struct Bound {
  sr3_plan* P;
  const ForwardCall& f;
  const Regions& R;
  char* ws; char* stats; float* film;      // the workspace, its statistics region, its FiLM table
  const float* params;
  hipStream_t st = nullptr;                // the caller's stream, or the plan's side stream (fork_side)
  hipEvent_t mid = nullptr;                // per-op timing: recorded between a split-K conv's GEMM kernel and its reduce
  char* cache = nullptr;                   // plan option feat_cache: the caller's feature cache
};

// pointer for an optional activation / statistics offset (NO_OFF: null): into `base` -- the workspace, or its statistics region -- or,
// a CACHE_TAG offset, into the feature cache (the branch tensor and its partials: run_forward refused a list that has one without a cache)
template <typename T> static T* bind(const Bound& b, char* base, size_t off) {
  if (off == NO_OFF) return nullptr;
  return reinterpret_cast<T*>((off & CACHE_TAG) ? b.cache + (off & ~CACHE_TAG) : base + off);
}

static FoldTail make_fold_tail(const FoldSpec& s, const Bound& b) {
  FoldTail f;
  memset(&f, 0, sizeof(f));
  f.groups = b.P->d.norm_groups; f.Ctot = s.Ctot; f.c_off = s.c_off;
  f.ostat = bind<const double>(b, b.stats, s.ostat); f.oC = s.oC; f.oT = s.oT; f.o_off = s.o_off;
  f.gamma = b.params + s.gamma; f.beta = b.params + s.beta; f.eps = 1e-5f;
  f.ss = reinterpret_cast<float*>(b.ws + b.R.ss_off + s.ss_rel);
  f.mr = s.has_mr ? reinterpret_cast<float*>(b.ws + b.R.mr_off + s.mr_rel) : nullptr;
  if (s.mod_row >= 0) { f.mod = b.film + s.mod_row; f.mod_stride = b.P->film_rows(); }
  return f;
}

// ---- derived-buffer preflight ------------------------------------------------------------------
// which operands of the derived buffer a conv's kernel reads: the transformed (Winograd) filters, the pre-split GEMM weights
static bool reads_wino(const Op::Conv& v) { return v.ch.tile_cfg == 11; }
static bool reads_wsplit(const Op::Conv& v) {
  return v.ch.has_wsplit && ((v.ch.tile_cfg >= 1 && v.ch.tile_cfg <= 4) || v.ch.tile_cfg == 22) && v.cp.igemm_split;
}

// A list that reads derived weights the plan does not hold is refused HERE, in front of the first launch (under stream capture a
// refusal between launches would leave a half-built graph); the first offending op in list order says which text
static int check_derived(const sr3_plan* P, const std::vector<Op>& ops, const float* params) {
  for (const Op& o : ops) {
    if (o.kind != OP_CONV) continue;
    if (reads_wino(o.conv)) {
      if (!P->derived_ptr) { set_error("the plan's derived (Winograd) weights are not bound: call sr3_plan_bind_derived + sr3_plan_prepare_derived"); return SR3_E_BADARG; }
      // stale filters must fail loudly, not compute with the previous weights: the buffer has to have been prepared from
      // THIS arena, under the current options, and not invalidated since (sr3_plan_invalidate_derived after an optimizer step)
      if (P->derived_from != params) {
        set_error("the plan's derived (Winograd) weights are stale or were prepared from another arena: call sr3_plan_prepare_derived");
        return SR3_E_BADARG;
      }
    }
    if (reads_wsplit(o.conv) && (!P->derived_ptr || P->derived_from != params)) {
      set_error("the plan's derived (pre-split 1x1 / stride-2) weights are not bound or stale: call sr3_plan_bind_derived + sr3_plan_prepare_derived");
      return SR3_E_BADARG;
    }
  }
  return SR3_OK;
}

// ---- one launch per op kind --------------------------------------------------------------------
static int launch_embed(const Op&, const Bound& b) {
  const sr3_plan* P = b.P;
  const ForwardCall& f = b.f;
  EmbedParams e;
  memset(&e, 0, sizeof(e));
  e.variant = P->d.variant; e.B = f.batch; e.inner = P->d.inner_channel;
  e.level = f.level; e.tstep = f.tstep; e.level_table = f.level_table; e.step_dev = f.step_dev; e.t_map = f.t_map; e.freq = f.freq;
  e.step_out = f.fuse ? const_cast<int*>(f.fuse->step_cur) : nullptr;
  e.w1 = b.params + P->emb_w1; e.b1 = b.params + P->emb_b1; e.w2 = b.params + P->emb_w2; e.b2 = b.params + P->emb_b2;
  e.wf = b.params + P->film_w; e.bf = b.params + P->film_b; e.F = P->film_rows();
  e.temb = reinterpret_cast<float*>(b.ws + b.R.temb_off); e.film = b.film;
  return embed_forward(e, b.st);
}

static int launch_conv_in(const Op& o, const Bound& b) {
  // virtual concat order is [cond | x] (diffusion.py:157); unconditional: x only
  const Op::ConvIn& v = o.conv_in;
  const ForwardCall& f = b.f;
  const float* a0 = f.cond_channels > 0 ? f.cond : f.x;
  const int Ca = f.cond_channels > 0 ? f.cond_channels : v.x_channels;
  const float* a1 = f.cond_channels > 0 ? f.x : nullptr;
  const int Cb = f.cond_channels > 0 ? v.x_channels : 0;
  return conv_in_nchw(a0, Ca, a1, Cb, f.batch, v.H, v.W, b.params + v.w, b.params + v.bias, v.Cout, bind<float>(b, b.ws, v.out),
                      bind<double>(b, b.stats, v.ostat), b.st);
}

static int launch_stats(const Op& o, const Bound& b) {
  const Op::Stats& v = o.stats;
  if (o.fold_fused) {
    FoldTail ft = make_fold_tail(o.tail, b);
    return chan_stats_fold(bind<const float>(b, b.ws, v.src), b.f.batch, v.pixels, v.channels, bind<double>(b, b.stats, v.stat), ft, b.st);
  }
  return chan_stats(bind<const float>(b, b.ws, v.src), b.f.batch, v.pixels, v.channels, bind<double>(b, b.stats, v.stat), b.st);
}

static int launch_fold(const Op& o, const Bound& b) {
  const Op::Fold& v = o.fold;
  return gn_finalize(bind<const double>(b, b.stats, v.stat0), v.C0, v.T0, bind<const double>(b, b.stats, v.stat1), v.C1, v.T1, b.f.batch, v.pixels,
                     b.P->d.norm_groups, b.params + v.gamma, b.params + v.beta, 1e-5f, bind<float>(b, b.ws, b.R.ss_off + o.ss_rel), b.st,
                     v.has_mr ? bind<float>(b, b.ws, b.R.mr_off + o.mr_rel) : nullptr, v.mod_row >= 0 ? b.film + v.mod_row : nullptr, b.P->film_rows());
}

static int launch_conv(const Op& o, const Bound& b) {
  const Op::Conv& v = o.conv;
  const ConvChoice& ch = v.ch;
  const DropCfg* drop = b.f.drop;
  ConvParams c = v.cp;
  c.src0 = bind<const float>(b, b.ws, v.src0);
  c.src1 = bind<const float>(b, b.ws, v.src1);
  c.w = b.params + v.w;
  c.bias = bind(b.params, v.bias);
  c.ss = c.act ? bind<const float>(b, b.ws, b.R.ss_off + o.ss_rel) : nullptr;
  c.film = v.film_row >= 0 ? b.film + v.film_row : nullptr;
  c.res0 = bind<const float>(b, b.ws, v.res0);
  c.res1 = bind<const float>(b, b.ws, v.res1);
  c.out = bind<float>(b, b.ws, v.out);
  c.ostat = bind<double>(b, b.stats, v.ostat);
  c.store_wt = b.P->opt.store_wt;
  c.gemm_epi = 1 + b.P->opt.launch_gemm_epi();
  if (drop && v.has_drop && drop->thresh != 0) {
    c.drop_seed = drop_layer_seed(drop->seed, v.drop_key); c.drop_thresh = drop->thresh; c.drop_scale = drop->scale;
  }
  if (v.x2_src0 != NO_OFF) {
    c.x2_src0 = bind<const float>(b, b.ws, v.x2_src0);
    c.x2_src1 = bind<const float>(b, b.ws, v.x2_src1);
    c.x2_w = b.params + v.x2_w;
    c.x2_bias = b.params + v.x2_bias;
  }
  if (reads_wino(v)) c.wino_u = b.P->derived_ptr + ch.wino_off;            // (bound and prepared from this arena: check_derived)
  if (reads_wsplit(v)) c.w_split = b.P->derived_ptr + ch.wsplit_off;
  FoldTail ft;
  if (o.fold_fused) { ft = make_fold_tail(o.tail, b); c.fold = &ft; }
  return conv_forward(c, ch.tile_cfg, ch.ksplit, bind<float>(b, b.ws, b.R.scratch_off), b.R.scratch_bytes, b.st, b.mid);
}

static int launch_attn(const Op& o, const Bound& b) {
  const Op::Attn& v = o.attn;
  // (one head: attention_forward's launches; more: attention_heads.hip)
  return attention_forward_heads(bind<const float>(b, b.ws, v.qkv), b.f.batch, v.tokens, v.channels, v.heads, bind<float>(b, b.ws, v.out), b.st,
                                 (b.P->opt.attn_split ? 1 : 0) | (v.tile_cfg == 24 ? 2 : 0));
}

static int launch_conv_out(const Op& o, const Bound& b) {
  const Op::ConvOut& v = o.conv_out;
  // the prediction rows alone -- the first rows of the same filters and bias -- unless all rows are asked for
  const int rows = (b.f.train || b.f.full_out) ? v.out_ch : v.out_ch - b.P->opt.var_channels;
  return conv_out_nchw(bind<const float>(b, b.ws, v.src), bind<const float>(b, b.ws, b.R.ss_off + o.ss_rel), b.f.batch, v.H, v.W, v.channels,
                       b.params + v.w, b.params + v.bias, rows, b.f.eps_out, b.st, b.f.fuse);
}

// ---- fork / join (plan option fork_side) -------------------------------------------------------
// Ops marked side_id run on the plan's side stream between a fork event (recorded on the caller's stream where the op sits in the
// list) and a join event their consumer (wait_id) waits for.  fork_op: the consumer's wait, then the fork; *st is the stream the op
// runs on.  join_op: the side op's join event
static int fork_op(sr3_plan* P, const Op& o, hipStream_t main_st, hipStream_t* st) {
  *st = main_st;
  if (o.wait_id >= 0 && o.wait_id < (int)P->join_ev.size()) SR3_HIP(hipStreamWaitEvent(main_st, P->join_ev[o.wait_id], 0));
  if (o.side_id < 0) return SR3_OK;
  if (!P->side_stream) SR3_HIP(hipStreamCreateWithFlags(&P->side_stream, hipStreamNonBlocking));
  while ((int)P->fork_ev.size() <= o.side_id) {
    hipEvent_t a, b;
    SR3_HIP(hipEventCreateWithFlags(&a, hipEventDisableTiming));
    SR3_HIP(hipEventCreateWithFlags(&b, hipEventDisableTiming));
    P->fork_ev.push_back(a); P->join_ev.push_back(b);
  }
  SR3_HIP(hipEventRecord(P->fork_ev[o.side_id], main_st));
  SR3_HIP(hipStreamWaitEvent(P->side_stream, P->fork_ev[o.side_id], 0));
  *st = P->side_stream;
  return SR3_OK;
}
static int join_op(sr3_plan* P, const Op& o, hipStream_t st) {
  if (o.side_id >= 0) SR3_HIP(hipEventRecord(P->join_ev[o.side_id], st));
  return SR3_OK;
}

// ---- the launch loop ---------------------------------------------------------------------------
int run_forward(sr3_plan* P, const ForwardCall& f) {
  const std::vector<Op>& ops = f.train ? P->tops : f.shallow ? P->sops : P->ops;
  const Regions& R = f.train ? P->t_regions : f.shallow ? P->sregions : P->regions;
  if (const int rc = check_derived(P, ops, f.params)) return rc;
  if (!f.train && P->opt.feat_cache && !f.cache) {
    // the full list of such a plan writes the branch tensor into the cache: without one there is nowhere to put it
    set_error("plan option feat_cache is on: the forward needs a feature cache (sr3_unet_forward_cached / sr3_reverse_step_cached)");
    return SR3_E_BADARG;
  }
  char* const ws = static_cast<char*>(f.workspace);
  Bound b = {P, f, R, ws, ws + R.stats_off, reinterpret_cast<float*>(ws + R.film_off), f.params};
  b.cache = static_cast<char*>(f.cache);
  const bool forking = !f.ev && !f.train;      // under per-op timing everything stays on one stream
  size_t i = 0;
  for (const Op& o : ops) {
    if (f.ev) SR3_HIP(hipEventRecord(f.ev[i], f.stream));
    b.st = f.stream;
    b.mid = f.mid ? f.mid[i] : nullptr;
    ++i;
    int rc = forking ? fork_op(P, o, f.stream, &b.st) : SR3_OK;
    if (rc) return rc;
    switch (o.kind) {
      case OP_RESERVED: break;
      case OP_EMBED: rc = launch_embed(o, b); break;
      case OP_CONV_IN: rc = launch_conv_in(o, b); break;
      case OP_STATS: rc = launch_stats(o, b); break;
      case OP_FOLD: rc = launch_fold(o, b); break;
      case OP_CONV: rc = launch_conv(o, b); break;
      case OP_ATTN: rc = launch_attn(o, b); break;
      case OP_CONV_OUT: rc = launch_conv_out(o, b); break;
    }
    if (!rc && forking) rc = join_op(P, o, b.st);
    if (rc) return rc;
  }
  if (f.ev) SR3_HIP(hipEventRecord(f.ev[i], f.stream));
  return SR3_OK;
}

// ---- per-op timing (sr3_unet_forward_profile) --------------------------------------------------
// one forward with a HIP event around every op (and between a split-K conv's two kernels), then the table: one row per op, one more
// (kind 59) per split-K reduce
int profile_forward(sr3_plan* plan, ForwardCall f, int max_ops, float* op_ms, int* op_kind, double* op_flops, int* n_ops) {
  int rc = SR3_OK;
  const int n = (int)plan->ops.size();
  std::vector<hipEvent_t> ev(n + 1, nullptr), mid(n, nullptr);
  for (auto* v : {&ev, &mid})
    for (auto& e : *v)
      if (hipError_t err = hipEventCreate(&e); err != hipSuccess && !rc) rc = hip_fail(err, "hipEventCreate");
  f.ev = ev.data(); f.mid = mid.data();
  if (!rc) rc = run_forward(plan, f);
  if (!rc) {
    hipError_t e = hipEventSynchronize(ev[n]);
    if (e != hipSuccess) rc = hip_fail(e, "hipEventSynchronize");
  }
  if (!rc) {
    int w = 0;
    for (int i = 0; i < n && !rc; ++i) {
      float ms = 0.f;
      if (hipError_t e = hipEventElapsedTime(&ms, ev[i], ev[i + 1]); e != hipSuccess) { rc = hip_fail(e, "hipEventElapsedTime"); break; }
      const Op& o = plan->ops[i];
      int kind = (int)o.kind * 10;
      double fl = 0.0;
      float red_ms = -1.f;
      if (o.kind == OP_CONV) {
        const ConvParams& c = o.conv.cp;
        const int tile = o.conv.ch.tile_cfg;
        WinoGeom wg;
        kind = profile_kind(tile, c.wino_split, c.igemm_split, tile == 11 && wino_geometry(c, &wg) && wg.NB != 1, o.conv.x2_src0 != NO_OFF);      // (tile_code.h)
        fl = conv_flops(c);
        if (o.conv.ch.ksplit > 1) {      // split the op into its GEMM kernel and its split-K reduce kernel
          float a = 0.f;
          if (hipError_t e = hipEventElapsedTime(&a, ev[i], mid[i]); e != hipSuccess) { rc = hip_fail(e, "hipEventElapsedTime"); break; }
          red_ms = ms - a;
          ms = a;
        }
      } else if (o.kind == OP_ATTN) {
        fl = attn_flops(f.batch, o.attn.tokens, o.attn.channels);
      }
      if (w + 2 > max_ops) { set_error("op buffer too small"); rc = SR3_E_NOMEM; break; }
      op_ms[w] = ms; op_kind[w] = kind; op_flops[w] = fl; ++w;
      if (red_ms >= 0.f) { op_ms[w] = red_ms; op_kind[w] = 59; op_flops[w] = 0.0; ++w; }
    }
    *n_ops = w;
  }
  for (auto& e : ev) if (e) (void)hipEventDestroy(e);
  for (auto& e : mid) if (e) (void)hipEventDestroy(e);
  return rc;
}

}  // namespace sr3
