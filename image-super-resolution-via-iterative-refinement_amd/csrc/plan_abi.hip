// UNet plan, the C ABI: error plumbing, the sr3_plan_* entries and the forward / reverse-step entries (include/sr3_mi355x.h).
// plan_build.hip compiles the launch list, plan_run.hip replays it.
#include <stdarg.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>

#include <new>
#include <vector>

#include "plan_internal.h"
#include "tile_code.h"

namespace sr3 {

// ---- error plumbing ----------------------------------------------------------------------------
static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
int hip_fail(hipError_t e, const char* what) {
  set_error("HIP error %d (%s) at %s", (int)e, hipGetErrorString(e), what);
  (void)hipGetLastError();
  return (int)e > 0 ? (int)e : 1;
}
const char* last_error() { return g_err; }

}  // namespace sr3

// ---- the checks of PLAN_OPTIONS' rows (plan_internal.h) ----------------------------------------
int check_store_wt(const sr3_plan*, const char*, int value) {
  if (value < 0 || value > STORE_WT_ALL) { set_error("store_wt %d: a mask of bits 0-2 (0 .. %d)", value, (int)STORE_WT_ALL); return SR3_E_BADARG; }
  return SR3_OK;
}
int check_gemm_epi(const sr3_plan*, const char*, int value) {
  if (value < 0 || value > 2) { set_error("gemm_epi %d: 0 (4-byte epilogue), 1 (16-byte stores) or 2 (16-byte stores written through L2)", value); return SR3_E_BADARG; }
  return SR3_OK;
}
int check_var_channels(const sr3_plan* plan, const char*, int value) {
  if (value != 0 && value * 2 != plan->out_ch) {
    set_error("var_channels %d: 0 or half of out_channel %d (the variance head of a learned-variance model)", value, plan->out_ch);
    return SR3_E_BADARG;
  }
  return SR3_OK;
}
int check_attn_heads(const sr3_plan* plan, const char* key, int value) {
  const bool dim = !strcmp(key, "attn_head_dim");
  if (dim ? value < 0 : value < 1) { set_error("%s %d: needs a value >= %d", key, value, dim ? 0 : 1); return SR3_E_BADARG; }
  if (dim ? (value > 0 && plan->opt.attn_heads != 1) : (value != 1 && plan->opt.attn_head_dim != 0)) {
    set_error("%s %d: attn_heads (%d) and attn_head_dim (%d) are mutually exclusive", key, value, plan->opt.attn_heads, plan->opt.attn_head_dim);
    return SR3_E_BADARG;
  }
  // every attention level must take it: the channels divide, and a head's width is a multiple of 4
  for (const std::vector<Layer>* grp : {&plan->downs, &plan->mid, &plan->ups})
    for (const Layer& L : *grp) {
      if (L.kind != L_RES || !L.res.attn || (dim && value == 0)) continue;
      const int C = L.res.cout;
      const int d = dim ? value : (C % value ? 0 : C / value);
      if (d == 0 || C % d || (d & 3)) {
        if (dim) set_error("attn_head_dim %d: the attention of %s has %d channels (needs a multiple of 4 that divides them)", value, L.res.name.c_str(), C);
        else set_error("attn_heads %d: the attention of %s has %d channels (needs a divisor with a head width that is a multiple of 4)", value, L.res.name.c_str(), C);
        return SR3_E_BADARG;
      }
    }
  return SR3_OK;
}
// feat_cache = d: the shallow forward is the first d entries of downs and the last d res blocks of ups, which must all sit on the top
// resolution level -- the shallow part never crosses a Downsample or an Upsample
static int check_feat_cache(const sr3_plan* plan, int value) {
  if (value != 0 && (value < 1 || value > plan->d.res_blocks + 1)) {
    set_error("feat_cache %d: the depth of the shallow forward is 1 .. %d (res_blocks + 1: it stays on the top resolution level), or 0 for off",
              value, plan->d.res_blocks + 1);
    return SR3_E_UNSUPPORTED;
  }
  return SR3_OK;
}

// ---- C ABI -------------------------------------------------------------------------------------
extern "C" {

int sr3_version(void) { return SR3_ABI_VERSION; }
const char* sr3_last_error(void) { return sr3::last_error(); }
int sr3_selftest_split3(int* scratch_dev, int* mismatches, void* stream) {
  if (!scratch_dev || !mismatches) { sr3::set_error("null argument"); return SR3_E_BADARG; }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int rc = sr3::split3_selftest(scratch_dev, st);
  if (rc) return rc;
  SR3_HIP(hipMemcpyAsync(mismatches, scratch_dev, sizeof(int), hipMemcpyDeviceToHost, st));
  SR3_HIP(hipStreamSynchronize(st));
  if (*mismatches != 0) { sr3::set_error("split3 self-test: %d of 2097152 elements do not satisfy x == h + m + l exactly (compiler / ISA change?)", *mismatches); return SR3_E_UNSUPPORTED; }
  return SR3_OK;
}

int sr3_plan_create(const sr3_unet_desc* desc, sr3_plan** out) { return sr3_plan_create_ex(desc, 0u, out); }
int sr3_plan_create_ex(const sr3_unet_desc* desc, unsigned flags, sr3_plan** out) {
  if (!desc || !out) { set_error("null argument"); return SR3_E_BADARG; }
  if (flags & ~SR3_UNET_FLAGS_ALL) { set_error("sr3_plan_create_ex: unknown flag bits 0x%x", flags & ~SR3_UNET_FLAGS_ALL); *out = nullptr; return SR3_E_BADARG; }
  sr3_plan* P = new (std::nothrow) sr3_plan();
  if (!P) { set_error("out of host memory"); return SR3_E_NOMEM; }
#ifdef SR3_EXPERIMENTS
  // A/B builds only: defaults of plan options from the environment (a release library's arithmetic does not depend on the environment)
  { const char* e = getenv("SR3_WGRAD_SPLIT"); if (e) P->opt.wgrad_split = atoi(e); }
  { const char* e = getenv("SR3_WINO2"); if (e) P->opt.wino2 = atoi(e); }
#endif
  P->d = *desc;
  P->scale_shift = (flags & SR3_UNET_SCALE_SHIFT_NORM) != 0;
  const int rc = build_structure(P);
  if (rc) { delete P; *out = nullptr; return rc; }
  *out = P;
  return SR3_OK;
}
void sr3_plan_destroy(sr3_plan* plan) { delete plan; }
int sr3_plan_num_params(const sr3_plan* plan) { return plan ? (int)plan->params.size() : 0; }
int sr3_plan_param_info(const sr3_plan* plan, int index, sr3_param_info* out) {
  if (!plan || !out || index < 0 || index >= (int)plan->params.size()) { set_error("bad param index"); return SR3_E_BADARG; }
  *out = plan->params[index];
  return SR3_OK;
}
size_t sr3_plan_param_floats(const sr3_plan* plan) { return plan ? plan->param_floats : 0; }
// the launch list the inspection entries look at: that of the cond_channels the plan last ran with (none yet: unconditional)
static int build_inspected(sr3_plan* plan, int batch) { return build_forward(plan, batch, plan->built_cond >= 0 ? plan->built_cond : 0); }
int sr3_plan_num_ops(sr3_plan* plan, int batch) {
  if (!plan) return 0;
  return build_inspected(plan, batch) ? -1 : (int)plan->ops.size();
}
// the shallow list of plan option feat_cache (the _cached inspection twins): refused on a plan without the option
static int build_inspected_shallow(sr3_plan* plan, int batch) {
  if (!plan->opt.feat_cache) { set_error("the plan has no shallow forward: plan option feat_cache is off"); return SR3_E_BADARG; }
  return build_inspected(plan, batch);
}
static int op_info(const std::vector<Op>& ops, int batch, int index, sr3_op_info* out);
int sr3_plan_op_info(sr3_plan* plan, int batch, int index, sr3_op_info* out) {
  if (!plan || !out) { set_error("null argument"); return SR3_E_BADARG; }
  if (const int rc = build_inspected(plan, batch)) return rc;
  return op_info(plan->ops, batch, index, out);
}
int sr3_plan_num_ops_cached(sr3_plan* plan, int batch) {
  if (!plan) return 0;
  return build_inspected_shallow(plan, batch) ? -1 : (int)plan->sops.size();
}
int sr3_plan_op_info_cached(sr3_plan* plan, int batch, int index, sr3_op_info* out) {
  if (!plan || !out) { set_error("null argument"); return SR3_E_BADARG; }
  if (const int rc = build_inspected_shallow(plan, batch)) return rc;
  return op_info(plan->sops, batch, index, out);
}
size_t sr3_feature_cache_bytes(sr3_plan* plan, int batch) {
  if (!plan || !plan->opt.feat_cache) return 0;
  return build_inspected(plan, batch) ? 0 : plan->cache_bytes;
}
static int op_info(const std::vector<Op>& ops, int batch, int index, sr3_op_info* out) {
  if (index < 0 || index >= (int)ops.size()) { set_error("op index out of range"); return SR3_E_BADARG; }
  const Op& o = ops[index];
  memset(out, 0, sizeof(*out));
  out->kind = (int)o.kind * 10;
  if (o.kind == OP_CONV) {
    const ConvParams& c = o.conv.cp;
    const ConvChoice& ch = o.conv.ch;
    out->tile_cfg = tile_encode(ch.tile_cfg, c.wino_split, c.igemm_split, ch.has_wsplit, c.wino_full);
    out->ksplit = ch.ksplit;
    out->ksize = c.ksize; out->stride = c.stride; out->upsample = c.ups;
    out->cin = c.C0 + c.C1; out->cout = c.Cout; out->h_out = c.Ho; out->w_out = c.Wo;
    out->fused_res_conv_cin = c.x2_C0 + c.x2_C1;             // (0 without the fused segment)
    out->fused_output_stats = o.conv.ostat != NO_OFF ? 1 : 0;
    out->flops = conv_flops(c);
  } else if (o.kind == OP_CONV_IN) {
    const Op::ConvIn& v = o.conv_in;
    out->ksize = 3; out->stride = 1; out->cin = v.x_channels + v.cond_channels; out->cout = v.Cout; out->h_out = v.H; out->w_out = v.W;
    out->fused_output_stats = v.ostat != NO_OFF ? 1 : 0;
  } else if (o.kind == OP_ATTN) {
    out->h_out = o.attn.tokens; out->cin = out->cout = o.attn.channels;
    out->tile_cfg = o.attn.tile_cfg;                         // 24: the key-blocked kernel (plan option attn_long); 0: the strip kernels
    out->flops = attn_flops(batch, o.attn.tokens, o.attn.channels);
  }
  return SR3_OK;
}
int sr3_plan_op_side(sr3_plan* plan, int batch, int index, int* side_id, int* wait_id) {
  if (!plan) { set_error("null argument"); return SR3_E_BADARG; }
  if (const int rc = build_inspected(plan, batch)) return rc;
  if (index < 0 || index >= (int)plan->ops.size()) { set_error("op index out of range"); return SR3_E_BADARG; }
  if (side_id) *side_id = plan->ops[index].side_id;
  if (wait_id) *wait_id = plan->ops[index].wait_id;
  return SR3_OK;
}
int sr3_plan_op_fold(sr3_plan* plan, int batch, int index, int* fold, int* mod_row) {
  if (!plan) { set_error("null argument"); return SR3_E_BADARG; }
  if (const int rc = build_inspected(plan, batch)) return rc;
  if (index < 0 || index >= (int)plan->ops.size()) { set_error("op index out of range"); return SR3_E_BADARG; }
  const Op& o = plan->ops[index];
  const bool own = o.kind == OP_FOLD;
  if (fold) *fold = own ? 1 : (!o.fold_fused ? 0 : (o.kind == OP_CONV ? 2 : 3));
  if (mod_row) *mod_row = own ? o.fold.mod_row : (o.fold_fused ? o.tail.mod_row : -1);
  return SR3_OK;
}
double sr3_plan_forward_flops(sr3_plan* plan, int batch) {
  if (!plan) return 0;
  return build_inspected(plan, batch) ? -1 : plan->flops;
}
int sr3_store_wt_fits(size_t bytes) { return store_wt_fits(bytes) ? 1 : 0; }
// look up, validate, store, apply the row's effects, return the previous value (PLAN_OPTIONS, plan_internal.h)
int sr3_plan_set_option(sr3_plan* plan, const char* key, int value) {
  if (!plan || !key) return SR3_E_BADARG;
  const OptionRow* row = nullptr;
  for (const OptionRow& r : PLAN_OPTIONS)
    if (!strcmp(key, r.name)) { row = &r; break; }
  if (!row) { set_error("unknown option %s", key); return SR3_E_BADARG; }
  if (row->check)
    if (const int rc = row->check(plan, key, value)) return rc;
#ifndef SR3_EXPERIMENTS
  if ((row->effects & OPT_EXPERIMENT) && value != 0) {
    set_error("option %s selects an experiment kernel that this library was built without (csrc/build.sh -DSR3_EXPERIMENTS)", key);
    return SR3_E_UNSUPPORTED;
  }
#endif
  int& slot = plan->opt.*(row->slot);
  const int prev = slot;
  slot = value;
  if (row->slot == &PlanOptions::gemm_epi) plan->opt.gemm_epi_named = true;
  if (row->effects & OPT_FORWARD) { plan->built_batch = -1; plan->cache_filled = nullptr; }      // (a feature cache is one launch list's)
  if (row->effects & OPT_TRAIN) plan->train_batch = -1;
  if (row->effects & OPT_STALE) plan->derived_from = nullptr;
  if ((row->effects & OPT_RELAY) && prev != value) layout_derived(plan);     // (the buffer has to be re-bound and re-prepared)
  return prev;
}
// plan option feat_cache through its own entry: validate, store, drop the compiled forward (and with it what a cache was filled for)
int sr3_plan_set_feature_cache(sr3_plan* plan, int depth) {
  if (!plan) { set_error("null plan"); return SR3_E_BADARG; }
  if (const int rc = check_feat_cache(plan, depth)) return rc;
  const int prev = plan->opt.feat_cache;
  plan->opt.feat_cache = depth;
  plan->built_batch = -1;
  plan->cache_filled = nullptr;
  return prev;
}
int sr3_plan_num_taps(sr3_plan* plan) { return plan ? (int)plan->taps.size() : 0; }
int sr3_plan_tap_info(sr3_plan* plan, int index, char* name, int name_len, size_t* offset, int* C, int* H, int* W) {
  if (!plan || index < 0 || index >= (int)plan->taps.size()) { set_error("bad tap index"); return SR3_E_BADARG; }
  const Tap& t = plan->taps[index];
  if (name && name_len > 0) snprintf(name, name_len, "%s", t.name.c_str());
  if (offset) *offset = t.off;
  if (C) *C = t.C;
  if (H) *H = t.H;
  if (W) *W = t.W;
  return SR3_OK;
}

size_t sr3_plan_derived_bytes(const sr3_plan* plan) { return plan ? plan->derived_floats * sizeof(float) : 0; }
int sr3_plan_bind_derived(sr3_plan* plan, void* buffer, size_t bytes) {
  if (!plan) { set_error("null plan"); return SR3_E_BADARG; }
  if (buffer && bytes < plan->derived_floats * sizeof(float)) {
    set_error("derived buffer too small (%zu < %zu)", bytes, plan->derived_floats * sizeof(float));
    return SR3_E_NOMEM;
  }
  if ((uintptr_t)buffer & 15) { set_error("derived buffer is not 16-byte aligned"); return SR3_E_ALIGN; }
  plan->derived_ptr = static_cast<float*>(buffer);
  plan->derived_bound_bytes = buffer ? bytes : 0;
  plan->derived_from = nullptr;               // a freshly bound buffer holds nothing yet
  return SR3_OK;
}
int sr3_plan_invalidate_derived(sr3_plan* plan) {
  if (!plan) { set_error("null plan"); return SR3_E_BADARG; }
  plan->derived_from = nullptr;
  return SR3_OK;
}
int sr3_plan_prepare_derived(sr3_plan* plan, const float* params, void* stream) {
  if (!plan || !params) { set_error("null argument"); return SR3_E_BADARG; }
  if (!plan->derived_ptr) { set_error("no derived buffer bound"); return SR3_E_BADARG; }
  for (const auto& d : plan->derived) {
    int rc = wino_transform_weights(params + d.w, d.Cout, d.Cin, plan->derived_ptr + d.off, static_cast<hipStream_t>(stream));
    if (rc) return rc;
    if (plan->opt.wino_split) {
      rc = wino_transform_weights(params + d.w, d.Cout, d.Cin, plan->derived_ptr + d.off + wino_weight_floats(d.Cout, d.Cin),
                                  static_cast<hipStream_t>(stream), true);
      if (rc) return rc;
    }
  }
  for (const auto& d : plan->wsplits) {
    const int rc = igemm_split_weights(params + d.w, d.Cout, d.taps, d.Cin, plan->derived_ptr + d.off, static_cast<hipStream_t>(stream));
    if (rc) return rc;
  }
  plan->derived_from = params;
  return SR3_OK;
}

int sr3_plan_set_geometry(sr3_plan* plan, int height, int width) {
  if (!plan) { set_error("null plan"); return SR3_E_BADARG; }
  const int div = 1 << (plan->d.n_mults - 1);
  if (height == 0 && width == 0) {
    height = width = plan->d.image_size;
  } else if (height <= 0 || width <= 0 || (height % div) || (width % div)) {
    set_error("geometry %d x %d: height and width must be positive multiples of %d (2^(n_mults-1): the UNet halves the image %d times)",
              height, width, div, plan->d.n_mults - 1);
    return SR3_E_BADARG;
  }
  const bool native = height == plan->d.image_size && width == plan->d.image_size;
  const int h = native ? 0 : height, w = native ? 0 : width;
  if (h == plan->geo_h && w == plan->geo_w) return SR3_OK;
  plan->geo_h = h; plan->geo_w = w;
  plan->built_batch = -1;            // the launch list is rebuilt; the derived filters do not depend on the geometry
  return SR3_OK;
}
int sr3_plan_get_geometry(const sr3_plan* plan, int* height, int* width) {
  if (!plan) { set_error("null plan"); return SR3_E_BADARG; }
  if (height) *height = plan_height(plan);
  if (width) *width = plan_width(plan);
  return SR3_OK;
}

size_t sr3_workspace_bytes(sr3_plan* plan, int batch) {
  if (!plan) return 0;
  return build_inspected(plan, batch) ? 0 : plan->ws_bytes;
}

// What the inference entries check before a forward, in this order: the entry's own required pointers (`given`) and the call's, the
// launch list (build_forward), the workspace size, alignment, what the variant needs.  FC_STEP: a reverse step -- eps_out is optional,
// z is aligned too, the level comes from level_table.  FC_PROFILE: sr3_unet_forward_profile checks its own pointers, the list and the
// size (without the two numbers) alone
enum { FC_STEP = 1, FC_PROFILE = 2 };
static int check_forward_call(sr3_plan* plan, ForwardCall& f, unsigned what, bool given = true, const float* z = nullptr) {
  const bool step = what & FC_STEP, profile = what & FC_PROFILE;
  if (!plan || !given || (!profile && (!f.x || !f.params || !f.workspace || !f.freq || (!step && !f.eps_out)))) { set_error("null argument"); return SR3_E_BADARG; }
  if (!f.cond) f.cond_channels = 0;
  if (const int rc = build_forward(plan, f.batch, f.cond_channels)) return rc;
  if (f.workspace_bytes < plan->ws_bytes) {
    if (profile) set_error("workspace too small");
    else set_error("workspace too small: %zu < %zu", f.workspace_bytes, plan->ws_bytes);
    return SR3_E_NOMEM;
  }
  if (profile) return SR3_OK;
  if (((uintptr_t)f.workspace & 255) || ((uintptr_t)f.params & 15) || ((uintptr_t)f.x & 15) || ((uintptr_t)f.eps_out & 15) || ((uintptr_t)z & 15)) {
    set_error("misaligned pointer (workspace 256 B, tensors 16 B)");
    return SR3_E_ALIGN;
  }
  const bool sr3_variant = plan->d.variant == SR3_VARIANT_SR3;
  if (step) {
    if (sr3_variant && !f.level_table) { set_error("SR3 variant needs level_table"); return SR3_E_BADARG; }
    return SR3_OK;
  }
  if (sr3_variant && !f.level && !f.step_dev) { set_error("SR3 variant needs noise_level or step_dev"); return SR3_E_BADARG; }
  if (plan->d.variant == SR3_VARIANT_DDPM && !f.tstep && !f.step_dev) { set_error("DDPM variant needs timestep or step_dev"); return SR3_E_BADARG; }
  return SR3_OK;
}

int sr3_unet_forward(sr3_plan* plan, const float* x_nchw, const float* cond_nchw, int cond_channels,
                     const float* noise_level, const int64_t* timestep, const float* freq, const float* level_table,
                     const int* step_dev, const float* params, void* workspace, size_t workspace_bytes,
                     float* eps_out_nchw, int batch, void* stream) {
  ForwardCall f = {.x = x_nchw, .cond = cond_nchw, .cond_channels = cond_channels, .level = noise_level, .tstep = timestep, .freq = freq,
                   .level_table = level_table, .step_dev = step_dev, .params = params, .workspace = workspace,
                   .workspace_bytes = workspace_bytes, .eps_out = eps_out_nchw, .batch = batch, .stream = static_cast<hipStream_t>(stream)};
  if (const int rc = check_forward_call(plan, f, 0)) return rc;
  return run_forward(plan, f);
}
// ... with the variance head: eps_out_nchw is [B, out_channel, H, W] (plan option var_channels; without it the same call as above)
int sr3_unet_forward_full(sr3_plan* plan, const float* x_nchw, const float* cond_nchw, int cond_channels,
                          const float* noise_level, const int64_t* timestep, const float* freq, const float* level_table,
                          const int* step_dev, const float* params, void* workspace, size_t workspace_bytes,
                          float* eps_out_nchw, int batch, void* stream, const int* t_map) {
  if (t_map && !step_dev) { set_error("sr3_unet_forward_full: t_map goes with step_dev"); return SR3_E_BADARG; }
  ForwardCall f = {.x = x_nchw, .cond = cond_nchw, .cond_channels = cond_channels, .level = noise_level, .tstep = timestep, .freq = freq,
                   .level_table = level_table, .step_dev = step_dev, .t_map = t_map, .params = params, .workspace = workspace,
                   .workspace_bytes = workspace_bytes, .eps_out = eps_out_nchw, .batch = batch, .stream = static_cast<hipStream_t>(stream),
                   .full_out = true};
  if (const int rc = check_forward_call(plan, f, 0)) return rc;
  return run_forward(plan, f);
}

// What the _cached entries check behind check_forward_call, in this order, before anything is launched: the cache pointer, its size and
// alignment; refresh = 0: the option, then that the last refresh filled THIS cache at this batch and geometry.  What a refresh filled
// is recorded behind its forward (run_cached)
static int check_feature_cache(sr3_plan* plan, ForwardCall& f, void* cache, size_t cache_bytes, int refresh) {
  if (!refresh && !plan->opt.feat_cache) {
    set_error("a cached forward (refresh = 0) needs a plan built with option feat_cache");
    return SR3_E_BADARG;
  }
  if (!plan->opt.feat_cache) return SR3_OK;      // (refresh = 1 on a plan without the option: the plain forward, the cache is not looked at)
  if (!cache) { set_error("null feature cache"); return SR3_E_BADARG; }
  if (cache_bytes < plan->cache_bytes) { set_error("feature cache too small: %zu < %zu", cache_bytes, plan->cache_bytes); return SR3_E_NOMEM; }
  if ((uintptr_t)cache & 255) { set_error("misaligned feature cache (256 B)"); return SR3_E_ALIGN; }
  const int h = plan_height(plan), w = plan_width(plan);
  if (!refresh && (plan->cache_filled != cache || plan->cache_batch != f.batch || plan->cache_h != h || plan->cache_w != w)) {
    if (!plan->cache_filled) set_error("the feature cache was never filled: run a refresh (refresh = 1) first");
    else set_error("the feature cache was filled at batch %d, geometry %d x %d%s: a cached forward at batch %d, geometry %d x %d needs a refresh first",
                   plan->cache_batch, plan->cache_h, plan->cache_w, plan->cache_filled != cache ? " in another buffer" : "", f.batch, h, w);
    return SR3_E_BADARG;
  }
  f.cache = cache; f.shallow = !refresh;
  return SR3_OK;
}
// the forward of a _cached entry.  A refresh that went through records what it filled; one that was refused behind the checks above (a
// missing or stale derived buffer) or whose launch failed leaves no fill on record: nothing trustworthy is in the cache then
static int run_cached(sr3_plan* plan, const ForwardCall& f) {
  const int rc = run_forward(plan, f);
  if (f.cache && !f.shallow) {
    plan->cache_filled = rc == SR3_OK ? f.cache : nullptr;
    plan->cache_batch = f.batch; plan->cache_h = plan_height(plan); plan->cache_w = plan_width(plan);
  }
  return rc;
}

// sr3_unet_forward_full on a plan under option feat_cache: refresh = 1 the full list, which leaves the branch tensor in feat_cache;
// refresh = 0 the shallow list, which reads it
int sr3_unet_forward_cached(sr3_plan* plan, const float* x_nchw, const float* cond_nchw, int cond_channels,
                            const float* noise_level, const int64_t* timestep, const float* freq, const float* level_table,
                            const int* step_dev, const float* params, void* workspace, size_t workspace_bytes,
                            float* eps_out_nchw, int batch, void* stream, const int* t_map, void* feat_cache, size_t feat_cache_bytes,
                            int refresh) {
  if (t_map && !step_dev) { set_error("sr3_unet_forward_cached: t_map goes with step_dev"); return SR3_E_BADARG; }
  ForwardCall f = {.x = x_nchw, .cond = cond_nchw, .cond_channels = cond_channels, .level = noise_level, .tstep = timestep, .freq = freq,
                   .level_table = level_table, .step_dev = step_dev, .t_map = t_map, .params = params, .workspace = workspace,
                   .workspace_bytes = workspace_bytes, .eps_out = eps_out_nchw, .batch = batch, .stream = static_cast<hipStream_t>(stream),
                   .full_out = true};
  if (const int rc = check_forward_call(plan, f, 0)) return rc;
  if (const int rc = check_feature_cache(plan, f, feat_cache, feat_cache_bytes, refresh)) return rc;
  return run_cached(plan, f);
}

// One whole reverse step (include/sr3_mi355x.h): the forward above with the p_sample update and the counter decrement inside the
// output conv's kernel -- two graph nodes fewer per step than sr3_unet_forward + sr3_p_sample_step + sr3_step_decrement.
// _hist: the multistep tail (tab_c3 and the history buffer, both or neither); _ex forwards here with neither.
// _cached: the same step on a plan under option feat_cache -- refresh = 1 the full forward (writes the cache), 0 the shallow one (reads
// it); have_cache = false: the plain entries, which a plan under the option refuses (run_forward)
static int reverse_step(sr3_plan* plan, float* x_nchw, const float* cond_nchw, int cond_channels, const float* freq,
                        const float* level_table, int* step2_dev, const float* params, void* workspace, size_t workspace_bytes,
                        const float* z_nchw, const float* ta, const float* tb, const float* tc1, const float* tc2, const float* tsig,
                        int clip_denoised, float* eps_out_nchw, int batch, void* stream, const int* t_map, const float* tc3,
                        float* hist_nchw, bool have_cache, void* feat_cache, size_t feat_cache_bytes, int refresh) {
  // the embedding kernel reads t from slot 1 and copies it to slot 0; the tail reads slot 0 and writes t - 1 to slot 1: no kernel
  // both reads and writes a slot, so no launch of the step races with another block of itself
  ForwardCall f = {.x = x_nchw, .cond = cond_nchw, .cond_channels = cond_channels, .freq = freq, .level_table = level_table,
                   .step_dev = step2_dev ? step2_dev + 1 : nullptr, .t_map = t_map, .params = params, .workspace = workspace,
                   .workspace_bytes = workspace_bytes, .eps_out = eps_out_nchw, .batch = batch, .stream = static_cast<hipStream_t>(stream)};
  if (const int rc = check_forward_call(plan, f, FC_STEP, step2_dev && ta && tb && tc1 && tc2 && tsig, z_nchw)) return rc;
  const size_t image_bytes = (size_t)batch * (plan->d.out_channel - plan->opt.var_channels) * plan_height(plan) * plan_width(plan) * sizeof(float);
  if (const int rc = check_step_history("reverse_step", tc3, hist_nchw, x_nchw, eps_out_nchw, image_bytes, true)) return rc;
  if (have_cache)
    if (const int rc = check_feature_cache(plan, f, feat_cache, feat_cache_bytes, refresh)) return rc;
  StepFuse tail;
  tail.x = x_nchw; tail.z = z_nchw; tail.tb = StepTables{ta, tb, tc1, tc2, tsig};
  tail.step_cur = step2_dev; tail.step_next = step2_dev + 1; tail.clip = clip_denoised; tail.c3 = tc3; tail.hist = hist_nchw;
  f.fuse = &tail;
  return run_cached(plan, f);
}
int sr3_reverse_step_hist(sr3_plan* plan, float* x_nchw, const float* cond_nchw, int cond_channels, const float* freq,
                          const float* level_table, int* step2_dev, const float* params, void* workspace, size_t workspace_bytes,
                          const float* z_nchw, const float* ta, const float* tb, const float* tc1, const float* tc2, const float* tsig,
                          int clip_denoised, float* eps_out_nchw, int batch, void* stream, const int* t_map, const float* tc3,
                          float* hist_nchw) {
  return reverse_step(plan, x_nchw, cond_nchw, cond_channels, freq, level_table, step2_dev, params, workspace, workspace_bytes, z_nchw, ta, tb,
                      tc1, tc2, tsig, clip_denoised, eps_out_nchw, batch, stream, t_map, tc3, hist_nchw, false, nullptr, 0, 1);
}
int sr3_reverse_step_cached(sr3_plan* plan, float* x_nchw, const float* cond_nchw, int cond_channels, const float* freq,
                            const float* level_table, int* step2_dev, const float* params, void* workspace, size_t workspace_bytes,
                            const float* z_nchw, const float* ta, const float* tb, const float* tc1, const float* tc2, const float* tsig,
                            int clip_denoised, float* eps_out_nchw, int batch, void* stream, const int* t_map, const float* tc3,
                            float* hist_nchw, void* feat_cache, size_t feat_cache_bytes, int refresh) {
  return reverse_step(plan, x_nchw, cond_nchw, cond_channels, freq, level_table, step2_dev, params, workspace, workspace_bytes, z_nchw, ta, tb,
                      tc1, tc2, tsig, clip_denoised, eps_out_nchw, batch, stream, t_map, tc3, hist_nchw, true, feat_cache, feat_cache_bytes,
                      refresh);
}

int sr3_reverse_step_ex(sr3_plan* plan, float* x_nchw, const float* cond_nchw, int cond_channels, const float* freq,
                        const float* level_table, int* step2_dev, const float* params, void* workspace, size_t workspace_bytes,
                        const float* z_nchw, const float* ta, const float* tb, const float* tc1, const float* tc2, const float* tsig,
                        int clip_denoised, float* eps_out_nchw, int batch, void* stream, const int* t_map) {
  return sr3_reverse_step_hist(plan, x_nchw, cond_nchw, cond_channels, freq, level_table, step2_dev, params, workspace, workspace_bytes,
                               z_nchw, ta, tb, tc1, tc2, tsig, clip_denoised, eps_out_nchw, batch, stream, t_map, nullptr, nullptr);
}

int sr3_reverse_step(sr3_plan* plan, float* x_nchw, const float* cond_nchw, int cond_channels, const float* freq,
                     const float* level_table, int* step2_dev, const float* params, void* workspace, size_t workspace_bytes,
                     const float* z_nchw, const float* ta, const float* tb, const float* tc1, const float* tc2, const float* tsig,
                     int clip_denoised, float* eps_out_nchw, int batch, void* stream) {
  return sr3_reverse_step_ex(plan, x_nchw, cond_nchw, cond_channels, freq, level_table, step2_dev, params, workspace, workspace_bytes,
                             z_nchw, ta, tb, tc1, tc2, tsig, clip_denoised, eps_out_nchw, batch, stream, nullptr);
}

int sr3_unet_forward_profile(sr3_plan* plan, const float* x_nchw, const float* cond_nchw, int cond_channels,
                             const float* noise_level, const int64_t* timestep, const float* freq, const float* params,
                             void* workspace, size_t workspace_bytes, float* eps_out_nchw, int batch, void* stream,
                             int max_ops, float* op_ms, int* op_kind, double* op_flops, int* n_ops) {
  ForwardCall f = {.x = x_nchw, .cond = cond_nchw, .cond_channels = cond_channels, .level = noise_level, .tstep = timestep, .freq = freq,
                   .params = params, .workspace = workspace, .workspace_bytes = workspace_bytes, .eps_out = eps_out_nchw, .batch = batch,
                   .stream = static_cast<hipStream_t>(stream)};
  if (const int rc = check_forward_call(plan, f, FC_PROFILE, op_ms && op_kind && op_flops && n_ops)) return rc;
  return profile_forward(plan, f, max_ops, op_ms, op_kind, op_flops, n_ops);
}

}  // extern "C"
