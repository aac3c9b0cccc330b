// UNet plan: topology, parameter arena, activation plan and the forward driver.
//
// Mirrors UNet.__init__ / UNet.forward of the reference (model/sr3_modules/unet.py:162-259,
// model/ddpm_modules/unet.py:148-243) as a static op list over the HIP kernels of this library.
// Nothing here is a translation of the reference modules: the forward is compiled once per batch
// size into a flat list of kernel launches over a liveness-planned NHWC workspace.
#include <stdarg.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "plan_internal.h"
#include "tile_code.h"
#include "train.h"

namespace sr3 {

// ---------------------------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------------------------
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

// ---------------------------------------------------------------------------------------------
// parameter table
// ---------------------------------------------------------------------------------------------
static size_t add_param(sr3_plan* P, const std::string& name, int ndim, const int* shape, int pack, size_t* cursor) {
  sr3_param_info pi;
  memset(&pi, 0, sizeof(pi));
  snprintf(pi.name, sizeof(pi.name), "%s", name.c_str());
  pi.ndim = ndim;
  size_t n = 1;
  for (int i = 0; i < ndim; ++i) { pi.shape[i] = shape[i]; n *= (size_t)shape[i]; }
  pi.pack = pack;
  pi.numel = n;
  *cursor = (*cursor + 3) & ~(size_t)3;   // 16-byte alignment of every tensor
  pi.offset = *cursor;
  *cursor += n;
  P->pindex[name] = (int)P->params.size();
  P->params.push_back(pi);
  return pi.offset;
}
static size_t add_vec(sr3_plan* P, const std::string& name, int n, size_t* cur) {
  int s[1] = {n};
  return add_param(P, name, 1, s, 0, cur);
}
static size_t add_mat(sr3_plan* P, const std::string& name, int o, int i, size_t* cur) {
  int s[2] = {o, i};
  return add_param(P, name, 2, s, 0, cur);
}
static size_t add_conv(sr3_plan* P, const std::string& name, int o, int i, int k, size_t* cur) {
  int s[4] = {o, i, k, k};
  return add_param(P, name, 4, s, k == 1 ? 0 : 1, cur);
}

static bool in_list(const int* v, int n, int x) {
  for (int i = 0; i < n; ++i) if (v[i] == x) return true;
  return false;
}

static int build_structure(sr3_plan* P) {
  const sr3_unet_desc& d = P->d;
  const int inner = d.inner_channel;
  const bool ddpm = d.variant == SR3_VARIANT_DDPM;
  if (inner <= 0 || (inner & 3)) { set_error("inner_channel must be a positive multiple of 4 (got %d)", inner); return SR3_E_UNSUPPORTED; }
  if (d.n_mults < 1 || d.n_mults > 8 || d.n_attn_res < 0 || d.n_attn_res > 8) { set_error("bad n_mults/n_attn_res"); return SR3_E_BADARG; }
  if (d.norm_groups <= 0) { set_error("norm_groups must be > 0"); return SR3_E_BADARG; }
  if (d.in_channel <= 0 || d.in_channel > 16) { set_error("in_channel %d unsupported", d.in_channel); return SR3_E_UNSUPPORTED; }
  const int out_ch = d.out_channel > 0 ? d.out_channel : d.in_channel;
  // 6 and 8: a prediction and its variance head (2C of C = 3 / 4), runnable under plan option var_channels alone (check_out_rows)
  if (out_ch > 4 && out_ch != 6 && out_ch != 8) { set_error("out_channel %d > 4 unsupported", out_ch); return SR3_E_UNSUPPORTED; }
  if ((d.image_size >> (d.n_mults - 1)) < 1 || (d.image_size & ((1 << (d.n_mults - 1)) - 1))) {
    set_error("image_size %d not divisible by 2^%d", d.image_size, d.n_mults - 1);
    return SR3_E_BADARG;
  }
  P->out_ch = out_ch;

  // ---- pass 1: topology (same walk as UNet.__init__) ----
  struct Proto { LayerKind kind; int cin, cout, skip; bool attn; };
  std::vector<Proto> pd, pm, pu;
  std::vector<int> feat;
  int pre = inner, now_res = d.image_size;
  feat.push_back(pre);
  pd.push_back({L_CONV_IN, d.in_channel, inner, 0, false});
  for (int ind = 0; ind < d.n_mults; ++ind) {
    const bool is_last = ind == d.n_mults - 1;
    const bool use_attn = in_list(d.attn_res, d.n_attn_res, now_res);
    const int cm = inner * d.channel_mults[ind];
    for (int r = 0; r < d.res_blocks; ++r) {
      pd.push_back({L_RES, pre, cm, 0, use_attn});
      feat.push_back(cm);
      pre = cm;
    }
    if (!is_last) {
      pd.push_back({L_DOWN, pre, pre, 0, false});
      feat.push_back(pre);
      now_res /= 2;
    }
  }
  pm.push_back({L_RES, pre, pre, 0, true});
  pm.push_back({L_RES, pre, pre, 0, false});
  for (int ind = d.n_mults - 1; ind >= 0; --ind) {
    const bool is_last = ind < 1;
    const bool use_attn = in_list(d.attn_res, d.n_attn_res, now_res);
    const int cm = inner * d.channel_mults[ind];
    for (int r = 0; r < d.res_blocks + 1; ++r) {
      const int skip = feat.back();
      feat.pop_back();
      pu.push_back({L_RES, pre + skip, cm, skip, use_attn});
      pre = cm;
    }
    if (!is_last) {
      pu.push_back({L_UP, pre, pre, 0, false});
      now_res *= 2;
    }
  }
  P->fin_cin = pre;

  // ---- pass 2: arena.  FiLM projections first (contiguous => one GEMV for all blocks) ----
  size_t cur = 0;
  int F = 0;
  auto count_f = [&](const std::vector<Proto>& v) { for (auto& p : v) if (p.kind == L_RES) F += p.cout; };
  count_f(pd); count_f(pm); count_f(pu);
  P->F = F;
  P->film_w = cur; cur += (size_t)F * inner;
  cur = (cur + 3) & ~(size_t)3;
  P->film_b = cur; cur += (size_t)F;
  int frow = 0;

  const char* emb = ddpm ? "time_mlp" : "noise_level_mlp";
  P->emb_w1 = add_mat(P, std::string(emb) + ".1.weight", 4 * inner, inner, &cur);
  P->emb_b1 = add_vec(P, std::string(emb) + ".1.bias", 4 * inner, &cur);
  P->emb_w2 = add_mat(P, std::string(emb) + ".3.weight", inner, 4 * inner, &cur);
  P->emb_b2 = add_vec(P, std::string(emb) + ".3.bias", inner, &cur);

  auto emit = [&](const std::vector<Proto>& protos, const char* grp, std::vector<Layer>& out) {
    for (size_t i = 0; i < protos.size(); ++i) {
      const Proto& pr = protos[i];
      Layer L;
      L.kind = pr.kind;
      L.cin = pr.cin;
      L.cout = pr.cout;
      char nm[64];
      snprintf(nm, sizeof(nm), "%s.%zu", grp, i);
      L.name = nm;
      L.w = L.b = 0;
      std::string n = nm;
      if (pr.kind == L_CONV_IN) {
        L.w = add_conv(P, n + ".weight", pr.cout, pr.cin, 3, &cur);
        L.b = add_vec(P, n + ".bias", pr.cout, &cur);
      } else if (pr.kind == L_DOWN || pr.kind == L_UP) {
        L.w = add_conv(P, n + ".conv.weight", pr.cout, pr.cin, 3, &cur);
        L.b = add_vec(P, n + ".conv.bias", pr.cout, &cur);
      } else {
        ResLayer& R = L.res;
        R.name = n;
        R.cin = pr.cin; R.cout = pr.cout; R.skip = pr.skip; R.attn = pr.attn;
        R.film_off = frow;
        std::string rb = n + ".res_block";
        // FiLM rows live in the contiguous block; the table entries point into it
        {
          sr3_param_info pi;
          memset(&pi, 0, sizeof(pi));
          std::string wn = rb + (ddpm ? ".mlp.1.weight" : ".noise_func.noise_func.0.weight");
          std::string bn = rb + (ddpm ? ".mlp.1.bias" : ".noise_func.noise_func.0.bias");
          snprintf(pi.name, sizeof(pi.name), "%s", wn.c_str());
          pi.ndim = 2; pi.shape[0] = pr.cout; pi.shape[1] = inner; pi.pack = 0;
          pi.numel = (size_t)pr.cout * inner; pi.offset = P->film_w + (size_t)frow * inner;
          P->pindex[wn] = (int)P->params.size(); P->params.push_back(pi);
          memset(&pi, 0, sizeof(pi));
          snprintf(pi.name, sizeof(pi.name), "%s", bn.c_str());
          pi.ndim = 1; pi.shape[0] = pr.cout; pi.pack = 0; pi.numel = (size_t)pr.cout; pi.offset = P->film_b + frow;
          P->pindex[bn] = (int)P->params.size(); P->params.push_back(pi);
        }
        frow += pr.cout;
        R.gn1_w = add_vec(P, rb + ".block1.block.0.weight", pr.cin, &cur);
        R.gn1_b = add_vec(P, rb + ".block1.block.0.bias", pr.cin, &cur);
        R.c1_w = add_conv(P, rb + ".block1.block.3.weight", pr.cout, pr.cin, 3, &cur);
        R.c1_b = add_vec(P, rb + ".block1.block.3.bias", pr.cout, &cur);
        R.gn2_w = add_vec(P, rb + ".block2.block.0.weight", pr.cout, &cur);
        R.gn2_b = add_vec(P, rb + ".block2.block.0.bias", pr.cout, &cur);
        R.c2_w = add_conv(P, rb + ".block2.block.3.weight", pr.cout, pr.cout, 3, &cur);
        R.c2_b = add_vec(P, rb + ".block2.block.3.bias", pr.cout, &cur);
        R.has_rc = pr.cin != pr.cout;
        R.rc_w = R.rc_b = 0;
        if (R.has_rc) {
          R.rc_w = add_conv(P, rb + ".res_conv.weight", pr.cout, pr.cin, 1, &cur);
          R.rc_b = add_vec(P, rb + ".res_conv.bias", pr.cout, &cur);
        }
        R.an_w = R.an_b = R.qkv_w = R.ao_w = R.ao_b = 0;
        if (pr.attn) {
          std::string at = n + ".attn";
          R.an_w = add_vec(P, at + ".norm.weight", pr.cout, &cur);
          R.an_b = add_vec(P, at + ".norm.bias", pr.cout, &cur);
          R.qkv_w = add_conv(P, at + ".qkv.weight", 3 * pr.cout, pr.cout, 1, &cur);
          R.ao_w = add_conv(P, at + ".out.weight", pr.cout, pr.cout, 1, &cur);
          R.ao_b = add_vec(P, at + ".out.bias", pr.cout, &cur);
        }
      }
      out.push_back(L);
    }
  };
  emit(pd, "downs", P->downs);
  emit(pm, "mid", P->mid);
  emit(pu, "ups", P->ups);
  P->fin_gn_w = add_vec(P, "final_conv.block.0.weight", P->fin_cin, &cur);
  P->fin_gn_b = add_vec(P, "final_conv.block.0.bias", P->fin_cin, &cur);
  P->fin_w = add_conv(P, "final_conv.block.3.weight", out_ch, P->fin_cin, 3, &cur);
  P->fin_b = add_vec(P, "final_conv.block.3.bias", out_ch, &cur);
  P->param_floats = (cur + 3) & ~(size_t)3;
  layout_derived(P);

  // every GroupNorm must divide
  auto chk = [&](int c) { return c % d.norm_groups == 0; };
  bool ok = chk(P->fin_cin);
  for (auto* v : {&P->downs, &P->mid, &P->ups})
    for (auto& L : *v)
      if (L.kind == L_RES) ok = ok && chk(L.res.cin) && chk(L.res.cout);
  if (!ok) { set_error("a GroupNorm channel count is not divisible by norm_groups=%d", d.norm_groups); return SR3_E_BADARG; }
  return SR3_OK;
}

// ---------------------------------------------------------------------------------------------
// activation plan (first-fit free list, byte offsets; sizes scale with batch)
// ---------------------------------------------------------------------------------------------
struct Arena {
  struct Blk { size_t off, size; };
  std::vector<Blk> free_list;
  size_t top = 0, high = 0;
  size_t alloc(size_t bytes) {
    bytes = (bytes + 255) & ~(size_t)255;
    for (size_t i = 0; i < free_list.size(); ++i) {
      if (free_list[i].size >= bytes) {
        const size_t off = free_list[i].off;
        free_list[i].off += bytes;
        free_list[i].size -= bytes;
        if (free_list[i].size == 0) free_list.erase(free_list.begin() + i);
        return off;
      }
    }
    const size_t off = top;
    top += bytes;
    if (top > high) high = top;
    return off;
  }
  void release(size_t off, size_t bytes) {
    bytes = (bytes + 255) & ~(size_t)255;
    free_list.push_back({off, bytes});
    std::sort(free_list.begin(), free_list.end(), [](const Blk& a, const Blk& b) { return a.off < b.off; });
    for (size_t i = 0; i + 1 < free_list.size();) {
      if (free_list[i].off + free_list[i].size == free_list[i + 1].off) {
        free_list[i].size += free_list[i + 1].size;
        free_list.erase(free_list.begin() + i + 1);
      } else {
        ++i;
      }
    }
    if (!free_list.empty() && free_list.back().off + free_list.back().size == top) {
      top = free_list.back().off;
      free_list.pop_back();
    }
  }
};

// Does the RAGGED two-workgroup Winograd tile (tile_cfg 23) beat the kernel this conv would otherwise land on?  Measured inside the
// forward of the SR3 16 -> 128 network, conv + reduce + statistics + fold against the same group on the fallback kernels
// (profiles/geometry_wino_ragged_probe.txt): 0.24-0.57 of the fallback's time on every map that fills at
// least a third of its rounded-up tile grid (8x12: 75 %, 44x32: 92 %, 22x16: 69 %, 11x8: 34 %, 8x8 upsampled: 50 %), 1.2-1.27 of it
// on the 4x4 maps (12.5 %: seven eighths of every tile is padding, and the im2col kernel under 16-way split-K is not slower
// there).  Nothing was measured between 12.5 % and 34 %: the threshold sits in the gap, at a quarter.
bool wino_ragged_wins(const ConvParams& c) {
  const long padded = (long)((c.Ho + 7) / 8 * 8) * ((c.Wo + 15) / 16 * 16);
  return 4L * c.Ho * c.Wo >= padded;
}

// Which 3x3 stride-1 convs run on the Winograd kernels (plan option `winograd`; 0: none), train-mode dropout convs included; an explicit
// tile_cfg / split_bf16 keep the direct halo kernels (the fused res_conv segment has no Winograd form: res_conv is then its own 1x1 GEMM)
// 1: the tiles of today's rules (wino_geometry of the 8-wave kernel decides, *wg is that geometry; choose_conv then picks the instantiation);
// 2: only at a geometry other than image_size x image_size (so the native launch list never moves), inference plans and -- plan option
// train_geom -- the training forward's convs without dropout: a map the rule
// above refuses on the two-workgroup kernel -- its plain form where the map is a whole multiple of the 8 x 16 tile, its RAGGED form
// (plan option wino_ragged) where wino_ragged_wins says the padded tile beats the fallback
static int wino_mode(const sr3_plan* P, const ConvParams& c, size_t w, bool has_q, bool has_drop, bool train, WinoGeom* wg) {
  if (!P->winograd || P->tile_cfg != 0 || P->split_bf16 || has_q) return 0;
  if (has_drop && (c.C1 != 0 || c.ups != 0 || c.act == 0)) return 0;    // the dropout form: single source, no upsampling
  if (c.ksize != 3 || c.stride != 1 || !P->derived_of.count(w)) return 0;
  if (wino_geometry(c, wg)) return 1;
  if ((train && !P->train_geom) || has_drop || plan_native_geometry(P) || !P->wino_split || !P->wino2) return 0;
  ConvParams r = c;
  r.wino_split = wino2_fits(c) ? 2 : 3;
  if (r.wino_split == 3 && !(P->wino_ragged && wino_ragged_wins(c))) return 0;
  return wino_geometry(r, wg) ? 2 : 0;
}

// The kernel one conv of a plan runs on (ConvChoice, plan_internal.h): THE place where the planner decides it (Builder::conv only emits what
// this returns).  RULE_HEAD stops behind the first conv_pick, with neither the split_bf16 tile nor igemm_split: what Builder::fuses_res_conv
// has always asked
enum ChoiceRule { RULE_FULL, RULE_HEAD };
static ConvChoice choose_conv(const sr3_plan* P, ConvParams c, size_t w, bool has_q, bool has_drop, bool train, ChoiceRule rule = RULE_FULL) {
  ConvChoice ch = {P->tile_cfg, P->ksplit, 0, 0, 0, 0, false, 0};
  const bool full = rule == RULE_FULL;
  auto repick = [&](int tile) { const ConvPick pk = conv_pick(c, tile, P->ksplit); ch.tile_cfg = pk.tile; ch.ksplit = pk.ksplit; };
  // opt-in: the 3 x bf16 split MFMA instantiation of the 8-wave tile wherever it fits (inference plans only)
  HaloGeom sg; WinoGeom wg;
  if (full && P->split_bf16 && !train && ch.tile_cfg == 0 && c.ksize == 3 && c.stride == 1 && c.Cout > 64 && halo_geometry(c, 10, &sg)) ch.tile_cfg = 10;
  ch.wino_mode = wino_mode(P, c, w, has_q, has_drop, train, &wg);
  if (ch.wino_mode) {
    ch.tile_cfg = 11;
    ch.wino_off = P->derived_of.at(w);
    // plan option wino_split: the 3 x bf16 split instantiation where it exists (the one-image tile; training plan and train-mode
    // dropout included); 2: the 8 x 16 tile of conv3x3_wino2.hip, 3: its ragged form.  Its filters sit behind the conv's fp32 ones
    if (ch.wino_mode == 2) c.wino_split = wino2_fits(c) ? 2 : 3;
    else if (P->wino_split && (wg.NB == 1 || (P->wino_split8 && !has_drop))) c.wino_split = (P->wino2 && !has_drop && wg.NB == 1) ? 2 : 1;
    if (c.wino_split) ch.wino_off += wino_weight_floats(c.Cout, c.C0 + c.C1);
  }
  if (full) {
    c.igemm_split = igemm_split_rule(P, c);      // (read by conv_pick / conv_forward only when the conv lands on the im2col kernel)
    // (... unless the plain GEMM kernel takes the layer on its 64-column tile: plan options gemm2 + gemm_s2 + gemm_n64, below)
    if (P->gemm_split && P->gemm2 && P->gemm_s2 && P->gemm_n64 && c.ksize == 3 && c.stride == 2 && P->wsplit_of.count(w) && gemm1x1_fits(c, 2)) c.igemm_split = 1;
  }
  repick(ch.tile_cfg);
  ch.wino_split = c.wino_split;
  // plan option wino_up = 0 (A/B knob): Upsample's conv keeps all sixteen positions on the two-workgroup kernel (reported as tile 25 / 26)
  ch.wino_full = (ch.tile_cfg == 11 && c.wino_split >= 2 && c.ups == 1 && !P->wino_up) ? 1 : 0;
  if (!full) return ch;
  const bool presplit = c.igemm_split && P->wsplit_of.count(w);      // (a SPLIT conv whose pre-split weights the derived buffer holds)
  if (P->gemm_tile >= 1 && P->gemm_tile <= 4 && ch.tile_cfg >= 1 && ch.tile_cfg <= 4 && P->tile_cfg == 0) repick(P->gemm_tile);       // A/B knob: one im2col tile for every conv of that kernel
  if (presplit && ch.tile_cfg >= 1 && ch.tile_cfg <= 4 && P->gemm2 && P->tile_cfg == 0 && P->gemm_tile == 0) {
    // plan option gemm2: 1x1 stride-1 convs -- and Downsample's 3x3 stride-2 ones -- the plain GEMM kernel fits (gemm1x1.hip)
    if (gemm1x1_fits(c, 2) && (c.ksize == 1 || P->gemm_s2) && (!(c.Cout & 127) || P->gemm_n64)) { repick(22); ch.has_wsplit = true; }
  }
  if (presplit && ch.tile_cfg >= 1 && ch.tile_cfg <= 4 && P->gemm_wpre) ch.has_wsplit = true;       // the SPLIT tile reads its weights pre-split from the derived buffer
  if (ch.has_wsplit) ch.wsplit_off = P->wsplit_of.at(w);
  if (has_drop && ch.tile_cfg == 9) repick(5);       // no dropout instantiation of the 8-wave tile
  // dropout convs on the 256x64 tile run its 8-wave form (conv3x3_halo_forward); SR3_DROP_CFG5 forces the
  // half-empty 128x128 tile instead (A/B knob)
  static const bool use5 = getenv("SR3_DROP_CFG5") != nullptr;
  if (has_drop && ch.tile_cfg == 6 && use5) repick(5);
  // opt-in: run the halo-tile convs on the 3 x bf16 split MFMA instantiations (inference plans only)
  if (P->split_bf16 && !train && ch.tile_cfg == 5) ch.tile_cfg = 7;
  else if (P->split_bf16 && !train && ch.tile_cfg == 9) ch.tile_cfg = 10;
  else if (P->split_bf16 && !train && ch.tile_cfg == 6) ch.tile_cfg = 8;
  ch.igemm_split = c.igemm_split;
  return ch;
}

struct Builder {
  sr3_plan* P;
  int B;
  Arena act;
  std::vector<Tensor> T;          // tensor table; handles are indices (shared state, no copies)
  size_t stats_cursor = 0;
  size_t max_scratch = 0;
  int max_cin = 0;
  double flops = 0;
  std::vector<Op>& ops;
  bool train = false;
  size_t gn_cursor = 0, mr_cursor = 0;     // train: persistent per-GroupNorm tables
  size_t cur_ss = 0, cur_mr = 0;           // tables written by the most recent fold
  size_t cur_gamma = 0, cur_beta = 0;
  Builder(sr3_plan* p, int b, bool tr = false) : P(p), B(b), ops(tr ? p->tops : p->ops), train(tr) {}

  int make(int C, int H, int W) {
    Tensor t;
    t.C = C; t.H = H; t.W = W;
    t.bytes = (size_t)B * H * W * C * sizeof(float);
    t.off = act.alloc(t.bytes);
    t.valid = true;
    T.push_back(t);
    return (int)T.size() - 1;
  }
  void drop(int h) {
    if (h < 0 || !T[h].valid) return;
    if (train) return;                     // the backward needs every activation
    if (!P->keep_all) act.release(T[h].off, T[h].bytes);
    T[h].valid = false;
  }
  void stat_slot(int h, int parts) {
    Tensor& t = T[h];
    t.stat_T = parts;
    t.stat_off = stats_cursor;
    stats_cursor += (size_t)B * parts * t.C * 2 * sizeof(double);
    t.stats_done = true;
  }
  void ensure_stats(int h) {
    Tensor& t = T[h];
    if (t.stats_done) return;
    stat_slot(h, chan_stats_slices(B, t.H * t.W, t.C));
    Op o; o.kind = OP_STATS;
    o.stats = {t.off, t.stat_off, t.H * t.W, t.C};
    ops.push_back(o);
    last_stats_op = (int)ops.size() - 1; last_stats_h = h;
  }
  int last_conv_op = -1, last_conv_out = -1, last_stats_op = -1, last_stats_h = -1;
  // plan option fold_fuse: can the kernel that completes `fresh` (one of x0 / x1) also do this fold?  Fills the op's `tail`.
  bool fuse_fold_into(Op& L, int fresh, int x0, int x1, size_t gamma, size_t beta, size_t ss_rel, size_t mr_rel, bool has_mr) {
    const int other = fresh == x0 ? x1 : x0;
    const int Cf = T[x0].C + (x1 >= 0 ? T[x1].C : 0);
    const int c_off = fresh == x0 ? 0 : T[x0].C;
    if (!fold_tail_fits(T[fresh].C, Cf, c_off, P->d.norm_groups)) return false;
    if (other >= 0 && !T[other].stats_done) return false;
    L.fold_fused = true;
    FoldSpec& f = L.tail;
    f.Ctot = Cf; f.c_off = c_off;
    if (other >= 0) { f.ostat = T[other].stat_off; f.oC = T[other].C; f.oT = T[other].stat_T; f.o_off = fresh == x0 ? T[x0].C : 0; }
    f.gamma = gamma; f.beta = beta; f.ss_rel = ss_rel; f.mr_rel = mr_rel; f.has_mr = has_mr;
    T[fresh].stat_T = 1;              // the fused kernel holds whole-image sums: one partial per image
    return true;
  }
  void fold(int x0, int x1, size_t gamma, size_t beta) {
    const int Cf = T[x0].C + (x1 >= 0 ? T[x1].C : 0);
    // the tables this fold writes, whichever kernel does it: per-GroupNorm slots in training, the one shared region (offset 0) in inference
    size_t ss_rel = 0, mr_rel = 0;
    if (train) {
      ss_rel = gn_cursor; gn_cursor += ((size_t)B * Cf * 2 * sizeof(float) + 255) & ~(size_t)255;
      mr_rel = mr_cursor; mr_cursor += ((size_t)B * P->d.norm_groups * 2 * sizeof(float) + 255) & ~(size_t)255;
    }
    cur_ss = ss_rel; cur_mr = mr_rel; cur_gamma = gamma; cur_beta = beta;
    max_cin = std::max(max_cin, Cf);
    if (P->fold_fuse && !ops.empty()) {
      // (a) the op just emitted is a split-K conv whose reduce writes the statistics of x0 / x1: its reduce folds too
      Op& L = ops.back();
      if (last_conv_op == (int)ops.size() - 1 && L.kind == OP_CONV && L.conv.ch.ksplit > 1 && L.conv.ostat != NO_OFF && (last_conv_out == x0 || last_conv_out == x1) &&
          fuse_fold_into(L, last_conv_out, x0, x1, gamma, beta, ss_rel, mr_rel, train)) return;
    }
    ensure_stats(x0);
    if (x1 >= 0) ensure_stats(x1);
    // (b) ... or a stand-alone statistics pass of x0 / x1: it folds too
    if (P->fold_fuse && !ops.empty() && last_stats_op == (int)ops.size() - 1 && (last_stats_h == x0 || last_stats_h == x1) &&
        fuse_fold_into(ops.back(), last_stats_h, x0, x1, gamma, beta, ss_rel, mr_rel, train)) return;
    Op o; o.kind = OP_FOLD;
    Op::Fold& f = o.fold;
    f.stat0 = T[x0].stat_off; f.C0 = T[x0].C; f.T0 = T[x0].stat_T;
    if (x1 >= 0) { f.stat1 = T[x1].stat_off; f.C1 = T[x1].C; f.T1 = T[x1].stat_T; }
    f.pixels = T[x0].H * T[x0].W;
    f.gamma = gamma; f.beta = beta; f.has_mr = train;
    o.ss_rel = ss_rel; o.mr_rel = mr_rel;
    ops.push_back(o);
  }
  // generic conv over the virtual concat (x0|x1); residual is the concat view (r0|r1).  Emission only: choose_conv picks the kernel
  int conv(const ConvSpec& s) {
    const int x0 = s.x0, x1 = s.x1, Cout = s.Cout;
    const bool has_q = s.q0 >= 0;
    auto off = [&](int h) { return h >= 0 ? T[h].off : NO_OFF; };
    Op o; o.kind = OP_CONV;
    Op::Conv& v = o.conv;
    ConvParams& c = v.cp;
    c = conv_shape(B, T[x0].H, T[x0].W, s.ups, s.stride, s.ksize, T[x0].C, x1 >= 0 ? T[x1].C : 0, Cout);
    const int Ho = c.Ho, Wo = c.Wo;
    const int out = make(Cout, Ho, Wo);
    c.act = s.act; c.film_stride = P->F;
    c.RC0 = s.r0 >= 0 ? T[s.r0].C : 0; c.RC1 = s.r1 >= 0 ? T[s.r1].C : 0;
    v.src0 = T[x0].off; v.src1 = off(x1);
    v.w = s.w; v.bias = s.bias;
    v.film_row = s.film_row;
    v.res0 = off(s.r0); v.res1 = off(s.r1);
    v.out = T[out].off;
    o.ss_rel = s.act ? cur_ss : 0;
    v.has_drop = train && s.drop_key >= 0; v.drop_key = (unsigned)(s.drop_key >= 0 ? s.drop_key : 0);
    v.ch = choose_conv(P, c, s.w, has_q, v.has_drop, train);
    const ConvChoice& ch = v.ch;
    c.wino_split = ch.wino_split; c.wino_full = ch.wino_full; c.igemm_split = ch.igemm_split;
    if (train) {
      Rec r;
      r.kind = R_CONV; r.s = s; r.out = out;
      r.gamma = cur_gamma; r.beta = cur_beta; r.ss_off = cur_ss; r.mr_off = cur_mr;
      P->recs.push_back(r);
    }
    if (has_q) {   // fused 1x1 segment (res_conv); caller checked fuses_res_conv()
      c.x2_C0 = T[s.q0].C; c.x2_C1 = s.q1 >= 0 ? T[s.q1].C : 0;
      v.x2_src0 = T[s.q0].off; v.x2_src1 = off(s.q1);
      v.x2_w = s.qw; v.x2_bias = s.qb;
    }
    if (ch.ksplit > 1) max_scratch = std::max(max_scratch, (size_t)ch.ksplit * B * Ho * Wo * Cout * sizeof(float));
    // split-K convs leave the statistics to the (cheap, small-tensor) stand-alone pass
    auto writes_stats = [&](int parts) { stat_slot(out, parts); v.ostat = T[out].stat_off; };
    if (s.want_stats && P->fuse_stats && ch.ksplit == 1 && ch.tile_cfg == 11) {
      WinoGeom wg = {};      // (stays empty -- no slices -- where plan option tile_cfg forces tile 11 on a conv it does not fit)
      wino_geometry(c, &wg);
      writes_stats(wino_stats_slices(wg));
    } else if (s.want_stats && P->fuse_stats && ch.ksplit == 1 && ch.tile_cfg >= 5) {
      HaloGeom hg;
      if (halo_geometry(c, ch.tile_cfg, &hg)) writes_stats(halo_stats_slices(hg));
    } else if (s.want_stats && P->fuse_stats && ch.ksplit > 1) {
      const int rpb = splitk_rows_per_block(c, true);      // statistics come out of the split-K reduce
      if (rpb > 0) writes_stats((Ho * Wo) / rpb);
    }
    ops.push_back(o);
    last_conv_op = (int)ops.size() - 1; last_conv_out = out;
    flops += conv_flops(c);
    return out;
  }
  // Does block2's conv of this block -- on a map the size of tensor `at` -- take res_conv as a second K-segment?  Only the unsplit halo kernel:
  // the Winograd kernel has no second segment (training plan included), and under split-K the fused segment runs in the last split only (50
  // k-steps there vs 18 in the others for a 1024-channel res_conv at 8x8: measured 43 TF).  Otherwise res_conv is its own 1x1 GEMM and joins
  // as a residual.  Asked by fork_side before h1 exists, and again when block2's conv is emitted: one rule, the head of choose_conv
  bool fuses_res_conv(int at, const ResLayer& R) {
    if (!P->fuse_res) return false;
    ConvParams c = conv_shape(B, T[at].H, T[at].W, 0, 1, 3, R.cout, 0, R.cout);
    c.act = 2;
    const ConvChoice ch = choose_conv(P, c, R.c2_w, false, train, train, RULE_HEAD);
    return !ch.wino_mode && ch.tile_cfg >= 5 && ch.ksplit == 1;
  }
  std::string refused;     // inference: the first layer no kernel can run at this geometry (build_forward refuses the plan with it)
  int n_side = 0;          // plan option fork_side: ops handed to the side stream so far (Op::side_id)
  int res_block(int x0, int x1, const ResLayer& R) {
    fold(x0, x1, R.gn1_w, R.gn1_b);
    // plan option fork_side (inference): res_conv reads only the block input, so it is emitted HERE -- behind the fold, in front of block1's
    // conv -- and launched on the side stream; block2's conv, which adds it as its residual, waits for it.  Only unsplit: a split-K res_conv
    // would share the slab region with block1's conv.  (The fold stays where fold_fuse looks for it: behind the op that completes x.)
    const ConvSpec res_conv = {.x0 = x0, .x1 = x1, .Cout = R.cout, .ksize = 1, .w = R.rc_w, .bias = R.rc_b};
    int r_side = -1, r_id = -1;
    if (R.has_rc && P->fork_side && !train && !fuses_res_conv(x0, R)) {
      r_side = conv(res_conv);
      if (ops.back().kind == OP_CONV && ops.back().conv.ch.ksplit == 1) { r_id = n_side++; ops.back().side_id = r_id; }
    }
    const int h1 = conv({.x0 = x0, .x1 = x1, .Cout = R.cout, .act = 2, .w = R.c1_w, .bias = R.c1_b, .film_row = R.film_off, .want_stats = true});
    fold(h1, -1, R.gn2_w, R.gn2_b);
    // block2's conv; what it adds: res_conv's output (its own launch), res_conv as a fused K-segment over the block input, or the input itself
    ConvSpec block2 = {.x0 = h1, .Cout = R.cout, .act = 2, .w = R.c2_w, .bias = R.c2_b, .want_stats = true, .drop_key = R.film_off};
    int out;
    if (r_side >= 0) {
      block2.r0 = r_side;
      out = conv(block2);
      if (r_id >= 0) ops[last_conv_op].wait_id = r_id;
      drop(r_side);
    } else if (R.has_rc && fuses_res_conv(h1, R)) {
      block2.q0 = x0; block2.q1 = x1; block2.qw = R.rc_w; block2.qb = R.rc_b;
      out = conv(block2);
    } else if (R.has_rc) {
      block2.r0 = conv(res_conv);
      out = conv(block2);
      drop(block2.r0);
    } else {
      block2.r0 = x0; block2.r1 = x1;
      out = conv(block2);
    }
    drop(h1);
    if (R.attn) {
      fold(out, -1, R.an_w, R.an_b);
      const int qkv = conv({.x0 = out, .Cout = 3 * R.cout, .ksize = 1, .act = 1, .w = R.qkv_w});
      const int o = make(R.cout, T[out].H, T[out].W);
      Op a; a.kind = OP_ATTN;
      const int tokens = T[out].H * T[out].W;
      a.attn = {T[qkv].off, T[o].off, tokens, R.cout, 0, plan_attn_heads(P, R.cout)};
      const bool geo = !train || P->train_geom;       // (a training plan off the native geometry exists under train_geom only)
      if (geo && P->attn_long && !attention_fits(tokens, R.cout)) a.attn.tile_cfg = 24;       // the key-blocked kernel: any token count
      else if (geo && refused.empty() && !attention_fits(tokens, R.cout)) {
        char msg[256];
        snprintf(msg, sizeof(msg), "attention of %s: the %d x %d level has %d tokens, more than the attention kernel holds in LDS", R.name.c_str(),
                 T[out].H, T[out].W, tokens);
        refused = msg;
      }
      ops.push_back(a);
      if (train) { Rec r; r.kind = R_ATTN; r.qkv = qkv; r.o = o; r.heads = a.attn.heads; P->recs.push_back(r); }
      flops += attn_flops(B, tokens, R.cout);
      drop(qkv);
      const int out2 = conv({.x0 = o, .Cout = R.cout, .ksize = 1, .w = R.ao_w, .bias = R.ao_b, .r0 = out, .want_stats = true});
      drop(o);
      drop(out);
      out = out2;
    }
    return out;
  }
};

// the UNet.forward walk (downs -> mid -> ups -> final), emitting ops through the builder
static void walk_forward(sr3_plan* P, Builder& bld, int cond_channels) {
  const sr3_unet_desc& d = P->d;
  std::vector<Op>& ops = bld.ops;
  const int B = bld.B;
  const int inner = d.inner_channel;
  const bool geo = !bld.train || P->train_geom;      // (training: native geometry only, unless plan option train_geom)
  const int IH = geo ? plan_height(P) : d.image_size, IW = geo ? plan_width(P) : d.image_size;

  { Op o; o.kind = OP_EMBED; ops.push_back(o); }
  bld.flops += 2.0 * B * (2.0 * 4 * inner * inner + (double)P->F * inner);

  auto tap = [&](const std::string& name, int h) {
    if (!bld.train) P->taps.push_back({name, bld.T[h].off, bld.T[h].C, bld.T[h].H, bld.T[h].W});
  };
  std::vector<int> feats;
  int cur = -1;
  for (auto& L : P->downs) {
    if (L.kind == L_CONV_IN) {
      cur = bld.make(L.cout, IH, IW);
      Op o; o.kind = OP_CONV_IN;
      Op::ConvIn& v = o.conv_in;
      v.x_channels = d.in_channel - cond_channels; v.cond_channels = cond_channels; v.Cout = L.cout; v.H = IH; v.W = IW;
      v.w = L.w; v.bias = L.b; v.out = bld.T[cur].off;
      if (const int slices = P->fuse_stats ? conv_in_stat_slices(d.in_channel, IH, IW, L.cout) : 0) {
        bld.stat_slot(cur, slices);          // the MFMA form writes the GroupNorm partials of its output itself
        v.ostat = bld.T[cur].stat_off;
      }
      ops.push_back(o);
      if (bld.train) { Rec r; r.kind = R_CONV_IN; r.out = cur; r.s.w = L.w; r.s.bias = L.b; P->recs.push_back(r); }
      bld.flops += 2.0 * B * IH * IW * (double)L.cout * L.cin * 9;
    } else if (L.kind == L_RES) {
      cur = bld.res_block(cur, -1, L.res);   // the input stays alive: it is a skip feature
    } else {
      cur = bld.conv({.x0 = cur, .Cout = L.cout, .stride = 2, .w = L.w, .bias = L.b, .want_stats = true});
    }
    feats.push_back(cur);
    tap(L.name, cur);
  }
  // `cur` is feats.back() here: skip features are released by the up block that consumes them
  bool cur_is_skip = true;
  for (auto& L : P->mid) {
    const int nxt = bld.res_block(cur, -1, L.res);
    if (!cur_is_skip) bld.drop(cur);
    cur = nxt;
    cur_is_skip = false;
    tap(L.name, cur);
  }
  for (auto& L : P->ups) {
    int nxt;
    if (L.kind == L_RES) {
      const int skip = feats.back();
      feats.pop_back();
      nxt = bld.res_block(cur, skip, L.res);
      bld.drop(cur);
      bld.drop(skip);
    } else {
      nxt = bld.conv({.x0 = cur, .Cout = L.cout, .ups = 1, .w = L.w, .bias = L.b, .want_stats = true});
      bld.drop(cur);
    }
    cur = nxt;
    tap(L.name, cur);
  }
  bld.fold(cur, -1, P->fin_gn_w, P->fin_gn_b);
  {
    Op o; o.kind = OP_CONV_OUT;
    o.conv_out = {bld.T[cur].off, P->fin_w, P->fin_b, bld.T[cur].C, P->out_ch, IH, IW};
    o.ss_rel = bld.cur_ss;
    ops.push_back(o);
    if (bld.train) {
      Rec r; r.kind = R_CONV_OUT; r.s.x0 = cur; r.s.w = P->fin_w; r.s.bias = P->fin_b; r.s.act = 2; r.gamma = P->fin_gn_w; r.beta = P->fin_gn_b;
      r.ss_off = bld.cur_ss; r.mr_off = bld.cur_mr;
      P->recs.push_back(r);
    }
    bld.flops += 2.0 * B * IH * IW * (double)P->out_ch * bld.T[cur].C * 9;
  }
}

// derived (Winograd) filters of every 3x3 stride-1 conv: the two convs of each ResnetBlock and the Upsample convs.  Slot of a
// conv: its fp32 fragment-major filters, followed -- plan option wino_split -- by the 3 x bf16 split form of the same filters
// (both are kept: the four-image 8x8 tile, the dropout instantiation and the training plan read the fp32 form)
void layout_derived(sr3_plan* P) {
  P->derived.clear();
  P->derived_of.clear();
  size_t dcur = 0;
  auto reg = [&](size_t w, int Cout, int Cin) {
    if (Cin & 3) return;
    P->derived.push_back({w, Cout, Cin, dcur});
    P->derived_of[w] = dcur;
    dcur += wino_weight_floats(Cout, Cin) + (P->wino_split ? wino_weight_floats(Cout, Cin, true) : 0);
  };
  for (auto* v : {&P->downs, &P->mid, &P->ups})
    for (auto& L : *v) {
      if (L.kind == L_RES) { reg(L.res.c1_w, L.res.cout, L.res.cin); reg(L.res.c2_w, L.res.cout, L.res.cout); }
      else if (L.kind == L_UP) reg(L.w, L.cout, L.cin);
    }
  // the im2col SPLIT tiles' weights, pre-split (plan option gemm_split): res_conv and the attention projections (1x1), Downsample
  // (3x3 stride 2; Cout <= 64 stays on the fp32 MFMA: choose_conv)
  P->wsplits.clear();
  P->wsplit_of.clear();
  if (P->gemm_split && (P->gemm_wpre || P->gemm2)) {
    auto regw = [&](size_t w, int Cout, int taps, int Cin) {
      if (Cin & 3) return;
      if (!P->gemm_wpre && ((taps != 1 && !(taps == 9 && P->gemm_s2)) || (Cout & (P->gemm_n64 ? 63 : 127)) || (Cin & 31))) return;     // gemm2 alone: only what gemm1x1.hip can take (1x1; Downsample's 3x3 stride 2)
      P->wsplits.push_back({w, Cout, taps, Cin, dcur});
      P->wsplit_of[w] = dcur;
      dcur += igemm_wsplit_floats(Cout, taps, Cin);
    };
    for (auto* v : {&P->downs, &P->mid, &P->ups})
      for (auto& L : *v) {
        if (L.kind == L_RES) {
          if (L.res.has_rc) regw(L.res.rc_w, L.res.cout, 1, L.res.cin);
          if (L.res.attn) { regw(L.res.qkv_w, 3 * L.res.cout, 1, L.res.cout); regw(L.res.ao_w, L.res.cout, 1, L.res.cout); }
        } else if (L.kind == L_DOWN && (L.cout > 64 || (P->gemm2 && P->gemm_s2 && P->gemm_n64 && L.cout == 64))) {
          regw(L.w, L.cout, 9, L.cin);
        }
      }
  }
  P->derived_floats = dcur;
  P->derived_from = nullptr;
  if (P->derived_bound_bytes < dcur * sizeof(float)) { P->derived_ptr = nullptr; P->derived_bound_bytes = 0; }   // re-bind a larger one
}

static int build_forward(sr3_plan* P, int B, int cond_channels) {
  if (const int rc = check_out_rows(P)) return rc;
  if (P->built_batch == B && P->built_cond == cond_channels && P->built_h == plan_height(P) && P->built_w == plan_width(P)) return SR3_OK;
  const sr3_unet_desc& d = P->d;
  if (B <= 0) { set_error("batch must be > 0"); return SR3_E_BADARG; }
  if (cond_channels < 0 || cond_channels >= d.in_channel) { set_error("cond_channels %d out of range (in_channel %d)", cond_channels, d.in_channel); return SR3_E_BADARG; }
  P->ops.clear();
  P->taps.clear();
  P->built_batch = -1;
  Builder bld(P, B);
  const int inner = d.inner_channel;
  walk_forward(P, bld, cond_channels);
  if (!bld.refused.empty()) {
    // a geometry no kernel can run is refused HERE, when the launch list is built: never after a launch has been enqueued
    set_error("geometry %d x %d unsupported: %s", plan_height(P), plan_width(P), bld.refused.c_str());
    P->ops.clear();
    P->taps.clear();
    return SR3_E_UNSUPPORTED;
  }
  if (P->fork_side && !P->ops.empty() && P->ops[0].kind == OP_EMBED) {
    // ... and the embedding MLP + FiLM projections (first op, reads only the noise level): beside the input conv, joined by the first conv that
    // adds a FiLM row
    for (Op& o : P->ops)
      if (o.kind == OP_CONV && o.conv.film_row >= 0) {
        if (o.wait_id < 0) { o.wait_id = bld.n_side; P->ops[0].side_id = bld.n_side++; }
        break;
      }
  }
  // ---- fixed regions after the activation arena (high-water mark) ----
  size_t off = (bld.act.high + 255) & ~(size_t)255;
  Regions& R = P->regions;           // (no mean / rstd tables in inference: mr_off stays 0, no op has_mr)
  R.stats_off = off; off += (bld.stats_cursor + 255) & ~(size_t)255;
  R.ss_off = off; off += ((size_t)B * std::max(bld.max_cin, 4) * 2 * sizeof(float) + 255) & ~(size_t)255;
  R.temb_off = off; off += ((size_t)B * inner * sizeof(float) + 255) & ~(size_t)255;
  R.film_off = off; off += ((size_t)B * P->F * sizeof(float) + 255) & ~(size_t)255;
  R.scratch_off = off; R.scratch_bytes = bld.max_scratch; off += (bld.max_scratch + 255) & ~(size_t)255;
  P->ws_bytes = off;
  P->flops = bld.flops;
  P->built_batch = B;
  P->built_cond = cond_channels;
  P->built_h = plan_height(P); P->built_w = plan_width(P);
  return SR3_OK;
}

// ---------------------------------------------------------------------------------------------
// forward driver
// ---------------------------------------------------------------------------------------------
// pointer into the workspace / the arena for an optional offset (NO_OFF: null)
template <typename T> static T* bind(char* base, size_t off) { return off == NO_OFF ? nullptr : reinterpret_cast<T*>(base + off); }
static const float* bind(const float* params, size_t off) { return off == NO_OFF ? nullptr : params + off; }

static FoldTail make_fold_tail(const FoldSpec& s, int groups, const float* params, char* ws, const Regions& R) {
  FoldTail f;
  memset(&f, 0, sizeof(f));
  f.groups = groups; f.Ctot = s.Ctot; f.c_off = s.c_off;
  f.ostat = bind<const double>(ws + R.stats_off, s.ostat); f.oC = s.oC; f.oT = s.oT; f.o_off = s.o_off;
  f.gamma = params + s.gamma; f.beta = params + s.beta; f.eps = 1e-5f;
  f.ss = reinterpret_cast<float*>(ws + R.ss_off + s.ss_rel);
  f.mr = s.has_mr ? reinterpret_cast<float*>(ws + R.mr_off + s.mr_rel) : nullptr;
  return f;
}

int run_forward(sr3_plan* P, bool train, const float* x, const float* cond, int cond_channels, const float* level,
                const int64_t* tstep, const float* freq, const float* level_table, const int* step_dev,
                const float* params, char* ws, float* eps_out, int B, hipStream_t st,
                hipEvent_t* ev, hipEvent_t* mid, const DropCfg* drop, const StepFuse* fuse, const int* t_map, bool full_out) {
  const sr3_unet_desc& d = P->d;
  const Regions& R = train ? P->t_regions : P->regions;
  size_t op_index = 0;
  float* film = reinterpret_cast<float*>(ws + R.film_off);
  char* const stats = ws + R.stats_off;
  // plan option fork_side: ops marked side_id run on the plan's side stream between a fork event (recorded on the caller's stream where the
  // op sits in the list) and a join event their consumer (wait_id) waits for; under per-op timing (ev) everything stays on one stream
  const bool forking = !ev && !train;
  hipStream_t const main_st = st;
  for (const Op& o : train ? P->tops : P->ops) {
    int rc = SR3_OK;
    st = main_st;
    if (ev) SR3_HIP(hipEventRecord(ev[op_index], st));
    ++op_index;
    if (forking && o.wait_id >= 0 && o.wait_id < (int)P->join_ev.size())
      SR3_HIP(hipStreamWaitEvent(main_st, P->join_ev[o.wait_id], 0));
    if (forking && o.side_id >= 0) {
      if (!P->side_stream) SR3_HIP(hipStreamCreateWithFlags(&P->side_stream, hipStreamNonBlocking));
      while ((int)P->fork_ev.size() <= o.side_id) {
        hipEvent_t a, b;
        SR3_HIP(hipEventCreateWithFlags(&a, hipEventDisableTiming));
        SR3_HIP(hipEventCreateWithFlags(&b, hipEventDisableTiming));
        P->fork_ev.push_back(a); P->join_ev.push_back(b);
      }
      SR3_HIP(hipEventRecord(P->fork_ev[o.side_id], main_st));
      SR3_HIP(hipStreamWaitEvent(P->side_stream, P->fork_ev[o.side_id], 0));
      st = P->side_stream;
    }
    switch (o.kind) {
      case OP_RESERVED:
        break;
      case OP_EMBED: {
        EmbedParams e;
        memset(&e, 0, sizeof(e));
        e.variant = d.variant; e.B = B; e.inner = d.inner_channel;
        e.level = level; e.tstep = tstep; e.level_table = level_table; e.step_dev = step_dev; e.t_map = t_map; e.freq = freq;
        e.step_out = fuse ? const_cast<int*>(fuse->step_cur) : nullptr;
        e.w1 = params + P->emb_w1; e.b1 = params + P->emb_b1; e.w2 = params + P->emb_w2; e.b2 = params + P->emb_b2;
        e.wf = params + P->film_w; e.bf = params + P->film_b; e.F = P->F;
        e.temb = reinterpret_cast<float*>(ws + R.temb_off); e.film = film;
        rc = embed_forward(e, st);
        break;
      }
      case OP_CONV_IN: {
        // virtual concat order is [cond | x] (diffusion.py:157); unconditional: x only
        const Op::ConvIn& v = o.conv_in;
        const float* a = cond_channels > 0 ? cond : x;
        const int Ca = cond_channels > 0 ? cond_channels : v.x_channels;
        const float* b = cond_channels > 0 ? x : nullptr;
        const int Cb = cond_channels > 0 ? v.x_channels : 0;
        rc = conv_in_nchw(a, Ca, b, Cb, B, v.H, v.W, params + v.w, params + v.bias, v.Cout, bind<float>(ws, v.out),
                          bind<double>(stats, v.ostat), st);
        break;
      }
      case OP_STATS: {
        const Op::Stats& v = o.stats;
        if (o.fold_fused) {
          FoldTail ft = make_fold_tail(o.tail, d.norm_groups, params, ws, R);
          rc = chan_stats_fold(bind<const float>(ws, v.src), B, v.pixels, v.channels, bind<double>(stats, v.stat), ft, st);
          break;
        }
        rc = chan_stats(bind<const float>(ws, v.src), B, v.pixels, v.channels, bind<double>(stats, v.stat), st);
        break;
      }
      case OP_FOLD: {
        const Op::Fold& v = o.fold;
        rc = gn_finalize(bind<const double>(stats, v.stat0), v.C0, v.T0, bind<const double>(stats, v.stat1), v.C1, v.T1, B, v.pixels,
                         d.norm_groups, params + v.gamma, params + v.beta, 1e-5f, bind<float>(ws, R.ss_off + o.ss_rel), st,
                         v.has_mr ? bind<float>(ws, R.mr_off + o.mr_rel) : nullptr);
        break;
      }
      case OP_CONV: {
        const Op::Conv& v = o.conv;
        const ConvChoice& ch = v.ch;
        ConvParams c = v.cp;
        c.src0 = bind<const float>(ws, v.src0);
        c.src1 = bind<const float>(ws, v.src1);
        c.w = params + v.w;
        c.bias = bind(params, v.bias);
        c.ss = c.act ? bind<const float>(ws, R.ss_off + o.ss_rel) : nullptr;
        c.film = v.film_row >= 0 ? film + v.film_row : nullptr;
        c.res0 = bind<const float>(ws, v.res0);
        c.res1 = bind<const float>(ws, v.res1);
        c.out = bind<float>(ws, v.out);
        c.ostat = bind<double>(stats, v.ostat);
        c.store_wt = P->store_wt;
        c.gemm_epi = 1 + P->launch_gemm_epi();
        if (drop && v.has_drop && drop->thresh != 0) {
          c.drop_seed = drop_layer_seed(drop->seed, v.drop_key); c.drop_thresh = drop->thresh; c.drop_scale = drop->scale;
        }
        if (v.x2_src0 != NO_OFF) {
          c.x2_src0 = bind<const float>(ws, v.x2_src0);
          c.x2_src1 = bind<const float>(ws, v.x2_src1);
          c.x2_w = params + v.x2_w;
          c.x2_bias = params + v.x2_bias;
        }
        if (ch.tile_cfg == 11) {
          if (!P->derived_ptr) { set_error("the plan's derived (Winograd) weights are not bound: call sr3_plan_bind_derived + sr3_plan_prepare_derived"); return SR3_E_BADARG; }
          // stale filters must fail loudly, not compute with the previous weights: the buffer has to have been prepared from
          // THIS arena, under the current options, and not invalidated since (sr3_plan_invalidate_derived after an optimizer step)
          if (P->derived_from != params) {
            set_error("the plan's derived (Winograd) weights are stale or were prepared from another arena: call sr3_plan_prepare_derived");
            return SR3_E_BADARG;
          }
          c.wino_u = P->derived_ptr + ch.wino_off;
        }
        if (ch.has_wsplit && ((ch.tile_cfg >= 1 && ch.tile_cfg <= 4) || ch.tile_cfg == 22) && c.igemm_split) {
          if (!P->derived_ptr || P->derived_from != params) {
            set_error("the plan's derived (pre-split 1x1 / stride-2) weights are not bound or stale: call sr3_plan_bind_derived + sr3_plan_prepare_derived");
            return SR3_E_BADARG;
          }
          c.w_split = P->derived_ptr + ch.wsplit_off;
        }
        FoldTail ft;
        if (o.fold_fused) { ft = make_fold_tail(o.tail, d.norm_groups, params, ws, R); c.fold = &ft; }
        rc = conv_forward(c, ch.tile_cfg, ch.ksplit, bind<float>(ws, R.scratch_off), R.scratch_bytes, st, mid ? mid[op_index - 1] : nullptr);
        break;
      }
      case OP_ATTN: {
        const Op::Attn& v = o.attn;
        // (one head: attention_forward's launches; more: attention_heads.hip)
        rc = attention_forward_heads(bind<const float>(ws, v.qkv), B, v.tokens, v.channels, v.heads, bind<float>(ws, v.out), st,
                                     (P->attn_split ? 1 : 0) | (v.tile_cfg == 24 ? 2 : 0));
        break;
      }
      case OP_CONV_OUT: {
        const Op::ConvOut& v = o.conv_out;
        // the prediction rows alone -- the first rows of the same filters and bias -- unless all rows are asked for
        rc = conv_out_nchw(bind<const float>(ws, v.src), bind<const float>(ws, R.ss_off + o.ss_rel), B, v.H, v.W, v.channels,
                           params + v.w, params + v.bias, (train || full_out) ? v.out_ch : v.out_ch - P->var_channels, eps_out, st, fuse);
        break;
      }
    }
    if (rc) return rc;
    if (forking && o.side_id >= 0) SR3_HIP(hipEventRecord(P->join_ev[o.side_id], st));
  }
  st = main_st;
  if (ev) SR3_HIP(hipEventRecord(ev[op_index], st));
  return SR3_OK;
}

// the forward walk of the training plan (build_train, train_plan.hip)
TrainWalk walk_train(sr3_plan* P, int B, int cond_channels) {
  P->tops.clear();
  P->recs.clear();
  Builder bld(P, B, true);
  walk_forward(P, bld, cond_channels);
  P->ttens = bld.T;
  TrainWalk w;
  w.act_high = bld.act.high; w.stats_bytes = bld.stats_cursor; w.gn_bytes = bld.gn_cursor; w.mr_bytes = bld.mr_cursor;
  w.max_scratch = bld.max_scratch; w.refused = bld.refused;
  return w;
}

}  // namespace sr3

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
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

int sr3_plan_create(const sr3_unet_desc* desc, sr3_plan** out) {
  if (!desc || !out) { set_error("null argument"); return SR3_E_BADARG; }
  sr3_plan* P = new (std::nothrow) sr3_plan();
  if (!P) { set_error("out of host memory"); return SR3_E_NOMEM; }
#ifdef SR3_EXPERIMENTS
  // A/B builds only: defaults of plan options from the environment (a release library's arithmetic does not depend on the environment)
  { const char* e = getenv("SR3_WGRAD_SPLIT"); if (e) P->wgrad_split = atoi(e); }
  { const char* e = getenv("SR3_WINO2"); if (e) P->wino2 = atoi(e); }
#endif
  P->d = *desc;
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
int sr3_plan_num_ops(sr3_plan* plan, int batch) {
  if (!plan) return 0;
  const int cond = plan->built_cond >= 0 ? plan->built_cond : 0;
  if (build_forward(plan, batch, cond)) return -1;
  return (int)plan->ops.size();
}
int sr3_plan_op_info(sr3_plan* plan, int batch, int index, sr3_op_info* out) {
  if (!plan || !out) { set_error("null argument"); return SR3_E_BADARG; }
  const int cond = plan->built_cond >= 0 ? plan->built_cond : 0;
  const int rc = build_forward(plan, batch, cond);
  if (rc) return rc;
  if (index < 0 || index >= (int)plan->ops.size()) { set_error("op index out of range"); return SR3_E_BADARG; }
  const Op& o = plan->ops[index];
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
  const int cond = plan->built_cond >= 0 ? plan->built_cond : 0;
  const int rc = build_forward(plan, batch, cond);
  if (rc) return rc;
  if (index < 0 || index >= (int)plan->ops.size()) { set_error("op index out of range"); return SR3_E_BADARG; }
  if (side_id) *side_id = plan->ops[index].side_id;
  if (wait_id) *wait_id = plan->ops[index].wait_id;
  return SR3_OK;
}
double sr3_plan_forward_flops(sr3_plan* plan, int batch) {
  if (!plan) return 0;
  const int cond = plan->built_cond >= 0 ? plan->built_cond : 0;
  if (build_forward(plan, batch, cond)) return -1;
  return plan->flops;
}
int sr3_store_wt_fits(size_t bytes) { return store_wt_fits(bytes) ? 1 : 0; }
int sr3_plan_set_option(sr3_plan* plan, const char* key, int value) {
  if (!plan || !key) return SR3_E_BADARG;
  int* slot = nullptr;
  if (!strcmp(key, "fuse_stats")) slot = &plan->fuse_stats;
  else if (!strcmp(key, "tile_cfg")) slot = &plan->tile_cfg;
  else if (!strcmp(key, "ksplit")) slot = &plan->ksplit;
  else if (!strcmp(key, "keep_all")) slot = &plan->keep_all;
  else if (!strcmp(key, "fuse_res")) slot = &plan->fuse_res;
  else if (!strcmp(key, "split_bf16")) slot = &plan->split_bf16;
  else if (!strcmp(key, "winograd")) slot = &plan->winograd;
  else if (!strcmp(key, "wino_split")) slot = &plan->wino_split;
  else if (!strcmp(key, "wino_split8")) slot = &plan->wino_split8;
  else if (!strcmp(key, "wgrad_split")) { const int prev = plan->wgrad_split; plan->wgrad_split = value; return prev; }   // no rebuild (the slabs are sized for both)
  else if (!strcmp(key, "attn_split")) { const int prev = plan->attn_split; plan->attn_split = value; return prev; }   // no rebuild
  else if (!strcmp(key, "store_wt")) {   // no rebuild (read at launch)
    if (value < 0 || value > STORE_WT_ALL) { set_error("store_wt %d: a mask of bits 0-2 (0 .. %d)", value, (int)STORE_WT_ALL); return SR3_E_BADARG; }
    const int prev = plan->store_wt; plan->store_wt = value; return prev;
  }
  else if (!strcmp(key, "gemm_epi")) {   // no rebuild (read at launch)
    if (value < 0 || value > 2) { set_error("gemm_epi %d: 0 (4-byte epilogue), 1 (16-byte stores) or 2 (16-byte stores written through L2)", value); return SR3_E_BADARG; }
    const int prev = plan->gemm_epi; plan->gemm_epi = value; plan->gemm_epi_named = true; return prev;
  }
  else if (!strcmp(key, "attn_long")) slot = &plan->attn_long;
  else if (!strcmp(key, "gemm_split")) slot = &plan->gemm_split;
  else if (!strcmp(key, "gemm_wpre")) slot = &plan->gemm_wpre;
  else if (!strcmp(key, "gemm2")) slot = &plan->gemm2;
  else if (!strcmp(key, "gemm_s2")) slot = &plan->gemm_s2;
  else if (!strcmp(key, "fork_side")) slot = &plan->fork_side;
  else if (!strcmp(key, "gemm_n64")) slot = &plan->gemm_n64;
  else if (!strcmp(key, "fold_fuse")) slot = &plan->fold_fuse;
  else if (!strcmp(key, "gemm_tile")) slot = &plan->gemm_tile;
  else if (!strcmp(key, "wino2")) slot = &plan->wino2;
  else if (!strcmp(key, "wino_ragged")) slot = &plan->wino_ragged;
  else if (!strcmp(key, "wino_up")) slot = &plan->wino_up;
  else if (!strcmp(key, "train_geom")) slot = &plan->train_geom;
  else if (!strcmp(key, "loss_l2")) { const int prev = plan->loss_l2; plan->loss_l2 = value; return prev; }   // no rebuild
  else if (!strcmp(key, "var_channels")) {
    if (value != 0 && value * 2 != plan->out_ch) {
      set_error("var_channels %d: 0 or half of out_channel %d (the variance head of a learned-variance model)", value, plan->out_ch);
      return SR3_E_BADARG;
    }
    slot = &plan->var_channels;
  }
  else if (!strcmp(key, "attn_heads") || !strcmp(key, "attn_head_dim")) {
    const bool dim = !strcmp(key, "attn_head_dim");
    if (dim ? value < 0 : value < 1) { set_error("%s %d: needs a value >= %d", key, value, dim ? 0 : 1); return SR3_E_BADARG; }
    if (dim ? (value > 0 && plan->attn_heads != 1) : (value != 1 && plan->attn_head_dim != 0)) {
      set_error("%s %d: attn_heads (%d) and attn_head_dim (%d) are mutually exclusive", key, value, plan->attn_heads, plan->attn_head_dim);
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
    slot = dim ? &plan->attn_head_dim : &plan->attn_heads;
  }
  if (!slot) { set_error("unknown option %s", key); return SR3_E_BADARG; }
#ifndef SR3_EXPERIMENTS
  if (slot == &plan->split_bf16 && value != 0) {
    set_error("option %s selects an experiment kernel that this library was built without (csrc/build.sh -DSR3_EXPERIMENTS)", key);
    return SR3_E_UNSUPPORTED;
  }
#endif
  const int prev = *slot;
  *slot = value;
  plan->built_batch = -1;
  plan->train_batch = -1;
  // which convs read transformed filters depends on these: a forward must not run on filters prepared for another choice
  if (slot == &plan->winograd || slot == &plan->tile_cfg || slot == &plan->split_bf16) plan->derived_from = nullptr;
  if ((slot == &plan->wino_split || slot == &plan->gemm_split || slot == &plan->gemm_wpre || slot == &plan->gemm2 || slot == &plan->gemm_s2 || slot == &plan->gemm_n64) && prev != value) layout_derived(plan);     // (the buffer has to be re-bound and re-prepared)
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
    if (plan->wino_split) {
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
  const int cond = plan->built_cond >= 0 ? plan->built_cond : 0;
  if (build_forward(plan, batch, cond)) return 0;
  return plan->ws_bytes;
}

static int unet_forward_rows(sr3_plan* plan, const float* x_nchw, const float* cond_nchw, int cond_channels,
                             const float* noise_level, const int64_t* timestep, const float* freq, const float* level_table,
                             const int* step_dev, const float* params, void* workspace, size_t workspace_bytes,
                             float* eps_out_nchw, int batch, void* stream, bool full_out, const int* t_map = nullptr) {
  if (!plan || !x_nchw || !params || !workspace || !eps_out_nchw || !freq) { set_error("null argument"); return SR3_E_BADARG; }
  if (!cond_nchw) cond_channels = 0;
  const int rc = build_forward(plan, batch, cond_channels);
  if (rc) return rc;
  if (workspace_bytes < plan->ws_bytes) { set_error("workspace too small: %zu < %zu", workspace_bytes, plan->ws_bytes); return SR3_E_NOMEM; }
  if (((uintptr_t)workspace & 255) || ((uintptr_t)params & 15) || ((uintptr_t)x_nchw & 15) || ((uintptr_t)eps_out_nchw & 15)) {
    set_error("misaligned pointer (workspace 256 B, tensors 16 B)");
    return SR3_E_ALIGN;
  }
  if (plan->d.variant == SR3_VARIANT_SR3 && !noise_level && !step_dev) { set_error("SR3 variant needs noise_level or step_dev"); return SR3_E_BADARG; }
  if (plan->d.variant == SR3_VARIANT_DDPM && !timestep && !step_dev) { set_error("DDPM variant needs timestep or step_dev"); return SR3_E_BADARG; }
  return run_forward(plan, false, x_nchw, cond_nchw, cond_channels, noise_level, timestep, freq, level_table,
                     step_dev, params, static_cast<char*>(workspace), eps_out_nchw, batch, static_cast<hipStream_t>(stream),
                     nullptr, nullptr, nullptr, nullptr, t_map, full_out);
}

int sr3_unet_forward(sr3_plan* plan, const float* x_nchw, const float* cond_nchw, int cond_channels,
                     const float* noise_level, const int64_t* timestep, const float* freq, const float* level_table,
                     const int* step_dev, const float* params, void* workspace, size_t workspace_bytes,
                     float* eps_out_nchw, int batch, void* stream) {
  return unet_forward_rows(plan, x_nchw, cond_nchw, cond_channels, noise_level, timestep, freq, level_table, step_dev, params, workspace,
                           workspace_bytes, eps_out_nchw, batch, stream, false);
}
// ... with the variance head: eps_out_nchw is [B, out_channel, H, W] (plan option var_channels; without it the same call as above)
int sr3_unet_forward_full(sr3_plan* plan, const float* x_nchw, const float* cond_nchw, int cond_channels,
                          const float* noise_level, const int64_t* timestep, const float* freq, const float* level_table,
                          const int* step_dev, const float* params, void* workspace, size_t workspace_bytes,
                          float* eps_out_nchw, int batch, void* stream, const int* t_map) {
  if (t_map && !step_dev) { set_error("sr3_unet_forward_full: t_map goes with step_dev"); return SR3_E_BADARG; }
  return unet_forward_rows(plan, x_nchw, cond_nchw, cond_channels, noise_level, timestep, freq, level_table, step_dev, params, workspace,
                           workspace_bytes, eps_out_nchw, batch, stream, true, t_map);
}

// One whole reverse step (include/sr3_mi355x.h): the forward above with the p_sample update and the counter decrement inside the
// output conv's kernel -- two graph nodes fewer per step than sr3_unet_forward + sr3_p_sample_step + sr3_step_decrement.
// _hist: the multistep tail (tab_c3 and the history buffer, both or neither); _ex forwards here with neither.
int sr3_reverse_step_hist(sr3_plan* plan, float* x_nchw, const float* cond_nchw, int cond_channels, const float* freq,
                          const float* level_table, int* step2_dev, const float* params, void* workspace, size_t workspace_bytes,
                          const float* z_nchw, const float* ta, const float* tb, const float* tc1, const float* tc2, const float* tsig,
                          int clip_denoised, float* eps_out_nchw, int batch, void* stream, const int* t_map, const float* tc3,
                          float* hist_nchw) {
  if (!plan || !x_nchw || !params || !workspace || !freq || !step2_dev || !ta || !tb || !tc1 || !tc2 || !tsig) { set_error("null argument"); return SR3_E_BADARG; }
  if (!cond_nchw) cond_channels = 0;
  const int rc = build_forward(plan, batch, cond_channels);
  if (rc) return rc;
  if (workspace_bytes < plan->ws_bytes) { set_error("workspace too small: %zu < %zu", workspace_bytes, plan->ws_bytes); return SR3_E_NOMEM; }
  if (((uintptr_t)workspace & 255) || ((uintptr_t)params & 15) || ((uintptr_t)x_nchw & 15) || ((uintptr_t)eps_out_nchw & 15) || ((uintptr_t)z_nchw & 15)) {
    set_error("misaligned pointer (workspace 256 B, tensors 16 B)");
    return SR3_E_ALIGN;
  }
  if (plan->d.variant == SR3_VARIANT_SR3 && !level_table) { set_error("SR3 variant needs level_table"); return SR3_E_BADARG; }
  const size_t image_bytes = (size_t)batch * (plan->d.out_channel - plan->var_channels) * plan_height(plan) * plan_width(plan) * sizeof(float);
  if (const int rc = check_step_history("reverse_step", tc3, hist_nchw, x_nchw, eps_out_nchw, image_bytes, true)) return rc;
  StepFuse f;
  f.x = x_nchw; f.z = z_nchw; f.tb = StepTables{ta, tb, tc1, tc2, tsig};
  f.step_cur = step2_dev; f.step_next = step2_dev + 1; f.clip = clip_denoised; f.c3 = tc3; f.hist = hist_nchw;
  // the embedding kernel reads t from slot 1 and copies it to slot 0; the tail reads slot 0 and writes t - 1 to slot 1: no kernel
  // both reads and writes a slot, so no launch of the step races with another block of itself
  return run_forward(plan, false, x_nchw, cond_nchw, cond_channels, nullptr, nullptr, freq, level_table,
                     step2_dev + 1, params, static_cast<char*>(workspace), eps_out_nchw, batch, static_cast<hipStream_t>(stream),
                     nullptr, nullptr, nullptr, &f, t_map);
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
  if (!plan || !op_ms || !op_kind || !op_flops || !n_ops) { set_error("null argument"); return SR3_E_BADARG; }
  if (!cond_nchw) cond_channels = 0;
  int rc = build_forward(plan, batch, cond_channels);
  if (rc) return rc;
  if (workspace_bytes < plan->ws_bytes) { set_error("workspace too small"); return SR3_E_NOMEM; }
  const int n = (int)plan->ops.size();
  std::vector<hipEvent_t> ev(n + 1, nullptr), mid(n, nullptr);
  for (auto* v : {&ev, &mid})
    for (auto& e : *v)
      if (hipError_t err = hipEventCreate(&e); err != hipSuccess && !rc) rc = hip_fail(err, "hipEventCreate");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (!rc)
    rc = run_forward(plan, false, x_nchw, cond_nchw, cond_channels, noise_level, timestep, freq, nullptr,
                     nullptr, params, static_cast<char*>(workspace), eps_out_nchw, batch, st, ev.data(), mid.data());
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
        fl = attn_flops(batch, o.attn.tokens, o.attn.channels);
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

}  // extern "C"
