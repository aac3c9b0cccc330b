// UNet plan, the planner: topology, parameter arena, activation plan and the launch list of a forward.
//
// Mirrors UNet.__init__ / UNet.forward of the reference (model/sr3_modules/unet.py:162-259,
// model/ddpm_modules/unet.py:148-243) as a static op list over the HIP kernels of this library.
// Nothing here is a translation of the reference modules: the forward is compiled once per batch
// size into a flat list of kernel launches over a liveness-planned NHWC workspace.  plan_run.hip replays the list,
// plan_abi.hip holds the sr3_plan_* entries.
#include <stdlib.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "plan_internal.h"
#include "tile_code.h"

namespace sr3 {

// ---- parameter table ---------------------------------------------------------------------------
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

int build_structure(sr3_plan* P) {
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
  const int fmul = P->scale_shift ? 2 : 1;      // rows per output channel of a block's projection
  P->film_w = cur; cur += (size_t)P->film_rows() * inner;
  cur = (cur + 3) & ~(size_t)3;
  P->film_b = cur; cur += (size_t)P->film_rows();
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
          pi.ndim = 2; pi.shape[0] = fmul * pr.cout; pi.shape[1] = inner; pi.pack = 0;
          pi.numel = (size_t)fmul * pr.cout * inner; pi.offset = P->film_w + (size_t)fmul * frow * inner;
          P->pindex[wn] = (int)P->params.size(); P->params.push_back(pi);
          memset(&pi, 0, sizeof(pi));
          snprintf(pi.name, sizeof(pi.name), "%s", bn.c_str());
          pi.ndim = 1; pi.shape[0] = fmul * pr.cout; pi.pack = 0; pi.numel = (size_t)fmul * pr.cout; pi.offset = P->film_b + fmul * frow;
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

// ---- activation plan (first-fit free list, byte offsets; sizes scale with batch) ---------------
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
  if (!P->opt.winograd || P->opt.tile_cfg != 0 || P->opt.split_bf16 || has_q) return 0;
  if (has_drop && (c.C1 != 0 || c.ups != 0 || c.act == 0)) return 0;    // the dropout form: single source, no upsampling
  if (c.ksize != 3 || c.stride != 1 || !P->derived_of.count(w)) return 0;
  if (wino_geometry(c, wg)) return 1;
  if ((train && !P->opt.train_geom) || has_drop || plan_native_geometry(P) || !P->opt.wino_split || !P->opt.wino2) return 0;
  ConvParams r = c;
  r.wino_split = wino2_fits(c) ? 2 : 3;
  if (r.wino_split == 3 && !(P->opt.wino_ragged && wino_ragged_wins(c))) return 0;
  return wino_geometry(r, wg) ? 2 : 0;
}

// The kernel one conv of a plan runs on (ConvChoice, plan_internal.h): THE place where the planner decides it (Builder::conv only emits what
// this returns).  RULE_HEAD stops behind the first conv_pick, with neither the split_bf16 tile nor igemm_split: what Builder::fuses_res_conv
// has always asked
enum ChoiceRule { RULE_FULL, RULE_HEAD };
static ConvChoice choose_conv(const sr3_plan* P, ConvParams c, size_t w, bool has_q, bool has_drop, bool train, ChoiceRule rule = RULE_FULL) {
  ConvChoice ch = {P->opt.tile_cfg, P->opt.ksplit, 0, 0, 0, 0, false, 0};
  const bool full = rule == RULE_FULL;
  auto repick = [&](int tile) { const ConvPick pk = conv_pick(c, tile, P->opt.ksplit); ch.tile_cfg = pk.tile; ch.ksplit = pk.ksplit; };
  // opt-in: the 3 x bf16 split MFMA instantiation of the 8-wave tile wherever it fits (inference plans only)
  HaloGeom sg; WinoGeom wg;
  if (full && P->opt.split_bf16 && !train && ch.tile_cfg == 0 && c.ksize == 3 && c.stride == 1 && c.Cout > 64 && halo_geometry(c, 10, &sg)) ch.tile_cfg = 10;
  ch.wino_mode = wino_mode(P, c, w, has_q, has_drop, train, &wg);
  if (ch.wino_mode) {
    ch.tile_cfg = 11;
    ch.wino_off = P->derived_of.at(w);
    // plan option wino_split: the 3 x bf16 split instantiation where it exists (the one-image tile; training plan and train-mode
    // dropout included); 2: the 8 x 16 tile of conv3x3_wino2.hip, 3: its ragged form.  Its filters sit behind the conv's fp32 ones
    if (ch.wino_mode == 2) c.wino_split = wino2_fits(c) ? 2 : 3;
    else if (P->opt.wino_split && (wg.NB == 1 || (P->opt.wino_split8 && !has_drop))) c.wino_split = (P->opt.wino2 && !has_drop && wg.NB == 1) ? 2 : 1;
    if (c.wino_split) ch.wino_off += wino_weight_floats(c.Cout, c.C0 + c.C1);
  }
  if (full) {
    c.igemm_split = igemm_split_rule(P, c);      // (read by conv_pick / conv_forward only when the conv lands on the im2col kernel)
    // (... unless the plain GEMM kernel takes the layer on its 64-column tile: plan options gemm2 + gemm_s2 + gemm_n64, below)
    if (P->opt.gemm_split && P->opt.gemm2 && P->opt.gemm_s2 && P->opt.gemm_n64 && c.ksize == 3 && c.stride == 2 && P->wsplit_of.count(w) && gemm1x1_fits(c, 2)) c.igemm_split = 1;
  }
  repick(ch.tile_cfg);
  ch.wino_split = c.wino_split;
  // plan option wino_up = 0 (A/B knob): Upsample's conv keeps all sixteen positions on the two-workgroup kernel (reported as tile 25 / 26)
  ch.wino_full = (ch.tile_cfg == 11 && c.wino_split >= 2 && c.ups == 1 && !P->opt.wino_up) ? 1 : 0;
  if (!full) return ch;
  const bool presplit = c.igemm_split && P->wsplit_of.count(w);      // (a SPLIT conv whose pre-split weights the derived buffer holds)
  if (P->opt.gemm_tile >= 1 && P->opt.gemm_tile <= 4 && ch.tile_cfg >= 1 && ch.tile_cfg <= 4 && P->opt.tile_cfg == 0) repick(P->opt.gemm_tile);       // A/B knob: one im2col tile for every conv of that kernel
  if (presplit && ch.tile_cfg >= 1 && ch.tile_cfg <= 4 && P->opt.gemm2 && P->opt.tile_cfg == 0 && P->opt.gemm_tile == 0) {
    // plan option gemm2: 1x1 stride-1 convs -- and Downsample's 3x3 stride-2 ones -- the plain GEMM kernel fits (gemm1x1.hip)
    if (gemm1x1_fits(c, 2) && (c.ksize == 1 || P->opt.gemm_s2) && (!(c.Cout & 127) || P->opt.gemm_n64)) { repick(22); ch.has_wsplit = true; }
  }
  if (presplit && ch.tile_cfg >= 1 && ch.tile_cfg <= 4 && P->opt.gemm_wpre) ch.has_wsplit = true;       // the SPLIT tile reads its weights pre-split from the derived buffer
  if (ch.has_wsplit) ch.wsplit_off = P->wsplit_of.at(w);
  if (has_drop && ch.tile_cfg == 9) repick(5);       // no dropout instantiation of the 8-wave tile
  // dropout convs on the 256x64 tile run its 8-wave form (conv3x3_halo_forward); SR3_DROP_CFG5 forces the
  // half-empty 128x128 tile instead (A/B knob)
  static const bool use5 = getenv("SR3_DROP_CFG5") != nullptr;
  if (has_drop && ch.tile_cfg == 6 && use5) repick(5);
  // opt-in: run the halo-tile convs on the 3 x bf16 split MFMA instantiations (inference plans only)
  if (P->opt.split_bf16 && !train && ch.tile_cfg == 5) ch.tile_cfg = 7;
  else if (P->opt.split_bf16 && !train && ch.tile_cfg == 9) ch.tile_cfg = 10;
  else if (P->opt.split_bf16 && !train && ch.tile_cfg == 6) ch.tile_cfg = 8;
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
  Builder(sr3_plan* p, int b, bool tr = false) : P(p), B(b), ops(tr ? p->tops : p->ops), train(tr) {}
  Builder(sr3_plan* p, int b, std::vector<Op>& list) : P(p), B(b), ops(list) {}      // (the shallow list of plan option feat_cache)
  size_t cache_cursor = 0;        // plan option feat_cache: bytes of the feature cache laid out so far (the branch tensor, its partials)

  // cached: the tensor lives in the caller's feature cache (CACHE_TAG offsets), outside the arena -- the one branch tensor of a list
  int make(int C, int H, int W, bool cached = false) {
    Tensor t;
    t.C = C; t.H = H; t.W = W;
    t.bytes = (size_t)B * H * W * C * sizeof(float);
    if (cached) {
      t.off = CACHE_TAG | cache_cursor;
      cache_cursor += (t.bytes + 255) & ~(size_t)255;
      t.cached = true;
    } else {
      t.off = act.alloc(t.bytes);
    }
    t.valid = true;
    T.push_back(t);
    return (int)T.size() - 1;
  }
  // the shallow list's branch source: the tensor the full list left in the cache, statistics partials included
  int adopt(const Tensor& t) {
    T.push_back(t);
    return (int)T.size() - 1;
  }
  void drop(int h) {
    if (h < 0 || !T[h].valid) return;
    if (train) return;                     // the backward needs every activation
    if (!P->opt.keep_all && !T[h].cached) act.release(T[h].off, T[h].bytes);
    T[h].valid = false;
  }
  void stat_slot(int h, int parts) {
    Tensor& t = T[h];
    t.stat_T = parts;
    const size_t bytes = (size_t)B * parts * t.C * 2 * sizeof(double);
    if (t.cached) { t.stat_off = CACHE_TAG | cache_cursor; cache_cursor += (bytes + 255) & ~(size_t)255; }      // kept with the tensor
    else { t.stat_off = stats_cursor; stats_cursor += bytes; }
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
  bool fuse_fold_into(Op& L, int fresh, int x0, int x1, size_t gamma, size_t beta, size_t ss_rel, size_t mr_rel, bool has_mr, int mod_row) {
    const int other = fresh == x0 ? x1 : x0;
    const int Cf = T[x0].C + (x1 >= 0 ? T[x1].C : 0);
    const int c_off = fresh == x0 ? 0 : T[x0].C;
    if (!fold_tail_fits(T[fresh].C, Cf, c_off, P->d.norm_groups)) return false;
    if (other >= 0 && !T[other].stats_done) return false;
    L.fold_fused = true;
    FoldSpec& f = L.tail;
    f.Ctot = Cf; f.c_off = c_off;
    if (other >= 0) { f.ostat = T[other].stat_off; f.oC = T[other].C; f.oT = T[other].stat_T; f.o_off = fresh == x0 ? T[x0].C : 0; }
    f.gamma = gamma; f.beta = beta; f.ss_rel = ss_rel; f.mr_rel = mr_rel; f.has_mr = has_mr; f.mod_row = mod_row;
    T[fresh].stat_T = 1;              // the fused kernel holds whole-image sums: one partial per image
    return true;
  }
  // the GroupNorm fold of the virtual concat (x0|x1), as a launch of its own or the tail of the op that completes its last source;
  // returns what the conv behind it reads (ConvSpec::gn).  mod_row: the rows of the FiLM table that modulate the pairs (Op::Fold::mod_row)
  FoldOut fold(int x0, int x1, size_t gamma, size_t beta, int mod_row = -1) {
    const int Cf = T[x0].C + (x1 >= 0 ? T[x1].C : 0);
    // the tables this fold writes, whichever kernel does it: per-GroupNorm slots in training, the one shared region (offset 0) in inference
    size_t ss_rel = 0, mr_rel = 0;
    if (train) {
      ss_rel = gn_cursor; gn_cursor += ((size_t)B * Cf * 2 * sizeof(float) + 255) & ~(size_t)255;
      mr_rel = mr_cursor; mr_cursor += ((size_t)B * P->d.norm_groups * 2 * sizeof(float) + 255) & ~(size_t)255;
    }
    const FoldOut done = {ss_rel, mr_rel, gamma, beta, mod_row};
    max_cin = std::max(max_cin, Cf);
    if (P->opt.fold_fuse && !ops.empty()) {
      // (a) the op just emitted is a split-K conv whose reduce writes the statistics of x0 / x1: its reduce folds too
      Op& L = ops.back();
      if (last_conv_op == (int)ops.size() - 1 && L.kind == OP_CONV && L.conv.ch.ksplit > 1 && L.conv.ostat != NO_OFF && (last_conv_out == x0 || last_conv_out == x1) &&
          fuse_fold_into(L, last_conv_out, x0, x1, gamma, beta, ss_rel, mr_rel, train, mod_row)) return done;
    }
    ensure_stats(x0);
    if (x1 >= 0) ensure_stats(x1);
    // (b) ... or a stand-alone statistics pass of x0 / x1: it folds too
    if (P->opt.fold_fuse && !ops.empty() && last_stats_op == (int)ops.size() - 1 && (last_stats_h == x0 || last_stats_h == x1) &&
        fuse_fold_into(ops.back(), last_stats_h, x0, x1, gamma, beta, ss_rel, mr_rel, train, mod_row)) return done;
    Op o; o.kind = OP_FOLD;
    Op::Fold& f = o.fold;
    f.stat0 = T[x0].stat_off; f.C0 = T[x0].C; f.T0 = T[x0].stat_T;
    if (x1 >= 0) { f.stat1 = T[x1].stat_off; f.C1 = T[x1].C; f.T1 = T[x1].stat_T; }
    f.pixels = T[x0].H * T[x0].W;
    f.gamma = gamma; f.beta = beta; f.has_mr = train; f.mod_row = mod_row;
    o.ss_rel = ss_rel; o.mr_rel = mr_rel;
    ops.push_back(o);
    return done;
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
    const int out = make(Cout, Ho, Wo, s.to_cache);
    c.act = s.act; c.film_stride = P->film_rows();
    c.RC0 = s.r0 >= 0 ? T[s.r0].C : 0; c.RC1 = s.r1 >= 0 ? T[s.r1].C : 0;
    v.src0 = T[x0].off; v.src1 = off(x1);
    v.w = s.w; v.bias = s.bias;
    v.film_row = s.film_row;
    v.res0 = off(s.r0); v.res1 = off(s.r1);
    v.out = T[out].off;
    o.ss_rel = s.gn.ss_rel;          // (act == 0: no fold in front, 0)
    v.has_drop = train && s.drop_key >= 0; v.drop_key = (unsigned)(s.drop_key >= 0 ? s.drop_key : 0);
    v.ch = choose_conv(P, c, s.w, has_q, v.has_drop, train);
    const ConvChoice& ch = v.ch;
    c.wino_split = ch.wino_split; c.wino_full = ch.wino_full; c.igemm_split = ch.igemm_split;
    if (train) {
      Rec r;
      r.kind = R_CONV; r.s = s; r.out = out;
      r.gamma = s.gn.gamma; r.beta = s.gn.beta; r.ss_off = s.gn.ss_rel; r.mr_off = s.gn.mr_rel;
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
    if (s.want_stats && P->opt.fuse_stats && ch.ksplit == 1 && ch.tile_cfg == 11) {
      WinoGeom wg = {};      // (stays empty -- no slices -- where plan option tile_cfg forces tile 11 on a conv it does not fit)
      wino_geometry(c, &wg);
      writes_stats(wino_stats_slices(wg));
    } else if (s.want_stats && P->opt.fuse_stats && ch.ksplit == 1 && ch.tile_cfg >= 5) {
      HaloGeom hg;
      if (halo_geometry(c, ch.tile_cfg, &hg)) writes_stats(halo_stats_slices(hg));
    } else if (s.want_stats && P->opt.fuse_stats && ch.ksplit > 1) {
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
    if (!P->opt.fuse_res) return false;
    ConvParams c = conv_shape(B, T[at].H, T[at].W, 0, 1, 3, R.cout, 0, R.cout);
    c.act = 2;
    const ConvChoice ch = choose_conv(P, c, R.c2_w, false, train, train, RULE_HEAD);
    return !ch.wino_mode && ch.tile_cfg >= 5 && ch.ksplit == 1;
  }
  std::string refused;     // inference: the first layer no kernel can run at this geometry (build_forward refuses the plan with it)
  int n_side = 0;          // plan option fork_side: ops handed to the side stream so far (Op::side_id)
  // to_cache (plan option feat_cache): the block's output -- block2's conv, or the attention's out projection -- is the branch tensor
  int res_block(int x0, int x1, const ResLayer& R, bool to_cache = false) {
    const FoldOut gn1 = fold(x0, x1, R.gn1_w, R.gn1_b);
    // plan option fork_side (inference): res_conv reads only the block input, so it is emitted HERE -- behind the fold, in front of block1's
    // conv -- and launched on the side stream; block2's conv, which adds it as its residual, waits for it.  Only unsplit: a split-K res_conv
    // would share the slab region with block1's conv.  (The fold stays where fold_fuse looks for it: behind the op that completes x.)
    const ConvSpec res_conv = {.x0 = x0, .x1 = x1, .Cout = R.cout, .ksize = 1, .w = R.rc_w, .bias = R.rc_b};
    int r_side = -1, r_id = -1;
    if (R.has_rc && P->opt.fork_side && !train && !fuses_res_conv(x0, R)) {
      r_side = conv(res_conv);
      if (ops.back().kind == OP_CONV && ops.back().conv.ch.ksplit == 1) { r_id = n_side++; ops.back().side_id = r_id; }
    }
    // the block's rows of the FiLM table: added to conv1's output, or (scale_shift: 2 Cout rows at 2 * film_off) modulating GN2's fold
    const bool ssn = P->scale_shift;
    const int h1 = conv({.x0 = x0, .x1 = x1, .Cout = R.cout, .act = 2, .gn = gn1, .w = R.c1_w, .bias = R.c1_b, .film_row = ssn ? -1 : R.film_off, .want_stats = true});
    const FoldOut gn2 = fold(h1, -1, R.gn2_w, R.gn2_b, ssn ? 2 * R.film_off : -1);
    // block2's conv; what it adds: res_conv's output (its own launch), res_conv as a fused K-segment over the block input, or the input itself
    ConvSpec block2 = {.x0 = h1, .Cout = R.cout, .act = 2, .gn = gn2, .w = R.c2_w, .bias = R.c2_b, .want_stats = true, .to_cache = to_cache && !R.attn,
                        .drop_key = R.film_off};
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
      const FoldOut gna = fold(out, -1, R.an_w, R.an_b);
      const int qkv = conv({.x0 = out, .Cout = 3 * R.cout, .ksize = 1, .act = 1, .gn = gna, .w = R.qkv_w});
      const int o = make(R.cout, T[out].H, T[out].W);
      Op a; a.kind = OP_ATTN;
      const int tokens = T[out].H * T[out].W;
      a.attn = {T[qkv].off, T[o].off, tokens, R.cout, 0, plan_attn_heads(P, R.cout)};
      const bool geo = !train || P->opt.train_geom;       // (a training plan off the native geometry exists under train_geom only)
      if (geo && P->opt.attn_long && !attention_fits(tokens, R.cout)) a.attn.tile_cfg = 24;       // the key-blocked kernel: any token count
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
      const int out2 = conv({.x0 = o, .Cout = R.cout, .ksize = 1, .w = R.ao_w, .bias = R.ao_b, .r0 = out, .want_stats = true,
                             .to_cache = to_cache});
      drop(o);
      drop(out);
      out = out2;
    }
    return out;
  }
};

// the UNet.forward walk (downs -> mid -> ups -> final), emitting ops through the builder.  Plan option feat_cache = d (inference): the full
// walk binds the tensor that enters the d-th last up block -- the branch tensor -- and its statistics partials to the feature cache;
// shallow = d walks the shallow forward instead: the first d entries of downs, then the last d up blocks from the cached branch tensor
static void walk_forward(sr3_plan* P, Builder& bld, int cond_channels, int shallow = 0) {
  const sr3_unet_desc& d = P->d;
  std::vector<Op>& ops = bld.ops;
  const int B = bld.B;
  const int inner = d.inner_channel;
  const bool geo = !bld.train || P->opt.train_geom;      // (training: native geometry only, unless plan option train_geom)
  const int IH = geo ? plan_height(P) : d.image_size, IW = geo ? plan_width(P) : d.image_size;

  { Op o; o.kind = OP_EMBED; ops.push_back(o); }
  bld.flops += 2.0 * B * (2.0 * 4 * inner * inner + (double)P->film_rows() * inner);

  // (taps are the full list's workspace offsets: the branch tensor, which lives in the cache, has none)
  auto tap = [&](const std::string& name, int h) {
    if (!bld.train && !shallow && !bld.T[h].cached) P->taps.push_back({name, bld.T[h].off, bld.T[h].C, bld.T[h].H, bld.T[h].W});
  };
  const int cache_d = bld.train ? 0 : (shallow ? shallow : P->opt.feat_cache);
  const int first_up = (int)P->ups.size() - cache_d;      // the first up block of the shallow forward (check_feat_cache: never negative)
  int n_down = 0, branch = -1;
  std::vector<int> feats;
  int cur = -1;
  for (auto& L : P->downs) {
    if (shallow && n_down++ == shallow) break;
    if (L.kind == L_CONV_IN) {
      cur = bld.make(L.cout, IH, IW);
      Op o; o.kind = OP_CONV_IN;
      Op::ConvIn& v = o.conv_in;
      v.x_channels = d.in_channel - cond_channels; v.cond_channels = cond_channels; v.Cout = L.cout; v.H = IH; v.W = IW;
      v.w = L.w; v.bias = L.b; v.out = bld.T[cur].off;
      if (const int slices = P->opt.fuse_stats ? conv_in_stat_slices(d.in_channel, IH, IW, L.cout) : 0) {
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
    if (shallow) break;
    const int nxt = bld.res_block(cur, -1, L.res, cache_d && first_up == 0 && &L == &P->mid.back());
    if (!cur_is_skip) bld.drop(cur);
    cur = nxt;
    cur_is_skip = false;
    tap(L.name, cur);
  }
  int n_up = 0;
  for (auto& L : P->ups) {
    const int i = n_up++;
    if (shallow && i < first_up) continue;
    if (cache_d && i == first_up) {
      if (shallow) cur = bld.adopt(P->branch);
      branch = cur;
    }
    const bool to_cache = cache_d && !shallow && i + 1 == first_up;      // this entry's output enters the first shallow up block
    int nxt;
    if (L.kind == L_RES) {
      const int skip = feats.back();
      feats.pop_back();
      nxt = bld.res_block(cur, skip, L.res, to_cache);
      bld.drop(cur);
      bld.drop(skip);
    } else {
      nxt = bld.conv({.x0 = cur, .Cout = L.cout, .ups = 1, .w = L.w, .bias = L.b, .want_stats = true, .to_cache = to_cache});
      bld.drop(cur);
    }
    cur = nxt;
    tap(L.name, cur);
  }
  if (cache_d && !shallow) P->branch = bld.T[branch];      // (its partials are laid out by now: the first shallow up block's fold read them)
  const FoldOut gnf = bld.fold(cur, -1, P->fin_gn_w, P->fin_gn_b);
  {
    Op o; o.kind = OP_CONV_OUT;
    o.conv_out = {bld.T[cur].off, P->fin_w, P->fin_b, bld.T[cur].C, P->out_ch, IH, IW};
    o.ss_rel = gnf.ss_rel;
    ops.push_back(o);
    if (bld.train) {
      Rec r; r.kind = R_CONV_OUT; r.s.x0 = cur; r.s.w = P->fin_w; r.s.bias = P->fin_b; r.s.act = 2; r.s.gn = gnf;
      r.gamma = gnf.gamma; r.beta = gnf.beta; r.ss_off = gnf.ss_rel; r.mr_off = gnf.mr_rel;
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
    dcur += wino_weight_floats(Cout, Cin) + (P->opt.wino_split ? wino_weight_floats(Cout, Cin, true) : 0);
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
  if (P->opt.gemm_split && (P->opt.gemm_wpre || P->opt.gemm2)) {
    auto regw = [&](size_t w, int Cout, int taps, int Cin) {
      if (Cin & 3) return;
      if (!P->opt.gemm_wpre && ((taps != 1 && !(taps == 9 && P->opt.gemm_s2)) || (Cout & (P->opt.gemm_n64 ? 63 : 127)) || (Cin & 31))) return;     // gemm2 alone: only what gemm1x1.hip can take (1x1; Downsample's 3x3 stride 2)
      P->wsplits.push_back({w, Cout, taps, Cin, dcur});
      P->wsplit_of[w] = dcur;
      dcur += igemm_wsplit_floats(Cout, taps, Cin);
    };
    for (auto* v : {&P->downs, &P->mid, &P->ups})
      for (auto& L : *v) {
        if (L.kind == L_RES) {
          if (L.res.has_rc) regw(L.res.rc_w, L.res.cout, 1, L.res.cin);
          if (L.res.attn) { regw(L.res.qkv_w, 3 * L.res.cout, 1, L.res.cout); regw(L.res.ao_w, L.res.cout, 1, L.res.cout); }
        } else if (L.kind == L_DOWN && (L.cout > 64 || (P->opt.gemm2 && P->opt.gemm_s2 && P->opt.gemm_n64 && L.cout == 64))) {
          regw(L.w, L.cout, 9, L.cin);
        }
      }
  }
  P->derived_floats = dcur;
  P->derived_from = nullptr;
  if (P->derived_bound_bytes < dcur * sizeof(float)) { P->derived_ptr = nullptr; P->derived_bound_bytes = 0; }   // re-bind a larger one
}

int build_forward(sr3_plan* P, int B, int cond_channels) {
  if (const int rc = check_out_rows(P)) return rc;
  if (P->built_batch == B && P->built_cond == cond_channels && P->built_h == plan_height(P) && P->built_w == plan_width(P)) return SR3_OK;
  const sr3_unet_desc& d = P->d;
  if (B <= 0) { set_error("batch must be > 0"); return SR3_E_BADARG; }
  if (cond_channels < 0 || cond_channels >= d.in_channel) { set_error("cond_channels %d out of range (in_channel %d)", cond_channels, d.in_channel); return SR3_E_BADARG; }
  P->ops.clear();
  P->sops.clear();
  P->taps.clear();
  P->cache_bytes = 0;
  P->built_batch = -1;
  const int inner = d.inner_channel;
  // one launch list -- the full forward, or (plan option feat_cache) the shallow one -- and its regions; returns the workspace it needs
  auto compile = [&](Builder& bld, std::vector<Op>& ops, Regions& R, int shallow, size_t* ws_bytes) {
    walk_forward(P, bld, cond_channels, shallow);
    if (!bld.refused.empty()) {
      // a geometry no kernel can run is refused HERE, when the launch list is built: never after a launch has been enqueued
      set_error("geometry %d x %d unsupported: %s", plan_height(P), plan_width(P), bld.refused.c_str());
      P->ops.clear();
      P->sops.clear();
      P->taps.clear();
      return SR3_E_UNSUPPORTED;
    }
    if (P->opt.fork_side && !ops.empty() && ops[0].kind == OP_EMBED) {
      // ... and the embedding MLP + FiLM projections (first op, reads only the noise level): beside the input conv, joined by the first op that
      // reads the FiLM table (op_reads_film: a conv that adds a row, or a fold -- fused or its own launch -- that a row modulates)
      for (Op& o : ops)
        if (op_reads_film(o)) {
          if (o.wait_id < 0) { o.wait_id = bld.n_side; ops[0].side_id = bld.n_side++; }
          break;
        }
    }
    // ---- fixed regions after the activation arena (high-water mark) ----
    size_t off = (bld.act.high + 255) & ~(size_t)255;
    // (no mean / rstd tables in inference: mr_off stays 0, no op has_mr)
    R.stats_off = off; off += (bld.stats_cursor + 255) & ~(size_t)255;
    R.ss_off = off; off += ((size_t)B * std::max(bld.max_cin, 4) * 2 * sizeof(float) + 255) & ~(size_t)255;
    R.temb_off = off; off += ((size_t)B * inner * sizeof(float) + 255) & ~(size_t)255;
    R.film_off = off; off += ((size_t)B * P->film_rows() * sizeof(float) + 255) & ~(size_t)255;
    R.scratch_off = off; R.scratch_bytes = bld.max_scratch; off += (bld.max_scratch + 255) & ~(size_t)255;
    *ws_bytes = off;
    return (int)SR3_OK;
  };
  Builder bld(P, B);
  if (const int rc = compile(bld, P->ops, P->regions, 0, &P->ws_bytes)) return rc;
  if (P->opt.feat_cache) {
    // the shallow list: its own arena and regions inside the same workspace (sized for the larger list); nothing of the cache lives there
    P->cache_bytes = bld.cache_cursor;
    Builder sb(P, B, P->sops);
    size_t shallow_bytes = 0;
    if (const int rc = compile(sb, P->sops, P->sregions, P->opt.feat_cache, &shallow_bytes)) return rc;
    P->ws_bytes = std::max(P->ws_bytes, shallow_bytes);
  }
  P->flops = bld.flops;
  P->built_batch = B;
  P->built_cond = cond_channels;
  P->built_h = plan_height(P); P->built_w = plan_width(P);
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
