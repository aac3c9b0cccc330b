// Per-op C entry points (include/sr3_mi355x.h): one kernel on caller-owned tensors, outside any plan -- reverse-step update, q_sample, the conv
// entries and their scratch / slice queries, GroupNorm, attention, embedding, the NCHW convs.  Plans and the sr3_plan_* entries: plan_abi.hip.
#include "plan_internal.h"
#include "tile_code.h"

namespace {

// The derived form of its filters a per-op conv call needs: made behind the split-K slabs in the caller's scratch (sr3_conv_scratch_bytes
// accounts for it; a plan keeps them in its derived buffer).
enum Derive { DERIVE_IGEMM_WSPLIT, DERIVE_WINO, DERIVE_WINO_SPLIT };
size_t derive_bytes(const ConvParams& c, Derive kind) {
  const int Cin = c.C0 + c.C1;
  return (kind == DERIVE_IGEMM_WSPLIT ? igemm_wsplit_floats(c.Cout, c.ksize * c.ksize, Cin) : wino_weight_floats(c.Cout, Cin, kind == DERIVE_WINO_SPLIT)) * sizeof(float);
}
// runs the transform of c.w into the scratch behind the slabs of this launch; *out is the result, *scratch_bytes shrinks to the slabs
int derive_behind_slabs(const ConvParams& c, int tile, int ksplit, Derive kind, void* scratch, size_t* scratch_bytes, hipStream_t st, float** out) {
  const size_t slab = conv_splitk_bytes(c, tile, ksplit);
  const size_t need = derive_bytes(c, kind);
  if (!scratch || *scratch_bytes < slab + need) {
    set_error("conv: %s (%zu < %zu)", kind == DERIVE_IGEMM_WSPLIT ? "scratch too small for the pre-split weights" : "Winograd scratch too small", *scratch_bytes, slab + need);
    return SR3_E_NOMEM;
  }
  *out = reinterpret_cast<float*>(static_cast<char*>(scratch) + slab);
  *scratch_bytes = slab;
  const int Cin = c.C0 + c.C1;
  return kind == DERIVE_IGEMM_WSPLIT ? igemm_split_weights(c.w, c.Cout, c.ksize * c.ksize, Cin, *out, st)
                                     : wino_transform_weights(c.w, c.Cout, Cin, *out, st, kind == DERIVE_WINO_SPLIT);
}

// the scratch of the per-op conv entries: split-K slabs with the derived filters behind them, laid out as a plan lays out its 256-byte
// aligned regions -- checked before anything is derived into it
int check_scratch_aligned(const void* scratch) {
  if ((uintptr_t)scratch & 255) { set_error("conv: scratch is not 256-byte aligned"); return SR3_E_ALIGN; }
  return SR3_OK;
}

}  // namespace

extern "C" {

int sr3_p_sample_step(float* x, const float* eps, const float* z, const float* ta, const float* tb, const float* tc1,
                      const float* tc2, const float* tsig, const int* step_dev, const int64_t* t_per_sample,
                      int step_host, int batch, int elems_per_image, void* stream) {
  if (!x || !eps || !ta || !tb || !tc1 || !tc2 || !tsig) { set_error("null argument"); return SR3_E_BADARG; }
  StepTables t{ta, tb, tc1, tc2, tsig};
  return p_sample_update(x, eps, z, t, step_dev, t_per_sample, step_host, batch, elems_per_image,
                         static_cast<hipStream_t>(stream));
}
int sr3_p_sample_step_ex(float* x, const float* eps, const float* z, const float* ta, const float* tb, const float* tc1,
                         const float* tc2, const float* tsig, const int* step_dev, const int64_t* t_per_sample,
                         int step_host, int batch, int elems_per_image, int clip_denoised, void* stream) {
  if (!x || !eps || !ta || !tb || !tc1 || !tc2 || !tsig) { set_error("null argument"); return SR3_E_BADARG; }
  StepTables t{ta, tb, tc1, tc2, tsig};
  return p_sample_update(x, eps, z, t, step_dev, t_per_sample, step_host, batch, elems_per_image,
                         static_cast<hipStream_t>(stream), clip_denoised != 0);
}
int sr3_p_sample_step_hist(float* x, const float* eps, const float* z, const float* ta, const float* tb, const float* tc1,
                           const float* tc2, const float* tsig, const int* step_dev, const int64_t* t_per_sample,
                           int step_host, int batch, int elems_per_image, int clip_denoised, const float* tc3, float* hist,
                           void* stream) {
  if (!x || !eps || !ta || !tb || !tc1 || !tc2 || !tsig) { set_error("null argument"); return SR3_E_BADARG; }
  if (batch <= 0 || elems_per_image <= 0) { set_error("p_sample_step_hist: sizes must be positive"); return SR3_E_BADARG; }
  StepTables t{ta, tb, tc1, tc2, tsig};
  return p_sample_update(x, eps, z, t, step_dev, t_per_sample, step_host, batch, elems_per_image,
                         static_cast<hipStream_t>(stream), clip_denoised != 0, tc3, hist);
}
int sr3_step_decrement(int* step_dev, void* stream) { return step_decrement(step_dev, static_cast<hipStream_t>(stream)); }
int sr3_q_sample(const float* x0, const float* z, const float* ca, const float* cb, int batch, int elems_per_image,
                 float* out, void* stream) {
  if (!x0 || !z || !ca || !cb || !out) { set_error("null argument"); return SR3_E_BADARG; }
  return q_sample(x0, z, ca, cb, batch, elems_per_image, out, static_cast<hipStream_t>(stream));
}

int sr3_conv_f32(const float* src0, int C0, const float* src1, int C1, int B, int Hs, int Ws, int ups, int stride,
                 int ksize, int Cout, const float* w, const float* bias, const float* ss, int act, const float* film,
                 int film_stride, const float* res0, int RC0, const float* res1, int RC1, float* out, double* out_stats,
                 int tile_cfg, int ksplit, void* scratch, size_t scratch_bytes, void* stream) {
  if (!src0 || !w || !out) { set_error("null argument"); return SR3_E_BADARG; }
  if (const int rc = check_scratch_aligned(scratch)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  ConvParams c = conv_shape(B, Hs, Ws, ups, stride, ksize, C0, src1 ? C1 : 0, Cout);
  c.src0 = src0; c.src1 = src1; c.w = w; c.bias = bias; c.ss = ss; c.act = act; c.film = film; c.film_stride = film_stride;
  c.res0 = res0; c.res1 = res1; c.RC0 = res0 ? RC0 : 0; c.RC1 = res1 ? RC1 : 0;
  c.out = out; c.ostat = out_stats;
  const TileCode t = tile_decode(tile_cfg);
  c.wino_split = t.wino_split; c.wino_full = t.wino_full; c.igemm_split = t.igemm_split; c.gemm_epi = t.gemm_epi; tile_cfg = t.tile;
  if (t.wpre) {
    // the weights pre-split into bf16 planes (what a plan does, in its derived buffer): derived here
    // (the rows fill the tile that runs: 32 or 64)
    if (tile_cfg == 22 && !gemm1x1_fits(c, gemm1x1_rows(c) / 32)) { set_error("conv: the 1x1 GEMM kernel (tile 22) does not fit this problem"); return SR3_E_UNSUPPORTED; }
    float* q = nullptr;
    if (const int rc = derive_behind_slabs(c, tile_cfg, ksplit, DERIVE_IGEMM_WSPLIT, scratch, &scratch_bytes, st, &q)) return rc;
    c.w_split = q;
  }
  if (tile_cfg == 11 && (ksize != 3 || stride != 1)) { set_error("conv: the Winograd kernel does not fit this problem (3x3 stride 1 only)"); return SR3_E_UNSUPPORTED; }
  if (tile_cfg == 11) {
    // Winograd form through the per-op entry: the transformed filters are derived here; a plan keeps them in its derived buffer instead
    const Derive kind = t.wino_split ? DERIVE_WINO_SPLIT : DERIVE_WINO;
#ifdef SR3_WINO_ABLATIONS
    const size_t total = scratch_bytes;
#endif
    float* u = nullptr;
    if (const int rc = derive_behind_slabs(c, tile_cfg, ksplit, kind, scratch, &scratch_bytes, st, &u)) return rc;
    c.wino_u = u;
#ifdef SR3_WINO_ABLATIONS
    // tooling build only: room behind the filters for the kernel's phase time stamps (SR3_WINO_DBG=64, tools/wino_phases.py)
    if (total >= scratch_bytes + derive_bytes(c, kind) + (1u << 20)) c.partial = reinterpret_cast<float*>(reinterpret_cast<char*>(u) + derive_bytes(c, kind));
#endif
  }
  return conv_forward(c, tile_cfg, ksplit, static_cast<float*>(scratch), scratch_bytes, st);
}
int sr3_block_conv_f32(const float* src0, int C0, const float* src1, int C1, int B, int H, int W, int Cout,
                       const float* w, const float* bias, const float* ss, int act, const float* film, int film_stride,
                       const float* x2_src0, int x2_C0, const float* x2_src1, int x2_C1, const float* x2_w,
                       const float* x2_bias, float* out, double* out_stats, int tile_cfg, int ksplit, void* scratch,
                       size_t scratch_bytes, void* stream) {
  if (!src0 || !w || !out || !x2_src0 || !x2_w) { set_error("null argument"); return SR3_E_BADARG; }
  if (const int rc = check_scratch_aligned(scratch)) return rc;
  ConvParams c = conv_shape(B, H, W, 0, 1, 3, C0, src1 ? C1 : 0, Cout);
  c.src0 = src0; c.src1 = src1; c.w = w; c.bias = bias; c.ss = ss; c.act = act; c.film = film; c.film_stride = film_stride;
  c.out = out; c.ostat = out_stats;
  c.x2_src0 = x2_src0; c.x2_src1 = x2_src1; c.x2_C0 = x2_C0; c.x2_C1 = x2_src1 ? x2_C1 : 0; c.x2_w = x2_w; c.x2_bias = x2_bias;
  return conv_forward(c, tile_cfg, ksplit, static_cast<float*>(scratch), scratch_bytes, static_cast<hipStream_t>(stream));   // (tile_cfg: the kernel tile itself, not decoded)
}
int sr3_conv_dropout_f32(const float* src0, int C0, int B, int H, int W, int Cout, const float* w, const float* bias,
                         const float* ss, int act, const float* film, int film_stride, const float* res0, int RC0,
                         const float* x2_src0, int x2_C0, const float* x2_src1, int x2_C1, const float* x2_w,
                         const float* x2_bias, float* out, double* out_stats, int tile_cfg, int ksplit, void* scratch,
                         size_t scratch_bytes, unsigned drop_seed, float drop_p, void* stream) {
  if (!src0 || !w || !out || !ss) { set_error("null argument"); return SR3_E_BADARG; }
  if (drop_p < 0.f || drop_p >= 1.f) { set_error("drop_p out of range"); return SR3_E_BADARG; }
  if (const int rc = check_scratch_aligned(scratch)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  ConvParams c = conv_shape(B, H, W, 0, 1, 3, C0, 0, Cout);
  c.src0 = src0; c.w = w; c.bias = bias; c.ss = ss; c.act = act; c.film = film; c.film_stride = film_stride;
  c.res0 = res0; c.RC0 = res0 ? RC0 : 0;
  c.out = out; c.ostat = out_stats;
  if (x2_src0) {
    if (!x2_w) { set_error("x2_src0 needs x2_w"); return SR3_E_BADARG; }
    c.x2_src0 = x2_src0; c.x2_src1 = x2_src1; c.x2_C0 = x2_C0; c.x2_C1 = x2_src1 ? x2_C1 : 0; c.x2_w = x2_w; c.x2_bias = x2_bias;
  }
  // same mapping p -> (threshold, scale) as sr3_train_step
  c.drop_seed = drop_seed;
  dropout_consts(drop_p, &c.drop_thresh, &c.drop_scale);
  TileCode t = tile_decode(tile_cfg);
  if (tile_cfg != 12) t = TileCode{tile_cfg, 0, 0, false};     // THIS ENTRY: of the composite numbers only 12 is decoded; 13-23 reach conv_forward as they are
  c.wino_split = t.wino_split; tile_cfg = t.tile;
  if (tile_cfg == 11) {       // Winograd form: the transformed filters are derived here (as sr3_conv_f32)
    if (c.x2_w) { set_error("conv: the Winograd kernel has no fused 1x1 segment"); return SR3_E_UNSUPPORTED; }
    float* u = nullptr;
    if (const int rc = derive_behind_slabs(c, tile_cfg, ksplit, t.wino_split ? DERIVE_WINO_SPLIT : DERIVE_WINO, scratch, &scratch_bytes, st, &u)) return rc;
    c.wino_u = u;
  }
  return conv_forward(c, tile_cfg, ksplit, static_cast<float*>(scratch), scratch_bytes, st);
}
unsigned sr3_dropout_threshold(float drop_p, float* scale_out) {
  unsigned t = 0;
  float s = 1.f;
  if (drop_p > 0.f && drop_p < 1.f) dropout_consts(drop_p, &t, &s);
  if (scale_out) *scale_out = s;
  return t;
}
int sr3_gemm_tile(int B, int Ho, int Wo, int Cin, int Cout, int ksize, int* rows, int* cols) {
  if (ksize != 1 && ksize != 3) return 0;
  const ConvParams c = ksize == 3 ? conv_shape(B, 2 * Ho, 2 * Wo, 0, 2, 3, Cin, 0, Cout) : conv_shape(B, Ho, Wo, 0, 1, 1, Cin, 0, Cout);
  if (B <= 0 || Ho <= 0 || Wo <= 0 || Cin <= 0 || Cout <= 0 || !gemm1x1_fits(c, gemm1x1_rows(c) / 32)) return 0;
  if (rows) *rows = gemm1x1_rows(c);
  if (cols) *cols = gemm1x1_cols(c);
  return 1;
}
size_t sr3_conv_scratch_bytes(int B, int Ho, int Wo, int Cin, int Cout, int ksize, int tile_cfg, int ksplit) {
  const TileCode t = tile_decode(tile_cfg);
  // the entry does not know the stride.  Winograd and the rest below: the stride-1 input dims
  ConvParams c = conv_shape(B, Ho, Wo, 0, 1, ksize, Cin, 0, Cout);
  c.igemm_split = t.igemm_split;
  if (t.tile == 11) {      // the geometry (hence the split) needs the input dims; + the derived filters
    c.wino_split = t.wino_split == 3 ? 3 : 0;      // THIS ENTRY: only the ragged tile grid is told to the automatic split; 12 and 13 are sized as tile 11
    return conv_splitk_bytes(c, 11, ksplit) + derive_bytes(c, t.wino_split ? DERIVE_WINO_SPLIT : DERIVE_WINO);
  }
  if (t.tile == 22) {      // the GEMM kernel: 1x1 stride 1, or 3x3 stride 2 (ksize 3); pre-split weights behind the slabs
    if (ksize == 3) { c = conv_shape(B, 2 * Ho, 2 * Wo, 0, 2, 3, Cin, 0, Cout); c.igemm_split = 1; }
    return conv_splitk_bytes(c, 22, ksplit) + derive_bytes(c, DERIVE_IGEMM_WSPLIT);
  }
  const size_t extra = t.wpre ? derive_bytes(c, DERIVE_IGEMM_WSPLIT) : 0;      // + the pre-split weights behind the slabs
  // THIS ENTRY: the larger of the stride-1 sizing (halo kernel eligible) and one with neither input dims nor stride (the im2col sizing)
  const size_t b = conv_splitk_bytes(c, t.tile, ksplit);
  c.Hs = c.Ws = c.stride = 0;
  const size_t a = conv_splitk_bytes(c, t.tile, ksplit);
  return (a > b ? a : b) + extra;
}
int sr3_groupnorm_stats_f32(const float* x, int B, int HW, int C, double* stat, void* stream) {
  if (!x || !stat) { set_error("null argument"); return SR3_E_BADARG; }
  return chan_stats(x, B, HW, C, stat, static_cast<hipStream_t>(stream));
}
int sr3_groupnorm_stats_slices(int B, int HW, int C) { return chan_stats_slices(B, HW, C); }
int sr3_conv_stats_slices(int B, int Hs, int Ws, int ups, int Cin, int Cout, int tile_cfg, int ksplit) {
  ConvParams c = conv_shape(B, Hs, Ws, ups, 1, 3, Cin, 0, Cout);
  const TileCode t = tile_decode(tile_cfg);
  c.wino_split = t.wino_split; c.igemm_split = t.igemm_split; tile_cfg = t.tile;
  if (tile_cfg == 22) c.igemm_split = 0;      // THIS ENTRY: the GEMM kernel's number leaves igemm_split clear
  const ConvPick pk = conv_pick(c, tile_cfg, ksplit);
  tile_cfg = pk.tile;
  if (pk.ksplit > 1) {
    const int rpb = splitk_rows_per_block(c, true);
    return rpb > 0 ? (c.Ho * c.Wo) / rpb : 0;
  }
  if (tile_cfg == 11) {
    WinoGeom wg;
    return wino_geometry(c, &wg) ? wino_stats_slices(wg) : 0;
  }
  HaloGeom g;
  if (tile_cfg < 5 || !halo_geometry(c, tile_cfg, &g)) return 0;
  return halo_stats_slices(g);
}
int sr3_groupnorm_fold_f32(const double* stat0, int C0, int T0, const double* stat1, int C1, int T1, int B, int HW,
                           int groups, const float* gamma, const float* beta, float eps, float* ss, void* stream) {
  if (!stat0 || !gamma || !beta || !ss) { set_error("null argument"); return SR3_E_BADARG; }
  return gn_finalize(stat0, C0, T0, stat1, stat1 ? C1 : 0, stat1 ? T1 : 0, B, HW, groups, gamma, beta, eps, ss,
                     static_cast<hipStream_t>(stream));
}
int sr3_groupnorm_fold_mr_f32(const double* stat0, int C0, int T0, const double* stat1, int C1, int T1, int B, int HW,
                              int groups, const float* gamma, const float* beta, float eps, float* ss, float* mr, void* stream) {
  if (!stat0 || !gamma || !beta || !ss || !mr) { set_error("null argument"); return SR3_E_BADARG; }
  return gn_finalize(stat0, C0, T0, stat1, stat1 ? C1 : 0, stat1 ? T1 : 0, B, HW, groups, gamma, beta, eps, ss,
                     static_cast<hipStream_t>(stream), mr);
}
// ... with the scale-shift modulation of the pairs (fold_modulate, small_kernels.hip); mr may be NULL.  Nothing is launched on a refusal
int sr3_groupnorm_fold_mod_f32(const double* stat0, int C0, int T0, const double* stat1, int C1, int T1, int B, int HW,
                               int groups, const float* gamma, const float* beta, float eps, float* ss, float* mr, const float* mod,
                               int mod_stride, void* stream) {
  const char* who = "sr3_groupnorm_fold_mod_f32";
  if (!stat0 || !gamma || !beta || !ss || !mod) { set_error("%s: stat0 / gamma / beta / ss / mod is NULL", who); return SR3_E_BADARG; }
  if (!stat1) C1 = T1 = 0;
  if (B <= 0 || HW <= 0 || C0 <= 0 || C1 < 0 || T0 <= 0 || (stat1 && T1 <= 0) || groups <= 0) {
    set_error("%s: batch %d, pixels %d, channels %d | %d, partials %d | %d and groups %d must be positive (C1 >= 0)", who, B, HW, C0, C1, T0, T1, groups);
    return SR3_E_BADARG;
  }
  const int C = C0 + C1;
  if ((C0 & 3) || (C1 & 3)) { set_error("%s: channel counts must be multiples of 4 (C0 %d, C1 %d)", who, C0, C1); return SR3_E_UNSUPPORTED; }
  if (C % groups) { set_error("%s: %d channels do not divide into %d groups", who, C, groups); return SR3_E_UNSUPPORTED; }
  if (mod_stride < 2 * C) { set_error("%s: mod_stride %d is below the 2 x %d values of an image", who, mod_stride, C); return SR3_E_BADARG; }
  return gn_finalize(stat0, C0, T0, stat1, C1, T1, B, HW, groups, gamma, beta, eps, ss, static_cast<hipStream_t>(stream), mr, mod, mod_stride);
}
int sr3_attention_f32(const float* qkv, int B, int N, int C, float* out, void* stream) {
  if (!qkv || !out) { set_error("null argument"); return SR3_E_BADARG; }
  return attention_forward(qkv, B, N, C, out, static_cast<hipStream_t>(stream));
}
int sr3_attention_ex_f32(const float* qkv, int B, int N, int C, float* out, int split, void* stream) {
  if (!qkv || !out) { set_error("null argument"); return SR3_E_BADARG; }
  return attention_forward(qkv, B, N, C, out, static_cast<hipStream_t>(stream), split);
}
int sr3_film_embed_f32(int variant, int B, int inner, const float* level, const int64_t* timestep, const float* freq,
                       const float* w1, const float* b1, const float* w2, const float* b2, const float* wf,
                       const float* bf, int F, float* temb_scratch, float* film_out, void* stream) {
  EmbedParams e;
  memset(&e, 0, sizeof(e));
  e.variant = variant; e.B = B; e.inner = inner; e.level = level; e.tstep = timestep; e.freq = freq;
  e.w1 = w1; e.b1 = b1; e.w2 = w2; e.b2 = b2; e.wf = wf; e.bf = bf; e.F = F; e.temb = temb_scratch; e.film = film_out;
  return embed_forward(e, static_cast<hipStream_t>(stream));
}
int sr3_conv_in_f32(const float* a, int Ca, const float* b, int Cb, int B, int H, int W, const float* w,
                    const float* bias, int Cout, float* out, void* stream) {
  return conv_in_nchw(a, Ca, b, b ? Cb : 0, B, H, W, w, bias, Cout, out, nullptr, static_cast<hipStream_t>(stream));
}
int sr3_conv_out_f32(const float* x, const float* ss, int B, int H, int W, int C, const float* w, const float* bias,
                     int Cout, float* out, void* stream) {
  return conv_out_nchw(x, ss, B, H, W, C, w, bias, Cout, out, static_cast<hipStream_t>(stream));
}

}  // extern "C"
