// Internal plan structures shared by plan_build.hip (planner), plan_run.hip (forward driver), plan_abi.hip (C ABI) and train_plan.hip
// (training step).
#pragma once
#include <map>
#include <string>
#include <vector>

#include "../../include/sr3_mi355x.h"
#include "sr3_common.h"

namespace sr3 {

// ---------------------------------------------------------------------------------------------
// plan data
// ---------------------------------------------------------------------------------------------
struct Tensor {
  size_t off = 0;       // byte offset in the workspace
  size_t bytes = 0;
  int C = 0, H = 0, W = 0;
  size_t stat_off = 0;  // byte offset of the partial statistics [B][T][C][2] doubles (valid once stats_done)
  int stat_T = 0;       // partials per image
  bool stats_done = false;
  bool valid = false;
  bool cached = false;  // plan option feat_cache: the branch tensor -- off and stat_off are CACHE_TAG offsets into the caller's feature cache
};

struct ResLayer {
  std::string name;     // e.g. "downs.1"
  int cin, cout, skip;  // cin includes skip
  bool attn;
  int film_off;         // channel offset among the res blocks: the sum of Cout of the blocks in front.  The block's first row of the FiLM
                        // table (2 * film_off under scale_shift, where a block has 2 * Cout rows) and its dropout key
  size_t gn1_w, gn1_b, c1_w, c1_b, gn2_w, gn2_b, c2_w, c2_b, rc_w, rc_b;
  bool has_rc;
  size_t an_w, an_b, qkv_w, ao_w, ao_b;
};

enum LayerKind { L_CONV_IN, L_RES, L_DOWN, L_UP };
struct Layer {
  LayerKind kind;
  std::string name;
  int cin, cout;
  size_t w, b;  // conv_in / down / up
  ResLayer res;
};

// an optional workspace / arena offset that is absent (plan_run.hip binds a null pointer for it)
static constexpr size_t NO_OFF = ~(size_t)0;
// plan option feat_cache: an activation / statistics offset with this bit set counts from the start of the caller-owned feature cache,
// not from the workspace (plan_run.hip resolves it; NO_OFF is tested first).  Without the option no offset of a launch list carries it
static constexpr size_t CACHE_TAG = (size_t)1 << 62;

// The kernel one conv of a plan runs on, as choose_conv (plan_build.hip) decided it
struct ConvChoice {
  int tile_cfg, ksplit;            // what conv_forward is called with
  int wino_split, igemm_split;     // the ConvParams fields of these names
  int wino_mode;                   // 0: the Winograd rule did not take the conv; 1 / 2: wino_mode (plan_build.hip)
  size_t wino_off;                 // tile_cfg 11: float offset of this conv's transformed filters in the derived buffer
  bool has_wsplit;                 // im2col SPLIT tile / tile 22: its weights pre-split into bf16 planes sit in the derived buffer ...
  size_t wsplit_off;               // ... at this float offset (ConvParams::w_split)
  int wino_full = 0;               // ConvParams::wino_full
};

// The NEXT op's GroupNorm fold done by an op's last kernel (plan option fold_fuse): a split-K conv's reduce, or the stand-alone
// statistics pass.  The host side of FoldTail (sr3_common.h): Builder::fuse_fold_into fills it, make_fold_tail binds it
struct FoldSpec {
  int Ctot = 0, c_off = 0;
  size_t ostat = NO_OFF;           // the other concat source's partials (bytes in the statistics region; NO_OFF: single source)
  int oC = 0, oT = 0, o_off = 0;
  size_t gamma = 0, beta = 0;      // float offsets into the parameter arena
  size_t ss_rel = 0, mr_rel = 0;   // the consumer's tables, as Op::ss_rel / mr_rel
  bool has_mr = false;
  int mod_row = -1;                // first row of the FiLM table that modulates the pairs (scale_shift; -1: none), as Op::Fold::mod_row
};

// numeric values are part of sr3_unet_forward_profile's op_kind encoding (kind * 10)
enum OpKind { OP_RESERVED, OP_EMBED, OP_CONV_IN, OP_STATS, OP_FOLD, OP_CONV, OP_ATTN, OP_CONV_OUT };

// One launch of a compiled forward: the payload of its kind, and what several kinds share.  Activations are byte offsets into the
// workspace, statistics partials byte offsets into its statistics region, parameters float offsets into the arena
struct Op {
  OpKind kind;
  struct ConvIn {
    int x_channels = 0, cond_channels = 0, Cout = 0, H = 0, W = 0;
    size_t w = 0, bias = 0, out = 0, ostat = NO_OFF;
  } conv_in;
  struct Stats { size_t src = 0, stat = 0; int pixels = 0, channels = 0; } stats;
  struct Fold {                      // the partials of the virtual concat (stat0|stat1) -> the consumer's tables at ss_rel / mr_rel
    size_t stat0 = 0, stat1 = NO_OFF;
    int C0 = 0, C1 = 0, T0 = 0, T1 = 0, pixels = 0;      // channels, partials per image of either source
    size_t gamma = 0, beta = 0;
    bool has_mr = false;
    int mod_row = -1;                // scale_shift: first row of the FiLM table that modulates the pairs -- the consumer's channel count of
                                     // scales, then as many shifts (-1: none)
  } fold;
  struct Conv {
    ConvParams cp = {};              // geometry (pointers filled at launch)
    ConvChoice ch = {};              // the kernel, as choose_conv returned it
    size_t src0 = 0, src1 = NO_OFF, res0 = NO_OFF, res1 = NO_OFF, out = 0, ostat = NO_OFF;
    size_t w = 0, bias = NO_OFF;
    int film_row = -1;               // first row of the FiLM table added to the output (-1: none)
    size_t x2_src0 = NO_OFF, x2_src1 = NO_OFF, x2_w = 0, x2_bias = 0;      // fused 1x1 segment (res_conv); x2_src0 == NO_OFF: none
    bool has_drop = false;
    unsigned drop_key = 0;
  } conv;
  struct Attn { size_t qkv = 0, out = 0; int tokens = 0, channels = 0, tile_cfg = 0, heads = 1; } attn;      // tile_cfg 24: the key-blocked kernel
  struct ConvOut { size_t src = 0, w = 0, bias = 0; int channels = 0, out_ch = 0, H = 0, W = 0; } conv_out;
  size_t ss_rel = 0, mr_rel = 0;   // GroupNorm tables: offset inside the scale/shift region (0 in inference)
  bool fold_fused = false;         // OP_CONV (split-K) / OP_STATS: the last kernel does the fold `tail` too
  FoldSpec tail;
  // plan option fork_side (inference plans): side_id >= 0 -- this op depends on nothing the ops between it and its consumer write, so it
  // is launched on the plan's side stream (forked from the caller's stream by an event, joined by event side_id); wait_id >= 0 -- the
  // caller's stream waits for join event wait_id before this op (the consumer).  Inside a stream capture the pair becomes a parallel
  // branch of the graph.
  int side_id = -1, wait_id = -1;
};

// Does this op read the FiLM table the embed op writes?  A conv that adds a row to its output; a GroupNorm fold a row modulates, as a
// launch of its own or as the tail of a split-K conv / a statistics pass.  THE rule the embed op's join is derived from (fork_side)
inline bool op_reads_film(const Op& o) {
  if (o.kind == OP_CONV && o.conv.film_row >= 0) return true;
  if (o.kind == OP_FOLD && o.fold.mod_row >= 0) return true;
  return (o.kind == OP_CONV || o.kind == OP_STATS) && o.fold_fused && o.tail.mod_row >= 0;
}

// every term is an integer far below 2^53: the sums over a launch list are exact in any order
inline double conv_flops(const ConvParams& c) {
  return 2.0 * c.B * c.Ho * c.Wo * (double)c.Cout * ((double)(c.C0 + c.C1) * c.ksize * c.ksize + (c.x2_C0 + c.x2_C1));
}
inline double attn_flops(int B, int tokens, int channels) { return 4.0 * B * (double)tokens * (double)tokens * channels; }

struct Tap { std::string name; size_t off; int C, H, W; };

// where the fixed regions of a compiled forward live inside the workspace: statistics partials, GroupNorm scale/shift tables, mean/rstd
// tables (training only), time embedding, FiLM table, split-K slabs
struct Regions {
  size_t stats_off = 0, ss_off = 0, mr_off = 0, temb_off = 0, film_off = 0, scratch_off = 0, scratch_bytes = 0;
};

// What one GroupNorm fold of the forward walk wrote (Builder::fold returns it): its tables, as Op::ss_rel / mr_rel, and its parameters
struct FoldOut { size_t ss_rel = 0, mr_rel = 0, gamma = 0, beta = 0; int mod_row = -1; };      // mod_row: as Op::Fold::mod_row

// One conv of the forward, for Builder::conv: sources and residuals are tensor handles (-1: absent), parameters arena offsets
struct ConvSpec {
  int x0 = -1, x1 = -1;            // source: the virtual concat (x0|x1)
  int Cout = 0, ksize = 3, stride = 1, ups = 0;
  int act = 0;                     // ConvParams::act: what the prologue does with the GroupNorm fold in front of this conv ...
  FoldOut gn;                      // ... and that fold (act == 0: none, the op's ss_rel is 0)
  size_t w = 0, bias = NO_OFF;
  int film_row = -1;               // first row of the FiLM table added to the output
  int r0 = -1, r1 = -1;            // residual: the concat view (r0|r1)
  bool want_stats = false;         // a GroupNorm reads the output: fuse its statistics where the kernel can
  bool to_cache = false;           // plan option feat_cache: the output is the branch tensor, bound to the feature cache
  int q0 = -1, q1 = -1; size_t qw = 0, qb = 0;       // fused 1x1 segment (res_conv) over (q0|q1); caller checked fuses_res_conv()
  int drop_key = -1;               // train-mode dropout on the activated input: the layer's key (drop_layer_seed)
};

// One data-gradient conv of the backward (dOut -> dA on the flipped-transposed filters) as build_train resolved it: dgrad_conv
// (train_plan.hip) launches exactly this
enum WuKind { WU_NONE, WU_WINO, WU_WINO_SPLIT, WU_GEMM };     // the derived filters it reads from the t_wu region: none, Winograd
                                                              // fp32 / 3 x bf16 split, the pre-split 1x1 weights of gemm1x1.hip
struct Dgrad {
  ConvParams c = {};               // shape, wino_split, igemm_split (pointers are bound at launch)
  int tile = 0, ksplit = 0;        // what conv_forward is called with: tile 11, 22 or 0 (conv_pick chooses)
  int wu = WU_NONE;
};

// one logical operation of the forward, recorded for the backward walk (train mode): what the forward walk emitted it from ...
enum RecKind { R_CONV_IN, R_CONV, R_ATTN, R_CONV_OUT };
struct Rec {
  int kind = R_CONV;
  ConvSpec s;                        // (R_CONV_IN / R_CONV_OUT: x0, w, bias, act alone)
  int out = -1;                      // tensor handle of the output
  size_t gamma = 0, beta = 0;        // GroupNorm of this conv's prologue: parameter arena offsets ...
  size_t ss_off = 0, mr_off = 0;     // ... and its persistent tables (bytes in the workspace)
  int qkv = -1, o = -1, heads = 1;   // attention
  // ... and its backward, resolved once by build_train (train_plan.hip): run_train only binds pointers and launches
  ConvParams dw = {}, dqw = {};      // shape of the weight gradient: the conv's own, the fused res_conv segment's
  Dgrad dx, dq;                      // data gradient: the conv's own (R_CONV, R_CONV_OUT), the fused segment's
  bool acc_x0 = true, acc_x1 = true, acc_r0 = true, acc_r1 = true, acc_q0 = true, acc_q1 = true;     // false: the first write of that
                                     // tensor's gradient in the backward walk, a plain store (the gradient mirror is not zeroed)
  size_t param_end = 0;              // largest end offset of this record's parameters in the arena (gradient-ready marks)
};

struct DropCfg { unsigned seed, thresh; float scale; };
inline unsigned drop_layer_seed(unsigned seed, unsigned key) { return seed + (key + 1u) * 0x632BE5ABu; }

}  // namespace sr3

using namespace sr3;

// Every plan option (sr3_plan_set_option), held as sr3_plan::opt.  PLAN_OPTIONS below says what setting each one does
struct PlanOptions {
  int var_channels = 0;      // learned reverse-process variance (plan option var_channels): the last var_channels of the out_ch filter rows
                             // are the variance head v, the first out_ch - var_channels the prediction.  0 or out_ch / 2.  Inference
                             // forwards and every step tail run the prediction rows alone (the filters are [co][9][C]: the first rows of
                             // the same buffer) unless the caller asks for all rows; the training forward always runs all of them
  int fuse_stats = 1, fuse_res = 1, tile_cfg = 0, ksplit = 0, keep_all = 0, split_bf16 = 0;
  int winograd = 1;          // 3x3 stride-1 convs of the inference plan on the Winograd F(2x2,3x3) kernel (conv3x3_wino.hip)
  int wino2 = 1;             // wino_split convs of the one-image tile without dropout on the two-workgroups-per-CU kernel (conv3x3_wino2.hip,
                             // 8 x 16 pixel tile; round 6).  0: the 8-wave kernel of conv3x3_wino.hip everywhere
  int wino_split = 1;        // ... on its 3 x bf16 split instantiation (bf16 MFMA, fp32-class results; gated by tests/: error not
                             // above the fp32-MFMA instantiation's on every layer shape, 2000-step drift) where that exists: the
                             // one-image tile of the inference plan.  0: the exact-fp32 MFMA instantiation everywhere
  int wino_split8 = 1;       // ... and the four-image tile of the 8x8 maps too (round 5; no dropout form: the training forward keeps fp32)
  int wgrad_split = 1;       // training: weight gradients of the layers with > 64 channels either side on the split kernel (wgrad.hip; round 5)
  int attn_split = 1;        // SelfAttention's two contractions on the 3 x bf16 split instantiation of k_attention_v2 (round 5)
  int attn_long = 0;         // inference plans: an attention level the score-strip kernels cannot hold (!attention_fits) runs on the key-blocked
                             // kernel of attention_long.hip (tile_cfg 24) instead of refusing the geometry; levels the strip kernels hold keep them.
                             // Off by default ONLY because a test pins the refusal text of a fresh plan; nothing else speaks against 1
  int attn_heads = 1;        // multi-head SelfAttention (attention_heads.hip): heads of every attention level ...
  int attn_head_dim = 0;     // ... or (0 = off) the width of a head, the count being the level's channels / attn_head_dim.  Mutually exclusive;
                             // sr3_plan_set_option refuses a value a level cannot take, so plan_attn_heads always divides
  int gemm_tile = 0;         // A/B knob: force this im2col tile (1-4) on every conv of that kernel; 0 = conv_pick's choice
  int gemm_split = 1;        // the im2col kernel (1x1 and stride-2 convs) on its 3 x bf16 split instantiations (conv_igemm.hip)
  int gemm_wpre = 0;         // 1: ... reading their weights pre-split AND in MFMA fragment order from the derived buffer, straight from global
                             // memory (round 6's form: no LDS staging of the weights; tiles 18-21 at the ABI).  Measured SLOWER in the forward
                             // again (1.50-1.52 vs 1.44-1.46 ms over the 33 launches, profiles/r06_gemm_wpre_fragment_major.txt: every wave
                             // fetches its own fragments, 3x the weight traffic of one staged copy per workgroup, and the A staging that
                             // bounds these launches is unchanged) -- off by default, an A/B knob.  0: weights split while staged (14-17)
  int fold_fuse = 1;         // the GroupNorm fold of a consumer done by the kernel that completes its (last) source where that is a split-K
                             // reduce or a stand-alone statistics pass (k_rows_fold; round 6): 32 of the 61 fold launches of the C2 forward
  int gemm2 = 1;             // 1x1 stride-1 convs (res_conv, the attention projections) on the plain GEMM kernel of gemm1x1.hip where it fits
                             // (Cout % 128 == 0, channels % 32 == 0, rows % 64 == 0): pre-split weights in fragment order read straight from
                             // global memory, A rows split once per 128 output channels, staging arithmetic hand-placed between the MFMAs
                             // (round 6; 27 of the 33 launches of the C2 forward: 1.09 -> 0.80 ms, profiles/r06_gemm1x1.txt).  0: the im2col kernel
  int gemm_s2 = 1;           // ... and Downsample's 3x3 stride-2 convs on that kernel's stride-2 form (needs gemm2; Cout % 128 == 0; last session of
                             // round 6: the three launches of the C2 forward 171 -> 118 us)
  int gemm_n64 = 1;          // ... and the layers with Cout % 128 != 0 (Cout % 64 == 0: the res_convs of the 128 x 128 level, Downsample 64 -> 64) on
                             // its 64-column tile (waves 2 x 2); 0: they keep the im2col kernel
  int wino_ragged = 1;       // inference plans at a geometry other than image_size x image_size: 3x3 stride-1 convs on maps that are not whole
                             // multiples of the 8 x 16 tile on the two-workgroup kernel's RAGGED instantiation (tile_cfg 23) where the measured rule
                             // (wino_ragged_wins, plan_build.hip) says so; 0: they fall back to the general kernels (A/B knob)
  int wino_up = 1;           // Upsample's conv (ups = 1) on the two-workgroup Winograd kernel: its UP instantiation, which skips the seven of the sixteen
                             // positions whose operand is exactly zero on a nearest x2 map (same bits); 0: all sixteen (tile_cfg 25 / 26; A/B knob)
  int store_wt = 3;          // STORE_WT_* bits (sr3_common.h), one per kernel family: its 16-byte epilogue stores are written through L2 (sc1), so the
                             // kernel boundary behind it has no dirty lines to write back.  Same bits under every value; read at launch, no rebuild;
                             // 0 = plain stores everywhere.  Default: the families that measured faster (profiles/store_wt_ab.txt)
  int gemm_epi = GEMM_EPI_DEFAULT;   // the epilogue of the GEMM kernel (tile 22; gemm1x1.hip): 0 = 4-byte stores, one per accumulator register; 1 = the
                             // accumulator blocks transposed through LDS, 16-byte loads and stores; 2 = ... written through L2 as store_wt's families
                             // are.  Same bits under every value; read at launch, no rebuild; the training forward and the data gradients on that
                             // kernel follow it.  Default: the fastest form that cleared the bar (profiles/gemm_epi_ab.txt)
  bool gemm_epi_named = false;       // sr3_plan_set_option set it: a named form refuses a problem its 16-byte accesses cannot take, the untouched default
                             // runs such a problem on form 0 (gemm1x1_forward); launch_gemm_epi() is what a launch passes on
  int launch_gemm_epi() const { return gemm_epi_named ? gemm_epi : -1; }      // (ConvParams::gemm_epi = 1 + this: 0 = the library's default)
  int train_geom = 0;        // training follows the plan's geometry (sr3_plan_set_geometry) too: sr3_train_workspace_bytes / sr3_train_step build the
                             // training plan at plan_height x plan_width.  0: training is refused at any geometry but image_size x image_size.
                             // Off by default ONLY because tests pin that refusal text; at the native geometry both values build the same plan
  int fork_side = 0;         // res_conv (and the embedding MLP) on a side stream beside block1's conv: see Op::side_id; A/B knob
  int loss_l2 = 0;           // training loss: 0 = L1 (sum), 1 = L2 (sum)  (set_loss, diffusion.py:84-90)
  int feat_cache = 0;        // inference plans: d in 1 .. res_blocks + 1 compiles a second, shallow launch list -- the embedding, the first d entries
                             // of downs, the last d res blocks of ups, the output conv -- whose first up block reads the tensor entering it
                             // (the branch tensor) and its GroupNorm partials from a caller-owned feature cache, which the full list writes
                             // (sr3_unet_forward_cached / sr3_reverse_step_cached).  0: off, one list, no cache.  Set by
                             // sr3_plan_set_feature_cache, an entry of its own: no row of PLAN_OPTIONS
};

// What setting an option does, beyond storing the value (sr3_plan_set_option, plan_abi.hip, applies exactly these)
enum OptionEffect {
  OPT_FORWARD = 1,         // the compiled forward is dropped (even when the value did not change)
  OPT_TRAIN = 2,           // ... and the training plan
  OPT_REBUILD = OPT_FORWARD | OPT_TRAIN,
  OPT_STALE = 4,           // which convs read transformed filters depends on it: a forward must not run on filters prepared for another choice
  OPT_RELAY = 8,           // the derived buffer's layout depends on it: laid out again when the value changed (re-bind and re-prepare)
  OPT_EXPERIMENT = 16,     // selects an experiment kernel: a value other than 0 needs a library built with -DSR3_EXPERIMENTS
};
// a key's own check of a value (null: every int is taken): SR3_OK, or the code with the error text set
typedef int (*OptionCheck)(const sr3_plan* plan, const char* key, int value);
int check_store_wt(const sr3_plan*, const char*, int);
int check_gemm_epi(const sr3_plan*, const char*, int);
int check_var_channels(const sr3_plan*, const char*, int);
int check_attn_heads(const sr3_plan*, const char*, int);      // attn_heads and attn_head_dim
struct OptionRow { const char* name; int PlanOptions::*slot; unsigned effects; OptionCheck check; };
// One row per key.  No effect flags: read at launch (store_wt, gemm_epi, attn_split) or where the training step is run (wgrad_split: the
// slabs are sized for both values; loss_l2), no rebuild
static const OptionRow PLAN_OPTIONS[] = {
  {"fuse_stats", &PlanOptions::fuse_stats, OPT_REBUILD, nullptr},
  {"tile_cfg", &PlanOptions::tile_cfg, OPT_REBUILD | OPT_STALE, nullptr},
  {"ksplit", &PlanOptions::ksplit, OPT_REBUILD, nullptr},
  {"keep_all", &PlanOptions::keep_all, OPT_REBUILD, nullptr},
  {"fuse_res", &PlanOptions::fuse_res, OPT_REBUILD, nullptr},
  {"split_bf16", &PlanOptions::split_bf16, OPT_REBUILD | OPT_STALE | OPT_EXPERIMENT, nullptr},
  {"winograd", &PlanOptions::winograd, OPT_REBUILD | OPT_STALE, nullptr},
  {"wino_split", &PlanOptions::wino_split, OPT_REBUILD | OPT_RELAY, nullptr},
  {"wino_split8", &PlanOptions::wino_split8, OPT_REBUILD, nullptr},
  {"wgrad_split", &PlanOptions::wgrad_split, 0, nullptr},
  {"attn_split", &PlanOptions::attn_split, 0, nullptr},
  {"store_wt", &PlanOptions::store_wt, 0, check_store_wt},
  {"gemm_epi", &PlanOptions::gemm_epi, 0, check_gemm_epi},
  {"attn_long", &PlanOptions::attn_long, OPT_REBUILD, nullptr},
  {"gemm_split", &PlanOptions::gemm_split, OPT_REBUILD | OPT_RELAY, nullptr},
  {"gemm_wpre", &PlanOptions::gemm_wpre, OPT_REBUILD | OPT_RELAY, nullptr},
  {"gemm2", &PlanOptions::gemm2, OPT_REBUILD | OPT_RELAY, nullptr},
  {"gemm_s2", &PlanOptions::gemm_s2, OPT_REBUILD | OPT_RELAY, nullptr},
  {"fork_side", &PlanOptions::fork_side, OPT_REBUILD, nullptr},
  {"gemm_n64", &PlanOptions::gemm_n64, OPT_REBUILD | OPT_RELAY, nullptr},
  {"fold_fuse", &PlanOptions::fold_fuse, OPT_REBUILD, nullptr},
  {"gemm_tile", &PlanOptions::gemm_tile, OPT_REBUILD, nullptr},
  {"wino2", &PlanOptions::wino2, OPT_REBUILD, nullptr},
  {"wino_ragged", &PlanOptions::wino_ragged, OPT_REBUILD, nullptr},
  {"wino_up", &PlanOptions::wino_up, OPT_REBUILD, nullptr},
  {"train_geom", &PlanOptions::train_geom, OPT_REBUILD, nullptr},
  {"loss_l2", &PlanOptions::loss_l2, 0, nullptr},
  {"var_channels", &PlanOptions::var_channels, OPT_REBUILD, check_var_channels},
  {"attn_heads", &PlanOptions::attn_heads, OPT_REBUILD, check_attn_heads},
  {"attn_head_dim", &PlanOptions::attn_head_dim, OPT_REBUILD, check_attn_heads},
};

struct sr3_plan {
  sr3_unet_desc d;
  std::vector<sr3_param_info> params;
  std::map<std::string, int> pindex;
  size_t param_floats = 0;
  int F = 0;                 // sum of Cout over the res blocks: what ResLayer::film_off and the dropout keys count in
  bool scale_shift = false;  // SR3_UNET_SCALE_SHIFT_NORM (sr3_plan_create_ex): a block's projection has 2 Cout rows, scales then shifts, which
                             // modulate its second GroupNorm -- GN2(h) (1 + scale) + shift -- in place of a row added to conv1's output
  int film_rows() const { return scale_shift ? 2 * F : F; }      // rows of the FiLM weight, bias, table and gradient table
  size_t film_w = 0, film_b = 0;
  size_t emb_w1 = 0, emb_b1 = 0, emb_w2 = 0, emb_b2 = 0;
  std::vector<Layer> downs, mid, ups;
  size_t fin_gn_w = 0, fin_gn_b = 0, fin_w = 0, fin_b = 0;
  int fin_cin = 0, out_ch = 0;
  PlanOptions opt;
  int geo_h = 0, geo_w = 0;  // sr3_plan_set_geometry: image height / width of the next forward (0: image_size)
  hipStream_t side_stream = nullptr;          // fork_side: created at the first forked forward, on the device current then
  std::vector<hipEvent_t> fork_ev, join_ev;   // one pair per forked op of the compiled forward
  ~sr3_plan() {
    for (hipEvent_t e : fork_ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : join_ev) (void)hipEventDestroy(e);
    if (side_stream) (void)hipStreamDestroy(side_stream);
  }
  // derived weights: U = G g G^T of every 3x3 stride-1 conv, fragment-major (caller-owned buffer, bound by pointer)
  struct Derived { size_t w; int Cout, Cin; size_t off; };
  std::vector<Derived> derived;
  std::map<size_t, size_t> derived_of;     // weight arena offset -> float offset in the derived buffer
  // ... and, plan option gemm_split, the 1x1 / stride-2 weights of the im2col SPLIT tiles as three bf16 planes (conv_igemm.hip)
  struct WSplit { size_t w; int Cout, taps, Cin; size_t off; };
  std::vector<WSplit> wsplits;
  std::map<size_t, size_t> wsplit_of;      // weight arena offset -> float offset in the derived buffer
  size_t derived_floats = 0;
  float* derived_ptr = nullptr;
  size_t derived_bound_bytes = 0;
  const float* derived_from = nullptr;   // the arena sr3_plan_prepare_derived last ran on (null: never / invalidated)
  // compiled forward
  int built_batch = -1;
  int built_cond = -1;
  int built_h = 0, built_w = 0;
  std::vector<Op> ops;
  std::vector<Tap> taps;
  size_t ws_bytes = 0;
  Regions regions;
  double flops = 0;
  // ---- plan option feat_cache: the shallow forward and the feature cache (built by build_forward behind the full list) ----
  std::vector<Op> sops;              // the shallow launch list
  Regions sregions;                  // ... and its regions inside the same workspace (ws_bytes covers both lists)
  sr3::Tensor branch;                // the branch tensor as the full list leaves it: CACHE_TAG offsets, partials per image
  size_t cache_bytes = 0;            // the feature cache: the branch tensor, then its statistics partials
  // what the last refresh filled (host bookkeeping; a cached forward is refused on anything else)
  const void* cache_filled = nullptr;
  int cache_batch = -1, cache_h = 0, cache_w = 0;
  // ---- training step (train_plan.hip) ----
  int train_batch = -1, train_cond = -1;
  int train_h = 0, train_w = 0;      // geometry the training plan was built for (with batch and cond_channels: its key; options reset train_batch)
  std::vector<Op> tops;              // forward ops in train mode (no buffer reuse, persistent GN tables)
  std::vector<sr3::Tensor> ttens;    // tensor table of the train forward
  std::vector<sr3::Rec> recs;
  size_t t_act_bytes = 0;            // activations; gradients mirror them at +t_act_bytes
  Regions t_regions;                 // ... of the train forward (its scratch region doubles as the backward's)
  size_t t_dA_off = 0, t_z_off = 0, t_dq_off = 0, t_wt_off = 0, t_slab_off = 0, t_part_off = 0, t_gs_off = 0;
  size_t t_dfilm_off = 0, t_xnoisy_off = 0, t_eps_off = 0, t_geps_off = 0, t_inpad_off = 0, t_dwtmp_off = 0;
  size_t t_ws_bytes = 0, t_embscr_off = 0, t_a_off = 0;
  size_t t_wu_off = 0, t_wu_bytes = 0;   // derived filters of the data-gradient conv being run (Dgrad::wu)
  std::vector<size_t> t_unproc_max;  // [ri]: max parameter end offset still unwritten before record ri-1 is processed
  int t_final_x = -1;                // tensor handle feeding the output Block
  size_t t_final_ss = 0, t_final_mr = 0;
  int t_conv_in_out = -1;
};


namespace sr3 {
struct Builder;
inline int plan_height(const sr3_plan* P) { return P->geo_h > 0 ? P->geo_h : P->d.image_size; }
inline int plan_width(const sr3_plan* P) { return P->geo_w > 0 ? P->geo_w : P->d.image_size; }
// heads of an attention level of `channels` channels (plan options attn_heads / attn_head_dim)
inline int plan_attn_heads(const sr3_plan* P, int channels) { return P->opt.attn_head_dim > 0 ? channels / P->opt.attn_head_dim : P->opt.attn_heads; }
inline int plan_image_channels(const sr3_plan* P) { return P->out_ch - P->opt.var_channels; }      // channels of x, z, eps of a step
// more than 4 output rows exist only as a prediction with its variance head: refused where a launch list is built
inline int check_out_rows(const sr3_plan* P) {
  if (P->out_ch > 4 && P->opt.var_channels == 0) { set_error("out_channel %d > 4 unsupported", P->out_ch); return SR3_E_UNSUPPORTED; }
  return SR3_OK;
}
inline bool plan_native_geometry(const sr3_plan* P) { return plan_height(P) == P->d.image_size && plan_width(P) == P->d.image_size; }
// One forward, as its caller asks for it: the inference entries (plan_abi.hip) and run_train fill it by name; fields named as TrainStep's
struct ForwardCall {
  // inputs.  SR3: level, or step_dev indexing level_table; DDPM: tstep, or step_dev (through t_map where given)
  const float* x = nullptr; const float* cond = nullptr; int cond_channels = 0;
  const float* level = nullptr; const int64_t* tstep = nullptr; const float* freq = nullptr;
  const float* level_table = nullptr; const int* step_dev = nullptr; const int* t_map = nullptr;
  // buffers
  const float* params = nullptr; void* workspace = nullptr; size_t workspace_bytes = 0;
  float* eps_out = nullptr; int batch = 0; hipStream_t stream = nullptr;
  // optional parts: per-op timing (n + 1 events around the ops, one per split-K op), train-mode dropout, the reverse step's tail inside
  // the output conv, all out_ch rows of the output conv in eps_out (the variance head too), the training plan's forward (P->tops)
  hipEvent_t* ev = nullptr; hipEvent_t* mid = nullptr; const DropCfg* drop = nullptr; const StepFuse* fuse = nullptr;
  bool full_out = false, train = false;
  // plan option feat_cache: the caller's feature cache; shallow: replay P->sops over P->sregions, reading it (else the full list writes it)
  void* cache = nullptr; bool shallow = false;
};
// replays P->ops over P->regions, or (f.train) P->tops over P->t_regions.  A plan whose derived buffer is missing or stale is refused
// before the first launch
int run_forward(sr3_plan* P, const ForwardCall& f);
// ... with a HIP event around every op, then sr3_unet_forward_profile's table (plan_run.hip)
int profile_forward(sr3_plan* plan, ForwardCall f, int max_ops, float* op_ms, int* op_kind, double* op_flops, int* n_ops);
int build_structure(sr3_plan* P);                              // plan_build.hip: topology and parameter table of a new plan
int build_forward(sr3_plan* P, int B, int cond_channels);      // plan_build.hip: the launch list (cached by batch, cond_channels, geometry)
// The forward walk in train mode (plan_build.hip): fills P->tops, P->ttens and P->recs (every activation kept, persistent GroupNorm
// tables) and returns what build_train lays the workspace out by
struct TrainWalk {
  size_t act_high = 0;                               // high-water mark of the activation arena
  size_t stats_bytes = 0, gn_bytes = 0, mr_bytes = 0;     // statistics partials, GroupNorm scale/shift tables, mean/rstd tables
  size_t max_scratch = 0;                            // largest split-K slab set of the forward
  std::string refused;                               // non-empty: the first layer no kernel can run at this geometry
};
TrainWalk walk_train(sr3_plan* P, int B, int cond_channels);
int build_train(sr3_plan* P, int B, int cond_channels);      // train_plan.hip
bool wino_ragged_wins(const ConvParams& c);
// Does a conv that lands on the im2col kernel run its 3 x bf16 split instantiation (plan option gemm_split)?  The 9-tap layers
// with Cout <= 64 (Downsample of the first level) stay on the fp32 MFMA, which is faster there (67 vs 81 us in the forward).  ONE
// rule for choose_conv (the forward) and choose_dgrad (the data gradients)
inline int igemm_split_rule(const sr3_plan* P, const ConvParams& c) { return (P->opt.gemm_split && !(c.ksize == 3 && c.Cout <= 64)) ? 1 : 0; }
void layout_derived(sr3_plan* P);
}  // namespace sr3
