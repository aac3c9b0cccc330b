/* libsr3_mi355x.so -- C ABI of the MI355X-native SR3 / DDPM iterative-refinement engine.
 *
 * The reference (Janspiry/Image-Super-Resolution-via-Iterative-Refinement) is pure PyTorch and has
 * no FFI of its own; the drop-in boundary is its Python surface (model.networks.define_G,
 * GaussianDiffusion, DDPM -- see INTEGRATION.md).  This header is the C layer underneath that
 * surface: plain pointers and sizes only, no torch types.  Each entry cites the reference code it
 * replaces (paths relative to the reference root).
 *
 * Conventions
 *  - every pointer named *_dev / every `const float*` tensor argument is a DEVICE pointer
 *    (tensor.data_ptr()); `stream` is a hipStream_t passed as void* (0 = default stream);
 *  - all calls are asynchronous on `stream`, never synchronise, never allocate or free device
 *    memory (workspaces are sized by a query and passed in), and are hipGraph-capturable;
 *  - return value: 0 ok, >0 a hipError_t, <0 an engine error (SR3_E_*); sr3_last_error() returns a
 *    thread-local message; no C++ exception crosses the ABI;
 *  - public tensors (x, cond, eps, z) are NCHW fp32 as in the reference; internal activations are
 *    NHWC fp32 inside the workspace.
 */
#ifndef SR3_MI355X_H
#define SR3_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SR3_ABI_VERSION 1

#define SR3_E_BADARG (-1)
#define SR3_E_UNSUPPORTED (-2)
#define SR3_E_ALIGN (-3)
#define SR3_E_NOMEM (-4)
#define SR3_E_STATE (-5)

#define SR3_VARIANT_SR3 0  /* model/sr3_modules: continuous noise-level conditioning */
#define SR3_VARIANT_DDPM 1 /* model/ddpm_modules: integer-timestep conditioning      */

/* Mirrors the arguments of UNet.__init__ (model/sr3_modules/unet.py:162-173,
 * model/ddpm_modules/unet.py:148-159) as filled by define_G (model/networks.py:91-101). */
typedef struct sr3_unet_desc {
  int variant;
  int in_channel, out_channel, inner_channel, norm_groups;
  int n_mults;
  int channel_mults[8];
  int n_attn_res;
  int attn_res[8];
  int res_blocks;
  int image_size;
} sr3_unet_desc;

/* One entry of the parameter table: where a reference state_dict tensor lives in the packed
 * parameter arena.  pack: 0 = copied as is (row-major), 1 = conv weight OIHW -> OHWI. */
typedef struct sr3_param_info {
  char name[128]; /* reference key without the "denoise_fn." prefix, e.g. downs.1.res_block.block1.block.3.weight */
  int ndim;
  int shape[4];   /* reference shape (OIHW for convs) */
  int pack;
  size_t offset;  /* float offset inside the arena */
  size_t numel;
} sr3_param_info;

typedef struct sr3_plan sr3_plan;

int sr3_version(void);
const char* sr3_last_error(void);
/* Device self-test of the 3 x bf16 operand split every SPLIT kernel rests on (x == h + m + l exactly, 2^21 fp32 patterns):
 * scratch_dev = one int of device memory, *mismatches (host) = offending elements; SR3_E_UNSUPPORTED when it is not 0.
 * (No reference counterpart: the reference computes in IEEE fp32; this guards the claim that the split path is fp32-class.) */
int sr3_selftest_split3(int* scratch_dev, int* mismatches, void* stream);

/* UNet construction (model/sr3_modules/unet.py:162-233): builds the layer list, the parameter
 * table and the activation plan.  No device work. */
int sr3_plan_create(const sr3_unet_desc* desc, sr3_plan** out);
/* ... with architecture flags (sr3_plan_create is flags 0).  An unknown bit: SR3_E_BADARG, the bits named.
 * SR3_UNET_SCALE_SHIFT_NORM (config key model.unet.scale_shift_norm; ADM's use_scale_shift_norm): a res block's projection of the
 * time / noise embedding has 2 Cout rows -- its keys keep their names, their shapes become [2 Cout, inner] and [2 Cout] -- read as
 * (scale, shift) = (rows [0, Cout), rows [Cout, 2 Cout)), and the block computes
 *   h = conv1(silu(GN1(x)))  (no row is added);  out = conv2(dropout(silu(GN2(h) (1 + scale) + shift))) + res(x)
 * in place of h = conv1(...) + row.  Every entry that takes the plan follows. */
#define SR3_UNET_SCALE_SHIFT_NORM 1u
#define SR3_UNET_FLAGS_ALL 1u
int sr3_plan_create_ex(const sr3_unet_desc* desc, unsigned flags, sr3_plan** out);
void sr3_plan_destroy(sr3_plan* plan);
int sr3_plan_num_params(const sr3_plan* plan);
int sr3_plan_param_info(const sr3_plan* plan, int index, sr3_param_info* out);
size_t sr3_plan_param_floats(const sr3_plan* plan);
/* ordered list of kernels one forward launches, for inspection / DESIGN.md: returns count */
int sr3_plan_num_ops(sr3_plan* plan, int batch);
/* one entry of that list: kind as in sr3_unet_forward_profile's op_kind / 10 * 10 (10 embed, 20 input conv, 30
 * statistics, 40 GroupNorm fold, 50 convolution, 60 attention, 70 output block); for convolutions the tile
 * configuration the plan picked (1-4 im2col kernel, 5-10 halo-tile kernel, see sr3_conv_f32), the split-K factor, the
 * geometry and what is fused into the launch.  Host-only (no device work): lets tools and tests inspect the plan. */
typedef struct sr3_op_info {
  int kind, tile_cfg, ksplit;
  int ksize, stride, upsample;
  int cin, cout, h_out, w_out;          /* attention: cin = cout = channels, h_out = tokens; tile_cfg 24 = the key-blocked kernel, 0 = the strip kernels */
  int fused_res_conv_cin;               /* > 0: the 1x1 res_conv of that many input channels runs inside this launch */
  int fused_output_stats;               /* 1: the launch also writes the next GroupNorm's partial statistics */
  double flops;
} sr3_op_info;
int sr3_plan_op_info(sr3_plan* plan, int batch, int index, sr3_op_info* out);
/* plan option fork_side: *side_id >= 0 -- op `index` is launched on the plan's side stream, forked from the caller's stream by an event
 * where the op sits in the list; *wait_id >= 0 -- the caller's stream waits for the side op of that id before this op (its consumer).
 * Both -1 for every op of a plan without the option.  Host-only. */
int sr3_plan_op_side(sr3_plan* plan, int batch, int index, int* side_id, int* wait_id);
/* The GroupNorm fold op `index` does: *fold 0 none, 1 the op is a fold launch (kind 40), 2 the split-K reduce of this conv folds the next
 * op's GroupNorm too, 3 this statistics pass does (plan option fold_fuse); *mod_row >= 0: the first row of the FiLM table whose 2 C
 * values per image -- scales, then shifts -- modulate the pairs that fold writes (SR3_UNET_SCALE_SHIFT_NORM), -1: none.  Host-only. */
int sr3_plan_op_fold(sr3_plan* plan, int batch, int index, int* fold, int* mod_row);
/* The same two for the shallow launch list of a plan under option feat_cache (below): what sr3_unet_forward_cached /
 * sr3_reverse_step_cached launch with refresh = 0.  Host-only.  On a plan without the option: -1 / SR3_E_BADARG. */
int sr3_plan_num_ops_cached(sr3_plan* plan, int batch);
int sr3_plan_op_info_cached(sr3_plan* plan, int batch, int index, sr3_op_info* out);
/* algorithmic FLOPs (contractions only) of one forward for `batch` images */
double sr3_plan_forward_flops(sr3_plan* plan, int batch);
/* host predicate of plan option store_wt: may a tensor (or a set of split-K slabs) of `bytes` bytes be written with write-through buffer
 * stores (32-bit offsets: bytes < 4 GiB)?  1 yes, 0: plain stores. */
int sr3_store_wt_fits(size_t bytes);
/* host query: the workgroup tile the plain GEMM kernel (tile 22 / 27-29) runs this problem on -- *rows 32 or 64, *cols 64 (four waves
 * 2 x 2) or 128 (four waves side by side) -- for a 1x1 stride-1 (ksize 1) or 3x3 stride-2 (ksize 3) conv with B x Ho x Wo output
 * pixels.  Returns 1, or 0 when the kernel does not take the problem (then *rows and *cols are left alone).  Either pointer may be NULL. */
int sr3_gemm_tile(int B, int Ho, int Wo, int Cin, int Cout, int ksize, int* rows, int* cols);
/* tuning knobs: key in {"fuse_stats", "fuse_res", "tile_cfg", "ksplit", "keep_all", "split_bf16", "winograd",
 * "wino_split", "wino_split8", "wino2", "wino_ragged", "wino_up", "gemm_split", "gemm2", "gemm_s2", "gemm_n64", "fork_side", "gemm_wpre", "gemm_tile", "fold_fuse", "wgrad_split", "attn_split",
 * "attn_long", "store_wt", "gemm_epi", "train_geom", "loss_l2", "var_channels", "attn_heads", "attn_head_dim"};
 * returns previous value.
 * wino_split (default 1): the Winograd convolutions that run on the kernel's one-image tile (maps >= 16x16) use its 3 x bf16
 *   split instantiation: every fp32 operand as x = h + m + l (three bf16 terms, each residual exact in fp32), every product as
 *   the six bf16 MFMA products hh, hm, mh, mm, hl, lh with fp32 accumulation (v_mfma_f32_32x32x16_bf16) -- fp32-class results
 *   (dropped terms <= 2^-24 of a product; measured not less accurate than the fp32-MFMA instantiation on every layer shape,
 *   tests/test_gpu_ops.py), not the bit pattern of the fp32 MFMA.  The derived buffer then holds both forms of every filter
 *   (sr3_plan_derived_bytes grows 2.5x; re-bind after toggling).  0: v_mfma_f32_32x32x2_f32 everywhere.
 * gemm_split (default 1): the same 3 x bf16 split arithmetic for the convolutions of the im2col kernel (every 1x1 conv --
 *   res_conv, attention qkv / out -- and the stride-2 Downsample convs), operands split while they are staged into LDS.
 *   0: v_mfma_f32_32x32x2_f32.
 * gemm_tile (default 0 = automatic; A/B runs): force im2col tile 1-4 (128x128 / 128x64 / 64x64 / 64x128) on every convolution of that
 *   kernel -- how profiles/r04f_gemm_split_sweep.txt timed the tiles inside the forward.
 * wino_split8 (default 1, round 5): the four-image tile of the 8x8 maps on its 3 x bf16 split instantiation too (no dropout form:
 *   a training forward's dropout convs on 8x8 maps keep the fp32 MFMA).
 * wino2 (default 1, round 6): the wino_split convolutions of the one-image tile without dropout -- every 3x3 stride-1 convolution on
 *   maps >= 16 wide in an inference plan, block1 / Upsample convs and the data gradients in a training plan -- run as TWO independent
 *   four-wave workgroups per CU on an 8 x 16 pixel tile (conv3x3_wino2.hip; reported as tile 13): same arithmetic and derived filters,
 *   a wave owns one transform column and all four rows.  0: the 8-wave kernel of conv3x3_wino.hip everywhere (tile 12).
 * wino_ragged (default 1; needs wino_split and wino2; inference plans whose geometry is not image_size x image_size, see
 *   sr3_plan_set_geometry): 3x3 stride-1 convolutions on maps that are not whole multiples of the 8 x 16 tile run on the two-workgroup
 *   kernel's ragged instantiation (reported as tile 23: the tile grid is rounded up, the kernel masks the overhang) where the
 *   measured rule of DESIGN.md says the padded tile beats the fallback.  0: they land on the general kernels (A/B knob).
 * wino_up (default 1): Upsample's convolution (nearest x2, then 3x3) on the two-workgroup kernel runs that kernel's upsample
 *   instantiation: on a nearest x2 map, row 2 and column 2 of the Winograd input transform are exactly zero, so seven of the sixteen
 *   positions are skipped -- their MFMAs, operand builds and filter fragments.  Same bits as the sixteen-position loop for finite
 *   filters (a filter holding inf / NaN is the one input where 0 x inf would differ); still reported as tile 13 / 23.  0: all sixteen
 *   positions (reported as tile 25 / 26; A/B knob).
 * gemm2 (default 1, round 6; needs gemm_split): 1x1 stride-1 convolutions with Cout % 128 == 0, channel counts % 32 == 0 and
 *   B * H * W % 64 == 0 (res_conv, attention qkv / out of the BASELINE networks) run as a plain GEMM on the same 3 x bf16 split
 *   arithmetic (gemm1x1.hip; reported as tile 22): 64 x 128 tile, weights pre-split in MFMA fragment order in the derived buffer
 *   (6 bytes per weight: sr3_plan_derived_bytes grows; re-bind after toggling) and read straight from global memory, the A rows
 *   split once per 128 output channels; a training plan's 1x1 data gradients use it too.  0: the im2col kernel (tiles 14-17).
 * gemm_s2 (default 1, round 6; needs gemm2): Downsample's 3x3 stride-2 pad-1 convolutions with Cout % 128 == 0 (one source, no
 *   activation, even maps) run on the same kernel's stride-2 form (also reported as tile 22): the GEMM's k-steps walk (32-channel
 *   chunk, tap), the A row of a tap is the NHWC row of the shifted input pixel, padding rows are zeroed where they are staged;
 *   54 bytes per weight in the derived buffer.  0: the im2col kernel (tile 16).
 * gemm_n64 (default 1, round 6; needs gemm2): the layers with Cout % 128 != 0 and Cout % 64 == 0 (res_conv of the first resolution level,
 *   Downsample 64 -> 64 with gemm_s2, data gradients towards 64 / 192 channels) on the same kernel's 64 x 64 tile, its four waves 2 x 2.
 *   0: they keep the im2col kernel (tile 16; Downsample 64 -> 64 its fp32 form, tile 2).
 * fork_side (default 0; A/B knob, inference plans): every unsplit res_conv is emitted in front of its block's first conv and launched
 *   on a side stream the plan owns (fork / join by events: a parallel branch once the forward is captured into a graph), block2's conv
 *   waits for it; the embedding MLP runs beside the input conv the same way.  Results are bit-identical (same kernels, same operands).
 * fold_fuse (default 1, round 6): the GroupNorm fold of a consumer is done by the kernel that completes its last source where that
 *   is a split-K reduce or a stand-alone statistics pass (one workgroup per (image, consumer group), no atomics): those fold
 *   launches leave the launch list (sr3_plan_num_ops shrinks), the conv outputs are bit-identical, the folded (scale, shift) pairs
 *   differ in the order of their double-precision sums only.  0: every fold is a launch of its own.
 * gemm_wpre (default 0): the im2col split tiles read their weights pre-split AND in MFMA fragment order straight from the derived
 *   buffer (tiles 18-21; round 6's form, no LDS staging of the weights) instead of splitting them while staging (14-17, what a plan
 *   runs); measured slower in every layout tried (profiles/r05c_*, profiles/r06_gemm_wpre_fragment_major.txt), kept as an A/B knob.
 * wgrad_split (default 1, round 5; training): weight gradients of the layers with more than 64 input AND output channels on
 *   v_mfma_f32_32x32x16_bf16 with 3-way split operands (wgrad.hip), gated by the batch-64 gradient tests against float64 autograd;
 *   0: the fp32-MFMA weight-gradient kernels.  No rebuild of the plan.
 * attn_split (default 1, round 5): SelfAttention's two contractions (Q K^T, P V) on the 3 x bf16 split instantiation of the
 *   staging-free kernel, gated against float64 like the convolutions; 0: v_mfma_f32_32x32x2_f32.  No rebuild of the plan.
 * attn_long (default 0; inference plans): an attention level with more tokens than the score-strip kernels hold in LDS (about 1088: every
 *   image above 256 x 256 in area with attention at the 1/8-resolution level) runs on the key-blocked kernel of csrc/attention_long.hip
 *   (online softmax over chunks of 512 keys, LDS use independent of the token count; reported as tile_cfg 24 on the attention op) instead
 *   of refusing the geometry.  A level the strip kernels hold keeps them: launch list, workspace and output bits are those of
 *   attn_long = 0 there.  attn_split selects the arithmetic as for the strip kernels.  The default is 0 for ONE reason: a test pins the
 *   refusal of a fresh plan at 384 x 384; a later change that rewrites that test can flip it.
 * attn_heads (default 1) / attn_head_dim (default 0 = off): multi-head SelfAttention (the reference module's n_head; sr3_attention_heads_f32
 *   has the layout).  attn_heads = H: every attention level runs H heads of C / H channels.  attn_head_dim = d: every level runs C / d
 *   heads of d channels, so levels of different width get different head counts (ADM's num_head_channels).  Mutually exclusive: setting
 *   one while the other is on is SR3_E_BADARG.  A value some attention level cannot take (C not divisible, head width not a multiple of
 *   4) is SR3_E_BADARG with the level and its channels in the message; the plan keeps its previous value.  The weights keep their
 *   shapes, the launch list its length and kinds; the attention ops carry their head count to the forward and the training backward.
 *   With both at their defaults every launch and bit is the single-head one.  Rebuilds the launch list.
 * store_wt (default 3; a mask, 0 .. 7): which kernels write their 16-byte epilogue stores THROUGH L2 (buffer stores with sc1) instead of
 *   leaving the lines dirty for the kernel boundary to write back: 1 the two-workgroup Winograd kernel (outputs and split-K slabs),
 *   2 the 8-wave Winograd kernel, 4 the split-K reduce kernels (k_rows_fold, k_splitk_reduce).  The plain GEMM has an option of its
 *   own (gemm_epi, below); the input conv stores 4 bytes per lane, attention 8 at its batch-16 shape.
 *   Every value gives the same bits; read at launch, no rebuild of the plan.  A
 *   tensor or slab set of 4 GiB or more keeps plain stores (sr3_store_wt_fits).  What was measured: DESIGN.md section 3.2c.
 * gemm_epi (default 2; 0, 1 or 2, SR3_E_BADARG otherwise): the epilogue of the plain GEMM kernel (tile 22: gemm2, gemm_s2, gemm_n64; the training
 *   forward and the 1x1 / stride-2 data gradients on that kernel too).  0: every lane stores its accumulator registers as 4-byte
 *   elements.  1: each wave transposes its 32 x 32 accumulator blocks through LDS, so that a lane owns four consecutive output
 *   channels of a row: bias, FiLM row, residual and the store are 16 bytes wide (needs RC0 % 4 == 0, film_stride % 4 == 0 and 16-byte
 *   aligned bias / film / residual / out: once the option has been SET, or under tiles 28 / 29, a launch that does not meet them is
 *   SR3_E_UNSUPPORTED / SR3_E_ALIGN; a plan whose option was never set, and tile 22, run such a launch on form 0 instead).  2: ... and those stores are written through L2
 *   as store_wt's families are (outputs and split-K slabs; 4 GiB or more keep plain stores).  Every value gives the same bits (the
 *   additions per element keep their order); read at launch, no rebuild: launch list, workspace and derived buffer do not depend on
 *   it, and the ops still report tile 22.  The per-op entries name the forms as tiles 27 / 28 / 29 (= gemm_epi 0 / 1 / 2); tile 22
 *   there is the form a fresh plan runs.  The default and what was measured: DESIGN.md section 3.2c, profiles/gemm_epi_ab.txt.
 * train_geom (default 0; training): sr3_train_workspace_bytes and sr3_train_step follow sr3_plan_set_geometry like the forward does: the
 *   training plan is built for the plan's height x width (hr / cond / z are [B, C, height, width]) and cached by (batch, cond_channels,
 *   height, width).  Its forward picks every conv through the inference planner's rule (the ragged Winograd tile 23 included, for the convs
 *   without dropout), the data gradients through the same rule, the 3x3 weight gradients of the <= 64-channel layers keep the 9-tap
 *   kernel on every map whose width is a multiple of 8; an attention level beyond the score strip needs attn_long (forward on the
 *   key-blocked kernel, backward on its key-blocked path with the dK / dV slabs -- no atomics) and is refused without it.  At
 *   image_size x image_size the launch list, the workspace and every bit of the result are those of train_geom = 0.  0: training is
 *   refused at any other geometry.  The default is 0 only because tests pin that refusal; nothing else speaks against 1.
 * var_channels (default 0): learned reverse-process variance (Nichol & Dhariwal 2021).  0, or half of out_channel (SR3_E_BADARG otherwise):
 *   the last var_channels filter rows of the output conv are the variance head v, the first out_channel - var_channels the prediction,
 *   and x / z / eps of every step are [B, out_channel - var_channels, H, W].  sr3_unet_forward and every reverse-step entry launch the
 *   output conv on the prediction rows alone (the first rows of the same filters: the bits of the network made of those rows), so every
 *   sampler runs on such a checkpoint with its table sigma; sr3_unet_forward_full returns all rows (for sr3_learned_var_step), the
 *   training forward always computes them (sr3_train_step_ex2).  A plan with out_channel 6 or 8 can be created without it but builds no
 *   launch list: SR3_E_UNSUPPORTED "out_channel %d > 4 unsupported", as sr3_plan_create says for every other out_channel above 4.
 * loss_l2 (default 0): sr3_train_step uses nn.MSELoss(reduction='sum') instead of nn.L1Loss(reduction='sum')
 *   (GaussianDiffusion(loss_type='l2'), model/sr3_modules/diffusion.py:84-90).
 * split_bf16 (default 0, experimental; needs -DSR3_EXPERIMENTS, refused otherwise): run the halo-tile 3x3 convolutions of the inference plan on
 *   v_mfma_f32_32x32x16_bf16 with every fp32 operand split into three bf16 terms (x = h + m + l) and the six
 *   products hh, hm, mh, mm, hl, lh accumulated in fp32 -- fp32-class accuracy (dropped terms <= 2^-23 of a
 *   product), not the bit pattern of the fp32 MFMA.  Operands are split while they are staged into LDS (a pre-split
 *   weight copy was measured slower: 1.5x the L2->LDS bytes). */
int sr3_plan_set_option(sr3_plan* plan, const char* key, int value);

/* Debug taps: where each top-level layer output (downs.i / mid.i / ups.i, NHWC) lives inside the
 * workspace after a forward.  Only meaningful with option keep_all = 1 (no buffer reuse). */
int sr3_plan_num_taps(sr3_plan* plan);
int sr3_plan_tap_info(sr3_plan* plan, int index, char* name, int name_len, size_t* offset, int* C, int* H, int* W);

/* Geometry.  Height and width of the images the NEXT forward / reverse step / workspace query / plan inspection of this plan works
 * on; (0, 0) restores image_size x image_size (the state after sr3_plan_create).  Both must be positive multiples of 2^(n_mults-1)
 * (SR3_E_BADARG otherwise; the plan keeps its previous geometry).  The UNet is fully convolutional; attention placement stays where
 * UNet.__init__ put it from image_size (reference behaviour: model/sr3_modules/unet.py:235-259 never looks at the size).  Host only:
 * invalidates the built launch list (like an option change), not the derived filters.  Every layer picks its kernel through the same
 * fits-predicates as at the native size and lands on the general kernels where nothing faster fits; a geometry NO kernel can run
 * (an attention level with more tokens than the attention kernel holds in LDS, in a plan without option attn_long) is refused with
 * SR3_E_UNSUPPORTED and a message naming the level and its token count when the launch list is built -- by sr3_workspace_bytes (returns 0) / sr3_plan_num_ops
 * (returns -1) / the forward itself before it enqueues anything.  Training follows the geometry under plan option train_geom; without it
 * training is native-size only: sr3_train_workspace_bytes returns 0 and sr3_train_step SR3_E_UNSUPPORTED while the geometry is not
 * image_size x image_size. */
int sr3_plan_set_geometry(sr3_plan* plan, int height, int width);
int sr3_plan_get_geometry(const sr3_plan* plan, int* height, int* width);

/* Derived weights.  The inference plan runs its 3x3 stride-1 convolutions as Winograd F(2x2,3x3) (plan option
 * "winograd", default 1), which reads the transformed filters U = G g G^T from a caller-owned device buffer of
 * sr3_plan_derived_bytes bytes (16/9 of the 3x3 weights).  Bind it once (the pointer is kept, and baked into captured
 * graphs), and re-run sr3_plan_prepare_derived on the stream whenever the parameter arena changed (checkpoint load,
 * optimizer step): ~55 small launches.
 * STALE FILTERS FAIL LOUDLY: sr3_unet_forward / sr3_train_step return SR3_E_BADARG when the plan needs the filters and
 * (a) none is bound, (b) the buffer was never prepared, (c) it was prepared from a different `params` pointer than the
 * call's, (d) one of the plan options winograd / tile_cfg / split_bf16 / wino_split was set since (wino_split also changes
 * sr3_plan_derived_bytes and un-binds a buffer that is now too small), or (e) sr3_plan_invalidate_derived was called
 * after the last prepare.  The library cannot see writes to the arena (sr3_adam_step takes no plan): a caller that
 * updates parameters in place calls sr3_plan_invalidate_derived right after the update and prepares again before the
 * next forward.  The buffer contract at sr3_workspace_bytes holds for this buffer too: exactly sr3_plan_derived_bytes bytes, 16-byte
 * aligned (SR3_E_NOMEM / SR3_E_ALIGN from sr3_plan_bind_derived otherwise), prior contents irrelevant -- sr3_plan_prepare_derived writes
 * every byte a forward reads. */
size_t sr3_plan_derived_bytes(const sr3_plan* plan);
int sr3_plan_bind_derived(sr3_plan* plan, void* buffer, size_t bytes);
int sr3_plan_prepare_derived(sr3_plan* plan, const float* params, void* stream);
int sr3_plan_invalidate_derived(sr3_plan* plan);
/* sr3_workspace_bytes: workspace bytes for sr3_unet_forward / sr3_reverse_step* at this batch size and the plan's current geometry
 * (activations, statistics, FiLM table, split-K slabs).
 * THE BUFFER CONTRACT of every caller-owned workspace, derived buffer and scratch of this library (tests/test_gpu_workspace_contract.py,
 * tests/test_gpu_scratch_contract.py, tests/test_scratch_contract_cpu.py):
 *   1. a buffer of exactly the queried byte count is enough (aligned as the entry states: 256 bytes for a workspace);
 *   2. nothing outside it is written;
 *   3. what it held before the call does not matter -- zeros, NaN patterns, the leftovers of another batch size, geometry or plan: the
 *      results are the same bits.  No zeroing is ever needed, and none should be done (it is a pass over HBM per call).
 * A buffer below the query, or a misaligned one, is refused on the host before anything is launched (SR3_E_NOMEM naming both sizes /
 * SR3_E_ALIGN; the few entries that document SR3_E_BADARG for a small scratch keep that code). */
size_t sr3_workspace_bytes(sr3_plan* plan, int batch);

/* UNet.forward (model/sr3_modules/unet.py:235-259, model/ddpm_modules/unet.py:220-243).
 *   x_nchw    : (B, in_channel - cond_channels, H, W)  the noisy image; H x W = the plan's geometry (sr3_plan_set_geometry;
 *               image_size x image_size unless set)
 *   cond_nchw : (B, cond_channels, H, W) or NULL -- the conditioning image; the engine consumes the
 *               pair as the virtual concat torch.cat([cond, x], 1) (model/sr3_modules/diffusion.py:157)
 *   noise_level : (B) fp32, SR3 variant (the (B,1) tensor of diffusion.py:153-154), else NULL
 *   timestep  : (B) int64, DDPM variant, else NULL
 *   freq      : (inner_channel/2) fp32 frequency table (PositionalEncoding / TimeEmbedding.inv_freq)
 *   level_table/step_dev : optional graph-replay source of the conditioning value: when step_dev is
 *               non-NULL the level is level_table[*step_dev + 1] (SR3) or the timestep *step_dev (DDPM)
 *   params    : packed parameter arena (see sr3_plan_param_info)
 *   eps_out_nchw : (B, out_channel, H, W) */
int sr3_unet_forward(sr3_plan* plan, const float* x_nchw, const float* cond_nchw, int cond_channels,
                     const float* noise_level, const int64_t* timestep, const float* freq,
                     const float* level_table, const int* step_dev, const float* params,
                     void* workspace, size_t workspace_bytes, float* eps_out_nchw, int batch,
                     void* stream);

/* The same forward with every output row: eps_out_nchw is (B, out_channel, H, W), the prediction channels followed by the variance
 * head of a plan under option var_channels (without the option: sr3_unet_forward's call).  t_map (with step_dev; DDPM variant): the
 * timestep is t_map[*step_dev], as in sr3_reverse_step_ex; NULL: *step_dev. */
int sr3_unet_forward_full(sr3_plan* plan, const float* x_nchw, const float* cond_nchw, int cond_channels,
                          const float* noise_level, const int64_t* timestep, const float* freq,
                          const float* level_table, const int* step_dev, const float* params,
                          void* workspace, size_t workspace_bytes, float* eps_out_nchw, int batch,
                          void* stream, const int* t_map);

/* Same forward, run eagerly with a hipEvent pair around every launch of the plan (events are
 * recorded on `stream`).  Measurement aid for bench.py's roofline leg; not capturable.
 * One entry per kernel launch.  op_kind: 10 embed+FiLM, 20 input conv, 30 GN statistics, 40 GN fold,
 * 51..54 im2col implicit-GEMM conv (tile config), 55/56 halo-tile 3x3 conv k_conv3x3_halo<2,2,false> /
 * <4,1,false>, 57/58 the same with the fused 1x1 res_conv segment (<.,.,true>), 59 split-K reduce,
 * 60 attention, 70 output Block.  op_flops: algorithmic FLOPs of contractions (0 for HBM-bound helpers). */
int sr3_unet_forward_profile(sr3_plan* plan, const float* x_nchw, const float* cond_nchw, int cond_channels,
                             const float* noise_level, const int64_t* timestep, const float* freq,
                             const float* params, void* workspace, size_t workspace_bytes, float* eps_out_nchw,
                             int batch, void* stream, int max_ops, float* op_ms, int* op_kind, double* op_flops,
                             int* n_ops);

/* Fused elementwise tail of p_mean_variance + p_sample (model/sr3_modules/diffusion.py:141-149,
 * 162-174; model/ddpm_modules/diffusion.py:151-198), in place on x:
 *   x0 = a[t] x - b[t] eps ; clamp(-1,1) ; mean = c1[t] x0 + c2[t] x ; x = mean + sigma[t] z
 * tables (length T, fp32): a = sqrt_recip_alphas_cumprod, b = sqrt_recipm1_alphas_cumprod,
 * c1/c2 = posterior_mean_coef1/2, sigma[t] = exp(0.5 posterior_log_variance_clipped[t]), sigma[0] = 0.
 * t is *step_dev if non-NULL, else t_per_sample[b] if non-NULL, else step_host.  z may be NULL (= 0). */
int sr3_p_sample_step(float* x_nchw, const float* eps_nchw, const float* z_nchw, const float* tab_a,
                      const float* tab_b, const float* tab_c1, const float* tab_c2, const float* tab_sigma,
                      const int* step_dev, const int64_t* t_per_sample, int step_host, int batch,
                      int elems_per_image, void* stream);
/* The same update with the reference's `clip_denoised` switch (p_mean_variance, model/sr3_modules/diffusion.py:162-163,
 * model/ddpm_modules/diffusion.py:184-185): clip_denoised == 0 skips the clamp of x0; != 0 is sr3_p_sample_step. */
int sr3_p_sample_step_ex(float* x_nchw, const float* eps_nchw, const float* z_nchw, const float* tab_a,
                         const float* tab_b, const float* tab_c1, const float* tab_c2, const float* tab_sigma,
                         const int* step_dev, const int64_t* t_per_sample, int step_host, int batch,
                         int elems_per_image, int clip_denoised, void* stream);
/* The tail of a MULTISTEP sampler (DPM-Solver++(2M) in the tail's linear form): the update also takes the previous step's x0,
 *   x0 = a[t] x - b[t] eps ; clamp(-1,1) if clip_denoised ; x = ((c1[t] x0 + c2[t] x) + c3[t] hist) + sigma[t] z ; hist <- x0
 * every product and sum rounded separately in fp32, in exactly that association.  hist_nchw has the layout of x_nchw; an element's
 * history is read and then overwritten by the thread that owns the element.  The caller zero-fills it before a chain's first step
 * (whose c3 is 0: 0 * NaN is NaN).  tab_c3 and hist_nchw are both set or both NULL; both NULL is sr3_p_sample_step_ex, bit for bit.
 * Any elems_per_image (a size that is no multiple of 4, or a pointer off a 16-byte boundary, takes the one-element-per-thread form).
 * SR3_E_BADARG: NULL required pointer, non-positive size, only one of tab_c3 / hist_nchw, hist_nchw overlapping x_nchw or eps_nchw.
 * Nothing is launched on a refusal. */
int sr3_p_sample_step_hist(float* x_nchw, const float* eps_nchw, const float* z_nchw, const float* tab_a,
                           const float* tab_b, const float* tab_c1, const float* tab_c2, const float* tab_sigma,
                           const int* step_dev, const int64_t* t_per_sample, int step_host, int batch,
                           int elems_per_image, int clip_denoised, const float* tab_c3, float* hist_nchw, void* stream);
/* *step_dev -= 1 on the stream (loop counter of p_sample_loop, diffusion.py:193, for graph replay) */
int sr3_step_decrement(int* step_dev, void* stream);

/* One WHOLE iteration of the reference's reverse loop (model/sr3_modules/diffusion.py:190-196 `for i in reversed(range(T)): img = p_sample(img, i, ...)`
 * with p_sample = :169-174, p_mean_variance :151-167; model/ddpm_modules/diffusion.py:200-215) as one capturable call:
 *   eps = UNet(cat(cond, x), level(t))  ;  x <- p_sample update of (x, eps, z, t)  ;  t <- t - 1
 * = sr3_unet_forward + sr3_p_sample_step_ex + sr3_step_decrement, with the last two inside the output convolution's kernel (the thread
 * that produces an element of eps updates the same element of x; separately rounded operations, bit-identical to the three-call form):
 * two kernel nodes fewer per replayed step.
 *   x_nchw      : [B, C, H, W] the image, in / out (H x W = the plan's geometry)
 *   step2_dev   : TWO ints.  step2_dev[1] = t of this step on entry (the caller sets it to T - 1 before the first step) and t - 1 on
 *                 completion; step2_dev[0] is scratch (the step's first kernel copies t there for its last one).  t must stay >= 0.
 *   level_table : SR3: level = level_table[t + 1] (sqrt_alphas_cumprod_prev); DDPM: ignored (the timestep is t)
 *   z_nchw      : the step's noise or NULL (= 0); tab_*: the schedule tables of sr3_p_sample_step (sigma[0] = 0 replaces `t > 0`)
 *   eps_out_nchw: NULL, or where to also store eps (parity checks)
 * The counter is a STEP INDEX: tab_* and level_table are indexed by it, and nothing else in the step reads it.  In the reference's
 * loop the index is the training timestep; a sampler that walks a subset of the timesteps passes tables built for its walk
 * (one row per step taken) and counts its steps down instead -- see sr3_reverse_step_ex for the DDPM variant. */
int sr3_reverse_step(sr3_plan* plan, float* x_nchw, const float* cond_nchw, int cond_channels, const float* freq,
                     const float* level_table, int* step2_dev, const float* params, void* workspace, size_t workspace_bytes,
                     const float* z_nchw, const float* tab_a, const float* tab_b, const float* tab_c1, const float* tab_c2,
                     const float* tab_sigma, int clip_denoised, float* eps_out_nchw, int batch, void* stream);
/* sr3_reverse_step for a walk through a subset of the timesteps (a strided DDIM sampler: S steps over tau[0] < ... < tau[S-1]).
 *   t_map : device array, one int per step index: the timestep the DDPM UNet is conditioned on when the counter reads that index
 *           (t_map[j] = tau[j]; the embedding kernel reads t_map[step2_dev[1]]).  NULL: index = timestep, i.e. sr3_reverse_step.
 *           The SR3 variant ignores it: its level_table, indexed by the step index (level_table[j + 1] = the level of tau[j]), already
 *           is the map.
 * tab_* and level_table are indexed by the step index j, exactly as in sr3_reverse_step; the caller sets step2_dev[1] = S - 1 before
 * the first step and fills the tables with the coefficients of its update rule in the tail's form
 *   x0 = clamp(a[j] x - b[j] eps) ; x = c1[j] x0 + c2[j] x + sigma[j] z. */
int sr3_reverse_step_ex(sr3_plan* plan, float* x_nchw, const float* cond_nchw, int cond_channels, const float* freq,
                        const float* level_table, int* step2_dev, const float* params, void* workspace, size_t workspace_bytes,
                        const float* z_nchw, const float* tab_a, const float* tab_b, const float* tab_c1, const float* tab_c2,
                        const float* tab_sigma, int clip_denoised, float* eps_out_nchw, int batch, void* stream, const int* t_map);
/* sr3_reverse_step_ex with the multistep tail of sr3_p_sample_step_hist in the output convolution's epilogue (its own instantiations of
 * that kernel: the step without history runs the code it ran before):
 *   x0 = clamp(a[j] x - b[j] eps) ; x = ((c1[j] x0 + c2[j] x) + c3[j] hist) + sigma[j] z ; hist <- x0.
 *   tab_c3    : one more table indexed by the step index j;  hist_nchw : [B, C, H, W], 16-byte aligned, in / out -- zero-filled by the
 *               caller before a chain's first step.  Both set or both NULL (NULL: sr3_reverse_step_ex, bit for bit).
 * Still one capturable call with the same kernel nodes.  Bit-identical to sr3_unet_forward + sr3_p_sample_step_hist + sr3_step_decrement.
 * SR3_E_BADARG besides sr3_reverse_step_ex's: only one of tab_c3 / hist_nchw; hist_nchw overlapping x_nchw or eps_out_nchw (checked
 * before any launch). */
int sr3_reverse_step_hist(sr3_plan* plan, float* x_nchw, const float* cond_nchw, int cond_channels, const float* freq,
                          const float* level_table, int* step2_dev, const float* params, void* workspace, size_t workspace_bytes,
                          const float* z_nchw, const float* tab_a, const float* tab_b, const float* tab_c1, const float* tab_c2,
                          const float* tab_sigma, int clip_denoised, float* eps_out_nchw, int batch, void* stream, const int* t_map,
                          const float* tab_c3, float* hist_nchw);

/* ---- feature-cached forward (engine extension; plan option feat_cache; DeepCache, Ma et al. 2023) --------------------------
 * Consecutive reverse steps feed the network almost the same input, and what lies below the top resolution level moves little between
 * them: a cached step recomputes only the shallow forward of the option's depth and reads everything deeper, as one tensor, from the
 * last full step.  An approximation the caller opts into; how often to refresh is the caller's schedule.
 * sr3_plan_set_feature_cache: plan option feat_cache = depth (default 0 = off; inference plans), set through this entry rather than as a
 *   key of sr3_plan_set_option; returns the previous value like it.  depth d in 1 .. res_blocks + 1 (SR3_E_UNSUPPORTED otherwise, the
 *   range named) compiles a second, shallow launch list next to the full one -- the embedding, the first d entries of downs (the input
 *   conv and d - 1 res blocks), the last d res blocks of ups with their attention, the output conv: all on the top resolution level --
 *   whose first up block reads the tensor that enters it in the full forward (the branch tensor) and its GroupNorm partials from a
 *   caller-owned feature cache.  The full list of such a plan runs the ops, kernels and bits of a plan without the option, with the
 *   branch tensor's producer writing into the cache; it runs through the two _cached entries alone (every other forward entry refuses a
 *   plan under the option: it has no cache to write).  sr3_workspace_bytes covers both lists.  The training plan does not look at it.
 * sr3_feature_cache_bytes: the size of the cache for `batch` images at the plan's geometry (the branch tensor, then its GroupNorm
 *   partials); 0 on a plan without the option.  The cache is the caller's, 256-byte aligned, and no part of the workspace: the
 *   workspace may hold anything between a refresh and the cached forwards behind it, the cache must be left alone.
 * sr3_unet_forward_cached: sr3_unet_forward_full's call.  refresh = 1: the full forward, which also leaves the branch tensor in
 *   feat_cache -- eps bit-identical to sr3_unet_forward_full on a plan without the option.  refresh = 0: the shallow forward on
 *   (x, level) reading feat_cache.
 * sr3_reverse_step_cached: sr3_reverse_step_hist's call, the tail and the counter decrement in the output conv as there.
 * Checked before any launch, behind the checks of the plain entry: feat_cache NULL (SR3_E_BADARG), feat_cache_bytes too small
 * (SR3_E_NOMEM), not 256-byte aligned (SR3_E_ALIGN); refresh = 0 on a plan without the option, on a cache no refresh has filled, or at
 * a batch / geometry / buffer other than the last refresh's (SR3_E_BADARG).  The bookkeeping is the host's, made when the call is
 * issued (or captured).  refresh = 1 on a plan without the option is the plain forward; the cache is not looked at. */
int sr3_plan_set_feature_cache(sr3_plan* plan, int depth);
size_t sr3_feature_cache_bytes(sr3_plan* plan, int batch);
int sr3_unet_forward_cached(sr3_plan* plan, const float* x_nchw, const float* cond_nchw, int cond_channels,
                            const float* noise_level, const int64_t* timestep, const float* freq,
                            const float* level_table, const int* step_dev, const float* params,
                            void* workspace, size_t workspace_bytes, float* eps_out_nchw, int batch,
                            void* stream, const int* t_map, void* feat_cache, size_t feat_cache_bytes, int refresh);
int sr3_reverse_step_cached(sr3_plan* plan, float* x_nchw, const float* cond_nchw, int cond_channels, const float* freq,
                            const float* level_table, int* step2_dev, const float* params, void* workspace, size_t workspace_bytes,
                            const float* z_nchw, const float* tab_a, const float* tab_b, const float* tab_c1, const float* tab_c2,
                            const float* tab_sigma, int clip_denoised, float* eps_out_nchw, int batch, void* stream, const int* t_map,
                            const float* tab_c3, float* hist_nchw, void* feat_cache, size_t feat_cache_bytes, int refresh);

/* ---- tiled sampling (engine extension; no reference counterpart) ------------------------------
 * An image larger than the training size is sampled as ONE chain whose eps comes from overlapping tiles of the training size: per
 * reverse step the tiles are cut out of the running image (sr3_tile_gather), the UNet predicts eps on batches of them
 * (sr3_unet_forward with step_dev = step2_dev + 1) and sr3_tiled_step blends the predictions and applies the p_sample update to the
 * whole image.  Tile order: (b * ny + iy) * nx + ix; tile (iy, ix) is the th x tw window at (oy[iy], ox[ix]).  Origins are any
 * integers in [0, H - th] / [0, W - tw] (no alignment); what the kernels read from the device arrays is clamped into that range. */

/* dst_tiles[i] = the window of tile first_tile + i, i < n_tiles (a contiguous range of the tile order: it may start and end inside
 * an image), all `channels` channels: [n_tiles, channels, th, tw] out of src_nchw [batch, channels, height, width].  Bit copy.
 * oy_dev [ny], ox_dev [nx]: device int arrays.  SR3_E_BADARG: NULL pointer, non-positive size, th > height, tw > width, a tile range
 * outside [0, batch * ny * nx); SR3_E_UNSUPPORTED: batch * channels * height * width >= 2^31. */
int sr3_tile_gather(const float* src_nchw, int batch, int channels, int height, int width, const int* oy_dev, int ny,
                    const int* ox_dev, int nx, int first_tile, int n_tiles, int th, int tw, float* dst_tiles, void* stream);

/* The tail of one tiled reverse step, in place on x_nchw [batch, channels, height, width]:
 *   eps(p) = the covering tile's value unchanged where ONE tile covers pixel p (no multiply, no divide), else
 *            (sum_i wy_i wx_i eps_i(p)) / (sum_i wy_i wx_i) over the covering tiles in ascending tile index, every product, sum and
 *            the quotient rounded separately in fp32; wy_i = wy_dev[y - oy[iy]], wx_i = wx_dev[x - ox[ix]]  (wy_dev [th], wx_dev [tw] > 0)
 *   x0 = a[j] x - b[j] eps ; clamp(-1, 1) if clip_denoised ; x = c1[j] x0 + c2[j] x + sigma[j] z      (sr3_p_sample_step_ex's operations)
 * with j = step2_dev[1] on entry; step2_dev[1] = j - 1 on completion (step2_dev[0] is scratch, as in sr3_reverse_step).  With one
 * tile of the image's size this is sr3_p_sample_step_ex + sr3_step_decrement bit for bit.
 *   eps_tiles    : [batch * ny * nx, channels, th, tw]
 *   oy_host/ox_host : NULL, or host copies of the origin lists for validation: each must start at 0, increase strictly, end at
 *                  height - th / width - tw and leave no gap between consecutive tiles (SR3_E_BADARG otherwise)
 *   z_nchw       : the step's noise or NULL (= 0); tab_*: as sr3_reverse_step; eps_out_nchw: NULL, or where the blended eps goes
 * Gather form (a thread owns pixels and reads the tiles covering them): no atomics, bitwise reproducible.  Two launches.
 * SR3_E_BADARG: NULL required pointer, non-positive size, th > height, tw > width, bad host origins; SR3_E_UNSUPPORTED:
 * batch * channels * height * width >= 2^31; SR3_E_ALIGN: width % 4 == 0 and x / z / eps_out not 16-byte aligned.  Nothing is
 * launched on a refusal. */
int sr3_tiled_step(float* x_nchw, const float* eps_tiles, int batch, int channels, int height, int width, const int* oy_dev, int ny,
                   const int* ox_dev, int nx, const float* wy_dev, const float* wx_dev, int th, int tw, const int* oy_host,
                   const int* ox_host, const float* z_nchw, const float* tab_a, const float* tab_b, const float* tab_c1,
                   const float* tab_c2, const float* tab_sigma, int* step2_dev, int clip_denoised, float* eps_out_nchw, void* stream);
/* sr3_tiled_step with the multistep tail: the blend first, then sr3_p_sample_step_hist's operations on the whole image.  tab_c3 /
 * hist_nchw ([batch, channels, height, width], a whole-image buffer as z_nchw is): both set or both NULL (NULL: sr3_tiled_step, bit for
 * bit).  SR3_E_BADARG besides sr3_tiled_step's: only one of the two; hist_nchw overlapping x_nchw or eps_out_nchw.  SR3_E_ALIGN: width
 * % 4 == 0 and hist_nchw not 16-byte aligned.  Nothing is launched on a refusal. */
int sr3_tiled_step_hist(float* x_nchw, const float* eps_tiles, int batch, int channels, int height, int width, const int* oy_dev, int ny,
                        const int* ox_dev, int nx, const float* wy_dev, const float* wx_dev, int th, int tw, const int* oy_host,
                        const int* ox_host, const float* z_nchw, const float* tab_a, const float* tab_b, const float* tab_c1,
                        const float* tab_c2, const float* tab_sigma, int* step2_dev, int clip_denoised, float* eps_out_nchw, void* stream,
                        const float* tab_c3, float* hist_nchw);

/* ---- LR-consistent sampling (engine extension; no reference counterpart) ------------------------
 * The range / null-space projection of DDNM (Wang et al. 2022) for the block x block average pool, in the tail of a reverse step: every
 * step shifts each block of the predicted x0 so that its mean is the target's (times `strength`), and keeps the rest from the network. */

/* dst_means[b, c, by, bx] = the mean of the block x block block (by, bx) of src_nchw [batch, channels, height, width], summed in double
 * in a fixed order and rounded once: [batch, channels, height / block, width / block].  What sr3_consistent_step's targets are made
 * with, and what measures a result's consistency error max |block_mean(SR) - block_mean(LR upsampled)|.  Any alignment (a width or
 * block that is no multiple of 4, or a src_nchw off a 16-byte boundary, takes the one-element-per-thread form).
 * SR3_E_BADARG: NULL src_nchw / dst_means, non-positive size, block not in {2, 4, 8, 16, 32} or not dividing both height and width,
 * dst_means overlapping src_nchw; SR3_E_UNSUPPORTED: batch * channels * height * width >= 2^31.  Nothing is launched on a refusal. */
int sr3_block_mean_f32(const float* src_nchw, int batch, int channels, int height, int width, int block, float* dst_means, void* stream);

/* The tail of one LR-consistent reverse step, in place on x_nchw [batch, channels, height, width], with j = step2_dev[1] on entry,
 * r = block, y = target_means [batch, channels, height / r, width / r]:
 *   x0  = a[j] x - b[j] eps ; clamp(-1, 1) if clip_denoised          (sr3_p_sample_step_ex's operations; clamp first, then project:
 *                                                                     the projected value may leave [-1, 1])
 *   S   = sum over the r x r block of (double) x0                    (fixed order, no atomics)
 *   d   = (float)((double) strength * ((double) y - S / (double)(r r)))      one rounding to fp32
 *   x0' = x0 + d
 *   x   = ((c1[j] x0' + c2[j] x) + c3[j] hist) + sigma[j] z ; hist <- x0'    (sr3_p_sample_step_hist's operations and association;
 *                                                                             tab_c3 / hist_nchw both NULL: no history term)
 * every fp32 product, sum and difference rounded separately.  step2_dev[1] = j - 1 on completion (step2_dev[0] is scratch, as in
 * sr3_tiled_step).  With strength 1 the block means of x0' are the target's to rounding.  eps_nchw is the network's output for this
 * step (sr3_unet_forward with step_dev = step2_dev + 1); z_nchw: the step's noise or NULL (= 0); tab_*: as sr3_reverse_step.
 * Two launches; bitwise reproducible.  Any alignment (width % 4 != 0, block % 4 != 0 or a pointer off a 16-byte boundary takes the
 * one-element-per-thread form, the same bits).
 * SR3_E_BADARG (the message names the argument): NULL required pointer, non-positive size, block not in {2, 4, 8, 16, 32} or not
 * dividing both height and width, strength NaN or outside (0, 1], only one of tab_c3 / hist_nchw, hist_nchw overlapping x_nchw or
 * eps_nchw, target_means overlapping x_nchw; SR3_E_UNSUPPORTED: batch * channels * height * width >= 2^31.  Nothing is launched on a
 * refusal. */
int sr3_consistent_step(float* x_nchw, const float* eps_nchw, const float* z_nchw, const float* target_means, int batch, int channels,
                        int height, int width, int block, float strength, const float* tab_a, const float* tab_b, const float* tab_c1,
                        const float* tab_c2, const float* tab_sigma, int* step2_dev, int clip_denoised, const float* tab_c3,
                        float* hist_nchw, void* stream);

/* ---- zero-shot restoration (engine extension; no reference counterpart) --------------------------
 * Inpainting and colourisation with a trained model and no training (RePaint, Lugmayr et al. 2022; DDNM, Wang et al. 2022): the range /
 * null-space projection of the predicted x0 for a pixel mask or a channel sum, in the tail of a reverse step, and the forward jump of
 * the resampled walk.  Every entry checks its arguments on the host, names the offending one in sr3_last_error and launches nothing on
 * a refusal; everything a call writes is checked against every other argument.  No host synchronisation, no allocation: capturable.
 * Any alignment (width % 4 != 0 -- elems_per_image % 4 != 0 for the jump -- or a pointer off a 16-byte boundary takes the
 * one-element-per-thread form, the same bits).  Every fp32 product, sum and difference is rounded separately, in the order written:
 * bitwise reproducible, and bit-identical to the same expression in IEEE fp32 anywhere. */

/* dst_nchw[b, 0, y, x] = ((a0 src[b, 0, y, x] + a1 src[b, 1, y, x]) + a2 src[b, 2, y, x]) + a3 src[b, 3, y, x] over the `channels` <= 4
 * planes of src_nchw [batch, channels, height, width]; gray_a_host: `channels` floats on the HOST, read during the call.  What the
 * gray operator's target is made with from a colour image, and what measures a result's error.  One launch.
 * SR3_E_BADARG: NULL pointer, non-positive size, channels > 4, a weight that is not finite, dst_nchw overlapping src_nchw;
 * SR3_E_UNSUPPORTED: batch * channels * height * width >= 2^31. */
int sr3_gray_f32(const float* src_nchw, int batch, int channels, int height, int width, const float* gray_a_host, float* dst_nchw,
                 void* stream);

/* The tail of one restoring reverse step, in place on x_nchw [batch, channels, height, width], with j = step2_dev[1] on entry and
 * l = strength:
 *   x0 = a[j] x - b[j] eps ; clamp(-1, 1) if clip_denoised                    (clamp first, then project, as sr3_consistent_step)
 *   op 0 (mask):  w = l m ;  x0' = (w y) + ((1 - w) x0)                        y = target [batch, channels, height, width] the known image,
 *                 m = mask [batch, mask_channels, height, width], mask_channels 1 (one plane for all channels) or channels, values
 *                 in [0, 1], 1 = known.  The lerp form: w = 1 gives y exactly, w = 0 gives x0 exactly.
 *   op 1 (gray):  g = ((a0 x0_0 + a1 x0_1) + a2 x0_2) + a3 x0_3 ;  r = y - g ;  x0'_c = x0_c + ((l p[c]) r)
 *                 y = target [batch, 1, height, width]; a = gray_a_host, p = gray_p_host = a / sum a^2 (the pseudo-inverse; the host
 *                 computes it in double and rounds once): `channels` <= 4 floats each on the HOST, read during the call and handed
 *                 to the kernel by value.  mask / mask_channels are not read.
 *   x  = ((c1[j] x0' + c2[j] x) + c3[j] hist) + sigma[j] z ; hist <- x0'       (sr3_p_sample_step_hist's operations and association;
 *                                                                              tab_c3 / hist_nchw both NULL: no history term)
 * step2_dev[1] = j - 1 on completion (step2_dev[0] is scratch, as in sr3_tiled_step).  eps_nchw is the network's output for this step;
 * z_nchw: the step's noise or NULL (= 0); tab_*: as sr3_reverse_step.  Two launches.
 * SR3_E_BADARG (the message names the argument): NULL required pointer (op 0: mask; op 1: the weights), op not 0 or 1, non-positive
 * size, mask_channels not 1 or channels (op 0), channels > 4 (op 1), strength NaN or outside (0, 1], only one of tab_c3 / hist_nchw,
 * hist_nchw overlapping x_nchw or eps_nchw, anything written (x_nchw, hist_nchw, step2_dev) overlapping another argument, a weight that
 * is not finite; SR3_E_UNSUPPORTED: batch * channels * height * width >= 2^31. */
int sr3_restore_step(float* x_nchw, const float* eps_nchw, const float* z_nchw, int op, const float* target, const float* mask,
                     int mask_channels, const float* gray_a_host, const float* gray_p_host, int batch, int channels, int height,
                     int width, float strength, const float* tab_a, const float* tab_b, const float* tab_c1, const float* tab_c2,
                     const float* tab_sigma, int* step2_dev, int clip_denoised, const float* tab_c3, float* hist_nchw, void* stream);

/* The jump of a resampled walk (RePaint's "jump", DDNM's "time travel"): with c = step2_dev[1] on entry, c in [-1, rows - 2], and
 * r = c + 1, every one of the batch * elems_per_image values becomes  x = (ra[r] x) + (rs[r] z)  and step2_dev[1] = to[r]: the chain
 * is diffused forward from the level of counter c to that of counter to[r] > c (ra = sqrt(abar(to) / abar(c)), rs = sqrt(1 - ra^2),
 * the host's, in double, rounded once).  tab_ra / tab_rs (float) and tab_to (int): `rows` entries each on the device; a row at which
 * no jump is defined holds ra = 1, rs = 0, to = c, so a launch there changes nothing; a counter outside [-1, rows - 2] touches
 * nothing at all.  z is required.  step2_dev[0] is scratch.  Two launches.
 * SR3_E_BADARG: NULL pointer, non-positive rows / batch / elems_per_image, x or step2_dev overlapping another argument;
 * SR3_E_UNSUPPORTED: batch * elems_per_image >= 2^31. */
int sr3_travel_back_f32(float* x, const float* z, const float* tab_ra, const float* tab_rs, const int* tab_to, int rows, int* step2_dev,
                        int batch, int elems_per_image, void* stream);

/* ---- back-projection sampling (engine extension; no reference counterpart) -----------------------
 * Iterative back-projection (Irani & Peleg 1991; the low-pass swap of ILVR, Choi et al. 2021, applied to x0) in the tail of a reverse
 * step, under the resize the datasets are made with: Pillow's antialiased bicubic / bilinear resample, as fp32 planes.  A resample of
 * one axis (in -> out elements) is given by two tables the HOST computes (sr3_hip.diffusion.resample_tables: Pillow's precompute_coeffs
 * in float64, rounded once): bounds, int [out, 2] = (first tap, count), and weights, float [out, ksize], zero past the count.  One
 * output value is  acc = +0 ; for t ascending: acc = acc + src[first + t] * w[t], every product and every sum rounded separately (no
 * fma), one thread per value, no atomics: bitwise reproducible.  (first, count) are clamped on the device -- first into [0, in], count
 * into [0, min(ksize, in - first)] -- so no table can take a kernel outside its tensors.  No host synchronisation, no allocation:
 * capturable. */

/* dst [planes, out_height, out_width] = the resample of src [planes, height, width]: the horizontal pass into tmp [planes, height,
 * out_width], then the vertical pass (Pillow's order).  *_dev: device tables; bounds_h_host / bounds_v_host: optional host copies of the
 * bounds, checked before the launch (every row inside [0, in] with 1 <= count <= ksize).  Any alignment (the vertical pass moves 16
 * bytes a thread where out_width % 4 == 0 and tmp and dst are 16-byte aligned; the same bits otherwise).  Two launches.
 * SR3_E_BADARG (the message names the argument): NULL src / dst / tmp / device table, non-positive size, ksize_h / ksize_v < 1, dst or
 * tmp overlapping src, each other or a table, a bad host bounds row; SR3_E_UNSUPPORTED: planes * height * width (or the element count
 * of tmp or dst) >= 2^31.  Nothing is launched on a refusal. */
int sr3_resample_f32(const float* src, int planes, int height, int width, float* dst, int out_height, int out_width,
                     const int* bounds_h_dev, const float* weights_h_dev, int ksize_h, const int* bounds_v_dev,
                     const float* weights_v_dev, int ksize_v, float* tmp, const int* bounds_h_host, const int* bounds_v_host,
                     void* stream);

/* bytes of scratch sr3_backproject_step needs (x0, the horizontal pass's intermediate, the LR residual); 0 for sizes the step refuses */
size_t sr3_backproject_scratch_bytes(int batch, int channels, int height, int width, int scale);

/* The tail of one back-projected reverse step, in place on x_nchw [batch, channels, height, width], with j = step2_dev[1] on entry,
 * s = scale, y = y_lr [batch, channels, height / s, width / s] the LR target, D the resample (height, width) -> (height / s, width / s)
 * of the down_* tables and U the resample back of the up_* tables (each as sr3_resample_f32 defines it):
 *   x0 = a[j] x - b[j] eps ; clamp(-1, 1) if clip_denoised                  (clamp first, as sr3_consistent_step)
 *   `iterations` times:   r = y - D(x0) ;  x0 = x0 + strength * U(r)        (each operation rounded separately)
 *   x  = ((c1[j] x0 + c2[j] x) + c3[j] hist) + sigma[j] z ; hist <- x0      (sr3_p_sample_step_hist's operations and association;
 *                                                                            tab_c3 / hist_nchw both NULL: no history term)
 * step2_dev[1] = j - 1 on completion (step2_dev[0] is scratch, as in sr3_tiled_step).  A contraction towards D(x0) = y, not a projection:
 * the residual shrinks with every iteration and does not vanish.  eps_nchw is the network's output for this step (sr3_unet_forward with
 * step_dev = step2_dev + 1); z_nchw: the step's noise or NULL (= 0); tab_*: as sr3_reverse_step.  scratch: the caller's,
 * sr3_backproject_scratch_bytes bytes, written before it is read.  2 + 3 * iterations launches; bitwise reproducible.  Any alignment
 * (width % 4 != 0 or a pointer off a 16-byte boundary takes the one-element-per-thread form, the same bits).
 * SR3_E_BADARG (the message names the argument): NULL required pointer, non-positive size, scale < 2 or not dividing both height and
 * width, iterations outside 1..16, strength NaN or outside (0, 2), a ksize < 1, only one of tab_c3 / hist_nchw, hist_nchw overlapping
 * x_nchw or eps_nchw, NULL or too small scratch, anything written (x_nchw, hist_nchw, scratch, step2_dev) overlapping another argument;
 * SR3_E_ALIGN: scratch not 4-byte aligned; SR3_E_UNSUPPORTED: batch * channels * height * width >= 2^31.  Nothing is launched on a
 * refusal. */
int sr3_backproject_step(float* x_nchw, const float* eps_nchw, const float* z_nchw, const float* y_lr, int batch, int channels, int height,
                         int width, int scale, int iterations, float strength, const int* down_bounds_h, const float* down_weights_h,
                         int down_ksize_h, const int* down_bounds_v, const float* down_weights_v, int down_ksize_v,
                         const int* up_bounds_h, const float* up_weights_h, int up_ksize_h, const int* up_bounds_v,
                         const float* up_weights_v, int up_ksize_v, const float* tab_a, const float* tab_b, const float* tab_c1,
                         const float* tab_c2, const float* tab_sigma, int* step2_dev, int clip_denoised, const float* tab_c3,
                         float* hist_nchw, void* scratch, size_t scratch_bytes, void* stream);

/* ---- guided sampling (engine extension; no reference counterpart) --------------------------------
 * Classifier-free guidance (Ho & Salimans 2022) and dynamic thresholding (Saharia et al. 2022, section 2.3) in the tail of a reverse
 * step, and the conditioning dropout that trains a model for guidance.  Every entry checks its arguments on the host, names the
 * offending one in sr3_last_error and launches nothing on a refusal; SR3_E_UNSUPPORTED: batch * (values per image) >= 2^31.  No host
 * synchronisation, no allocation: capturable; the scratch is the caller's and initialised by the call's own kernels.  Integer counters
 * only: bitwise reproducible. */

/* dst[b] = keep_dev[b] ? src[b] : +0.0 for the `batch` images of `elems_per_image` values (keep_dev: `batch` int32 on the device): a bit
 * copy of the kept images.  dst == src is the in-place form; any alignment (elems_per_image % 4 == 0 and both pointers 16-byte aligned
 * take the 16-byte form, the same bits).  SR3_E_BADARG: NULL pointer, non-positive size, dst overlapping src partially or keep_dev. */
int sr3_cond_drop_f32(const float* src, const int* keep_dev, int batch, int elems_per_image, float* dst, void* stream);

/* Self-conditioning (Chen et al. 2022, "Analog Bits", section 3.2): the network's own estimate of x0, written into `channels` channels of
 * its conditioning tensor for the next forward to read.
 *   x0 = a[row] x - b[row] out ; clamp(-1, 1) if clip        (sr3_p_sample_step's operations: every product and the difference rounded
 *                                                             separately in fp32 -- bit for bit the x0 a step tail forms from the same x, out)
 *   dst[b][dst_first_channel + c] = keep_dev[b] ? x0[b][c] : +0.0      for c < channels; every other channel of dst is left untouched
 * x_nchw, out_nchw: [batch, channels, height, width]; dst_nchw: [batch, dst_channels, height, width].  step_dev non-NULL: row = *step_dev
 * for the whole batch, read on the device -- the sampling form: capturable, behind sr3_unet_forward and in front of the step's tail, which
 * alone moves the counter.  step_dev NULL: row = b, tab_a / tab_b hold `batch` rows -- the training form, coefficients per image.
 * keep_dev: `batch` int32 on the device, or NULL (every image kept); a dropped image's x and out are not read.  width % 4 == 0 with
 * x_nchw, out_nchw and dst_nchw 16-byte aligned takes the 16-byte form, anything else the one-element form: the same bits.  Plain
 * stores, no atomics, no host synchronisation.  SR3_E_BADARG: NULL x_nchw / out_nchw / tab_a / tab_b / dst_nchw, non-positive batch,
 * channels, height, width or dst_channels, negative dst_first_channel, dst_first_channel + channels > dst_channels, dst_nchw overlapping
 * any other argument; SR3_E_UNSUPPORTED: batch * dst_channels * height * width >= 2^31.  Each message names the argument; nothing is
 * launched on a refusal. */
int sr3_selfcond_x0_f32(const float* x_nchw, const float* out_nchw, const float* tab_a, const float* tab_b, const int* step_dev,
                        const int* keep_dev, int clip, int batch, int channels, int height, int width, float* dst_nchw,
                        int dst_channels, int dst_first_channel, void* stream);

/* Noise conditioning augmentation (Ho et al. 2021, "Cascaded Diffusion Models", section 4.2; Sahak et al. 2023): the conditioning image
 * diffused to a level of its own, written into `channels` channels of the tensor the network reads, with the level as one more plane.
 *   aug = s[b] == 0 ? src : a[b] src + s[b] eps              (both products and the sum rounded separately in fp32, no contraction;
 *                                                             s = the noise's standard deviation, a = sqrt(1 - s^2), both the host's)
 *   dst[b][dst_first_channel + c]        = keep_dev[b] ? aug  : +0.0      for c < channels
 *   dst[b][dst_first_channel + channels] = keep_dev[b] ? s[b] : +0.0      with level_channel != 0 only
 * and every other channel of dst is left untouched.  src_nchw, eps_nchw: [batch, channels, height, width]; dst_nchw: [batch,
 * dst_channels, height, width]; a_dev, s_dev: `batch` fp32 on the device; keep_dev: `batch` int32 on the device, or NULL (every image
 * kept).  eps_nchw NULL is the form that reads no noise: the channels are copied (a_dev is not read and may be NULL), the level plane is
 * still s.  An image at s[b] == 0 is a bit copy of src and its eps is not read; a dropped image's src and eps are not read, and its level
 * plane is +0.0 too -- the all-zero tensor the second forward of a guided step reads.  height * width % 4 == 0 with src_nchw, eps_nchw
 * and dst_nchw 16-byte aligned takes the 16-byte form, anything else the one-element form: the same bits.  One launch, plain stores, no
 * atomics, no host synchronisation.  Checked in this order, nothing launched on a refusal, each message names the argument --
 * SR3_E_BADARG: NULL src_nchw / s_dev / dst_nchw, NULL a_dev with eps_nchw given, non-positive batch, channels, height or width,
 * non-positive dst_channels, negative dst_first_channel, dst_first_channel + channels (+ 1 with the level channel) > dst_channels;
 * SR3_E_UNSUPPORTED: batch * dst_channels * height * width >= 2^31; SR3_E_BADARG: dst_nchw overlapping any other argument. */
int sr3_cond_augment_f32(const float* src_nchw, const float* eps_nchw, const float* a_dev, const float* s_dev, const int* keep_dev,
                         int level_channel, float* dst_nchw, int dst_channels, int dst_first_channel, int batch, int channels,
                         int height, int width, void* stream);

/* out_dev[b] = the abs-quantile of the n values of image b of src [batch, n]: with v_lo, v_hi the rank_lo-th and (rank_lo + 1)-th
 * smallest |src[b][i]| (0-based; v_hi = v_lo when rank_lo == n - 1),
 *   out_dev[b] = (float)((double) v_lo + frac * ((double) v_hi - (double) v_lo))        one rounding
 * (v_lo itself where v_hi == v_lo or frac == 0: the formula's value for finite data, and no inf - inf for an infinite v_lo).  The host
 * derives the ranks from a percentile p in float64: pos = p (n - 1), rank_lo = floor(pos), frac = pos - rank_lo.  The selection is
 * exact -- a radix select on the bit patterns  bits & 0x7fffffff, which order like the values: ties, +-0, denormals and +-inf come out
 * exactly; a NaN sorts above inf.  n <= 8192: one workgroup per image, one launch, the scratch is not touched; larger: five launches,
 * 4096 values per workgroup.  Any n >= 1, any alignment of src.
 * scratch: sr3_abs_quantile_scratch_bytes(batch, n) bytes (0 for arguments the call would refuse), 4-byte aligned, contents arbitrary.
 * SR3_E_BADARG: NULL src / out_dev / scratch, non-positive size, rank_lo outside [0, n), frac outside [0, 1), scratch_bytes too small,
 * out_dev or scratch overlapping src or each other; SR3_E_ALIGN: scratch not 4-byte aligned. */
size_t sr3_abs_quantile_scratch_bytes(int batch, int n);
int sr3_abs_quantile_f32(const float* src, int batch, int n, int rank_lo, double frac, float* out_dev, void* scratch, size_t scratch_bytes,
                         void* stream);

/* The tail of one guided reverse step, in place on x_nchw [batch, channels, height, width], with j = step2_dev[1] on entry and
 * n = channels * height * width:
 *   out = out_c                                            (out_u NULL)
 *   out = out_u + scale * (out_c - out_u)                  (out_c / out_u: the network's output on the real / on a zero condition)
 *   x0  = a[j] x - b[j] out
 *   mode 0: x0' = x0 ;  mode 1: x0' = clamp(x0, -1, 1)     (= clip_denoised)
 *   mode 2: s_b = max(1, abs-quantile of image b's x0 at (rank_lo, frac), as sr3_abs_quantile_f32) ; x0' = clamp(x0, -s_b, s_b) / s_b
 *   x   = ((c1[j] x0' + c2[j] x) + c3[j] hist) + sigma[j] z ; hist <- x0'      (tab_c3 / hist_nchw both NULL: no history term)
 * every fp32 product, sum, difference and quotient rounded separately.  step2_dev[1] = j - 1 on completion (step2_dev[0] is scratch, as
 * in sr3_tiled_step: only the last kernel writes slot 1).  z_nchw: the step's noise or NULL (= 0); tab_*: as sr3_reverse_step.
 * Mode 2 only: x0_scratch [batch, channels, height, width] and q_scratch of sr3_abs_quantile_scratch_bytes(batch, n) bytes.
 * thr_out_dev [batch] or NULL: receives s_b (mode 2) or 1.0.  Modes 0 and 1: two launches; mode 2: the counter copy, x0 into
 * x0_scratch, the select's launches on it, the mix.  width % 4 == 0 and 16-byte aligned pointers take four values per thread, anything
 * else one, the same bits.  out_u NULL in mode 1 is sr3_p_sample_step_hist + sr3_step_decrement, bit for bit.
 * SR3_E_BADARG: NULL required pointer, non-positive size, mode outside 0..2, scale not finite, only one of tab_c3 / hist_nchw; mode 2:
 * rank_lo outside [0, n), frac outside [0, 1), x0_scratch / q_scratch NULL or q_scratch_bytes too small; anything the step writes
 * (x_nchw, hist_nchw, x0_scratch, q_scratch, thr_out_dev) overlapping another argument. */
int sr3_guided_step(float* x_nchw, const float* out_c, const float* out_u, float scale, const float* z_nchw, int batch, int channels,
                    int height, int width, const float* tab_a, const float* tab_b, const float* tab_c1, const float* tab_c2,
                    const float* tab_sigma, const float* tab_c3, float* hist_nchw, int* step2_dev, int mode, int rank_lo, double frac,
                    float* x0_scratch, void* q_scratch, size_t q_scratch_bytes, float* thr_out_dev, void* stream);

/* ---- learned reverse-process variance (engine extension; Nichol & Dhariwal 2021, "Improved DDPM") ------------------------
 * The tail of an ancestral step whose sigma the network predicts.  out_nchw [batch, 2 * channels, height, width]: the prediction
 * channels, then the raw variance channels v (sr3_unet_forward_full).  With j = step2_dev[1] on entry:
 *   x0    = a[j] x - b[j] out_c ; clamp(-1, 1) if clip_denoised
 *   mean  = c1[j] x0 + c2[j] x                                   (bit-identical to sr3_p_sample_step's mean)
 *   f     = (v + 1) / 2 ; sigma = exp((f * tab_log_beta[j] + (1 - f) * tab_log_beta_tilde[j]) / 2), 0 where tab_sigma[j] == 0
 *   x     = mean + sigma z                                       (z_nchw NULL: zeros)
 * every product, sum and difference of the mean and of sigma z rounded separately; sigma itself is plain fp32.  step2_dev[1] = j - 1
 * on completion (step2_dev[0] is scratch, as in sr3_tiled_step).  Two launches (the counter copy, the tail); height * width % 4 == 0
 * and 16-byte aligned pointers take four values per thread, anything else one, the same bits.  Capturable.  The arguments are checked
 * in this order and nothing is launched on a refusal: a NULL required pointer (SR3_E_BADARG, named); a non-positive size
 * (SR3_E_BADARG); 2 * batch * channels * height * width >= 2^31 (SR3_E_UNSUPPORTED); tab_c3 or hist_nchw given (SR3_E_UNSUPPORTED: a
 * multistep rule has no learned-variance form); x_nchw or step2_dev overlapping another argument (SR3_E_BADARG). */
int sr3_learned_var_step(float* x_nchw, const float* out_nchw, const float* z_nchw, int batch, int channels, int height, int width,
                         const float* tab_a, const float* tab_b, const float* tab_c1, const float* tab_c2, const float* tab_sigma,
                         const float* tab_log_beta, const float* tab_log_beta_tilde, int* step2_dev, int clip_denoised,
                         const float* tab_c3, float* hist_nchw, void* stream);

/* ---- progressive distillation (engine extension; no reference counterpart) ------------------------
 * Salimans & Ho 2022: a frozen teacher takes two deterministic DDIM steps, the student learns to land on the same point in one.  The two
 * entries are the elementwise passes between the teacher's forwards (sr3_unet_forward) and the student's step (sr3_train_step_ex).
 * Images are [batch, elems_per_image] fp32; every coefficient is a device array of `batch` fp32 values the host computed in float64
 * and rounded once.  Every product, sum and difference is rounded separately; no division, no atomics: bitwise reproducible.  One
 * launch each; elems_per_image % 4 == 0 and 16-byte aligned image pointers take four values per thread, anything else one, the same
 * bits.  No host synchronisation, no allocation: capturable.  The arguments are checked on the host, the offending one is named in
 * sr3_last_error and nothing is launched on a refusal.  SR3_E_BADARG: NULL required pointer, non-positive size, a non-finite scale
 * with out_u given, an output overlapping an input or the other output; SR3_E_UNSUPPORTED: batch * elems_per_image >= 2^31. */

/* One teacher step:
 *   out    = out_c                                  (out_u NULL)
 *   out    = out_u + scale * (out_c - out_u)        (out_c / out_u: the output on the real / on a zero condition; sr3_guided_step's)
 *   x0     = a[b] x - b[b] out ; clamp(-1, 1) if clip_denoised
 *   x0_out <- x0 ;  x_next <- c1[b] x0 + c2[b] x
 * x_next == x is the in-place form (allowed; a partial overlap is not). */
int sr3_teacher_step_f32(const float* x, const float* out_c, const float* out_u, float scale, const float* a, const float* b,
                         const float* c1, const float* c2, int batch, int elems_per_image, int clip_denoised, float* x_next,
                         float* x0_out, void* stream);

/* The teacher's second step fused with the student's regression target (the point the teacher lands on is never written):
 *   x0b     = clamp?(a[b] x_mid - b[b] out)         (out combined as above)
 *   x_tgt   <- w1[b] x0_first + w2[b] x0b           (w1 + w2 = 1: a convex combination of the teacher's two x0 predictions)
 *   eps_tgt <- s1[b] z_t - s2[b] x_tgt              (s1 = 1 / sigma_t, s2 = alpha_t / sigma_t: z_t = alpha_t x_tgt + sigma_t eps_tgt) */
int sr3_distill_target_f32(const float* z_t, const float* x_mid, const float* out_c, const float* out_u, float scale,
                           const float* x0_first, const float* a, const float* b, const float* w1, const float* w2, const float* s1,
                           const float* s2, int batch, int elems_per_image, int clip_denoised, float* x_tgt, float* eps_tgt,
                           void* stream);

/* q_sample (model/sr3_modules/diffusion.py:212-219; model/ddpm_modules/diffusion.py:259-267):
 * out = ca[b] * x0 + cb[b] * z */
int sr3_q_sample(const float* x0, const float* z, const float* ca, const float* cb, int batch,
                 int elems_per_image, float* out, void* stream);

/* ---- training step ------------------------------------------------------------------------- */

/* Workspace of sr3_train_step (activations kept for the backward, their gradient mirror, scratch) at the plan's geometry.  Without plan
 * option train_geom training runs at image_size x image_size only: 0 (and a message) while sr3_plan_set_geometry has the plan at
 * another geometry; with it, 0 only for a geometry no kernel can run (an attention level beyond the score strip without attn_long).
 * The buffer contract at sr3_workspace_bytes holds: exactly this many bytes, nothing outside them written, prior contents irrelevant
 * (the activation-gradient mirror is not zeroed: every tensor's first writer stores). */
size_t sr3_train_workspace_bytes(sr3_plan* plan, int batch, int cond_channels);

/* One training step up to the gradients: `l_pix = netG(data); l_pix.backward()` of
 * DDPM.optimize_parameters (model/model.py:50-54) over GaussianDiffusion.p_losses
 * (model/sr3_modules/diffusion.py:221-246, model/ddpm_modules/diffusion.py:278-294):
 *   x_noisy = q_ca[b] * hr + q_cb[b] * z ; eps = UNet(cat(cond, x_noisy), level) ;
 *   *loss_sum_out = sum |z - eps| ; grads = d(grad_scale * loss_sum) / d params
 * (grad_scale = 1 / (b*c*h*w), model.py:52-53).  The random draws (t / gamma, z) are made by the caller
 * (torch / numpy RNG, as in the reference) and passed in.  `grads` has the layout of the parameter
 * arena and is overwritten: every float of [0, sr3_plan_param_floats) is written, whatever the arena held (NaN included).  That covers
 * the arena's padding floats, which belong to no parameter -- the output conv's bias slot is 4 floats wide (8 with a variance head) and
 * receives the column sums of all lanes of dOut, whose pad lanes are 0: they come out +0, so sr3_grad_norm and the Adam entries can take
 * the whole arena length.  dropout_p > 0 applies nn.Dropout(p) between Swish and the conv of every
 * block2 (unet.py:83-88,100-101) with a counter-based mask: activated element i (NHWC linear index) of
 * the block with FiLM row offset k is kept iff hash32(i*0x9E3779B9 + dropout_seed + (k+1)*0x632BE5AB) >=
 * p*2^32 and scaled by 1/(1-p); the mask is regenerated, never stored, by the backward.
 * Gradient-ready marks (data-parallel overlap): mark_offsets[k] (descending arena offsets) / mark_events[k]
 * (hipEvent_t): event k is recorded on `stream` as soon as the gradient of every parameter at arena offset
 * >= mark_offsets[k] has been enqueued, so a communication stream can all-reduce that tail bucket while the
 * rest of the backward still runs (replaces nn.DataParallel's reduce_add, model/networks.py:113-115). */
int sr3_train_step(sr3_plan* plan, const float* hr_nchw, const float* cond_nchw, int cond_channels,
                   const float* z_nchw, const float* q_ca, const float* q_cb, const float* noise_level,
                   const int64_t* timestep, const float* freq, const float* params, float* grads,
                   void* workspace, size_t workspace_bytes, float* loss_sum_out, float grad_scale, float dropout_p,
                   unsigned dropout_seed, int n_marks, const size_t* mark_offsets, void* const* mark_events,
                   int batch, void* stream);

/* sr3_train_step under another training objective (no counterpart in the reference, whose network predicts the noise under an
 * unweighted L1 / L2): per image b the regression target is tgt_z[b] * z + tgt_x0[b] * hr and the loss weight is weight[b],
 *   d = (tgt_z[b] * z + tgt_x0[b] * hr) - out ;  *loss_sum_out = sum weight[b] * rho(d) ;  grads = d(grad_scale * that) / d params.
 * tgt_z / tgt_x0 / weight: `batch` floats each on the device, all three or none (all NULL: target z, weight 1).  v-prediction
 * (Salimans & Ho 2022) is tgt_z = sqrt(abar), tgt_x0 = -sqrt(1 - abar); x0-prediction is (0, 1); Min-SNR-gamma weights (Hang et
 * al. 2023) go in `weight` (sr3_hip.diffusion.prediction_coefs / loss_weights compute them).
 * loss_kind: -1 the plan's loss_l2 option; 0 L1, rho = |d| (gradient 0 at d = 0); 1 L2, rho = d^2; 2 Huber, rho = d^2 / 2 for
 * |d| <= huber_delta, else huber_delta * (|d| - huber_delta / 2) (torch.nn.HuberLoss(reduction='sum', delta)); huber_delta is read
 * with loss_kind 2 only.  With the pointers NULL and loss_kind -1 / 0 / 1 the launches are sr3_train_step's, which IS this call with
 * (NULL, NULL, NULL, -1, 0).  The loss sum keeps its fixed-order two-stage reduction in double: no atomics, the same bits every run.
 * SR3_E_BADARG (nothing is launched, the message names the argument): only some of tgt_z / tgt_x0 / weight given, loss_kind
 * outside -1..2, loss_kind 2 with a huber_delta that is not finite and > 0. */
int sr3_train_step_ex(sr3_plan* plan, const float* hr_nchw, const float* cond_nchw, int cond_channels,
                      const float* z_nchw, const float* q_ca, const float* q_cb, const float* noise_level,
                      const int64_t* timestep, const float* freq, const float* params, float* grads,
                      void* workspace, size_t workspace_bytes, float* loss_sum_out, float grad_scale, float dropout_p,
                      unsigned dropout_seed, int n_marks, const size_t* mark_offsets, void* const* mark_events,
                      int batch, const float* tgt_z, const float* tgt_x0, const float* weight, int loss_kind,
                      float huber_delta, void* stream);

/* The loss kernel of sr3_train_step_ex alone, on caller-owned tensors: z, out (the network output) and hr are NCHW
 * [batch][channels][pixels], channels 1..4; g_nhwc4 [batch][pixels][4] receives -weight[b] * rho'(d) * scale with the lanes
 * >= channels written 0, *loss_sum_out the weighted loss sum.  tgt_z / tgt_x0 / weight as above (hr_nchw may be NULL when they
 * are); loss_kind 0..2 (there is no plan to defer to).  scratch: sr3_loss_grad_scratch_bytes() bytes, 8-byte aligned (the blocks'
 * partial sums).  SR3_E_BADARG as above, and for a NULL tensor, batch / pixels <= 0, channels outside 1..4; SR3_E_ALIGN for a
 * misaligned scratch. */
size_t sr3_loss_grad_scratch_bytes(void);
int sr3_loss_grad_f32(const float* z_nchw, const float* out_nchw, const float* hr_nchw, const float* tgt_z,
                      const float* tgt_x0, const float* weight, int batch, int channels /* 1..4 */, int pixels,
                      int loss_kind, float huber_delta, float scale, float* g_nhwc4, float* loss_sum_out,
                      void* scratch /* sr3_loss_grad_scratch_bytes() */, void* stream);

/* sr3_train_step_ex of a plan with a variance head (plan option var_channels; out_channel = 2 C): the hybrid loss
 * L_simple + vlb_lambda * L_vlb of Nichol & Dhariwal 2021 in place of the pixel loss.  step_scalars: per image 8 floats on the device,
 *   {a, b, c1, c2, log beta, log beta~, last, 0}:  x0^ = a x_t - b out_c (not clamped) ; mu_theta = c1 x0^ + c2 x_t, a constant -- no
 *   L_vlb gradient reaches the prediction rows ; mu_q = c1 hr + c2 x_t ; log sigma_theta^2 = f log beta + (1 - f) log beta~ with
 *   f = (v + 1) / 2 ; last != 0 marks the walk's last step.  Per element, in bits:
 *     not last:  KL(N(mu_q, beta~) || N(mu_theta, sigma_theta^2)) / ln 2
 *     last:      -log2 of the mass of N(mu_theta, sigma_theta^2) on the bin hr +- 1/255 (open below -0.999 and above 0.999), with
 *                Phi(u) = (1 + tanh(sqrt(2 / pi) (u + 0.044715 u^3))) / 2 and logs of max(., 1e-12)
 *   *loss_sum_out = sum weight[b] rho(d) + vlb_lambda * sum vlb  (so one grad_scale = 1 / (b c h w) makes both terms means) ;
 *   *vlb_sum_out (may be NULL) = sum vlb.  The prediction rows' loss and gradient are sr3_train_step_ex's, term for term; the variance
 *   rows receive vlb_lambda * grad_scale * d vlb / d v in closed form.  Fixed-order two-stage sums in double: the same bits every run.
 * SR3_E_BADARG besides sr3_train_step_ex's: step_scalars NULL, a plan without var_channels (and sr3_train_step / _ex on a plan with
 * it), vlb_lambda negative or not finite. */
int sr3_train_step_ex2(sr3_plan* plan, const float* hr_nchw, const float* cond_nchw, int cond_channels,
                       const float* z_nchw, const float* q_ca, const float* q_cb, const float* noise_level,
                       const int64_t* timestep, const float* freq, const float* params, float* grads,
                       void* workspace, size_t workspace_bytes, float* loss_sum_out, float grad_scale, float dropout_p,
                       unsigned dropout_seed, int n_marks, const size_t* mark_offsets, void* const* mark_events,
                       int batch, const float* tgt_z, const float* tgt_x0, const float* weight, int loss_kind,
                       float huber_delta, const float* step_scalars, float vlb_lambda, float* vlb_sum_out, void* stream);

/* The loss kernel of sr3_train_step_ex2 alone: out_nchw is [batch][2 * channels][pixels], z / hr / xt [batch][channels][pixels],
 * channels 1..4; g_nhwc8 [batch][pixels][8]: lanes 0 .. channels - 1 as sr3_loss_grad_f32's (bit-identical), lanes channels ..
 * 2 * channels - 1 = vlb_lambda * scale * d vlb / d v, the rest 0.  scratch: sr3_hybrid_loss_grad_scratch_bytes() bytes, 8-byte
 * aligned.  Refusals as sr3_loss_grad_f32's, and for a NULL hr / xt / step_scalars or a vlb_lambda that is negative or not finite. */
size_t sr3_hybrid_loss_grad_scratch_bytes(void);
int sr3_hybrid_loss_grad_f32(const float* z_nchw, const float* out_nchw, const float* hr_nchw, const float* xt_nchw,
                             const float* tgt_z, const float* tgt_x0, const float* weight, const float* step_scalars,
                             float vlb_lambda, int batch, int channels /* 1..4 */, int pixels, int loss_kind, float huber_delta,
                             float scale, float* g_nhwc8, float* loss_sum_out, float* vlb_sum_out,
                             void* scratch /* sr3_hybrid_loss_grad_scratch_bytes() */, void* stream);

/* ---- the variational bound by timestep (engine extension; Nichol & Dhariwal 2021) ------------------------
 * Per-image terms of the bound from (x0, x_t, the network's output, the step's scalars): what an evaluation walk adds up to bits per
 * dimension, and what a loss-aware timestep sampler reads back from a training step.
 *   x0, x_t [batch, channels, pixels]; out [batch, out_channels, pixels]: the prediction planes, then (var_mode 0) the variance planes v
 *   table [table_rows, 8]: rows {a, b, c1, c2, log beta, log beta~ (clipped), last, 0} (sr3_train_step_ex2's step_scalars layout)
 *   the row of image b: table[rows_per_image[b]] (the training form), or table[j] for every image with j = step2_dev[1] (the evaluation
 *   form); exactly one of the two is given.  A row index outside [0, table_rows) gives that image NaN (rows_per_image) or writes no
 *   output (step2_dev); nothing is read or written out of bounds.
 *   var_mode 0: learned, out_channels = 2 * channels; 1: fixed small, v = -1 (log sigma^2 = log beta~); 2: fixed large, v = +1
 *   (log sigma^2 = log beta); out_channels = channels for 1 and 2.
 * Per element, all fp32, sr3_train_step_ex2's term in the same operation order:
 *   x0^ = a x_t - b out_c ; clamp(-1, 1) if clip_denoised ; f = (v + 1) / 2 ; lv = f log beta + (1 - f) log beta~
 *   last == 0:  vlb = (-1 + lv - log beta~ + exp(log beta~ - lv) + (c1 (x0 - x0^))^2 exp(-lv)) / 2 / ln 2
 *   last != 0:  vlb = -log2 max(mass, 1e-12), the mass of N(c1 x0^ + c2 x_t, e^lv) on the bin x0 +- 1/255 (open below -0.999 and above
 *               0.999), Phi(u) = (1 + tanh(sqrt(2 / pi) (u + 0.044715 u^3))) / 2
 *   vb_out[b] = mean over channels * pixels of vlb (bits / dim) ; x0_mse_out[b] = mean of (x0 - x0^)^2.
 * With step2_dev both outputs are [table_rows, batch] and row j is written; the second launch then sets step2_dev[1] = j - 1, so the
 * pair drives a captured loop.  step2_dev is the loops' counter pair: slot 1 is the counter; slot 0, the scratch copy of the steps that
 * begin with a copy launch (sr3_tiled_step), is neither read nor written here -- every reader of the step runs before the second
 * launch and reads slot 1.
 * Sums in double in a fixed order: 16 block partials per image into `scratch` (a thread adds its elements in index order, a block
 * folds its threads in a fixed tree), then one block adds each image's partials in index order.  No atomics: the same bits every run.
 * channels * pixels % 4 == 0 with 16-byte aligned image pointers reads 16 bytes per access, anything else one float: the same bits.
 * scratch: sr3_vlb_terms_partials_bytes(batch) bytes, 8-byte aligned; the buffer contract at sr3_workspace_bytes holds (exactly this
 * size, prior contents irrelevant).  Two launches, no host synchronisation: capturable.  Checked in this order, nothing is launched
 * on a refusal and the message names the argument: a NULL required pointer (SR3_E_BADARG); both or neither of rows_per_image /
 * step2_dev (SR3_E_BADARG); a non-positive size, var_mode outside 0..2, out_channels not matching var_mode (SR3_E_BADARG);
 * batch * out_channels * pixels >= 2^31 (SR3_E_UNSUPPORTED); scratch_bytes too small (SR3_E_NOMEM); an output, the scratch or
 * step2_dev overlapping another argument (SR3_E_BADARG); a misaligned scratch (SR3_E_ALIGN). */
size_t sr3_vlb_terms_partials_bytes(int batch);
int sr3_vlb_terms_f32(const float* x0, const float* x_t, const float* out, int out_channels, const float* table, int table_rows,
                      const int* rows_per_image, int* step2_dev, int var_mode, int clip_denoised, int batch, int channels, int pixels,
                      float* vb_out, float* x0_mse_out, void* scratch /* sr3_vlb_terms_partials_bytes(batch) */, size_t scratch_bytes,
                      void* stream);

/* The prior term of the bound: out[b] = mean over elems_per_image of KL(N(sqrt_abar x0, var) || N(0, 1)) / ln 2
 *   = (-1 - log_var + var + (sqrt_abar x0)^2) / 2 / ln 2 per element in fp32, with abar of the walk's last step: sqrt_abar = sqrt(abar),
 * var = 1 - abar, log_var = log(1 - abar), evaluated by the host in float64 and rounded once.  Reduction, scratch
 * (sr3_vlb_terms_partials_bytes(batch)), access widths and the order of the checks as sr3_vlb_terms_f32's; a scalar that is not finite
 * is SR3_E_BADARG. */
int sr3_prior_bpd_f32(const float* x0, int batch, int elems_per_image, float sqrt_abar, float var, float log_var, float* out,
                      void* scratch, size_t scratch_bytes, void* stream);

/* sr3_q_sample indexed by the device step counter, so that a captured loop can noise x0 afresh each step:
 *   out = tab_ca[j] * x0 + tab_cb[j] * z,  j = step_dev[0]
 * products and sum rounded separately: sr3_q_sample's bits with ca[b] = tab_ca[j], cb[b] = tab_cb[j].  j outside [0, table_rows)
 * writes nothing.  One launch; batch * elems_per_image % 4 == 0 with 16-byte aligned pointers takes four values per thread, anything
 * else one, the same bits.  Checks in order: NULL pointer, non-positive size (SR3_E_BADARG); batch * elems_per_image >= 2^31
 * (SR3_E_UNSUPPORTED); out overlapping an input (SR3_E_BADARG). */
int sr3_q_sample_step_f32(const float* x0, const float* z, const float* tab_ca, const float* tab_cb, int table_rows, const int* step_dev,
                          int batch, int elems_per_image, float* out, void* stream);

/* sr3_train_step_ex2 that also returns the step's per-image terms of the bound: per_image_out [batch, 2] = {vb, x0_mse} of
 * sr3_vlb_terms_f32 on the step's own x_noisy and output (clip_denoised 0, image b on row b of step_scalars), one launch pair behind the
 * loss kernel; scratch: sr3_vlb_terms_partials_bytes(batch) bytes, 8-byte aligned.  Every launch of sr3_train_step_ex2 runs unchanged,
 * so loss, vlb sum and gradients are its bits.  It also takes a plan WITHOUT a variance head: then the step is sr3_train_step_ex's
 * (vlb_lambda and vlb_sum_out are not read) and the terms are var_mode 1's; step_scalars is required either way.  per_image_out NULL:
 * sr3_train_step_ex2 / sr3_train_step_ex, the same launches.  vlb_weight (`batch` floats on the device, or NULL = 1; read with a
 * variance head only): per image, vlb_lambda * vlb_weight[b] stands where vlb_lambda does -- *loss_sum_out = sum weight[b] rho(d) +
 * vlb_lambda sum_b vlb_weight[b] vlb_b, the variance rows receive vlb_lambda vlb_weight[b] grad_scale d vlb / d v; *vlb_sum_out stays
 * the plain sum.  What an importance-sampled step needs: `weight` reaches L_simple alone, so 1 / (T p_t) goes into both tables.  NULL
 * passes the kernel the same arguments as sr3_train_step_ex2 does: the same operations, the same bits.  SR3_E_BADARG besides theirs: scratch NULL with per_image_out given,
 * per_image_out or scratch overlapping each other or the workspace; SR3_E_NOMEM: scratch_bytes too small; SR3_E_ALIGN: scratch. */
int sr3_train_step_ex3(sr3_plan* plan, const float* hr_nchw, const float* cond_nchw, int cond_channels,
                       const float* z_nchw, const float* q_ca, const float* q_cb, const float* noise_level,
                       const int64_t* timestep, const float* freq, const float* params, float* grads,
                       void* workspace, size_t workspace_bytes, float* loss_sum_out, float grad_scale, float dropout_p,
                       unsigned dropout_seed, int n_marks, const size_t* mark_offsets, void* const* mark_events,
                       int batch, const float* tgt_z, const float* tgt_x0, const float* weight, int loss_kind,
                       float huber_delta, const float* step_scalars, float vlb_lambda, float* vlb_sum_out,
                       float* per_image_out, void* scratch, size_t scratch_bytes, const float* vlb_weight, void* stream);

/* torch.optim.Adam step (model/model.py:39-40,55; defaults beta 0.9/0.999, eps 1e-8, no weight decay)
 * fused over the whole arena; `step` is the 1-based step count for the bias corrections.
 * SR3_E_BADARG (nothing is launched, the message names the argument): a NULL params / grads / exp_avg / exp_avg_sq,
 * n % 4 != 0, step < 1.  SR3_E_ALIGN (nothing is launched): a pointer that is not 16-byte aligned. */
int sr3_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, size_t n, float lr,
                  float beta1, float beta2, float eps, int step, void* stream);

/* The same Adam step with the exponential moving average (EMA) of the weights updated in the same pass over the arena
 * (config train.ema_scheduler; the SR3 paper samples from EMA weights).  params / exp_avg / exp_avg_sq come out
 * bit-identical to sr3_adam_step on the same inputs in every mode (both run one kernel template); no atomics.
 *   ema       : arena-shaped fp32 buffer, in / out; may be NULL with ema_mode 0
 *   ema_mode  : 0  no EMA work, ema is not touched;
 *               1  ema = p_new, an exact copy (the steps before step_start_ema);
 *               2  ema = ema + (p_new - ema) * w,  w = 1 - ema_decay evaluated in double from the decimal the fp32
 *                  argument stands for and rounded once to fp32 (as 1 - beta1 is); p_new == ema leaves ema unchanged
 *                  exactly.  An fp32 EMA drops an update smaller than half an ulp of ema (at decay 0.9999: a weight
 *                  that moved by less than ~6e-4 relative since the EMA last followed it).
 *   ema_decay : in [0, 1); read in mode 2 only, checked in every mode
 * SR3_E_BADARG (nothing is launched, the message names the argument): a NULL params / grads / exp_avg / exp_avg_sq,
 * NULL ema with ema_mode != 0, ema_mode outside 0..2, ema_decay outside [0, 1), n % 4 != 0, step < 1.  SR3_E_ALIGN: a
 * pointer that is not 16-byte aligned.  As with sr3_adam_step the caller invalidates the derived filters afterwards
 * (sr3_plan_invalidate_derived); filters prepared from `params` say nothing about `ema` and vice versa: a forward on
 * the EMA weights prepares them from the EMA arena (the stale-filter check (c) above compares the pointers). */
int sr3_adam_ema_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, size_t n,
                      float lr, float beta1, float beta2, float eps, int step, float ema_decay, int ema_mode,
                      void* stream);

/* Global L2 norm of the gradient arena, for clipping by it (config train.optimizer.clip_grad_norm): the device-side half of
 * torch.nn.utils.clip_grad_norm_(params, max_norm), which the reference never calls -- no counterpart there.  No host
 * synchronisation: four floats are written to out4_dev (16-byte aligned, caller-owned):
 *   [0] norm = (float)sqrt(sum g^2), the sum in double;  [1] coef = min(1, max_norm / (norm + 1e-6f)) in fp32 (torch's clip
 *   coefficient), 1 when max_norm <= 0 (norm only);  [2] 1.0f when the norm is finite, else 0.0f;  [3] 0.
 * The grid is a compile-time constant (at most 512 blocks of 256 threads) and every sum has one order (thread: stride order;
 * wave: xor shuffle; block: waves in order; blocks in index order), no atomics: the same bits on every run and every device.
 * scratch: the blocks' partial sums, 8-byte aligned; the byte count comes from the query below (at most 4096).
 * SR3_E_BADARG (nothing is launched, the message names the argument): NULL grads / scratch / out4_dev, n % 4 != 0, a NaN
 * max_norm, scratch_bytes too small.  SR3_E_ALIGN: grads or out4_dev not 16-byte aligned, scratch not 8-byte aligned. */
size_t sr3_grad_norm_scratch_bytes(size_t n);
int sr3_grad_norm(const float* grads, size_t n, float max_norm, void* scratch, size_t scratch_bytes, float* out4_dev,
                  void* stream);

/* Gradient accumulation over micro-batches (config train.optimizer.accumulate; the reference steps once per loader batch -- no
 * counterpart; what `loss.backward()` called K times without zero_grad() does to .grad in torch): acc = first ? g : acc + g,
 * one fp32 add per element.  out4_dev != NULL: the norm / coef / flag of the RESULT as above, from the same pass -- bit-equal
 * to the stand-alone norm entry on acc afterwards (same grid, same order); scratch / scratch_bytes / max_norm are read only
 * then.  SR3_E_BADARG: NULL acc / g, n % 4 != 0, and with out4_dev the refusals of the norm entry.  SR3_E_ALIGN as there. */
int sr3_grad_accumulate(float* acc, const float* g, size_t n, int first, float max_norm, void* scratch,
                        size_t scratch_bytes, float* out4_dev, void* stream);

/* sr3_adam_ema_step with the gradient scaled by scale4_dev[1] and the whole update skipped when scale4_dev[2] == 0 (scale4_dev:
 * the four floats the two entries above write; no counterpart in the reference, which neither clips nor guards).  The scaled
 * gradient is an fp32 product rounded on its own, so with coef == 1.0f params / exp_avg / exp_avg_sq / ema come out bit-identical
 * to the unscaled entry, and with coef < 1 bit-identical to it on a gradient multiplied by coef in fp32 beforehand.  Flag 0 (a
 * non-finite norm): nothing is written, every buffer keeps its bits -- where torch's clip_grad_norm_ would write NaN.
 * Arguments and refusals as the unscaled entry; in addition SR3_E_BADARG for a NULL scale4_dev and SR3_E_ALIGN when it is not
 * 16-byte aligned.  `step` is the host's count: it advances on a skipped step too (no host synchronisation). */
int sr3_adam_ema_step_scaled(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, size_t n,
                             float lr, float beta1, float beta2, float eps, int step, float ema_decay, int ema_mode,
                             const float* scale4_dev, void* stream);

/* ---- per-op entry points (unit tests, micro-benchmarks) ------------------------------------ */

/* Block / Conv2d / Downsample / Upsample / res_conv / qkv / out as one implicit-GEMM call:
 * NHWC in/out, input = virtual concat (src0|src1), optional x2 nearest upsample, stride 1|2,
 * ksize 1|3 (pad ksize/2), prologue act 0 none | 1 x*scale+shift | 2 silu(x*scale+shift) with
 * ss[B][Cin][2]; epilogue + bias + film[b*film_stride+n] + residual (res0|res1 concat view).
 * weights OHWI.  tile_cfg/ksplit 0 = auto (direct kernels only); tile_cfg 11 = Winograd F(2x2,3x3) (3x3 stride 1, H and W
 * multiples of 16, or 8x8 maps with B % 4 == 0 -- four images per workgroup tile, split-K only; the transformed filters are
 * derived into `scratch` by this entry point); tile_cfg 12 = the same kernel's 3 x bf16 split instantiation (one-image tile
 * only, and the four-image tile of the 8x8 maps; what plan option wino_split selects there), 13 = the same arithmetic as two
 * four-wave workgroups per CU on an 8 x 16 pixel tile (conv3x3_wino2.hip; W >= 16 and a multiple of 16, H a multiple of 8, no
 * dropout form; what plan option wino2 -- default on -- selects on maps >= 16 wide), 23 = that kernel's ragged instantiation: any
 * map size (tile grid ceil(W / 16) x ceil(H / 8), the overhang masked; same arithmetic, same filters; on a map that is a whole
 * multiple of the tile the bits of 13; what plan option wino_ragged selects at a non-native geometry); with ups = 1, 13 and 23 run
 * the nine Winograd positions whose operand is not identically zero on a nearest x2 map, and 25 / 26 = 13 / 23 with all sixteen
 * positions (same bits; what plan option wino_up = 0 selects; without upsampling 25 / 26 are 13 / 23); tile_cfg 1-4 = the
 * im2col kernel's 128x128 / 128x64 / 64x64 / 64x128 tiles on the exact-fp32 MFMA, 14-17 = the same tiles on the 3 x bf16 split
 * instantiation with both operands split while they are staged (what plan option gemm_split selects: what a plan runs), 18-21 =
 * the same with the weights pre-split into bf16 planes in MFMA fragment order and read straight from global memory (plan option
 * gemm_wpre, default off: a plan keeps the planes in its derived buffer; this entry point derives them into `scratch`; results
 * are bit-identical to 14-17); 22 = the plain GEMM kernel of gemm1x1.hip (what plan options gemm2 / gemm_s2 -- default on -- select: 1x1
 * stride 1, or 3x3 stride 2 with one source, act 0 and an even map; no upsampling, Cout % 64 == 0, C0 and C1 % 32 == 0,
 * Ho * Wo % 32 == 0, B * Ho * Wo a multiple of the tile's rows (sr3_gemm_tile: 64, or 32 where the 32-row tile runs), act 0 | 1; anything else is refused with "does not fit"; same pre-split weights as
 * 18-21, derived into `scratch`), with the epilogue a fresh plan runs; 27 / 28 / 29 = 22 with the epilogue of plan option
 * gemm_epi = 0 / 1 / 2 named explicitly (4-byte stores / 16-byte loads and stores behind a transpose through LDS / those stores
 * written through L2; same bits; 28 and 29 need RC0 % 4 == 0, film_stride % 4 == 0 and 16-byte aligned bias, film, res0, res1, out).
 * scratch: split-K slabs (+ the Winograd filters for tile_cfg 11-13 and 23, the pre-split weights for 18-22 and 27-29), sized by
 * sr3_conv_scratch_bytes, 256-byte aligned (SR3_E_ALIGN otherwise, for the three conv entries).  For this and every per-op scratch
 * below the buffer contract at sr3_workspace_bytes holds: exactly the queried bytes, nothing outside them written, prior contents
 * irrelevant (split-K slabs, statistics slices and padded lanes are written before they are read). */
int sr3_conv_f32(const float* src0, int C0, const float* src1, int C1, int B, int Hs, int Ws, int ups,
                 int stride, int ksize, int Cout, const float* w_ohwi, const float* bias, const float* ss,
                 int act, const float* film, int film_stride, const float* res0, int RC0, const float* res1,
                 int RC1, float* out, double* out_stats, int tile_cfg, int ksplit, void* scratch,
                 size_t scratch_bytes, void* stream);
/* ResnetBlock tail in one launch (unet.py:105-110): out = conv3x3(act(src0|src1)) + bias + film
 *   + conv1x1(x2_src0|x2_src1; x2_w [Cout][x2_C0+x2_C1]) + x2_bias  -- block2's conv with `res_conv(x)`
 * accumulated as a second K-segment of the same output tile (halo kernel: tile_cfg 0 | 5 | 6). */
int sr3_block_conv_f32(const float* src0, int C0, const float* src1, int C1, int B, int H, int W, int Cout,
                       const float* w_ohwi, const float* bias, const float* ss, int act, const float* film,
                       int film_stride, const float* x2_src0, int x2_C0, const float* x2_src1, int x2_C1,
                       const float* x2_w, const float* x2_bias, float* out, double* out_stats, int tile_cfg,
                       int ksplit, void* scratch, size_t scratch_bytes, void* stream);
/* Train-mode `Block` (unet.py:80-91 with nn.Dropout active, :86): out = conv3x3(dropout(act(src0))) + bias + film
 *   [+ residual res0] [+ conv1x1(x2_src0|x2_src1) + x2_bias], the op sr3_train_step launches for every block2.
 * Mask: NHWC element i of the activated input is kept iff hash32(i * 0x9E3779B9 + drop_seed) >= drop_p * 2^32 and
 * scaled by 1 / (1 - drop_p) (drop_seed is the per-layer seed).  Single source, no upsampling; x2_* may be NULL.
 * tile_cfg 11 / 12 run the Winograd kernel's dropout instantiations (fp32 MFMA / 3 x bf16 split; what sr3_train_step uses on
 * maps >= 16x16 with wino_split = 0 / 1; no x2 segment:
 * scratch then also holds the transformed filters, as for sr3_conv_f32 -- sr3_conv_scratch_bytes accounts for them). */
int sr3_conv_dropout_f32(const float* src0, int C0, int B, int H, int W, int Cout, const float* w_ohwi,
                         const float* bias, const float* ss, int act, const float* film, int film_stride,
                         const float* res0, int RC0, const float* x2_src0, int x2_C0, const float* x2_src1, int x2_C1,
                         const float* x2_w, const float* x2_bias, float* out, double* out_stats, int tile_cfg,
                         int ksplit, void* scratch, size_t scratch_bytes, unsigned drop_seed, float drop_p,
                         void* stream);
/* The keep threshold and scale every dropout kernel derives from p: floor(p * 2^32) and 1 / (1 - p), evaluated in double
 * on the decimal value the fp32 argument stands for (0.2f -> 0.2), as nn.Dropout's p is a Python float.  Host only. */
unsigned sr3_dropout_threshold(float drop_p, float* scale_out);
size_t sr3_conv_scratch_bytes(int B, int Ho, int Wo, int Cin, int Cout, int ksize, int tile_cfg, int ksplit);
/* nn.GroupNorm statistics (unet.py:84,119) as PARTIAL per-(image, channel) {sum, sumsq} in double of
 * an NHWC tensor: stat[B][T][C][2] with T = sr3_groupnorm_stats_slices(B, HW, C).  Plain stores (no
 * atomics, no zeroing needed); summed in a fixed order by the fold => bitwise reproducible. */
int sr3_groupnorm_stats_slices(int B, int HW, int C);
int sr3_groupnorm_stats_f32(const float* x_nhwc, int B, int HW, int C, double* stat, void* stream);
/* T of the partial statistics sr3_conv_f32 writes into out_stats (0: this geometry cannot fuse them) */
int sr3_conv_stats_slices(int B, int Hs, int Ws, int ups, int Cin, int Cout, int tile_cfg, int ksplit);
/* fold partial statistics of the concat (stat0|stat1) with gamma/beta into ss[B][C0+C1][2] */
int sr3_groupnorm_fold_f32(const double* stat0, int C0, int T0, const double* stat1, int C1, int T1, int B, int HW,
                           int groups, const float* gamma, const float* beta, float eps, float* ss, void* stream);
/* SelfAttention core (unet.py:127-139): qkv NHWC [B][N][3C] -> out [B][N][C] */
int sr3_attention_f32(const float* qkv, int B, int N, int C, float* out, void* stream);
/* ... with a mode (`split`).  Bit 0: QK^T and PV as six bf16 MFMA products of 3-way split fp32 operands, fp32 accumulation (plan option
 * attn_split; fp32-class results, gated against float64 in tests/), where the shape takes the staging-free kernel.  Bit 1: the
 * key-blocked kernel (plan option attn_long; csrc/attention_long.hip): any N > 0 and C % 4 == 0, also where the score strip fits; bit 0
 * then selects the split arithmetic where C % 128 == 0 (other C run an fp32-MFMA form).  Without bit 1, N beyond the LDS score strip
 * (about 1088 tokens) is refused with SR3_E_UNSUPPORTED; B * N * 3C >= 2^31 is refused in every mode. */
int sr3_attention_ex_f32(const float* qkv, int B, int N, int C, float* out, int split, void* stream);
/* backward of the attention core (autograd of unet.py:127-139): dqkv [B][N][3C] from qkv, d(out) [B][N][C]; out_fwd
 * (the forward output) may be NULL when N <= ~480 -- larger N use a key-blocked pass that reads it */
int sr3_attention_bwd_f32(const float* qkv, const float* dout, const float* out_fwd, int B, int N, int C, float* dqkv,
                          void* stream);
/* ... bitwise reproducible: every 32-query block hands its dK / dV contribution to a slab of its own in `scratch`
 * (sr3_attention_bwd_scratch_bytes(B, N, C) = ceil(N / 32) * B * N * 2C floats) and a second kernel sums the slabs in block
 * order -- no atomics, no memset (sr3_attention_bwd_f32 adds with fp32 atomics).  What sr3_train_step runs.  scratch: 16-byte aligned
 * (SR3_E_ALIGN), at least the queried bytes (SR3_E_NOMEM). */
size_t sr3_attention_bwd_scratch_bytes(int B, int N, int C);
int sr3_attention_bwd_ex_f32(const float* qkv, const float* dout, const float* out_fwd, int B, int N, int C, float* dqkv,
                             void* scratch, size_t scratch_bytes, void* stream);
/* Multi-head SelfAttention core (the reference module's n_head, unet.py:113-142): `heads` heads of d = C / heads channels over the same
 * tensors.  Head h owns channels [3 d h, 3 d (h + 1)) of a qkv row as q_h | k_h | v_h (the module's view (b, n_head, 3 d, h, w)) and
 * channels [d h, d (h + 1)) of an out row; S_h = Q_h K_h^T / sqrt(C) -- the FULL C, as in the module --, P_h = softmax over keys,
 * O_h = P_h V_h.  heads == 1: the launches and bits of sr3_attention_ex_f32 in every mode.  mode bits 0 (split arithmetic) and 1
 * (key-blocked kernel) as there; bit 2 keeps 64- and 32-channel heads off their own kernel (a measurement knob).  Kernels: d = 64 / 32
 * on k_attention_heads (csrc/attention_heads.hip; fp32-MFMA and split instantiations, any N the score strip holds, ragged included),
 * d % 128 == 0 on the staging-free kernels, every other d % 4 == 0 on the LDS-staged fp32-MFMA kernel, every d under bit 1.
 * Refused: heads < 1 or C % heads != 0 (SR3_E_BADARG), (C / heads) % 4 != 0 (SR3_E_UNSUPPORTED), B * N * 3C >= 2^31, B * heads > 65535,
 * N beyond the score strip without bit 1 (SR3_E_UNSUPPORTED) -- each with the numbers in sr3_last_error(). */
int sr3_attention_heads_f32(const float* qkv, int B, int N, int C, int heads, float* out, int mode, void* stream);
/* ... its backward, in the slab form of sr3_attention_bwd_ex_f32 (fp32 MFMA; no atomics, no memset: bitwise reproducible).  scratch:
 * sr3_attention_bwd_scratch_bytes(B, N, C) bytes -- the slab total does not depend on heads --, 16-byte aligned (SR3_E_ALIGN), not
 * shorter (SR3_E_NOMEM).  heads == 1: the bits of sr3_attention_bwd_ex_f32.  Refusals as the forward's. */
int sr3_attention_bwd_heads_f32(const float* qkv, const float* dout, const float* out_fwd, int B, int N, int C, int heads, float* dqkv,
                                void* scratch, size_t scratch_bytes, void* stream);
/* Weight gradient of one convolution (autograd of nn.Conv2d inside `l_pix.backward()`, model/model.py:50-54), per op -- what
 * sr3_train_step runs per layer: dw[n][tap][c] = sum over output pixels of dy[m][n] * a_tap[m][c], with a = the convolution's
 * (virtual concat, optionally x2-upsampled, optionally GroupNorm-affine / SiLU-activated: act, ss as in sr3_conv_f32) input.
 * dy NHWC [B, Ho, Wo, Cout]; dw OHWI [Cout][ksize^2][C0 + C1], overwritten.  split != 0: the 3 x bf16 split kernel where it applies
 * (more than 64 channels on both sides; plan option wgrad_split), else the fp32-MFMA kernels.  scratch: the per-pixel-range slabs
 * (sr3_conv_wgrad_scratch_bytes), summed in double in a fixed order; 16-byte aligned (SR3_E_ALIGN), at least the queried bytes where the
 * shape splits its pixels (SR3_E_NOMEM). */
size_t sr3_conv_wgrad_scratch_bytes(int B, int Hs, int Ws, int ups, int stride, int ksize, int C0, int C1, int Cout, int split);
int sr3_conv_wgrad_f32(const float* src0, int C0, const float* src1, int C1, int B, int Hs, int Ws, int ups, int stride, int ksize,
                       int Cout, const float* ss, int act, const float* dy, float* dw_ohwi, int split, void* scratch,
                       size_t scratch_bytes, void* stream);
/* sr3_groupnorm_fold_f32 that also keeps mr[B][groups][2] = (mean, rstd) per (image, group): what the training forward keeps
 * for the GroupNorm backward below. */
int sr3_groupnorm_fold_mr_f32(const double* stat0, int C0, int T0, const double* stat1, int C1, int T1, int B, int HW,
                              int groups, const float* gamma, const float* beta, float eps, float* ss, float* mr, void* stream);
/* ... under a scale-shift modulation (SR3_UNET_SCALE_SHIFT_NORM): mod + b * mod_stride points at image b's 2 C values, C = C0 + C1
 * scales s then C shifts t (mod_stride >= 2 C), and the pairs written are those of GN(x) (1 + s) + t:
 *   sc = rstd gamma_c ; sh = beta_c - mean sc ; m = 1 + s_bc ; ss = (sc m, fma(sh, m, t_bc)), each step rounded to fp32 in this order
 * -- the same bits a plan's fused folds write.  mr may be NULL.  Host checks as the backward entries below (NULL mod, mod_stride
 * < 2 C: SR3_E_BADARG; C0 / C1 % 4, C % groups: SR3_E_UNSUPPORTED); nothing is launched on a refusal. */
int sr3_groupnorm_fold_mod_f32(const double* stat0, int C0, int T0, const double* stat1, int C1, int T1, int B, int HW,
                               int groups, const float* gamma, const float* beta, float eps, float* ss, float* mr, const float* mod,
                               int mod_stride, void* stream);

/* ---- the training backward's own kernels, per op (autograd of `l_pix.backward()`, model/model.py:50-54): each entry runs the
 * functions sr3_train_step's backward walk runs, on caller-owned tensors.  Every entry checks its arguments on the host and launches
 * nothing on a refusal: SR3_E_BADARG for a NULL required pointer (the second source's with C1 > 0 too), a non-positive size or an
 * argument out of its range, SR3_E_UNSUPPORTED for a well-formed problem the kernels do not take -- a channel count that is no multiple
 * of 4, channels % groups != 0, a tensor of 2^31 elements, an odd map under a stride-2 conv, an upsampled stride-2 conv --,
 * SR3_E_NOMEM for a scratch that is too small, SR3_E_ALIGN for a misaligned scratch.  Fixed-order sums, no atomics: the same bits
 * every run. */

/* Backward of GroupNorm (+ SiLU with act 2; act 1: the affine alone) (+ dropout) in front of a conv (Block, unet.py:80-91), over the
 * virtual concat x = (x0 | x1), NHWC [B][HW][C0 | C1].  dA [B][HW][C0 + C1], the gradient w.r.t. the activated (and dropped) input,
 * is REWRITTEN IN PLACE with du, the gradient w.r.t. u = x * scale + shift.  ss [B][C][2] and mr [B][groups][2] are the forward's
 * tables (sr3_groupnorm_fold_mr_f32).  drop_seed is the layer's seed and drop_p the probability, mapped to (threshold, scale) as by
 * sr3_dropout_threshold; the mask is sr3_conv_dropout_f32's, over the NHWC index of the concat.  Outputs: dgamma, dbeta [C]
 * (overwritten); dx0 / dx1 (C1 0: one source, x1 and dx1 are not read), accumulated into where acc0 / acc1 != 0, plain stores otherwise; aout (may be NULL)
 * [B][HW][C] = dropout(act(u)), the conv's input as the weight gradient reads it.  scratch: 8-byte aligned,
 * sr3_groupnorm_act_bwd_scratch_bytes(B, HW, C0 + C1, groups) bytes (0 for a shape the entry refuses). */
size_t sr3_groupnorm_act_bwd_scratch_bytes(int B, int HW, int C, int groups);
int sr3_groupnorm_act_bwd_f32(float* dA, const float* x0, int C0, const float* x1, int C1, int B, int HW, const float* ss,
                              const float* mr, int groups, int act, const float* gamma, unsigned drop_seed, float drop_p,
                              float* dgamma, float* dbeta, float* dx0, int acc0, float* dx1, int acc1, float* aout,
                              void* scratch, size_t scratch_bytes, void* stream);
/* ... of a GroupNorm folded under a scale-shift modulation (sr3_groupnorm_fold_mod_f32: ss holds the modulated pairs, mod / mod_stride
 * are that call's).  gamma_c (1 + s_bc) stands where gamma_c does in dx; dgamma_c = sum_b (1 + s_bc) sum du xhat, dbeta_c = sum_b
 * (1 + s_bc) sum du; and the rows' gradients go to dmod, in the layout and stride of mod (only the 2 C entries per image are written):
 *   d shift_bc = sum du ;  d scale_bc = sum du GN(x) = gamma_c sum du xhat + beta_c sum du      (all in double, rounded once)
 * which is why this entry takes beta too (GN(x) cannot be recovered from the pairs where 1 + s = 0).  Rows of zeros give the plain
 * entry's dx, dgamma and dbeta bits.  The scratch is the plain entry's: sr3_groupnorm_act_bwd_scratch_bytes. */
int sr3_groupnorm_act_bwd_mod_f32(float* dA, const float* x0, int C0, const float* x1, int C1, int B, int HW, const float* ss,
                                  const float* mr, int groups, int act, const float* gamma, unsigned drop_seed, float drop_p,
                                  float* dgamma, float* dbeta, float* dx0, int acc0, float* dx1, int acc1, float* aout,
                                  void* scratch, size_t scratch_bytes, const float* beta, const float* mod, int mod_stride,
                                  float* dmod, void* stream);

/* Data gradient of one convolution, the "main segment" of the backward walk: dy [B, Ho, Wo, CoutP] (the forward conv's output
 * gradient; Ho x Wo from Hs, Ws, ups, stride, ksize as in sr3_conv_f32) -> dA [B, Hs << ups, Ws << ups, Cin], the gradient w.r.t.
 * the conv's (upsampled) input, before it is routed to the sources.  w_ohwi [Cout_w][ksize^2][Cin] holds Cout_w <= CoutP filters:
 * the filters are flipped and transposed with the missing rows zero (the output conv's 3 -> 4 / 6 -> 8 padding; the lanes of dy
 * beyond Cout_w then contribute exactly 0 whatever finite value they hold), dy is zero-inserted for stride 2 (even Hs, Ws only:
 * SR3_E_UNSUPPORTED otherwise), and the same conv kernels run on the result.  `plan` gives the options and the geometry state the
 * step's choice reads (winograd, wino_split, wino2, wino_ragged, gemm_split, gemm2, gemm_n64, train_geom and whether the plan's
 * geometry is the native one); nothing else of the plan is touched.  scratch: 256-byte aligned, sr3_conv_dgrad_scratch_bytes bytes;
 * derived: 256-byte aligned room for the derived filters of the chosen kernel (*derived_bytes of the query; may be NULL / 0; *base_bytes of the
 * query, may be NULL: the bytes of the scratch in front of its split-K slabs -- a scratch of exactly that size has room for no slab).  As in
 * the step, derived filters that do not fit send the conv to the general kernels; a scratch below what the kernel then needs is
 * refused.  *tile_out: the tile_cfg number of sr3_conv_f32 the conv ran on, *ksplit_out its split-K factor, *derived_kind_out 0 none,
 * 1 Winograd fp32, 2 Winograd 3 x bf16 split, 3 the pre-split 1x1 weights (each may be NULL). */
size_t sr3_conv_dgrad_scratch_bytes(sr3_plan* plan, int B, int Hs, int Ws, int ups, int stride, int ksize, int Cin, int CoutP,
                                    size_t* derived_bytes, size_t* base_bytes);
int sr3_conv_dgrad_f32(sr3_plan* plan, const float* dy, const float* w_ohwi, int Cout_w, int CoutP, int B, int Hs, int Ws, int ups,
                       int stride, int ksize, int Cin, float* dA, void* scratch, size_t scratch_bytes, void* derived,
                       size_t derived_bytes, int* tile_out, int* ksplit_out, int* derived_kind_out, void* stream);

/* Routing of a gradient g [B, Hs << ups, Ws << ups, C0 + C1] to the two sources of a virtual concat, d0 [B, Hs, Ws, C0] and d1
 * [B, Hs, Ws, C1] (C1 0: one source, d1 is not read): ups 1 sums the 2 x 2 children of a source pixel, ((a + b) + c) + d in row-major order (the
 * backward of the nearest x2 upsample); acc0 / acc1 != 0 adds the destination's old value last, 0 is a plain store. */
int sr3_grad_route_f32(const float* g, int C0, int C1, int B, int Hs, int Ws, int ups, float* d0, int acc0, float* d1, int acc1,
                       void* stream);

/* Column sums of g [B][HW][C], accumulated in double and rounded once: dbias[c] = the sum over images and pixels (the bias
 * gradient), dfilm[b * film_stride + c] = the sum over the pixels of image b (a conv's rows of the FiLM gradient table; film_stride
 * >= C, every other element of the table is left untouched).  Either may be NULL, not both.  scratch: 8-byte aligned,
 * sr3_colsums_scratch_bytes bytes. */
size_t sr3_colsums_scratch_bytes(int B, int HW, int C);
int sr3_colsums_f32(const float* g, int B, int HW, int C, float* dbias, float* dfilm, int film_stride, void* scratch,
                    size_t scratch_bytes, void* stream);

/* Backward of sr3_film_embed_f32: dfilm [B][F] -> the gradients of the embedding MLP (dw1 [4 inner][inner], db1, dw2
 * [inner][4 inner], db2) and of the FiLM projections (dwf [F][inner], dbf [F]), all overwritten; the forward is recomputed from
 * level / timestep and freq.  inner must divide 256 (SR3_E_UNSUPPORTED otherwise).  scratch: sr3_embed_bwd_scratch_bytes bytes. */
size_t sr3_embed_bwd_scratch_bytes(int B, int inner);
int sr3_embed_bwd_f32(int variant, int B, int inner, int F, const float* level, const int64_t* timestep, const float* freq,
                      const float* w1, const float* b1, const float* w2, const float* b2, const float* wf, const float* dfilm,
                      float* dw1, float* db1, float* dw2, float* db2, float* dwf, float* dbf, void* scratch, size_t scratch_bytes,
                      void* stream);

/* noise-level / timestep embedding + MLP + all FiLM rows (unet.py:18-50,179-184): see sr3_common.h */
int sr3_film_embed_f32(int variant, int B, int inner, const float* level, const int64_t* timestep,
                       const float* freq, const float* w1, const float* b1, const float* w2, const float* b2,
                       const float* wf, const float* bf, int F, float* temb_scratch, float* film_out,
                       void* stream);
/* first conv (NCHW concat in -> NHWC) and final Block (NHWC -> NCHW) */
int sr3_conv_in_f32(const float* a_nchw, int Ca, const float* b_nchw, int Cb, int B, int H, int W,
                    const float* w_ohwi, const float* bias, int Cout, float* out_nhwc, void* stream);
int sr3_conv_out_f32(const float* x_nhwc, const float* ss, int B, int H, int W, int C, const float* w_ohwi,
                     const float* bias, int Cout, float* out_nchw, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SR3_MI355X_H */
