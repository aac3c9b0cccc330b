// Shared by plan_build.hip (the planner), plan_run.hip / plan_abi.hip (the profile's and the op list's tile numbers) and abi_ops.hip (the per-op entries): the codec of the public tile_cfg numbers, the shape-only ConvParams.
#pragma once
#include <string.h>
#include "sr3_common.h"

namespace sr3 {

// One public tile_cfg number (sr3_conv_f32 & co, sr3_op_info::tile_cfg), taken apart into what conv_forward is called with:
//   0-11 the kernel tile itself (0: conv_pick chooses; 1-4 im2col; 5-10 halo; 11 Winograd, fp32 MFMA)
//   12, 13, 23: tile 11 with ConvParams::wino_split 1, 2, 3 (3 x bf16 split: 8-wave kernel; 8 x 16 tile of conv3x3_wino2.hip; its ragged form)
//   14-17: im2col tiles 1-4 with ConvParams::igemm_split (3 x bf16 split); 18-21: ... with pre-split weights (ConvParams::w_split)
//   25, 26: 13 / 23 with ConvParams::wino_full (the sixteen-position loop even where ups = 1 would select the nine-position one; same bits)
//   22: the plain GEMM kernel of gemm1x1.hip (always split, always pre-split weights); 24: attention ops only (attention_long.hip), passes through
//   27, 28, 29: 22 with ConvParams::gemm_epi 1, 2, 3 (the epilogue of plan option gemm_epi = 0 / 1 / 2 named; 22 itself leaves it to the default)
// The only place in the library that knows the numbers; the one other copy is the TILE name table of tools/dump_plan.py.
struct TileCode { int tile; int wino_split; int igemm_split; bool wpre; int wino_full = 0; int gemm_epi = 0; };
inline TileCode tile_decode(int abi_tile) {
  if (abi_tile == 12 || abi_tile == 13) return {11, abi_tile - 11, 0, false};
  if (abi_tile == 23) return {11, 3, 0, false};
  if (abi_tile == 25 || abi_tile == 26) return {11, abi_tile - 23, 0, false, 1};
  if (abi_tile >= 14 && abi_tile <= 17) return {abi_tile - 13, 0, 1, false};
  if (abi_tile >= 18 && abi_tile <= 21) return {abi_tile - 17, 0, 1, true};
  if (abi_tile == 22) return {22, 0, 1, true};
  if (abi_tile >= 27 && abi_tile <= 29) return {22, 0, 1, true, 0, abi_tile - 26};
  return {abi_tile, 0, 0, false};
}
inline int tile_encode(int tile, int wino_split, int igemm_split, bool has_wsplit, int wino_full = 0) {
  if (tile == 11 && wino_split >= 2 && wino_full) return 23 + wino_split;
  if (tile == 11 && wino_split) return wino_split == 3 ? 23 : 11 + wino_split;
  if (tile >= 1 && tile <= 4 && igemm_split) return (has_wsplit ? 17 : 13) + tile;
  return tile;
}
// ... and the number sr3_unet_forward_profile reports for a conv's kernel (op_kind; 59 is the split-K reduce behind a conv):
//   51-54 im2col kernel tiles, 651-654 the same on their 3 x bf16 split instantiation; 55 / 56 halo-tile 3x3 kernel (57 / 58: with the fused
//   1x1 segment), 155-158 the same four on the opt-in split-bf16 instantiations, 255 / 257 the 8-wave 256x128 tile (cfg 9), 355 / 357 its
//   split-bf16 twin (cfg 10); 455 the Winograd F(2x2,3x3) kernel (cfg 11), 555 its 3 x bf16 split instantiation (plan option wino_split),
//   575 the two-workgroups-per-CU split kernel (conv3x3_wino2.hip), 585 its ragged instantiation, each + 10 on the four-image tile of the
//   8x8 maps (465, 565); 232 the 1x1 GEMM kernel (gemm1x1.hip)
inline int profile_kind(int tile, int wino_split, int igemm_split, bool four_image, bool fused_segment) {
  static const int base[13] = {0, 1, 2, 3, 4, 5, 6, 105, 106, 205, 305, 405, 505};
  if (tile == 22) return 232;
  int kind = 50 + base[(tile == 11 && wino_split) ? 12 : tile] + ((tile >= 5 && fused_segment) ? 2 : 0);
  if (tile == 11) kind += (wino_split == 2 ? 20 : wino_split == 3 ? 30 : 0) + (four_image ? 10 : 0);
  if (tile >= 1 && tile <= 4 && igemm_split) kind += 600;
  return kind;
}

// ConvParams with the shape fields alone: everything else zero, ksplit 1 (conv_forward sets the real one)
inline ConvParams conv_shape(int B, int Hs, int Ws, int ups, int stride, int ksize, int C0, int C1, int Cout) {
  ConvParams c;
  memset(&c, 0, sizeof(c));
  c.B = B; c.Hs = Hs; c.Ws = Ws; c.ups = ups; c.stride = stride; c.ksize = ksize; c.C0 = C0; c.C1 = C1; c.Cout = Cout;
  const int pad = ksize / 2;
  c.Ho = ((Hs << ups) + 2 * pad - ksize) / stride + 1;
  c.Wo = ((Ws << ups) + 2 * pad - ksize) / stride + 1;
  c.ksplit = 1;
  return c;
}

}  // namespace sr3
