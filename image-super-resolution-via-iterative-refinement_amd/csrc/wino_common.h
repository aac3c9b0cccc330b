// What the two Winograd kernels (conv3x3_wino.hip: 8 waves, one workgroup per CU; conv3x3_wino2.hip: 4 waves, two per CU) must agree on:
// the filter layout one writes and both read, the raw tile's LDS pixel layout, the walk over the tile list and the K-range split.
#pragma once
#include "sr3_common.h"

namespace sr3 {

constexpr int WBN = 64;         // output channels per workgroup (a cout block)
constexpr int WCK = 16;         // input channels per chunk
constexpr int WRS = 20;         // LDS pixel stride (floats) of the raw halo: 16 channels + 4 pad
constexpr int WSHIFT = 4;       // every second ROW PAIR of the raw halo is shifted by 4 floats more: with this layout the transform's
                                // ds_read_b128 (lane = tile of a 4 x 8 tile block, two channel quads) hit 16 distinct bank quads per 16-lane group

// The split filters (k_wino_weights_split writes them; the SPLIT instantiation of k_conv3x3_wino and every k_conv3x3_wino2 read them): every
// U = G g G^T value as three bf16 terms, laid out as the B operand of v_mfma_f32_32x32x16_bf16 (one MFMA = a whole 16-channel chunk):
//   ufrag_s[cout_blk][chunk][pos 16][nblk 2][plane 3 (h, m, l)][lane 64][8 bf16]
// Lane l holds U_pos[n = cout_blk*64 + nblk*32 + (l & 31)] for the 8 channels k = 0..7 of its half hq = l >> 5: channel = chunk*16 +
// (k < 4 ? 4 hq + k : 8 + 4 hq + (k - 4)) -- the order in which the kernels' transform lanes hold their channels (quad hq of either half
// chunk), so V needs no shuffle.  WUS: bf16 elements of one (position, n block) fragment group; a position is 2 WUS bf16 = WUS floats.
constexpr int WUS = 3 * 64 * 8;

// Persistent workgroups walk the (cout block major) tile list.  XCD-aware order: consecutive workgroup ids go round-robin to the 8 XCDs;
// each XCD gets one contiguous range of the list, so that the U fragments of a cout block stay inside one L2 (gridDim.x is a multiple of 8
// whenever the tile count is, so a workgroup's tiles stay on its XCD's range).  Tile v of ntiles -> its cout block, tile column / row and
// batch tile (sp_tiles = tiles_w * tiles_h * nbt spatial tiles per cout block); how many pixels a tile row spans is the kernel's.
struct WinoTile { int cb, tw_i, th_i, b0; };
__device__ __forceinline__ WinoTile wino_decode_tile(int v, int ntiles, int sp_tiles, const WinoGeom& g) {
  WinoTile t;
  int bid = v;
  if ((ntiles & 7) == 0) bid = (bid & 7) * (ntiles >> 3) + (bid >> 3);
  // bid / sp_tiles by a host-side magic number (0: one tile per cout block, the quotient is bid itself)
  t.cb = g.sp_magic ? (int)(((unsigned long long)(unsigned)bid * g.sp_magic) >> 32) : bid;
  int sp = bid - t.cb * sp_tiles;
  if (g.pow2) {
    t.tw_i = sp & (g.tiles_w - 1);
    t.th_i = (sp >> g.log_tw) & (g.tiles_h - 1);
    t.b0 = sp >> (g.log_tw + g.log_th);
  } else {
    t.tw_i = sp % g.tiles_w;
    sp /= g.tiles_w;
    t.th_i = sp % g.tiles_h;
    t.b0 = sp / g.tiles_h;
  }
  return t;
}

// split-K over chunks: split `split` of ksplit runs chunks [c_begin, c_end) of the conv's nch
struct WinoKRange { int nch, c_begin, c_end; };
__device__ __forceinline__ WinoKRange wino_k_range(int Cin, int ksplit, unsigned split) {
  const int nch = (Cin + WCK - 1) / WCK;
  const int cper = (nch + ksplit - 1) / ksplit;
  const int c_begin = split * cper;
  return WinoKRange{nch, c_begin, min(nch, c_begin + cper)};
}

}  // namespace sr3
