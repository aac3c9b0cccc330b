// Conv dispatch: which kernel family and tile a conv runs on (conv_pick), how far it splits K, and the launch itself (conv_forward) --
// over the im2col kernel (conv_igemm.hip), the halo kernel (conv3x3_halo.hip), the two Winograd kernels (conv3x3_wino.hip,
// conv3x3_wino2.hip) and the plain GEMM (gemm1x1.hip), with the split-K reduce of small_kernels.hip behind them.  Host code only.
#include <stdlib.h>

#include "sr3_common.h"

namespace sr3 {
namespace {
inline int cdiv(int a, int b) { return (a + b - 1) / b; }
struct TileCfg { int bm, bn; };
const TileCfg kCfgs[5] = {{0, 0}, {128, 128}, {128, 64}, {64, 64}, {64, 128}};      // the im2col tiles 1-4

// ---- the knobs: environment variables, each read once per process at its first use, and compile-time thresholds ----
// A/B knob: never pick the 8-wave 256x128 tile
bool env_no_wide() { static const bool v = getenv("SR3_NO_WIDE") != nullptr; return v; }
// halo / im2col kernels: split K until the grid gives ~2 workgroups per CU (in-run A/B on MI355X: threshold 384 -> 14.87 ms per
// step, 256 -> 14.96 ms; SR3_KSPLIT_TILES overrides)
long env_ksplit_tiles() { static const long v = getenv("SR3_KSPLIT_TILES") ? atol(getenv("SR3_KSPLIT_TILES")) : 384; return v; }
// profiling ablations of the conv kernels (ConvParams::dbg)
int env_conv_dbg() { static const char* e = getenv("SR3_CONV_DBG"); return e ? atoi(e) : 0; }
// 1x1 GEMM kernel (gemm1x1.hip; two workgroups per CU): split K below one round of workgroups, >= 4 k-steps (128 channels) per split
#ifndef SR3_G1_SPLIT_BELOW
#define SR3_G1_SPLIT_BELOW 128
#endif
// the stride-2 form walks 9 k-steps per 32-channel chunk: K is long (>= 36 steps at 128 channels) and the maps are small, so it
// splits whenever the tiles do not fill the 512 slots, >= 8 k-steps per split
#ifndef SR3_G1_S2_SPLIT_BELOW
#define SR3_G1_S2_SPLIT_BELOW 512
#endif
}  // namespace

ConvPick conv_pick(const ConvParams& p, int tile_cfg, int ksplit) {
  const int M = p.B * p.Ho * p.Wo;
  const int taps = p.ksize * p.ksize;
  const int nchunks = cdiv(p.C0 + p.C1, 32);
  const bool no_wide = env_no_wide();
  if (tile_cfg == 0) {
    HaloGeom g;
    if (p.ksize == 3 && p.stride == 1) {
      if (p.Cout <= 64 && halo_geometry(p, 6, &g)) tile_cfg = 6;
      else if (p.Cout > 64 && !no_wide && halo_geometry(p, 9, &g) &&
               (long)cdiv(p.Cout, 128) * g.tiles_w * g.tiles_h * cdiv(p.B, g.NB) >= 256)
        tile_cfg = 9;     // 8-wave 256x128 tile: half the weight traffic, when it still fills every CU
      else if (halo_geometry(p, 5, &g)) tile_cfg = 5;
    }
  }
  // 3 x bf16 split instantiations: the 64x64 tile as well.  In isolation (warm operands) the larger split tiles win on most
  // layer shapes (128x128: qkv 71 vs 94 us), but INSIDE the forward -- activations just written by the previous kernel, weights
  // from HBM -- they lose by up to 2.5x on the short-K layers (one round of 384-512 workgroups loads, computes and stores in
  // lock step), and per-launch timing of the whole forward with every tile forced in turn (plan option gemm_tile,
  // profiles/r04f_gemm_split_sweep.txt) gives 64x64 2.31 / 1.96 / 1.59 / 2.02 ms for tiles 1-4 (fp32 MFMA: 2.59 / 2.27 / 1.86 / 2.34)
  if (tile_cfg == 0 && p.igemm_split && (p.ksize == 1 || p.stride == 2)) tile_cfg = 3;
  if (tile_cfg == 0 && p.ksize == 1) tile_cfg = 3;   // 1x1 convs: the 64x64 tile measured fastest on every layer shape of the
                                                     // BASELINE networks (76-81 vs 58-64 TF at 16x16, 78 vs 69 at 128x128)
  if (tile_cfg == 0) {
    // im2col kernel: largest tile that still gives >= ~2 workgroups per CU
    const int order_wide[3] = {1, 2, 3};
    const int order_narrow[2] = {2, 3};
    const int* order = p.Cout > 64 ? order_wide : order_narrow;
    const int norder = p.Cout > 64 ? 3 : 2;
    tile_cfg = order[norder - 1];
    for (int k = 0; k < norder; ++k) {
      const TileCfg c = kCfgs[order[k]];
      if ((long)cdiv(M, c.bm) * cdiv(p.Cout, c.bn) >= 448) { tile_cfg = order[k]; break; }
    }
  }
  if (ksplit != 0) return {tile_cfg, ksplit};
  // every branch fills in split_k's five numbers (sr3_common.h): workgroups, threshold, round of workgroup slots, units of K, units per split
  if (tile_cfg == 22) {
    const long tiles = (long)(M / gemm1x1_rows(p)) * (p.Cout / gemm1x1_cols(p));
    return {22, taps == 9 ? split_k(tiles, SR3_G1_S2_SPLIT_BELOW, 512, nchunks * taps, 8) : split_k(tiles, SR3_G1_SPLIT_BELOW, 512, nchunks, 4)};
  }
  if (tile_cfg == 11) {
    // Winograd kernel: one 8-wave workgroup per CU, so one full round of 256 is the target (512 for the four-wave workgroups of
    // conv3x3_wino2.hip, two per CU); a split keeps >= 4 chunks (64 input channels)
    // (tried in round 6: no split from half a round on for the 8 x 16 tile -- 11 reduce launches fewer, the convs 0.13-0.24 ms slower:
    // a wash, profiles/r06_wino2_experiments.txt)
    WinoGeom wg;
    if (!wino_geometry(p, &wg)) return {11, 1};
    const int units = wino_chunks(p), maxck = wino_max_chunks_per_split(wg);
    const long round = p.wino_split >= 2 ? 512 : 256;
    int ks = split_k(wino_workgroups(p, wg), round, round, units, 4);
    // (split_k has already dropped the empty splits, which keeps cdiv(units, ks): the two extras see what they saw before it did)
    if (wg.NB != 1 && ks < 2 && units >= 2) ks = 2;          // the four-image tile (8 x 8 maps) has no direct epilogue
    if (cdiv(units, ks) > maxck) ks = cdiv(units, maxck);    // chunks per split the kernel's LDS block of GroupNorm pairs holds
    return {11, split_shrink(units, ks)};
  }
  if (tile_cfg >= 5) {
    HaloGeom g;
    if (!halo_geometry(p, tile_cfg, &g)) return {tile_cfg, 1};
    const long tiles = (long)cdiv(p.Cout, halo_cfg_bn(tile_cfg)) * g.tiles_w * g.tiles_h * cdiv(p.B, g.NB), below = env_ksplit_tiles();
    // the 8-wave tiles run one workgroup per CU: one full round of 256 is the target there
    const bool wide = halo_cfg_one_wg_per_cu(tile_cfg);
    return {tile_cfg, split_k(tiles, wide ? 256 : below, wide ? 256 : 512, nchunks, 2)};
  }
  const TileCfg c = kCfgs[tile_cfg];
  return {tile_cfg, split_k((long)cdiv(M, c.bm) * cdiv(p.Cout, c.bn), env_ksplit_tiles(), 512, nchunks * taps, 6)};
}

// rows per block of the split-K reduce kernel; with statistics it must divide Ho*Wo (0: cannot fuse)
int splitk_rows_per_block(const ConvParams& p, bool stats) {
  const long M = (long)p.B * p.Ho * p.Wo;
  const int HoWo = p.Ho * p.Wo;
  int rpb = 64;
  while (rpb > 4 && M / rpb < 1024) rpb >>= 1;
  if (stats) {
    while (rpb > 1 && HoWo % rpb) rpb >>= 1;
    if (HoWo % rpb || HoWo / rpb > 256) return 0;
  }
  return rpb;
}

size_t conv_splitk_bytes(const ConvParams& p, int tile_cfg, int ksplit) {
  const int ks = conv_pick(p, tile_cfg, ksplit).ksplit;
  return ks <= 1 ? 0 : (size_t)ks * p.B * p.Ho * p.Wo * p.Cout * sizeof(float);
}

int conv_forward(const ConvParams& pin, int tile_cfg, int ksplit, float* scratch, size_t scratch_bytes, hipStream_t st, hipEvent_t mid) {
  ConvParams p = pin;
  const int Cin = p.C0 + p.C1;
  if ((p.C0 & 3) || (p.C1 & 3) || (p.Cout & 3)) { set_error("conv: channel counts must be multiples of 4 (C0=%d C1=%d Cout=%d)", p.C0, p.C1, p.Cout); return SR3_E_UNSUPPORTED; }
  if (p.ksize != 1 && p.ksize != 3) { set_error("conv: ksize %d unsupported", p.ksize); return SR3_E_UNSUPPORTED; }
  if (p.stride != 1 && p.stride != 2) { set_error("conv: stride %d unsupported", p.stride); return SR3_E_UNSUPPORTED; }
  if (p.act != 0 && !p.ss) { set_error("conv: act needs ss"); return SR3_E_BADARG; }
  if (p.drop_thresh != 0 && (p.C1 != 0 || p.ups != 0 || p.act == 0)) { set_error("conv: dropout needs a single-source, non-upsampled, activated input"); return SR3_E_UNSUPPORTED; }
  if (p.C1 > 0 && !p.src1) { set_error("conv: C1 > 0 needs src1"); return SR3_E_BADARG; }
  if (p.res0 && p.RC0 + p.RC1 != p.Cout) { set_error("conv: residual channels %d+%d != Cout %d", p.RC0, p.RC1, p.Cout); return SR3_E_BADARG; }
  const int pad = p.ksize / 2;
  const int Hi = p.Hs << p.ups, Wi = p.Ws << p.ups;
  if ((Hi + 2 * pad - p.ksize) / p.stride + 1 != p.Ho || (Wi + 2 * pad - p.ksize) / p.stride + 1 != p.Wo) {
    set_error("conv: output dims %dx%d inconsistent with input %dx%d k%d s%d", p.Ho, p.Wo, Hi, Wi, p.ksize, p.stride);
    return SR3_E_BADARG;
  }
  {
    const double lim = 2147483647.0;
    const double e_in = (double)p.B * p.Hs * p.Ws * (double)(p.C0 > p.C1 ? p.C0 : p.C1);
    const double e_w = (double)p.Cout * p.ksize * p.ksize * (double)Cin;
    const double e_ss = (double)p.B * Cin * 2.0;
    if (e_in >= lim || e_w >= lim || e_ss >= lim) { set_error("conv: tensor exceeds 2^31 elements (32-bit offsets)"); return SR3_E_UNSUPPORTED; }
  }
  const ConvPick pk = conv_pick(p, tile_cfg, ksplit);
  tile_cfg = pk.tile;
  p.ksplit = ksplit = pk.ksplit;
  // write-through stores are buffer stores with 32-bit offsets: an output, or a set of slabs, of 4 GiB or more keeps plain stores
  if (!store_wt_fits((size_t)ksplit * p.B * p.Ho * p.Wo * p.Cout * sizeof(float))) p.store_wt = 0;
  if (p.ostat && ksplit == 1 && (tile_cfg < 5 || tile_cfg >= 22)) { set_error("conv: fused output statistics need the halo kernel or split-K"); return SR3_E_UNSUPPORTED; }
  if (p.ostat && ksplit > 1 && splitk_rows_per_block(p, true) == 0) { set_error("conv: Ho*Wo does not allow fused split-K statistics"); return SR3_E_UNSUPPORTED; }
  p.dbg = env_conv_dbg();
  if (ksplit > 1) {
    const size_t need = (size_t)ksplit * p.B * p.Ho * p.Wo * p.Cout * sizeof(float);
    if (!scratch || scratch_bytes < need) { set_error("conv: split-K scratch too small (%zu < %zu)", scratch_bytes, need); return SR3_E_NOMEM; }
    p.partial = scratch;
  }
  if (p.x2_w && (tile_cfg < 5 || tile_cfg == 11 || tile_cfg >= 22 || p.ups)) { set_error("conv: the fused 1x1 segment needs the halo kernel without upsampling"); return SR3_E_UNSUPPORTED; }
  if (p.x2_w && ((p.x2_C0 & 3) || (p.x2_C1 & 3) || !p.x2_src0 || (p.x2_C1 > 0 && !p.x2_src1))) { set_error("conv: bad x2 segment"); return SR3_E_BADARG; }
  int rc;
  if (tile_cfg == 22) {
    rc = gemm1x1_forward(p, 2, st);
  } else if (tile_cfg == 11) {
    rc = conv3x3_wino_forward(p, p.wino_u, st);
  } else if (tile_cfg >= 5) {
    HaloGeom g;
    if (tile_cfg > 10 || !halo_geometry(p, tile_cfg, &g)) { set_error("conv: halo tile_cfg %d does not fit this problem", tile_cfg); return SR3_E_UNSUPPORTED; }
    const int nchunks = cdiv(Cin, 32);
    if (split_leaves_empty(nchunks, ksplit)) { set_error("conv: ksplit %d leaves an empty split over %d chunks", ksplit, nchunks); return SR3_E_BADARG; }
    rc = conv3x3_halo_forward(p, tile_cfg, g, st);
  } else {
    rc = conv_igemm_forward(p, tile_cfg, st);
  }
  if (rc) return rc;
  if (ksplit > 1) {
    if (mid) SR3_HIP(hipEventRecord(mid, st));
    return splitk_reduce(p, st);
  }
  return SR3_OK;
}

}  // namespace sr3
