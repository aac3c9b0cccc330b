// The loops the attention kernels share (device code only; included by attention.hip, attention_long.hip, attention_heads.hip, attention_bwd.hip).
// A kernel keeps its signature, LDS layout, grid mapping, barriers and epilogue, and composes:
//   qk_scores + emit_scores   scores of KP 32-key blocks, Q / K fragments straight from global memory   (k_attention_v2, k_attention_long, k_attention_heads)
//   pv_accumulate             acc += P_strip V, V fragments straight from global memory                   (k_attention_v2, k_attention_long, k_attention_heads)
//   strip_softmax             exact row softmax of a strip, eight lanes per row                           (k_attention, k_attention_v2, k_attention_heads, k_attention_bwd)
//   max8 / sum8, acc_row, AtVec<TN>, AT_* staging constants                                               (all)
// Every function keeps ONE order of additions: kernels that share a function share its bits.
// The LDS-staged loops of k_attention, k_attention_long_gen and k_attention_bwd are NOT here: no common form keeps the register
// allocation of all three (profiles/attention_core_codegen.txt), so each kernel has its own.
#pragma once
#include "sr3_common.h"

namespace sr3 {

constexpr int AT_LDK = 36;    // Q/K staging row stride (32 + 4 pad floats)
constexpr int AT_LDV = 132;   // V staging row stride (128 + 4)
constexpr int AT_QK_STAGE = (32 + 128) * AT_LDK;     // floats: 32 A rows + 128 B rows of 32 channels
constexpr int AT_V_STAGE = 32 * AT_LDV;              //         32 keys of a 128-channel panel
constexpr int AT_STAGE = AT_QK_STAGE > AT_V_STAGE ? AT_QK_STAGE : AT_V_STAGE;

// TN consecutive channels of one key: what a lane loads for its TN interleaved 32-channel MFMA tiles
template <int TN> struct AtVec;
template <> struct AtVec<1> { typedef float type; };
template <> struct AtVec<2> { typedef float type __attribute__((ext_vector_type(2))); };
template <> struct AtVec<4> { typedef f32x4 type; };
template <int TN> __device__ __forceinline__ float at_elem(const typename AtVec<TN>::type& v, int t) { return v[t]; }
template <> __device__ __forceinline__ float at_elem<1>(const float& v, int) { return v; }
template <int TN> __device__ __forceinline__ typename AtVec<TN>::type at_zero() { typename AtVec<TN>::type z = {}; return z; }
template <> __device__ __forceinline__ float at_zero<1>() { return 0.f; }

__device__ __forceinline__ f32x4 ldf4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
// row of a 32x32 MFMA tile that accumulator register r of a lane holds (the column is lane & 31); kh = 4 * (lane >> 5).
// A kernel that already holds kh as the first k of its operand fragments passes that variable, so the compiler shares the
// row-times-stride products; the staged kernels pass the expression.
__device__ __forceinline__ int acc_row(int r, int kh) { return (r & 3) + 8 * (r >> 2) + kh; }
// maximum / sum over the eight lanes that share a strip row (tid >> 3)
__device__ __forceinline__ float max8(float v) {
  v = fmaxf(v, __shfl_xor(v, 1));
  v = fmaxf(v, __shfl_xor(v, 2));
  return fmaxf(v, __shfl_xor(v, 4));
}
__device__ __forceinline__ float sum8(float v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  return v + __shfl_xor(v, 4);
}

// acc[p] = Q_block K_block(p)^T over all C channels, operands in fragment form from global memory.  qrow / krow[p]: this lane's
// query / key row (lane & 31) at its first channel -- (lane >> 5) * 4 (fp32: a lane's operand for 4 consecutive k-steps of
// v_mfma_f32_32x32x2_f32 is 16 contiguous bytes) or (lane >> 5) * 8 (SPLIT: 8 k of v_mfma_f32_32x32x16_bf16, three bf16 terms per
// operand, six products).  The KP key blocks share the Q fragment; 32 channels of operands stay in flight (the tail re-fetches the
// last group: the loads stay unconditional).  C % 32 == 0.  BLOCKED: every 32 channels go into a fresh accumulator that is then
// added to the total -- C / 32 roundings at the magnitude of the score instead of C (C / 16 x 6 when SPLIT); it changes the bits.
template <int KP, bool SPLIT, bool BLOCKED>
__device__ __forceinline__ void qk_scores(const float* qrow, const float* const (&krow)[KP], int C, f32x16 (&acc)[KP]) {
  constexpr int GK = SPLIT ? 16 : 8;                        // channels per operand group
  constexpr int D = 32 / GK, H = GK / 8;                    // groups in flight; f32x4 per lane, row and group
  const int G = SPLIT ? C >> 4 : C >> 3;
  const f32x16 zero = {};
  f32x16 blk[KP];
  f32x16 (&sc)[KP] = BLOCKED ? blk : acc;
#pragma unroll
  for (int p = 0; p < KP; ++p) acc[p] = blk[p] = zero;
  // (the operand loads are written out twice, not wrapped in a lambda: wrapped, the compiler issues each load in the iteration that
  // uses it and the prefetch distance is gone)
  f32x4 a[D][H], k4[D][KP][H];
#pragma unroll
  for (int d = 0; d < D; ++d)
#pragma unroll
    for (int h = 0; h < H; ++h) {
      a[d][h] = ldf4(qrow + d * GK + h * 4);
#pragma unroll
      for (int p = 0; p < KP; ++p) k4[d][p][h] = ldf4(krow[p] + d * GK + h * 4);
    }
  for (int g0 = 0; g0 < G; g0 += D) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      if constexpr (SPLIT) {
        bf16x8 qa[3];
        split3x8(a[d][0], a[d][1], qa[0], qa[1], qa[2]);
#pragma unroll
        for (int p = 0; p < KP; ++p) {
          bf16x8 kb[3];
          split3x8(k4[d][p][0], k4[d][p][1], kb[0], kb[1], kb[2]);
          mfma_split6(qa, kb, sc[p]);
        }
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int p = 0; p < KP; ++p) sc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[d][0][q], k4[d][p][0][q], sc[p], 0, 0, 0);
      }
      const int gn = min(g0 + d + D, G - 1) * GK;
#pragma unroll
      for (int h = 0; h < H; ++h) {
        a[d][h] = ldf4(qrow + gn + h * 4);
#pragma unroll
        for (int p = 0; p < KP; ++p) k4[d][p][h] = ldf4(krow[p] + gn + h * 4);
      }
    }
    if constexpr (BLOCKED) {
#pragma unroll
      for (int p = 0; p < KP; ++p) { acc[p] += sc[p]; sc[p] = zero; }
    }
  }
}

// strip[row][key] = acc / sqrt_c for this lane's 16 rows of a 32x32 score tile (key = the tile's column of this lane; kh: see acc_row)
__device__ __forceinline__ void emit_scores(float* strip, int stride, int key, int kh, const f32x16& acc, float sqrt_c) {
#pragma unroll
  for (int r = 0; r < 16; ++r) strip[acc_row(r, kh) * stride + key] = acc[r] / sqrt_c;
}

// acc[t] += P V over `groups` groups of 8 (SPLIT: 16) keys.  prow: this lane's strip row (lane & 31) at key (lane >> 5) * 4
// (SPLIT: * 8).  load_first(d, q) / load_v(g, q): the TN channels of this lane at key q of the lane's half of group d / g -- two
// functors for one value, because the first 32 keys have compile-time d and q: the strip kernel addresses them with one product
// each, (d GK + q) * rowstride, and the later ones as (g GK) * rowstride + q * rowstride, and the compiler's load schedule depends
// on it; the key-blocked kernel passes its clamped-and-selected loader twice.  The wave's TN 32-channel tiles take INTERLEAVED
// channels c0 + TN n + t (tile t, column n), so one load feeds all TN tiles.  32 keys of V stay in flight; the tail re-fetches
// the last group.
template <int TN, bool SPLIT, class LoadFirst, class LoadV>
__device__ __forceinline__ void pv_accumulate(const float* prow, LoadFirst load_first, LoadV load_v, int groups, f32x16 (&acc)[TN]) {
  constexpr int GK = SPLIT ? 16 : 8, D = 32 / GK, Q = GK / 2;
  typename AtVec<TN>::type vb[D][Q];
#pragma unroll
  for (int d = 0; d < D; ++d)
#pragma unroll
    for (int q = 0; q < Q; ++q) vb[d][q] = load_first(d, q);
  for (int g0 = 0; g0 < groups; g0 += D) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const f32x4 p0 = ldf4(prow + (g0 + d) * GK);
      if constexpr (SPLIT) {
        const f32x4 p1 = ldf4(prow + (g0 + d) * GK + 4);
        bf16x8 pa[3];
        split3x8(p0, p1, pa[0], pa[1], pa[2]);
#pragma unroll
        for (int t = 0; t < TN; ++t) {
          const f32x4 v0 = {at_elem<TN>(vb[d][0], t), at_elem<TN>(vb[d][1], t), at_elem<TN>(vb[d][2], t), at_elem<TN>(vb[d][3], t)};
          const f32x4 v1 = {at_elem<TN>(vb[d][4], t), at_elem<TN>(vb[d][5], t), at_elem<TN>(vb[d][6], t), at_elem<TN>(vb[d][7], t)};
          bf16x8 vv[3];
          split3x8(v0, v1, vv[0], vv[1], vv[2]);
          mfma_split6(pa, vv, acc[t]);
        }
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int t = 0; t < TN; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(p0[q], at_elem<TN>(vb[d][q], t), acc[t], 0, 0, 0);
      }
      const int gn = min(g0 + d + D, groups - 1);
#pragma unroll
      for (int q = 0; q < Q; ++q) vb[d][q] = load_v(gn, q);
    }
  }
}

// In-place exact softmax of strip rows over their N valid keys; columns N .. npad - 1 become 0.  Thread (row = tid >> 3, sub = tid & 7).
__device__ __forceinline__ void strip_softmax(float* strip, int stride, int tid, int N, int npad) {
  const int row = tid >> 3, sub = tid & 7;
  float* sr = strip + row * stride;
  float mx = -INFINITY;
  for (int k = sub; k < N; k += 8) mx = fmaxf(mx, sr[k]);
  mx = max8(mx);
  float sum = 0.f;
  for (int k = sub; k < N; k += 8) { const float e = expf(sr[k] - mx); sr[k] = e; sum += e; }
  sum = sum8(sum);
  for (int k = sub; k < N; k += 8) sr[k] = sr[k] / sum;
  for (int k = N + sub; k < npad; k += 8) sr[k] = 0.f;
}

}  // namespace sr3
