// Multi-head self-attention (the reference SelfAttention's n_head, model/sr3_modules/unet.py:113-142): H heads of d = C / H channels
// over the NHWC qkv tensor [B][N][3C].  The module views qkv as (batch, n_head, 3 d, h, w) and chunks the 3 d, so head h owns channels
// [3 d h, 3 d (h + 1)) of a row as q_h | k_h | v_h;  S_h = Q_h K_h^T / sqrt(C) -- the divisor is the FULL channel count, as in the
// module --, P_h = softmax_keys(S_h), and O_h = P_h V_h goes to channels [d h, d (h + 1)) of out [B][N][C].  H = 1 is attention.hip.
//
// k_attention_heads<TN, KP, SPLIT>: heads of d = 32 TN channels (64 or 32), any N the 32-query score strip holds (N <= 1248).
//   One 4-wave workgroup owns 32 query rows of one (image, head) pair; workgroups are numbered so that a pair's land on one XCD when
//   the pair count is a multiple of 8 (k_attention_v2's mapping: the pair's K / V are what its workgroups share).
//   phase 1  scores into the LDS strip S[32][Npad + 4]: the 32-key blocks go round the four waves (KP of them share a Q fragment),
//            operands straight from global memory in fragment form -- attention_core.h's qk_scores over the d channels;
//   phase 2  attention_core.h's exact row softmax;
//   phase 3  O = P V has only TN 32-channel tiles, too few for four waves, so the KEYS are split: wave w multiplies its contiguous
//            quarter of the 32-key blocks (pv_accumulate, the wave's TN tiles on interleaved channels), waves 1-3 park their partial
//            tiles in LDS (over the strip, which is dead by then), and wave 0 adds them in wave order and stores.  One order of
//            additions, no atomics: bitwise reproducible.
//   Ragged N: a key or query row >= N is read from row N - 1 (a valid address); such a key's score column is zeroed by the softmax
//   and its V row replaced by zeros, such a query row is not stored.
//   SPLIT: both contractions on v_mfma_f32_32x32x16_bf16 with 3 x bf16 operands (six products, fp32 accumulation), as k_attention_v2's.
// Every other head width runs on the MH instantiations of the single-head kernels (attention_forward_strided): d % 128 == 0 on the
// staging-free kernels, any d % 4 == 0 on the LDS-staged fp32 kernel, and every width under mode bit 1 (key-blocked).
#include "attention_core.h"
#include "train.h"

namespace sr3 {

constexpr int AH_RED = 3 * 16 * 64;       // floats per 32-channel tile of the three parked partials

template <int TN, int KP, bool SPLIT>
__global__ __launch_bounds__(256) void k_attention_heads(const float* __restrict__ qkv, int pairs, int N, int heads,
                                                          float* __restrict__ out) {
  extern __shared__ f32x4 smem_v[];
  float* S = reinterpret_cast<float*>(smem_v);              // [32][Npad + 4]; after phase 3: [3 waves][TN][16][64] partial tiles
  constexpr int d = 32 * TN;
  const int Npad = (N + 31) & ~31, LDS_S = Npad + 4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int qblocks = Npad >> 5;
  int pr, qb;                                               // (image, head) pair and query block of this workgroup
  if ((pairs & 7) == 0) {
    const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
    pr = xcd + 8 * (j / qblocks);
    qb = j % qblocks;
  } else {
    pr = blockIdx.x / qblocks;
    qb = blockIdx.x % qblocks;
  }
  const int b = pr / heads, hd = pr % heads;
  const int m0 = qb * 32;
  const int Ct = d * heads, rowstride = 3 * Ct;
  const float* base = qkv + (size_t)b * N * rowstride + hd * 3 * d;
  const int ln = lane & 31, kh = (lane >> 5) * 4;
  const int koff = SPLIT ? (lane >> 5) * 8 : kh;            // first k of this lane's operand fragments
  const float sqrt_c = sqrtf((float)Ct);
  const int KB = Npad >> 5;                                 // 32-key blocks (the last one may be ragged)

  // ---------------- phase 1 ----------------
  {
    const float* qrow = base + (size_t)min(m0 + ln, N - 1) * rowstride + koff;
    for (int kb0 = wave * KP; kb0 < KB; kb0 += 4 * KP) {
      const float* krow[KP];
#pragma unroll
      for (int p = 0; p < KP; ++p) krow[p] = base + (size_t)min(min(kb0 + p, KB - 1) * 32 + ln, N - 1) * rowstride + d + koff;
      f32x16 acc[KP];
      qk_scores<KP, SPLIT, false>(qrow, krow, d, acc);
#pragma unroll
      for (int p = 0; p < KP; ++p)
        if (kb0 + p < KB) emit_scores(S, LDS_S, (kb0 + p) * 32 + ln, kh, acc[p], sqrt_c);
    }
  }
  __syncthreads();

  // ---------------- phase 2: row softmax (columns N .. Npad - 1 become 0) ----------------
  strip_softmax(S, LDS_S, tid, N, Npad);
  __syncthreads();

  // ---------------- phase 3: this wave's quarter of the keys ----------------
  typedef typename AtVec<TN>::type vec_t;
  constexpr int GK = SPLIT ? 16 : 8;                        // keys per operand group
  f32x16 acc[TN];
#pragma unroll
  for (int t = 0; t < TN; ++t)
#pragma unroll
    for (int r_ = 0; r_ < 16; ++r_) acc[t][r_] = 0.f;
  {
    const int kb_lo = (wave * KB) >> 2, kb_hi = ((wave + 1) * KB) >> 2;
    const int key0 = kb_lo * 32 + koff;
    const float* vbase = base + 2 * d + TN * ln;
    auto vload = [&](int g, int q) {                         // a key >= N: row N - 1, replaced by zeros
      const int key = key0 + g * GK + q;
      const vec_t v = *reinterpret_cast<const vec_t*>(vbase + (size_t)min(key, N - 1) * rowstride);
      return key < N ? v : at_zero<TN>();
    };
    if (kb_hi > kb_lo) pv_accumulate<TN, SPLIT>(S + ln * LDS_S + key0, vload, vload, (kb_hi - kb_lo) * (32 / GK), acc);
  }
  __syncthreads();                                            // the strip is dead: its memory takes the partial tiles

  // ---------------- fixed-order reduce over the four waves, store ----------------
  if (wave > 0) {
#pragma unroll
    for (int t = 0; t < TN; ++t)
#pragma unroll
      for (int r_ = 0; r_ < 16; ++r_) S[(((wave - 1) * TN + t) * 16 + r_) * 64 + lane] = acc[t][r_];
  }
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int w = 0; w < 3; ++w)
#pragma unroll
      for (int t = 0; t < TN; ++t)
#pragma unroll
        for (int r_ = 0; r_ < 16; ++r_) acc[t][r_] += S[((w * TN + t) * 16 + r_) * 64 + lane];
    float* orow = out + ((size_t)b * N + m0) * Ct + hd * d + TN * ln;
#pragma unroll
    for (int r_ = 0; r_ < 16; ++r_) {
      const int row = acc_row(r_, kh);
      vec_t o;
      if constexpr (TN == 1) o = acc[0][r_];
      else {
#pragma unroll
        for (int t = 0; t < TN; ++t) o[t] = acc[t][r_];
      }
      if (m0 + row < N) *reinterpret_cast<vec_t*>(orow + (size_t)row * Ct) = o;
    }
  }
}

namespace {
// LDS bytes of k_attention_heads: the score strip, or the three parked partials where that is more
inline size_t attention_heads_smem(int N, int d) {
  const size_t strip = (size_t)32 * (((N + 31) & ~31) + 4), red = (size_t)AH_RED * (d / 32);
  return (strip > red ? strip : red) * sizeof(float);
}
inline bool attention_heads_fits(int N, int d) { return (d == 64 || d == 32) && N > 0 && attention_heads_smem(N, d) <= 160 * 1024; }

int launch_attention_heads(const float* qkv, int B, int N, int d, int heads, float* out, hipStream_t st, bool split) {
  using Kernel = decltype(&k_attention_heads<1, 1, false>);
  static constexpr Kernel kernels[2][2][2] = {{{k_attention_heads<1, 1, false>, k_attention_heads<1, 1, true>},
                                               {k_attention_heads<1, 2, false>, k_attention_heads<1, 2, true>}},
                                              {{k_attention_heads<2, 1, false>, k_attention_heads<2, 1, true>},
                                               {k_attention_heads<2, 2, false>, k_attention_heads<2, 2, true>}}};
  static std::atomic<uint64_t> done[2][2][2];
  const int qblocks = (N + 31) / 32;
  const int ti = d == 64, pi = qblocks >= 8;                // two key blocks per wave and round share the Q fragment
  const Kernel kern = kernels[ti][pi][split];
  if (int rc = ensure_max_lds(reinterpret_cast<const void*>(kern), 160 * 1024, done[ti][pi][split])) return rc;
  hipLaunchKernelGGL(kern, dim3((unsigned)qblocks * B * heads), dim3(256), attention_heads_smem(N, d), st, qkv, B * heads, N, heads, out);
  SR3_LAUNCH_CHECK("k_attention_heads");
  return SR3_OK;
}
}  // namespace

int attention_heads_check(const char* who, int C, int heads) {
  if (heads < 1) { set_error("%s: heads %d < 1", who, heads); return SR3_E_BADARG; }
  if (C <= 0 || C % heads) { set_error("%s: %d channels do not divide into %d heads", who, C, heads); return SR3_E_BADARG; }
  if ((C / heads) & 3) { set_error("%s: head width %d (%d channels / %d heads) is not a multiple of 4", who, C / heads, C, heads); return SR3_E_UNSUPPORTED; }
  return SR3_OK;
}

int attention_forward_heads(const float* qkv, int B, int N, int C, int heads, float* out, hipStream_t st, int mode) {
  if (int rc = attention_heads_check("attention", C, heads)) return rc;
  if (heads == 1) return attention_forward(qkv, B, N, C, out, st, mode & 3);
  if (B <= 0 || N <= 0) { set_error("attention: needs B, N > 0"); return SR3_E_UNSUPPORTED; }
  if ((double)B * N * 3.0 * C >= 2147483647.0) { set_error("attention: qkv exceeds 2^31 elements"); return SR3_E_UNSUPPORTED; }
  if ((long)B * heads > 65535) { set_error("attention: %d images x %d heads exceed the grid (65535 pairs)", B, heads); return SR3_E_UNSUPPORTED; }
  const int d = C / heads;
  if (!(mode & 6) && attention_heads_fits(N, d)) return launch_attention_heads(qkv, B, N, d, heads, out, st, (mode & 1) != 0);
  return attention_forward_strided(qkv, B, N, C, heads, out, st, mode & 3);
}

}  // namespace sr3

extern "C" int sr3_attention_heads_f32(const float* qkv, int B, int N, int C, int heads, float* out, int mode, void* stream) {
  if (!qkv || !out) { sr3::set_error("null argument"); return SR3_E_BADARG; }
  return sr3::attention_forward_heads(qkv, B, N, C, heads, out, static_cast<hipStream_t>(stream), mode);
}
extern "C" int sr3_attention_bwd_heads_f32(const float* qkv, const float* dout, const float* out_fwd, int B, int N, int C, int heads,
                                           float* dqkv, void* scratch, size_t scratch_bytes, void* stream) {
  if (!qkv || !dout || !dqkv || !scratch) { sr3::set_error("null argument"); return SR3_E_BADARG; }
  if ((uintptr_t)scratch & 15) { sr3::set_error("attention_bwd: scratch is not 16-byte aligned"); return SR3_E_ALIGN; }
  if (int rc = sr3::attention_heads_check("attention_bwd", C, heads)) return rc;
  if ((long)B * heads > 65535) { sr3::set_error("attention_bwd: %d images x %d heads exceed the grid (65535 pairs)", B, heads); return SR3_E_UNSUPPORTED; }
  return sr3::attention_backward(qkv, dout, out_fwd, B, N, C, dqkv, static_cast<hipStream_t>(stream), static_cast<float*>(scratch),
                                 scratch_bytes, heads);
}
