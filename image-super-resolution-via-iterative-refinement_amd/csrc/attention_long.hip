// Key-blocked single-head attention: O = softmax(Q K^T / sqrt(C)) V for ANY token count N, with LDS use independent of N.
// (attention.hip keeps a 32-query score strip over ALL keys in LDS, which ends at about 1088 tokens; plan option attn_long and
// bit 1 of attention_forward's mode select this file.)
//
// One 4-wave workgroup owns 32 query rows of one image (and one channel slice of the output: gridDim.y) and walks the keys in chunks
// of AL_KC = 512.  Per chunk:
//   phase 1  scores of the chunk into the LDS strip S[32][AL_KC + 4] (as k_attention_v2: operands straight from global memory in
//            fragment form, two key blocks per wave share the Q fragment).  The channel sum is BLOCKED: 32 channels at a time go
//            into a fresh accumulator that is then added to the total -- C / 32 roundings at the magnitude of the score instead of
//            C (C / 16 x 6 on the split path).  At thousands of tokens some logits are in the thousands, where one fp32 ulp of the
//            score is 5e-4 of a probability: the plain chain's error in the scores is what bounds the output's accuracy there;
//   phase 2  online softmax: eight lanes per query row keep the row's running maximum m and running sum l in registers; the chunk's
//            scores become p = exp(s - m_new) in place, l = alpha l + sum(p) with alpha = exp(m_old - m_new), alpha goes to LDS;
//   phase 3  acc = alpha acc + P_chunk V_chunk, the accumulators (32 rows x 128 TN channels per wave = 16 TN registers per lane,
//            TN <= 4) living in registers across the chunks.
// After the last chunk the accumulators are divided by l and the rows < N are stored.  No atomics, fixed summation order: bitwise
// reproducible.  66 KB of LDS: two workgroups per CU (one's softmax runs beside the other's MFMA).
// Ragged N (N % 32 != 0): a key >= N is loaded from row N - 1 (a valid address) and discarded -- its score is overwritten with
// p = 0 before the maximum is taken, its V row is replaced by zeros by a select; a query row >= N computes on row N - 1 and is
// not stored.
// k_attention_long<TN, SPLIT>: C % 128 == 0 (SPLIT: 3 x bf16 split arithmetic on v_mfma_f32_32x32x16_bf16, six products, fp32
// accumulation; otherwise v_mfma_f32_32x32x2_f32).  k_attention_long_gen: any C % 4 == 0, the LDS-staged fp32-MFMA form of
// k_attention with the same chunk walk (one 128-channel panel per workgroup).
#include "sr3_common.h"

namespace sr3 {

constexpr int AL_KC = 512;            // keys per chunk
constexpr int AL_LDS = AL_KC + 4;     // strip row stride (floats)
constexpr int AL_STRIP = 32 * AL_LDS;

template <int TN> struct AlVec;
template <> struct AlVec<1> { typedef float type; };
template <> struct AlVec<2> { typedef float type __attribute__((ext_vector_type(2))); };
template <> struct AlVec<4> { typedef f32x4 type; };
template <int TN> __device__ __forceinline__ float al_elem(const typename AlVec<TN>::type& v, int t) { return v[t]; }
template <> __device__ __forceinline__ float al_elem<1>(const float& v, int) { return v; }
template <int TN> __device__ __forceinline__ typename AlVec<TN>::type al_zero() { typename AlVec<TN>::type z = {}; return z; }
template <> __device__ __forceinline__ float al_zero<1>() { return 0.f; }

// phase 2 of one chunk (both kernels): S holds the scores of keys [0, kvalid) of the chunk, kpad = kvalid rounded up to 32.
// Thread (row = tid >> 3, sub = tid & 7); m_run / l_run are that row's running maximum / sum (the same in its eight lanes).
__device__ __forceinline__ void al_chunk_softmax(float* S, float* alpha_s, int tid, int kvalid, int kpad, float& m_run, float& l_run) {
  const int row = tid >> 3, sub = tid & 7;
  float* sr = S + row * AL_LDS;
  float mx = -INFINITY;
  for (int k = sub; k < kvalid; k += 8) mx = fmaxf(mx, sr[k]);
  mx = fmaxf(mx, __shfl_xor(mx, 1));
  mx = fmaxf(mx, __shfl_xor(mx, 2));
  mx = fmaxf(mx, __shfl_xor(mx, 4));
  const float m_new = fmaxf(m_run, mx);
  const float alpha = expf(m_run - m_new);          // first chunk: exp(-inf) = 0
  float sum = 0.f;
  for (int k = sub; k < kvalid; k += 8) { const float e = expf(sr[k] - m_new); sr[k] = e; sum += e; }
  sum += __shfl_xor(sum, 1);
  sum += __shfl_xor(sum, 2);
  sum += __shfl_xor(sum, 4);
  for (int k = kvalid + sub; k < kpad; k += 8) sr[k] = 0.f;
  l_run = alpha * l_run + sum;
  m_run = m_new;
  if (sub == 0) alpha_s[row] = alpha;
}

template <int TN, bool SPLIT>
__global__ __launch_bounds__(256, 2) void k_attention_long(const float* __restrict__ qkv, int N, int C, int qblocks,
                                                            float* __restrict__ out) {
  extern __shared__ f32x4 smem_v[];
  float* S = reinterpret_cast<float*>(smem_v);              // [32][AL_LDS]
  float* alpha_s = S + AL_STRIP;                            // [32] this chunk's rescale factors
  float* l_s = alpha_s + 32;                                // [32] final sums
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / qblocks, m0 = (blockIdx.x % qblocks) * 32;
  const int rowstride = 3 * C;
  const float* base = qkv + (size_t)b * N * rowstride;
  const int ln = lane & 31, kh = (lane >> 5) * 4, k8 = (lane >> 5) * 8;
  const float sqrt_c = sqrtf((float)C);
  constexpr int KP = 2;                                     // key blocks per wave and round (they share the Q fragment)
  constexpr int D = 4, DS = 2;                              // operand groups in flight (fp32 / split)
  typedef typename AlVec<TN>::type vec_t;
  const int c0 = blockIdx.y * (128 * TN) + wave * (32 * TN);                            // this wave's 32 TN channels
  const size_t qoff = (size_t)min(m0 + ln, N - 1) * rowstride;
  const float* vbase = base + 2 * C + c0 + TN * ln;

  f32x16 acc[TN];
#pragma unroll
  for (int t = 0; t < TN; ++t)
#pragma unroll
    for (int r_ = 0; r_ < 16; ++r_) acc[t][r_] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;

  for (int k0 = 0; k0 < N; k0 += AL_KC) {
    const int kvalid = min(AL_KC, N - k0);
    const int KB = (kvalid + 31) >> 5;                      // 32-key blocks of this chunk (the last one may be ragged)

    // ---------------- phase 1: scores of the chunk ----------------
    if constexpr (SPLIT) {
      const int G = C >> 4;                                 // groups of 16 channels = one bf16 MFMA k-step; G % 2 == 0 (C % 128 == 0)
      const float* qrow = base + qoff + k8;
      for (int kb0 = wave * KP; kb0 < KB; kb0 += 4 * KP) {
        const float* krow[KP];
#pragma unroll
        for (int p = 0; p < KP; ++p) krow[p] = base + (size_t)min(k0 + min(kb0 + p, KB - 1) * 32 + ln, N - 1) * rowstride + C + k8;
        f32x16 sc[KP], tot[KP];                             // sc: the current block of 32 channels; tot: the sum of the blocks
#pragma unroll
        for (int p = 0; p < KP; ++p)
#pragma unroll
          for (int r_ = 0; r_ < 16; ++r_) sc[p][r_] = tot[p][r_] = 0.f;
        f32x4 a[DS][2], k4[DS][KP][2];
#pragma unroll
        for (int d = 0; d < DS; ++d)
#pragma unroll
          for (int hlf = 0; hlf < 2; ++hlf) {
            a[d][hlf] = *reinterpret_cast<const f32x4*>(qrow + d * 16 + hlf * 4);
#pragma unroll
            for (int p = 0; p < KP; ++p) k4[d][p][hlf] = *reinterpret_cast<const f32x4*>(krow[p] + d * 16 + hlf * 4);
          }
        for (int g0 = 0; g0 < G; g0 += DS) {
#pragma unroll
          for (int d = 0; d < DS; ++d) {
            bf16x8 qa[3];
            split3x8(a[d][0], a[d][1], qa[0], qa[1], qa[2]);
#pragma unroll
            for (int p = 0; p < KP; ++p) {
              bf16x8 kb[3];
              split3x8(k4[d][p][0], k4[d][p][1], kb[0], kb[1], kb[2]);
              mfma_split6(qa, kb, sc[p]);
            }
            const int gn = min(g0 + d + DS, G - 1) * 16;      // (the tail re-fetches the last group: the loads stay unconditional)
#pragma unroll
            for (int hlf = 0; hlf < 2; ++hlf) {
              a[d][hlf] = *reinterpret_cast<const f32x4*>(qrow + gn + hlf * 4);
#pragma unroll
              for (int p = 0; p < KP; ++p) k4[d][p][hlf] = *reinterpret_cast<const f32x4*>(krow[p] + gn + hlf * 4);
            }
          }
#pragma unroll
          for (int p = 0; p < KP; ++p)
#pragma unroll
            for (int r_ = 0; r_ < 16; ++r_) { tot[p][r_] += sc[p][r_]; sc[p][r_] = 0.f; }
        }
#pragma unroll
        for (int p = 0; p < KP; ++p) {
          if (kb0 + p < KB) {
            const int key = (kb0 + p) * 32 + ln;
#pragma unroll
            for (int r_ = 0; r_ < 16; ++r_) S[((r_ & 3) + 8 * (r_ >> 2) + kh) * AL_LDS + key] = tot[p][r_] / sqrt_c;
          }
        }
      }
    } else {
      const int G = C >> 3;                                 // G % D == 0 (C % 128 == 0)
      const float* qrow = base + qoff + kh;
      for (int kb0 = wave * KP; kb0 < KB; kb0 += 4 * KP) {
        const float* krow[KP];
#pragma unroll
        for (int p = 0; p < KP; ++p) krow[p] = base + (size_t)min(k0 + min(kb0 + p, KB - 1) * 32 + ln, N - 1) * rowstride + C + kh;
        f32x16 sc[KP], tot[KP];                             // sc: the current block of 32 channels; tot: the sum of the blocks
#pragma unroll
        for (int p = 0; p < KP; ++p)
#pragma unroll
          for (int r_ = 0; r_ < 16; ++r_) sc[p][r_] = tot[p][r_] = 0.f;
        f32x4 a[D], k4[D][KP];
#pragma unroll
        for (int d = 0; d < D; ++d) {
          a[d] = *reinterpret_cast<const f32x4*>(qrow + d * 8);
#pragma unroll
          for (int p = 0; p < KP; ++p) k4[d][p] = *reinterpret_cast<const f32x4*>(krow[p] + d * 8);
        }
        for (int g0 = 0; g0 < G; g0 += D) {
#pragma unroll
          for (int d = 0; d < D; ++d) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
              for (int p = 0; p < KP; ++p) sc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[d][q], k4[d][p][q], sc[p], 0, 0, 0);
            const int gn = min(g0 + d + D, G - 1) * 8;
            a[d] = *reinterpret_cast<const f32x4*>(qrow + gn);
#pragma unroll
            for (int p = 0; p < KP; ++p) k4[d][p] = *reinterpret_cast<const f32x4*>(krow[p] + gn);
          }
#pragma unroll
          for (int p = 0; p < KP; ++p)
#pragma unroll
            for (int r_ = 0; r_ < 16; ++r_) { tot[p][r_] += sc[p][r_]; sc[p][r_] = 0.f; }
        }
#pragma unroll
        for (int p = 0; p < KP; ++p) {
          if (kb0 + p < KB) {
            const int key = (kb0 + p) * 32 + ln;
#pragma unroll
            for (int r_ = 0; r_ < 16; ++r_) S[((r_ & 3) + 8 * (r_ >> 2) + kh) * AL_LDS + key] = tot[p][r_] / sqrt_c;
          }
        }
      }
    }
    __syncthreads();

    // ---------------- phase 2: online softmax of the chunk ----------------
    al_chunk_softmax(S, alpha_s, tid, kvalid, KB * 32, m_run, l_run);
    __syncthreads();

    // ---------------- phase 3: acc = alpha acc + P V ----------------
    {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 al = *reinterpret_cast<const f32x4*>(alpha_s + 8 * g + kh);       // rows 8 g + kh + (0..3) = registers 4 g + (0..3)
#pragma unroll
        for (int t = 0; t < TN; ++t)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[t][4 * g + e] *= al[e];
      }
      if constexpr (SPLIT) {
        const int G16 = KB * 2;                               // groups of 16 keys
        const float* prow = S + ln * AL_LDS + k8;
        auto vload = [&](int g, int q) {
          const int key = k0 + g * 16 + k8 + q;
          const vec_t v = *reinterpret_cast<const vec_t*>(vbase + (size_t)min(key, N - 1) * rowstride);
          return key < N ? v : al_zero<TN>();
        };
        vec_t vb[DS][8];
#pragma unroll
        for (int d = 0; d < DS; ++d)
#pragma unroll
          for (int q = 0; q < 8; ++q) vb[d][q] = vload(d, q);
        for (int g0 = 0; g0 < G16; g0 += DS) {
#pragma unroll
          for (int d = 0; d < DS; ++d) {
            const f32x4 p0 = *reinterpret_cast<const f32x4*>(prow + (g0 + d) * 16);
            const f32x4 p1 = *reinterpret_cast<const f32x4*>(prow + (g0 + d) * 16 + 4);
            bf16x8 pa[3];
            split3x8(p0, p1, pa[0], pa[1], pa[2]);
#pragma unroll
            for (int t = 0; t < TN; ++t) {
              const f32x4 v0 = {al_elem<TN>(vb[d][0], t), al_elem<TN>(vb[d][1], t), al_elem<TN>(vb[d][2], t), al_elem<TN>(vb[d][3], t)};
              const f32x4 v1 = {al_elem<TN>(vb[d][4], t), al_elem<TN>(vb[d][5], t), al_elem<TN>(vb[d][6], t), al_elem<TN>(vb[d][7], t)};
              bf16x8 vv[3];
              split3x8(v0, v1, vv[0], vv[1], vv[2]);
              mfma_split6(pa, vv, acc[t]);
            }
            const int gn = min(g0 + d + DS, G16 - 1);          // (the tail re-fetches the last group)
#pragma unroll
            for (int q = 0; q < 8; ++q) vb[d][q] = vload(gn, q);
          }
        }
      } else {
        const int G = KB * 4;                                 // groups of 8 keys
        const float* prow = S + ln * AL_LDS + kh;
        auto vload = [&](int g, int q) {
          const int key = k0 + g * 8 + kh + q;
          const vec_t v = *reinterpret_cast<const vec_t*>(vbase + (size_t)min(key, N - 1) * rowstride);
          return key < N ? v : al_zero<TN>();
        };
        vec_t vb[D][4];
#pragma unroll
        for (int d = 0; d < D; ++d)
#pragma unroll
          for (int q = 0; q < 4; ++q) vb[d][q] = vload(d, q);
        for (int g0 = 0; g0 < G; g0 += D) {
#pragma unroll
          for (int d = 0; d < D; ++d) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(prow + (g0 + d) * 8);
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
              for (int t = 0; t < TN; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q], al_elem<TN>(vb[d][q], t), acc[t], 0, 0, 0);
            const int gn = min(g0 + d + D, G - 1);
#pragma unroll
            for (int q = 0; q < 4; ++q) vb[d][q] = vload(gn, q);
          }
        }
      }
    }
    __syncthreads();                                          // the strip and alpha are free for the next chunk
  }

  // ---------------- epilogue: O = acc / l ----------------
  if ((tid & 7) == 0) l_s[tid >> 3] = l_run;
  __syncthreads();
  float* orow = out + ((size_t)b * N + m0) * C + c0 + TN * ln;
#pragma unroll
  for (int r_ = 0; r_ < 16; ++r_) {
    const int row = (r_ & 3) + 8 * (r_ >> 2) + kh;
    const float l = l_s[row];
    vec_t o;
    if constexpr (TN == 1) o = acc[0][r_] / l;
    else {
#pragma unroll
      for (int t = 0; t < TN; ++t) o[t] = acc[t][r_] / l;
    }
    if (m0 + row < N) *reinterpret_cast<vec_t*>(orow + (size_t)row * C) = o;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Any C % 4 == 0: k_attention's LDS-staged fp32-MFMA form (single staging buffer) with the chunk walk.  gridDim.y = 128-channel
// panels of the output; each recomputes the scores (these shapes are the small test networks').
// ---------------------------------------------------------------------------------------------------------------
constexpr int ALG_LDK = 36;    // Q/K staging row stride (32 + 4 pad floats)
constexpr int ALG_LDV = 132;   // V staging row stride (128 + 4)
constexpr int ALG_QK_STAGE = (32 + 128) * ALG_LDK;
constexpr int ALG_V_STAGE = 32 * ALG_LDV;
constexpr int ALG_STAGE = ALG_QK_STAGE > ALG_V_STAGE ? ALG_QK_STAGE : ALG_V_STAGE;

__global__ __launch_bounds__(256) void k_attention_long_gen(const float* __restrict__ qkv, int N, int C, int qblocks,
                                                             float* __restrict__ out) {
  extern __shared__ f32x4 smem_v[];
  float* S = reinterpret_cast<float*>(smem_v);              // [32][AL_LDS]
  float* stg = S + AL_STRIP;                                // [ALG_STAGE]
  float* alpha_s = stg + ALG_STAGE;                         // [32]
  float* l_s = alpha_s + 32;                                // [32]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / qblocks, m0 = (blockIdx.x % qblocks) * 32;
  const int cp = blockIdx.y * 128;                          // this workgroup's channel panel
  const int rowstride = 3 * C;
  const float* base = qkv + (size_t)b * N * rowstride;
  const int kq = tid & 7, lrow = tid >> 3;                  // loaders: 8 float4 per 32-channel row
  const int ln = lane & 31, kh = (lane >> 5) * 4;
  const float sqrt_c = sqrtf((float)C);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const int nc = (C + 31) / 32;
  const bool wave_out = (cp + wave * 32) < C;

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;

  for (int k0 = 0; k0 < N; k0 += AL_KC) {
    const int kvalid = min(AL_KC, N - k0);
    const int kpad = (kvalid + 31) & ~31;

    // ---------------- phase 1 ----------------
    {
      const int nsteps = ((kpad + 127) / 128) * nc;
      f32x4 rq, rk[4];
      bool qok, kok[4];
      auto load = [&](int s) {
        const int kb = (s / nc) * 128;
        const int c = (s % nc) * 32 + kq * 4;
        const bool cv = c < C;
        const int m = m0 + lrow;
        qok = cv && m < N;
        rq = *reinterpret_cast<const f32x4*>(base + (qok ? m * rowstride + c : 0));
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int key = k0 + kb + lrow + 32 * i;
          kok[i] = cv && key < N;
          rk[i] = *reinterpret_cast<const f32x4*>(base + (kok[i] ? key * rowstride + C + c : 0));
        }
      };
      auto store = [&]() {
        float* Qs = stg;
        float* Ks = Qs + 32 * ALG_LDK;
        *reinterpret_cast<f32x4*>(&Qs[lrow * ALG_LDK + kq * 4]) = qok ? rq : zero;
#pragma unroll
        for (int i = 0; i < 4; ++i)
          *reinterpret_cast<f32x4*>(&Ks[(lrow + 32 * i) * ALG_LDK + kq * 4]) = kok[i] ? rk[i] : zero;
      };
      f32x16 sc;
#pragma unroll
      for (int r = 0; r < 16; ++r) sc[r] = 0.f;
      load(0);
      store();
      __syncthreads();
      for (int s = 0; s < nsteps; ++s) {
        const bool more = s + 1 < nsteps;
        if (more) load(s + 1);
        const int kb = (s / nc) * 128;
        if (kb + wave * 32 < kpad) {
          const float* Qs = stg;
          const float* Ks = Qs + 32 * ALG_LDK;
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(&Qs[ln * ALG_LDK + kk * 8 + kh]);
            const f32x4 k4 = *reinterpret_cast<const f32x4*>(&Ks[(wave * 32 + ln) * ALG_LDK + kk * 8 + kh]);
#pragma unroll
            for (int q = 0; q < 4; ++q) sc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q], k4[q], sc, 0, 0, 0);
          }
          if ((s % nc) == nc - 1) {           // last channel chunk of this key block: emit the scores
            const int key = kb + wave * 32 + ln;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              S[((r & 3) + 8 * (r >> 2) + kh) * AL_LDS + key] = sc[r] / sqrt_c;
              sc[r] = 0.f;
            }
          }
        }
        __syncthreads();
        if (more) store();
        __syncthreads();
      }
    }

    // ---------------- phase 2 ----------------
    al_chunk_softmax(S, alpha_s, tid, kvalid, kpad, m_run, l_run);
    __syncthreads();

    // ---------------- phase 3 ----------------
    {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] *= alpha_s[(r & 3) + 8 * (r >> 2) + kh];
      const int nk = kpad / 32;
      f32x4 rv[4];
      bool vok[4];
      auto load = [&](int s) {
        const int c = cp + (tid & 31) * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int key = k0 + s * 32 + (tid >> 5) + 8 * i;
          vok[i] = key < N && c < C;
          rv[i] = *reinterpret_cast<const f32x4*>(base + (vok[i] ? key * rowstride + 2 * C + c : 0));
        }
      };
      auto store = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          *reinterpret_cast<f32x4*>(&stg[((tid >> 5) + 8 * i) * ALG_LDV + (tid & 31) * 4]) = vok[i] ? rv[i] : zero;
      };
      load(0);
      store();
      __syncthreads();
      for (int s = 0; s < nk; ++s) {
        const bool more = s + 1 < nk;
        if (more) load(s + 1);
        if (wave_out) {
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(&S[ln * AL_LDS + s * 32 + kk * 8 + kh]);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const float bv = stg[(kk * 8 + kh + q) * ALG_LDV + wave * 32 + ln];
              acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q], bv, acc, 0, 0, 0);
            }
          }
        }
        __syncthreads();
        if (more) store();
        __syncthreads();
      }
    }
  }

  if ((tid & 7) == 0) l_s[tid >> 3] = l_run;
  __syncthreads();
  const int c = cp + wave * 32 + ln;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + kh;
    const int m = m0 + row;
    if (wave_out && m < N && c < C) out[((size_t)b * N + m) * C + c] = acc[r] / l_s[row];
  }
}

namespace {
template <int TN, bool SPLIT>
int launch_attention_long(const float* qkv, int B, int N, int C, int zsplit, float* out, hipStream_t st) {
  static std::atomic<uint64_t> done{0};
  const int smem = (AL_STRIP + 64) * (int)sizeof(float);
  auto kern = k_attention_long<TN, SPLIT>;
  if (int rc = ensure_max_lds(reinterpret_cast<const void*>(kern), smem, done)) return rc;
  const int qblocks = (N + 31) / 32;
  hipLaunchKernelGGL(kern, dim3((unsigned)qblocks * B, zsplit), dim3(256), smem, st, qkv, N, C, qblocks, out);
  SR3_LAUNCH_CHECK("k_attention_long");
  return SR3_OK;
}
}  // namespace

int attention_long_forward(const float* qkv, int B, int N, int C, float* out, hipStream_t st, bool split) {
  if (B <= 0 || N <= 0 || C <= 0 || (C & 3)) { set_error("attention: needs B, N > 0 and C %% 4 == 0"); return SR3_E_UNSUPPORTED; }
  const int qblocks = (N + 31) / 32;
  if (C % 128 == 0) {
    // channels per workgroup: the largest of 512 / 256 / 128 that divides C (the accumulators of a wave are 16 TN registers), halved
    // while the grid would leave CUs idle (each channel slice recomputes the scores)
    int cz = (C % 512 == 0) ? 512 : ((C % 256 == 0) ? 256 : 128);
    while ((long)qblocks * B * (C / cz) < 256 && cz > 128) cz >>= 1;
    const int zsplit = C / cz;
    if (cz == 512) return split ? launch_attention_long<4, true>(qkv, B, N, C, zsplit, out, st) : launch_attention_long<4, false>(qkv, B, N, C, zsplit, out, st);
    if (cz == 256) return split ? launch_attention_long<2, true>(qkv, B, N, C, zsplit, out, st) : launch_attention_long<2, false>(qkv, B, N, C, zsplit, out, st);
    return split ? launch_attention_long<1, true>(qkv, B, N, C, zsplit, out, st) : launch_attention_long<1, false>(qkv, B, N, C, zsplit, out, st);
  }
  static std::atomic<uint64_t> done{0};
  const int smem = (AL_STRIP + ALG_STAGE + 64) * (int)sizeof(float);
  if (int rc = ensure_max_lds(reinterpret_cast<const void*>(k_attention_long_gen), smem, done)) return rc;
  hipLaunchKernelGGL(k_attention_long_gen, dim3((unsigned)qblocks * B, (C + 127) / 128), dim3(256), smem, st, qkv, N, C, qblocks, out);
  SR3_LAUNCH_CHECK("k_attention_long_gen");
  return SR3_OK;
}

}  // namespace sr3
