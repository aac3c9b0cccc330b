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
// Phases 1 and 3 of k_attention_long are the loops of attention_core.h (qk_scores with the blocked sum, pv_accumulate with the
// clamped-and-selected V loader); the chunk walk, the online softmax, the epilogue and k_attention_long_gen's staged loops are this file's.
// k_attention_long<TN, SPLIT>: C % 128 == 0 (SPLIT: 3 x bf16 split arithmetic on v_mfma_f32_32x32x16_bf16, six products, fp32
// accumulation; otherwise v_mfma_f32_32x32x2_f32).  k_attention_long_gen: any C % 4 == 0, the LDS-staged fp32-MFMA form of
// k_attention with the same chunk walk (one 128-channel panel per workgroup).
#include "attention_core.h"

namespace sr3 {

constexpr int AL_KC = 512;            // keys per chunk
constexpr int AL_LDS = AL_KC + 4;     // strip row stride (floats)
constexpr int AL_STRIP = 32 * AL_LDS;

// phase 2 of one chunk (both kernels): S holds the scores of keys [0, kvalid) of the chunk, kpad = kvalid rounded up to 32.
// Thread (row = tid >> 3, sub = tid & 7); m_run / l_run are that row's running maximum / sum (the same in its eight lanes).
__device__ __forceinline__ void al_chunk_softmax(float* S, float* alpha_s, int tid, int kvalid, int kpad, float& m_run, float& l_run) {
  const int row = tid >> 3, sub = tid & 7;
  float* sr = S + row * AL_LDS;
  float mx = -INFINITY;
  for (int k = sub; k < kvalid; k += 8) mx = fmaxf(mx, sr[k]);
  mx = max8(mx);
  const float m_new = fmaxf(m_run, mx);
  const float alpha = expf(m_run - m_new);          // first chunk: exp(-inf) = 0
  float sum = 0.f;
  for (int k = sub; k < kvalid; k += 8) { const float e = expf(sr[k] - m_new); sr[k] = e; sum += e; }
  sum = sum8(sum);
  for (int k = kvalid + sub; k < kpad; k += 8) sr[k] = 0.f;
  l_run = alpha * l_run + sum;
  m_run = m_new;
  if (sub == 0) alpha_s[row] = alpha;
}

// MH (both kernels): as k_attention's -- C is one head's width, blockIdx.x / qblocks the (image, head) pair.
template <int TN, bool SPLIT, bool MH>
__global__ __launch_bounds__(256, 2) void k_attention_long(const float* __restrict__ qkv, int N, int C, int qblocks,
                                                            float* __restrict__ out, int heads) {
  extern __shared__ f32x4 smem_v[];
  float* S = reinterpret_cast<float*>(smem_v);              // [32][AL_LDS]
  float* alpha_s = S + AL_STRIP;                            // [32] this chunk's rescale factors
  float* l_s = alpha_s + 32;                                // [32] final sums
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bh = blockIdx.x / qblocks, m0 = (blockIdx.x % qblocks) * 32;
  const int b = MH ? bh / heads : bh, hd = MH ? bh % heads : 0;
  const int Ct = MH ? C * heads : C;                        // channels of an out row
  const int rowstride = 3 * Ct;
  const float* base = qkv + (size_t)b * N * rowstride + (MH ? hd * 3 * C : 0);
  const int ln = lane & 31, kh = (lane >> 5) * 4;
  const int koff = SPLIT ? (lane >> 5) * 8 : kh;            // first k of this lane's operand fragments
  const float sqrt_c = sqrtf((float)Ct);
  constexpr int KP = 2;                                     // key blocks per wave and round (they share the Q fragment)
  constexpr int GK = SPLIT ? 16 : 8;                        // keys per operand group of phase 3
  typedef typename AtVec<TN>::type vec_t;
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

    // ---------------- phase 1: scores of the chunk (blocked channel sum) ----------------
    for (int kb0 = wave * KP; kb0 < KB; kb0 += 4 * KP) {
      const float* krow[KP];
#pragma unroll
      for (int p = 0; p < KP; ++p) krow[p] = base + (size_t)min(k0 + min(kb0 + p, KB - 1) * 32 + ln, N - 1) * rowstride + C + koff;
      f32x16 tot[KP];
      qk_scores<KP, SPLIT, true>(base + qoff + koff, krow, C, tot);
#pragma unroll
      for (int p = 0; p < KP; ++p)
        if (kb0 + p < KB) emit_scores(S, AL_LDS, (kb0 + p) * 32 + ln, kh, tot[p], sqrt_c);
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
      auto vload = [&](int g, int q) {                       // a key >= N: row N - 1, replaced by zeros
        const int key = k0 + g * GK + koff + q;
        const vec_t v = *reinterpret_cast<const vec_t*>(vbase + (size_t)min(key, N - 1) * rowstride);
        return key < N ? v : at_zero<TN>();
      };
      pv_accumulate<TN, SPLIT>(S + ln * AL_LDS + koff, vload, vload, KB * (32 / GK), acc);
    }
    __syncthreads();                                          // the strip and alpha are free for the next chunk
  }

  // ---------------- epilogue: O = acc / l ----------------
  if ((tid & 7) == 0) l_s[tid >> 3] = l_run;
  __syncthreads();
  float* orow = out + ((size_t)b * N + m0) * Ct + (MH ? hd * C : 0) + c0 + TN * ln;
#pragma unroll
  for (int r_ = 0; r_ < 16; ++r_) {
    const int row = acc_row(r_, kh);
    const float l = l_s[row];
    vec_t o;
    if constexpr (TN == 1) o = acc[0][r_] / l;
    else {
#pragma unroll
      for (int t = 0; t < TN; ++t) o[t] = acc[t][r_] / l;
    }
    if (m0 + row < N) *reinterpret_cast<vec_t*>(orow + (size_t)row * Ct) = o;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Any C % 4 == 0: k_attention's LDS-staged fp32-MFMA form (single staging buffer) with the chunk walk.  gridDim.y = 128-channel
// panels of the output; each recomputes the scores (these shapes are the small test networks').
// ---------------------------------------------------------------------------------------------------------------
template <bool MH>
__global__ __launch_bounds__(256) void k_attention_long_gen(const float* __restrict__ qkv, int N, int C, int qblocks,
                                                             float* __restrict__ out, int heads) {
  extern __shared__ f32x4 smem_v[];
  float* S = reinterpret_cast<float*>(smem_v);              // [32][AL_LDS]
  float* stg = S + AL_STRIP;                                // [AT_STAGE]
  float* alpha_s = stg + AT_STAGE;                         // [32]
  float* l_s = alpha_s + 32;                                // [32]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bh = blockIdx.x / qblocks, m0 = (blockIdx.x % qblocks) * 32;
  const int b = MH ? bh / heads : bh, hd = MH ? bh % heads : 0;
  const int Ct = MH ? C * heads : C;                        // channels of an out row
  const int cp = blockIdx.y * 128;                          // this workgroup's channel panel
  const int rowstride = 3 * Ct;
  const float* base = qkv + (size_t)b * N * rowstride + (MH ? hd * 3 * C : 0);
  const int kq = tid & 7, lrow = tid >> 3;                  // loaders: 8 float4 per 32-channel row
  const int ln = lane & 31, kh = (lane >> 5) * 4;
  const float sqrt_c = sqrtf((float)Ct);
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
        float* Ks = Qs + 32 * AT_LDK;
        *reinterpret_cast<f32x4*>(&Qs[lrow * AT_LDK + kq * 4]) = qok ? rq : zero;
#pragma unroll
        for (int i = 0; i < 4; ++i)
          *reinterpret_cast<f32x4*>(&Ks[(lrow + 32 * i) * AT_LDK + kq * 4]) = kok[i] ? rk[i] : zero;
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
          const float* Ks = Qs + 32 * AT_LDK;
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(&Qs[ln * AT_LDK + kk * 8 + kh]);
            const f32x4 k4 = *reinterpret_cast<const f32x4*>(&Ks[(wave * 32 + ln) * AT_LDK + kk * 8 + kh]);
#pragma unroll
            for (int q = 0; q < 4; ++q) sc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q], k4[q], sc, 0, 0, 0);
          }
          if ((s % nc) == nc - 1) {           // last channel chunk of this key block: emit the scores
            const int key = kb + wave * 32 + ln;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              S[acc_row(r, kh) * AL_LDS + key] = sc[r] / sqrt_c;
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
      for (int r = 0; r < 16; ++r) acc[r] *= alpha_s[acc_row(r, kh)];
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
          *reinterpret_cast<f32x4*>(&stg[((tid >> 5) + 8 * i) * AT_LDV + (tid & 31) * 4]) = vok[i] ? rv[i] : zero;
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
              const float bv = stg[(kk * 8 + kh + q) * AT_LDV + wave * 32 + ln];
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
    const int row = acc_row(r, kh);
    const int m = m0 + row;
    if (wave_out && m < N && c < C) out[((size_t)b * N + m) * Ct + (MH ? hd * C : 0) + c] = acc[r] / l_s[row];
  }
}

namespace {
// k_attention_long<TN, SPLIT> by (tn, split): one table, one launcher
#define SR3_AL_ROWS(MH) \
  {{k_attention_long<1, false, MH>, k_attention_long<1, true, MH>}, {k_attention_long<2, false, MH>, k_attention_long<2, true, MH>}, \
   {k_attention_long<4, false, MH>, k_attention_long<4, true, MH>}}
int launch_attention_long(int tn, bool split, const float* qkv, int B, int N, int C, int zsplit, float* out, hipStream_t st, int heads) {
  using Kernel = decltype(&k_attention_long<1, false, false>);
  static constexpr Kernel kernels[2][3][2] = {SR3_AL_ROWS(false), SR3_AL_ROWS(true)};
  static std::atomic<uint64_t> done[2][3][2];
  const int ti = tn >> 1;                                   // 1, 2, 4 -> 0, 1, 2
  const bool mh = heads > 1;
  const Kernel kern = kernels[mh][ti][split];
  const int smem = (AL_STRIP + 64) * (int)sizeof(float);
  if (int rc = ensure_max_lds(reinterpret_cast<const void*>(kern), smem, done[mh][ti][split])) return rc;
  const int qblocks = (N + 31) / 32;
  hipLaunchKernelGGL(kern, dim3((unsigned)qblocks * B, zsplit), dim3(256), smem, st, qkv, N, C, qblocks, out, heads);
  SR3_LAUNCH_CHECK("k_attention_long");
  return SR3_OK;
}
#undef SR3_AL_ROWS
}  // namespace

// heads > 1: C is one head's width (the rows hold heads * C channels), every (image, head) pair a grid entry of its own
int attention_long_forward(const float* qkv, int B, int N, int C, float* out, hipStream_t st, bool split, int heads) {
  B *= heads;
  if (B <= 0 || N <= 0 || C <= 0 || (C & 3)) { set_error("attention: needs B, N > 0 and C %% 4 == 0"); return SR3_E_UNSUPPORTED; }
  const int qblocks = (N + 31) / 32;
  if (C % 128 == 0) {
    // channels per workgroup: the largest of 512 / 256 / 128 that divides C (the accumulators of a wave are 16 TN registers), halved
    // while the grid would leave CUs idle (each channel slice recomputes the scores)
    int cz = (C % 512 == 0) ? 512 : ((C % 256 == 0) ? 256 : 128);
    while ((long)qblocks * B * (C / cz) < 256 && cz > 128) cz >>= 1;
    const int zsplit = C / cz;
    return launch_attention_long(cz / 128, split, qkv, B, N, C, zsplit, out, st, heads);
  }
  static std::atomic<uint64_t> done[2];
  const bool mh = heads > 1;
  auto kern = mh ? k_attention_long_gen<true> : k_attention_long_gen<false>;
  const int smem = (AL_STRIP + AT_STAGE + 64) * (int)sizeof(float);
  if (int rc = ensure_max_lds(reinterpret_cast<const void*>(kern), smem, done[mh])) return rc;
  hipLaunchKernelGGL(kern, dim3((unsigned)qblocks * B, (C + 127) / 128), dim3(256), smem, st, qkv, N, C, qblocks, out, heads);
  SR3_LAUNCH_CHECK("k_attention_long_gen");
  return SR3_OK;
}

}  // namespace sr3
