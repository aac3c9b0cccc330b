// Single-head self-attention core of SelfAttention.forward (model/sr3_modules/unet.py:127-139):
//   S = Q K^T / sqrt(C) ; P = softmax_keys(S) ; O = P V          (n_head == 1, head dim == C; more heads: attention_heads.hip, which
//   runs head widths other than 64 / 32 on the MH instantiations of the kernels below)
// qkv is the NHWC output of the 1x1 qkv conv: [B][N][3C] with q | k | v along channels
// (the reference's `.view(b, 1, 3C, h, w).chunk(3, dim=2)`), O is [B][N][C].
//
// One workgroup (4 waves) owns 32 query rows of one image.  N <= 1024 tokens, so a full score
// strip S[32][N] lives in LDS (no online softmax): phase 1 fills it with exact-fp32 MFMA
// (v_mfma_f32_32x32x2_f32, each wave a 32-key block), phase 2 does the row softmax in place,
// phase 3 multiplies the strip with V (each wave a 32-channel block of a 128-channel panel).
// Q/K/V tiles are register-prefetched one step ahead (unconditional loads, masks applied at the
// LDS write) and double-buffered in LDS when the strip leaves room (NSTAGE = 2).  When the grid
// would leave CUs idle, the channel panels of phase 3 are split over gridDim.z workgroups (each
// recomputes the cheap score strip).
// k_attention_v2's two contraction loops and the row softmax of both kernels are attention_core.h's; the LDS-staged loops of
// k_attention are its own.
#include <stdlib.h>

#include "attention_core.h"

namespace sr3 {

// MH (multi-head, attention_heads.hip's dispatch): C is ONE head's width d and blockIdx.y the (image, head) pair; head h owns
// channels [3 d h, 3 d (h + 1)) of a qkv row as q | k | v and [d h, d (h + 1)) of an out row, the rows keep the strides of all
// heads * d channels, and the scale stays sqrt(heads * d).  MH = false compiles to the single-head code as it was.
template <int NSTAGE, bool MH>
__global__ __launch_bounds__(256) void k_attention(const float* __restrict__ qkv, int N, int C,
                                                    float* __restrict__ out, int heads) {
  extern __shared__ f32x4 smem_v[];
  float* smem = reinterpret_cast<float*>(smem_v);
  const int Npad = (N + 31) & ~31;
  const int LDS_S = Npad + 4;
  float* S = smem;                      // [32][LDS_S]
  float* stg = smem + 32 * LDS_S;       // NSTAGE staging buffers

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = MH ? blockIdx.y / heads : blockIdx.y, hd = MH ? blockIdx.y % heads : 0;
  const int Ct = MH ? C * heads : C;              // channels of an out row
  const int m0 = blockIdx.x * 32;
  const int rowstride = 3 * Ct;
  const float* base = qkv + (size_t)b * N * rowstride + (MH ? hd * 3 * C : 0);
  const int kq = tid & 7, lrow = tid >> 3;        // loaders: 8 float4 per 32-channel row
  const int kh = (lane >> 5) * 4;
  const float sqrt_c = sqrtf((float)Ct);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

  // ---------------- phase 1: S = Q K^T / sqrt(C) ----------------
  {
    const int nc = (C + 31) / 32;
    const int nsteps = (Npad / 128 + ((Npad & 127) ? 1 : 0)) * nc;
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
        const int key = kb + lrow + 32 * i;
        kok[i] = cv && key < N;
        rk[i] = *reinterpret_cast<const f32x4*>(base + (kok[i] ? key * rowstride + C + c : 0));
      }
    };
    auto store = [&](int st) {
      float* Qs = stg + st * AT_STAGE;
      float* Ks = Qs + 32 * AT_LDK;
      *reinterpret_cast<f32x4*>(&Qs[lrow * AT_LDK + kq * 4]) = qok ? rq : zero;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        *reinterpret_cast<f32x4*>(&Ks[(lrow + 32 * i) * AT_LDK + kq * 4]) = kok[i] ? rk[i] : zero;
    };
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    load(0);
    store(0);
    __syncthreads();
    for (int s = 0; s < nsteps; ++s) {
      const int cur = (NSTAGE == 2) ? (s & 1) : 0;
      const bool more = s + 1 < nsteps;
      if (more) load(s + 1);
      const int kb = (s / nc) * 128;
      const bool wave_active = (kb + wave * 32) < Npad;
      if (wave_active) {
        const float* Qs = stg + cur * AT_STAGE;
        const float* Ks = Qs + 32 * AT_LDK;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const f32x4 a = *reinterpret_cast<const f32x4*>(&Qs[(lane & 31) * AT_LDK + kk * 8 + kh]);
          const f32x4 k4 = *reinterpret_cast<const f32x4*>(&Ks[(wave * 32 + (lane & 31)) * AT_LDK + kk * 8 + kh]);
#pragma unroll
          for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q], k4[q], acc, 0, 0, 0);
        }
        if ((s % nc) == nc - 1) {           // last channel chunk of this key block: emit the scores
          const int key = kb + wave * 32 + (lane & 31);
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int row = acc_row(r, 4 * (lane >> 5));
            S[row * LDS_S + key] = acc[r] / sqrt_c;
            acc[r] = 0.f;
          }
        }
      }
      if (NSTAGE == 1) __syncthreads();
      if (more) store((NSTAGE == 2) ? (cur ^ 1) : 0);
      __syncthreads();
    }
  }

  // ---------------- phase 2: row softmax over the N valid keys ----------------
  {
    strip_softmax(S, LDS_S, tid, N, Npad);
  }
  __syncthreads();

  // ---------------- phase 3: O = P V  (this workgroup's share of the 128-channel panels) --------
  {
    const int npan = (C + 127) / 128;
    const int pan_per = (npan + gridDim.z - 1) / gridDim.z;
    const int pan0 = blockIdx.z * pan_per;
    const int pan1 = min(npan, pan0 + pan_per);
    const int nk = Npad / 32;
    const int nsteps = (pan1 - pan0) * nk;
    f32x4 rv[4];
    bool vok[4];
    auto load = [&](int s) {
      const int cp = (pan0 + s / nk) * 128;
      const int k0 = (s % nk) * 32;
      const int c = cp + (tid & 31) * 4;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = k0 + (tid >> 5) + 8 * i;
        vok[i] = key < N && c < C;
        rv[i] = *reinterpret_cast<const f32x4*>(base + (vok[i] ? key * rowstride + 2 * C + c : 0));
      }
    };
    auto store = [&](int st) {
      float* Vs = stg + st * AT_STAGE;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        *reinterpret_cast<f32x4*>(&Vs[((tid >> 5) + 8 * i) * AT_LDV + (tid & 31) * 4]) = vok[i] ? rv[i] : zero;
    };
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    if (nsteps > 0) {
      load(0);
      store(0);
    }
    __syncthreads();
    for (int s = 0; s < nsteps; ++s) {
      const int cur = (NSTAGE == 2) ? (s & 1) : 0;
      const bool more = s + 1 < nsteps;
      if (more) load(s + 1);
      const int cp = (pan0 + s / nk) * 128;
      const int k0 = (s % nk) * 32;
      const bool wave_active = (cp + wave * 32) < C;
      if (wave_active) {
        const float* Vs = stg + cur * AT_STAGE;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const f32x4 a = *reinterpret_cast<const f32x4*>(&S[(lane & 31) * LDS_S + k0 + kk * 8 + kh]);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float bv = Vs[(kk * 8 + kh + q) * AT_LDV + wave * 32 + (lane & 31)];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q], bv, acc, 0, 0, 0);
          }
        }
        if ((s % nk) == nk - 1) {           // last key chunk of this panel: write the output block
          const int c = cp + wave * 32 + (lane & 31);
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int m = m0 + acc_row(r, 4 * (lane >> 5));
            if (m < N && c < C) out[((size_t)b * N + m) * Ct + (MH ? hd * C : 0) + c] = acc[r];
            acc[r] = 0.f;
          }
        }
      }
      if (NSTAGE == 1) __syncthreads();
      if (more) store((NSTAGE == 2) ? (cur ^ 1) : 0);
      __syncthreads();
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Round 3: the same computation with NO operand staging -- every MFMA operand except the probabilities comes straight from
// global memory in fragment form, because on this part nothing overlaps the fp32 MFMA (profiles/archive/r03_mfma_overlap.txt), so
// the cheapest operand is the one that costs the fewest instructions:
//   phase 1  S = Q K^T / sqrt(C): a lane's A / B operand for 4 consecutive k-steps is 16 contiguous bytes of ITS query /
//            key row (qkv is channel-contiguous), i.e. one global_load_dwordx4; a key block belongs to exactly one wave, so
//            LDS would only add a write and a read per fragment.  KP key blocks per wave share the Q fragment.
//   phase 2  exact row softmax in the LDS strip (as above).
//   phase 3  O = P V: A = P from the strip (one ds_read_b128 per 4 k-steps); the wave's TN 32-channel MFMA tiles take the
//            INTERLEAVED channels c0 + TN n + t (tile t, column n), so one TN-float load per lane and k-step feeds all TN
//            tiles and the accumulators of a row come out as TN consecutive channels (vector stores).
// No barrier inside either loop; D = 4 operand groups are in flight per wave (the grid is one workgroup per CU, i.e. one wave
// per SIMD: the L2 latency has to be covered inside the wave).  Workgroups are numbered so that all workgroups of an image
// land on ONE XCD (round-robin dispatch: linear id mod 8): its K / V are then fetched into one L2 instead of eight.
// The k order of both contractions is the one of k_attention (bitwise equal results).
// Shapes: N % 32 == 0, N <= 1024, C % 128 == 0, (C / zsplit) % (128 TN) == 0; the rest stays on k_attention.
// ---------------------------------------------------------------------------------------------------------------
// SPLIT (round 5; plan option attn_split): both contractions on v_mfma_f32_32x32x16_bf16 with every fp32 operand as three bf16
// terms and six products per fp32 product, fp32 accumulation -- the arithmetic of the SPLIT conv kernels (fp32-class results,
// gated against float64 in tests/).  A lane's operand is then 8 consecutive k of its row: 32 contiguous bytes of its query / key
// row (phase 1), 8 probabilities of the strip and 8 keys' worth of its TN channels (phase 3), split in registers; D = 2 groups
// of 16 k in flight.
// MH: as k_attention's -- C is one head's width, B the number of (image, head) pairs (the XCD mapping keeps a PAIR on one XCD: its K / V
// are what its workgroups share).
template <int KP, int TN, bool SPLIT, bool MH>
__global__ __launch_bounds__(256) void k_attention_v2(const float* __restrict__ qkv, int B, int N, int C, int zsplit,
                                                       float* __restrict__ out, int heads) {
  extern __shared__ f32x4 smem_v[];
  float* S = reinterpret_cast<float*>(smem_v);              // [32][N + 4]
  const int LDS_S = N + 4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // (query block, channel split, image) of this workgroup; B % 8 == 0: image = xcd + 8 * (...), xcd = linear id mod 8
  const int qblocks = N >> 5, per_img = qblocks * zsplit;
  int b, r;
  if ((B & 7) == 0) {
    const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
    b = xcd + 8 * (j / per_img);
    r = j % per_img;
  } else {
    b = blockIdx.x / per_img;
    r = blockIdx.x % per_img;
  }
  const int m0 = (r % qblocks) * 32, zi = r / qblocks;
  int hd = 0;
  if constexpr (MH) { hd = b % heads; b /= heads; }
  const int Ct = MH ? C * heads : C;                        // channels of an out row
  const int rowstride = 3 * Ct;
  const float* base = qkv + (size_t)b * N * rowstride + (MH ? hd * 3 * C : 0);
  const int ln = lane & 31, kh = (lane >> 5) * 4;
  const float sqrt_c = sqrtf((float)Ct);
  constexpr int D = 4;                                      // operand groups in flight

  // ---------------- phase 1 ----------------
  {
    const int KB = N >> 5;
    const int koff = SPLIT ? (lane >> 5) * 8 : kh;          // first channel of this lane's operand fragments
    const float* qrow = base + (size_t)(m0 + ln) * rowstride + koff;
    for (int kb0 = wave * KP; kb0 < KB; kb0 += 4 * KP) {
      const float* krow[KP];
#pragma unroll
      for (int p = 0; p < KP; ++p) krow[p] = base + (size_t)(min(kb0 + p, KB - 1) * 32 + ln) * rowstride + C + koff;
      f32x16 acc[KP];
      qk_scores<KP, SPLIT, false>(qrow, krow, C, acc);
#pragma unroll
      for (int p = 0; p < KP; ++p)
        if (kb0 + p < KB) emit_scores(S, LDS_S, (kb0 + p) * 32 + ln, kh, acc[p], sqrt_c);
    }
  }
  __syncthreads();

  // ---------------- phase 2: row softmax ----------------
  {
    strip_softmax(S, LDS_S, tid, N, N);
  }
  __syncthreads();

  // ---------------- phase 3 ----------------
  {
    typedef typename AtVec<TN>::type vec_t;
    const int Cz = C / zsplit;
    const int cz0 = zi * Cz;
    for (int cw = wave * 32 * TN; cw < Cz; cw += 4 * 32 * TN) {
      const int c0 = cz0 + cw;
      f32x16 acc[TN];
#pragma unroll
      for (int t = 0; t < TN; ++t)
#pragma unroll
        for (int r_ = 0; r_ < 16; ++r_) acc[t][r_] = 0.f;
      constexpr int GK = SPLIT ? 16 : 8;                      // keys per operand group
      const int koff = SPLIT ? (lane >> 5) * 8 : kh;
      const float* vcol = base + 2 * C + c0 + TN * ln + (size_t)koff * rowstride;       // key koff, this lane's TN channels
      pv_accumulate<TN, SPLIT>(S + ln * LDS_S + koff,
          [&](int d, int q) { return *reinterpret_cast<const vec_t*>(vcol + (size_t)(d * GK + q) * rowstride); },
          [&](int g, int q) { return *reinterpret_cast<const vec_t*>(vcol + (size_t)(g * GK) * rowstride + (size_t)q * rowstride); },
          N >> (SPLIT ? 4 : 3), acc);
      float* orow = out + ((size_t)b * N + m0) * Ct + (MH ? hd * C : 0) + c0 + TN * ln;
#pragma unroll
      for (int r_ = 0; r_ < 16; ++r_) {
        const int row = acc_row(r_, kh);
        vec_t o;
        if constexpr (TN == 1) o = acc[0][r_];
        else {
#pragma unroll
          for (int t = 0; t < TN; ++t) o[t] = acc[t][r_];
        }
        *reinterpret_cast<vec_t*>(orow + (size_t)row * Ct) = o;
      }
    }
  }
}

namespace {
// k_attention_v2<KP, TN, SPLIT> by (pairs, tn, split): one table, one launcher
// (heads > 1: the MH instantiations, C one head's width and B the (image, head) pairs)
using AttnV2Kernel = decltype(&k_attention_v2<1, 1, false, false>);
#define SR3_V2_ROW(KP, MH) \
  {{k_attention_v2<KP, 1, false, MH>, k_attention_v2<KP, 1, true, MH>}, {k_attention_v2<KP, 2, false, MH>, k_attention_v2<KP, 2, true, MH>}, \
   {k_attention_v2<KP, 4, false, MH>, k_attention_v2<KP, 4, true, MH>}}
int launch_attention_v2(bool pairs, int tn, bool split, const float* qkv, int B, int N, int C, int zsplit, float* out, hipStream_t st,
                        int heads = 1) {
  static constexpr AttnV2Kernel kernels[2][2][3][2] = {{SR3_V2_ROW(1, false), SR3_V2_ROW(2, false)}, {SR3_V2_ROW(1, true), SR3_V2_ROW(2, true)}};
  static std::atomic<uint64_t> done[2][2][3][2];
  const int ti = tn >> 1;                                   // 1, 2, 4 -> 0, 1, 2
  const bool mh = heads > 1;
  const AttnV2Kernel kern = kernels[mh][pairs][ti][split];
  const int smem = 32 * (N + 4) * (int)sizeof(float);
  if (int rc = ensure_max_lds(reinterpret_cast<const void*>(kern), 160 * 1024, done[mh][pairs][ti][split])) return rc;
  hipLaunchKernelGGL(kern, dim3((unsigned)((N / 32) * B * zsplit)), dim3(256), smem, st, qkv, B, N, C, zsplit, out, heads);
  SR3_LAUNCH_CHECK("k_attention_v2");
  return SR3_OK;
}
#undef SR3_V2_ROW
}  // namespace

namespace {
inline bool attention_v2_fits(int N, int C) { return (N & 31) == 0 && N <= 1024 && (C % 128) == 0; }
// LDS bytes of k_attention<nstage> for N tokens (score strip + staging buffers)
inline size_t attention_v1_smem(int N, int nstage) { return ((size_t)32 * (((N + 31) & ~31) + 4) + (size_t)nstage * AT_STAGE) * sizeof(float); }
}  // namespace

bool attention_fits(int N, int C) {
  if (N <= 0 || (C & 3)) return false;
  return attention_v2_fits(N, C) || attention_v1_smem(N, 1) <= 160 * 1024;
}

namespace {
// the strip kernels for `heads` heads of C channels each (heads == 1: the single-head instantiations; otherwise B counts (image, head) pairs)
int attention_strip(const float* qkv, int B, int N, int C, float* out, hipStream_t st, int split, int heads);
}  // namespace

int attention_forward(const float* qkv, int B, int N, int C, float* out, hipStream_t st, int mode) {
  if (C & 3) { set_error("attention: C %% 4 != 0"); return SR3_E_UNSUPPORTED; }
  if ((double)B * N * 3.0 * C >= 2147483647.0) { set_error("attention: qkv exceeds 2^31 elements"); return SR3_E_UNSUPPORTED; }
  const int split = mode & 1;
  if (mode & 2) return attention_long_forward(qkv, B, N, C, out, st, split != 0);     // the key-blocked kernel, at any N
  return attention_strip(qkv, B, N, C, out, st, split, 1);
}

// heads > 1 on the generalised kernels (attention_heads.hip dispatches: its own kernel takes the 64- and 32-channel heads first)
int attention_forward_strided(const float* qkv, int B, int N, int C, int heads, float* out, hipStream_t st, int mode) {
  const int d = C / heads;
  if (mode & 2) return attention_long_forward(qkv, B, N, d, out, st, (mode & 1) != 0, heads);
  return attention_strip(qkv, B * heads, N, d, out, st, mode & 1, heads);
}

namespace {
int attention_strip(const float* qkv, int B, int N, int C, float* out, hipStream_t st, int split, int heads) {
  // the staging-free kernel wherever the shape allows it (SR3_ATTN_V1=1, read once: A/B knob for the profiles)
  static const bool force_v1 = [] { const char* e = getenv("SR3_ATTN_V1"); return e && e[0] == '1'; }();
  if (!force_v1 && attention_v2_fits(N, C)) {
    const int qblocks = N / 32;
    int zsplit = 1;                                       // channel split of phase 3 (each split recomputes the score strip)
    while ((long)qblocks * B * zsplit < 256 && (C / (zsplit * 2)) % 128 == 0 && zsplit < 4) zsplit *= 2;
    const int Cz = C / zsplit;
    const int tn = (Cz % 512 == 0) ? 4 : ((Cz % 256 == 0) ? 2 : 1);
    const bool pairs = N / 32 >= 8;                       // two key blocks per wave and round share the Q fragment
    return launch_attention_v2(pairs, tn, split != 0, qkv, B, N, C, zsplit, out, st, heads);
  }
  int nstage = 2;
  size_t smem = attention_v1_smem(N, 2);
  if (smem > 160 * 1024) { nstage = 1; smem = attention_v1_smem(N, 1); }
  if (smem > 160 * 1024) { set_error("attention: N=%d does not fit the LDS score strip", N); return SR3_E_UNSUPPORTED; }
  const int qblocks = (N + 31) / 32;
  const int npan = (C + 127) / 128;
  int zsplit = 1;
  while (zsplit * 2 <= npan && (long)qblocks * B * zsplit < 256) zsplit *= 2;
  static std::atomic<uint64_t> attr_done[2][3];
  const bool mh = heads > 1;
  auto kern = mh ? (nstage == 2 ? k_attention<2, true> : k_attention<1, true>) : (nstage == 2 ? k_attention<2, false> : k_attention<1, false>);
  // the attribute is an upper bound: allow the whole 160 KB LDS once per (instantiation, device)
  if (int rc = ensure_max_lds(reinterpret_cast<const void*>(kern), 160 * 1024, attr_done[mh][nstage])) return rc;
  hipLaunchKernelGGL(kern, dim3(qblocks, B, zsplit), dim3(256), smem, st, qkv, N, C, out, heads);
  SR3_LAUNCH_CHECK("k_attention");
  return SR3_OK;
}
}  // namespace

}  // namespace sr3
