// Guided sampling (include/sr3_mi355x.h: sr3_cond_drop_f32, sr3_abs_quantile_f32, sr3_guided_step): classifier-free guidance (Ho & Salimans
// 2022) and dynamic thresholding (Saharia et al. 2022, section 2.3) in the tail of a reverse step, and the conditioning dropout that trains
// a model for it.
//
// The step (j = step2_dev[1] on entry, n = C H W values per image):
//
//   out = out_c                                             one forward (out_u NULL)
//   out = add_rn(out_u, mul_rn(scale, sub_rn(out_c, out_u)))   two forwards: the conditional one and the one on a zero condition
//   x0  = sub_rn(mul_rn(a[j], x), mul_rn(b[j], out))        step_x0 of sr3_common.h, without its clamp
//   mode 0: x0' = x0 ;  mode 1: x0' = clamp(x0, -1, 1) ;
//   mode 2: s_b = fmaxf(1, q_b), q_b = the abs-quantile of image b's x0 ;  x0' = __fdiv_rn(clamp(x0, -s_b, s_b), s_b)
//   x   = step_mix<HIST>(x0', x, z, hist) ; hist <- x0' ; step2_dev[1] = j - 1
//
// The abs-quantile is an exact order statistic: with the ranks (rank_lo, frac) the host computed from the percentile,
//   q = (float)((double) v_lo + frac * ((double) v_hi - (double) v_lo)),   v_lo, v_hi = the rank_lo-th and (rank_lo + 1)-th smallest |x0|
// (q = v_lo itself where v_hi == v_lo or frac == 0: what the formula gives for every finite value, and no inf - inf or 0 * inf for an
// infinite one).  The bit patterns of non-negative floats order like unsigned integers, so v_lo is found by a radix select on the
// 31-bit key  bits & 0x7fffffff  in three passes of 11 / 10 / 10 bits: a pass counts, in a histogram in LDS, the digit of every value whose
// higher digits are the ones already chosen, then the bin that holds the wanted rank is chosen and the rank reduced to one inside it.
// v_hi needs no pass of its own: it is v_lo again when the last bin holds another value past the rank (a tie), else the next non-empty
// bin of the last histogram, else the smallest key whose upper 21 bits exceed v_lo's -- an integer minimum the last pass takes along.
// Counters are integers (LDS and global atomics): their sums do not depend on the order, the result is bitwise reproducible.
//
// Work split.  n <= Q_SINGLE_MAX: one workgroup per image runs the three passes and the finish in ONE launch, everything in LDS.  Larger
// images: Q_CHUNK values per workgroup, one launch per pass -- k_q_init (zero the global histograms), k_q_hist<0..2> (histogram of the
// chunk in LDS, the non-empty bins added to the image's global histogram; each workgroup first chooses the earlier passes' bins from
// the global histograms the earlier launches completed: 2048 + 1024 counters out of the L2, no hand-off inside a launch), k_q_out.
// A NaN is a key above inf's; every index is a masked digit, so whatever the values are the kernels stay inside their buffers.
#include "step_tail.h"

namespace sr3 {
namespace {

constexpr int QT = 256;                  // threads of every workgroup here (four wavefronts of 64)
constexpr int Q_BINS = 2048;             // bins of the widest pass; the stride of one pass's histogram in the scratch
constexpr int Q_CHUNK = 4096;            // split form: values per workgroup (16 per thread)
constexpr int Q_SINGLE_MAX = 8192;       // the single-workgroup form runs images up to this many values (32 per thread and pass)
constexpr unsigned Q_NONE = 0xffffffffu; // no key: above every key, NaNs included

__host__ __device__ constexpr int q_shift(int p) { return p == 0 ? 20 : p == 1 ? 10 : 0; }
__host__ __device__ constexpr int q_nbins(int p) { return p == 0 ? 2048 : 1024; }

__device__ __forceinline__ unsigned q_key(float v) { return __float_as_uint(v) & 0x7fffffffu; }

// the bin that holds rank k of a histogram, k's rank inside that bin, the bin's count, and the next non-empty bin above it (or Q_NONE)
struct QPick { unsigned bin, k, cnt, next; };

// All QT threads call it.  h: NB counters in LDS or in global memory (complete: written before the last barrier / by an earlier launch),
// their sum > k; tmp: 8 words of LDS.  A thread owns NB / QT consecutive bins; an inclusive scan over the wavefront (__shfl_up) and
// the four wavefronts' totals give every thread the count below its first bin, and the one thread whose bins straddle k publishes.
template <int NB>
__device__ QPick block_pick(const unsigned* h, unsigned k, unsigned* tmp) {
  constexpr int PER = NB / QT;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  unsigned c[PER], sum = 0;
#pragma unroll
  for (int i = 0; i < PER; ++i) { c[i] = h[t * PER + i]; sum += c[i]; }
  unsigned inc = sum;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned o = __shfl_up(inc, d);
    if (lane >= d) inc += o;
  }
  if (lane == 63) tmp[w] = inc;
  if (t == 0) { tmp[4] = 0; tmp[5] = 0; tmp[6] = 0; tmp[7] = Q_NONE; }      // (k beyond the sum: bin 0, never an index out of range)
  __syncthreads();
  unsigned excl = inc - sum;
  for (int i = 0; i < w; ++i) excl += tmp[i];
  if (excl <= k && k - excl < sum) {
    unsigned r = k - excl;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      if (r < c[i]) { tmp[4] = t * PER + i; tmp[5] = r; tmp[6] = c[i]; break; }
      r -= c[i];
    }
  }
  __syncthreads();
  const unsigned bin = tmp[4];
  unsigned nx = Q_NONE;
#pragma unroll
  for (int i = PER - 1; i >= 0; --i) {
    if (c[i] != 0 && (unsigned)(t * PER + i) > bin) nx = t * PER + i;
  }
  if (nx != Q_NONE) atomicMin(&tmp[7], nx);
  __syncthreads();
  const QPick r = {bin, tmp[5], tmp[6], tmp[7]};
  __syncthreads();                       // (tmp is free for the next call)
  return r;
}

// pass P over src[lo, hi): count digit P of every key whose digits above it are key_hi's; the last pass also keeps the smallest key
// whose upper digits are greater (a candidate for v_hi).  lh: the pass's histogram in LDS, zeroed and behind a barrier.
template <int P>
__device__ __forceinline__ void q_accumulate(const float* src, unsigned lo, unsigned hi, unsigned key_hi, unsigned* lh, unsigned& above) {
  for (unsigned i = lo + threadIdx.x; i < hi; i += QT) {
    const unsigned key = q_key(src[i]);
    if constexpr (P == 0) {
      atomicAdd(&lh[key >> q_shift(0)], 1u);
    } else {
      const unsigned top = key >> q_shift(P - 1), want = key_hi >> q_shift(P - 1);
      if (top == want) atomicAdd(&lh[(key >> q_shift(P)) & (q_nbins(P) - 1)], 1u);
      else if (P == 2 && top > want && key < above) above = key;
    }
  }
}

__device__ __forceinline__ void q_zero(unsigned* lh, int nb) {
  for (int i = threadIdx.x; i < nb; i += QT) lh[i] = 0;
  __syncthreads();
}

// the keys of v_lo and v_hi -> the quantile, one rounding; each double operation rounded on its own (opaque: never one half of an fma)
__device__ __forceinline__ float q_lerp(unsigned lo, unsigned hi, double frac) {
  const float v_lo = __uint_as_float(lo);
  if (hi == lo || frac == 0.0) return v_lo;
  double d = (double)__uint_as_float(hi) - (double)v_lo;
  asm volatile("" : "+v"(d));
  double m = frac * d;
  asm volatile("" : "+v"(m));
  return (float)((double)v_lo + m);
}

// after the last pass: pk = its pick, key_hi = v_lo's key, above = the smallest key beyond the last histogram's range or Q_NONE
__device__ __forceinline__ unsigned q_v_hi(const QPick& pk, unsigned key_hi, unsigned above) {
  if (pk.k + 1 < pk.cnt) return key_hi;                                          // the next rank sits in v_lo's own bin: a tie
  if (pk.next != Q_NONE) return (key_hi & ~(unsigned)(q_nbins(2) - 1)) | pk.next;
  return above != Q_NONE ? above : key_hi;                                       // (nothing above: rank_lo is the last rank)
}

template <int P>
__device__ __forceinline__ void q_single_pass(const float* p, unsigned n, unsigned* lh, unsigned* tmp, unsigned& key_hi, unsigned& k,
                                              unsigned& above, QPick& pk) {
  q_zero(lh, q_nbins(P));
  q_accumulate<P>(p, 0, n, key_hi, lh, above);
  __syncthreads();
  pk = block_pick<q_nbins(P)>(lh, k, tmp);
  key_hi |= pk.bin << q_shift(P);
  k = pk.k;
}

// one workgroup per image, everything in one launch
__global__ __launch_bounds__(QT) void k_q_single(const float* __restrict__ src, unsigned n, unsigned rank_lo, double frac,
                                                  float* __restrict__ out) {
  __shared__ unsigned lh[Q_BINS];
  __shared__ unsigned tmp[8];
  __shared__ unsigned s_above;
  const float* p = src + (size_t)blockIdx.x * n;
  unsigned key_hi = 0, k = rank_lo, above = Q_NONE;
  QPick pk;
  if (threadIdx.x == 0) s_above = Q_NONE;
  q_single_pass<0>(p, n, lh, tmp, key_hi, k, above, pk);
  q_single_pass<1>(p, n, lh, tmp, key_hi, k, above, pk);
  q_single_pass<2>(p, n, lh, tmp, key_hi, k, above, pk);
  if (above != Q_NONE) atomicMin(&s_above, above);
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = q_lerp(key_hi, q_v_hi(pk, key_hi, s_above), frac);
}

// ---- the split form.  Scratch: [bpad floats: a result slot per image for sr3_guided_step][bpad words: min-above][batch x 3 x Q_BINS
// counters], bpad = batch rounded up to 4 ----
__host__ __device__ inline size_t q_bpad(int batch) { return ((size_t)batch + 3) & ~(size_t)3; }
inline size_t q_scratch_words(int batch) { return 2 * q_bpad(batch) + (size_t)batch * 3 * Q_BINS; }

// min-above <- Q_NONE, counters <- 0: `words` words from the min-above block on, the first `bpad` of them the min-above block
__global__ __launch_bounds__(QT) void k_q_init(unsigned* __restrict__ w, unsigned bpad, unsigned words) {
  const unsigned i = blockIdx.x * QT + threadIdx.x;
  if (i < words) w[i] = i < bpad ? Q_NONE : 0u;
}

// the bins the passes before P chose, from the image's global histograms (complete: earlier launches wrote them)
template <int P>
__device__ __forceinline__ QPick q_replay(const unsigned* gh, unsigned* tmp, unsigned& key_hi, unsigned& k) {
  QPick pk = {0, 0, 0, Q_NONE};
  if constexpr (P >= 1) { pk = block_pick<q_nbins(0)>(gh, k, tmp); key_hi |= pk.bin << q_shift(0); k = pk.k; }
  if constexpr (P >= 2) { pk = block_pick<q_nbins(1)>(gh + Q_BINS, k, tmp); key_hi |= pk.bin << q_shift(1); k = pk.k; }
  if constexpr (P >= 3) { pk = block_pick<q_nbins(2)>(gh + 2 * Q_BINS, k, tmp); key_hi |= pk.bin << q_shift(2); k = pk.k; }
  return pk;
}

// workgroup = (image, chunk): pass P over the chunk, added to the image's histogram P
template <int P>
__global__ __launch_bounds__(QT) void k_q_hist(const float* __restrict__ src, unsigned n, unsigned chunks, unsigned rank_lo,
                                                unsigned* minab, unsigned* hist) {
  __shared__ unsigned lh[Q_BINS];
  __shared__ unsigned tmp[8];
  const unsigned b = blockIdx.x / chunks, c = blockIdx.x % chunks;
  unsigned* gh = hist + (size_t)b * 3 * Q_BINS;
  unsigned key_hi = 0, k = rank_lo, above = Q_NONE;
  q_replay<P>(gh, tmp, key_hi, k);
  q_zero(lh, q_nbins(P));
  const unsigned lo = c * Q_CHUNK, hi = n - lo < (unsigned)Q_CHUNK ? n : lo + Q_CHUNK;
  q_accumulate<P>(src + (size_t)b * n, lo, hi, key_hi, lh, above);
  __syncthreads();
  for (int i = threadIdx.x; i < q_nbins(P); i += QT) {
    if (lh[i] != 0) atomicAdd(&gh[P * Q_BINS + i], lh[i]);
  }
  if (P == 2 && above != Q_NONE) atomicMin(&minab[b], above);
}

// one workgroup per image: the three picks again, then the finish
__global__ __launch_bounds__(QT) void k_q_out(unsigned rank_lo, double frac, const unsigned* minab, const unsigned* hist,
                                               float* __restrict__ out) {
  __shared__ unsigned tmp[8];
  unsigned key_hi = 0, k = rank_lo;
  const QPick pk = q_replay<3>(hist + (size_t)blockIdx.x * 3 * Q_BINS, tmp, key_hi, k);
  if (threadIdx.x == 0) out[blockIdx.x] = q_lerp(key_hi, q_v_hi(pk, key_hi, minab[blockIdx.x]), frac);
}

// the arguments of a select, before anything is launched (who: the entry's name in the message)
int check_quantile(const char* who, int batch, int n, int rank_lo, double frac, const void* scratch, size_t scratch_bytes) {
  if (batch <= 0 || n <= 0) { set_error("%s: batch and the values per image must be positive (got %d, %d)", who, batch, n); return SR3_E_BADARG; }
  if ((size_t)batch * (size_t)n >= ((size_t)1 << 31)) { set_error("%s: image batch too large (batch * values per image >= 2^31)", who); return SR3_E_UNSUPPORTED; }
  if (rank_lo < 0 || rank_lo >= n) { set_error("%s: rank_lo must lie in [0, %d) (got %d)", who, n, rank_lo); return SR3_E_BADARG; }
  if (!(frac >= 0.0 && frac < 1.0)) { set_error("%s: frac must lie in [0, 1) (got %g)", who, frac); return SR3_E_BADARG; }
  if (!scratch) { set_error("%s: scratch is NULL", who); return SR3_E_BADARG; }
  const size_t need = q_scratch_words(batch) * sizeof(unsigned);
  if (scratch_bytes < need) { set_error("%s: scratch_bytes %zu is too small (sr3_abs_quantile_scratch_bytes: %zu)", who, scratch_bytes, need); return SR3_E_BADARG; }
  if ((uintptr_t)scratch & 3) { set_error("misaligned pointer (scratch: 4 B)"); return SR3_E_ALIGN; }
  return SR3_OK;
}

// out[b] = the abs-quantile of src[b, 0 .. n): the body of sr3_abs_quantile_f32 and of sr3_guided_step's mode 2 (arguments checked)
int abs_quantile(const float* src, int batch, int n, int rank_lo, double frac, float* out, void* scratch, hipStream_t st) {
  if (n <= Q_SINGLE_MAX) {
    hipLaunchKernelGGL(k_q_single, dim3(batch), dim3(QT), 0, st, src, (unsigned)n, (unsigned)rank_lo, frac, out);
    SR3_LAUNCH_CHECK("k_q_single");
    return SR3_OK;
  }
  const unsigned bpad = (unsigned)q_bpad(batch);
  unsigned* minab = static_cast<unsigned*>(scratch) + bpad;
  unsigned* hist = minab + bpad;
  const unsigned words = bpad + (unsigned)batch * 3 * Q_BINS;
  const unsigned chunks = ((unsigned)n + Q_CHUNK - 1) / Q_CHUNK;
  const dim3 grid((unsigned)batch * chunks);
  hipLaunchKernelGGL(k_q_init, dim3((words + QT - 1) / QT), dim3(QT), 0, st, minab, bpad, words);
  hipLaunchKernelGGL(k_q_hist<0>, grid, dim3(QT), 0, st, src, (unsigned)n, chunks, (unsigned)rank_lo, minab, hist);
  hipLaunchKernelGGL(k_q_hist<1>, grid, dim3(QT), 0, st, src, (unsigned)n, chunks, (unsigned)rank_lo, minab, hist);
  hipLaunchKernelGGL(k_q_hist<2>, grid, dim3(QT), 0, st, src, (unsigned)n, chunks, (unsigned)rank_lo, minab, hist);
  hipLaunchKernelGGL(k_q_out, dim3(batch), dim3(QT), 0, st, (unsigned)rank_lo, frac, minab, hist, out);
  SR3_LAUNCH_CHECK("k_q_hist");
  return SR3_OK;
}

// ---- conditioning dropout: dst[b] = keep[b] ? src[b] : +0.0, moved as words (a bit copy) ----
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

template <int V>
__global__ __launch_bounds__(256) void k_cond_drop(const unsigned* src, const int* __restrict__ keep, unsigned per, unsigned* dst,
                                                    unsigned total) {
  const unsigned e = (blockIdx.x * 256u + threadIdx.x) * V;
  if (e >= total) return;
  const bool kp = keep[e / per] != 0;
  if constexpr (V == 4) {
    u32x4 v = {0u, 0u, 0u, 0u};
    if (kp) v = *reinterpret_cast<const u32x4*>(src + e);
    *reinterpret_cast<u32x4*>(dst + e) = v;
  } else {
    dst[e] = kp ? src[e] : 0u;
  }
}

// ---- the guided step ----
struct GuidedStep {
  StepFuse f;                // the step's tail on x; step_cur: step_copy put j there (clip: `mode` rules)
  const float* out_c;        // the network's output on the real condition
  const float* out_u;        // ... on the zero condition, or null: no guidance
  float scale;
  int mode;                  // 0 x0 as it is, 1 clamp to [-1, 1], 2 dynamic threshold
  float* x0;                 // mode 2: x0 of the whole batch (k_guided_x0 writes it, the select and k_guided_mix read it)
  const float* q;            // mode 2: the abs-quantile per image
  float* thr;                // out: s_b per image, or null
  unsigned per, total;       // values per image, of the batch
};

__device__ __forceinline__ float guided_x0(const GuidedStep& s, const StepCoef& cf, float x, float oc, float ou) {
  return step_x0(cf, false, x, guided_out(s.out_u != nullptr, s.scale, oc, ou));
}

// x0 of the guided output into the scratch (mode 2: the select needs the whole image's x0 before any of it is thresholded)
template <int V>
__global__ __launch_bounds__(256) void k_guided_x0(GuidedStep s) {
  const int j = s.f.step_cur[0];
  const StepCoef cf = load_step_coef<false>(s.f.tb, nullptr, j);
  const unsigned e = (blockIdx.x * 256u + threadIdx.x) * V;
  if (e >= s.total) return;
  float xv[V], cv[V], uv[V] = {}, ov[V];
  load_v<V>(s.f.x + e, xv);
  load_v<V>(s.out_c + e, cv);
  if (s.out_u) load_v<V>(s.out_u + e, uv);
#pragma unroll
  for (int k = 0; k < V; ++k) ov[k] = guided_x0(s, cf, xv[k], cv[k], uv[k]);
  store_v<V>(s.x0 + e, ov);
}

// the rule for x0 and the posterior mix; the last kernel of the step: the only one that writes the counter's slot 1 (tail_begin)
template <bool HIST, int V>
__global__ __launch_bounds__(256) void k_guided_mix(GuidedStep s) {
  const StepFuse& f = s.f;
  const StepCoef cf = tail_begin<HIST>(f, blockIdx.x == 0 && threadIdx.x == 0);
  const unsigned e = (blockIdx.x * 256u + threadIdx.x) * V;
  if (e >= s.total) return;
  const unsigned b = e / s.per;                                         // (V = 4: per % 4 == 0, a quad lies in one image)
  const float sb = s.mode == 2 ? fmaxf(1.f, s.q[b]) : 1.f;
  if (s.thr && e == b * s.per) s.thr[b] = sb;
  float xv[V], x0[V], zv[V], hv[V];
  load_v<V>(f.x + e, xv);
  if (s.mode == 2) {
    load_v<V>(s.x0 + e, x0);
#pragma unroll
    for (int k = 0; k < V; ++k) x0[k] = __fdiv_rn(fminf(fmaxf(x0[k], -sb), sb), sb);
  } else {
    float cv[V], uv[V] = {};
    load_v<V>(s.out_c + e, cv);
    if (s.out_u) load_v<V>(s.out_u + e, uv);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      x0[k] = guided_x0(s, cf, xv[k], cv[k], uv[k]);
      if (s.mode == 1) x0[k] = fminf(fmaxf(x0[k], -1.f), 1.f);
    }
  }
  tail_load_zh<HIST, V>(f, e, zv, hv);
  tail_mix_store<HIST, V>(f, cf, e, x0, xv, zv, hv);
}

}  // namespace
}  // namespace sr3

using namespace sr3;

extern "C" {

int sr3_cond_drop_f32(const float* src, const int* keep_dev, int batch, int elems_per_image, float* dst, void* stream) {
  if (!src) { set_error("cond_drop: src is NULL"); return SR3_E_BADARG; }
  if (!keep_dev) { set_error("cond_drop: keep_dev is NULL"); return SR3_E_BADARG; }
  if (!dst) { set_error("cond_drop: dst is NULL"); return SR3_E_BADARG; }
  if (batch <= 0 || elems_per_image <= 0) { set_error("cond_drop: batch and elems_per_image must be positive (got %d, %d)", batch, elems_per_image); return SR3_E_BADARG; }
  const size_t total = (size_t)batch * (size_t)elems_per_image;
  if (total >= ((size_t)1 << 31)) { set_error("cond_drop: image batch too large (batch * elems_per_image >= 2^31)"); return SR3_E_UNSUPPORTED; }
  if (dst != src && overlaps(src, total * sizeof(float), dst, total * sizeof(float))) { set_error("cond_drop: dst overlaps src partially (dst == src is the in-place form)"); return SR3_E_BADARG; }
  if (overlaps(keep_dev, (size_t)batch * sizeof(int), dst, total * sizeof(float))) { set_error("cond_drop: dst overlaps keep_dev"); return SR3_E_BADARG; }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool vec = (elems_per_image & 3) == 0 && vec16(src, dst);
  const unsigned items = (unsigned)(vec ? total / 4 : total);
  const dim3 grid((items + 255) / 256);
  const unsigned* s = reinterpret_cast<const unsigned*>(src);
  unsigned* d = reinterpret_cast<unsigned*>(dst);
  dispatch_bools([&](auto v4) {
    hipLaunchKernelGGL((k_cond_drop<v4() ? 4 : 1>), grid, dim3(256), 0, st, s, keep_dev, (unsigned)elems_per_image, d, (unsigned)total);
  }, vec);
  SR3_LAUNCH_CHECK("k_cond_drop");
  return SR3_OK;
}

size_t sr3_abs_quantile_scratch_bytes(int batch, int n) {
  if (batch <= 0 || n <= 0 || (size_t)batch * (size_t)n >= ((size_t)1 << 31)) return 0;
  return q_scratch_words(batch) * sizeof(unsigned);
}

int sr3_abs_quantile_f32(const float* src, int batch, int n, int rank_lo, double frac, float* out_dev, void* scratch, size_t scratch_bytes,
                         void* stream) {
  if (!src) { set_error("abs_quantile: src is NULL"); return SR3_E_BADARG; }
  if (!out_dev) { set_error("abs_quantile: out_dev is NULL"); return SR3_E_BADARG; }
  if (const int rc = check_quantile("abs_quantile", batch, n, rank_lo, frac, scratch, scratch_bytes)) return rc;
  const size_t sbytes = q_scratch_words(batch) * sizeof(unsigned);
  if (overlaps(src, (size_t)batch * n * sizeof(float), out_dev, (size_t)batch * sizeof(float))) { set_error("abs_quantile: out_dev overlaps src"); return SR3_E_BADARG; }
  if (overlaps(scratch, sbytes, src, (size_t)batch * n * sizeof(float)) || overlaps(scratch, sbytes, out_dev, (size_t)batch * sizeof(float))) {
    set_error("abs_quantile: scratch overlaps src or out_dev");
    return SR3_E_BADARG;
  }
  return abs_quantile(src, batch, n, rank_lo, frac, out_dev, scratch, static_cast<hipStream_t>(stream));
}

int sr3_guided_step(float* x_nchw, const float* out_c, const float* out_u, float scale, const float* z_nchw, int batch, int channels,
                    int height, int width, const float* tab_a, const float* tab_b, const float* tab_c1, const float* tab_c2,
                    const float* tab_sigma, const float* tab_c3, float* hist_nchw, int* step2_dev, int mode, int rank_lo, double frac,
                    float* x0_scratch, void* q_scratch, size_t q_scratch_bytes, float* thr_out_dev, void* stream) {
  const char* who = "guided_step";
  const Req req[] = {{x_nchw, "x_nchw"}, {out_c, "out_c"}, {tab_a, "tab_a"}, {tab_b, "tab_b"}, {tab_c1, "tab_c1"}, {tab_c2, "tab_c2"},
      {tab_sigma, "tab_sigma"}, {step2_dev, "step2_dev"}};
  if (const int rc = check_required(who, req)) return rc;
  if (const int rc = check_image_dims(who, batch, channels, height, width)) return rc;
  const size_t per = (size_t)channels * height * width, total = (size_t)batch * per;
  if (const int rc = check_image_limit(who, total)) return rc;
  if (mode < 0 || mode > 2) { set_error("%s: mode must be 0 (none), 1 (static) or 2 (dynamic) (got %d)", who, mode); return SR3_E_BADARG; }
  if (!(scale - scale == 0.f)) { set_error("%s: scale must be finite (got %g)", who, (double)scale); return SR3_E_BADARG; }
  const size_t bytes = total * sizeof(float);
  if (mode == 2) {
    if (!x0_scratch) { set_error("%s: x0_scratch is NULL (mode 2 needs it)", who); return SR3_E_BADARG; }
    if (const int rc = check_quantile(who, batch, (int)per, rank_lo, frac, q_scratch, q_scratch_bytes)) return rc;
  }
  if (const int rc = check_step_history(who, tab_c3, hist_nchw, x_nchw, out_c, bytes)) return rc;
  // what the step writes (x, the history, the two scratch buffers, the thresholds) shares no byte with anything else it touches
  const size_t qbytes = q_scratch_words(batch) * sizeof(unsigned);
  const Buf buf[] = {
      {x_nchw, bytes, "x_nchw", true}, {hist_nchw, bytes, "hist_nchw", true}, {mode == 2 ? x0_scratch : nullptr, bytes, "x0_scratch", true},
      {mode == 2 ? q_scratch : nullptr, qbytes, "q_scratch", true}, {thr_out_dev, (size_t)batch * sizeof(float), "thr_out_dev", true},
      {out_c, bytes, "out_c", false}, {out_u, bytes, "out_u", false}, {z_nchw, bytes, "z_nchw", false},
      {step2_dev, 2 * sizeof(int), "step2_dev", true}};
  if (const int rc = check_overlaps(who, buf, 0)) return rc;      // (named_last: the other argument is named where one of the two is x itself)
  const bool vec = (width & 3) == 0 && vec16(x_nchw, out_c, out_u, z_nchw, hist_nchw, mode == 2 ? x0_scratch : nullptr);
  GuidedStep s;
  s.f = StepFuse{x_nchw, z_nchw, StepTables{tab_a, tab_b, tab_c1, tab_c2, tab_sigma}, step2_dev, step2_dev + 1, mode == 1, tab_c3, hist_nchw};
  s.out_c = out_c; s.out_u = out_u; s.scale = scale; s.mode = mode;
  s.x0 = mode == 2 ? x0_scratch : nullptr;
  s.q = mode == 2 ? static_cast<const float*>(q_scratch) : nullptr;      // (the scratch's result slots: [batch] floats at its start)
  s.thr = thr_out_dev; s.per = (unsigned)per; s.total = (unsigned)total;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (const int rc = step_copy(step2_dev, st)) return rc;
  const unsigned items = (unsigned)(vec ? total / 4 : total);
  const dim3 grid((items + 255) / 256);
  if (mode == 2) {
    dispatch_bools([&](auto v4) { hipLaunchKernelGGL((k_guided_x0<v4() ? 4 : 1>), grid, dim3(256), 0, st, s); }, vec);
    SR3_LAUNCH_CHECK("k_guided_x0");
    if (const int rc = abs_quantile(x0_scratch, batch, (int)per, rank_lo, frac, static_cast<float*>(q_scratch), q_scratch, st)) return rc;
  }
  dispatch_bools([&](auto hist, auto v4) { hipLaunchKernelGGL((k_guided_mix<hist(), v4() ? 4 : 1>), grid, dim3(256), 0, st, s); },
                 hist_nchw != nullptr, vec);
  SR3_LAUNCH_CHECK("k_guided_mix");
  return SR3_OK;
}

}  // extern "C"
