// Back-projection sampling (include/sr3_mi355x.h: sr3_resample_f32, sr3_backproject_step, sr3_backproject_scratch_bytes): iterative
// back-projection (Irani & Peleg 1991; ILVR's low-pass swap, Choi et al. 2021, applied to x0) under the resize the datasets are made
// with -- Pillow's antialiased bicubic / bilinear resample -- inside the tail of a reverse step.
//
// The operator.  A resample of one axis is a banded matrix given by two tables the HOST makes (sr3_hip.diffusion.resample_tables, Pillow's
// precompute_coeffs in float64, rounded once to fp32): bounds [out, 2] = (first tap, count) and weights [out, ksize].  Nothing here
// evaluates a filter or touches a double.  A 2-D resample is the horizontal pass into an fp32 intermediate [planes, H, OW], then the
// vertical pass (Pillow's order).  One output value:
//
//   acc = +0 ; for t = 0 .. count - 1 (ascending):  acc = add_rn(acc, mul_rn(src[first + t], w[t]))
//
// every product and every sum rounded on its own (mul_rn / add_rn of sr3_common.h: no fma), no atomics, one thread per output value:
// the bits do not depend on the launch geometry, the alignment or the run.
//
// Safety.  (first, count) are clamped on the device: first into [0, in], count into [0, min(ksize, in - first)] -- whatever a table
// holds, a kernel reads inside its source row / column and inside the weight table, and writes only its own output element.
//
// The step (K = iterations, lambda = strength, j = step2_dev[1] on entry, y = the LR target, D: (H, W) -> (H / s, W / s), U: back):
//
//   k_step_copy                                   slot 0 <- j
//   k_bp_x0        x0 = step_x0(x, eps)           -> scratch x0                                      (16-byte form: 4 elements a thread)
//   K times:
//     k_resample_h   t  = D_h x0                  -> scratch tmp [B C, H, W / s]                     (one value a thread, lanes along x)
//     k_resample_v   r  = sub_rn(y, D_v t)        -> scratch r [B C, H / s, W / s]                   (RESID; 16-byte form where W / s % 4 == 0)
//     k_bp_up        x0 = add_rn(x0, mul_rn(lambda, U r))       in place; the LAST one instead goes on with
//                    x  = step_mix<HIST>(x0, x, z, hist) ; hist <- x0 ; slot 1 <- j - 1              (16-byte form: 4 elements a thread)
//
// 2 + 3 K launches.  k_bp_up does U in one kernel: a thread computes, for each of the <= ksize_v (5 for an up-sample) rows of r its
// vertical taps cover, the horizontal sum over that row's <= ksize_h taps in the order above, and then their vertical sum in the order
// above -- the values the two-pass definition keeps in its intermediate, the same bits, without the intermediate or its launch.  r is
// 1 / s^2 of the image and stays in the cache.  No LDS: there is no launch left for it to remove.
#include "step_tail.h"

namespace sr3 {
namespace {

// one axis of a resample: tables of `out` rows for a source axis of `in` elements
struct Axis {
  const int* bounds;        // [out, 2]: first tap, count
  const float* weights;     // [out, ksize]
  int ksize, in, out;
};

// row o of the tables, clamped so that [first, first + count) lies inside [0, in) and count inside the weight row
__device__ __forceinline__ void taps_of(const Axis& a, int o, int& first, int& count, const float*& w) {
  int f = a.bounds[2 * o], c = a.bounds[2 * o + 1];
  f = f < 0 ? 0 : (f > a.in ? a.in : f);
  const int room = a.in - f < a.ksize ? a.in - f : a.ksize;
  c = c < 0 ? 0 : (c > room ? room : c);
  first = f; count = c; w = a.weights + (size_t)o * a.ksize;
}

// sum over the taps of src[first + t * stride] * w[t], ascending, every operation rounded on its own, from +0
__device__ __forceinline__ float tap_sum(const float* __restrict__ src, size_t stride, int count, const float* __restrict__ w) {
  float acc = 0.f;
  for (int t = 0; t < count; ++t, src += stride) acc = add_rn(acc, mul_rn(src[0], w[t]));
  return acc;
}

// horizontal pass: dst[p, y, ox] = sum_t src[p, y, first(ox) + t] w[ox, t]; `rows` = planes * H; consecutive lanes take consecutive ox
// of one row, so together they read one contiguous segment of it
__global__ __launch_bounds__(256) void k_resample_h(const float* __restrict__ src, float* __restrict__ dst, Axis ax, unsigned total) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const unsigned row = i / (unsigned)ax.out, ox = i % (unsigned)ax.out;
  int first, count;
  const float* w;
  taps_of(ax, (int)ox, first, count, w);
  dst[i] = tap_sum(src + (size_t)row * ax.in + first, 1, count, w);
}

// vertical pass: dst[p, oy, x] = sum_t src[p, first(oy) + t, x] w[oy, t] over rows of width W; RESID: dst = sub_rn(y, that).  A thread
// owns V consecutive x (V = 4: one 16-byte access per tap row), lanes along x.
template <bool RESID, int V>
__global__ __launch_bounds__(256) void k_resample_v(const float* __restrict__ src, float* __restrict__ dst, const float* __restrict__ y,
                                                     Axis ax, int W, unsigned total) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const unsigned wv = (unsigned)W / V;
  const unsigned xq = i % wv, rest = i / wv;
  const unsigned oy = rest % (unsigned)ax.out, p = rest / (unsigned)ax.out;
  int first, count;
  const float* w;
  taps_of(ax, (int)oy, first, count, w);
  const float* s = src + ((size_t)p * ax.in + first) * W + (size_t)xq * V;
  const size_t o = ((size_t)p * ax.out + oy) * W + (size_t)xq * V;
  if constexpr (V == 4) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < count; ++t, s += W) {
      const f32x4 q = *reinterpret_cast<const f32x4*>(s);
      const float wt = w[t];
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[k] = add_rn(acc[k], mul_rn(q[k], wt));
    }
    if (RESID) {
      const f32x4 yq = *reinterpret_cast<const f32x4*>(y + o);
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[k] = sub_rn(yq[k], acc[k]);
    }
    *reinterpret_cast<f32x4*>(dst + o) = acc;
  } else {
    float acc = tap_sum(s, (size_t)W, count, w);
    if (RESID) acc = sub_rn(y[o], acc);
    dst[o] = acc;
  }
}

// x0 = step_x0(x, eps) at row j = step_cur[0] of the tables -> x0 (scratch)
template <bool CLIP, int V>
__global__ __launch_bounds__(256) void k_bp_x0(const float* __restrict__ x, const float* __restrict__ eps, float* __restrict__ x0,
                                                StepTables tb, const int* __restrict__ step_cur, unsigned total) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const StepCoef cf = load_step_coef<false>(tb, nullptr, step_cur[0]);
  const size_t e = (size_t)i * V;
  float xv[V], ev[V], o[V];
  load_v<V>(x + e, xv);
  load_v<V>(eps + e, ev);
#pragma unroll
  for (int k = 0; k < V; ++k) o[k] = step_x0(cf, CLIP, xv[k], ev[k]);
  store_v<V>(x0 + e, o);
}

struct BpUp {
  StepFuse f;               // LAST only: the step's mix on x [B, C, H, W] (z, tables, counter slots, c3, hist)
  float* x0;                // [B, C, H, W] scratch, in / out
  const float* r;           // [B, C, H / s, W / s] the LR residual
  Axis uh, uv;              // the up-sample's horizontal (W / s -> W) and vertical (H / s -> H) tables
  float strength;
  unsigned total;           // items = B * C * H * W / V
};

// (U r)[p, oy, ox]: for each vertical tap row of r the horizontal sum, then their vertical sum -- the two-pass definition's bits
__device__ __forceinline__ float up_value(const BpUp& s, const float* __restrict__ rp, int vfirst, int vcount, const float* __restrict__ wv,
                                          int ox) {
  int hfirst, hcount;
  const float* wh;
  taps_of(s.uh, ox, hfirst, hcount, wh);
  float acc = 0.f;
  const float* row = rp + (size_t)vfirst * s.uh.in + hfirst;
  for (int t = 0; t < vcount; ++t, row += s.uh.in) acc = add_rn(acc, mul_rn(tap_sum(row, 1, hcount, wh), wv[t]));
  return acc;
}

template <bool LAST, bool HIST, int V>
__global__ __launch_bounds__(256) void k_bp_up(BpUp s) {
  const StepFuse& f = s.f;
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  StepCoef cf = {};
  if (LAST) cf = tail_begin<HIST>(f, i == 0);
  if (i >= s.total) return;
  const unsigned W = (unsigned)s.uh.out, H = (unsigned)s.uv.out;
  const unsigned wq = W / V;
  const unsigned xq = i % wq, rest = i / wq;
  const unsigned oy = rest % H, p = rest / H;
  int vfirst, vcount;
  const float* wv;
  taps_of(s.uv, (int)oy, vfirst, vcount, wv);
  const float* rp = s.r + (size_t)p * s.uv.in * s.uh.in;
  const size_t e = (size_t)i * V;
  float x0v[V], xv[V], zv[V], hv[V];
  load_v<V>(s.x0 + e, x0v);
  if (LAST) tail_load<HIST, V>(f, e, xv, zv, hv);
#pragma unroll
  for (int k = 0; k < V; ++k) x0v[k] = add_rn(x0v[k], mul_rn(s.strength, up_value(s, rp, vfirst, vcount, wv, (int)(xq * V + k))));
  if (LAST) tail_mix_store<HIST, V>(f, cf, e, x0v, xv, zv, hv);
  else store_v<V>(s.x0 + e, x0v);
}

inline dim3 grid_of(size_t items) { return dim3((unsigned)((items + 255) / 256)); }
inline size_t round4(size_t floats) { return (floats + 3) & ~(size_t)3; }

const size_t LIMIT = (size_t)1 << 31;      // (sr3_resample_f32's three limits; the step's is check_image_limit)

// the two passes of one resample, planes [planes, H, W] -> [planes, OH, OW] through tmp [planes, H, OW]; y: RESID target or null
int launch_resample(const float* src, float* dst, float* tmp, const float* y, int planes, int H, int W, int OH, int OW, const Axis& h,
                    const Axis& v, hipStream_t st) {
  const size_t n_tmp = (size_t)planes * H * OW;
  hipLaunchKernelGGL(k_resample_h, grid_of(n_tmp), dim3(256), 0, st, src, tmp, h, (unsigned)n_tmp);
  SR3_LAUNCH_CHECK("k_resample_h");
  const size_t n_dst = (size_t)planes * OH * OW;
  const bool vec = (OW & 3) == 0 && vec16(tmp, dst, y);
  const size_t items = vec ? n_dst / 4 : n_dst;
  dispatch_bools([&](auto resid, auto v4) {
    hipLaunchKernelGGL((k_resample_v<resid(), v4() ? 4 : 1>), grid_of(items), dim3(256), 0, st, tmp, dst, y, v, OW, (unsigned)items);
  }, y != nullptr, vec);
  SR3_LAUNCH_CHECK("k_resample_v");
  return SR3_OK;
}

// a host copy of a bounds table: every row inside [0, in] with 1 <= count <= ksize
int check_host_bounds(const char* who, const char* name, const int* b, int out, int in, int ksize) {
  for (int o = 0; o < out; ++o) {
    const long f = b[2 * o], c = b[2 * o + 1];
    if (f < 0 || c < 1 || c > ksize || f + c > in) {
      set_error("%s: %s row %d (first %ld, count %ld) is not inside [0, %d] with 1 <= count <= ksize %d", who, name, o, f, c, in, ksize);
      return SR3_E_BADARG;
    }
  }
  return SR3_OK;
}

// the sizes of the step, before anything is launched; *total = B * C * H * W
int check_bp_sizes(const char* who, int batch, int channels, int height, int width, int scale, size_t* total) {
  if (const int rc = check_image_dims(who, batch, channels, height, width)) return rc;
  if (scale < 2) { set_error("%s: scale must be at least 2 (got %d)", who, scale); return SR3_E_BADARG; }
  if (height % scale || width % scale) { set_error("%s: scale %d does not divide height %d and width %d", who, scale, height, width); return SR3_E_BADARG; }
  *total = (size_t)batch * channels * height * width;
  return check_image_limit(who, *total);
}

struct BpLayout { size_t x0, tmp, r, floats; };      // offsets in floats, each a multiple of 4 (16 bytes)
BpLayout bp_layout(size_t total, int scale) {
  BpLayout l;
  l.x0 = 0;
  l.tmp = round4(total);
  l.r = l.tmp + round4(total / scale);
  l.floats = l.r + round4(total / scale / scale);
  return l;
}

}  // namespace
}  // namespace sr3

using namespace sr3;

extern "C" {

int sr3_resample_f32(const float* src, int planes, int height, int width, float* dst, int out_height, int out_width,
                     const int* bounds_h_dev, const float* weights_h_dev, int ksize_h, const int* bounds_v_dev,
                     const float* weights_v_dev, int ksize_v, float* tmp, const int* bounds_h_host, const int* bounds_v_host,
                     void* stream) {
  const Req req[] = {{src, "src"}, {dst, "dst"}, {bounds_h_dev, "bounds_h_dev"}, {weights_h_dev, "weights_h_dev"}, {bounds_v_dev, "bounds_v_dev"},
      {weights_v_dev, "weights_v_dev"}, {tmp, "tmp"}};
  if (const int rc = check_required("resample", req)) return rc;
  if (planes <= 0 || height <= 0 || width <= 0 || out_height <= 0 || out_width <= 0) {
    set_error("resample: planes, height, width, out_height and out_width must be positive (got %d, %d, %d, %d, %d)", planes, height, width,
              out_height, out_width);
    return SR3_E_BADARG;
  }
  if (ksize_h < 1) { set_error("resample: ksize_h must be at least 1 (got %d)", ksize_h); return SR3_E_BADARG; }
  if (ksize_v < 1) { set_error("resample: ksize_v must be at least 1 (got %d)", ksize_v); return SR3_E_BADARG; }
  const size_t n_src = (size_t)planes * height * width, n_tmp = (size_t)planes * height * out_width,
               n_dst = (size_t)planes * out_height * out_width;
  if (n_src >= LIMIT) { set_error("resample: src too large (planes * height * width >= 2^31)"); return SR3_E_UNSUPPORTED; }
  if (n_tmp >= LIMIT) { set_error("resample: tmp too large (planes * height * out_width >= 2^31)"); return SR3_E_UNSUPPORTED; }
  if (n_dst >= LIMIT) { set_error("resample: dst too large (planes * out_height * out_width >= 2^31)"); return SR3_E_UNSUPPORTED; }
  if (overlaps(dst, n_dst * sizeof(float), src, n_src * sizeof(float))) { set_error("resample: dst overlaps src"); return SR3_E_BADARG; }
  if (overlaps(tmp, n_tmp * sizeof(float), src, n_src * sizeof(float))) { set_error("resample: tmp overlaps src"); return SR3_E_BADARG; }
  if (overlaps(tmp, n_tmp * sizeof(float), dst, n_dst * sizeof(float))) { set_error("resample: tmp overlaps dst"); return SR3_E_BADARG; }
  const struct { const void* p; size_t bytes; const char* name; } tabs[] = {
      {bounds_h_dev, (size_t)out_width * 2 * sizeof(int), "bounds_h_dev"}, {weights_h_dev, (size_t)out_width * ksize_h * sizeof(float), "weights_h_dev"},
      {bounds_v_dev, (size_t)out_height * 2 * sizeof(int), "bounds_v_dev"}, {weights_v_dev, (size_t)out_height * ksize_v * sizeof(float), "weights_v_dev"}};
  for (const auto& t : tabs) {
    if (overlaps(t.p, t.bytes, dst, n_dst * sizeof(float))) { set_error("resample: dst overlaps %s", t.name); return SR3_E_BADARG; }
    if (overlaps(t.p, t.bytes, tmp, n_tmp * sizeof(float))) { set_error("resample: tmp overlaps %s", t.name); return SR3_E_BADARG; }
  }
  if (bounds_h_host) {
    if (const int rc = check_host_bounds("resample", "bounds_h_host", bounds_h_host, out_width, width, ksize_h)) return rc;
  }
  if (bounds_v_host) {
    if (const int rc = check_host_bounds("resample", "bounds_v_host", bounds_v_host, out_height, height, ksize_v)) return rc;
  }
  const Axis h{bounds_h_dev, weights_h_dev, ksize_h, width, out_width};
  const Axis v{bounds_v_dev, weights_v_dev, ksize_v, height, out_height};
  return launch_resample(src, dst, tmp, nullptr, planes, height, width, out_height, out_width, h, v, static_cast<hipStream_t>(stream));
}

size_t sr3_backproject_scratch_bytes(int batch, int channels, int height, int width, int scale) {
  size_t total = 0;
  if (check_bp_sizes("backproject_scratch_bytes", batch, channels, height, width, scale, &total)) return 0;
  return bp_layout(total, scale).floats * sizeof(float);
}

int sr3_backproject_step(float* x_nchw, const float* eps_nchw, const float* z_nchw, const float* y_lr, int batch, int channels, int height,
                         int width, int scale, int iterations, float strength, const int* down_bounds_h, const float* down_weights_h,
                         int down_ksize_h, const int* down_bounds_v, const float* down_weights_v, int down_ksize_v,
                         const int* up_bounds_h, const float* up_weights_h, int up_ksize_h, const int* up_bounds_v,
                         const float* up_weights_v, int up_ksize_v, const float* tab_a, const float* tab_b, const float* tab_c1,
                         const float* tab_c2, const float* tab_sigma, int* step2_dev, int clip_denoised, const float* tab_c3,
                         float* hist_nchw, void* scratch, size_t scratch_bytes, void* stream) {
  const char* who = "backproject_step";
  const Req req[] = {{x_nchw, "x_nchw"}, {eps_nchw, "eps_nchw"}, {y_lr, "y_lr"},
      {down_bounds_h, "down_bounds_h"}, {down_weights_h, "down_weights_h"}, {down_bounds_v, "down_bounds_v"}, {down_weights_v, "down_weights_v"},
      {up_bounds_h, "up_bounds_h"}, {up_weights_h, "up_weights_h"}, {up_bounds_v, "up_bounds_v"}, {up_weights_v, "up_weights_v"},
      {tab_a, "tab_a"}, {tab_b, "tab_b"}, {tab_c1, "tab_c1"}, {tab_c2, "tab_c2"}, {tab_sigma, "tab_sigma"}, {step2_dev, "step2_dev"}};
  if (const int rc = check_required(who, req)) return rc;
  size_t total = 0;
  if (const int rc = check_bp_sizes(who, batch, channels, height, width, scale, &total)) return rc;
  if (iterations < 1 || iterations > 16) { set_error("%s: iterations must lie in 1..16 (got %d)", who, iterations); return SR3_E_BADARG; }
  if (!(strength > 0.f && strength < 2.f)) { set_error("%s: strength must lie in (0, 2) (got %g)", who, (double)strength); return SR3_E_BADARG; }
  const struct { int k; const char* name; } ks[] = {{down_ksize_h, "down_ksize_h"}, {down_ksize_v, "down_ksize_v"}, {up_ksize_h, "up_ksize_h"},
                                                    {up_ksize_v, "up_ksize_v"}};
  for (const auto& q : ks) {
    if (q.k < 1) { set_error("%s: %s must be at least 1 (got %d)", who, q.name, q.k); return SR3_E_BADARG; }
  }
  const size_t bytes = total * sizeof(float);
  if (const int rc = check_step_history(who, tab_c3, hist_nchw, x_nchw, eps_nchw, bytes)) return rc;
  if (!scratch) { set_error("%s: scratch is NULL", who); return SR3_E_BADARG; }
  const BpLayout lay = bp_layout(total, scale);
  if (scratch_bytes < lay.floats * sizeof(float)) {
    set_error("%s: scratch_bytes %zu is too small (sr3_backproject_scratch_bytes: %zu)", who, scratch_bytes, lay.floats * sizeof(float));
    return SR3_E_BADARG;
  }
  if ((uintptr_t)scratch & 3) { set_error("misaligned pointer (scratch: 4 B)"); return SR3_E_ALIGN; }
  const int OH = height / scale, OW = width / scale;
  const size_t n_lr = total / scale / scale;
  // what the call writes (x, hist, scratch, the counter) against everything else it is given
  const size_t fl = sizeof(float);
  const Buf bufs[] = {{x_nchw, bytes, "x_nchw", true}, {eps_nchw, bytes, "eps_nchw", false}, {z_nchw, bytes, "z_nchw", false},
      {y_lr, n_lr * fl, "y_lr", false}, {hist_nchw, bytes, "hist_nchw", true}, {scratch, lay.floats * fl, "scratch", true},
      {step2_dev, 2 * sizeof(int), "step2_dev", true},
      {down_bounds_h, (size_t)OW * 2 * sizeof(int), "down_bounds_h", false}, {down_weights_h, (size_t)OW * down_ksize_h * fl, "down_weights_h", false},
      {down_bounds_v, (size_t)OH * 2 * sizeof(int), "down_bounds_v", false}, {down_weights_v, (size_t)OH * down_ksize_v * fl, "down_weights_v", false},
      {up_bounds_h, (size_t)width * 2 * sizeof(int), "up_bounds_h", false}, {up_weights_h, (size_t)width * up_ksize_h * fl, "up_weights_h", false},
      {up_bounds_v, (size_t)height * 2 * sizeof(int), "up_bounds_v", false}, {up_weights_v, (size_t)height * up_ksize_v * fl, "up_weights_v", false},
      {tab_a, fl, "tab_a", false}, {tab_b, fl, "tab_b", false}, {tab_c1, fl, "tab_c1", false}, {tab_c2, fl, "tab_c2", false},
      {tab_sigma, fl, "tab_sigma", false}, {tab_c3, fl, "tab_c3", false}};
  if (const int rc = check_overlaps(who, bufs)) return rc;
  float* sc = static_cast<float*>(scratch);
  float* x0 = sc + lay.x0;
  float* tmp = sc + lay.tmp;
  float* r = sc + lay.r;
  const int planes = batch * channels;
  const Axis dh{down_bounds_h, down_weights_h, down_ksize_h, width, OW};
  const Axis dv{down_bounds_v, down_weights_v, down_ksize_v, height, OH};
  const bool vec = (width & 3) == 0 && vec16(scratch, x_nchw, eps_nchw, z_nchw, hist_nchw);
  const size_t items = vec ? total / 4 : total;
  const StepTables tb{tab_a, tab_b, tab_c1, tab_c2, tab_sigma};
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (const int rc = step_copy(step2_dev, st)) return rc;
  dispatch_bools([&](auto clip, auto v4) {
    hipLaunchKernelGGL((k_bp_x0<clip(), v4() ? 4 : 1>), grid_of(items), dim3(256), 0, st, x_nchw, eps_nchw, x0, tb, step2_dev, (unsigned)items);
  }, clip_denoised != 0, vec);
  SR3_LAUNCH_CHECK("k_bp_x0");
  BpUp s;
  s.f = StepFuse{x_nchw, z_nchw, tb, step2_dev, step2_dev + 1, clip_denoised, tab_c3, hist_nchw};
  s.x0 = x0; s.r = r;
  s.uh = Axis{up_bounds_h, up_weights_h, up_ksize_h, OW, width};
  s.uv = Axis{up_bounds_v, up_weights_v, up_ksize_v, OH, height};
  s.strength = strength; s.total = (unsigned)items;
  for (int it = 0; it < iterations; ++it) {
    if (const int rc = launch_resample(x0, r, tmp, y_lr, planes, height, width, OH, OW, dh, dv, st)) return rc;
    if (it + 1 < iterations) {
      dispatch_bools([&](auto v4) { hipLaunchKernelGGL((k_bp_up<false, false, v4() ? 4 : 1>), grid_of(items), dim3(256), 0, st, s); }, vec);
    } else {
      dispatch_bools([&](auto hist, auto v4) { hipLaunchKernelGGL((k_bp_up<true, hist(), v4() ? 4 : 1>), grid_of(items), dim3(256), 0, st, s); },
                     hist_nchw != nullptr, vec);
    }
    SR3_LAUNCH_CHECK("k_bp_up");
  }
  return SR3_OK;
}

}  // extern "C"
