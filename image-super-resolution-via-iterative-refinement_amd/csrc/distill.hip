// Progressive distillation (include/sr3_mi355x.h: sr3_teacher_step_f32, sr3_distill_target_f32; Salimans & Ho 2022): the two elementwise
// passes between the frozen teacher's forwards and the student's training step.  A student step k goes from node 2k of the teacher's
// walk to node 2k - 2; the teacher covers it in two deterministic DDIM steps through node 2k - 1.
//
//   the teacher's step (n = values per image, every coefficient one fp32 per image):
//     out    = out_c                                                one forward (out_u NULL)
//     out    = add_rn(out_u, mul_rn(scale, sub_rn(out_c, out_u)))   two forwards: guided_out of step_tail.h, sr3_guided_step's
//     x0     = sub_rn(mul_rn(a[b], x), mul_rn(b[b], out)) ; clamp(-1, 1) if clip_denoised        (step_x0 of sr3_common.h)
//     x0_out <- x0 ;  x_next <- add_rn(mul_rn(c1[b], x0), mul_rn(c2[b], x))
//
//   the second teacher step fused with the regression target (z_e, the point the teacher lands on, is never formed: eliminating it
//   leaves a convex combination of the two x0 predictions, no difference of nearly equal numbers and no large reciprocal):
//     x0b     = clamp?(a[b] x_mid - b[b] out)
//     x_tgt   <- add_rn(mul_rn(w1[b], x0_first), mul_rn(w2[b], x0b))
//     eps_tgt <- sub_rn(mul_rn(s1[b], z_t), mul_rn(s2[b], x_tgt))
//
// Both are HBM-bound: one launch each, a thread owns four consecutive values of one image as one 16-byte access or one value (n % 4 == 0
// and step_tail.h's vec16 / load_v / store_v); the same operations on the same operands either way, so the same bits.  No division,
// no atomics, no fused multiply-add: the host computed every coefficient in float64 and rounded it once.  The argument checks are
// step_tail.h's (check_required, one Buf table under check_overlaps; x_next == x is its in-place pair).
#include "step_tail.h"

namespace sr3 {
namespace {

struct DistillArgs {
  const float* x;            // teacher step: the start point; target: x_mid, the point between the teacher's two steps
  const float* out_c;        // the teacher's output on the real condition
  const float* out_u;        // ... on the zero condition, or null: no guidance
  float scale;
  const float* a;            // x0 = a x - b out, per image
  const float* b;
  const float* p1;           // teacher step: c1, c2 ;  target: w1, w2
  const float* p2;
  const float* z_t;          // target only: the start point of the student's step, the teacher's first x0, s1, s2
  const float* x0_first;
  const float* s1;
  const float* s2;
  float* o1;                 // teacher step: x_next (may be x itself), x0_out ;  target: x_tgt, eps_tgt
  float* o2;
  bool clip;
  unsigned per, total;       // values per image, of the batch
};

__device__ __forceinline__ float teacher_x0(const DistillArgs& s, float a, float b, float x, float oc, float ou) {
  const float out = guided_out(s.out_u != nullptr, s.scale, oc, ou);
  float x0 = sub_rn(mul_rn(a, x), mul_rn(b, out));
  if (s.clip) x0 = fminf(fmaxf(x0, -1.f), 1.f);
  return x0;
}

// (x is read in full before x_next is written, by the one thread that owns the element: x_next == x is safe)
template <int V>
__global__ __launch_bounds__(256) void k_teacher_step(DistillArgs s) {
  const unsigned e = (blockIdx.x * 256u + threadIdx.x) * V;
  if (e >= s.total) return;
  const unsigned img = e / s.per;                                        // (V = 4: per % 4 == 0, a quad lies in one image)
  const float a = s.a[img], b = s.b[img], c1 = s.p1[img], c2 = s.p2[img];
  float xv[V], cv[V], uv[V] = {}, x0[V], nx[V];
  load_v<V>(s.x + e, xv);
  load_v<V>(s.out_c + e, cv);
  if (s.out_u) load_v<V>(s.out_u + e, uv);
#pragma unroll
  for (int k = 0; k < V; ++k) {
    x0[k] = teacher_x0(s, a, b, xv[k], cv[k], uv[k]);
    nx[k] = add_rn(mul_rn(c1, x0[k]), mul_rn(c2, xv[k]));
  }
  store_v<V>(s.o2 + e, x0);
  store_v<V>(s.o1 + e, nx);
}

template <int V>
__global__ __launch_bounds__(256) void k_distill_target(DistillArgs s) {
  const unsigned e = (blockIdx.x * 256u + threadIdx.x) * V;
  if (e >= s.total) return;
  const unsigned img = e / s.per;
  const float a = s.a[img], b = s.b[img], w1 = s.p1[img], w2 = s.p2[img], s1 = s.s1[img], s2 = s.s2[img];
  float xv[V], cv[V], uv[V] = {}, fv[V], zv[V], xt[V], et[V];
  load_v<V>(s.x + e, xv);
  load_v<V>(s.out_c + e, cv);
  if (s.out_u) load_v<V>(s.out_u + e, uv);
  load_v<V>(s.x0_first + e, fv);
  load_v<V>(s.z_t + e, zv);
#pragma unroll
  for (int k = 0; k < V; ++k) {
    const float x0b = teacher_x0(s, a, b, xv[k], cv[k], uv[k]);
    xt[k] = add_rn(mul_rn(w1, fv[k]), mul_rn(w2, x0b));
    et[k] = sub_rn(mul_rn(s1, zv[k]), mul_rn(s2, xt[k]));
  }
  store_v<V>(s.o1 + e, xt);
  store_v<V>(s.o2 + e, et);
}

int check_sizes(const char* who, int batch, int elems_per_image, const float* out_u, float scale) {
  if (batch <= 0 || elems_per_image <= 0) { set_error("%s: batch and elems_per_image must be positive (got %d, %d)", who, batch, elems_per_image); return SR3_E_BADARG; }
  if ((size_t)batch * (size_t)elems_per_image >= ((size_t)1 << 31)) { set_error("%s: image batch too large (batch * elems_per_image >= 2^31)", who); return SR3_E_UNSUPPORTED; }
  if (out_u && !(scale - scale == 0.f)) { set_error("%s: scale must be finite (got %g)", who, (double)scale); return SR3_E_BADARG; }
  return SR3_OK;
}

}  // namespace
}  // namespace sr3

using namespace sr3;

extern "C" {

int sr3_teacher_step_f32(const float* x, const float* out_c, const float* out_u, float scale, const float* a, const float* b, const float* c1,
                         const float* c2, int batch, int elems_per_image, int clip_denoised, float* x_next, float* x0_out, void* stream) {
  const Req req[] = {{x, "x"}, {out_c, "out_c"}, {a, "a"}, {b, "b"}, {c1, "c1"}, {c2, "c2"}, {x_next, "x_next"}, {x0_out, "x0_out"}};
  if (const int rc = check_required("teacher_step", req)) return rc;
  if (const int rc = check_sizes("teacher_step", batch, elems_per_image, out_u, scale)) return rc;
  const size_t total = (size_t)batch * (size_t)elems_per_image, bytes = total * sizeof(float), cbytes = (size_t)batch * sizeof(float);
  const Buf bufs[] = {{x_next, bytes, "x_next", true}, {x0_out, bytes, "x0_out", true}, {x, bytes, "x", false}, {out_c, bytes, "out_c", false},
      {out_u, bytes, "out_u", false}, {a, cbytes, "a", false}, {b, cbytes, "b", false}, {c1, cbytes, "c1", false}, {c2, cbytes, "c2", false}};
  if (const int rc = check_overlaps("teacher_step", bufs, -1, 0, 2)) return rc;
  const bool vec = (elems_per_image & 3) == 0 && vec16(x, out_c, out_u, x_next, x0_out);
  DistillArgs s = {};
  s.x = x; s.out_c = out_c; s.out_u = out_u; s.scale = scale; s.a = a; s.b = b; s.p1 = c1; s.p2 = c2;
  s.o1 = x_next; s.o2 = x0_out; s.clip = clip_denoised != 0; s.per = (unsigned)elems_per_image; s.total = (unsigned)total;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned items = (unsigned)(vec ? total / 4 : total);
  const dim3 grid((items + 255) / 256);
  dispatch_bools([&](auto v4) { hipLaunchKernelGGL((k_teacher_step<v4() ? 4 : 1>), grid, dim3(256), 0, st, s); }, vec);
  SR3_LAUNCH_CHECK("k_teacher_step");
  return SR3_OK;
}

int sr3_distill_target_f32(const float* z_t, const float* x_mid, const float* out_c, const float* out_u, float scale, const float* x0_first,
                           const float* a, const float* b, const float* w1, const float* w2, const float* s1, const float* s2, int batch,
                           int elems_per_image, int clip_denoised, float* x_tgt, float* eps_tgt, void* stream) {
  const Req req[] = {{z_t, "z_t"}, {x_mid, "x_mid"}, {out_c, "out_c"}, {x0_first, "x0_first"}, {a, "a"}, {b, "b"}, {w1, "w1"}, {w2, "w2"},
      {s1, "s1"}, {s2, "s2"}, {x_tgt, "x_tgt"}, {eps_tgt, "eps_tgt"}};
  if (const int rc = check_required("distill_target", req)) return rc;
  if (const int rc = check_sizes("distill_target", batch, elems_per_image, out_u, scale)) return rc;
  const size_t total = (size_t)batch * (size_t)elems_per_image, bytes = total * sizeof(float), cbytes = (size_t)batch * sizeof(float);
  const Buf bufs[] = {{x_tgt, bytes, "x_tgt", true}, {eps_tgt, bytes, "eps_tgt", true}, {z_t, bytes, "z_t", false}, {x_mid, bytes, "x_mid", false},
      {out_c, bytes, "out_c", false}, {out_u, bytes, "out_u", false}, {x0_first, bytes, "x0_first", false}, {a, cbytes, "a", false},
      {b, cbytes, "b", false}, {w1, cbytes, "w1", false}, {w2, cbytes, "w2", false}, {s1, cbytes, "s1", false}, {s2, cbytes, "s2", false}};
  if (const int rc = check_overlaps("distill_target", bufs)) return rc;
  const bool vec = (elems_per_image & 3) == 0 && vec16(z_t, x_mid, out_c, out_u, x0_first, x_tgt, eps_tgt);
  DistillArgs s = {};
  s.x = x_mid; s.out_c = out_c; s.out_u = out_u; s.scale = scale; s.a = a; s.b = b; s.p1 = w1; s.p2 = w2;
  s.z_t = z_t; s.x0_first = x0_first; s.s1 = s1; s.s2 = s2;
  s.o1 = x_tgt; s.o2 = eps_tgt; s.clip = clip_denoised != 0; s.per = (unsigned)elems_per_image; s.total = (unsigned)total;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned items = (unsigned)(vec ? total / 4 : total);
  const dim3 grid((items + 255) / 256);
  dispatch_bools([&](auto v4) { hipLaunchKernelGGL((k_distill_target<v4() ? 4 : 1>), grid, dim3(256), 0, st, s); }, vec);
  SR3_LAUNCH_CHECK("k_distill_target");
  return SR3_OK;
}

}  // extern "C"
