// The frame around the tail of a reverse step, stated once for the kernels that own a whole tail (k_tiled_step, k_consistent_step,
// k_guided_mix, k_bp_up<LAST>), the two distillation passes and k_p_sample_update.  The arithmetic is sr3_common.h's (step_x0,
// step_mix, load_step_coef, check_step_history); this is what stands around it:
//
//   device   load_v / store_v       V = 4: one 16-byte access of four consecutive floats; V = 1: one float.  The host chose V (vec16)
//            tail_begin             the prologue: j = step_cur[0], one thread writes step_next[0] = j - 1, row j of the tables
//            tail_load              x / z / hist of the V elements at e (z null: zeros; no history: not read); tail_load_zh: z / hist alone
//            tail_mix_store         step_mix on them with the caller's x0, then x and hist <- x0 stored
//            guided_out             the classifier-free combination out_u + scale (out_c - out_u)
//   host     check_required, check_image_dims, check_image_limit, check_overlaps (one Buf table per entry), vec16, dispatch_bools
//
// A new rule on x0 is one kernel -- tail_begin, tail_load, its own x0, tail_mix_store -- and one entry that runs these checks in its
// own order (the order is part of the ABI: tests/golden/step_refusals.json pins code and text of every refusal).
#pragma once
#include <type_traits>

#include "sr3_common.h"

namespace sr3 {

// ---- device ----
template <int V>
__device__ __forceinline__ void load_v(const float* p, float (&v)[V]) {
  if constexpr (V == 4) {
    const f32x4 q = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = q[k];
  } else {
    v[0] = p[0];
  }
}
template <int V>
__device__ __forceinline__ void store_v(float* p, const float (&v)[V]) {
  if constexpr (V == 4) {
    const f32x4 q = {v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(p) = q;
  } else {
    p[0] = v[0];
  }
}

// `first`: true in exactly one thread of the launch.  Nobody reads step_next's slot before the next step's first kernel, and
// step_cur's was written by an earlier launch (step_copy), so no thread of this kernel races with another.
template <bool HIST>
__device__ __forceinline__ StepCoef tail_begin(const StepFuse& f, bool first) {
  const int j = f.step_cur[0];
  if (first) f.step_next[0] = j - 1;
  return load_step_coef<HIST>(f.tb, f.c3, j);
}

// The thread owns elements e .. e + V - 1: it reads their history before and stores it after (tail_mix_store).  tail_load_zh: z (null:
// zeros) and the history (HIST false: not read, zeros); tail_load: x and those.  A kernel whose x0 takes many registers to make
// (k_guided_mix) reads x first and z / hist after x0 is made; the others read all three at once.
template <bool HIST, int V>
__device__ __forceinline__ void tail_load_zh(const StepFuse& f, size_t e, float (&zv)[V], float (&hv)[V]) {
#pragma unroll
  for (int k = 0; k < V; ++k) zv[k] = hv[k] = 0.f;
  if (f.z) load_v<V>(f.z + e, zv);
  if (HIST) load_v<V>(f.hist + e, hv);
}
template <bool HIST, int V>
__device__ __forceinline__ void tail_load(const StepFuse& f, size_t e, float (&xv)[V], float (&zv)[V], float (&hv)[V]) {
  load_v<V>(f.x + e, xv);
  tail_load_zh<HIST, V>(f, e, zv, hv);
}
template <bool HIST, int V>
__device__ __forceinline__ void tail_mix_store(const StepFuse& f, const StepCoef& cf, size_t e, const float (&x0)[V], float (&xv)[V],
                                               const float (&zv)[V], float (&hv)[V]) {
#pragma unroll
  for (int k = 0; k < V; ++k) xv[k] = step_mix<HIST>(cf, x0[k], xv[k], zv[k], hv[k]);
  store_v<V>(f.x + e, xv);
  if (HIST) store_v<V>(f.hist + e, hv);
}

// two forwards (guided): the conditional output and the one on a zero condition; one forward: the conditional output as it is
__device__ __forceinline__ float guided_out(bool guided, float scale, float oc, float ou) {
  return guided ? add_rn(ou, mul_rn(scale, sub_rn(oc, ou))) : oc;
}

// ---- host: the argument checks of an entry, before anything is launched (who: the entry's name in the message).  static: the
// library exports its C entries, not these ----
struct Req { const void* p; const char* name; };
template <size_t N>
static inline int check_required(const char* who, const Req (&req)[N]) {
  for (const Req& q : req) {
    if (!q.p) { set_error("%s: %s is NULL", who, q.name); return SR3_E_BADARG; }
  }
  return SR3_OK;
}

// two checks, not one: an entry's own size rules (block, scale) come between them, and which fault is reported is observable
static inline int check_image_dims(const char* who, int batch, int channels, int height, int width) {
  if (batch <= 0 || channels <= 0 || height <= 0 || width <= 0) {
    set_error("%s: batch, channels, height and width must be positive (got %d, %d, %d, %d)", who, batch, channels, height, width);
    return SR3_E_BADARG;
  }
  return SR3_OK;
}
static inline int check_image_limit(const char* who, size_t total) {
  if (total >= ((size_t)1 << 31)) { set_error("%s: image batch too large (batch * channels * height * width >= 2^31)", who); return SR3_E_UNSUPPORTED; }
  return SR3_OK;
}

// every argument of an entry that is memory; a null (optional, absent) one takes no part
struct Buf { const void* p; size_t bytes; const char* name; bool written; };

// What the call writes shares no byte with anything else it is given: every written buffer, in table order, against every other one,
// in table order; the first pair found is reported as "<written> overlaps <other>".  named_last: the index of the one buffer that is
// named second even where it is the written one (sr3_guided_step's x), or -1.  same_w / same_r: the one pair (written, read) that may
// be the same buffer exactly -- the in-place form; a partial overlap of the two says so -- or -1s.
template <size_t N>
static inline int check_overlaps(const char* who, const Buf (&bufs)[N], int named_last = -1, int same_w = -1, int same_r = -1) {
  for (int i = 0; i < (int)N; ++i) {
    const Buf& w = bufs[i];
    if (!w.p || !w.written) continue;
    for (int j = 0; j < (int)N; ++j) {
      const Buf& o = bufs[j];
      if (!o.p || j == i) continue;
      const bool in_place = i == same_w && j == same_r;
      if ((in_place && w.p == o.p) || !overlaps(w.p, w.bytes, o.p, o.bytes)) continue;
      if (in_place) set_error("%s: %s overlaps %s partially (%s == %s is the in-place form)", who, w.name, o.name, w.name, o.name);
      else if (i == named_last) set_error("%s: %s overlaps %s", who, o.name, w.name);
      else set_error("%s: %s overlaps %s", who, w.name, o.name);
      return SR3_E_BADARG;
    }
  }
  return SR3_OK;
}

// the 16-byte path: every pointer a multiple of 16 (a null one is); the caller adds its own divisibility rule (W % 4, n % 4, r % 4)
template <class... P>
static inline bool vec16(const P*... p) { return (((uintptr_t)0 | ... | (uintptr_t)p) & 15) == 0; }

// runtime bools -> template arguments: f is called with one std::true_type / std::false_type per bool, in order
template <class F>
static inline void dispatch_bools(F&& f) { f(); }
template <class F, class... R>
static inline void dispatch_bools(F&& f, bool b, R... rest) {
  if (b) dispatch_bools([&](auto... c) { f(std::true_type{}, c...); }, rest...);
  else dispatch_bools([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}

}  // namespace sr3
