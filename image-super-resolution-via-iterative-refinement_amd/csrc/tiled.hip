// Tiled sampling (include/sr3_mi355x.h: sr3_tile_gather, sr3_tiled_step): the two HBM-bound kernels that run once per reverse step on
// the FULL image when the UNet itself runs on overlapping tiles of its training size -- cutting tile batches out of the running image,
// and the step's tail: blend the tiles' eps into one field, p_sample update, counter decrement.
//
// Both are in gather form: a thread owns output elements and reads what it needs, so there are no atomics and no zero-fill, and the
// result does not depend on launch order (bitwise reproducible).  Origins are arbitrary integers: a thread moves four consecutive x
// positions as one 16-byte access where the address allows (checked per access, on the address itself) and as four scalar accesses
// otherwise; the side that is always aligned (the tile batch of the gather; x, z and eps_out of the step) is always a vector access.
// Origins read from the device arrays are clamped into [0, L - t], so no origin, however wrong, makes a kernel leave its tensors.
#include "step_tail.h"

namespace sr3 {
namespace {

__device__ __forceinline__ int clamp_origin(int o, int L, int t) { return min(max(o, 0), L - t); }

// four consecutive floats at p: one 16-byte load where p allows
__device__ __forceinline__ f32x4 load4(const float* p) {
  if (((uintptr_t)p & 15) == 0) return *reinterpret_cast<const f32x4*>(p);
  f32x4 v = {p[0], p[1], p[2], p[3]};
  return v;
}

// dst[i][c][y][x] = src[b][c][oy[iy] + y][ox[ix] + x] for the tiles first_tile + i, i < n, of the order (b * ny + iy) * nx + ix.
// V = 4: a thread moves four x positions of one tile row (tw % 4 == 0, dst 16-byte aligned); V = 1: one element.
template <int V>
__global__ __launch_bounds__(256) void k_tile_gather(const float* __restrict__ src, int C, int H, int W, const int* __restrict__ oy,
                                                      int ny, const int* __restrict__ ox, int nx, int first_tile, int th, int tw,
                                                      float* __restrict__ dst, size_t total) {
  const int twv = tw / V;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int xq = (int)(i % twv);
    size_t r = i / twv;
    const int y = (int)(r % th); r /= th;
    const int c = (int)(r % C);
    const int g = first_tile + (int)(r / C);
    const int ix = g % nx, iy = (g / nx) % ny, b = g / (nx * ny);
    const int sy = clamp_origin(oy[iy], H, th) + y, sx = clamp_origin(ox[ix], W, tw) + xq * V;
    const float* s = src + (((size_t)b * C + c) * H + sy) * W + sx;
    if constexpr (V == 4) *reinterpret_cast<f32x4*>(dst + i * 4) = load4(s);
    else dst[i] = s[0];
  }
}

struct TiledStep {
  StepFuse f;                // the step's tail on x [B, C, H, W]; step_cur: k_step_copy put j there (clip: the kernel's template argument rules)
  const float* eps;          // [B * ny * nx, C, th, tw]
  const int* oy; const int* ox;
  const float* wy; const float* wx;
  float* eps_out;            // or null
  int C, H, W, ny, nx, th, tw;
};

// the tiles covering coordinate p along one axis are a contiguous range of the (increasing) origin list
__device__ __forceinline__ void cover(const int* __restrict__ o, int n, int L, int t, int p, int& lo, int& hi) {
  lo = n; hi = -1;
  for (int k = 0; k < n; ++k) {
    const int ok = clamp_origin(o[k], L, t);
    if (ok <= p && p < ok + t) { lo = min(lo, k); hi = k; }
  }
}

// eps of one pixel: the single covering tile's value as it is, else the weighted mean over the covering tiles in ascending tile index
__device__ __forceinline__ float blend_pixel(const TiledStep& s, int b, int c, int y, int x, int iy0, int iy1, int ix0, int ix1) {
  const size_t plane = (size_t)s.th * s.tw;
  if (iy0 == iy1 && ix0 == ix1) {
    const int ty = y - clamp_origin(s.oy[iy0], s.H, s.th), tx = x - clamp_origin(s.ox[ix0], s.W, s.tw);
    return s.eps[((((size_t)b * s.ny + iy0) * s.nx + ix0) * s.C + c) * plane + (size_t)ty * s.tw + tx];
  }
  float num = 0.f, den = 0.f;
  for (int iy = iy0; iy <= iy1; ++iy) {
    const int ty = y - clamp_origin(s.oy[iy], s.H, s.th);
    const float wyv = s.wy[min(max(ty, 0), s.th - 1)];
    for (int ix = ix0; ix <= ix1; ++ix) {
      const int tx = x - clamp_origin(s.ox[ix], s.W, s.tw);
      if ((unsigned)ty >= (unsigned)s.th || (unsigned)tx >= (unsigned)s.tw) continue;      // (only under origins that do not increase)
      const float w = mul_rn(wyv, s.wx[tx]);
      const float e = s.eps[((((size_t)b * s.ny + iy) * s.nx + ix) * s.C + c) * plane + (size_t)ty * s.tw + tx];
      num = add_rn(num, mul_rn(w, e));
      den = add_rn(den, w);
    }
  }
  return iy0 > iy1 || ix0 > ix1 ? 0.f : num / den;      // (no covering tile: only under origins the host entry would have refused)
}

// the same for four consecutive x positions that the same tile columns cover: the tiles' rows are read four values at a time
__device__ __forceinline__ f32x4 blend_quad(const TiledStep& s, int b, int c, int y, int x, int iy0, int iy1, int ix0, int ix1) {
  const size_t plane = (size_t)s.th * s.tw;
  if (iy0 == iy1 && ix0 == ix1) {
    const int ty = y - clamp_origin(s.oy[iy0], s.H, s.th), tx = x - clamp_origin(s.ox[ix0], s.W, s.tw);
    return load4(s.eps + ((((size_t)b * s.ny + iy0) * s.nx + ix0) * s.C + c) * plane + (size_t)ty * s.tw + tx);
  }
  f32x4 num = {0.f, 0.f, 0.f, 0.f}, den = {0.f, 0.f, 0.f, 0.f};
  if (iy0 > iy1 || ix0 > ix1) return num;
  for (int iy = iy0; iy <= iy1; ++iy) {
    const int ty = y - clamp_origin(s.oy[iy], s.H, s.th);
    const float wyv = s.wy[min(max(ty, 0), s.th - 1)];
    for (int ix = ix0; ix <= ix1; ++ix) {
      const int tx = x - clamp_origin(s.ox[ix], s.W, s.tw);
      if ((unsigned)ty >= (unsigned)s.th || tx < 0 || tx + 3 >= s.tw) continue;      // (only under origins that do not increase)
      const f32x4 e = load4(s.eps + ((((size_t)b * s.ny + iy) * s.nx + ix) * s.C + c) * plane + (size_t)ty * s.tw + tx);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float w = mul_rn(wyv, s.wx[tx + k]);
        num[k] = add_rn(num[k], mul_rn(w, e[k]));
        den[k] = add_rn(den[k], w);
      }
    }
  }
  f32x4 r;
#pragma unroll
  for (int k = 0; k < 4; ++k) r[k] = num[k] / den[k];
  return r;
}

// x <- p_sample update of (x, blended eps, z) at step index j = *step_cur; *step_next = j - 1 (tail_begin).  V = 4: a thread owns four x
// positions (W % 4 == 0, x / z / eps_out / hist 16-byte aligned); V = 1: one.  The update is step_x0 and the element I/O of step_tail.h,
// as every tail runs them; HIST: the multistep tail.
template <int V, bool CLIP, bool HIST>
__global__ __launch_bounds__(256) void k_tiled_step(TiledStep s, size_t total) {
  const StepFuse& f = s.f;
  const StepCoef cf = tail_begin<HIST>(f, blockIdx.x == 0 && threadIdx.x == 0);
  const int wv = s.W / V;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int x0 = (int)(i % wv) * V;
    size_t r = i / wv;
    const int y = (int)(r % s.H); r /= s.H;
    const int c = (int)(r % s.C), b = (int)(r / s.C);
    const size_t e0 = i * V;
    int iy0, iy1, ix0, ix1;
    cover(s.oy, s.ny, s.H, s.th, y, iy0, iy1);
    cover(s.ox, s.nx, s.W, s.tw, x0, ix0, ix1);
    float ev[V], xv[V], zv[V], hv[V], x0v[V];
    if constexpr (V == 4) {
      int jx0, jx1;
      cover(s.ox, s.nx, s.W, s.tw, x0 + 3, jx0, jx1);
      if (jx0 == ix0 && jx1 == ix1 && s.tw >= 4) {      // (tw >= 4: no tile fits between the first and the last of the four)
        const f32x4 q = blend_quad(s, b, c, y, x0, iy0, iy1, ix0, ix1);
#pragma unroll
        for (int k = 0; k < V; ++k) ev[k] = q[k];
      } else {                   // the four straddle a tile edge: each has its own set of columns
        ev[0] = blend_pixel(s, b, c, y, x0, iy0, iy1, ix0, ix1);
        ev[V - 1] = blend_pixel(s, b, c, y, x0 + 3, iy0, iy1, jx0, jx1);
        for (int k = 1; k < V - 1; ++k) {
          cover(s.ox, s.nx, s.W, s.tw, x0 + k, jx0, jx1);
          ev[k] = blend_pixel(s, b, c, y, x0 + k, iy0, iy1, jx0, jx1);
        }
      }
    } else {
      ev[0] = blend_pixel(s, b, c, y, x0, iy0, iy1, ix0, ix1);
    }
    tail_load<HIST, V>(f, e0, xv, zv, hv);
#pragma unroll
    for (int k = 0; k < V; ++k) x0v[k] = step_x0(cf, CLIP, xv[k], ev[k]);
    tail_mix_store<HIST, V>(f, cf, e0, x0v, xv, zv, hv);
    if (s.eps_out) store_v<V>(s.eps_out + e0, ev);
  }
}

// slot 0 <- slot 1: the step kernel reads slot 0 and writes slot 1, so no block of it races with another (as in sr3_reverse_step, where
// the embedding kernel makes the copy)
__global__ void k_step_copy(int* step2) { if (threadIdx.x == 0 && blockIdx.x == 0) step2[0] = step2[1]; }

int grid_for(size_t total) {
  const size_t blocks = (total + 255) / 256;
  return (int)(blocks > 4096 ? 4096 : blocks);
}

// host copy of an origin list: starts at 0, strictly increasing, ends at L - t, and no gap between consecutive tiles
int check_origins(const char* axis, const int* o, int n, int L, int t) {
  if (o[0] != 0 || o[n - 1] != L - t) { set_error("tiling: the %s origins must start at 0 and end at %d (got %d .. %d)", axis, L - t, o[0], o[n - 1]); return SR3_E_BADARG; }
  for (int k = 1; k < n; ++k) {
    if (o[k] <= o[k - 1]) { set_error("tiling: the %s origins are not strictly increasing at index %d", axis, k); return SR3_E_BADARG; }
    if (o[k] > o[k - 1] + t) { set_error("tiling: the %s tiles %d and %d leave a gap", axis, k - 1, k); return SR3_E_BADARG; }
  }
  return SR3_OK;
}

}  // namespace

int step_copy(int* step2, hipStream_t st) {
  hipLaunchKernelGGL(k_step_copy, dim3(1), dim3(64), 0, st, step2);
  SR3_LAUNCH_CHECK("k_step_copy");
  return SR3_OK;
}

}  // namespace sr3

using namespace sr3;

extern "C" {

int sr3_tile_gather(const float* src_nchw, int batch, int channels, int height, int width, const int* oy_dev, int ny, const int* ox_dev,
                    int nx, int first_tile, int n_tiles, int th, int tw, float* dst_tiles, void* stream) {
  if (!src_nchw || !oy_dev || !ox_dev || !dst_tiles) { set_error("tile_gather: null argument"); return SR3_E_BADARG; }
  if (batch <= 0 || channels <= 0 || height <= 0 || width <= 0 || ny <= 0 || nx <= 0 || th <= 0 || tw <= 0) { set_error("tile_gather: sizes must be positive"); return SR3_E_BADARG; }
  if (th > height || tw > width) { set_error("tile_gather: tile %d x %d larger than the image %d x %d", th, tw, height, width); return SR3_E_BADARG; }
  if ((size_t)batch * channels * height * width >= ((size_t)1 << 31) || (size_t)batch * ny * nx >= ((size_t)1 << 31)) { set_error("tile_gather: image batch too large (>= 2^31 elements)"); return SR3_E_UNSUPPORTED; }
  if (first_tile < 0 || n_tiles <= 0 || (size_t)first_tile + n_tiles > (size_t)batch * ny * nx) {
    set_error("tile_gather: tiles [%d, %d + %d) outside the %d x %d x %d tiles of the batch", first_tile, first_tile, n_tiles, batch, ny, nx);
    return SR3_E_BADARG;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t elems = (size_t)n_tiles * channels * th * tw;
  if ((tw & 3) == 0 && ((uintptr_t)dst_tiles & 15) == 0) {
    hipLaunchKernelGGL(k_tile_gather<4>, dim3(grid_for(elems / 4)), dim3(256), 0, st, src_nchw, channels, height, width, oy_dev, ny, ox_dev, nx,
                       first_tile, th, tw, dst_tiles, elems / 4);
  } else {
    hipLaunchKernelGGL(k_tile_gather<1>, dim3(grid_for(elems)), dim3(256), 0, st, src_nchw, channels, height, width, oy_dev, ny, ox_dev, nx,
                       first_tile, th, tw, dst_tiles, elems);
  }
  SR3_LAUNCH_CHECK("k_tile_gather");
  return SR3_OK;
}

int sr3_tiled_step_hist(float* x_nchw, const float* eps_tiles, int batch, int channels, int height, int width, const int* oy_dev, int ny,
                        const int* ox_dev, int nx, const float* wy_dev, const float* wx_dev, int th, int tw, const int* oy_host,
                        const int* ox_host, const float* z_nchw, const float* ta, const float* tb, const float* tc1, const float* tc2,
                        const float* tsig, int* step2_dev, int clip_denoised, float* eps_out_nchw, void* stream, const float* tc3,
                        float* hist_nchw) {
  if (!x_nchw || !eps_tiles || !oy_dev || !ox_dev || !wy_dev || !wx_dev || !ta || !tb || !tc1 || !tc2 || !tsig || !step2_dev) { set_error("tiled_step: null argument"); return SR3_E_BADARG; }
  if (batch <= 0 || channels <= 0 || height <= 0 || width <= 0 || ny <= 0 || nx <= 0 || th <= 0 || tw <= 0) { set_error("tiled_step: sizes must be positive"); return SR3_E_BADARG; }
  if (th > height || tw > width) { set_error("tiled_step: tile %d x %d larger than the image %d x %d", th, tw, height, width); return SR3_E_BADARG; }
  const size_t total = (size_t)batch * channels * height * width;
  if (total >= ((size_t)1 << 31) || (size_t)batch * ny * nx >= ((size_t)1 << 31)) { set_error("tiled_step: image batch too large (B * C * H * W >= 2^31)"); return SR3_E_UNSUPPORTED; }
  if (oy_host) { if (const int rc = check_origins("y", oy_host, ny, height, th)) return rc; }
  if (ox_host) { if (const int rc = check_origins("x", ox_host, nx, width, tw)) return rc; }
  if (const int rc = check_step_history("tiled_step", tc3, hist_nchw, x_nchw, eps_out_nchw, total * sizeof(float))) return rc;
  TiledStep s;
  s.f = StepFuse{x_nchw, z_nchw, StepTables{ta, tb, tc1, tc2, tsig}, step2_dev, step2_dev + 1, clip_denoised, tc3, hist_nchw};
  s.eps = eps_tiles; s.oy = oy_dev; s.ox = ox_dev; s.wy = wy_dev; s.wx = wx_dev; s.eps_out = eps_out_nchw;
  s.C = channels; s.H = height; s.W = width; s.ny = ny; s.nx = nx; s.th = th; s.tw = tw;
  const bool vec = (width & 3) == 0;
  if (vec && !vec16(x_nchw, z_nchw, eps_out_nchw, hist_nchw)) { set_error("tiled_step: misaligned pointer (x, z, eps_out, hist: 16 B)"); return SR3_E_ALIGN; }
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (const int rc = step_copy(step2_dev, st)) return rc;
  const size_t work = vec ? total / 4 : total;
  const dim3 grid(grid_for(work));
  dispatch_bools([&](auto v4, auto clip, auto hist) {
    hipLaunchKernelGGL((k_tiled_step<v4() ? 4 : 1, clip(), hist()>), grid, dim3(256), 0, st, s, work);
  }, vec, clip_denoised != 0, hist_nchw != nullptr);
  SR3_LAUNCH_CHECK("k_tiled_step");
  return SR3_OK;
}

int sr3_tiled_step(float* x_nchw, const float* eps_tiles, int batch, int channels, int height, int width, const int* oy_dev, int ny,
                   const int* ox_dev, int nx, const float* wy_dev, const float* wx_dev, int th, int tw, const int* oy_host,
                   const int* ox_host, const float* z_nchw, const float* ta, const float* tb, const float* tc1, const float* tc2,
                   const float* tsig, int* step2_dev, int clip_denoised, float* eps_out_nchw, void* stream) {
  return sr3_tiled_step_hist(x_nchw, eps_tiles, batch, channels, height, width, oy_dev, ny, ox_dev, nx, wy_dev, wx_dev, th, tw, oy_host,
                             ox_host, z_nchw, ta, tb, tc1, tc2, tsig, step2_dev, clip_denoised, eps_out_nchw, stream, nullptr, nullptr);
}

}  // extern "C"
