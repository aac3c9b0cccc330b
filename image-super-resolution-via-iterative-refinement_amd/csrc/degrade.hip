// The degradation between an HR crop and its LR / SR conditioning images, on the device next to transform_augment (io_metrics.hip)
// and the Pillow-exact resize (resize.hip):  HR --blur--> resize down --noise--> LR --resize up--> SR   (data/degrade.py)
//   sr3_blur_u8 : per-image k x k correlation in 16-bit fixed point, reflect-101 border, integer arithmetic => the result does not
//                 depend on the summation order and equals the NumPy restatement bit for bit
//   sr3_noise_u8: out = clamp(rint(in + sigma_i * z)), separately rounded fp32 multiply and add, round-half-even
#include <stdint.h>

#include "sr3_common.h"
#include "../../include/sr3_io_mi355x.h"

namespace sr3 {
namespace {

constexpr int BLUR_KMAX = 21;                 // largest kernel side
constexpr int BLUR_TH = 16, BLUR_TW = 32;     // output pixels per workgroup
constexpr int BLUR_NT = 256;
constexpr int BLUR_ONE = 1 << 16;             // fixed-point 1.0

// np.pad(mode='reflect') index; a tile's overhang past the image (rows / columns no output of the tile reads) is clamped into it
__device__ __forceinline__ int reflect101(int i, int n) {
  if (i < 0) i = -i;
  if (i >= n) i = 2 * n - 2 - i;
  return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

// One workgroup: a 16 x 32 pixel tile of one image.  LDS holds the u8 tile with its k/2 halo ((16 + 20) x (32 + 20) x 3 = 5616 B at
// most) beside the image's k x k weights (1764 B): 7.4 KB per workgroup, far below what the CU's wave slots could use (registers allow
// seven workgroups per CU, 52 KB of its 160 KB).  A thread
// owns NOUT elements of the tile's (row, x * C + c) plane, 256 apart: a wave reads 64 consecutive bytes per tap (16 banks, no conflict)
// and the tap's weight as one broadcast; v_mad_i32_i24 per tap and element (|w| < 2^23, sr3_io_mi355x.h).
template <int C>
__global__ __launch_bounds__(BLUR_NT) void k_blur_u8(const unsigned char* __restrict__ in, int H, int W, const int* __restrict__ weights,
                                                     int k, unsigned char* __restrict__ out) {
  constexpr int RW = BLUR_TW * C, NOUT = BLUR_TH * RW / BLUR_NT;
  static_assert(BLUR_TH * RW % BLUR_NT == 0, "whole elements per thread");
  __shared__ unsigned char tile[(BLUR_TH + BLUR_KMAX - 1) * (BLUR_TW + BLUR_KMAX - 1) * C];
  __shared__ int wsm[BLUR_KMAX * BLUR_KMAX];
  __shared__ int not_delta;
  const int tid = threadIdx.x, img = blockIdx.z;
  const int r = k >> 1, kk = k * k;
  const int y0 = blockIdx.y * BLUR_TH, x0 = blockIdx.x * BLUR_TW;
  const size_t per = (size_t)H * W * C;
  const unsigned char* ib = in + img * per;
  unsigned char* ob = out + img * per;
  const int* wi = weights + (size_t)img * kk;

  if (tid == 0) not_delta = 0;
  __syncthreads();
  bool nd = false;
  for (int i = tid; i < kk; i += BLUR_NT) {
    const int w = wi[i];
    wsm[i] = w;
    nd |= w != (i == kk / 2 ? BLUR_ONE : 0);
  }
  if (nd) not_delta = 1;                       // every writer stores the same value
  __syncthreads();

  // the thread's elements: e = tid + j * 256 -> (row y, byte xc of the row)
  int ey[NOUT], exc[NOUT];
#pragma unroll
  for (int j = 0; j < NOUT; ++j) {
    const int e = tid + j * BLUR_NT;
    ey[j] = e / RW;
    exc[j] = e - ey[j] * RW;
  }
  const int row_bytes = W * C;

  if (!not_delta) {                            // centre tap 1.0, rest 0: (65536 v + 32768) >> 16 == v -- copy, the same bytes
#pragma unroll
    for (int j = 0; j < NOUT; ++j) {
      const int y = y0 + ey[j], xb = x0 * C + exc[j];
      if (y < H && xb < row_bytes) ob[(size_t)y * row_bytes + xb] = ib[(size_t)y * row_bytes + xb];
    }
    return;
  }

  const int PW = BLUR_TW + 2 * r, PH = BLUR_TH + 2 * r;
  for (int i = tid; i < PH * PW; i += BLUR_NT) {
    const int py = i / PW, px = i - py * PW;
    const int gy = reflect101(y0 + py - r, H), gx = reflect101(x0 + px - r, W);
    const unsigned char* p = ib + ((size_t)gy * W + gx) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) tile[i * C + c] = p[c];
  }
  __syncthreads();

  const int stride = PW * C;
  int base[NOUT], acc[NOUT];
#pragma unroll
  for (int j = 0; j < NOUT; ++j) { base[j] = ey[j] * stride + exc[j]; acc[j] = BLUR_ONE >> 1; }
  for (int dy = 0; dy < k; ++dy) {
    for (int dx = 0; dx < k; ++dx) {
      const int w = wsm[dy * k + dx];
      const int off = dy * stride + dx * C;
#pragma unroll
      for (int j = 0; j < NOUT; ++j) acc[j] += __mul24(w, (int)tile[base[j] + off]);
    }
  }
#pragma unroll
  for (int j = 0; j < NOUT; ++j) {
    const int y = y0 + ey[j], xb = x0 * C + exc[j];
    if (y < H && xb < row_bytes) {
      const int v = acc[j] >> 16;              // arithmetic shift
      ob[(size_t)y * row_bytes + xb] = (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
    }
  }
}

// (in and out may be the same buffer: a thread reads its element before it writes it, and neither pointer is __restrict__)
__global__ __launch_bounds__(256) void k_noise_u8(const unsigned char* in, size_t per, const float* __restrict__ sigma,
                                                  const float* __restrict__ z, unsigned char* out) {
  const int img = blockIdx.y;
  const unsigned char* ib = in + img * per;
  const float* zb = z + img * per;
  unsigned char* ob = out + img * per;
  const float s = sigma[img];
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < per; i += (size_t)gridDim.x * blockDim.x) {
    unsigned char v = ib[i];
    if (s != 0.f) {                            // sigma 0: the identity, whatever z holds
      const float f = rintf(add_rn((float)v, mul_rn(s, zb[i])));
      v = (unsigned char)fminf(fmaxf(f, 0.f), 255.f);
    }
    ob[i] = v;
  }
}

}  // namespace
}  // namespace sr3

using namespace sr3;

extern "C" {

int sr3_blur_u8(const uint8_t* in_hwc, int n_images, int H, int W, int C, const int32_t* weights, int k, uint8_t* out_hwc, void* stream) {
  if (!in_hwc) { set_error("blur_u8: in_hwc is NULL"); return SR3_E_BADARG; }
  if (!weights) { set_error("blur_u8: weights is NULL"); return SR3_E_BADARG; }
  if (!out_hwc) { set_error("blur_u8: out_hwc is NULL"); return SR3_E_BADARG; }
  if (n_images <= 0 || n_images > 65535) { set_error("blur_u8: n_images %d outside 1..65535", n_images); return SR3_E_BADARG; }
  if (H <= 0 || (H + BLUR_TH - 1) / BLUR_TH > 65535) { set_error("blur_u8: H %d outside 1..%d", H, 65535 * BLUR_TH); return SR3_E_BADARG; }
  if (W <= 0) { set_error("blur_u8: W %d is not positive", W); return SR3_E_BADARG; }
  if (C != 1 && C != 3) { set_error("blur_u8: C %d is not 1 or 3", C); return SR3_E_BADARG; }
  if (k < 1 || k > BLUR_KMAX || !(k & 1)) { set_error("blur_u8: k %d is not an odd number in 1..%d", k, BLUR_KMAX); return SR3_E_BADARG; }
  if (k / 2 >= (H < W ? H : W)) { set_error("blur_u8: k %d reflects past a %d x %d image (k / 2 must be below min(H, W))", k, H, W); return SR3_E_BADARG; }
  const size_t bytes = (size_t)n_images * H * W * C;
  if (overlaps(in_hwc, bytes, out_hwc, bytes)) { set_error("blur_u8: out_hwc overlaps in_hwc (the blur does not run in place)"); return SR3_E_BADARG; }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((W + BLUR_TW - 1) / BLUR_TW, (H + BLUR_TH - 1) / BLUR_TH, n_images);
  if (C == 3) hipLaunchKernelGGL(k_blur_u8<3>, grid, dim3(BLUR_NT), 0, st, in_hwc, H, W, weights, k, out_hwc);
  else hipLaunchKernelGGL(k_blur_u8<1>, grid, dim3(BLUR_NT), 0, st, in_hwc, H, W, weights, k, out_hwc);
  SR3_LAUNCH_CHECK("k_blur_u8");
  return SR3_OK;
}

int sr3_noise_u8(const uint8_t* in, int n_images, size_t elems_per_image, const float* sigma, const float* z, uint8_t* out, void* stream) {
  if (!in) { set_error("noise_u8: in is NULL"); return SR3_E_BADARG; }
  if (!sigma) { set_error("noise_u8: sigma is NULL"); return SR3_E_BADARG; }
  if (!z) { set_error("noise_u8: z is NULL"); return SR3_E_BADARG; }
  if (!out) { set_error("noise_u8: out is NULL"); return SR3_E_BADARG; }
  if (n_images <= 0 || n_images > 65535) { set_error("noise_u8: n_images %d outside 1..65535", n_images); return SR3_E_BADARG; }
  if (elems_per_image == 0) { set_error("noise_u8: elems_per_image is 0"); return SR3_E_BADARG; }
  const size_t bytes = (size_t)n_images * elems_per_image;
  if (in != out && overlaps(in, bytes, out, bytes)) { set_error("noise_u8: out overlaps in partially (in place means out == in)"); return SR3_E_BADARG; }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t b = (elems_per_image + 255) / 256;
  hipLaunchKernelGGL(k_noise_u8, dim3((unsigned)(b > 1024 ? 1024 : b), n_images), dim3(256), 0, st, in, elems_per_image, sigma, z, out);
  SR3_LAUNCH_CHECK("k_noise_u8");
  return SR3_OK;
}

}  // extern "C"
