// The degradation between an HR crop and its LR / SR conditioning images, on the device next to transform_augment (io_metrics.hip)
// and the Pillow-exact resize (resize.hip):  HR --blur--> resize down --noise--> [jpeg] LR --resize up--> SR   (data/degrade.py)
//   sr3_blur_u8 : per-image k x k correlation in 16-bit fixed point, reflect-101 border, integer arithmetic => the result does not
//                 depend on the summation order and equals the NumPy restatement bit for bit
//   sr3_noise_u8: out = clamp(rint(in + sigma_i * z)), separately rounded fp32 multiply and add, round-half-even
//   sr3_noise_ex_u8: the same with a per-image mode -- Gaussian or Poisson (shot) noise, per channel or one value per pixel (gray); the
//                 Poisson draw is a binary search of an integer CDF table => equals the NumPy restatement bit for bit
//   sr3_jpeg_u8 : the lossy half of a JPEG round trip on the LR image (between the noise and the resize up), libjpeg's integer arithmetic
//                 as Pillow drives it => equals Pillow's save / open bytes and the NumPy restatement bit for bit
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

// k = #{j : row[j] <= r} of a non-decreasing row of kmax entries: at most ceil(log2(kmax + 1)) probes (9 of the 384-column Poisson table)
__device__ __forceinline__ int count_le(const int* __restrict__ row, int kmax, int r) {
  int lo = 0, hi = kmax;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (row[mid] <= r) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ unsigned char noise_clamp(float f) { return (unsigned char)fminf(fmaxf(rintf(f), 0.f), 255.f); }

// One thread per pixel; the thread owns the pixel's C bytes, reads them before it writes them (in and out may be the same buffer:
// neither pointer is __restrict__).  A pixel is C bytes at byte offset C * p and its draws C words at word offset C * p: for C == 3
// nothing wider than a byte resp. a dword is aligned, for C == 1 there is one of each -- so the accesses are the natural ones.
// mode (low two bits): bit 0 = gray (one draw per pixel), bit 1 = Poisson.  A mode whose draws are absent (z resp. r / table NULL)
// copies, as strength 0 does: nothing is dereferenced that the caller did not pass.
template <int C>
__global__ __launch_bounds__(256) void k_noise_ex_u8(const unsigned char* in, int HW, const int* __restrict__ mode,
                                                     const float* __restrict__ strength, const float* __restrict__ z,
                                                     const int* __restrict__ r, const int* __restrict__ table, int kmax, unsigned char* out) {
  const int img = blockIdx.y;
  const unsigned pu = blockIdx.x * 256u + threadIdx.x;
  if (pu >= (unsigned)HW) return;                // (n * H * W * C < 2^31: the host checked)
  const size_t o = ((size_t)img * HW + pu) * C;
  int v[C];
#pragma unroll
  for (int c = 0; c < C; ++c) v[c] = in[o + c];
  const float s = strength[img];
  const int m = mode[img] & 3;
  const bool gray = m & 1, poisson = m & 2;
  if (s != 0.f && !poisson && z) {
    float zz[C];
#pragma unroll
    for (int c = 0; c < C; ++c) zz[c] = z[o + (gray ? 0 : c)];
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = noise_clamp(add_rn((float)v[c], mul_rn(s, zz[c])));
  } else if (s != 0.f && poisson && r && table) {
    if (gray && C == 3) {
      const int Y = (19595 * v[0] + 38470 * v[1] + 7471 * v[2] + 32768) >> 16;      // the JPEG kernel's luma (FIX(.299), ...): <= 255
      const int k = count_le(table + (size_t)Y * kmax, kmax, r[o]);
      const float d = mul_rn(s, (float)(k - Y));
#pragma unroll
      for (int c = 0; c < C; ++c) v[c] = noise_clamp(add_rn((float)v[c], d));
    } else {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const int k = count_le(table + (size_t)v[c] * kmax, kmax, r[o + c]);
        v[c] = noise_clamp(add_rn((float)v[c], mul_rn(s, (float)(k - v[c]))));
      }
    }
  }
#pragma unroll
  for (int c = 0; c < C; ++c) out[o + c] = (unsigned char)v[c];
}

// ---- JPEG: libjpeg's lossy half as Pillow drives it ("islow" integer DCT, fancy up-sampling), without the entropy coder ----
// Two kernels with the decoded planes in scratch between them: k_jpeg_codec reads `in` and writes scratch, k_jpeg_finish reads scratch
// (and, for a pass-through image, its own element of `in`) and writes `out` -- so out == in is safe.
// scratch, per image: Y (H x W bytes), then for C == 3 Cb and Cr (ph x pw each: H x W at 4:4:4, ceil(H/2) x ceil(W/2) at 4:2:0).
constexpr int JPEG_NT = 256;                  // four waves, eight 8 x 8 blocks each
constexpr int JPEG_BLOCKS = JPEG_NT / 8;      // blocks per workgroup
constexpr int JPEG_BS = 72, JPEG_RS = 9;      // LDS strides (ints) of a block and of a row: see k_jpeg_codec
constexpr int jfix(double v) { return (int)(v * 65536 + 0.5); }
constexpr int F_0_298 = 2446, F_0_390 = 3196, F_0_541 = 4433, F_0_765 = 6270, F_0_899 = 7373, F_1_175 = 9633;
constexpr int F_1_501 = 12299, F_1_847 = 15137, F_1_961 = 16069, F_2_053 = 16819, F_2_562 = 20995, F_3_072 = 25172;

// Annex K: luminance, chrominance; row-major (row = vertical frequency)
__constant__ unsigned char JPEG_BASE_Q[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// plane 0 / 1 / 2 = Y / Cb / Cr of an RGB pixel (C == 1: the byte is Y)
template <int C>
__device__ __forceinline__ int jpeg_component(const unsigned char* px, int plane) {
  if constexpr (C == 1) return px[0];
  const int R = px[0], G = px[1], B = px[2];
  if (plane == 0) return (jfix(.299) * R + jfix(.587) * G + jfix(.114) * B + 32768) >> 16;
  if (plane == 1) return (-jfix(.16874) * R - jfix(.33126) * G + jfix(.5) * B + (128 << 16) + 32767) >> 16;
  return (jfix(.5) * R - jfix(.41869) * G - jfix(.08131) * B + (128 << 16) + 32767) >> 16;
}

// the odd half both transforms share (Loeffler-Ligtenberg-Moschytz, 12 multiplies in all): four inputs -> the four rotated sums
__device__ __forceinline__ void dct_odd(int& t4, int& t5, int& t6, int& t7) {
  int z1 = t4 + t7, z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * F_1_175;
  t4 *= F_0_298; t5 *= F_2_053; t6 *= F_3_072; t7 *= F_1_501;
  z1 *= -F_0_899; z2 *= -F_2_562;
  z3 = z3 * -F_1_961 + z5; z4 = z4 * -F_0_390 + z5;
  t4 += z1 + z3; t5 += z2 + z4; t6 += z2 + z3; t7 += z1 + z4;
}

// one forward pass over eight values in place; FIRST: the row pass (outputs scaled up by 2 bits), else the column pass
template <bool FIRST>
__device__ __forceinline__ void fdct8(int (&d)[8]) {
  constexpr int N = FIRST ? 11 : 15;
  const int t0 = d[0] + d[7], t1 = d[1] + d[6], t2 = d[2] + d[5], t3 = d[3] + d[4];
  int t7 = d[0] - d[7], t6 = d[1] - d[6], t5 = d[2] - d[5], t4 = d[3] - d[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  d[0] = FIRST ? (t10 + t11) << 2 : descale(t10 + t11, 2);
  d[4] = FIRST ? (t10 - t11) << 2 : descale(t10 - t11, 2);
  const int z1 = (t12 + t13) * F_0_541;
  d[2] = descale(z1 + t13 * F_0_765, N);
  d[6] = descale(z1 - t12 * F_1_847, N);
  dct_odd(t4, t5, t6, t7);
  d[7] = descale(t4, N); d[5] = descale(t5, N); d[3] = descale(t6, N); d[1] = descale(t7, N);
}

// one inverse pass, descaled by N bits (11: columns, 18: rows)
template <int N>
__device__ __forceinline__ void idct8(int (&c)[8]) {
  const int z1 = (c[2] + c[6]) * F_0_541;
  const int t2 = z1 - c[6] * F_1_847, t3 = z1 + c[2] * F_0_765;
  const int t0 = (c[0] + c[4]) << 13, t1 = (c[0] - c[4]) << 13;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  int a0 = c[7], a1 = c[5], a2 = c[3], a3 = c[1];
  dct_odd(a0, a1, a2, a3);
  c[0] = descale(t10 + a3, N); c[7] = descale(t10 - a3, N);
  c[1] = descale(t11 + a2, N); c[6] = descale(t11 - a2, N);
  c[2] = descale(t12 + a1, N); c[5] = descale(t12 - a1, N);
  c[3] = descale(t13 + a0, N); c[4] = descale(t13 - a0, N);
}

// lane (block b, row r) holds row r of its block -> lane (b, column j) holds column j, through the wave's own LDS strip, and back the
// same way.  Block stride 72 and row stride 9 ints: a 32-lane half writes v[c] to banks 8 (b + r) + r + c and reads from banks
// 8 b + 9 r' + j, (b, r) resp. (b, j) over 4 x 8 -- all 32 distinct either way (ds_write_b32 / ds_read_b32 bank on 32 dwords).
__device__ __forceinline__ void jpeg_transpose(int* blk, int l, int (&v)[8]) {
  __syncthreads();                               // the strip's previous readers are done
#pragma unroll
  for (int c = 0; c < 8; ++c) blk[l * JPEG_RS + c] = v[c];
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 8; ++r) v[r] = blk[r * JPEG_RS + l];
}

// grid (ceil(blocks per image / 32), n_images).  The blocks of an image: by x bx of Y, then (C == 3) cy x cx of Cb and of Cr.
template <int C, bool SUB>
__global__ __launch_bounds__(JPEG_NT) void k_jpeg_codec(const unsigned char* __restrict__ in, int H, int W, const int* __restrict__ quality,
                                                        unsigned char* __restrict__ scratch, size_t scratch_per_image) {
  __shared__ int qt[2][64];
  __shared__ int strip[JPEG_BLOCKS * JPEG_BS];
  const int tid = threadIdx.x, img = blockIdx.y;
  int q = quality[img];
  if (q <= 0) return;                            // pass-through image (the whole workgroup: one image per blockIdx.y)
  q = q > 100 ? 100 : q;
  if (tid < 128) {
    const int s = q < 50 ? 5000 / q : 200 - 2 * q;
    const int t = ((int)JPEG_BASE_Q[tid >> 6][tid & 63] * s + 50) / 100;
    qt[tid >> 6][tid & 63] = t < 1 ? 1 : (t > 255 ? 255 : t);
  }
  const int bx = (W + 7) >> 3, by = (H + 7) >> 3;
  const int ph = SUB ? (H + 1) >> 1 : H, pw = SUB ? (W + 1) >> 1 : W;      // a chroma plane's real samples
  const int cx = (pw + 7) >> 3, cy = (ph + 7) >> 3;
  const int nY = bx * by, nC = C == 3 ? cx * cy : 0;
  const int g = blockIdx.x * JPEG_BLOCKS + (tid >> 3), l = tid & 7;
  const bool active = g < nY + 2 * nC;
  const int plane = g < nY ? 0 : (g < nY + nC ? 1 : 2);
  const int gb = g - (plane == 0 ? 0 : (plane == 1 ? nY : nY + nC));
  const int nbx = plane == 0 ? bx : cx;
  const int brow = gb / nbx, bcol = gb - brow * nbx;
  const unsigned char* ib = in + (size_t)img * H * W * C;
  int* blk = strip + (tid >> 3) * JPEG_BS;

  // the lane's row of samples - 128; padding = index clamp
  int v[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) v[c] = 0;
  if (active) {
    if (SUB && plane != 0) {
      // rows: the full-resolution plane padded to an even row count, down-sampled, THEN the down-sampled plane's last row replicated;
      // columns: the full-resolution plane's last column replicated, then down-sampled (the bias follows the padded column's parity)
      int rr = brow * 8 + l;
      rr = rr < ph ? rr : ph - 1;
      const int y0 = 2 * rr, y1 = 2 * rr + 1 < H ? 2 * rr + 1 : H - 1;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int cc = bcol * 8 + c;
        const int x0 = 2 * cc < W ? 2 * cc : W - 1, x1 = 2 * cc + 1 < W ? 2 * cc + 1 : W - 1;
        const int sum = jpeg_component<C>(ib + ((size_t)y0 * W + x0) * C, plane) + jpeg_component<C>(ib + ((size_t)y0 * W + x1) * C, plane) +
                        jpeg_component<C>(ib + ((size_t)y1 * W + x0) * C, plane) + jpeg_component<C>(ib + ((size_t)y1 * W + x1) * C, plane);
        v[c] = ((sum + 1 + (cc & 1)) >> 2) - 128;
      }
    } else {
      int y = brow * 8 + l;
      y = y < H ? y : H - 1;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        int x = bcol * 8 + c;
        x = x < W ? x : W - 1;
        v[c] = jpeg_component<C>(ib + ((size_t)y * W + x) * C, plane) - 128;
      }
    }
  }

  fdct8<true>(v);                                // rows
  jpeg_transpose(blk, l, v);                     // now column l: v[u] = vertical frequency u (qt is visible behind the barriers too)
  fdct8<false>(v);                               // columns: 8 x the true coefficients
  const int* tq = qt[plane == 0 ? 0 : 1];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int t = tq[u * 8 + l], qv = t << 3;
    const int a = v[u] < 0 ? -v[u] : v[u];
    const int cq = (int)((unsigned)(a + (qv >> 1)) / (unsigned)qv) * t;      // quantise, dequantise
    v[u] = v[u] < 0 ? -cq : cq;
  }
  idct8<11>(v);                                  // columns
  jpeg_transpose(blk, l, v);                     // row l again
  idct8<18>(v);                                  // rows

  if (!active) return;
  const int oh = plane == 0 ? H : ph, ow = plane == 0 ? W : pw;
  const int y = brow * 8 + l;
  if (y >= oh) return;
  unsigned char* ob = scratch + (size_t)img * scratch_per_image + (plane == 0 ? 0 : (size_t)H * W + (size_t)(plane - 1) * ph * pw) + (size_t)y * ow;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int x = bcol * 8 + c, s = v[c] + 128;
    if (x < ow) ob[x] = (unsigned char)(s < 0 ? 0 : (s > 255 ? 255 : s));
  }
}

// one thread per pixel: fancy h2v2 up-sampling of the chroma planes (SUB), YCbCr -> RGB.  in and out may be the same buffer: a
// pass-through thread reads its pixel before it writes it, every other thread reads scratch only (neither pointer is __restrict__).
template <int C, bool SUB>
__global__ __launch_bounds__(256) void k_jpeg_finish(const unsigned char* in, int H, int W, const int* __restrict__ quality,
                                                     const unsigned char* __restrict__ scratch, size_t scratch_per_image, unsigned char* out) {
  const int img = blockIdx.y;
  const unsigned iu = blockIdx.x * 256u + threadIdx.x;
  if (iu >= (unsigned)(H * W)) return;           // (H * W < 2^31: the host checked)
  const int i = (int)iu;
  const size_t o = ((size_t)img * H * W + i) * C;
  if (quality[img] <= 0) {
    unsigned char p[C];
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] = in[o + c];
#pragma unroll
    for (int c = 0; c < C; ++c) out[o + c] = p[c];
    return;
  }
  const unsigned char* sb = scratch + (size_t)img * scratch_per_image;
  const int Y = sb[i];
  if constexpr (C == 1) { out[o] = (unsigned char)Y; return; }
  const int ph = SUB ? (H + 1) >> 1 : H, pw = SUB ? (W + 1) >> 1 : W;
  int cbcr[2];
  if (SUB) {
    const int y = i / W, x = i - y * W;
    const int r = y >> 1, c = x >> 1;
    int rn = (y & 1) ? r + 1 : r - 1, cn = (x & 1) ? c + 1 : c - 1;      // the nearer neighbours, clamped to the real samples
    rn = rn < 0 ? 0 : (rn >= ph ? ph - 1 : rn);
    cn = cn < 0 ? 0 : (cn >= pw ? pw - 1 : cn);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const unsigned char* p = sb + (size_t)H * W + (size_t)k * ph * pw;
      const int s_this = 3 * p[r * pw + c] + p[rn * pw + c], s_near = 3 * p[r * pw + cn] + p[rn * pw + cn];
      cbcr[k] = (3 * s_this + s_near + ((x & 1) ? 7 : 8)) >> 4;
    }
  } else {
    cbcr[0] = sb[(size_t)H * W + i];
    cbcr[1] = sb[(size_t)2 * H * W + i];
  }
  const int xb = cbcr[0] - 128, zr = cbcr[1] - 128;
  const int R = Y + ((jfix(1.402) * zr + 32768) >> 16);
  const int G = Y + ((-jfix(.34414) * xb - jfix(.71414) * zr + 32768) >> 16);
  const int B = Y + ((jfix(1.772) * xb + 32768) >> 16);
  out[o] = (unsigned char)(R < 0 ? 0 : (R > 255 ? 255 : R));
  out[o + 1] = (unsigned char)(G < 0 ? 0 : (G > 255 ? 255 : G));
  out[o + 2] = (unsigned char)(B < 0 ? 0 : (B > 255 ? 255 : B));
}

// bytes of one image's decoded planes; 0: a geometry sr3_jpeg_u8 refuses
size_t jpeg_scratch_per_image(int n_images, int H, int W, int C, int subsampling) {
  if (n_images <= 0 || n_images > 65535 || H <= 0 || W <= 0 || (C != 1 && C != 3)) return 0;
  if (C == 3 && subsampling != 0 && subsampling != 2) return 0;
  if ((double)n_images * H * W * C >= 2147483648.0) return 0;
  const size_t luma = (size_t)H * W;
  if (C == 1) return luma;
  return subsampling == 2 ? luma + 2 * (size_t)((H + 1) / 2) * ((W + 1) / 2) : 3 * luma;
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

int sr3_noise_ex_u8(const uint8_t* in_hwc, int n_images, int H, int W, int C, const int32_t* mode, const float* strength, const float* z,
                    const int32_t* r, const int32_t* table, int kmax, uint8_t* out_hwc, void* stream) {
  if (!in_hwc) { set_error("noise_ex_u8: in_hwc is NULL"); return SR3_E_BADARG; }
  if (!mode) { set_error("noise_ex_u8: mode is NULL"); return SR3_E_BADARG; }
  if (!strength) { set_error("noise_ex_u8: strength is NULL"); return SR3_E_BADARG; }
  if (!out_hwc) { set_error("noise_ex_u8: out_hwc is NULL"); return SR3_E_BADARG; }
  if (n_images <= 0 || n_images > 65535) { set_error("noise_ex_u8: n_images %d outside 1..65535", n_images); return SR3_E_BADARG; }
  if (H <= 0) { set_error("noise_ex_u8: H %d is not positive", H); return SR3_E_BADARG; }
  if (W <= 0) { set_error("noise_ex_u8: W %d is not positive", W); return SR3_E_BADARG; }
  if (C != 1 && C != 3) { set_error("noise_ex_u8: C %d is not 1 or 3", C); return SR3_E_BADARG; }
  if ((double)n_images * H * W * C >= 2147483648.0) {
    set_error("noise_ex_u8: %d images of %d x %d x %d are 2^31 bytes or more", n_images, H, W, C);
    return SR3_E_BADARG;
  }
  if (table && (kmax < 1 || kmax > 1024)) { set_error("noise_ex_u8: kmax %d outside 1..1024 (the table's columns)", kmax); return SR3_E_BADARG; }
  const size_t bytes = (size_t)n_images * H * W * C;
  if (in_hwc != out_hwc && overlaps(in_hwc, bytes, out_hwc, bytes)) {
    set_error("noise_ex_u8: out_hwc overlaps in_hwc partially (in place means out_hwc == in_hwc)");
    return SR3_E_BADARG;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int HW = H * W;
  const dim3 grid((unsigned)(((size_t)HW + 255) / 256), n_images);
  if (C == 3) hipLaunchKernelGGL(k_noise_ex_u8<3>, grid, dim3(256), 0, st, in_hwc, HW, mode, strength, z, r, table, kmax, out_hwc);
  else hipLaunchKernelGGL(k_noise_ex_u8<1>, grid, dim3(256), 0, st, in_hwc, HW, mode, strength, z, r, table, kmax, out_hwc);
  SR3_LAUNCH_CHECK("k_noise_ex_u8");
  return SR3_OK;
}

size_t sr3_jpeg_scratch_bytes(int n_images, int H, int W, int C, int subsampling) {
  return (size_t)(n_images > 0 ? n_images : 0) * jpeg_scratch_per_image(n_images, H, W, C, subsampling);
}

int sr3_jpeg_u8(const uint8_t* in_hwc, int n_images, int H, int W, int C, const int32_t* quality, int subsampling, uint8_t* out_hwc,
                void* scratch, size_t scratch_bytes, void* stream) {
  if (!in_hwc) { set_error("jpeg_u8: in_hwc is NULL"); return SR3_E_BADARG; }
  if (!quality) { set_error("jpeg_u8: quality is NULL"); return SR3_E_BADARG; }
  if (!out_hwc) { set_error("jpeg_u8: out_hwc is NULL"); return SR3_E_BADARG; }
  if (!scratch) { set_error("jpeg_u8: scratch is NULL"); return SR3_E_BADARG; }
  if (n_images <= 0 || n_images > 65535) { set_error("jpeg_u8: n_images %d outside 1..65535", n_images); return SR3_E_BADARG; }
  if (H <= 0) { set_error("jpeg_u8: H %d is not positive", H); return SR3_E_BADARG; }
  if (W <= 0) { set_error("jpeg_u8: W %d is not positive", W); return SR3_E_BADARG; }
  if (C != 1 && C != 3) { set_error("jpeg_u8: C %d is not 1 or 3", C); return SR3_E_BADARG; }
  if (C == 3 && subsampling != 0 && subsampling != 2) {
    set_error("jpeg_u8: subsampling %d is not 0 (4:4:4) or 2 (4:2:0)", subsampling);
    return SR3_E_BADARG;
  }
  const size_t per = jpeg_scratch_per_image(n_images, H, W, C, subsampling);
  if (per == 0) { set_error("jpeg_u8: %d images of %d x %d x %d are 2^31 bytes or more", n_images, H, W, C); return SR3_E_BADARG; }
  const size_t need = per * n_images, bytes = (size_t)n_images * H * W * C;
  if (scratch_bytes < need) { set_error("jpeg_u8: scratch_bytes %zu is below the %zu sr3_jpeg_scratch_bytes asks for", scratch_bytes, need); return SR3_E_BADARG; }
  if (in_hwc != out_hwc && overlaps(in_hwc, bytes, out_hwc, bytes)) { set_error("jpeg_u8: out_hwc overlaps in_hwc partially (in place means out_hwc == in_hwc)"); return SR3_E_BADARG; }
  if (overlaps(scratch, need, in_hwc, bytes) || overlaps(scratch, need, out_hwc, bytes)) { set_error("jpeg_u8: scratch overlaps in_hwc or out_hwc"); return SR3_E_BADARG; }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool sub = C == 3 && subsampling == 2;
  const int ph = sub ? (H + 1) / 2 : H, pw = sub ? (W + 1) / 2 : W;
  const int blocks = ((H + 7) / 8) * ((W + 7) / 8) + (C == 3 ? 2 * ((ph + 7) / 8) * ((pw + 7) / 8) : 0);
  const dim3 ga((blocks + JPEG_BLOCKS - 1) / JPEG_BLOCKS, n_images), gb((unsigned)(((size_t)H * W + 255) / 256), n_images);
  unsigned char* sc = static_cast<unsigned char*>(scratch);
  if (C == 1) {
    hipLaunchKernelGGL((k_jpeg_codec<1, false>), ga, dim3(JPEG_NT), 0, st, in_hwc, H, W, quality, sc, per);
    SR3_LAUNCH_CHECK("k_jpeg_codec");
    hipLaunchKernelGGL((k_jpeg_finish<1, false>), gb, dim3(256), 0, st, in_hwc, H, W, quality, sc, per, out_hwc);
  } else if (sub) {
    hipLaunchKernelGGL((k_jpeg_codec<3, true>), ga, dim3(JPEG_NT), 0, st, in_hwc, H, W, quality, sc, per);
    SR3_LAUNCH_CHECK("k_jpeg_codec");
    hipLaunchKernelGGL((k_jpeg_finish<3, true>), gb, dim3(256), 0, st, in_hwc, H, W, quality, sc, per, out_hwc);
  } else {
    hipLaunchKernelGGL((k_jpeg_codec<3, false>), ga, dim3(JPEG_NT), 0, st, in_hwc, H, W, quality, sc, per);
    SR3_LAUNCH_CHECK("k_jpeg_codec");
    hipLaunchKernelGGL((k_jpeg_finish<3, false>), gb, dim3(256), 0, st, in_hwc, H, W, quality, sc, per, out_hwc);
  }
  SR3_LAUNCH_CHECK("k_jpeg_finish");
  return SR3_OK;
}

}  // extern "C"
