// vn_resize.hip — scene-cache frame resize for gfx950: the reference's
// skimage.transform.resize(frame, image_size, anti_aliasing=True) on uint8 frames, stored as
// round(255 x) bytes (DESIGN.md "Scene ingest: resize on the device").
//
// Three stages per output byte, each in the reference's own arithmetic:
//   1. Gaussian along the rows axis on the uint8 input, fp64, scipy's symmetric order
//      acc = x[i] w[R]; acc += (x[i+j] + x[i-j]) w[j+R] for j = -R..-1, products and sums
//      rounded separately (contraction is off for this file), floor to a byte;
//   2. the same along the columns axis on those bytes, floor to a byte;
//   3. bilinear sampling of those bytes in integers, S / D rounded to nearest, ties to even.
// Borders mirror without repeating the edge sample, with period 2 (n - 1).
//
// One 256-thread workgroup resizes a band of output rows of one frame. Only the filtered rows
// r0 / r1 of an output row are ever sampled, so stage 1 produces exactly those two rows per
// output row, over all input columns, into LDS (each pass is pointwise in the other axis).
// Stage 2 runs from LDS only at the columns c0 / c1 an output byte samples, and stage 3
// follows in registers: nothing but the input is read from and the output written to HBM.
// The taps travel in the kernel arguments (at most 2 x 33 doubles), so a call allocates and
// copies nothing.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "vn_common.h"

#pragma clang fp contract(off)

namespace vn {

constexpr int kRzThreads = 256;
constexpr int kRzMaxRadius = VN_RESIZE_MAX_RADIUS;
constexpr int kRzMaxRowBytes = VN_RESIZE_MAX_ROW_BYTES;
constexpr int kRzLdsBytes = 2 * kRzMaxRowBytes;  // 48 KB: one output row's r0 / r1 at the widest
constexpr int kRzMaxBand = 16;                   // output rows per workgroup

struct ResizeArgs {
  const uint8_t* src;
  uint8_t* dst;
  int h, w, c, oh, ow;
  int rr, rc;        // radii
  int band, bands;   // output rows per workgroup, workgroups per frame
  int stride;        // LDS bytes per filtered row
  double tr[kRzMaxRadius + 1];  // w[j + R] for j = -R..0, rows axis
  double tc[kRzMaxRadius + 1];  // columns axis
};

// Mirror without repeating the edge: index i of an axis of n samples, any number of reflections.
__device__ __forceinline__ int rz_mirror(int i, int n) {
  if ((unsigned)i < (unsigned)n) return i;
  if (n == 1) return 0;
  const int p = 2 * (n - 1);
  int m = i % p;
  if (m < 0) m += p;
  return m < n ? m : p - m;
}

__global__ __launch_bounds__(kRzThreads) void resize_kernel(ResizeArgs a) {
  extern __shared__ uint8_t rz_rows[];  // [2 * band][stride]: rows r0, r1 of each output row
  const int f = blockIdx.x / a.bands, b = blockIdx.x - f * a.bands;
  const int i0 = b * a.band, nb = min(a.band, a.oh - i0);
  const int wc = a.w * a.c;
  const uint8_t* src = a.src + (int64_t)f * a.h * wc;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t dr = 2 * (int64_t)a.oh, dc = 2 * (int64_t)a.ow;

  // stage 1: one wave per filtered row, lanes along the row's bytes
  for (int slot = wave; slot < 2 * nb; slot += kRzThreads / 64) {
    const int64_t num = (2 * (int64_t)(i0 + (slot >> 1)) + 1) * a.h - a.oh;
    const int r0 = (int)(num / dr);
    const int r = (slot & 1) ? min(r0 + (num - r0 * dr > 0 ? 1 : 0), a.h - 1) : r0;
    uint8_t* out = rz_rows + slot * a.stride;
    const uint8_t* mid = src + (int64_t)r * wc;
    for (int x = lane; x < wc; x += 64) {
      double acc = (double)mid[x] * a.tr[a.rr];
      for (int j = -a.rr; j < 0; ++j) {
        const double lo = (double)src[(int64_t)rz_mirror(r + j, a.h) * wc + x];
        const double hi = (double)src[(int64_t)rz_mirror(r - j, a.h) * wc + x];
        acc = acc + (lo + hi) * a.tr[j + a.rr];
      }
      out[x] = (uint8_t)(int)acc;  // acc >= 0: truncation is floor
    }
  }
  __syncthreads();

  // stages 2 and 3: one thread per output byte of the band
  const int owc = a.ow * a.c;
  uint8_t* dst = a.dst + ((int64_t)f * a.oh + i0) * owc;
  for (int t = threadIdx.x; t < nb * owc; t += kRzThreads) {
    const int il = t / owc, rem = t - il * owc;
    const int j = rem / a.c, ch = rem - j * a.c;
    const int64_t num_r = (2 * (int64_t)(i0 + il) + 1) * a.h - a.oh;
    const int64_t nr = num_r % dr;
    const int64_t num_c = (2 * (int64_t)j + 1) * a.w - a.ow;
    const int c0 = (int)(num_c / dc);
    const int64_t nc = num_c - c0 * dc;
    const int c1 = min(c0 + (nc > 0 ? 1 : 0), a.w - 1);
    const uint8_t* v0 = rz_rows + (2 * il) * a.stride + ch;
    const uint8_t* v1 = v0 + a.stride;
    double g[2][2];  // [row r0 / r1][column c0 / c1]
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int cc = k ? c1 : c0;
      double acc0 = (double)v0[cc * a.c] * a.tc[a.rc];
      double acc1 = (double)v1[cc * a.c] * a.tc[a.rc];
      for (int q = -a.rc; q < 0; ++q) {
        const int lo = rz_mirror(cc + q, a.w) * a.c, hi = rz_mirror(cc - q, a.w) * a.c;
        const double wq = a.tc[q + a.rc];
        acc0 = acc0 + ((double)v0[lo] + (double)v0[hi]) * wq;
        acc1 = acc1 + ((double)v1[lo] + (double)v1[hi]) * wq;
      }
      g[0][k] = (double)(int)acc0;
      g[1][k] = (double)(int)acc1;
    }
    const int64_t s = (dc - nc) * (dr - nr) * (int64_t)g[0][0] + nc * (dr - nr) * (int64_t)g[0][1] +
                      (dc - nc) * nr * (int64_t)g[1][0] + nc * nr * (int64_t)g[1][1];
    const int64_t d = dr * dc;
    int64_t qv = s / d;
    const int64_t twice = 2 * (s - qv * d);
    if (twice > d || (twice == d && (qv & 1))) ++qv;
    dst[t] = (uint8_t)qv;
  }
}

}  // namespace vn

using namespace vn;

extern "C" int vn_resize_frames(const uint8_t* src_dev, int64_t n, int h, int w, int c, int oh, int ow,
                                const double* taps_rows_host, int radius_rows, const double* taps_cols_host,
                                int radius_cols, uint8_t* dst_dev, vn_stream_t stream) {
  if (!src_dev || !dst_dev) return fail(VN_EINVAL, "vn_resize_frames: NULL frames");
  if (n <= 0 || h <= 0 || w <= 0 || oh <= 0 || ow <= 0)
    return fail(VN_EINVAL, "vn_resize_frames: sizes must be positive");
  if (c != 1 && c != 3) return fail(VN_EINVAL, "vn_resize_frames: channels must be 1 or 3");
  if (oh > h || ow > w) return fail(VN_EINVAL, "vn_resize_frames: upsampling is not supported (oh <= h, ow <= w)");
  if (radius_rows < 0 || radius_cols < 0 || radius_rows > kRzMaxRadius || radius_cols > kRzMaxRadius)
    return fail(VN_EINVAL, "vn_resize_frames: radius must lie in 0.." + std::to_string(kRzMaxRadius));
  if ((!taps_rows_host && radius_rows != 0) || (!taps_cols_host && radius_cols != 0))
    return fail(VN_EINVAL, "vn_resize_frames: a skipped axis (NULL taps) has radius 0");
  if ((int64_t)w * c > kRzMaxRowBytes)
    return fail(VN_EINVAL, "vn_resize_frames: rows of more than " + std::to_string(kRzMaxRowBytes) + " bytes");
  if (oh == h && ow == w) {
    VN_HIP(hipMemcpyAsync(dst_dev, src_dev, (size_t)n * h * w * c, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return VN_OK;
  }
  ResizeArgs a;
  a.h = h;
  a.w = w;
  a.c = c;
  a.oh = oh;
  a.ow = ow;
  a.rr = radius_rows;
  a.rc = radius_cols;
  // a skipped axis is the one tap 1.0: x * 1.0 floors to x, the pass changes nothing
  for (int k = 0; k <= kRzMaxRadius; ++k) {
    a.tr[k] = taps_rows_host ? (k <= radius_rows ? taps_rows_host[k] : 0.0) : 1.0;
    a.tc[k] = taps_cols_host ? (k <= radius_cols ? taps_cols_host[k] : 0.0) : 1.0;
  }
  a.stride = (w * c + 3) / 4 * 4;
  a.band = std::max(1, std::min({oh, kRzMaxBand, kRzLdsBytes / (2 * a.stride)}));
  a.bands = (oh + a.band - 1) / a.band;
  const size_t lds = (size_t)2 * a.band * a.stride;
  // whole frames per launch, within the grid's 2^31 - 1 workgroups
  const int64_t per_launch = std::max<int64_t>(1, (int64_t)0x40000000 / a.bands);
  for (int64_t f0 = 0; f0 < n; f0 += per_launch) {
    const int64_t nf = std::min(per_launch, n - f0);
    a.src = src_dev + f0 * h * w * c;
    a.dst = dst_dev + f0 * oh * ow * c;
    hipLaunchKernelGGL(resize_kernel, dim3((unsigned)(nf * a.bands)), dim3(kRzThreads), lds, (hipStream_t)stream, a);
    VN_HIP(hipGetLastError());
  }
  return VN_OK;
}
