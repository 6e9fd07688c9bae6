// The frame side of rendering whole views (the reference's evaluation/eval.py --eval_rendering and the trainer's do_vis pictures, which
// assemble chunks with torch.cat, quantise with numpy on the host, lay images out with torchvision's make_grid and average the squared
// error with a float32 torch.mean): chunk outputs -> byte frames, a depth plane and a squared-error plane; the error sum; the finite
// range of the depth plane and its grey picture; the make_grid canvas.  Pure streams: one element per lane, consecutive lanes on
// consecutive bytes / floats.  No float atomics; every result is the same bytes on every run.
//
// Definitions (tests/render_f64.py restates them in numpy).  All arithmetic is IEEE float32, one rounding per step:
//   byte(x)     t = 255 * x;  0 if t is NaN or t <= 0;  255 if t >= 255;  else trunc(t)
//   rgb8        byte(rgb)
//   normal8     byte((n + 1) / 2)
//   err         d = rgb - gt;  e = d * d
//   sum         float64 sum of float32 values over a fixed 256-ary tree: the leaves are runs of 256 consecutive elements (the last one
//               padded with +0); a run is summed as lane t += lane t ^ 32, ^ 16, ... ^ 1 within each 64 and then ((w0 + w1) + (w2 + w3));
//               the run sums are summed the same way, level by level, until one value is left
//   range       lo = min, hi = max over the finite values; (0, 0) if there is none
//   grey        0 if d is not finite or hi == lo; else byte-clamp of trunc(((255 * (d - lo)) / (hi - lo)))
//   grid        torchvision.utils.make_grid(nrow, padding = 2, pad_value = 0): xmaps = min(nrow, N), ymaps = ceil(N / xmaps), image k at row
//               (k / xmaps)(H + 2) + 2, column (k % xmaps)(W + 2) + 2 of a (ymaps (H + 2) + 2) x (xmaps (W + 2) + 2) canvas; N = 1 is a copy
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "block_util.hpp"      // block_sum, block_minmax
#include "device_util.hpp"     // rounded

namespace neat {

constexpr int FRAME_WG = 256;
constexpr int FRAME_RANGE_BLOCKS = 1024;                         // partial (min, max) pairs of the range pass

__device__ __forceinline__ unsigned char frame_byte(float x) {
#pragma clang fp contract(off)
  const float t = rounded(255.0f * x);
  if (!(t > 0.0f)) return 0;                                     // NaN, zero, negatives, -inf
  if (t >= 255.0f) return 255;                                   // +inf too
  return (unsigned char)(int)t;                                  // 0 < t < 255: the conversion truncates
}

// ---- (a) one chunk into the frame ---------------------------------------------------------------------------------------------------------
// element e of [0, 3n): channel e % 3 of chunk pixel e / 3 = frame element 3 p0 + e.  Lanes e < n also carry the depth of pixel p0 + e.
__global__ __launch_bounds__(FRAME_WG) void frame_put_kernel(const float* __restrict__ rgb, const float* __restrict__ normal,
                                                             const float* __restrict__ depth, const float* __restrict__ gt, int n, long long p0,
                                                             unsigned char* __restrict__ rgb8, unsigned char* __restrict__ normal8,
                                                             float* __restrict__ depth_out, float* __restrict__ err) {
#pragma clang fp contract(off)
  const long long e = (long long)blockIdx.x * FRAME_WG + threadIdx.x;
  if (e >= 3ll * n) return;
  const long long q = 3 * p0 + e;
  if (rgb) {
    const float x = rgb[e];
    if (rgb8) rgb8[q] = frame_byte(x);
    if (gt) {
      const float d = rounded(x - gt[q]);
      err[q] = d * d;
    }
  }
  if (normal) {
    const float h = rounded(normal[e] + 1.0f);
    normal8[q] = frame_byte(rounded(h / 2.0f));
  }
  if (depth && e < n) depth_out[p0 + e] = depth[e];
}

// ---- (b) the error sum --------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(FRAME_WG) void frame_sum_kernel(const T* __restrict__ x, long long n, double* __restrict__ out) {
  __shared__ double sh[FRAME_WG / 64];
  const long long i = (long long)blockIdx.x * FRAME_WG + threadIdx.x;
  const double s = block_sum<FRAME_WG>(i < n ? (double)x[i] : 0.0, sh);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// ---- (c) the finite range of a plane and its grey picture -----------------------------------------------------------------------------------
// partial[2 b], partial[2 b + 1] = (min, max) over the finite values block b strides over; (+inf, -inf) if it met none
__global__ __launch_bounds__(FRAME_WG) void frame_range_partial_kernel(const float* __restrict__ x, long long n, float* __restrict__ partial) {
  __shared__ float sh[8];
  float lo[1] = {INFINITY}, hi[1] = {-INFINITY};
  for (long long i = (long long)blockIdx.x * FRAME_WG + threadIdx.x; i < n; i += (long long)gridDim.x * FRAME_WG) {
    const float v = x[i];
    if (isfinite(v)) { lo[0] = fminf(lo[0], v); hi[0] = fmaxf(hi[0], v); }
  }
  block_minmax<FRAME_WG>(lo, hi, sh);
  if (threadIdx.x == 0) { partial[2 * blockIdx.x] = lo[0]; partial[2 * blockIdx.x + 1] = hi[0]; }
}
__global__ __launch_bounds__(FRAME_WG) void frame_range_finish_kernel(const float* __restrict__ partial, int blocks, float* __restrict__ out) {
  __shared__ float sh[8];
  float lo[1] = {INFINITY}, hi[1] = {-INFINITY};
  for (int b = threadIdx.x; b < blocks; b += FRAME_WG) { lo[0] = fminf(lo[0], partial[2 * b]); hi[0] = fmaxf(hi[0], partial[2 * b + 1]); }
  block_minmax<FRAME_WG>(lo, hi, sh);
  if (threadIdx.x == 0) {
    const bool any = lo[0] <= hi[0];
    out[0] = any ? lo[0] : 0.0f;
    out[1] = any ? hi[0] : 0.0f;
  }
}
__global__ __launch_bounds__(FRAME_WG) void frame_grey_kernel(const float* __restrict__ x, long long n, const float* __restrict__ range,
                                                              unsigned char* __restrict__ out) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * FRAME_WG + threadIdx.x;
  if (i >= n) return;
  const float lo = range[0], hi = range[1], d = x[i];
  unsigned char b = 0;
  if (isfinite(d) && hi != lo) {
    const float t = rounded(rounded(255.0f * rounded(d - lo)) / rounded(hi - lo));
    b = !(t > 0.0f) ? 0 : (t >= 255.0f ? 255 : (unsigned char)(int)t);
  }
  out[i] = b;
}

// ---- (d) the make_grid canvas ---------------------------------------------------------------------------------------------------------------
// one lane per canvas byte; total = the canvas bytes, cw3 = the bytes of a canvas row, pad = 2 (0 for a single image)
__global__ __launch_bounds__(FRAME_WG) void frame_grid_kernel(const unsigned char* __restrict__ images, int N, int H, int W, int xmaps, int pad,
                                                              long long total, int cw3, unsigned char* __restrict__ canvas) {
  const long long i = (long long)blockIdx.x * FRAME_WG + threadIdx.x;
  if (i >= total) return;
  const int r = (int)(i / cw3), c3 = (int)(i % cw3);
  const int c = c3 / 3, ch = c3 % 3;
  unsigned char v = 0;
  if (r >= pad && c >= pad) {
    const int cy = (r - pad) / (H + pad), y = (r - pad) % (H + pad);
    const int cx = (c - pad) / (W + pad), x = (c - pad) % (W + pad);
    const long long k = (long long)cy * xmaps + cx;
    if (y < H && x < W && cx < xmaps && k < N) v = images[((k * H + y) * W + x) * 3 + ch];
  }
  canvas[i] = v;
}

}  // namespace neat
