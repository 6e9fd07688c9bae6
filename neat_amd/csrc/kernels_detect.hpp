// 2-D line-segment detection in the views (neat_amd/detect.py; the rule: DESIGN 3j, restated in float64 by tests/detect_f64.py).  An
// a-contrario detector of the LSD family over the line-support regions of Burns, Hanson and Riseman: 8-connected components of the
// quantised gradient orientation in two overlapping partitions of the circle.  Nothing depends on an order of visits: labels are the
// smallest pixel index of a component, sizes and votes are integer atomics, every float64 sum over a region runs in ascending pixel
// index on all lanes of one wavefront, and the lists are compacted in order.  Float64 throughout, with contraction into fused
// multiply-adds switched off in every function that forms a value the reference forms (the products and sums are the reference's, one
// IEEE operation each), so the decisions are the reference's and two runs give the same bytes.  The only transcendental functions are
// those of the NFA (lgamma, exp, log).
//
// Maps: a labelling problem is `maps` pictures of h x w codes (0..7, 255 = unused).  The detector's maps are (view, partition), view-major,
// so that ascending element index e = (2 v + p) h w + i is the output order (view, partition, label).
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stddef.h>

#include "block_util.hpp"           // block_sum, block_exscan, block_carry_scan, block_compact
#include "device_util.hpp"
#include "graph_util.hpp"           // uf_find, uf_union

namespace neat {

constexpr int DET_TILE = 16;                     // a workgroup labels a 16 x 16 tile in LDS, one thread a pixel
constexpr int DET_WG = DET_TILE * DET_TILE;
constexpr int DET_WAVES = DET_WG / 64;           // region kernel: one wavefront per candidate
constexpr unsigned char DET_UNUSED = 255;

struct DetectConsts { double cos_tau, density, logNT, p; };      // what the region kernel tests with

__device__ __forceinline__ double detect_grey_at(const unsigned char* __restrict__ img, int ch, size_t pix) {
  if (ch == 1) return (double)img[pix];
  const unsigned char* p = img + 3 * pix;
  return (double)((77 * (int)p[0] + 150 * (int)p[1] + 29 * (int)p[2] + 128) >> 8);
}

// ---- grey, and for scale < 1 the sampled Gaussian: taps_x [Ws][ntaps], taps_y [Hs][ntaps] (normalised, from the host), the first tap of
// output position i at source floor(i / scale + 0.5) - (ntaps - 1) / 2, source indices clamped to the image.  Rows first, then columns,
// each acc = acc + tap * value in tap order from 0.  ntaps = 0: scale 1.
__global__ __launch_bounds__(DET_WG) void detect_grey_kernel(const unsigned char* __restrict__ img, int V, int H, int W, int ch, double scale,
                                                             const double* __restrict__ taps_x, const double* __restrict__ taps_y, int ntaps,
                                                             int Hs, int Ws, double* __restrict__ grey) {
#pragma clang fp contract(off)
  const size_t idx = (size_t)blockIdx.x * DET_WG + threadIdx.x;
  if (idx >= (size_t)V * Hs * Ws) return;
  const int x = (int)(idx % Ws), y = (int)((idx / Ws) % Hs);
  const size_t v = idx / ((size_t)Ws * Hs);
  const unsigned char* base = img + v * (size_t)H * W * ch;
  if (ntaps == 0) { grey[idx] = detect_grey_at(base, ch, (size_t)y * W + x); return; }
  const int hh = (ntaps - 1) / 2;
  const int fx = (int)floor((double)x / scale + 0.5) - hh, fy = (int)floor((double)y / scale + 0.5) - hh;
  double out = 0.0;
  for (int ty = 0; ty < ntaps; ++ty) {
    const int sy = min(max(fy + ty, 0), H - 1);
    double row = 0.0;
    for (int tx = 0; tx < ntaps; ++tx) {
      const int sx = min(max(fx + tx, 0), W - 1);
      row = row + taps_x[(size_t)x * ntaps + tx] * detect_grey_at(base, ch, (size_t)sy * W + sx);
    }
    out = out + taps_y[(size_t)y * ntaps + ty] * row;
  }
  grey[idx] = out;
}

// ---- gradient on the (Hs - 1) x (Ws - 1) grid of 2 x 2 blocks a b / c d, and the two orientation codes of a used position
__global__ __launch_bounds__(DET_WG) void detect_gradient_kernel(const double* __restrict__ grey, int V, int Hs, int Ws, double rho2, double c1,
                                                                 double* __restrict__ gx_out, double* __restrict__ gy_out,
                                                                 unsigned char* __restrict__ code) {
#pragma clang fp contract(off)
  const int h = Hs - 1, w = Ws - 1;
  const size_t hw = (size_t)h * w, idx = (size_t)blockIdx.x * DET_WG + threadIdx.x;
  if (idx >= (size_t)V * hw) return;
  const size_t v = idx / hw, i = idx % hw;
  const int x = (int)(i % w), y = (int)(i / w);
  const double* g = grey + v * (size_t)Hs * Ws + (size_t)y * Ws + x;
  const double a = g[0], b = g[1], c = g[Ws], d = g[Ws + 1];
  const double gx = ((b + d) - (a + c)) * 0.5, gy = ((c + d) - (a + b)) * 0.5;
  const double m2 = gx * gx + gy * gy;
  gx_out[idx] = gx;
  gy_out[idx] = gy;
  unsigned char c0 = DET_UNUSED, c1o = DET_UNUSED;
  if (m2 >= rho2) {
    const double ax = fabs(gx), ay = fabs(gy);
    const bool sx = gx < 0.0, sy = gy < 0.0;
    c0 = (unsigned char)((sy ? 4 : 0) + (sx ? 2 : 0) + (ay > ax ? 1 : 0));
    const bool not_h = ay > c1 * ax, not_v = ax > c1 * ay;
    if (!not_h) c1o = sx ? 4 : 0;
    else if (!not_v) c1o = sy ? 6 : 2;
    else c1o = sx ? (sy ? 5 : 3) : (sy ? 7 : 1);
  }
  code[(2 * v) * hw + i] = c0;
  code[(2 * v + 1) * hw + i] = c1o;
}

// ---- connected components: uf_union of graph_util.hpp, at workgroup scope in a tile's LDS and at agent scope along the tile borders
__device__ __forceinline__ int detect_tiles(int n) { return (n + DET_TILE - 1) / DET_TILE; }

// one workgroup per (map, tile): the tile's components in LDS, then label = the root's index in the map (-1: unused).  With `size`,
// the per-region accumulators of the detector are reset here too.
__global__ __launch_bounds__(DET_WG) void detect_label_tile_kernel(const unsigned char* __restrict__ code, int h, int w, int* __restrict__ label,
                                                                   int* __restrict__ size, int* __restrict__ votes, int* __restrict__ xmin,
                                                                   int* __restrict__ xmax, int* __restrict__ ymax) {
  __shared__ int s_lab[DET_WG];
  __shared__ unsigned char s_code[DET_WG];
  const int tnx = detect_tiles(w), tiles = tnx * detect_tiles(h);
  const int m = blockIdx.x / tiles, t = blockIdx.x % tiles;
  const int x0 = (t % tnx) * DET_TILE, y0 = (t / tnx) * DET_TILE;
  const int tid = threadIdx.x, lx = tid & (DET_TILE - 1), ly = tid / DET_TILE;
  const int x = x0 + lx, y = y0 + ly;
  const bool in = x < w && y < h;
  const size_t e = (size_t)m * h * w + (size_t)y * w + x;
  const unsigned char c = in ? code[e] : DET_UNUSED;
  s_code[tid] = c;
  s_lab[tid] = c != DET_UNUSED ? tid : -1;
  __syncthreads();
  if (c != DET_UNUSED) {          // the four neighbours before this pixel in raster order: every 8-adjacent pair is seen once
    if (lx > 0 && s_code[tid - 1] == c) uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(s_lab, tid, tid - 1);
    if (ly > 0) {
      if (lx > 0 && s_code[tid - DET_TILE - 1] == c) uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(s_lab, tid, tid - DET_TILE - 1);
      if (s_code[tid - DET_TILE] == c) uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(s_lab, tid, tid - DET_TILE);
      if (lx < DET_TILE - 1 && s_code[tid - DET_TILE + 1] == c) uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(s_lab, tid, tid - DET_TILE + 1);
    }
  }
  __syncthreads();
  if (!in) return;
  int r = -1;
  if (c != DET_UNUSED) {
    const int lr = uf_find<__HIP_MEMORY_SCOPE_WORKGROUP>(s_lab, tid);
    r = (y0 + lr / DET_TILE) * w + x0 + (lr & (DET_TILE - 1));
  }
  label[e] = r;
  if (size) { size[e] = 0; votes[e] = 0; xmin[e] = INT_MAX; xmax[e] = -1; ymax[e] = -1; }
}

// one thread per element: a pixel joins those of its four earlier neighbours that lie in another tile
__global__ __launch_bounds__(DET_WG) void detect_label_merge_kernel(const unsigned char* __restrict__ code, int maps, int h, int w,
                                                                    int* __restrict__ label) {
  const size_t hw = (size_t)h * w, idx = (size_t)blockIdx.x * DET_WG + threadIdx.x;
  if (idx >= (size_t)maps * hw) return;
  const size_t m = idx / hw;
  const int i = (int)(idx % hw), x = i % w, y = i / w;
  const bool left = (x & (DET_TILE - 1)) == 0, top = (y & (DET_TILE - 1)) == 0, right = (x & (DET_TILE - 1)) == DET_TILE - 1;
  if (!left && !top && !right) return;
  const unsigned char* cm = code + m * hw;
  const unsigned char c = cm[i];
  if (c == DET_UNUSED) return;
  int* L = label + m * hw;
  if (left && x > 0 && cm[i - 1] == c) uf_union<__HIP_MEMORY_SCOPE_AGENT>(L, i, i - 1);
  if (y > 0) {
    if ((left || top) && x > 0 && cm[i - w - 1] == c) uf_union<__HIP_MEMORY_SCOPE_AGENT>(L, i, i - w - 1);
    if (top && cm[i - w] == c) uf_union<__HIP_MEMORY_SCOPE_AGENT>(L, i, i - w);
    if ((top || right) && x + 1 < w && cm[i - w + 1] == c) uf_union<__HIP_MEMORY_SCOPE_AGENT>(L, i, i - w + 1);
  }
}

// path compression: label = the root.  With `size` also the region's pixel count and bounding box (integer atomics; ymin is the root's row)
__global__ __launch_bounds__(DET_WG) void detect_label_flatten_kernel(int maps, int h, int w, int* __restrict__ label, int* __restrict__ size,
                                                                      int* __restrict__ xmin, int* __restrict__ xmax, int* __restrict__ ymax) {
  const size_t hw = (size_t)h * w, idx = (size_t)blockIdx.x * DET_WG + threadIdx.x;
  if (idx >= (size_t)maps * hw) return;
  const size_t m = idx / hw;
  const int i = (int)(idx % hw);
  int* L = label + m * hw;
  if (__hip_atomic_load(L + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 0) return;
  const int r = uf_find<__HIP_MEMORY_SCOPE_AGENT>(L, i);
  __hip_atomic_store(L + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (size) {
    const size_t er = m * hw + r;
    atomicAdd(size + er, 1);
    atomicMin(xmin + er, i % w);
    atomicMax(xmax + er, i % w);
    atomicMax(ymax + er, i / w);
  }
}

// ---- a used pixel votes for the partition in which its region is the larger (partition 0 on a tie)
__global__ __launch_bounds__(DET_WG) void detect_vote_kernel(int V, int hw, const int* __restrict__ label, const int* __restrict__ size,
                                                             int* __restrict__ votes) {
  const size_t idx = (size_t)blockIdx.x * DET_WG + threadIdx.x;
  if (idx >= (size_t)V * hw) return;
  const size_t v = idx / hw, i = idx % hw, e0 = 2 * v * hw, e1 = e0 + hw;
  const int l0 = label[e0 + i];
  if (l0 < 0) return;
  const int l1 = label[e1 + i];
  if (size[e0 + l0] >= size[e1 + l1]) atomicAdd(votes + e0 + l0, 1);
  else atomicAdd(votes + e1 + l1, 1);
}

__device__ __forceinline__ bool detect_is_candidate(const int* __restrict__ label, const int* __restrict__ size, const int* __restrict__ votes,
                                                    size_t e, int hw, int min_reg) {
  return label[e] == (int)(e % hw) && size[e] >= min_reg && 2 * votes[e] >= size[e];
}

// ---- the candidate regions in element order: counts per workgroup, their offsets (one workgroup), then the list
__global__ __launch_bounds__(DET_WG) void detect_cand_count_kernel(long long el2, int hw, int min_reg, const int* __restrict__ label,
                                                                   const int* __restrict__ size, const int* __restrict__ votes,
                                                                   int* __restrict__ bcnt) {
  __shared__ int sh[DET_WAVES];
  const size_t e = (size_t)blockIdx.x * DET_WG + threadIdx.x;
  const int f = e < (size_t)el2 && detect_is_candidate(label, size, votes, e, hw, min_reg) ? 1 : 0;
  const int s = block_sum<DET_WG>(f, sh);
  if (threadIdx.x == 0) bcnt[blockIdx.x] = s;
}

__global__ __launch_bounds__(1024) void detect_cand_scan_kernel(int blocks, const int* __restrict__ bcnt, int* __restrict__ boff, int cap,
                                                                int* __restrict__ counters) {
  __shared__ int s_wave[16];
  const long long total = block_carry_scan(blocks, [&](int b) { return bcnt[b]; }, [&](int b, long long e) { boff[b] = (int)e; }, s_wave);
  if (threadIdx.x == 0) { counters[0] = (int)(total < cap ? total : cap); counters[1] = 0; }
}

__global__ __launch_bounds__(DET_WG) void detect_cand_emit_kernel(long long el2, int hw, int min_reg, const int* __restrict__ label,
                                                                  const int* __restrict__ size, const int* __restrict__ votes,
                                                                  const int* __restrict__ boff, int cap, int* __restrict__ cand) {
  __shared__ int s_wave[DET_WAVES];
  const size_t e = (size_t)blockIdx.x * DET_WG + threadIdx.x;
  const int f = e < (size_t)el2 && detect_is_candidate(label, size, votes, e, hw, min_reg) ? 1 : 0;
  int total;
  const int at = boff[blockIdx.x] + block_exscan(f, s_wave, &total);
  if (f && at < cap) cand[at] = (int)e;
}

// ---- one wavefront per candidate.  walk(): the region's pixels in ascending index, found in its bounding box 64 positions at a time;
// every lane runs f on every pixel, so the sums are the sequential ones and all lanes hold them.
template <class F>
__device__ __forceinline__ void detect_walk(const int* __restrict__ lab, const double* __restrict__ gx, const double* __restrict__ gy, int w,
                                            int root, int bx0, int bx1, int by0, int by1, F f) {
  const int lane = threadIdx.x & 63, bw = bx1 - bx0 + 1, area = bw * (by1 - by0 + 1);
  for (int p0 = 0; p0 < area; p0 += 64) {
    const int pos = p0 + lane;
    int x = 0, y = 0;
    double vx = 0.0, vy = 0.0;
    bool mine = false;
    if (pos < area) {
      x = bx0 + pos % bw; y = by0 + pos / bw;
      const int i = y * w + x;
      mine = lab[i] == root;
      if (mine) { vx = gx[i]; vy = gy[i]; }
    }
    unsigned long long bal = __ballot(mine);
    while (bal) {
      const int src = __ffsll((long long)bal) - 1;
      bal &= bal - 1;
      f(__shfl(x, src), __shfl(y, src), __shfl(vx, src), __shfl(vy, src));
    }
  }
}

__device__ __forceinline__ int detect_clamp_int(double v, int lo, int hi) { return (int)fmin(fmax(v, (double)lo), (double)hi); }

// rec [6] = x1 y1 x2 y2 width nfa; keep = the density and NFA tests passed
__global__ __launch_bounds__(DET_WG) void detect_region_kernel(const int* __restrict__ cand, const int* __restrict__ counters, int h, int w,
                                                               double scale, DetectConsts K, const unsigned char* __restrict__ code,
                                                               const int* __restrict__ label, const int* __restrict__ xmin,
                                                               const int* __restrict__ xmax, const int* __restrict__ ymax,
                                                               const double* __restrict__ gx_all, const double* __restrict__ gy_all,
                                                               double* __restrict__ rec, int* __restrict__ n_out, int* __restrict__ k_out,
                                                               int* __restrict__ keep) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, c = blockIdx.x * DET_WAVES + (threadIdx.x >> 6);
  if (c >= counters[0]) return;                  // whole wavefronts leave; the kernel has no barrier
  const int e = cand[c], hw = h * w, m = e / hw, root = e % hw;
  const int* lab = label + (size_t)m * hw;
  const unsigned char* cm = code + (size_t)m * hw;
  const double* gx = gx_all + (size_t)(m >> 1) * hw;
  const double* gy = gy_all + (size_t)(m >> 1) * hw;
  const int bx0 = xmin[e], bx1 = xmax[e], by0 = root / w, by1 = ymax[e];
  double sumw = 0.0, sx = 0.0, sy = 0.0;
  detect_walk(lab, gx, gy, w, root, bx0, bx1, by0, by1, [&](int x, int y, double vx, double vy) {
    const double wt = sqrt(vx * vx + vy * vy);
    sumw = sumw + wt; sx = sx + wt * (double)x; sy = sy + wt * (double)y;
  });
  const double cx = sx / sumw, cy = sy / sumw;
  double a = 0.0, b = 0.0, d = 0.0;
  detect_walk(lab, gx, gy, w, root, bx0, bx1, by0, by1, [&](int x, int y, double vx, double vy) {
    const double wt = sqrt(vx * vx + vy * vy), dx = (double)x - cx, dy = (double)y - cy;
    a = a + (wt * dy) * dy; b = b + (wt * dx) * dx; d = d + (wt * dx) * dy;
  });
  const double Ixx = a / sumw, Iyy = b / sumw, Ixy = -d / sumw, dI = Ixx - Iyy;
  const double lam = 0.5 * ((Ixx + Iyy) - sqrt(dI * dI + 4.0 * (Ixy * Ixy)));
  double ux = fabs(Ixx) > fabs(Iyy) ? Ixy : lam - Iyy, uy = fabs(Ixx) > fabs(Iyy) ? lam - Ixx : Ixy;
  const double nrm = sqrt(ux * ux + uy * uy);
  if (nrm > 0.0) { ux = ux / nrm; uy = uy / nrm; } else { ux = 1.0; uy = 0.0; }
  double l0 = INFINITY, l1 = -INFINITY, t0 = INFINITY, t1 = -INFINITY, S = 0.0;
  detect_walk(lab, gx, gy, w, root, bx0, bx1, by0, by1, [&](int x, int y, double vx, double vy) {
    const double dx = (double)x - cx, dy = (double)y - cy;
    const double l = dx * ux + dy * uy, t = dy * ux - dx * uy;
    l0 = fmin(l0, l); l1 = fmax(l1, l); t0 = fmin(t0, t); t1 = fmax(t1, t);
    S = S + (vy * ux - vx * uy);
  });
  const double s = S > 0.0 ? 1.0 : (S < 0.0 ? -1.0 : 0.0);
  const double wd = t1 - t0, pad = wd < 1.0 ? (1.0 - wd) * 0.5 : 0.0, t0p = t0 - pad, t1p = t1 + pad;
  // the rectangle's bounding box with a margin; any superset of the rectangle gives the same counts
  double pxl = INFINITY, pxh = -INFINITY, pyl = INFINITY, pyh = -INFINITY;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const double ll = (q & 2) ? l1 : l0, tt = (q & 1) ? t1p : t0p;
    const double px = cx + ll * ux - tt * uy, py = cy + ll * uy + tt * ux;
    pxl = fmin(pxl, px); pxh = fmax(pxh, px); pyl = fmin(pyl, py); pyh = fmax(pyh, py);
  }
  const int rx0 = detect_clamp_int(floor(pxl) - 1.0, 0, w - 1), rx1 = detect_clamp_int(ceil(pxh) + 1.0, 0, w - 1);
  const int ry0 = detect_clamp_int(floor(pyl) - 1.0, 0, h - 1), ry1 = detect_clamp_int(ceil(pyh) + 1.0, 0, h - 1);
  const int rw = rx1 - rx0 + 1, area = rw * (ry1 - ry0 + 1);
  int n = 0, k = 0;
  for (int p0 = 0; p0 < area; p0 += 64) {
    const int pos = p0 + lane;
    bool inside = false, aligned = false;
    if (pos < area) {
      const int x = rx0 + pos % rw, y = ry0 + pos / rw, i = y * w + x;
      const double dx = (double)x - cx, dy = (double)y - cy;
      const double l = dx * ux + dy * uy, t = dy * ux - dx * uy;
      inside = l >= l0 && l <= l1 && t >= t0p && t <= t1p;
      if (inside && cm[i] != DET_UNUSED) {
        const double vx = gx[i], vy = gy[i], gn = vy * ux - vx * uy;
        aligned = gn * s > 0.0 && fabs(gn) >= sqrt(vx * vx + vy * vy) * K.cos_tau;
      }
    }
    n += __popcll(__ballot(inside));
    k += __popcll(__ballot(aligned));
  }
  const bool dense = !((double)k < K.density * (double)n);
  double nfa = -INFINITY;
  if (dense) {          // -(logNT + log10 of the binomial tail sum_{i = k..n} C(n, i) p^i (1 - p)^(n - i)), a log-sum-exp over the lanes
    const double lp = log(K.p), lq = log(1.0 - K.p), lgn = lgamma((double)n + 1.0);
    double mx = -INFINITY;
    for (int i = k + lane; i <= n; i += 64)
      mx = fmax(mx, lgn - lgamma((double)i + 1.0) - lgamma((double)(n - i) + 1.0) + (double)i * lp + (double)(n - i) * lq);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off));
    double sum = 0.0;
    for (int i = k + lane; i <= n; i += 64)
      sum += exp(lgn - lgamma((double)i + 1.0) - lgamma((double)(n - i) + 1.0) + (double)i * lp + (double)(n - i) * lq - mx);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    nfa = -(K.logNT + (mx + log(sum)) / log(10.0));
  }
  if (lane == 0) {
    double* r = rec + 6 * (size_t)c;
    r[0] = ((cx + l0 * ux) + 0.5) / scale; r[1] = ((cy + l0 * uy) + 0.5) / scale;
    r[2] = ((cx + l1 * ux) + 0.5) / scale; r[3] = ((cy + l1 * uy) + 0.5) / scale;
    r[4] = wd; r[5] = nfa;
    n_out[c] = n; k_out[c] = k;
    keep[c] = dense && nfa > 0.0 ? 1 : 0;
  }
}

// ---- one workgroup: the kept candidates in order -> the outputs; offsets [V + 1] = the lines of the views before v
__global__ __launch_bounds__(1024) void detect_output_kernel(const int* __restrict__ cand, int* __restrict__ counters, int cap, int V, int hw,
                                                             const double* __restrict__ rec, const int* __restrict__ n_in,
                                                             const int* __restrict__ k_in, const int* __restrict__ keep, int* __restrict__ idx,
                                                             double* __restrict__ lines, double* __restrict__ width, double* __restrict__ nfa,
                                                             int* __restrict__ n_out, int* __restrict__ k_out, int* __restrict__ offsets) {
  __shared__ int s_wave[16], s_base;
  const int C = min(counters[0], cap);
  const int N = block_compact(C, [&](int c) { return keep[c] != 0; }, idx, s_wave, &s_base);
  __syncthreads();
  for (int q = threadIdx.x; q < N; q += blockDim.x) {
    const int c = idx[q];
    const double* r = rec + 6 * (size_t)c;
#pragma unroll
    for (int j = 0; j < 4; ++j) lines[4 * (size_t)q + j] = r[j];
    width[q] = r[4]; nfa[q] = r[5]; n_out[q] = n_in[c]; k_out[q] = k_in[c];
  }
  for (int v = threadIdx.x; v <= V; v += blockDim.x) {          // first q whose view is v or later
    int lo = 0, hi = N;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (cand[idx[mid]] / (2 * hw) < v) lo = mid + 1; else hi = mid; }
    offsets[v] = lo;
  }
  if (threadIdx.x == 0) counters[1] = N;
}

}  // namespace neat
