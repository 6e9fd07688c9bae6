// Post-processing of a parsed line soup between parsing and scoring: fuse (code/evaluation/fusion.py :79-141), refine
// (code/evaluation/refinement.py :95-198) and snap (code/evaluation/nms.py :156-204) as device launches.  As in kernels_parse.hpp all
// arithmetic is fp32, there are no float atomics (no atomics at all in this file), every reduction has a fixed shape, so every result is
// bit-identical from run to run, and nothing synchronises with the host: sizes that depend on the data (lines left, cells, peaks, edges)
// live in device memory and buffers are sized by their bounds.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>

#include "block_util.hpp"           // block_carry_scan, block_compact
#include "kernels_parse.hpp"        // parse_d4, PARSE_WG / PARSE_GT_CHUNK; project_point behind it

namespace neat {

// ---- match (fusion.py :105-114, refinement.py :132-150): grid (line tiles, views), view = view0 + blockIdx.y.  The line's end points go
// through project_point; the view's detections go through LDS in chunks (a broadcast read, as parse_match_kernel).  best = min over the
// detections j of min(dis1_j, dis2_j) (dis2: the detection against the reversed line), lowest j on ties; a row with a NaN distance never
// matches.  matched = best < thr, and with `refine` also all four projected coordinates in [0, width] x [0, height] (inclusive).
//   refine = 0 (fuse): label[blockIdx.y ncap + i] = j or -1, and present[off_v + j] = 1 (every store writes the same byte)
//   refine = 1: label [2 ncap] as parse_group reads it: row i = j if matched as is, row ncap + i = j if matched reversed (dis2_j strictly
//               the smaller), all others -1, the rows beyond the *n_dev lines of the set included
__global__ __launch_bounds__(PARSE_WG) void post_match_kernel(const float* __restrict__ lines, const int* __restrict__ n_dev, int ncap,
                                                              const float* __restrict__ det, int det_stride, const int* __restrict__ det_off,
                                                              const float* __restrict__ K3, const float* __restrict__ w2c, int view0, float thr,
                                                              int refine, float width, float height, int* __restrict__ label,
                                                              unsigned char* __restrict__ present) {
  __shared__ float4 s_gt[PARSE_GT_CHUNK];
  const int v = view0 + blockIdx.y;
  const int n = n_dev ? min(*n_dev, ncap) : ncap;
  const int i = blockIdx.x * PARSE_WG + threadIdx.x;
  if ((int)(blockIdx.x * PARSE_WG) >= n) {                 // whole workgroup beyond the lines (uniform exit before any barrier)
    if (refine && i < ncap) { label[i] = -1; label[(size_t)ncap + i] = -1; }
    return;
  }
  float u[4] = {0.f, 0.f, 0.f, 0.f};
  if (i < n) {
    for (int h = 0; h < 2; ++h) {
      const float x[3] = {lines[6 * (size_t)i + 3 * h], lines[6 * (size_t)i + 3 * h + 1], lines[6 * (size_t)i + 3 * h + 2]};
      float cam[3], w;
      project_point(K3 + 9 * v, w2c + 12 * v, x, cam, w);
      u[2 * h] = cam[0] / w; u[2 * h + 1] = cam[1] / w;
    }
  }
  const int g0 = det_off[v], m = det_off[v + 1] - g0;
  float best = INFINITY, best1 = INFINITY;
  int bj = -1;
  bool nan = false;
  for (int c0 = 0; c0 < m; c0 += PARSE_GT_CHUNK) {
    const int cn = min(PARSE_GT_CHUNK, m - c0);
    __syncthreads();
    for (int k = threadIdx.x; k < cn; k += PARSE_WG) {
      const float* g = det + (size_t)(g0 + c0 + k) * det_stride;
      s_gt[k] = make_float4(g[0], g[1], g[2], g[3]);
    }
    __syncthreads();
    for (int k = 0; k < cn; ++k) {
      const float4 g = s_gt[k];
      const float d1 = parse_d4(u[0], u[1], u[2], u[3], g), d2 = parse_d4(u[2], u[3], u[0], u[1], g);
      if (d1 != d1 || d2 != d2) nan = true;
      else { const float d = fminf(d1, d2); if (d < best) { best = d; best1 = d1; bj = c0 + k; } }
    }
  }
  if (i >= ncap) return;
  bool ok = i < n && bj >= 0 && !nan && best < thr;
  if (refine) {
    ok = ok && u[0] >= 0.f && u[0] <= width && u[2] >= 0.f && u[2] <= width && u[1] >= 0.f && u[1] <= height && u[3] >= 0.f && u[3] <= height;
    const bool rev = best != best1;
    label[i] = (ok && !rev) ? bj : -1;
    label[(size_t)ncap + i] = (ok && rev) ? bj : -1;
  } else {
    label[(size_t)blockIdx.y * ncap + i] = ok ? bj : -1;
    if (ok) present[g0 + bj] = 1;
  }
}

// ---- fuse (:116-122): the reference walks the sorted matched labels of a view with enumerate and adds scores_gt[rank], the rank of the label
// among the labels matched in that view.  One workgroup per view: rank[off_v + j] = matched detections of the view below j.
__global__ __launch_bounds__(1024) void post_rank_kernel(const unsigned char* __restrict__ present, const int* __restrict__ det_off,
                                                         int* __restrict__ rank) {
  __shared__ int s_wave[16];
  const int g0 = det_off[blockIdx.x], m = det_off[blockIdx.x + 1] - g0;
  block_carry_scan(m, [&](int l) { return present[g0 + l] != 0 ? 1 : 0; }, [&](int l, long long e) { rank[g0 + l] = (int)e; }, s_wave);
}

// one thread per line (:121-122, :131-133): the score sum in view order (the reference's order, so the fp32 sum is the reference's),
// score = sum / max(count, 1), keep = score > keep_thr.  by_label: the matched detection's own score instead of the ranked one.
__global__ __launch_bounds__(PARSE_WG) void post_fuse_score_kernel(const int* __restrict__ label, int n, int V, const float* __restrict__ det,
                                                                   int det_stride, const int* __restrict__ det_off, const int* __restrict__ rank,
                                                                   int by_label, float keep_thr, float* __restrict__ score,
                                                                   int* __restrict__ count, unsigned char* __restrict__ keep) {
  const int i = blockIdx.x * PARSE_WG + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
  int c = 0;
  for (int v = 0; v < V; ++v) {
    const int j = label[(size_t)v * n + i];
    if (j < 0) continue;
    const int g0 = det_off[v];
    const int r = by_label ? j : rank[g0 + j];
    s += det[(size_t)(g0 + r) * det_stride + 4];
    ++c;
  }
  const float sc = s / fmaxf((float)c, 1.f);
  score[i] = sc;
  count[i] = c;
  keep[i] = sc > keep_thr ? 1 : 0;
}

// one workgroup: the flagged lines, in order -> out, *n_out
__global__ __launch_bounds__(1024) void post_keep_kernel(const float* __restrict__ lines, int n, const unsigned char* __restrict__ keep,
                                                         int* __restrict__ idx_ws, float* __restrict__ out, int* __restrict__ n_out) {
  __shared__ int s_wave[16], s_base;
  const int k = block_compact(n, [&](int i) { return keep[i] != 0; }, idx_ws, s_wave, &s_base);
  __syncthreads();
  for (int q = threadIdx.x; q < 6 * k; q += blockDim.x) out[q] = lines[6 * (size_t)idx_ws[q / 6] + q % 6];
  if (threadIdx.x == 0) *n_out = k;
}

// ---- refine (:179-181): the next set = the lines that matched nothing, in order, then the group means (parse_group's output: one line
// per matched detection, ascending).  U + L <= *n_cur: every group has a member, so the set never grows.
__global__ __launch_bounds__(1024) void post_refine_assemble_kernel(const float* __restrict__ cur, const int* __restrict__ n_cur, int ncap,
                                                                    const int* __restrict__ label, const float* __restrict__ glines,
                                                                    const int* __restrict__ gcount, int* __restrict__ idx_ws,
                                                                    float* __restrict__ next, int* __restrict__ n_next) {
  __shared__ int s_wave[16], s_base;
  const int n = min(*n_cur, ncap);
  const int U = block_compact(n, [&](int i) { return label[i] < 0 && label[(size_t)ncap + i] < 0; }, idx_ws, s_wave, &s_base);
  __syncthreads();
  const int L = min(*gcount, ncap - U);
  for (int q = threadIdx.x; q < 6 * U; q += blockDim.x) next[q] = cur[6 * (size_t)idx_ws[q / 6] + q % 6];
  for (int q = threadIdx.x; q < 6 * L; q += blockDim.x) next[6 * (size_t)U + q] = glines[q];
  if (threadIdx.x == 0) *n_next = U + L;
}

// ---- snap (nms.py :162-174).  One workgroup: box = (min [3], max [3], delta [3] = (max - min) / (G - 1)) over the M end points.
__global__ __launch_bounds__(1024) void post_snap_bbox_kernel(const float* __restrict__ pts, int M, int G, float* __restrict__ box) {
  __shared__ float s_lo[3][1024], s_hi[3][1024];
  const int tid = threadIdx.x;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int e = tid; e < M; e += 1024) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { const float p = pts[3 * (size_t)e + a]; lo[a] = fminf(lo[a], p); hi[a] = fmaxf(hi[a], p); }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) { s_lo[a][tid] = lo[a]; s_hi[a][tid] = hi[a]; }
  __syncthreads();
  for (int h = 512; h > 0; h >>= 1) {
    if (tid < h) {
#pragma unroll
      for (int a = 0; a < 3; ++a) { s_lo[a][tid] = fminf(s_lo[a][tid], s_lo[a][tid + h]); s_hi[a][tid] = fmaxf(s_hi[a][tid], s_hi[a][tid + h]); }
    }
    __syncthreads();
  }
  if (tid < 3) {
    box[tid] = s_lo[tid][0];
    box[3 + tid] = s_hi[tid][0];
    box[6 + tid] = __fdiv_rn(s_hi[tid][0] - s_lo[tid][0], (float)(G - 1));
  }
}

// cell = round((p - min) / delta): an IEEE division, then round-half-to-even (numpy.round); a zero-extent axis has cell 0
__global__ __launch_bounds__(PARSE_WG) void post_snap_key_kernel(const float* __restrict__ pts, int M, int G, const float* __restrict__ box,
                                                                 int* __restrict__ key) {
  const int e = blockIdx.x * PARSE_WG + threadIdx.x;
  if (e >= M) return;
  int c[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float d = box[6 + a];
    const float q = d > 0.f ? rintf(__fdiv_rn(pts[3 * (size_t)e + a] - box[a], d)) : 0.f;
    c[a] = (int)fminf(fmaxf(q, 0.f), (float)(G - 1));
  }
  key[e] = (c[0] * G + c[1]) * G + c[2];
}

// one workgroup over the sorted keys: head[u] = first position of the u-th occupied cell, *n_cells = occupied cells
__global__ __launch_bounds__(1024) void post_snap_cells_kernel(const int* __restrict__ skey, int M, int* __restrict__ head, int* __restrict__ n_cells) {
  __shared__ int s_wave[16], s_base;
  const int U = block_compact(M, [&](int i) { return i == 0 || skey[i] != skey[i - 1]; }, head, s_wave, &s_base);
  if (threadIdx.x == 0) *n_cells = U;
}

__device__ __forceinline__ int post_cell_count(const int* __restrict__ skey, const int* __restrict__ head, int U, int M, int k) {
  int lo = 0, hi = U;                                     // first cell with key >= k
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (skey[head[mid]] < k) lo = mid + 1; else hi = mid; }
  if (lo >= U || skey[head[lo]] != k) return 0;
  return (lo + 1 < U ? head[lo + 1] : M) - head[lo];
}

// one thread per occupied cell (:178-184): a peak holds at least as many end points as every cell of its 3 x 3 x 3 neighbourhood inside the grid
__global__ __launch_bounds__(PARSE_WG) void post_snap_peak_kernel(const int* __restrict__ skey, const int* __restrict__ head,
                                                                  const int* __restrict__ n_cells, int M, int G, int* __restrict__ flag,
                                                                  int* __restrict__ cnt) {
  const int u = blockIdx.x * PARSE_WG + threadIdx.x, U = *n_cells;
  if (u >= U || u >= M) return;
  const int k = skey[head[u]];
  const int c = (u + 1 < U ? head[u + 1] : M) - head[u];
  const int iz = k % G, iy = (k / G) % G, ix = k / (G * G);
  bool peak = true;
  for (int dx = -1; dx <= 1; ++dx)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dz = -1; dz <= 1; ++dz) {
        const int x = ix + dx, y = iy + dy, z = iz + dz;
        if ((dx | dy | dz) == 0 || x < 0 || y < 0 || z < 0 || x >= G || y >= G || z >= G) continue;
        if (post_cell_count(skey, head, U, M, (x * G + y) * G + z) > c) peak = false;
      }
  flag[u] = peak ? 1 : 0;
  cnt[u] = c;
}

// node i of torch.linspace(lo, hi, G) in float32: lo + step i below the middle, hi - step (G - 1 - i) from it on, each one fused multiply-add
__device__ __forceinline__ float post_linspace_node(float lo, float hi, float step, int G, int i) {
  return i < G / 2 ? fmaf(step, (float)i, lo) : fmaf(-step, (float)(G - 1 - i), hi);
}

// one workgroup: the peaks in ascending key order (row-major (ix, iy, iz), as nonzero()) -> junctions [P,3], pcount [P], *n_peaks
__global__ __launch_bounds__(1024) void post_snap_select_kernel(const int* __restrict__ skey, const int* __restrict__ head,
                                                                const int* __restrict__ n_cells, int M, int G, const float* __restrict__ box,
                                                                const int* __restrict__ flag, const int* __restrict__ cnt, int* __restrict__ pidx,
                                                                float* __restrict__ junc, int* __restrict__ pcount, int* __restrict__ n_peaks) {
  __shared__ int s_wave[16], s_base;
  const int U = min(*n_cells, M);
  const int P = block_compact(U, [&](int u) { return flag[u] != 0; }, pidx, s_wave, &s_base);
  __syncthreads();
  for (int p = threadIdx.x; p < P; p += blockDim.x) {
    const int u = pidx[p], k = skey[head[u]];
    const int c[3] = {k / (G * G), (k / G) % G, k % G};
#pragma unroll
    for (int a = 0; a < 3; ++a) junc[3 * (size_t)p + a] = post_linspace_node(box[a], box[3 + a], box[6 + a], G, c[a]);
    pcount[p] = cnt[u];
  }
  if (threadIdx.x == 0) *n_peaks = P;
}

// one thread per end point (:191-194): the nearest peak by squared distance, lowest index on ties; the peaks go through LDS in chunks
__global__ __launch_bounds__(PARSE_WG) void post_snap_nearest_kernel(const float* __restrict__ pts, int M, const float* __restrict__ junc,
                                                                     const int* __restrict__ n_peaks, int* __restrict__ near,
                                                                     float* __restrict__ dist2) {
  __shared__ float s_j[3 * PARSE_GT_CHUNK];
  const int P = min(*n_peaks, M);
  const int e = blockIdx.x * PARSE_WG + threadIdx.x;
  float p[3] = {0.f, 0.f, 0.f};
  if (e < M) { p[0] = pts[3 * (size_t)e]; p[1] = pts[3 * (size_t)e + 1]; p[2] = pts[3 * (size_t)e + 2]; }
  float best = INFINITY;
  int bi = -1;
  for (int c0 = 0; c0 < P; c0 += PARSE_GT_CHUNK) {
    const int cn = min(PARSE_GT_CHUNK, P - c0);
    __syncthreads();
    for (int k = threadIdx.x; k < 3 * cn; k += PARSE_WG) s_j[k] = junc[3 * (size_t)c0 + k];
    __syncthreads();
    for (int k = 0; k < cn; ++k) {
      const float a0 = s_j[3 * k] - p[0], a1 = s_j[3 * k + 1] - p[1], a2 = s_j[3 * k + 2] - p[2];
      const float d = (a0 * a0 + a1 * a1) + a2 * a2;
      if (d < best) { best = d; bi = c0 + k; }
    }
  }
  if (e < M) { near[e] = bi; dist2[e] = best; }
}

__device__ __forceinline__ bool post_snap_line_kept(const int* __restrict__ near, const float* __restrict__ dist2, float max_snap, int i) {
  if (near[2 * i] < 0 || near[2 * i + 1] < 0) return false;
  return max_snap < 0.f || (sqrtf(dist2[2 * i]) < max_snap && sqrtf(dist2[2 * i + 1]) < max_snap);
}

// one workgroup (:195-200): the kept lines' peak pairs, in line order.  max_snap < 0 keeps every line, as the reference does.
__global__ __launch_bounds__(1024) void post_snap_edges_kernel(const int* __restrict__ near, const float* __restrict__ dist2, int n, float max_snap,
                                                               const float* __restrict__ junc, int* __restrict__ idx_ws, int* __restrict__ edges,
                                                               float* __restrict__ lines_out, int* __restrict__ n_edges) {
  __shared__ int s_wave[16], s_base;
  const int E = block_compact(n, [&](int i) { return post_snap_line_kept(near, dist2, max_snap, i); }, idx_ws, s_wave, &s_base);
  __syncthreads();
  for (int q = threadIdx.x; q < 2 * E; q += blockDim.x) {
    const int j = near[2 * idx_ws[q >> 1] + (q & 1)];
    edges[q] = j;
#pragma unroll
    for (int d = 0; d < 3; ++d) lines_out[3 * (size_t)q + d] = junc[3 * (size_t)j + d];
  }
  if (threadIdx.x == 0) *n_edges = E;
}

// --unique: the pair (min, max) of a kept line with two different peaks as one 64-bit key, all others the largest key
constexpr unsigned long long POST_NO_PAIR = ~0ull;
__global__ __launch_bounds__(PARSE_WG) void post_snap_pairkey_kernel(const int* __restrict__ near, const float* __restrict__ dist2, int n,
                                                                     float max_snap, unsigned long long* __restrict__ pkey) {
  const int i = blockIdx.x * PARSE_WG + threadIdx.x;
  if (i >= n) return;
  unsigned long long k = POST_NO_PAIR;
  if (post_snap_line_kept(near, dist2, max_snap, i) && near[2 * i] != near[2 * i + 1]) {
    const unsigned a = (unsigned)min(near[2 * i], near[2 * i + 1]), b = (unsigned)max(near[2 * i], near[2 * i + 1]);
    k = ((unsigned long long)a << 32) | b;
  }
  pkey[i] = k;
}

// one workgroup over the sorted pair keys: the distinct pairs, ascending
__global__ __launch_bounds__(1024) void post_snap_unique_kernel(const unsigned long long* __restrict__ spkey, int n, const float* __restrict__ junc,
                                                                int* __restrict__ idx_ws, int* __restrict__ edges, float* __restrict__ lines_out,
                                                                int* __restrict__ n_edges) {
  __shared__ int s_wave[16], s_base;
  const int E = block_compact(n, [&](int i) { return spkey[i] != POST_NO_PAIR && (i == 0 || spkey[i] != spkey[i - 1]); }, idx_ws, s_wave, &s_base);
  __syncthreads();
  for (int q = threadIdx.x; q < 2 * E; q += blockDim.x) {
    const unsigned long long k = spkey[idx_ws[q >> 1]];
    const int j = (q & 1) ? (int)(k & 0xffffffffull) : (int)(k >> 32);
    edges[q] = j;
#pragma unroll
    for (int d = 0; d < 3; ++d) lines_out[3 * (size_t)q + d] = junc[3 * (size_t)j + d];
  }
  if (threadIdx.x == 0) *n_edges = E;
}

}  // namespace neat
