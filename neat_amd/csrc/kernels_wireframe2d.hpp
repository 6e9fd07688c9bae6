// 2-D wireframes with shared junctions from the views' detected segments (neat_amd/detect.py junctions / wireframes; the rule: DESIGN 3o,
// restated in float64 by tests/junctions2d_f64.py).  The ends of a view's segments that meet near the crossing of their lines are joined
// into components; a component of two ends or more becomes one junction at the least-squares point of its members' lines; a lone end
// that stops at another segment's inside moves onto it (a T); the segments between distinct vertices, one per vertex pair, are the edges.
//
// Float64 throughout, contraction into fused multiply-adds off in every function that forms a value the reference forms: every product,
// sum, quotient and square root is the reference's, one IEEE operation each in the order written here, so the vertices are the
// reference's bits and the decisions are the reference's.  No transcendental function.  Nothing depends on an order of execution: the
// components are a union-find with atomicMin whose roots are the smallest member, the only other atomic is an integer atomicMax, a
// junction's sums run in ascending endpoint order in every lane, and the lists are counted, scanned and filled in order.  Two runs give
// the same bytes.
//
// Segments are numbered over all views in (view, index) order; segoff [V + 1] are the views' first numbers.  End k of segment g is
// endpoint 2 g + k.  The three pair passes (meet, T, duplicate edges) are one workgroup of WF_WG threads per (view, tile of WF_WG of
// its segments), one thread a segment, with the view's segments passing through LDS in tiles of WF_WG partners.
#pragma once
#include <float.h>
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stddef.h>

#include "block_util.hpp"           // block_carry_scan
#include "graph_util.hpp"           // uf_union, uf_flatten_kernel, wave_members

namespace neat {

constexpr int WF_WG = 256;                       // pair kernels: threads a workgroup = segments a tile
constexpr int WF_WAVES = WF_WG / 64;             // component kernel: one wavefront per endpoint
constexpr int WF_REC = 8;                        // doubles per segment: p, q, u, L, g; u is NaN for a segment that takes part in nothing

// a view's segments [a0, a1), whatever segoff holds: nothing outside [0, S] is ever indexed
__device__ __forceinline__ void wf_view_range(const int* __restrict__ segoff, int a, int S, int* a0, int* a1) {
  *a0 = max(0, min(segoff[a], S));
  *a1 = max(*a0, min(segoff[a + 1], S));
}

// ---- per segment, once: its view, its record, and its two endpoints as their own roots
__global__ __launch_bounds__(WF_WG) void wf_segment_kernel(const double* __restrict__ seg, const int* __restrict__ segoff, int V, int S, double gap,
                                                           double frac, double* __restrict__ rec, int* __restrict__ view,
                                                           int* __restrict__ parent, int* __restrict__ last) {
#pragma clang fp contract(off)
  const int g = blockIdx.x * WF_WG + threadIdx.x;
  if (g >= S) return;
  int lo = 0, hi = V;                            // the last view that starts at or before g (views may be empty)
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (segoff[mid] <= g) lo = mid; else hi = mid; }
  view[g] = lo;
  const double px = seg[4 * (size_t)g], py = seg[4 * (size_t)g + 1], qx = seg[4 * (size_t)g + 2], qy = seg[4 * (size_t)g + 3];
  const double dx = qx - px, dy = qy - py;
  const double L = sqrt(dx * dx + dy * dy);
  const bool ok = L > 0.0 && L <= DBL_MAX;
  double* R = rec + (size_t)WF_REC * g;
  R[0] = px; R[1] = py; R[2] = qx; R[3] = qy;
  R[4] = ok ? dx / L : NAN; R[5] = ok ? dy / L : NAN;
  R[6] = L; R[7] = fmin(gap, frac * L);
  parent[2 * g] = 2 * g; parent[2 * g + 1] = 2 * g + 1;
  last[2 * g] = 2 * g; last[2 * g + 1] = 2 * g + 1;
}

// The crossing of the lines of A and B, A the segment of the lower index.  False unless |c| >= sin_min (a NaN fails)
__device__ __forceinline__ bool wf_cross(const double* A, const double* B, double sin_min, double* X, double* Y) {
#pragma clang fp contract(off)
  const double c = A[4] * B[5] - A[5] * B[4];
  if (!(fabs(c) >= sin_min)) return false;
  const double wx = B[0] - A[0], wy = B[1] - A[1];
  const double t = (wx * B[5] - wy * B[4]) / c;
  *X = A[0] + t * A[4]; *Y = A[1] + t * A[5];
  return true;
}

// (X - e).o for end k of the segment R: e = p, o = -u (k = 0) or e = q, o = +u (k = 1)
__device__ __forceinline__ double wf_along(const double* R, int k, double X, double Y) {
#pragma clang fp contract(off)
  const double ox = k ? R[4] : -R[4], oy = k ? R[5] : -R[5];
  return (X - R[2 * k]) * ox + (Y - R[2 * k + 1]) * oy;
}

__device__ __forceinline__ double wf_dist(double X, double Y, double ex, double ey) {
#pragma clang fp contract(off)
  const double dx = X - ex, dy = Y - ey;
  return sqrt(dx * dx + dy * dy);
}

// a tile of nt partners' records, from segment first on, into LDS; a barrier before (the last tile has been walked) and after
__device__ __forceinline__ void wf_load_tile(double* s_b, const double* __restrict__ rec, int first, int nt) {
  __syncthreads();
  for (int k = threadIdx.x; k < nt * WF_REC; k += WF_WG) s_b[k] = rec[(size_t)first * WF_REC + k];
  __syncthreads();
}

// ---- pair pass 1: every pair i < j of a view once, by the thread of i; ends that meet are joined
__global__ __launch_bounds__(WF_WG) void wf_meet_kernel(const int* __restrict__ segoff, int S, int tiles, const double* __restrict__ rec,
                                                        double sin_min, int* parent) {
#pragma clang fp contract(off)
  __shared__ double s_b[WF_WG * WF_REC];
  const int tile = blockIdx.x % tiles, a = blockIdx.x / tiles;
  int a0, a1;
  wf_view_range(segoff, a, S, &a0, &a1);
  const int na = a1 - a0;
  if (tile * WF_WG >= na) return;                // the whole workgroup: the grid is sized for the largest view
  const int i = tile * WF_WG + threadIdx.x;
  const bool live = i < na;
  double A[WF_REC];
#pragma unroll
  for (int q = 0; q < WF_REC; ++q) A[q] = rec[(size_t)(a0 + (live ? i : 0)) * WF_REC + q];
  for (int j0 = tile * WF_WG; j0 < na; j0 += WF_WG) {
    const int nt = min(WF_WG, na - j0);
    wf_load_tile(s_b, rec, a0 + j0, nt);
    if (!live) continue;
    for (int jj = max(0, i + 1 - j0); jj < nt; ++jj) {
      const double* B = s_b + WF_REC * jj;
      double X, Y;
      if (!wf_cross(A, B, sin_min, &X, &Y)) continue;
#pragma unroll
      for (int ki = 0; ki < 2; ++ki) {
        const double ea = wf_along(A, ki, X, Y);
        if (!(ea >= -A[7] && ea <= A[7])) continue;
#pragma unroll
        for (int kj = 0; kj < 2; ++kj) {
          const double eb = wf_along(B, kj, X, Y);
          if (eb >= -B[7] && eb <= B[7]) uf_union<__HIP_MEMORY_SCOPE_AGENT>(parent, 2 * (a0 + i) + ki, 2 * (a0 + j0 + jj) + kj);
        }
      }
    }
  }
}

// one workgroup, after uf_flatten_kernel (label = the root = the component's lowest endpoint; last[root] = its highest): vidx [2 S] =
// the roots before each endpoint = a root's place in the vertex list; voff [V + 1] = the views' first vertices
__global__ __launch_bounds__(1024) void wf_vertex_scan_kernel(int S, int V, const int* __restrict__ segoff, const int* __restrict__ label,
                                                              int* __restrict__ vidx, int* __restrict__ voff) {
  __shared__ int s_wave[16];
  const long long tot = block_carry_scan(2 * S, [&](int e) { return label[e] == e ? 1 : 0; }, [&](int e, long long x) { vidx[e] = (int)x; }, s_wave);
  __syncthreads();
  for (int v = threadIdx.x; v <= V; v += blockDim.x) {
    const int s = max(0, min(segoff[v], S));
    voff[v] = s < S ? vidx[2 * s] : (int)tot;
  }
}

// ---- one wavefront per junction, at its root r: its members are the endpoints in [r, last[r]] with label r (wave_members); every lane
// adds the five sums of all of them in ascending order, so all lanes hold the same bits
__global__ __launch_bounds__(WF_WG) void wf_junction_kernel(int n, const int* __restrict__ label, const int* __restrict__ last,
                                                            const int* __restrict__ vidx, const double* __restrict__ rec,
                                                            const double* __restrict__ weight, double* __restrict__ vertices,
                                                            int* __restrict__ degree, int* __restrict__ kind, double* __restrict__ score,
                                                            double* __restrict__ spread, int* __restrict__ t_edge) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, r = blockIdx.x * WF_WAVES + (threadIdx.x >> 6);
  if (r >= n || label[r] != r) return;           // whole wavefronts leave; the kernel has no barrier
  const int end = last[r];
  if (end == r) return;                          // a lone end: the T pass writes it
  double a11 = 0.0, a12 = 0.0, a22 = 0.0, b1 = 0.0, b2 = 0.0, sc = -INFINITY;
  const int m = wave_members(label, r, end, lane, [&](int e) { sc = fmax(sc, weight[e >> 1]); }, [&](int e) {
#pragma clang fp contract(off)
    const double* R = rec + (size_t)WF_REC * (e >> 1);
    const double nx = -R[5], ny = R[4];
    const double c = nx * R[0] + ny * R[1];
    a11 = a11 + nx * nx; a12 = a12 + nx * ny; a22 = a22 + ny * ny;
    b1 = b1 + nx * c; b2 = b2 + ny * c;
  });
  const double det = a11 * a22 - a12 * a12;
  const double X = (a22 * b1 - a12 * b2) / det, Y = (a11 * b2 - a12 * b1) / det;
  double sp = 0.0;
  wave_members_each(label, r, end, lane, [&](int e) {
    const double* R = rec + (size_t)WF_REC * (e >> 1);
    sp = fmax(sp, wf_dist(X, Y, R[2 * (e & 1)], R[2 * (e & 1) + 1]));
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { sc = fmax(sc, __shfl_xor(sc, o)); sp = fmax(sp, __shfl_xor(sp, o)); }
  if (lane != 0) return;
  const int q = vidx[r];
  vertices[2 * (size_t)q] = X; vertices[2 * (size_t)q + 1] = Y;
  degree[q] = m; kind[q] = 1; score[q] = sc; spread[q] = sp; t_edge[q] = -1;
}

// ---- pair pass 2: a lone end of i against the inside of every other segment j of the view (the crossing formed with the lower index
// first, as the meet pass formed it); the nearest along i wins, the lowest j on a tie.  Writes the lone ends' vertices and every end's vertex
__global__ __launch_bounds__(WF_WG) void wf_tee_kernel(const int* __restrict__ segoff, int S, int tiles, const double* __restrict__ rec,
                                                       const double* __restrict__ weight, double sin_min, int t_on,
                                                       const int* __restrict__ label, const int* __restrict__ last, const int* __restrict__ vidx,
                                                       const int* __restrict__ voff, double* __restrict__ vertices, int* __restrict__ degree,
                                                       int* __restrict__ kind, double* __restrict__ score, double* __restrict__ spread,
                                                       int* __restrict__ t_edge, int* __restrict__ ends) {
#pragma clang fp contract(off)
  __shared__ double s_b[WF_WG * WF_REC];
  const int tile = blockIdx.x % tiles, a = blockIdx.x / tiles;
  int a0, a1;
  wf_view_range(segoff, a, S, &a0, &a1);
  const int na = a1 - a0;
  if (tile * WF_WG >= na) return;
  const int i = tile * WF_WG + threadIdx.x;
  const bool live = i < na;
  const int g = a0 + (live ? i : 0);
  double A[WF_REC];
#pragma unroll
  for (int q = 0; q < WF_REC; ++q) A[q] = rec[(size_t)g * WF_REC + q];
  bool lone[2];
  double best[2] = {INFINITY, INFINITY}, bx[2] = {0.0, 0.0}, by[2] = {0.0, 0.0};
  int bj[2] = {-1, -1};
#pragma unroll
  for (int k = 0; k < 2; ++k) lone[k] = live && label[2 * g + k] == 2 * g + k && last[2 * g + k] == 2 * g + k;
  const bool search = t_on && (lone[0] || lone[1]);
  for (int j0 = 0; j0 < na; j0 += WF_WG) {
    const int nt = min(WF_WG, na - j0);
    wf_load_tile(s_b, rec, a0 + j0, nt);
    if (!search) continue;
    for (int jj = 0; jj < nt; ++jj) {
      const int j = j0 + jj;
      if (j == i) continue;
      const double* B = s_b + WF_REC * jj;
      double X, Y;
      if (!(j > i ? wf_cross(A, B, sin_min, &X, &Y) : wf_cross(B, A, sin_min, &X, &Y))) continue;
      const double s = (X - B[0]) * B[4] + (Y - B[1]) * B[5];
      if (!(s > B[7] && s < B[6] - B[7])) continue;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const double ea = fabs(wf_along(A, k, X, Y));
        if (lone[k] && ea <= A[7] && ea < best[k]) { best[k] = ea; bj[k] = j; bx[k] = X; by[k] = Y; }
      }
    }
  }
  if (!live) return;
  const int v0 = voff[a];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int e = 2 * g + k;
    ends[e] = vidx[label[e]] - v0;
    if (!lone[k]) continue;
    const int q = vidx[e];
    const bool t = bj[k] >= 0;
    vertices[2 * (size_t)q] = t ? bx[k] : A[2 * k]; vertices[2 * (size_t)q + 1] = t ? by[k] : A[2 * k + 1];
    degree[q] = 1; kind[q] = t ? 2 : 0; score[q] = weight[g];
    spread[q] = t ? wf_dist(bx[k], by[k], A[2 * k], A[2 * k + 1]) : 0.0;
    t_edge[q] = bj[k];
  }
}

// ---- pair pass 3: a segment is an edge unless both ends are one vertex, or another segment of the view joins the same two vertices
// with a larger weight (the lower index on equal weights)
__global__ __launch_bounds__(WF_WG) void wf_duplicate_kernel(const int* __restrict__ segoff, int S, int tiles, const int* __restrict__ ends,
                                                             const double* __restrict__ weight, int* __restrict__ keep) {
  __shared__ int s_lo[WF_WG], s_hi[WF_WG];
  __shared__ double s_w[WF_WG];
  const int tile = blockIdx.x % tiles, a = blockIdx.x / tiles;
  int a0, a1;
  wf_view_range(segoff, a, S, &a0, &a1);
  const int na = a1 - a0;
  if (tile * WF_WG >= na) return;
  const int i = tile * WF_WG + threadIdx.x;
  const bool live = i < na;
  const int g = a0 + (live ? i : 0);
  const int lo = min(ends[2 * g], ends[2 * g + 1]), hi = max(ends[2 * g], ends[2 * g + 1]);
  const double w = weight[g];
  bool beaten = false;
  for (int j0 = 0; j0 < na; j0 += WF_WG) {
    const int nt = min(WF_WG, na - j0);
    __syncthreads();
    if ((int)threadIdx.x < nt) {
      const int p = a0 + j0 + threadIdx.x;
      s_lo[threadIdx.x] = min(ends[2 * p], ends[2 * p + 1]); s_hi[threadIdx.x] = max(ends[2 * p], ends[2 * p + 1]); s_w[threadIdx.x] = weight[p];
    }
    __syncthreads();
    for (int jj = 0; jj < nt; ++jj) {
      const int j = j0 + jj;
      if (j != i && s_lo[jj] == lo && s_hi[jj] == hi && (s_w[jj] > w || (s_w[jj] == w && j < i))) beaten = true;
    }
  }
  if (live) keep[g] = lo != hi && !beaten ? 1 : 0;
}

// one workgroup: eidx [S] = the edges before each segment; eoff [V + 1] = the views' first edges
__global__ __launch_bounds__(1024) void wf_edge_scan_kernel(int S, int V, const int* __restrict__ segoff, const int* __restrict__ keep,
                                                            int* __restrict__ eidx, int* __restrict__ eoff) {
  __shared__ int s_wave[16];
  const long long tot = block_carry_scan(S, [&](int g) { return keep[g]; }, [&](int g, long long x) { eidx[g] = (int)x; }, s_wave);
  __syncthreads();
  for (int v = threadIdx.x; v <= V; v += blockDim.x) {
    const int s = max(0, min(segoff[v], S));
    eoff[v] = s < S ? eidx[s] : (int)tot;
  }
}

__global__ __launch_bounds__(WF_WG) void wf_edge_fill_kernel(int S, const int* __restrict__ segoff, const int* __restrict__ view,
                                                             const int* __restrict__ keep, const int* __restrict__ eidx,
                                                             const int* __restrict__ ends, const double* __restrict__ weight,
                                                             int* __restrict__ edges, double* __restrict__ eweight, int* __restrict__ esrc) {
  const int g = blockIdx.x * WF_WG + threadIdx.x;
  if (g >= S || !keep[g]) return;
  const int q = eidx[g];
  edges[2 * (size_t)q] = ends[2 * g]; edges[2 * (size_t)q + 1] = ends[2 * g + 1];
  eweight[q] = weight[g];
  esrc[q] = g - segoff[view[g]];
}

}  // namespace neat
