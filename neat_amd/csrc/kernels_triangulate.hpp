// 3-D line segments triangulated from the views' 2-D detections (neat_amd/triangulate.py; the rule: DESIGN 3k, restated in float64 by
// tests/triangulate_f64.py).  Every 2-D segment of a view is paired with every segment of the view's M nearest views: the partner's
// back-projected plane cuts the two viewing rays of the segment's end points, which gives a hypothesis (two depths).  The hypotheses of
// a segment vote for each other across the neighbour slots; the best one is the segment's 3-D estimate; estimates that were paired
// and lie on one line are joined into components; a component seen from enough views becomes a line.
//
// Float64 throughout, contraction into fused multiply-adds off in every function that forms a value the reference forms: every product,
// sum and quotient is the reference's, one IEEE operation each in the order written here, so the depths are the reference's bits and
// the decisions are the reference's.  The only transcendental function is the exp of the score.  Nothing depends on an order of
// execution: the lists are counted, scanned and filled in order, the components are a union-find with atomicMin whose roots are the
// smallest member, the only other atomic is an integer atomicMax.  Two runs give the same bytes.
//
// Cameras: TRI_CAM doubles a view, from the host (triangulate.camera_block): K^-1 [9], R [9] world -> camera, t [3], K [9], P = K [R|t]
// [12], C [3].  Segments are numbered over all views in (view, index) order; segoff [V + 1] are the views' first numbers.
#pragma once
#include <float.h>
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stddef.h>

#include "block_util.hpp"           // block_carry_scan, block_compact
#include "graph_util.hpp"           // uf_union, uf_flatten_kernel, wave_members_each

namespace neat {

constexpr int TRI_WG = 256;                      // pair kernel: one thread per segment of the view, tiles of TRI_WG partners in LDS
constexpr int TRI_WAVES = TRI_WG / 64;           // score, link and component kernels: one wavefront per segment
constexpr int TRI_CAM = 48;
constexpr int TRI_KINV = 0, TRI_R = 9, TRI_T = 18, TRI_K = 21, TRI_P = 30, TRI_C = 42;
constexpr int TRI_SEGA = 9, TRI_SEGB = 10;       // doubles per segment: as the paired one (d_1, d_2, n_a), as the partner (below)

__device__ __forceinline__ double tri_norm3(double x, double y, double z) {
#pragma clang fp contract(off)
  return sqrt((x * x + y * y) + z * z);
}

// ---- per segment, once: the viewing rays of its end points and their plane's normal; its back-projected plane pi = P^T (q1 x q2), the
// direction u = q2 - q1 with u.u, and |pi_xyz|.  view [S]: the segment's view
__global__ __launch_bounds__(TRI_WG) void tri_segment_kernel(const double* __restrict__ seg, const int* __restrict__ segoff, int V, int S,
                                                             const double* __restrict__ cam, double* __restrict__ sega,
                                                             double* __restrict__ segb, int* __restrict__ view) {
#pragma clang fp contract(off)
  const int g = blockIdx.x * TRI_WG + threadIdx.x;
  if (g >= S) return;
  int lo = 0, hi = V;                            // the last view that starts at or before g (views may be empty)
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (segoff[mid] <= g) lo = mid; else hi = mid; }
  view[g] = lo;
  const double* c = cam + (size_t)TRI_CAM * lo;
  const double* Ki = c + TRI_KINV;
  const double* R = c + TRI_R;
  const double* P = c + TRI_P;
  const double x1 = seg[4 * (size_t)g], y1 = seg[4 * (size_t)g + 1], x2 = seg[4 * (size_t)g + 2], y2 = seg[4 * (size_t)g + 3];
  double d[2][3];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const double x = k ? x2 : x1, y = k ? y2 : y1;
    double r[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) r[q] = (Ki[3 * q] * x + Ki[3 * q + 1] * y) + Ki[3 * q + 2];
#pragma unroll
    for (int q = 0; q < 3; ++q) d[k][q] = (R[q] * r[0] + R[3 + q] * r[1]) + R[6 + q] * r[2];
  }
  const double n0 = d[0][1] * d[1][2] - d[0][2] * d[1][1], n1 = d[0][2] * d[1][0] - d[0][0] * d[1][2], n2 = d[0][0] * d[1][1] - d[0][1] * d[1][0];
  const double nn = tri_norm3(n0, n1, n2);
  double* A = sega + (size_t)TRI_SEGA * g;
#pragma unroll
  for (int q = 0; q < 3; ++q) { A[q] = d[0][q]; A[3 + q] = d[1][q]; }
  A[6] = n0 / nn; A[7] = n1 / nn; A[8] = n2 / nn;
  const double l0 = y1 - y2, l1 = x2 - x1, l2 = x1 * y2 - y1 * x2;
  double* B = segb + (size_t)TRI_SEGB * g;
#pragma unroll
  for (int q = 0; q < 4; ++q) B[q] = (P[q] * l0 + P[4 + q] * l1) + P[8 + q] * l2;
  const double ux = x2 - x1, uy = y2 - y1;
  B[4] = x1; B[5] = y1; B[6] = ux; B[7] = uy; B[8] = ux * ux + uy * uy;
  B[9] = tri_norm3(B[0], B[1], B[2]);
}

struct TriView { double C[3], R[9], t[3], K[6]; };      // of a pair launch: the view's centre, the neighbour's pose and first two rows of K

// The pair test.  q: the partner's ten doubles with q[3] replaced by e = pi_xyz . C_a + pi_w.  Every comparison is one that a NaN fails
__device__ __forceinline__ bool tri_pair(const double* q, const double (&d1)[3], const double (&d2)[3], const double (&n)[3], const TriView& w,
                                         double cos_min, double overlap_min, double* s1_out, double* s2_out) {
#pragma clang fp contract(off)
  const double c = fabs((n[0] * q[0] + n[1] * q[1]) + n[2] * q[2]) / q[9];
  if (!(c <= cos_min)) return false;
  const double s1 = -q[3] / ((q[0] * d1[0] + q[1] * d1[1]) + q[2] * d1[2]);
  const double s2 = -q[3] / ((q[0] * d2[0] + q[1] * d2[1]) + q[2] * d2[2]);
  if (!(s1 > 0.0 && s2 > 0.0 && s1 <= DBL_MAX && s2 <= DBL_MAX)) return false;
  double t[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const double s = k ? s2 : s1;
    const double (&d)[3] = k ? d2 : d1;
    const double X0 = w.C[0] + s * d[0], X1 = w.C[1] + s * d[1], X2 = w.C[2] + s * d[2];
    const double x0 = ((w.R[0] * X0 + w.R[1] * X1) + w.R[2] * X2) + w.t[0];
    const double x1 = ((w.R[3] * X0 + w.R[4] * X1) + w.R[5] * X2) + w.t[1];
    const double x2 = ((w.R[6] * X0 + w.R[7] * X1) + w.R[8] * X2) + w.t[2];
    if (!(x2 > 0.0)) return false;
    const double y0 = ((w.K[0] * x0 + w.K[1] * x1) + w.K[2] * x2) / x2, y1 = ((w.K[3] * x0 + w.K[4] * x1) + w.K[5] * x2) / x2;
    t[k] = ((y0 - q[4]) * q[6] + (y1 - q[5]) * q[7]) / q[8];
    if (!(fabs(t[k]) <= DBL_MAX)) return false;
  }
  const double lo = fmin(t[0], t[1]), hi = fmax(t[0], t[1]);
  const double inter = fmin(hi, 1.0) - fmax(lo, 0.0), uni = fmax(hi, 1.0) - fmin(lo, 0.0);
  if (!(inter >= overlap_min * uni)) return false;
  *s1_out = s1; *s2_out = s2;
  return true;
}

// ---- one workgroup per (view a, slot m, tile of TRI_WG segments of a); the partners of b = nb[a][m] pass through LDS in tiles.
// FILL = false counts the hypotheses per (segment, slot); FILL = true runs the same test again and writes them from off[segment][slot]
// on, in partner order: the list is exact in size and in (a, i, m, j) order
template <bool FILL>
__global__ __launch_bounds__(TRI_WG) void tri_match_kernel(const int* __restrict__ segoff, const int* __restrict__ nb, int M, int tiles,
                                                           const double* __restrict__ cam, const double* __restrict__ sega,
                                                           const double* __restrict__ segb, double cos_min, double overlap_min,
                                                           int* __restrict__ cnt, const int* __restrict__ off, int H, int* __restrict__ hyp_m,
                                                           int* __restrict__ hyp_j, double* __restrict__ hyp_s) {
#pragma clang fp contract(off)
  __shared__ double s_b[TRI_WG * TRI_SEGB];
  const int tile = blockIdx.x % tiles, m = (blockIdx.x / tiles) % M, a = blockIdx.x / (tiles * M);
  const int a0 = segoff[a], na = segoff[a + 1] - a0;
  if (tile * TRI_WG >= na) return;               // the whole workgroup: the grid is sized for the largest view
  const int b = nb[a * M + m], b0 = segoff[b], nbs = segoff[b + 1] - b0;
  const int i = tile * TRI_WG + threadIdx.x;
  const bool live = i < na;
  const int g = a0 + (live ? i : 0);
  double d1[3], d2[3], n[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) { d1[q] = sega[(size_t)TRI_SEGA * g + q]; d2[q] = sega[(size_t)TRI_SEGA * g + 3 + q]; n[q] = sega[(size_t)TRI_SEGA * g + 6 + q]; }
  TriView w;
  const double* ca = cam + (size_t)TRI_CAM * a;
  const double* cb = cam + (size_t)TRI_CAM * b;
#pragma unroll
  for (int q = 0; q < 3; ++q) { w.C[q] = ca[TRI_C + q]; w.t[q] = cb[TRI_T + q]; }
#pragma unroll
  for (int q = 0; q < 9; ++q) w.R[q] = cb[TRI_R + q];
#pragma unroll
  for (int q = 0; q < 6; ++q) w.K[q] = cb[TRI_K + q];
  int count = 0;
  size_t at = FILL && live ? (size_t)off[(size_t)g * M + m] : 0;
  for (int j0 = 0; j0 < nbs; j0 += TRI_WG) {
    const int nt = min(TRI_WG, nbs - j0);
    __syncthreads();                             // the tile before this one has been walked
    for (int k = threadIdx.x; k < nt * TRI_SEGB; k += TRI_WG) s_b[k] = segb[(size_t)(b0 + j0) * TRI_SEGB + k];
    __syncthreads();
    if ((int)threadIdx.x < nt) {
      double* q = s_b + TRI_SEGB * threadIdx.x;
      q[3] = ((q[0] * w.C[0] + q[1] * w.C[1]) + q[2] * w.C[2]) + q[3];
    }
    __syncthreads();
    if (!live) continue;
    for (int jj = 0; jj < nt; ++jj) {
      double s1, s2;
      if (!tri_pair(s_b + TRI_SEGB * jj, d1, d2, n, w, cos_min, overlap_min, &s1, &s2)) continue;
      if (FILL) {
        if (at >= (size_t)H) break;              // never taken: the two passes decide alike; the list's end is a bound all the same
        hyp_m[at] = m; hyp_j[at] = j0 + jj; hyp_s[2 * at] = s1; hyp_s[2 * at + 1] = s2; ++at;
      } else ++count;
    }
  }
  if (!FILL && live) cnt[(size_t)g * M + m] = count;
}

// one workgroup: off = the exclusive scan of cnt [S M] (clamped to an int: a total beyond one is refused by the host before the fill),
// hoff [S + 1] = the segments' first hypotheses, *total = the exact count
__global__ __launch_bounds__(1024) void tri_scan_kernel(int S, int M, const int* __restrict__ cnt, int* __restrict__ off, int* __restrict__ hoff,
                                                        long long* __restrict__ total) {
  __shared__ int s_wave[16];
  const long long tot = block_carry_scan(S * M, [&](int i) { return cnt[i]; },
                                         [&](int i, long long e) {
                                           const int c = (int)(e < (long long)INT_MAX ? e : (long long)INT_MAX);
                                           off[i] = c;
                                           if (i % M == 0) hoff[i / M] = c;
                                         }, s_wave);
  if (threadIdx.x == 0) { hoff[S] = (int)(tot < (long long)INT_MAX ? tot : (long long)INT_MAX); *total = tot; }
}

// ---- one wavefront per 2-D segment: lanes over its hypotheses h (striding beyond 64), each walking all h' in list order with a running
// minimum of the exponent per slot (the largest similarity of a slot is the exp of minus its least exponent: one exp a slot, not one
// a pair), added in slot order (the list is in slot order).  The estimate is the arg-max, the lowest index on a tie
__global__ __launch_bounds__(TRI_WG) void tri_score_kernel(int S, const int* __restrict__ view, const int* __restrict__ hoff,
                                                           const int* __restrict__ hyp_m, const double* __restrict__ hyp_s,
                                                           const double* __restrict__ cam, const double* __restrict__ sega, double sigma_px,
                                                           double min_score, int* __restrict__ best, double* __restrict__ estimate,
                                                           double* __restrict__ score, double* __restrict__ radius, int* __restrict__ kept) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, g = blockIdx.x * TRI_WAVES + (threadIdx.x >> 6);
  if (g >= S) return;                            // whole wavefronts leave; the kernel has no barrier
  // the same for the whole wavefront, and said so: the walk over h' then reads through the scalar cache
  const int h0 = __builtin_amdgcn_readfirstlane(hoff[g]), nh = __builtin_amdgcn_readfirstlane(hoff[g + 1]) - h0;
  const double* c = cam + (size_t)TRI_CAM * view[g];
  const double f = c[TRI_K];
  double bs = -1.0;
  int bh = INT_MAX;
  for (int h = lane; h < nh; h += 64) {
    const int m = hyp_m[h0 + h];
    const double s1 = hyp_s[2 * (size_t)(h0 + h)], s2 = hyp_s[2 * (size_t)(h0 + h) + 1];
    const double g1 = (sigma_px * s1) / f, g2 = (sigma_px * s2) / f;
    const double w1 = 1.0 / (2.0 * (g1 * g1)), w2 = 1.0 / (2.0 * (g2 * g2));      // once a hypothesis: the pair loop has no division
    double sc = 0.0, cur = INFINITY;             // cur: the least exponent of the slot; its exp is the slot's largest similarity
    int slot = -1;
    for (int hp = 0; hp < nh; ++hp) {
      const int mp = hyp_m[h0 + hp];
      if (mp != slot) {
        if (slot >= 0 && slot != m) sc = sc + exp(-cur);
        slot = mp; cur = INFINITY;
      }
      if (mp == m) continue;
      const double e1 = s1 - hyp_s[2 * (size_t)(h0 + hp)], e2 = s2 - hyp_s[2 * (size_t)(h0 + hp) + 1];
      cur = fmin(cur, (e1 * e1) * w1 + (e2 * e2) * w2);
    }
    if (slot >= 0 && slot != m) sc = sc + exp(-cur);
    if (sc > bs) { bs = sc; bh = h; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double os = __shfl_xor(bs, o);
    const int oh = __shfl_xor(bh, o);
    if (os > bs || (os == bs && oh < bh)) { bs = os; bh = oh; }
  }
  if (lane != 0) return;
  double* E = estimate + 6 * (size_t)g;
  if (nh == 0) {
#pragma unroll
    for (int q = 0; q < 6; ++q) E[q] = 0.0;
    best[g] = -1; score[g] = 0.0; radius[g] = 0.0; kept[g] = 0;
    return;
  }
  const double* A = sega + (size_t)TRI_SEGA * g;
  double r = 0.0;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const double s = hyp_s[2 * (size_t)(h0 + bh) + k];
#pragma unroll
    for (int q = 0; q < 3; ++q) E[3 * k + q] = c[TRI_C + q] + s * A[3 * k + q];
    r = fmax(r, ((sigma_px * s) / f) * tri_norm3(A[3 * k], A[3 * k + 1], A[3 * k + 2]));
  }
  best[g] = h0 + bh; score[g] = bs; radius[g] = r;
  kept[g] = bs >= min_score ? 1 : 0;
}

// ---- the link graph over the kept estimates.  parent = the output label array: a kept estimate starts as its own root
__global__ __launch_bounds__(TRI_WG) void tri_link_init_kernel(int S, const int* __restrict__ kept, int* __restrict__ parent, int* __restrict__ last) {
  const int g = blockIdx.x * TRI_WG + threadIdx.x;
  if (g >= S) return;
  parent[g] = kept[g] ? g : -1;
  last[g] = -1;
}

// distance of point p to the infinite line through a and b
__device__ __forceinline__ double tri_line_dist(const double* p, const double* a, const double* b) {
#pragma clang fp contract(off)
  const double w0 = p[0] - a[0], w1 = p[1] - a[1], w2 = p[2] - a[2], d0 = b[0] - a[0], d1 = b[1] - a[1], d2 = b[2] - a[2];
  return tri_norm3(w1 * d2 - w2 * d1, w2 * d0 - w0 * d2, w0 * d1 - w1 * d0) / tri_norm3(d0, d1, d2);
}

__device__ __forceinline__ bool tri_linked(const double* e, const double* f, double re, double rf) {
#pragma clang fp contract(off)
  const double tol = 2.0 * fmax(re, rf);
  return tri_line_dist(f, e, e + 3) <= tol && tri_line_dist(f + 3, e, e + 3) <= tol && tri_line_dist(e, f, f + 3) <= tol &&
         tri_line_dist(e + 3, f, f + 3) <= tol;
}

// one wavefront per kept estimate, lanes over the partners of all its hypotheses
__global__ __launch_bounds__(TRI_WG) void tri_link_kernel(int S, int M, const int* __restrict__ view, const int* __restrict__ segoff,
                                                          const int* __restrict__ nb, const int* __restrict__ hoff, const int* __restrict__ hyp_m,
                                                          const int* __restrict__ hyp_j, const int* __restrict__ kept,
                                                          const double* __restrict__ estimate, const double* __restrict__ radius, int* parent) {
  const int lane = threadIdx.x & 63, g = blockIdx.x * TRI_WAVES + (threadIdx.x >> 6);
  if (g >= S || !kept[g]) return;
  const int h0 = hoff[g], nh = hoff[g + 1] - h0, a = view[g];
  for (int h = lane; h < nh; h += 64) {
    const int p = segoff[nb[a * M + hyp_m[h0 + h]]] + hyp_j[h0 + h];
    if (kept[p] && tri_linked(estimate + 6 * (size_t)g, estimate + 6 * (size_t)p, radius[g], radius[p]))
      uf_union<__HIP_MEMORY_SCOPE_AGENT>(parent, g, p);
  }
}

// ---- one wavefront per component, at its root r (uf_flatten_kernel has made label = the root = the lowest estimate, last[root] = the
// highest): its members are the g in [r, last[r]] with label r, met in ascending order (which is view order) 64 at a time.  Distinct
// views = the changes of view along them; the axis = the best score, lowest index on a tie; tau = the extent of all members' end
// points along the axis
__global__ __launch_bounds__(TRI_WG) void tri_component_kernel(int S, const int* __restrict__ label, const int* __restrict__ last,
                                                               const int* __restrict__ view, const double* __restrict__ score,
                                                               const double* __restrict__ estimate, int* __restrict__ nviews,
                                                               int* __restrict__ axis, double* __restrict__ tau) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, r = blockIdx.x * TRI_WAVES + (threadIdx.x >> 6);
  if (r >= S || label[r] != r) return;
  const int end = last[r];
  int nv = 0, prev = -1, ba = INT_MAX;
  double bs = -1.0;
  for (int g0 = r; g0 <= end; g0 += 64) {
    const int g = g0 + lane;
    const bool mine = g <= end && label[g] == r;
    const int vw = mine ? view[g] : -1;
    const unsigned long long bal = __ballot(mine), below = bal & ((1ull << lane) - 1ull);
    const int pl = below ? 63 - __clzll((long long)below) : -1;
    const int sv = __shfl(vw, pl < 0 ? 0 : pl);
    const int pv = pl < 0 ? prev : sv;
    nv += __popcll(__ballot(mine && vw != pv));
    if (bal) prev = __shfl(vw, 63 - __clzll((long long)bal));
    if (mine) { const double sc = score[g]; if (sc > bs) { bs = sc; ba = g; } }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double os = __shfl_xor(bs, o);
    const int oa = __shfl_xor(ba, o);
    if (os > bs || (os == bs && oa < ba)) { bs = os; ba = oa; }
  }
  if (ba > end) ba = r;                          // never taken: a kept score is no less than 0
  const double* A = estimate + 6 * (size_t)ba;
  const double b0 = A[3] - A[0], b1 = A[4] - A[1], b2 = A[5] - A[2], bn = tri_norm3(b0, b1, b2);
  const double u0 = b0 / bn, u1 = b1 / bn, u2 = b2 / bn;
  double lo = INFINITY, hi = -INFINITY;
  wave_members_each(label, r, end, lane, [&](int g) {
#pragma clang fp contract(off)
    const double* E = estimate + 6 * (size_t)g;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const double t = ((E[3 * k] - A[0]) * u0 + (E[3 * k + 1] - A[1]) * u1) + (E[3 * k + 2] - A[2]) * u2;
      lo = fmin(lo, t); hi = fmax(hi, t);
    }
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { lo = fmin(lo, __shfl_xor(lo, o)); hi = fmax(hi, __shfl_xor(hi, o)); }
  if (lane == 0) { nviews[r] = nv; axis[r] = ba; tau[2 * (size_t)r] = lo; tau[2 * (size_t)r + 1] = hi; }
}

// ---- one workgroup: the components with min_views views at least, in label order -> the lines; members [S] = a segment's line, -1 for none
__global__ __launch_bounds__(1024) void tri_output_kernel(int S, int min_views, const int* __restrict__ label, const int* __restrict__ nviews,
                                                          const int* __restrict__ axis, const double* __restrict__ tau,
                                                          const double* __restrict__ estimate, const double* __restrict__ score,
                                                          int* __restrict__ idx, int* members, double* __restrict__ lines3d,
                                                          int* __restrict__ views, double* __restrict__ support, int* __restrict__ n_lines) {
#pragma clang fp contract(off)
  __shared__ int s_wave[16], s_base;
  const int N = block_compact(S, [&](int g) { return label[g] == g && nviews[g] >= min_views; }, idx, s_wave, &s_base);
  for (int g = threadIdx.x; g < S; g += blockDim.x) members[g] = -1;
  __syncthreads();
  for (int q = threadIdx.x; q < N; q += blockDim.x) {
    const int r = idx[q], a = axis[r];
    const double* A = estimate + 6 * (size_t)a;
    const double b0 = A[3] - A[0], b1 = A[4] - A[1], b2 = A[5] - A[2], bn = tri_norm3(b0, b1, b2);
    const double u[3] = {b0 / bn, b1 / bn, b2 / bn};
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c) lines3d[6 * (size_t)q + 3 * k + c] = A[c] + tau[2 * (size_t)r + k] * u[c];
    views[q] = nviews[r];
    support[q] = score[a];
    members[r] = q;
  }
  __syncthreads();
  for (int g = threadIdx.x; g < S; g += blockDim.x) {
    const int l = label[g];
    if (l >= 0 && l != g) members[g] = members[l];
  }
  if (threadIdx.x == 0) *n_lines = N;
}

}  // namespace neat
