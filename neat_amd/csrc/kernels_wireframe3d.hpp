// 3-D wireframes with shared junctions from the triangulated lines and the views' 2-D graphs (neat_amd/triangulate.py wireframe; the rule:
// DESIGN 3p, restated in float64 by tests/wireframe3d_f64.py).  A 3-D line end inherits the 2-D vertices of its member segments' ends;
// two ends of different lines that share a 2-D vertex in enough views, and whose lines nearly cross there, are linked; a component of
// two ends or more becomes one junction at the least-squares point of its members' lines; the lines between distinct vertices, one per
// vertex pair, are the edges.
//
// Float64 throughout, contraction into fused multiply-adds off in every function that forms a value the reference forms: every product,
// sum and quotient is the reference's, one IEEE operation each in the order written here.  No transcendental function; the one square
// root is the spread's.  Nothing depends on an order of execution: the lists are sorted keys (rocprim's radix sort, in neat_aux.hip)
// that are counted, scanned and filled in order; the components are a union-find with atomicMin whose roots are the smallest member; the
// other atomics are integer atomicMax; a junction's sums run in ascending end order in every lane.  Two runs give the same bytes.
//
// End e of line L is end id q = 2 L + e, below 2^24.  A record is (2-D vertex << 32) | q, one per segment end that lies at a line end; a
// pair key is (q << 40) | (q' << 16) | view, q < q' of different lines, one per pair of distinct records of one 2-D vertex.  ~0 marks an
// unused key of either list and sorts behind every used one.
#pragma once
#include <float.h>
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stddef.h>

#include "block_util.hpp"           // block_carry_scan
#include "graph_util.hpp"           // uf_union, uf_flatten_kernel, wave_members, count_scan_kernel

namespace neat {

constexpr int WF3_WG = 256;
constexpr int WF3_WAVES = WF3_WG / 64;           // component kernel: one wavefront per end id
constexpr unsigned long long WF3_NONE = ~0ull;

typedef unsigned long long wf3_key;

__device__ __forceinline__ double wf3_dot(double ax, double ay, double az, double bx, double by, double bz) {
#pragma clang fp contract(off)
  return (ax * bx + ay * by) + az * bz;
}

// ---- per end id: its own root; no link yet
__global__ __launch_bounds__(WF3_WG) void wf3_init_kernel(int n2, int* __restrict__ parent, int* __restrict__ last, int* __restrict__ lvotes) {
  const int e = blockIdx.x * WF3_WG + threadIdx.x;
  if (e >= n2) return;
  parent[e] = e; last[e] = e; lvotes[e] = 0;
}

// ---- per segment: the record of each end (WF3_NONE for an end that carries nothing), and the view of its 2-D vertices
__global__ __launch_bounds__(WF3_WG) void wf3_ends_kernel(const double* __restrict__ lines3d, int N, const int* __restrict__ members,
                                                          const double* __restrict__ estimate, const int* __restrict__ endv,
                                                          const int* __restrict__ view, int V, int S, int NV, double end_frac,
                                                          wf3_key* __restrict__ rkey, int* vview) {
#pragma clang fp contract(off)
  const int g = blockIdx.x * WF3_WG + threadIdx.x;
  if (g >= S) return;
  const int L = members[g], a = view[g];
  const bool ok = L >= 0 && L < N && a >= 0 && a < V;
  double A[3] = {0.0, 0.0, 0.0}, u[3] = {0.0, 0.0, 0.0};
  if (ok) {
#pragma unroll
    for (int c = 0; c < 3; ++c) { A[c] = lines3d[6 * (size_t)L + c]; u[c] = lines3d[6 * (size_t)L + 3 + c] - A[c]; }
  }
  const double uu = wf3_dot(u[0], u[1], u[2], u[0], u[1], u[2]), hi = 1.0 - end_frac;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int gv = endv[2 * (size_t)g + k];
    wf3_key key = WF3_NONE;
    if (ok && gv >= 0 && gv < NV) {
      atomicMax(vview + gv, a);
      const double* P = estimate + 6 * (size_t)g + 3 * k;
      const double tau = wf3_dot(P[0] - A[0], P[1] - A[1], P[2] - A[2], u[0], u[1], u[2]) / uu;
      if (tau <= end_frac) key = ((wf3_key)gv << 32) | (wf3_key)(2 * L);
      else if (tau >= hi) key = ((wf3_key)gv << 32) | (wf3_key)(2 * L + 1);
    }
    rkey[2 * (size_t)g + k] = key;
  }
}

// The pairs a sorted record i starts: it is the first of its equals, and every later distinct record of its 2-D vertex with another line
// is one pair.  emit(q', c) is called for the c-th of them in order; returns their number
template <class E>
__device__ __forceinline__ int wf3_walk_records(const wf3_key* __restrict__ rs, int n, int i, E emit) {
  const wf3_key key = rs[i];
  if (key == WF3_NONE || (i > 0 && rs[i - 1] == key)) return 0;
  const unsigned q = (unsigned)key;
  int c = 0;
  for (int j = i + 1; j < n && (rs[j] >> 32) == (key >> 32); ++j) {
    if (rs[j] == rs[j - 1]) continue;
    const unsigned p = (unsigned)rs[j];
    if ((p >> 1) != (q >> 1)) emit(p, c++);
  }
  return c;
}

__global__ __launch_bounds__(WF3_WG) void wf3_pair_count_kernel(const wf3_key* __restrict__ rs, int n, int* __restrict__ rcnt) {
  const int i = blockIdx.x * WF3_WG + threadIdx.x;
  if (i >= n) return;
  rcnt[i] = wf3_walk_records(rs, n, i, [](unsigned, int) {});
}

// the pair keys, once count_scan_kernel has made roff [n] = the pairs before each record and *total = all of them: at most pairs_max
// keys (the rest of pkey stays WF3_NONE; the total tells the host that some were left out)
__global__ __launch_bounds__(WF3_WG) void wf3_pair_fill_kernel(const wf3_key* __restrict__ rs, int n, const long long* __restrict__ roff,
                                                               const int* __restrict__ vview, int NV, long long pairs_max, wf3_key* __restrict__ pkey) {
  const int i = blockIdx.x * WF3_WG + threadIdx.x;
  if (i >= n) return;
  const wf3_key key = rs[i];
  if (key == WF3_NONE) return;
  const int gv = (int)(key >> 32);
  if (gv < 0 || gv >= NV) return;
  const wf3_key head = ((wf3_key)(unsigned)key << 40) | (wf3_key)(vview[gv] & 0xffff);
  const long long first = roff[i];
  wf3_walk_records(rs, n, i, [&](unsigned p, int c) {
    if (first + c < pairs_max) pkey[first + c] = head | ((wf3_key)p << 16);
  });
}

// ---- per sorted pair key that starts a run of one (q, q'): the distinct views along the run are its votes; with enough of them the
// geometry test, and the link
__global__ __launch_bounds__(WF3_WG) void wf3_link_kernel(const wf3_key* __restrict__ ps, long long n, const double* __restrict__ lines3d, int N,
                                                          int min_votes, double reach, double sin_min, int* parent, int* lvotes) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * WF3_WG + threadIdx.x;
  if (i >= n) return;
  const wf3_key key = ps[i];
  if (key == WF3_NONE || (i > 0 && (ps[i - 1] >> 16) == (key >> 16))) return;
  int votes = 1;
  for (long long j = i + 1; j < n && (ps[j] >> 16) == (key >> 16); ++j) votes += ps[j] != ps[j - 1] ? 1 : 0;
  if (votes < min_votes) return;
  const int q0 = (int)(key >> 40), q1 = (int)((key >> 16) & 0xffffff);
  if (q0 >= 2 * N || q1 >= 2 * N) return;
  const double* P = lines3d + 6 * (size_t)(q0 >> 1);
  const double* Q = lines3d + 6 * (size_t)(q1 >> 1);
  const double ux = P[3] - P[0], uy = P[4] - P[1], uz = P[5] - P[2];
  const double vx = Q[3] - Q[0], vy = Q[4] - Q[1], vz = Q[5] - Q[2];
  const double a = wf3_dot(ux, uy, uz, ux, uy, uz), b = wf3_dot(ux, uy, uz, vx, vy, vz), c = wf3_dot(vx, vy, vz, vx, vy, vz);
  const double rx = Q[0] - P[0], ry = Q[1] - P[1], rz = Q[2] - P[2];
  const double d = wf3_dot(ux, uy, uz, rx, ry, rz), e_ = wf3_dot(vx, vy, vz, rx, ry, rz);
  const double wx = uy * vz - uz * vy, wy = uz * vx - ux * vz, wz = ux * vy - uy * vx;
  const double ww = wf3_dot(wx, wy, wz, wx, wy, wz);
  if (ww < (sin_min * sin_min) * (a * c)) return;
  const double den = a * c - b * b;
  const double s = (c * d - b * e_) / den, t = (b * d - a * e_) / den;
  const double dx = (P[0] + s * ux) - (Q[0] + t * vx), dy = (P[1] + s * uy) - (Q[1] + t * vy), dz = (P[2] + s * uz) - (Q[2] + t * vz);
  const double delta2 = wf3_dot(dx, dy, dz, dx, dy, dz);
  const double least = a < c ? a : c;
  if (!(fabs(s - (double)(q0 & 1)) <= reach && fabs(t - (double)(q1 & 1)) <= reach && delta2 <= (reach * reach) * least)) return;
  uf_union<__HIP_MEMORY_SCOPE_AGENT>(parent, q0, q1);
  atomicMax(lvotes + q0, votes);
  atomicMax(lvotes + q1, votes);
}

// one workgroup: vidx [2 N] = the roots before each end id = a root's place in the vertex list; *n_vertices = their number
__global__ __launch_bounds__(1024) void wf3_vertex_scan_kernel(int n2, const int* __restrict__ label, int* __restrict__ vidx, int* __restrict__ n_vertices) {
  __shared__ int s_wave[16];
  const long long tot = block_carry_scan(n2, [&](int e) { return label[e] == e ? 1 : 0; }, [&](int e, long long x) { vidx[e] = (int)x; }, s_wave);
  if (threadIdx.x == 0) *n_vertices = (int)tot;
}

// ---- one wavefront per vertex, at its root r (uf_flatten_kernel has made label = the root, last[root] = the highest member): its
// members are the end ids in [r, last[r]] with label r (wave_members); every lane adds the sums of all of them in ascending order, so all
// lanes hold the same bits
__global__ __launch_bounds__(WF3_WG) void wf3_vertex_kernel(int n2, const int* __restrict__ label, const int* __restrict__ last,
                                                            const int* __restrict__ vidx, const int* __restrict__ lvotes,
                                                            const double* __restrict__ lines3d, double* __restrict__ vertices,
                                                            int* __restrict__ degree, int* __restrict__ kind, int* __restrict__ votes,
                                                            double* __restrict__ spread) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, r = blockIdx.x * WF3_WAVES + (threadIdx.x >> 6);
  if (r >= n2 || label[r] != r) return;          // whole wavefronts leave; the kernel has no barrier
  const int end = last[r], slot = vidx[r];
  if (end == r) {                                // a free end stays where it is
    if (lane == 0) {
      const double* E = lines3d + 3 * (size_t)r;
      vertices[3 * (size_t)slot] = E[0]; vertices[3 * (size_t)slot + 1] = E[1]; vertices[3 * (size_t)slot + 2] = E[2];
      degree[slot] = 1; kind[slot] = 0; votes[slot] = 0; spread[slot] = 0.0;
    }
    return;
  }
  double m00 = 0.0, m01 = 0.0, m02 = 0.0, m11 = 0.0, m12 = 0.0, m22 = 0.0, y0 = 0.0, y1 = 0.0, y2 = 0.0, sx = 0.0, sy = 0.0, sz = 0.0;
  int vt = 0;
  const int m = wave_members(label, r, end, lane, [&](int e) { vt = max(vt, lvotes[e]); }, [&](int q) {
#pragma clang fp contract(off)
    const double* A = lines3d + 6 * (size_t)(q >> 1);
    const double ux = A[3] - A[0], uy = A[4] - A[1], uz = A[5] - A[2];
    const double uu = wf3_dot(ux, uy, uz, ux, uy, uz);
    const double p00 = 1.0 - (ux * ux) / uu, p01 = -((ux * uy) / uu), p02 = -((ux * uz) / uu);
    const double p11 = 1.0 - (uy * uy) / uu, p12 = -((uy * uz) / uu), p22 = 1.0 - (uz * uz) / uu;
    m00 = m00 + p00; m01 = m01 + p01; m02 = m02 + p02; m11 = m11 + p11; m12 = m12 + p12; m22 = m22 + p22;
    y0 = y0 + ((p00 * A[0] + p01 * A[1]) + p02 * A[2]);
    y1 = y1 + ((p01 * A[0] + p11 * A[1]) + p12 * A[2]);
    y2 = y2 + ((p02 * A[0] + p12 * A[1]) + p22 * A[2]);
    const double* E = A + 3 * (q & 1);
    sx = sx + E[0]; sy = sy + E[1]; sz = sz + E[2];
  });
  const double c00 = m11 * m22 - m12 * m12, c01 = m02 * m12 - m01 * m22, c02 = m01 * m12 - m02 * m11;
  const double c11 = m00 * m22 - m02 * m02, c12 = m01 * m02 - m00 * m12, c22 = m00 * m11 - m01 * m01;
  const double det = (m00 * c00 + m01 * c01) + m02 * c02;
  double X, Y, Z;
  if (det > 0.0 && det <= DBL_MAX) {
    X = ((c00 * y0 + c01 * y1) + c02 * y2) / det; Y = ((c01 * y0 + c11 * y1) + c12 * y2) / det; Z = ((c02 * y0 + c12 * y1) + c22 * y2) / det;
  } else {
    const double n = (double)m;
    X = sx / n; Y = sy / n; Z = sz / n;
  }
  double sp = 0.0;
  wave_members_each(label, r, end, lane, [&](int e) {
#pragma clang fp contract(off)
    const double* E = lines3d + 3 * (size_t)e;
    const double dx = X - E[0], dy = Y - E[1], dz = Z - E[2];
    sp = fmax(sp, sqrt(wf3_dot(dx, dy, dz, dx, dy, dz)));
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { vt = max(vt, __shfl_xor(vt, o)); sp = fmax(sp, __shfl_xor(sp, o)); }
  if (lane != 0) return;
  vertices[3 * (size_t)slot] = X; vertices[3 * (size_t)slot + 1] = Y; vertices[3 * (size_t)slot + 2] = Z;
  degree[slot] = m; kind[slot] = 1; votes[slot] = vt; spread[slot] = sp;
}

// ---- per line: its two vertices, and the key (lower vertex, higher vertex) of the line as an edge; WF3_NONE when both ends are one vertex
__global__ __launch_bounds__(WF3_WG) void wf3_edge_key_kernel(int N, const int* __restrict__ label, const int* __restrict__ vidx,
                                                              wf3_key* __restrict__ ekey, int* __restrict__ eline, int* __restrict__ keep) {
  const int L = blockIdx.x * WF3_WG + threadIdx.x;
  if (L >= N) return;
  const int v0 = vidx[label[2 * L]], v1 = vidx[label[2 * L + 1]];
  ekey[L] = v0 == v1 ? WF3_NONE : ((wf3_key)min(v0, v1) << 32) | (wf3_key)max(v0, v1);
  eline[L] = L;
  keep[L] = 0;
}

// per sorted edge key that starts a run: the run's line of the largest support stays, the lowest index on a tie
__global__ __launch_bounds__(WF3_WG) void wf3_edge_pick_kernel(int N, const wf3_key* __restrict__ es, const int* __restrict__ ls,
                                                               const double* __restrict__ support, int* __restrict__ keep) {
  const int i = blockIdx.x * WF3_WG + threadIdx.x;
  if (i >= N) return;
  const wf3_key key = es[i];
  if (key == WF3_NONE || (i > 0 && es[i - 1] == key)) return;
  int best = ls[i];
  double bs = support[best];
  for (int j = i + 1; j < N && es[j] == key; ++j) {
    const int L = ls[j];
    const double s = support[L];
    if (s > bs || (s == bs && L < best)) { best = L; bs = s; }
  }
  keep[best] = 1;
}

// one workgroup: eidx [N] = the edges before each line; the two counts.  More pairs than the workspace holds: n_vertices = -1 and
// n_edges = the pairs there are (capped at INT_MAX), for the host to call again
__global__ __launch_bounds__(1024) void wf3_edge_scan_kernel(int N, const int* __restrict__ keep, int* __restrict__ eidx, const long long* __restrict__ total,
                                                             long long pairs_max, int* __restrict__ n_vertices, int* __restrict__ n_edges) {
  __shared__ int s_wave[16];
  const long long tot = block_carry_scan(N, [&](int L) { return keep[L]; }, [&](int L, long long x) { eidx[L] = (int)x; }, s_wave);
  if (threadIdx.x != 0) return;
  const long long pairs = *total;
  if (pairs > pairs_max) { *n_vertices = -1; *n_edges = (int)(pairs < INT_MAX ? pairs : INT_MAX); }
  else *n_edges = (int)tot;
}

__global__ __launch_bounds__(WF3_WG) void wf3_edge_fill_kernel(int N, const int* __restrict__ keep, const int* __restrict__ eidx,
                                                               const int* __restrict__ label, const int* __restrict__ vidx,
                                                               int* __restrict__ edges, int* __restrict__ esrc) {
  const int L = blockIdx.x * WF3_WG + threadIdx.x;
  if (L >= N || !keep[L]) return;
  const int slot = eidx[L];
  edges[2 * (size_t)slot] = vidx[label[2 * L]]; edges[2 * (size_t)slot + 1] = vidx[label[2 * L + 1]];
  esrc[slot] = L;
}

}  // namespace neat
