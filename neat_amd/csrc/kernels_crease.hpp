// Crease lines of a triangle mesh (neat_amd/creases.py): the junctions and straight edges of a model, read from its triangles alone,
// in the format of a scene's lines.json.  DESIGN 3n states the rule, tests/creases_f64.py restates it in float64 numpy, and the device
// equals it array for array.  Every decision is float64 products and sums in the written order, every product rounded on its own
// (rounded(), contraction off); no division, square root or trigonometric function runs here: the host hands over cos(angle),
// sin^2(turn) and the deviation as a length.
//
// Three calls share one workspace (crease_layout, ws_layout.hpp); each is sorts (rocprim, stable), per-element kernels and scans:
//   edges   weld (three stable sorts of the coordinate bits z, y, x; the first of a group is its lowest index), faces (normal n and
//           q = n.n, dropped when two welded ids agree or q == 0), half-edges (key lo << 32 | hi, value 3 f + corner; one stable sort),
//           kinds at the first half-edge of each key, the feature edges compacted in key order.
//   chains  incidences (vertex << 32 | edge, sorted) -> every vertex of a feature edge is an end or passed through; the two edges of a
//           passed-through vertex are united (the smaller root wins, so the label is the chain's lowest edge); edges sorted by label;
//           one wavefront per chain decides whether it is one straight line; lines per chain and junction flags counted and scanned.
//   fill    the lines written chain by chain, sorted by (kind, curved) and then stably by (a, b), re-indexed into the junction list.
// The only atomic is the union-find's integer fetch-min (uf_union, graph_util.hpp); everything else is a plain vector store,
// and where several lanes store to one word they store the same value.  Two runs give the same bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "device_util.hpp"     // rounded
#include "graph_util.hpp"      // uf_find, uf_union; the tiled scan

namespace neat {

constexpr int CR_WG = 256;
constexpr int CR_WAVES = CR_WG / 64;
constexpr unsigned long long CR_KEY_NONE = ~0ull;      // the half-edges of a dropped face: they sort last

__device__ __forceinline__ double cr_dot(double ax, double ay, double az, double bx, double by, double bz) {
#pragma clang fp contract(off)
  return (rounded(ax * bx) + rounded(ay * by)) + rounded(az * bz);
}
// |a x b|^2
__device__ __forceinline__ double cr_cross2(double ax, double ay, double az, double bx, double by, double bz) {
#pragma clang fp contract(off)
  const double cx = rounded(ay * bz) - rounded(az * by);
  const double cy = rounded(az * bx) - rounded(ax * bz);
  const double cz = rounded(ax * by) - rounded(ay * bx);
  return cr_dot(cx, cy, cz, cx, cy, cz);
}
__device__ __forceinline__ int cr_lo32(unsigned long long k) { return (int)(unsigned)(k & 0xffffffffull); }
__device__ __forceinline__ int cr_hi32(unsigned long long k) { return (int)(unsigned)(k >> 32); }
__device__ __forceinline__ unsigned long long cr_pack(int hi, int lo) { return ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo; }

// ---- the refusals: status = 1 for a face index outside the vertices, 2 for a non-finite coordinate (every writer of one launch stores the same value)
__global__ __launch_bounds__(CR_WG) void crease_check_kernel(const double* __restrict__ verts, int nv, const int* __restrict__ faces, int nf,
                                                            int* __restrict__ status) {
  const size_t i = (size_t)blockIdx.x * CR_WG + threadIdx.x;
  if (i < 3 * (size_t)nf && (faces[i] < 0 || faces[i] >= nv)) status[0] = 1;
  if (i < 3 * (size_t)nv && !isfinite(verts[i])) status[1] = 2;
}

// ---- weld.  The key of a round is the bit pattern of one coordinate (-0.0 as 0.0) of the vertex that stands at this place so far
__global__ __launch_bounds__(CR_WG) void crease_vkey_kernel(const double* __restrict__ verts, int nv, int axis, const int* __restrict__ order,
                                                           unsigned long long* __restrict__ key, int* __restrict__ val) {
  const int i = blockIdx.x * CR_WG + threadIdx.x;
  if (i >= nv) return;
  const int v = order ? order[i] : i;
  const double x = verts[3 * (size_t)v + axis];
  key[i] = (unsigned long long)__double_as_longlong(x == 0.0 ? 0.0 : x);
  val[i] = v;
}
// head[i] = the vertex at place i of the sorted order starts a group (finite coordinates: == is bit equality but for the zeros)
__global__ __launch_bounds__(CR_WG) void crease_vhead_kernel(const double* __restrict__ verts, int nv, const int* __restrict__ order,
                                                            int* __restrict__ head) {
  const int i = blockIdx.x * CR_WG + threadIdx.x;
  if (i >= nv) return;
  int h = 1;
  if (i > 0) {
    const double* a = verts + 3 * (size_t)order[i];
    const double* b = verts + 3 * (size_t)order[i - 1];
    h = !(a[0] == b[0] && a[1] == b[1] && a[2] == b[2]);
  }
  head[i] = h;
}
__global__ __launch_bounds__(CR_WG) void crease_vrep_kernel(int nv, const int* __restrict__ order, const int* __restrict__ head,
                                                           const int* __restrict__ group, int* __restrict__ rep) {
  const int i = blockIdx.x * CR_WG + threadIdx.x;
  if (i < nv && head[i]) rep[group[i]] = order[i];
}
__global__ __launch_bounds__(CR_WG) void crease_weld_kernel(int nv, const int* __restrict__ order, const int* __restrict__ head,
                                                           const int* __restrict__ group, const int* __restrict__ rep, int* __restrict__ weld) {
  const int i = blockIdx.x * CR_WG + threadIdx.x;
  if (i < nv) weld[order[i]] = rep[group[i] + head[i] - 1];
}

// ---- faces: one lane per face.  fn [nf][4] = n, q; three half-edges, corner k from welded vertex k to k + 1
__global__ __launch_bounds__(CR_WG) void crease_face_kernel(const double* __restrict__ verts, const int* __restrict__ faces, int nf,
                                                           const int* __restrict__ weld, double* __restrict__ fn,
                                                           unsigned long long* __restrict__ key, int* __restrict__ val) {
#pragma clang fp contract(off)
  const int f = blockIdx.x * CR_WG + threadIdx.x;
  if (f >= nf) return;
  int w[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) w[k] = weld[faces[3 * (size_t)f + k]];
  const double* a = verts + 3 * (size_t)w[0];
  const double* b = verts + 3 * (size_t)w[1];
  const double* c = verts + 3 * (size_t)w[2];
  const double e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2];
  const double e2x = c[0] - a[0], e2y = c[1] - a[1], e2z = c[2] - a[2];
  const double nx = rounded(e1y * e2z) - rounded(e1z * e2y);
  const double ny = rounded(e1z * e2x) - rounded(e1x * e2z);
  const double nz = rounded(e1x * e2y) - rounded(e1y * e2x);
  const double q = cr_dot(nx, ny, nz, nx, ny, nz);
  const bool keep = w[0] != w[1] && w[1] != w[2] && w[2] != w[0] && q != 0.0;
  *reinterpret_cast<double4*>(fn + 4 * (size_t)f) = make_double4(nx, ny, nz, q);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int p = w[k], r = w[(k + 1) % 3];
    key[3 * (size_t)f + k] = keep ? cr_pack(p < r ? p : r, p < r ? r : p) : CR_KEY_NONE;
    val[3 * (size_t)f + k] = 3 * f + k;
  }
}

// ---- kinds: one lane per sorted half-edge.  mark[i] = 1 + kind at the first half-edge of a kept edge, else 0; *halves = the number of
// half-edges of kept faces (its one writer is the last of them; the host has zeroed it)
__global__ __launch_bounds__(CR_WG) void crease_kind_kernel(const unsigned long long* __restrict__ key, const int* __restrict__ val, int M,
                                                           const int* __restrict__ faces, const int* __restrict__ weld,
                                                           const double* __restrict__ fn, double cosa, int boundary, int* __restrict__ mark,
                                                           int* __restrict__ halves) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * CR_WG + threadIdx.x;
  if (i >= M) return;
  const unsigned long long k = key[i];
  int out = 0;
  if (k != CR_KEY_NONE) {
    if (i + 1 == M || key[i + 1] == CR_KEY_NONE) *halves = i + 1;
    if (i == 0 || key[i - 1] != k) {
      const int m = 1 + (i + 1 < M && key[i + 1] == k) + (i + 2 < M && key[i + 1] == k && key[i + 2] == k);
      if (m == 1) {
        out = boundary ? 2 : 0;
      } else if (m >= 3) {
        out = 3;
      } else {
        const int h1 = val[i], h2 = val[i + 1], lo = cr_hi32(k);
        const bool fwd1 = weld[faces[h1]] == lo, fwd2 = weld[faces[h2]] == lo;      // faces[3 f + corner]: the half-edge's first vertex
        const double4 n1 = *reinterpret_cast<const double4*>(fn + 4 * (size_t)(h1 / 3));
        const double4 n2 = *reinterpret_cast<const double4*>(fn + 4 * (size_t)(h2 / 3));
        double d = cr_dot(n1.x, n1.y, n1.z, n2.x, n2.y, n2.z);
        if (fwd1 == fwd2) d = -d;
        const double s = rounded(rounded(cosa * cosa) * rounded(n1.w * n2.w)), dd = rounded(d * d);
        const bool crease = cosa >= 0.0 ? (d < 0.0 || dd < s) : (d < 0.0 && dd > s);
        out = crease ? 1 : 0;
      }
    }
  }
  mark[i] = out;
}
__global__ __launch_bounds__(CR_WG) void crease_edge_kernel(const unsigned long long* __restrict__ key, int M, const int* __restrict__ mark,
                                                           const int* __restrict__ slot, int* __restrict__ elo, int* __restrict__ ehi,
                                                           int* __restrict__ ekind) {
  const int i = blockIdx.x * CR_WG + threadIdx.x;
  if (i >= M || !mark[i]) return;
  const int e = slot[i];
  elo[e] = cr_hi32(key[i]);
  ehi[e] = cr_lo32(key[i]);
  ekind[e] = mark[i] - 1;
}
// counts of the edges call: status, welded vertices, dropped faces, E, E of kind 0, 1, 2 ([3..6] are the scans' totals already)
__global__ void crease_edges_counts_kernel(int nf, const int* __restrict__ halves, int* __restrict__ counts) {
  counts[2] = nf - halves[0] / 3;
}

// ---- vertices of the feature edges
__global__ __launch_bounds__(CR_WG) void crease_incidence_kernel(int E, const int* __restrict__ elo, const int* __restrict__ ehi,
                                                                unsigned long long* __restrict__ key, int* __restrict__ parent) {
  const int e = blockIdx.x * CR_WG + threadIdx.x;
  if (e >= E) return;
  key[2 * (size_t)e] = cr_pack(elo[e], e);
  key[2 * (size_t)e + 1] = cr_pack(ehi[e], e);
  parent[e] = e;
}
__device__ __forceinline__ int cr_far(const int* __restrict__ elo, const int* __restrict__ ehi, int e, int v) { return elo[e] == v ? ehi[e] : elo[e]; }

// one lane per sorted incidence; the first of a vertex decides: vstate = 1 an end, 2 passed through (its two edges are then united)
__global__ __launch_bounds__(CR_WG) void crease_vertex_kernel(const unsigned long long* __restrict__ key, int n, const double* __restrict__ verts,
                                                             const int* __restrict__ elo, const int* __restrict__ ehi,
                                                             const int* __restrict__ ekind, double sin2, int* __restrict__ vstate,
                                                             int* __restrict__ parent) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * CR_WG + threadIdx.x;
  if (i >= n) return;
  const int v = cr_hi32(key[i]);
  if (i > 0 && cr_hi32(key[i - 1]) == v) return;
  const int deg = 1 + (i + 1 < n && cr_hi32(key[i + 1]) == v) + (i + 2 < n && cr_hi32(key[i + 2]) == v);
  bool pass = false;
  int e1 = 0, e2 = 0;
  if (deg == 2) {
    e1 = cr_lo32(key[i]);
    e2 = cr_lo32(key[i + 1]);
    if (ekind[e1] == ekind[e2]) {
      const double* p = verts + 3 * (size_t)v;
      const double* a = verts + 3 * (size_t)cr_far(elo, ehi, e1, v);
      const double* b = verts + 3 * (size_t)cr_far(elo, ehi, e2, v);
      const double ux = a[0] - p[0], uy = a[1] - p[1], uz = a[2] - p[2];
      const double wx = b[0] - p[0], wy = b[1] - p[1], wz = b[2] - p[2];
      const double uw = cr_dot(ux, uy, uz, wx, wy, wz);
      const double bound = rounded(sin2 * rounded(cr_dot(ux, uy, uz, ux, uy, uz) * cr_dot(wx, wy, wz, wx, wy, wz)));
      pass = uw < 0.0 && cr_cross2(ux, uy, uz, wx, wy, wz) <= bound;
    }
  }
  vstate[v] = pass ? 2 : 1;
  if (pass) uf_union<__HIP_MEMORY_SCOPE_AGENT>(parent, e1, e2);
}
__global__ __launch_bounds__(CR_WG) void crease_label_kernel(int E, int* __restrict__ parent, unsigned long long* __restrict__ key) {
  const int e = blockIdx.x * CR_WG + threadIdx.x;
  if (e < E) key[e] = cr_pack(uf_find<__HIP_MEMORY_SCOPE_AGENT>(parent, e), e);
}
__global__ __launch_bounds__(CR_WG) void crease_chain_head_kernel(const unsigned long long* __restrict__ key, int E, int* __restrict__ head) {
  const int i = blockIdx.x * CR_WG + threadIdx.x;
  if (i < E) head[i] = i == 0 || cr_hi32(key[i - 1]) != cr_hi32(key[i]);
}
// start[c] = the place of chain c's first edge, start[chains] = E
__global__ __launch_bounds__(CR_WG) void crease_chain_start_kernel(int E, const int* __restrict__ head, const int* __restrict__ slot,
                                                                  int* __restrict__ start) {
  const int i = blockIdx.x * CR_WG + threadIdx.x;
  if (i >= E) return;
  if (head[i]) start[slot[i]] = i;
  if (i == E - 1) start[slot[i] + head[i]] = E;
}

// One wavefront per chain: its end incidences (count, lowest and highest id), then the ballot over the deviation of its vertices.
// FILL = false: info [c][4] = straight, a, b, kind; nlines [c] (0 for c past the last chain); the flags of the vertices that lines end at.
// FILL = true: the lines of chain c from place off[c] on: ab = a << 32 | b, tag = kind << 1 | curved
template <bool FILL>
__global__ __launch_bounds__(CR_WG) void crease_chain_kernel(const unsigned long long* __restrict__ key, int E, const int* __restrict__ n_chains,
                                                            const int* __restrict__ start, const double* __restrict__ verts,
                                                            const int* __restrict__ elo, const int* __restrict__ ehi,
                                                            const int* __restrict__ ekind, const int* __restrict__ vstate, double dev,
                                                            int* __restrict__ info, int* __restrict__ nlines, int* __restrict__ jflag,
                                                            const int* __restrict__ off, int n_lines, unsigned long long* __restrict__ ab,
                                                            int* __restrict__ tag) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * CR_WAVES + (threadIdx.x >> 6);
  if (c >= E) return;                                          // whole wavefronts leave; the kernel has no barrier
  if (c >= *n_chains) {
    if (!FILL && lane == 0) nlines[c] = 0;
    return;
  }
  const int s = start[c], t = start[c + 1];
  if (FILL) {
    const int straight = info[4 * (size_t)c], kind = info[4 * (size_t)c + 3], o = off[c];
    if (straight) {
      if (lane == 0 && o < n_lines) { ab[o] = cr_pack(info[4 * (size_t)c + 1], info[4 * (size_t)c + 2]); tag[o] = kind << 1; }
    } else {
      for (int j = s + lane; j < t; j += 64) {
        const int e = cr_lo32(key[j]), l = o + (j - s);
        if (l < n_lines) { ab[l] = cr_pack(elo[e], ehi[e]); tag[l] = (kind << 1) | 1; }
      }
    }
    return;
  }
  int ends = 0, a = INT_MAX, b = -1;
  for (int j = s + lane; j < t; j += 64) {
    const int e = cr_lo32(key[j]);
    const int v[2] = {elo[e], ehi[e]};
#pragma unroll
    for (int k = 0; k < 2; ++k)
      if (vstate[v[k]] == 1) { ++ends; a = min(a, v[k]); b = max(b, v[k]); }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ends += __shfl_xor(ends, o);
    a = min(a, __shfl_xor(a, o));
    b = max(b, __shfl_xor(b, o));
  }
  bool straight = ends == 2 && a < b;
  if (straight) {
    const double* A = verts + 3 * (size_t)a;
    const double* B = verts + 3 * (size_t)b;
    const double dx = B[0] - A[0], dy = B[1] - A[1], dz = B[2] - A[2];
    const double bound = rounded(rounded(dev * dev) * cr_dot(dx, dy, dz, dx, dy, dz));
    for (int j0 = s; j0 < t; j0 += 64) {
      const int j = j0 + lane;
      bool ok = true;
      if (j < t) {
        const int e = cr_lo32(key[j]);
        const int v[2] = {elo[e], ehi[e]};
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const double* p = verts + 3 * (size_t)v[k];
          ok = ok && cr_cross2(p[0] - A[0], p[1] - A[1], p[2] - A[2], dx, dy, dz) <= bound;
        }
      }
      if (!__all(ok)) straight = false;
    }
  }
  if (straight) {
    if (lane == 0) { jflag[a] = 1; jflag[b] = 1; }
  } else {
    for (int j = s + lane; j < t; j += 64) {
      const int e = cr_lo32(key[j]);
      jflag[elo[e]] = 1;
      jflag[ehi[e]] = 1;
    }
  }
  if (lane == 0) {
    *reinterpret_cast<int4*>(info + 4 * (size_t)c) = make_int4(straight ? 1 : 0, straight ? a : 0, straight ? b : 0, ekind[cr_lo32(key[s])]);
    nlines[c] = straight ? 1 : t - s;
  }
}

// ---- output
__global__ __launch_bounds__(CR_WG) void crease_tagkey_kernel(int n, const int* __restrict__ tag, unsigned long long* __restrict__ key,
                                                             int* __restrict__ val) {
  const int i = blockIdx.x * CR_WG + threadIdx.x;
  if (i < n) { key[i] = (unsigned long long)tag[i]; val[i] = i; }
}
__global__ __launch_bounds__(CR_WG) void crease_abkey_kernel(int n, const int* __restrict__ order, const unsigned long long* __restrict__ ab,
                                                            unsigned long long* __restrict__ key) {
  const int i = blockIdx.x * CR_WG + threadIdx.x;
  if (i < n) key[i] = ab[order[i]];
}
__global__ __launch_bounds__(CR_WG) void crease_lines_kernel(int n, const unsigned long long* __restrict__ key, const int* __restrict__ order,
                                                            const int* __restrict__ tag, const int* __restrict__ jmap, int* __restrict__ lines,
                                                            unsigned char* __restrict__ kind, unsigned char* __restrict__ curved) {
  const int i = blockIdx.x * CR_WG + threadIdx.x;
  if (i >= n) return;
  const int t = tag[order[i]];
  *reinterpret_cast<int2*>(lines + 2 * (size_t)i) = make_int2(jmap[cr_hi32(key[i])], jmap[cr_lo32(key[i])]);
  kind[i] = (unsigned char)(t >> 1);
  curved[i] = (unsigned char)(t & 1);
}
__global__ __launch_bounds__(CR_WG) void crease_junction_kernel(const double* __restrict__ verts, int nv, const int* __restrict__ jflag,
                                                               const int* __restrict__ jmap, int n_junc, double* __restrict__ junctions,
                                                               int* __restrict__ vertex) {
  const int v = blockIdx.x * CR_WG + threadIdx.x;
  if (v >= nv || !jflag[v]) return;
  const int j = jmap[v];
  if (j >= n_junc) return;
#pragma unroll
  for (int a = 0; a < 3; ++a) junctions[3 * (size_t)j + a] = verts[3 * (size_t)v + a];
  vertex[j] = v;
}

}  // namespace neat
