// The evaluation mesh of a checkpoint (the reference's plots.get_surface_high_res_mesh / get_surface_by_grid(higher_res=True),
// code/utils/plots.py:140-316, and the second half of evaluation/eval.py:132-162, which go through trimesh on the host): the points of
// a grid in a rotated frame, the surface moments of a mesh that give that frame, affine maps and bounds of vertex rows, and the cut of a
// mesh by an axis-aligned plane.  No atomics; every sum is a fixed-shape tree, so two runs give the same bytes.
//
// Definitions (tests/evalmesh_f64.py restates them in float64):
//   oriented    node (i, j, k) has local coordinates p_a = b0_a + i step_a in float64 (two roundings; the last node exactly b1_a: the
//   points      arithmetic of mesh.linspace_f32 before its rounding to float32) and goes to x = c + R^T p:
//               x_a = float(c_a + ((R_0a p_0 + R_1a p_1) + R_2a p_2)), every product and sum rounded to float64, no contraction
//   moments     per triangle (a, b, c) relative to the origin o, in float64: A = |(b - a) x (c - a)| / 2, g = (a + b + c) / 3;
//               area A, first moment A g, second moment A / 12 (a a^T + b b^T + c c^T + 9 g g^T) (exact integrals of 1, x, x x^T);
//               a triangle with A = 0 adds nothing; one with a non-finite vertex, a non-finite area or an index outside [0, nv) adds
//               nothing and is counted, and the count comes back as the error flag
//   moment sum  leaves = runs of MOMENTS_TILE consecutive triangles: lane t adds triangles t, t + 256, ... of the run in that order, the
//               256 lane sums are added as lane t += lane t ^ 32, ^ 16, ... ^ 1 within each 64 and then ((w0 + w1) + (w2 + w3)); the
//               leaf sums are added 256 at a time in the same way, level by level, until one value is left
//   affine      row v -> ((A_r0 x + A_r1 y) + A_r2 z) + A_r3 per output r, every product and sum rounded to float64, no contraction,
//               rounded to float32 once (rows) or kept in float64 (bounds: min and max per output over the rows, NaN skipped)
//   cut         one plane: d(v) = sign ((double) v[axis] - value), value a float32; a vertex is inside iff d >= 0 (on the plane is
//               inside; NaN is outside).  A face with vertices (v0, v1, v2):
//                 three inside   kept as it is
//                 none inside    dropped
//                 one inside, i (j, k the next two in the face's order)          (i, c_ij, c_ik)
//                 two inside, o the outside one (i, j the next two in order)      (i, j, c_jo) and (i, c_jo, c_io): the quad i, j, c_jo, c_io
//                                                                                  is split along the diagonal from i, the first inside
//                                                                                  vertex after the outside one
//               c_ab = the cut vertex of the edge from inside vertex a to outside vertex b: a + t (b - a), t = d_a / (d_a - d_b) in
//               float64, rounded to float32 once, its `axis` coordinate set to `value` exactly.  One cut vertex per crossing edge, named
//               by the key a nv + b and shared by both incident faces (the mesh stays connected across the cut).
//   cut order   the old vertices that a surviving face uses as inside vertices, in their old order; then the cut vertices ascending by
//               (a, b); faces by source face, then by emitted triangle.  (The unique ascending keys, and the two exclusive scans over
//               the per-vertex use flags and the per-face counts, are int sorts / scans done by the caller between cut_count and cut_emit.)
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "block_util.hpp"        // block_sum, block_minmax
#include "device_util.hpp"       // rounded
#include "kernels_mesh.hpp"      // MeshAxes

namespace neat {

constexpr int EMESH_WG = 256;
constexpr int MOMENTS_TILE = 1024;        // triangles per workgroup of the moments' leaf pass: MOMENTS_TILE / EMESH_WG per lane
constexpr int MOMENTS_N = 11;             // area, 3 first moments, 6 second moments, the count of rejected triangles
constexpr int BOUNDS_BLOCKS = 1024;       // partial (min, max) sextuples of the bounds pass

struct Frame3 { double R[9], c[3]; };     // x = c + R^T p
struct Affine34 { double a[12]; };        // row-major [3][4]
struct CutPlane { int axis; double value, sign; };

// ---- (a) oriented grid points -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double emesh_coord64(const MeshAxes& g, int a, int i) {
#pragma clang fp contract(off)
  return i == g.n[a] - 1 ? g.b1[a] : rounded(rounded((double)i * g.step[a]) + g.b0[a]);
}
// t + ((m0 x + m1 y) + m2 z), one rounding per operation
__device__ __forceinline__ double emesh_dot3_add(double m0, double m1, double m2, double x, double y, double z, double t) {
#pragma clang fp contract(off)
  const double s = rounded(rounded(rounded(m0 * x) + rounded(m1 * y)) + rounded(m2 * z));
  return rounded(t + s);
}

__global__ __launch_bounds__(EMESH_WG) void grid_points_affine_kernel(float* __restrict__ x_fm, int ldp, long long first, int count, MeshAxes g,
                                                                      Frame3 f) {
  const int p = blockIdx.x * EMESH_WG + threadIdx.x;
  if (p >= ldp) return;
  float x = 0.f, y = 0.f, z = 0.f;
  if (p < count) {
    const long long node = first + p;
    const long long ij = node / g.n[2];
    const double p0 = emesh_coord64(g, 0, (int)(ij / g.n[1]));
    const double p1 = emesh_coord64(g, 1, (int)(ij % g.n[1]));
    const double p2 = emesh_coord64(g, 2, (int)(node % g.n[2]));
    x = (float)emesh_dot3_add(f.R[0], f.R[3], f.R[6], p0, p1, p2, f.c[0]);
    y = (float)emesh_dot3_add(f.R[1], f.R[4], f.R[7], p0, p1, p2, f.c[1]);
    z = (float)emesh_dot3_add(f.R[2], f.R[5], f.R[8], p0, p1, p2, f.c[2]);
  }
  x_fm[p] = x;
  x_fm[(size_t)ldp + p] = y;
  x_fm[2 * (size_t)ldp + p] = z;
}

// ---- (b) surface moments --------------------------------------------------------------------------------------------------------------------
// the value of component c of a level's block b: into the next level's [MOMENTS_N][stride], or (last level) into out [10] and the flag
__device__ __forceinline__ void moments_put(int c, double s, double* __restrict__ dst, long long stride, long long b, bool last,
                                            double* __restrict__ out, int* __restrict__ flag) {
  if (!last) dst[(size_t)c * stride + b] = s;
  else if (c < MOMENTS_N - 1) out[c] = s;
  else *flag = s > 0.0 ? 1 : 0;
}

__device__ __forceinline__ void moments_of_triangle(const float* __restrict__ verts, int nv, const int* __restrict__ faces, long long f,
                                                    const double* o, double* acc) {
  const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
  if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= nv || i1 >= nv || i2 >= nv) { acc[10] += 1.0; return; }
  double a[3], b[3], c[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    a[k] = (double)verts[3 * (size_t)i0 + k] - o[k];
    b[k] = (double)verts[3 * (size_t)i1 + k] - o[k];
    c[k] = (double)verts[3 * (size_t)i2 + k] - o[k];
  }
  const double ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2];
  const double wx = c[0] - a[0], wy = c[1] - a[1], wz = c[2] - a[2];
  const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
  const double A = 0.5 * sqrt(nx * nx + ny * ny + nz * nz);
  bool fin = isfinite(A);
#pragma unroll
  for (int k = 0; k < 3; ++k) fin = fin && isfinite(a[k]) && isfinite(b[k]) && isfinite(c[k]);
  if (!fin) { acc[10] += 1.0; return; }
  if (!(A > 0.0)) return;
  const double g[3] = {(a[0] + b[0] + c[0]) / 3.0, (a[1] + b[1] + c[1]) / 3.0, (a[2] + b[2] + c[2]) / 3.0};
  acc[0] += A;
#pragma unroll
  for (int k = 0; k < 3; ++k) acc[1 + k] += A * g[k];
  const double w = A / 12.0;
  int q = 4;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int s = r; s < 3; ++s) acc[q++] += w * (a[r] * a[s] + b[r] * b[s] + c[r] * c[s] + 9.0 * g[r] * g[s]);
}

struct Origin3 { double o[3]; };

// leaf pass: block b sums triangles [b MOMENTS_TILE, (b + 1) MOMENTS_TILE)
__global__ __launch_bounds__(EMESH_WG) void mesh_moments_kernel(const float* __restrict__ verts, int nv, const int* __restrict__ faces, int nf,
                                                                Origin3 o, double* __restrict__ dst, long long stride, bool last,
                                                                double* __restrict__ out, int* __restrict__ flag) {
  __shared__ double sh[EMESH_WG / 64];
  double acc[MOMENTS_N];
#pragma unroll
  for (int c = 0; c < MOMENTS_N; ++c) acc[c] = 0.0;
  for (int s0 = 0; s0 < MOMENTS_TILE; s0 += EMESH_WG) {
    const long long f = (long long)blockIdx.x * MOMENTS_TILE + s0 + threadIdx.x;
    if (f < nf) moments_of_triangle(verts, nv, faces, f, o.o, acc);
  }
#pragma unroll
  for (int c = 0; c < MOMENTS_N; ++c) {
    const double s = block_sum<EMESH_WG>(acc[c], sh);
    if (threadIdx.x == 0) moments_put(c, s, dst, stride, blockIdx.x, last, out, flag);
  }
}

// a level above the leaves: src [MOMENTS_N][m] -> block (b, c) sums src[c][256 b .. 256 b + 255]
__global__ __launch_bounds__(EMESH_WG) void mesh_moments_level_kernel(const double* __restrict__ src, long long m, double* __restrict__ dst,
                                                                      long long stride, bool last, double* __restrict__ out,
                                                                      int* __restrict__ flag) {
  __shared__ double sh[EMESH_WG / 64];
  const int c = blockIdx.y;
  const long long i = (long long)blockIdx.x * EMESH_WG + threadIdx.x;
  const double s = block_sum<EMESH_WG>(i < m ? src[(size_t)c * m + i] : 0.0, sh);
  if (threadIdx.x == 0) moments_put(c, s, dst, stride, blockIdx.x, last, out, flag);
}

// ---- (c) affine map and bounds of vertex rows -------------------------------------------------------------------------------------------------
__device__ __forceinline__ void affine_row(const float* __restrict__ v, const Affine34& A, double* y) {
  const double x0 = (double)v[0], x1 = (double)v[1], x2 = (double)v[2];
#pragma unroll
  for (int r = 0; r < 3; ++r) y[r] = emesh_dot3_add(A.a[4 * r], A.a[4 * r + 1], A.a[4 * r + 2], x0, x1, x2, A.a[4 * r + 3]);
}

__global__ __launch_bounds__(EMESH_WG) void affine_rows3_kernel(float* __restrict__ v, int n, Affine34 A) {
  const int p = blockIdx.x * EMESH_WG + threadIdx.x;
  if (p >= n) return;
  float* q = v + 3 * (size_t)p;
  double y[3];
  affine_row(q, A, y);
  q[0] = (float)y[0]; q[1] = (float)y[1]; q[2] = (float)y[2];
}

// partial [6 b .. 6 b + 5] = (min x, min y, min z, max x, max y, max z) of the mapped rows block b strides over; (+inf, -inf) if none
__global__ __launch_bounds__(EMESH_WG) void affine_bounds3_partial_kernel(const float* __restrict__ v, int n, Affine34 A, double* __restrict__ partial) {
  __shared__ double sh[24];
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (long long i = (long long)blockIdx.x * EMESH_WG + threadIdx.x; i < n; i += (long long)gridDim.x * EMESH_WG) {
    double y[3];
    affine_row(v + 3 * (size_t)i, A, y);
#pragma unroll
    for (int r = 0; r < 3; ++r) { lo[r] = fmin(lo[r], y[r]); hi[r] = fmax(hi[r], y[r]); }
  }
  block_minmax<EMESH_WG>(lo, hi, sh);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int r = 0; r < 3; ++r) { partial[6 * blockIdx.x + r] = lo[r]; partial[6 * blockIdx.x + 3 + r] = hi[r]; }
  }
}
__global__ __launch_bounds__(EMESH_WG) void affine_bounds3_finish_kernel(const double* __restrict__ partial, int blocks, double* __restrict__ out) {
  __shared__ double sh[24];
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int b = threadIdx.x; b < blocks; b += EMESH_WG) {
#pragma unroll
    for (int r = 0; r < 3; ++r) { lo[r] = fmin(lo[r], partial[6 * b + r]); hi[r] = fmax(hi[r], partial[6 * b + 3 + r]); }
  }
  block_minmax<EMESH_WG>(lo, hi, sh);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int r = 0; r < 3; ++r) { out[r] = lo[r]; out[3 + r] = hi[r]; }
  }
}

// ---- (d) the cut of a mesh by one plane ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double cut_dist(const float* __restrict__ verts, int v, const CutPlane& p) {
  return p.sign * ((double)verts[3 * (size_t)v + p.axis] - p.value);
}
// bit l set iff vertex l of the face is inside; 0 for a face with an index outside [0, nv) (dropped)
__device__ __forceinline__ unsigned cut_face_mask(const float* __restrict__ verts, int nv, const int* i, const CutPlane& p) {
  if (i[0] < 0 || i[1] < 0 || i[2] < 0 || i[0] >= nv || i[1] >= nv || i[2] >= nv) return 0u;
  unsigned m = 0;
#pragma unroll
  for (int l = 0; l < 3; ++l) m |= (cut_dist(verts, i[l], p) >= 0.0 ? 1u : 0u) << l;
  return m;
}
// the two crossing edges of a cut face as (inside, outside) pairs of local vertices, in the order the emitted triangles name them:
// one inside i: (i, j), (i, k); two inside, outside o: (j, o), (i, o).  *first = i.
__device__ __forceinline__ void cut_face_edges(unsigned m, int* first, int* ea, int* eb) {
  if (__popc(m) == 1) {
    const int i = m == 1u ? 0 : (m == 2u ? 1 : 2), j = (i + 1) % 3, k = (i + 2) % 3;
    *first = i; ea[0] = i; eb[0] = j; ea[1] = i; eb[1] = k;
  } else {
    const int o = m == 6u ? 0 : (m == 5u ? 1 : 2), i = (o + 1) % 3, j = (o + 2) % 3;
    *first = i; ea[0] = j; eb[0] = o; ea[1] = i; eb[1] = o;
  }
}

// pass 1, one lane per face: the number of triangles it leaves, the keys of its crossing edges (-1: none), the inside vertices it uses
__global__ __launch_bounds__(EMESH_WG) void cut_count_kernel(const float* __restrict__ verts, int nv, const int* __restrict__ faces, int nf, CutPlane p,
                                                             int* __restrict__ fcnt, long long* __restrict__ ekey, int* __restrict__ used) {
  const int f = blockIdx.x * EMESH_WG + threadIdx.x;
  if (f >= nf) return;
  const int i[3] = {faces[3 * (size_t)f], faces[3 * (size_t)f + 1], faces[3 * (size_t)f + 2]};
  const unsigned m = cut_face_mask(verts, nv, i, p);
  const int inside = __popc(m);
  long long k0 = -1, k1 = -1;
  if (inside == 1 || inside == 2) {
    int first, ea[2], eb[2];
    cut_face_edges(m, &first, ea, eb);
    k0 = (long long)i[ea[0]] * nv + i[eb[0]];
    k1 = (long long)i[ea[1]] * nv + i[eb[1]];
  }
  fcnt[f] = inside == 0 ? 0 : (inside == 2 ? 2 : 1);
  ekey[2 * (size_t)f] = k0;
  ekey[2 * (size_t)f + 1] = k1;
#pragma unroll
  for (int l = 0; l < 3; ++l)
    if ((m >> l) & 1u) used[i[l]] = 1;      // every writer stores the same value
}

// pass 2a, one lane per old vertex and per cut vertex: vmap = the exclusive scan of `used`, ukey = the unique keys ascending
__global__ __launch_bounds__(EMESH_WG) void cut_verts_kernel(const float* __restrict__ verts, int nv, CutPlane p, const int* __restrict__ used,
                                                             const int* __restrict__ vmap, const long long* __restrict__ ukey, int ncut, int nkeep,
                                                             float* __restrict__ out, int nout) {
  const long long t = (long long)blockIdx.x * EMESH_WG + threadIdx.x;
  if (t < nv) {
    if (!used[t]) return;
    const int d = vmap[t];
    if (d < 0 || d >= nout) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) out[3 * (size_t)d + k] = verts[3 * (size_t)t + k];
    return;
  }
  const long long c = t - nv;
  if (c >= ncut || nkeep + c >= nout) return;
  const long long key = ukey[c];
  const long long a = key / nv, b = key % nv;
  if (key < 0 || a >= nv) return;
  const double da = cut_dist(verts, (int)a, p), db = cut_dist(verts, (int)b, p);
  const double tt = da / (da - db);
  float* q = out + 3 * (size_t)(nkeep + c);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double xa = (double)verts[3 * (size_t)a + k], xb = (double)verts[3 * (size_t)b + k];
    q[k] = k == p.axis ? (float)p.value : (float)rounded(xa + rounded(tt * rounded(xb - xa)));      // no contraction: one rounding per step
  }
}

__device__ __forceinline__ int cut_key_rank(const long long* __restrict__ ukey, int ncut, long long key) {      // lower bound
  int lo = 0, hi = ncut;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ukey[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// pass 2b, one lane per source face: its triangles at foff[f] (the exclusive scan of fcnt)
__global__ __launch_bounds__(EMESH_WG) void cut_faces_kernel(const float* __restrict__ verts, int nv, const int* __restrict__ faces, int nf, CutPlane p,
                                                             const int* __restrict__ foff, const int* __restrict__ vmap,
                                                             const long long* __restrict__ ukey, int ncut, int nkeep, int* __restrict__ out,
                                                             int nf_out) {
  const int f = blockIdx.x * EMESH_WG + threadIdx.x;
  if (f >= nf) return;
  const int i[3] = {faces[3 * (size_t)f], faces[3 * (size_t)f + 1], faces[3 * (size_t)f + 2]};
  const unsigned m = cut_face_mask(verts, nv, i, p);
  const int inside = __popc(m);
  if (inside == 0) return;
  const int base = foff[f];
  if (base < 0 || base + (inside == 2 ? 2 : 1) > nf_out) return;
  int* q = out + 3 * (size_t)base;
  if (inside == 3) { q[0] = vmap[i[0]]; q[1] = vmap[i[1]]; q[2] = vmap[i[2]]; return; }
  int first, ea[2], eb[2];
  cut_face_edges(m, &first, ea, eb);
  const int c0 = nkeep + cut_key_rank(ukey, ncut, (long long)i[ea[0]] * nv + i[eb[0]]);
  const int c1 = nkeep + cut_key_rank(ukey, ncut, (long long)i[ea[1]] * nv + i[eb[1]]);
  if (inside == 1) {
    q[0] = vmap[i[first]]; q[1] = c0; q[2] = c1;                     // (i, c_ij, c_ik)
  } else {
    const int vi = vmap[i[first]], vj = vmap[i[(first + 1) % 3]];
    q[0] = vi; q[1] = vj; q[2] = c0;                                 // (i, j, c_jo)
    q[3] = vi; q[4] = c0; q[5] = c1;                                 // (i, c_jo, c_io)
  }
}

}  // namespace neat
