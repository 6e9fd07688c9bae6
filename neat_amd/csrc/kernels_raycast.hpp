// Ray casting against an indexed triangle mesh (neat_amd/raycast.py): where a ray first meets a triangle, or whether it meets one at
// all before t_max.  A tree over the triangles is built and walked on the device; the answer is the one of the brute-force rule over
// all triangles, whatever the tree looks like.  DESIGN 3h; tests/raycast_f64.py states the rule and a model of the tree in float64.
//
// Rule (Woop, Benthin, Wald 2013, "Watertight ray/triangle intersection", decided in float64).  Ray (o, d), both float32 widened
// exactly; triangle (v0, v1, v2) float64.
//   axes      kz = the axis of the largest |d| (the lowest on a tie), kx = kz + 1, ky = kx + 1 (mod 3), kx and ky swapped when d[kz] < 0.
//             Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz].
//   shear     A = v0 - o, B = v1 - o, C = v2 - o;  Ax = A[kx] - Sx A[kz], Ay = A[ky] - Sy A[kz], likewise B and C.
//   edges     U = Cx By - Cy Bx, V = Ax Cy - Ay Cx, W = Bx Ay - By Ax.
//   accept    U, V, W all >= 0 or all <= 0 (both windings, edges inclusive); det = (U + V) + W != 0;
//             t = ((U Sz A[kz] + V Sz B[kz]) + W Sz C[kz]) / det with t_min <= t < t_max.  uv = (V / det, W / det): the hit is
//             (1 - u - v) v0 + u v1 + v v2.
//   closest   the smallest t; ties in t go to the lowest original face index.
//   never hit a triangle with a non-finite vertex or with (v1 - v0) x (v2 - v0) = 0 in every component.
// Device form: every product above is rounded on its own before the sum or difference that uses it (rounded(), device_util.hpp, and
// contraction switched off in these functions), so no product is fused into an fma: the two triangles that share an edge compute the
// same two products for it and get edge values of equal magnitude and opposite sign, and no ray slips between them.  Divisions
// are the correctly rounded float64 division.  tests/raycast_f64.py does the same operations in numpy float64.
//
// Tree.  Triangles sorted by the 63-bit Morton key of their centroid in the box of the centroids (rocprim radix_sort_pairs; triangles
// that are never hit sort last).  L = the power of two >= max(nf, 1) leaves, one sorted triangle per leaf, in heap order: node k has
// children 2k and 2k + 1, the leaves are nodes L .. 2L - 1, leaf L + i holds sorted triangle i.  Boxes are float32 [lo xyz | hi xyz],
// rounded outwards from the float64 bounds; padding leaves and never-hit triangles carry the empty box (lo = +inf, hi = -inf).
// Refit: raycast_leaf_kernel reduces the subtree over each workgroup's 256 leaves through LDS between __syncthreads(); the levels above
// those subtree roots are raycast_top_kernel, one workgroup.  No workgroup waits for another inside a launch.
//
// Walk.  One ray per lane, near child first, a box is left out only when its entry distance is > the best t so far (never >=), so the
// result is the brute-force minimum under the tie rule in any order.  The state is the node index and a bit trail (bit j set: the
// sibling of the ancestor j levels up is still to be visited) in two registers: no stack, no scratch.  The box test is the slab test
// in float64 on the box widened by 2^-26 of its largest distance from the origin of the ray (DESIGN 3h has the argument that it never
// refuses a box holding a triangle the rule accepts).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "block_util.hpp"      // block_minmax
#include "device_util.hpp"

namespace neat {

constexpr int RC_WG = 256;
constexpr int RC_TOP_WG = 1024;
constexpr int RC_TRI_STRIDE = 10;            // doubles per sorted triangle: 9 coordinates, then the original face index in the low 4 bytes
constexpr unsigned long long RC_KEY_LAST = 0x7fffffffffffffffull;

// the three vertices of face g -> valid (finite, non-zero area).  The caller has checked the indices.
__device__ __forceinline__ bool rc_triangle(const double* __restrict__ verts, const int* __restrict__ faces, int g, double* __restrict__ v) {
#pragma clang fp contract(off)
  bool finite = true;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const size_t i = (size_t)faces[3 * (size_t)g + c];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      v[3 * c + a] = verts[3 * i + a];
      finite = finite && isfinite(v[3 * c + a]);
    }
  }
  const double e1x = v[3] - v[0], e1y = v[4] - v[1], e1z = v[5] - v[2];
  const double e2x = v[6] - v[0], e2y = v[7] - v[1], e2z = v[8] - v[2];
  const double nx = rounded(e1y * e2z) - rounded(e1z * e2y);
  const double ny = rounded(e1z * e2x) - rounded(e1x * e2z);
  const double nz = rounded(e1x * e2y) - rounded(e1y * e2x);
  return finite && (nx != 0.0 || ny != 0.0 || nz != 0.0);
}

__device__ __forceinline__ bool rc_indices_ok(const int* __restrict__ faces, int g, int nv) {
  const int a = faces[3 * (size_t)g], b = faces[3 * (size_t)g + 1], c = faces[3 * (size_t)g + 2];
  return a >= 0 && a < nv && b >= 0 && b < nv && c >= 0 && c < nv;
}

__device__ __forceinline__ void rc_centroid(const double* __restrict__ v, double* __restrict__ c) {
#pragma clang fp contract(off)
#pragma unroll
  for (int a = 0; a < 3; ++a) c[a] = ((v[a] + v[3 + a]) + v[6 + a]) / 3.0;
}

// ---- prep: the index check (before any vertex is read), then each workgroup's box of the centroids of its valid triangles
__global__ __launch_bounds__(RC_WG) void raycast_prep_kernel(const double* __restrict__ verts, int nv, const int* __restrict__ faces, int nf,
                                                            int* __restrict__ status, double* __restrict__ partial) {
  __shared__ double sh[24];
  const int g = blockIdx.x * RC_WG + threadIdx.x;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  if (g < nf) {
    if (!rc_indices_ok(faces, g, nv)) {
      status[0] = 1;                      // every writer stores the same value
    } else {
      double v[9], c[3];
      if (rc_triangle(verts, faces, g, v)) {
        rc_centroid(v, c);
#pragma unroll
        for (int a = 0; a < 3; ++a) { lo[a] = c[a]; hi[a] = c[a]; }
      }
    }
  }
  block_minmax<RC_WG>(lo, hi, sh);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { partial[6 * (size_t)blockIdx.x + a] = lo[a]; partial[6 * (size_t)blockIdx.x + 3 + a] = hi[a]; }
  }
}

// ---- one workgroup: the partial boxes -> the box of all centroids
__global__ __launch_bounds__(RC_WG) void raycast_scene_box_kernel(const double* __restrict__ partial, int n, double* __restrict__ box) {
  __shared__ double sh[24];
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int i = threadIdx.x; i < n; i += RC_WG) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      lo[a] = fmin(lo[a], partial[6 * (size_t)i + a]);
      hi[a] = fmax(hi[a], partial[6 * (size_t)i + 3 + a]);
    }
  }
  block_minmax<RC_WG>(lo, hi, sh);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { box[a] = lo[a]; box[3 + a] = hi[a]; }
  }
}

__device__ __forceinline__ unsigned long long rc_spread21(unsigned long long x) {      // bit i -> bit 3 i
  x &= 0x1fffffull;
  x = (x | (x << 32)) & 0x1f00000000ffffull;
  x = (x | (x << 16)) & 0x1f0000ff0000ffull;
  x = (x | (x << 8)) & 0x100f00f00f00f00full;
  x = (x | (x << 4)) & 0x10c30c30c30c30c3ull;
  x = (x | (x << 2)) & 0x1249249249249249ull;
  return x;
}

// ---- the Morton key of each triangle's centroid (21 bits an axis); never-hit triangles, and all of them after a bad index, sort last
__global__ __launch_bounds__(RC_WG) void raycast_key_kernel(const double* __restrict__ verts, const int* __restrict__ faces, int nf,
                                                           const int* __restrict__ status, const double* __restrict__ box,
                                                           unsigned long long* __restrict__ key, int* __restrict__ val) {
  const int g = blockIdx.x * RC_WG + threadIdx.x;
  if (g >= nf) return;
  unsigned long long k = RC_KEY_LAST;
  if (status[0] == 0) {
    double v[9], c[3];
    if (rc_triangle(verts, faces, g, v)) {
      rc_centroid(v, c);
      k = 0;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const double ext = box[3 + a] - box[a];
        double q = ext > 0.0 ? (c[a] - box[a]) / ext * 2097152.0 : 0.0;
        q = q >= 0.0 ? q : 0.0;                         // a NaN too
        q = q <= 2097151.0 ? q : 2097151.0;
        k |= rc_spread21((unsigned long long)q) << a;
      }
    }
  }
  key[g] = k;
  val[g] = g;
}

__device__ __forceinline__ float rc_round_down(double x) {
  float f = (float)x;
  if ((double)f > x) f = nextafterf(f, -INFINITY);
  return f;
}
__device__ __forceinline__ float rc_round_up(double x) {
  float f = (float)x;
  if ((double)f < x) f = nextafterf(f, INFINITY);
  return f;
}

// ---- leaves and the subtree above each workgroup's `per` = min(L, 256) leaves.  nodes [2 L][6] float32, tris [nf][RC_TRI_STRIDE] float64
__global__ __launch_bounds__(RC_WG) void raycast_leaf_kernel(const double* __restrict__ verts, const int* __restrict__ faces, int nf, int L, int per,
                                                            const int* __restrict__ status, const int* __restrict__ sorted,
                                                            float* __restrict__ nodes, double* __restrict__ tris) {
  __shared__ float s_box[RC_WG][6];
  const int tid = threadIdx.x;
  const int g = blockIdx.x * per + tid;
  float b[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
  if (tid < per && g < nf) {
    double v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int id = -1;
    if (status[0] == 0) {
      id = sorted[g];
      if (id >= 0 && id < nf && rc_triangle(verts, faces, id, v)) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          b[a] = rc_round_down(fmin(fmin(v[a], v[3 + a]), v[6 + a]));
          b[3 + a] = rc_round_up(fmax(fmax(v[a], v[3 + a]), v[6 + a]));
        }
      }
    }
    double* t = tris + (size_t)RC_TRI_STRIDE * g;
#pragma unroll
    for (int a = 0; a < 9; ++a) t[a] = v[a];
    t[9] = __longlong_as_double((long long)id);
  }
  if (tid < per) {
#pragma unroll
    for (int a = 0; a < 6; ++a) { s_box[tid][a] = b[a]; nodes[6 * (size_t)(L + g) + a] = b[a]; }
  }
  const int first = L + blockIdx.x * per;          // heap index of this workgroup's first leaf
  int shift = 1;
  for (int w = per >> 1; w >= 1; w >>= 1, ++shift) {
    __syncthreads();
    float m[6];
    if (tid < w) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        m[a] = fminf(s_box[2 * tid][a], s_box[2 * tid + 1][a]);
        m[3 + a] = fmaxf(s_box[2 * tid][3 + a], s_box[2 * tid + 1][3 + a]);
      }
    }
    __syncthreads();
    if (tid < w) {
      const size_t node = (size_t)(first >> shift) + tid;
#pragma unroll
      for (int a = 0; a < 6; ++a) { s_box[tid][a] = m[a]; nodes[6 * node + a] = m[a]; }
    }
  }
}

// ---- one workgroup: the levels above the `roots` subtree roots (nodes roots .. 2 roots - 1), level by level
__global__ __launch_bounds__(RC_TOP_WG) void raycast_top_kernel(float* nodes, int roots) {
  for (int n = roots >> 1; n >= 1; n >>= 1) {
    for (int j = threadIdx.x; j < n; j += RC_TOP_WG) {
      const size_t k = (size_t)n + j;
      const float* l = nodes + 6 * (2 * k);
      const float* r = l + 6;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        nodes[6 * k + a] = fminf(l[a], r[a]);
        nodes[6 * k + 3 + a] = fmaxf(l[3 + a], r[3 + a]);
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------------------------------ the walk
struct RcRay {
  double ox, oy, oz, dx, dy, dz, ix, iy, iz;      // origin, direction, 1 / direction
  double okx, oky, okz, Sx, Sy, Sz;               // the permuted origin and the shear
  int kx, ky, kz;
};

__device__ __forceinline__ double rc_sel(double x, double y, double z, int k) { return k == 0 ? x : (k == 1 ? y : z); }

__device__ __forceinline__ void rc_ray_setup(RcRay& r) {
#pragma clang fp contract(off)
  int kz = 0;
  double m = fabs(r.dx);
  if (fabs(r.dy) > m) { kz = 1; m = fabs(r.dy); }
  if (fabs(r.dz) > m) { kz = 2; }
  int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
  const double dkz = rc_sel(r.dx, r.dy, r.dz, kz);
  if (dkz < 0.0) { const int t = kx; kx = ky; ky = t; }
  r.kx = kx; r.ky = ky; r.kz = kz;
  r.Sx = rc_sel(r.dx, r.dy, r.dz, kx) / dkz;
  r.Sy = rc_sel(r.dx, r.dy, r.dz, ky) / dkz;
  r.Sz = 1.0 / dkz;
  r.okx = rc_sel(r.ox, r.oy, r.oz, kx); r.oky = rc_sel(r.ox, r.oy, r.oz, ky); r.okz = rc_sel(r.ox, r.oy, r.oz, kz);
  r.ix = 1.0 / r.dx; r.iy = 1.0 / r.dy; r.iz = 1.0 / r.dz;
}

// one slab: false = the ray misses the slab [a, b] (already relative to the origin and widened)
__device__ __forceinline__ bool rc_slab(double a, double b, double d, double inv, double& en, double& ex) {
#pragma clang fp contract(off)
  if (d == 0.0) return a <= 0.0 && b >= 0.0;
  const double t1 = a * inv, t2 = b * inv;
  en = fmax(en, fmin(t1, t2));
  ex = fmin(ex, fmax(t1, t2));
  return true;
}

// the conservative box test -> the box may hold a hit with t_min <= t <= best; entry = its entry distance
__device__ __forceinline__ bool rc_box(float lx, float ly, float lz, float hx, float hy, float hz, const RcRay& r, double t_min, double best,
                                       double& entry) {
#pragma clang fp contract(off)
  entry = INFINITY;
  if (!(lx <= hx && ly <= hy && lz <= hz)) return false;          // the empty box
  double ax = (double)lx - r.ox, bx = (double)hx - r.ox;
  double ay = (double)ly - r.oy, by = (double)hy - r.oy;
  double az = (double)lz - r.oz, bz = (double)hz - r.oz;
  const double M = fmax(fmax(fmax(fabs(ax), fabs(bx)), fmax(fabs(ay), fabs(by))), fmax(fabs(az), fabs(bz)));
  const double pad = M * 1.4901161193847656e-08;                  // 2^-26
  ax -= pad; ay -= pad; az -= pad; bx += pad; by += pad; bz += pad;
  double en = -INFINITY, ex = INFINITY;
  if (!rc_slab(ax, bx, r.dx, r.ix, en, ex)) return false;
  if (!rc_slab(ay, by, r.dy, r.iy, en, ex)) return false;
  if (!rc_slab(az, bz, r.dz, r.iz, en, ex)) return false;
  entry = en;
  return en <= ex && en <= best && ex >= t_min;
}

// the rule for one triangle -> accepted with t_min <= t < t_max (the caller compares with its best)
__device__ __forceinline__ bool rc_hit(const double* __restrict__ tv, const RcRay& r, double t_min, double t_max, double& t, double& u,
                                       double& v) {
#pragma clang fp contract(off)
  const double2* p = (const double2*)tv;
  const double2 q0 = p[0], q1 = p[1], q2 = p[2], q3 = p[3];
  const double q4 = tv[8];
  // v0 = (q0.x, q0.y, q1.x), v1 = (q1.y, q2.x, q2.y), v2 = (q3.x, q3.y, q4)
  const double Akz = rc_sel(q0.x, q0.y, q1.x, r.kz) - r.okz, Bkz = rc_sel(q1.y, q2.x, q2.y, r.kz) - r.okz, Ckz = rc_sel(q3.x, q3.y, q4, r.kz) - r.okz;
  const double Ax = (rc_sel(q0.x, q0.y, q1.x, r.kx) - r.okx) - rounded(r.Sx * Akz), Ay = (rc_sel(q0.x, q0.y, q1.x, r.ky) - r.oky) - rounded(r.Sy * Akz);
  const double Bx = (rc_sel(q1.y, q2.x, q2.y, r.kx) - r.okx) - rounded(r.Sx * Bkz), By = (rc_sel(q1.y, q2.x, q2.y, r.ky) - r.oky) - rounded(r.Sy * Bkz);
  const double Cx = (rc_sel(q3.x, q3.y, q4, r.kx) - r.okx) - rounded(r.Sx * Ckz), Cy = (rc_sel(q3.x, q3.y, q4, r.ky) - r.oky) - rounded(r.Sy * Ckz);
  const double U = rounded(Cx * By) - rounded(Cy * Bx);
  const double V = rounded(Ax * Cy) - rounded(Ay * Cx);
  const double W = rounded(Bx * Ay) - rounded(By * Ax);
  if (!((U >= 0.0 && V >= 0.0 && W >= 0.0) || (U <= 0.0 && V <= 0.0 && W <= 0.0))) return false;
  const double det = (U + V) + W;
  if (det == 0.0) return false;
  const double Az = rounded(r.Sz * Akz), Bz = rounded(r.Sz * Bkz), Cz = rounded(r.Sz * Ckz);
  const double T = (rounded(U * Az) + rounded(V * Bz)) + rounded(W * Cz);
  t = T / det;
  if (!(t >= t_min && t < t_max)) return false;
  u = V / det;
  v = W / det;
  return true;
}

// The walk of one ray: the closest accepted hit with t_min <= t < t_max, or (ANY) the first one the walk meets.  best comes in as t_max and
// goes out as the hit's t; id = the original face index (-1: a miss), leaf = its place among the sorted triangles; n_nodes, n_tris count
// the node boxes and the triangles tested.  raycast_cast_kernel and the kernels of kernels_scenegen.hpp call it
struct RcHit {
  double t, u, v;
  int id, leaf;
  unsigned n_nodes, n_tris;
};

template <bool ANY>
__device__ __forceinline__ RcHit rc_walk(const float* __restrict__ nodes, const double* __restrict__ tris, int nf, int L, const RcRay& r, double t_min,
                                         double t_max) {
  double best = t_max, bu = 0.0, bv = 0.0;
  int best_id = -1, best_leaf = -1;
  unsigned n_nodes = 1, n_tris = 0;
  int node = 1;
  unsigned trail = 0;
  double e0, e1;
  bool alive;
  {
    const float* b = nodes + 6;
    alive = rc_box(b[0], b[1], b[2], b[3], b[4], b[5], r, t_min, best, e0);
  }
  while (alive) {
    bool descend = false;
    if (node >= L) {
      const int leaf = node - L;
      if (leaf < nf) {
        const double* tv = tris + (size_t)RC_TRI_STRIDE * leaf;
        double t, u, v;
        ++n_tris;
        if (rc_hit(tv, r, t_min, t_max, t, u, v)) {
          const int id = (int)__double_as_longlong(tv[9]);
          if (t < best || (t == best && id < best_id)) {
            best = t; best_id = id; best_leaf = leaf; bu = u; bv = v;
            if (ANY) break;
          }
        }
      }
    } else {
      const float4* c = (const float4*)(nodes + 12 * (size_t)node);        // the two children, 48 bytes, 16-byte aligned
      const float4 c0 = c[0], c1 = c[1], c2 = c[2];
      n_nodes += 2;
      const bool h0 = rc_box(c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, r, t_min, best, e0);
      const bool h1 = rc_box(c1.z, c1.w, c2.x, c2.y, c2.z, c2.w, r, t_min, best, e1);
      if (h0 || h1) {
        const int both = (h0 && h1) ? 1 : 0;
        const int right = both ? (e1 < e0 ? 1 : 0) : (h1 ? 1 : 0);
        node = 2 * node + right;
        trail = (trail << 1) | (unsigned)both;
        descend = true;
      }
    }
    if (descend) continue;
    for (;;) {                        // back up to the nearest ancestor whose sibling is still to be visited
      if (trail == 0) { alive = false; break; }
      const int s = __ffs((int)trail) - 1;
      node >>= s;
      trail >>= s;
      node ^= 1;
      trail ^= 1u;
      const float* b = nodes + 6 * (size_t)node;
      ++n_nodes;
      if (rc_box(b[0], b[1], b[2], b[3], b[4], b[5], r, t_min, best, e0)) break;
    }
  }
  RcHit h;
  h.t = best; h.u = bu; h.v = bv; h.id = best_id; h.leaf = best_leaf; h.n_nodes = n_nodes; h.n_tris = n_tris;
  return h;
}

// ---- cast: closest hit, or (ANY) the first accepted hit.  counts [R][2]: node boxes tested, triangles tested; null to skip
template <bool ANY>
__global__ __launch_bounds__(RC_WG) void raycast_cast_kernel(const float* __restrict__ nodes, const double* __restrict__ tris, int nf, int L,
                                                            const float* __restrict__ origins, const float* __restrict__ dirs,
                                                            const float* __restrict__ t_min_p, const float* __restrict__ t_max_p, int R,
                                                            float* __restrict__ t_out, int* __restrict__ tri_out, float* __restrict__ uv_out,
                                                            unsigned* __restrict__ counts) {
  const int i = blockIdx.x * RC_WG + threadIdx.x;
  if (i >= R) return;
  RcRay r;
  r.ox = origins[3 * (size_t)i]; r.oy = origins[3 * (size_t)i + 1]; r.oz = origins[3 * (size_t)i + 2];
  r.dx = dirs[3 * (size_t)i]; r.dy = dirs[3 * (size_t)i + 1]; r.dz = dirs[3 * (size_t)i + 2];
  rc_ray_setup(r);
  const double t_min = t_min_p ? (double)t_min_p[i] : 0.0;
  const double t_max = t_max_p ? (double)t_max_p[i] : (double)INFINITY;
  const RcHit h = rc_walk<ANY>(nodes, tris, nf, L, r, t_min, t_max);
  const bool hit = h.id >= 0;
  t_out[i] = hit ? (float)h.t : INFINITY;
  tri_out[i] = hit ? h.id : -1;
  uv_out[2 * (size_t)i] = hit ? (float)h.u : 0.f;
  uv_out[2 * (size_t)i + 1] = hit ? (float)h.v : 0.f;
  if (counts) { counts[2 * (size_t)i] = h.n_nodes; counts[2 * (size_t)i + 1] = h.n_tris; }
}

}  // namespace neat
