// The closest point on an indexed triangle mesh (neat_amd/raycast.py closest): a second walk over the tree of kernels_raycast.hpp, one
// query point per lane.  The answer is the one of the brute-force rule over all triangles, whatever the tree looks like.  DESIGN 3m;
// tests/closest_f64.py states the rule in float64.
//
// Rule (Ericson, Real-Time Collision Detection 5.1.5, decided in float64).  Query p, triangle (a, b, c), all float64.
//   dots      ab = b - a, ac = c - a, ap = p - a, bp = p - b, cp = p - c;  d1 = ab.ap, d2 = ac.ap, d3 = ab.bp, d4 = ac.bp, d5 = ab.cp,
//             d6 = ac.cp, each (x x' + y y') + z z';  vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4.
//   regions   in the book's order, the first that holds, every comparison inclusive:
//             A   d1 <= 0, d2 <= 0                                  q = a                      uv = (0, 0)
//             B   d3 >= 0, d4 <= d3                                 q = b                      uv = (1, 0)
//             AB  vc <= 0, d1 >= 0, d3 <= 0    s = d1 / (d1 - d3)   q = a + s ab               uv = (s, 0)
//             C   d6 >= 0, d5 <= d6                                 q = c                      uv = (0, 1)
//             AC  vb <= 0, d2 >= 0, d6 <= 0    s = d2 / (d2 - d6)   q = a + s ac               uv = (0, s)
//             BC  va <= 0, d4 - d3 >= 0, d5 - d6 >= 0
//                            s = (d4 - d3) / ((d4 - d3) + (d5 - d6))  q = b + s (c - b)        uv = (1 - s, s)
//             in  den = (va + vb) + vc, s = vb / den, t = vc / den  q = (a + s ab) + t ac      uv = (s, t)
//   distance  d = p - q, d2 = (dx dx + dy dy) + dz dz, from the q that is returned.
//   accept    d2 <= max_d2 (inclusive; a NaN never is).  The smallest d2 wins; ties go to the lowest original face index.
//   never     a triangle with a non-finite vertex or zero area (rc_triangle) is never closest: the build gives it the empty box.
// Device form: as in rc_hit every product is rounded on its own before the sum or difference that uses it (rounded(), contraction off),
// divisions are the correctly rounded float64 division, so the numbers are those of numpy float64 and do not depend on the compiler's
// choice of fma.
//
// Walk.  That of rc_walk: near child first, the node index and a bit trail in two registers, no stack, no scratch.  The lower bound of a
// node is the squared distance from p to its float32 box in float64, per axis max(lo - p, 0, p - hi), each axis first shrunk by
//   pad = 2^-26 M + 2^-48 A,   M = the largest |lo - p|, |hi - p| over the axes,   A = the largest |lo|, |hi| over the axes
// and a box is left out only when that bound is > the best d2 so far (never >=), so a tie with a lower face index is still visited and
// the order of the visits does not show in the result.  DESIGN 3m has the argument that the shrunk bound is never above the computed d2
// of a triangle inside the box.
#pragma once
#include "kernels_raycast.hpp"

namespace neat {

// lb = the shrunk lower bound of the squared distance from p to a box -> the box may hold a triangle with d2 <= best.  The empty box
// (padding leaves, never-closest triangles) never does
__device__ __forceinline__ bool cp_box(float lx, float ly, float lz, float hx, float hy, float hz, double px, double py, double pz, double best,
                                       double& lb) {
#pragma clang fp contract(off)
  lb = INFINITY;
  if (!(lx <= hx && ly <= hy && lz <= hz)) return false;
  const double ax = (double)lx - px, bx = px - (double)hx;
  const double ay = (double)ly - py, by = py - (double)hy;
  const double az = (double)lz - pz, bz = pz - (double)hz;
  const double M = fmax(fmax(fmax(fabs(ax), fabs(bx)), fmax(fabs(ay), fabs(by))), fmax(fabs(az), fabs(bz)));
  const double A = (double)fmaxf(fmaxf(fmaxf(fabsf(lx), fabsf(hx)), fmaxf(fabsf(ly), fabsf(hy))), fmaxf(fabsf(lz), fabsf(hz)));
  const double pad = rounded(M * 1.4901161193847656e-08) + rounded(A * 3.5527136788005009e-15);          // 2^-26, 2^-48
  const double ex = fmax(fmax(ax, bx) - pad, 0.0), ey = fmax(fmax(ay, by) - pad, 0.0), ez = fmax(fmax(az, bz) - pad, 0.0);
  lb = (rounded(ex * ex) + rounded(ey * ey)) + rounded(ez * ez);
  return !(lb > best);
}

__device__ __forceinline__ double cp_dot(double ax, double ay, double az, double bx, double by, double bz) {
#pragma clang fp contract(off)
  return (rounded(ax * bx) + rounded(ay * by)) + rounded(az * bz);
}

// the rule for one triangle -> d2, the closest point q and its barycentrics (u, v)
__device__ __forceinline__ double cp_triangle(const double* __restrict__ tv, double px, double py, double pz, double& qx, double& qy, double& qz,
                                              double& u, double& v) {
#pragma clang fp contract(off)
  const double2* t2 = (const double2*)tv;
  const double2 q0 = t2[0], q1 = t2[1], q2 = t2[2], q3 = t2[3];
  const double ax = q0.x, ay = q0.y, az = q1.x, bx = q1.y, by = q2.x, bz = q2.y, cx = q3.x, cy = q3.y, cz = tv[8];
  const double abx = bx - ax, aby = by - ay, abz = bz - az;
  const double acx = cx - ax, acy = cy - ay, acz = cz - az;
  const double d1 = cp_dot(abx, aby, abz, px - ax, py - ay, pz - az), d2 = cp_dot(acx, acy, acz, px - ax, py - ay, pz - az);
  const double d3 = cp_dot(abx, aby, abz, px - bx, py - by, pz - bz), d4 = cp_dot(acx, acy, acz, px - bx, py - by, pz - bz);
  const double d5 = cp_dot(abx, aby, abz, px - cx, py - cy, pz - cz), d6 = cp_dot(acx, acy, acz, px - cx, py - cy, pz - cz);
  if (d1 <= 0.0 && d2 <= 0.0) {
    qx = ax; qy = ay; qz = az; u = 0.0; v = 0.0;
  } else if (d3 >= 0.0 && d4 <= d3) {
    qx = bx; qy = by; qz = bz; u = 1.0; v = 0.0;
  } else {
    const double vc = rounded(d1 * d4) - rounded(d3 * d2);
    if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
      const double s = d1 / (d1 - d3);
      qx = ax + rounded(s * abx); qy = ay + rounded(s * aby); qz = az + rounded(s * abz); u = s; v = 0.0;
    } else if (d6 >= 0.0 && d5 <= d6) {
      qx = cx; qy = cy; qz = cz; u = 0.0; v = 1.0;
    } else {
      const double vb = rounded(d5 * d2) - rounded(d1 * d6);
      if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
        const double s = d2 / (d2 - d6);
        qx = ax + rounded(s * acx); qy = ay + rounded(s * acy); qz = az + rounded(s * acz); u = 0.0; v = s;
      } else {
        const double va = rounded(d3 * d6) - rounded(d5 * d4);
        const double e43 = d4 - d3, e56 = d5 - d6;
        if (va <= 0.0 && e43 >= 0.0 && e56 >= 0.0) {
          const double s = e43 / (e43 + e56);
          qx = bx + rounded(s * (cx - bx)); qy = by + rounded(s * (cy - by)); qz = bz + rounded(s * (cz - bz)); u = 1.0 - s; v = s;
        } else {
          const double den = (va + vb) + vc;
          const double s = vb / den, t = vc / den;
          qx = (ax + rounded(s * abx)) + rounded(t * acx); qy = (ay + rounded(s * aby)) + rounded(t * acy);
          qz = (az + rounded(s * abz)) + rounded(t * acz); u = s; v = t;
        }
      }
    }
  }
  const double dx = px - qx, dy = py - qy, dz = pz - qz;
  return (rounded(dx * dx) + rounded(dy * dy)) + rounded(dz * dz);
}

// ---- closest: one query per lane.  counts [N][2]: node boxes tested, triangles tested; null to skip
__global__ __launch_bounds__(RC_WG) void raycast_closest_kernel(const float* __restrict__ nodes, const double* __restrict__ tris, int nf, int L,
                                                               const double* __restrict__ points, int N, double max_d2,
                                                               double* __restrict__ d2_out, int* __restrict__ tri_out,
                                                               double* __restrict__ point_out, double* __restrict__ uv_out,
                                                               unsigned* __restrict__ counts) {
  const int i = blockIdx.x * RC_WG + threadIdx.x;
  if (i >= N) return;
  const double px = points[3 * (size_t)i], py = points[3 * (size_t)i + 1], pz = points[3 * (size_t)i + 2];
  double best = max_d2, bqx = 0.0, bqy = 0.0, bqz = 0.0, bu = 0.0, bv = 0.0;
  int best_id = -1;                    // compared as unsigned: every face index is below "none", so d2 == max_d2 is accepted
  unsigned n_nodes = 0, n_tris = 0;
  int node = 1;
  unsigned trail = 0;
  bool alive = false;
  double l0, l1;
  if (isfinite(px) && isfinite(py) && isfinite(pz)) {
    const float* b = nodes + 6;
    n_nodes = 1;
    alive = cp_box(b[0], b[1], b[2], b[3], b[4], b[5], px, py, pz, best, l0);
  }
  while (alive) {
    bool descend = false;
    if (node >= L) {
      const int leaf = node - L;
      if (leaf < nf) {
        const double* tv = tris + (size_t)RC_TRI_STRIDE * leaf;
        double qx, qy, qz, u, v;
        ++n_tris;
        const double d2 = cp_triangle(tv, px, py, pz, qx, qy, qz, u, v);
        const int id = (int)__double_as_longlong(tv[9]);
        if (d2 < best || (d2 == best && (unsigned)id < (unsigned)best_id)) {
          best = d2; best_id = id; bqx = qx; bqy = qy; bqz = qz; bu = u; bv = v;
        }
      }
    } else {
      const float4* c = (const float4*)(nodes + 12 * (size_t)node);        // the two children, 48 bytes, 16-byte aligned
      const float4 c0 = c[0], c1 = c[1], c2 = c[2];
      n_nodes += 2;
      const bool h0 = cp_box(c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, px, py, pz, best, l0);
      const bool h1 = cp_box(c1.z, c1.w, c2.x, c2.y, c2.z, c2.w, px, py, pz, best, l1);
      if (h0 || h1) {
        const int both = (h0 && h1) ? 1 : 0;
        const int right = both ? (l1 < l0 ? 1 : 0) : (h1 ? 1 : 0);
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
      if (cp_box(b[0], b[1], b[2], b[3], b[4], b[5], px, py, pz, best, l0)) break;
    }
  }
  const bool hit = best_id >= 0;
  d2_out[i] = hit ? best : INFINITY;
  tri_out[i] = hit ? best_id : -1;
  point_out[3 * (size_t)i] = hit ? bqx : 0.0; point_out[3 * (size_t)i + 1] = hit ? bqy : 0.0; point_out[3 * (size_t)i + 2] = hit ? bqz : 0.0;
  uv_out[2 * (size_t)i] = hit ? bu : 0.0; uv_out[2 * (size_t)i + 1] = hit ? bv : 0.0;
  if (counts) { counts[2 * (size_t)i] = n_nodes; counts[2 * (size_t)i + 1] = n_tris; }
}

}  // namespace neat
