// A training scene from a mesh and its wireframe (neat_amd/scenegen.py): shaded, anti-aliased pictures of the mesh and, per view, the
// visible runs of the ground-truth edges.  Both walk the tree of kernels_raycast.hpp with its rule (rc_walk), in float64 throughout;
// DESIGN 3l states the rule, tests/scenegen_f64.py restates it in numpy over all triangles, and the device equals it byte for byte.
// As in kernels_raycast.hpp every product is rounded on its own (rounded(), contraction off) and divisions and square roots are the
// correctly rounded ones.
//
// Cameras.  K [V][9] (fx = K[0], skew = K[1], cx = K[2], fy = K[4], cy = K[5]) and pose [V][16], camera-to-world [R | c], float64.
//   pixel (u, v) -> ray      yl = (v - cy) / fy, xl = ((u - cx) - skew yl) / fx, d = (R[.][0] xl + R[.][1] yl) + R[.][2], origin c
//   world X -> camera        Xc[a] = (R[0][a] (X - c)[0] + R[1][a] (X - c)[1]) + R[2][a] (X - c)[2]
//   camera -> picture        x = (fx (Xc[0] / Xc[2]) + skew (Xc[1] / Xc[2])) + cx, y = fy (Xc[1] / Xc[2]) + cy
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "device_util.hpp"
#include "graph_util.hpp"      // count_scan_kernel: the runs before each (view, edge)
#include "kernels_raycast.hpp"

namespace neat {

constexpr int SG_WG = 256;
constexpr int SG_WAVES = SG_WG / 64;
constexpr int SG_MAX_SS = 16;                 // sub-samples per pixel axis
constexpr int SG_MAX_SAMPLES = 1 << 16;       // samples of one edge in one view

struct SgCam {
  double fx, sk, cx, fy, cy;
  double R[3][3], c[3];
};

__device__ __forceinline__ SgCam sg_camera(const double* __restrict__ K, const double* __restrict__ pose, int view) {
  const double* k = K + 9 * (size_t)view;
  const double* p = pose + 16 * (size_t)view;
  SgCam m;
  m.fx = k[0]; m.sk = k[1]; m.cx = k[2]; m.fy = k[4]; m.cy = k[5];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int a = 0; a < 3; ++a) m.R[r][a] = p[4 * r + a];
    m.c[r] = p[4 * r + 3];
  }
  return m;
}

__device__ __forceinline__ double sg_norm3(double x, double y, double z) {
#pragma clang fp contract(off)
  return sqrt((rounded(x * x) + rounded(y * y)) + rounded(z * z));
}

// ---- pictures.  One lane per pixel; a wavefront is an 8 x 8 tile of pixels and a workgroup a 16 x 16 one.  The lane adds its ss^2
// samples in row-major order: colour = albedo (ambient + (1 - ambient) |n.d| / (|n| |d|)) on a hit, n = (v1 - v0) x (v2 - v0) of the
// closest triangle, background on a miss; byte = floor(255 mean + 0.5), clamped; mask = 255 where a sample hit
// The walk waits on dependent node loads, so the fifth wavefront a SIMD counts: with that budget the kernel takes 93 VGPRs and no scratch
// (left alone: 101 and four wavefronts; 0.214 s against 0.193 s for 236 M rays, NOTEBOOK "Scene generation")
struct SgShade { double albedo, ambient, background; };

__global__ __launch_bounds__(SG_WG) __attribute__((amdgpu_waves_per_eu(5, 5))) void scenegen_shade_kernel(const float* __restrict__ nodes, const double* __restrict__ tris, int nf, int L,
                                                              const double* __restrict__ K, const double* __restrict__ pose, int H, int W, int ss,
                                                              SgShade sh, unsigned char* __restrict__ rgb, unsigned char* __restrict__ mask) {
#pragma clang fp contract(off)
  const int tiles_x = (W + 15) >> 4, tiles_y = (H + 15) >> 4;
  const int tile = blockIdx.x % (tiles_x * tiles_y), view = blockIdx.x / (tiles_x * tiles_y);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int x = (tile % tiles_x) * 16 + (wave & 1) * 8 + (lane & 7);
  const int y = (tile / tiles_x) * 16 + (wave >> 1) * 8 + (lane >> 3);
  if (x >= W || y >= H) return;
  const SgCam m = sg_camera(K, pose, view);
  const double k1 = 1.0 - sh.ambient;
  double sum = 0.0;
  bool any = false;
  for (int j = 0; j < ss; ++j) {
    const double v = ((double)y + ((double)j + 0.5) / (double)ss) - 0.5;
    const double yl = (v - m.cy) / m.fy;
    for (int i = 0; i < ss; ++i) {
      const double u = ((double)x + ((double)i + 0.5) / (double)ss) - 0.5;
      const double xl = ((u - m.cx) - rounded(m.sk * yl)) / m.fx;
      RcRay r;
      r.ox = m.c[0]; r.oy = m.c[1]; r.oz = m.c[2];
      r.dx = (rounded(m.R[0][0] * xl) + rounded(m.R[0][1] * yl)) + m.R[0][2];
      r.dy = (rounded(m.R[1][0] * xl) + rounded(m.R[1][1] * yl)) + m.R[1][2];
      r.dz = (rounded(m.R[2][0] * xl) + rounded(m.R[2][1] * yl)) + m.R[2][2];
      rc_ray_setup(r);
      const RcHit h = rc_walk<false>(nodes, tris, nf, L, r, 0.0, (double)INFINITY);
      double col = sh.background;
      if (h.id >= 0) {
        const double* t = tris + (size_t)RC_TRI_STRIDE * h.leaf;
        const double e1x = t[3] - t[0], e1y = t[4] - t[1], e1z = t[5] - t[2];
        const double e2x = t[6] - t[0], e2y = t[7] - t[1], e2z = t[8] - t[2];
        const double nx = rounded(e1y * e2z) - rounded(e1z * e2y);
        const double ny = rounded(e1z * e2x) - rounded(e1x * e2z);
        const double nz = rounded(e1x * e2y) - rounded(e1y * e2x);
        const double nd = (rounded(nx * r.dx) + rounded(ny * r.dy)) + rounded(nz * r.dz);
        const double den = rounded(sg_norm3(nx, ny, nz) * sg_norm3(r.dx, r.dy, r.dz));
        col = rounded(sh.albedo * (sh.ambient + rounded(k1 * (fabs(nd) / den))));
        any = true;
      }
      sum += col;
    }
  }
  const double q = floor(rounded(255.0 * (sum / (double)(ss * ss))) + 0.5);
  const unsigned char byte = q >= 255.0 ? 255 : (q >= 0.0 ? (unsigned char)(int)q : 0);      // a NaN gives 0
  const size_t px = ((size_t)view * H + y) * W + x;
  rgb[3 * px] = byte; rgb[3 * px + 1] = byte; rgb[3 * px + 2] = byte;
  mask[px] = any ? 255 : 0;
}

// ---- edges.  The values of one (view, edge), the same in every lane of its wavefront
struct SgEdge {
  int n;                         // samples; 0: the edge gives nothing in this view
  bool cut0, cut1;               // the end was cut at z = near or at the border of the picture
  double ax, ay, bx, by;         // the projections of the ends after the cut at z = near
  double t0, t1;                 // Liang-Barsky: the part of a -> b inside the picture
  double Az, Bz;                 // camera depths of those ends
  double Aw[3], Bw[3];           // and their places in the world
  double c[3];
};

__device__ __forceinline__ void sg_to_camera(const SgCam& m, const double* __restrict__ X, double* __restrict__ Xc) {
#pragma clang fp contract(off)
  const double d0 = X[0] - m.c[0], d1 = X[1] - m.c[1], d2 = X[2] - m.c[2];
#pragma unroll
  for (int a = 0; a < 3; ++a) Xc[a] = (rounded(m.R[0][a] * d0) + rounded(m.R[1][a] * d1)) + rounded(m.R[2][a] * d2);
}

__device__ __forceinline__ void sg_project(const SgCam& m, const double* __restrict__ Xc, double& x, double& y) {
#pragma clang fp contract(off)
  const double ix = Xc[0] / Xc[2], iy = Xc[1] / Xc[2];
  x = (rounded(m.fx * ix) + rounded(m.sk * iy)) + m.cx;
  y = rounded(m.fy * iy) + m.cy;
}

// one Liang-Barsky boundary: false = the segment lies outside
__device__ __forceinline__ bool sg_clip(double p, double q, double& t0, double& t1) {
  if (p == 0.0) return !(q < 0.0);
  const double r = q / p;
  if (p < 0.0) {
    if (r > t1) return false;
    if (r > t0) t0 = r;
  } else {
    if (r < t0) return false;
    if (r < t1) t1 = r;
  }
  return true;
}

// the place of parameter tau on the cut 2-D segment; tau = 1 is the end itself
__device__ __forceinline__ void sg_point2(const SgEdge& e, double tau, double& x, double& y) {
#pragma clang fp contract(off)
  x = tau == 1.0 ? e.bx : e.ax + rounded(tau * (e.bx - e.ax));
  y = tau == 1.0 ? e.by : e.ay + rounded(tau * (e.by - e.ay));
}

__device__ __forceinline__ double sg_len2(double x0, double y0, double x1, double y1) {
#pragma clang fp contract(off)
  const double dx = x1 - x0, dy = y1 - y0;
  return sqrt(rounded(dx * dx) + rounded(dy * dy));
}

__device__ __forceinline__ double sg_tau(const SgEdge& e, int k) {
#pragma clang fp contract(off)
  if (k == 0) return e.t0;
  if (k == e.n - 1) return e.t1;
  return e.t0 + rounded((e.t1 - e.t0) * ((double)k / (double)(e.n - 1)));
}

// the 3-D point of parameter tau by the perspective-correct parameter sigma; sigma = 1 is the end itself
__device__ __forceinline__ void sg_point3(const SgEdge& e, double tau, double* __restrict__ X) {
#pragma clang fp contract(off)
  const double wa = rounded(tau * e.Az), wb = rounded((1.0 - tau) * e.Bz);
  const double sigma = wa / (wa + wb);
#pragma unroll
  for (int a = 0; a < 3; ++a) X[a] = sigma == 1.0 ? e.Bw[a] : e.Aw[a] + rounded(sigma * (e.Bw[a] - e.Aw[a]));
}

__device__ __forceinline__ SgEdge sg_edge_setup(const SgCam& m, const double* __restrict__ P0, const double* __restrict__ P1, int H, int W,
                                                double step, double near) {
#pragma clang fp contract(off)
  SgEdge e;
  e.n = 0; e.cut0 = false; e.cut1 = false; e.t0 = 0.0; e.t1 = 1.0;
#pragma unroll
  for (int a = 0; a < 3; ++a) { e.Aw[a] = P0[a]; e.Bw[a] = P1[a]; e.c[a] = m.c[a]; }
  double A[3], B[3];
  sg_to_camera(m, P0, A);
  sg_to_camera(m, P1, B);
  e.ax = e.ay = e.bx = e.by = 0.0; e.Az = A[2]; e.Bz = B[2];
  if (!(A[2] >= near) && !(B[2] >= near)) return e;
  if (!(A[2] >= near)) {
    const double s = (near - A[2]) / (B[2] - A[2]);
    A[0] = A[0] + rounded(s * (B[0] - A[0])); A[1] = A[1] + rounded(s * (B[1] - A[1])); A[2] = near;
#pragma unroll
    for (int a = 0; a < 3; ++a) e.Aw[a] = P0[a] + rounded(s * (P1[a] - P0[a]));
    e.cut0 = true;
  } else if (!(B[2] >= near)) {
    const double s = (near - B[2]) / (A[2] - B[2]);
    B[0] = B[0] + rounded(s * (A[0] - B[0])); B[1] = B[1] + rounded(s * (A[1] - B[1])); B[2] = near;
#pragma unroll
    for (int a = 0; a < 3; ++a) e.Bw[a] = P1[a] + rounded(s * (P0[a] - P1[a]));
    e.cut1 = true;
  }
  e.Az = A[2]; e.Bz = B[2];
  sg_project(m, A, e.ax, e.ay);
  sg_project(m, B, e.bx, e.by);
  const double dx = e.bx - e.ax, dy = e.by - e.ay;
  if (!sg_clip(-dx, e.ax - (-0.5), e.t0, e.t1) || !sg_clip(dx, ((double)W - 0.5) - e.ax, e.t0, e.t1) ||
      !sg_clip(-dy, e.ay - (-0.5), e.t0, e.t1) || !sg_clip(dy, ((double)H - 0.5) - e.ay, e.t0, e.t1))
    return e;
  if (e.t0 > 0.0) e.cut0 = true;
  if (e.t1 < 1.0) e.cut1 = true;
  double x0, y0, x1, y1;
  sg_point2(e, e.t0, x0, y0);
  sg_point2(e, e.t1, x1, y1);
  const double q = ceil(sg_len2(x0, y0, x1, y1) / step);
  if (!(q >= 0.0)) return e;                                   // a NaN: a non-finite junction or camera
  e.n = q >= (double)(SG_MAX_SAMPLES - 1) ? SG_MAX_SAMPLES : (int)q + 1;      // the host has refused pictures that could need more
  return e;
}

// sample k is visible: the ray from the camera centre towards it meets no triangle with 0 <= t < |X - c| - bias
__device__ __forceinline__ bool sg_visible(const float* __restrict__ nodes, const double* __restrict__ tris, int nf, int L, const SgEdge& e, int k,
                                           double bias) {
#pragma clang fp contract(off)
  double X[3];
  sg_point3(e, sg_tau(e, k), X);
  const double dx = X[0] - e.c[0], dy = X[1] - e.c[1], dz = X[2] - e.c[2];
  const double dist = sg_norm3(dx, dy, dz);
  if (!(dist > bias)) return false;
  RcRay r;
  r.ox = e.c[0]; r.oy = e.c[1]; r.oz = e.c[2];
  r.dx = dx / dist; r.dy = dy / dist; r.dz = dz / dist;
  rc_ray_setup(r);
  return rc_walk<true>(nodes, tris, nf, L, r, 0.0, dist - bias).id < 0;
}

// One wavefront per (view, edge), 64 samples a round: __ballot gives the word of visible samples, every lane walks its bits and carries
// the open run into the next round.  FILL = false counts the runs kept (2-D length >= min_len) into cnt [V E]; FILL = true writes run
// number i of the pair at off[pair] + i, so the list is in (view, edge, run) order: idx [N][4] (view, edge, first, last sample),
// p2 [N][4], p3 [N][6] the ends in the picture and in the world, junc [N][2]: the end is the junction itself
template <bool FILL>
__global__ __launch_bounds__(SG_WG) void scenegen_edge_kernel(const float* __restrict__ nodes, const double* __restrict__ tris, int nf, int L,
                                                             const double* __restrict__ junctions, const int* __restrict__ edges, int E,
                                                             const double* __restrict__ K, const double* __restrict__ pose, int V, int H, int W,
                                                             double step, double min_len, double bias, double near, int* __restrict__ cnt,
                                                             const int* __restrict__ off, int N, int* __restrict__ idx, double* __restrict__ p2,
                                                             double* __restrict__ p3, unsigned char* __restrict__ junc) {
  const int lane = threadIdx.x & 63;
  const long long pair = (long long)blockIdx.x * SG_WAVES + (threadIdx.x >> 6);
  if (pair >= (long long)V * E) return;                        // whole wavefronts leave; the kernel has no barrier
  const int view = (int)(pair / E), edge = (int)(pair % E);
  const SgCam m = sg_camera(K, pose, view);
  const SgEdge e = sg_edge_setup(m, junctions + 3 * (size_t)edges[2 * (size_t)edge], junctions + 3 * (size_t)edges[2 * (size_t)edge + 1], H, W, step,
                                 near);
  int runs = 0, open = -1;
  const int base_out = FILL ? off[pair] : 0;
  for (int base = 0; base <= e.n; base += 64) {               // one round past the last sample closes a run that reaches it
    const int k = base + lane;
    const bool vis = k < e.n && sg_visible(nodes, tris, nf, L, e, k, bias);
    const unsigned long long word = __ballot(vis);
    for (int b = 0; b < 64 && base + b <= e.n; ++b) {
      const int kb = base + b;
      const bool v = (word >> b) & 1ull;
      if (v && open < 0) open = kb;
      if (!v && open >= 0) {                                    // the run [open, kb - 1]
        const int last = kb - 1;
        double x0, y0, x1, y1;
        sg_point2(e, sg_tau(e, open), x0, y0);
        sg_point2(e, sg_tau(e, last), x1, y1);
        if (sg_len2(x0, y0, x1, y1) >= min_len) {
          if (FILL && lane == 0 && base_out + runs < N) {
            const size_t o = (size_t)(base_out + runs);
            double X0[3], X1[3];
            sg_point3(e, sg_tau(e, open), X0);
            sg_point3(e, sg_tau(e, last), X1);
            idx[4 * o] = view; idx[4 * o + 1] = edge; idx[4 * o + 2] = open; idx[4 * o + 3] = last;
            p2[4 * o] = x0; p2[4 * o + 1] = y0; p2[4 * o + 2] = x1; p2[4 * o + 3] = y1;
#pragma unroll
            for (int a = 0; a < 3; ++a) { p3[6 * o + a] = X0[a]; p3[6 * o + 3 + a] = X1[a]; }
            junc[2 * o] = (open == 0 && !e.cut0) ? 1 : 0;
            junc[2 * o + 1] = (last == e.n - 1 && !e.cut1) ? 1 : 0;
          }
          ++runs;
        }
        open = -1;
      }
    }
  }
  if (!FILL && lane == 0) cnt[pair] = runs;
}

}  // namespace neat
