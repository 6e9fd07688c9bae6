// Headless pictures of a wireframe and of the surface mesh behind it (the reference's code/visualization/show.py draws through an open3d
// window and matplotlib's savefig on a workstation; code/evaluation/show-mesh.py shows the mesh alone): a depth pass over the triangles, a
// coverage pass over the segments, one over the endpoint discs, and one resolve to bytes.  All F frames of a turntable travel in one launch.
// Every geometric decision is float64 with every product and sum rounded on its own (fp contraction is off in these functions and the
// operands pass through rounded()), so tests/show_f64.py restates the picture in numpy and the buffers compare bit for bit up to the last
// place of a square root or a quotient.  Integer atomics only: a 64-bit unsigned minimum on the depth key and an unsigned maximum on the
// bits of a non-negative float32 coverage.  A minimum and a maximum commute, so no result depends on the order the atomics land in.
// No kernel loops without a bound that is fixed before it starts.
//
// Definitions (p = (x, y) = (column j, row i) is a pixel centre):
//   camera      Xc = ((R0 X0 + R1 X1) + R2 X2) + T per row; x = (fx Xc.x) / Xc.z + cx, y = (fy Xc.y) / Xc.z + cy, depth z = Xc.z
//   dropped     a primitive with a non-finite coordinate (world, camera or screen) or a screen coordinate beyond 2^40 in magnitude;
//               a segment with both ends at z < near; a triangle with any vertex at z < near or with A = 0
//   near cut    the end b behind the plane moves to Pb + t (Po - Pb), t = (near - zb) / (zo - zb), in camera space; its z becomes near
//   triangle    E_ab(p) = (b.x - a.x)(p.y - a.y) - (b.y - a.y)(p.x - a.x), A = E_ab(c); covered iff sign(A) E >= 0 for ab, bc, ca;
//               1/z = (E_bc/A / z_a + E_ca/A / z_b) + E_ab/A / z_c; key = bits(float32(z)) << 32 | triangle index, the minimum wins
//   segment     u = clamp(((p - P0) . d) / (d . d), 0, 1) (0 for a zero-length one), q = P0 + u d, dist = |p - q|,
//               cov = clamp(hw - dist, 0, 1) with hw = width / 2 + 0.5; 1/z = (1 - u) / z0 + u / z1; visible iff z <= depth(p) + bias;
//               C(p) = max over segments of float32(cov (visible ? 1 : hidden_alpha))
//   point       the same with dist to the projected point, hw = radius + 0.5 and the point's own depth
//   resolve     rgb = base (1 - C) + line C, then rgb (1 - Cp) + point Cp; base = bg or mesh (0.25 + 0.75 |n_z| / |n|) with n the camera-space
//               cross product (b - a) x (c - a) of the winning triangle; byte = floor(255 rgb + 0.5)
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>

#include "device_util.hpp"     // rounded

namespace neat {

constexpr int SHOW_WG = 256;
constexpr int SHOW_CAM_DOUBLES = 21;                            // K [3,3] then [R|T] [3,4], row-major
constexpr int SHOW_TRI_SMALL = 32;                              // a triangle whose clipped box holds at most this many pixels stays with its lane
constexpr int SHOW_TRI_BANDS = 16;                              // bands of rows a queued box is cut into
constexpr int SHOW_QUEUE_CAP = 1 << 20;                         // boxes the queue of large triangles holds
constexpr int SHOW_LARGE_BLOCKS = 2048;                         // workgroups of the pass over the queue
constexpr double SHOW_COORD_MAX = 1099511627776.0;              // 2^40
constexpr unsigned long long SHOW_KEY_CLEAR = 0x7f800000ffffffffull;      // depth +inf, no triangle

struct ShowCam { double fx, fy, cx, cy, R[9], T[3]; };

__device__ __forceinline__ ShowCam show_cam(const double* __restrict__ cams, int f) {
  const double* c = cams + (size_t)SHOW_CAM_DOUBLES * f;
  ShowCam m;
  m.fx = c[0]; m.cx = c[2]; m.fy = c[4]; m.cy = c[5];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    m.R[3 * r] = c[9 + 4 * r]; m.R[3 * r + 1] = c[10 + 4 * r]; m.R[3 * r + 2] = c[11 + 4 * r]; m.T[r] = c[12 + 4 * r];
  }
  return m;
}
__device__ __forceinline__ bool show_finite3(const double* v) { return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]); }
__device__ __forceinline__ void show_to_cam(const ShowCam& m, const double* X, double* Xc) {
#pragma clang fp contract(off)
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double a = rounded(m.R[3 * r] * X[0]), b = rounded(m.R[3 * r + 1] * X[1]), c = rounded(m.R[3 * r + 2] * X[2]);
    Xc[r] = rounded(rounded(rounded(a + b) + c) + m.T[r]);
  }
}
// -> false: a screen coordinate that is not finite or beyond 2^40
__device__ __forceinline__ bool show_project(const ShowCam& m, const double* Xc, double* x, double* y) {
#pragma clang fp contract(off)
  *x = rounded(rounded(rounded(m.fx * Xc[0]) / Xc[2]) + m.cx);
  *y = rounded(rounded(rounded(m.fy * Xc[1]) / Xc[2]) + m.cy);
  return fabs(*x) <= SHOW_COORD_MAX && fabs(*y) <= SHOW_COORD_MAX;          // false for a NaN too
}
__device__ __forceinline__ int show_clampi(double v, int lo, int hi) {       // v finite
  return (int)fmin(fmax(v, (double)lo), (double)hi);
}
__device__ __forceinline__ double show_depth_of(unsigned long long key) { return (double)__uint_as_float((unsigned)(key >> 32)); }

// ---- (a) clear ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SHOW_WG) void show_clear_kernel(unsigned long long* __restrict__ key, unsigned* __restrict__ cov,
                                                             unsigned* __restrict__ covp, int* __restrict__ status, long long total) {
  const long long p = (long long)blockIdx.x * SHOW_WG + threadIdx.x;
  if (p == 0) status[0] = 0;
  if (p >= total) return;
  key[p] = SHOW_KEY_CLEAR; cov[p] = 0u; covp[p] = 0u;
}

// ---- (b) the mesh's depth keys -----------------------------------------------------------------------------------------------------------
struct ShowTri {
  double ax, ay, bx, by, cx, cy, za, zb, zc, A;
  int x0, x1, y0, y1;        // the box of pixel centres, clipped to the frame; empty if x1 < x0 or y1 < y0
};
// -> 0 drawn, 1 dropped, 2 a vertex index out of range
__device__ __forceinline__ int show_tri_setup(const double* __restrict__ verts, int nv, const int* __restrict__ faces, int k, const ShowCam& m,
                                              double near, int H, int W, ShowTri& T) {
#pragma clang fp contract(off)
  const int i0 = faces[3 * (size_t)k], i1 = faces[3 * (size_t)k + 1], i2 = faces[3 * (size_t)k + 2];
  if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= nv || i1 >= nv || i2 >= nv) return 2;
  const double* va = verts + 3 * (size_t)i0;
  const double* vb = verts + 3 * (size_t)i1;
  const double* vc = verts + 3 * (size_t)i2;
  if (!show_finite3(va) || !show_finite3(vb) || !show_finite3(vc)) return 1;
  double a[3], b[3], c[3];
  show_to_cam(m, va, a); show_to_cam(m, vb, b); show_to_cam(m, vc, c);
  if (!show_finite3(a) || !show_finite3(b) || !show_finite3(c)) return 1;
  if (a[2] < near || b[2] < near || c[2] < near) return 1;
  if (!show_project(m, a, &T.ax, &T.ay) || !show_project(m, b, &T.bx, &T.by) || !show_project(m, c, &T.cx, &T.cy)) return 1;
  T.za = a[2]; T.zb = b[2]; T.zc = c[2];
  T.A = rounded(rounded(rounded(T.bx - T.ax) * rounded(T.cy - T.ay)) - rounded(rounded(T.by - T.ay) * rounded(T.cx - T.ax)));
  if (!(T.A != 0.0) || !isfinite(T.A)) return 1;
  T.x0 = show_clampi(ceil(fmin(fmin(T.ax, T.bx), T.cx)), 0, W);
  T.x1 = show_clampi(floor(fmax(fmax(T.ax, T.bx), T.cx)), -1, W - 1);
  T.y0 = show_clampi(ceil(fmin(fmin(T.ay, T.by), T.cy)), 0, H);
  T.y1 = show_clampi(floor(fmax(fmax(T.ay, T.by), T.cy)), -1, H - 1);
  return 0;
}
__device__ __forceinline__ double show_edge(double ax, double ay, double bx, double by, double px, double py) {
#pragma clang fp contract(off)
  return rounded(rounded(rounded(bx - ax) * rounded(py - ay)) - rounded(rounded(by - ay) * rounded(px - ax)));
}
__device__ __forceinline__ void show_tri_pixel(const ShowTri& T, int j, int i, unsigned k, unsigned long long* __restrict__ key_row) {
#pragma clang fp contract(off)
  const double px = (double)j, py = (double)i;
  double eab = show_edge(T.ax, T.ay, T.bx, T.by, px, py);
  double ebc = show_edge(T.bx, T.by, T.cx, T.cy, px, py);
  double eca = show_edge(T.cx, T.cy, T.ax, T.ay, px, py);
  const bool in = T.A > 0.0 ? (eab >= 0.0 && ebc >= 0.0 && eca >= 0.0) : (eab <= 0.0 && ebc <= 0.0 && eca <= 0.0);
  if (!in) return;
  const double la = rounded(ebc / T.A), lb = rounded(eca / T.A), lc = rounded(eab / T.A);
  const double iz = rounded(rounded(rounded(la / T.za) + rounded(lb / T.zb)) + rounded(lc / T.zc));
  const float zf = (float)rounded(1.0 / iz);
  if (!(zf > 0.0f)) return;                       // weights that round to nothing: no depth to order by
  atomicMin(&key_row[j], ((unsigned long long)__float_as_uint(zf) << 32) | k);
}

// all 64 lanes walk rows [r0, r1) of a triangle's clipped box, 64 pixels per step
__device__ __forceinline__ void show_tri_rows(const ShowTri& S, int r0, int r1, unsigned k, unsigned long long* __restrict__ kf, int W, int lane) {
  const int bw = S.x1 - S.x0 + 1;
  const long long n = (long long)bw * (r1 - r0);
  const long long steps = (n + 63) / 64;
  for (long long s = 0; s < steps; ++s) {
    const long long q = s * 64 + lane;
    if (q < n) {
      const int i = r0 + (int)(q / bw), j = S.x0 + (int)(q % bw);
      show_tri_pixel(S, j, i, k, kf + (size_t)i * W);
    }
  }
}

// one lane per (frame, triangle): a small box is walked by its lane.  A large one is queued (its index t = f nf + k) for
// show_mesh_large_kernel, which spreads the queue over the device; the queue's order is whatever the counter hands out and changes no
// result (every pixel takes a minimum).  What the queue cannot hold is walked here, one box after the other by all 64 lanes, each of
// which sets the triangle up again (uniform loads) rather than passing thirteen doubles through shuffles.
__global__ __launch_bounds__(SHOW_WG) void show_mesh_kernel(const double* __restrict__ verts, int nv, const int* __restrict__ faces, int nf,
                                                            const double* __restrict__ cams, int F, int H, int W, double near,
                                                            unsigned long long* __restrict__ key, int* __restrict__ status,
                                                            unsigned long long* __restrict__ queued, long long* __restrict__ queue, int cap) {
  const long long t = (long long)blockIdx.x * SHOW_WG + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const long long t_wave = t - lane;
  const bool live = t < (long long)F * nf;
  int f = 0, k = 0, npix = 0;
  ShowTri T;
  if (live) {
    f = (int)(t / nf); k = (int)(t % nf);
    const ShowCam m = show_cam(cams, f);
    const int r = show_tri_setup(verts, nv, faces, k, m, near, H, W, T);
    if (r == 2) status[0] = 1;
    if (r == 0 && T.x1 >= T.x0 && T.y1 >= T.y0) {
      const long long n = (long long)(T.x1 - T.x0 + 1) * (T.y1 - T.y0 + 1);
      npix = (int)min(n, (long long)INT_MAX);
    }
  }
  if (npix > 0 && npix <= SHOW_TRI_SMALL) {
    const int bw = T.x1 - T.x0 + 1;
    unsigned long long* kf = key + (size_t)f * H * W;
    for (int q = 0; q < npix; ++q) {
      const int i = T.y0 + q / bw, j = T.x0 + q % bw;
      show_tri_pixel(T, j, i, (unsigned)k, kf + (size_t)i * W);
    }
  }
  const bool large = npix > SHOW_TRI_SMALL;
  unsigned long long big = __ballot(large);
  if (big != 0) {
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(queued, (unsigned long long)__popcll(big));
    base = __shfl(base, 0);
    const unsigned long long slot = base + (unsigned long long)__popcll(big & ((1ull << lane) - 1ull));
    const bool fits = large && slot < (unsigned long long)cap;
    if (fits) queue[slot] = t;
    big = __ballot(large && !fits);
  }
  for (int g = 0; g < 64 && big != 0; ++g) {
    const int src = __ffsll((long long)big) - 1;
    big &= big - 1;
    const long long ts = t_wave + src;
    const int fs = (int)(ts / nf), ks = (int)(ts % nf);
    const ShowCam m = show_cam(cams, fs);
    ShowTri S;
    if (show_tri_setup(verts, nv, faces, ks, m, near, H, W, S) != 0) continue;
    show_tri_rows(S, S.y0, S.y1 + 1, (unsigned)ks, key + (size_t)fs * H * W, W, lane);
  }
}

// the queued boxes, each cut into SHOW_TRI_BANDS bands of rows: a fixed grid of wavefronts takes (box, band) units in turn.  The number of
// units is read once, before the loop
__global__ __launch_bounds__(SHOW_WG) void show_mesh_large_kernel(const double* __restrict__ verts, int nv, const int* __restrict__ faces, int nf,
                                                                  const double* __restrict__ cams, int F, int H, int W, double near,
                                                                  unsigned long long* __restrict__ key,
                                                                  const unsigned long long* __restrict__ queued,
                                                                  const long long* __restrict__ queue, int cap) {
  const int lane = threadIdx.x & 63;
  const long long wave = (long long)blockIdx.x * (SHOW_WG / 64) + (threadIdx.x >> 6), waves = (long long)gridDim.x * (SHOW_WG / 64);
  const unsigned long long have = *queued;
  const long long units = (long long)(have < (unsigned long long)cap ? have : (unsigned long long)cap) * SHOW_TRI_BANDS;
  for (long long u = wave; u < units; u += waves) {
    const long long ts = queue[u / SHOW_TRI_BANDS];
    const int band = (int)(u % SHOW_TRI_BANDS);
    if (ts < 0 || ts >= (long long)F * nf) continue;
    const int fs = (int)(ts / nf), ks = (int)(ts % nf);
    const ShowCam m = show_cam(cams, fs);
    ShowTri S;
    if (show_tri_setup(verts, nv, faces, ks, m, near, H, W, S) != 0 || S.x1 < S.x0 || S.y1 < S.y0) continue;
    const long long bh = S.y1 - S.y0 + 1;
    const int r0 = S.y0 + (int)(bh * band / SHOW_TRI_BANDS), r1 = S.y0 + (int)(bh * (band + 1) / SHOW_TRI_BANDS);
    show_tri_rows(S, r0, r1, (unsigned)ks, key + (size_t)fs * H * W, W, lane);
  }
}

// ---- (c) the segments' coverage: a wavefront per (frame, segment) walks the major axis 64 pixels at a time, a lane the few pixels across ---
struct ShowSeg { double x0, y0, z0, x1, y1, z1; };
__device__ __forceinline__ bool show_seg_setup(const double* __restrict__ P, const ShowCam& m, double near, ShowSeg& S) {
#pragma clang fp contract(off)
  if (!show_finite3(P) || !show_finite3(P + 3)) return false;
  double a[3], b[3];
  show_to_cam(m, P, a); show_to_cam(m, P + 3, b);
  if (!show_finite3(a) || !show_finite3(b)) return false;
  const bool abehind = a[2] < near, bbehind = b[2] < near;
  if (abehind && bbehind) return false;
  if (abehind || bbehind) {
    double* e = abehind ? a : b;           // the end behind the plane
    const double* o = abehind ? b : a;
    const double t = rounded(rounded(near - e[2]) / rounded(o[2] - e[2]));
    e[0] = rounded(e[0] + rounded(t * rounded(o[0] - e[0])));
    e[1] = rounded(e[1] + rounded(t * rounded(o[1] - e[1])));
    e[2] = near;
  }
  if (!show_project(m, a, &S.x0, &S.y0) || !show_project(m, b, &S.x1, &S.y1)) return false;
  S.z0 = a[2]; S.z1 = b[2];
  return true;
}
// the value of pixel (px, py) under the segment: cov (visible ? 1 : alpha) as float32; 0 where the segment does not reach
__device__ __forceinline__ float show_seg_pixel(const ShowSeg& S, double dx, double dy, double l2, double px, double py, double hw, double bias,
                                                double alpha, unsigned long long key) {
#pragma clang fp contract(off)
  double u = 0.0;
  if (l2 > 0.0) {
    const double num = rounded(rounded(rounded(px - S.x0) * dx) + rounded(rounded(py - S.y0) * dy));
    u = fmin(fmax(rounded(num / l2), 0.0), 1.0);
  }
  const double qx = rounded(S.x0 + rounded(u * dx)), qy = rounded(S.y0 + rounded(u * dy));
  const double ex = rounded(px - qx), ey = rounded(py - qy);
  const double d = sqrt(rounded(rounded(ex * ex) + rounded(ey * ey)));
  const double cov = fmin(fmax(rounded(hw - d), 0.0), 1.0);
  if (!(cov > 0.0)) return 0.0f;
  const double iz = rounded(rounded(rounded(1.0 - u) / S.z0) + rounded(u / S.z1));
  const double z = rounded(1.0 / iz);
  const bool visible = z <= rounded(show_depth_of(key) + bias);
  return (float)(visible ? cov : rounded(cov * alpha));
}

__global__ __launch_bounds__(SHOW_WG) void show_lines_kernel(const double* __restrict__ lines, int n, const double* __restrict__ cams, int F,
                                                             int H, int W, double near, double hw, double bias, double alpha,
                                                             const unsigned long long* __restrict__ key, unsigned* __restrict__ cov) {
#pragma clang fp contract(off)
  const long long wv = (long long)blockIdx.x * (SHOW_WG / 64) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (wv >= (long long)F * n) return;
  const int f = (int)(wv / n), s = (int)(wv % n);
  const ShowCam m = show_cam(cams, f);
  ShowSeg S;
  if (!show_seg_setup(lines + 6 * (size_t)s, m, near, S)) return;
  const double dx = rounded(S.x1 - S.x0), dy = rounded(S.y1 - S.y0);
  const double l2 = rounded(rounded(dx * dx) + rounded(dy * dy));
  // the walk only has to visit every pixel nearer than hw; what it writes is show_seg_pixel's value.  Along the major axis a, inside the
  // segment's own range a pixel nearer than hw lies within sqrt(2) hw of the line across the minor axis (the slope is at most 1); past an
  // end, within 2 hw of that end
  const bool xmajor = fabs(dx) >= fabs(dy);
  const double a0 = xmajor ? S.x0 : S.y0, a1 = xmajor ? S.x1 : S.y1, b0 = xmajor ? S.y0 : S.x0, b1 = xmajor ? S.y1 : S.x1;
  const int An = xmajor ? W : H, Bn = xmajor ? H : W;
  const double amin = fmin(a0, a1), amax = fmax(a0, a1);
  const int lo = show_clampi(floor(amin - hw - 1e-3), 0, An), hi = show_clampi(ceil(amax + hw + 1e-3), -1, An - 1);
  if (hi < lo) return;
  const double slope = amax > amin ? (b1 - b0) / (a1 - a0) : 0.0;
  const unsigned long long* kf = key + (size_t)f * H * W;
  unsigned* cf = cov + (size_t)f * H * W;
  const int steps = (hi - lo) / 64 + 1;
  for (int st = 0; st < steps; ++st) {
    const int a = lo + st * 64 + lane;
    if (a > hi) continue;
    const double ad = (double)a, ac = fmin(fmax(ad, amin), amax);
    const double bc = b0 + (ac - a0) * slope;      // |ac - a0| <= 2^41 and |slope| <= 1: rounded to within 2^-10 of a pixel; the reaches below
                                                   // are sqrt(2) hw and 2 hw where hw itself would do (a pixel within hw of the segment is within
                                                   // hw of the line), so the slack that matters is (sqrt(2) - 1) hw >= 0.2, not the 1e-3
    const double reach = ((ad >= amin && ad <= amax) ? hw * 1.4143 : hw * 2.0) + 1e-3;
    const int blo = show_clampi(floor(bc - reach), 0, Bn), bhi = show_clampi(ceil(bc + reach), -1, Bn - 1);
    for (int b = blo; b <= bhi; ++b) {
      const int j = xmajor ? a : b, i = xmajor ? b : a;
      const size_t p = (size_t)i * W + j;
      const float v = show_seg_pixel(S, dx, dy, l2, (double)j, (double)i, hw, bias, alpha, kf[p]);
      if (v > 0.0f) atomicMax(&cf[p], __float_as_uint(v));
    }
  }
}

// ---- (d) the endpoint discs: a lane per (frame, point) ------------------------------------------------------------------------------------
__global__ __launch_bounds__(SHOW_WG) void show_points_kernel(const double* __restrict__ pts, int n, const double* __restrict__ cams, int F,
                                                              int H, int W, double near, double hw, double bias, double alpha,
                                                              const unsigned long long* __restrict__ key, unsigned* __restrict__ covp) {
#pragma clang fp contract(off)
  const long long t = (long long)blockIdx.x * SHOW_WG + threadIdx.x;
  if (t >= (long long)F * n) return;
  const int f = (int)(t / n), s = (int)(t % n);
  const ShowCam m = show_cam(cams, f);
  const double* P = pts + 3 * (size_t)s;
  if (!show_finite3(P)) return;
  double c[3];
  show_to_cam(m, P, c);
  if (!show_finite3(c) || c[2] < near) return;
  ShowSeg S;
  if (!show_project(m, c, &S.x0, &S.y0)) return;
  S.x1 = S.x0; S.y1 = S.y0; S.z0 = S.z1 = c[2];
  const int j0 = show_clampi(floor(S.x0 - hw - 1e-3), 0, W), j1 = show_clampi(ceil(S.x0 + hw + 1e-3), -1, W - 1);
  const int i0 = show_clampi(floor(S.y0 - hw - 1e-3), 0, H), i1 = show_clampi(ceil(S.y0 + hw + 1e-3), -1, H - 1);
  const unsigned long long* kf = key + (size_t)f * H * W;
  unsigned* cf = covp + (size_t)f * H * W;
  for (int i = i0; i <= i1; ++i)
    for (int j = j0; j <= j1; ++j) {
      const size_t p = (size_t)i * W + j;
      const float v = show_seg_pixel(S, 0.0, 0.0, 0.0, (double)j, (double)i, hw, bias, alpha, kf[p]);
      if (v > 0.0f) atomicMax(&cf[p], __float_as_uint(v));
    }
}

// ---- (e) resolve: four pixels per lane, 16-byte loads of the three buffers, three 4-byte stores of the twelve bytes -----------------------
struct ShowStyle { double bg[3], line[3], point[3], mesh[3]; };

__device__ __forceinline__ double show_shade(const double* __restrict__ verts, int nv, const int* __restrict__ faces, unsigned k,
                                             const ShowCam& m) {
#pragma clang fp contract(off)
  const int i0 = faces[3 * (size_t)k], i1 = faces[3 * (size_t)k + 1], i2 = faces[3 * (size_t)k + 2];
  if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= nv || i1 >= nv || i2 >= nv) return 0.25;      // not the arrays the keys were made from
  double a[3], b[3], c[3];
  show_to_cam(m, verts + 3 * (size_t)i0, a);
  show_to_cam(m, verts + 3 * (size_t)i1, b);
  show_to_cam(m, verts + 3 * (size_t)i2, c);
  const double ux = rounded(b[0] - a[0]), uy = rounded(b[1] - a[1]), uz = rounded(b[2] - a[2]);
  const double vx = rounded(c[0] - a[0]), vy = rounded(c[1] - a[1]), vz = rounded(c[2] - a[2]);
  const double nx = rounded(rounded(uy * vz) - rounded(uz * vy));
  const double ny = rounded(rounded(uz * vx) - rounded(ux * vz));
  const double nz = rounded(rounded(ux * vy) - rounded(uy * vx));
  const double len = sqrt(rounded(rounded(rounded(nx * nx) + rounded(ny * ny)) + rounded(nz * nz)));
  const double c_ = len > 0.0 ? rounded(fabs(nz) / len) : 0.0;
  return rounded(0.25 + rounded(0.75 * c_));
}
__device__ __forceinline__ unsigned show_pixel_rgb(unsigned long long key, float C, float Cp, const double* __restrict__ verts, int nv,
                                                   const int* __restrict__ faces, int nf, const ShowCam& m, const ShowStyle& st) {
#pragma clang fp contract(off)
  const unsigned k = (unsigned)key;
  const bool hit = k < (unsigned)nf;                 // 0xffffffff: no triangle
  const double shade = hit ? show_shade(verts, nv, faces, k, m) : 1.0;
  const double c = (double)C, cp = (double)Cp;
  unsigned out = 0;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    double v = hit ? rounded(st.mesh[ch] * shade) : st.bg[ch];
    v = rounded(rounded(v * rounded(1.0 - c)) + rounded(st.line[ch] * c));
    v = rounded(rounded(v * rounded(1.0 - cp)) + rounded(st.point[ch] * cp));
    const double b = fmin(fmax(floor(rounded(rounded(255.0 * v) + 0.5)), 0.0), 255.0);
    out |= (unsigned)b << (8 * ch);
  }
  return out;
}
__global__ __launch_bounds__(SHOW_WG) void show_resolve_kernel(const double* __restrict__ verts, int nv, const int* __restrict__ faces,
                                                               int nf, const double* __restrict__ cams, int H, int W, long long total, ShowStyle st,
                                                               const unsigned long long* __restrict__ key, const float* __restrict__ cov,
                                                               const float* __restrict__ covp, const int* __restrict__ status,
                                                               unsigned char* __restrict__ out) {
  const long long p0 = ((long long)blockIdx.x * SHOW_WG + threadIdx.x) * 4;
  if (p0 >= total || status[0] != 0) return;             // a face index out of range: the picture is not written
  const long long hw = (long long)H * W;
  if (p0 + 4 <= total) {
    const ulonglong2 k01 = *reinterpret_cast<const ulonglong2*>(key + p0), k23 = *reinterpret_cast<const ulonglong2*>(key + p0 + 2);
    const float4 c = *reinterpret_cast<const float4*>(cov + p0), cp = *reinterpret_cast<const float4*>(covp + p0);
    const unsigned long long ks[4] = {k01.x, k01.y, k23.x, k23.y};
    const float cs[4] = {c.x, c.y, c.z, c.w}, cps[4] = {cp.x, cp.y, cp.z, cp.w};
    unsigned rgb[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const ShowCam m = show_cam(cams, (int)((p0 + q) / hw));
      rgb[q] = show_pixel_rgb(ks[q], cs[q], cps[q], verts, nv, faces, nf, m, st);
    }
    unsigned* o = reinterpret_cast<unsigned*>(out + 3 * p0);       // 12 p0' bytes in: 4-byte aligned
    o[0] = rgb[0] | (rgb[1] << 24);
    o[1] = (rgb[1] >> 8) | (rgb[2] << 16);
    o[2] = (rgb[2] >> 16) | (rgb[3] << 8);
  } else {
    for (long long p = p0; p < total; ++p) {
      const ShowCam m = show_cam(cams, (int)(p / hw));
      const unsigned rgb = show_pixel_rgb(key[p], cov[p], covp[p], verts, nv, faces, nf, m, st);
      out[3 * p] = (unsigned char)rgb; out[3 * p + 1] = (unsigned char)(rgb >> 8); out[3 * p + 2] = (unsigned char)(rgb >> 16);
    }
  }
}

}  // namespace neat
