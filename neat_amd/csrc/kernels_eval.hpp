// Scoring a reconstruction against ground truth (the reference's code/evaluation/eval-dtu.py, eval-lsr-dtu.py, eval-wfr-dtu.py, eval-abc.py,
// which use open3d, an sklearn kd-tree on the host and a sequential thinning loop): triangle sampling with ordered compaction, a uniform
// cell grid over a cloud, radius thinning by rounds, a capped nearest-point query, the observation-mask flags and the ABC cost matrices.
// Every keep / remove, inside / outside and nearer / farther decision compares float64 quantities computed in the reference's order
// (DESIGN 3c): squared distances are ((dx dx) + dy dy) + dz dz with every product and sum rounded on its own (fp contraction is off in
// these functions and the operands pass through rounded()), numpy's norm is sqrt((x x + y y) + z z), its cross a b - c d with both
// products rounded.  Integer atomics only (histogram, scatter cursor, the undecided counter); nothing depends on their order: every
// choice between equal distances is made on the point index.  No kernel loops without a bound that is fixed before it starts.
//
// Definitions (tests/eval_f64.py restates them in numpy):
//   cell        c = floor((p - origin) / cell) per axis, clamped into the grid's box for cloud points and left as it is for queries
//   bucket      the cell's linear index in a dense box, or a hash of (cx, cy, cz) modulo the bucket count; a bucket may hold points of
//               several cells, which costs distance tests and changes no result (every candidate is tested by its true distance)
//   thinning    point c stays iff no earlier staying point lies within the radius (<=); a round decides every point whose earlier
//               neighbours are all decided: removed if one of them stays, kept if all are removed
//   nearest     the lowest (squared distance, index) over the cloud; rings of cells outwards, ring r is farther than (r - 1) cell
//   sampling    eval-dtu.py:48-71: per triangle the (i, j) of mgrid[:n1+1, :n2+1] with (i+.5)/max(n1,1e-7) + (j+.5)/max(n2,1e-7) < 1,
//               triangle-major, then i, then j
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>

#include "block_util.hpp"      // block_carry_scan
#include "device_util.hpp"     // rounded

namespace neat {

constexpr int EVAL_WG = 256;
constexpr int EVAL_SCAN_WG = 1024;
constexpr int EVAL_TRI_MAXN = 30000;      // lattice steps per triangle side: beyond it the triangle's count would leave int32

struct EvalGrid {
  double o[3], cell;
  int dim[3], buckets, dense, n;
  const int* start;       // [buckets + 1]
  const int* sidx;        // [n] point index per slot
  const double* spts;     // [n,3] the points in slot order
};

__device__ __forceinline__ double eval_d2(double ax, double ay, double az, double bx, double by, double bz) {
#pragma clang fp contract(off)
  const double dx = ax - bx, dy = ay - by, dz = az - bz;
  const double xx = rounded(dx * dx), yy = rounded(dy * dy), zz = rounded(dz * dz);
  return rounded(rounded(xx + yy) + zz);
}
// numpy.linalg.norm over a last axis of three
__device__ __forceinline__ double eval_norm3(double x, double y, double z) {
#pragma clang fp contract(off)
  const double xx = rounded(x * x), yy = rounded(y * y), zz = rounded(z * z);
  return sqrt(rounded(rounded(xx + yy) + zz));
}

__device__ __forceinline__ int eval_cell1(double x, double o, double cell) {
  const double c = floor((x - o) / cell);
  return (int)fmin(fmax(c, -268435456.0), 268435456.0);      // far-away queries keep a valid (lower) ring bound; a NaN lands on the lower clamp
}
__device__ __forceinline__ unsigned eval_bucket(const EvalGrid& g, int cx, int cy, int cz) {      // 0 <= c < dim
  if (g.dense) return ((unsigned)cx * (unsigned)g.dim[1] + (unsigned)cy) * (unsigned)g.dim[2] + (unsigned)cz;
  unsigned h = (unsigned)cx * 73856093u ^ (unsigned)cy * 19349663u ^ (unsigned)cz * 83492791u;
  h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
  return h % (unsigned)g.buckets;
}
__device__ __forceinline__ int eval_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- (a) the grid: bucket per point + histogram, exclusive scan, scatter ----------------------------------------------------------------
__global__ __launch_bounds__(EVAL_WG) void eval_grid_bin_kernel(const double* __restrict__ pts, EvalGrid g, int* __restrict__ bucket_of,
                                                                int* __restrict__ cnt) {
  const int i = blockIdx.x * EVAL_WG + threadIdx.x;
  if (i >= g.n) return;
  const double* p = pts + 3 * (size_t)i;
  const int cx = eval_clampi(eval_cell1(p[0], g.o[0], g.cell), 0, g.dim[0] - 1);
  const int cy = eval_clampi(eval_cell1(p[1], g.o[1], g.cell), 0, g.dim[1] - 1);
  const int cz = eval_clampi(eval_cell1(p[2], g.o[2], g.cell), 0, g.dim[2] - 1);
  const unsigned b = eval_bucket(g, cx, cy, cz);
  bucket_of[i] = (int)b;
  atomicAdd(&cnt[b], 1);
}

// one workgroup: out[0..n] = exclusive sums of in[0..n), out[n] and *total the sum; *total = -1 if an input is negative or the sum
// leaves int32 (the offsets are then never used)
__global__ __launch_bounds__(EVAL_SCAN_WG) void eval_exscan_kernel(const int* __restrict__ in, int* __restrict__ out, int n, int* __restrict__ total) {
  __shared__ int s_wave[EVAL_SCAN_WG / 64];
  __shared__ int s_bad;
  if (threadIdx.x == 0) s_bad = 0;
  __syncthreads();
  const long long carry = block_carry_scan(n, [&](int t) {
    const int v = in[t];
    if (v < 0) s_bad = 1;
    return v < 0 ? 0 : v;
  }, [&](int t, long long e) { out[t] = (int)min(e, (long long)INT_MAX); }, s_wave);
  __syncthreads();
  if (threadIdx.x == 0) {
    const bool ok = !s_bad && carry <= INT_MAX;
    out[n] = (int)min(carry, (long long)INT_MAX);
    if (total) *total = ok ? (int)carry : -1;
  }
}

// cnt holds the histogram and is counted down to zero: the slot of a point within its bucket is whatever the countdown hands it
__global__ __launch_bounds__(EVAL_WG) void eval_grid_scatter_kernel(const double* __restrict__ pts, int n, const int* __restrict__ bucket_of,
                                                                    int* __restrict__ cnt, const int* __restrict__ start,
                                                                    int* __restrict__ sidx, double* __restrict__ spts) {
  const int i = blockIdx.x * EVAL_WG + threadIdx.x;
  if (i >= n) return;
  const int b = bucket_of[i];
  const int slot = start[b] + atomicSub(&cnt[b], 1) - 1;
  if (slot < 0 || slot >= n) return;
  sidx[slot] = i;
  const double* p = pts + 3 * (size_t)i;
  double* q = spts + 3 * (size_t)slot;
  q[0] = p[0]; q[1] = p[1]; q[2] = p[2];
}

// ---- (b) one round of the thinning.  state: 0 undecided, 1 kept, 2 removed.  A state changes once, from 0, and a decided state read
// during the round it was written in is as final as one read later, so the rounds need no double buffer.
__global__ __launch_bounds__(EVAL_WG) void eval_thin_round_kernel(const double* __restrict__ pts, EvalGrid g, double r2,
                                                                  unsigned char* state, int* __restrict__ undecided) {
  const int i = blockIdx.x * EVAL_WG + threadIdx.x;
  const volatile unsigned char* vstate = state;
  const bool active = i < g.n && vstate[i] == 0;
  bool pending = false, removed = false;
  if (active) {
    const double px = pts[3 * (size_t)i], py = pts[3 * (size_t)i + 1], pz = pts[3 * (size_t)i + 2];
    const int cx = eval_clampi(eval_cell1(px, g.o[0], g.cell), 0, g.dim[0] - 1);
    const int cy = eval_clampi(eval_cell1(py, g.o[1], g.cell), 0, g.dim[1] - 1);
    const int cz = eval_clampi(eval_cell1(pz, g.o[2], g.cell), 0, g.dim[2] - 1);
    for (int c = 0; c < 27 && !removed; ++c) {
      const int x = cx + c / 9 - 1, y = cy + (c / 3) % 3 - 1, z = cz + c % 3 - 1;
      if (x < 0 || y < 0 || z < 0 || x >= g.dim[0] || y >= g.dim[1] || z >= g.dim[2]) continue;
      const unsigned b = eval_bucket(g, x, y, z);
      const int s1 = g.start[b + 1];
      for (int s = g.start[b]; s < s1; ++s) {
        const int j = g.sidx[s];
        if (j >= i) continue;
        const double* q = g.spts + 3 * (size_t)s;
        if (eval_d2(px, py, pz, q[0], q[1], q[2]) <= r2) {
          const unsigned char st = vstate[j];
          if (st == 1) { removed = true; break; }
          if (st == 0) pending = true;
        }
      }
    }
    if (removed) state[i] = 2;
    else if (!pending) state[i] = 1;
  }
  const bool waits = active && !removed && pending;
  const unsigned long long m = __ballot(waits);
  if (m != 0 && (threadIdx.x & 63) == (__ffsll((long long)m) - 1)) atomicAdd(undecided, __popcll(m));
}

// ---- (c) the nearest cloud point of every query, if one lies within the cap: dist = sqrt(d2), idx; otherwise inf, -1.  cap2 is the
// squared cap (the caller widens it by a few ulp and takes the `< max_dist` decision on the distance itself, as the reference does).
__global__ __launch_bounds__(EVAL_WG) void eval_nearest_kernel(EvalGrid g, const double* __restrict__ qs, int m, double cap, double cap2,
                                                               double* __restrict__ dist, int* __restrict__ idx) {
  const int t = blockIdx.x * EVAL_WG + threadIdx.x;
  if (t >= m) return;
  const double qx = qs[3 * (size_t)t], qy = qs[3 * (size_t)t + 1], qz = qs[3 * (size_t)t + 2];
  const int cx = eval_cell1(qx, g.o[0], g.cell), cy = eval_cell1(qy, g.o[1], g.cell), cz = eval_cell1(qz, g.o[2], g.cell);
  // rings that meet the box: from the query cell's Chebyshev distance to the box up to its farthest cell
  int r0 = 0, r1 = 0;
  {
    const int c[3] = {cx, cy, cz};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int below = -c[a], above = c[a] - (g.dim[a] - 1);
      r0 = max(r0, max(below, above));
      r1 = max(r1, max(c[a], g.dim[a] - 1 - c[a]));
    }
  }
  double best = INFINITY;
  int besti = -1;
  const double slack = 1.0 - 1e-6;         // the cell of a coordinate is exact to far better than this
  for (int r = r0; r <= r1; ++r) {
    const double lb = (double)(r - 1) * g.cell * slack;      // every point of ring r and beyond is farther than this
    if (r > 0 && lb > 0.0 && (lb >= cap || lb * lb >= best)) break;
    const int z0 = max(cz - r, 0), z1 = min(cz + r, g.dim[2] - 1);
    const int y0 = max(cy - r, 0), y1 = min(cy + r, g.dim[1] - 1);
    const int x0 = max(cx - r, 0), x1 = min(cx + r, g.dim[0] - 1);
    for (int z = z0; z <= z1; ++z) {
      const bool zface = z == cz - r || z == cz + r;
      for (int y = y0; y <= y1; ++y) {
        const bool face = zface || y == cy - r || y == cy + r;
        const int step = face ? 1 : max(2 * r, 1);            // off the faces only x = cx - r and cx + r belong to the ring
        for (int x = face ? x0 : cx - r; x <= x1; x += step) {
          if (x < x0) continue;
          const unsigned b = eval_bucket(g, x, y, z);
          const int s1 = g.start[b + 1];
          for (int s = g.start[b]; s < s1; ++s) {
            const double* p = g.spts + 3 * (size_t)s;
            const double d2 = eval_d2(qx, qy, qz, p[0], p[1], p[2]);
            if (d2 > cap2) continue;
            const int j = g.sidx[s];
            if (d2 < best || (d2 == best && j < besti)) { best = d2; besti = j; }
          }
        }
      }
    }
  }
  dist[t] = besti >= 0 ? sqrt(best) : INFINITY;
  idx[t] = besti;
}

// ---- (d) eval-dtu.py:98-110 per point: bit 0 = inside the padded box, bit 1 = also inside the voxel grid and in an observed voxel.
// lo / hi are the float32 sums BB[0] - patch and BB[1] + 2 patch widened to float64, bb0 = BB[0] widened.
struct EvalObs {
  double lo[3], hi[3], bb0[3], res;
  int shape[3], f32_quotient;
};
__global__ __launch_bounds__(EVAL_WG) void eval_obs_mask_kernel(const double* __restrict__ pts, int n, EvalObs a,
                                                                const unsigned char* __restrict__ mask, unsigned char* __restrict__ flags) {
  const int i = blockIdx.x * EVAL_WG + threadIdx.x;
  if (i >= n) return;
  bool in = true, gin = true;
  long long v[3] = {0, 0, 0};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double p = pts[3 * (size_t)i + c];
    in = in && p >= a.lo[c] && p < a.hi[c];
    const double q = (p - a.bb0[c]) / a.res;
    const double gq = a.f32_quotient ? (double)rintf((float)q) : rint(q);
    gin = gin && gq >= 0.0 && gq < (double)a.shape[c];
    v[c] = gin ? (long long)gq : 0;
  }
  unsigned char f = in ? 1 : 0;
  if (in && gin && mask[((size_t)v[0] * a.shape[1] + (size_t)v[1]) * a.shape[2] + (size_t)v[2]]) f |= 2;
  flags[i] = f;
}

// ---- (e) triangle sampling ------------------------------------------------------------------------------------------------------------
struct EvalTri {
  double a[3], v1[3], v2[3], d1, d2;
  int n1, n2;            // n1 < 0: no samples (zero area); n1 = INT_MAX: too many
};
__device__ __forceinline__ void eval_tri_setup(const double* __restrict__ verts, int nv, const int* __restrict__ faces, int t, double density,
                                               EvalTri& T) {
#pragma clang fp contract(off)
  const int i0 = faces[3 * (size_t)t], i1 = faces[3 * (size_t)t + 1], i2 = faces[3 * (size_t)t + 2];
  T.n1 = -1; T.n2 = -1;
  if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= nv || i1 >= nv || i2 >= nv) { T.n1 = INT_MAX; return; }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    T.a[c] = verts[3 * (size_t)i0 + c];
    T.v1[c] = verts[3 * (size_t)i1 + c] - T.a[c];
    T.v2[c] = verts[3 * (size_t)i2 + c] - T.a[c];
  }
  const double l1 = eval_norm3(T.v1[0], T.v1[1], T.v1[2]), l2 = eval_norm3(T.v2[0], T.v2[1], T.v2[2]);
  const double c0 = rounded(rounded(T.v1[1] * T.v2[2]) - rounded(T.v1[2] * T.v2[1]));
  const double c1 = rounded(rounded(T.v1[2] * T.v2[0]) - rounded(T.v1[0] * T.v2[2]));
  const double c2 = rounded(rounded(T.v1[0] * T.v2[1]) - rounded(T.v1[1] * T.v2[0]));
  const double area2 = eval_norm3(c0, c1, c2);
  if (!(area2 > 0.0)) return;
  const double thr = rounded(density * sqrt(rounded(rounded(l1 * l2) / area2)));
  const double n1 = floor(l1 / thr), n2 = floor(l2 / thr);
  if (!(n1 >= 0.0 && n1 <= (double)EVAL_TRI_MAXN && n2 >= 0.0 && n2 <= (double)EVAL_TRI_MAXN)) { T.n1 = INT_MAX; return; }
  T.n1 = (int)n1; T.n2 = (int)n2;
  T.d1 = fmax(n1, 1e-7); T.d2 = fmax(n2, 1e-7);
}
__device__ __forceinline__ bool eval_tri_in(const EvalTri& T, double k0, int j) {
#pragma clang fp contract(off)
  return rounded(k0 + ((double)j + 0.5) / T.d2) < 1.0;
}
// the number of j in 0..n2 of row i: the predicate falls once along j, so an estimate and two bounded walks find the edge
__device__ __forceinline__ int eval_tri_row(const EvalTri& T, int i, double* k0_out) {
  const double k0 = ((double)i + 0.5) / T.d1;
  *k0_out = k0;
  int je = (int)fmin(fmax(floor((1.0 - k0) * T.d2 - 0.5), -1.0), (double)T.n2);
  for (int g = 0; g <= T.n2 && je < T.n2 && eval_tri_in(T, k0, je + 1); ++g) ++je;
  for (int g = 0; g <= T.n2 && je >= 0 && !eval_tri_in(T, k0, je); ++g) --je;
  return je + 1;
}

// one wavefront per triangle, a row of the lattice per lane
__global__ __launch_bounds__(EVAL_WG) void eval_tri_count_kernel(const double* __restrict__ verts, int nv, const int* __restrict__ faces, int nf,
                                                                 double density, int* __restrict__ counts) {
  const int t = blockIdx.x * (EVAL_WG / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (t >= nf) return;
  EvalTri T;
  eval_tri_setup(verts, nv, faces, t, density, T);
  int c = 0;
  if (T.n1 >= 0 && T.n1 != INT_MAX) {
    double k0;
    for (int i = lane; i <= T.n1; i += 64) c += eval_tri_row(T, i, &k0);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if (lane == 0) counts[t] = T.n1 == INT_MAX ? -1 : c;
}

__global__ __launch_bounds__(EVAL_WG) void eval_tri_emit_kernel(const double* __restrict__ verts, int nv, const int* __restrict__ faces, int nf,
                                                                double density, const int* __restrict__ offs, double* __restrict__ out, int total) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * (EVAL_WG / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (t >= nf) return;
  EvalTri T;
  eval_tri_setup(verts, nv, faces, t, density, T);
  if (T.n1 < 0 || T.n1 == INT_MAX) return;
  int carry = offs[t];
  for (int i0 = 0; i0 <= T.n1; i0 += 64) {
    const int i = i0 + lane;
    double k0 = 0.0;
    const int rc = i <= T.n1 ? eval_tri_row(T, i, &k0) : 0;
    int x = rc;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(x, o); if (lane >= o) x += y; }
    const int base = carry + x - rc;
    carry += __shfl(x, 63);
    for (int j = 0; j < rc; ++j) {
      const int o = base + j;
      if (o < 0 || o >= total) break;
      const double k1 = ((double)j + 0.5) / T.d2;
      double* q = out + 3 * (size_t)o;
#pragma unroll
      for (int c = 0; c < 3; ++c) q[c] = rounded(rounded(rounded(T.v1[c] * k0) + rounded(T.v2[c] * k1)) + T.a[c]);
    }
  }
}

// ---- (f) eval-abc.py: cost [n_pred, n_gt] between sets of `ends` points (1: junctions, the distance; 2: lines, the lower mean endpoint
// distance of the two endpoint orders, :86-88)
__global__ __launch_bounds__(EVAL_WG) void eval_line_cost_kernel(const double* __restrict__ pred, int n_pred, const double* __restrict__ gt, int n_gt,
                                                                 int ends, double* __restrict__ cost) {
#pragma clang fp contract(off)
  const long long t = (long long)blockIdx.x * EVAL_WG + threadIdx.x;
  if (t >= (long long)n_pred * n_gt) return;
  const int i = (int)(t / n_gt), j = (int)(t % n_gt);
  const double* p = pred + 3 * (size_t)ends * i;
  const double* q = gt + 3 * (size_t)ends * j;
  if (ends == 1) { cost[t] = eval_norm3(p[0] - q[0], p[1] - q[1], p[2] - q[2]); return; }
  const double d00 = eval_norm3(p[0] - q[0], p[1] - q[1], p[2] - q[2]), d11 = eval_norm3(p[3] - q[3], p[4] - q[4], p[5] - q[5]);
  const double d01 = eval_norm3(p[0] - q[3], p[1] - q[4], p[2] - q[5]), d10 = eval_norm3(p[3] - q[0], p[4] - q[1], p[5] - q[2]);
  cost[t] = fmin(rounded(d00 + d11) / 2.0, rounded(d01 + d10) / 2.0);
}

}  // namespace neat
