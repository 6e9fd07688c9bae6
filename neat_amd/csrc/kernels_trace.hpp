// Sphere tracing of an SDF along rays (neat_amd/trace.py): where a ray first meets the zero level.  The SDF itself is queried by the
// caller between the launches here (ops.sdf_values with radius 0 = the raw, unclamped network, or any field); these kernels are the
// per-ray state machine around it and the ordered compaction of the rays that still need a query.  Per-ray state is fp32, the ray set-up
// (sphere chord, clip) float64 rounded once.  No atomics, every scan has a fixed order: two runs give the same lists, the same number
// of evaluations and the same bytes.  Nothing here synchronises with the host: the active count is written to device memory (ctl[0])
// and read by the caller once per iteration to size its next query; ctl[1] is the running number of evaluations.
//
// Definitions (tests/trace_f64.py restates them in float64).  Ray (o, d), |d| = 1, bounding sphere of radius r:
//   chord     b = o.d, disc = b^2 - (o.o - r^2); disc <= 0: MISS.  [t0, t1] = [max(-b - sqrt(disc), near), min(-b + sqrt(disc), t_end)],
//             both rounded to fp32; t0 < t1 is false (an empty interval, a NaN): MISS.  Neither costs a query.
//   start     f(t0) < 0: INSIDE, depth t0.  Otherwise f(t0) is the first value of the march.
//   march     0 <= f < eps: HIT at t.  f < 0: bracket [t_prev, t], refine.  Else, if t = t1 (the query at the end has been made, so a hit
//             exactly at the end is not lost): MISS; if max_steps advances have been made: UNCONVERGED; else t_prev = t, f_prev = f,
//             t = min(t + relax f, t1).
//   refine    up to refine_steps rounds on the bracket [a, b], f(a) >= 0 > f(b), w = b - a: the secant point s = a + w fa / (fa - fb),
//             kept inside the middle 90 % of the bracket (clamped to [a + 0.05 w, b - 0.05 w]: a root within 5 % of an end then costs
//             one round that shrinks the bracket twentyfold, where the midpoint would halve it from the far side round after round
//             and never move the near end).  The query replaces the end of its sign; if the same end is replaced twice in a row the
//             value kept for the other end is halved (Illinois), so neither end stays put on a convex or concave f.
//             0 <= f(s) < eps: HIT at s.  After the last round: HIT at a, the last point with f >= 0.
//   NaN       a NaN value ends the ray as UNCONVERGED.
//   steps     queries made for the ray: at most 1 + max_steps + refine_steps; the sum over the rays = the evaluations counted.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "block_util.hpp"     // block_exscan, block_carry_scan
#include "ws_layout.hpp"      // TraceWs

namespace neat {

constexpr int TRACE_WG = 256;
enum : unsigned char { TRACE_MISS = 0, TRACE_HIT = 1, TRACE_INSIDE = 2, TRACE_UNCONVERGED = 3,      // what neat_trace_finish reports
                       TRACE_START = 4, TRACE_MARCH = 5, TRACE_REFINE = 6 };                         // rays that still need a query

__device__ __forceinline__ void trace_point(const float* __restrict__ o, const float* __restrict__ d, int r, float t, float* __restrict__ out) {
  out[0] = __fmaf_rn(t, d[3 * (size_t)r], o[3 * (size_t)r]);
  out[1] = __fmaf_rn(t, d[3 * (size_t)r + 1], o[3 * (size_t)r + 1]);
  out[2] = __fmaf_rn(t, d[3 * (size_t)r + 2], o[3 * (size_t)r + 2]);
}

// the flags of this workgroup's list positions -> its count
__device__ __forceinline__ void trace_tile_count(const TraceWs& w, int alive) {
  __shared__ int s_wave[TRACE_WG / 64];
  int tot;
  block_exscan(alive, s_wave, &tot);
  if (threadIdx.x == 0) w.tile[blockIdx.x] = tot;
}

// ---- init: chord, clip, first state; flag[r] = the ray needs a query
__global__ __launch_bounds__(TRACE_WG) void trace_init_kernel(TraceWs w, const float* __restrict__ o, const float* __restrict__ d,
                                                              const float* __restrict__ t_end, int R, double radius, double near) {
  const int r = blockIdx.x * TRACE_WG + threadIdx.x;
  int alive = 0;
  if (r < R) {
    const double ox = o[3 * (size_t)r], oy = o[3 * (size_t)r + 1], oz = o[3 * (size_t)r + 2];
    const double dx = d[3 * (size_t)r], dy = d[3 * (size_t)r + 1], dz = d[3 * (size_t)r + 2];
    const double b = ox * dx + oy * dy + oz * dz;
    const double disc = b * b - ((ox * ox + oy * oy + oz * oz) - radius * radius);
    float t0 = 0.f, t1 = 0.f;
    if (disc > 0.0) {
      const double sq = sqrt(disc);
      double lo = -b - sq, hi = -b + sq;
      lo = lo > near ? lo : near;
      if (t_end) { const double e = (double)t_end[r]; hi = (e < hi || e != e) ? e : hi; }
      t0 = (float)lo; t1 = (float)hi;
      alive = t0 < t1 ? 1 : 0;
    }
    w.t[r] = t0; w.t1[r] = t1; w.ta[r] = t0; w.fa[r] = 0.f; w.tb[r] = t0; w.fb[r] = 0.f; w.side[r] = 0;
    w.steps[r] = 0; w.march[r] = 0; w.refine[r] = 0;
    w.phase[r] = alive ? TRACE_START : TRACE_MISS;
    w.flag[r] = (unsigned char)alive;
  }
  trace_tile_count(w, alive);
}

// ---- one workgroup of 1024 walks all the tile counts (the host caps R at 2^24 rays = 65536 tiles = 64 rounds): they become exclusive offsets, in order; ctl[0] = the active count, ctl[1] += it (reset: = it)
__global__ __launch_bounds__(1024) void trace_scan_kernel(int* __restrict__ tile, int tiles, long long* __restrict__ ctl, int reset) {
  __shared__ int s_wave[16];
  const long long carry = block_carry_scan(tiles, [&](int t) { return tile[t]; }, [&](int t, long long e) { tile[t] = (int)e; }, s_wave);
  if (threadIdx.x == 0) { ctl[0] = carry; ctl[1] = (reset ? 0 : ctl[1]) + carry; }
}

// ---- emit: the flagged entries of the first n list positions, in order, into ids_out; their query points row-major [count, 3].
// ids_in = nullptr: position = ray (after init).
__global__ __launch_bounds__(TRACE_WG) void trace_emit_kernel(TraceWs w, const int* __restrict__ ids_in, int* __restrict__ ids_out, int n, int R,
                                                              const float* __restrict__ o, const float* __restrict__ d, float* __restrict__ points) {
  __shared__ int s_wave[TRACE_WG / 64];
  const int i = blockIdx.x * TRACE_WG + threadIdx.x;
  const int alive = i < n ? (int)w.flag[i] : 0;
  int tot;
  const int pos = w.tile[blockIdx.x] + block_exscan(alive, s_wave, &tot);
  if (!alive) return;
  const int r = ids_in ? ids_in[i] : i;
  if (r < 0 || r >= R || pos < 0 || pos >= R) return;      // never true for lists these kernels wrote
  ids_out[pos] = r;
  trace_point(o, d, r, w.t[r], points + 3 * (size_t)pos);
}

// the query point of a refinement round on the bracket [ta, tb]
__device__ __forceinline__ float trace_refine_point(float ta, float fa, float tb, float fb) {
  const float wd = tb - ta;
  const float s = ta + wd * (fa / (fa - fb));
  return fminf(fmaxf(s, ta + 0.05f * wd), tb - 0.05f * wd);
}

// the ray's state machine for one value -> 1 if it needs another query (w.t[r] is then the new point)
__device__ __forceinline__ int trace_advance(const TraceWs& w, int r, float f, float eps, float relax, int max_steps, int refine_steps) {
  unsigned char ph = w.phase[r];
  if (ph < TRACE_START) return 0;
  const float t = w.t[r];
  w.steps[r] += 1;
  if (f != f) { w.phase[r] = TRACE_UNCONVERGED; return 0; }
  if (ph == TRACE_START) {
    if (f < 0.f) { w.phase[r] = TRACE_INSIDE; return 0; }
    ph = TRACE_MARCH;
  }
  if (ph == TRACE_MARCH) {
    if (f >= 0.f && f < eps) { w.phase[r] = TRACE_HIT; return 0; }
    if (f < 0.f) {
      const float ta = w.ta[r], fa = w.fa[r];
      if (refine_steps <= 0) { w.t[r] = ta; w.phase[r] = TRACE_HIT; return 0; }
      w.tb[r] = t; w.fb[r] = f; w.refine[r] = 0; w.side[r] = 0;
      w.t[r] = trace_refine_point(ta, fa, t, f);
      w.phase[r] = TRACE_REFINE;
      return 1;
    }
    const float t1 = w.t1[r];
    if (t >= t1) { w.phase[r] = TRACE_MISS; return 0; }
    const int m = w.march[r];
    if (m >= max_steps) { w.phase[r] = TRACE_UNCONVERGED; return 0; }
    w.march[r] = m + 1; w.ta[r] = t; w.fa[r] = f;
    w.t[r] = fminf(__fmaf_rn(relax, f, t), t1);
    w.phase[r] = TRACE_MARCH;
    return 1;
  }
  // TRACE_REFINE
  float ta = w.ta[r], fa = w.fa[r], tb = w.tb[r], fb = w.fb[r];
  const unsigned char side = w.side[r];
  if (f >= 0.f) {
    if (f < eps) { w.phase[r] = TRACE_HIT; return 0; }
    ta = t; fa = f;
    if (side == 1) fb *= 0.5f;
    w.side[r] = 1;
  } else {
    tb = t; fb = f;
    if (side == 2) fa *= 0.5f;
    w.side[r] = 2;
  }
  w.ta[r] = ta; w.fa[r] = fa; w.tb[r] = tb; w.fb[r] = fb;
  const int k = w.refine[r] + 1;
  if (k >= refine_steps) { w.t[r] = ta; w.phase[r] = TRACE_HIT; return 0; }
  w.refine[r] = k;
  w.t[r] = trace_refine_point(ta, fa, tb, fb);
  return 1;
}

// ---- step: the values of the first n entries of the active list `ids` (never more than the device's own count) through the state machine
__global__ __launch_bounds__(TRACE_WG) void trace_advance_kernel(TraceWs w, const int* __restrict__ ids, const float* __restrict__ values, int n,
                                                                 int R, const long long* __restrict__ ctl, float eps, float relax, int max_steps,
                                                                 int refine_steps) {
  const int i = blockIdx.x * TRACE_WG + threadIdx.x;
  int alive = 0;
  if (i < n && (long long)i < ctl[0]) {
    const int r = ids[i];
    if (r >= 0 && r < R) alive = trace_advance(w, r, values[i], eps, relax, max_steps, refine_steps);
  }
  if (i < n) w.flag[i] = (unsigned char)alive;
  trace_tile_count(w, alive);
}

// ---- finish: depth (NaN unless HIT or INSIDE), state, steps, the hit points (NaN rows likewise); a ray left active reads UNCONVERGED
__global__ __launch_bounds__(TRACE_WG) void trace_finish_kernel(TraceWs w, const float* __restrict__ o, const float* __restrict__ d, int R,
                                                                float* __restrict__ depth, unsigned char* __restrict__ state,
                                                                int* __restrict__ steps, float* __restrict__ points) {
  const int r = blockIdx.x * TRACE_WG + threadIdx.x;
  if (r >= R) return;
  const unsigned char ph = w.phase[r];
  const unsigned char st = ph < TRACE_START ? ph : TRACE_UNCONVERGED;
  const bool has = st == TRACE_HIT || st == TRACE_INSIDE;
  const float t = has ? w.t[r] : NAN;
  if (depth) depth[r] = t;
  if (state) state[r] = st;
  if (steps) steps[r] = w.steps[r];
  if (points) {
    float* q = points + 3 * (size_t)r;
    if (has) trace_point(o, d, r, t, q);
    else { q[0] = NAN; q[1] = NAN; q[2] = NAN; }
  }
}

// ---- the rays from F centres towards N x S targets (visibility queries): target (n, j) = a_n + j / (S - 1) (b_n - a_n) of the segment
// rows [a | b] (`stride` floats per row; S = 1: the point a_n), float64 arithmetic.  Ray f (N S) + n S + j: origin c_f, unit direction,
// t_end = |p - c| - bias; ok = the target lies inside the bounding sphere and no nearer to the centre than near + bias (a target that
// fails either is not visible whatever its ray finds).
__global__ __launch_bounds__(TRACE_WG) void trace_target_rays_kernel(const float* __restrict__ centres, int F, const float* __restrict__ rows,
                                                                     int stride, int N, int S, double radius, double near, double bias,
                                                                     float* __restrict__ o, float* __restrict__ d, float* __restrict__ t_end,
                                                                     unsigned char* __restrict__ ok) {
  const long long i = (long long)blockIdx.x * TRACE_WG + threadIdx.x;
  const long long per = (long long)N * S;
  if (i >= per * F) return;
  const int f = (int)(i / per);
  const long long q = i - (long long)f * per;
  const int n = (int)(q / S), j = (int)(q - (long long)n * S);
  const float* row = rows + (size_t)n * stride;
  double p[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double a = row[c];
    p[c] = S > 1 ? a + ((double)j / (double)(S - 1)) * ((double)row[3 + c] - a) : a;
  }
  const double cx = centres[3 * f], cy = centres[3 * f + 1], cz = centres[3 * f + 2];
  const double vx = p[0] - cx, vy = p[1] - cy, vz = p[2] - cz;
  const double L = sqrt(vx * vx + vy * vy + vz * vz);
  const double inv = L > 0.0 ? 1.0 / L : 0.0;
  o[3 * i] = (float)cx; o[3 * i + 1] = (float)cy; o[3 * i + 2] = (float)cz;
  d[3 * i] = (float)(vx * inv); d[3 * i + 1] = (float)(vy * inv); d[3 * i + 2] = (float)(vz * inv);
  t_end[i] = (float)(L - bias);
  const bool inside = p[0] * p[0] + p[1] * p[1] + p[2] * p[2] <= radius * radius;
  ok[i] = (inside && L >= near + bias) ? 1 : 0;
}

}  // namespace neat
