// Components, their member walks and the scans of count arrays shared by the graph-building tools (kernels_detect / triangulate / crease /
// wireframe2d / wireframe3d / scenegen).  As in block_util.hpp the device functions are templates or __forceinline__; the
// two kernels that are no templates belong to neat_aux.hip, the one unit that includes this file.  The only atomics are integer fetch-min
// and fetch-max, which end the same in any order of arrival, and every walk and scan runs in index order: the same bits on every run.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>

#include "block_util.hpp"           // block_exscan, block_carry_scan

namespace neat {

// ---- connected components as a label-equivalence union-find: parent[n] <= n always, so a root is the smallest index of its tree.
// SCOPE: workgroup for the tile in LDS, agent for the merge along the tile borders in global memory (atomics reach the other XCDs'
// workgroups at agent scope; a stale parent read elsewhere is still an ancestor, so a find over it is still right)
template <int SCOPE>
__device__ __forceinline__ int uf_find(int* L, int n) {
  int p = __hip_atomic_load(L + n, __ATOMIC_RELAXED, SCOPE);
  while (p != n) { n = p; p = __hip_atomic_load(L + n, __ATOMIC_RELAXED, SCOPE); }
  return n;
}
template <int SCOPE>
__device__ __forceinline__ void uf_union(int* L, int a, int b) {
  bool done;
  do {
    a = uf_find<SCOPE>(L, a);
    b = uf_find<SCOPE>(L, b);
    if (a < b) { const int old = __hip_atomic_fetch_min(L + b, a, __ATOMIC_RELAXED, SCOPE); done = old == b; b = old; }
    else if (b < a) { const int old = __hip_atomic_fetch_min(L + a, b, __ATOMIC_RELAXED, SCOPE); done = old == a; a = old; }
    else done = true;
  } while (!done);
}

// label = the root = the component's lowest member; last[root] = its highest.  An entry with a negative parent is in no component and
// is skipped.  last of a member that is no root is whatever the caller's own start left there: nobody reads it
constexpr int UF_WG = 256;
__global__ __launch_bounds__(UF_WG) void uf_flatten_kernel(int n, int* parent, int* __restrict__ last) {
  const int e = blockIdx.x * UF_WG + threadIdx.x;
  if (e >= n) return;
  if (__hip_atomic_load(parent + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 0) return;
  const int r = uf_find<__HIP_MEMORY_SCOPE_AGENT>(parent, e);
  __hip_atomic_store(parent + e, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  atomicMax(last + r, e);
}

// ---- one wavefront at a component's root r: its members are the e in [r, end = last[r]] with label r, met 64 at a time.  each(e) runs
// in the lane that owns member e; ordered(e) runs in every lane for every member in ascending order, so sums formed there are the same
// bits in all lanes.  Returns the number of members.  The whole wavefront calls this together
template <class E, class O>
__device__ __forceinline__ int wave_members(const int* __restrict__ label, int r, int end, int lane, E each, O ordered) {
  int m = 0;
  for (int e0 = r; e0 <= end; e0 += 64) {
    const int e = e0 + lane;
    const bool mine = e <= end && label[e] == r;
    unsigned long long bal = __ballot(mine);
    m += __popcll(bal);
    if (mine) each(e);
    for (; bal; bal &= bal - 1ull) ordered(e0 + __builtin_ctzll(bal));
  }
  return m;
}
// the lane-parallel pass alone
template <class E>
__device__ __forceinline__ void wave_members_each(const int* __restrict__ label, int r, int end, int lane, E each) {
  for (int e = r + lane; e <= end; e += 64)
    if (label[e] == r) each(e);
}

// ---- one workgroup: off [n] = the exclusive scan of cnt (kept below the top of Off), *total = the exact sum.  For lists that one
// workgroup walks in a few rounds; tiled_scan (neat_aux.hip) is the one for lists of millions
template <class Off>
__global__ __launch_bounds__(1024) void count_scan_kernel(int n, const int* __restrict__ cnt, Off* __restrict__ off, long long* __restrict__ total) {
  __shared__ int s_wave[16];
  constexpr long long top = sizeof(Off) == sizeof(int) ? (long long)INT_MAX : LLONG_MAX;
  const long long tot = block_carry_scan(n, [&](int i) { return cnt[i]; }, [&](int i, long long e) { off[i] = (Off)(e < top ? e : top); }, s_wave);
  if (threadIdx.x == 0) *total = tot;
}

// ---- the device-wide scan of an int-valued function of the index: the sums of tiles of SCAN_WG, one workgroup over the tile sums, then
// the tiles again (tiled_scan in neat_aux.hip launches the three)
constexpr int SCAN_WG = 1024;
struct IsNonzero { const int* p; __device__ int operator()(int i) const { return p[i] != 0; } };
struct IsEqual { const int* p; int v; __device__ int operator()(int i) const { return p[i] == v; } };
struct Value { const int* p; __device__ int operator()(int i) const { return p[i]; } };
template <class F>
__global__ __launch_bounds__(SCAN_WG) void scan_tile_kernel(int n, F f, int* __restrict__ tile) {
  __shared__ int s_wave[16];
  const int i = blockIdx.x * SCAN_WG + threadIdx.x;
  int tot;
  block_exscan(i < n ? f(i) : 0, s_wave, &tot);
  if (threadIdx.x == 0) tile[blockIdx.x] = tot;
}
// tile sums -> their exclusive offsets in place; *total = the sum (the host has bounded it below 2^31)
__global__ __launch_bounds__(SCAN_WG) void scan_top_kernel(int tiles, int* __restrict__ tile, int* __restrict__ total) {
  __shared__ int s_wave[16];
  const long long tot = block_carry_scan(tiles, [&](int i) { return tile[i]; }, [&](int i, long long e) { tile[i] = (int)e; }, s_wave);
  if (threadIdx.x == 0) *total = (int)tot;
}
template <class F>
__global__ __launch_bounds__(SCAN_WG) void scan_apply_kernel(int n, F f, const int* __restrict__ tile, int* __restrict__ out) {
  __shared__ int s_wave[16];
  const int i = blockIdx.x * SCAN_WG + threadIdx.x;
  int tot;
  const int e = block_exscan(i < n ? f(i) : 0, s_wave, &tot);
  if (i < n) out[i] = tile[blockIdx.x] + e;
}

}  // namespace neat
