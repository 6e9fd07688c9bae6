// Workgroup-wide scans, reductions and compaction shared by the tool kernels (kernels_parse / mesh / evalmesh / eval / frame / trace / post /
// raycast / detect / triangulate / wireframe2d / wireframe3d), by the scans of graph_util.hpp (which scenegen and crease use) and, for
// block_compact, by lsap_kernel.  As in device_util.hpp, the translation units share one namespace, so only templates and
// __forceinline__ functions belong here.  No atomics and a fixed order everywhere: a result is the same bits on every run.  Every
// function ends with a barrier, so it may be called again at once with the same LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace neat {

// exclusive scan of v over the workgroup (any whole number of waves up to 16) in thread order; *total = the sum.  s_wave: one int per wave
__device__ __forceinline__ int block_exscan(int v, int* s_wave, int* total) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  int x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(x, o); if (lane >= o) x += y; }
  if (lane == 63) s_wave[wave] = x;
  __syncthreads();
  int off = 0, tot = 0;
  for (int w = 0; w < nw; ++w) { const int sw = s_wave[w]; off += w < wave ? sw : 0; tot += sw; }
  __syncthreads();
  *total = tot;
  return off + x - v;
}

// One workgroup walks n ints in rounds of blockDim.x with a running 64-bit carry: store(i, sum of load(j) over j < i) for every i < n,
// in order; returns the sum of all.  A caller clamps or narrows in its store.
template <class L, class S>
__device__ __forceinline__ long long block_carry_scan(int n, L load, S store, int* s_wave) {
  long long carry = 0;
  for (int i0 = 0; i0 < n; i0 += blockDim.x) {
    const int i = i0 + threadIdx.x;
    const int v = i < n ? load(i) : 0;
    int tot;
    const int e = block_exscan(v, s_wave, &tot);
    if (i < n) store(i, carry + e);
    carry += tot;
  }
  return carry;
}

// sum over a workgroup of WG = 256 threads (int or double): lane t += lane t ^ 32, ^ 16, ... ^ 1 within each wave, then (w0 + w1) +
// (w2 + w3).  The float64 sums of kernels_frame.hpp and kernels_evalmesh.hpp are defined by this association.  sh: one value per wave
template <int WG, class T>
__device__ __forceinline__ T block_sum(T v, T* sh) {
  static_assert(WG == 256, "four waves");
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const T s = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  __syncthreads();
  return s;
}

// min of lo[c] and max of hi[c] per component over a workgroup of WG = 256 threads (float or double: fmin / fmax are overloaded), the same
// butterfly and wave tree as block_sum; every thread gets the result.  fmin / fmax drop a NaN operand, so only an all-NaN input gives
// NaN.  sh: 8 values per component
template <int WG, class T, int C>
__device__ __forceinline__ void block_minmax(T (&lo)[C], T (&hi)[C], T* sh) {
  static_assert(WG == 256, "four waves");
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < C; ++c) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      lo[c] = fmin(lo[c], __shfl_xor(lo[c], off));
      hi[c] = fmax(hi[c], __shfl_xor(hi[c], off));
    }
    if ((threadIdx.x & 63) == 0) { sh[8 * c + wave] = lo[c]; sh[8 * c + 4 + wave] = hi[c]; }
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const T* s = sh + 8 * c;
    lo[c] = fmin(fmin(s[0], s[1]), fmin(s[2], s[3]));
    hi[c] = fmax(fmax(s[4], s[5]), fmax(s[6], s[7]));
  }
  __syncthreads();
}

// ordered compaction of the indices i in [0,n) with flag(i) != 0 into out[]; returns the count (all threads)
template <class F>
__device__ int block_compact(int n, F flag, int* out, int* s_wave, int* s_base) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  if (tid == 0) *s_base = 0;
  __syncthreads();
  for (int b0 = 0; b0 < n; b0 += blockDim.x) {
    const int i = b0 + tid;
    const bool f = i < n && flag(i);
    const unsigned long long bal = __ballot(f);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) s_wave[wave] = __popcll(bal);
    __syncthreads();
    int off = *s_base;
    for (int w = 0; w < wave; ++w) off += s_wave[w];
    if (f) out[off + before] = i;
    __syncthreads();
    if (tid == 0) { int t = 0; for (int w = 0; w < nw; ++w) t += s_wave[w]; *s_base += t; }
    __syncthreads();
  }
  const int total = *s_base;
  __syncthreads();          // everyone has read the count before a later call resets it (a fast thread 0 used to race ahead)
  return total;
}

}  // namespace neat
