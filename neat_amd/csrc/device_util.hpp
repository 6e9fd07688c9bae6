// Device helpers shared by the network kernels (kernels.hpp) and the precision-independent kernels (kernels_sampler.hpp,
// kernels_junction.hpp): the two translation units live in the same namespace, so only __forceinline__ functions belong here.
#pragma once
#include "bf16_common.hpp"

namespace neat {

// A value the compiler may not fuse into an fma with its consumer.  (HIP's __fmul_rn / __fadd_rn are plain operators under the default
// -ffp-contract=fast and DO get contracted: the round-5 form of points_from_rays_kernel and eik_points_kernel compiled to v_fmac_f32 / v_pk_fma_f32.)
__device__ __forceinline__ float rounded(float x) { asm volatile("" : "+v"(x)); return x; }
__device__ __forceinline__ double rounded(double x) { asm volatile("" : "+v"(x)); return x; }      // the float64 decisions of kernels_eval.hpp

__device__ __forceinline__ float wave_incl_scan(float v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const float t = __shfl_up(v, off);
    if (lane >= off) v += t;
  }
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
// Laplace density (density.py:21-26) and its derivative pieces
__device__ __forceinline__ float laplace_sigma(float s, float beta) {
  const float sg = (s > 0.0f) ? 1.0f : ((s < 0.0f) ? -1.0f : 0.0f);
  return (1.0f / beta) * (0.5f + 0.5f * sg * expm1f(-fabsf(s) / beta));
}

// pixel -> ray (rend_util.py:55-81,95-108)
__device__ __forceinline__ void camera_ray(const float* __restrict__ uv, const float* __restrict__ pose, const float* __restrict__ Kin,
                                           int kstride, int r, float* __restrict__ dirs, float* __restrict__ origins) {
  const float fx = Kin[0], sk = Kin[1], cx = Kin[2], fy = Kin[kstride + 1], cy = Kin[kstride + 2];
  const float u = uv[r * 2], v = uv[r * 2 + 1];
  const float xl = (u - cx + cy * sk / fy - sk * v / fy) / fx;
  const float yl = (v - cy) / fy;
  float w[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float wc = pose[c * 4 + 0] * xl + pose[c * 4 + 1] * yl + pose[c * 4 + 2] * 1.0f + pose[c * 4 + 3] * 1.0f;
    w[c] = wc - pose[c * 4 + 3];
  }
  const float n = fmaxf(sqrtf(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]), 1e-12f);
  dirs[r * 3 + 0] = w[0] / n; dirs[r * 3 + 1] = w[1] / n; dirs[r * 3 + 2] = w[2] / n;
  if (origins) {          // the camera centre once per ray (the callers' `cam_loc.unsqueeze(1).repeat(1, R, 1)`, rend_a :395)
#pragma unroll
    for (int c = 0; c < 3; ++c) origins[r * 3 + c] = pose[c * 4 + 3];
  }
}

}  // namespace neat
