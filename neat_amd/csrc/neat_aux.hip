// C entry points of libneat_hip.so that have no 16-bit storage type (see include/neat_hip.h): camera, eikonal points, the depth
// samplers, batch gather / copy, Adam, the junction MLP, the losses, LSAP, DBSCAN, the wireframe parsing stages, the surface mesh, the evaluation
// mesh, the evaluation of a reconstruction, the wireframe / mesh pictures, the frames of rendered views, the sphere tracer,
// the fuse / refine / snap post-processing, ray casting against a triangle mesh, volume weights.
// Compiled once (build.sh), without NEAT_HALF; the network orchestration and its f16 twin are neat_net.hip.  What crosses the
// boundary: the point stride of an SDF workspace, which the callers of the samplers pass in (neat_sdf_ldp), and the two tuning keys below.
#include "kernels_sampler.hpp"
#include "kernels_junction.hpp"
#include "kernels_parse.hpp"
#include "kernels_mesh.hpp"
#include "kernels_evalmesh.hpp"
#include "kernels_eval.hpp"
#include "kernels_show.hpp"
#include "kernels_frame.hpp"
#include "kernels_trace.hpp"
#include "kernels_post.hpp"
#include "kernels_raycast.hpp"
#include "kernels_closest.hpp"
#include "kernels_scenegen.hpp"
#include "kernels_detect.hpp"
#include "kernels_triangulate.hpp"
#include "kernels_crease.hpp"
#include "kernels_wireframe2d.hpp"
#include "kernels_wireframe3d.hpp"
#include "ws_layout.hpp"
#include "../../include/neat_hip.h"
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits.h>
#include <math.h>
#include <rocprim/device/device_radix_sort.hpp>

using namespace neat;

// tuning keys 28 and 30: neat_set_tuning (neat_net.hip) hands them over
__attribute__((visibility("hidden"))) int neat_aux_set_tuning(int key, int value);

namespace {

int g_ffn_mfma = 1;         // the 256 x 256 layers of the global-junction MLP (forward and data backward) on the fp32 matrix pipe (ffn_mfma_kernel) instead
                            // of the vector-ALU kernel (tuning key 28)
int g_sampler_ablate = 0;   // probes: sampler_round_kernel without its bisection (1) / refine (2) / final (4) part (tuning key 30)

#define NEAT_CHECK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return (int)e_; } while (0)
#define NEAT_PASS(expr) do { const int r_ = (expr); if (r_ != 0) return r_; } while (0)
inline dim3 grid1(int n, int b = 256) { return dim3((n + b - 1) / b); }

// rocprim's radix sort of bits [bit0, bit1) into a workspace's sort region of `room` bytes (sort_scratch_bytes, ws_layout.hpp): ask what
// it wants, -2 if that is more than the room, then sort.  run = false is the question alone, for a caller that refuses before its
// first launch
template <class K>
int sort_keys(void* tmp, size_t room, K* in, K* out, size_t n, unsigned bit0, unsigned bit1, hipStream_t st, bool run = true) {
  size_t tb = 0;
  NEAT_CHECK(rocprim::radix_sort_keys(nullptr, tb, in, out, n, bit0, bit1, st));
  if (tb > room) return -2;
  return run ? (int)rocprim::radix_sort_keys(tmp, tb, in, out, n, bit0, bit1, st) : 0;
}
template <class K, class V>
int sort_pairs(void* tmp, size_t room, K* kin, K* kout, V* vin, V* vout, size_t n, unsigned bit0, unsigned bit1, hipStream_t st, bool run = true) {
  size_t tb = 0;
  NEAT_CHECK(rocprim::radix_sort_pairs(nullptr, tb, kin, kout, vin, vout, n, bit0, bit1, st));
  if (tb > room) return -2;
  return run ? (int)rocprim::radix_sort_pairs(tmp, tb, kin, kout, vin, vout, n, bit0, bit1, st) : 0;
}

// out [n] = the exclusive scan of f over [0, n) (null: the total alone), *total = its sum; tile: n / SCAN_WG + 1 ints.  Three launches over
// tiles of SCAN_WG (graph_util.hpp), for lists of millions; a list that one workgroup walks in a few rounds takes count_scan_kernel
template <class F>
void tiled_scan(int n, F f, int* tile, int* out, int* total, hipStream_t st) {
  const int tiles = (n + SCAN_WG - 1) / SCAN_WG;
  if (tiles > 0) hipLaunchKernelGGL(scan_tile_kernel<F>, dim3(tiles), dim3(SCAN_WG), 0, st, n, f, tile);
  hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(SCAN_WG), 0, st, tiles, tile, total);
  if (tiles > 0 && out) hipLaunchKernelGGL(scan_apply_kernel<F>, dim3(tiles), dim3(SCAN_WG), 0, st, n, f, (const int*)tile, out);
}

__global__ void volume_weights_kernel(const float* __restrict__ z, const float* __restrict__ sdf, int R, int S,
                                      const float* __restrict__ beta_ptr, float* __restrict__ weights) {
  const float beta = *beta_ptr;
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  float carry = 0.0f;
  for (int i0 = 0; i0 < S; i0 += 64) {
    const int i = i0 + lane;
    const bool ok = i < S;
    const int p = r * S + (ok ? i : S - 1);
    const float delta = (i + 1 < S) ? z[p + 1] - z[p] : 1e10f;
    const float e = ok ? delta * laplace_sigma(sdf[p], beta) : 0.0f;
    const float incl = wave_incl_scan(e, lane);
    float excl = __shfl_up(incl, 1);
    if (lane == 0) excl = 0.0f;
    if (ok) weights[p] = (1.0f - expf(-e)) * expf(-(carry + excl));
    carry += __shfl(incl, 63);
  }
}

}  // namespace

int neat_aux_set_tuning(int key, int value) {
  if (key == 28 && (value == 0 || value == 1)) { g_ffn_mfma = value; return 0; }
  if (key == 30 && value >= 0 && value <= 7) { g_sampler_ablate = value; return 0; }
  return -1;
}

extern "C" {

int neat_camera_rays(const float* uv, const float* pose, const float* K, int kstride, int R, float* dirs, float* origins, void* stream) {
  if (R <= 0) return 0;
  hipLaunchKernelGGL(camera_rays_kernel, grid1(R), dim3(256), 0, (hipStream_t)stream, uv, pose, K, kstride, R, dirs, origins);
  return (int)hipGetLastError();
}

int neat_eik_points(const float* uniform, const float* origins, const float* dirs, const float* z_eik, const float* extra, int R, int J,
                    float* out, const float* z, int S, const long long* idx, void* stream) {
  if (R <= 0 || J < 0) return R == 0 && J == 0 ? 0 : -1;
  if (!uniform || !origins || !dirs || !out || (J > 0 && !extra)) return -1;
  if (!z_eik && (!z || !idx || S <= 0)) return -1;           // the depth per ray: given, or picked from the ray's S depths by idx
  hipLaunchKernelGGL(eik_points_kernel, grid1((2 * R + J) * 3), dim3(256), 0, (hipStream_t)stream, uniform, origins, dirs, z_eik, extra, R, J, out,
                     z, S, idx);
  return (int)hipGetLastError();
}

int neat_sampler_bound(const float* z, int n, int R, const float* sdf_old, const float* sdf_new, const int* order, int n_old,
                       const float* beta_in, const float* beta0, float eps, int iters, float* sdf_out, float* beta_out,
                       int* flag, void* stream) {
  if (R <= 0) return 0;
  if (n < 2 || n > SMAX || !z || !sdf_new || !beta_in || !beta0 || !sdf_out || !beta_out || !flag) return -1;
  SamplerBoundArgs a{z, n, R, sdf_old, sdf_new, order, n_old, beta_in, beta0, eps, iters, sdf_out, beta_out, flag, nullptr, 0};
  hipLaunchKernelGGL(sampler_bound_kernel, dim3(R), dim3(BOUND_T), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int neat_sampler_resample(const float* z, const float* sdf, int n, int R, const float* beta, int refine, float add_tiny,
                          const float* u, int u_stride, int N, float* samples, float* z_merged, int* order, void* stream) {
  if (R <= 0) return 0;
  if (n < 2 || n > SMAX || N < 1 || N > SMAX || !z || !sdf || !beta || !u || !samples || (refine && (!z_merged || !order))) return -1;
  SamplerResampleArgs a{};
  a.z = z; a.sdf = sdf; a.n = n; a.R = R; a.beta = beta; a.refine = refine; a.add_tiny = add_tiny; a.u = u; a.u_stride = u_stride; a.N = N;
  a.samples = samples; a.z_merged = z_merged; a.order = order;
  hipLaunchKernelGGL(sampler_resample_kernel, dim3(R), dim3(BOUND_T), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int neat_sampler_finish(const float* samples, int N, const float* z, int n, const int* pick, int n_extra, float near, float far,
                        int R, const int* eik_idx, float* z_vals, float* z_eik, void* stream) {
  if (R <= 0) return 0;
  if (N + 2 + n_extra > SMAX || !samples || !z || (n_extra > 0 && !pick) || !eik_idx || !z_vals || !z_eik) return -1;
  SamplerFinishArgs a{samples, N, z, n, pick, n_extra, near, far, R, eik_idx, z_vals, z_eik, n};
  hipLaunchKernelGGL(sampler_finish_kernel, dim3(R), dim3(64), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int neat_sample_pdf(const float* bins, const float* weights, int nb, int R, const float* u, int u_stride, int N, float* samples,
                    const float* z_merge, int nz, float* z_out, void* stream) {
  if (R <= 0) return 0;
  if (nb < 2 || nb > SMAX || N < 1 || N > SMAX || !bins || !weights || !u || !samples || (z_merge && (!z_out || nz < 0 || nz + N > SMAX))) return -1;
  SamplePdfArgs a{bins, weights, nb, R, u, u_stride, N, samples, z_merge, nz, z_out};
  hipLaunchKernelGGL(sample_pdf_kernel, dim3(R), dim3(64), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int neat_uniform_depths(const float* near_r, float near_s, const float* far_r, float far_s, const float* t, const float* rnd, int R, int N,
                        float* z, void* stream) {
  if (R <= 0 || N <= 0) return 0;
  if (!t || !z) return -1;
  hipLaunchKernelGGL(uniform_depths_kernel, dim3((R * N + 255) / 256), dim3(256), 0, (hipStream_t)stream, near_r, near_s, far_r, far_s, t, rnd, R, N, z);
  return (int)hipGetLastError();
}

int neat_sampler_init(const float* z, int R, int n, const float* beta, float beta_min, float beta_c, float* beta0, float* beta_ray,
                      int* ctl, int nctl, void* stream) {
  return neat_sampler_init_rays(z, R, n, beta, beta_min, beta_c, beta0, beta_ray, ctl, nctl, nullptr, nullptr, nullptr, 0, nullptr, 0, 0, 0,
                                nullptr, stream);
}

int neat_sampler_init_rays(const float* z, int R, int n, const float* beta, float beta_min, float beta_c, float* beta0, float* beta_ray,
                           int* ctl, int nctl, const float* origins, const float* dirs, float* x_fm, int ldp, const float* keys, int n_step,
                           int n_cand, int n_extra, int* pick_all, void* stream) {
  if (R <= 0 || n < 2 || n > SMAX || !z || !beta || !beta0 || !beta_ray || nctl < 0 || (nctl > 0 && !ctl)) return -1;
  if (x_fm && (!origins || !dirs || (long long)ldp < (long long)R * n)) return -1;
  const bool picks = keys != nullptr;
  if (picks && (!pick_all || n_step < 1 || n_cand < 1 || n_extra < 2 || n_extra > n_step || n_step * n_cand > SMAX)) return -1;
  SamplerInitArgs a{z, R, n, beta, beta_min, beta_c, beta0, beta_ray, ctl, nctl, origins, dirs, x_fm, ldp, keys, n_step, n_cand, n_extra, pick_all,
                    (R + 3) / 4, picks ? (n_step * n_cand + 255) / 256 : 0};
  hipLaunchKernelGGL(sampler_init_kernel, dim3(a.init_blocks + n_cand * a.pick_parts), dim3(256), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int neat_sampler_round(const float* z, int n, int R, const float* sdf_old, const float* sdf_new, const int* order, int n_old,
                       const float* beta_in, const float* beta0, float eps, int iters, float* sdf_out, float* beta_out, int* ctl, int round,
                       int max_rounds, float add_tiny, const float* u_refine, int N_refine, float* samples_refine, float* z_merged,
                       int* order_out, const float* origins, const float* dirs, float* x_fm, int ldp, const float* u_final,
                       int u_final_stride, int N_final, float* samples_final, float* z_final, int ld_final, void* stream) {
  if (R <= 0) return 0;
  const bool last = round + 1 >= max_rounds;
  if (n < 2 || n > SMAX || !z || !sdf_new || (order && !sdf_old) || !beta_in || !beta0 || !sdf_out || !beta_out || !ctl || round < 0 ||
      round >= max_rounds || N_final < 1 || N_final > SMAX || !u_final || !samples_final || !z_final || ld_final < n) return -1;
  if (!last && (N_refine < 1 || n + N_refine > SMAX || !u_refine || !samples_refine || !z_merged || !order_out ||
                (x_fm && (!origins || !dirs || (long long)ldp < (long long)R * N_refine)))) return -1;
  SamplerRoundArgs a{z, n, R, sdf_old, sdf_new, order, n_old, beta_in, beta0, eps, iters, sdf_out, beta_out, ctl, round, max_rounds, add_tiny,
                     u_refine, N_refine, samples_refine, z_merged, order_out, origins, dirs, x_fm, ldp, u_final, u_final_stride, N_final,
                     samples_final, z_final, ld_final, g_sampler_ablate};
  hipLaunchKernelGGL(sampler_round_kernel, dim3(R), dim3(BOUND_T), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int neat_sampler_finish_picked(const float* samples, int N, const float* z_final, int ld_final, const int* n_final, const int* pick_all,
                               int n_step, int n_extra, float near, float far, int R, const int* eik_idx, float* z_vals, float* z_eik,
                               void* stream) {
  if (R <= 0) return 0;
  if (N + 2 + n_extra > SMAX || ld_final > SMAX || !samples || !z_final || !n_final || n_extra == 1 || n_extra < 0 || n_step < 1 || !eik_idx ||
      !z_vals || !z_eik) return -1;
  SamplerFinishArgs a{samples, N, z_final, 0, pick_all, n_extra, near, far, R, eik_idx, z_vals, z_eik, ld_final};
  a.n_final = n_final; a.n_step = n_step;
  hipLaunchKernelGGL(sampler_finish_kernel, dim3(R), dim3(64), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int neat_sampler_bound_dev(const float* z, int n, int R, const float* sdf_old, const float* sdf_new, const int* order, int n_old,
                           const float* beta_in, const float* beta0, float eps, int iters, float* sdf_out, float* beta_out,
                           int* open, const int* gate, int gate_value, void* stream) {
  if (R <= 0) return 0;
  if (n < 2 || n > SMAX || !z || !sdf_new || !beta_in || !beta0 || !sdf_out || !beta_out || !open) return -1;
  SamplerBoundArgs a{z, n, R, sdf_old, sdf_new, order, n_old, beta_in, beta0, eps, iters, sdf_out, beta_out, open, gate, gate_value};
  hipLaunchKernelGGL(sampler_bound_kernel, dim3(R), dim3(BOUND_T), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int neat_sampler_resample_dev(const float* z, const float* sdf, int n, int R, const float* beta, float add_tiny,
                              const float* u_refine, int N_refine, float* samples_refine, float* z_merged, int* order,
                              const float* u_final, int u_final_stride, int N_final, float* samples_final, float* z_final, int ld_final,
                              int* n_final, const int* open, int* cont, int round, int max_rounds, void* stream) {
  if (R <= 0) return 0;
  if (n < 2 || n > SMAX || N_refine < 1 || N_final < 1 || n + N_refine > SMAX || ld_final < n || !z || !sdf || !beta || !u_refine || !u_final ||
      !samples_refine || !z_merged || !order || !samples_final || !z_final || !n_final || !open || !cont || round < 0 || round >= max_rounds)
    return -1;
  SamplerResampleArgs a{};
  a.z = z; a.sdf = sdf; a.n = n; a.R = R; a.beta = beta; a.refine = 1; a.add_tiny = add_tiny;
  a.u = u_refine; a.u_stride = 0; a.N = N_refine; a.samples = samples_refine; a.z_merged = z_merged; a.order = order;
  a.open = open; a.cont = cont; a.round = round; a.max_rounds = max_rounds;
  a.u_final = u_final; a.u_final_stride = u_final_stride; a.N_final = N_final; a.samples_final = samples_final;
  a.z_final = z_final; a.ld_final = ld_final; a.n_final = n_final;
  hipLaunchKernelGGL(sampler_resample_kernel, dim3(R), dim3(BOUND_T), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int neat_sampler_finish_dev(const float* samples, int N, const float* z_final, int ld_final, const int* n_final, const float* keys,
                            int n_extra, int* pick, float near, float far, int R, const int* eik_idx, float* z_vals, float* z_eik,
                            void* stream) {
  if (R <= 0) return 0;
  if (N + 2 + n_extra > SMAX || ld_final > SMAX || !samples || !z_final || !n_final || (n_extra > 0 && !pick) || n_extra == 1 || !eik_idx ||
      !z_vals || !z_eik) return -1;
  if (n_extra > 0) hipLaunchKernelGGL(sampler_pick_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, n_final, keys, n_extra, pick);
  SamplerFinishArgs a{samples, N, z_final, 0, pick, n_extra, near, far, R, eik_idx, z_vals, z_eik, ld_final};
  hipLaunchKernelGGL(sampler_finish_kernel, dim3(R), dim3(64), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int neat_encode_lines(const float* lines, int N, int H, int W, float* lmap, int* label, unsigned char* valid, void* stream) {
  if (N < 0 || H <= 0 || W <= 0 || (N > 0 && !lines) || !lmap || !label) return -1;
  hipLaunchKernelGGL(encode_lines_kernel, grid1(H * W), dim3(256), 0, (hipStream_t)stream, lines, N, H, W, lmap, label, valid);
  return (int)hipGetLastError();
}

int neat_gather_batch(const int* pool, int npool, const long long* draw, int n, int W, const float* att, const float* rgb, const int* labels,
                      const float* lines, int nlines, float* uv, float* uv_proj, float* rgb_out, float* lines_out, long long* labels_out,
                      long long* pixel_out, void* stream) {
  if (n < 0 || npool <= 0 || W <= 0 || nlines <= 0 || !pool || !att || !rgb || !labels || !lines) return -1;
  if (n == 0) return 0;
  if (!draw || !uv || !uv_proj || !rgb_out || !lines_out || !labels_out || !pixel_out) return -1;
  GatherBatchArgs a{pool, draw, n, W, npool, att, rgb, labels, lines, nlines, uv, uv_proj, rgb_out, lines_out, labels_out, pixel_out};
  hipLaunchKernelGGL(gather_batch_kernel, grid1(n), dim3(256), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int neat_copy_batch(const void* const* src, void* const* dst, const long long* nbytes, int n, void* stream) {
  if (n < 0 || n > COPY_BATCH_MAX) return -1;
  if (n == 0) return 0;
  if (!src || !dst || !nbytes) return -1;
  CopyBatchArgs a{};
  long long mx = 0;
  for (int i = 0; i < n; ++i) {
    if (!src[i] || !dst[i] || nbytes[i] < 0 || (nbytes[i] & 3) || ((size_t)src[i] & 3) || ((size_t)dst[i] & 3)) return -1;
    a.src[i] = (const unsigned*)src[i]; a.dst[i] = (unsigned*)dst[i]; a.words[i] = nbytes[i] >> 2;
    mx = nbytes[i] > mx ? nbytes[i] : mx;
  }
  a.n = n;
  const int by = (int)((mx / 4 + 1023) / 1024);          // 256 threads x 4 words per block
  hipLaunchKernelGGL(copy_batch_kernel, dim3(by < 1 ? 1 : (by > 1024 ? 1024 : by), n), dim3(256), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int neat_adam_step(float* params, const float* const* grads, const long long* seg_offsets, const int* seg_steps, int nseg,
                   float* exp_avg, float* exp_avg_sq, float lr, float beta1, float beta2, float eps, void* stream) {
  if (nseg <= 0) return 0;
  if (!params || !grads || !seg_offsets || !seg_steps || !exp_avg || !exp_avg_sq || nseg > ADAM_MAXSEG) return -1;
  AdamSegs segs{};
  for (int s = 0; s < nseg; ++s) {
    segs.g[s] = grads[s]; segs.off[s] = seg_offsets[s];
    if (grads[s]) {
      if (seg_steps[s] < 1) return -1;
      const double bc1 = 1.0 - pow((double)beta1, (double)seg_steps[s]), bc2 = 1.0 - pow((double)beta2, (double)seg_steps[s]);
      segs.lr_over_bc1[s] = (float)((double)lr / bc1); segs.inv_sqrt_bc2[s] = (float)(1.0 / sqrt(bc2));
    }
  }
  segs.off[nseg] = seg_offsets[nseg];
  segs.nseg = nseg;
  const long long n = seg_offsets[nseg];
  if (n <= 0) return 0;
  const long long per_block = 1024LL * ADAM_PASSES;    // ADAM_PASSES float4 passes of 256 threads
  const long long blocks = (n + per_block - 1) / per_block;
  hipLaunchKernelGGL(adam_flat_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, params, segs, exp_avg,
                     exp_avg_sq, n, beta1, beta2, eps, (const float*)nullptr);
  return (int)hipGetLastError();
}

int neat_adam_step_coef(float* params, const float* const* grads, const long long* seg_offsets, int nseg, float* exp_avg, float* exp_avg_sq,
                        const float* coef, float beta1, float beta2, float eps, void* stream) {
  if (nseg <= 0) return 0;
  if (!params || !grads || !seg_offsets || !exp_avg || !exp_avg_sq || !coef || nseg > ADAM_MAXSEG) return -1;
  AdamSegs segs{};
  for (int s = 0; s < nseg; ++s) { segs.g[s] = grads[s]; segs.off[s] = seg_offsets[s]; }
  segs.off[nseg] = seg_offsets[nseg];
  segs.nseg = nseg;
  const long long n = seg_offsets[nseg];
  if (n <= 0) return 0;
  const long long per_block = 1024LL * ADAM_PASSES;
  const long long blocks = (n + per_block - 1) / per_block;
  hipLaunchKernelGGL(adam_flat_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, params, segs, exp_avg,
                     exp_avg_sq, n, beta1, beta2, eps, coef);
  return (int)hipGetLastError();
}

int neat_ffn_forward(const float* x, int J, const float* W0, const float* b0, const float* W1, const float* b1, const float* W2,
                     const float* b2, float* h1, float* h2, float* y, void* stream) {
  if (J <= 0) return 0;
  if (!x || !W0 || !b0 || !W1 || !b1 || !W2 || !b2 || !h1 || !h2 || !y) return -1;
  hipStream_t st = (hipStream_t)stream;
  if (J > FFN_FUSED_MIN_ROWS) {       // many rows: one fused launch, 8 rows per workgroup
    hipLaunchKernelGGL(ffn_forward_kernel, dim3((J + FFN_RB - 1) / FFN_RB), dim3(FFN_H), 0, st, x, J, W0, b0, W1, b1, W2, b2, h1, h2, y);
    return (int)hipGetLastError();
  }
  // few rows (the 64 latents of the ABC scenes): one launch per layer, each spread over rows x 32-output blocks
  const dim3 gh((J + FFN_RB - 1) / FFN_RB, FFN_H / 32), g3((J + FFN_RB - 1) / FFN_RB, 1);
  const float* nogate = nullptr; float* noy2 = nullptr;
  if (g_ffn_mfma) {      // the two 256 x 256 layers on the fp32 matrix pipe (tuning key 28)
    const dim3 gm((J + 31) / 32, FFN_H / 32);
    hipLaunchKernelGGL(ffn_mfma_kernel<false>, gm, dim3(256), 0, st, x, J, W0, b0, nogate, 1, h1);
    hipLaunchKernelGGL(ffn_mfma_kernel<false>, gm, dim3(256), 0, st, (const float*)h1, J, W1, b1, nogate, 1, h2);
  } else {
    hipLaunchKernelGGL(ffn_dense_kernel<false>, gh, dim3(256), 0, st, x, J, FFN_H, FFN_H, W0, b0, nogate, 1, h1, noy2);
    hipLaunchKernelGGL(ffn_dense_kernel<false>, gh, dim3(256), 0, st, (const float*)h1, J, FFN_H, FFN_H, W1, b1, nogate, 1, h2, noy2);
  }
  hipLaunchKernelGGL(ffn_dense_kernel<false>, g3, dim3(256), 0, st, (const float*)h2, J, FFN_H, 3, W2, b2, nogate, 0, y, noy2);
  return (int)hipGetLastError();
}

int neat_ffn_backward(const float* x, int J, const float* W0, const float* W1, const float* W2, const float* h1, const float* h2,
                      const float* dy, float* ws2, float* dx, float* dW0, float* db0, float* dW1, float* db1, float* dW2, float* db2,
                      void* stream) {
  if (J <= 0) return 0;
  if (!x || !W0 || !W1 || !W2 || !h1 || !h2 || !dy || !ws2 || !dx || !dW0 || !db0 || !dW1 || !db1 || !dW2 || !db2) return -1;
  float* d_a1 = ws2; float* d_a2 = ws2 + (size_t)J * FFN_H;
  hipStream_t st = (hipStream_t)stream;
  if (J > FFN_FUSED_MIN_ROWS)
    hipLaunchKernelGGL(ffn_backward_data_kernel, dim3((J + FFN_RB - 1) / FFN_RB), dim3(FFN_H), 0, st, dy, J, W0, W1, W2, h1, h2, d_a1, d_a2, dx);
  else {
    const dim3 gh((J + FFN_RB - 1) / FFN_RB, FFN_H / 32);
    const float* nobias = nullptr; const float* nogate = nullptr; float* noy2 = nullptr;
    hipLaunchKernelGGL(ffn_dense_kernel<true>, gh, dim3(256), 0, st, dy, J, 3, FFN_H, W2, nobias, h2, 0, d_a2, noy2);
    if (g_ffn_mfma) {
      const dim3 gm((J + 31) / 32, FFN_H / 32);
      hipLaunchKernelGGL(ffn_mfma_kernel<true>, gm, dim3(256), 0, st, (const float*)d_a2, J, W1, nobias, h1, 0, d_a1);
      hipLaunchKernelGGL(ffn_mfma_kernel<true>, gm, dim3(256), 0, st, (const float*)d_a1, J, W0, nobias, nogate, 0, dx);
    } else {
      hipLaunchKernelGGL(ffn_dense_kernel<true>, gh, dim3(256), 0, st, (const float*)d_a2, J, FFN_H, FFN_H, W1, nobias, h1, 0, d_a1, noy2);
      hipLaunchKernelGGL(ffn_dense_kernel<true>, gh, dim3(256), 0, st, (const float*)d_a1, J, FFN_H, FFN_H, W0, nobias, nogate, 0, dx, noy2);
    }
  }
  if (g_ffn_mfma)
    hipLaunchKernelGGL(ffn_wgrad_mfma_kernel, dim3(FFN_H / 32, FFN_H / 32, 3), dim3(64 * FFN_WNW), 0, (hipStream_t)stream, x, h1, h2, d_a1, d_a2, dy, J, dW0, db0,
                       dW1, db1, dW2, db2);
  else
  hipLaunchKernelGGL(ffn_backward_weights_kernel, dim3(FFN_H / FFN_RN, 3), dim3(64 * FFN_JG), 0, (hipStream_t)stream, x, h1, h2, d_a1, d_a2, dy, J, dW0, db0,
                     dW1, db1, dW2, db2);
  return (int)hipGetLastError();
}

int neat_loss_terms(const float* rgb, const float* rgb_gt, int R, const float* gtheta, int E, const float* loc3, const float* loc2c, int K,
                    const float* glo3, const float* glo2c, int J, float* scal, float* d_rgb, float* d_gtheta, float* pair_cost,
                    float eik_grad_scale, void* stream) {
  if (R <= 0 || !rgb || !rgb_gt || !scal || !d_rgb || E < 0 || K < 0 || J < 0) return -1;
  if ((E > 0 && (!gtheta || !d_gtheta)) || (K > 0 && J > 0 && (!loc3 || !loc2c || !glo3 || !glo2c || !pair_cost))) return -1;
  LossTermsArgs a{rgb, rgb_gt, R, gtheta, E, loc3, loc2c, (J > 0 ? K : 0), glo3, glo2c, J, scal, d_rgb, d_gtheta, pair_cost, eik_grad_scale};
  hipLaunchKernelGGL(loss_terms_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int neat_loss_lines_terms(const float* pred_px, const float* pred_calib, const float* gt5, const float* Kmat, int L, float threshold, float* out3,
                          float* d_pred_calib, float grad_scale, const float* rgb, const float* rgb_gt, int R, const float* gtheta, int E,
                          const float* loc3, const float* loc2c, int K, const float* glo3, const float* glo2c, int J, float* scal, float* d_rgb,
                          float* d_gtheta, float* pair_cost, float eik_grad_scale, const float* w2c, const float* lines3d, float* d_lines3d,
                          void* stream) {
  if (L <= 0 || !pred_px || !pred_calib || !gt5 || !Kmat || !out3 || !d_pred_calib) return -1;
  if (d_lines3d && (!w2c || !lines3d)) return -1;
  if (R <= 0 || !rgb || !rgb_gt || !scal || !d_rgb || E < 0 || K < 0 || J < 0) return -1;
  if ((E > 0 && (!gtheta || !d_gtheta)) || (K > 0 && J > 0 && (!loc3 || !loc2c || !glo3 || !glo2c || !pair_cost))) return -1;
  LineLossesArgs l{pred_px, pred_calib, gt5, Kmat, L, threshold, out3, d_pred_calib, grad_scale, w2c, lines3d, d_lines3d};
  LossTermsArgs a{rgb, rgb_gt, R, gtheta, E, loc3, loc2c, (J > 0 ? K : 0), glo3, glo2c, J, scal, d_rgb, d_gtheta, pair_cost, eik_grad_scale};
  hipLaunchKernelGGL(loss_lines_terms_kernel, dim3(2), dim3(1024), 0, (hipStream_t)stream, l, a);
  return (int)hipGetLastError();
}

int neat_loss_pairs(const long long* ri, const long long* ci, const int* n_match, int Kmax, const float* loc3, const float* loc2c,
                    const float* loc2, const float* glo3, const float* glo2c, const float* glo2, int J, const float* pair_cost, float* scal,
                    float* d_glo3, float* d_glo2c, const float* line_loss, float w_eik, float w_line, float w_j3, float w_j2, int weighted_grads,
                    float* total, const float* w2c, void* stream) {
  if (Kmax < 0 || J <= 0 || !ri || !ci || !n_match || !loc3 || !loc2c || !loc2 || !glo3 || !glo2c || !glo2 || !pair_cost || !scal ||
      !d_glo3 || !d_glo2c || !line_loss) return -1;
  LossPairsArgs a{ri, ci, n_match, Kmax, loc3, loc2c, loc2, glo3, glo2c, glo2, J, pair_cost, scal, d_glo3, d_glo2c, line_loss, w_eik, w_line,
                  w_j3, w_j2, weighted_grads, total, w2c};
  hipLaunchKernelGGL(loss_pairs_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int neat_l3d(const float* x, const float* o, const float* d, const float* normal, int R, float* l3d, void* stream) {
  if (R <= 0) return 0;
  if (!x || !o || !d || !normal || !l3d) return -1;
  hipLaunchKernelGGL(l3d_kernel, dim3((R + 255) / 256), dim3(256), 0, (hipStream_t)stream, x, o, d, normal, R, l3d);
  return (int)hipGetLastError();
}

int neat_junction_cost(const float* cand2d, const float* gt2d, int V, int C, float* cost, void* stream) {
  if (V <= 0 || C <= 0) return 0;
  if (!cand2d || !gt2d || !cost) return -1;
  hipLaunchKernelGGL(junction_cost_kernel, dim3((V * C + 255) / 256), dim3(256), 0, (hipStream_t)stream, cand2d, gt2d, V, C, cost);
  return (int)hipGetLastError();
}

int neat_junction_gate(const long long* rows, const long long* cols, int K, const float* cost, int C, const float* cand3d,
                       const float* cand2d, const float* cand2d_calib, int use_median, float* median, unsigned char* good, float* j3d,
                       float* j2d, float* j2d_calib, void* stream) {
  if (K <= 0) return 0;
  if (K > 2048 || !rows || !cols || !cost || !cand3d || !cand2d || !cand2d_calib || !good || !j3d || !j2d || !j2d_calib ||
      (use_median && !median)) return -1;
  JunctionGateArgs a{rows, cols, K, cost, C, cand3d, cand2d, cand2d_calib, use_median, median, good, j3d, j2d, j2d_calib};
  hipLaunchKernelGGL(junction_gate_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int neat_inv_small(const float* A, int n, int lda, float* out, void* stream) {
  if (!A || !out || n < 1 || n > 4 || lda < n) return -1;
  hipLaunchKernelGGL(inv_small_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, A, n, lda, out);
  return (int)hipGetLastError();
}

int neat_camera_mats(const float* pose, const float* K, int kstride, float* w2c, float* K3, void* stream) {
  if (!pose || !K || !w2c || !K3 || kstride < 3) return -1;
  hipLaunchKernelGGL(camera_mats_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, pose, K, kstride, w2c, K3);
  return (int)hipGetLastError();
}

int neat_project2d(const float* K, const float* w2c, const float* X, int N, float* uv, void* stream) {
  if (N <= 0) return 0;
  if (!K || !w2c || !X || !uv) return -1;
  hipLaunchKernelGGL(project2d_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, K, w2c, X, N, uv);
  return (int)hipGetLastError();
}

int neat_project2d_pair(const float* K, const float* K2, const float* w2c, const float* X, int N, float* uv, float* uv2, void* stream) {
  if (N <= 0) return 0;
  if (!K || !K2 || !w2c || !X || !uv || !uv2) return -1;
  hipLaunchKernelGGL(project2d_pair_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, K, K2, w2c, X, N, uv, uv2);
  return (int)hipGetLastError();
}

int neat_camera_setup(const float* uv, const float* uv2, const float* pose, const float* K, int kstride, int R, float* dirs, float* origins,
                      float* dirs2, float* w2c, float* K3, void* stream) {
  if (R <= 0 || !uv || !pose || !K || !dirs || !origins || (uv2 && !dirs2) || !w2c || !K3 || kstride < 3) return -1;
  hipLaunchKernelGGL(camera_setup_kernel, grid1(R), dim3(256), 0, (hipStream_t)stream, uv, uv2, pose, K, kstride, R, dirs, origins, dirs2, w2c, K3);
  return (int)hipGetLastError();
}

int neat_project2d_backward(const float* K, const float* w2c, const float* X, int N, const float* d_uv, float* d_X, void* stream) {
  if (N <= 0) return 0;
  if (!K || !w2c || !X || !d_uv || !d_X) return -1;
  hipLaunchKernelGGL(project2d_bwd_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, K, w2c, X, N, d_uv, d_X);
  return (int)hipGetLastError();
}

int neat_line_loss(const float* pred, const float* gt, const float* weight, int R, float threshold, float* out2, float* per_line,
                   float* d_pred, void* stream) {
  if (R <= 0 || !pred || !gt || !weight || !out2 || !per_line || !d_pred) return -1;
  hipLaunchKernelGGL(line_loss_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, pred, gt, weight, R, threshold, out2, per_line, d_pred);
  return (int)hipGetLastError();
}

int neat_line_losses(const float* pred_px, const float* pred_calib, const float* gt5, const float* K, int R, float threshold, float* out3,
                     float* d_pred_calib, float grad_scale, void* stream) {
  if (R <= 0 || !pred_px || !pred_calib || !gt5 || !K || !out3 || !d_pred_calib) return -1;
  hipLaunchKernelGGL(line_losses_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, pred_px, pred_calib, gt5, K, R, threshold, out3, d_pred_calib, grad_scale);
  return (int)hipGetLastError();
}

size_t neat_lsap_ws_bytes(int nr, int nc) { LsapWs w; lsap_layout(nullptr, nr, nc, &w); return w.total; }

int neat_lsap(const float* cost, int nr, int nc, const unsigned char* row_mask, const unsigned char* col_mask, long long* row_ind,
              long long* col_ind, int* n_match, void* ws, void* stream) {
  if (nr < 0 || nc < 0 || !n_match) return -1;
  if (nr == 0 || nc == 0) return (int)hipMemsetAsync(n_match, 0, sizeof(int), (hipStream_t)stream);
  if (!cost || !row_ind || !col_ind || !ws) return -1;
  LsapWs w;
  lsap_layout(ws, nr, nc, &w);
  LsapArgs a{cost, nr, nc, row_mask, row_ind, col_ind, n_match, w.d, w.i};
  a.col_mask = col_mask;
  const size_t mx = (size_t)(nr > nc ? nr : nc), dbytes = ws_offset(ws, w.i);
  size_t lds = 0;
  constexpr size_t LSAP_LDS_MAX = 156 * 1024;
  a.cost_lds_off = -1;
  if (w.total <= LSAP_LDS_MAX) {
    NEAT_CHECK(lds_limit<&lsap_kernel>((int)LSAP_LDS_MAX));
    a.use_lds = 1; a.lds_int_off = (int)dbytes; lds = (w.total + 15) & ~(size_t)15;
    const size_t cbytes = (size_t)nr * nc * sizeof(float);
    if (lds + cbytes <= LSAP_LDS_MAX) { a.cost_lds_off = (int)lds; lds += cbytes; }      // the cost matrix too (8 x 2048 fits)
  }
  // threads: two columns per thread, whole waves (a small problem does not pay 16-wave barriers; eight columns per thread measured slower)
  int threads = (int)((mx + 1) / 2 + 63) / 64 * 64;
  threads = threads < 64 ? 64 : (threads > LSAP_WG ? LSAP_WG : threads);
  hipLaunchKernelGGL(lsap_kernel, dim3(1), dim3(threads), lds, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

size_t neat_dbscan_ws_bytes(int n) { DbscanWs w; dbscan_layout(nullptr, n, &w); return w.total; }

int neat_dbscan_means(const float* points, int n, double eps, float* centres, unsigned char* valid, int* count, void* ws, void* stream) {
  if (n <= 0 || n > DBSCAN_MAXN || !points || !centres || !valid || !count || !ws || !(eps > 0.0)) return -1;
  DbscanWs w;
  dbscan_layout(ws, n, &w);
  hipLaunchKernelGGL(dbscan_init_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, w.parent, w.has_nb, n);
  hipLaunchKernelGGL(dbscan_union_kernel, dim3(n), dim3(128), 0, (hipStream_t)stream, points, n, eps * eps, w.parent, w.has_nb);
  // mode 2 (18 n bytes of dynamic LDS fit next to the 32 KB of labels): O(n) fixed-point sums; else one wavefront per cluster over all
  // points, read from LDS (mode 1: 12 n bytes fit) or from global memory (mode 0)
  const size_t acc_bytes = (size_t)(n / 2) * 28 + (size_t)n * 4, pbytes = (size_t)n * 12;
  const int mode = acc_bytes <= 96 * 1024 ? 2 : (pbytes <= 96 * 1024 ? 1 : 0);
  if (mode) NEAT_CHECK(lds_limit<&dbscan_finish_kernel>(96 * 1024));
  hipLaunchKernelGGL(dbscan_finish_kernel, dim3(1), dim3(1024), mode == 2 ? acc_bytes : (mode == 1 ? pbytes : 0), (hipStream_t)stream, points, n,
                     w.parent, w.has_nb, centres, valid, count, mode);
  return (int)hipGetLastError();
}

int neat_volume_weights(const float* z, const float* sdf, int R, int S, const float* beta, float* weights, void* stream) {
  if (R <= 0 || S <= 0) return 0;
  hipLaunchKernelGGL(volume_weights_kernel, dim3((R + 3) / 4), dim3(256), 0, (hipStream_t)stream, z, sdf, R, S, beta, weights);
  return (int)hipGetLastError();
}

// ---- ABI v15: wireframe parsing (kernels_parse.hpp) -----------------------------------------------------------------------------
int neat_parse_match(const float* lines2d, int n, const float* gt, int m, int gt_stride, float threshold, int* label, float* mindis,
                     void* stream) {
  if (n < 0 || m < 0 || (m > 0 && (!gt || gt_stride < 4))) return -1;
  if (n == 0) return 0;
  if (!lines2d || !label || !mindis) return -1;
  hipLaunchKernelGGL(parse_match_kernel, grid1(n, PARSE_WG), dim3(PARSE_WG), 0, (hipStream_t)stream, lines2d, n, gt, m, gt_stride, threshold,
                     label, mindis);
  return (int)hipGetLastError();
}

size_t neat_parse_group_ws_bytes(int n, int m) { ParseGroupWs w; return parse_group_layout(nullptr, n, m, PARSE_TILE, &w) ? w.total : 0; }

int neat_parse_group(const int* label, const float* lines3d, const float* l3d, int n, int m, float* lines, float* scores, int* count,
                     void* ws, void* stream) {
  ParseGroupWs w;
  if (!parse_group_layout(ws, n, m, PARSE_TILE, &w) || !count) return -1;
  hipStream_t st = (hipStream_t)stream;
  if (n == 0 || m == 0) return (int)hipMemsetAsync(count, 0, sizeof(int), st);
  if (!label || !lines3d || !l3d || !lines || !scores || !ws) return -1;
  NEAT_CHECK(hipMemsetAsync(w.run, 0, (size_t)w.tiles * m * sizeof(int), st));
  hipLaunchKernelGGL(parse_group_tile_kernel, dim3(w.tiles), dim3(PARSE_WG), 0, st, label, 2 * n, m, w.run, w.order, 0);
  hipLaunchKernelGGL(parse_group_scan_kernel, dim3(1), dim3(1024), 0, st, w.run, w.tiles, m, w.cnt, w.start, w.slot, count);
  hipLaunchKernelGGL(parse_group_tile_kernel, dim3(w.tiles), dim3(PARSE_WG), 0, st, label, 2 * n, m, w.run, w.order, 1);
  hipLaunchKernelGGL(parse_group_reduce_kernel, dim3(m), dim3(PARSE_WG), 0, st, w.order, w.cnt, w.start, w.slot, lines3d, l3d, n, lines, scores);
  return (int)hipGetLastError();
}

size_t neat_parse_vote_ws_bytes(int J, int mcap) { ParseVoteWs w; return parse_vote_layout(nullptr, J, mcap, &w) ? w.total : 0; }

int neat_parse_vote(const float* junctions, int J, const float* lines, const int* count, int mcap, float threshold, int view, int* votes,
                    int* first, void* ws, void* stream) {
  if (J < 0 || mcap < 0 || view < 0) return -1;
  if (J == 0 || mcap == 0) return 0;
  ParseVoteWs w;
  if (!junctions || !lines || !count || !votes || !first || !ws || !parse_vote_layout(ws, J, mcap, &w)) return -1;
  hipStream_t st = (hipStream_t)stream;
  const size_t total = (size_t)J * w.nc;
  hipLaunchKernelGGL(parse_vote_cost_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, junctions, J, lines, count, w.nc, w.cost, w.cmask);
  NEAT_CHECK(hipGetLastError());
  const int e = neat_lsap(w.cost, J, w.nc, nullptr, w.cmask, w.rows, w.cols, w.n_match, w.lsap, stream);
  if (e != 0) return e;
  hipLaunchKernelGGL(parse_vote_apply_kernel, grid1(w.k), dim3(256), 0, st, w.rows, w.cols, w.n_match, w.k, w.cost, w.nc, threshold, view, votes, first);
  return (int)hipGetLastError();
}

size_t neat_parse_graph_ws_bytes(int V, int mcap, int J) { ParseGraphWs w; return parse_graph_layout(nullptr, V, mcap, J, &w) ? w.total : 0; }

int neat_parse_graph(const float* vlines, const float* vscores, const int* vcount, int V, int mcap, float score_threshold,
                     const float* junctions, const int* votes, const int* first, int J, float* lines_out, float* junc_out,
                     unsigned char* graph, int* pairs, float* wfi, int ecap, int* counts, void* ws, void* stream) {
  ParseGraphWs w;
  if (!parse_graph_layout(ws, V, mcap, J, &w) || ecap < 0 || !counts) return -1;
  hipStream_t st = (hipStream_t)stream;
  if ((V > 0 && mcap > 0 && (!vlines || !vscores || !vcount || !lines_out || !ws)) ||
      (J > 0 && (!junctions || !votes || !first || !junc_out || !graph || !ws)) || (ecap > 0 && (!pairs || !wfi))) return -1;
  NEAT_CHECK(hipMemsetAsync(counts, 0, 3 * sizeof(int), st));
  const int ncap = V * mcap;
  if (ncap == 0 && J == 0) return 0;
  hipLaunchKernelGGL(parse_select_kernel, dim3(2), dim3(1024), 0, st, vlines, vscores, vcount, V, mcap, score_threshold, junctions, votes, first,
                     J, lines_out, junc_out, w.idx, counts);
  if (J == 0 || ncap == 0) return (int)hipGetLastError();
  NEAT_CHECK(hipMemsetAsync(graph, 0, (size_t)J * J, st));
  hipLaunchKernelGGL(parse_graph_mark_kernel, grid1(ncap, PARSE_WG), dim3(PARSE_WG), 0, st, lines_out, junc_out, counts, ncap, J, graph);
  hipLaunchKernelGGL(parse_edge_count_kernel, dim3(J), dim3(64), 0, st, graph, counts, J, w.rowcnt);
  hipLaunchKernelGGL(parse_edge_write_kernel, dim3(J), dim3(64), 0, st, graph, counts, J, w.rowcnt, J, junc_out, ecap, pairs, wfi);
  return (int)hipGetLastError();
}

size_t neat_parse_visibility_ws_bytes(int ecap, int V) { ParseVisWs w; return parse_vis_layout(nullptr, ecap, V, &w) ? w.total : 0; }

int neat_parse_visibility(const float* lines, const int* n_lines, int ecap, const float* gt, int gt_stride, const int* gt_off,
                          const float* K3, const float* w2c, int V, float ckdist, int ckview, int* vis_count, float* checked,
                          int* n_checked, void* ws, void* stream) {
  ParseVisWs w;
  if (!parse_vis_layout(ws, ecap, V, &w) || !n_checked) return -1;
  hipStream_t st = (hipStream_t)stream;
  if (ecap == 0) return (int)hipMemsetAsync(n_checked, 0, sizeof(int), st);
  if (!lines || !vis_count || !checked || !ws || (V > 0 && (!gt_off || !K3 || !w2c || gt_stride < 4))) return -1;
  if (V > 0)
    hipLaunchKernelGGL(parse_vis_kernel, dim3((ecap + PARSE_WG - 1) / PARSE_WG, V), dim3(PARSE_WG), 0, st, lines, n_lines, ecap, gt, gt_stride,
                       gt_off, K3, w2c, ckdist, w.vis);
  hipLaunchKernelGGL(parse_vis_count_kernel, dim3(1), dim3(1024), 0, st, lines, n_lines, ecap, V, w.vis, ckview, vis_count, w.idx, checked, n_checked);
  return (int)hipGetLastError();
}

// ---- added to ABI v15: the SDF's level surface as a triangle mesh (kernels_mesh.hpp) -------------------------------------------------------
static bool mesh_axes(const int* n, const double* b0, const double* b1, MeshAxes* g) {
  if (!n || !b0 || !b1) return false;
  for (int a = 0; a < 3; ++a) {
    if (n[a] < 2 || !std::isfinite(b0[a]) || !std::isfinite(b1[a])) return false;
    g->n[a] = n[a]; g->b0[a] = b0[a]; g->b1[a] = b1[a]; g->step[a] = (b1[a] - b0[a]) / (double)(n[a] - 1);
  }
  return true;
}
int neat_grid_points(float* x_fm, int ldp, long long first_node, int count, const int* n, const double* b0, const double* b1, void* stream) {
  MeshAxes g;
  if (!x_fm || count < 0 || ldp < count || first_node < 0 || !mesh_axes(n, b0, b1, &g)) return -1;
  if (first_node + count > (long long)n[0] * n[1] * n[2]) return -1;
  if (ldp == 0) return 0;
  hipLaunchKernelGGL(grid_points_kernel, grid1(ldp), dim3(256), 0, (hipStream_t)stream, x_fm, ldp, first_node, count, g);
  return (int)hipGetLastError();
}

size_t neat_mesh_ws_bytes(int nx, int ny, int nz) { MeshWs w; return mesh_layout(nullptr, nx, ny, nz, MESH_TILE, &w) ? w.total : 0; }

static int mesh_args(const float* grid, int nx, int ny, int nz, float level, void* ws, MeshArgs* a) {      // -> tiles; 0: refused
  MeshWs w;
  if (!mesh_layout(ws, nx, ny, nz, MESH_TILE, &w) || !grid || !ws || level != level) return 0;
  *a = MeshArgs{};
  a->grid = grid; a->nx = nx; a->ny = ny; a->nz = nz; a->nodes = w.nodes; a->level = level;
  a->emask = w.emask; a->vbase = w.vbase; a->tile_v = w.tile_v; a->tile_f = w.tile_f;
  return w.tiles;
}

int neat_mesh_count(const float* grid, int nx, int ny, int nz, float level, void* ws, int* counts, void* stream) {
  MeshArgs a;
  const int tiles = mesh_args(grid, nx, ny, nz, level, ws, &a);
  if (!tiles || !counts) return -1;
  a.counts = counts;
  hipLaunchKernelGGL(mesh_count_kernel, dim3(tiles), dim3(MESH_WG), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(mesh_scan_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, a.tile_v, a.tile_f, tiles, counts);
  return (int)hipGetLastError();
}

int neat_mesh_emit(const float* grid, int nx, int ny, int nz, const double* b0, const double* b1, float level, void* ws, float* verts, int nv,
                   int* faces, int nf, void* stream) {
  MeshArgs a;
  const int tiles = mesh_args(grid, nx, ny, nz, level, ws, &a), n[3] = {nx, ny, nz};
  if (!tiles || nv < 0 || nf < 0 || (nv > 0 && !verts) || (nf > 0 && !faces) || !mesh_axes(n, b0, b1, &a.ax)) return -1;
  if (nv == 0) return 0;                 // no vertex, hence no face
  a.verts = verts; a.nv = nv; a.faces = faces; a.nf = nf;
  hipLaunchKernelGGL(mesh_verts_kernel, dim3(tiles), dim3(MESH_WG), 0, (hipStream_t)stream, a);
  if (nf > 0) hipLaunchKernelGGL(mesh_faces_kernel, dim3(tiles), dim3(MESH_WG), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int neat_unit_rows3(float* g, int n, void* stream) {
  if (n < 0 || (n > 0 && !g)) return -1;
  if (n == 0) return 0;
  hipLaunchKernelGGL(mesh_normalize_kernel, grid1(n), dim3(256), 0, (hipStream_t)stream, g, n);
  return (int)hipGetLastError();
}

// ---- added to ABI v15: the evaluation mesh of a checkpoint (kernels_evalmesh.hpp) ------------------------------------------------------
static bool finite_all(const double* x, int n) {
  if (!x) return false;
  for (int i = 0; i < n; ++i) if (!std::isfinite(x[i])) return false;
  return true;
}

int neat_grid_points_affine(float* x_fm, int ldp, long long first_node, int count, const int* n, const double* b0, const double* b1,
                            const double* R, const double* c, void* stream) {
  MeshAxes g;
  if (!x_fm || count < 0 || ldp < count || first_node < 0 || !mesh_axes(n, b0, b1, &g) || !finite_all(R, 9) || !finite_all(c, 3)) return -1;
  if (first_node + count > (long long)n[0] * n[1] * n[2]) return -1;
  if (ldp == 0) return 0;
  Frame3 f;
  for (int i = 0; i < 9; ++i) f.R[i] = R[i];
  for (int i = 0; i < 3; ++i) f.c[i] = c[i];
  hipLaunchKernelGGL(grid_points_affine_kernel, grid1(ldp, EMESH_WG), dim3(EMESH_WG), 0, (hipStream_t)stream, x_fm, ldp, first_node, count, g, f);
  return (int)hipGetLastError();
}

size_t neat_mesh_moments_ws_bytes(int nf) { SumTreeWs t; return sum_tree_layout(nullptr, nf, MOMENTS_TILE, EMESH_WG, MOMENTS_N, &t) ? t.total : 0; }

int neat_mesh_moments(const float* verts, int nv, const int* faces, int nf, const double* origin, void* ws, double* out, int* flag, void* stream) {
  SumTreeWs t;
  if (nv < 0 || !sum_tree_layout(ws, nf, MOMENTS_TILE, EMESH_WG, MOMENTS_N, &t) || !out || !flag || !finite_all(origin, 3) ||
      (nf > 0 && (!faces || !verts || nv == 0))) return -1;
  hipStream_t st = (hipStream_t)stream;
  if (nf == 0) {
    NEAT_CHECK(hipMemsetAsync(out, 0, (MOMENTS_N - 1) * sizeof(double), st));
    return (int)hipMemsetAsync(flag, 0, sizeof(int), st);
  }
  if (t.levels > 0 && (!ws || ((uintptr_t)ws & 7))) return -1;
  Origin3 o;
  for (int i = 0; i < 3; ++i) o.o[i] = origin[i];
  hipLaunchKernelGGL(mesh_moments_kernel, dim3((unsigned)t.m[0]), dim3(EMESH_WG), 0, st, verts, nv, faces, nf, o, t.level[0], t.m[0], t.levels == 0, out, flag);
  for (int k = 0; k < t.levels; ++k)
    hipLaunchKernelGGL(mesh_moments_level_kernel, dim3((unsigned)t.m[k + 1], MOMENTS_N), dim3(EMESH_WG), 0, st, (const double*)t.level[k], t.m[k],
                       t.level[k + 1], t.m[k + 1], k + 1 == t.levels, out, flag);
  return (int)hipGetLastError();
}

static bool affine_arg(const double* A, Affine34* a) {
  if (!finite_all(A, 12)) return false;
  for (int i = 0; i < 12; ++i) a->a[i] = A[i];
  return true;
}

int neat_affine_rows3(float* v, int n, const double* A, void* stream) {
  Affine34 a;
  if (n < 0 || (n > 0 && !v) || !affine_arg(A, &a)) return -1;
  if (n == 0) return 0;
  hipLaunchKernelGGL(affine_rows3_kernel, grid1(n, EMESH_WG), dim3(EMESH_WG), 0, (hipStream_t)stream, v, n, a);
  return (int)hipGetLastError();
}

size_t neat_affine_bounds3_ws_bytes(void) { double* p; return partials_layout(nullptr, BOUNDS_BLOCKS, 6, &p); }

int neat_affine_bounds3(const float* v, int n, const double* A, void* ws, double* out, void* stream) {
  Affine34 a;
  if (n < 1 || !v || !out || !ws || ((uintptr_t)ws & 7) || !affine_arg(A, &a)) return -1;
  double* partial;
  partials_layout(ws, BOUNDS_BLOCKS, 6, &partial);
  const int blocks = std::max(1, std::min(BOUNDS_BLOCKS, (n + EMESH_WG - 1) / EMESH_WG));
  hipLaunchKernelGGL(affine_bounds3_partial_kernel, dim3(blocks), dim3(EMESH_WG), 0, (hipStream_t)stream, v, n, a, partial);
  hipLaunchKernelGGL(affine_bounds3_finish_kernel, dim3(1), dim3(EMESH_WG), 0, (hipStream_t)stream, (const double*)partial, blocks, out);
  return (int)hipGetLastError();
}

static bool cut_plane(int axis, double value, int sign, CutPlane* p) {
  if (axis < 0 || axis > 2 || (sign != 1 && sign != -1) || !std::isfinite(value) || (double)(float)value != value) return false;
  p->axis = axis; p->value = value; p->sign = (double)sign;
  return true;
}

int neat_mesh_cut_count(const float* verts, int nv, const int* faces, int nf, int axis, double value, int sign, int* fcnt, long long* ekey,
                        int* used, void* stream) {
  CutPlane p;
  if (nv < 1 || nf < 1 || !verts || !faces || !fcnt || !ekey || !used || !cut_plane(axis, value, sign, &p)) return -1;
  NEAT_CHECK(hipMemsetAsync(used, 0, (size_t)nv * sizeof(int), (hipStream_t)stream));
  hipLaunchKernelGGL(cut_count_kernel, grid1(nf, EMESH_WG), dim3(EMESH_WG), 0, (hipStream_t)stream, verts, nv, faces, nf, p, fcnt, ekey, used);
  return (int)hipGetLastError();
}

int neat_mesh_cut_emit(const float* verts, int nv, const int* faces, int nf, int axis, double value, int sign, const int* used, const int* vmap,
                       const int* foff, const long long* ukey, int ncut, int nkeep, float* out_verts, int nv_out, int* out_faces, int nf_out,
                       void* stream) {
  CutPlane p;
  if (nv < 1 || nf < 1 || !verts || !faces || !used || !vmap || !foff || !cut_plane(axis, value, sign, &p)) return -1;
  if (ncut < 0 || nkeep < 0 || nkeep > nv || (ncut > 0 && !ukey) || (long long)nkeep + ncut != (long long)nv_out || nf_out < 0) return -1;
  if ((nv_out > 0 && !out_verts) || (nf_out > 0 && !out_faces)) return -1;
  if (nv_out == 0 || nf_out == 0) return 0;
  const long long lanes = (long long)nv + ncut;
  if ((lanes + EMESH_WG - 1) / EMESH_WG > (long long)INT_MAX) return -1;
  hipLaunchKernelGGL(cut_verts_kernel, dim3((unsigned)((lanes + EMESH_WG - 1) / EMESH_WG)), dim3(EMESH_WG), 0, (hipStream_t)stream, verts, nv, p, used,
                     vmap, ukey, ncut, nkeep, out_verts, nv_out);
  hipLaunchKernelGGL(cut_faces_kernel, grid1(nf, EMESH_WG), dim3(EMESH_WG), 0, (hipStream_t)stream, verts, nv, faces, nf, p, foff, vmap, ukey, ncut,
                     nkeep, out_faces, nf_out);
  return (int)hipGetLastError();
}

// ---- added to ABI v15: scoring a reconstruction against ground truth (kernels_eval.hpp) ------------------------------------------------
static bool eval_grid_args(const neat_eval_grid_t* h, EvalGrid* g) {
  if (!h || h->n < 0 || h->buckets < 1 || !(h->cell > 0.0) || !std::isfinite(h->cell) || !h->start) return false;
  long long cells = 1;
  for (int a = 0; a < 3; ++a) {
    if (h->dim[a] < 1 || h->dim[a] > (1 << 20) || !std::isfinite(h->origin[a])) return false;
    g->o[a] = h->origin[a]; g->dim[a] = h->dim[a];
    cells = cells > INT_MAX ? cells : cells * h->dim[a];
  }
  if (h->dense && cells != (long long)h->buckets) return false;
  if (h->n > 0 && (!h->sidx || !h->spts)) return false;
  g->cell = h->cell; g->buckets = h->buckets; g->dense = h->dense ? 1 : 0; g->n = h->n;
  g->start = h->start; g->sidx = h->sidx; g->spts = h->spts;
  return true;
}

size_t neat_eval_grid_ws_bytes(int n, int buckets) { EvalGridWs w; return eval_grid_layout(nullptr, n, buckets, &w) ? w.total : 0; }

int neat_eval_grid(const double* points, const neat_eval_grid_t* grid, int* start, int* sidx, double* spts, void* ws, void* stream) {
  EvalGrid g;
  EvalGridWs w;
  if (!eval_grid_args(grid, &g) || !ws || start != grid->start || sidx != grid->sidx || spts != grid->spts || (g.n > 0 && !points)) return -1;
  if (!eval_grid_layout(ws, g.n, g.buckets, &w)) return -1;
  hipStream_t st = (hipStream_t)stream;
  NEAT_CHECK(hipMemsetAsync(w.cnt, 0, (size_t)g.buckets * sizeof(int), st));
  if (g.n > 0) hipLaunchKernelGGL(eval_grid_bin_kernel, grid1(g.n, EVAL_WG), dim3(EVAL_WG), 0, st, points, g, w.bucket_of, w.cnt);
  hipLaunchKernelGGL(eval_exscan_kernel, dim3(1), dim3(EVAL_SCAN_WG), 0, st, (const int*)w.cnt, start, g.buckets, (int*)nullptr);
  if (g.n > 0) hipLaunchKernelGGL(eval_grid_scatter_kernel, grid1(g.n, EVAL_WG), dim3(EVAL_WG), 0, st, points, g.n, (const int*)w.bucket_of, w.cnt,
                                  (const int*)start, sidx, spts);
  return (int)hipGetLastError();
}

int neat_eval_thin_round(const double* points, const neat_eval_grid_t* grid, double radius, unsigned char* state, int* undecided, void* stream) {
  EvalGrid g;
  if (!eval_grid_args(grid, &g) || !(radius >= 0.0) || !(radius <= grid->cell) || !undecided || (g.n > 0 && (!points || !state))) return -1;
  if (g.n == 0) return 0;
  hipLaunchKernelGGL(eval_thin_round_kernel, grid1(g.n, EVAL_WG), dim3(EVAL_WG), 0, (hipStream_t)stream, points, g, radius * radius, state, undecided);
  return (int)hipGetLastError();
}

int neat_eval_nearest(const neat_eval_grid_t* grid, const double* queries, int m, double max_dist, double* dist, int* idx, void* stream) {
  EvalGrid g;
  if (!eval_grid_args(grid, &g) || m < 0 || !(max_dist >= 0.0) || (m > 0 && (!queries || !dist || !idx))) return -1;
  if (m == 0) return 0;
  const double cap = max_dist * (1.0 + 1e-12);       // the `< max_dist` decision is the caller's, on the distance
  hipLaunchKernelGGL(eval_nearest_kernel, grid1(m, EVAL_WG), dim3(EVAL_WG), 0, (hipStream_t)stream, g, queries, m, cap, cap * cap, dist, idx);
  return (int)hipGetLastError();
}

int neat_eval_obs_mask(const double* points, int n, const double* lo, const double* hi, const double* bb0, double res, const unsigned char* mask,
                       const int* shape, int f32_quotient, unsigned char* flags, void* stream) {
  if (n < 0 || !lo || !hi || !bb0 || !shape || !mask || !(res > 0.0) || !std::isfinite(res) || (n > 0 && (!points || !flags))) return -1;
  EvalObs a;
  for (int c = 0; c < 3; ++c) {
    if (shape[c] < 1) return -1;
    a.lo[c] = lo[c]; a.hi[c] = hi[c]; a.bb0[c] = bb0[c]; a.shape[c] = shape[c];
  }
  a.res = res; a.f32_quotient = f32_quotient ? 1 : 0;
  if (n == 0) return 0;
  hipLaunchKernelGGL(eval_obs_mask_kernel, grid1(n, EVAL_WG), dim3(EVAL_WG), 0, (hipStream_t)stream, points, n, a, mask, flags);
  return (int)hipGetLastError();
}

size_t neat_eval_tri_ws_bytes(int nf) { EvalTriWs w; return eval_tri_layout(nullptr, nf, &w) ? w.total : 0; }

static inline bool eval_tri_ok(const double* verts, int nv, const int* faces, int nf, double density, void* ws, EvalTriWs* w) {
  return nv >= 0 && eval_tri_layout(ws, nf, w) && ws && density > 0.0 && std::isfinite(density) && (nf == 0 || (verts && faces && nv > 0));
}

int neat_eval_tri_count(const double* verts, int nv, const int* faces, int nf, double density, void* ws, int* total, void* stream) {
  EvalTriWs w;
  if (!eval_tri_ok(verts, nv, faces, nf, density, ws, &w) || !total) return -1;
  hipStream_t st = (hipStream_t)stream;
  if (nf > 0) hipLaunchKernelGGL(eval_tri_count_kernel, grid1(nf, EVAL_WG / 64), dim3(EVAL_WG), 0, st, verts, nv, faces, nf, density, w.counts);
  hipLaunchKernelGGL(eval_exscan_kernel, dim3(1), dim3(EVAL_SCAN_WG), 0, st, (const int*)w.counts, w.offs, nf, total);
  return (int)hipGetLastError();
}

int neat_eval_tri_emit(const double* verts, int nv, const int* faces, int nf, double density, void* ws, double* out, int total, void* stream) {
  EvalTriWs w;
  if (!eval_tri_ok(verts, nv, faces, nf, density, ws, &w) || total < 0 || (total > 0 && !out)) return -1;
  if (nf == 0 || total == 0) return 0;
  hipLaunchKernelGGL(eval_tri_emit_kernel, grid1(nf, EVAL_WG / 64), dim3(EVAL_WG), 0, (hipStream_t)stream, verts, nv, faces, nf, density,
                     (const int*)w.offs, out, total);
  return (int)hipGetLastError();
}

int neat_eval_line_cost(const double* pred, int n_pred, const double* gt, int n_gt, int ends, double* cost, void* stream) {
  if (n_pred < 0 || n_gt < 0 || (ends != 1 && ends != 2)) return -1;
  const long long total = (long long)n_pred * n_gt;
  if (total == 0) return 0;
  if (!pred || !gt || !cost || total > INT_MAX) return -1;
  hipLaunchKernelGGL(eval_line_cost_kernel, dim3((unsigned)((total + EVAL_WG - 1) / EVAL_WG)), dim3(EVAL_WG), 0, (hipStream_t)stream, pred, n_pred, gt,
                     n_gt, ends, cost);
  return (int)hipGetLastError();
}

// ---- added to ABI v15: pictures of a wireframe and of the mesh behind it (kernels_show.hpp) ---------------------------------------------
static inline bool show_grid_ok(long long items, int per_block) { return (items + per_block - 1) / per_block <= (long long)INT_MAX; }
static inline dim3 show_grid(long long items, int per_block) { return dim3((unsigned)((items + per_block - 1) / per_block)); }
static inline bool show_common(const double* cams, double near, void* ws) { return cams && ws && near > 0.0 && std::isfinite(near); }

size_t neat_show_ws_bytes(int F, int H, int W) { ShowWs s; return show_layout(nullptr, F, H, W, SHOW_QUEUE_CAP, &s) ? s.total : 0; }

int neat_show_ws_layout(int F, int H, int W, size_t* offsets) {
  ShowWs s;
  if (!offsets || !show_layout(nullptr, F, H, W, SHOW_QUEUE_CAP, &s)) return -1;
  const void* part[4] = {s.key, s.cov, s.covp, s.status};
  for (int i = 0; i < 4; ++i) offsets[i] = ws_offset(nullptr, part[i]);
  return 0;
}

int neat_show_clear(void* ws, int F, int H, int W, void* stream) {
  ShowWs s;
  if (!ws || !show_layout(ws, F, H, W, SHOW_QUEUE_CAP, &s) || !show_grid_ok(s.pixels, SHOW_WG)) return -1;
  hipLaunchKernelGGL(show_clear_kernel, show_grid(s.pixels, SHOW_WG), dim3(SHOW_WG), 0, (hipStream_t)stream, s.key, s.cov, s.covp, s.status, s.pixels);
  return (int)hipGetLastError();
}

int neat_show_mesh(const double* verts, int nv, const int* faces, int nf, const double* cams, int F, int H, int W, double near, void* ws,
                   void* stream) {
  ShowWs s;
  if (!show_layout(ws, F, H, W, SHOW_QUEUE_CAP, &s) || !show_common(cams, near, ws) || nv < 0 || nf < 0 || (nf > 0 && (!verts || !faces || nv < 1))) return -1;
  const long long items = (long long)F * nf;
  if (!show_grid_ok(items, SHOW_WG)) return -1;
  if (nf == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  NEAT_CHECK(hipMemsetAsync(s.queued, 0, sizeof(unsigned long long), st));
  hipLaunchKernelGGL(show_mesh_kernel, show_grid(items, SHOW_WG), dim3(SHOW_WG), 0, st, verts, nv, faces, nf, cams, F, H, W, near, s.key, s.status,
                     s.queued, s.queue, SHOW_QUEUE_CAP);
  hipLaunchKernelGGL(show_mesh_large_kernel, dim3(SHOW_LARGE_BLOCKS), dim3(SHOW_WG), 0, st, verts, nv, faces, nf, cams, F, H, W, near, s.key,
                     (const unsigned long long*)s.queued, (const long long*)s.queue, SHOW_QUEUE_CAP);
  return (int)hipGetLastError();
}

static inline bool show_cover_ok(double size, double bias, double hidden_alpha) {
  return size >= 0.0 && std::isfinite(size) && std::isfinite(bias) && hidden_alpha >= 0.0 && hidden_alpha <= 1.0;
}

int neat_show_lines(const double* lines, int n, const double* cams, int F, int H, int W, double near, double width, double bias,
                    double hidden_alpha, void* ws, void* stream) {
  ShowWs s;
  if (!show_layout(ws, F, H, W, SHOW_QUEUE_CAP, &s) || !show_common(cams, near, ws) || n < 0 || (n > 0 && !lines) || !show_cover_ok(width, bias,
      hidden_alpha)) return -1;
  const long long items = (long long)F * n;
  if (!show_grid_ok(items, SHOW_WG / 64)) return -1;
  if (n == 0) return 0;
  hipLaunchKernelGGL(show_lines_kernel, show_grid(items, SHOW_WG / 64), dim3(SHOW_WG), 0, (hipStream_t)stream, lines, n, cams, F, H, W, near,
                     width / 2.0 + 0.5, bias, hidden_alpha, (const unsigned long long*)s.key, s.cov);
  return (int)hipGetLastError();
}

int neat_show_points(const double* points, int n, const double* cams, int F, int H, int W, double near, double radius, double bias,
                     double hidden_alpha, void* ws, void* stream) {
  ShowWs s;
  if (!show_layout(ws, F, H, W, SHOW_QUEUE_CAP, &s) || !show_common(cams, near, ws) || n < 0 || (n > 0 && !points) || !show_cover_ok(radius, bias,
      hidden_alpha)) return -1;
  const long long items = (long long)F * n;
  if (!show_grid_ok(items, SHOW_WG)) return -1;
  if (n == 0) return 0;
  hipLaunchKernelGGL(show_points_kernel, show_grid(items, SHOW_WG), dim3(SHOW_WG), 0, (hipStream_t)stream, points, n, cams, F, H, W, near,
                     radius + 0.5, bias, hidden_alpha, (const unsigned long long*)s.key, s.covp);
  return (int)hipGetLastError();
}

int neat_show_resolve(const double* verts, int nv, const int* faces, int nf, const double* cams, int F, int H, int W, const double* colors, void* ws,
                      unsigned char* out, void* stream) {
  ShowWs s;
  if (!show_layout(ws, F, H, W, SHOW_QUEUE_CAP, &s) || !cams || !ws || !colors || !out || ((uintptr_t)out & 3) || nv < 0 || nf < 0 ||
      (nf > 0 && (!verts || !faces || nv < 1)))
    return -1;
  ShowStyle st;
  for (int c = 0; c < 3; ++c) {
    st.bg[c] = colors[c]; st.line[c] = colors[3 + c]; st.point[c] = colors[6 + c]; st.mesh[c] = colors[9 + c];
  }
  for (int c = 0; c < 12; ++c) if (!(colors[c] >= 0.0 && colors[c] <= 1.0)) return -1;
  const long long quads = (s.pixels + 3) / 4;
  if (!show_grid_ok(quads, SHOW_WG)) return -1;
  hipLaunchKernelGGL(show_resolve_kernel, show_grid(quads, SHOW_WG), dim3(SHOW_WG), 0, (hipStream_t)stream, verts, nv, faces, nf, cams, H, W, s.pixels, st,
                     (const unsigned long long*)s.key, (const float*)s.cov, (const float*)s.covp, (const int*)s.status, out);
  return (int)hipGetLastError();
}

// ---- frames of rendered views (kernels_frame.hpp) ----------------------------------------------------------------------------------------
static inline bool frame_blocks_ok(long long items) { return (items + FRAME_WG - 1) / FRAME_WG <= (long long)INT_MAX; }
static inline dim3 frame_blocks(long long items) { return dim3((unsigned)((items + FRAME_WG - 1) / FRAME_WG)); }

int neat_frame_put(const float* rgb, const float* normal, const float* depth, const float* gt, int n, long long p0, long long P,
                   unsigned char* rgb8, unsigned char* normal8, float* depth_out, float* err, void* stream) {
  if (n < 0 || p0 < 0 || P < 0 || p0 > P || (long long)n > P - p0) return -1;
  if ((normal && !normal8) || (depth && !depth_out) || (gt && (!rgb || !err))) return -1;
  if (n == 0 || (!rgb && !normal && !depth)) return 0;
  hipLaunchKernelGGL(frame_put_kernel, frame_blocks(3ll * n), dim3(FRAME_WG), 0, (hipStream_t)stream, rgb, normal, depth, gt, n, p0, rgb8, normal8,
                     depth_out, err);
  return (int)hipGetLastError();
}

size_t neat_frame_sum_ws_bytes(long long n) { SumTreeWs t; return sum_tree_layout(nullptr, n, FRAME_WG, FRAME_WG, 1, &t) ? t.total : 0; }

int neat_frame_sum(const float* x, long long n, void* ws, double* out, void* stream) {
  SumTreeWs t;
  if (!sum_tree_layout(ws, n, FRAME_WG, FRAME_WG, 1, &t) || !out || (n > 0 && !x) || !frame_blocks_ok(n)) return -1;
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) return (int)hipMemsetAsync(out, 0, sizeof(double), st);
  if (t.levels > 0 && (!ws || ((uintptr_t)ws & 7))) return -1;
  hipLaunchKernelGGL(frame_sum_kernel<float>, dim3((unsigned)t.m[0]), dim3(FRAME_WG), 0, st, x, n, t.levels ? t.level[0] : out);
  for (int k = 0; k < t.levels; ++k)
    hipLaunchKernelGGL(frame_sum_kernel<double>, dim3((unsigned)t.m[k + 1]), dim3(FRAME_WG), 0, st, (const double*)t.level[k], t.m[k],
                       k + 1 < t.levels ? t.level[k + 1] : out);
  return (int)hipGetLastError();
}

size_t neat_frame_range_ws_bytes(void) { float* p; return partials_layout(nullptr, FRAME_RANGE_BLOCKS, 2, &p); }

int neat_frame_range(const float* x, long long n, void* ws, float* range, void* stream) {
  if (n < 0 || !range || !ws || ((uintptr_t)ws & 3) || (n > 0 && !x)) return -1;
  float* partial;
  partials_layout(ws, FRAME_RANGE_BLOCKS, 2, &partial);
  const int blocks = (int)std::max(1ll, std::min((long long)FRAME_RANGE_BLOCKS, (n + FRAME_WG - 1) / FRAME_WG));
  hipLaunchKernelGGL(frame_range_partial_kernel, dim3(blocks), dim3(FRAME_WG), 0, (hipStream_t)stream, x, n, partial);
  hipLaunchKernelGGL(frame_range_finish_kernel, dim3(1), dim3(FRAME_WG), 0, (hipStream_t)stream, (const float*)partial, blocks, range);
  return (int)hipGetLastError();
}

int neat_frame_grey(const float* x, long long n, const float* range, unsigned char* out, void* stream) {
  if (n < 0 || !range || (n > 0 && (!x || !out)) || !frame_blocks_ok(n)) return -1;
  if (n == 0) return 0;
  hipLaunchKernelGGL(frame_grey_kernel, frame_blocks(n), dim3(FRAME_WG), 0, (hipStream_t)stream, x, n, range, out);
  return (int)hipGetLastError();
}

int neat_frame_grid(const unsigned char* images, int N, int H, int W, int nrow, unsigned char* canvas, void* stream) {
  if (!images || !canvas || N < 1 || H < 1 || W < 1 || nrow < 1 || H > 32768 || W > 32768) return -1;
  const int xmaps = std::min(nrow, N), ymaps = (N + xmaps - 1) / xmaps, pad = N == 1 ? 0 : 2;
  const long long ch = (long long)ymaps * (H + pad) + pad, cw3 = 3 * ((long long)xmaps * (W + pad) + pad);
  if (cw3 > (long long)INT_MAX || ch > (long long)INT_MAX || !frame_blocks_ok(ch * cw3)) return -1;
  hipLaunchKernelGGL(frame_grid_kernel, frame_blocks(ch * cw3), dim3(FRAME_WG), 0, (hipStream_t)stream, images, N, H, W, xmaps, pad, ch * cw3, (int)cw3,
                     canvas);
  return (int)hipGetLastError();
}

// ---- added to ABI v15: sphere tracing of an SDF along rays (kernels_trace.hpp) ------------------------------------------------------------
static inline int trace_tiles(int R) { return (R + TRACE_WG - 1) / TRACE_WG; }

size_t neat_trace_ws_bytes(int R) { TraceWs w; return trace_layout(nullptr, R, TRACE_WG, &w); }

size_t neat_trace_list_offset(int R, int parity) {
  TraceWs w;
  if ((parity != 0 && parity != 1) || !trace_layout(nullptr, R, TRACE_WG, &w)) return 0;
  return ws_offset(nullptr, w.ids[parity]);
}

static inline bool trace_common(const float* origins, const float* dirs, int R, void* ws, TraceWs* w) {
  return origins && dirs && ws && !((uintptr_t)ws & 255) && trace_layout(ws, R, TRACE_WG, w);
}

int neat_trace_init(const float* origins, const float* dirs, const float* t_end, int R, double radius, double near, void* ws, float* points,
                    long long* ctl, void* stream) {
  TraceWs w;
  if (!trace_common(origins, dirs, R, ws, &w) || !points || !ctl || !(radius > 0.0) || !std::isfinite(radius) || !std::isfinite(near)) return -1;
  const int tiles = trace_tiles(R);
  hipLaunchKernelGGL(trace_init_kernel, dim3(tiles), dim3(TRACE_WG), 0, (hipStream_t)stream, w, origins, dirs, t_end, R, radius, near);
  hipLaunchKernelGGL(trace_scan_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, w.tile, tiles, ctl, 1);
  hipLaunchKernelGGL(trace_emit_kernel, dim3(tiles), dim3(TRACE_WG), 0, (hipStream_t)stream, w, (const int*)nullptr, w.ids[0], R, R, origins, dirs,
                     points);
  return (int)hipGetLastError();
}

int neat_trace_step(const float* origins, const float* dirs, const float* values, int n, int R, int parity, float eps, float relax,
                    int max_steps, int refine_steps, void* ws, float* points, long long* ctl, void* stream) {
  TraceWs w;
  if (!trace_common(origins, dirs, R, ws, &w) || !points || !ctl || n < 0 || n > R || (n > 0 && !values) || (parity != 0 && parity != 1)) return -1;
  if (!(eps > 0.f) || !(relax > 0.f) || !std::isfinite(eps) || !std::isfinite(relax) || max_steps < 0 || refine_steps < 0 || refine_steps > 64) return -1;
  const int tiles = std::max(trace_tiles(n), 1);
  hipLaunchKernelGGL(trace_advance_kernel, dim3(tiles), dim3(TRACE_WG), 0, (hipStream_t)stream, w, (const int*)w.ids[parity], values, n, R,
                     (const long long*)ctl, eps, relax, max_steps, refine_steps);
  hipLaunchKernelGGL(trace_scan_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, w.tile, tiles, ctl, 0);
  hipLaunchKernelGGL(trace_emit_kernel, dim3(tiles), dim3(TRACE_WG), 0, (hipStream_t)stream, w, (const int*)w.ids[parity], w.ids[parity ^ 1], n, R,
                     origins, dirs, points);
  return (int)hipGetLastError();
}

int neat_trace_finish(const float* origins, const float* dirs, int R, void* ws, float* depth, unsigned char* state, int* steps,
                      float* hit_points, void* stream) {
  TraceWs w;
  if (!trace_common(origins, dirs, R, ws, &w)) return -1;
  hipLaunchKernelGGL(trace_finish_kernel, dim3(trace_tiles(R)), dim3(TRACE_WG), 0, (hipStream_t)stream, w, origins, dirs, R, depth,
                     state, steps, hit_points);
  return (int)hipGetLastError();
}

int neat_trace_target_rays(const float* centres, int F, const float* rows, int stride, int N, int S, double radius, double near, double bias,
                           float* origins, float* dirs, float* t_end, unsigned char* ok, void* stream) {
  if (F < 0 || N < 0 || S < 1 || stride < (S > 1 ? 6 : 3) || !std::isfinite(radius) || !std::isfinite(near) || !std::isfinite(bias)) return -1;
  const long long total = (long long)F * N * S;
  if (total > (long long)INT_MAX) return -1;
  if (total == 0) return 0;
  if (!centres || !rows || !origins || !dirs || !t_end || !ok) return -1;
  hipLaunchKernelGGL(trace_target_rays_kernel, dim3((unsigned)((total + TRACE_WG - 1) / TRACE_WG)), dim3(TRACE_WG), 0, (hipStream_t)stream, centres, F,
                     rows, stride, N, S, radius, near, bias, origins, dirs, t_end, ok);
  return (int)hipGetLastError();
}

// ---- added to ABI v15: fuse, refine and snap of a parsed line soup (kernels_post.hpp) ----------------------------------------------------------
size_t neat_post_fuse_ws_bytes(int n, int V, int mtot) { PostFuseWs w; return post_fuse_layout(nullptr, n, V, mtot, &w) ? w.total : 0; }

int neat_post_fuse(const float* lines, int n, const float* det, int det_stride, const int* det_off, int mtot, const float* K3, const float* w2c,
                   int V, float dis_threshold, float keep_threshold, int by_label, float* score, int* count, unsigned char* keep, float* kept,
                   int* n_kept, void* ws, void* stream) {
  PostFuseWs w;
  if (!post_fuse_layout(ws, n, V, mtot, &w) || !n_kept || (by_label != 0 && by_label != 1)) return -1;
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) return (int)hipMemsetAsync(n_kept, 0, sizeof(int), st);
  if (!lines || !score || !count || !keep || !kept || !ws || (V > 0 && (!det_off || !K3 || !w2c)) || (mtot > 0 && (!det || det_stride < 5))) return -1;
  if (V > 0) {
    if (mtot > 0) NEAT_CHECK(hipMemsetAsync(w.present, 0, (size_t)mtot, st));
    hipLaunchKernelGGL(post_match_kernel, dim3((n + PARSE_WG - 1) / PARSE_WG, V), dim3(PARSE_WG), 0, st, lines, (const int*)nullptr, n, det,
                       det_stride, det_off, K3, w2c, 0, dis_threshold, 0, 0.f, 0.f, w.label, w.present);
    hipLaunchKernelGGL(post_rank_kernel, dim3(V), dim3(1024), 0, st, w.present, det_off, w.rank);
  }
  hipLaunchKernelGGL(post_fuse_score_kernel, grid1(n, PARSE_WG), dim3(PARSE_WG), 0, st, w.label, n, V, det, det_stride, det_off, w.rank, by_label,
                     keep_threshold, score, count, keep);
  hipLaunchKernelGGL(post_keep_kernel, dim3(1), dim3(1024), 0, st, lines, n, keep, w.idx, kept, n_kept);
  return (int)hipGetLastError();
}

int neat_post_select(const float* lines, int n, const unsigned char* keep, float* out, int* n_out, void* ws, void* stream) {
  if (n < 0 || n > INT_MAX / 6 || !n_out) return -1;
  if (n == 0) return (int)hipMemsetAsync(n_out, 0, sizeof(int), (hipStream_t)stream);
  if (!lines || !keep || !out || !ws) return -1;
  hipLaunchKernelGGL(post_keep_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, lines, n, keep, (int*)ws, out, n_out);
  return (int)hipGetLastError();
}

size_t neat_post_refine_ws_bytes(int ncap, int mmax) { PostRefineWs w; return post_refine_layout(nullptr, ncap, mmax, PARSE_TILE, &w) ? w.total : 0; }

int neat_post_refine_view(const float* cur, const int* n_cur, int ncap, const float* det, int det_stride, const int* det_off, int m, int mmax,
                          const float* K3, const float* w2c, int view, float dis_threshold, float width, float height, float* next, int* n_next,
                          void* ws, void* stream) {
  PostRefineWs w;
  if (m < 0 || m > mmax || view < 0 || !post_refine_layout(ws, ncap, mmax, PARSE_TILE, &w)) return -1;
  if (ncap == 0) return 0;
  if (!cur || !n_cur || !next || !n_next || !ws || !det_off || !K3 || !w2c || (m > 0 && (!det || det_stride < 4))) return -1;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(post_match_kernel, dim3((ncap + PARSE_WG - 1) / PARSE_WG, 1), dim3(PARSE_WG), 0, st, cur, n_cur, ncap, det, det_stride, det_off,
                     K3, w2c, view, dis_threshold, 1, width, height, w.label, (unsigned char*)nullptr);
  NEAT_CHECK(hipGetLastError());
  // the stable grouping by label and the means of the groups after reversal: parse_group's (its score output is not used; l3d = the lines)
  const int e = neat_parse_group(w.label, cur, cur, ncap, m, w.glines, w.gscores, w.gcount, w.group, stream);
  if (e != 0) return e;
  hipLaunchKernelGGL(post_refine_assemble_kernel, dim3(1), dim3(1024), 0, st, cur, n_cur, ncap, w.label, w.glines, w.gcount, w.idx, next,
                     n_next);
  return (int)hipGetLastError();
}

size_t neat_post_snap_ws_bytes(int n, int G) { PostSnapWs w; return post_snap_layout(nullptr, n, G, &w) ? w.total : 0; }

int neat_post_snap(const float* lines, int n, int G, float max_snap, int unique, float* junctions, int* pcount, int* edges, float* lines_out,
                   int* counts, void* ws, void* stream) {
  PostSnapWs w;
  if (n < 0 || !post_grid_ok(G) || !counts || (unique != 0 && unique != 1) || max_snap != max_snap) return -1;   // G > 1024: refused before any launch
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) return (int)hipMemsetAsync(counts, 0, 2 * sizeof(int), st);
  if (!post_snap_layout(ws, n, G, &w) || !lines || !junctions || !pcount || !edges || !lines_out || !ws) return -1;
  const int M = 2 * n;
  hipLaunchKernelGGL(post_snap_bbox_kernel, dim3(1), dim3(1024), 0, st, lines, M, G, w.box);
  hipLaunchKernelGGL(post_snap_key_kernel, grid1(M, PARSE_WG), dim3(PARSE_WG), 0, st, lines, M, G, (const float*)w.box, w.key);
  NEAT_CHECK(hipGetLastError());
  NEAT_PASS(sort_keys(w.sort, w.sort_bytes, w.key, w.skey, (size_t)M, 0u, 32u, st));
  hipLaunchKernelGGL(post_snap_cells_kernel, dim3(1), dim3(1024), 0, st, (const int*)w.skey, M, w.head, w.counts);
  hipLaunchKernelGGL(post_snap_peak_kernel, grid1(M, PARSE_WG), dim3(PARSE_WG), 0, st, (const int*)w.skey, (const int*)w.head, (const int*)w.counts, M, G,
                     w.flag, w.cnt);
  hipLaunchKernelGGL(post_snap_select_kernel, dim3(1), dim3(1024), 0, st, (const int*)w.skey, (const int*)w.head, (const int*)w.counts, M, G,
                     (const float*)w.box, (const int*)w.flag, (const int*)w.cnt, w.pidx, junctions, pcount, counts);
  hipLaunchKernelGGL(post_snap_nearest_kernel, grid1(M, PARSE_WG), dim3(PARSE_WG), 0, st, lines, M, (const float*)junctions, (const int*)counts,
                     w.near, w.dist2);
  if (!unique) {
    hipLaunchKernelGGL(post_snap_edges_kernel, dim3(1), dim3(1024), 0, st, (const int*)w.near, (const float*)w.dist2, n, max_snap,
                       (const float*)junctions, w.idx, edges, lines_out, counts + 1);
    return (int)hipGetLastError();
  }
  hipLaunchKernelGGL(post_snap_pairkey_kernel, grid1(n, PARSE_WG), dim3(PARSE_WG), 0, st, (const int*)w.near, (const float*)w.dist2, n, max_snap, w.pkey);
  NEAT_CHECK(hipGetLastError());
  NEAT_PASS(sort_keys(w.sort, w.sort_bytes, w.pkey, w.spkey, (size_t)n, 0u, 64u, st));
  hipLaunchKernelGGL(post_snap_unique_kernel, dim3(1), dim3(1024), 0, st, (const unsigned long long*)w.spkey, n, (const float*)junctions, w.idx, edges,
                     lines_out, counts + 1);
  return (int)hipGetLastError();
}

// ---- added to ABI v15: ray casting against a triangle mesh (kernels_raycast.hpp) ---------------------------------------------------------------
size_t neat_raycast_bvh_bytes(int nf) { RaycastWs w; return raycast_layout(nullptr, nullptr, nf, RC_WG, RC_TRI_STRIDE, &w) ? w.bvh_total : 0; }

size_t neat_raycast_ws_bytes(int nf) { RaycastWs w; return raycast_layout(nullptr, nullptr, nf, RC_WG, RC_TRI_STRIDE, &w) ? w.ws_total : 0; }

int neat_raycast_build(const double* verts, int nv, const int* faces, int nf, void* bvh, void* ws, void* stream) {
  RaycastWs w;
  if (nv < 0 || !bvh || ((uintptr_t)bvh & 255) || !raycast_layout(bvh, ws, nf, RC_WG, RC_TRI_STRIDE, &w)) return -1;
  if (nf > 0 && (!faces || !ws || ((uintptr_t)ws & 255) || (nv > 0 && !verts))) return -1;
  hipStream_t st = (hipStream_t)stream;
  NEAT_CHECK(hipMemsetAsync(w.status, 0, 256, st));
  if (nf > 0) {
    NEAT_PASS(sort_pairs(w.sort, w.sort_bytes, w.key, w.skey, w.val, w.sval, (size_t)nf, 0u, 64u, st, false));      // asked before anything is launched
    hipLaunchKernelGGL(raycast_prep_kernel, dim3(w.tiles), dim3(RC_WG), 0, st, verts, nv, faces, nf, w.status, w.partial);
    hipLaunchKernelGGL(raycast_scene_box_kernel, dim3(1), dim3(RC_WG), 0, st, (const double*)w.partial, w.tiles, w.box);
    hipLaunchKernelGGL(raycast_key_kernel, dim3(w.tiles), dim3(RC_WG), 0, st, verts, faces, nf, (const int*)w.status, (const double*)w.box, w.key, w.val);
    NEAT_CHECK(hipGetLastError());
    NEAT_PASS(sort_pairs(w.sort, w.sort_bytes, w.key, w.skey, w.val, w.sval, (size_t)nf, 0u, 64u, st));
  }
  hipLaunchKernelGGL(raycast_leaf_kernel, dim3(w.L / w.per), dim3(RC_WG), 0, st, verts, faces, nf, w.L, w.per, (const int*)w.status,
                       (const int*)(nf > 0 ? w.sval : nullptr),
                     w.nodes, w.tris);
  if (w.L > w.per) hipLaunchKernelGGL(raycast_top_kernel, dim3(1), dim3(RC_TOP_WG), 0, st, w.nodes, w.L / w.per);
  return (int)hipGetLastError();
}

int neat_raycast_cast(const void* bvh, int nf, const float* origins, const float* dirs, const float* t_min, const float* t_max, int R, int any_hit,
                      float* t, int* tri, float* uv, unsigned* counts, void* stream) {
  RaycastWs w;
  if (!bvh || ((uintptr_t)bvh & 255) || !raycast_layout(const_cast<void*>(bvh), nullptr, nf, RC_WG, RC_TRI_STRIDE, &w) || R < 0 || R > INT_MAX / 4 ||
      (any_hit != 0 && any_hit != 1)) return -1;
  if (R == 0) return 0;
  if (!origins || !dirs || !t || !tri || !uv) return -1;
  if (any_hit)
    hipLaunchKernelGGL(raycast_cast_kernel<true>, grid1(R, RC_WG), dim3(RC_WG), 0, (hipStream_t)stream, (const float*)w.nodes, (const double*)w.tris,
                         nf, w.L, origins, dirs, t_min, t_max,
                       R, t, tri, uv, counts);
  else
    hipLaunchKernelGGL(raycast_cast_kernel<false>, grid1(R, RC_WG), dim3(RC_WG), 0, (hipStream_t)stream, (const float*)w.nodes,
                         (const double*)w.tris, nf, w.L, origins, dirs, t_min, t_max,
                       R, t, tri, uv, counts);
  return (int)hipGetLastError();
}

// ---- added to ABI v15: the closest point on the mesh of a tree (kernels_closest.hpp) ------------------------------------------------------------
int neat_raycast_closest(const void* bvh, int nf, const double* points, int N, double max_d2, double* d2, int* tri, double* point, double* uv,
                         unsigned* counts, void* stream) {
  RaycastWs w;
  if (!bvh || ((uintptr_t)bvh & 255) || !raycast_layout(const_cast<void*>(bvh), nullptr, nf, RC_WG, RC_TRI_STRIDE, &w) || N < 0 || N > INT_MAX / 4 ||
      !(max_d2 >= 0.0)) return -1;                                        // a NaN bound too
  if (N == 0) return 0;
  if (!points || !d2 || !tri || !point || !uv) return -1;
  hipLaunchKernelGGL(raycast_closest_kernel, grid1(N, RC_WG), dim3(RC_WG), 0, (hipStream_t)stream, (const float*)w.nodes, (const double*)w.tris, nf,
                     w.L, points, N, max_d2, d2, tri, point, uv, counts);
  return (int)hipGetLastError();
}

// ---- added to ABI v15: 2-D line-segment detection in the views (kernels_detect.hpp) ------------------------------------------------------------
static int detect_label_launch(const unsigned char* code, long long maps, int h, int w, int* label, int* size, int* votes, int* xmin, int* xmax,
                               int* ymax, hipStream_t st) {
  const long long tiles = (long long)((h + DET_TILE - 1) / DET_TILE) * ((w + DET_TILE - 1) / DET_TILE), el = maps * h * w;
  const dim3 per_element((unsigned)((el + DET_WG - 1) / DET_WG));
  hipLaunchKernelGGL(detect_label_tile_kernel, dim3((unsigned)(maps * tiles)), dim3(DET_WG), 0, st, code, h, w, label, size, votes, xmin, xmax, ymax);
  hipLaunchKernelGGL(detect_label_merge_kernel, per_element, dim3(DET_WG), 0, st, code, (int)maps, h, w, label);
  hipLaunchKernelGGL(detect_label_flatten_kernel, per_element, dim3(DET_WG), 0, st, (int)maps, h, w, label, size, xmin, xmax, ymax);
  return (int)hipGetLastError();
}

int neat_detect_label(const unsigned char* codes, int V, int h, int w, int* labels, void* stream) {
  if (!detect_maps_ok(V, h, w, DET_TILE)) return -1;
  if ((long long)V * h * w == 0) return 0;
  if (!codes || !labels) return -1;
  return detect_label_launch(codes, V, h, w, labels, nullptr, nullptr, nullptr, nullptr, nullptr, (hipStream_t)stream);
}

size_t neat_detect_scratch_bytes(int V, int H, int W, double scale, int min_reg) {
  DetectWs d;
  return detect_layout(nullptr, V, H, W, scale, min_reg, DET_TILE, DET_WG, &d) ? d.total : 0;
}

int neat_detect_lines(const unsigned char* images, int V, int H, int W, int channels, double scale, const double* taps_x, const double* taps_y,
                      int ntaps, double rho2, double c1, double cos_tau, double density, double logNT, double p, int min_reg, void* ws, int cap,
                      double* lines, double* width, double* nfa, int* n, int* k, int* offsets, void* stream) {
  DetectWs d;
  if ((channels != 1 && channels != 3) || !offsets || ntaps < 0 || (ntaps > 0 && ntaps % 2 == 0) || !(rho2 > 0.0) || !(c1 > 0.0) ||
      !(p > 0.0 && p < 1.0) || !std::isfinite(cos_tau) || !std::isfinite(density) || !std::isfinite(logNT) ||
      !detect_layout(ws, V, H, W, scale, min_reg, DET_TILE, DET_WG, &d))
    return -1;
  hipStream_t st = (hipStream_t)stream;
  if (d.el == 0) return (int)hipMemsetAsync(offsets, 0, ((size_t)V + 1) * sizeof(int), st);
  if (!images || !ws || ((uintptr_t)ws & 255) || cap < d.cap || !lines || !width || !nfa || !n || !k) return -1;
  if ((scale < 1.0) != (ntaps > 0) || (ntaps > 0 && (!taps_x || !taps_y))) return -1;
  const DetectConsts K = {cos_tau, density, logNT, p};
  const int hw = d.h * d.w;
  const dim3 per_pixel((unsigned)((d.px + DET_WG - 1) / DET_WG)), per_pos((unsigned)((d.el + DET_WG - 1) / DET_WG)), per_element((unsigned)d.blocks);
  hipLaunchKernelGGL(detect_grey_kernel, per_pixel, dim3(DET_WG), 0, st, images, V, H, W, channels, scale, taps_x, taps_y, ntaps, d.Hs, d.Ws, d.grey);
  hipLaunchKernelGGL(detect_gradient_kernel, per_pos, dim3(DET_WG), 0, st, (const double*)d.grey, V, d.Hs, d.Ws, rho2, c1, d.gx, d.gy, d.code);
  NEAT_CHECK(hipGetLastError());
  const int e = detect_label_launch(d.code, 2ll * V, d.h, d.w, d.label, d.size, d.votes, d.xmin, d.xmax, d.ymax, st);
  if (e != 0) return e;
  hipLaunchKernelGGL(detect_vote_kernel, per_pos, dim3(DET_WG), 0, st, V, hw, (const int*)d.label, (const int*)d.size, d.votes);
  hipLaunchKernelGGL(detect_cand_count_kernel, per_element, dim3(DET_WG), 0, st, 2 * d.el, hw, min_reg, (const int*)d.label, (const int*)d.size,
                     (const int*)d.votes, d.bcnt);
  hipLaunchKernelGGL(detect_cand_scan_kernel, dim3(1), dim3(1024), 0, st, d.blocks, (const int*)d.bcnt, d.boff, d.cap, d.counters);
  hipLaunchKernelGGL(detect_cand_emit_kernel, per_element, dim3(DET_WG), 0, st, 2 * d.el, hw, min_reg, (const int*)d.label, (const int*)d.size,
                     (const int*)d.votes, (const int*)d.boff, d.cap, d.cand);
  NEAT_CHECK(hipGetLastError());
  hipLaunchKernelGGL(detect_region_kernel, dim3((unsigned)((d.cap + DET_WAVES - 1) / DET_WAVES)), dim3(DET_WG), 0, st, (const int*)d.cand,
                     (const int*)d.counters, d.h, d.w, scale, K, (const unsigned char*)d.code, (const int*)d.label, (const int*)d.xmin,
                     (const int*)d.xmax, (const int*)d.ymax, (const double*)d.gx, (const double*)d.gy, d.rec, d.n, d.k, d.keep);
  hipLaunchKernelGGL(detect_output_kernel, dim3(1), dim3(1024), 0, st, (const int*)d.cand, d.counters, d.cap, V, hw, (const double*)d.rec,
                     (const int*)d.n, (const int*)d.k, (const int*)d.keep, d.idx, lines, width, nfa, n, k, offsets);
  return (int)hipGetLastError();
}

// ---- added to ABI v15: 3-D segments triangulated from the views' 2-D segments (kernels_triangulate.hpp) ---------------------------------------
size_t neat_tri_scratch_bytes(int V, int S, int M, int nmax) {
  TriWs w;
  return tri_layout(nullptr, V, S, M, nmax, TRI_WG, &w) ? w.total : 0;
}

static bool tri_thresholds_ok(double cos_min, double overlap_min) { return std::isfinite(cos_min) && std::isfinite(overlap_min); }

int neat_tri_count(const double* segments, const int* segoff, int V, int S, int nmax, const int* nb, int M, const double* cam, double cos_min,
                   double overlap_min, void* ws, int* view, int* hoff, long long* total, void* stream) {
  TriWs w;
  if (!tri_thresholds_ok(cos_min, overlap_min) || !tri_layout(ws, V, S, M, nmax, TRI_WG, &w) || !hoff || !total) return -1;
  hipStream_t st = (hipStream_t)stream;
  if (S > 0 && (!segments || !segoff || !cam || !ws || ((uintptr_t)ws & 255) || !view || (M > 0 && !nb))) return -1;
  if (S > 0) hipLaunchKernelGGL(tri_segment_kernel, grid1(S, TRI_WG), dim3(TRI_WG), 0, st, segments, segoff, V, S, cam, w.sega, w.segb, view);
  if (S == 0 || M == 0 || w.tiles == 0) {
    NEAT_CHECK(hipMemsetAsync(hoff, 0, ((size_t)S + 1) * sizeof(int), st));
    NEAT_CHECK(hipMemsetAsync(total, 0, sizeof(long long), st));
    return (int)hipGetLastError();
  }
  hipLaunchKernelGGL(tri_match_kernel<false>, dim3((unsigned)((long long)V * M * w.tiles)), dim3(TRI_WG), 0, st, segoff, nb, M, w.tiles, cam,
                     (const double*)w.sega, (const double*)w.segb, cos_min, overlap_min, w.cnt, (const int*)nullptr, 0, (int*)nullptr,
                     (int*)nullptr, (double*)nullptr);
  hipLaunchKernelGGL(tri_scan_kernel, dim3(1), dim3(1024), 0, st, S, M, (const int*)w.cnt, w.off, hoff, total);
  return (int)hipGetLastError();
}

int neat_tri_fill(const int* segoff, int V, int S, int nmax, const int* nb, int M, const double* cam, double cos_min, double overlap_min,
                  void* ws, long long H, int* hyp_m, int* hyp_j, double* hyp_s, void* stream) {
  TriWs w;
  if (!tri_thresholds_ok(cos_min, overlap_min) || !tri_layout(ws, V, S, M, nmax, TRI_WG, &w) || H < 0 || H > 0x7fffffffLL / 2) return -1;
  if (H == 0) return 0;
  if (S == 0 || M == 0 || !segoff || !nb || !cam || !ws || ((uintptr_t)ws & 255) || !hyp_m || !hyp_j || !hyp_s) return -1;
  hipLaunchKernelGGL(tri_match_kernel<true>, dim3((unsigned)((long long)V * M * w.tiles)), dim3(TRI_WG), 0, (hipStream_t)stream, segoff, nb, M,
                     w.tiles, cam, (const double*)w.sega, (const double*)w.segb, cos_min, overlap_min, (int*)nullptr, (const int*)w.off, (int)H,
                     hyp_m, hyp_j, hyp_s);
  return (int)hipGetLastError();
}

int neat_tri_lines(const int* segoff, int V, int S, int nmax, const int* nb, int M, const double* cam, void* ws, const int* view, const int* hoff,
                   long long H, const int* hyp_m, const int* hyp_j, const double* hyp_s, double sigma_px, double min_score, int min_views,
                   double* estimate, double* score, int* kept, int* label, int* members, double* lines3d, int* views, double* support,
                   int* n_lines, void* stream) {
  TriWs w;
  if (!(sigma_px > 0.0) || !std::isfinite(sigma_px) || !std::isfinite(min_score) || min_views < 0 || !n_lines || H < 0 ||
      H > 0x7fffffffLL / 2 || !tri_layout(ws, V, S, M, nmax, TRI_WG, &w))
    return -1;
  hipStream_t st = (hipStream_t)stream;
  if (S == 0) return (int)hipMemsetAsync(n_lines, 0, sizeof(int), st);
  if (!segoff || !cam || !ws || ((uintptr_t)ws & 255) || !view || !hoff || !estimate || !score || !kept || !label || !members || !lines3d ||
      !views || !support || (H > 0 && (!nb || !hyp_m || !hyp_j || !hyp_s)))
    return -1;
  const dim3 per_seg(grid1(S, TRI_WG)), per_wave(grid1(S, TRI_WAVES));
  hipLaunchKernelGGL(tri_score_kernel, per_wave, dim3(TRI_WG), 0, st, S, view, hoff, hyp_m, hyp_s, cam, (const double*)w.sega, sigma_px,
                     min_score, w.best, estimate, score, w.radius, kept);
  hipLaunchKernelGGL(tri_link_init_kernel, per_seg, dim3(TRI_WG), 0, st, S, (const int*)kept, label, w.last);
  NEAT_CHECK(hipGetLastError());
  if (H > 0)
    hipLaunchKernelGGL(tri_link_kernel, per_wave, dim3(TRI_WG), 0, st, S, M, view, segoff, nb, hoff, hyp_m, hyp_j, (const int*)kept,
                       (const double*)estimate, (const double*)w.radius, label);
  hipLaunchKernelGGL(uf_flatten_kernel, grid1(S, UF_WG), dim3(UF_WG), 0, st, S, label, w.last);
  hipLaunchKernelGGL(tri_component_kernel, per_wave, dim3(TRI_WG), 0, st, S, (const int*)label, (const int*)w.last, view, (const double*)score,
                     (const double*)estimate, w.nviews, w.axis, w.tau);
  hipLaunchKernelGGL(tri_output_kernel, dim3(1), dim3(1024), 0, st, S, min_views, (const int*)label, (const int*)w.nviews, (const int*)w.axis,
                     (const double*)w.tau, (const double*)estimate, (const double*)score, w.idx, members, lines3d, views, support, n_lines);
  return (int)hipGetLastError();
}

// ---- added to ABI v15: a training scene from a mesh and its wireframe (kernels_scenegen.hpp) -------------------------------------------------
size_t neat_scenegen_scratch_bytes(int V, int E) {
  ScenegenWs w;
  return scenegen_layout(nullptr, V, E, &w) ? w.total : 0;
}

int neat_scenegen_shade(const void* bvh, int nf, const double* K, const double* pose, int V, int H, int W, int ss, double albedo, double ambient,
                        double background, unsigned char* rgb, unsigned char* mask, void* stream) {
  RaycastWs t;
  if (!bvh || ((uintptr_t)bvh & 255) || !raycast_layout(const_cast<void*>(bvh), nullptr, nf, RC_WG, RC_TRI_STRIDE, &t) || ss < 1 || ss > SG_MAX_SS ||
      !scenegen_picture_ok(V, H, W) || !std::isfinite(albedo) || !std::isfinite(ambient) || !std::isfinite(background))
    return -1;
  if (V == 0) return 0;
  if (!K || !pose || !rgb || !mask) return -1;
  const SgShade sh = {albedo, ambient, background};
  hipLaunchKernelGGL(scenegen_shade_kernel, dim3((unsigned)((long long)V * ((H + 15) / 16) * ((W + 15) / 16))), dim3(SG_WG), 0, (hipStream_t)stream,
                     (const float*)t.nodes, (const double*)t.tris, nf, t.L, K, pose, H, W, ss, sh, rgb, mask);
  return (int)hipGetLastError();
}

// every argument of the edge pass that a launch turns into a loop bound or an index; the 2-D segment of an edge is cut to the picture, so
// no edge needs more samples than the picture's diagonal does
static bool scenegen_edge_args_ok(const void* bvh, int nf, int V, int E, int H, int W, double step, double min_len, double bias, double near,
                                  RaycastWs* t) {
  if (!bvh || ((uintptr_t)bvh & 255) || !raycast_layout(const_cast<void*>(bvh), nullptr, nf, RC_WG, RC_TRI_STRIDE, t)) return false;
  if (!scenegen_picture_ok(V, H, W) || !scenegen_counts_ok(V, E)) return false;
  if (!(step > 0.0) || !std::isfinite(step) || !std::isfinite(min_len) || !(bias >= 0.0) || !std::isfinite(bias) || !(near > 0.0) || !std::isfinite(near))
    return false;
  return std::ceil(std::sqrt((double)W * W + (double)H * H) / step) + 2.0 <= (double)SG_MAX_SAMPLES;
}

int neat_scenegen_edge_count(const void* bvh, int nf, const double* junctions, int J, const int* edges, int E, const double* K, const double* pose,
                             int V, int H, int W, double step, double min_len, double bias, double near, void* ws, long long* total, void* stream) {
  RaycastWs t;
  ScenegenWs w;
  if (!scenegen_edge_args_ok(bvh, nf, V, E, H, W, step, min_len, bias, near, &t) || J < 0 || !total || !scenegen_layout(ws, V, E, &w)) return -1;
  if (E > 0 && !edges) return -1;
  for (long long i = 0; i < 2ll * E; ++i)
    if (edges[i] < 0 || edges[i] >= J) return -1;                      // `edges` is the host's list
  hipStream_t st = (hipStream_t)stream;
  NEAT_CHECK(hipMemsetAsync(total, 0, sizeof(long long), st));
  if ((long long)V * E == 0) return 0;
  if (!junctions || !K || !pose || !ws || ((uintptr_t)ws & 255)) return -1;
  NEAT_CHECK(hipMemcpyAsync(w.edges, edges, 2 * (size_t)E * sizeof(int), hipMemcpyHostToDevice, st));
  NEAT_CHECK(hipStreamSynchronize(st));                                 // the host's list may go away when this call returns
  const int pairs = V * E;
  hipLaunchKernelGGL(scenegen_edge_kernel<false>, grid1(pairs, SG_WAVES), dim3(SG_WG), 0, st, (const float*)t.nodes, (const double*)t.tris, nf, t.L,
                     junctions, (const int*)w.edges, E, K, pose, V, H, W, step, min_len, bias, near, w.cnt, (const int*)nullptr, 0, (int*)nullptr,
                     (double*)nullptr, (double*)nullptr, (unsigned char*)nullptr);
  hipLaunchKernelGGL(count_scan_kernel<int>, dim3(1), dim3(1024), 0, st, pairs, (const int*)w.cnt, w.off, total);
  return (int)hipGetLastError();
}

int neat_scenegen_edge_fill(const void* bvh, int nf, const double* junctions, int J, int E, const double* K, const double* pose, int V, int H, int W,
                            double step, double min_len, double bias, double near, void* ws, long long N, int* idx, double* p2, double* p3,
                            unsigned char* junc, void* stream) {
  RaycastWs t;
  ScenegenWs w;
  if (!scenegen_edge_args_ok(bvh, nf, V, E, H, W, step, min_len, bias, near, &t) || J < 0 || N < 0 || N > 0x7fffffffLL / 8 ||
      !scenegen_layout(ws, V, E, &w))
    return -1;
  if (N == 0) return 0;
  if ((long long)V * E == 0 || !junctions || !K || !pose || !ws || ((uintptr_t)ws & 255) || !idx || !p2 || !p3 || !junc) return -1;
  hipLaunchKernelGGL(scenegen_edge_kernel<true>, grid1(V * E, SG_WAVES), dim3(SG_WG), 0, (hipStream_t)stream, (const float*)t.nodes,
                     (const double*)t.tris, nf, t.L, junctions, (const int*)w.edges, E, K, pose, V, H, W, step, min_len, bias, near, (int*)nullptr,
                     (const int*)w.off, (int)N, idx, p2, p3, junc);
  return (int)hipGetLastError();
}

}  // extern "C"

// ---- added to ABI v15: the crease lines of a triangle mesh (kernels_crease.hpp) -----------------------------------------------------------
namespace {

// the counts that an earlier call left in the workspace are the ones the host passes back
int crease_state_is(const CreaseWs& w, int first, int n, const int* want, hipStream_t st) {
  int got[3] = {0, 0, 0};
  NEAT_CHECK(hipMemcpyAsync(got, w.state + first, n * sizeof(int), hipMemcpyDeviceToHost, st));
  NEAT_CHECK(hipStreamSynchronize(st));
  for (int i = 0; i < n; ++i)
    if (got[i] != want[i]) return -1;
  return 0;
}

constexpr int CR_ST_HALVES = 2, CR_ST_CHAINS = 3, CR_ST_EDGES = 4, CR_ST_LINES = 5, CR_ST_JUNCTIONS = 6;

}  // namespace

extern "C" {

size_t neat_crease_scratch_bytes(int nv, int nf) {
  CreaseWs w;
  return crease_layout(nullptr, nv, nf, SCAN_WG, &w) ? w.total : 0;
}

int neat_crease_edges(const double* verts, int nv, const int* faces, int nf, double cos_angle, int boundary, void* ws, int* counts, void* stream) {
  CreaseWs w;
  if (!crease_layout(ws, nv, nf, SCAN_WG, &w) || !ws || ((uintptr_t)ws & 255) || !counts || !(cos_angle > -1.0 && cos_angle < 1.0) ||
      (boundary != 0 && boundary != 1) || (nv > 0 && !verts) || (nf > 0 && !faces))
    return -1;
  hipStream_t st = (hipStream_t)stream;
  NEAT_CHECK(hipMemsetAsync(counts, 0, 8 * sizeof(int), st));
  NEAT_CHECK(hipMemsetAsync(w.state, 0, 64 * sizeof(int), st));
  const long long words = 3ll * std::max(nv, nf);
  if (words > 0) {
    hipLaunchKernelGGL(crease_check_kernel, dim3((unsigned)((words + CR_WG - 1) / CR_WG)), dim3(CR_WG), 0, st, verts, nv, faces, nf, w.state);
    NEAT_CHECK(hipGetLastError());
  }
  int status[2] = {0, 0};
  NEAT_CHECK(hipMemcpyAsync(status, w.state, sizeof(status), hipMemcpyDeviceToHost, st));
  NEAT_CHECK(hipStreamSynchronize(st));                                 // nothing below reads a vertex through an index that was not checked
  if (status[0] || status[1]) {
    const int s = status[0] ? 1 : 2;
    NEAT_CHECK(hipMemcpyAsync(counts, &s, sizeof(int), hipMemcpyHostToDevice, st));
    return (int)hipStreamSynchronize(st);
  }
  if (nv > 0) {
    for (int axis = 2; axis >= 0; --axis) {
      hipLaunchKernelGGL(crease_vkey_kernel, grid1(nv, CR_WG), dim3(CR_WG), 0, st, verts, nv, axis, (const int*)(axis == 2 ? nullptr : w.vb), w.ka, w.va);
      NEAT_CHECK(hipGetLastError());
      NEAT_PASS(sort_pairs(w.sort, w.sort_bytes, w.ka, w.kb, w.va, w.vb, (size_t)nv, 0u, 64u, st));
    }
    hipLaunchKernelGGL(crease_vhead_kernel, grid1(nv, CR_WG), dim3(CR_WG), 0, st, verts, nv, (const int*)w.vb, w.vhead);
    tiled_scan(nv, IsNonzero{w.vhead}, w.tile, w.vslot, counts + 1, st);
    hipLaunchKernelGGL(crease_vrep_kernel, grid1(nv, CR_WG), dim3(CR_WG), 0, st, nv, (const int*)w.vb, (const int*)w.vhead, (const int*)w.vslot, w.rep);
    hipLaunchKernelGGL(crease_weld_kernel, grid1(nv, CR_WG), dim3(CR_WG), 0, st, nv, (const int*)w.vb, (const int*)w.vhead, (const int*)w.vslot,
                       (const int*)w.rep, w.weld);
  }
  if (nf > 0) {
    hipLaunchKernelGGL(crease_face_kernel, grid1(nf, CR_WG), dim3(CR_WG), 0, st, verts, faces, nf, (const int*)w.weld, w.fn, w.ka, w.va);
    NEAT_CHECK(hipGetLastError());
    NEAT_PASS(sort_pairs(w.sort, w.sort_bytes, w.ka, w.kb, w.va, w.vb, (size_t)w.M, 0u, 64u, st));
    hipLaunchKernelGGL(crease_kind_kernel, grid1(w.M, CR_WG), dim3(CR_WG), 0, st, (const unsigned long long*)w.kb, (const int*)w.vb, w.M, faces,
                       (const int*)w.weld, (const double*)w.fn, cos_angle, boundary, w.mark, w.state + CR_ST_HALVES);
    tiled_scan(w.M, IsNonzero{w.mark}, w.tile, w.slot, counts + 3, st);
    for (int kind = 0; kind < 3; ++kind) tiled_scan(w.M, IsEqual{w.mark, kind + 1}, w.tile, nullptr, counts + 4 + kind, st);
    hipLaunchKernelGGL(crease_edge_kernel, grid1(w.M, CR_WG), dim3(CR_WG), 0, st, (const unsigned long long*)w.kb, w.M, (const int*)w.mark,
                       (const int*)w.slot, w.elo, w.ehi, w.ekind);
  }
  hipLaunchKernelGGL(crease_edges_counts_kernel, dim3(1), dim3(1), 0, st, nf, (const int*)(w.state + CR_ST_HALVES), counts);
  NEAT_CHECK(hipGetLastError());
  return (int)hipMemcpyAsync(w.state + CR_ST_EDGES, counts + 3, sizeof(int), hipMemcpyDeviceToDevice, st);
}

int neat_crease_chains(const double* verts, int nv, int nf, int E, double sin2_turn, double dev, void* ws, int* counts, void* stream) {
  CreaseWs w;
  if (!crease_layout(ws, nv, nf, SCAN_WG, &w) || !ws || ((uintptr_t)ws & 255) || !counts || E < 0 || E > w.M || !(sin2_turn >= 0.0 && sin2_turn <= 1.0) ||
      !(dev >= 0.0) || !std::isfinite(dev) || (E > 0 && !verts))
    return -1;
  hipStream_t st = (hipStream_t)stream;
  NEAT_PASS(crease_state_is(w, CR_ST_EDGES, 1, &E, st));
  NEAT_CHECK(hipMemsetAsync(counts, 0, 4 * sizeof(int), st));
  NEAT_CHECK(hipMemsetAsync(w.state + CR_ST_LINES, 0, 2 * sizeof(int), st));
  if (E == 0) return 0;
  NEAT_CHECK(hipMemsetAsync(w.vstate, 0, (size_t)nv * sizeof(int), st));
  NEAT_CHECK(hipMemsetAsync(w.jflag, 0, (size_t)nv * sizeof(int), st));
  hipLaunchKernelGGL(crease_incidence_kernel, grid1(E, CR_WG), dim3(CR_WG), 0, st, E, (const int*)w.elo, (const int*)w.ehi, w.ka, w.parent);
  NEAT_CHECK(hipGetLastError());
  NEAT_PASS(sort_keys(w.sort, w.sort_bytes, w.ka, w.kb, 2 * (size_t)E, 0u, 64u, st));
  hipLaunchKernelGGL(crease_vertex_kernel, grid1(2 * E, CR_WG), dim3(CR_WG), 0, st, (const unsigned long long*)w.kb, 2 * E, verts, (const int*)w.elo,
                     (const int*)w.ehi, (const int*)w.ekind, sin2_turn, w.vstate, w.parent);
  hipLaunchKernelGGL(crease_label_kernel, grid1(E, CR_WG), dim3(CR_WG), 0, st, E, w.parent, w.ka);
  NEAT_CHECK(hipGetLastError());
  NEAT_PASS(sort_keys(w.sort, w.sort_bytes, w.ka, w.ckey, (size_t)E, 0u, 64u, st));
  hipLaunchKernelGGL(crease_chain_head_kernel, grid1(E, CR_WG), dim3(CR_WG), 0, st, (const unsigned long long*)w.ckey, E, w.mark);
  tiled_scan(E, IsNonzero{w.mark}, w.tile, w.slot, w.state + CR_ST_CHAINS, st);
  hipLaunchKernelGGL(crease_chain_start_kernel, grid1(E, CR_WG), dim3(CR_WG), 0, st, E, (const int*)w.mark, (const int*)w.slot, w.cstart);
  hipLaunchKernelGGL(crease_chain_kernel<false>, grid1(E, CR_WAVES), dim3(CR_WG), 0, st, (const unsigned long long*)w.ckey, E,
                     (const int*)(w.state + CR_ST_CHAINS), (const int*)w.cstart, verts, (const int*)w.elo, (const int*)w.ehi, (const int*)w.ekind,
                     (const int*)w.vstate, dev, w.cinfo, w.cnl, w.jflag, (const int*)nullptr, 0, (unsigned long long*)nullptr, (int*)nullptr);
  tiled_scan(E, Value{w.cnl}, w.tile, w.coff, counts + 1, st);
  tiled_scan(nv, IsNonzero{w.jflag}, w.tile, w.jmap, counts + 2, st);
  NEAT_CHECK(hipGetLastError());
  NEAT_CHECK(hipMemcpyAsync(counts, w.state + CR_ST_CHAINS, sizeof(int), hipMemcpyDeviceToDevice, st));
  return (int)hipMemcpyAsync(w.state + CR_ST_LINES, counts + 1, 2 * sizeof(int), hipMemcpyDeviceToDevice, st);
}

int neat_crease_fill(const double* verts, int nv, int nf, int E, void* ws, int n_lines, int n_junc, double* junctions, int* vertex, int* lines,
                     unsigned char* kind, unsigned char* curved, void* stream) {
  CreaseWs w;
  if (!crease_layout(ws, nv, nf, SCAN_WG, &w) || !ws || ((uintptr_t)ws & 255) || E < 0 || E > w.M || n_lines < 0 || n_lines > E || n_junc < 0 ||
      n_junc > nv || (long long)n_junc > 2ll * n_lines || (n_lines > 0 && n_junc < 2))
    return -1;
  if (n_lines == 0) return 0;
  if (!verts || !junctions || !vertex || !lines || !kind || !curved) return -1;
  hipStream_t st = (hipStream_t)stream;
  const int want[3] = {E, n_lines, n_junc};
  NEAT_PASS(crease_state_is(w, CR_ST_EDGES, 3, want, st));
  hipLaunchKernelGGL(crease_chain_kernel<true>, grid1(E, CR_WAVES), dim3(CR_WG), 0, st, (const unsigned long long*)w.ckey, E,
                     (const int*)(w.state + CR_ST_CHAINS), (const int*)w.cstart, verts, (const int*)w.elo, (const int*)w.ehi, (const int*)w.ekind,
                     (const int*)w.vstate, 0.0, w.cinfo, (int*)nullptr, (int*)nullptr, (const int*)w.coff, n_lines, w.lab, w.ltag);
  hipLaunchKernelGGL(crease_tagkey_kernel, grid1(n_lines, CR_WG), dim3(CR_WG), 0, st, n_lines, (const int*)w.ltag, w.ka, w.va);
  NEAT_CHECK(hipGetLastError());
  NEAT_PASS(sort_pairs(w.sort, w.sort_bytes, w.ka, w.kb, w.va, w.vb, (size_t)n_lines, 0u, 3u, st));
  hipLaunchKernelGGL(crease_abkey_kernel, grid1(n_lines, CR_WG), dim3(CR_WG), 0, st, n_lines, (const int*)w.vb, (const unsigned long long*)w.lab, w.ka);
  NEAT_CHECK(hipGetLastError());
  NEAT_PASS(sort_pairs(w.sort, w.sort_bytes, w.ka, w.kb, w.vb, w.va, (size_t)n_lines, 0u, 64u, st));
  hipLaunchKernelGGL(crease_lines_kernel, grid1(n_lines, CR_WG), dim3(CR_WG), 0, st, n_lines, (const unsigned long long*)w.kb, (const int*)w.va,
                     (const int*)w.ltag, (const int*)w.jmap, lines, kind, curved);
  hipLaunchKernelGGL(crease_junction_kernel, grid1(nv, CR_WG), dim3(CR_WG), 0, st, verts, nv, (const int*)w.jflag, (const int*)w.jmap, n_junc, junctions,
                     vertex);
  return (int)hipGetLastError();
}

// ---- added to ABI v15: 2-D wireframes with shared junctions from the views' segments (kernels_wireframe2d.hpp) -------------------------------
size_t neat_wf2d_scratch_bytes(int V, int S, int nmax) {
  Wf2dWs w;
  return wf2d_layout(nullptr, V, S, nmax, WF_WG, &w) ? w.total : 0;
}

int neat_wf2d_build(const double* segments, const int* segoff, const double* weight, int V, int S, int nmax, double gap, double frac, double sin_min,
                    int t_junctions, void* ws, double* vertices, int* degree, int* kind, double* score, double* spread, int* t_edge, int* voff,
                    int* ends, int* edges, double* eweight, int* esrc, int* eoff, void* stream) {
  Wf2dWs w;
  if (!(gap > 0.0) || !std::isfinite(gap) || !(frac > 0.0 && frac < 0.5) || !(sin_min > 0.0 && sin_min <= 1.0) || !voff || !eoff ||
      !wf2d_layout(ws, V, S, nmax, WF_WG, &w))
    return -1;
  hipStream_t st = (hipStream_t)stream;
  if (S == 0) {
    NEAT_CHECK(hipMemsetAsync(voff, 0, ((size_t)V + 1) * sizeof(int), st));
    return (int)hipMemsetAsync(eoff, 0, ((size_t)V + 1) * sizeof(int), st);
  }
  if (!segments || !segoff || !weight || !ws || ((uintptr_t)ws & 255) || !vertices || !degree || !kind || !score || !spread || !t_edge || !ends ||
      !edges || !eweight || !esrc)
    return -1;
  const dim3 per_seg(grid1(S, WF_WG)), per_wave(grid1(2 * S, WF_WAVES)), pairs((unsigned)((long long)V * w.tiles));
  hipLaunchKernelGGL(wf_segment_kernel, per_seg, dim3(WF_WG), 0, st, segments, segoff, V, S, gap, frac, w.rec, w.view, w.parent, w.last);
  hipLaunchKernelGGL(wf_meet_kernel, pairs, dim3(WF_WG), 0, st, segoff, S, w.tiles, (const double*)w.rec, sin_min, w.parent);
  hipLaunchKernelGGL(uf_flatten_kernel, grid1(2 * S, UF_WG), dim3(UF_WG), 0, st, 2 * S, w.parent, w.last);
  NEAT_CHECK(hipGetLastError());
  hipLaunchKernelGGL(wf_vertex_scan_kernel, dim3(1), dim3(1024), 0, st, S, V, segoff, (const int*)w.parent, w.vidx, voff);
  hipLaunchKernelGGL(wf_junction_kernel, per_wave, dim3(WF_WG), 0, st, 2 * S, (const int*)w.parent, (const int*)w.last, (const int*)w.vidx,
                     (const double*)w.rec, weight, vertices, degree, kind, score, spread, t_edge);
  hipLaunchKernelGGL(wf_tee_kernel, pairs, dim3(WF_WG), 0, st, segoff, S, w.tiles, (const double*)w.rec, weight, sin_min, t_junctions ? 1 : 0,
                     (const int*)w.parent, (const int*)w.last, (const int*)w.vidx, (const int*)voff, vertices, degree, kind, score, spread, t_edge,
                     ends);
  NEAT_CHECK(hipGetLastError());
  hipLaunchKernelGGL(wf_duplicate_kernel, pairs, dim3(WF_WG), 0, st, segoff, S, w.tiles, (const int*)ends, weight, w.keep);
  hipLaunchKernelGGL(wf_edge_scan_kernel, dim3(1), dim3(1024), 0, st, S, V, segoff, (const int*)w.keep, w.eidx, eoff);
  hipLaunchKernelGGL(wf_edge_fill_kernel, per_seg, dim3(WF_WG), 0, st, S, segoff, (const int*)w.view, (const int*)w.keep, (const int*)w.eidx,
                     (const int*)ends, weight, edges, eweight, esrc);
  return (int)hipGetLastError();
}

// ---- added to ABI v15: 3-D wireframes with shared junctions from the lines and the views' 2-D graphs (kernels_wireframe3d.hpp) ---------------
size_t neat_wf3d_scratch_bytes(int V, int S, int N, int NV, long long pairs_max) {
  Wf3dWs w;
  return wf3d_layout(nullptr, V, S, N, NV, pairs_max, &w) ? w.total_bytes : 0;
}

int neat_wf3d_build(const double* lines3d, const double* support, int N, const int* members, const double* estimate, const int* endv, const int* view,
                    int V, int S, int NV, long long pairs_max, double end_frac, double reach, double sin_min, int min_votes, void* ws, double* vertices,
                    int* degree, int* kind, int* votes, double* spread, int* n_vertices, int* edges, int* esrc, int* n_edges, void* stream) {
  Wf3dWs w;
  if (!(end_frac > 0.0 && end_frac < 0.5) || !(reach > 0.0 && reach <= 1.0) || !(sin_min > 0.0 && sin_min <= 1.0) || min_votes < 1 || !n_vertices ||
      !n_edges || !wf3d_layout(ws, V, S, N, NV, pairs_max, &w))
    return -1;
  hipStream_t st = (hipStream_t)stream;
  if (N == 0) {
    NEAT_CHECK(hipMemsetAsync(n_vertices, 0, sizeof(int), st));
    return (int)hipMemsetAsync(n_edges, 0, sizeof(int), st);
  }
  if (!lines3d || !support || !ws || ((uintptr_t)ws & 255) || !vertices || !degree || !kind || !votes || !spread || !edges || !esrc ||
      (S > 0 && (!members || !estimate || !endv || !view)))
    return -1;
  const size_t n_rec = 2 * (size_t)S, n_pair = (size_t)pairs_max;
  // what the three sorts want, asked before anything is launched
  if (n_rec > 0) NEAT_PASS(sort_keys(w.sort, w.sort_bytes, w.rkey, w.rskey, n_rec, 0u, 64u, st, false));
  if (n_rec > 0 && n_pair > 0) NEAT_PASS(sort_keys(w.sort, w.sort_bytes, w.pkey, w.pskey, n_pair, 0u, 64u, st, false));
  NEAT_PASS(sort_pairs(w.sort, w.sort_bytes, w.ekey, w.eskey, w.eline, w.esline, (size_t)N, 0u, 64u, st, false));
  const int n2 = 2 * N;
  NEAT_CHECK(hipMemsetAsync(w.total, 0, sizeof(long long), st));
  hipLaunchKernelGGL(wf3_init_kernel, grid1(n2, WF3_WG), dim3(WF3_WG), 0, st, n2, w.parent, w.last, w.lvotes);
  if (n_rec > 0) {
    NEAT_CHECK(hipMemsetAsync(w.vview, 0, (size_t)NV * sizeof(int), st));
    hipLaunchKernelGGL(wf3_ends_kernel, grid1(S, WF3_WG), dim3(WF3_WG), 0, st, lines3d, N, members, estimate, endv, view, V, S, NV, end_frac, w.rkey,
                       w.vview);
    NEAT_CHECK(hipGetLastError());
    NEAT_PASS(sort_keys(w.sort, w.sort_bytes, w.rkey, w.rskey, n_rec, 0u, 64u, st));
    hipLaunchKernelGGL(wf3_pair_count_kernel, grid1(2 * S, WF3_WG), dim3(WF3_WG), 0, st, (const wf3_key*)w.rskey, 2 * S, w.rcnt);
    hipLaunchKernelGGL(count_scan_kernel<long long>, dim3(1), dim3(1024), 0, st, 2 * S, (const int*)w.rcnt, w.roff, w.total);
    if (n_pair > 0) {
      NEAT_CHECK(hipMemsetAsync(w.pkey, 0xff, n_pair * sizeof(wf3_key), st));
      hipLaunchKernelGGL(wf3_pair_fill_kernel, grid1(2 * S, WF3_WG), dim3(WF3_WG), 0, st, (const wf3_key*)w.rskey, 2 * S, (const long long*)w.roff,
                         (const int*)w.vview, NV, pairs_max, w.pkey);
      NEAT_CHECK(hipGetLastError());
      NEAT_PASS(sort_keys(w.sort, w.sort_bytes, w.pkey, w.pskey, n_pair, 0u, 64u, st));
      hipLaunchKernelGGL(wf3_link_kernel, dim3((unsigned)((pairs_max + WF3_WG - 1) / WF3_WG)), dim3(WF3_WG), 0, st, (const wf3_key*)w.pskey, pairs_max, lines3d, N, min_votes, reach,
                         sin_min, w.parent, w.lvotes);
    }
  }
  hipLaunchKernelGGL(uf_flatten_kernel, grid1(n2, UF_WG), dim3(UF_WG), 0, st, n2, w.parent, w.last);
  NEAT_CHECK(hipGetLastError());
  hipLaunchKernelGGL(wf3_vertex_scan_kernel, dim3(1), dim3(1024), 0, st, n2, (const int*)w.parent, w.vidx, n_vertices);
  hipLaunchKernelGGL(wf3_vertex_kernel, grid1(n2, WF3_WAVES), dim3(WF3_WG), 0, st, n2, (const int*)w.parent, (const int*)w.last, (const int*)w.vidx,
                     (const int*)w.lvotes, lines3d, vertices, degree, kind, votes, spread);
  hipLaunchKernelGGL(wf3_edge_key_kernel, grid1(N, WF3_WG), dim3(WF3_WG), 0, st, N, (const int*)w.parent, (const int*)w.vidx, w.ekey, w.eline, w.keep);
  NEAT_CHECK(hipGetLastError());
  NEAT_PASS(sort_pairs(w.sort, w.sort_bytes, w.ekey, w.eskey, w.eline, w.esline, (size_t)N, 0u, 64u, st));
  hipLaunchKernelGGL(wf3_edge_pick_kernel, grid1(N, WF3_WG), dim3(WF3_WG), 0, st, N, (const wf3_key*)w.eskey, (const int*)w.esline, support, w.keep);
  hipLaunchKernelGGL(wf3_edge_scan_kernel, dim3(1), dim3(1024), 0, st, N, (const int*)w.keep, w.eidx, (const long long*)w.total, pairs_max, n_vertices,
                     n_edges);
  hipLaunchKernelGGL(wf3_edge_fill_kernel, grid1(N, WF3_WG), dim3(WF3_WG), 0, st, N, (const int*)w.keep, (const int*)w.eidx, (const int*)w.parent,
                     (const int*)w.vidx, edges, esrc);
  return (int)hipGetLastError();
}

}  // extern "C"
