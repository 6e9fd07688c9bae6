/* neat_hip.h -- C ABI of libneat_hip.so: the MI355X (gfx950) implementation of NEAT's volumetric-
 * rendering hot path.  Plain pointers and sizes only (no torch types).  A pointer parameter is a DEVICE
 * pointer (to float32 unless its type or the text says otherwise) or an opaque handle -- `stream`, a
 * hipStream_t passed as void*; a workspace `ws`; a `bvh` -- unless it is marked NEAT_HOST: those the entry
 * point itself reads or writes on the host before it returns, so they must be host memory and may be
 * freed after the call.  Pointer fields inside the structs are device pointers.  Every call is
 * asynchronous on its stream, never synchronises, never allocates, never keeps caller memory, unless
 * its own text says so.
 * Return value: 0 on success, otherwise a hipError_t (or -1 for bad arguments).
 *
 * This file is also the one written copy of the signatures: neat_amd/_lib.py builds its ctypes binding by
 * reading it, so a declaration keeps the plain form `int|size_t neat_x(T a, const T* b, NEAT_HOST const T* c, ...);`
 * with the scalar types int, float, double, long long and size_t.
 *
 * The reference (cherubicXN/neat) has no native layer: these entry points replace the ATen op
 * sequences issued by the Python lines cited on each function (paths relative to the reference's
 * code/ directory).  INTEGRATION.md shows the ctypes binding a reference maintainer would add.
 *
 * Layouts: "row-major [P,C]" is the torch layout the reference uses.  Workspaces are opaque float
 * arenas sized by the *_ws_floats() queries; they carry the activations saved for backward.
 */
#ifndef NEAT_HIP_H
#define NEAT_HIP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define NEAT_HOST             /* marks a pointer parameter the entry point dereferences on the host (expands to nothing) */
#define NEAT_NUM_LAYERS 19   /* implicit_network.lin0..8, rendering_network.lin0..4, attraction_network.lin0..4 */
#define NEAT_FEATURE 256

/* Raw parameters exactly as in the reference state_dict (weight-normed Linear layers:
 * model/networks/neat_wfr_rend_a.py:71-72,167-168,227-228): weight_v [out,in], weight_g [out,1], bias [out]. */
typedef struct neat_net_params {
  const float* v[NEAT_NUM_LAYERS];
  const float* g[NEAT_NUM_LAYERS];
  const float* b[NEAT_NUM_LAYERS];
} neat_net_params;

/* Gradient destinations, same shapes as neat_net_params (overwritten, not accumulated).  A NULL dv[l]
 * skips layer l (e.g. the heads when only the SDF network was run). */
typedef struct neat_net_grads {
  float* dv[NEAT_NUM_LAYERS];
  float* dg[NEAT_NUM_LAYERS];
  float* db[NEAT_NUM_LAYERS];
} neat_net_grads;

int neat_abi_version(void);      /* 15 */

/* `precision` selects the build of the GEMM-class kernels:
 *   NEAT_F32  (0): exact-f32 MFMA, fp32 activations  -- parity build (outputs within 1e-4 of the reference)
 *   NEAT_BF16 (1): bf16 MFMA with fp32 accumulate, bf16 hidden activations -- throughput build
 *   NEAT_BF16X3 (2): the NEAT_F32 build (same layouts, workspaces, packed weights, kernels) whose two GEMM kernels evaluate every
 *                    product as three bf16 MFMAs on hi/lo splits of both operands, fp32 accumulate (~2^-17 relative per product):
 *                    fp32-grade parity at a multiple of the f32-MFMA rate
 *   NEAT_F16 (3): the NEAT_BF16 build with IEEE half instead of bf16 as the 16-bit type: v_mfma_f32_32x32x16_f16, fp32 accumulate,
 *                 f16 hidden activations (BASELINE config 5, "fp16 MFMA with fp32 accumulate").  Same kernels, layouts, workspaces
 *                 and speed; 3 more mantissa bits (errors ~8x below NEAT_BF16's), 5 exponent bits: the backward pass runs on
 *                 cotangents scaled by 4096 internally (scaled where the caller's cotangents are read, scaled back on the finished
 *                 gradients; nothing visible at this interface).
 *   NEAT_F16X3 (4): the NEAT_F16 build (layouts, workspaces + lo planes, the whole backward pass) whose three FORWARD chains -- SDF
 *                   primal (rend_a :78-96), SDF adjoint = normals (:121-127), both heads (:139-255) -- are fused launches that
 *                   evaluate every product as three f16 MFMAs on hi/lo splits of both operands (~22 mantissa bits): forward outputs
 *                   within 1e-4 of the reference like NEAT_F32, gradients at the fp32 build's bar (the backward pass reads the hi
 *                   planes = exactly what NEAT_F16 saves), at about the speed of NEAT_F16.
 *   NEAT_F16X3_FASTVALUES (5): accepted by the VALUES-mode calls only (neat_sdf_forward mode 0, neat_sdf_values_gated,
 *                   neat_sdf_ws_floats) together with a NEAT_F16X3 pack: the query runs through NEAT_F16's one-product chain (3x
 *                   faster).  For a depth sampler that may trade the reference's exact samples for speed (the sampled distribution
 *                   stays the reference's to ~1e-4 of the depth range, tests/test_gpu_parity.py::test_sampler_vs_reference_golden).
 * Packed weights, workspaces and forward/backward calls of one pass must use the same value. */
#define NEAT_F32 0
#define NEAT_BF16 1
#define NEAT_BF16X3 2
#define NEAT_F16 3
#define NEAT_F16X3 4
#define NEAT_F16X3_FASTVALUES 5

/* ---- a15: weight norm + packing (replaces the per-call `_weight_norm` pre-hook) -------------------
 * Computes W = g * v/|v| for all 19 layers once per step and stores W and W^T in MFMA-fragment order. */
size_t neat_packed_floats(int precision);
int neat_pack_weights(NEAT_HOST const neat_net_params* net, float* packed, int precision, void* stream);

/* ---- a1: pixel -> unit ray directions (utils/rend_util.py:55-81 get_camera_params, :95-108 lift) --
 * uv [R,2], pose [4,4] cam-to-world, K row stride `kstride` (3 or 4).  dirs [R,3].  Origin = pose[:3,3]. */
int neat_camera_rays(const float* uv, const float* pose, const float* K, int kstride, int R, float* dirs, float* origins /* [R,3] or NULL: the camera centre per ray */,
                     void* stream);
/* a12: the eikonal points of a training step (neat_wfr_rend_a.py:515-527) as one array [2R + J, 3]:
 * [uniform [R,3] (drawn by the caller) | origins + z_eik dirs | extra [J,3] (the global junctions, J may be 0)].
 * z_eik [R] = the depth drawn per ray; NULL (ABI v12): picked here as z[r, idx[r]] from the ray's S depths z [R,S] with the drawn
 * indices idx [R] (int64) -- the `torch.gather(z_vals, 1, idx)` of model/ray_sampler.py:276-277 without a launch of its own. */
int neat_eik_points(const float* uniform, const float* origins, const float* dirs, const float* z_eik, const float* extra, int R, int J,
                    float* out, const float* z, int S, const long long* idx, void* stream);

/* ---- a4+a5: SDF / implicit network (neat_wfr_rend_a.py:78-137) -----------------------------------
 * mode 0: values only  -> sdf[P] = get_sdf_vals(x)            (:131-137), nothing saved
 * mode 1: outputs      -> forward() [P,257], clamped sdf, feature, d sdf/dx (get_outputs :111-129 /
 *                         gradient :98-109 when radius <= 0), activations saved in `ws` for backward.
 * radius > 0 enables the bounding-sphere clamp min(sdf, scale*(radius-|x|)).
 * Any of out257 / sdf / feat / grad may be NULL.  x is row-major [P,3]. */
size_t neat_sdf_ws_floats(int P, int mode, int precision);
int neat_sdf_forward(const float* packed, NEAT_HOST const neat_net_params* net, const float* x, int P, int mode, int precision,
                     float radius, float scale, float* ws,
                     float* out257, float* sdf, float* feat, float* grad, void* stream);
/* Backward of mode-1 forward (autograd incl. the double backward through d sdf/dx, which the reference
 * gets from create_graph=True at :121-127).  Cotangents are row-major and may be NULL (= zero):
 * d_out257 [P,257] (of forward()), d_sdf [P] (of the clamped sdf), d_feat [P,256], d_grad [P,3].
 * Writes grads->dv/dg/db[0..8]. */
int neat_sdf_backward(const float* packed, NEAT_HOST const neat_net_params* net, float* ws, int P, int precision,
                      const float* d_out257, const float* d_sdf, const float* d_feat, const float* d_grad,
                      NEAT_HOST const neat_net_grads* grads, void* stream);
/* ABI v14: neat_sdf_backward, differentiated in the query points x as well (rend_a :111-137 are plain autograd in x: get_outputs,
 * gradient, forward and get_sdf_vals; the normal, built with create_graph=True at :121-127, included).  Same arguments plus
 * scale (the forward's sphere scale: the clamped sdf s (radius - |x|) and its gradient -s x/|x| depend on it) and d_x [P,3] row-major,
 * which receives dL/dx of L = <d_out257, forward()> + <d_sdf, sdf> + <d_feat, feat> + <d_grad, d sdf/dx>, first order (d_x itself is
 * not differentiable).  grads may be NULL, and so may any layer's dv/dg/db (all three together): no weight gradient is formed for those
 * layers -- a frozen network whose input points are optimised.  The parameter gradients it does write equal neat_sdf_backward's. */
int neat_sdf_backward_x(const float* packed, NEAT_HOST const neat_net_params* net, float* ws, int P, int precision, float scale,
                        const float* d_out257, const float* d_sdf, const float* d_feat, const float* d_grad,
                        NEAT_HOST const neat_net_grads* grads, float* d_x, void* stream);

/* ---- a6+a7: the two heads on given inputs (RenderingNetwork.forward :235-255,
 * AttractionFieldNetwork.forward :175-197), row-major inputs; rgb [P,3], lines [P,2,3]. */
size_t neat_heads_ws_floats(int P, int precision);
int neat_heads_forward(const float* packed, NEAT_HOST const neat_net_params* net, const float* points, const float* normals,
                       const float* view_dirs, const float* feats, int P, int precision, float* ws,
                       float* rgb, float* lines, void* stream);

/* ---- a5-a10 fused main pass: VolSDFNetwork.forward :392-422 (+ :530-536 normal_map in eval) -------
 * origins/dirs [R,3], z [R,S] sorted depths, beta = DEVICE pointer to one float (a pointer so that no host sync is needed); the
 * density's beta is |*beta| + beta_min (model/density.py:28-30; ABI v12): pass the raw parameter density.beta and the module's
 * beta_min, or -- as up to v11 -- the value of get_beta() and 0.
 * Outputs (row-major, NULL to skip where noted): points [R,S,3] (opt), weights [R,S] (opt),
 * sdf [R,S] (opt), rgb [R,3], lines3d [R,2,3], depth [R], xyz [R,3], normal_map [R,3] (opt). */
size_t neat_render_ws_floats(int R, int S, int E, int precision);
int neat_render_forward(const float* packed, NEAT_HOST const neat_net_params* net, const float* origins, const float* dirs,
                        const float* z, int R, int S, int precision, const float* beta, float beta_min, float radius, float scale, float* ws,
                        float* points, float* weights, float* sdf, float* rgb, float* lines3d, float* depth,
                        float* xyz, float* normal_map, const float* eik_points, int E, float* eik_grad, void* stream);
/* a12 folded in: `eik_points` [E,3] (may be NULL with E = 0) are E extra points appended to the R*S ray samples for
 * the SDF network only; eik_grad [E,3] receives ImplicitNetwork.gradient (:98-109, no sphere clamp) at those points.
 * This removes ~66 latency-bound small launches per training step (the 2R eikonal points of :515-527).
 *
 * Backward of neat_render_forward.  Cotangents d_rgb [R,3], d_lines3d [R,6], d_depth [R], d_xyz [R,3], d_eik_grad [E,3],
 * d_acc [R] = cotangent of the ray's opacity acc_map = sum_i w_i (the white_bkgd term of :411-413; ABI v11) (NULL = zero).  lines3d uses detached weights exactly as :410.  Writes all 19 layers' grads and the
 * per-ray partial derivative wrt the density's beta, dbeta_ray [R].  dbeta (device pointer to one float, or NULL; ABI v12) receives
 * the gradient of *beta itself: sgn(*beta) * sum_r dbeta_ray[r], summed in a fixed order by one more tiny launch (the `.sum()` and the
 * backward of `.abs()` of density.py:29-30). */
int neat_render_backward(const float* packed, NEAT_HOST const neat_net_params* net, float* ws, const float* dirs,
                         const float* z, int R, int S, int E, int precision, const float* beta, float beta_min,
                         const float* d_rgb, const float* d_lines3d, const float* d_depth, const float* d_xyz,
                         const float* d_eik_grad, const float* d_acc, NEAT_HOST const neat_net_grads* grads, float* dbeta_ray, float* dbeta, void* stream);

/* Forward-only variant for eval / inference callers (code/neat-final-parsing.py:203-218 drives `model(s)` in 2048-ray chunks under
 * model.eval(); training/volsdf_train.py:312-320 renders validation images the same way): same arguments and results as
 * neat_render_forward with E = 0, but the workspace keeps nothing for a backward pass (hidden activations of the adjoint chain and
 * of the two heads ping-pong between two buffers): about a quarter of neat_render_ws_floats. */
size_t neat_render_eval_ws_floats(int R, int S, int precision);
int neat_render_forward_eval(const float* packed, NEAT_HOST const neat_net_params* net, const float* origins, const float* dirs,
                             const float* z, int R, int S, int precision, const float* beta, float beta_min, float radius, float scale, float* ws,
                             float* points, float* weights, float* sdf, float* rgb, float* lines3d, float* depth,
                             float* xyz, float* normal_map, void* stream);

/* ---- a2: UniformSampler.get_z_vals (model/ray_sampler.py:61-95): N depths per ray between near and far (per ray [R] if the pointer
 * is given, else the scalar), stratified jitter with rnd [R,N] in training (NULL: the plain grid).  t [N] = the linspace(0, 1, N)
 * grid.  Operations rounded one by one like the reference's elementwise ops: bit-identical to them. */
int neat_uniform_depths(const float* near_r, float near_s, const float* far_r, float far_s, const float* t, const float* rnd, int R, int N,
                        float* z, void* stream);

/* ---- a13: sample_pdf (model/ray_sampler.py:16-59) and the sort of UniformSampler.get_z_vals_fine (:97-106), one wavefront per ray:
 * bins [R,nb], weights [R,nb-1] (the caller passes weights[..., 1:-1] and the interval mid points), u [N] (u_stride 0) or [R,N]
 * -> samples [R,N]; z_merge [R,nz] given: z_out [R,nz+N] = sort(cat[z_merge, samples]).  fp64 CDF rounded once per knot. */
int neat_sample_pdf(const float* bins, const float* weights, int nb, int R, const float* u, int u_stride, int N, float* samples,
                    const float* z_merge, int nz, float* z_out, void* stream);

/* ---- a3: ErrorBoundSampler bookkeeping (model/ray_sampler.py:130-293), one wavefront per ray --------------------
 * One round of Algorithm 1 = neat_sdf_forward(mode 0) on the new samples, then:
 *  neat_sampler_bound    : merge the sdf values (order from the previous round, :152-157), d* per interval (:161-173),
 *                          per-ray bisection of beta on [beta0, beta_in] (:177-185, get_error_bound :285-293);
 *                          *flag |= 1 if any ray still has beta > beta0 (the batch-global test of :200 -- the host
 *                          reads the flag once per round, as the reference syncs once per round).
 *  neat_sampler_resample : pdf (error-bound opacity :205-215 if refine, rendering weights + 1e-5 :217-226 otherwise),
 *                          CDF, inverse-CDF sampling at u (:237-249); refine also emits the sorted union with the old
 *                          grid and its gather order (:254).  u has N entries per ray (u_stride = N) or is shared (0).
 *  neat_sampler_finish   : [final samples | near | far | picked grid points] sorted (:259-272) and the eikonal depth.
 * All tensors row-major; n, N <= 1024. */
int neat_sampler_bound(const float* z, int n, int R, const float* sdf_old, const float* sdf_new, const int* order, int n_old,
                       const float* beta_in, const float* beta0, float eps, int iters, float* sdf_out, float* beta_out,
                       int* flag, void* stream);
int neat_sampler_resample(const float* z, const float* sdf, int n, int R, const float* beta, int refine, float add_tiny,
                          const float* u, int u_stride, int N, float* samples, float* z_merged, int* order, void* stream);
int neat_sampler_finish(const float* samples, int N, const float* z, int n, const int* pick, int n_extra, float near, float far,
                        int R, const int* eik_idx, float* z_vals, float* z_eik, void* stream);

/* ---- a3 without host synchronisation (HIP-graph capturable) -----------------------------------------------------
 * The reference reads `beta.max() > beta0` on the host once per round (:200).  Here the rounds are a FIXED sequence of max_rounds
 * launches and the decision lives in device memory: int32 open[max_rounds] (zero-initialised; the bound kernel of round k ORs into
 * open[k]) and int32 cont[max_rounds] (the resample launch of round k writes 1 = "refined, go on" or 2 = "final samples drawn").
 * A launch of round k > 0 does nothing unless cont[k-1] == 1, so the rounds after the final one cost only their launch.
 *  neat_sdf_values_gated     : neat_sdf_forward(mode 0) that returns at once unless *gate == gate_value (gate = &cont[k-1], 1).
 *  neat_sdf_values_rays      : the same for the points o + z d of R rays x S depths (sdf [R S]): the round's `cam_loc + samples * dirs`
 *                              (:146) is formed by the launch that lays the points out for the SDF kernels (ABI v12).
 *  neat_sampler_init         : what precedes the first round (:131-143) in one launch (ABI v12): beta0[0] = |*beta| + beta_min
 *                              (density.py:29-30), beta_ray[r] = sqrt(beta_c sum_i (z[r,i+1] - z[r,i])^2) with beta_c = 1 / (4 log(1 + eps)),
 *                              and the nctl control words of the rounds zeroed.
 *  neat_sampler_bound_dev    : neat_sampler_bound with `open` = &open[k] and the same gate.
 *  neat_sampler_resample_dev : decides refine = *open && round + 1 < max_rounds on the device.  refine: N_refine samples at u_refine
 *                              (shared by the rays), merged grid and order, as neat_sampler_resample(refine=1).  Otherwise the N_final
 *                              output samples at u_final (stride u_final_stride), a copy of this round's grid into z_final
 *                              [R, ld_final] and its size into *n_final.
 *  neat_sampler_finish_dev   : picks the n_extra grid points on the device (sizes come from *n_final): keys == NULL ->
 *                              linspace(0, n-1, n_extra).long() (:266, eval); keys [>= n] -> the indices of the n_extra smallest
 *                              keys, a uniformly random subset like randperm(n)[:n_extra] (:264, training); then as
 *                              neat_sampler_finish.  `pick` [n_extra] receives the indices. */
int neat_sdf_values_gated(const float* packed, NEAT_HOST const neat_net_params* net, const float* x, int P, int precision, float radius,
                          float scale, float* ws, float* sdf, const int* gate, int gate_value, void* stream);
int neat_sdf_values_rays(const float* packed, NEAT_HOST const neat_net_params* net, const float* origins, const float* dirs, const float* z, int R,
                         int S, int precision, float radius, float scale, float* ws, float* sdf, const int* gate, int gate_value,
                         void* stream);
int neat_sampler_init(const float* z, int R, int n, const float* beta, float beta_min, float beta_c, float* beta0, float* beta_ray,
                      int* ctl, int nctl, void* stream);
int neat_sampler_bound_dev(const float* z, int n, int R, const float* sdf_old, const float* sdf_new, const int* order, int n_old,
                           const float* beta_in, const float* beta0, float eps, int iters, float* sdf_out, float* beta_out,
                           int* open, const int* gate, int gate_value, void* stream);
int neat_sampler_resample_dev(const float* z, const float* sdf, int n, int R, const float* beta, float add_tiny,
                              const float* u_refine, int N_refine, float* samples_refine, float* z_merged, int* order,
                              const float* u_final, int u_final_stride, int N_final, float* samples_final, float* z_final, int ld_final,
                              int* n_final, const int* open, int* cont, int round, int max_rounds, void* stream);
int neat_sampler_finish_dev(const float* samples, int N, const float* z_final, int ld_final, const int* n_final, const float* keys,
                            int n_extra, int* pick, float near, float far, int R, const int* eik_idx, float* z_vals, float* z_eik,
                            void* stream);

/* ---- a3, one launch per round (ABI v13; replaces bound_dev + resample_dev + the layout launch of neat_sdf_values_rays per round) ------
 * The same arithmetic as the entry points above, reference model/ray_sampler.py:145-254 per round.  Control words
 * ctl = int32 open[max_rounds] | ran[max_rounds] | n_final (zeroed by neat_sampler_init_rays): round k ORs 1 into open[k] when a ray's
 * beta is still above beta0 (the batch-global test of :200); a launch of round k > 0 (this one and the round's SDF query, gate =
 * &open[k-1], gate_value 1) does nothing unless open[k-1] is set.  Because the test cannot be read inside the launch that produces it,
 * a round prepares both outcomes: every ray refines (rounds before the last), and the rays whose own beta has reached beta0 -- all
 * rays in the last round -- also draw the final samples, copy the grid to z_final and write n_final; the last round that ran wins.
 *  neat_sdf_ldp             : point stride of the SDF kernels' feature-major layout for P points (the first 3 rows of a
 *                             neat_sdf_ws_floats workspace are x [3][ldp]).
 *  neat_sdf_values_laid_out : neat_sdf_values_gated on points that already sit in the workspace's x rows.
 *  neat_sampler_init_rays   : neat_sampler_init + (x_fm != NULL) the first round's query points cam_loc + z dirs (:146) into x_fm,
 *                             + (keys != NULL) for every possible final grid size n_step (c + 1), c < n_cand, the n_extra smallest
 *                             of its first n keys in key order -> pick_all [n_cand][n_extra] (the training-mode randperm(n)[:n_extra]
 *                             of :264-265 as neat_sampler_finish_dev draws it, computed beside the prologue instead of behind the rounds).
 *  neat_sampler_round       : merge + d* + bisection (as neat_sampler_bound), then refine: N_refine samples at u_refine, merged grid
 *                             z_merged / order_out [R, n + N_refine], and the NEXT round's query points into x_fm [3][ldp] (the
 *                             workspace of the next neat_sdf_values_laid_out; NULL: not wanted); final: N_final samples at u_final.
 *  neat_sampler_finish_picked : neat_sampler_finish with the grid size read from *n_final and the picks from
 *                             pick_all[n / n_step - 1] (pick_all == NULL: linspace(0, n - 1, n_extra).long(), eval mode :266). */
int neat_sdf_ldp(int P, int precision);
int neat_sdf_values_laid_out(const float* packed, NEAT_HOST const neat_net_params* net, int P, int precision, float radius, float scale, float* ws,
                             float* sdf, const int* gate, int gate_value, void* stream);
int neat_sampler_init_rays(const float* z, int R, int n, const float* beta, float beta_min, float beta_c, float* beta0, float* beta_ray,
                           int* ctl, int nctl, const float* origins, const float* dirs, float* x_fm, int ldp, const float* keys, int n_step,
                           int n_cand, int n_extra, int* pick_all, void* stream);
int neat_sampler_round(const float* z, int n, int R, const float* sdf_old, const float* sdf_new, const int* order, int n_old,
                       const float* beta_in, const float* beta0, float eps, int iters, float* sdf_out, float* beta_out, int* ctl, int round,
                       int max_rounds, float add_tiny, const float* u_refine, int N_refine, float* samples_refine, float* z_merged,
                       int* order_out, const float* origins, const float* dirs, float* x_fm, int ldp, const float* u_final,
                       int u_final_stride, int N_final, float* samples_final, float* z_final, int ld_final, void* stream);
int neat_sampler_finish_picked(const float* samples, int N, const float* z_final, int ld_final, const int* n_final, const int* pick_all,
                               int n_step, int n_extra, float near, float far, int R, const int* eik_idx, float* z_vals, float* z_eik,
                               void* stream);

/* ---- 8f-1 (next row): dataset attraction field, replacement for the un-vendored hawp.base._C.encodels ------------
 * (datasets/blender_hawp_dataset.py:96, scene_hawp_dataset.py:95).  lines [N,4] = (x1,y1,x2,y2) in pixels;
 * lmap [6,H,W] = closest point - pixel (0:2), endpoint 1 - pixel (2:4), endpoint 2 - pixel (4:6), all (x,y);
 * label [H,W] int32 = index of the nearest segment (the reference's labels_onehot.max(dim=0)[1]);
 * valid [H,W] uint8 (may be null) = the reference's labels_onehot.max(dim=0)[0], which the dataset multiplies into its support mask
 *   (blender_hawp_dataset.py:98,130): 1 where the pixel HAS a nearest segment -- i.e. at least one segment with finite coordinates
 *   exists; 0 everywhere for N = 0 (then lmap = 0, label = 0) and for segments that are all non-finite.  A zero-length segment is a
 *   segment (a point).
 * PARITY UNPINNED: hawp is an empty submodule here; semantics are those the call sites rely on. */
int neat_encode_lines(const float* lines, int N, int H, int W, float* lmap, int* label, unsigned char* valid, void* stream);

/* ---- 8f-1, batch assembly on the device: the ray sampling of Dataset.__getitem__ (datasets/blender_hawp_dataset.py:186-198,
 * scene_hawp_dataset.py:179-190) with the view's maps resident in HBM.  pool [npool] int32 = pixels of the line support
 * (mask.nonzero()); draw [n] int64 = the step's draws into the pool (made on the host: np.random.choice's stream for the ABC class);
 * att [HW,2] foot points, rgb [HW,3], labels [HW] int32 (nearest segment), lines [nlines,5].  Per ray i, pixel p = pool[draw[i]]:
 * uv [n,2] = (p mod W, p div W), uv_proj [n,2] = att[p], rgb_out [n,3], lines_out [n,5] = lines[labels[p]], labels_out [n],
 * pixel_out [n] = p. */
int neat_gather_batch(const int* pool, int npool, const long long* draw, int n, int W, const float* att, const float* rgb, const int* labels,
                      const float* lines, int nlines, float* uv, float* uv_proj, float* rgb_out, float* lines_out, long long* labels_out,
                      long long* pixel_out, void* stream);

/* ---- step prefix: the fresh batch's tensors (datasets' collate output, training/volsdf_train.py:361-364 `model_input[...] = ...cuda()`)
 * and the step's CPU-drawn randoms (the reference draws on the host: model/ray_sampler.py:86-93,132; neat_wfr_rend_a.py:330-335) into the
 * persistent tensors a captured step reads, as ONE launch: copy i moves nbytes[i] bytes from src[i] to dst[i] (n <= 16).  A source may be
 * device memory or pinned host memory (hipHostMalloc: the kernel reads it over the bus -- no separate copy-engine transfer and none of
 * the idle gaps between a copy and the next kernel).  Pointers 4-byte aligned, sizes multiples of 4. */
int neat_copy_batch(NEAT_HOST const void* const* src, NEAT_HOST void* const* dst, NEAT_HOST const long long* nbytes, int n, void* stream);

/* ---- a11 / a14 glue as single launches.  neat_project2d = VolSDFNetwork.project2D (model/networks/neat_wfr_rend_a.py:317-326):
 * K [3,3] and w2c [3,4] = [R|T] row-major on the device, X [N,3] -> uv [N,2]; its backward gives d_X from d_uv.
 * neat_line_loss = VolSDFLoss.get_line_loss (model/networks/loss_wfr.py:34-45): pred, gt [R,4], weight [R] ->
 * out2 = {loss, number of gated lines}, per_line [R], d_pred [R,4] = d loss / d pred. */
/* junction block pieces (model/networks/neat_wfr_rend_a.py:441-489) as single launches: neat_l3d (:441-447: plane intersection per ray),
 * neat_junction_cost (:472: cost[v][c] = |cand2d[c] - gt2d[v]|), neat_junction_gate (:474-489: matched costs of the neat_lsap pairs,
 * median or 10 px gate, matched candidates gathered into padded [K,.] arrays + mask; K <= 2048). */
int neat_l3d(const float* x, const float* o, const float* d, const float* normal, int R, float* l3d, void* stream);
int neat_junction_cost(const float* cand2d, const float* gt2d, int V, int C, float* cost, void* stream);
int neat_junction_gate(const long long* rows, const long long* cols, int K, const float* cost, int C, const float* cand3d,
                       const float* cand2d, const float* cand2d_calib, int use_median, float* median, unsigned char* good, float* j3d,
                       float* j2d, float* j2d_calib, void* stream);
/* the tail of VolSDFLoss.forward (model/networks/loss_wfr.py:68-137) as two launches around the junction matching (neat_lsap):
 * neat_loss_terms -> scal[0] = L1 rgb loss (mean), scal[1] = eikonal loss, d_rgb [R,3], d_gtheta [E,3] (cotangents for unit
 * upstream gradient), pair_cost [K,J] = cdist_1(loc3, glo3) + 0.1 cdist_1(loc2c, glo2c);
 * neat_loss_pairs (ri, ci, n_match from neat_lsap over pair_cost) -> scal[2..5] = mean 3-D / calibrated 2-D / pixel 2-D pair
 * distance and the count of pairs with cost < 10, scal[6] = rgb + w_eik eik + w_line line_loss[0] + w_j3 j3d + w_j2 j2d;
 * d_glo3 [J,3], d_glo2c [J,2] = cotangents of the global junctions.
 * ABI v12: the cotangents can leave as gradients of the TOTAL loss scal[6], so that the backward pass has nothing left to multiply:
 * d_gtheta carries eik_grad_scale (pass w_eik, or 1), d_glo3 / d_glo2c carry w_j3 / w_j2 when weighted_grads != 0; `total` (or NULL)
 * receives scal[6] once more, in an allocation of its own (the differentiable output of the caller's autograd node). */
int neat_loss_terms(const float* rgb, const float* rgb_gt, int R, const float* gtheta, int E, const float* loc3, const float* loc2c, int K,
                    const float* glo3, const float* glo2c, int J, float* scal, float* d_rgb, float* d_gtheta, float* pair_cost,
                    float eik_grad_scale, void* stream);
/* ABI v13: neat_line_losses and neat_loss_terms (independent of each other) as the two workgroups of one launch; same arithmetic.
 * d_lines3d != NULL: pred_calib = neat_project2d(identity, w2c, lines3d [L,2,3]) (rend_a :441); the gradient of the line term is carried
 * through that projection here (d_lines3d [L,2,3], neat_project2d_backward's arithmetic).  Likewise neat_loss_pairs with w2c != NULL:
 * glo2c = neat_project2d(identity, w2c, glo3) (:496) and d_glo3 receives d_glo2c's share -- the projections' backward launches and the
 * accumulation of the global junctions' two gradients disappear from the step. */
int neat_loss_lines_terms(const float* pred_px, const float* pred_calib, const float* gt5, const float* Kmat, int L, float threshold, float* out3,
                          float* d_pred_calib, float grad_scale, const float* rgb, const float* rgb_gt, int R, const float* gtheta, int E,
                          const float* loc3, const float* loc2c, int K, const float* glo3, const float* glo2c, int J, float* scal, float* d_rgb,
                          float* d_gtheta, float* pair_cost, float eik_grad_scale, const float* w2c, const float* lines3d, float* d_lines3d,
                          void* stream);
int neat_loss_pairs(const long long* ri, const long long* ci, const int* n_match, int Kmax, const float* loc3, const float* loc2c,
                    const float* loc2, const float* glo3, const float* glo2c, const float* glo2, int J, const float* pair_cost, float* scal,
                    float* d_glo3, float* d_glo2c, const float* line_loss, float w_eik, float w_line, float w_j3, float w_j2, int weighted_grads,
                    float* total, const float* w2c, void* stream);
/* global-junction MLP ffn(latents) (rend_a :303-313, :491): x [J,256] -> relu(W0 x + b0) -> relu(W1 . + b1) -> W2 . + b2 = y [J,3];
 * torch nn.Linear layouts (W [out,in]); h1, h2 [J,256] are saved for the backward; ws2 = 2 J 256 floats of scratch. */
int neat_ffn_forward(const float* x, int J, const float* W0, const float* b0, const float* W1, const float* b1, const float* W2,
                     const float* b2, float* h1, float* h2, float* y, void* stream);
int neat_ffn_backward(const float* x, int J, const float* W0, const float* W1, const float* W2, const float* h1, const float* h2,
                      const float* dy, float* ws2, float* dx, float* dW0, float* db0, float* dW1, float* db1, float* dW2, float* db2,
                      void* stream);
/* inverse of one n x n matrix (n <= 4, row stride lda): pose.inverse() (rend_a :440), K.inverse() (loss_wfr.py:59) */
int neat_inv_small(const float* A, int n, int lda, float* out, void* stream);
/* what the junction block's projections read (rend_a :424-431, :440) in one launch (ABI v12): w2c [3,4] = the first three rows of
 * pose^-1 (pose [4,4] cam-to-world, contiguous) and K3 [3,3] = the contiguous copy of the intrinsics' 3x3 block (row stride kstride) */
int neat_camera_mats(const float* pose, const float* K, int kstride, float* w2c, float* K3, void* stream);
int neat_project2d(const float* K, const float* w2c, const float* X, int N, float* uv, void* stream);
int neat_project2d_backward(const float* K, const float* w2c, const float* X, int N, const float* d_uv, float* d_X, void* stream);
/* ABI v13: the junction block's camera-only work and its double projections as single launches.
 *  neat_camera_setup   : neat_camera_rays for `uv` (dirs, origins) and -- uv2 != NULL -- for `uv2` (dirs2; rend_a :444), plus
 *                        neat_camera_mats (w2c [3,4], K3 [3,3]); same arithmetic as the three launches.
 *  neat_project2d_pair : neat_project2d of the same points with K (-> uv) and with K2 (-> uv2): rend_a :436-441 (lines2d / lines2d_calib),
 *                        :469-471 (junction candidates), :493-496 (global junctions) project with the intrinsics and with the identity. */
int neat_camera_setup(const float* uv, const float* uv2, const float* pose, const float* K, int kstride, int R, float* dirs, float* origins,
                      float* dirs2, float* w2c, float* K3, void* stream);
int neat_project2d_pair(const float* K, const float* K2, const float* w2c, const float* X, int N, float* uv, float* uv2, void* stream);
int neat_line_loss(const float* pred, const float* gt, const float* weight, int R, float threshold, float* out2, float* per_line,
                   float* d_pred, void* stream);
/* Both line terms of VolSDFLoss.forward (loss_wfr.py:52-65) in one launch: pred_px / pred_calib [R,4] = the projected 3-D lines in
 * pixel and in calibrated coordinates, gt5 [R,5] = (x1, y1, x2, y2, weight), K [3,3].  out3 = (l2d pixel term, calibrated line
 * loss, #segments the pixel term accepts); the ground-truth end points are calibrated with K^-1 inside; d_pred_calib [R,4] =
 * grad_scale * d out3[1] / d pred_calib (grad_scale, ABI v12: the line term's weight in the total loss, or 1).  Same arithmetic as
 * neat_line_loss + neat_inv_small + neat_project2d on the same inputs. */
int neat_line_losses(const float* pred_px, const float* pred_calib, const float* gt5, const float* K, int R, float threshold, float* out3,
                     float* d_pred_calib, float grad_scale, void* stream);

/* ---- a16: Adam step over one flat fp32 parameter buffer = torch.optim.Adam(lr) as the reference trainer builds it
 * (training/volsdf_train.py:177; no weight decay, no amsgrad).  The parameters and both moments are flat [n]; the
 * gradients stay where autograd left them: grads[s] (device pointer, or NULL = no gradient this step: that segment is
 * skipped like torch does) covers elements [seg_offsets[s], seg_offsets[s+1]); seg_steps[s] = 1-based count of the steps
 * that segment has taken including this one (torch counts steps per tensor) -- host arrays, nseg <= 96. */
int neat_adam_step(float* params, NEAT_HOST const float* const* grads, NEAT_HOST const long long* seg_offsets, NEAT_HOST const int* seg_steps, int nseg,
                   float* exp_avg, float* exp_avg_sq, float lr, float beta1, float beta2, float eps, void* stream);
/* ABI v13: neat_adam_step with its step-dependent numbers in DEVICE memory -- coef [2 nseg] = (lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t))
 * per segment -- so that the launch can be captured in the step's HIP graph and replayed; grads[s] == NULL: segment untouched. */
int neat_adam_step_coef(float* params, NEAT_HOST const float* const* grads, NEAT_HOST const long long* seg_offsets, int nseg, float* exp_avg, float* exp_avg_sq,
                        const float* coef, float beta1, float beta2, float eps, void* stream);

/* ---- 8f-2 (next row): device-side rectangular assignment = scipy.optimize.linear_sum_assignment as called at
 * model/networks/neat_wfr_rend_a.py:473 and model/networks/loss_wfr.py:108 (same algorithm, float64 duals, same tie
 * rule => same assignment), without the host round trip.  cost [nr,nc] float32 row-major; row_mask [nr] bytes or NULL
 * (rows with 0 do not take part: replaces the reference's `[good]` compaction); outputs row_ind/col_ind
 * [min(nr,nc)] int64 sorted by row and padded with -1, *n_match = number of pairs (-1 if a cost is not finite). */
size_t neat_lsap_ws_bytes(int nr, int nc);
int neat_lsap(const float* cost, int nr, int nc, const unsigned char* row_mask, const unsigned char* col_mask, long long* row_ind,
              long long* col_ind, int* n_match, void* ws, void* stream);
/* (col_mask [nc] bytes or NULL: columns with 0 do not take part -- padded candidate sets such as the DBSCAN centres below) */

/* DBSCAN(eps, min_samples = 2) + cluster means of n <= 8192 3-D points = VolSDFNetwork.cluster_dbscan
 * (model/networks/neat_wfr_rend_a.py:328-339; sklearn on the host in the reference).  centres: (n/2) x 3 floats followed
 * by n/2 ints of scratch; clusters in sklearn's order (by first member), padded; valid [n/2] bytes; *count = clusters. */
size_t neat_dbscan_ws_bytes(int n);
int neat_dbscan_means(const float* points, int n, double eps, float* centres, unsigned char* valid, int* count, void* ws, void* stream);

/* ---- ABI v15: wireframe parsing of a trained model (code/neat-final-parsing.py: initial_recon :159-302,
 * get_wireframe_from_lines_and_junctions :134-157, visibility_checking :305-336).  fp32, no float atomics, every result bit-identical
 * from run to run.  Sizes that depend on the data (labels present, lines kept, junctions, edges) are written to device memory.
 *
 * neat_parse_match (:226-236): lines2d [n,4] = one view's predicted 2-D lines; row i < n is line i, row n + i its reverse (x2,y2,x1,y1).
 *   gt: m ground-truth lines, row stride gt_stride (>= 4: (x1,y1,x2,y2,...)).  label [2n] int32 = argmin_j |row - gt_j|^2 (lowest j on
 *   ties) if that minimum is < threshold, else -1; mindis [2n] = the minimum (+inf if m = 0; NaN for a row with a NaN distance).
 * neat_parse_group (:237-257): the rows of each label present, in row order: lines [m,2,3] (capacity) receives, in ascending label order,
 *   the mean of the rows' lines3d (rows >= n: the reversed line), scores [m] the mean of |(p - v0) x (p - v1)| / max(|v1 - v0|, 1e-6)
 *   over the same rows (p = the row's l3d [n,3]); *count = L, the labels present.  ws: neat_parse_group_ws_bytes(n, m).
 * neat_parse_vote (:259-272): cost [J, 2 mcap] = |junction - endpoint| (endpoints = lines.reshape(-1,3), the first 2 *count of them),
 *   the assignment of neat_lsap, and one vote per pair with cost < threshold: votes[j] += 1 (votes [J] int32, zeroed by the caller before
 *   the first view); the first vote of a junction stamps first[2j..2j+1] = (view, pair index).  ws: neat_parse_vote_ws_bytes(J, mcap).
 * neat_parse_graph (:278-295, :134-157 with rel_matching_distance_threshold = 0): vlines [V,mcap,2,3], vscores [V,mcap], vcount [V] as
 *   the group calls left them -> lines_out [V mcap,2,3] = the lines with score < score_threshold (view, then label order), junc_out [J,3] =
 *   the junctions with more than one vote in the order of their first vote, graph [J,J] bytes (row stride J; the K x K block is the
 *   reference's 0/1 graph), pairs [ecap,2] int32 + wfi [ecap,2,3] = graph.triu().nonzero() in row-major order (the diagonal included) and
 *   the junctions it names; counts [3] = (N lines, K junctions, E edges).  ws: neat_parse_graph_ws_bytes(V, mcap, J).
 * neat_parse_visibility (:305-336), all views in one launch: lines [ecap,2,3] (the first *n_lines of them, or ecap if n_lines is NULL);
 *   gt: the views' ground-truth lines packed (row stride gt_stride), view v's at rows [gt_off[v], gt_off[v+1]) (gt_off [V+1] int32 on the
 *   device); K3 [V,3,3], w2c [V,3,4] (neat_camera_mats per view).  vis_count [ecap] int32 = views in which the projected line is within
 *   squared distance < ckdist of a ground-truth line in either orientation (a view without ground-truth lines sees nothing); checked
 *   [ecap,2,3] = the lines with vis_count >= ckview, in order, *n_checked of them.  ws: neat_parse_visibility_ws_bytes(ecap, V). */
int neat_parse_match(const float* lines2d, int n, const float* gt, int m, int gt_stride, float threshold, int* label, float* mindis,
                     void* stream);
size_t neat_parse_group_ws_bytes(int n, int m);
int neat_parse_group(const int* label, const float* lines3d, const float* l3d, int n, int m, float* lines, float* scores, int* count,
                     void* ws, void* stream);
size_t neat_parse_vote_ws_bytes(int J, int mcap);
int neat_parse_vote(const float* junctions, int J, const float* lines, const int* count, int mcap, float threshold, int view, int* votes,
                    int* first, void* ws, void* stream);
size_t neat_parse_graph_ws_bytes(int V, int mcap, int J);
int neat_parse_graph(const float* vlines, const float* vscores, const int* vcount, int V, int mcap, float score_threshold,
                     const float* junctions, const int* votes, const int* first, int J, float* lines_out, float* junc_out,
                     unsigned char* graph, int* pairs, float* wfi, int ecap, int* counts, void* ws, void* stream);
size_t neat_parse_visibility_ws_bytes(int ecap, int V);
int neat_parse_visibility(const float* lines, const int* n_lines, int ecap, const float* gt, int gt_stride, const int* gt_off,
                          const float* K3, const float* w2c, int V, float ckdist, int ckview, int* vis_count, float* checked,
                          int* n_checked, void* ws, void* stream);

/* ---- added to ABI v15 (new symbols only, nothing existing changes, so the version number stays): the zero-level surface of the SDF as an indexed triangle mesh (code/utils/plots.py: get_surface_trace :101-138 and
 * get_grid_uniform :318-329; the reference evaluates the grid through PyTorch in 100 000-point chunks and runs skimage's marching cubes
 * on the host).  fp32 / int32, no atomics, fixed-order scans: two runs give the same bytes.  No entry point synchronises with the host.
 *
 * A grid has n[a] >= 2 nodes per axis over [b0[a], b1[a]], fewer than 2^31 nodes in all, x slowest and z fastest; node i of an axis sits
 * at float(b0 + i (b1 - b0) / (n - 1)) evaluated in float64, the last node exactly at b1 (numpy.linspace, :322-324).  n, b0, b1 are HOST
 * arrays of three.
 * neat_grid_points : the points of `count` consecutive nodes from linear node `first_node` into x_fm [3][ldp] (feature-major, ldp >= count;
 *   columns count..ldp are zeroed) = the x rows of a neat_sdf_ws_floats workspace at stride neat_sdf_ldp, ready for
 *   neat_sdf_values_laid_out: no [N,3] point tensor exists.
 * Marching tetrahedra on an fp32 grid [nx][ny][nz] (definitions: neat_amd/csrc/kernels_mesh.hpp).  A node is inside iff
 *   v < level; an edge (7 classes per node: to the node at offset bits (4,2,1) of class + 1) carries one vertex iff its nodes differ in
 *   that and both values are finite, at a + t (b - a), t = (level - va) / (vb - va) from the inside node a; each cell is cut into the six
 *   tetrahedra around its main diagonal; a tetrahedron with a non-finite corner emits nothing.  Vertices ascend by (node, class), faces
 *   by (cell, tetrahedron, triangle); triangle normals point towards increasing values.
 * neat_mesh_ws_bytes : workspace of the two calls below (about 5 bytes per node); 0 for a grid they reject.
 * neat_mesh_count : edge bits per node and the per-tile counts into ws; counts[0] = vertices, counts[1] = faces on the device
 *   (-1, -1 if either exceeds int32).  The caller reads them once, allocates and calls
 * neat_mesh_emit : verts [nv,3] fp32 and faces [nf,3] int32 for the same grid, level and ws; nv, nf as counted (writes beyond them are
 *   dropped).  Bad arguments (an axis under 2 nodes, 2^31 nodes or more, null pointers, a NaN level) return -1 before any launch.
 * neat_unit_rows3 : rows of g [n,3] scaled to unit length in place (vertex normals from the SDF gradient at the vertices). */
int neat_grid_points(float* x_fm, int ldp, long long first_node, int count, NEAT_HOST const int* n, NEAT_HOST const double* b0, NEAT_HOST const double* b1, void* stream);
size_t neat_mesh_ws_bytes(int nx, int ny, int nz);
int neat_mesh_count(const float* grid, int nx, int ny, int nz, float level, void* ws, int* counts, void* stream);
int neat_mesh_emit(const float* grid, int nx, int ny, int nz, NEAT_HOST const double* b0, NEAT_HOST const double* b1, float level, void* ws, float* verts, int nv,
                   int* faces, int nf, void* stream);
int neat_unit_rows3(float* g, int n, void* stream);

/* ---- added to ABI v15 (new symbols only, nothing existing changes, so the version number stays): the evaluation mesh of a checkpoint
 * (code/utils/plots.py: get_surface_high_res_mesh :140-218, get_surface_by_grid :221-316, get_grid :331-362; code/evaluation/eval.py
 * :132-162; the reference samples 10 000 random surface points, aligns a grid to their principal axes, cuts with trimesh's slice_plane
 * and moves to world coordinates on the host).  Definitions: neat_amd/csrc/kernels_evalmesh.hpp, DESIGN 3b.  No atomics, fixed-shape
 * sums: two runs give the same bytes.  No entry point synchronises with the host.  R [3][3], c [3], origin [3], A [3][4] are HOST
 * float64 arrays, row-major.
 * neat_grid_points_affine : neat_grid_points in a frame: node (i, j, k) with local coordinates p (the linspace rule in float64, before
 *   its rounding) goes to x = c + R^T p, x_a = float(c_a + ((R_0a p_0 + R_1a p_1) + R_2a p_2)) with every operation rounded to float64.
 * neat_mesh_moments : out [10] float64 on the device = area, int (x - o) dA [3], int (x - o)(x - o)^T dA (xx, xy, xz, yy, yz, zz) of
 *   the mesh verts [nv,3] fp32, faces [nf,3] int32, exact per triangle, summed over a fixed tree.  A triangle of zero area adds nothing;
 *   one with a non-finite vertex or an index outside [0, nv) adds nothing and sets flag[0] (device int) to 1, else 0.
 *   ws = neat_mesh_moments_ws_bytes(nf) bytes, 8-byte aligned (not read for nf <= 1024).
 * neat_affine_rows3 : rows of v [n,3] fp32 become A [v; 1] in place, evaluated in float64 as ((A_r0 x + A_r1 y) + A_r2 z) + A_r3,
 *   rounded to fp32 once.
 * neat_affine_bounds3 : out [6] float64 on the device = min (3) and max (3) of the same mapped rows in float64; v is not written.
 *   n >= 1; ws = neat_affine_bounds3_ws_bytes() bytes, 8-byte aligned.
 * The cut of a mesh by the half-space sign (x[axis] - value) >= 0 (sign = +1 or -1; value must be a float32 value), in two calls with
 *   integer sorts / scans by the caller in between:
 * neat_mesh_cut_count : fcnt [nf] int32 = triangles each face leaves (0, 1 or 2); ekey [2 nf] int64 = keys a nv + b of its crossing
 *   edges from inside vertex a to outside vertex b (-1: none); used [nv] int32 = 1 for a vertex some surviving face has inside, else 0.
 * neat_mesh_cut_emit : vmap [nv] = exclusive scan of used, foff [nf] = exclusive scan of fcnt, ukey [ncut] = the unique keys >= 0
 *   ascending, nkeep = sum of used -> out_verts [nkeep + ncut, 3] (kept vertices in their order, then one cut vertex per key at
 *   a + t (b - a), t = d_a / (d_a - d_b) in float64, the axis coordinate exactly `value`) and out_faces [nf_out,3], nf_out = sum of fcnt
 *   (by source face, then by emitted triangle; winding kept).  Writes beyond nv_out / nf_out are dropped.
 * Bad arguments return -1 before any launch. */
int neat_grid_points_affine(float* x_fm, int ldp, long long first_node, int count, NEAT_HOST const int* n, NEAT_HOST const double* b0, NEAT_HOST const double* b1,
                            NEAT_HOST const double* R, NEAT_HOST const double* c, void* stream);
size_t neat_mesh_moments_ws_bytes(int nf);
int neat_mesh_moments(const float* verts, int nv, const int* faces, int nf, NEAT_HOST const double* origin, void* ws, double* out, int* flag, void* stream);
int neat_affine_rows3(float* v, int n, NEAT_HOST const double* A, void* stream);
size_t neat_affine_bounds3_ws_bytes(void);
int neat_affine_bounds3(const float* v, int n, NEAT_HOST const double* A, void* ws, double* out, void* stream);
int neat_mesh_cut_count(const float* verts, int nv, const int* faces, int nf, int axis, double value, int sign, int* fcnt, long long* ekey,
                        int* used, void* stream);
int neat_mesh_cut_emit(const float* verts, int nv, const int* faces, int nf, int axis, double value, int sign, const int* used, const int* vmap,
                       const int* foff, const long long* ukey, int ncut, int nkeep, float* out_verts, int nv_out, int* out_faces, int nf_out,
                       void* stream);

/* ---- added to ABI v15 (new symbols only, nothing existing changes, so the version number stays): scoring a reconstruction against
 * ground truth on the device (code/evaluation/eval-dtu.py, eval-lsr-dtu.py, eval-wfr-dtu.py, eval-abc.py; the reference uses an sklearn
 * kd-tree on the host and a sequential thinning loop).  Points are float64 [n,3] row-major; every decision (keep / remove, inside /
 * outside, nearer / farther) compares float64 quantities computed in the reference's order, squared distances as ((dx dx) + dy dy) + dz dz
 * without fused multiply-adds (definitions: neat_amd/csrc/kernels_eval.hpp).  Asynchronous on the stream, no allocation; only
 * integer atomics, and no result depends on their order.  Bad arguments return -1 before any launch.
 *
 * neat_eval_grid_t describes a uniform cell grid over a cloud of n points: the cell of a point is floor((p - origin) / cell) per axis,
 *   clamped into dim; its bucket is the cell's linear index (dense = 1, buckets = dim[0] dim[1] dim[2]) or a hash of the cell modulo
 *   `buckets` (dense = 0).  start [buckets + 1], sidx [n] (the point of every slot) and spts [n,3] (the points in slot order) are the
 *   caller's device arrays; neat_eval_grid fills them (ws: neat_eval_grid_ws_bytes(n, buckets)) and the queries below read them.
 * neat_eval_thin_round : one round of radius thinning in index order (point c stays iff no earlier staying point lies within radius,
 *   <=): state [n] bytes (0 undecided, 1 kept, 2 removed; zeroed by the caller before the first round); every undecided point whose
 *   earlier neighbours are all decided is decided, and the number still undecided is ADDED to *undecided.  Needs radius <= grid->cell.
 *   The caller repeats rounds until a round adds nothing; the lowest undecided point is always decidable, so n rounds suffice.
 * neat_eval_nearest : per query the nearest cloud point (ties: the lowest index) among those within max_dist (widened by 1e-12
 *   relative; the caller takes the `< max_dist` decision): dist [m] = its distance, idx [m] its index; inf and -1 if there is none.
 * neat_eval_obs_mask (eval-dtu.py:98-110): flags [n] bytes, bit 0 = lo <= p < hi on all axes, bit 1 = bit 0 and the voxel
 *   rint((p - bb0) / res) lies inside mask [shape[0]][shape[1]][shape[2]] (bytes) and is non-zero there; f32_quotient = 1 rounds the
 *   quotient to float32 first (eval-lsr-dtu.py:106, eval-wfr-dtu.py:55).  lo, hi, bb0, shape are HOST arrays of three.
 * neat_eval_tri_count / neat_eval_tri_emit (eval-dtu.py:48-71): the lattice samples of every triangle of faces [nf,3] int32 over
 *   verts [nv,3], triangle-major, then i, then j.  count writes *total on the device (-1: a vertex index out of range, a triangle with
 *   more than 30000 lattice steps on a side, or more samples than int32 holds); the caller reads it once, allocates out [total,3] and
 *   calls emit with the same arguments and ws (neat_eval_tri_ws_bytes(nf)).
 * neat_eval_line_cost (eval-abc.py:43, :86-88): cost [n_pred, n_gt]; ends = 1: point sets [n,3], the Euclidean distance; ends = 2:
 *   lines [n,2,3], the lower of the two endpoint orders' mean endpoint distance. */
typedef struct {
  double origin[3];
  double cell;
  int dim[3];
  int buckets;
  int dense;
  int n;
  const int* start;
  const int* sidx;
  const double* spts;
} neat_eval_grid_t;
size_t neat_eval_grid_ws_bytes(int n, int buckets);
int neat_eval_grid(const double* points, NEAT_HOST const neat_eval_grid_t* grid, int* start, int* sidx, double* spts, void* ws, void* stream);
int neat_eval_thin_round(const double* points, NEAT_HOST const neat_eval_grid_t* grid, double radius, unsigned char* state, int* undecided, void* stream);
int neat_eval_nearest(NEAT_HOST const neat_eval_grid_t* grid, const double* queries, int m, double max_dist, double* dist, int* idx, void* stream);
int neat_eval_obs_mask(const double* points, int n, NEAT_HOST const double* lo, NEAT_HOST const double* hi, NEAT_HOST const double* bb0, double res, const unsigned char* mask,
                       NEAT_HOST const int* shape, int f32_quotient, unsigned char* flags, void* stream);
size_t neat_eval_tri_ws_bytes(int nf);
int neat_eval_tri_count(const double* verts, int nv, const int* faces, int nf, double density, void* ws, int* total, void* stream);
int neat_eval_tri_emit(const double* verts, int nv, const int* faces, int nf, double density, void* ws, double* out, int total, void* stream);
int neat_eval_line_cost(const double* pred, int n_pred, const double* gt, int n_gt, int ends, double* cost, void* stream);

/* ---- added to ABI v15 (new symbols only, nothing existing changes, so the version number stays): pictures of a wireframe and of the
 * surface mesh behind it, headless (code/visualization/show.py draws through an open3d window and matplotlib; code/evaluation/show-mesh.py
 * shows the mesh alone).  F frames per call: cams [F,21] float64, per frame K [3,3] then [R|T] [3,4] (world to camera), row-major; of K
 * only fx = K00, fy = K11, cx = K02, cy = K12 are read.  Pixel (row i, column j) has its centre at projected (x, y) = (j, i).  Every
 * geometric decision is float64 with each product and sum rounded on its own (definitions: neat_amd/csrc/kernels_show.hpp, DESIGN 3d;
 * tests/show_f64.py restates them).  Asynchronous on the stream, no allocation; only integer atomics (a 64-bit minimum, a 32-bit maximum),
 * and no result depends on their order.  Bad arguments (F, H or W < 1 or H, W > 32768, null pointers, near <= 0, a negative width or
 * radius, hidden_alpha outside [0, 1], a colour outside [0, 1], an output that is not 4-byte aligned) return -1 before any launch.
 *
 * neat_show_ws_bytes / neat_show_ws_layout : the workspace of (F, H, W) and the byte offsets of its four parts: offsets[0] the depth
 *   keys, uint64 [F,H,W] = bits(float32 depth) << 32 | winning triangle (0x7f800000ffffffff where no triangle covers); [1] the line
 *   coverage and [2] the point coverage, float32 [F,H,W]; [3] one int32 status word (1: a face index out of range), followed by the
 *   mesh pass's own queue of large triangles.
 * neat_show_clear   : keys to "nothing", coverages and status to 0.
 * neat_show_mesh    : verts [nv,3] float64, faces [nf,3] int32; per pixel centre inside a triangle (edges inclusive, both windings) the
 *   minimum key.  A triangle with a vertex nearer than `near`, of zero screen area or with a non-finite coordinate is dropped; a face
 *   index out of range sets the status word, and neat_show_resolve then writes nothing (the caller reads the word once).
 * neat_show_lines   : lines [n,2,3] float64; coverage clamp(width / 2 + 0.5 - distance, 0, 1) times (visible ? 1 : hidden_alpha), the
 *   maximum over the segments; visible iff the segment's perspective-correct depth at the pixel <= the key's depth + bias.  Segments are
 *   cut at z = near.  Call after neat_show_mesh on the same stream.
 * neat_show_points  : points [n,3] float64 as discs of radius + 0.5 - distance, the same visibility rule.
 * neat_show_resolve : out [F,H,W,3] bytes; colors = HOST array of twelve: background, line, point, mesh rgb in [0, 1]. */
size_t neat_show_ws_bytes(int F, int H, int W);
int neat_show_ws_layout(int F, int H, int W, NEAT_HOST size_t* offsets);
int neat_show_clear(void* ws, int F, int H, int W, void* stream);
int neat_show_mesh(const double* verts, int nv, const int* faces, int nf, const double* cams, int F, int H, int W, double near, void* ws,
                   void* stream);
int neat_show_lines(const double* lines, int n, const double* cams, int F, int H, int W, double near, double width, double bias,
                    double hidden_alpha, void* ws, void* stream);
int neat_show_points(const double* points, int n, const double* cams, int F, int H, int W, double near, double radius, double bias,
                     double hidden_alpha, void* ws, void* stream);
int neat_show_resolve(const double* verts, int nv, const int* faces, int nf, const double* cams, int F, int H, int W, NEAT_HOST const double* colors,
                      void* ws, unsigned char* out, void* stream);

/* ---- added to ABI v15 (new symbols only, so the version number stays): the frame side of rendering whole views of a checkpoint
 * (code/evaluation/eval.py --eval_rendering and the trainer's do_vis pictures assemble, quantise and average on the host).  Definitions:
 * neat_amd/csrc/kernels_frame.hpp; tests/render_f64.py restates them.  All arithmetic is IEEE float32 with one rounding per
 * step unless said otherwise.  Asynchronous on the stream, no allocation, no float atomics: two runs give the same bytes.  Bad arguments
 * return -1 before any launch.
 *
 * neat_frame_put   : the ONE launch per chunk.  rgb [n,3], normal [n,3], depth [n]: a chunk's outputs for the frame pixels p0 .. p0+n-1
 *   of a frame of P pixels; each may be null.  Writes rgb8 [P,3] = byte(rgb) (if rgb8 is not null), normal8 [P,3] = byte((normal + 1) / 2),
 *   depth_out [P] = depth and, with gt [P,3], err [P,3] = (rgb - gt)^2; nothing outside the chunk's pixels.
 *   byte(x) = clamp(trunc(255 x), 0, 255), 0 for a NaN.  -1 for n < 0, p0 < 0, p0 + n > P, or an input without its output.
 * neat_frame_sum   : out[0] = the float64 sum of x [n] float32 over a fixed 256-ary tree (independent of any launch geometry);
 *   ws = neat_frame_sum_ws_bytes(n) bytes, 8-byte aligned (not read for n <= 256).
 * neat_frame_range : range[0], range[1] = the minimum and maximum of the finite values of x [n], (0, 0) if there is none, left in device
 *   memory; ws = neat_frame_range_ws_bytes() bytes.
 * neat_frame_grey  : out [n] bytes = clamp(trunc((255 (x - lo)) / (hi - lo)), 0, 255) with (lo, hi) = range[0..1] read on the device;
 *   0 where x is not finite or hi == lo.
 * neat_frame_grid  : images [N,H,W,3] bytes onto the canvas of torchvision.utils.make_grid(nrow, padding = 2, pad_value = 0):
 *   xmaps = min(nrow, N), ymaps = ceil(N / xmaps), canvas [(ymaps (H + 2) + 2), (xmaps (W + 2) + 2), 3], image k at row
 *   (k / xmaps)(H + 2) + 2 and column (k % xmaps)(W + 2) + 2, zeros elsewhere; N = 1: the canvas is the image, unpadded. */
int neat_frame_put(const float* rgb, const float* normal, const float* depth, const float* gt, int n, long long p0, long long P,
                   unsigned char* rgb8, unsigned char* normal8, float* depth_out, float* err, void* stream);
size_t neat_frame_sum_ws_bytes(long long n);
int neat_frame_sum(const float* x, long long n, void* ws, double* out, void* stream);
size_t neat_frame_range_ws_bytes(void);
int neat_frame_range(const float* x, long long n, void* ws, float* range, void* stream);
int neat_frame_grey(const float* x, long long n, const float* range, unsigned char* out, void* stream);
int neat_frame_grid(const unsigned char* images, int N, int H, int W, int nrow, unsigned char* canvas, void* stream);

/* ---- added to ABI v15 (new symbols only, so the version number stays): sphere tracing of an SDF along rays (neat_amd/trace.py).  The
 * SDF is queried by the caller between these launches (the raw network: neat_sdf_forward with radius 0, or any field); these are the
 * per-ray state machine and the ordered compaction of the rays that still need a query.  Definitions: neat_amd/csrc/kernels_trace.hpp,
 * DESIGN 3f; tests/trace_f64.py restates them in float64.  Asynchronous on the stream, no allocation, no atomics: two runs give the same
 * lists and the same bytes.  Bad arguments return -1 before any launch.  States: 0 MISS, 1 HIT, 2 INSIDE, 3 UNCONVERGED.
 *
 * ws = neat_trace_ws_bytes(R) bytes (0 for R < 1 or R > 2^24: the scan of the per-workgroup counts is one workgroup walking
 * ceil(R / 256) entries, 64 rounds at the cap; trace more rays in chunks, as neat_amd.trace.rays does), 256-byte aligned, kept from init to finish.  ctl: two int64 in device memory, ctl[0] = the
 * length of the current active list, ctl[1] = the evaluations asked for so far (the sum of those lengths).  The caller reads ctl[0]
 * after init and after every step, queries the SDF at points [ctl[0], 3] (row-major; `points` needs room for R rows) and hands the
 * values to the next step, with parity 0 for the first step and alternating from there; it stops at ctl[0] = 0.
 * neat_trace_list_offset : the byte offset in ws of active list `parity` (int32 ray ids; the list the step with that parity reads);
 *   0 for bad arguments (no list starts at 0).
 * neat_trace_init   : origins, dirs [R,3] (|dir| = 1), t_end [R] or null; the sphere chord and its clip to [near, t_end] in float64,
 *   the first state, the first active list (ray order) and its query points.
 * neat_trace_step   : values [n] of the current list's points, n <= R (entries past the device's own count are ignored); advances
 *   each ray, writes the next list (ray order kept), its points and ctl.
 * neat_trace_finish : depth [R] (NaN unless HIT or INSIDE), state [R] bytes, steps [R] (queries made per ray), hit_points [R,3] (NaN rows
 *   likewise); each may be null.  A ray still active reads UNCONVERGED.
 * neat_trace_target_rays : the rays from F centres [F,3] towards N x S targets: target (n, j) = a + j / (S - 1) (b - a) of row n =
 *   [a | b] (`stride` >= 6 floats per row; S = 1: the point a, stride >= 3), float64 arithmetic.  Ray (f N + n) S + j: origin the
 *   centre, unit direction, t_end = |p - c| - bias, ok = 1 iff |p| <= radius and |p - c| >= near + bias. */
size_t neat_trace_ws_bytes(int R);
size_t neat_trace_list_offset(int R, int parity);
int neat_trace_init(const float* origins, const float* dirs, const float* t_end, int R, double radius, double near, void* ws, float* points,
                    long long* ctl, void* stream);
int neat_trace_step(const float* origins, const float* dirs, const float* values, int n, int R, int parity, float eps, float relax,
                    int max_steps, int refine_steps, void* ws, float* points, long long* ctl, void* stream);
int neat_trace_finish(const float* origins, const float* dirs, int R, void* ws, float* depth, unsigned char* state, int* steps,
                      float* hit_points, void* stream);
int neat_trace_target_rays(const float* centres, int F, const float* rows, int stride, int N, int S, double radius, double near, double bias,
                           float* origins, float* dirs, float* t_end, unsigned char* ok, void* stream);

/* ---- added to ABI v15 (new symbols only): fuse, refine and snap of a parsed line soup against the views' 2-D detections
 * (code/evaluation/fusion.py :79-141, refinement.py :95-198, nms.py :156-204; neat_amd/post.py).  fp32, no atomics, fixed-shape
 * reductions: two runs give the same bytes.  No entry point synchronises with the host; counts that depend on the data are device memory.
 *
 * Shared inputs: lines [n,2,3]; det = the views' detections packed, row stride det_stride floats (x1, y1, x2, y2, score, ...), view v's at
 * rows [det_off[v], det_off[v+1]) (det_off [V+1] int32 on the device, mtot rows in all); K3 [V,3,3], w2c [V,3,4] (neat_camera_mats).
 * A line's cost in a view = min over the detections and both orientations of the squared 4-vector distance of its projection
 * (lowest detection on ties; a row with a NaN distance never matches; a view without detections sees nothing).
 *
 * neat_post_fuse, all views in one launch: a line is available in a view if its cost < dis_threshold.  It then receives the score
 *   (det column 4) of detection number r of that view, r = the RANK of its detection among the detections matched in that view
 *   (by_label = 0, the reference's enumerate) or r = its detection (by_label = 1), summed in view order; count [n] int32 = views that saw
 *   it, score [n] = sum / max(count, 1), keep [n] bytes = score > keep_threshold, kept [n,2,3] = those lines in order, *n_kept of them.
 *   ws: neat_post_fuse_ws_bytes(n, V, mtot).
 * neat_post_select: out [n,2,3] = the lines with keep[i] != 0, in order, *n_out of them (refine's pre-filter).  ws: n ints.
 * neat_post_refine_view, one view of the sequential walk: cur [ncap,2,3] holds *n_cur lines.  A line is possible if its projection lies
 *   in [0,width] x [0,height] (inclusive) and its cost < dis_threshold; it is reversed if the reversed orientation is strictly the closer at
 *   its detection.  next [ncap,2,3] = the lines that are not possible, in order, then the mean of the (reversed) members of every matched
 *   detection in ascending detection order (neat_parse_group's grouping and means); *n_next <= *n_cur.  m = the view's detections
 *   (<= mmax, the bound ws was sized with).  ws: neat_post_refine_ws_bytes(ncap, mmax).
 * neat_post_snap: end points -> cells of a G^3 grid over their bounding box (2 <= G <= 1024, anything else is refused before any
 *   launch): delta = (max - min) / (G - 1), cell = rint((p - min) / delta) (IEEE division, half to even; a zero-extent axis has cell 0).
 *   A cell is a peak if it holds at least as many end points as every cell of its 3x3x3 neighbourhood inside the grid; junctions [2n,3]
 *   (capacity) = the peaks in row-major (ix, iy, iz) order at the nodes of torch.linspace(min, max, G) (lo + step i below the middle,
 *   hi - step (G - 1 - i) from it on, fused multiply-adds), pcount [2n] their end points.  Every end point snaps to the nearest peak (squared
 *   distance, lowest index on ties).  edges [n,2] int32 / lines_out [n,2,3] = junctions[edges]: the lines whose two end points moved less
 *   than max_snap (max_snap < 0: all), in line order; with unique = 1 the distinct pairs (min, max) with min != max, ascending.
 *   counts [2] = (peaks, edges).  ws: neat_post_snap_ws_bytes(n, G) (0 for a refused G). */
size_t neat_post_fuse_ws_bytes(int n, int V, int mtot);
int neat_post_fuse(const float* lines, int n, const float* det, int det_stride, const int* det_off, int mtot, const float* K3, const float* w2c,
                   int V, float dis_threshold, float keep_threshold, int by_label, float* score, int* count, unsigned char* keep, float* kept,
                   int* n_kept, void* ws, void* stream);
int neat_post_select(const float* lines, int n, const unsigned char* keep, float* out, int* n_out, void* ws, void* stream);
size_t neat_post_refine_ws_bytes(int ncap, int mmax);
int neat_post_refine_view(const float* cur, const int* n_cur, int ncap, const float* det, int det_stride, const int* det_off, int m, int mmax,
                          const float* K3, const float* w2c, int view, float dis_threshold, float width, float height, float* next, int* n_next,
                          void* ws, void* stream);
size_t neat_post_snap_ws_bytes(int n, int G);
int neat_post_snap(const float* lines, int n, int G, float max_snap, int unique, float* junctions, int* pcount, int* edges, float* lines_out,
                   int* counts, void* ws, void* stream);

/* ---- added to ABI v15 (new symbols only, so the version number stays): ray casting against an indexed triangle mesh
 * (neat_amd/raycast.py; what open3d's RaycastingScene.cast_rays answers in code/evaluation/abc-analysis.py :44-56).  The rule of
 * intersection (Woop, Benthin, Wald 2013, decided in float64, both windings, edges inclusive, ties in t to the lowest face index), the
 * tree and the walk: neat_amd/csrc/kernels_raycast.hpp; tests/raycast_f64.py restates them in float64.  The result is the
 * brute-force minimum over all triangles under that rule.  Asynchronous on the stream, no allocation, no atomics: two runs give the
 * same bytes.  Bad arguments return -1 before any launch.
 *
 * neat_raycast_bvh_bytes / neat_raycast_ws_bytes : the sizes of the tree and of the build's workspace for nf faces, both 256-byte
 *   aligned caller-owned device memory; 0 for nf < 0 or nf > 2^24 (bvh_bytes(0) > 0: the empty tree).  ws is free after the build.
 * neat_raycast_build : verts [nv,3] float64, faces [nf,3] int32 (as neat_show_mesh takes them).  Triangles are sorted by the Morton key of
 *   their centroid (rocprim radix sort) into the implicit complete binary tree over a power of two of leaves, float32 boxes rounded
 *   outwards; a triangle with a non-finite vertex or zero area is never hit.  A face index outside [0, nv) is found before any vertex
 *   is read: the first int32 of bvh (the status word, 0 otherwise) becomes 1 and the tree is empty, so every cast misses.
 * neat_raycast_cast : origins, dirs [R,3] float32 (any length of dir; t is in units of it), t_min, t_max [R] or null (0 and +inf); a hit
 *   has t_min <= t < t_max.  any_hit = 0: the closest hit; 1: the first accepted hit the walk meets (visibility).  t [R] (+inf on a
 *   miss), tri [R] the original face index (-1 on a miss), uv [R,2] barycentrics (hit = (1 - u - v) v0 + u v1 + v v2; 0 on a miss),
 *   counts [R,2] uint32 (node boxes tested, triangles tested) or null.  nf = the build's. */
size_t neat_raycast_bvh_bytes(int nf);
size_t neat_raycast_ws_bytes(int nf);
int neat_raycast_build(const double* verts, int nv, const int* faces, int nf, void* bvh, void* ws, void* stream);
int neat_raycast_cast(const void* bvh, int nf, const float* origins, const float* dirs, const float* t_min, const float* t_max, int R, int any_hit,
                      float* t, int* tri, float* uv, unsigned* counts, void* stream);

/* ---- added to ABI v15 (new symbols only, so the version number stays): the closest point on the mesh of a tree that neat_raycast_build
 * made (neat_amd/raycast.py closest, line_distance; what open3d's and sklearn's nearest-neighbour queries against the vertices of the
 * ground-truth mesh stand in for in code/evaluation/eval-lsr-scannet.py).  The rule (Ericson, Real-Time Collision Detection 5.1.5,
 * decided in float64 without fused multiply-adds, ties in the squared distance to the lowest face index), the bound of the walk and
 * its argument: neat_amd/csrc/kernels_closest.hpp; tests/closest_f64.py restates the rule in float64.  The result is the
 * brute-force minimum over all triangles under that rule.  Asynchronous on the stream, no workspace, no allocation, no atomics: two
 * runs give the same bytes.
 *
 * neat_raycast_closest : bvh, nf as neat_raycast_cast takes them; points [N,3] float64; a triangle is accepted iff its squared
 *   distance is <= max_d2 (inclusive; +inf: no bound).  d2 [N] the squared distance (+inf on a miss), tri [N] the original face index
 *   (-1 on a miss), point [N,3] the closest point and uv [N,2] its barycentrics (point = (1 - u - v) v0 + u v1 + v v2; both 0 on a
 *   miss), counts [N,2] uint32 (node boxes tested, triangles tested) or null.  A query with a non-finite coordinate, the empty tree and
 *   the tree of a refused build (status 1) give misses.  Returns -1 before any launch for N < 0, nf outside the build's range, max_d2
 *   negative or NaN, or a null bvh, points, d2, tri, point or uv with N > 0. */
int neat_raycast_closest(const void* bvh, int nf, const double* points, int N, double max_d2, double* d2, int* tri, double* point, double* uv,
                         unsigned* counts, void* stream);

/* ---- added to ABI v15 (new symbols only, so the version number stays): 2-D line segments of the views (neat_amd/detect.py), the
 * files <scene>/<line_detector>/<image>.json that the datasets read.  An a-contrario detector of the LSD family over the line-support
 * regions of Burns, Hanson and Riseman; the rule: DESIGN 3j and neat_amd/csrc/kernels_detect.hpp, restated in float64 by
 * tests/detect_f64.py.  Asynchronous on the stream, no allocation, no read-back; integer atomics only and fixed-order float64 sums:
 * two runs give the same bytes.  Bad arguments return -1 before any launch.
 *
 * neat_detect_label : codes uint8 [V,h,w] (255 = unused, any other value a code) -> labels int32 [V,h,w]: the smallest linear index
 *   y w + x of the pixel's 8-connected component of equal code within its picture, -1 for unused.  The labelling step of the detector
 *   on its own.  Refused: a negative count, h w or V h w beyond 2^31 - 1.
 * neat_detect_scratch_bytes : the workspace of neat_detect_lines (256-byte aligned, caller-owned); 0 when refused: V < 0, H or W below
 *   2 with V > 0 or above 32768, scale outside (0, 1], min_reg < 1, more than 2^31 - 1 map elements.  The grey picture float64
 *   [V, Hs, Ws], Hs = ceil(scale H), is its first region, at offset 0.
 * neat_detect_lines : images uint8 [V,H,W,channels], channels 3 (grey = (77 R + 150 G + 29 B + 128) >> 8) or 1.  scale < 1: a sampled
 *   Gaussian from the host's tables taps_x [Ws][ntaps], taps_y [Hs][ntaps] (ntaps odd; the first tap of output i at source
 *   floor(i / scale + 0.5) - (ntaps - 1) / 2, sources clamped); scale = 1: ntaps = 0 and no tables.  The host's constants: rho2 =
 *   (q / sin tau)^2 the squared gradient threshold, c1 = sqrt(2) - 1, cos_tau, density (0.7), logNT = 2.5 (log10 Ws + log10 Hs),
 *   p = tau / 180 deg, min_reg = floor(-logNT / log10 p) + 1.  Outputs, `cap` rows each with cap >= 2 V ((Hs - 1) (Ws - 1) / min_reg) + 1:
 *   lines float64 [cap,4] (x1 y1 x2 y2 in the input picture's integer-pixel-centre coordinates), width, nfa (-log10 NFA) float64 [cap],
 *   n, k int32 [cap] (positions in the rectangle, aligned ones), in ascending (view, partition, label) order; offsets int32 [V + 1]:
 *   the lines of view v are rows offsets[v] .. offsets[v + 1].  V = 0 or a picture without a gradient grid: offsets all zero. */
int neat_detect_label(const unsigned char* codes, int V, int h, int w, int* labels, void* stream);
size_t neat_detect_scratch_bytes(int V, int H, int W, double scale, int min_reg);
int neat_detect_lines(const unsigned char* images, int V, int H, int W, int channels, double scale, const double* taps_x, const double* taps_y,
                      int ntaps, double rho2, double c1, double cos_tau, double density, double logNT, double p, int min_reg, void* ws, int cap,
                      double* lines, double* width, double* nfa, int* n, int* k, int* offsets, void* stream);

/* ---- added to ABI v15 (new symbols only, so the version number stays): 3-D line segments triangulated from the views' 2-D segments
 * (neat_amd/triangulate.py), the baseline the reference takes from Line3D++ files.  The rule: DESIGN 3k and
 * neat_amd/csrc/kernels_triangulate.hpp, restated in float64 by tests/triangulate_f64.py.  Float64 without contraction, counted /
 * scanned / filled lists, a union-find whose roots are the smallest member: two runs give the same bytes.  Asynchronous on the stream,
 * no allocation, no read-back.  Bad arguments return -1 before any launch.
 *
 * Shared inputs: segments float64 [S,4] = x1 y1 x2 y2 in pixels, all views' in (view, index) order; segoff int32 [V+1] the views' first
 * rows; nmax = the most segments of one view; nb int32 [V,M] the M nearest other views of a view, nearest first (M < V, or M = 0);
 * cam float64 [V,48] = K^-1 [9], R [9] world -> camera, t [3], K [9], P = K [R|t] [12], C [3], 3 unused, all row-major.
 * Refused: a negative count, V > 65535, 10 S, S M or V M ceil(nmax / 256) beyond 2^31 - 1, M >= V > 0, nmax > S, H beyond 2^30 - 1.
 *
 * neat_tri_scratch_bytes : the workspace (256-byte aligned, caller-owned) of the three calls, which share it; 0 when refused.
 * neat_tri_count : the per-segment constants, then the pair test over every (segment, segment of a neighbour) once, counting.
 *   cos_min = cos(angle_min), overlap_min as in the rule.  view int32 [S] = the segment's view; hoff int32 [S+1] = the segments' first
 *   hypotheses; *total (device, 64-bit) = the number of hypotheses H, which the host reads to allocate the list.
 * neat_tri_fill : the same test again, writing the H hypotheses in (view, segment, slot, partner) order: hyp_m int32 [H] the slot,
 *   hyp_j int32 [H] the partner's index in its view, hyp_s float64 [H,2] the depths s_1, s_2.  Same arguments as the count.
 * neat_tri_lines : score, link and lines.  Per segment: estimate float64 [S,2,3] (zeros without a hypothesis), score float64 [S],
 *   kept int32 [S] (score >= min_score), label int32 [S] (the component's lowest kept segment, -1 when not kept), members int32 [S]
 *   (the segment's line, -1 for none).  Per line, in label order: lines3d float64 [S,2,3], views int32 [S], support float64 [S]
 *   (capacity S each), *n_lines (device) of them. */
size_t neat_tri_scratch_bytes(int V, int S, int M, int nmax);
int neat_tri_count(const double* segments, const int* segoff, int V, int S, int nmax, const int* nb, int M, const double* cam, double cos_min,
                   double overlap_min, void* ws, int* view, int* hoff, long long* total, void* stream);
int neat_tri_fill(const int* segoff, int V, int S, int nmax, const int* nb, int M, const double* cam, double cos_min, double overlap_min,
                  void* ws, long long H, int* hyp_m, int* hyp_j, double* hyp_s, void* stream);
int neat_tri_lines(const int* segoff, int V, int S, int nmax, const int* nb, int M, const double* cam, void* ws, const int* view, const int* hoff,
                   long long H, const int* hyp_m, const int* hyp_j, const double* hyp_s, double sigma_px, double min_score, int min_views,
                   double* estimate, double* score, int* kept, int* label, int* members, double* lines3d, int* views, double* support,
                   int* n_lines, void* stream);

/* ---- added to ABI v15 (new symbols only, so the version number stays): a training scene from a mesh and its wireframe
 * (neat_amd/scenegen.py): shaded anti-aliased pictures of the mesh and the visible runs of the ground-truth edges, view by view.  Both
 * walk the tree of neat_raycast_build with its rule, in float64; the rule: DESIGN 3l and neat_amd/csrc/kernels_scenegen.hpp, restated
 * in float64 by tests/scenegen_f64.py, which the device equals byte for byte.  Asynchronous on the stream (but for the one copy of the
 * count call), no allocation, no read-back.  Bad arguments return -1 before any launch.
 *
 * Shared inputs: bvh, nf as neat_raycast_cast takes them; K float64 [V,3,3] and pose float64 [V,4,4], camera-to-world, both row-major.
 * Refused: V > 65535, H or W outside [1, 32768], V ceil(H / 16) ceil(W / 16) beyond 2^31 - 1.
 *
 * neat_scenegen_shade : rgb uint8 [V,H,W,3] and mask uint8 [V,H,W] (255 where a sub-sample hit).  ss x ss sub-samples a pixel,
 *   1 <= ss <= 16; albedo, ambient, background finite.
 * neat_scenegen_scratch_bytes : the workspace (256-byte aligned, caller-owned) that the two edge calls share; 0 when refused
 *   (a negative count, 8 E or 4 V E beyond 2^31 - 1).
 * neat_scenegen_edge_count : junctions float64 [J,3] on the device; edges int32 [E,2] ON THE HOST: the indices are checked there
 *   (each in [0, J)) and the list is copied into the workspace on the stream; the call waits for that copy, so the list may be freed
 *   when it returns.  step > 0 pixels between samples, a run is kept when its 2-D length
 *   is >= min_len, bias >= 0, near > 0.  Refused as well: ceil(sqrt(W^2 + H^2) / step) + 2 > 65536, the samples the longest edge a
 *   picture can hold would need.  *total (device, 64-bit) = the number of runs N, which the host reads to allocate the list.
 * neat_scenegen_edge_fill : the same pass again with the same arguments and the workspace of the count, writing the N runs in
 *   (view, edge, run) order: idx int32 [N,4] = view, edge, first and last sample; p2 float64 [N,4] = x1 y1 x2 y2 in the picture;
 *   p3 float64 [N,2,3] the ends in the world; junc uint8 [N,2]: the end is the edge's own junction, not a cut. */
size_t neat_scenegen_scratch_bytes(int V, int E);
int neat_scenegen_shade(const void* bvh, int nf, const double* K, const double* pose, int V, int H, int W, int ss, double albedo, double ambient,
                        double background, unsigned char* rgb, unsigned char* mask, void* stream);
int neat_scenegen_edge_count(const void* bvh, int nf, const double* junctions, int J, NEAT_HOST const int* edges, int E, const double* K, const double* pose,
                             int V, int H, int W, double step, double min_len, double bias, double near, void* ws, long long* total, void* stream);
int neat_scenegen_edge_fill(const void* bvh, int nf, const double* junctions, int J, int E, const double* K, const double* pose, int V, int H, int W,
                            double step, double min_len, double bias, double near, void* ws, long long N, int* idx, double* p2, double* p3,
                            unsigned char* junc, void* stream);

/* ---- added to ABI v15 (new symbols only, so the version number stays): the crease lines of a triangle mesh (neat_amd/creases.py):
 * the junctions and straight edges of a model read from its triangles, the lines.json that scenegen, raycast analysis and evaluate abc
 * start from.  The rule: DESIGN 3n and neat_amd/csrc/kernels_crease.hpp, restated in float64 by tests/creases_f64.py, which the device
 * equals array for array.  Float64 products and sums without contraction, no division or square root; stable sorts, scans and one
 * union-find whose roots are the smallest member: two runs give the same bytes.  No allocation.  Each call reads a few words back
 * from the workspace (so it waits for the stream once); bad arguments return -1 before any launch, -2: the sort wants more temporary
 * storage than the workspace holds.
 *
 * neat_crease_scratch_bytes : the workspace (256-byte aligned, caller-owned) that the three calls share, fixed by (nv, nf); 0 when
 *   refused: a negative count, nv > 2^26, nf > 2^24.
 * neat_crease_edges : verts float64 [nv,3], faces int32 [nf,3]; cos_angle = cos(angle) in (-1, 1); boundary 0 / 1: keep the edges of
 *   one face.  counts int32 [8] on the device: [0] status (0; 1 a face index outside the vertices; 2 a non-finite coordinate: nothing
 *   else is then made), [1] welded vertices, [2] dropped faces, [3] feature edges E, [4..6] E of kind 0 crease, 1 boundary, 2
 *   non-manifold.
 * neat_crease_chains : E as the edges call counted it (-1 otherwise); sin2_turn = sin^2(turn) in [0, 1]; dev >= 0 the deviation as a
 *   length.  counts int32 [4] on the device: [0] chains, [1] lines, [2] junctions.
 * neat_crease_fill : E, n_lines, n_junc as the two calls counted them (-1 otherwise).  junctions float64 [n_junc,3] the coordinates as
 *   given, vertex int32 [n_junc] the original index (the lowest of its welded group), ascending; lines int32 [n_lines,2] into that list,
 *   in ascending (vertex a, vertex b), then kind, then curved; kind uint8 [n_lines]; curved uint8 [n_lines]: a piece of a chain that is
 *   not one straight line. */
size_t neat_crease_scratch_bytes(int nv, int nf);
int neat_crease_edges(const double* verts, int nv, const int* faces, int nf, double cos_angle, int boundary, void* ws, int* counts, void* stream);
int neat_crease_chains(const double* verts, int nv, int nf, int E, double sin2_turn, double dev, void* ws, int* counts, void* stream);
int neat_crease_fill(const double* verts, int nv, int nf, int E, void* ws, int n_lines, int n_junc, double* junctions, int* vertex, int* lines,
                     unsigned char* kind, unsigned char* curved, void* stream);

/* ---- added to ABI v15 (new symbols only, so the version number stays): 2-D wireframes with shared junctions from the views' detected
 * segments (neat_amd/detect.py junctions): ends that meet near the crossing of their lines become one junction, a lone end that stops
 * at another segment's inside becomes a T, duplicate and collapsed segments are dropped.  The rule: DESIGN 3o and
 * neat_amd/csrc/kernels_wireframe2d.hpp, restated in float64 by tests/junctions2d_f64.py, which the device equals byte for byte.
 * Float64 without contraction, no transcendental function; a union-find whose roots are the smallest member, counted, scanned and
 * filled lists: two runs give the same bytes.  All views in one set of nine launches whose count does not depend on the data;
 * asynchronous on the stream, no allocation, no read-back.  Bad arguments return -1 before any launch.
 *
 * neat_wf2d_scratch_bytes : the workspace (256-byte aligned, caller-owned); 0 when refused: a negative count, V > 65535, nmax > S,
 *   segments without a view or with nmax = 0, 10 S or V ceil(nmax / 256) beyond 2^31 - 1.
 * neat_wf2d_build : segments float64 [S,4] = x1 y1 x2 y2 in (view, index) order, segoff int32 [V+1] ascending from 0 to S, weight
 *   float64 [S] (finite).  nmax: no view holds more segments (any upper bound up to S; it sizes the grids).  gap > 0 pixels,
 *   0 < frac < 0.5, 0 < sin_min <= 1 the sine of the least angle between two lines that may cross, t_junctions 0 / 1.
 *   Per vertex, capacity 2 S, the views one after the other, each in ascending order of the vertex's lowest endpoint (end k of segment i
 *   is endpoint 2 i + k): vertices float64 [.,2], degree int32 (ends joined), kind int32 (0 a free end, 1 a junction, 2 a T), score
 *   float64 (the largest weight of its segments), spread float64 (the largest distance from the vertex to an end it replaces), t_edge
 *   int32 (kind 2: the segment it stands on, numbered in its view; else -1); voff int32 [V+1] the views' first vertices, voff[V] the count.
 *   ends int32 [S,2]: the vertex of each end, numbered in its view.  Per edge, capacity S, in segment order: edges int32 [.,2] (vertices
 *   numbered in the view), eweight float64, esrc int32 (the segment, numbered in its view); eoff int32 [V+1]. */
size_t neat_wf2d_scratch_bytes(int V, int S, int nmax);
int neat_wf2d_build(const double* segments, const int* segoff, const double* weight, int V, int S, int nmax, double gap, double frac, double sin_min,
                    int t_junctions, void* ws, double* vertices, int* degree, int* kind, double* score, double* spread, int* t_edge, int* voff,
                    int* ends, int* edges, double* eweight, int* esrc, int* eoff, void* stream);

/* ---- added to ABI v15 (new symbols only, so the version number stays): 3-D wireframes with shared junctions from the triangulated
 * lines and the views' 2-D graphs (neat_amd/triangulate.py wireframe): a 3-D line end inherits the 2-D vertices of its member segments'
 * ends; ends of different lines that share a 2-D vertex in min_votes views and whose lines nearly cross there become one junction at
 * the least-squares point of their lines; collapsed and duplicate lines are dropped.  The rule: DESIGN 3p and
 * neat_amd/csrc/kernels_wireframe3d.hpp, restated in float64 by tests/wireframe3d_f64.py, which the device equals byte for byte.
 * Float64 without contraction, no transcendental function; sorted keys that are counted, scanned and filled, a union-find whose roots
 * are the smallest member: two runs give the same bytes.  Asynchronous on the stream, no allocation, no read-back.  Bad arguments
 * return -1 before any launch; -2: a sort wants more temporary storage than the workspace holds (before any launch too).
 *
 * neat_wf3d_scratch_bytes : the workspace (256-byte aligned, caller-owned) with room for pairs_max votes; 0 when refused: a negative
 *   count, V > 65535, 2 N >= 2^24, 6 S, NV or pairs_max beyond 2^31 - 1, segments without a view or a 2-D vertex.
 * neat_wf3d_build : lines3d float64 [N,2,3], support float64 [N] (finite), members int32 [S] (the line of each 2-D segment, -1 for
 *   none), estimate float64 [S,2,3] (the 3-D point of each segment end), as neat_tri_lines gives them; endv int32 [S,2] the 2-D vertex
 *   of each segment end, numbered over all views in [0, NV), a vertex in one view only; view int32 [S].  0 < end_frac < 0.5: how far
 *   from a line's end, as a share of its length, a segment end may lie and still be that end; 0 < reach <= 1: how far from its end,
 *   likewise, a line may cross another, and how far apart the two may pass; 0 < sin_min <= 1 the sine of the least angle between two
 *   lines that may cross; min_votes >= 1.  An entry of members, endv or view outside its range carries nothing.
 *   Per vertex, capacity 2 N, in ascending order of the vertex's lowest end id (end e of line L is 2 L + e): vertices float64 [.,3],
 *   degree int32 (ends joined), kind int32 (0 a free end, at the line's own end point; 1 a junction), votes int32 (the most views that
 *   voted for one of its links), spread float64 (the largest distance from the vertex to an end it replaces); n_vertices int32 [1].
 *   Per edge, capacity N, in line order: edges int32 [.,2] (the vertices of the line's ends 0 and 1), esrc int32 (the line);
 *   n_edges int32 [1].  When the views cast more votes than pairs_max, n_vertices is -1 and n_edges the room to ask for. */
size_t neat_wf3d_scratch_bytes(int V, int S, int N, int NV, long long pairs_max);
int neat_wf3d_build(const double* lines3d, const double* support, int N, const int* members, const double* estimate, const int* endv, const int* view,
                    int V, int S, int NV, long long pairs_max, double end_frac, double reach, double sin_min, int min_votes, void* ws, double* vertices,
                    int* degree, int* kind, int* votes, double* spread, int* n_vertices, int* edges, int* esrc, int* n_edges, void* stream);

/* ---- a9 alone: volume_rendering :540-554 given sdf [R,S] -> weights [R,S] (used by tests) -------- */
int neat_volume_weights(const float* z, const float* sdf, int R, int S, const float* beta, float* weights, void* stream);

/* ---- measurement support (bench.py): when enabled, every launch of the two GEMM-class kernels is bracketed by
 * HIP events on the caller's stream.  class 0 = layer_kernel (all MLP chains), class 1 = wgrad_kernel,
 * class 2 = the fused SDF primal chain (16-bit builds: PE + lin0..lin8 of the SDF network in one launch), class 3 = the fused
 * SDF adjoint chain (the normals), class 4 = the heads' fused chains (forward and backward, one launch per head each).
 * neat_prof_collect synchronises on the recorded events and returns the summed kernel time, the summed
 * ALGORITHMIC flops (2*N*K*P with the true layer dims), the summed ALGORITHMIC HBM bytes (each operand/result row once,
 * weights once) and the launch count since neat_prof_enable(1). */
/* A/B switches for benchmarking and for the cross-check tests (tests/test_gpu_parity.py::test_bf16_*_kernels_agree); every
 * setting computes the same result up to summation order.  Returns -1 for an unknown key / value.
 * Retired keys (closed experiments; their numbers are not reused and return -1): 3, 4, 5, 7, 10, 15, 18, 19, 20, 23.
 *   0 bf16 layer-kernel point tile (2 = 64 points (default), 4 = 128)
 *   1 weight gradient: 1 = tr16 streaming kernel (default), 0 = previous
 *   2 hidden layers: 1 = weight-stationary streaming kernel (default), 0 = previous
 *   6 partial reduction: 2 = one launch, 16-byte loads (default), 0 = group sums + finish, 1 = one 16-wave pass
 *   8 same-shaped weight gradients per launch (-1 = by problem size (default), 0 = one layer per launch, 2, 3, 6)
 *   9 point tiles of the persistent streaming kernels: 1 = interleaved over the workgroups (default), 2 = interleaved with an
 *     XCD-contiguous slot order (measured neutral), 0 = one contiguous range each
 *  11 non-temporal accesses, bit mask (default 15): 1 / 2 = aux0 / aux1 fetch of the layer kernels, 4 = weight-gradient operands,
 *     8 = `in` fetch of the layer kernels, 16 = out1 (m_l) store, 32 = out0 store (both stores measured neutral)
 *  12 layer kernels: 1 = 16-byte output stores through v_permlane32_swap (default; measured neutral), 0 = 8-byte stores
 *  13 16-bit builds: the adjoint chain (normals) as one fused launch (default 1), 0 = seed + eight streaming launches
 *  14 16-bit builds: the two heads as fused chains (kernels_heads.hpp): 2 = forward and backward (default), 1 = forward only,
 *     0 = one layer_kernel_ws launch per layer
 *  16 16-bit builds: weight gradients of the SDF layers 1..7 contracted inside the tangent / reverse launches that hold both
 *     operands in LDS (kernels_dw.hpp): 1 = from 49 152 points on (default), 2 = always, 0 = never (separate launches)
 *  17 probe switch of those launches (default 0; 4 = no partial stores: wrong results)
 *  21 16-bit builds: lin0's weight gradient (K = 39 PE columns) on the one-column-block variant of the streaming kernel: 0 = off,
 *     n = 1..4: on, with n times the point splits (default 1; 2 and 4 measured no faster)
 *  22 with key 16: the feature rows of lin8's weight gradient contracted inside lin8's reverse launch as well (default 1)
 *  24 with keys 16 and 22: the chain variables of those launches (tangents of h_2..h_7, cotangents of a_6..a_1) alternate between two
 *     buffers each instead of one array per layer (default 1; results bit-identical, fewer HBM write-backs)
 *  25 with key 16: consecutive layers of the tangent / reverse chains that share an epilogue variant run as ONE launch in which every
 *     workgroup loops over the layers for its own tiles (tangent 1-2 | 3 | 4-7, reverse 8 | 7-5 | 4 | 3-1: 15 launches -> 7; default 1;
 *     results bit-identical)
 *  28 the two 256 x 256 layers of the global-junction MLP (neat_ffn_forward / neat_ffn_backward's data path) on the fp32 matrix pipe
 *     (v_mfma_f32_32x32x2_f32: exact fp32 products, fixed summation order) instead of the vector-ALU kernel (default 1) */
int neat_set_tuning(int key, int value);
int neat_prof_enable(int on);
int neat_prof_collect(int cls, NEAT_HOST double* total_ms, NEAT_HOST double* total_flops, NEAT_HOST int* launches, NEAT_HOST double* total_bytes);

#ifdef __cplusplus
}
#endif
#endif
