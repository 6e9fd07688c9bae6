// Translation unit of the fused chain kernels (see fused_launch.hpp for why it is separate).
#if defined(NEAT_HALF) && NEAT_HALF      // the f16 twin of this translation unit (see neat_net.hip)
#define neat neat_f16
#endif
#include "kernels_fused.hpp"
#include "kernels_x3.hpp"
#include "kernels_heads.hpp"

namespace neat {

hipError_t launch_sdf_fused_w64(hipStream_t st, const FusedArgs& a, int ntiles, int nwg, bool full) {
  typedef F6Cfg<4, 1> C;
  // (the kernel's last argument: a negative workgroup count would interleave the batches over the workgroups; not used)
  NEAT_TRY((lds_limit<&sdf_fused_w64_kernel<4, false, 1>, &sdf_fused_w64_kernel<4, true, 1>>(C::LDS)));
  if (full) hipLaunchKernelGGL((sdf_fused_w64_kernel<4, false, 1>), dim3(nwg), dim3(C::THREADS), C::LDS, st, a, ntiles, nwg);
  else hipLaunchKernelGGL((sdf_fused_w64_kernel<4, true, 1>), dim3(nwg), dim3(C::THREADS), C::LDS, st, a, ntiles, nwg);
  return hipGetLastError();
}

hipError_t launch_sdf_adjoint_w64(hipStream_t st, const AdjArgs& a, int ntiles, int nwg, bool save) {
  typedef F6Cfg<4, 1> C;
  NEAT_TRY((lds_limit<&sdf_adjoint_w64_kernel<true>, &sdf_adjoint_w64_kernel<false>>(C::LDS)));
  if (save) hipLaunchKernelGGL((sdf_adjoint_w64_kernel<true>), dim3(nwg), dim3(C::THREADS), C::LDS, st, a, ntiles, nwg);
  else hipLaunchKernelGGL((sdf_adjoint_w64_kernel<false>), dim3(nwg), dim3(C::THREADS), C::LDS, st, a, ntiles, nwg);
  return hipGetLastError();
}

template <auto Kern, class A> static hipError_t x3_launch(hipStream_t st, int nbatches, int nwg, const A& args) {
  NEAT_TRY(lds_limit<Kern>(X3::LDS));
  const int grid = nbatches < nwg ? nbatches : nwg;
  if (grid <= 0) return hipSuccess;
  hipLaunchKernelGGL(Kern, dim3(grid), dim3(X3::THREADS), X3::LDS, st, args, nbatches);
  return hipGetLastError();
}

hipError_t launch_sdf_chain_x3(hipStream_t st, const FusedArgs& a, int nbatches, int nwg, bool full) {
  return full ? x3_launch<&sdf_chain_x3_kernel<false>>(st, nbatches, nwg, a) : x3_launch<&sdf_chain_x3_kernel<true>>(st, nbatches, nwg, a);
}

hipError_t launch_sdf_adjoint_x3(hipStream_t st, const AdjArgs& a, int nbatches, int nwg, bool save) {
  return save ? x3_launch<&sdf_adjoint_x3_kernel<true>>(st, nbatches, nwg, a) : x3_launch<&sdf_adjoint_x3_kernel<false>>(st, nbatches, nwg, a);
}

hipError_t launch_head_chain_x3(hipStream_t st, const HeadX3Args& a, int head, int nbatches, int nwg, bool save) {
  if (head == 0) return save ? x3_launch<&head_chain_x3_kernel<0, true>>(st, nbatches, nwg, a) : x3_launch<&head_chain_x3_kernel<0, false>>(st, nbatches, nwg, a);
  return save ? x3_launch<&head_chain_x3_kernel<1, true>>(st, nbatches, nwg, a) : x3_launch<&head_chain_x3_kernel<1, false>>(st, nbatches, nwg, a);
}

template <auto Kern, class A> static hipError_t hc_launch(hipStream_t st, int npairs, int nwg, const A& args) {
  NEAT_TRY(lds_limit<Kern>(HC::LDS));
  const int nb = (npairs + 1) / 2;
  const int grid = nb < nwg ? nb : nwg;
  if (grid <= 0) return hipSuccess;
  hipLaunchKernelGGL(Kern, dim3(grid), dim3(HC::THREADS), HC::LDS, st, args, npairs);
  return hipGetLastError();
}

hipError_t launch_head_chain(hipStream_t st, const HeadX3Args& a, int head, int npairs, int nwg, bool save) {
  if (head == 0) return save ? hc_launch<&head_chain_kernel<0, true>>(st, npairs, nwg, a) : hc_launch<&head_chain_kernel<0, false>>(st, npairs, nwg, a);
  return save ? hc_launch<&head_chain_kernel<1, true>>(st, npairs, nwg, a) : hc_launch<&head_chain_kernel<1, false>>(st, npairs, nwg, a);
}

hipError_t launch_head_bwd_chain(hipStream_t st, const HeadBwdArgs& a, int head, int npairs, int nwg) {
  return head == 0 ? hc_launch<&head_bwd_chain_kernel<0>>(st, npairs, nwg, a) : hc_launch<&head_bwd_chain_kernel<1>>(st, npairs, nwg, a);
}

}  // namespace neat
