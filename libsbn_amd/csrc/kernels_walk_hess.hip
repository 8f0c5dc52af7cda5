// The Hessian form of the second-generation matrix-core gradient walk (the branch-length
// Hessian call): gradient_walk_body (mi_phylo_walk2_device.h) with HESS = true,
// in a translation unit of its own with its own compile flags -- an extra instantiation of the
// body in kernels_walk.hip changed the register allocation of that file's kernels.
#include "mi_phylo_walk2_device.h"

namespace miphylo {

namespace {

// (one tile per wave, like the arena and analytic variants)
template <int R, bool RESCALE, bool ARENA, bool COMPACT>
__global__ __launch_bounds__(kTile, 2) void gradient_walk_hess_kernel(LikArgs a) {
  gradient_walk_body<R, RESCALE, false, ARENA, COMPACT, true>(a);
}

}  // namespace

// ------------------------------------------------------------------------
// Launch wrappers
// ------------------------------------------------------------------------
template <bool RESCALE, bool ARENA, bool COMPACT>
static void launch_walk_hess_variant(const LikArgs& a, dim3 grid, size_t lds, hipStream_t s) {
  allow_large_lds(reinterpret_cast<const void*>(gradient_walk_hess_kernel<kLlR, RESCALE, ARENA, COMPACT>), lds);
  hipLaunchKernelGGL((gradient_walk_hess_kernel<kLlR, RESCALE, ARENA, COMPACT>), grid, dim3(kTile), lds, s, a);
}
template <bool ARENA>
static void launch_walk_hess_form(const LikArgs& a, dim3 grid, size_t lds, bool rescale, hipStream_t s) {
  const bool compact = a.kp < 4;  // (as gradient_walk_lds_bytes_for sizes the tip words)
  if (rescale && compact) launch_walk_hess_variant<true, ARENA, true>(a, grid, lds, s);
  else if (rescale) launch_walk_hess_variant<true, ARENA, false>(a, grid, lds, s);
  else if (compact) launch_walk_hess_variant<false, ARENA, true>(a, grid, lds, s);
  else launch_walk_hess_variant<false, ARENA, false>(a, grid, lds, s);
}
// The Hessian form of the walk (K <= 4): a wave per pattern tile; the store is the engine's
// choice (a.store: 1 LDS, 2 arena), the LDS footprint that of the plain walk.
void launch_gradient_walk_hessian(const LikArgs& a_in, int count, bool rescale, hipStream_t s) {
  if (count <= 0) return;
  LikArgs a = a_in;
  a.kp = a.K == 1 ? 1 : (a.K == 2 ? 2 : 4);
  a.cat_groups = 1;
  const int gtiles = gradient_mfma_tiles(a.P, a.K);
  a.walk_evals = count;
  a.walk_groups = gtiles;
  a.walk_big_evals = 0;
  const dim3 grid((unsigned)((size_t)count * gtiles));
  if (a.store == 2) {
    launch_walk_arena_ladder(a, grid.x, rescale, false, [&](const LikArgs& part, size_t lds) {
      launch_walk_hess_form<true>(part, grid, lds, rescale, s);
    });
    return;
  }
  launch_walk_hess_form<false>(a, grid, gradient_walk_lds_bytes(a.n, a.K, rescale, false), rescale, s);
}

const char* gradient_walk_hess_kernel_name() { return "gradient_walk_hess_kernel"; }

}  // namespace miphylo
