// The SPR hill-climbing search on the device: taking subtree-prune-and-regraft
// moves in place, in the reference's numbering (mi_engine_spr_apply_unrooted), and the per-tree
// step between two rounds of mi_engine_spr_search_unrooted.  (gfx950 / CDNA4, wave64.)
// A workgroup is ONE wave and owns one tree: the barriers below order that wave's own loads
// and stores, nothing here waits on another wave.  The likelihood work of the search is the
// optimiser's and the scan's (kernels_walk_hess.hip, kernels_gradient.hip, kernels_spr.hip).
#include <hip/hip_runtime.h>

#include "mi_phylo_device_utils.h"
#include "mi_phylo_kernels.h"
#include "mi_phylo_spr_apply_device.h"

namespace miphylo {

namespace {
using namespace dev;

constexpr int kSprApplyLdsWords = kSprApplyArrays * kSprApplyLdsNodes + kSprApplyExtra;

__global__ __launch_bounds__(64) void spr_apply_kernel(SprApplyArgs a) {
  __shared__ int32_t lds[kSprApplyLdsWords];
  const int t = blockIdx.x, n = a.n;
  const size_t np = 2 * (size_t)n - 3, nl = np + 1;
  const int32_t* move = a.moves + (size_t)t * 3;
  // (two instances, so that the LDS one addresses LDS and not a generic pointer)
  if (2 * n - 2 <= kSprApplyLdsNodes)
    spr_apply_tree(n, t, a.parent_ids + t * np, a.bl + t * nl, move[0], move[1], move[2], lds, a.status,
                   a.out_parent_ids + t * np, a.out_bl + t * nl, nullptr, nullptr);
  else
    spr_apply_tree(n, t, a.parent_ids + t * np, a.bl + t * nl, move[0], move[1], move[2],
                   a.ws + t * spr_apply_ws_words(n), a.status, a.out_parent_ids + t * np, a.out_bl + t * nl,
                   nullptr, nullptr);
}

// ------------------------------------------------------------------------
// The step of one tree after a round's optimisation and scan (a wave per packed tree): take the
// scan's best move if its delta exceeds min_gain and the tree has moves left -- log it, write
// the neighbour into the other half of the pair (and into the packed inputs of the next round),
// count the tree in the round's word -- or stop: the outputs at the tree's own index, and the
// optimised lengths into both halves, so that a round that still carries the tree along finds
// a tree at its optimum.
// ------------------------------------------------------------------------
__global__ __launch_bounds__(64) void spr_search_step_kernel(SprSearchStepArgs a) {
  __shared__ int32_t lds[kSprApplyLdsWords];
  const int lane = threadIdx.x, p = blockIdx.x, n = a.n;
  const int t = a.map ? a.map[p] : p;
  if (a.status[t] != kSprSearchActive) return;  // (wave-uniform)
  const size_t np = 2 * (size_t)n - 3, nl = np + 1;
  const int32_t* move = a.best + (size_t)p * 3;
  const int s = move[0], dir = move[1], f = move[2];
  const int taken = a.move_count[t];
  const bool is_move = s >= 0 && s < (int)np && (dir == 0 || dir == 1);
  const double gain = is_move ? a.delta[((size_t)p * np + s) * 2 + dir] : 0.0;
  const bool better = n > 3 && gain > a.min_gain;  // (a NaN is not)
  const double* opt_bl = a.opt_bl + p * nl;
  if (better && taken < a.max_moves) {
    int32_t* pid2 = a.map ? a.pk_pid + p * np : nullptr;
    double* bl2 = a.map ? a.pk_bl + p * nl : nullptr;
    if (2 * n - 2 <= kSprApplyLdsNodes)
      spr_apply_tree(n, t, a.cur_pid + t * np, opt_bl, s, dir, f, lds, a.engine_status, a.next_pid + t * np,
                     a.next_bl + t * nl, pid2, bl2);
    else
      spr_apply_tree(n, t, a.cur_pid + t * np, opt_bl, s, dir, f, a.ws + p * spr_apply_ws_words(n),
                     a.engine_status, a.next_pid + t * np, a.next_bl + t * nl, pid2, bl2);
    if (lane == 0) {
      if (a.move_log) {
        int32_t* log = a.move_log + ((size_t)t * a.max_moves + taken) * 3;
        log[0] = s, log[1] = dir, log[2] = f;
      }
      if (a.move_gain) a.move_gain[(size_t)t * a.max_moves + taken] = gain;
      a.move_count[t] = taken + 1;
      atomicAdd(a.active, 1);
    }
    return;
  }
  for (int j = lane; j < (int)nl; j += 64) {
    const double len = opt_bl[j];
    a.out_bl[t * nl + j] = len;
    a.cur_bl[t * nl + j] = len;
    a.next_bl[t * nl + j] = len;
    if (a.map) a.pk_bl[p * nl + j] = len;
    if (j < (int)np) {
      const int32_t par = a.cur_pid[t * np + j];
      a.out_pid[t * np + j] = par;
      a.next_pid[t * np + j] = par;
    }
  }
  if (lane == 0) {
    a.out_ll[t] = a.opt_ll[p];
    if (a.out_best_delta) a.out_best_delta[t] = gain;
    if (a.out_opt_status) a.out_opt_status[t] = a.opt_status[p];
    a.status[t] = better ? 1 : 0;  // MI_SPR_SEARCH_MOVE_LIMIT : MI_SPR_SEARCH_LOCAL_OPTIMUM
  }
}

}  // namespace

void launch_spr_apply(const SprApplyArgs& a, hipStream_t s) {
  if (a.T <= 0) return;
  hipLaunchKernelGGL(spr_apply_kernel, dim3(a.T), dim3(64), 0, s, a);
}
void launch_spr_search_step(const SprSearchStepArgs& a, hipStream_t s) {
  if (a.count <= 0) return;
  hipLaunchKernelGGL(spr_search_step_kernel, dim3(a.count), dim3(64), 0, s, a);
}

}  // namespace miphylo
