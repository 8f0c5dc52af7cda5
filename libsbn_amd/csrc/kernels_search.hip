// The hill-climbing searches on the device: taking nearest-neighbour
// interchanges and subtree-prune-and-regraft moves in place, in the reference's numbering
// (mi_engine_{nni,spr}_apply_unrooted), and the per-tree step between two rounds of
// mi_engine_{nni,spr}_search_unrooted, one body for both kinds of move.  (gfx950 / CDNA4, wave64.)
// A workgroup is ONE wave and owns one tree: the barriers below order that wave's own loads
// and stores, nothing here waits on another wave.  The likelihood work of a search is the
// optimiser's and the scan's (kernels_walk_hess.hip, kernels_gradient.hip, kernels_nni.hip,
// kernels_spr.hip).
#include <hip/hip_runtime.h>

#include "mi_phylo_device_utils.h"
#include "mi_phylo_kernels.h"
#include "mi_phylo_spr_apply_device.h"  // (and with it mi_phylo_renumber_device.h)

namespace miphylo {

namespace {
using namespace dev;

constexpr int kNniApplyLdsWords = kNniApplyArrays * kNniApplyLdsNodes + kNniApplyExtra;
constexpr int kSprApplyLdsWords = kSprApplyArrays * kSprApplyLdsNodes + kSprApplyExtra;

__global__ __launch_bounds__(64) void nni_apply_kernel(MoveApplyArgs a) {
  __shared__ int32_t lds[kNniApplyLdsWords];
  const int t = blockIdx.x, n = a.n;
  const size_t np = 2 * (size_t)n - 3, nl = np + 1;
  const int code = a.moves[t];
  if (2 * n - 2 <= kNniApplyLdsNodes)
    renumber_tree<true>(n, t, a.parent_ids + t * np, a.bl + t * nl, code, lds, a.status, a.out_parent_ids + t * np,
                   a.out_bl + t * nl, nullptr, nullptr);
  else
    renumber_tree<true>(n, t, a.parent_ids + t * np, a.bl + t * nl, code, a.ws + t * nni_apply_ws_words(n), a.status,
                   a.out_parent_ids + t * np, a.out_bl + t * nl, nullptr, nullptr);
}

__global__ __launch_bounds__(64) void spr_apply_kernel(MoveApplyArgs a) {
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
// What the step kernel asks of a kind of move: the words of its working arrays in LDS and the
// largest tree they hold, the words per tree in the workspace otherwise, the words of a move;
// read(): the scan's best move of packed tree p and its delta (0.0: there is none); apply(): the
// neighbour (everything forced inline, so that `ws` keeps its address space); log(): the move
// into its place in the move log.
// ------------------------------------------------------------------------
struct NniMove {
  static constexpr int kLdsWords = kNniApplyLdsWords, kLdsNodes = kNniApplyLdsNodes, kWidth = 1;
  static __device__ __forceinline__ size_t ws_words(int n) { return nni_apply_ws_words(n); }
  int code;
  __device__ __forceinline__ double read(const int32_t* best, const double* delta, size_t p, size_t np) {
    code = best[p];
    return code >= 0 ? delta[p * (np + 2) * 2 + code] : 0.0;
  }
  __device__ __forceinline__ void apply(int n, int t, const int32_t* pid, const double* bl, int32_t* ws,
                                        int32_t* status, int32_t* out_pid, double* out_bl, int32_t* pid2,
                                        double* bl2) const {
    renumber_tree<true>(n, t, pid, bl, code, ws, status, out_pid, out_bl, pid2, bl2);
  }
  __device__ __forceinline__ void log(int32_t* at) const { at[0] = code; }
};

struct SprMove {
  static constexpr int kLdsWords = kSprApplyLdsWords, kLdsNodes = kSprApplyLdsNodes, kWidth = 3;
  static __device__ __forceinline__ size_t ws_words(int n) { return spr_apply_ws_words(n); }
  int s, dir, f;
  __device__ __forceinline__ double read(const int32_t* best, const double* delta, size_t p, size_t np) {
    const int32_t* move = best + p * 3;
    s = move[0], dir = move[1], f = move[2];
    const bool is_move = s >= 0 && s < (int)np && (dir == 0 || dir == 1);
    return is_move ? delta[(p * np + s) * 2 + dir] : 0.0;
  }
  __device__ __forceinline__ void apply(int n, int t, const int32_t* pid, const double* bl, int32_t* ws,
                                        int32_t* status, int32_t* out_pid, double* out_bl, int32_t* pid2,
                                        double* bl2) const {
    spr_apply_tree(n, t, pid, bl, s, dir, f, ws, status, out_pid, out_bl, pid2, bl2);
  }
  __device__ __forceinline__ void log(int32_t* at) const { at[0] = s, at[1] = dir, at[2] = f; }
};

// ------------------------------------------------------------------------
// The step of one tree after a round's optimisation and scan (a wave per packed tree): take the
// scan's best move if its delta exceeds min_gain and the tree has moves left -- log it, write
// the neighbour into the other half of the pair (and into the packed inputs of the next round),
// count the tree in the round's word -- or stop: the outputs at the tree's own index, and the
// optimised lengths into both halves, so that a round that still carries the tree along finds
// a tree at its optimum.
// ------------------------------------------------------------------------
template <class Move>
__global__ __launch_bounds__(64) void search_step_kernel(SearchStepArgs a) {
  __shared__ int32_t lds[Move::kLdsWords];
  const int lane = threadIdx.x, p = blockIdx.x, n = a.n;
  const int t = a.map ? a.map[p] : p;
  if (a.status[t] != kSearchActive) return;  // (wave-uniform)
  const size_t np = 2 * (size_t)n - 3, nl = np + 1;
  const int taken = a.move_count[t];
  Move move;
  const double gain = move.read(a.best, a.delta, p, np);
  const bool better = n > 3 && gain > a.min_gain;  // (a NaN is not)
  const double* opt_bl = a.opt_bl + p * nl;
  if (better && taken < a.max_moves) {
    int32_t* pid2 = a.map ? a.pk_pid + p * np : nullptr;
    double* bl2 = a.map ? a.pk_bl + p * nl : nullptr;
    // (two instances, so that the LDS one addresses LDS and not a generic pointer)
    if (2 * n - 2 <= Move::kLdsNodes)
      move.apply(n, t, a.cur_pid + t * np, opt_bl, lds, a.engine_status, a.next_pid + t * np, a.next_bl + t * nl,
                 pid2, bl2);
    else
      move.apply(n, t, a.cur_pid + t * np, opt_bl, a.ws + p * Move::ws_words(n), a.engine_status,
                 a.next_pid + t * np, a.next_bl + t * nl, pid2, bl2);
    if (lane == 0) {
      if (a.move_log) move.log(a.move_log + ((size_t)t * a.max_moves + taken) * Move::kWidth);
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
    a.status[t] = better ? 1 : 0;  // MI_{NNI,SPR}_SEARCH_MOVE_LIMIT : MI_{NNI,SPR}_SEARCH_LOCAL_OPTIMUM
  }
}

}  // namespace

void launch_nni_apply(const MoveApplyArgs& a, hipStream_t s) {
  if (a.T <= 0) return;
  hipLaunchKernelGGL(nni_apply_kernel, dim3(a.T), dim3(64), 0, s, a);
}
void launch_spr_apply(const MoveApplyArgs& a, hipStream_t s) {
  if (a.T <= 0) return;
  hipLaunchKernelGGL(spr_apply_kernel, dim3(a.T), dim3(64), 0, s, a);
}
void launch_nni_search_step(const SearchStepArgs& a, hipStream_t s) {
  if (a.count <= 0) return;
  hipLaunchKernelGGL(search_step_kernel<NniMove>, dim3(a.count), dim3(64), 0, s, a);
}
void launch_spr_search_step(const SearchStepArgs& a, hipStream_t s) {
  if (a.count <= 0) return;
  hipLaunchKernelGGL(search_step_kernel<SprMove>, dim3(a.count), dim3(64), 0, s, a);
}

}  // namespace miphylo
