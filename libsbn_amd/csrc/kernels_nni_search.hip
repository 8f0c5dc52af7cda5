// The NNI hill-climbing search on the device: taking nearest-neighbour
// interchanges in place, in the reference's numbering (mi_engine_nni_apply_unrooted), and the
// per-tree step between two rounds of mi_engine_nni_search_unrooted.  (gfx950 / CDNA4, wave64.)
// A workgroup is ONE wave and owns one tree: the barriers below order that wave's own loads
// and stores, nothing here waits on another wave.  The likelihood work of the search is the
// optimiser's and the scan's (kernels_walk_hess.hip, kernels_gradient.hip, kernels_nni.hip).
#include <hip/hip_runtime.h>

#include "mi_phylo_device_utils.h"
#include "mi_phylo_kernels.h"

namespace miphylo {

namespace {
using namespace dev;

__device__ __forceinline__ void copy_tree(int n, const int32_t* pid, const double* bl, int32_t* out_pid,
                                          double* out_bl) {
  const int root = 2 * n - 3;
  for (int j = threadIdx.x; j <= root; j += 64) {
    if (j < root) out_pid[j] = pid[j];
    out_bl[j] = bl[j];
  }
}

// ------------------------------------------------------------------------
// One NNI move of one tree by one wave, lanes over nodes: the result of mi_nni_neighbour
// (mi_phylo_nni.cpp), bit for bit.  code = 2 v + i: v's child `moved` (the second in child order
// for i = 0, the first for i = 1) and c, the first in child order of the other children of v's
// parent u, swap parents; leaves keep their ids, internal nodes are renumbered in post-order
// with the children ordered by largest leaf id, every length goes with its subtree.
//   1  parents in, checked (so that every index below is in range); children by three rounds
//      of "write your id into your parent's slot, see who stayed": no atomics
//   2  largest leaf id ML and internal-node count ISZ of every subtree of the OLD tree, whose
//      ids are a post-order (checked in 1: parent > child): ids in blocks of 64, ascending, a
//      block repeated until its nodes are done (a node waits for children in its own block)
//   3  the exchange.  u's subtree keeps its leaves, so ML and ISZ change at v alone; the child
//      order can change at v and at u
//   4  new ids without a stack: with (k1, k2[, k3]) the children of x in the new child order,
//      new_id[x] - new_id[k_j] = ISZ[x] - sum_{i <= j} ISZ[k_i] =: d[k_j], so
//      new_id[x] = 2n-3 - sum of d over the path from x to the root: pointer jumping
//      (ACC[x] += ACC[ANC[x]], ANC[x] = ANC[ANC[x]]), log2(depth) rounds.  It follows parent
//      links, not id order: that c's old id may be larger than v's does not matter.
//   5  every internal node writes its children's parent id and length at their new ids.
// ws: six arrays of R = 2n-2 words and kNniApplyExtra more (LDS or global).  A code that is
// neither -1 nor an inner edge's, or a tree that is not one, sets the status word and copies.
// (pid2, bl2): a second destination of the same result, or nullptr.
// ------------------------------------------------------------------------
__device__ __forceinline__ void nni_apply_tree(int n, int t, const int32_t* pid, const double* bl, int code,
                                               int32_t* ws, int32_t* status, int32_t* out_pid,
                                               double* out_bl, int32_t* pid2, double* bl2) {
  const int lane = threadIdx.x;
  const int root = 2 * n - 3, R = root + 1;
  const int v = code >> 1, which = code & 1;
  const bool move = code >= 0 && v >= n && v < root;  // (wave-uniform)
  if (!move) {
    if (code != -1 && lane == 0) set_status(status, kBadNniMove, t);
    copy_tree(n, pid, bl, out_pid, out_bl);
    if (pid2) copy_tree(n, pid, bl, pid2, bl2);
    return;
  }
  int32_t *P = ws, *K0 = ws + R, *K1 = ws + 2 * R, *ML = ws + 3 * R, *ISZ = ws + 4 * R, *ACC = ws + 5 * R;
  int32_t* third = ws + 6 * R;  // the root's third child

  // ---- 1 ----
  int bad = kOk;
  for (int x = lane; x < R; x += 64) {
    int p = root;
    if (x < root) {
      p = pid[x];
      if (p <= x || p > root || p < n) {
        bad = kBadParentIds;
        p = root;
      }
    }
    P[x] = p;
    K0[x] = -1;
    K1[x] = -1;
    ML[x] = x < n ? x : -1;
    ISZ[x] = x < n ? 0 : -1;  // (-1: not known yet)
    ACC[x] = 0;
  }
  if (lane == 0) third[0] = -1;
  __syncthreads();
  for (int x = lane; x < root; x += 64) K0[P[x]] = x;
  __syncthreads();
  for (int x = lane; x < root; x += 64)
    if (K0[P[x]] != x) K1[P[x]] = x;
  __syncthreads();
  for (int x = lane; x < root; x += 64) {
    const int p = P[x];
    if (K0[p] != x && K1[p] != x) {
      if (p == root) third[0] = x;
      else bad = kNotBifurcating;
    }
  }
  __syncthreads();
  // (2n-3 children in n-3 slots of two and one of three: all placed means all slots full)
  for (int x = lane; x < root; x += 64) {
    const int p = P[x];
    if (K0[p] != x && K1[p] != x && !(p == root && third[0] == x)) bad = kNotTrifurcatingRoot;
  }
  for (int x = n + lane; x <= root; x += 64)
    if (K0[x] < 0 || K1[x] < 0 || (x == root && third[0] < 0)) bad = x == root ? kNotTrifurcatingRoot : kNotBifurcating;
  if (__any(bad != kOk)) {
    if (bad != kOk) set_status(status, bad, t);
    copy_tree(n, pid, bl, out_pid, out_bl);
    if (pid2) copy_tree(n, pid, bl, pid2, bl2);
    return;
  }

  // ---- 2 ----
  for (int base = n; base <= root; base += 64) {
    const int x = base + lane;
    bool done = x > root;
    for (int it = 0; it < 64; it++) {  // (the lowest pending node of the block is done every time)
      if (!done) {
        const int a = K0[x], b = K1[x], c3 = x == root ? third[0] : a;
        const int ia = ISZ[a], ib = ISZ[b], ic = ISZ[c3];
        if (ia >= 0 && ib >= 0 && ic >= 0) {
          ML[x] = max(max(ML[a], ML[b]), ML[c3]);
          ISZ[x] = 1 + ia + ib + (x == root ? ic : 0);
          done = true;
        }
      }
      __syncthreads();
      if (!__any(!done)) break;
    }
  }

  // ---- 3 ---- (every lane reads the same words; lane 0 writes)
  {
    const int u = P[v];
    int a = K0[v], b = K1[v];
    if (ML[a] > ML[b]) {
      const int s = a;
      a = b;
      b = s;
    }
    const int keep = which == 0 ? a : b, moved = which == 0 ? b : a;
    const int k0 = K0[u], k1 = K1[u], k2 = u == root ? third[0] : v;
    int c = k0 != v ? k0 : k1;  // the first, in child order, of u's children other than v
    if (k1 != v && k1 != c && ML[k1] < ML[c]) c = k1;
    if (k2 != v && k2 != c && ML[k2] < ML[c]) c = k2;
    const int ml_v = max(ML[keep], ML[c]), isz_v = 1 + ISZ[keep] + ISZ[c];
    __syncthreads();
    if (lane == 0) {
      K0[v] = keep;
      K1[v] = c;
      P[c] = v;
      P[moved] = u;
      if (k0 == c) K0[u] = moved;
      else if (k1 == c) K1[u] = moved;
      else third[0] = moved;
      ML[v] = ml_v;
      ISZ[v] = isz_v;
    }
    __syncthreads();
  }

  // ---- 4 ---- (ANC is P, overwritten: 5 goes by the child arrays)
  for (int x = n + lane; x < root; x += 64) {
    const int p = P[x], mine = ML[x];
    const int s0 = K0[p], s1 = K1[p], s2 = p == root ? third[0] : s0;
    int before = 0;  // internal nodes of x's subtree and of the siblings in front of it
    if (ML[s0] <= mine) before += ISZ[s0];
    if (ML[s1] <= mine) before += ISZ[s1];
    if (p == root && ML[s2] <= mine) before += ISZ[s2];
    ACC[x] = ISZ[p] - before;
  }
  __syncthreads();
  for (int round = 0; round < 32; round++) {
    bool any = false;
    for (int base = n; base < root; base += 64) {
      const int x = base + lane;
      int a = root, acc_a = 0, anc_a = root;
      if (x < root) {
        a = P[x];
        if (a != root) {
          acc_a = ACC[a];
          anc_a = P[a];
        }
      }
      __syncthreads();  // (a node's pair is read whole before anyone writes it)
      if (a != root) {
        ACC[x] += acc_a;
        P[x] = anc_a;
        any = true;
      }
      __syncthreads();
    }
    if (!__any(any)) break;
  }

  // ---- 5 ----
  for (int x = n + lane; x <= root; x += 64) {
    const int me = root - ACC[x];
    const int kids[3] = {K0[x], K1[x], x == root ? third[0] : -1};
#pragma unroll
    for (int q = 0; q < 3; q++) {
      const int k = kids[q];
      if (k < 0) continue;
      const int id = k < n ? k : root - ACC[k];
      if ((unsigned)id >= (unsigned)root) continue;  // (cannot happen for a tree: nothing out of range)
      const double len = bl[k];
      out_pid[id] = me;
      out_bl[id] = len;
      if (pid2) {
        pid2[id] = me;
        bl2[id] = len;
      }
    }
  }
  if (lane == 0) {
    out_bl[root] = bl[root];
    if (bl2) bl2[root] = bl[root];
  }
}

__global__ __launch_bounds__(64) void nni_apply_kernel(NniApplyArgs a) {
  __shared__ int32_t lds[kNniApplyArrays * kNniApplyLdsNodes + kNniApplyExtra];
  const int t = blockIdx.x, n = a.n;
  const size_t np = 2 * (size_t)n - 3, nl = np + 1;
  const int code = a.moves[t];
  if (2 * n - 2 <= kNniApplyLdsNodes)
    nni_apply_tree(n, t, a.parent_ids + t * np, a.bl + t * nl, code, lds, a.status, a.out_parent_ids + t * np,
                   a.out_bl + t * nl, nullptr, nullptr);
  else
    nni_apply_tree(n, t, a.parent_ids + t * np, a.bl + t * nl, code, a.ws + t * nni_apply_ws_words(n), a.status,
                   a.out_parent_ids + t * np, a.out_bl + t * nl, nullptr, nullptr);
}

// ------------------------------------------------------------------------
// The step of one tree after a round's optimisation and scan (a wave per packed tree): take the
// scan's best move if its delta exceeds min_gain and the tree has moves left -- log it, write
// the neighbour into the other half of the pair (and into the packed inputs of the next round),
// count the tree in the round's word -- or stop: the outputs at the tree's own index, and the
// optimised lengths into both halves, so that a round that still carries the tree along finds
// a tree at its optimum.
// ------------------------------------------------------------------------
__global__ __launch_bounds__(64) void nni_search_step_kernel(NniSearchStepArgs a) {
  __shared__ int32_t lds[kNniApplyArrays * kNniApplyLdsNodes + kNniApplyExtra];
  const int lane = threadIdx.x, p = blockIdx.x, n = a.n;
  const int t = a.map ? a.map[p] : p;
  if (a.status[t] != kNniSearchActive) return;  // (wave-uniform)
  const size_t np = 2 * (size_t)n - 3, nl = np + 1, N = nl + 1;
  const int code = a.best[p];
  const int taken = a.move_count[t];
  const double gain = code >= 0 ? a.delta[p * N * 2 + code] : 0.0;
  const bool better = n > 3 && gain > a.min_gain;  // (a NaN is not)
  const double* opt_bl = a.opt_bl + p * nl;
  if (better && taken < a.max_moves) {
    int32_t* pid2 = a.map ? a.pk_pid + p * np : nullptr;
    double* bl2 = a.map ? a.pk_bl + p * nl : nullptr;
    if (2 * n - 2 <= kNniApplyLdsNodes)
      nni_apply_tree(n, t, a.cur_pid + t * np, opt_bl, code, lds, a.engine_status, a.next_pid + t * np,
                     a.next_bl + t * nl, pid2, bl2);
    else
      nni_apply_tree(n, t, a.cur_pid + t * np, opt_bl, code, a.ws + p * nni_apply_ws_words(n), a.engine_status,
                     a.next_pid + t * np, a.next_bl + t * nl, pid2, bl2);
    if (lane == 0) {
      if (a.move_log) a.move_log[(size_t)t * a.max_moves + taken] = code;
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
    a.status[t] = better ? 1 : 0;  // MI_NNI_SEARCH_MOVE_LIMIT : MI_NNI_SEARCH_LOCAL_OPTIMUM
  }
}

}  // namespace

void launch_nni_apply(const NniApplyArgs& a, hipStream_t s) {
  if (a.T <= 0) return;
  hipLaunchKernelGGL(nni_apply_kernel, dim3(a.T), dim3(64), 0, s, a);
}
void launch_nni_search_step(const NniSearchStepArgs& a, hipStream_t s) {
  if (a.count <= 0) return;
  hipLaunchKernelGGL(nni_search_step_kernel, dim3(a.count), dim3(64), 0, s, a);
}

}  // namespace miphylo
