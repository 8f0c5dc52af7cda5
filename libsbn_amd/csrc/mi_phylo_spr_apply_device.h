// One SPR move of one unrooted tree by ONE wave, lanes over nodes, without a stack: the result of
// mi_spr_neighbour (mi_phylo_spr.cpp), bit for bit.  Shared by the apply kernel
// and the step kernel of the SPR search (kernels_search.hip).  A workgroup is one wave: the
// barriers order that wave's own loads and stores, nothing here waits on another wave.
#pragma once
#include <hip/hip_runtime.h>

#include "mi_phylo_device_utils.h"
#include "mi_phylo_kernels.h"
#include "mi_phylo_renumber_device.h"

namespace miphylo {
namespace dev {

// children of every node from the parent links P by three rounds of "write your id into your
// parent's slot, see who stayed" (no atomics); the root's third child in third[0]
__device__ __forceinline__ void spr_children(int root, const int32_t* P, int32_t* K0, int32_t* K1, int32_t* third) {
  const int lane = threadIdx.x;
  for (int x = lane; x < root; x += 64) K0[P[x]] = x;
  __syncthreads();
  for (int x = lane; x < root; x += 64)
    if (K0[P[x]] != x) K1[P[x]] = x;
  __syncthreads();
  for (int x = lane; x < root; x += 64) {
    const int p = P[x];
    if (K0[p] != x && K1[p] != x && p == root) third[0] = x;
  }
  __syncthreads();
}

// ------------------------------------------------------------------------
// The move (s, dir, f) as the scan's best_move gives it: the part of the tree behind edge s
// (dir = 0: the clade below s, dir = 1: everything above s) is cut off and hung into the middle
// of edge f.  The node that goes (the hub: par[s] for dir = 0, s itself for dir = 1) leaves two
// edges that merge into one; its SLOT serves as the new attachment node, so that the top of the
// new tree is always slot 2n-3.
//   1  parents in, checked (every index below is in range, parent > child); children by three
//      rounds; the tree's shape checked: as renumber_tree
//   2  the walk from f to the root, every lane the same words (at most 2n-2 steps: parent >
//      child): is f in the clade of s; the children of s and of the root on that path.  The move is
//      checked here, before anything is written: f not in the moving part, not a name of the
//      merged edge
//   3  the surgery on the parent links, by lane 0, with SRC[x]: where the length above x comes
//      from (a node id: bl of that node; kMerged: the sum of the two merged edges; kHalf: half of
//      t_f).
//        dir = 0, hub u not the root: y (the sibling of s) goes under par[u] on the merged edge,
//          u goes above f
//        otherwise (hub h = s, or the root): h's children become f and par[f]; the parent links
//          from par[f] up to h's child on that side are reversed, each edge keeping its length
//          (at most 2n-2 steps); that child gets h's other child on the merged edge
//   4  children again from the new links; largest leaf id ML and internal-node count ISZ of every
//      subtree in an order-free form (the ids are no post-order any more): rounds of "done when
//      my children are done", at most 2n-2 rounds, the tree's height in practice
//   5  new ids by pointer jumping along the parent links and the write of every child at its new
//      id: steps 4 and 5 of renumber_tree
// ws: kSprApplyArrays arrays of R = 2n-2 words and kSprApplyExtra more (LDS or global).  A triple
// that is no move, or a tree that is not one, sets the status word and copies.
// (pid2, bl2): a second destination of the same result, or nullptr.
// ------------------------------------------------------------------------
__device__ __forceinline__ void spr_apply_tree(int n, int t, const int32_t* pid, const double* bl, int s, int dir,
                                               int f, int32_t* ws, int32_t* status, int32_t* out_pid,
                                               double* out_bl, int32_t* pid2, double* bl2) {
  constexpr int kMerged = -1, kHalf = -2;
  const int lane = threadIdx.x;
  const int root = 2 * n - 3, R = root + 1;
  const bool copy = s == -1 && dir == -1 && f == -1;
  const bool in_range = s >= 0 && s < root && f >= 0 && f < root && (dir == 0 || (dir == 1 && s >= n));
  if (copy || !in_range) {  // (wave-uniform)
    if (!copy && lane == 0) set_status(status, kBadSprMove, t);
    copy_tree(n, pid, bl, out_pid, out_bl);
    if (pid2) copy_tree(n, pid, bl, pid2, bl2);
    return;
  }
  int32_t *P = ws, *K0 = ws + R, *K1 = ws + 2 * R, *ML = ws + 3 * R, *ISZ = ws + 4 * R, *ACC = ws + 5 * R,
          *SRC = ws + 6 * R;
  int32_t* third = ws + 7 * R;  // the root's third child

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
    SRC[x] = x;
  }
  if (lane == 0) third[0] = -1;
  __syncthreads();
  spr_children(root, P, K0, K1, third);
  for (int x = lane; x < root; x += 64) {
    const int p = P[x];
    if (K0[p] != x && K1[p] != x && !(p == root && third[0] == x)) bad = p == root ? kNotTrifurcatingRoot : kNotBifurcating;
  }
  for (int x = n + lane; x <= root; x += 64)
    if (K0[x] < 0 || K1[x] < 0 || (x == root && third[0] < 0)) bad = x == root ? kNotTrifurcatingRoot : kNotBifurcating;

  // ---- 2 ---- (a tree whose parents are not above their children is not walked)
  const bool tree_ok = !__any(bad != kOk);
  bool inside = false;
  int below_s = -1, below_root = f;
  if (tree_ok) {
    int v = f, prev = -1;
    for (int it = 0; it < R && v < root; it++) {
      if (v == s) inside = true, below_s = prev;
      prev = v;
      v = P[v];
    }
    below_root = prev;
  }
  const int hub = dir == 0 ? P[s] : s;
  const int pf = P[f];
  const bool merged = f == hub || pf == hub;
  if (tree_ok && (merged || (dir == 0 ? inside : !inside))) bad = kBadSprMove;
  if (bad != kOk) {  // (kBadSprMove: every lane)
    if (lane == 0 || bad != kBadSprMove) set_status(status, bad, t);
  }
  if (__any(bad != kOk)) {
    copy_tree(n, pid, bl, out_pid, out_bl);
    if (pid2) copy_tree(n, pid, bl, pid2, bl2);
    return;
  }

  // ---- 3 ---- (every lane has read the same words above; lane 0 writes)
  int m0, m1;  // the two edges that merge, by the nodes below them
  const bool simple = dir == 0 && hub != root;
  if (simple) {
    m0 = K0[hub] == s ? K1[hub] : K0[hub];
    m1 = hub;
  } else {
    const int moving = dir == 0 ? s : -1;  // (dir = 1: the moving part is above s)
    const int k0 = K0[hub], k1 = K1[hub], k2 = hub == root ? third[0] : -1;
    m0 = k0 != moving ? k0 : k1;
    m1 = k2 >= 0 && k2 != moving && k2 != m0 ? k2 : (k1 != moving && k1 != m0 ? k1 : k0);
  }
  __syncthreads();
  if (lane == 0) {
    if (simple) {
      P[m0] = P[hub];
      SRC[m0] = kMerged;
      P[hub] = pf;
      SRC[hub] = kHalf;
    } else {
      const int top_child = dir == 0 ? below_root : below_s;  // hub's child above f
      const int other = top_child == m0 ? m1 : m0;
      int prev = hub, x = pf;
      for (int it = 0; it < R && x != hub; it++) {
        const int next = P[x];
        P[x] = prev;
        SRC[x] = prev == hub ? kHalf : prev;
        prev = x;
        x = next;
      }
      P[other] = top_child;
      SRC[other] = kMerged;
    }
    P[f] = hub;
    SRC[f] = kHalf;
    third[0] = -1;
  }
  for (int x = lane; x < R; x += 64) {
    K0[x] = -1;
    K1[x] = -1;
    ML[x] = x < n ? x : -1;
    ISZ[x] = x < n ? 0 : -1;  // (-1: not known yet)
    ACC[x] = 0;
  }
  __syncthreads();

  // ---- 4 ----
  spr_children(root, P, K0, K1, third);
  for (int round = 0; round < R; round++) {
    bool pending = false;
    for (int base = n; base <= root; base += 64) {
      const int x = base + lane;
      if (x <= root && ISZ[x] < 0) {
        const int a = K0[x], b = K1[x], c3 = x == root ? third[0] : a;
        const bool full = a >= 0 && b >= 0 && c3 >= 0;  // (always, for a tree: nothing out of range)
        const int ia = full ? ISZ[a] : -1, ib = full ? ISZ[b] : -1, ic = full ? ISZ[c3] : -1;
        if (ia >= 0 && ib >= 0 && ic >= 0) {
          ML[x] = max(max(ML[a], ML[b]), ML[c3]);
          ISZ[x] = 1 + ia + ib + (x == root ? ic : 0);
        } else {
          pending = true;
        }
      }
      __syncthreads();
    }
    if (!__any(pending)) break;
  }

  // ---- 5 ---- (ANC is P, overwritten: the write goes by the child arrays)
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
  const double merged_len = bl[m0] + bl[m1], half_len = 0.5 * bl[f];
  for (int x = n + lane; x <= root; x += 64) {
    const int me = root - ACC[x];
    const int kids[3] = {K0[x], K1[x], x == root ? third[0] : -1};
#pragma unroll
    for (int q = 0; q < 3; q++) {
      const int k = kids[q];
      if (k < 0) continue;
      const int id = k < n ? k : root - ACC[k];
      if ((unsigned)id >= (unsigned)root) continue;  // (cannot happen for a tree: nothing out of range)
      const int src = SRC[k];
      const double len = src == kMerged ? merged_len : src == kHalf ? half_len : bl[src];
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

}  // namespace dev
}  // namespace miphylo
