// Writing an unrooted tree in the reference's numbering by ONE wave, lanes over nodes, without a
// stack: leaves keep their ids, internal nodes are numbered in post-order with the children
// ordered by largest leaf id, the trifurcating root is 2n-3, every length goes with its subtree.
// Shared by the NNI move (kernels_search.hip: MOVE = true) and neighbour joining
// (kernels_nj.hip: MOVE = false, the tree as it is); everything here is inline, each kernel file
// gets its own copy.  A workgroup is one wave: the barriers order that wave's own loads and
// stores.
#pragma once
#include <hip/hip_runtime.h>

#include "mi_phylo_device_utils.h"
#include "mi_phylo_kernels.h"

namespace miphylo {
namespace dev {

__device__ __forceinline__ void copy_tree(int n, const int32_t* pid, const double* bl, int32_t* out_pid,
                                          double* out_bl) {
  const int root = 2 * n - 3;
  for (int j = threadIdx.x; j <= root; j += 64) {
    if (j < root) out_pid[j] = pid[j];
    out_bl[j] = bl[j];
  }
}

// ------------------------------------------------------------------------
// MOVE: one NNI move of one tree, the result of mi_nni_neighbour (mi_phylo_nni.cpp), bit for
// bit.  code = 2 v + i: v's child `moved` (the second in child order
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
// Not MOVE: `code` is not looked at, step 3 is left out -- the tree (pid, bl), whose ids need only
// be a post-order (parent > child), in the reference's numbering.
// ------------------------------------------------------------------------
template <bool MOVE>
__device__ __forceinline__ void renumber_tree(int n, int t, const int32_t* pid, const double* bl, int code,
                                               int32_t* ws, int32_t* status, int32_t* out_pid,
                                               double* out_bl, int32_t* pid2, double* bl2) {
  const int lane = threadIdx.x;
  const int root = 2 * n - 3, R = root + 1;
  const int v = code >> 1, which = code & 1;
  const bool move = !MOVE || (code >= 0 && v >= n && v < root);  // (wave-uniform)
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
  if (MOVE) {
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

}  // namespace dev
}  // namespace miphylo
