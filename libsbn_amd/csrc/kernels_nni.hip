// The NNI neighbourhood scan: the log-likelihood change of both
// nearest-neighbour interchanges across every inner edge of a tree, from ONE post-order and
// pre-order walk.  A member of the HBM-streamed family (mi_phylo_hbm_walk_device.h, DESIGN.md
// 4.15): the lane context, the post-order pass, a visit's operands and the child stores are the
// family's; the kernel's own are the LDS place table, S_of, the Nni3 accumulators and the
// exchange at R.  (gfx950 / CDNA4, wave64.)
#include <hip/hip_runtime.h>

#include "mi_phylo_device_utils.h"
#include "mi_phylo_hbm_walk_device.h"
#include "mi_phylo_kernels.h"

namespace miphylo {

namespace {
using namespace dev;

// ------------------------------------------------------------------------
// The walk of gradient_hbm_kernel without its two Q products, with the scan: at the visit of
// node u (children x, y; S_x = P_x L_x; `top` = q_u, or pi at the set-up root B) every INTERNAL
// child v = x with children (a, b) is the lower end of an inner edge, and with
//   cur = sum_s top [P_v (S_a o S_b)] S_y          (the tree itself, from the same operands)
//   X0  = sum_s top [P_v (S_a o S_y)] S_b          (v keeps a, takes y; b goes up)
//   X1  = sum_s top [P_v (S_b o S_y)] S_a          (v keeps b, takes y; a goes up)
// summed over the categories with their weights, delta_i += w_p log(X_i / cur).  L_a and L_b
// are still post-order vectors (parents are visited before children); every power of two that
// rescaling removed is in cur and X_i alike and cancels.  The set-up tree has B = 2n-2 with
// children (c0, R) and R = 2n-3 with children (c1, c2), both edges of length 0; c0, c1, c2 are
// the caller's root children, and the public definition (include/mi_phylo.h) exchanges with
// the FIRST other child of v's parent:
//   u < R:   that is y: (neighbour 0, neighbour 1) = (X0, X1)
//   u == R:  v is c1 or c2, the first other root child is c0, which sits ABOVE R: by
//            reversibility exchanging b with c0 is exchanging a with y: (X1, X0)
//   u == B:  v == c0, exchanged with c1; R's vector is taken apart again:
//            cur = sum pi [P_v (S_a o S_b)] (S_c1 o S_c2), X0 = sum pi [P_v (S_a o S_c1)] (S_b o S_c2),
//            X1  = sum pi [P_v (S_b o S_c1)] (S_a o S_c2);  R itself, as B's child, is no edge.
// g_part is [tree][tile][2][N] by node id (entries of nodes that are not inner edges are never
// written and never read).  The schedule may list the nodes in any post-order (the set-up
// kernels differ), so the wave first notes every node's place in it (LDS, n-1 words).
// ------------------------------------------------------------------------
struct Nni3 {
  double cur, x0, x1;
};

template <bool RESCALE, bool TIP_PARTIALS>
__global__ __launch_bounds__(kTile) void nni_scan_hbm_kernel(LikArgs a) {
  extern __shared__ int32_t nni_place[];  // [n-1]: node - n -> index of its schedule entry
  const HbmLane<TIP_PARTIALS> c(a);
  const DevModel* __restrict__ model = c.model;
  const SchedEntry* __restrict__ sched = c.sched;
  const int lane = c.lane, p = c.p, K = c.K, n = c.n, N = c.N;
  const double w = c.w;
  double* gout = c.g_row(2 * N);

  // S = P L of a node whose vector is still its post-order one
  auto S_of = [&](int node, int k) { return matvec(c.mat_of(node, k), c.vec_of(node, k)); };

  for (int i = lane; i < n - 1; i += kTile) nni_place[sched[i].node - n] = i;
  __syncthreads();
  auto entry_of = [&](int node) { return sched[__builtin_amdgcn_readfirstlane(nni_place[node - n])]; };

  hbm_post_order<RESCALE>(c);

  // ---- pre-order + the scan, parents before children ----
  for (int i = n - 2; i >= 0; i--) {
    const SchedEntry s = sched[i];
    const bool is_root = i == n - 2;
    const bool at_R = s.node == N - 2;
    // inner edges below this node: its internal children (B's second child is R: no edge)
    const bool scan0 = s.child0 >= n, scan1 = s.child1 >= n && !is_root;
    const SchedEntry e0 = scan0 ? entry_of(s.child0) : s;
    const SchedEntry e1 = scan1 ? entry_of(s.child1) : s;
    const SchedEntry eR = is_root ? entry_of(N - 2) : s;
    Nni3 acc0{0, 0, 0}, acc1{0, 0, 0};
    double mx0 = 0, mx1 = 0;
    for (int k = 0; k < K; k++) {
      const HbmVisit v = hbm_visit_operands(c, s, is_root, k);
      const double* __restrict__ M0 = v.M0;
      const double* __restrict__ M1 = v.M1;
      const D4 qv = v.qv, A = v.A, B = v.B;
      const double cw = model->cat_weight[k];
      if (scan0) {
        const D4 Sa = S_of(e0.child0, k), Sb = S_of(e0.child1, k);
        if (is_root) {
          const D4 Sc1 = S_of(eR.child0, k), Sc2 = S_of(eR.child1, k);
          acc0.cur += cw * dot4(mul4(qv, mul4(Sc1, Sc2)), matvec(M0, mul4(Sa, Sb)));
          acc0.x0 += cw * dot4(mul4(qv, mul4(Sb, Sc2)), matvec(M0, mul4(Sa, Sc1)));
          acc0.x1 += cw * dot4(mul4(qv, mul4(Sa, Sc2)), matvec(M0, mul4(Sb, Sc1)));
        } else {
          acc0.cur += cw * dot4(mul4(qv, B), matvec(M0, mul4(Sa, Sb)));
          acc0.x0 += cw * dot4(mul4(qv, Sb), matvec(M0, mul4(Sa, B)));
          acc0.x1 += cw * dot4(mul4(qv, Sa), matvec(M0, mul4(Sb, B)));
        }
      }
      if (scan1) {
        const D4 Sa = S_of(e1.child0, k), Sb = S_of(e1.child1, k);
        acc1.cur += cw * dot4(mul4(qv, A), matvec(M1, mul4(Sa, Sb)));
        acc1.x0 += cw * dot4(mul4(qv, Sb), matvec(M1, mul4(Sa, A)));
        acc1.x1 += cw * dot4(mul4(qv, Sa), matvec(M1, mul4(Sb, A)));
      }
      const D4 q0 = matTvec(M0, mul4(qv, B));
      const D4 q1 = matTvec(M1, mul4(qv, A));
      hbm_store_children<RESCALE>(c, s, k, q0, q1, mx0, mx1);
    }
    hbm_rescale_children<RESCALE>(c, s, mx0, mx1);
    if (scan0) {
      const double d0 = wave_sum(p < a.P ? w * log(acc0.x0 / acc0.cur) : 0.0);
      const double d1 = wave_sum(p < a.P ? w * log(acc0.x1 / acc0.cur) : 0.0);
      if (lane == 0) {
        gout[s.child0] = at_R ? d1 : d0;
        gout[N + s.child0] = at_R ? d0 : d1;
      }
    }
    if (scan1) {
      const double d0 = wave_sum(p < a.P ? w * log(acc1.x0 / acc1.cur) : 0.0);
      const double d1 = wave_sum(p < a.P ? w * log(acc1.x1 / acc1.cur) : 0.0);
      if (lane == 0) {
        gout[s.child1] = at_R ? d1 : d0;
        gout[N + s.child1] = at_R ? d0 : d1;
      }
    }
  }
}

// ------------------------------------------------------------------------
// Tile reduction and outputs of the scan, a workgroup per tree, by the family's tile sums
// (mi_phylo_hbm_walk_device.h): the log-likelihood is bit for bit that of a gradient call on the
// HBM path.  delta is [N][2] by node id, 0 where the node is not
// the lower end of an inner edge; the best move is the largest delta, the lowest code 2 v + i
// among equals (NaN entries are passed over), -1 for a three-taxon tree.
// ------------------------------------------------------------------------
__device__ __forceinline__ bool nni_better(double v, int code, double best, int best_code) {
  return v > best || (v == best && code < best_code);
}
__global__ __launch_bounds__(256) void nni_finalize_kernel(NniFinalizeArgs a) {
  __shared__ double llw[4];
  __shared__ double best_v[256];
  __shared__ int32_t best_c[256];
  const int t = blockIdx.x;
  const int N = a.N, n = a.n, W = 2 * N;
  ll_tile_shares(a.ll_part + (size_t)t * a.ll_tiles, a.ll_used, llw);
  const double* src = a.g_part + (size_t)t * a.g_tiles * W;
  // (the first inner edge's first move until something is larger)
  double bv = -__builtin_huge_val();
  int bc = 2 * n;
  for (int v = threadIdx.x; v < N; v += 256) {
    const bool edge = v >= n && v < N - 2;
    double r[2] = {0.0, 0.0};
    if (edge) {
#pragma unroll
      for (int q = 0; q < 2; q++) {
        r[q] = tile_column_sum(src, W, a.g_tiles, q * N + v);
        if (nni_better(r[q], 2 * v + q, bv, bc)) {
          bv = r[q];
          bc = 2 * v + q;
        }
      }
    }
    double* out = a.out_delta + ((size_t)t * N + v) * 2;
    out[0] = r[0];
    out[1] = r[1];
  }
  best_v[threadIdx.x] = bv;
  best_c[threadIdx.x] = bc;
  __syncthreads();
  if (threadIdx.x == 0) {
    if (a.out_ll) a.out_ll[t] = ll_tile_total(llw);
    if (a.out_best) {
      for (int i = 1; i < 256; i++)
        if (nni_better(best_v[i], best_c[i], bv, bc)) {
          bv = best_v[i];
          bc = best_c[i];
        }
      a.out_best[t] = n > 3 ? bc : -1;
    }
  }
}

}  // namespace

// ------------------------------------------------------------------------
// Launch wrappers
// ------------------------------------------------------------------------
void launch_nni_scan_hbm(const LikArgs& a, int count, bool rescale, hipStream_t s) {
  launch_hbm_member(a, count, rescale, sizeof(int32_t) * (size_t)(a.n - 1), s, [](auto R, auto TP) -> HbmKernel {
    return nni_scan_hbm_kernel<decltype(R)::value, decltype(TP)::value>;
  });
}
void launch_nni_finalize(const NniFinalizeArgs& a, hipStream_t s) {
  if (a.T <= 0) return;
  hipLaunchKernelGGL(nni_finalize_kernel, dim3(a.T), dim3(256), 0, s, a);
}
const char* nni_scan_kernel_name() { return "nni_scan_hbm_kernel"; }

}  // namespace miphylo
