// Marginal ancestral-state and rate-category posteriors per pattern: what the
// pre-order pass of the HBM-streamed family holds in registers at every visit, normalised and
// written out instead of contracted away.  A member of the HBM-streamed family
// (mi_phylo_hbm_walk_device.h): the lane context, the post-order pass, a visit's
// operands and the child stores are the family's; the kernel's own are J / T0 / T1, the parked
// category terms and the output stores.  (gfx950 / CDNA4, wave64.)
#include <hip/hip_runtime.h>

#include "mi_phylo_device_utils.h"
#include "mi_phylo_hbm_walk_device.h"
#include "mi_phylo_kernels.h"

namespace miphylo {

namespace {
using namespace dev;

// one row of posteriors from its numerators: the denominator is their sum as computed
__device__ __forceinline__ D4 normalise4(D4 j) {
  const double s = (j.x0 + j.x1) + (j.x2 + j.x3);
  return {j.x0 / s, j.x1 / s, j.x2 / s, j.x3 / s};
}
// the largest entry, the lowest state among equals; a NaN row (0/0) gives 0
__device__ __forceinline__ int argmax4(D4 v) {
  int best = 0;
  double m = v.x0;
  if (v.x1 > m) {
    m = v.x1;
    best = 1;
  }
  if (v.x2 > m) {
    m = v.x2;
    best = 2;
  }
  if (v.x3 > m) best = 3;
  return best;
}
__device__ __forceinline__ void add_scaled4(D4& acc, double c, D4 v) {
  acc.x0 += c * v.x0;
  acc.x1 += c * v.x1;
  acc.x2 += c * v.x2;
  acc.x3 += c * v.x3;
}

// ------------------------------------------------------------------------
// The walk of nni_scan_hbm_kernel without the scan.  Post-order: the family's (the
// log-likelihood partial is the scan's, bit for bit).  Pre-order, parents before
// children: at the visit of node u (children x, y; A = P_x L_x, B = P_y L_y; `qv` = q_u, or pi
// at the set-up root) q_u o A o B is the joint of u's state and the data in category k, so
//   J_u = sum_k c_k q_u,k o A_k o B_k,      state_post[u] = J_u / sum_s J_u[s]
// from the category loop the pass runs anyway.  Every power of two that rescaling removed is
// shared by the categories of a (node, pattern) and so sits in all four numerators alike.
// The set-up tree has B = 2n-2 with children (c0, R) and R = 2n-3 with children (c1, c2), both
// edges of length 0 (kernels_nni.hip): R is the caller's root and its row is written at its own
// visit (q_R = P_R^T (pi o S_c0) with P_R = P(0)); B's visit writes no row.  What B's visit
// does hold is sum_s pi_s L_root,k[s] = sum_s (pi o A o B)_s per category: the terms of
// cat_post.  They are parked in B's own arena slot, which the pre-order pass never reads (one
// word per category: no register array indexed by k), and normalised once their sum is known.
// A leaf child's q is formed at its parent's visit; q o (tip vector), summed over the categories
// and normalised, is the optional tip row.
// Outputs are indexed by the call's tree index (a.eval_offset + the launch's evaluation): a call
// cut into several launches writes the same bytes.  Lanes beyond P store nothing.
// ------------------------------------------------------------------------
template <bool RESCALE, bool TIP_PARTIALS>
__global__ __launch_bounds__(kTile) void ancestral_hbm_kernel(LikArgs a) {
  const HbmLane<TIP_PARTIALS> c(a);
  const DevModel* __restrict__ model = c.model;
  const int t = c.t, p = c.p, K = c.K, n = c.n;

  hbm_post_order<RESCALE>(c);

  // ---- pre-order, parents before children: the joints ----
  const bool live = c.live();
  const bool want_cat = a.anc_cat != nullptr || a.anc_rate != nullptr;
  for (int i = n - 2; i >= 0; i--) {
    const SchedEntry s = c.sched[i];
    const bool is_root = i == n - 2;
    const bool tip0 = a.anc_tip != nullptr && s.child0 < n;
    const bool tip1 = a.anc_tip != nullptr && s.child1 < n;
    D4 J{0, 0, 0, 0}, T0{0, 0, 0, 0}, T1{0, 0, 0, 0};
    double cat_sum = 0;
    double mx0 = 0, mx1 = 0;
    for (int k = 0; k < K; k++) {
      const HbmVisit v = hbm_visit_operands(c, s, is_root, k);
      const double cw = model->cat_weight[k];
      const D4 qA = mul4(v.qv, v.A), qB = mul4(v.qv, v.B);
      if (!is_root) {
        add_scaled4(J, cw, mul4(qA, v.B));
      } else if (want_cat) {
        const double cs = cw * dot4(qA, v.B);
        cat_sum += cs;
        c.plv_at(s.node, k)[0] = cs;
      }
      const D4 q0 = matTvec(v.M0, qB);
      const D4 q1 = matTvec(v.M1, qA);
      hbm_store_children<RESCALE>(c, s, k, q0, q1, mx0, mx1);
      if (tip0) add_scaled4(T0, cw, mul4(q0, v.L0));
      if (tip1) add_scaled4(T1, cw, mul4(q1, v.L1));
    }
    hbm_rescale_children<RESCALE>(c, s, mx0, mx1);
    if (!is_root && live) {
      const size_t row = ((size_t)t * (n - 2) + (s.node - n)) * a.P + p;
      const D4 post = normalise4(J);
      store4(a.anc_state + row * 4, post);
      if (a.anc_map) a.anc_map[row] = (int8_t)argmax4(post);
    }
    if (tip0 && live) store4(a.anc_tip + (((size_t)t * n + s.child0) * a.P + p) * 4, normalise4(T0));
    if (tip1 && live) store4(a.anc_tip + (((size_t)t * n + s.child1) * a.P + p) * 4, normalise4(T1));
    if (is_root && want_cat) {
      double rate = 0;
      for (int k = 0; k < K; k++) {
        const double post = c.plv_at(s.node, k)[0] / cat_sum;
        if (a.anc_cat && live) a.anc_cat[((size_t)t * a.P + p) * K + k] = post;
        rate += model->cat_rate[k] * post;
      }
      if (a.anc_rate && live) a.anc_rate[(size_t)t * a.P + p] = rate;
    }
  }
}

// ------------------------------------------------------------------------
// The call's log-likelihoods, a workgroup per tree, by the family's tile sums
// (mi_phylo_hbm_walk_device.h): that of a gradient call on the HBM path, bit for bit.
// ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ancestral_finalize_kernel(const double* __restrict__ ll_part, int ll_tiles,
                                                                 int ll_used, double* __restrict__ out_ll) {
  __shared__ double llw[4];
  const int t = blockIdx.x;
  ll_tile_shares(ll_part + (size_t)t * ll_tiles, ll_used, llw);
  __syncthreads();
  if (threadIdx.x == 0) out_ll[t] = ll_tile_total(llw);
}

}  // namespace

// ------------------------------------------------------------------------
// Launch wrappers
// ------------------------------------------------------------------------
void launch_ancestral_hbm(const LikArgs& a, int count, bool rescale, hipStream_t s) {
  launch_hbm_member(a, count, rescale, 0, s, [](auto R, auto TP) -> HbmKernel {
    return ancestral_hbm_kernel<decltype(R)::value, decltype(TP)::value>;
  });
}
void launch_ancestral_finalize(const double* ll_part, int T, int ll_tiles, int ll_used, double* out_ll,
                               hipStream_t s) {
  if (T <= 0 || !out_ll) return;
  hipLaunchKernelGGL(ancestral_finalize_kernel, dim3(T), dim3(256), 0, s, ll_part, ll_tiles, ll_used, out_ll);
}
const char* ancestral_kernel_name() { return "ancestral_hbm_kernel"; }

}  // namespace miphylo
