// Marginal ancestral-state and rate-category posteriors per pattern: what the
// pre-order pass of the HBM-streamed family holds in registers at every visit, normalised and
// written out instead of contracted away.  A member of the family of kernels_gradient.hip and
// kernels_nni.hip (one lane per pattern, one wave per (tree, 64-pattern tile), vectors through
// the `plv` arena as [node][category][pattern][state]), in a file of its own so that every other
// kernel's code stays exactly as it was.  (gfx950 / CDNA4, wave64.)
#include <hip/hip_runtime.h>

#include "mi_phylo_device_utils.h"
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
// The walk of nni_scan_hbm_kernel without the scan.  Post-order: gradient_hbm_kernel's, line for
// line (the log-likelihood partial is the scan's, bit for bit).  Pre-order, parents before
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
  const int lane = threadIdx.x;
  const TileEval te = xcd_tile_eval();
  const int tile = te.tile;
  const int e = a.eval_offset + te.eval;
  int t, mi;
  a.map.decode(e, t, mi);
  const DevModel* __restrict__ model = a.models + mi;
  const SchedEntry* __restrict__ sched = a.sched + (size_t)t * (a.n - 1);
  const int p = tile * kTile + lane;
  const int pc = p < a.P ? p : a.P - 1;
  const double w = p < a.P ? a.weights[pc] : 0.0;
  const int K = a.K, n = a.n, N = a.N;
  const size_t ppad = (size_t)a.tiles * kTile;
  const double* __restrict__ mats_e = a.mats + (size_t)e * (N - 1) * K * 16;
  double* plv_e = a.plv + (size_t)te.eval * (n - 1) * K * ppad * 4 + (size_t)p * 4;

  auto plv_at = [&](int node, int k) { return plv_e + ((size_t)(node - n) * K + k) * ppad * 4; };
  auto tip_L = [&](int node) {
    if (TIP_PARTIALS) return load4(a.tip_partials + ((size_t)node * a.P + pc) * 4);
    return tip_vector(a.tip_states[(size_t)node * a.P + pc]);
  };

  // ---- post-order (as gradient_hbm_kernel) ----
  int cum_exp = 0;
  double site = 0.0;
  for (int i = 0; i < n - 1; i++) {
    const SchedEntry s = sched[i];
    const bool is_root = i == n - 2;
    double mx = 0.0;
    for (int k = 0; k < K; k++) {
      const double* __restrict__ M0 = mats_e + ((size_t)s.child0 * K + k) * 16;
      const double* __restrict__ M1 = mats_e + ((size_t)s.child1 * K + k) * 16;
      const D4 L0 = s.child0 < n ? tip_L(s.child0) : load4(plv_at(s.child0, k));
      const D4 L1 = s.child1 < n ? tip_L(s.child1) : load4(plv_at(s.child1, k));
      const D4 L = mul4(matvec(M0, L0), matvec(M1, L1));
      if (RESCALE) mx = fmax(mx, max4(L));
      if (is_root && !RESCALE) {
        site += model->cat_weight[k] * (model->pi[0] * L.x0 + model->pi[1] * L.x1 +
                                        model->pi[2] * L.x2 + model->pi[3] * L.x3);
      } else {
        store4(plv_at(s.node, k), L);
      }
    }
    if (RESCALE) {
      const int ex = max_exponent(mx);
      cum_exp += ex;
      for (int k = 0; k < K; k++) {
        const D4 L = scale4(load4(plv_at(s.node, k)), -ex);
        if (is_root)
          site += model->cat_weight[k] * (model->pi[0] * L.x0 + model->pi[1] * L.x1 +
                                          model->pi[2] * L.x2 + model->pi[3] * L.x3);
        else
          store4(plv_at(s.node, k), L);
      }
    }
  }
  {
    double ll = log(site);
    if (RESCALE) ll += cum_exp * 0.6931471805599453;
    ll = p < a.P ? w * ll : 0.0;
    ll = wave_sum(ll);
    if (lane == 0) a.ll_part[(size_t)e * a.ll_tiles + tile] = ll;
  }

  // ---- pre-order, parents before children: the joints ----
  const bool live = p < a.P;
  const bool want_cat = a.anc_cat != nullptr || a.anc_rate != nullptr;
  for (int i = n - 2; i >= 0; i--) {
    const SchedEntry s = sched[i];
    const bool is_root = i == n - 2;
    const bool tip0 = a.anc_tip != nullptr && s.child0 < n;
    const bool tip1 = a.anc_tip != nullptr && s.child1 < n;
    D4 J{0, 0, 0, 0}, T0{0, 0, 0, 0}, T1{0, 0, 0, 0};
    double cat_sum = 0;
    double mx0 = 0, mx1 = 0;
    for (int k = 0; k < K; k++) {
      const double* __restrict__ M0 = mats_e + ((size_t)s.child0 * K + k) * 16;
      const double* __restrict__ M1 = mats_e + ((size_t)s.child1 * K + k) * 16;
      const D4 qv = is_root ? D4{model->pi[0], model->pi[1], model->pi[2], model->pi[3]}
                            : load4(plv_at(s.node, k));
      const D4 L0 = s.child0 < n ? tip_L(s.child0) : load4(plv_at(s.child0, k));
      const D4 L1 = s.child1 < n ? tip_L(s.child1) : load4(plv_at(s.child1, k));
      const D4 A = matvec(M0, L0), B = matvec(M1, L1);
      const double cw = model->cat_weight[k];
      const D4 qA = mul4(qv, A), qB = mul4(qv, B);
      if (!is_root) {
        add_scaled4(J, cw, mul4(qA, B));
      } else if (want_cat) {
        const double c = cw * dot4(qA, B);
        cat_sum += c;
        plv_at(s.node, k)[0] = c;
      }
      const D4 q0 = matTvec(M0, qB);
      const D4 q1 = matTvec(M1, qA);
      if (s.child0 >= n) {
        store4(plv_at(s.child0, k), q0);
        if (RESCALE) mx0 = fmax(mx0, max4(q0));
      } else if (tip0) {
        add_scaled4(T0, cw, mul4(q0, L0));
      }
      if (s.child1 >= n) {
        store4(plv_at(s.child1, k), q1);
        if (RESCALE) mx1 = fmax(mx1, max4(q1));
      } else if (tip1) {
        add_scaled4(T1, cw, mul4(q1, L1));
      }
    }
    if (RESCALE) {
      if (s.child0 >= n) {
        const int ex = max_exponent(mx0);
        for (int k = 0; k < K; k++)
          store4(plv_at(s.child0, k), scale4(load4(plv_at(s.child0, k)), -ex));
      }
      if (s.child1 >= n) {
        const int ex = max_exponent(mx1);
        for (int k = 0; k < K; k++)
          store4(plv_at(s.child1, k), scale4(load4(plv_at(s.child1, k)), -ex));
      }
    }
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
        const double post = plv_at(s.node, k)[0] / cat_sum;
        if (a.anc_cat && live) a.anc_cat[((size_t)t * a.P + p) * K + k] = post;
        rate += model->cat_rate[k] * post;
      }
      if (a.anc_rate && live) a.anc_rate[(size_t)t * a.P + p] = rate;
    }
  }
}

// ------------------------------------------------------------------------
// The call's log-likelihoods, a workgroup per tree: the tile partials summed in the order
// nni_finalize_kernel (kernels_nni.hip) and reduce_tiles_body (kernels_finalize.hip) sum them --
// thread i takes partials i, i + 256, ...; a wave's 64 by wave_sum; then (w0 + w1) + (w2 + w3) --
// so the result is that of a gradient call on the HBM path, bit for bit.
// ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ancestral_finalize_kernel(const double* __restrict__ ll_part, int ll_tiles,
                                                                 int ll_used, double* __restrict__ out_ll) {
  __shared__ double llw[4];
  const int t = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double llp = 0;
  for (int i = threadIdx.x; i < ll_used; i += 256) llp += ll_part[(size_t)t * ll_tiles + i];
  llp = wave_sum(llp);
  if (lane == 0) llw[wv] = llp;
  __syncthreads();
  if (threadIdx.x == 0) out_ll[t] = (llw[0] + llw[1]) + (llw[2] + llw[3]);
}

}  // namespace

// ------------------------------------------------------------------------
// Launch wrappers
// ------------------------------------------------------------------------
void launch_ancestral_hbm(const LikArgs& a, int count, bool rescale, hipStream_t s) {
  if (count <= 0) return;
  const dim3 grid(a.tiles, count), block(kTile);
  const bool tp = a.tip_partials != nullptr;
  auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, block, 0, s, a); };
  if (rescale) {
    if (tp) go(ancestral_hbm_kernel<true, true>);
    else go(ancestral_hbm_kernel<true, false>);
  } else {
    if (tp) go(ancestral_hbm_kernel<false, true>);
    else go(ancestral_hbm_kernel<false, false>);
  }
}
void launch_ancestral_finalize(const double* ll_part, int T, int ll_tiles, int ll_used, double* out_ll,
                               hipStream_t s) {
  if (T <= 0 || !out_ll) return;
  hipLaunchKernelGGL(ancestral_finalize_kernel, dim3(T), dim3(256), 0, s, ll_part, ll_tiles, ll_used, out_ll);
}
const char* ancestral_kernel_name() { return "ancestral_hbm_kernel"; }

}  // namespace miphylo
