// What the HBM-streamed kernel family shares: gradient_hbm_kernel and
// gradient_hbm_hess_kernel (kernels_gradient.hip), nni_scan_hbm_kernel (kernels_nni.hip),
// ancestral_hbm_kernel (kernels_ancestral.hip), placement_table_hbm_kernel
// (kernels_placement.hip) and spr_vectors_hbm_kernel (kernels_spr.hip), with the finalize kernels that sum their tile partials.  One lane per pattern, one wave per (evaluation, 64-pattern tile), partial-likelihood
// vectors through the `plv` arena as [evaluation][node][category][pattern][state] (32 B per lane,
// a wave reads or writes 2 KiB contiguous).  Each lane only ever re-reads what it wrote itself,
// so no inter-wave synchronisation is needed; the pre-order vector of a node overwrites its
// post-order vector in place once the latter is dead.
// The log-likelihood of every member equals the HBM gradient call's bit for bit, and the tests
// say so: the post-order pass and the tile sums exist once, here.  Everything is
// __forceinline__; each .hip file gets its own copy of the device code.
#pragma once
#include <type_traits>

#include "mi_phylo_device_utils.h"

namespace miphylo {
namespace dev {

// ------------------------------------------------------------------------
// The lane's view of its evaluation: which tree and model, which pattern, where its matrices
// and its column of the vector arena are.
// ------------------------------------------------------------------------
template <bool TIP_PARTIALS>
struct HbmLane {
  const LikArgs& a;
  int lane, tile, eval;  // eval: of this launch (the arena and the partial sums are per launch part)
  int e, t;              // evaluation and tree of the call
  const DevModel* __restrict__ model;
  const SchedEntry* __restrict__ sched;
  int p, pc;  // pattern, and the pattern a padding lane reads instead
  double w;   // pattern weight, 0 on a padding lane
  int K, n, N;
  size_t ppad;
  const double* __restrict__ mats_e;
  double* plv_e;

  __device__ __forceinline__ explicit HbmLane(const LikArgs& args) : a(args) {
    lane = threadIdx.x;
    const TileEval te = xcd_tile_eval();
    tile = te.tile;
    eval = te.eval;
    e = a.eval_offset + te.eval;
    int mi;
    a.map.decode(e, t, mi);
    model = a.models + mi;
    sched = a.sched + (size_t)t * (a.n - 1);
    p = tile * kTile + lane;
    pc = p < a.P ? p : a.P - 1;
    w = p < a.P ? a.weights[pc] : 0.0;
    K = a.K, n = a.n, N = a.N;
    ppad = (size_t)a.tiles * kTile;
    mats_e = a.mats + (size_t)e * (N - 1) * K * 16;
    plv_e = a.plv + (size_t)te.eval * (n - 1) * K * ppad * 4 + (size_t)p * 4;
  }
  __device__ __forceinline__ bool live() const { return p < a.P; }
  // this wave's row of g_part, `width` doubles per (gradient evaluation, tile)
  __device__ __forceinline__ double* g_row(int width) const {
    return a.g_part + ((size_t)(a.grad_offset + eval) * a.g_tiles + tile) * width;
  }
  __device__ __forceinline__ double* plv_at(int node, int k) const {
    return plv_e + ((size_t)(node - n) * K + k) * ppad * 4;
  }
  __device__ __forceinline__ const double* mat_of(int node, int k) const {
    return mats_e + ((size_t)node * K + k) * 16;
  }
  __device__ __forceinline__ D4 tip_L(int node) const {
    if (TIP_PARTIALS) return load4(a.tip_partials + ((size_t)node * a.P + pc) * 4);
    return tip_vector(a.tip_states[(size_t)node * a.P + pc]);
  }
  // the vector of a node: a tip's, or what the arena holds for an internal node
  __device__ __forceinline__ D4 vec_of(int node, int k) const {
    return node < n ? tip_L(node) : load4(plv_at(node, k));
  }
  __device__ __forceinline__ double root_term(int k, D4 L) const {
    return model->cat_weight[k] *
           (model->pi[0] * L.x0 + model->pi[1] * L.x1 + model->pi[2] * L.x2 + model->pi[3] * L.x3);
  }
};

// ------------------------------------------------------------------------
// Post-order pass: every internal node's vector into the arena (the root's is contracted with
// pi instead), then the tile's log-likelihood partial into ll_part.  Returns the lane's own
// unweighted log-likelihood (its pattern's; a padding lane: that of pattern P - 1).
// `tap` sees what the pass otherwise throws away: node(entry, ex) the power of two taken out of
// a node's vectors (rescaling only), root(site, cum_exp) the lane's likelihood site 2^cum_exp.
// ------------------------------------------------------------------------
struct HbmNoTap {
  __device__ __forceinline__ void node(const SchedEntry&, int) const {}
  __device__ __forceinline__ void root(double, int) const {}
};
template <bool RESCALE, bool TIP_PARTIALS, typename Tap = HbmNoTap>
__device__ __forceinline__ double hbm_post_order(const HbmLane<TIP_PARTIALS>& c, const Tap& tap = Tap{}) {
  const int n = c.n, K = c.K;
  int cum_exp = 0;
  double site = 0.0;
  for (int i = 0; i < n - 1; i++) {
    const SchedEntry s = c.sched[i];
    const bool is_root = i == n - 2;
    double mx = 0.0;
    for (int k = 0; k < K; k++) {
      const D4 L = mul4(matvec(c.mat_of(s.child0, k), c.vec_of(s.child0, k)),
                        matvec(c.mat_of(s.child1, k), c.vec_of(s.child1, k)));
      if (RESCALE) mx = fmax(mx, max4(L));
      if (is_root && !RESCALE) {
        site += c.root_term(k, L);
      } else {
        store4(c.plv_at(s.node, k), L);
      }
    }
    if (RESCALE) {
      // common exponent across categories (the ratio in the edge derivative needs it)
      const int ex = max_exponent(mx);
      cum_exp += ex;
      tap.node(s, ex);
      for (int k = 0; k < K; k++) {
        const D4 L = scale4(load4(c.plv_at(s.node, k)), -ex);
        if (is_root)
          site += c.root_term(k, L);
        else
          store4(c.plv_at(s.node, k), L);
      }
    }
  }
  tap.root(site, cum_exp);
  double ll = log(site);
  if (RESCALE) ll += cum_exp * 0.6931471805599453;
  const double lane_ll = ll;
  ll = c.live() ? c.w * ll : 0.0;
  ll = wave_sum(ll);
  if (c.lane == 0) c.a.ll_part[(size_t)c.e * c.a.ll_tiles + c.tile] = ll;
  return lane_ll;
}

// ------------------------------------------------------------------------
// Pre-order visit of schedule entry s (parents before children), category k.  The operands:
// the children's matrices and vectors, A = P_0 L_0, B = P_1 L_1, and qv = the node's own
// pre-order vector (pi at the set-up root).  A member forms q0 = M0^T (qv o B), q1 = M1^T (qv o A)
// from them, keeps what it wants, and hands q0 / q1 to hbm_store_children.
// ------------------------------------------------------------------------
struct HbmVisit {
  const double* __restrict__ M0;
  const double* __restrict__ M1;
  D4 qv, L0, L1, A, B;
};
template <bool TIP_PARTIALS>
__device__ __forceinline__ HbmVisit hbm_visit_operands(const HbmLane<TIP_PARTIALS>& c, const SchedEntry& s,
                                                       bool is_root, int k) {
  HbmVisit v;
  v.M0 = c.mat_of(s.child0, k);
  v.M1 = c.mat_of(s.child1, k);
  v.qv = is_root ? D4{c.model->pi[0], c.model->pi[1], c.model->pi[2], c.model->pi[3]}
                 : load4(c.plv_at(s.node, k));
  v.L0 = c.vec_of(s.child0, k);
  v.L1 = c.vec_of(s.child1, k);
  v.A = matvec(v.M0, v.L0);
  v.B = matvec(v.M1, v.L1);
  return v;
}
// the pre-order vectors of the internal children, over their post-order ones; mx0 / mx1: the
// running maxima over the categories (rescaling)
template <bool RESCALE, bool TIP_PARTIALS>
__device__ __forceinline__ void hbm_store_children(const HbmLane<TIP_PARTIALS>& c, const SchedEntry& s, int k,
                                                   D4 q0, D4 q1, double& mx0, double& mx1) {
  if (s.child0 >= c.n) {
    store4(c.plv_at(s.child0, k), q0);
    if (RESCALE) mx0 = fmax(mx0, max4(q0));
  }
  if (s.child1 >= c.n) {
    store4(c.plv_at(s.child1, k), q1);
    if (RESCALE) mx1 = fmax(mx1, max4(q1));
  }
}
// after the category loop: each internal child's vectors by their common exponent
template <bool RESCALE, bool TIP_PARTIALS>
__device__ __forceinline__ void hbm_rescale_children(const HbmLane<TIP_PARTIALS>& c, const SchedEntry& s,
                                                     double mx0, double mx1) {
  if (!RESCALE) return;
  if (s.child0 >= c.n) {
    const int ex = max_exponent(mx0);
    for (int k = 0; k < c.K; k++)
      store4(c.plv_at(s.child0, k), scale4(load4(c.plv_at(s.child0, k)), -ex));
  }
  if (s.child1 >= c.n) {
    const int ex = max_exponent(mx1);
    for (int k = 0; k < c.K; k++)
      store4(c.plv_at(s.child1, k), scale4(load4(c.plv_at(s.child1, k)), -ex));
  }
}

// ------------------------------------------------------------------------
// Tile sums of a finalize kernel (256 threads, a workgroup per tree), in the order
// reduce_tiles_body (kernels_finalize.hip) sums them, so that every member's log-likelihood and
// the Hessian call's gradient are bit for bit those of a gradient call on the HBM path.
// A column of g_part ([g_tiles][W]): wave w's share is tiles w, w + 8, ... and w + 4, w + 12, ...;
// then (w0 + w1) + (w2 + w3) -- here all four by the one thread that owns the column.
// ------------------------------------------------------------------------
__device__ __forceinline__ double wave_share(const double* src, int W, int g_tiles, int col, int wv) {
  double s0 = 0, s1 = 0;
  int i = wv;
  for (; i + 4 < g_tiles; i += 8) {
    s0 += src[(size_t)i * W + col];
    s1 += src[(size_t)(i + 4) * W + col];
  }
  if (i < g_tiles) s0 += src[(size_t)i * W + col];
  return s0 + s1;
}
__device__ __forceinline__ double tile_column_sum(const double* src, int W, int g_tiles, int col) {
  return (wave_share(src, W, g_tiles, col, 0) + wave_share(src, W, g_tiles, col, 1)) +
         (wave_share(src, W, g_tiles, col, 2) + wave_share(src, W, g_tiles, col, 3));
}
// The log-likelihood partials of a tree: thread i takes partials i, i + 256, ...; a wave's 64 by
// wave_sum into llw[wave].  After a __syncthreads() the tree's sum is ll_tile_total(llw).
__device__ __forceinline__ void ll_tile_shares(const double* ll_part_t, int ll_used, double* llw /* LDS [4] */) {
  double llp = 0;
  for (int i = threadIdx.x; i < ll_used; i += 256) llp += ll_part_t[i];
  llp = wave_sum(llp);
  if ((threadIdx.x & 63) == 0) llw[threadIdx.x >> 6] = llp;
}
__device__ __forceinline__ double ll_tile_total(const double* llw) { return (llw[0] + llw[1]) + (llw[2] + llw[3]); }

}  // namespace dev

// ------------------------------------------------------------------------
// Launch of a member: `pick(rescale, tip_partials)` names the instantiation (both arrive as
// std::true_type / std::false_type); `lds`: dynamic LDS of the workgroup.
// ------------------------------------------------------------------------
using HbmKernel = void (*)(LikArgs);
template <typename Pick>
inline void launch_hbm_member(const LikArgs& a, int count, bool rescale, size_t lds, hipStream_t s, Pick pick) {
  if (count <= 0) return;
  const bool tp = a.tip_partials != nullptr;
  using Yes = std::true_type;
  using No = std::false_type;
  const HbmKernel kernel = rescale ? (tp ? pick(Yes{}, Yes{}) : pick(Yes{}, No{}))
                                   : (tp ? pick(No{}, Yes{}) : pick(No{}, No{}));
  allow_large_lds(reinterpret_cast<const void*>(kernel), lds);
  hipLaunchKernelGGL(kernel, dim3(a.tiles, count), dim3(kTile), lds, s, a);
}

}  // namespace miphylo
