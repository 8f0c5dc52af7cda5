// The NNI neighbourhood scan: the log-likelihood change of both
// nearest-neighbour interchanges across every inner edge of a tree, from ONE post-order and
// pre-order walk.  A member of the HBM-streamed family of kernels_gradient.hip (one lane per
// pattern, one wave per (tree, 64-pattern tile), vectors through the `plv` arena as
// [node][category][pattern][state]), in a file of its own so that every other kernel's code
// stays exactly as it was.  (gfx950 / CDNA4, wave64.)
#include <hip/hip_runtime.h>

#include "mi_phylo_device_utils.h"
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
  const int lane = threadIdx.x;
  const TileEval te = xcd_tile_eval();
  const int tile = te.tile;
  const int e = a.eval_offset + te.eval;
  const int gi = a.grad_offset + te.eval;
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
  double* gout = a.g_part + ((size_t)gi * a.g_tiles + tile) * 2 * N;

  auto plv_at = [&](int node, int k) { return plv_e + ((size_t)(node - n) * K + k) * ppad * 4; };
  auto tip_L = [&](int node) {
    if (TIP_PARTIALS) return load4(a.tip_partials + ((size_t)node * a.P + pc) * 4);
    return tip_vector(a.tip_states[(size_t)node * a.P + pc]);
  };
  auto mat_of = [&](int node, int k) { return mats_e + ((size_t)node * K + k) * 16; };
  // S = P L of a node whose vector is still its post-order one
  auto S_of = [&](int node, int k) {
    return matvec(mat_of(node, k), node < n ? tip_L(node) : load4(plv_at(node, k)));
  };

  for (int i = lane; i < n - 1; i += kTile) nni_place[sched[i].node - n] = i;
  __syncthreads();
  auto entry_of = [&](int node) { return sched[__builtin_amdgcn_readfirstlane(nni_place[node - n])]; };

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
      const double* __restrict__ M0 = mats_e + ((size_t)s.child0 * K + k) * 16;
      const double* __restrict__ M1 = mats_e + ((size_t)s.child1 * K + k) * 16;
      const D4 qv = is_root ? D4{model->pi[0], model->pi[1], model->pi[2], model->pi[3]}
                            : load4(plv_at(s.node, k));
      const D4 L0 = s.child0 < n ? tip_L(s.child0) : load4(plv_at(s.child0, k));
      const D4 L1 = s.child1 < n ? tip_L(s.child1) : load4(plv_at(s.child1, k));
      const D4 A = matvec(M0, L0), B = matvec(M1, L1);
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
      if (s.child0 >= n) {
        store4(plv_at(s.child0, k), q0);
        if (RESCALE) mx0 = fmax(mx0, max4(q0));
      }
      if (s.child1 >= n) {
        store4(plv_at(s.child1, k), q1);
        if (RESCALE) mx1 = fmax(mx1, max4(q1));
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
// Tile reduction and outputs of the scan, a workgroup per tree.  Every column is summed in
// the order reduce_tiles_body (kernels_finalize.hip) sums it -- wave w's share (tiles w, w + 8,
// ... and w + 4, w + 12, ...), then (w0 + w1) + (w2 + w3) -- so the log-likelihood is bit for bit
// that of a gradient call on the HBM path.  delta is [N][2] by node id, 0 where the node is not
// the lower end of an inner edge; the best move is the largest delta, the lowest code 2 v + i
// among equals (NaN entries are passed over), -1 for a three-taxon tree.
// ------------------------------------------------------------------------
__device__ __forceinline__ double nni_wave_share(const double* src, int W, int g_tiles, int col, int wv) {
  double s0 = 0, s1 = 0;
  int i = wv;
  for (; i + 4 < g_tiles; i += 8) {
    s0 += src[(size_t)i * W + col];
    s1 += src[(size_t)(i + 4) * W + col];
  }
  if (i < g_tiles) s0 += src[(size_t)i * W + col];
  return s0 + s1;
}
__device__ __forceinline__ bool nni_better(double v, int code, double best, int best_code) {
  return v > best || (v == best && code < best_code);
}
__global__ __launch_bounds__(256) void nni_finalize_kernel(NniFinalizeArgs a) {
  __shared__ double llw[4];
  __shared__ double best_v[256];
  __shared__ int32_t best_c[256];
  const int t = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int N = a.N, n = a.n, W = 2 * N;
  double llp = 0;
  for (int i = threadIdx.x; i < a.ll_used; i += 256) llp += a.ll_part[(size_t)t * a.ll_tiles + i];
  llp = wave_sum(llp);
  if (lane == 0) llw[wv] = llp;
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
        const int c = q * N + v;
        r[q] = (nni_wave_share(src, W, a.g_tiles, c, 0) + nni_wave_share(src, W, a.g_tiles, c, 1)) +
               (nni_wave_share(src, W, a.g_tiles, c, 2) + nni_wave_share(src, W, a.g_tiles, c, 3));
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
    if (a.out_ll) a.out_ll[t] = (llw[0] + llw[1]) + (llw[2] + llw[3]);
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
  if (count <= 0) return;
  const dim3 grid(a.tiles, count), block(kTile);
  const bool tp = a.tip_partials != nullptr;
  const size_t lds = sizeof(int32_t) * (size_t)(a.n - 1);
  auto go = [&](auto kernel) {
    allow_large_lds(reinterpret_cast<const void*>(kernel), lds);
    hipLaunchKernelGGL(kernel, grid, block, lds, s, a);
  };
  if (rescale) {
    if (tp) go(nni_scan_hbm_kernel<true, true>);
    else go(nni_scan_hbm_kernel<true, false>);
  } else {
    if (tp) go(nni_scan_hbm_kernel<false, true>);
    else go(nni_scan_hbm_kernel<false, false>);
  }
}
void launch_nni_finalize(const NniFinalizeArgs& a, hipStream_t s) {
  if (a.T <= 0) return;
  hipLaunchKernelGGL(nni_finalize_kernel, dim3(a.T), dim3(256), 0, s, a);
}
const char* nni_scan_kernel_name() { return "nni_scan_hbm_kernel"; }

}  // namespace miphylo
