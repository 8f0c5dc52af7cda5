// Phylogenetic placement: score query sequences on every edge of a tree that is
// already built.  Three steps, all plain C++ with vector stores (gfx950 / CDNA4, wave64):
//   placement_table_hbm_kernel   a member of the HBM-streamed family (mi_phylo_hbm_walk_device.h,
//                                DESIGN.md 4.15): per caller edge, pendant length and pattern the
//                                five log-likelihoods S of "the query shows A / C / G / T / gap"
//                                at the edge's midpoint
//   placement_score_kernel       the hot path: sum_c w_c S[e][g][pattern(c)][x[q][c]] per (query,
//                                edge, pendant length) -- a gather-and-sum over the edge's table,
//                                which a workgroup holds in LDS --, and the maximum over g
//   placement_finalize_kernel    best edge and likelihood weight ratios per (tree, query), the
//                                trees' log-likelihoods by the family's tile sums
#include <hip/hip_runtime.h>

#include "mi_phylo_device_utils.h"
#include "mi_phylo_hbm_walk_device.h"
#include "mi_phylo_kernels.h"

namespace miphylo {

namespace {
using namespace dev;

constexpr int kG = kPlacementMaxPendants;

__device__ __forceinline__ void add_scaled4(D4& acc, double c, D4 v) {
  acc.x0 += c * v.x0;
  acc.x1 += c * v.x1;
  acc.x2 += c * v.x2;
  acc.x3 += c * v.x3;
}

// ------------------------------------------------------------------------
// The table entries of the edge above child `side` of schedule entry s (x, never 2n-3: the
// set-up tree's zero-length edge above R is no caller edge).  With g = qv o (sibling message) at
// the top of the edge, L = L_x at its bottom and H = P(r_k t_x / 2):
//   M_k = (H^T g) o (H L)                         the joint of the midpoint's state and the data
//   Z[g][a] = sum_k c_k sum_j M_k[j] R_g,k[j][a]   R_g,k = P(r_k l_g)
//   S[g][a] = s + log(Z[g][a] / ((Z[0] + Z[1]) + (Z[2] + Z[3]))),   S[g][4] = s
// One child at a time, so that one set of 4 G accumulators is live.  The operands are read
// before the visit's own category loop overwrites the child's slot.  Every power of two that
// rescaling removed sits in all four Z[g][.] alike.
// ------------------------------------------------------------------------
template <bool TIP_PARTIALS>
__device__ __forceinline__ void placement_edge(const HbmLane<TIP_PARTIALS>& c, const SchedEntry& s, bool is_root,
                                               int side, double s_p) {
  const LikArgs& a = c.a;
  const int x = side ? s.child1 : s.child0;
  const int G = a.place_G, K = c.K;
  const double* __restrict__ half_e = a.place_half + (size_t)c.e * (c.N - 1) * K * 16;
  const double* __restrict__ pend_t = a.place_pend + (size_t)c.t * G * K * 16;
  D4 Z[kG];
#pragma unroll
  for (int g = 0; g < kG; g++) Z[g] = D4{0, 0, 0, 0};
  for (int k = 0; k < K; k++) {
    const HbmVisit v = hbm_visit_operands(c, s, is_root, k);
    const D4 top = side ? mul4(v.qv, v.A) : mul4(v.qv, v.B);
    const D4 L = side ? v.L1 : v.L0;
    const double* __restrict__ H = half_e + ((size_t)x * K + k) * 16;
    const D4 M = mul4(matTvec(H, top), matvec(H, L));
    const double cw = c.model->cat_weight[k];
#pragma unroll
    for (int g = 0; g < kG; g++)
      if (g < G) add_scaled4(Z[g], cw, matTvec(pend_t + ((size_t)g * K + k) * 16, M));
  }
  // [tree of the launch][edge][g][code][pattern]: lane p stores 8 B, the wave 512 B contiguous
  const size_t E = 2 * (size_t)c.n - 3;
  double* out = a.place_table + (((size_t)(c.t - a.place_tree0) * E + x) * G) * 5 * c.ppad + c.p;
#pragma unroll
  for (int g = 0; g < kG; g++)
    if (g < G) {
      const double sum = (Z[g].x0 + Z[g].x1) + (Z[g].x2 + Z[g].x3);
      double* row = out + (size_t)g * 5 * c.ppad;
      row[0] = s_p + log(Z[g].x0 / sum);
      row[c.ppad] = s_p + log(Z[g].x1 / sum);
      row[2 * c.ppad] = s_p + log(Z[g].x2 / sum);
      row[3 * c.ppad] = s_p + log(Z[g].x3 / sum);
      row[4 * c.ppad] = s_p;
    }
}

// ------------------------------------------------------------------------
// The walk of ancestral_hbm_kernel with the table instead of the posteriors.  Post-order: the
// family's (log-likelihood partial bit for bit; the lane keeps its pattern's s).  Pre-order,
// parents before children: at the visit of u the edges above its children are scored
// (placement_edge), then the children's pre-order vectors replace their post-order ones as in
// every member.  The set-up tree has B = 2n-2 with children (c0, R) and R = 2n-3 with children
// (c1, c2): the three root edges come from B's visit (c0: top = pi o L_R) and R's visit (c1, c2:
// q_R = pi o P_c0 L_c0), B's child R is skipped.  Lanes beyond P repeat pattern P - 1 into the
// padding of their tile's row, which nobody reads.
// ------------------------------------------------------------------------
template <bool RESCALE, bool TIP_PARTIALS>
__global__ __launch_bounds__(kTile) void placement_table_hbm_kernel(LikArgs a) {
  const HbmLane<TIP_PARTIALS> c(a);
  const int K = c.K, n = c.n;

  const double s_p = hbm_post_order<RESCALE>(c);

  for (int i = n - 2; i >= 0; i--) {
    const SchedEntry s = c.sched[i];
    const bool is_root = i == n - 2;
    if (s.child0 != 2 * n - 3) placement_edge(c, s, is_root, 0, s_p);
    if (s.child1 != 2 * n - 3) placement_edge(c, s, is_root, 1, s_p);
    double mx0 = 0, mx1 = 0;
    for (int k = 0; k < K; k++) {
      const HbmVisit v = hbm_visit_operands(c, s, is_root, k);
      const D4 q0 = matTvec(v.M0, mul4(v.qv, v.B));
      const D4 q1 = matTvec(v.M1, mul4(v.qv, v.A));
      hbm_store_children<RESCALE>(c, s, k, q0, q1, mx0, mx1);
    }
    hbm_rescale_children<RESCALE>(c, s, mx0, mx1);
  }
}

// ------------------------------------------------------------------------
// Before the walk: halved effective lengths, the pendant lengths as one row per tree (the two
// extra launches of transition_kernel read them), and what a device-pointer call cannot check on
// the host.
// ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void placement_prepare_kernel(PlacePrepareArgs a) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < (size_t)a.T * a.N) a.half_bl[i] = 0.5 * a.bl_eff[i];
  if (i < (size_t)a.T * (a.G + 1)) {
    const int g = (int)(i % (a.G + 1));
    const double l = g < a.G ? a.pendant_lengths[g] : 0.0;
    a.pend_bl[i] = l;
    if (i < (size_t)a.G && !(l >= 0.0 && l <= 1.79769313486231570e308)) set_status(a.status, kBadPendantLength, g);
  }
  if (i < (size_t)a.C) {
    const int cp = a.column_pattern[i];
    if (cp < 0 || cp >= a.P) set_status(a.status, kBadColumnPattern, (int)i);
  }
}

// ------------------------------------------------------------------------
// The scoring.  Workgroup (query block, edge, tree): the edge's table [G][5][ppad] into LDS
// (LDS == true) or left where it is, then wave w of four takes the block's queries w, w + 4, ...
// THE ORDER (part of the interface, include/mi_phylo.h): for one (tree, query, edge, g), lane l
// of the wave adds w_c S[...] of the columns c = l, l + 64, l + 128, ... in ascending c, each
// term by one fused multiply-add into its running sum starting from +0.0 (columns of weight 0
// are skipped); the 64 running sums are added by the xor butterfly of wave_sum (offsets 32, 16,
// 8, 4, 2, 1).  It depends on C alone: not on Q, E, G, T, on the place in the launch, on how
// the call was cut into launches, nor on where the table is read from.
// LDS layout [g][code][ppad], ppad a multiple of 64: the byte address of (g, code, p) is
// 8 (g 5 + code) ppad + 8 p, so its bank (a / 4) mod 64 = 2 p mod 64 whatever the lane's code
// and g -- under the identity column map the 32 lanes of a half read 32 distinct even banks
// (and the odd ones with them): conflict-free ds_read_b64.
// A column_pattern entry outside [0, P) has been reported by placement_prepare_kernel; here it
// is clamped so that nothing is read out of bounds.
// ------------------------------------------------------------------------
template <bool LDS>
__global__ __launch_bounds__(256) void placement_score_kernel(PlaceScoreArgs a) {
  extern __shared__ double lds_table[];
  const int e = blockIdx.y, tl = blockIdx.z;
  const size_t row = (size_t)a.G * 5 * a.ppad;
  const double* __restrict__ src = a.table + ((size_t)tl * a.E + e) * row;
  const double* tab;
  if (LDS) {
    for (size_t i = threadIdx.x; i < row; i += 256) lds_table[i] = src[i];
    __syncthreads();
    tab = lds_table;
  } else {
    tab = src;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int t = a.tree0 + tl;
  const int q_end = min(a.Q, (int)(blockIdx.x + 1) * kPlacementQueryBlock);
  for (int q = blockIdx.x * kPlacementQueryBlock + wave; q < q_end; q += 4) {
    const int8_t* __restrict__ xq = a.query_states + (size_t)q * a.C;
    double acc[kG];
#pragma unroll
    for (int g = 0; g < kG; g++) acc[g] = 0.0;
    for (int c = lane; c < a.C; c += 64) {
      const double w = a.column_weights ? a.column_weights[c] : 1.0;
      if (w == 0.0) continue;
      const int xc = xq[c];
      const int code = (unsigned)xc < 4u ? xc : 4;
      int cp = a.column_pattern[c];
      cp = cp < 0 ? 0 : (cp >= a.P ? a.P - 1 : cp);
      const double* entry = tab + (size_t)code * a.ppad + cp;
#pragma unroll
      for (int g = 0; g < kG; g++)
        if (g < a.G) acc[g] = fma(w, entry[(size_t)g * 5 * a.ppad], acc[g]);
    }
    double best = 0.0;
    int best_g = 0;
#pragma unroll
    for (int g = 0; g < kG; g++)
      if (g < a.G) {
        const double ll = wave_sum(acc[g]);
        if (g == 0 || ll > best) {
          best = ll;
          best_g = g;
        }
      }
    if (lane == 0) {
      const size_t o = ((size_t)t * a.Q + q) * a.E + e;
      a.edge_ll[o] = best;
      if (a.pendant_index) a.pendant_index[o] = (int8_t)best_g;
    }
  }
}

// S for the caller: the padded rows of the workspace into [T][E][G][5][P]
// (rows: the (tree, edge, g, code) of this launch; `out` begins at its first tree)
__global__ __launch_bounds__(256) void placement_table_copy_kernel(const double* __restrict__ table, int P,
                                                                   size_t ppad, size_t rows,
                                                                   double* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * P) return;
  const size_t r = i / P, p = i - r * P;
  out[i] = table[r * ppad + p];
}

// ------------------------------------------------------------------------
// Per (tree, query), one thread: the edge of the largest edge_ll (the lowest among equals) and
// the likelihood weight ratios exp(edge_ll - m) / sum_e' exp(edge_ll[e'] - m), the sum in
// ascending e.  Then, a workgroup per tree, the log-likelihoods by the family's tile sums: those
// of a gradient call on the HBM path, bit for bit.
// ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void placement_finalize_kernel(PlaceFinalizeArgs a) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)a.T * a.Q) return;
  const double* __restrict__ row = a.edge_ll + i * a.E;
  double m = row[0];
  int best = 0;
  for (int e = 1; e < a.E; e++)
    if (row[e] > m) {
      m = row[e];
      best = e;
    }
  if (a.out_best_edge) a.out_best_edge[i] = best;
  if (a.out_lwr) {
    double sum = 0.0;
    for (int e = 0; e < a.E; e++) sum += exp(row[e] - m);
    double* out = a.out_lwr + i * a.E;
    for (int e = 0; e < a.E; e++) out[e] = exp(row[e] - m) / sum;
  }
}
__global__ __launch_bounds__(256) void placement_ll_kernel(const double* __restrict__ ll_part, int ll_tiles,
                                                           int ll_used, double* __restrict__ out_ll) {
  __shared__ double llw[4];
  const int t = blockIdx.x;
  ll_tile_shares(ll_part + (size_t)t * ll_tiles, ll_used, llw);
  __syncthreads();
  if (threadIdx.x == 0) out_ll[t] = ll_tile_total(llw);
}

constexpr size_t kScoreLdsLimit = 160 * 1024 - 1024;

}  // namespace

// ------------------------------------------------------------------------
// Launch wrappers
// ------------------------------------------------------------------------
void launch_placement_table_hbm(const LikArgs& a, int count, bool rescale, hipStream_t s) {
  launch_hbm_member(a, count, rescale, 0, s, [](auto R, auto TP) -> HbmKernel {
    return placement_table_hbm_kernel<decltype(R)::value, decltype(TP)::value>;
  });
}
const char* placement_kernel_name() { return "placement_table_hbm_kernel"; }

void launch_placement_prepare(const PlacePrepareArgs& a, hipStream_t s) {
  const size_t items = std::max(std::max((size_t)a.T * a.N, (size_t)a.T * (a.G + 1)), (size_t)a.C);
  hipLaunchKernelGGL(placement_prepare_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, a);
}

bool placement_table_fits_lds(int G, size_t ppad) { return sizeof(double) * G * 5 * ppad <= kScoreLdsLimit; }

void launch_placement_score(const PlaceScoreArgs& a, hipStream_t s) {
  if (a.trees <= 0) return;
  const dim3 grid((a.Q + kPlacementQueryBlock - 1) / kPlacementQueryBlock, a.E, a.trees);
  if (a.use_lds) {
    const size_t lds = sizeof(double) * a.G * 5 * a.ppad;
    allow_large_lds(reinterpret_cast<const void*>(placement_score_kernel<true>), lds);
    hipLaunchKernelGGL(placement_score_kernel<true>, grid, dim3(256), lds, s, a);
  } else {
    hipLaunchKernelGGL(placement_score_kernel<false>, grid, dim3(256), 0, s, a);
  }
}

void launch_placement_table_copy(const double* table, int trees, int tree0, int E, int G, int P, size_t ppad,
                                 double* out, hipStream_t s) {
  const size_t rows = (size_t)trees * E * G * 5;
  hipLaunchKernelGGL(placement_table_copy_kernel, dim3((unsigned)((rows * P + 255) / 256)), dim3(256), 0, s,
                     table, P, ppad, rows, out + (size_t)tree0 * E * G * 5 * P);
}

void launch_placement_finalize(const PlaceFinalizeArgs& a, hipStream_t s) {
  if (a.out_best_edge || a.out_lwr) {
    const size_t items = (size_t)a.T * a.Q;
    hipLaunchKernelGGL(placement_finalize_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, a);
  }
  if (a.out_ll)
    hipLaunchKernelGGL(placement_ll_kernel, dim3(a.T), dim3(256), 0, s, a.ll_part, a.ll_tiles, a.ll_used,
                       a.out_ll);
}

}  // namespace miphylo
