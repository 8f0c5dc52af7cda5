// The SPR neighbourhood scan: the log-likelihood change of every move "cut this
// edge, re-attach the loose part on the midpoint of that edge" of a tree at given branch lengths.
// Plain C++ with vector stores (gfx950 / CDNA4, wave64), no floating-point atomics:
//   spr_vectors_hbm_kernel   the sixth member of the HBM-streamed family
//                            (mi_phylo_hbm_walk_device.h): the family's post-order
//                            pass, then a pre-order pass into a SECOND arena -- the scan needs both
//                            directions at every edge --, and beside both arenas the cumulative
//                            power of two that rescaling took out of every stored vector
//   spr_regraft_kernel       the hot path: a wave takes a (tree, 64-pattern tile, pruned edge s)
//                            and walks outward from the prune point over the pruned tree, depth
//                            first: per target edge and category four matrix-vector products
//                            (side branch, two half-edge products for the score, the onward
//                            message)
//   spr_finalize_kernel      tile sums in the family's order, the table, the best target per
//                            (s, dir), the best move per tree, the trees' log-likelihoods
// Every vector here is CONDITIONAL on the state at its node (no stationary frequencies inside):
// for the reversible models of the engine pi_i P_ij = pi_j P_ji, so such vectors are carried by
// P in either direction along an edge and pi enters once, at the point where a score is formed.
// That makes the tree an unrooted graph for the regraft walk: no case for "through the root".
#include <hip/hip_runtime.h>

#include "mi_phylo_device_utils.h"
#include "mi_phylo_hbm_walk_device.h"
#include "mi_phylo_kernels.h"

namespace miphylo {

namespace {
using namespace dev;

constexpr double kLn2 = 0.6931471805599453;

// a value every lane of the wave holds alike (the tree and the walk's frames, read from LDS), as a
// scalar: the matrices it addresses then come by scalar loads and the branches on it are uniform
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// ------------------------------------------------------------------------
// What the post-order pass hands over (hbm_post_order's tap): the cumulative exponent below every
// internal node, and the root's mantissa and exponent -- L_p = site 2^site_exp.
// ------------------------------------------------------------------------
struct SprTap {
  int32_t* exp_down;  // the lane's column of [n-1][ppad]
  double* site;
  int32_t* site_exp;
  int n;
  size_t ppad;
  __device__ __forceinline__ int below(int node) const { return node < n ? 0 : exp_down[(size_t)(node - n) * ppad]; }
  __device__ __forceinline__ void node(const SchedEntry& s, int ex) const {
    exp_down[(size_t)(s.node - n) * ppad] = ex + below(s.child0) + below(s.child1);
  }
  __device__ __forceinline__ void root(double mantissa, int cum_exp) const {
    *site = mantissa;
    *site_exp = cum_exp;
  }
};

// ------------------------------------------------------------------------
// The walk.  Post-order: the family's, bit for bit (log-likelihood partial included).  Pre-order,
// parents before children: U_c, the vector at the TOP of the edge above c -- everything outside
// clade c, conditional on the state there -- for every node c of the set-up tree but its root:
//   U_c0 = Q o (P_c1 D_c1),  U_c1 = Q o (P_c0 D_c0),   Q = P_v U_v  (1 at the set-up root)
// into `up` [tree of the launch][2n-2 nodes][K][ppad][4]; D stays where the post-order pass put
// it.  Rescaling: one common exponent per stored vector over the categories, as the family's;
// exp_up / exp_down hold the cumulative ones.  Lanes beyond P repeat pattern P - 1 into padding.
// ------------------------------------------------------------------------
template <bool RESCALE, bool TIP_PARTIALS>
__global__ __launch_bounds__(kTile) void spr_vectors_hbm_kernel(LikArgs a, SprArgs w) {
  const HbmLane<TIP_PARTIALS> c(a);
  const int K = c.K, n = c.n;
  const size_t ppad = c.ppad, col = (size_t)c.eval * ppad + c.p;
  SprTap tap;
  tap.exp_down = w.exp_down + (size_t)c.eval * (n - 1) * ppad + c.p;
  tap.site = w.site + col;
  tap.site_exp = w.site_exp + col;
  tap.n = n;
  tap.ppad = ppad;
  hbm_post_order<RESCALE>(c, tap);

  double* up_e = w.up + (size_t)c.eval * (2 * n - 2) * K * ppad * 4 + (size_t)c.p * 4;
  int32_t* eu = w.exp_up + (size_t)c.eval * (2 * n - 2) * ppad + c.p;
  auto up_at = [&](int node, int k) { return up_e + ((size_t)node * K + k) * ppad * 4; };
  for (int i = n - 2; i >= 0; i--) {
    const SchedEntry s = c.sched[i];
    const bool is_root = i == n - 2;
    double mx0 = 0, mx1 = 0;
    for (int k = 0; k < K; k++) {
      const D4 Q = is_root ? D4{1.0, 1.0, 1.0, 1.0} : matvec(c.mat_of(s.node, k), load4(up_at(s.node, k)));
      const D4 A = matvec(c.mat_of(s.child0, k), c.vec_of(s.child0, k));
      const D4 B = matvec(c.mat_of(s.child1, k), c.vec_of(s.child1, k));
      const D4 u0 = mul4(Q, B), u1 = mul4(Q, A);
      store4(up_at(s.child0, k), u0);
      store4(up_at(s.child1, k), u1);
      if (RESCALE) {
        mx0 = fmax(mx0, max4(u0));
        mx1 = fmax(mx1, max4(u1));
      }
    }
    if (RESCALE) {
      const int above = is_root ? 0 : eu[(size_t)s.node * ppad];
      const int ex0 = max_exponent(mx0), ex1 = max_exponent(mx1);
      for (int k = 0; k < K; k++) {
        store4(up_at(s.child0, k), scale4(load4(up_at(s.child0, k)), -ex0));
        store4(up_at(s.child1, k), scale4(load4(up_at(s.child1, k)), -ex1));
      }
      eu[(size_t)s.child0 * ppad] = above + tap.below(s.child1) + ex0;
      eu[(size_t)s.child1 * ppad] = above + tap.below(s.child0) + ex1;
    }
  }
}

// halved effective lengths: transition_kernel makes P(r_k t_e / 2) of them
__global__ __launch_bounds__(256) void spr_half_lengths_kernel(const double* __restrict__ bl_eff, size_t count,
                                                               double* __restrict__ half_bl) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < count) half_bl[i] = 0.5 * bl_eff[i];
}

// "no such move" into the first tile's plane of the partial table: the regraft kernel writes the
// entries of the moves there are, in every tile's plane
__global__ __launch_bounds__(256) void spr_blank_kernel(SprArgs a) {
  const size_t W = 2 * (size_t)(2 * a.n - 3) * (2 * a.n - 3);
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)a.trees * W) return;
  const size_t tl = i / W;
  a.part[tl * a.tiles * W + (i - tl * W)] = -__builtin_huge_val();
}

// ------------------------------------------------------------------------
// The regraft walk's view of its tree, pattern and workspaces.  The tree is the caller's, as an
// unrooted graph (LDS): nb[0] the parent, nb[1] / nb[2] the children; the trifurcating root
// R = 2n-3 has its first child in the parent's place (and that child R as its parent).  A
// neighbour z of x lies BELOW x if z != R and par[z] == x.
//   into(x <- z)   everything behind z as seen from x, carried to x:  P_z D_z below, P_x U_x above
//   beyond(x -> z) the stored vector at the far end of the edge, not carried: D_z below, U_x above
//                  (the edge is the caller's edge z below, x above)
// ------------------------------------------------------------------------
template <bool RESCALE, bool TIP_PARTIALS>
struct SprLane {
  const SprArgs& a;
  const int32_t* par;
  const int32_t* kid0;
  const int32_t* kid1;
  int n, K, R, lane, tl, t, tile, p, pc;
  size_t ppad;
  double w;
  const DevModel* __restrict__ model;
  cdouble_ptr mats_t;
  cdouble_ptr half_t;
  const double* down_l;  // the lane's column of the launch tree's vectors
  const double* up_l;
  const int32_t* ed_l;
  const int32_t* eu_l;
  double* path_l;        // [depth_slots + 1][K][64][4]: the lane's column; the last slot is the moving part
  int32_t* path_exp_l;   // [depth_slots][64]

  __device__ __forceinline__ bool below(int z, int x) const { return z != R && uniform(par[z]) == x; }
  __device__ __forceinline__ cdouble_ptr mat(int node, int k) const { return mats_t + ((size_t)node * K + k) * 16; }
  __device__ __forceinline__ cdouble_ptr half(int node, int k) const { return half_t + ((size_t)node * K + k) * 16; }
  __device__ __forceinline__ D4 D(int z, int k) const {
    if (z < n) {
      if (TIP_PARTIALS) return load4(a.tip_partials + ((size_t)z * a.P + pc) * 4);
      return tip_vector(a.tip_states[(size_t)z * a.P + pc]);
    }
    return load4(down_l + ((size_t)(z - n) * K + k) * ppad * 4);
  }
  __device__ __forceinline__ D4 U(int x, int k) const { return load4(up_l + ((size_t)x * K + k) * ppad * 4); }
  __device__ __forceinline__ int eD(int z) const { return (RESCALE && z >= n) ? ed_l[(size_t)(z - n) * ppad] : 0; }
  __device__ __forceinline__ int eU(int x) const { return RESCALE ? eu_l[(size_t)x * ppad] : 0; }
  __device__ __forceinline__ D4 into(int x, int z, int k) const {
    return below(z, x) ? matvec(mat(z, k), D(z, k)) : matvec(mat(x, k), U(x, k));
  }
  __device__ __forceinline__ int into_exp(int x, int z) const { return below(z, x) ? eD(z) : eU(x); }
  __device__ __forceinline__ double* slot(int depth, int k) const {
    return path_l + ((size_t)depth * K + k) * kTile * 4;
  }
  // a freshly stored message of K categories: by its common exponent (returned), in place
  __device__ __forceinline__ int settle(int depth, double mx) const {
    if (!RESCALE) return 0;
    const int ex = max_exponent(mx);
    for (int k = 0; k < K; k++) store4(slot(depth, k), scale4(load4(slot(depth, k)), -ex));
    return ex;
  }
};

// ------------------------------------------------------------------------
// One target: the walk stands at node x with the message of path slot `depth` (everything behind
// the edge it came by), `zt` is the neighbour whose edge f is scored, `zs` the side branch.
//   a   = message o into(x <- zs)                  everything but zt's side, at x
//   L'  = sum_k c_k sum_j pi_j (H a)[j] (H b)[j] V[j]     H = P(r_k t_f / 2), b = beyond(x -> zt),
//                                                          V = the moving part on its branch
//   the wave's sum of w_p (log(L'_p / L_p) + (exponent difference) ln 2) into the tile's plane
// and, if the walk goes on through zt, the next message P_f a into slot depth + 1.
// ------------------------------------------------------------------------
template <bool RESCALE, bool TIP_PARTIALS>
__device__ __forceinline__ void spr_target(const SprLane<RESCALE, TIP_PARTIALS>& c, int x, int zt, int zs, int depth,
                                           bool go_on, int moving_exp, double site, int site_exp, size_t out_index) {
  const int K = c.K;
  const bool down = c.below(zt, x);
  const int f = down ? zt : x;
  double Z = 0.0, mx = 0.0;
  for (int k = 0; k < K; k++) {
    const D4 av = mul4(load4(c.slot(depth, k)), c.into(x, zs, k));
    const D4 b = down ? c.D(zt, k) : c.U(x, k);
    const D4 ha = matvec(c.half(f, k), av), hb = matvec(c.half(f, k), b);
    const D4 v = load4(c.slot(c.a.depth_slots, k));
    Z += c.model->cat_weight[k] * (c.model->pi[0] * (ha.x0 * hb.x0 * v.x0) + c.model->pi[1] * (ha.x1 * hb.x1 * v.x1) +
                                   c.model->pi[2] * (ha.x2 * hb.x2 * v.x2) + c.model->pi[3] * (ha.x3 * hb.x3 * v.x3));
    if (go_on) {
      const D4 next = matvec(c.mat(f, k), av);
      store4(c.slot(depth + 1, k), next);
      if (RESCALE) mx = fmax(mx, max4(next));
    }
  }
  int ea = 0;
  if (RESCALE) {
    ea = c.path_exp_l[(size_t)depth * kTile] + c.into_exp(x, zs);
    if (go_on) c.path_exp_l[(size_t)(depth + 1) * kTile] = ea + c.settle(depth + 1, mx);
  }
  double term = 0.0;
  if (c.p < c.a.P && c.w != 0.0) {
    double d = log(Z / site);
    if (RESCALE) d += (double)(ea + (down ? c.eD(zt) : c.eU(x)) + moving_exp - site_exp) * kLn2;
    term = c.w * d;
  }
  term = wave_sum(term);
  if (c.lane == 0) c.a.part[out_index + f] = term;
}

// ------------------------------------------------------------------------
// A wave per job = (tree of the launch, tile, pruned edge s), both directions of s; the grid is
// a.waves workgroups of one wave that take job after job (each owns a path workspace; which wave
// takes a job changes no result).  LDS: the tree [3][2n-2], the frames of the walk [3][depth_slots].
// A prune is (hub h, moving neighbour mv): dir 0 (h, mv) = (parent of s, s), dir 1 = (s, parent of
// s).  h goes, its other neighbours z1 and z2 are joined: the walk starts at z1 with the message
// P_(h,z1) into(h <- z2) and at z2 with P_(h,z2) into(h <- z1) -- the merged edge's two stored
// matrices in turn.  A frame is (node, where it was entered from, which of its two other
// neighbours is next); the distance of a frame's targets is its depth + 1.
// ------------------------------------------------------------------------
template <bool RESCALE, bool TIP_PARTIALS>
__global__ __launch_bounds__(kTile) void spr_regraft_kernel(SprArgs a) {
  extern __shared__ int32_t spr_lds[];
  const int n = a.n, K = a.K, V = 2 * n - 2, E = 2 * n - 3, R = 2 * n - 3, slots = a.depth_slots;
  int32_t* par = spr_lds;
  int32_t* kid0 = par + V;
  int32_t* kid1 = kid0 + V;
  int32_t* fr_node = kid1 + V;
  int32_t* fr_from = fr_node + slots;
  int32_t* fr_next = fr_from + slots;
  int32_t* valid = fr_next + slots;
  const int lane = threadIdx.x;
  const size_t ppad = (size_t)a.tiles * kTile, W = 2 * (size_t)E * E;

  SprLane<RESCALE, TIP_PARTIALS> c{a, par, kid0, kid1};
  c.n = n, c.K = K, c.R = R, c.lane = lane, c.ppad = ppad;
  c.path_l = a.path + (size_t)blockIdx.x * (slots + 1) * K * kTile * 4 + (size_t)lane * 4;
  c.path_exp_l = a.path_exp + (size_t)blockIdx.x * slots * kTile + lane;

  const long jobs = (long)a.trees * a.tiles * E;
  int have_tree = -1;
  for (long job = blockIdx.x; job < jobs; job += gridDim.x) {
    const int s = (int)(job % E), tile = (int)((job / E) % a.tiles), tl = (int)(job / ((long)E * a.tiles));
    const int t = a.tree0 + tl;
    if (tl != have_tree) {
      __syncthreads();
      for (int v = lane; v < V; v += kTile) par[v] = -1, kid0[v] = 0, kid1[v] = 0;
      if (lane == 0) *valid = 0;
      __syncthreads();
      const SchedEntry* sched = a.sched + (size_t)t * (n - 1);
      for (int i = lane; i < n - 1; i += kTile) {
        const SchedEntry e = sched[i];
        if ((unsigned)e.child0 >= (unsigned)V || (unsigned)e.child1 >= (unsigned)V) continue;
        if (e.node == 2 * n - 2) {
          // the set-up root (first child, R) is no node of the caller's tree
          const int first = e.child1 == R ? e.child0 : e.child0 == R ? e.child1 : R;
          if (first != R) par[first] = R, par[R] = first, *valid = 1;
        } else if (e.node >= n && e.node <= R) {
          kid0[e.node] = e.child0, kid1[e.node] = e.child1;
          par[e.child0] = e.node, par[e.child1] = e.node;
        }
      }
      __syncthreads();
      have_tree = tl;
    }
    if (!uniform(*valid)) continue;  // (a tree the set-up refused: reported through the status word)

    c.tl = tl, c.t = t, c.tile = tile;
    c.p = tile * kTile + lane;
    c.pc = c.p < a.P ? c.p : a.P - 1;
    c.w = c.p < a.P ? a.weights[c.pc] : 0.0;
    c.model = a.models + t;
    c.mats_t = as_const(a.mats + (size_t)t * (2 * n - 2) * K * 16);
    c.half_t = as_const(a.half + (size_t)t * (2 * n - 2) * K * 16);
    c.down_l = a.down + (size_t)tl * (n - 1) * K * ppad * 4 + (size_t)c.p * 4;
    c.up_l = a.up + (size_t)tl * V * K * ppad * 4 + (size_t)c.p * 4;
    c.ed_l = a.exp_down + (size_t)tl * (n - 1) * ppad + c.p;
    c.eu_l = a.exp_up + (size_t)tl * V * ppad + c.p;
    const double site = a.site[(size_t)tl * ppad + c.p];
    const int site_exp = RESCALE ? a.site_exp[(size_t)tl * ppad + c.p] : 0;

    for (int dir = 0; dir < 2; dir++) {
      if (dir == 1 && s < n) continue;
      const int above_s = uniform(par[s]);
      const int h = dir == 0 ? above_s : s, mv = dir == 0 ? s : above_s;
      if (h < n || mv < 0) continue;
      const int n0 = uniform(par[h]), n1 = uniform(kid0[h]), n2 = uniform(kid1[h]);
      const int z1 = mv == n0 ? n1 : n0, z2 = mv == n2 ? n1 : n2;
      if (z1 < 0 || z2 < 0 || z1 == z2) continue;
      const size_t out_index = ((size_t)tl * a.tiles + tile) * W + (size_t)(2 * s + dir) * E;
      // the moving part on its own branch
      for (int k = 0; k < K; k++) store4(c.slot(slots, k), c.into(h, mv, k));
      const int moving_exp = c.into_exp(h, mv);

      for (int side = 0; side < 2; side++) {
        const int start = side ? z2 : z1, other = side ? z1 : z2;
        if (start < n) continue;  // a leaf: nothing beyond it
        const int em = c.below(start, h) ? start : h;
        double mx = 0.0;
        for (int k = 0; k < K; k++) {
          const D4 m = matvec(c.mat(em, k), c.into(h, other, k));
          store4(c.slot(0, k), m);
          if (RESCALE) mx = fmax(mx, max4(m));
        }
        if (RESCALE) c.path_exp_l[0] = c.into_exp(h, other) + c.settle(0, mx);

        int depth = 0;
        fr_node[0] = start, fr_from[0] = h, fr_next[0] = 0;  // (every lane the same words)
        __syncthreads();
        while (depth >= 0) {
          const int x = uniform(fr_node[depth]), from = uniform(fr_from[depth]), next = uniform(fr_next[depth]);
          __syncthreads();
          if (next >= 2) {
            depth--;
            continue;
          }
          fr_next[depth] = next + 1;
          const int x0 = uniform(par[x]), x1 = uniform(kid0[x]), x2 = uniform(kid1[x]);
          const int o1 = from == x0 ? x1 : x0, o2 = from == x2 ? x1 : x2;
          const int zt = next ? o2 : o1, zs = next ? o1 : o2;
          const bool go_on = zt >= n && (a.radius == 0 || depth + 2 <= a.radius) && depth + 1 < slots;
          spr_target(c, x, zt, zs, depth, go_on, moving_exp, site, site_exp, out_index);
          if (go_on) {
            depth++;
            fr_node[depth] = zt, fr_from[depth] = x, fr_next[depth] = 0;
          }
          __syncthreads();
        }
      }
    }
  }
}

// ------------------------------------------------------------------------
// A workgroup per tree of the launch.  Thread i takes the rows (s, dir) = i, i + 256, ...: per
// target the tiles' partials by the family's tile sums (an entry the regraft kernel did not
// write is no move: -inf), the table if wanted, the largest entry of the row (the lowest f among
// equals).  Then one thread picks the best move over the rows in ascending code (2 s + dir) E + f,
// and the log-likelihood comes from the family's partials: a gradient call's on the HBM path.
// ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void spr_finalize_kernel(SprArgs a) {
  __shared__ double llw[4];
  const int tl = blockIdx.x, t = a.tree0 + tl;
  const int E = 2 * a.n - 3, rows = 2 * E;
  const size_t W = (size_t)rows * E;
  ll_tile_shares(a.ll_part + (size_t)t * a.ll_tiles, a.ll_used, llw);
  const double* src = a.part + (size_t)tl * a.tiles * W;
  const double none = -__builtin_huge_val();
  for (int r = threadIdx.x; r < rows; r += 256) {
    double best = none;
    int best_f = -1;
    for (int f = 0; f < E; f++) {
      const size_t col = (size_t)r * E + f;
      // (a move whose first tile's partial is itself -inf -- L'_p of 0 -- is taken for no move:
      // both are reported as -inf, so the table is the same; only best_target would show -1
      // for a row whose every move is -inf)
      const double v = src[col] == none ? none : tile_column_sum(src, (int)W, a.tiles, (int)col);
      if (a.out_delta) a.out_delta[((size_t)t * rows + r) * E + f] = v;
      if (v > best) best = v, best_f = f;
    }
    a.out_best_target[(size_t)t * rows + r] = best_f;
    a.out_best_delta[(size_t)t * rows + r] = best;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (a.out_ll) a.out_ll[t] = ll_tile_total(llw);
    if (a.out_best_move) {
      double best = none;
      int best_r = -1;
      for (int r = 0; r < rows; r++) {
        const double v = a.out_best_delta[(size_t)t * rows + r];
        if (v > best) best = v, best_r = r;
      }
      int32_t* move = a.out_best_move + (size_t)t * 3;
      move[0] = best_r < 0 ? -1 : best_r >> 1;
      move[1] = best_r < 0 ? -1 : best_r & 1;
      move[2] = best_r < 0 ? -1 : a.out_best_target[(size_t)t * rows + best_r];
    }
  }
}

size_t regraft_lds_bytes(int n, int depth_slots) {
  return sizeof(int32_t) * (3 * (size_t)(2 * n - 2) + 3 * (size_t)depth_slots + 1);
}

}  // namespace

// ------------------------------------------------------------------------
// Launch wrappers
// ------------------------------------------------------------------------
void launch_spr_half_lengths(const double* bl_eff, size_t count, double* half_bl, hipStream_t s) {
  hipLaunchKernelGGL(spr_half_lengths_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, bl_eff, count,
                     half_bl);
}

void launch_spr_vectors_hbm(const LikArgs& a, const SprArgs& w, int count, bool rescale, hipStream_t s) {
  if (count <= 0) return;
  const bool tp = a.tip_partials != nullptr;
  auto kernel = rescale ? (tp ? spr_vectors_hbm_kernel<true, true> : spr_vectors_hbm_kernel<true, false>)
                        : (tp ? spr_vectors_hbm_kernel<false, true> : spr_vectors_hbm_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3(a.tiles, count), dim3(kTile), 0, s, a, w);
}
const char* spr_kernel_name() { return "spr_vectors_hbm_kernel"; }

bool spr_regraft_fits_lds(int n, int depth_slots) { return regraft_lds_bytes(n, depth_slots) <= 64 * 1024; }

void launch_spr_regraft(const SprArgs& a, bool rescale, hipStream_t s) {
  const size_t W = 2 * (size_t)(2 * a.n - 3) * (2 * a.n - 3);
  const size_t cells = (size_t)a.trees * W;
  if (cells == 0) return;
  hipLaunchKernelGGL(spr_blank_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, a);
  const size_t jobs = (size_t)a.trees * a.tiles * (2 * a.n - 3);
  const bool tp = a.tip_partials != nullptr;
  auto kernel = rescale ? (tp ? spr_regraft_kernel<true, true> : spr_regraft_kernel<true, false>)
                        : (tp ? spr_regraft_kernel<false, true> : spr_regraft_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3((unsigned)std::min<size_t>(jobs, a.waves)), dim3(kTile),
                     regraft_lds_bytes(a.n, a.depth_slots), s, a);
}

void launch_spr_finalize(const SprArgs& a, hipStream_t s) {
  if (a.trees <= 0) return;
  hipLaunchKernelGGL(spr_finalize_kernel, dim3(a.trees), dim3(256), 0, s, a);
}

}  // namespace miphylo
