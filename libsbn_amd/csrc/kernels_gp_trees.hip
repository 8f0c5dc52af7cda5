// Trees of the subsplit DAG (gfx950 / CDNA4, wave64): which entries a rooted tree
// uses (mi_gp_tree_index), log q and the GP branch lengths of indexed trees (mi_gp_tree_log_prob,
// mi_gp_tree_branch_lengths), the per-block CDF with the Philox-driven draws (mi_gp_sample_trees),
// unranking (mi_gp_enumerate_trees) and de-rooting (mi_engine_deroot_trees).  The definitions are
// in include/mi_phylo.h.
//   gp_tree_index_kernel    a lane per tree: children, clade words and lowest taxon of every node
//                           (children before parents), the node of every subsplit by the hash
//                           table, CONFIRMED by comparing clade words; then every edge's entry by
//                           bisection of its block (sorted by child node)
//   gp_tree_log_prob_kernel a thread per tree: sum over v = 0 .. 2n-2 ascending, one accumulator
//   gp_tree_lengths_kernel  a thread per (tree, node)
//   gp_tree_cdf_kernel      a thread per block (and one for the rootsplits): cdf[j] = sum_{i <= j} q_i,
//                           ascending, one accumulator
//   gp_tree_build_kernel    a lane per tree, ONE body for the sampler and the enumerator: an entry is
//                           picked by a draw or by a rank; the tree grows in visit order (a parent
//                           before its children, a stack of pending clade-1 blocks), one descending
//                           pass gives every node's largest leaf, one post-order walk the ids; log q
//                           is then summed over the new ids ascending, as gp_tree_log_prob_kernel does
//   gp_tree_deroot_kernel   a lane per tree: the same largest-leaf pass and post-order walk, from the
//                           trifurcation
//   gp_train_keys_kernel / radix sort / gp_train_runs_kernel / gp_train_normalise_kernel
//                           the rooted TrainSimpleAverage by the key, stable sort and run-head scheme of
//                           kernels_sbn.hip: a run's head adds its trees' weights in ascending tree
//                           order; then a thread per block divides by the block's sum in entry order
// A lane's words are interleaved with its wave's (word j of lane l: store[j stride + l]), in LDS
// when at least 8 trees' words fit into 64 KiB, else in the object's workspace.
// FP64 and integers only; the one atomic is the integer compare-and-swap of the status word; nothing
// spins; every look-up table is read-only.  Compiled without contraction (FLAGS_kernels_gp_trees).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>  // before rocprim: its texture iterator calls memset from host code

#include <rocprim/rocprim.hpp>

#include "../../include/mi_phylo.h"
#include "mi_phylo_device.h"
#include "mi_phylo_device_utils.h"
#include "mi_phylo_gp_trees.h"
#include "mi_phylo_kernels.h"
#include "mi_phylo_philox_device.h"

namespace miphylo {

namespace {
using namespace dev;

struct Lane {
  int32_t* w;
  int stride;
  __device__ __forceinline__ int32_t& operator()(size_t j) const { return w[j * (size_t)stride]; }
};

// the lane's store: LDS (tpw lanes of a wave at work) or the workspace (all 64)
__device__ __forceinline__ Lane lane_store(int32_t* lds, int32_t* global, size_t words, int tpw, int in_lds) {
  Lane s;
  if (in_lds) {
    s.w = lds + threadIdx.x;
    s.stride = tpw;
  } else {
    s.w = global + (size_t)blockIdx.x * words * 64 + threadIdx.x;
    s.stride = 64;
  }
  return s;
}

// ---- the index ----
__device__ __forceinline__ void gp_tree_index(const GpTreesArgs& a, const int32_t* par, int32_t* ent, int32_t* nodes_out,
                                              const Lane& s, int t) {
  const int n = a.n, N = 2 * n - 1, W = a.W, G = a.G;
  const size_t K0 = 0, K1 = N, LOW = 2 * (size_t)N, NODE = 3 * (size_t)N, BITS = 4 * (size_t)N;
  for (int v = n; v < N; v++) s(K0 + v) = s(K1 + v) = -1;
  int code = kOk;
  for (int v = 0; v < N - 1; v++) {
    const int p = par[v];
    if (p < n || p >= N || p <= v) {
      if (code == kOk || code == kNotBifurcating) code = kBadParentIds;
    } else if (s(K0 + p) < 0) {
      s(K0 + p) = v;
    } else if (s(K1 + p) < 0) {
      s(K1 + p) = v;
    } else if (code == kOk) {
      code = kNotBifurcating;
    }
  }
  for (int v = n; v < N; v++)
    if (code == kOk && s(K1 + v) < 0) code = kNotBifurcating;
  if (code != kOk) {
    set_status(a.status, code, t);
    for (int v = 0; v < N; v++) {
      ent[v] = G;
      if (nodes_out) nodes_out[v] = -1;
    }
    return;
  }
  for (int v = 0; v < n; v++) {
    s(LOW + v) = v;
    s(NODE + v) = v;
    for (int w = 0; w < W; w++) s(BITS + (size_t)v * W + w) = w == v / 32 ? (int32_t)(1u << (v % 32)) : 0;
  }
  const uint32_t mask = (uint32_t)a.slots - 1;
  for (int v = n; v < N; v++) {
    int c0 = s(K0 + v), c1 = s(K1 + v);
    if (s(LOW + c1) < s(LOW + c0)) {  // clade 0 holds the lowest taxon
      const int tmp = c0;
      c0 = c1, c1 = tmp;
      s(K0 + v) = c0;
      s(K1 + v) = c1;
    }
    s(LOW + v) = s(LOW + c0);
    uint32_t h = kGpTreeHashSeed;
    for (int w = 0; w < W; w++) h = gp_tree_hash_step(h, (uint32_t)s(BITS + (size_t)c0 * W + w));
    for (int w = 0; w < W; w++) {
      const uint32_t x = (uint32_t)s(BITS + (size_t)c1 * W + w);
      h = gp_tree_hash_step(h, x);
      s(BITS + (size_t)v * W + w) = (int32_t)((uint32_t)s(BITS + (size_t)c0 * W + w) | x);
    }
    uint32_t slot = gp_tree_hash_end(h) & mask;
    int node = -1;
    for (int probe = 0; probe < a.slots; probe++) {
      const int cand = a.table[slot];
      if (cand < 0) break;
      const uint32_t* cl = a.clades + (size_t)cand * 2 * W;
      bool same = true;
      for (int w = 0; w < W && same; w++)
        same = cl[w] == (uint32_t)s(BITS + (size_t)c0 * W + w) && cl[W + w] == (uint32_t)s(BITS + (size_t)c1 * W + w);
      if (same) {
        node = cand;
        break;
      }
      slot = (slot + 1) & mask;
    }
    s(NODE + v) = node;
  }
  for (int v = 0; v < N - 1; v++) {
    const int p = par[v], pn = s(NODE + p), cn = s(NODE + v);
    int e = G;
    if (pn >= 0 && cn >= 0) {
      const int c = s(K0 + p) == v ? 0 : 1;
      int lo = a.block_range[((size_t)pn * 2 + c) * 2], hi = a.block_range[((size_t)pn * 2 + c) * 2 + 1];
      const int end = hi;
      while (lo < hi) {  // the first entry whose child is not below cn
        const int mid = (lo + hi) >> 1;
        if (a.edge[3 * (size_t)mid + 2] < cn) lo = mid + 1;
        else hi = mid;
      }
      if (lo < end && a.edge[3 * (size_t)lo + 2] == cn) e = lo;
    }
    ent[v] = e;
  }
  const int rn = s(NODE + N - 1);
  const int re = rn >= 0 ? a.root_entry[rn] : -1;
  ent[N - 1] = re >= 0 ? re : G;
  if (nodes_out)
    for (int v = 0; v < N; v++) nodes_out[v] = s(NODE + v);
}

__global__ __launch_bounds__(64) void gp_tree_index_kernel(GpTreesArgs a, int T, const int32_t* parent_ids, int32_t* out_entries,
                                                           int32_t* out_nodes, int tpw, int in_lds) {
  extern __shared__ __attribute__((aligned(16))) int32_t gp_trees_lds[];
  const int lane = threadIdx.x, t = blockIdx.x * tpw + lane, N = 2 * a.n - 1;
  if (lane >= tpw || t >= T) return;
  const Lane s = lane_store(gp_trees_lds, a.store, gp_tree_index_words(a.n), tpw, in_lds);
  gp_tree_index(a, parent_ids + (size_t)t * (N - 1), out_entries + (size_t)t * N, out_nodes ? out_nodes + (size_t)t * N : nullptr, s,
                t);
}

// ---- log q and the lengths ----
// sum over v = 0 .. 2n-2 ascending of log q[entries[v]], one accumulator; a sentinel (anything outside
// [0, G)) or a zero parameter gives -inf
__device__ __forceinline__ double gp_tree_log_q(const double* q, int G, const int32_t* ent, int N) {
  double lp = 0.0;
  for (int v = 0; v < N; v++) {
    const int e = ent[v];
    const double x = e >= 0 && e < G ? q[e] : 0.0;
    lp = lp + (x == 0.0 ? -INFINITY : log(x));
  }
  return lp;
}

__global__ __launch_bounds__(64) void gp_tree_log_prob_kernel(GpTreesArgs a, int T, const int32_t* entries, double* out) {
  const int t = blockIdx.x * 64 + threadIdx.x, N = 2 * a.n - 1;
  if (t < T) out[t] = gp_tree_log_q(a.q, a.G, entries + (size_t)t * N, N);
}

__device__ __forceinline__ double gp_tree_length(const double* b, int G, int e, int v, int N, double missing) {
  if (v == N - 1) return 0.0;
  return e >= 0 && e < G ? b[e] : missing;
}

__global__ __launch_bounds__(256) void gp_tree_lengths_kernel(GpTreesArgs a, int T, const int32_t* entries, double missing,
                                                              double* out) {
  const int N = 2 * a.n - 1;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)T * N) return;
  out[i] = gp_tree_length(a.b, a.G, entries[i], (int)(i % N), N, missing);
}

// ---- the CDF ----
// block 0: the rootsplits; block 1 + 2 (v - n) + c: (node v, clade c)
__global__ __launch_bounds__(64) void gp_tree_cdf_kernel(GpTreesArgs a, double* out_cdf) {
  const int blocks = 1 + 2 * (a.nodes - a.n);
  const int B = blockIdx.x * 64 + threadIdx.x;
  if (B >= blocks) return;
  int begin = 0, end = a.R;
  if (B > 0) {
    const size_t at = ((size_t)(a.n + (B - 1) / 2) * 2 + ((B - 1) & 1)) * 2;
    begin = a.block_range[at];
    end = a.block_range[at + 1];
  }
  double sum = 0.0;
  for (int j = begin; j < end; j++) {
    const double x = a.q[j];
    if (!(x >= 0.0) || x == INFINITY) set_status(a.status, kGpTreeBadParam, j);
    sum = sum + x;
    a.cdf[j] = sum;
    if (out_cdf) out_cdf[j] = sum;
  }
}

// ---- building a tree: the sampler and the enumerator ----
// u in [0, 1) of draw i of sample t (mi_engine_sbn_sample's rule)
__device__ __forceinline__ double philox_uniform(uint64_t seed, uint64_t t, uint32_t i) {
  uint32_t c[4] = {i, 0u, (uint32_t)t, (uint32_t)(t >> 32)};
  philox4x32_10(c, seed);
  const uint64_t bits = ((uint64_t)c[0] << 32) | c[1];
  return (double)(bits >> 11) * 0x1.0p-53;
}

// the entry of block [begin, end) that draw u picks: the smallest j with cdf[j] > u total, or, if the
// product rounded up to the total, the smallest j that reaches it; -1: the block's total is 0
__device__ __forceinline__ int pick_by_draw(const double* cdf, int begin, int end, double u) {
  const double total = cdf[end - 1];
  if (!(total > 0.0)) return -1;
  const double x = u * total;
  int lo = begin, hi = end;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cdf[mid] > x) hi = mid;
    else lo = mid + 1;
  }
  if (lo == end) {
    lo = begin, hi = end - 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (cdf[mid] >= total) hi = mid;
      else lo = mid + 1;
    }
  }
  return lo;
}

// the entry of block [begin, end) that holds rank r by the running sum of the counts below the
// entries' children; r becomes the remainder (the last entry takes whatever is left)
__device__ __forceinline__ int pick_by_rank(const GpTreesArgs& a, int begin, int end, uint64_t& r) {
  for (int j = begin; j < end - 1; j++) {
    const uint64_t c = a.below[a.edge[3 * (size_t)j + 2]];
    if (r < c) return j;
    r -= c;
  }
  return end - 1;
}

// Post-order ids n, n+1, ... of the internal nodes below `top` (internal node i is coded n + i as a
// child), children in the order of their largest leaves; `top` may have a third child `extra` (-1:
// none).  A stack entry is 4 i + the number of i's children already visited.
__device__ __forceinline__ void number_post_order(const Lane& s, int n, size_t K0, size_t K1, size_t L, size_t ID, size_t ST,
                                                  int top, int extra) {
  auto largest = [&](int c) { return c < n ? c : s(L + c - n); };
  auto kid = [&](int i, int st) {
    int c0 = s(K0 + i), c1 = s(K1 + i);
    if (largest(c0) > largest(c1)) {
      const int tmp = c0;
      c0 = c1, c1 = tmp;
    }
    if (i != top || extra < 0) return st == 0 ? c0 : c1;
    const int my = largest(extra);
    if (my < largest(c0)) return st == 0 ? extra : (st == 1 ? c0 : c1);
    if (my < largest(c1)) return st == 0 ? c0 : (st == 1 ? extra : c1);
    return st == 0 ? c0 : (st == 1 ? c1 : extra);
  };
  int next = n, sp = 0;
  s(ST + sp++) = 4 * top;
  while (sp > 0) {
    const int at = s(ST + sp - 1), i = at >> 2, st = at & 3;
    if (st < (i == top && extra >= 0 ? 3 : 2)) {
      s(ST + sp - 1) = at + 1;
      const int c = kid(i, st);
      if (c >= n) s(ST + sp++) = 4 * (c - n);
    } else {
      sp--;
      s(ID + i) = next++;
    }
  }
}

__device__ __forceinline__ void gp_tree_build(const GpTreesArgs& a, int sample, uint64_t seed, uint64_t number, int k, int32_t* par,
                                              int32_t* ent, double* out_log_q, double* lengths, const Lane& s) {
  const int n = a.n, N = 2 * n - 1, m = n - 1;
  const size_t DAG = 0, K0 = m, K1 = 2 * (size_t)m, E0 = 3 * (size_t)m, E1 = 4 * (size_t)m, L = 5 * (size_t)m, ID = 6 * (size_t)m,
               ST = 7 * (size_t)m, RLO = 8 * (size_t)m, RHI = 9 * (size_t)m;
  auto get_rank = [&](int i) { return (uint64_t)(uint32_t)s(RLO + i) | ((uint64_t)(uint32_t)s(RHI + i) << 32); };
  auto put_rank = [&](int i, uint64_t r) {
    s(RLO + i) = (int32_t)(uint32_t)r;
    s(RHI + i) = (int32_t)(uint32_t)(r >> 32);
  };
  int code = kOk, where = -1;
  uint32_t draw = 0;
  // the rootsplit
  uint64_t r = number;
  int e = sample ? pick_by_draw(a.cdf, 0, a.R, philox_uniform(seed, number, draw++)) : pick_by_rank(a, 0, a.R, r);
  int root_entry = e, count = 1, sp = 0, cur = 0, c = 0;
  if (e < 0) {
    code = kGpTreeEmptyBlock;
  } else {
    s(DAG + 0) = a.edge[3 * (size_t)e + 2];
    put_rank(0, r);
  }
  while (code == kOk) {
    const int v = s(DAG + cur);
    const int begin = a.block_range[((size_t)v * 2 + c) * 2], end = a.block_range[((size_t)v * 2 + c) * 2 + 1];
    if (sample) {
      e = pick_by_draw(a.cdf, begin, end, philox_uniform(seed, number, draw++));
      if (e < 0) {
        code = kGpTreeEmptyBlock, where = 2 * v + c;
        break;
      }
    } else {
      r = get_rank(cur);
      if (c == 0) {  // clade 0 is the slow digit
        const uint64_t base = a.options1[v];
        put_rank(cur, r % base);
        r = r / base;
      }
      e = pick_by_rank(a, begin, end, r);
    }
    const int child = a.edge[3 * (size_t)e + 2];
    s((c ? E1 : E0) + cur) = e;
    if (child < n) {
      s((c ? K1 : K0) + cur) = child;
      if (c == 0) {
        c = 1;
        continue;
      }
    } else {
      if (count >= m) {  // (cannot happen in a DAG the library built; keeps every index in bounds)
        code = kBadParentIds;
        break;
      }
      const int j = count++;
      s(DAG + j) = child;
      put_rank(j, r);
      s((c ? K1 : K0) + cur) = n + j;
      if (c == 0) s(ST + sp++) = cur;
      cur = j;
      c = 0;
      continue;
    }
    if (sp == 0) break;
    cur = s(ST + --sp);
    c = 1;
  }
  if (code == kOk && count != m) code = kBadParentIds;
  if (code != kOk) {
    if (atomicCAS(a.status, 0, code) == 0) {
      a.status[1] = k;
      a.status[3] = where;
    }
    for (int v = 0; v < N - 1; v++) par[v] = -1;
    for (int v = 0; v < N; v++) {
      ent[v] = -1;
      if (lengths) lengths[v] = NAN;
    }
    *out_log_q = NAN;
    return;
  }
  auto largest = [&](int x) { return x < n ? x : s(L + x - n); };
  for (int i = m - 1; i >= 0; i--) s(L + i) = max(largest(s(K0 + i)), largest(s(K1 + i)));
  number_post_order(s, n, K0, K1, L, ID, ST, 0, -1);
  auto id = [&](int x) { return x < n ? x : s(ID + x - n); };
  for (int i = 0; i < m; i++) {
    const int me = s(ID + i), x0 = id(s(K0 + i)), x1 = id(s(K1 + i));
    par[x0] = me;
    par[x1] = me;
    ent[x0] = s(E0 + i);
    ent[x1] = s(E1 + i);
  }
  ent[N - 1] = root_entry;
  *out_log_q = gp_tree_log_q(a.q, a.G, ent, N);
  if (lengths)
    for (int v = 0; v < N; v++) lengths[v] = gp_tree_length(a.b, a.G, ent[v], v, N, 0.0);
}

// vi: a fit's step: the first sample is the state's, `first` is not read
__global__ __launch_bounds__(64) void gp_tree_build_kernel(GpTreesArgs a, int K, int sample, uint64_t seed, int64_t first,
                                                           const ViState* vi, int32_t* out_parent_ids, int32_t* out_entries,
                                                           double* out_log_q, double* out_lengths, int tpw, int in_lds) {
  extern __shared__ __attribute__((aligned(16))) int32_t gp_trees_lds[];
  const int lane = threadIdx.x, k = blockIdx.x * tpw + lane, N = 2 * a.n - 1;
  if (lane >= tpw || k >= K) return;
  const Lane s = lane_store(gp_trees_lds, a.store, gp_tree_build_words(a.n), tpw, in_lds);
  if (vi) first = vi_sample_base(*vi);
  gp_tree_build(a, sample, seed, (uint64_t)(first + (int64_t)k), k, out_parent_ids + (size_t)k * (N - 1), out_entries + (size_t)k * N,
                out_log_q + k, out_lengths ? out_lengths + (size_t)k * N : nullptr, s);
}

// ---- de-rooting ----
// out_new_id [T][2n-1] or null: the unrooted id under which every rooted node's edge lands (both root
// children: the root edge; the root: -1)
__global__ __launch_bounds__(64) void gp_tree_deroot_kernel(int T, int n, const int32_t* parent_ids, const double* lengths,
                                                            int32_t* out_parent_ids, double* out_lengths, int32_t* out_root_edge,
                                                            int32_t* out_new_id, int32_t* store, int32_t* status) {
  const int t = blockIdx.x * 64 + threadIdx.x, N = 2 * n - 1, m = n - 1, E = 2 * n - 3;
  if (t >= T) return;
  Lane s;
  s.w = store + (size_t)blockIdx.x * gp_tree_deroot_words(n) * 64 + threadIdx.x;
  s.stride = 64;
  const size_t K0 = 0, K1 = m, L = 2 * (size_t)m, ID = 3 * (size_t)m, ST = 4 * (size_t)m;
  const int32_t* par = parent_ids + (size_t)t * (N - 1);
  int32_t* out = out_parent_ids + (size_t)t * E;
  double* bl = out_lengths ? out_lengths + (size_t)t * (E + 1) : nullptr;
  int32_t* nid = out_new_id ? out_new_id + (size_t)t * N : nullptr;
  for (int i = 0; i < m; i++) s(K0 + i) = s(K1 + i) = -1;
  int code = kOk;
  for (int v = 0; v < N - 1; v++) {
    const int p = par[v];
    if (p < n || p >= N || p <= v) {
      if (code == kOk || code == kNotBifurcating) code = kBadParentIds;
    } else if (s(K0 + p - n) < 0) {
      s(K0 + p - n) = v;
    } else if (s(K1 + p - n) < 0) {
      s(K1 + p - n) = v;
    } else if (code == kOk) {
      code = kNotBifurcating;
    }
  }
  for (int i = 0; i < m; i++)
    if (code == kOk && s(K1 + i) < 0) code = kNotBifurcating;
  if (code != kOk) {
    set_status(status, code, t);
    for (int v = 0; v < E; v++) out[v] = -1;
    if (bl)
      for (int v = 0; v <= E; v++) bl[v] = NAN;
    if (nid)
      for (int v = 0; v < N; v++) nid[v] = -1;
    out_root_edge[t] = -1;
    return;
  }
  auto largest = [&](int x) { return x < n ? x : s(L + x - n); };
  for (int i = 0; i < m; i++) s(L + i) = max(largest(s(K0 + i)), largest(s(K1 + i)));  // (a parent's id is above its children's)
  // the trifurcation x and the root's other child y
  const int ra = s(K0 + m - 1), rb = s(K1 + m - 1);
  int x = largest(ra) == n - 1 ? ra : rb;
  if (x < n) x = x == ra ? rb : ra;
  const int y = x == ra ? rb : ra, xi = x - n;
  number_post_order(s, n, K0, K1, L, ID, ST, xi, y);
  auto id = [&](int c) { return c < n ? c : s(ID + c - n); };
  const double* in = lengths ? lengths + (size_t)t * N : nullptr;
  for (int i = 0; i < m - 1; i++) {  // (every internal node but the root; y's parent is set below)
    const int me = s(ID + i);
    for (int c = 0; c < 2; c++) {
      const int kid = s((c ? K1 : K0) + i), ki = id(kid);
      out[ki] = me;
      if (bl) bl[ki] = in[kid];
      if (nid) nid[kid] = ki;
    }
  }
  const int yi = id(y);
  out[yi] = s(ID + xi);
  if (bl) {
    bl[yi] = in[y] + in[x];
    bl[E] = 0.0;
  }
  if (nid) {
    nid[y] = yi;
    nid[x] = yi;
    nid[N - 1] = -1;
  }
  out_root_edge[t] = yi;
}

// ---- the rooted TrainSimpleAverage ----
__global__ __launch_bounds__(256) void gp_train_keys_kernel(GpTrainArgs a) {
  const int N = 2 * a.n - 1;
  const size_t Q = (size_t)a.T * N, i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < (size_t)a.G) a.counts[i] = 0.0;
  if (i < (size_t)a.T && a.weights) {
    const double w = a.weights[i];
    if (!(w >= 0.0) || w == INFINITY) set_status(a.status, kSbnBadWeight, (int)i);
  }
  if (i >= Q) return;
  const int e = a.entries[i];
  const bool in = e >= 0 && e < a.G;
  if (!in) set_status(a.status, kGpTreeOutOfDag, (int)(i / N));
  a.keys[i] = in ? (uint32_t)e : (uint32_t)a.G;
  a.vals[i] = (uint32_t)i;
}

// the head of a run adds its run: the sort is stable, so the positions, and with them the trees, ascend
__global__ __launch_bounds__(256) void gp_train_runs_kernel(GpTrainArgs a) {
  const int N = 2 * a.n - 1;
  const size_t Q = (size_t)a.T * N, i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= Q) return;
  const uint32_t k = a.keys2[i];
  if (k >= (uint32_t)a.G || (i > 0 && a.keys2[i - 1] == k)) return;
  double sum = 0.0;
  for (size_t j = i; j < Q && a.keys2[j] == k; j++) sum = sum + (a.weights ? a.weights[a.vals2[j] / N] : 1.0);
  a.counts[k] = sum;
}

// per block and over the rootsplits, in entry order; a block whose total is 0 gets zeros
__global__ __launch_bounds__(64) void gp_train_normalise_kernel(GpTrainArgs a) {
  const int blocks = 1 + 2 * (a.nodes - a.n);
  const int B = blockIdx.x * 64 + threadIdx.x;
  if (B >= blocks) return;
  int begin = 0, end = a.R;
  if (B > 0) {
    const size_t at = ((size_t)(a.n + (B - 1) / 2) * 2 + ((B - 1) & 1)) * 2;
    begin = a.block_range[at];
    end = a.block_range[at + 1];
  }
  double total = 0.0;
  for (int j = begin; j < end; j++) total = total + a.counts[j];
  for (int j = begin; j < end; j++) a.out_q[j] = total == 0.0 ? 0.0 : a.counts[j] / total;
}

unsigned bits_for(size_t values) {  // keys are 0 .. values - 1
  unsigned bits = 1;
  while (bits < 32 && ((size_t)1 << bits) < values) bits++;
  return bits;
}

}  // namespace

// (room for keys of any width: a reservation does not depend on G)
size_t gp_train_sort_tmp_bytes(size_t count) {
  size_t bytes = 0;
  (void)rocprim::radix_sort_pairs(nullptr, bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                  count, 0, 32, (hipStream_t) nullptr);
  return bytes;
}

int launch_gp_train(const GpTrainArgs& a, hipStream_t s) {
  const size_t Q = (size_t)a.T * (2 * a.n - 1), most = std::max(Q, (size_t)a.G);
  hipLaunchKernelGGL(gp_train_keys_kernel, dim3((unsigned)((most + 255) / 256)), dim3(256), 0, s, a);
  size_t sort_bytes = a.sort_tmp_bytes;
  if (rocprim::radix_sort_pairs(a.sort_tmp, sort_bytes, a.keys, a.keys2, a.vals, a.vals2, Q, 0, bits_for((size_t)a.G + 1), s) !=
      hipSuccess)
    return 1;
  hipLaunchKernelGGL(gp_train_runs_kernel, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, s, a);
  const int blocks = 1 + 2 * (a.nodes - a.n);
  hipLaunchKernelGGL(gp_train_normalise_kernel, dim3((unsigned)((blocks + 63) / 64)), dim3(64), 0, s, a);
  return 0;
}

void launch_gp_tree_index(const GpTreesArgs& a, int T, const int32_t* parent_ids, int32_t* out_entries, int32_t* out_nodes,
                          hipStream_t s) {
  bool in_lds;
  const size_t words = gp_tree_index_words(a.n);
  const int tpw = gp_trees_per_wave(words, a.force_global != 0, in_lds);
  const size_t lds = in_lds ? words * 4 * tpw : 0;
  hipLaunchKernelGGL(gp_tree_index_kernel, dim3((unsigned)((T + tpw - 1) / tpw)), dim3(64), lds, s, a, T, parent_ids, out_entries,
                     out_nodes, tpw, in_lds ? 1 : 0);
}

void launch_gp_tree_log_prob(const GpTreesArgs& a, int T, const int32_t* entries, double* out_log_q, hipStream_t s) {
  hipLaunchKernelGGL(gp_tree_log_prob_kernel, dim3((unsigned)((T + 63) / 64)), dim3(64), 0, s, a, T, entries, out_log_q);
}

void launch_gp_tree_lengths(const GpTreesArgs& a, int T, const int32_t* entries, double missing, double* out, hipStream_t s) {
  const size_t count = (size_t)T * (2 * a.n - 1);
  hipLaunchKernelGGL(gp_tree_lengths_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, a, T, entries, missing, out);
}

void launch_gp_tree_cdf(const GpTreesArgs& a, double* out_cdf, hipStream_t s) {
  const int blocks = 1 + 2 * (a.nodes - a.n);
  hipLaunchKernelGGL(gp_tree_cdf_kernel, dim3((unsigned)((blocks + 63) / 64)), dim3(64), 0, s, a, out_cdf);
}

void launch_gp_tree_build(const GpTreesArgs& a, int K, int sample, uint64_t seed, int64_t first, const ViState* vi,
                          int32_t* out_parent_ids, int32_t* out_entries, double* out_log_q, double* out_lengths, hipStream_t s) {
  bool in_lds;
  const size_t words = gp_tree_build_words(a.n);
  const int tpw = gp_trees_per_wave(words, a.force_global != 0, in_lds);
  const size_t lds = in_lds ? words * 4 * tpw : 0;
  hipLaunchKernelGGL(gp_tree_build_kernel, dim3((unsigned)((K + tpw - 1) / tpw)), dim3(64), lds, s, a, K, sample, seed, first, vi,
                     out_parent_ids, out_entries, out_log_q, out_lengths, tpw, in_lds ? 1 : 0);
}

void launch_gp_tree_deroot(int T, int n, const int32_t* parent_ids, const double* lengths, int32_t* out_parent_ids,
                           double* out_lengths, int32_t* out_root_edge, int32_t* out_new_id, int32_t* store, int32_t* status,
                           hipStream_t s) {
  hipLaunchKernelGGL(gp_tree_deroot_kernel, dim3((unsigned)((T + 63) / 64)), dim3(64), 0, s, T, n, parent_ids, lengths,
                     out_parent_ids, out_lengths, out_root_edge, out_new_id, store, status);
}

}  // namespace miphylo
