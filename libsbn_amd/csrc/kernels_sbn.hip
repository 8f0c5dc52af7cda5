// Subsplit Bayesian networks over batches of unrooted trees (gfx950 / CDNA4,
// wave64): the support with its parameter numbering and every tree's slots (mi_engine_sbn_index),
// the probabilities of all rootings with the expected usages (mi_engine_sbn_log_prob), the
// segmented log-normalisation and the small vector kernels of the training loop.  The definitions
// (directed edges, slots, numbering, the order of every sum) are in include/mi_phylo.h.
//
// A clade has the integer name 2 split + side from the split table (kernels_splits.hip), so a
// PCSP is a key of three int32.  The support's steps, a launch each or more:
//   sbn_support_count_kernel  S: the splits whose first occurrence lies in a support tree (the
//                             table numbers by first occurrence: they are indices 0 .. S-1)
//   sbn_keys_kernel      a lane per tree: children, lowest taxon below and above every node (one
//                        ascending and one descending pass), the key of every slot
//   sbn_insert_kernel    two open-addressing tables of occurrence NUMBERS (PCSPs, and their
//                        parents): a prober that finds a slot taken compares its key with the
//                        owner's, which the previous launch wrote -- nothing spins
//   flag / sort / scan / scatter  first occurrences in the support get the key (parent's first
//                        occurrence, own first occurrence); one radix sort forms the blocks; the
//                        heads of the blocks are scanned into parent numbers; every occurrence
//                        takes the sorted position of its PCSP's first occurrence
// The probabilities: sbn_walk_kernel, a lane per tree, one ascending and one descending pass for
// the rootings, one more pair for the usages (log domain); a stable radix sort by parameter index
// and the head of every run adds its run in ascending (tree, entry) order (run maximum, then
// sum exp(x - max)).  FP64 throughout, integer vector atomics only (atomicCAS, atomicMin), and
// the file is compiled without contraction (FLAGS_kernels_sbn): every sum has the one order the
// header states.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>  // before rocprim: its texture iterator calls memset from host code

#include <rocprim/rocprim.hpp>

#include "mi_phylo_device_utils.h"
#include "mi_phylo_kernels.h"

namespace miphylo {

namespace {
using namespace dev;

constexpr uint64_t kNotFirst = ~0ull;

__device__ __forceinline__ uint32_t mix32(uint32_t h, uint32_t x) {  // (MurmurHash3's block and final mix)
  x *= 0xcc9e2d51u;
  x = (x << 15) | (x >> 17);
  x *= 0x1b873593u;
  h ^= x;
  h = (h << 13) | (h >> 19);
  h = h * 5u + 0xe6546b64u;
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}

// A lane's view of its tree's node arrays: word w of node v is words[(w nodes + v) tpw].
struct NodeStore {
  int32_t* words;
  double* doubles;
  int nodes, tpw;
  __device__ __forceinline__ int32_t& I(int w, int v) const { return words[((size_t)w * nodes + v) * tpw]; }
  __device__ __forceinline__ double& D(int a, int v) const { return doubles[((size_t)(1 + a) * nodes + v) * tpw]; }
};
__device__ __forceinline__ NodeStore node_store(char* store, int n, int tpw, int lane) {
  NodeStore s;
  s.words = reinterpret_cast<int32_t*>(store) + lane;
  s.doubles = reinterpret_cast<double*>(store) + lane;
  s.nodes = 2 * n - 2;
  s.tpw = tpw;
  return s;
}

// Children of every internal node in ascending id (words 0 and 1; the root's third in r2) and the
// tree's verdict as kernels_splits.hip gives it: a bad parent id before an arity.  Every index
// stays in bounds whatever the ids are.
__device__ __forceinline__ int build_children(const NodeStore& s, const int32_t* par, int n, int& r2) {
  const int E = 2 * n - 3, root = E;
  for (int v = n; v <= root; v++) s.I(0, v) = s.I(1, v) = -1;
  r2 = -1;
  bool bad_parent = false;
  int arity = kOk;
  for (int v = 0; v < E; v++) {
    const int p = par[v];
    if (p <= v || p > root || p < n) bad_parent = true;
    else if (s.I(0, p) < 0) s.I(0, p) = v;
    else if (s.I(1, p) < 0) s.I(1, p) = v;
    else if (p == root && r2 < 0) r2 = v;
    else if (arity == kOk) arity = p == root ? kNotTrifurcatingRoot : kNotBifurcating;
  }
  for (int v = n; v <= root; v++)
    if (arity == kOk && (s.I(1, v) < 0 || (v == root && r2 < 0))) arity = v == root ? kNotTrifurcatingRoot : kNotBifurcating;
  return bad_parent ? (int)kBadParentIds : arity;
}

// the two other children of the root, ascending, beside its child v
__device__ __forceinline__ void root_others(int r0, int r1, int r2, int v, int& a, int& b) {
  a = v == r0 ? r1 : r0;
  b = v == r2 ? r1 : r2;
}

// ---- the support ----
__global__ __launch_bounds__(256) void sbn_support_count_kernel(SbnIndexArgs a) {
  const int N = 2 * a.n - 1;
  const int total = *a.split_count;
  const int limit = a.T0 * N;  // entry numbers t (2n-1) + v of the support trees are below it
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256)
    if (a.split_first[i] < limit && (i + 1 == total || a.split_first[i + 1] >= limit)) a.counts[0] = i + 1;
}

__device__ __forceinline__ void sbn_keys(const SbnIndexArgs& a, char* store) {
  const int lane = threadIdx.x, n = a.n, E = 2 * n - 3, root = E;
  const int t = blockIdx.x * a.tpw + lane;
  if (lane >= a.tpw || t >= a.T) return;
  const NodeStore s = node_store(store, n, a.tpw, lane);
  const int32_t* par = a.parent_ids + (size_t)t * E;
  const int32_t* sp = a.split_index + (size_t)t * (E + 2);
  int32_t* key = a.occ_key + (size_t)t * 2 * E * 9;  // [2E][3][3]
  int r2;
  if (build_children(s, par, n, r2) != kOk) {  // (the split table has named the tree: the call fails)
    for (int i = 0; i < 2 * E * 3; i++) key[(size_t)i * 3] = -1;
    return;
  }
  const int r0 = s.I(0, root), r1 = s.I(1, root);
  // lowest taxon below (word 2) and above (word 3) every edge
  for (int v = 0; v < E; v++) s.I(2, v) = v < n ? v : min(s.I(2, s.I(0, v)), s.I(2, s.I(1, v)));
  for (int v = E - 1; v >= 0; v--) {
    const int p = par[v];
    if (p == root) {
      int x, y;
      root_others(r0, r1, r2, v, x, y);
      s.I(3, v) = min(s.I(2, x), s.I(2, y));
    } else {
      const int sib = s.I(0, p) == v ? s.I(1, p) : s.I(0, p);
      s.I(3, v) = min(s.I(3, p), s.I(2, sib));
    }
  }
  // the clade of directed edge 2v + s: the split of v, and its side
  auto clade = [&](int v, int side) { return 2 * sp[v] + ((s.I(2, v) == 0 ? 1 : 0) ^ side); };
  for (int v = 0; v < E; v++) {
    const int p = par[v];
    int x, y;  // the two other neighbours of p
    if (p == root) root_others(r0, r1, r2, v, x, y);
    else x = s.I(0, p) == v ? s.I(1, p) : s.I(0, p), y = p;
    const int cx = clade(x, 0), cy = p == root ? clade(y, 0) : clade(p, 1);
    const int mx = s.I(2, x), my = p == root ? s.I(2, y) : s.I(3, p);
    int32_t* k0 = key + (size_t)(2 * v) * 9;
    int32_t* k1 = k0 + 9;
    // s = 0: the clade below v; sisters: the complement, then x and y
    if (v >= n) {
      const int c0 = s.I(0, v), c1 = s.I(1, v);
      const int focal = clade(v, 0), child = clade(s.I(2, c0) < s.I(2, c1) ? c1 : c0, 0);
      const int sister[3] = {clade(v, 1), cx, cy};
      for (int k = 0; k < 3; k++) k0[k * 3] = sister[k], k0[k * 3 + 1] = focal, k0[k * 3 + 2] = child;
    } else {
      k0[0] = k0[3] = k0[6] = -1;
    }
    // s = 1: everything else; its focal node is p, whose child clades are x and y
    {
      const int focal = clade(v, 1), child = mx < my ? cy : cx;
      k1[0] = clade(v, 0), k1[1] = focal, k1[2] = child;
      for (int k = 1; k < 3; k++) {
        k1[k * 3] = v >= n ? clade(s.I(k - 1, v), 0) : -1;
        k1[k * 3 + 1] = focal, k1[k * 3 + 2] = child;
      }
    }
  }
}

__global__ __launch_bounds__(64) void sbn_keys_kernel(SbnIndexArgs a, int in_lds) {
  extern __shared__ __attribute__((aligned(16))) char sbn_lds[];
  if (in_lds) sbn_keys(a, sbn_lds);
  else sbn_keys(a, a.store + (size_t)blockIdx.x * sbn_store_bytes_per_wave(a.n, a.tpw));
}

__global__ __launch_bounds__(256) void sbn_init_kernel(SbnIndexArgs a) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < a.slots; i += stride) {
    a.slot_owner[i] = a.pslot_owner[i] = -1;
    a.slot_first[i] = a.pslot_first[i] = 0x7fffffff;
  }
}

// (a table has at least twice as many slots as occurrences: a free slot is always reached)
__device__ __forceinline__ uint32_t sbn_probe(const int32_t* keys, int words, int32_t* owner, uint32_t slots,
                                              uint32_t h, size_t o) {
  const int32_t* mine = keys + o * 3;
  uint32_t slot = h & (slots - 1);
  for (;; slot = (slot + 1) & (slots - 1)) {
    const int32_t got = atomicCAS(&owner[slot], -1, (int32_t)o);
    if (got == -1) break;
    const int32_t* theirs = keys + (size_t)got * 3;
    bool same = true;
    for (int k = 0; k < words && same; k++) same = mine[k] == theirs[k];
    if (same) break;
  }
  return slot;
}

__global__ __launch_bounds__(256) void sbn_insert_kernel(SbnIndexArgs a) {
  const size_t O = (size_t)a.T * (2 * a.n - 3) * 6;
  const size_t o = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= O) return;
  const int32_t* k = a.occ_key + o * 3;
  if (k[0] < 0) {
    a.occ_slot[o] = a.occ_pslot[o] = -1;
    return;
  }
  uint32_t hp = mix32(mix32(0x9747b28cu, (uint32_t)k[0]), (uint32_t)k[1]);
  uint32_t h = mix32(hp, (uint32_t)k[2]);
  if (a.hash_bits < 32) {
    h &= (1u << a.hash_bits) - 1u;
    hp &= (1u << a.hash_bits) - 1u;
  }
  const uint32_t slot = sbn_probe(a.occ_key, 3, a.slot_owner, a.slots, h, o);
  const uint32_t pslot = sbn_probe(a.occ_key, 2, a.pslot_owner, a.slots, hp, o);
  atomicMin(&a.slot_first[slot], (int32_t)o);
  atomicMin(&a.pslot_first[pslot], (int32_t)o);
  a.occ_slot[o] = (int32_t)slot;
  a.occ_pslot[o] = (int32_t)pslot;
}

__global__ __launch_bounds__(256) void sbn_flag_kernel(SbnIndexArgs a) {
  const size_t per_tree = (size_t)(2 * a.n - 3) * 6;
  const size_t O = (size_t)a.T * per_tree, limit = (size_t)a.T0 * per_tree;
  const size_t o = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= O) return;
  const int32_t slot = a.occ_slot[o];
  const bool first = slot >= 0 && o < limit && a.slot_first[slot] == (int32_t)o;
  a.keys[o] = first ? ((uint64_t)(uint32_t)a.pslot_first[a.occ_pslot[o]] << 32) | (uint64_t)o : kNotFirst;
  a.vals[o] = (uint32_t)o;
}

// sorted position r: the PCSP's number within the support; block heads; C
__global__ __launch_bounds__(256) void sbn_heads_kernel(SbnIndexArgs a) {
  const size_t O = (size_t)a.T * (2 * a.n - 3) * 6;
  const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= O) return;
  const uint64_t key = a.keys2[r];
  if (key == kNotFirst) {
    a.heads[r] = 0;
    if (r == 0) a.counts[1] = 0;
    return;
  }
  a.rank_of[a.vals2[r]] = (int32_t)r;
  a.heads[r] = r == 0 || (a.keys2[r - 1] >> 32) != (key >> 32) ? 1u : 0u;
  if (r + 1 == O || a.keys2[r + 1] == kNotFirst) a.counts[1] = (int32_t)(r + 1);
}

__global__ __launch_bounds__(256) void sbn_scatter_kernel(SbnIndexArgs a) {
  const int E = 2 * a.n - 3;
  const size_t per_tree = (size_t)E * 6;
  const size_t O = (size_t)a.T * per_tree, limit = (size_t)a.T0 * per_tree;
  const size_t o = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= O) return;
  const int S = a.counts[0], C = a.counts[1];
  const int parents = C > 0 ? (int)a.head_scan[C - 1] : 0;
  // every occurrence: the number of its PCSP, the sentinel S + C outside the support
  const int32_t slot = a.occ_slot[o];
  int32_t index = -1;
  if (slot >= 0) {
    const int32_t first = a.slot_first[slot];
    index = (size_t)first < limit ? S + a.rank_of[first] : S + C;
  }
  a.out_slot_index[o] = index;
  // every edge: its rootsplit
  if (o < (size_t)a.T * E) {
    const size_t t = o / E, v = o - t * E;
    const int32_t split = a.split_index[t * (E + 2) + v];
    a.out_root_index[o] = split < S ? split : S + C;
  }
  // the tables
  if (o < (size_t)C && C <= a.pcsp_capacity) {
    const size_t src = a.vals2[o];
    for (int k = 0; k < 3; k++) a.out_pcsp_clades[o * 3 + k] = a.occ_key[src * 3 + k];
    const int parent = (int)a.head_scan[o] - 1;
    a.out_pcsp_parent[o] = parent;
    if (a.heads[o]) a.out_parent_range[(size_t)parent * 2] = S + (int)o;
    if (o + 1 == (size_t)C || a.heads[o + 1]) a.out_parent_range[(size_t)parent * 2 + 1] = S + (int)o + 1;
  }
  if (S <= a.root_capacity)
    for (size_t i = o; i < (size_t)S * a.W; i += O) a.out_split_bits[i] = a.split_bits[i];
  if (o == 0) {
    a.out_counts[0] = S;
    a.out_counts[1] = C;
    a.out_counts[2] = parents;
    if ((S > a.root_capacity || C > a.pcsp_capacity) && atomicCAS(a.status, 0, (int)kSbnCapacity) == 0) {
      a.status[1] = S;
      a.status[3] = C;
    }
  }
}

// ---- the probabilities ----
// log(exp(x) + exp(y) + exp(z)), the terms added in that order
__device__ __forceinline__ double lse3(double x, double y, double z) {
  const double m = fmax(x, fmax(y, z));
  if (m == -INFINITY) return m;
  return m + log(exp(x - m) + exp(y - m) + exp(z - m));
}

__device__ __forceinline__ void sbn_walk(const SbnProbArgs& a, char* store) {
  const int lane = threadIdx.x, n = a.n, E = 2 * n - 3, root = E, P = a.P;
  const int t = blockIdx.x * a.tpw + lane;
  if (lane >= a.tpw || t >= a.T) return;
  const NodeStore s = node_store(store, n, a.tpw, lane);
  const int32_t* par = a.parent_ids + (size_t)t * E;
  const int32_t* ri = a.root_index + (size_t)t * E;
  const int32_t* si = a.slot_index + (size_t)t * E * 6;
  double* lp = a.out_rooting + (size_t)t * E;
  double* use = a.usage ? a.usage + (size_t)t * E * 7 : nullptr;
  const double ninf = -INFINITY;
  int r2;
  const int verdict = build_children(s, par, n, r2);
  double w = a.weights ? a.weights[t] : 1.0;
  if (verdict == kOk && !(w >= 0.0 && w < INFINITY)) set_status(a.status, kSbnBadWeight, t);
  if (verdict != kOk) set_status(a.status, verdict, t);
  if (verdict != kOk || !(w >= 0.0 && w < INFINITY)) {
    for (int v = 0; v < E; v++) lp[v] = ninf;
    a.out_log_q[t] = ninf;
    if (use)
      for (int i = 0; i < 7 * E; i++) use[i] = ninf;
    return;
  }
  const int r0 = s.I(0, root), r1 = s.I(1, root);
  // the parameter of slot (d, k); the sentinel and "no such slot" count as -inf
  bool outside = false;
  auto theta = [&](int d, int k) {
    const int j = si[d * 3 + k];
    if (j >= P) outside = true;
    return j >= 0 && j < P ? a.theta[j] : ninf;
  };
  double lq = ninf;
  if (!a.uniform) {
    // B below (double 0) and above (double 1) every edge: the sum over the focal clade's inner
    // child clades c of theta[slot(c, sister = c's sibling)] + B(c), child x before child y
    for (int v = n; v < E; v++) {
      const int c0 = s.I(0, v), c1 = s.I(1, v);
      double b = 0.0;
      if (c0 >= n) b = b + (theta(2 * c0, 1) + s.D(0, c0));
      if (c1 >= n) b = b + (theta(2 * c1, 1) + s.D(0, c1));
      s.D(0, v) = b;
    }
    for (int v = E - 1; v >= 0; v--) {
      const int p = par[v];
      double b = 0.0;
      if (p == root) {
        int x, y;
        root_others(r0, r1, r2, v, x, y);
        // (under the root, slots 1 and 2 of x are its two siblings in ascending id)
        if (x >= n) b = b + (theta(2 * x, y < v ? 1 : 2) + s.D(0, x));
        if (y >= n) b = b + (theta(2 * y, x < v ? 1 : 2) + s.D(0, y));
      } else {
        const bool first = s.I(0, p) == v;
        const int sib = first ? s.I(1, p) : s.I(0, p);
        if (sib >= n) b = b + (theta(2 * sib, 2) + s.D(0, sib));
        b = b + (theta(2 * p + 1, first ? 2 : 1) + s.D(1, p));
      }
      s.D(1, v) = b;
    }
    // log p_v = theta[root] + A(2v, 0) + A(2v + 1, 0); log q: the maximum, then the terms in ascending v
    double m = ninf;
    for (int v = 0; v < E; v++) {
      const int j = ri[v];
      if (j >= P) outside = true;
      double x = j >= 0 && j < P ? a.theta[j] : ninf;
      if (v >= n) x = x + (theta(2 * v, 0) + s.D(0, v));
      x = x + (theta(2 * v + 1, 0) + s.D(1, v));
      lp[v] = x;
      m = fmax(m, x);
    }
    if (m != ninf) {
      double sum = 0.0;
      for (int v = 0; v < E; v++) sum = sum + exp(lp[v] - m);
      lq = m + log(sum);
    }
    a.out_log_q[t] = lq;
  } else {
    for (int v = 0; v < E; v++) {
      if (ri[v] >= P) outside = true;
      for (int k = 0; k < 6; k++)
        if (si[v * 6 + k] >= P) outside = true;
    }
  }
  if (a.require_support && outside) set_status(a.status, kSbnOutOfSupport, t);
  if (!use) return;
  // log usage: rho_v w_t of the rooting itself; a region's sum for the other slots.  R below
  // (double 0) and above (double 1): log sum of rho over the edges of that side, the edge's own
  // first, then child x, then child y.
  const double shift = a.uniform ? log(w) : (lq == ninf || w == 0.0 ? ninf : log(w) - lq);
  auto rho = [&](int v) { return a.uniform ? shift : (shift == ninf ? ninf : lp[v] + shift); };
  for (int v = 0; v < E; v++)
    s.D(0, v) = v < n ? rho(v) : lse3(rho(v), s.D(0, s.I(0, v)), s.D(0, s.I(1, v)));
  for (int v = E - 1; v >= 0; v--) {
    const int p = par[v];
    int x, y;
    if (p == root) {
      root_others(r0, r1, r2, v, x, y);
      s.D(1, v) = lse3(rho(v), s.D(0, x), s.D(0, y));
    } else {
      x = s.I(0, p) == v ? s.I(1, p) : s.I(0, p);
      s.D(1, v) = lse3(rho(v), s.D(0, x), s.D(1, p));
    }
  }
  for (int v = 0; v < E; v++) {
    const int p = par[v];
    const double rv = rho(v);
    use[v] = rv;
    double* u = use + E + (size_t)v * 6;
    if (v >= n) {
      // slot 1's sister is x: the slot is used by the rootings beyond y, and the other way round
      int x, y;
      double beyond_x, beyond_y;
      if (p == root) {
        root_others(r0, r1, r2, v, x, y);
        beyond_x = s.D(0, x), beyond_y = s.D(0, y);
      } else {
        x = s.I(0, p) == v ? s.I(1, p) : s.I(0, p);
        beyond_x = s.D(0, x), beyond_y = s.D(1, p);
      }
      u[0] = rv, u[1] = beyond_y, u[2] = beyond_x;
      u[3] = rv, u[4] = s.D(0, s.I(1, v)), u[5] = s.D(0, s.I(0, v));
    } else {
      u[0] = u[1] = u[2] = ninf;
      u[3] = rv, u[4] = u[5] = ninf;
    }
  }
}

__global__ __launch_bounds__(64) void sbn_walk_kernel(SbnProbArgs a, int in_lds) {
  extern __shared__ __attribute__((aligned(16))) char sbn_lds[];
  if (in_lds) sbn_walk(a, sbn_lds);
  else sbn_walk(a, a.store + (size_t)blockIdx.x * sbn_store_bytes_per_wave(a.n, a.tpw));
}

// entry q = t 7E + i: i < E the rootsplit of edge i, else slot i - E; entries without a parameter
// get the key P and sort behind the rest
__global__ __launch_bounds__(256) void sbn_usage_keys_kernel(SbnProbArgs a) {
  const int E = 2 * a.n - 3;
  const size_t Q = (size_t)a.T * E * 7;
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (q < (size_t)a.P) a.out_counts[q] = -INFINITY;
  if (q >= Q) return;
  const size_t t = q / (7 * (size_t)E), i = q - t * 7 * E;
  const int32_t j = i < (size_t)E ? a.root_index[t * E + i] : a.slot_index[t * 6 * E + (i - E)];
  a.keys[q] = j >= 0 && j < a.P ? (uint32_t)j : (uint32_t)a.P;
  a.vals[q] = (uint32_t)q;
}

// sorted position p: the head of a run adds the run in ascending entry number (the sort is stable),
// one accumulator: the run's maximum m, then sum exp(x - m), then m + log.  A run of up to 16
// entries is added by its head's lane; a longer one by the whole wave, which loads 64 entries at a
// time, takes their exponentials side by side and adds them lane after lane -- the same additions
// in the same order, so a run's bits do not depend on which of the two adds it.
constexpr int kSbnShortRun = 16;
__global__ __launch_bounds__(256) void sbn_usage_runs_kernel(SbnProbArgs a) {
  const size_t Q = (size_t)a.T * (2 * a.n - 3) * 7;
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const uint32_t k = p < Q ? a.keys2[p] : (uint32_t)a.P;
  const bool head = k < (uint32_t)a.P && (p == 0 || a.keys2[p - 1] != k);
  bool is_long = false;
  if (head) {
    size_t end = p + 1;
    while (end < Q && end - p <= kSbnShortRun && a.keys2[end] == k) end++;
    is_long = end - p > kSbnShortRun;
    if (!is_long) {
      double x[kSbnShortRun], m = -INFINITY;
#pragma unroll
      for (int j = 0; j < kSbnShortRun; j++) {
        x[j] = p + j < end ? a.usage[a.vals2[p + j]] : -INFINITY;
        m = fmax(m, x[j]);
      }
      if (m != -INFINITY) {
        double sum = 0.0;
#pragma unroll
        for (int j = 0; j < kSbnShortRun; j++)
          if (p + j < end) sum = sum + exp(x[j] - m);
        a.out_counts[k] = m + log(sum);
      }
    }
  }
  unsigned long long todo = __ballot(is_long);
  while (todo) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const size_t begin = p - lane + src;  // (the head's position, the same in every lane)
    const uint32_t key = (uint32_t)__shfl((int)k, src, 64);
    // the run's end and its maximum
    size_t end = begin;
    double m = -INFINITY;
    for (;;) {
      const size_t q = end + lane;
      const bool in = q < Q && a.keys2[q] == key;
      if (in) m = fmax(m, a.usage[a.vals2[q]]);
      const unsigned long long out = ~__ballot(in);
      if (out) {
        end += __ffsll((long long)out) - 1;
        break;
      }
      end += 64;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
    if (m == -INFINITY) continue;
    double sum = 0.0;
    for (size_t q0 = begin; q0 < end; q0 += 64) {
      const size_t q = q0 + lane;
      const double e = q < end ? exp(a.usage[a.vals2[q]] - m) : 0.0;
      const int count = end - q0 < 64 ? (int)(end - q0) : 64;
      for (int j = 0; j < count; j++) sum = sum + __shfl(e, j, 64);
    }
    if (lane == 0) a.out_counts[key] = m + log(sum);
  }
}

// ---- the vector kernels ----
// out = in - logsumexp per block.  A block of up to 16 entries is one lane's: the maximum m, then
// sum exp(x - m) in ascending order.  A longer block is the wave's: lane l takes the maximum and
// then the sum of entries l, l + 64, ..., and the lanes meet in a butterfly (offsets 32, 16, .., 1).
// Either way one order for a block of a given length.  A wave looks at 64 blocks at a time.
constexpr int kSbnShortBlock = 16;
__global__ __launch_bounds__(64) void sbn_normalize_kernel(int S, int blocks, const int32_t* range, const double* in,
                                                           double* out) {
  const int lane = threadIdx.x;
  for (int base = blockIdx.x * 64; base < blocks; base += gridDim.x * 64) {
    const int b = base + lane;
    const bool valid = b < blocks;
    const int begin = !valid || b == 0 ? 0 : range[2 * (b - 1)];
    const int end = !valid ? 0 : (b == 0 ? S : range[2 * (b - 1) + 1]);
    const bool is_long = end - begin > kSbnShortBlock;
    if (valid && !is_long) {
      double x[kSbnShortBlock], m = -INFINITY;
#pragma unroll
      for (int j = 0; j < kSbnShortBlock; j++) {
        x[j] = begin + j < end ? in[begin + j] : -INFINITY;
        m = fmax(m, x[j]);
      }
      double sum = 0.0;
      if (m != -INFINITY) {
#pragma unroll
        for (int j = 0; j < kSbnShortBlock; j++)
          if (begin + j < end) sum = sum + exp(x[j] - m);
      }
      const double z = m == -INFINITY ? 0.0 : m + log(sum);  // (a block that is all -inf stays -inf)
#pragma unroll
      for (int j = 0; j < kSbnShortBlock; j++)
        if (begin + j < end) out[begin + j] = x[j] - z;
    }
    unsigned long long todo = __ballot(is_long);
    while (todo) {
      const int src = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int lo = __shfl(begin, src, 64), hi = __shfl(end, src, 64);
      double m = -INFINITY;
      for (int j = lo + lane; j < hi; j += 64) m = fmax(m, in[j]);
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
      double sum = 0.0;
      if (m != -INFINITY)
        for (int j = lo + lane; j < hi; j += 64) sum = sum + exp(in[j] - m);
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) sum = sum + __shfl_xor(sum, off, 64);
      const double z = m == -INFINITY ? 0.0 : m + log(sum);
      for (int j = lo + lane; j < hi; j += 64) out[j] = in[j] - z;
    }
  }
}

__global__ __launch_bounds__(256) void sbn_check_params_kernel(int P, const double* theta, int32_t* status) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < P && !(theta[j] < INFINITY)) set_status(status, kSbnBadParam, j);
}

__global__ __launch_bounds__(256) void sbn_combine_kernel(int P, const double* x, const double* y, double shift, double* out) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= P) return;
  if (!y) {
    out[j] = x[j] + shift;
    return;
  }
  const double u = x[j], v = y[j] + shift, m = fmax(u, v);
  out[j] = m == -INFINITY ? m : m + log(exp(u - m) + exp(v - m));
}

// one wave: lane l adds terms l, l + 64, ... in ascending order, the lanes meet in a butterfly
__global__ __launch_bounds__(64) void sbn_score_kernel(int T, const double* w, const double* log_q, int P, const double* log_m,
                                                       const double* theta, double* out) {
  const int lane = threadIdx.x;
  double sum = 0.0;
  for (int t = lane; t < T; t += 64) {
    const double wt = w ? w[t] : 1.0;
    if (wt != 0.0) sum = sum + wt * log_q[t];
  }
  if (log_m)
    for (int j = lane; j < P; j += 64) {
      const double mj = exp(log_m[j]);
      if (mj != 0.0) sum = sum + mj * theta[j];
    }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sum = sum + __shfl_xor(sum, off, 64);
  if (lane == 0) *out = sum;
}

unsigned bits_for(size_t values) {  // keys are 0 .. values - 1
  unsigned bits = 1;
  while (bits < 32 && ((size_t)1 << bits) < values) bits++;
  return bits;
}

}  // namespace

size_t sbn_index_sort_tmp_bytes(size_t occurrences) {
  size_t need = 0;
  uint64_t* k = nullptr;
  uint32_t* v = nullptr;
  (void)rocprim::radix_sort_pairs(nullptr, need, k, k, v, v, std::max<size_t>(occurrences, 1), 0, 64);
  return (need + 255) & ~(size_t)255;
}

size_t sbn_index_scan_tmp_bytes(size_t occurrences) {
  size_t need = 0;
  uint32_t* none = nullptr;
  (void)rocprim::inclusive_scan(nullptr, need, none, none, std::max<size_t>(occurrences, 1), rocprim::plus<uint32_t>());
  return (need + 255) & ~(size_t)255;
}

size_t sbn_prob_sort_tmp_bytes(size_t entries, int P) {
  size_t need = 0;
  uint32_t* none = nullptr;
  (void)rocprim::radix_sort_pairs(nullptr, need, none, none, none, none, std::max<size_t>(entries, 1), 0,
                                  bits_for((size_t)P + 1));
  return (need + 255) & ~(size_t)255;
}

void sbn_prepare(int n, int tpw) {
  if (n > sbn_lds_taxa(tpw)) return;
  const size_t lds = sbn_store_bytes_per_wave(n, tpw);
  allow_large_lds(reinterpret_cast<const void*>(sbn_keys_kernel), lds);
  allow_large_lds(reinterpret_cast<const void*>(sbn_walk_kernel), lds);
}

int launch_sbn_index(const SbnIndexArgs& a, hipStream_t s) {
  const size_t O = (size_t)a.T * (2 * a.n - 3) * 6;
  const unsigned blocks = (unsigned)((O + 255) / 256);
  const bool in_lds = a.n <= sbn_lds_taxa(a.tpw);
  const size_t lds = in_lds ? sbn_store_bytes_per_wave(a.n, a.tpw) : 0;
  sbn_prepare(a.n, a.tpw);
  hipLaunchKernelGGL(sbn_support_count_kernel, dim3((unsigned)std::min<size_t>((O / 6 + 255) / 256, 1024)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(sbn_init_kernel, dim3((unsigned)std::min<size_t>((a.slots + 255) / 256, 4096)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(sbn_keys_kernel, dim3((unsigned)sbn_wave_count(a.T, a.tpw)), dim3(64), lds, s, a, in_lds ? 1 : 0);
  hipLaunchKernelGGL(sbn_insert_kernel, dim3(blocks), dim3(256), 0, s, a);
  hipLaunchKernelGGL(sbn_flag_kernel, dim3(blocks), dim3(256), 0, s, a);
  size_t sort_bytes = a.sort_tmp_bytes;
  if (rocprim::radix_sort_pairs(a.sort_tmp, sort_bytes, a.keys, a.keys2, a.vals, a.vals2, O, 0, 64, s) != hipSuccess)
    return 1;
  hipLaunchKernelGGL(sbn_heads_kernel, dim3(blocks), dim3(256), 0, s, a);
  size_t scan_bytes = a.scan_tmp_bytes;
  if (rocprim::inclusive_scan(a.scan_tmp, scan_bytes, a.heads, a.head_scan, O, rocprim::plus<uint32_t>(), s) != hipSuccess)
    return 1;
  hipLaunchKernelGGL(sbn_scatter_kernel, dim3(blocks), dim3(256), 0, s, a);
  return 0;
}

int launch_sbn_log_prob(const SbnProbArgs& a, hipStream_t s) {
  const bool in_lds = a.n <= sbn_lds_taxa(a.tpw);
  const size_t lds = in_lds ? sbn_store_bytes_per_wave(a.n, a.tpw) : 0;
  sbn_prepare(a.n, a.tpw);
  hipLaunchKernelGGL(sbn_walk_kernel, dim3((unsigned)sbn_wave_count(a.T, a.tpw)), dim3(64), lds, s, a, in_lds ? 1 : 0);
  if (!a.out_counts) return 0;
  const size_t Q = (size_t)a.T * (2 * a.n - 3) * 7;
  const unsigned blocks = (unsigned)((std::max<size_t>(Q, a.P) + 255) / 256);
  hipLaunchKernelGGL(sbn_usage_keys_kernel, dim3(blocks), dim3(256), 0, s, a);
  size_t sort_bytes = a.sort_tmp_bytes;
  if (rocprim::radix_sort_pairs(a.sort_tmp, sort_bytes, a.keys, a.keys2, a.vals, a.vals2, Q, 0,
                                bits_for((size_t)a.P + 1), s) != hipSuccess)
    return 1;
  hipLaunchKernelGGL(sbn_usage_runs_kernel, dim3(blocks), dim3(256), 0, s, a);
  return 0;
}

void launch_sbn_normalize(int S, int parents, const int32_t* parent_range, const double* in, double* out, hipStream_t s) {
  const int blocks = parents + 1;
  hipLaunchKernelGGL(sbn_normalize_kernel, dim3((unsigned)std::min((blocks + 63) / 64, 4096)), dim3(64), 0, s, S, blocks,
                     parent_range, in, out);
}

void launch_sbn_check_params(int P, const double* theta, int32_t* status, hipStream_t s) {
  hipLaunchKernelGGL(sbn_check_params_kernel, dim3((unsigned)(P + 255) / 256), dim3(256), 0, s, P, theta, status);
}

void launch_sbn_combine(int P, const double* a, const double* b, double shift, double* out, hipStream_t s) {
  hipLaunchKernelGGL(sbn_combine_kernel, dim3((unsigned)(P + 255) / 256), dim3(256), 0, s, P, a, b, shift, out);
}

void launch_sbn_score(int T, const double* weights, const double* log_q, int P, const double* log_m, const double* theta,
                      double* out, hipStream_t s) {
  hipLaunchKernelGGL(sbn_score_kernel, dim3(1), dim3(64), 0, s, T, weights, log_q, P, log_m, theta, out);
}

}  // namespace miphylo
