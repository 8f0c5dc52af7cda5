// Sampling from a subsplit Bayesian network and the gradient of the variational objective
// (gfx950 / CDNA4, wave64): the descent table of a support
// (mi_engine_sbn_descent), the per-block CDF with the Philox-driven draws (mi_engine_sbn_sample)
// and the signed, linear-domain accumulation of the usages (mi_engine_sbn_topology_gradient).
// The definitions (entries, the order of the draws, de-rooting, every sum's order) are in
// include/mi_phylo.h.
//   sbn_descent_kernel   a lane per support tree: children, lowest taxon below and above every
//                        node (as sbn_keys_kernel), then every slot writes its parameter's pair
//   sbn_cdf_kernel       a lane per short block, the wave per long one: the same ascending sum
//   sbn_sample_kernel    a lane per sample: the draws build the rooted tree in draw order (a node's
//                        children, a stack of pending entries), one descending pass gives every
//                        node's largest leaf, one post-order walk from the trifurcation the ids
//   sbn_factor_sums_kernel, sbn_factors_kernel   log F and sum log_f once, by one wave; then a thread
//                        per tree: its factor a_t (VIMCO: a fresh logsumexp each, O(K^2))
//   sbn_gradient_keys_kernel / radix sort / sbn_gradient_runs_kernel / sbn_gradient_blocks_kernel
//                        the key, stable sort and run-head scheme of kernels_sbn.hip with a linear
//                        signed run sum, then G_j - exp(theta_j) sum of the block
// FP64 throughout, one integer atomic (the status word), and the file is compiled without
// contraction (FLAGS_kernels_sbn_vi): every sum has the one order the header states.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>  // before rocprim: its texture iterator calls memset from host code

#include <rocprim/rocprim.hpp>

#include "../../include/mi_phylo.h"
#include "mi_phylo_device_utils.h"
#include "mi_phylo_kernels.h"
#include "mi_phylo_philox_device.h"

namespace miphylo {

namespace {
using namespace dev;

// A lane's view of its tree's node arrays, the layout of kernels_sbn.hip: word w of node v is
// words[(w nodes + v) tpw].
struct NodeStore {
  int32_t* words;
  int nodes, tpw;
  __device__ __forceinline__ int32_t& I(int w, int v) const { return words[((size_t)w * nodes + v) * tpw]; }
};
__device__ __forceinline__ NodeStore node_store(char* store, int n, int tpw, int lane) {
  NodeStore s;
  s.words = reinterpret_cast<int32_t*>(store) + lane;
  s.nodes = 2 * n - 2;
  s.tpw = tpw;
  return s;
}

// Children of every internal node in ascending id (words 0 and 1; the root's third in r2) and the
// tree's verdict, as kernels_sbn.hip forms them.  Every index stays in bounds whatever the ids are.
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

__device__ __forceinline__ void root_others(int r0, int r1, int r2, int v, int& a, int& b) {
  a = v == r0 ? r1 : r0;
  b = v == r2 ? r1 : r2;
}

// ---- the descent table ----
__device__ __forceinline__ void sbn_descent(const SbnDescentArgs& a, char* store) {
  const int lane = threadIdx.x, n = a.n, E = 2 * n - 3, root = E, S = a.S, P = a.S + a.C;
  const int t = blockIdx.x * a.tpw + lane;
  if (lane >= a.tpw || t >= a.T0) return;
  const NodeStore s = node_store(store, n, a.tpw, lane);
  const int32_t* par = a.parent_ids + (size_t)t * E;
  const int32_t* ri = a.root_index + (size_t)t * E;
  const int32_t* si = a.slot_index + (size_t)t * E * 6;
  int r2;
  const int verdict = build_children(s, par, n, r2);
  if (verdict != kOk) {
    set_status(a.status, verdict, t);
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
  bool sentinel = false;
  // the entry of slot (d, k): its PCSP's block, or the leaf below d's node
  auto entry = [&](int d, int k) -> int {
    if (!(d & 1) && (d >> 1) < n) return ~(d >> 1);
    const int j = si[d * 3 + k];
    if (j < S || j >= P) {
      sentinel = true;
      return 0;
    }
    return a.pcsp_parent[j - S];
  };
  auto put = [&](int j, int e0, int e1) {
    if (j < 0 || j >= P) {
      sentinel = true;
      return;
    }
    if (sentinel) return;
    a.out_descent[2 * (size_t)j] = e0;
    a.out_descent[2 * (size_t)j + 1] = e1;
  };
  for (int v = 0; v < E && !sentinel; v++) {
    const int p = par[v];
    // the rooting on edge v: the stored split is the side without taxon 0
    {
      const int below = entry(2 * v, 0), above = entry(2 * v + 1, 0);
      const bool zero_below = s.I(2, v) == 0;
      const int j = ri[v];
      if (j >= S) sentinel = true;
      else put(j, zero_below ? above : below, zero_below ? below : above);
    }
    // s = 0: the focal node is v; its child directed edges 2 c0 and 2 c1, each with its sibling
    // as the sister (slot 1)
    if (v >= n) {
      const int c0 = s.I(0, v), c1 = s.I(1, v);
      const int e0 = entry(2 * c0, 1), e1 = entry(2 * c1, 1);
      const bool child_is_c1 = s.I(2, c0) < s.I(2, c1);  // the child clade: the one without the lowest taxon
      for (int k = 0; k < 3; k++) {
        const int j = si[(2 * v) * 3 + k];
        if (j < 0) continue;
        put(j, child_is_c1 ? e1 : e0, child_is_c1 ? e0 : e1);
      }
    }
    // s = 1: the focal node is p; its child clades are p's other two neighbours
    {
      int ex, ey, mx, my;
      if (p == root) {
        int x, y;
        root_others(r0, r1, r2, v, x, y);
        ex = entry(2 * x, y < v ? 1 : 2);
        ey = entry(2 * y, x < v ? 1 : 2);
        mx = s.I(2, x), my = s.I(2, y);
      } else {
        const bool first = s.I(0, p) == v;
        const int sib = first ? s.I(1, p) : s.I(0, p);
        ex = entry(2 * sib, 2);
        ey = entry(2 * p + 1, first ? 2 : 1);
        mx = s.I(2, sib), my = s.I(3, p);
      }
      const bool child_is_y = mx < my;
      for (int k = 0; k < 3; k++) {
        const int j = si[(2 * v + 1) * 3 + k];
        if (j < 0) continue;
        put(j, child_is_y ? ey : ex, child_is_y ? ex : ey);
      }
    }
  }
  if (sentinel) set_status(a.status, kSbnSupportSentinel, t);
}

__global__ __launch_bounds__(64) void sbn_descent_kernel(SbnDescentArgs a, int in_lds) {
  extern __shared__ __attribute__((aligned(16))) char sbn_lds[];
  if (in_lds) sbn_descent(a, sbn_lds);
  else sbn_descent(a, a.store + (size_t)blockIdx.x * sbn_store_bytes_per_wave(a.n, a.tpw));
}

// sum + lane 0's value + lane 1's + ... + lane (count - 1)'s, in that order; `mine` is the running
// sum after the lane's own value
__device__ __forceinline__ double add_in_lane_order(double sum, double e, int count, int lane, double& mine) {
  if (count == 64) {
#pragma unroll 8
    for (int j = 0; j < 64; j++) {
      sum = sum + __shfl(e, j, 64);
      if (lane == j) mine = sum;
    }
  } else {
    for (int j = 0; j < count; j++) {
      sum = sum + __shfl(e, j, 64);
      if (lane == j) mine = sum;
    }
  }
  return sum;
}

// ---- the CDF ----
// cdf[j] = sum_{i <= j in block} exp(phi_i - m), ascending, one accumulator.  A block of up to 16
// entries is one lane's.  A longer one is the wave's: 64 exponentials side by side, added lane
// after lane -- the same additions in the same order.  A wave looks at 64 blocks at a time.
constexpr int kSbnShortBlock = 16;
__global__ __launch_bounds__(64) void sbn_cdf_kernel(SbnSampleArgs a) {
  const int lane = threadIdx.x, blocks = a.parents + 1, S = a.S, P = a.S + a.C;
  for (int base = blockIdx.x * 64; base < blocks; base += gridDim.x * 64) {
    const int b = base + lane;
    bool valid = b < blocks;
    int begin = !valid || b == 0 ? 0 : a.parent_range[2 * (b - 1)];
    int end = !valid ? 0 : (b == 0 ? S : a.parent_range[2 * (b - 1) + 1]);
    if (valid && b > 0 && !(begin >= S && begin < end && end <= P)) {  // (reported by the sample that visits it)
      valid = false;
      begin = end = 0;
    }
    const bool is_long = end - begin > kSbnShortBlock;
    if (valid && !is_long) {
      double m = -INFINITY;
      for (int j = begin; j < end; j++) m = fmax(m, a.phi[j]);
      double sum = 0.0;
      for (int j = begin; j < end; j++) {
        const double x = a.phi[j];
        sum = sum + (m == -INFINITY || x == -INFINITY ? 0.0 : exp(x - m));
        a.cdf[j] = sum;
      }
      a.block_max[b] = m;
    }
    unsigned long long todo = __ballot(is_long);
    while (todo) {
      const int src = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int lo = __shfl(begin, src, 64), hi = __shfl(end, src, 64);
      double m = -INFINITY;
      for (int j = lo + lane; j < hi; j += 64) m = fmax(m, a.phi[j]);
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
      double sum = 0.0;
      for (int q0 = lo; q0 < hi; q0 += 256) {  // (four loads in flight per lane; the additions keep their order)
        double e[4];
#pragma unroll
        for (int c = 0; c < 4; c++) {
          const int q = q0 + 64 * c + lane;
          const double x = q < hi ? a.phi[q] : -INFINITY;
          e[c] = m == -INFINITY || x == -INFINITY ? 0.0 : exp(x - m);
        }
#pragma unroll
        for (int c = 0; c < 4; c++) {
          const int first = q0 + 64 * c;
          if (first < hi) {
            double mine = 0.0;
            sum = add_in_lane_order(sum, e[c], min(hi - first, 64), lane, mine);
            if (first + lane < hi) a.cdf[first + lane] = mine;
          }
        }
      }
      if (lane == 0) a.block_max[base + src] = m;
    }
  }
}

// ---- the sampler ----
// u in [0, 1) of draw i of sample t (the rounds: mi_phylo_philox_device.h)
__device__ __forceinline__ double philox_uniform(uint64_t seed, uint64_t t, uint32_t i) {
  uint32_t c[4] = {i, 0u, (uint32_t)t, (uint32_t)(t >> 32)};
  philox4x32_10(c, seed);
  const uint64_t bits = ((uint64_t)c[0] << 32) | c[1];
  return (double)(bits >> 11) * 0x1.0p-53;
}

__device__ __forceinline__ void report(int32_t* status, int code, int sample, int block) {
  if (atomicCAS(status, 0, code) == 0) {
    status[1] = sample;
    status[3] = block;
  }
}

// Words of internal node i (0 .. n-2, in draw order: a parent before its children): 0, 1 its
// children (a leaf's id, n + i' for internal node i', or -1 - block while entry 1 is pending);
// 2 the largest leaf below; 3 its new id; word 4 is the stack.
__device__ __forceinline__ void sbn_sample(const SbnSampleArgs& a, char* store) {
  const int lane = threadIdx.x, n = a.n, E = 2 * n - 3, S = a.S, P = a.S + a.C;
  const int k = blockIdx.x * a.tpw + lane;
  if (lane >= a.tpw || k >= a.K) return;
  const NodeStore s = node_store(store, n, a.tpw, lane);
  int32_t* par = a.out_parent_ids + (size_t)k * E;
  int32_t* chosen = a.out_params + (size_t)k * (n - 1);
  const uint64_t t = (uint64_t)((a.vi ? vi_sample_base(*a.vi) : a.first_sample) + (int64_t)k);
  int code = kOk, where = 0;
  double lp = 0.0;
  int count = 0, sp = 0, block = -1, slot = -1;  // block -1: the rootsplits
  for (;;) {
    const int i = count;
    if (i >= n - 1) {
      code = kSbnBadDescent;
      break;
    }
    const int begin = block < 0 ? 0 : a.parent_range[2 * block], end = block < 0 ? S : a.parent_range[2 * block + 1];
    if (block >= 0 && !(begin >= S && begin < end && end <= P)) {
      code = kSbnBadDescent;
      break;
    }
    const double total = a.cdf[end - 1];
    if (!(total > 0.0)) {
      code = kSbnEmptyBlock, where = block;  // (-1: the rootsplits)
      break;
    }
    const double x = philox_uniform(a.seed, t, (uint32_t)i) * total;
    int lo = begin, hi = end;  // the smallest j with cdf[j] > x
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (a.cdf[mid] > x) hi = mid;
      else lo = mid + 1;
    }
    if (lo == end) {  // x rounded up to the total: the smallest j that reaches it
      lo = begin, hi = end - 1;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a.cdf[mid] >= total) hi = mid;
        else lo = mid + 1;
      }
    }
    const int j = lo;
    chosen[i] = j;
    lp = lp + ((a.phi[j] - a.block_max[block + 1]) - log(total));
    count++;
    if (slot >= 0) s.I(slot & 1, slot >> 1) = n + i;
    const int e0 = a.descent[2 * (size_t)j], e1 = a.descent[2 * (size_t)j + 1];
    if ((e0 >= 0 ? e0 >= a.parents : ~e0 >= n) || (e1 >= 0 ? e1 >= a.parents : ~e1 >= n)) {
      code = kSbnBadDescent;
      break;
    }
    if (e1 >= 0) s.I(1, i) = -1 - e1, s.I(4, sp++) = 2 * i + 1;
    else s.I(1, i) = ~e1;
    if (e0 >= 0) s.I(0, i) = -1 - e0, s.I(4, sp++) = 2 * i;
    else s.I(0, i) = ~e0;
    if (sp == 0) break;
    slot = s.I(4, --sp);
    block = -1 - s.I(slot & 1, slot >> 1);
  }
  if (code == kOk && count != n - 1) code = kSbnBadDescent;
  if (code != kOk) {
    report(a.status, code, k, where);
    for (int v = 0; v < E; v++) par[v] = -1;
    for (int i = 0; i < n - 1; i++) chosen[i] = -1;
    a.out_root_edge[k] = -1;
    a.out_log_prob[k] = NAN;
    return;
  }
  a.out_log_prob[k] = lp;
  // the largest leaf below every node: children come after their parent
  auto largest = [&](int c) { return c < n ? c : s.I(2, c - n); };
  for (int i = n - 2; i >= 0; i--) s.I(2, i) = max(largest(s.I(0, i)), largest(s.I(1, i)));
  // the trifurcation x and the root's other child y
  const int ra = s.I(0, 0), rb = s.I(1, 0);
  int x = largest(ra) == n - 1 ? ra : rb;
  if (x < n) x = x == ra ? rb : ra;
  const int y = x == ra ? rb : ra, xi = x - n;
  // child st of node i in the order of the largest leaves (the trifurcation has y as well)
  auto kid = [&](int i, int st) {
    int c0 = s.I(0, i), c1 = s.I(1, i);
    if (largest(c0) > largest(c1)) {
      const int tmp = c0;
      c0 = c1, c1 = tmp;
    }
    if (i != xi) return st == 0 ? c0 : c1;
    const int my = largest(y);
    if (my < largest(c0)) return st == 0 ? y : (st == 1 ? c0 : c1);
    if (my < largest(c1)) return st == 0 ? c0 : (st == 1 ? y : c1);
    return st == 0 ? c0 : (st == 1 ? c1 : y);
  };
  // post-order ids from n on: a stack entry is 4 i + the number of i's children already visited
  int next = n;
  sp = 0;
  s.I(4, sp++) = 4 * xi;
  while (sp > 0) {
    const int top = s.I(4, sp - 1), i = top >> 2, st = top & 3;
    if (st < (i == xi ? 3 : 2)) {
      s.I(4, sp - 1) = top + 1;
      const int c = kid(i, st);
      if (c >= n) s.I(4, sp++) = 4 * (c - n);
    } else {
      sp--;
      s.I(3, i) = next++;
    }
  }
  auto id = [&](int c) { return c < n ? c : s.I(3, c - n); };
  for (int v = 0; v < E; v++) par[v] = -1;
  for (int i = 1; i < n - 1; i++) {
    const int me = s.I(3, i);
    par[id(s.I(0, i))] = me;
    par[id(s.I(1, i))] = me;
    if (i == xi) par[id(y)] = me;
  }
  a.out_root_edge[k] = id(y);
}

__global__ __launch_bounds__(64) void sbn_sample_kernel(SbnSampleArgs a, int in_lds) {
  extern __shared__ __attribute__((aligned(16))) char sbn_lds[];
  if (in_lds) sbn_sample(a, sbn_lds);
  else sbn_sample(a, a.store + (size_t)blockIdx.x * sbn_store_bytes_per_wave(a.n, a.tpw));
}

// ---- the gradient ----
// log F = logsumexp(log_f) (the maximum, then ascending) and sum log_f (ascending), once per call:
// one wave, four loads per lane in flight, the additions lane after lane.  sums[0] = log F,
// sums[1] = sum log_f.
__global__ __launch_bounds__(64) void sbn_factor_sums_kernel(SbnGradientArgs a) {
  const int lane = threadIdx.x, K = a.T;
  const double* f = a.log_f;
  double m = -INFINITY;
  for (int i = lane; i < K; i += 64) m = fmax(m, f[i]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
  double sum = 0.0, total = 0.0;
  for (int q0 = 0; q0 < K; q0 += 256) {
    double x[4];
#pragma unroll
    for (int c = 0; c < 4; c++) x[c] = q0 + 64 * c + lane < K ? f[q0 + 64 * c + lane] : 0.0;
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const int first = q0 + 64 * c;
      if (first < K) {
        double mine;
        const int count = min(K - first, 64);
        sum = add_in_lane_order(sum, first + lane < K ? exp(x[c] - m) : 0.0, count, lane, mine);
        total = add_in_lane_order(total, x[c], count, lane, mine);
      }
    }
  }
  if (lane == 0) {
    a.sums[0] = m + log(sum);
    a.sums[1] = total;
  }
}

// a_t of one tree; VIMCO: a fresh logsumexp per tree, its sums in ascending order
__global__ __launch_bounds__(256) void sbn_factors_kernel(SbnGradientArgs a) {
  const int t = blockIdx.x * 256 + threadIdx.x, K = a.T;
  if (t >= K) return;
  const double* f = a.log_f;
  if (a.estimator == MI_SBN_FACTORS_GIVEN) {
    a.out_factors[t] = f[t];
    return;
  }
  const double log_F = a.sums[0], total = a.sums[1], log_K = log((double)K);
  double factor = (log_F - log_K) - exp(f[t] - log_F);
  if (a.estimator == MI_SBN_FACTORS_VIMCO) {
    const double mean = (total - f[t]) / (double)(K - 1);
    double m2 = -INFINITY;
    for (int i = 0; i < K; i++) m2 = fmax(m2, i == t ? mean : f[i]);
    double sum2 = 0.0;
    for (int i = 0; i < K; i++) sum2 = sum2 + exp((i == t ? mean : f[i]) - m2);
    factor = factor - ((m2 + log(sum2)) - log_K);
  }
  a.out_factors[t] = factor;
}

// entry q = t 7E + i: i < E the rootsplit of edge i, else slot i - E; entries without a parameter
// get the key P and sort behind the rest
__global__ __launch_bounds__(256) void sbn_gradient_keys_kernel(SbnGradientArgs a) {
  const int E = 2 * a.n - 3;
  const size_t Q = (size_t)a.T * E * 7;
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (q < (size_t)a.P) a.G[q] = 0.0;
  if (q >= Q) return;
  const size_t t = q / (7 * (size_t)E), i = q - t * 7 * E;
  const int32_t j = i < (size_t)E ? a.root_index[t * E + i] : a.slot_index[t * 6 * E + (i - E)];
  a.keys[q] = j >= 0 && j < a.P ? (uint32_t)j : (uint32_t)a.P;
  a.vals[q] = (uint32_t)q;
}

// the term of entry q: a_t times its usage in the linear domain; an unused entry adds nothing
__device__ __forceinline__ double gradient_term(const SbnGradientArgs& a, uint32_t q) {
  const double u = a.usage[q];
  if (u == -INFINITY) return 0.0;
  return a.out_factors[q / (7u * (uint32_t)(2 * a.n - 3))] * exp(u);
}

// sorted position p: the head of a run adds the run in ascending entry number (the sort is stable),
// one accumulator.  A run of up to 16 entries is added by its head's lane; a longer one by the
// whole wave, 64 terms side by side, added lane after lane: the same additions in the same order.
constexpr int kSbnShortRun = 16;
__global__ __launch_bounds__(256) void sbn_gradient_runs_kernel(SbnGradientArgs a) {
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
      double sum = 0.0;
      for (size_t q = p; q < end; q++) sum = sum + gradient_term(a, a.vals2[q]);
      a.G[k] = sum;
    }
  }
  unsigned long long todo = __ballot(is_long);
  while (todo) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const size_t begin = p - lane + src;  // (the head's position, the same in every lane)
    const uint32_t key = (uint32_t)__shfl((int)k, src, 64);
    double sum = 0.0;
    for (size_t q0 = begin;; q0 += 64) {
      const size_t q = q0 + lane;
      const bool in = q < Q && a.keys2[q] == key;
      const double term = in ? gradient_term(a, a.vals2[q]) : 0.0;
      const unsigned long long out = ~__ballot(in);
      const int count = out ? __ffsll((long long)out) - 1 : 64;
      for (int j = 0; j < count; j++) sum = sum + __shfl(term, j, 64);
      if (out) break;
    }
    if (lane == 0) a.G[key] = sum;
  }
}

// out[j] = G_j - exp(theta_j) sum of G over j's block, the sum ascending with one accumulator.  A
// block of up to 16 entries is one lane's; a longer one the wave's (loads side by side, additions
// lane after lane: the same order).  A wave looks at 64 blocks at a time.
__global__ __launch_bounds__(64) void sbn_gradient_blocks_kernel(SbnGradientArgs a) {
  const int lane = threadIdx.x, blocks = a.parents + 1;
  for (int base = blockIdx.x * 64; base < blocks; base += gridDim.x * 64) {
    const int b = base + lane;
    bool valid = b < blocks;
    int begin = !valid || b == 0 ? 0 : a.parent_range[2 * (b - 1)];
    int end = !valid ? 0 : (b == 0 ? a.S : a.parent_range[2 * (b - 1) + 1]);
    if (valid && b > 0 && !(begin >= a.S && begin < end && end <= a.P)) begin = end = 0;  // (as the CDF and the sampler)
    const bool is_long = end - begin > kSbnShortBlock;
    if (valid && !is_long) {
      double sum = 0.0;
      for (int j = begin; j < end; j++) sum = sum + a.G[j];
      for (int j = begin; j < end; j++) {
        const double th = a.theta[j];
        a.out_gradient[j] = th == -INFINITY ? a.G[j] : a.G[j] - exp(th) * sum;
      }
    }
    unsigned long long todo = __ballot(is_long);
    while (todo) {
      const int src = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int lo = __shfl(begin, src, 64), hi = __shfl(end, src, 64);
      double sum = 0.0;
      for (int q0 = lo; q0 < hi; q0 += 256) {
        double g[4];
#pragma unroll
        for (int c = 0; c < 4; c++) g[c] = q0 + 64 * c + lane < hi ? a.G[q0 + 64 * c + lane] : 0.0;
#pragma unroll
        for (int c = 0; c < 4; c++) {
          const int first = q0 + 64 * c;
          double mine;
          if (first < hi) sum = add_in_lane_order(sum, g[c], min(hi - first, 64), lane, mine);
        }
      }
      for (int j = lo + lane; j < hi; j += 64) {
        const double th = a.theta[j];
        a.out_gradient[j] = th == -INFINITY ? a.G[j] : a.G[j] - exp(th) * sum;
      }
    }
  }
}

unsigned bits_for(size_t values) {  // keys are 0 .. values - 1
  unsigned bits = 1;
  while (bits < 32 && ((size_t)1 << bits) < values) bits++;
  return bits;
}

}  // namespace

void sbn_vi_prepare(int n, int tpw) {
  if (n > sbn_lds_taxa(tpw)) return;
  const size_t lds = sbn_store_bytes_per_wave(n, tpw);
  allow_large_lds(reinterpret_cast<const void*>(sbn_descent_kernel), lds);
  allow_large_lds(reinterpret_cast<const void*>(sbn_sample_kernel), lds);
}

void launch_sbn_descent(const SbnDescentArgs& a, hipStream_t s) {
  const bool in_lds = a.n <= sbn_lds_taxa(a.tpw);
  const size_t lds = in_lds ? sbn_store_bytes_per_wave(a.n, a.tpw) : 0;
  sbn_vi_prepare(a.n, a.tpw);
  hipLaunchKernelGGL(sbn_descent_kernel, dim3((unsigned)sbn_wave_count(a.T0, a.tpw)), dim3(64), lds, s, a, in_lds ? 1 : 0);
}

void launch_sbn_sample(const SbnSampleArgs& a, hipStream_t s) {
  const bool in_lds = a.n <= sbn_lds_taxa(a.tpw);
  const size_t lds = in_lds ? sbn_store_bytes_per_wave(a.n, a.tpw) : 0;
  sbn_vi_prepare(a.n, a.tpw);
  hipLaunchKernelGGL(sbn_cdf_kernel, dim3((unsigned)std::min((a.parents + 1 + 63) / 64, 4096)), dim3(64), 0, s, a);
  hipLaunchKernelGGL(sbn_sample_kernel, dim3((unsigned)sbn_wave_count(a.K, a.tpw)), dim3(64), lds, s, a, in_lds ? 1 : 0);
}

// the factors a_t alone: reads T, estimator, log_f and sums; writes out_factors
void launch_sbn_factors(const SbnGradientArgs& a, hipStream_t s) {
  if (a.estimator != MI_SBN_FACTORS_GIVEN) hipLaunchKernelGGL(sbn_factor_sums_kernel, dim3(1), dim3(64), 0, s, a);
  hipLaunchKernelGGL(sbn_factors_kernel, dim3((unsigned)(a.T + 255) / 256), dim3(256), 0, s, a);
}

int launch_sbn_gradient(const SbnGradientArgs& a, hipStream_t s) {
  const size_t Q = (size_t)a.T * (2 * a.n - 3) * 7;
  const unsigned blocks = (unsigned)((std::max<size_t>(Q, a.P) + 255) / 256);
  launch_sbn_factors(a, s);
  hipLaunchKernelGGL(sbn_gradient_keys_kernel, dim3(blocks), dim3(256), 0, s, a);
  size_t sort_bytes = a.sort_tmp_bytes;
  if (rocprim::radix_sort_pairs(a.sort_tmp, sort_bytes, a.keys, a.keys2, a.vals, a.vals2, Q, 0,
                                bits_for((size_t)a.P + 1), s) != hipSuccess)
    return 1;
  hipLaunchKernelGGL(sbn_gradient_runs_kernel, dim3(blocks), dim3(256), 0, s, a);
  hipLaunchKernelGGL(sbn_gradient_blocks_kernel, dim3((unsigned)std::min((a.parents + 1 + 63) / 64, 4096)), dim3(64), 0, s, a);
  return 0;
}

}  // namespace miphylo
