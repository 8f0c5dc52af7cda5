// Split tables of a batch of unrooted trees and the Robinson-Foulds distances from their indices
// (gfx950 / CDNA4, wave64).  Integer work with exact answers; the only
// floating-point sums (the split statistics, the branch score) have ONE order each, stated in
// include/mi_phylo.h, and the file is compiled without contraction (FLAGS_kernels_splits), so a
// host loop in IEEE doubles gives the same bits.
//
// An occurrence is an edge of a tree, o = t (2n-3) + v.  Four steps, a launch each or more:
//   tree_splits_kernel   the leaf set below every edge (one ascending pass over the nodes: a
//                        parent's id is above its children's), minorised, hashed, written out
//   split_insert_kernel  an open-addressing table of occurrence NUMBERS: a prober that finds a
//                        slot taken compares its bitset with the owner's, which the previous
//                        launch wrote completely -- nothing spins, nothing is published
//   flag / scan / scatter  first occurrences flagged, an exclusive scan numbers them (rocPRIM),
//                        every occurrence takes the number at its split's first occurrence
//   sort / runs          (statistics only) a stable radix sort by split index keeps a split's
//                        occurrences in tree order; the head of a run adds it front to back
// Only integer vector atomics (atomicCAS, atomicMin, atomicAdd on int32), and every result is
// independent of the order in which the lanes arrive.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>  // before rocprim: its texture iterator calls memset from host code

#include <rocprim/rocprim.hpp>

#include "mi_phylo_device_utils.h"
#include "mi_phylo_kernels.h"

namespace miphylo {

namespace {
using namespace dev;

__device__ __forceinline__ uint64_t mix64(uint64_t x) {  // (the 64-bit finaliser of MurmurHash3)
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdULL;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ULL;
  x ^= x >> 33;
  return x;
}

// Lane map: a tree's lanes are Wp = split_lane_words(n) neighbours, lane w of them owns word
// wi = 64 pass + w of every node's bitset; a wave holds 64 / Wp trees.  A lane only ever touches
// its own word column (store[node * 64 + lane]), so the ascending pass needs no barrier; the
// barriers below order the validity counters, which share column 0 of a tree, and the passes.
__device__ __forceinline__ void tree_splits(const SplitArgs& a, uint32_t* store) {
  const int lane = threadIdx.x, n = a.n, W = a.W;
  const int E = 2 * n - 3, nodes = E + 1, root = E;
  const int Wp = split_lane_words(n), per = 64 / Wp;
  const int g = lane / Wp, w = lane - g * Wp;
  const int t = blockIdx.x * per + g;
  const bool live = t < a.T;
  const int32_t* par = a.parent_ids + (size_t)(live ? t : 0) * E;
  const unsigned long long group = (Wp == 64 ? ~0ull : ((1ull << Wp) - 1)) << (g * Wp);
  uint32_t* col = store + lane;
  uint32_t* cnt = store + g * Wp;  // child counts of the tree's nodes, in its column 0

  for (int v = w; v < nodes; v += Wp) cnt[(size_t)v * 64] = 0;
  __syncthreads();
  int bad = kOk;
  for (int v = w; v < E; v += Wp) {
    const int p = par[v];
    if (p <= v || p > root || p < n) bad = kBadParentIds;
    else atomicAdd(&cnt[(size_t)p * 64], 1u);
  }
  __syncthreads();
  for (int v = n + w; v < nodes; v += Wp)
    if (bad == kOk && cnt[(size_t)v * 64] != (v == root ? 3u : 2u)) bad = v == root ? kNotTrifurcatingRoot : kNotBifurcating;
  // the tree's verdict: a bad parent id before an arity, the lowest lane's among arities
  const unsigned long long bad_parent = __ballot(bad == kBadParentIds) & group;
  const unsigned long long bad_any = __ballot(bad != kOk) & group;
  const int first_bad = bad_any ? __ffsll((long long)bad_any) - 1 : lane;
  const int arity_code = __shfl(bad, first_bad, 64);
  const int verdict = bad_parent ? (int)kBadParentIds : (bad_any ? arity_code : (int)kOk);
  if (live && w == 0 && verdict != kOk) set_status(a.status, verdict, t);
  // (a refused tree keeps its leaves' singletons and empty internal nodes: in bounds, and the
  // call fails)
  const bool ok = live && verdict == kOk;
  __syncthreads();

  const int passes = (W + 63) / 64;  // (more than one only where Wp == 64)
  for (int pass = 0; pass < passes; pass++) {
    const int wi = pass * 64 + w;
    for (int v = 0; v < nodes; v++) col[(size_t)v * 64] = (v < n && (v >> 5) == wi) ? 1u << (v & 31) : 0u;
    if (ok) {
      // below[parent[v]] |= below[v], ascending; the parents of eight steps are read ahead
      for (int v0 = 0; v0 < E; v0 += 8) {
        int pv[8];
#pragma unroll
        for (int k = 0; k < 8; k++) pv[k] = v0 + k < E ? par[v0 + k] : root;
#pragma unroll
        for (int k = 0; k < 8; k++)
          if (v0 + k < E) col[(size_t)pv[k] * 64] |= col[(size_t)(v0 + k) * 64];
      }
    }
    const uint32_t mask = wi < W - 1 ? ~0u : (wi == W - 1 ? ((n & 31) ? (1u << (n & 31)) - 1u : ~0u) : 0u);
    for (int v = 0; v < E; v++) {
      const size_t o = (size_t)(live ? t : 0) * E + v;
      uint32_t x = col[(size_t)v * 64];
      int flip;
      if (pass == 0) {
        flip = __shfl((int)(x & 1u), g * Wp, 64);  // (the tree's lane of word 0: bit 0 is taxon 0)
        if (live && w == 0 && passes > 1) a.occ_slot[o] = flip;
      } else {
        flip = live ? a.occ_slot[o] : 0;
      }
      if (flip) x = ~x & mask;
      uint64_t h = wi < W ? mix64(((uint64_t)(wi + 1) << 32) ^ x) : 0;
      for (int off = Wp >> 1; off > 0; off >>= 1) h ^= __shfl_xor(h, off, 64);
      if (live && wi < W) a.occ_bits[o * W + wi] = x;
      if (live && w == 0) a.occ_hash[o] = mix64((pass ? a.occ_hash[o] : 0) ^ h);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(64) void tree_splits_kernel(SplitArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t split_lds[];
  if (a.n <= kSplitLdsTaxa) tree_splits(a, split_lds);
  else tree_splits(a, a.store + (size_t)blockIdx.x * (split_store_bytes_per_wave(a.n) / 4));
}

__global__ __launch_bounds__(256) void split_init_kernel(SplitArgs a) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < a.slots; i += stride) {
    a.slot_owner[i] = -1;
    a.slot_first[i] = 0x7fffffff;
    a.slot_trees[i] = 0;
  }
}

__global__ __launch_bounds__(256) void split_insert_kernel(SplitArgs a) {
  const size_t O = (size_t)a.T * (2 * a.n - 3);
  const size_t o = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= O) return;
  uint32_t h = (uint32_t)a.occ_hash[o];
  if (a.hash_bits < 32) h &= (1u << a.hash_bits) - 1u;
  const uint32_t* mine = a.occ_bits + o * a.W;
  uint32_t slot = h & (a.slots - 1);
  // (the table has at least twice as many slots as occurrences: a free slot is always reached)
  for (;; slot = (slot + 1) & (a.slots - 1)) {
    const int32_t owner = atomicCAS(&a.slot_owner[slot], -1, (int32_t)o);
    if (owner == -1) break;
    const uint32_t* theirs = a.occ_bits + (size_t)owner * a.W;
    bool same = true;
    for (int k = 0; k < a.W && same; k++) same = mine[k] == theirs[k];
    if (same) break;
  }
  atomicMin(&a.slot_first[slot], (int32_t)o);
  atomicAdd(&a.slot_trees[slot], 1);
  a.occ_slot[o] = (int32_t)slot;
}

// (the hashes are dead from here on: their words hold the flags [O] and the ranks [O])
__global__ __launch_bounds__(256) void split_flag_kernel(SplitArgs a) {
  const size_t O = (size_t)a.T * (2 * a.n - 3);
  const size_t o = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= O) return;
  reinterpret_cast<uint32_t*>(a.occ_hash)[o] = a.slot_first[a.occ_slot[o]] == (int32_t)o ? 1u : 0u;
}

__global__ __launch_bounds__(256) void split_scatter_kernel(SplitArgs a) {
  const int E = 2 * a.n - 3, N = E + 2;
  const size_t O = (size_t)a.T * E;
  const size_t o = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= O) return;
  const uint32_t* flags = reinterpret_cast<const uint32_t*>(a.occ_hash);
  const uint32_t* ranks = flags + O;
  const int t = (int)(o / E), v = (int)(o - (size_t)t * E);
  const int32_t slot = a.occ_slot[o];
  const int32_t first = a.slot_first[slot];
  const uint32_t index = ranks[first];
  int32_t* row = a.out_index + (size_t)t * N;
  row[v] = (int32_t)index;
  if (v == 0) row[E] = row[E + 1] = -1;
  if (a.keys) {
    a.keys[o] = index;
    a.vals[o] = (uint32_t)o;
  }
  if (first == (int32_t)o && index < (uint32_t)a.capacity) {
    for (int k = 0; k < a.W; k++) a.out_bits[(size_t)index * a.W + k] = a.occ_bits[o * a.W + k];
    a.out_first[index] = t * N + v;
    a.out_trees[index] = a.slot_trees[slot];
  }
  if (o == O - 1) {
    const uint32_t S = ranks[o] + flags[o];
    *a.out_count = (int32_t)S;
    if (S > (uint32_t)a.capacity && atomicCAS(a.status, 0, (int)kSplitCapacity) == 0) a.status[1] = (int32_t)S;
  }
}

// sorted position p: the head of a run (a split's first tree) adds the run in tree order, one
// accumulator per column (the sort is stable: a split's occurrences stay in ascending t)
__global__ __launch_bounds__(256) void split_runs_kernel(SplitArgs a) {
  const int E = 2 * a.n - 3;
  const size_t O = (size_t)a.T * E;
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= O) return;
  const uint32_t k = a.keys2[p];
  if (k >= (uint32_t)a.capacity || (p > 0 && a.keys2[p - 1] == k)) return;
  // the run's length is the split's tree count (written by the launch before): eight entries'
  // loads are in flight at once, the additions keep their order
  const size_t end = p + (size_t)a.out_trees[k];
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (size_t q0 = p; q0 < end; q0 += 8) {
    double w[8], l[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const uint32_t o = a.vals2[q0 + j < end ? q0 + j : p];
      const uint32_t t = o / (uint32_t)E, v = o - t * (uint32_t)E;
      w[j] = a.weights ? a.weights[t] : 1.0;
      l[j] = a.bl ? a.bl[(size_t)t * (E + 1) + v] : 0.0;
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
      if (q0 + j >= end) break;
      s0 = __dadd_rn(s0, w[j]);
      if (a.bl) {
        s1 = __dadd_rn(s1, __dmul_rn(w[j], l[j]));
        s2 = __dadd_rn(s2, __dmul_rn(w[j], __dmul_rn(l[j], l[j])));
      }
    }
  }
  a.out_stats[(size_t)k * 3] = s0;
  a.out_stats[(size_t)k * 3 + 1] = s1;
  a.out_stats[(size_t)k * 3 + 2] = s2;
}

int key_bits(size_t occurrences) {  // keys are 0 .. occurrences - 1
  int bits = 1;
  while (bits < 32 && ((size_t)1 << bits) < occurrences) bits++;
  return bits;
}

// ---- Robinson-Foulds distances ----
__host__ __device__ inline int rf_padded(int E) {
  int p = 1;
  while (p < E) p <<= 1;
  return p;
}

// a wave per tree: its (index, length) list sorted by index, bitonic in LDS; negative indices
// ("not a parameter") sort to the end and are dropped
__global__ __launch_bounds__(64) void rf_sort_kernel(RfArgs a) {
  extern __shared__ __attribute__((aligned(16))) char rf_lds[];
  const int lane = threadIdx.x, t = blockIdx.x;
  const int E = 2 * a.n - 3, Ep = rf_padded(E);
  double* len = reinterpret_cast<double*>(rf_lds);     // [Ep]
  uint32_t* key = reinterpret_cast<uint32_t*>(len + Ep);  // [Ep]
  for (int i = lane; i < Ep; i += 64) {
    const int32_t k = i < E ? a.split_index[(size_t)t * (E + 2) + i] : -1;
    key[i] = k < 0 ? ~0u : (uint32_t)k;
    len[i] = (i < E && a.bl) ? a.bl[(size_t)t * (E + 1) + i] : 0.0;
  }
  __syncthreads();
  for (int size = 2; size <= Ep; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = lane; i < Ep / 2; i += 64) {
        const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
        const bool up = (lo & size) == 0;
        const uint32_t kl = key[lo], kh = key[hi];
        if ((kl > kh) == up && kl != kh) {
          key[lo] = kh;
          key[hi] = kl;
          const double x = len[lo];
          len[lo] = len[hi];
          len[hi] = x;
        }
      }
      __syncthreads();
    }
  int count = 0;
  for (int i = lane; i < E; i += 64) {
    count += key[i] != ~0u;
    a.sorted_index[(size_t)t * E + i] = (int32_t)key[i];
    a.sorted_length[(size_t)t * E + i] = len[i];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) count += __shfl_xor(count, off, 64);
  if (lane == 0) a.sorted_count[t] = count;
}

// a workgroup per tree a, its sorted list in LDS; a lane per tree b >= a merges b's list from
// memory against it.  RF counts the indices >= n of one tree only; the branch score adds
// (l_a - l_b)^2 over the indices of either tree in ascending index order, one accumulator.
__global__ __launch_bounds__(256) void rf_pairs_kernel(RfArgs a) {
  extern __shared__ __attribute__((aligned(16))) char rf_lds[];
  const int ta = blockIdx.x, T = a.T, n = a.n;
  const int E = 2 * n - 3;
  const int na = a.sorted_count[ta];
  double* la = reinterpret_cast<double*>(rf_lds);       // [E]
  int32_t* ka = reinterpret_cast<int32_t*>(la + E);     // [E]
  for (int i = threadIdx.x; i < na; i += 256) {
    ka[i] = a.sorted_index[(size_t)ta * E + i];
    la[i] = a.sorted_length[(size_t)ta * E + i];
  }
  __syncthreads();
  for (int tb = ta + threadIdx.x; tb < T; tb += 256) {
    const int nb = a.sorted_count[tb];
    const int32_t* kb = a.sorted_index + (size_t)tb * E;
    const double* lb = a.sorted_length + (size_t)tb * E;
    int i = 0, j = 0, rf = 0;
    double bs = 0.0;
    while (i < na || j < nb) {
      const int32_t x = i < na ? ka[i] : 0x7fffffff, y = j < nb ? kb[j] : 0x7fffffff;
      const double d = __dsub_rn(x <= y ? la[i] : 0.0, y <= x ? lb[j] : 0.0);
      bs = __dadd_rn(bs, __dmul_rn(d, d));
      if (x != y && (x < y ? x : y) >= n) rf++;
      i += x <= y;
      j += y <= x;
    }
    a.out_rf[(size_t)ta * T + tb] = rf;
    a.out_rf[(size_t)tb * T + ta] = rf;
    if (a.out_bs) {
      a.out_bs[(size_t)ta * T + tb] = bs;
      a.out_bs[(size_t)tb * T + ta] = bs;
    }
  }
}

}  // namespace

size_t split_scan_tmp_bytes(size_t occurrences) {
  size_t need = 0;
  uint32_t* none = nullptr;
  (void)rocprim::exclusive_scan(nullptr, need, none, none, 0u, std::max<size_t>(occurrences, 1),
                                rocprim::plus<uint32_t>());
  return (need + 255) & ~(size_t)255;
}

size_t split_sort_tmp_bytes(size_t occurrences) {
  size_t need = 0;
  uint32_t* none = nullptr;
  (void)rocprim::radix_sort_pairs(nullptr, need, none, none, none, none, std::max<size_t>(occurrences, 1), 0,
                                  (unsigned)key_bits(occurrences));
  return (need + 255) & ~(size_t)255;
}

int launch_split_index(const SplitArgs& a, hipStream_t s) {
  const size_t O = (size_t)a.T * (2 * a.n - 3);
  const unsigned blocks = (unsigned)((O + 255) / 256);
  const size_t lds = a.n <= kSplitLdsTaxa ? split_store_bytes_per_wave(a.n) : 0;
  hipLaunchKernelGGL(split_init_kernel, dim3((unsigned)std::min<size_t>((a.slots + 255) / 256, 4096)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(tree_splits_kernel, dim3((unsigned)split_wave_count(a.T, a.n)), dim3(64), lds, s, a);
  hipLaunchKernelGGL(split_insert_kernel, dim3(blocks), dim3(256), 0, s, a);
  hipLaunchKernelGGL(split_flag_kernel, dim3(blocks), dim3(256), 0, s, a);
  uint32_t* flags = reinterpret_cast<uint32_t*>(a.occ_hash);
  size_t scan_bytes = a.scan_tmp_bytes;
  if (rocprim::exclusive_scan(a.scan_tmp, scan_bytes, flags, flags + O, 0u, O, rocprim::plus<uint32_t>(), s) !=
      hipSuccess)
    return 1;
  hipLaunchKernelGGL(split_scatter_kernel, dim3(blocks), dim3(256), 0, s, a);
  if (!a.out_stats) return 0;
  size_t sort_bytes = a.sort_tmp_bytes;
  if (rocprim::radix_sort_pairs(a.sort_tmp, sort_bytes, a.keys, a.keys2, a.vals, a.vals2, O, 0,
                                (unsigned)key_bits(O), s) != hipSuccess)
    return 1;
  hipLaunchKernelGGL(split_runs_kernel, dim3(blocks), dim3(256), 0, s, a);
  return 0;
}

void launch_rf(const RfArgs& a, hipStream_t s) {
  const int E = 2 * a.n - 3;
  hipLaunchKernelGGL(rf_sort_kernel, dim3(a.T), dim3(64), (size_t)rf_padded(E) * 12, s, a);
  hipLaunchKernelGGL(rf_pairs_kernel, dim3(a.T), dim3(256), (size_t)E * 12, s, a);
}

}  // namespace miphylo
