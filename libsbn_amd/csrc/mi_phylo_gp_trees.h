// Trees of the subsplit DAG: what kernels_gp_trees.hip and mi_phylo_gp_trees.cpp
// share -- the arguments, the hash of a subsplit's clade words (the host builds the table the
// kernels probe), the per-tree store's size and the launchers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace miphylo {

// The topology counts saturate here: a DAG of 2^62 trees or more is not enumerated.
constexpr uint64_t kGpTreesCountCap = (uint64_t)1 << 62;

// FNV-1a over the 2 W clade words of a subsplit (clade 0's words, then clade 1's), word by word,
// with a final avalanche.  The table has a power-of-two number of slots, at least twice the
// subsplits, holds node ids (-1: empty) and is probed linearly; a hit is CONFIRMED by comparing
// the 2 W words with the node's clades, so identification is exact.
__host__ __device__ inline uint32_t gp_tree_hash_step(uint32_t h, uint32_t word) { return (h ^ word) * 16777619u; }
__host__ __device__ inline uint32_t gp_tree_hash_end(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  return h;
}
constexpr uint32_t kGpTreeHashSeed = 2166136261u;

// Words (int32) a lane keeps per tree.  The index kernel: per node its two children, its lowest
// taxon and its DAG node (4 words) and W clade words.  The build kernel: per internal node its DAG
// node, two children, two entries, largest leaf, new id, a stack slot and a 64-bit rank (10 words).
inline __host__ __device__ size_t gp_tree_index_words(int n) { return (size_t)(2 * n - 1) * (4 + (n + 31) / 32); }
inline __host__ __device__ size_t gp_tree_build_words(int n) { return (size_t)(n - 1) * 10; }
// De-rooting: per internal node two children, largest leaf, new id and a stack slot (device memory).
inline __host__ __device__ size_t gp_tree_deroot_words(int n) { return (size_t)(n - 1) * 5; }
// Trees per wave when the store is LDS (64 KiB of it): a lane per tree, the trees' words interleaved.
// Fewer than 8 lanes at work: the store is the workspace in device memory, 64 trees per wave.
constexpr size_t kGpTreesLds = 64 * 1024;
constexpr int kGpTreesMinLanes = 8;
// force_global (MI_PHYLO_GP_TREES_STORE=global): the workspace whatever the size (measurement, tests; same bits).
inline int gp_trees_per_wave(size_t words, bool force_global, bool& in_lds) {
  const size_t fit = kGpTreesLds / (4 * words);
  in_lds = !force_global && fit >= (size_t)kGpTreesMinLanes;
  return in_lds ? (int)(fit < 64 ? fit : 64) : 64;
}

struct GpTreesArgs {
  int n, W, nodes, R, G, slots;   // slots: of the hash table (a power of two)
  const int32_t* edge;            // [G][3]
  const int32_t* block_range;     // [nodes][2][2]
  const uint32_t* clades;         // [nodes][2][W]
  const int32_t* table;           // [slots] node or -1
  const int32_t* root_entry;      // [nodes] the rootsplit entry of a node, or -1
  const uint64_t* below;          // [nodes] topologies below, saturated at kGpTreesCountCap
  const uint64_t* options1;       // [nodes] the sum of `below` over the children of clade 1's block (the fast digit's base)
  const double* q;                // [G]
  const double* b;                // [G]
  double* cdf;                    // [G] workspace (the sampler's)
  int32_t* store;                 // per-tree workspace when the store is not LDS
  int32_t* status;
  int force_global;               // the per-tree store is the workspace whatever the size
};

// The rooted TrainSimpleAverage: keys (the entry of every (tree, node), G for a sentinel) and values (the
// position), a stable radix sort, a sum per run by the run's head, then the normalisation per block.
struct GpTrainArgs {
  int T, n, nodes, R, G;
  const int32_t* entries;      // [T][2n-1]
  const double* weights;       // [T] or null: all 1
  const int32_t* block_range;  // [nodes][2][2]
  uint32_t *keys, *keys2, *vals, *vals2;  // [T (2n-1)] each
  void* sort_tmp;
  size_t sort_tmp_bytes;
  double* counts;  // [G]
  double* out_q;   // [G]
  int32_t* status;
};
size_t gp_train_sort_tmp_bytes(size_t count);
int launch_gp_train(const GpTrainArgs& a, hipStream_t s);

// T trees [T][2n-2] -> out_entries [T][2n-1], out_nodes [T][2n-1] or null
void launch_gp_tree_index(const GpTreesArgs& a, int T, const int32_t* parent_ids, int32_t* out_entries, int32_t* out_nodes,
                          hipStream_t s);
void launch_gp_tree_log_prob(const GpTreesArgs& a, int T, const int32_t* entries, double* out_log_q, hipStream_t s);
void launch_gp_tree_lengths(const GpTreesArgs& a, int T, const int32_t* entries, double missing, double* out, hipStream_t s);
// out_cdf: a second copy, or null
void launch_gp_tree_cdf(const GpTreesArgs& a, double* out_cdf, hipStream_t s);
// sample != 0: draws (seed, first + k); else tree number first + k of the DAG.  out_lengths may be null.
// vi (or null): a fit's state in device memory, whose sample base replaces `first`.
struct ViState;
void launch_gp_tree_build(const GpTreesArgs& a, int K, int sample, uint64_t seed, int64_t first, const ViState* vi,
                          int32_t* out_parent_ids, int32_t* out_entries, double* out_log_q, double* out_lengths, hipStream_t s);
// rooted [T][2n-2] (+ lengths [T][2n-1] or null) -> unrooted [T][2n-3] (+ [T][2n-2] or null), root edge [T];
// store: gp_tree_deroot_words(n) words for every tree of ceil(T / 64) waves; out_new_id [T][2n-1] or null: the
// unrooted id under which every rooted node's edge lands (both root children: the root edge; the root: -1)
void launch_gp_tree_deroot(int T, int n, const int32_t* parent_ids, const double* lengths, int32_t* out_parent_ids,
                           double* out_lengths, int32_t* out_root_edge, int32_t* out_new_id, int32_t* store, int32_t* status,
                           hipStream_t s);

}  // namespace miphylo
