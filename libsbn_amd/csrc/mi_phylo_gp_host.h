// The generalized-pruning object on the host: the subsplit DAG, the hybrid
// request tables and struct mi_gp.  Shared by mi_phylo_gp.cpp (the DAG's builder, the sweeps, the
// hybrid marginals, the optimiser) and mi_phylo_gp_trees.cpp (the tree side).  Host code only.
#pragma once
#include <map>
#include <tuple>
#include <vector>

#include "mi_phylo_engine.h"
#include "mi_phylo_gp_trees.h"

namespace miphylo {

constexpr double kGpDefaultThreshold = 0x1p-256;

// The DAG on the host.  Node ids: leaves 0..n-1, then the subsplits by first occurrence.  Clade 0
// of a subsplit is the one that holds its lowest taxon (the reference's "sorted" side: the larger
// chunk of the bitset order), clade 1 the other ("rotated").
struct GpDag {
  int n = 0, W = 0, nodes = 0, R = 0, G = 0;
  std::vector<uint32_t> clades;      // [nodes][2][W]; a leaf: its own bit in clade 0
  std::vector<int32_t> level;        // [nodes] clade size
  std::vector<int32_t> edge;         // [G][3]
  std::vector<int32_t> block_range;  // [nodes][2][2]
  std::vector<int32_t> in_range;     // [nodes][2]
  std::vector<int32_t> in_edges;
  std::vector<int32_t> order;        // internal nodes by (level, id)
  std::vector<std::pair<int, int>> levels;  // (first, count) into order, ascending level
  std::vector<double> below;         // [nodes] topologies below
  double topology_count = 0.0;
  std::map<std::tuple<int, int, int>, int> index;  // (parent, clade, child) -> entry
  std::map<int, int> root_index;                   // root node -> entry
};

struct HybridTables {
  int F = 0, S = 0, Z = 1, widest = 0;  // formed entries, summands, gridDim.z, the largest summand count of an entry
  bool too_large = false;
  int64_t cap = 0;
  std::vector<int32_t> desc;       // [G][kGpHybridDesc]
  std::vector<int32_t> formed;     // [F]
  std::vector<int32_t> levels;     // [levels][2]
};

}  // namespace miphylo

struct mi_gp {
  mi_engine* e = nullptr;
  miphylo::GpDag d;
  bool dag_only = false;  // mi_engine_gp_create_dag: no model, no codes, no vectors
  bool several_shards = false;  // made on a handle of several shards (e is its first): a variational fit refuses it
  int P = 0, Pp = 0, tiles = 0, I = 0;
  double threshold = miphylo::kGpDefaultThreshold;
  bool stale = true;  // the vectors are not those of the current b and q
  Buffer pool, matrix;
  GpArgs a{};         // the device pointers (b, q: the object's)
  double *b = nullptr, *q = nullptr, *params = nullptr;
  DevModel* model = nullptr;
  uint8_t* codes = nullptr;
  int32_t *d_edge = nullptr, *d_block = nullptr, *d_in_range = nullptr, *d_in_edges = nullptr, *d_order = nullptr;
  // outputs of the host forms
  double *o_gpcsp = nullptr, *o_marg = nullptr, *o_deriv = nullptr, *o_g = nullptr, *o_h = nullptr, *o_s = nullptr;
  // the optimiser: trial point and its values, kept derivatives, counters (each G + 2 entries where the step kernel
  // takes a tree's row)
  double *start = nullptr, *trial = nullptr, *tr_ll = nullptr, *tr_g = nullptr, *tr_h = nullptr, *tr_s = nullptr,
         *k_g = nullptr, *k_h = nullptr, *k_s = nullptr, *alpha = nullptr, *ll = nullptr, *trace = nullptr;
  int32_t *evals = nullptr, *status = nullptr, *active = nullptr;
  // hybrid marginals: the request tables and their device copies (made at creation), the outputs
  // of the host form, and what mi_gp_reserve_hybrid allocates: the evolve arrays and the partial sums
  miphylo::HybridTables ht;
  int32_t *d_hdesc = nullptr, *d_hformed = nullptr, *d_hlevels = nullptr;
  double *o_hybrid = nullptr, *o_summands = nullptr;  // (o_summands [S]: part of the reservation)
  Buffer hybrid;
  bool hybrid_reserved = false;
  GpHybridArgs h{};
  // the tree side (mi_gp_reserve_trees): the tables the tree kernels read and the per-tree
  // workspace, for tree_capacity trees
  Buffer trees;
  int tree_capacity = 0;
  uint64_t topologies = 0;  // the DAG's topology count, saturated at 2^62 (once `counted`)
  bool counted = false;
  miphylo::GpTreesArgs t{};
  miphylo::GpTrainArgs train{};  // the rooted TrainSimpleAverage's workspace
  // the by-value pieces of a variational step (mi_gp_reserve_vi): their workspace, for
  // vi_capacity trees (the sort's arrays are `train`'s)
  Buffer vi_ws;
  int vi_capacity = 0;
  struct ViWork {
    double *log_q, *qn, *usage, *sums, *factors, *terms;  // [G] x 3, [2], [cap], [cap][2n-2][2]
  } vw{};
};
