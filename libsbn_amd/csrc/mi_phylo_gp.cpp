// Generalized pruning: the subsplit DAG of a batch of rooted topologies (host
// code), the object that keeps the DAG, its vectors, the branch lengths b[G] and the SBN parameters
// q[G] on the device (mi_engine_gp_create, mi_gp_destroy), the two sweeps (mi_gp_populate*), what
// is read from them (mi_gp_likelihoods*, mi_gp_branch_derivatives*), the SBN estimate and the
// branch-length optimisation of the marginal.  The kernels are kernels_gp.hip's; the optimiser's
// step is kernels_branch_opt.hip's, with the DAG in the part of one tree of G - R branches.
#include <cmath>
#include <map>
#include <set>
#include <tuple>
#include <vector>

#include "mi_phylo_engine.h"
#include "mi_phylo_gp_host.h"

namespace {

constexpr double kGpDefaultLength = 0.1;        // the reference's default_branch_length_
constexpr int kGpMaxIterations = 1000;          // (the step kernel's counter array)
// The summand kernel deals an entry's (rootward, sister) pairs over blockIdx.z: as many as the widest entry has,
// at most this (MI_PHYLO_GP_HYBRID_Z sets another number)
constexpr int kGpHybridMaxZ = 16;
// The summands of all requests of one DAG, at most (they are indexed by int32 together with the pattern tiles)
constexpr int64_t kGpHybridMaxSummands = (int64_t)1 << 28;

int popcount_words(const uint32_t* w, int W) {
  int c = 0;
  for (int i = 0; i < W; i++) c += __builtin_popcount(w[i]);
  return c;
}
int lowest_bit(const uint32_t* w, int W) {
  for (int i = 0; i < W; i++)
    if (w[i]) return 32 * i + __builtin_ctz(w[i]);
  return -1;
}

// one tree: each node's DAG node id (tree_node[v]) and its children by clade (kids[v][c]); new subsplits are numbered
int add_tree(GpDag& d, int tree, const int32_t* pid, std::map<std::vector<uint32_t>, int>& ids,
             std::vector<int32_t>& tree_node, std::vector<int32_t>& kids) {
  const int n = d.n, N = 2 * n - 1, W = d.W;
  std::vector<int32_t> child(2 * (size_t)N, -1);
  for (int v = 0; v < N - 1; v++) {
    const int p = pid[v];
    if (p < n || p >= N || p <= v)
      return fail("generalized pruning: tree " + std::to_string(tree) + " is not in the parent-id form of a rooted tree");
    if (child[2 * p] < 0) child[2 * p] = v;
    else if (child[2 * p + 1] < 0) child[2 * p + 1] = v;
    else return fail("generalized pruning: tree " + std::to_string(tree) + " is not bifurcating");
  }
  for (int v = n; v < N; v++)
    if (child[2 * v + 1] < 0) return fail("generalized pruning: tree " + std::to_string(tree) + " is not bifurcating");
  std::vector<uint32_t> bits((size_t)N * W, 0);
  tree_node.assign(N, -1);
  kids.assign(2 * (size_t)N, -1);
  for (int v = 0; v < n; v++) {
    bits[(size_t)v * W + v / 32] = 1u << (v % 32);
    tree_node[v] = v;
  }
  std::vector<uint32_t> key(2 * (size_t)W);
  for (int v = n; v < N; v++) {
    int a = child[2 * v], b = child[2 * v + 1];
    const uint32_t *ba = &bits[(size_t)a * W], *bb = &bits[(size_t)b * W];
    if (lowest_bit(bb, W) < lowest_bit(ba, W)) {
      std::swap(a, b);
      std::swap(ba, bb);
    }
    for (int w = 0; w < W; w++) {
      bits[(size_t)v * W + w] = ba[w] | bb[w];
      key[w] = ba[w];
      key[W + w] = bb[w];
    }
    auto it = ids.find(key);
    if (it == ids.end()) {
      it = ids.emplace(key, d.nodes++).first;
      d.clades.insert(d.clades.end(), key.begin(), key.end());
      d.level.push_back(popcount_words(&bits[(size_t)v * W], W));
    }
    tree_node[v] = it->second;
    kids[2 * v] = a;
    kids[2 * v + 1] = b;
  }
  return 0;
}

int build_dag(int n, int T, const int32_t* parent_ids, const double* bl, GpDag& d, std::vector<double>& b) {
  d.n = n;
  d.W = (n + 31) / 32;
  d.nodes = n;
  const int N = 2 * n - 1, W = d.W;
  d.clades.assign((size_t)n * 2 * W, 0);
  d.level.assign(n, 1);
  for (int v = 0; v < n; v++) d.clades[((size_t)v * 2) * W + v / 32] = 1u << (v % 32);
  std::map<std::vector<uint32_t>, int> ids;
  std::set<std::tuple<int, int, int>> edges;
  std::vector<int> roots;
  std::vector<int32_t> tree_node, kids;
  std::vector<std::vector<int32_t>> all_nodes(T), all_kids(T);
  for (int t = 0; t < T; t++) {
    if (add_tree(d, t, parent_ids + (size_t)t * (N - 1), ids, tree_node, kids)) return 1;
    for (int v = n; v < N; v++)
      for (int c = 0; c < 2; c++) edges.insert({tree_node[v], c, tree_node[kids[2 * v + c]]});
    const int root = tree_node[N - 1];
    if (!d.root_index.count(root)) {
      d.root_index[root] = (int)roots.size();
      roots.push_back(root);
    }
    if (bl) {  // (the hot start below reads every tree once more)
      all_nodes[t] = tree_node;
      all_kids[t] = kids;
    }
  }
  d.R = (int)roots.size();
  d.G = d.R + (int)edges.size();
  d.edge.resize(3 * (size_t)d.G);
  d.block_range.assign(4 * (size_t)d.nodes, 0);
  for (int i = 0; i < d.R; i++) {
    d.edge[3 * i] = d.edge[3 * i + 1] = -1;
    d.edge[3 * i + 2] = roots[i];
  }
  int e = d.R;
  for (const auto& t : edges) {  // (the set's order: node, clade, child)
    const int parent = std::get<0>(t), clade = std::get<1>(t), child = std::get<2>(t);
    d.edge[3 * e] = parent;
    d.edge[3 * e + 1] = clade;
    d.edge[3 * e + 2] = child;
    int32_t* range = &d.block_range[((size_t)parent * 2 + clade) * 2];
    if (range[1] == 0) range[0] = e;
    range[1] = e + 1;
    d.index[t] = e++;
  }
  // the entries into every node, ascending
  std::vector<int> count(d.nodes, 0);
  for (int i = 0; i < d.G; i++) count[d.edge[3 * i + 2]]++;
  d.in_range.resize(2 * (size_t)d.nodes);
  int at = 0;
  for (int v = 0; v < d.nodes; v++) {
    d.in_range[2 * v] = d.in_range[2 * v + 1] = at;
    at += count[v];
  }
  d.in_edges.resize(d.G);
  for (int i = 0; i < d.G; i++) d.in_edges[d.in_range[2 * d.edge[3 * i + 2] + 1]++] = i;
  // levels
  for (int v = n; v < d.nodes; v++) d.order.push_back(v);
  std::stable_sort(d.order.begin(), d.order.end(), [&](int x, int y) { return d.level[x] < d.level[y]; });
  for (size_t i = 0; i < d.order.size();) {
    size_t j = i;
    while (j < d.order.size() && d.level[d.order[j]] == d.level[d.order[i]]) j++;
    d.levels.push_back({(int)i, (int)(j - i)});
    i = j;
  }
  // SubsplitDAG::CountTopologies
  d.below.assign(d.nodes, 1.0);
  for (int v : d.order)
    for (int c = 0; c < 2; c++) {
      double options = 0.0;
      for (int i = d.block_range[(v * 2 + c) * 2]; i < d.block_range[(v * 2 + c) * 2 + 1]; i++) options += d.below[d.edge[3 * i + 2]];
      d.below[v] *= options;
    }
  d.topology_count = 0.0;
  for (int i = 0; i < d.R; i++) d.topology_count += d.below[roots[i]];
  // branch lengths: 0.1, or HotStartBranchLengths (the mean over the trees that hold the entry); rootsplits 0
  b.assign(d.G, kGpDefaultLength);
  for (int i = 0; i < d.R; i++) b[i] = 0.0;
  if (bl) {
    std::vector<double> sum(d.G, 0.0);
    std::vector<int> seen(d.G, 0);
    for (int t = 0; t < T; t++)
      for (int v = n; v < N; v++)
        for (int c = 0; c < 2; c++) {
          const int kid = all_kids[t][2 * v + c];
          const int i = d.index.at({all_nodes[t][v], c, all_nodes[t][kid]});
          sum[i] += bl[(size_t)t * N + kid];
          seen[i]++;
        }
    for (int i = d.R; i < d.G; i++)
      if (seen[i]) b[i] = sum[i] / seen[i];
  }
  return 0;
}

// The quartet hybrid requests (GPDAG::QuartetHybridRequestOf).  The central entry e = (t,c) -> s
// has four lists: rootward, the entries into t with the rootsplits skipped (a range of in_edges); sister,
// block(t,1-c); rotated, block(s,1); sorted, block(s,0).  It is fully formed iff none is empty.  Its summands are
// numbered from `first` with the rootward index outermost, then sister, rotated, and sorted innermost.
// A DAG whose requests have more than `cap` summands in all (kGpHybridMaxSummands unless a caller gives another)
// gets no request tables: too_large, nothing marked formed, F = S = 0, and every hybrid call refuses; whatever
// else the object does is untouched by it.  Nothing here grows with S.
// (struct HybridTables: mi_phylo_gp_host.h)
void build_hybrid_tables(const GpDag& d, int64_t cap, HybridTables& h) {
  h = HybridTables{};
  h.cap = cap;
  h.desc.assign((size_t)d.G * kGpHybridDesc, 0);
  for (const auto& l : d.levels) h.levels.insert(h.levels.end(), {l.first, l.second});
  // the lists and every request's summand count first: nothing is marked formed unless the total is under the cap
  std::vector<int64_t> counts(d.G, 0);
  int64_t total = 0;
  for (int e = d.R; e < d.G; e++) {
    const int t = d.edge[3 * e], c = d.edge[3 * e + 1], s = d.edge[3 * e + 2];
    int32_t* row = &h.desc[(size_t)e * kGpHybridDesc];
    int gb = d.in_range[2 * t];
    const int ge = d.in_range[2 * t + 1];
    while (gb < ge && d.in_edges[gb] < d.R) gb++;
    row[4] = gb;
    row[5] = ge;
    const int32_t* lists[3] = {&d.block_range[(t * 2 + (1 - c)) * 2], &d.block_range[(s * 2 + 1) * 2],
                               &d.block_range[(s * 2 + 0) * 2]};
    int64_t count = ge - gb;
    for (int k = 0; k < 3; k++) {
      row[6 + 2 * k] = lists[k][0];
      row[7 + 2 * k] = lists[k][1];
      count = std::min(count * (lists[k][1] - lists[k][0]), cap + 1);  // (saturated: four factors of up to G each)
    }
    counts[e] = count;
    total = std::min(total + count, cap + 1);
  }
  if (total > cap) {
    h.too_large = true;
    return;
  }
  int pairs = 1;
  total = 0;
  for (int e = d.R; e < d.G; e++) {
    if (counts[e] == 0) continue;
    int32_t* row = &h.desc[(size_t)e * kGpHybridDesc];
    row[0] = 1;
    row[1] = (int32_t)total;
    row[2] = (int32_t)counts[e];
    total += counts[e];
    pairs = std::max(pairs, (row[5] - row[4]) * (row[7] - row[6]));
    h.widest = std::max(h.widest, row[2]);
    h.formed.push_back(e);
  }
  h.F = (int)h.formed.size();
  h.S = (int)total;
  h.Z = std::min(pairs, kGpHybridMaxZ);
}

int refuse_too_large(const HybridTables& t) {
  return fail("generalized pruning: this DAG's hybrid requests have more than " + std::to_string(t.cap) +
              " summands in all; hybrid marginals are not served for it");
}

// SubsplitDAG::BuildUniformOnTopologicalSupportPrior
std::vector<double> uniform_prior(const GpDag& d) {
  std::vector<double> q(d.G, 1.0);
  for (int v = d.n; v < d.nodes; v++)
    for (int c = 0; c < 2; c++) {
      const int begin = d.block_range[(v * 2 + c) * 2], end = d.block_range[(v * 2 + c) * 2 + 1];
      double options = 0.0;
      for (int i = begin; i < end; i++) options += d.below[d.edge[3 * i + 2]];
      for (int i = begin; i < end; i++) q[i] = d.below[d.edge[3 * i + 2]] / options;
    }
  for (int i = 0; i < d.R; i++) q[i] = d.below[d.edge[3 * i + 2]] / d.topology_count;
  return q;
}

// SubsplitDAG::UnconditionalNodeProbabilities: parents before children (descending level)
void node_probabilities(const GpDag& d, const double* q, double* out) {
  std::fill(out, out + d.nodes, 0.0);
  for (int i = 0; i < d.R; i++) out[d.edge[3 * i + 2]] += q[i];
  for (size_t k = d.order.size(); k-- > 0;) {
    const int v = d.order[k];
    for (int c = 0; c < 2; c++)
      for (int i = d.block_range[(v * 2 + c) * 2]; i < d.block_range[(v * 2 + c) * 2 + 1]; i++)
        out[d.edge[3 * i + 2]] += out[v] * q[i];
  }
}

}  // namespace

// (struct mi_gp: mi_phylo_gp_host.h)

namespace {

size_t cut(mi_gp* g, char* base) {
  const size_t G = g->d.G, I = g->I, Pp = g->Pp, nodes = g->d.nodes, n = g->d.n;
  GpArgs& a = g->a;
  Cutter c{base};
  c.take(g->b, G + 2);
  c.take(g->q, G);
  c.take(g->d_edge, 3 * G);
  c.take(g->d_block, 4 * nodes);
  c.take(g->d_in_range, 2 * nodes);
  c.take(g->d_in_edges, G);
  c.take(g->d_order, I);
  if (g->dag_only) return c.at;  // (no model, no codes, no vectors, no outputs: DESIGN.md 4.27)
  c.take(g->model, 1);
  c.take(g->params, (size_t)g->e->param_count);
  c.take(g->codes, (size_t)distance_code_rows((int)n) * distance_code_stride(g->P));
  c.take(a.mats, 16 * G);
  c.take(a.expl, 8 * G);
  c.take(a.phat, I * 2 * 4 * Pp);
  c.take(a.p, I * 4 * Pp);
  c.take(a.r, I * 2 * 4 * Pp);
  c.take(a.ephat, I * 2 * Pp);
  c.take(a.ep, I * Pp);
  c.take(a.er, I * 2 * Pp);
  c.take(a.marg, Pp);
  c.take(a.emarg, Pp);
  c.take(a.log_marg, Pp);
  c.take(a.partial, (G + 1) * (size_t)g->tiles * kGpSums);
  c.take(a.sums, (G + 1) * kGpSums);
  c.take(g->o_gpcsp, G);
  c.take(g->o_marg, 1);
  c.take(g->o_deriv, 2 * G);
  c.take(g->o_g, G);
  c.take(g->o_h, G);
  c.take(g->o_s, G);
  c.take(g->start, G + 2);
  c.take(g->trial, G + 2);
  c.take(g->tr_ll, 1);
  c.take(g->tr_g, G + 2);
  c.take(g->tr_h, G + 2);
  c.take(g->tr_s, G + 2);
  c.take(g->k_g, G + 2);
  c.take(g->k_h, G + 2);
  c.take(g->k_s, G + 2);
  c.take(g->alpha, 1);
  c.take(g->ll, 1);
  c.take(g->trace, (size_t)kGpMaxIterations);
  c.take(g->evals, 1);
  c.take(g->status, 1);
  c.take(g->active, (size_t)kGpMaxIterations);
  c.take(g->d_hdesc, G * kGpHybridDesc);
  c.take(g->d_hformed, g->ht.formed.size());
  c.take(g->d_hlevels, g->ht.levels.size());
  c.take(g->o_hybrid, G);
  return c.at;
}

// both sweeps at branch lengths `b` (a device pointer), on stream s; matrix: the [G][P] output or nullptr
int enqueue_populate(mi_gp* g, hipStream_t s, const double* b, double* matrix) {
  GpArgs a = g->a;
  a.b = b;
  a.matrix = matrix;
  const GpDag& d = g->d;
  launch_gp_matrices(a, s);
  for (const auto& l : d.levels) launch_gp_rootward(a, l.first, l.second, s);
  launch_gp_marginal(a, s);
  for (size_t k = d.levels.size(); k-- > 0;) launch_gp_leafward(a, d.levels[k].first, d.levels[k].second, s);
  launch_gp_leaves(a, s);
  launch_gp_finalize(a, s);
  HIP_TRY(hipGetLastError());
  mi_engine* e = g->e;
  e->dominant = "gp_leafward_kernel";
  e->last_walk_launches = 2 * (int)d.levels.size() + 1;
  e->last_evals = 1;
  e->last_grad_evals = 1;
  e->last_path = "gp_populate n=" + std::to_string(d.n) + " nodes=" + std::to_string(d.nodes) + " G=" + std::to_string(d.G) +
                 " levels=" + std::to_string(d.levels.size()) + " tiles=" + std::to_string(g->tiles) +
                 (matrix ? " matrix" : "");
  return 0;
}

// a DAG-only object (mi_engine_gp_create_dag) has no vectors: whatever reads or writes them refuses it
int refuse_dag_only(const mi_gp* g, const char* call) {
  if (!g->dag_only) return 0;
  return fail(std::string("generalized pruning: ") + call +
              " needs the vectors, and this object is DAG-only (mi_engine_gp_create_dag); create it with mi_engine_gp_create");
}

int populate(mi_gp* g, hipStream_t s) {
  if (refuse_dag_only(g, "populate")) return 1;
  HIP_TRY(hipSetDevice(g->e->spec.device));
  if (enqueue_populate(g, s, g->b, nullptr)) return 1;
  g->stale = false;
  return 0;
}

// the host forms read fresh vectors: populate if b or q changed since
int fresh(mi_gp* g) {
  if (g->stale && populate(g, g->e->stream)) return 1;
  return 0;
}

int check_vector(const mi_gp* g, const double* v, int32_t count, const char* what) {
  if (!v) return fail(std::string("generalized pruning: null ") + what);
  if (count != g->d.G)
    return fail(std::string("generalized pruning: ") + what + " has " + std::to_string(count) + " entries, the DAG " +
                std::to_string(g->d.G));
  return 0;
}

}  // namespace

// mi_engine_gp_create and mi_engine_gp_create_dag: the same DAG, numbering, initial q and b; the DAG-only object
// takes any engine, and nothing that depends on the model or the patterns is allocated or launched for it
static int gp_create(mi_engine* e, int32_t T, int32_t n, const int32_t* parent_ids, const double* branch_lengths,
                     const double* model_params, double rescaling_threshold, bool dag_only, mi_gp** out) {
  if (!e) return fail("null engine");
  if (!out) return fail("null output pointer");
  *out = nullptr;
  const bool several_shards = e->shards.size() > 1;
  if (dag_only) {
    if (!e->shards.empty()) e = e->shards[0];  // (a handle of several shards: its first)
  } else {
    if (e->shards.size() == 1) e = e->shards[0];  // (a handle of one shard is its one engine)
    if (!e->shards.empty()) return fail("generalized pruning runs on a single engine, not on a sharded handle");
    if (e->s != 4) return fail("generalized pruning is 4-state only");
    if (e->K != 1) return fail("generalized pruning takes one rate category (this engine has " + std::to_string(e->K) + ")");
  }
  if (n != e->n) return fail("generalized pruning: trees of " + std::to_string(n) + " taxa, the engine has " + std::to_string(e->n));
  if (n < 3) return fail("generalized pruning needs at least 3 taxa");
  if (T < 1) return fail("tree_count must be positive");
  if (!parent_ids) return fail("null tree arrays");
  if (!dag_only && e->param_count > 0 && !model_params) return fail("generalized pruning: this engine's model takes parameters");
  if (rescaling_threshold == 0.0) rescaling_threshold = kGpDefaultThreshold;
  if (!(rescaling_threshold > 0x1p-500 && rescaling_threshold <= 1.0))
    return fail("generalized pruning: rescaling_threshold must be in (2^-500, 1]");
  mi_gp* g = new mi_gp;
  g->e = e;
  g->dag_only = dag_only;
  g->several_shards = several_shards;
  g->threshold = rescaling_threshold;
  std::vector<double> b;
  auto make = [&]() -> int {
    if (build_dag(n, T, parent_ids, branch_lengths, g->d, b)) return 1;
    const GpDag& d = g->d;
    build_hybrid_tables(d, kGpHybridMaxSummands, g->ht);
    // (a launch takes a level's nodes, or the leaves, in its second grid dimension)
    size_t widest = (size_t)n;
    for (const auto& l : d.levels) widest = std::max(widest, (size_t)l.second);
    if (widest > 65535) return fail("generalized pruning: more than 65535 taxa, or nodes on one level of the DAG");
    g->P = e->P;
    g->tiles = (e->P + kGpTile - 1) / kGpTile;
    g->Pp = g->tiles * kGpTile;
    g->I = d.nodes - n;
    HIP_TRY(hipSetDevice(e->spec.device));
    if (e->status.ensure(sizeof(int32_t) * kStatusWords)) return 1;
    if (!e->opt_word) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&e->opt_word.h), 256, hipHostMallocDefault));
    const size_t bytes = cut(g, nullptr);
    if (g->pool.ensure(bytes)) return 1;
    HIP_TRY(hipMemset(g->pool.ptr, 0, bytes));
    cut(g, g->pool.as<char>());
    b.resize((size_t)d.G + 2, 0.0);
    const std::vector<double> q = uniform_prior(d);
    if ((!dag_only && upload(g->params, model_params, sizeof(double) * e->param_count)) || upload(g->b, b.data(), sizeof(double) * b.size()) ||
        upload(g->q, q.data(), sizeof(double) * q.size()) || upload(g->d_edge, d.edge.data(), sizeof(int32_t) * d.edge.size()) ||
        upload(g->d_block, d.block_range.data(), sizeof(int32_t) * d.block_range.size()) ||
        upload(g->d_in_range, d.in_range.data(), sizeof(int32_t) * d.in_range.size()) ||
        upload(g->d_in_edges, d.in_edges.data(), sizeof(int32_t) * d.in_edges.size()) ||
        upload(g->d_order, d.order.data(), sizeof(int32_t) * d.order.size()))
      return 1;
    if (dag_only) return 0;  // (everything below belongs to the vectors)
    if (upload(g->d_hdesc, g->ht.desc.data(), sizeof(int32_t) * g->ht.desc.size()) ||
        upload(g->d_hformed, g->ht.formed.data(), sizeof(int32_t) * g->ht.formed.size()) ||
        upload(g->d_hlevels, g->ht.levels.data(), sizeof(int32_t) * g->ht.levels.size()))
      return 1;
    // the model instance, by the set-up every other call uses (no trees in this launch), and the tip codes
    hipStream_t s = e->stream;
    DeviceCall dc;
    dc.T = 1;
    dc.params = g->params;
    CallPlan p{};
    p.models_per_tree = 1;
    ModelSetupArgs ms = model_setup_args(e, dc, p);
    ms.models = g->model;
    TreeSetupArgs none{};
    none.n = n;
    none.status = e->status.as<int32_t>();
    launch_setup(none, ms, e->sw, s);
    const bool partials = !e->spec.use_tip_states && e->tip_partials.ptr;
    launch_distance_codes(e->tip_states.as<int8_t>(), partials ? e->tip_partials.as<double>() : nullptr, n, e->P, g->codes, s);
    HIP_TRY(hipGetLastError());
    if (check_status(e, s)) return 1;  // (a GTR row that does not sum to one)
    GpArgs& a = g->a;
    a.n = n;
    a.P = g->P;
    a.Pp = g->Pp;
    a.tiles = g->tiles;
    a.G = d.G;
    a.R = d.R;
    a.I = g->I;
    a.threshold = g->threshold;
    a.model = g->model;
    a.Cp = distance_code_stride(g->P);
    a.codes = g->codes;
    a.weights = e->weights.as<double>();
    a.b = g->b;
    a.q = g->q;
    a.edge = g->d_edge;
    a.block_range = g->d_block;
    a.in_range = g->d_in_range;
    a.in_edges = g->d_in_edges;
    a.order = g->d_order;
    return 0;
  };
  if (make()) {
    delete g;
    return 1;
  }
  *out = g;
  return 0;
}

extern "C" {

int32_t mi_engine_gp_create(mi_engine* e, int32_t T, int32_t n, const int32_t* parent_ids, const double* branch_lengths,
                            const double* model_params, double rescaling_threshold, mi_gp** out) {
  return gp_create(e, T, n, parent_ids, branch_lengths, model_params, rescaling_threshold, false, out);
}
int32_t mi_engine_gp_create_dag(mi_engine* e, int32_t T, int32_t n, const int32_t* parent_ids, const double* branch_lengths,
                                mi_gp** out) {
  return gp_create(e, T, n, parent_ids, branch_lengths, nullptr, 0.0, true, out);
}

void mi_gp_destroy(mi_gp* g) {
  if (!g) return;
  (void)hipSetDevice(g->e->spec.device);
  (void)hipStreamSynchronize(g->e->stream);
  delete g;
}

int32_t mi_gp_sizes(const mi_gp* g, int32_t* out) {
  if (!g || !out) return fail("null object or output pointer");
  const int32_t sizes[8] = {g->d.n, g->d.nodes, g->d.R, g->d.G, g->P, g->d.W, (int32_t)g->d.levels.size(), kGpTile};
  std::copy(sizes, sizes + 8, out);
  return 0;
}

int32_t mi_gp_structure(const mi_gp* g, int32_t* out_entries, int32_t* out_block_range, uint32_t* out_clades,
                        int32_t* out_levels, double* out_topology_count) {
  if (!g) return fail("null object");
  const GpDag& d = g->d;
  if (out_entries) std::copy(d.edge.begin(), d.edge.end(), out_entries);
  if (out_block_range) std::copy(d.block_range.begin(), d.block_range.end(), out_block_range);
  if (out_clades) std::copy(d.clades.begin(), d.clades.end(), out_clades);
  if (out_levels) std::copy(d.level.begin(), d.level.end(), out_levels);
  if (out_topology_count) *out_topology_count = d.topology_count;
  return 0;
}

// GPInstance::PrettyIndexer: a rootsplit is the smaller chunk's bit string, a PCSP
// "<sister>|<focal>|<the child's smaller chunk>" (a leaf child: zeros).  Entries are separated by '\n'.
int32_t mi_gp_strings(const mi_gp* g, char* buffer, int64_t capacity, int64_t* out_needed) {
  if (!g) return fail("null object");
  const GpDag& d = g->d;
  auto bits = [&](int node, int clade) {
    std::string s(d.n, '0');
    const uint32_t* w = &d.clades[((size_t)node * 2 + clade) * d.W];
    for (int x = 0; x < d.n; x++)
      if (w[x / 32] >> (x % 32) & 1) s[x] = '1';
    return s;
  };
  std::string all;
  for (int i = 0; i < d.G; i++) {
    const int t = d.edge[3 * i], c = d.edge[3 * i + 1], s = d.edge[3 * i + 2];
    if (i) all += '\n';
    if (i < d.R) all += bits(s, 1);
    else all += bits(t, 1 - c) + "|" + bits(t, c) + "|" + (s < d.n ? std::string(d.n, '0') : bits(s, 1));
  }
  if (out_needed) *out_needed = (int64_t)all.size() + 1;
  if (buffer) {
    if (capacity < (int64_t)all.size() + 1) return fail("generalized pruning: the string buffer is too small");
    std::memcpy(buffer, all.c_str(), all.size() + 1);
  }
  return 0;
}

int32_t mi_gp_set_branch_lengths(mi_gp* g, const double* b, int32_t count) {
  if (!g) return fail("null object");
  if (check_vector(g, b, count, "branch_lengths")) return 1;
  for (int i = 0; i < count; i++)
    if (!(b[i] >= 0.0) || std::isinf(b[i])) return fail("generalized pruning: branch lengths must be finite and not negative");
  std::vector<double> v(b, b + count);
  for (int i = 0; i < g->d.R; i++) v[i] = 0.0;  // (a rootsplit entry carries no branch)
  HIP_TRY(hipSetDevice(g->e->spec.device));
  HIP_TRY(hipStreamSynchronize(g->e->stream));
  g->stale = true;
  return upload(g->b, v.data(), sizeof(double) * count);
}
int32_t mi_gp_get_branch_lengths(mi_gp* g, double* out) {
  if (!g || !out) return fail("null object or output pointer");
  HIP_TRY(hipSetDevice(g->e->spec.device));
  HIP_TRY(hipStreamSynchronize(g->e->stream));
  return download(out, g->b, sizeof(double) * g->d.G);
}
int32_t mi_gp_set_sbn_parameters(mi_gp* g, const double* q, int32_t count) {
  if (!g) return fail("null object");
  if (check_vector(g, q, count, "sbn_parameters")) return 1;
  for (int i = 0; i < count; i++)
    if (!(q[i] >= 0.0) || std::isinf(q[i])) return fail("generalized pruning: SBN parameters must be finite and not negative");
  HIP_TRY(hipSetDevice(g->e->spec.device));
  HIP_TRY(hipStreamSynchronize(g->e->stream));
  g->stale = true;
  return upload(g->q, q, sizeof(double) * count);
}
int32_t mi_gp_get_sbn_parameters(mi_gp* g, double* out) {
  if (!g || !out) return fail("null object or output pointer");
  HIP_TRY(hipSetDevice(g->e->spec.device));
  HIP_TRY(hipStreamSynchronize(g->e->stream));
  return download(out, g->q, sizeof(double) * g->d.G);
}

int32_t mi_gp_node_probabilities(const mi_gp* g, const double* q, int32_t count, double* out) {
  if (!g || !out) return fail("null object or output pointer");
  if (check_vector(g, q, count, "sbn_parameters")) return 1;
  node_probabilities(g->d, q, out);
  return 0;
}
int32_t mi_gp_inverted_probabilities(const mi_gp* g, const double* q, int32_t count, double* out) {
  if (!g || !out) return fail("null object or output pointer");
  if (check_vector(g, q, count, "sbn_parameters")) return 1;
  const GpDag& d = g->d;
  std::vector<double> node(d.nodes);
  node_probabilities(d, q, node.data());
  for (int i = 0; i < d.R; i++) out[i] = 1.0;
  for (int i = d.R; i < d.G; i++) out[i] = node[d.edge[3 * i]] * q[i] / node[d.edge[3 * i + 2]];
  return 0;
}

int32_t mi_gp_populate_device(mi_gp* g, void* stream) {
  if (!g) return fail("null object");
  return populate(g, pick_stream(g->e, stream));
}
int32_t mi_gp_populate(mi_gp* g) {
  if (!g) return fail("null object");
  if (populate(g, g->e->stream)) return 1;
  HIP_TRY(hipStreamSynchronize(g->e->stream));
  return 0;
}

int32_t mi_gp_likelihoods_device(mi_gp* g, void* stream, double* out_per_gpcsp, double* out_log_marginal) {
  if (!g) return fail("null object");
  if (refuse_dag_only(g, "likelihoods")) return 1;
  HIP_TRY(hipSetDevice(g->e->spec.device));
  launch_gp_outputs(g->a, out_per_gpcsp, out_log_marginal, nullptr, nullptr, nullptr, nullptr, pick_stream(g->e, stream));
  HIP_TRY(hipGetLastError());
  return 0;
}
int32_t mi_gp_likelihoods(mi_gp* g, double* out_per_gpcsp, double* out_log_marginal, double* out_pattern, double* out_matrix) {
  if (!g) return fail("null object");
  if (refuse_dag_only(g, "likelihoods")) return 1;
  mi_engine* e = g->e;
  HIP_TRY(hipSetDevice(e->spec.device));
  const size_t G = g->d.G, P = g->P;
  if (out_matrix) {
    if (g->matrix.ensure(sizeof(double) * G * P)) return 1;
    if (enqueue_populate(g, e->stream, g->b, g->matrix.as<double>())) return 1;
    g->stale = false;
  } else if (fresh(g)) {
    return 1;
  }
  if (mi_gp_likelihoods_device(g, nullptr, g->o_gpcsp, g->o_marg)) return 1;
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (download(out_per_gpcsp, g->o_gpcsp, sizeof(double) * G) || download(out_log_marginal, g->o_marg, sizeof(double)) ||
      download(out_pattern, g->a.log_marg, sizeof(double) * P) ||
      download(out_matrix, g->matrix.ptr, sizeof(double) * G * P))
    return 1;
  return 0;
}

int32_t mi_gp_branch_derivatives_device(mi_gp* g, void* stream, double* out_ll_derivative, double* out_gradient,
                                        double* out_hessian, double* out_gsq) {
  if (!g) return fail("null object");
  if (refuse_dag_only(g, "branch_derivatives")) return 1;
  HIP_TRY(hipSetDevice(g->e->spec.device));
  launch_gp_outputs(g->a, nullptr, nullptr, out_ll_derivative, out_gradient, out_hessian, out_gsq, pick_stream(g->e, stream));
  HIP_TRY(hipGetLastError());
  return 0;
}
int32_t mi_gp_branch_derivatives(mi_gp* g, double* out_ll_derivative, double* out_gradient, double* out_hessian,
                                 double* out_gsq) {
  if (!g) return fail("null object");
  if (refuse_dag_only(g, "branch_derivatives")) return 1;
  HIP_TRY(hipSetDevice(g->e->spec.device));
  if (fresh(g)) return 1;
  if (mi_gp_branch_derivatives_device(g, nullptr, g->o_deriv, g->o_g, g->o_h, g->o_s)) return 1;
  HIP_TRY(hipStreamSynchronize(g->e->stream));
  const size_t G = g->d.G, d = sizeof(double);
  if (download(out_ll_derivative, g->o_deriv, d * 2 * G) || download(out_gradient, g->o_g, d * G) ||
      download(out_hessian, g->o_h, d * G) || download(out_gsq, g->o_s, d * G))
    return 1;
  return 0;
}

// GPEngine / GPInstance::EstimateSBNParameters: populate, likelihoods, then per block and for the rootsplits
// q <- softmax(per_gpcsp_log_likelihood + log q); a block of one entry gets 1.  One logsumexp per block, in order.
// With hybrid [G] (UpdateSBNProbabilities' other branch): a block whose entries all have a finite hybrid marginal
// takes softmax(hybrid + log q) instead; the rootsplits never do.
static int estimate_sbn(mi_gp* g, const double* hybrid, double* out_q) {
  const GpDag& d = g->d;
  std::vector<double> ll(d.G), q(d.G);
  if (mi_gp_likelihoods(g, ll.data(), nullptr, nullptr, nullptr)) return 1;
  if (download(q.data(), g->q, sizeof(double) * d.G)) return 1;
  auto block = [&](int begin, int end, bool may_be_hybrid) {
    if (end - begin == 1) {
      q[begin] = 1.0;
      return;
    }
    bool use = may_be_hybrid && hybrid;
    for (int i = begin; use && i < end; i++) use = std::isfinite(hybrid[i]);
    if (use) std::copy(hybrid + begin, hybrid + end, ll.begin() + begin);
    double m = -INFINITY;
    for (int i = begin; i < end; i++) {
      ll[i] += std::log(q[i]);
      m = std::max(m, ll[i]);
    }
    double sum = 0.0;
    for (int i = begin; i < end; i++) sum += std::exp(ll[i] - m);
    const double lse = m + std::log(sum);
    for (int i = begin; i < end; i++) q[i] = std::exp(ll[i] - lse);
  };
  block(0, d.R, false);
  for (int v = d.n; v < d.nodes; v++)
    for (int c = 0; c < 2; c++) block(d.block_range[(v * 2 + c) * 2], d.block_range[(v * 2 + c) * 2 + 1], true);
  for (double x : q)
    if (!(x >= 0.0)) return fail("generalized pruning: the SBN estimate is not finite (a likelihood of zero?)");
  g->stale = true;
  if (upload(g->q, q.data(), sizeof(double) * d.G)) return 1;
  if (out_q) std::copy(q.begin(), q.end(), out_q);
  return 0;
}
int32_t mi_gp_estimate_sbn_parameters(mi_gp* g, double* out_q) {
  if (!g) return fail("null object");
  if (refuse_dag_only(g, "estimate_sbn_parameters")) return 1;
  return estimate_sbn(g, nullptr, out_q);
}
int32_t mi_gp_estimate_sbn_parameters_hybrid(mi_gp* g, double* out_q) {
  if (!g) return fail("null object");
  if (refuse_dag_only(g, "estimate_sbn_parameters_hybrid")) return 1;
  std::vector<double> hybrid(g->d.G);
  if (mi_gp_hybrid_marginals(g, hybrid.data(), nullptr)) return 1;
  return estimate_sbn(g, hybrid.data(), out_q);
}

// ---- quartet hybrid marginals ----
int32_t mi_gp_hybrid_requests(const mi_gp* g, int32_t* out_requests, int32_t* out_summand_entries,
                              int32_t* out_summand_count) {
  if (!g) return fail("null object");
  const HybridTables& t = g->ht;
  if (t.too_large) return refuse_too_large(t);
  for (int e = 0; e < g->d.G; e++) {
    const int32_t* row = &t.desc[(size_t)e * kGpHybridDesc];
    // (formed, first summand, summand count: a row's first three words)
    if (out_requests) std::copy(row, row + 3, out_requests + 3 * (size_t)e);
    if (!out_summand_entries || !row[0]) continue;
    int32_t* out = out_summand_entries + 4 * (size_t)row[1];  // (written on demand: the object keeps no [S][4] table)
    for (int ig = row[4]; ig < row[5]; ig++)
      for (int a = row[6]; a < row[7]; a++)
        for (int b = row[8]; b < row[9]; b++)
          for (int o = row[10]; o < row[11]; o++, out += 4) {
            out[0] = g->d.in_edges[ig];
            out[1] = a;
            out[2] = b;
            out[3] = o;
          }
  }
  if (out_summand_count) *out_summand_count = t.S;
  return 0;
}

// Host code only, no engine and no device: the DAG of the batch and its requests, counted.
int32_t mi_gp_hybrid_request_count(int32_t T, int32_t n, const int32_t* parent_ids, int64_t max_summands,
                                   int32_t* out_formed, int64_t* out_summands) {
  if (n < 3) return fail("generalized pruning needs at least 3 taxa");
  if (T < 1) return fail("tree_count must be positive");
  if (!parent_ids) return fail("null tree arrays");
  if (max_summands < 0 || max_summands > kGpHybridMaxSummands)
    return fail("generalized pruning: max_summands must be in [0, 2^28] (0: 2^28, the library's limit)");
  GpDag d;
  std::vector<double> b;
  if (build_dag(n, T, parent_ids, nullptr, d, b)) return 1;
  HybridTables t;
  build_hybrid_tables(d, max_summands ? max_summands : kGpHybridMaxSummands, t);
  if (t.too_large) return refuse_too_large(t);
  if (out_formed) *out_formed = t.F;
  if (out_summands) *out_summands = t.S;
  return 0;
}

int32_t mi_gp_reserve_hybrid(mi_gp* g) {
  if (!g) return fail("null object");
  if (refuse_dag_only(g, "reserve_hybrid")) return 1;
  if (g->hybrid_reserved) return 0;
  const HybridTables& t = g->ht;
  if (t.too_large) return refuse_too_large(t);
  const size_t G = g->d.G, Pp = g->Pp, nodes = g->d.nodes;
  if (G > 65535) return fail("generalized pruning: hybrid marginals take at most 65535 entries");
  GpHybridArgs& h = g->h;
  auto lay = [&](char* base, size_t& evolve, size_t& partial) {
    Cutter c{base};
    c.take(h.z, G * 4 * Pp);
    c.take(h.a, G * 4 * Pp);
    c.take(h.ez, G * Pp);
    c.take(h.ea, G * Pp);
    evolve = c.at;
    c.take(h.partial, (size_t)t.S * g->tiles);
    c.take(h.summ, (size_t)t.S);
    c.take(g->o_summands, (size_t)t.S);
    partial = c.at - evolve;
    c.take(h.pr, nodes);
    c.take(h.log_pr, nodes);
    c.take(h.inv, G);
    return c.at;
  };
  size_t evolve = 0, partial = 0;
  const size_t bytes = lay(nullptr, evolve, partial);
  if (evolve + partial > g->e->plv_budget)
    return fail("generalized pruning: hybrid marginals need " + std::to_string(evolve) + " bytes of evolved vectors and " +
                std::to_string(partial) + " bytes of partial sums and summands (" + std::to_string(t.S) +
                " summands), over the budget of " + std::to_string(g->e->plv_budget) + " bytes (MI_PHYLO_PLV_BYTES)");
  HIP_TRY(hipSetDevice(g->e->spec.device));
  if (g->hybrid.ensure(bytes)) return 1;
  HIP_TRY(hipMemset(g->hybrid.ptr, 0, bytes));
  lay(g->hybrid.as<char>(), evolve, partial);
  h.L = (int)g->d.levels.size();
  h.F = t.F;
  h.S = t.S;
  h.Z = g->e->sw.gp_hybrid_z > 0 ? g->e->sw.gp_hybrid_z : t.Z;
  h.level_range = g->d_hlevels;
  h.desc = g->d_hdesc;
  h.formed = g->d_hformed;
  h.widest = t.widest;
  g->hybrid_reserved = true;
  return 0;
}

int32_t mi_gp_hybrid_marginals_device(mi_gp* g, void* stream, double* out_hybrid, double* out_summands) {
  if (!g) return fail("null object");
  if (refuse_dag_only(g, "hybrid_marginals")) return 1;
  if (!out_hybrid) return fail("null output pointer");
  if (!g->hybrid_reserved)
    return fail("generalized pruning: mi_gp_hybrid_marginals_device before mi_gp_reserve_hybrid (the device form allocates nothing)");
  HIP_TRY(hipSetDevice(g->e->spec.device));
  launch_gp_hybrid(g->a, g->h, out_hybrid, out_summands, pick_stream(g->e, stream));
  HIP_TRY(hipGetLastError());
  mi_engine* e = g->e;
  e->dominant = "gp_hybrid_summand_kernel";
  e->last_path = "gp_hybrid formed=" + std::to_string(g->ht.F) + " summands=" + std::to_string(g->ht.S) +
                 " tiles=" + std::to_string(g->tiles) + " z=" + std::to_string(g->h.Z);
  return 0;
}

int32_t mi_gp_hybrid_marginals(mi_gp* g, double* out_hybrid, double* out_summands) {
  if (!g) return fail("null object");
  if (refuse_dag_only(g, "hybrid_marginals")) return 1;
  HIP_TRY(hipSetDevice(g->e->spec.device));
  if (mi_gp_reserve_hybrid(g)) return 1;
  if (fresh(g)) return 1;
  if (mi_gp_hybrid_marginals_device(g, nullptr, g->o_hybrid, out_summands ? g->o_summands : nullptr)) return 1;
  HIP_TRY(hipStreamSynchronize(g->e->stream));
  if (download(out_hybrid, g->o_hybrid, sizeof(double) * g->d.G) ||
      download(out_summands, g->o_summands, sizeof(double) * g->ht.S))
    return 1;
  return 0;
}

// Maximise log_marginal over all branch lengths at once by the rule of DESIGN.md 4.9: the DAG is one tree of
// G - R branches for branch_opt_step_kernel (a row of N = G - R + 2 entries).  An evaluation is both sweeps at the
// trial point.  out_trace [max_iterations]: the accepted marginal after each evaluation.
int32_t mi_gp_optimize_branch_lengths(mi_gp* g, const mi_branch_opt_options* options, double* out_trace,
                                      int32_t* out_evaluations, int32_t* out_status) {
  if (!g) return fail("null object");
  if (refuse_dag_only(g, "optimize_branch_lengths")) return 1;
  if (!out_status) return fail("null output pointer");
  mi_engine* e = g->e;
  mi_branch_opt_options o = options ? *options : kBranchOptDefaults;
  if (!options) {
    o.min_length = std::exp(-13.9);
    o.max_length = std::exp(1.1);
  }
  if (check_branch_opt_options(o)) return 1;
  if (o.max_iterations > kGpMaxIterations) return fail("generalized pruning: max_iterations is at most 1000");
  HIP_TRY(hipSetDevice(e->spec.device));
  hipStream_t s = e->stream;
  const GpDag& d = g->d;
  const int R = d.R, nb = d.G - R;
  HIP_TRY(hipMemsetAsync(g->active, 0, sizeof(int32_t) * o.max_iterations, s));
  HIP_TRY(hipMemcpyAsync(g->start, g->b, sizeof(double) * (d.G + 2), hipMemcpyDeviceToDevice, s));
  BranchOptArgs st{};
  st.N = nb + 2;
  st.T = 1;
  st.count = 1;
  st.evals_max = o.max_iterations;
  st.tol = o.tolerance;
  st.tmin = o.min_length;
  st.tmax = o.max_length;
  st.map = nullptr;
  st.tr_ll = g->tr_ll;
  st.tr_g = g->tr_g + R;
  st.tr_h = g->tr_h + R;
  st.tr_s = g->tr_s + R;
  st.trial = g->trial + R;
  st.trial_full = nullptr;
  st.bl = g->b + R;
  st.ll = g->ll;
  st.g = g->k_g + R;
  st.h = g->k_h + R;
  st.s = g->k_s + R;
  st.alpha = g->alpha;
  st.evals = g->evals;
  st.status = g->status;
  st.active = g->active;
  launch_branch_opt_init(st, g->start + R, s);
  // (entries 0 .. R-1 of the trial point are never written: zero since creation)
  int passes = 0;
  for (int it = 0; it < o.max_iterations; it++) {
    if (enqueue_populate(g, s, g->trial, nullptr)) return 1;
    launch_gp_outputs(g->a, nullptr, g->tr_ll, nullptr, g->tr_g, g->tr_h, g->tr_s, s);
    st.pass = it;
    launch_branch_opt_step(st, s);
    HIP_TRY(hipMemcpyAsync(g->trace + it, g->ll, sizeof(double), hipMemcpyDeviceToDevice, s));
    passes++;
    if (it + 1 == o.max_iterations) break;
    if ((it + 1) % o.check_interval) continue;
    HIP_TRY(hipMemcpyAsync(e->opt_word, g->active + it, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (*e->opt_word <= 0) break;
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s));
  g->stale = true;  // (the vectors are the last trial point's)
  int32_t evals = 0;
  if (download(&evals, g->evals, sizeof evals) || download(out_status, g->status, sizeof(int32_t))) return 1;
  if (out_evaluations) *out_evaluations = evals;
  if (out_trace && download(out_trace, g->trace, sizeof(double) * evals)) return 1;
  e->last_path += " opt evals=" + std::to_string(evals) + " passes=" + std::to_string(passes);
  e->last_evals = e->last_grad_evals = evals;
  return 0;
}

}  // extern "C"
