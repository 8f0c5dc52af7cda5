// Trees of the subsplit DAG: the tables the tree kernels read and the per-tree
// workspace (mi_gp_reserve_trees), the index of rooted trees into the DAG, log q and the GP branch
// lengths of indexed trees, the rooted TrainSimpleAverage, the sampler, the enumerator, and
// de-rooting on any engine.  The kernels are kernels_gp_trees.hip's.  A *_device form enqueues on
// the caller's stream and allocates and synchronises nothing; a host form reserves on first use and
// is one HostCall on the object's engine.
#include <cmath>
#include <vector>

#include "mi_phylo_engine.h"
#include "mi_phylo_gp_host.h"

namespace {

uint64_t add_capped(uint64_t a, uint64_t b) { return std::min(a + b, kGpTreesCountCap); }  // (both at most 2^62)
uint64_t mul_capped(uint64_t a, uint64_t b) {
  const unsigned __int128 p = (unsigned __int128)a * b;
  return p > kGpTreesCountCap ? kGpTreesCountCap : (uint64_t)p;
}

// what the kernels read beyond the object's entries and block ranges
struct TreeTables {
  std::vector<int32_t> table, root_entry;
  std::vector<uint64_t> below, options1;
  uint64_t topologies = 0;
};

void build_tree_tables(const GpDag& d, TreeTables& t) {
  const int W = d.W, I = d.nodes - d.n;
  size_t slots = 16;
  while (slots < 2 * (size_t)I) slots *= 2;
  t.table.assign(slots, -1);
  for (int v = d.n; v < d.nodes; v++) {
    uint32_t h = kGpTreeHashSeed;
    for (int w = 0; w < 2 * W; w++) h = gp_tree_hash_step(h, d.clades[(size_t)v * 2 * W + w]);
    size_t slot = gp_tree_hash_end(h) & (slots - 1);
    while (t.table[slot] >= 0) slot = (slot + 1) & (slots - 1);
    t.table[slot] = v;
  }
  t.root_entry.assign(d.nodes, -1);
  for (int i = 0; i < d.R; i++) t.root_entry[d.edge[3 * i + 2]] = i;
  t.below.assign(d.nodes, 1);
  t.options1.assign(d.nodes, 1);
  for (int v : d.order) {
    uint64_t options[2] = {0, 0};
    for (int c = 0; c < 2; c++)
      for (int i = d.block_range[(v * 2 + c) * 2]; i < d.block_range[(v * 2 + c) * 2 + 1]; i++)
        options[c] = add_capped(options[c], t.below[d.edge[3 * i + 2]]);
    t.options1[v] = options[1];
    t.below[v] = mul_capped(options[0], options[1]);
  }
  t.topologies = 0;
  for (int i = 0; i < d.R; i++) t.topologies = add_capped(t.topologies, t.below[d.edge[3 * i + 2]]);
}

struct TreeLayout {
  uint32_t* clades;
  int32_t *table, *root_entry;
  uint64_t *below, *options1;
  double* cdf;
  int32_t* store;
  // the rooted TrainSimpleAverage
  uint32_t *keys, *keys2, *vals, *vals2;
  char* sort_tmp;
  double *counts, *new_q;
  size_t sort_bytes, tables_end;
};

// Sizes (base null) or cuts the reservation.  It writes into `l` alone: the object keeps its pointers until a
// new allocation has succeeded, so a refused reservation leaves a smaller, earlier one in working order.
size_t lay_trees(const mi_gp* g, size_t slots, int cap, char* base, TreeLayout& l) {
  const GpDag& d = g->d;
  const size_t N = 2 * (size_t)d.n - 1, waves = ((size_t)cap + 63) / 64;
  bool index_lds, build_lds;
  const size_t iw = gp_tree_index_words(d.n), bw = gp_tree_build_words(d.n);
  gp_trees_per_wave(iw, g->e->sw.gp_trees_global, index_lds);
  gp_trees_per_wave(bw, g->e->sw.gp_trees_global, build_lds);
  const size_t store_words = waves * 64 * std::max(index_lds ? 0 : iw, build_lds ? 0 : bw);
  Cutter c{base};
  c.take(l.clades, (size_t)d.nodes * 2 * d.W);
  c.take(l.table, slots);
  c.take(l.root_entry, (size_t)d.nodes);
  c.take(l.below, (size_t)d.nodes);
  c.take(l.options1, (size_t)d.nodes);
  c.take(l.cdf, (size_t)d.G);
  c.take(l.counts, (size_t)d.G);
  c.take(l.new_q, (size_t)d.G);
  l.tables_end = c.at;
  c.take(l.store, store_words);
  c.take(l.keys, cap * N);
  c.take(l.keys2, cap * N);
  c.take(l.vals, cap * N);
  c.take(l.vals2, cap * N);
  l.sort_bytes = gp_train_sort_tmp_bytes(cap * N);
  c.take(l.sort_tmp, l.sort_bytes);
  return c.at;
}

int reserve_trees(mi_gp* g, int cap) {
  if (cap < 1) return fail("generalized pruning: tree_capacity must be positive");
  if (cap <= g->tree_capacity) return 0;
  mi_engine* e = g->e;
  const GpDag& d = g->d;
  TreeTables tt;
  build_tree_tables(d, tt);
  TreeLayout l{};
  const size_t bytes = lay_trees(g, tt.table.size(), cap, nullptr, l);
  if (bytes - l.tables_end > e->plv_budget)
    return fail("generalized pruning: the workspace of " + std::to_string(cap) + " trees of " + std::to_string(d.n) +
                " taxa takes " + std::to_string(bytes - l.tables_end) + " bytes, over the budget of " +
                std::to_string(e->plv_budget) + " bytes (MI_PHYLO_PLV_BYTES); index, sample or enumerate fewer trees per call");
  HIP_TRY(hipSetDevice(e->spec.device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (e->status.ensure(sizeof(int32_t) * kStatusWords)) return 1;
  g->tree_capacity = 0;
  if (g->trees.ensure(bytes)) return 1;
  HIP_TRY(hipMemset(g->trees.ptr, 0, bytes));
  lay_trees(g, tt.table.size(), cap, g->trees.as<char>(), l);
  if (upload(l.clades, d.clades.data(), sizeof(uint32_t) * d.clades.size()) ||
      upload(l.table, tt.table.data(), sizeof(int32_t) * tt.table.size()) ||
      upload(l.root_entry, tt.root_entry.data(), sizeof(int32_t) * tt.root_entry.size()) ||
      upload(l.below, tt.below.data(), sizeof(uint64_t) * tt.below.size()) ||
      upload(l.options1, tt.options1.data(), sizeof(uint64_t) * tt.options1.size()))
    return 1;
  GpTreesArgs& a = g->t;
  a.n = d.n;
  a.W = d.W;
  a.nodes = d.nodes;
  a.R = d.R;
  a.G = d.G;
  a.slots = (int)tt.table.size();
  a.edge = g->d_edge;
  a.block_range = g->d_block;
  a.clades = l.clades;
  a.table = l.table;
  a.root_entry = l.root_entry;
  a.below = l.below;
  a.options1 = l.options1;
  a.q = g->q;
  a.b = g->b;
  a.cdf = l.cdf;
  a.store = l.store;
  a.status = e->status.as<int32_t>();
  a.force_global = e->sw.gp_trees_global ? 1 : 0;
  GpTrainArgs& tr = g->train;
  tr.n = d.n;
  tr.nodes = d.nodes;
  tr.R = d.R;
  tr.G = d.G;
  tr.block_range = g->d_block;
  tr.keys = l.keys;
  tr.keys2 = l.keys2;
  tr.vals = l.vals;
  tr.vals2 = l.vals2;
  tr.sort_tmp = l.sort_tmp;
  tr.sort_tmp_bytes = l.sort_bytes;
  tr.counts = l.counts;
  tr.out_q = l.new_q;
  tr.status = a.status;
  g->topologies = tt.topologies;
  g->counted = true;
  g->tree_capacity = cap;
  return 0;
}

// a *_device form: the reservation must be there already
int check_reserved(const mi_gp* g, int T, const char* call) {
  if (T < 1) return fail("tree_count must be positive");
  if (T > g->tree_capacity)
    return fail(std::string("generalized pruning: ") + call + " of " + std::to_string(T) + " trees, mi_gp_reserve_trees reserved " +
                std::to_string(g->tree_capacity) + " (the device form allocates nothing)");
  return 0;
}

void note(mi_gp* g, const char* kernel, int T, size_t words) {
  bool in_lds;
  gp_trees_per_wave(words, g->e->sw.gp_trees_global, in_lds);
  mi_engine* e = g->e;
  e->dominant = kernel;
  e->last_path = "gp_trees n=" + std::to_string(g->d.n) + " T=" + std::to_string(T) + " store=" + (in_lds ? "lds" : "global");
}

int build_device(mi_gp* g, hipStream_t s, int K, int sample, uint64_t seed, int64_t first, int32_t* out_parent_ids,
                 int32_t* out_entries, double* out_log_q, double* out_lengths, double* out_cdf) {
  if (!out_parent_ids || !out_entries || !out_log_q) return fail("null output pointer");
  HIP_TRY(hipSetDevice(g->e->spec.device));
  if (sample) launch_gp_tree_cdf(g->t, out_cdf, s);
  launch_gp_tree_build(g->t, K, sample, seed, first, nullptr, out_parent_ids, out_entries, out_log_q, out_lengths, s);
  HIP_TRY(hipGetLastError());
  note(g, "gp_tree_build_kernel", K, gp_tree_build_words(g->d.n));
  return 0;
}

// the DAG's topology count (saturated), known before anything is reserved: host arithmetic on the DAG
void count_topologies(mi_gp* g) {
  if (g->counted) return;
  TreeTables tt;
  build_tree_tables(g->d, tt);
  g->topologies = tt.topologies;
  g->counted = true;
}

int check_enumeration(mi_gp* g, int64_t first, int32_t count) {
  if (count < 1) return fail("tree_count must be positive");
  count_topologies(g);
  if (g->topologies >= kGpTreesCountCap)
    return fail("generalized pruning: this DAG has 2^62 topologies or more; its trees are not enumerated (sampling serves any DAG)");
  if (first < 0 || (uint64_t)first + (uint64_t)count > g->topologies)
    return fail("generalized pruning: trees " + std::to_string(first) + " .. " + std::to_string(first + count - 1) +
                " were asked for, the DAG has " + std::to_string(g->topologies) + " topologies");
  return 0;
}

// the host side of sample / enumerate
int build_host(mi_gp* g, int K, int sample, uint64_t seed, int64_t first, int32_t* out_parent_ids, int32_t* out_entries,
               double* out_log_q, double* out_lengths, double* out_cdf) {
  if (K < 1) return fail("tree_count must be positive");
  if (!sample && check_enumeration(g, first, K)) return 1;  // (the range first: nothing is allocated for a refused one)
  if (reserve_trees(g, K)) return 1;
  const size_t N = 2 * (size_t)g->d.n - 1;
  Unwanted spare;
  HostCall c;
  c.out = {fixed(spare(out_parent_ids, K * (N - 1)), K * (N - 1)), fixed(spare(out_entries, K * N), K * N),
           fixed(spare(out_log_q, (size_t)K), (size_t)K), fixed(out_lengths, K * N), fixed(out_cdf, (size_t)g->d.G)};
  c.enqueue = [=](mi_engine* e, int, const HostArray*, const HostArray* out) {
    return build_device(g, e->stream, K, sample, seed, first, out[0].at<int32_t>(), out[1].at<int32_t>(), out[2].at<double>(),
                        out[3].at<double>(), out[4].at<double>());
  };
  c.deliver_on_error = true;  // (the outputs are written for every sample, the refused one's as -1 and NaN)
  return run_on_engine(g->e, c);
}

}  // namespace

extern "C" {

int32_t mi_gp_reserve_trees(mi_gp* g, int32_t tree_capacity) {
  if (!g) return fail("null object");
  return reserve_trees(g, tree_capacity);
}

int32_t mi_gp_topology_count(mi_gp* g, uint64_t* out_count) {
  if (!g || !out_count) return fail("null object or output pointer");
  count_topologies(g);
  *out_count = g->topologies;
  return 0;
}

int32_t mi_gp_tree_index_device(mi_gp* g, void* stream, int32_t T, const int32_t* parent_ids, int32_t* out_entries,
                                int32_t* out_nodes) {
  if (!g) return fail("null object");
  if (!parent_ids || !out_entries) return fail("null tree arrays or output pointer");
  if (check_reserved(g, T, "mi_gp_tree_index_device")) return 1;
  HIP_TRY(hipSetDevice(g->e->spec.device));
  launch_gp_tree_index(g->t, T, parent_ids, out_entries, out_nodes, pick_stream(g->e, stream));
  HIP_TRY(hipGetLastError());
  note(g, "gp_tree_index_kernel", T, gp_tree_index_words(g->d.n));
  return 0;
}
int32_t mi_gp_tree_index(mi_gp* g, int32_t T, const int32_t* parent_ids, int32_t* out_entries, int32_t* out_nodes) {
  if (!g) return fail("null object");
  if (!parent_ids || !out_entries) return fail("null tree arrays or output pointer");
  if (T < 1) return fail("tree_count must be positive");
  if (reserve_trees(g, T)) return 1;
  const size_t N = 2 * (size_t)g->d.n - 1;
  HostCall c;
  c.in = {fixed(parent_ids, T * (N - 1))};
  c.out = {fixed(out_entries, T * N), fixed(out_nodes, T * N)};
  c.enqueue = [=](mi_engine* e, int, const HostArray* in, const HostArray* out) {
    return mi_gp_tree_index_device(g, e->stream, T, in[0].at<const int32_t>(), out[0].at<int32_t>(), out[1].at<int32_t>());
  };
  return run_on_engine(g->e, c);
}

int32_t mi_gp_tree_log_prob_device(mi_gp* g, void* stream, int32_t T, const int32_t* entries, double* out_log_q) {
  if (!g) return fail("null object");
  if (!entries || !out_log_q) return fail("null input or output pointer");
  if (check_reserved(g, T, "mi_gp_tree_log_prob_device")) return 1;
  HIP_TRY(hipSetDevice(g->e->spec.device));
  launch_gp_tree_log_prob(g->t, T, entries, out_log_q, pick_stream(g->e, stream));
  HIP_TRY(hipGetLastError());
  g->e->dominant = "gp_tree_log_prob_kernel";
  return 0;
}
int32_t mi_gp_tree_log_prob(mi_gp* g, int32_t T, const int32_t* entries, double* out_log_q) {
  if (!g) return fail("null object");
  if (!entries || !out_log_q) return fail("null input or output pointer");
  if (T < 1) return fail("tree_count must be positive");
  if (reserve_trees(g, T)) return 1;
  const size_t N = 2 * (size_t)g->d.n - 1;
  HostCall c;
  c.in = {fixed(entries, T * N)};
  c.out = {fixed(out_log_q, (size_t)T)};
  c.enqueue = [=](mi_engine* e, int, const HostArray* in, const HostArray* out) {
    return mi_gp_tree_log_prob_device(g, e->stream, T, in[0].at<const int32_t>(), out[0].at<double>());
  };
  return run_on_engine(g->e, c);
}

int32_t mi_gp_tree_branch_lengths_device(mi_gp* g, void* stream, int32_t T, const int32_t* entries, double missing_length,
                                         double* out_branch_lengths) {
  if (!g) return fail("null object");
  if (!entries || !out_branch_lengths) return fail("null input or output pointer");
  if (check_reserved(g, T, "mi_gp_tree_branch_lengths_device")) return 1;
  HIP_TRY(hipSetDevice(g->e->spec.device));
  launch_gp_tree_lengths(g->t, T, entries, missing_length, out_branch_lengths, pick_stream(g->e, stream));
  HIP_TRY(hipGetLastError());
  g->e->dominant = "gp_tree_lengths_kernel";
  return 0;
}
int32_t mi_gp_tree_branch_lengths(mi_gp* g, int32_t T, const int32_t* entries, double missing_length, double* out_branch_lengths) {
  if (!g) return fail("null object");
  if (!entries || !out_branch_lengths) return fail("null input or output pointer");
  if (T < 1) return fail("tree_count must be positive");
  if (reserve_trees(g, T)) return 1;
  const size_t N = 2 * (size_t)g->d.n - 1;
  HostCall c;
  c.in = {fixed(entries, T * N)};
  c.out = {fixed(out_branch_lengths, T * N)};
  c.enqueue = [=](mi_engine* e, int, const HostArray* in, const HostArray* out) {
    return mi_gp_tree_branch_lengths_device(g, e->stream, T, in[0].at<const int32_t>(), missing_length, out[0].at<double>());
  };
  return run_on_engine(g->e, c);
}

int32_t mi_gp_train_simple_average(mi_gp* g, int32_t T, const int32_t* entries, const double* tree_weights, double* out_q) {
  if (!g) return fail("null object");
  if (!entries) return fail("null input pointer");
  if (T < 1) return fail("tree_count must be positive");
  if (reserve_trees(g, T)) return 1;
  const size_t N = 2 * (size_t)g->d.n - 1, G = g->d.G;
  HostCall c;
  c.in = {fixed(entries, T * N), fixed(tree_weights, (size_t)T)};
  c.out = {fixed(out_q, G)};
  c.enqueue = [=](mi_engine* e, int, const HostArray* in, const HostArray* out) {
    GpTrainArgs a = g->train;
    a.T = T;
    a.entries = in[0].at<const int32_t>();
    a.weights = in[1].at<const double>();
    if (launch_gp_train(a, e->stream)) return fail("generalized pruning: the radix sort of the training entries failed");
    HIP_TRY(hipGetLastError());
    e->dominant = "gp_train_runs_kernel";
    if (out[0].dev) HIP_TRY(hipMemcpyAsync(out[0].dev, a.out_q, sizeof(double) * G, hipMemcpyDeviceToDevice, e->stream));
    return 0;
  };
  if (run_on_engine(g->e, c)) return 1;  // (a sentinel names its tree; q is left as it was)
  HIP_TRY(hipMemcpy(g->q, g->train.out_q, sizeof(double) * G, hipMemcpyDeviceToDevice));
  g->stale = true;
  return 0;
}

int32_t mi_gp_sample_trees_device(mi_gp* g, void* stream, int32_t K, uint64_t seed, int64_t first_sample, int32_t* out_parent_ids,
                                  int32_t* out_entries, double* out_log_q, double* out_branch_lengths, double* out_cdf) {
  if (!g) return fail("null object");
  if (check_reserved(g, K, "mi_gp_sample_trees_device")) return 1;
  if (first_sample < 0) return fail("generalized pruning: first_sample must not be negative");
  return build_device(g, pick_stream(g->e, stream), K, 1, seed, first_sample, out_parent_ids, out_entries, out_log_q,
                      out_branch_lengths, out_cdf);
}
int32_t mi_gp_sample_trees(mi_gp* g, int32_t K, uint64_t seed, int64_t first_sample, int32_t* out_parent_ids, int32_t* out_entries,
                           double* out_log_q, double* out_branch_lengths, double* out_cdf) {
  if (!g) return fail("null object");
  if (first_sample < 0) return fail("generalized pruning: first_sample must not be negative");
  return build_host(g, K, 1, seed, first_sample, out_parent_ids, out_entries, out_log_q, out_branch_lengths, out_cdf);
}

int32_t mi_gp_enumerate_trees_device(mi_gp* g, void* stream, int64_t first, int32_t count, int32_t* out_parent_ids,
                                     int32_t* out_entries, double* out_log_q, double* out_branch_lengths) {
  if (!g) return fail("null object");
  if (check_reserved(g, count, "mi_gp_enumerate_trees_device")) return 1;
  if (check_enumeration(g, first, count)) return 1;
  return build_device(g, pick_stream(g->e, stream), count, 0, 0, first, out_parent_ids, out_entries, out_log_q, out_branch_lengths,
                      nullptr);
}
int32_t mi_gp_enumerate_trees(mi_gp* g, int64_t first, int32_t count, int32_t* out_parent_ids, int32_t* out_entries,
                              double* out_log_q, double* out_branch_lengths) {
  if (!g) return fail("null object");
  return build_host(g, count, 0, 0, first, out_parent_ids, out_entries, out_log_q, out_branch_lengths, nullptr);
}

// ---- de-rooting (any engine) ----
int32_t mi_engine_reserve_deroot(mi_engine* e, int32_t T, int32_t n) {
  if (!e) return fail("null engine");
  if (!e->shards.empty()) e = e->shards[0];
  if (T < 1) return fail("tree_count must be positive");
  if (n < 3) return fail("de-rooting needs at least 3 taxa");
  const size_t bytes = (((size_t)T + 63) / 64) * 64 * gp_tree_deroot_words(n) * 4;  // (the node words: what the device form checks)
  if (bytes > e->plv_budget)
    return fail("de-rooting " + std::to_string(T) + " trees of " + std::to_string(n) + " taxa takes " + std::to_string(bytes) +
                " bytes of workspace, over the budget of " + std::to_string(e->plv_budget) + " bytes (MI_PHYLO_PLV_BYTES)");
  HIP_TRY(hipSetDevice(e->spec.device));
  if (e->status.ensure(sizeof(int32_t) * kStatusWords)) return 1;
  if (bytes > e->deroot_ws.bytes) HIP_TRY(hipStreamSynchronize(e->stream));
  return e->deroot_ws.ensure(bytes);
}

int32_t mi_engine_deroot_trees_mapped_device(mi_engine* e, void* stream, int32_t T, int32_t n, const int32_t* parent_ids,
                                             const double* branch_lengths, int32_t* out_parent_ids, double* out_branch_lengths,
                                             int32_t* out_root_edge, int32_t* out_new_id) {
  if (!e) return fail("null engine");
  if (!e->shards.empty()) e = e->shards[0];
  if (T < 1) return fail("tree_count must be positive");
  if (n < 3) return fail("de-rooting needs at least 3 taxa");
  if (!parent_ids || !out_parent_ids || !out_root_edge) return fail("null tree arrays or output pointer");
  if (out_branch_lengths && !branch_lengths) return fail("de-rooting: out_branch_lengths without branch_lengths");
  const size_t words = (((size_t)T + 63) / 64) * 64 * gp_tree_deroot_words(n);
  if (words * 4 > e->deroot_ws.bytes)
    return fail("de-rooting " + std::to_string(T) + " trees of " + std::to_string(n) +
                " taxa before mi_engine_reserve_deroot reserved them (the device form allocates nothing)");
  HIP_TRY(hipSetDevice(e->spec.device));
  launch_gp_tree_deroot(T, n, parent_ids, branch_lengths, out_parent_ids, out_branch_lengths, out_root_edge, out_new_id,
                        e->deroot_ws.as<int32_t>(), e->status.as<int32_t>(), pick_stream(e, stream));
  HIP_TRY(hipGetLastError());
  e->dominant = "gp_tree_deroot_kernel";
  e->last_path = "deroot n=" + std::to_string(n) + " T=" + std::to_string(T);
  return 0;
}
int32_t mi_engine_deroot_trees_device(mi_engine* e, void* stream, int32_t T, int32_t n, const int32_t* parent_ids,
                                      const double* branch_lengths, int32_t* out_parent_ids, double* out_branch_lengths,
                                      int32_t* out_root_edge) {
  return mi_engine_deroot_trees_mapped_device(e, stream, T, n, parent_ids, branch_lengths, out_parent_ids, out_branch_lengths,
                                              out_root_edge, nullptr);
}

int32_t mi_engine_deroot_trees_mapped(mi_engine* e, int32_t T, int32_t n, const int32_t* parent_ids, const double* branch_lengths,
                                      int32_t* out_parent_ids, double* out_branch_lengths, int32_t* out_root_edge,
                                      int32_t* out_new_id) {
  if (!e) return fail("null engine");
  if (!e->shards.empty()) e = e->shards[0];
  if (!parent_ids || !out_parent_ids || !out_root_edge) return fail("null tree arrays or output pointer");
  if (out_branch_lengths && !branch_lengths) return fail("de-rooting: out_branch_lengths without branch_lengths");
  if (mi_engine_reserve_deroot(e, T, n)) return 1;
  const size_t N = 2 * (size_t)n - 1;
  HostCall c;
  c.in = {fixed(parent_ids, T * (N - 1)), fixed(branch_lengths, T * N)};
  c.out = {fixed(out_parent_ids, T * (N - 2)), fixed(out_branch_lengths, T * (N - 1)), fixed(out_root_edge, (size_t)T),
           fixed(out_new_id, T * N)};
  c.enqueue = [=](mi_engine* e, int, const HostArray* in, const HostArray* out) {
    return mi_engine_deroot_trees_mapped_device(e, e->stream, T, n, in[0].at<const int32_t>(), in[1].at<const double>(),
                                                out[0].at<int32_t>(), out[1].at<double>(), out[2].at<int32_t>(),
                                                out[3].at<int32_t>());
  };
  return run_on_engine(e, c);
}
int32_t mi_engine_deroot_trees(mi_engine* e, int32_t T, int32_t n, const int32_t* parent_ids, const double* branch_lengths,
                               int32_t* out_parent_ids, double* out_branch_lengths, int32_t* out_root_edge) {
  return mi_engine_deroot_trees_mapped(e, T, n, parent_ids, branch_lengths, out_parent_ids, out_branch_lengths, out_root_edge,
                                       nullptr);
}

}  // extern "C"
