// Split tables of tree batches: the table of distinct splits with the index of
// every branch into it (mi_engine_split_index*), Robinson-Foulds distances and squared branch
// scores from the indices (mi_engine_rf_distances*), their reservation, and the majority-rule
// consensus tree of a table (mi_consensus_tree: host arithmetic, no device is touched).  The
// device forms only enqueue.  Any engine serves: the taxon count is an argument and the
// alignment plays no part; a sharded handle lets its first shard do the work.
#include <cmath>

#include "mi_phylo_engine.h"

namespace {

// the occurrence workspace and the table, one block (mi_engine::split_ws)
struct SplitLayout {
  size_t O, slots, scan_bytes;
  size_t occ_bits, occ_hash, occ_slot, slot_owner, slot_first, slot_trees, scan_tmp, total;
};
size_t round256(size_t x) { return (x + 255) & ~(size_t)255; }
SplitLayout split_layout(int T, int n) {
  SplitLayout l{};
  l.O = (size_t)T * (2 * (size_t)n - 3);
  l.slots = split_table_slots(l.O);
  l.scan_bytes = split_scan_tmp_bytes(l.O);
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t here = at;
    at += round256(bytes);
    return here;
  };
  l.occ_bits = take(l.O * split_words(n) * 4);
  l.occ_hash = take(l.O * 8);
  l.occ_slot = take(l.O * 4);
  l.slot_owner = take(l.slots * 4);
  l.slot_first = take(l.slots * 4);
  l.slot_trees = take(l.slots * 4);
  l.scan_tmp = take(l.scan_bytes);
  l.total = at;
  return l;
}
size_t split_store_bytes(int T, int n) {
  return n <= kSplitLdsTaxa ? 0 : split_wave_count(T, n) * split_store_bytes_per_wave(n);
}
size_t split_sort_bytes(size_t O) { return round256(O * 4) * 4 + split_sort_tmp_bytes(O); }
size_t rf_ws_bytes(int T, int n) {
  const size_t TE = (size_t)T * (2 * (size_t)n - 3);
  return round256(TE * 8) + round256(TE * 4) + round256((size_t)T * 4);
}

int check_split_shape(const mi_engine* e, int T, int n) {
  if (!e) return fail("null engine");
  if (T < 1) return fail("tree_count must be positive");
  if (n < 3) return fail("split tables need at least 3 taxa");
  // (occurrence numbers and table slots are 32-bit)
  if ((size_t)T * (2 * (size_t)n - 3) >= ((size_t)1 << 30))
    return fail("split index: tree_count (2 taxon_count - 3) must stay below 2^30");
  return 0;
}

// The split table is not chunked: a batch whose workspace is over the arena budget is refused.
int reserve_split_index(mi_engine* e, int T, int n, bool stats) {
  const SplitLayout l = split_layout(T, n);
  const size_t store = split_store_bytes(T, n), sort = stats ? split_sort_bytes(l.O) : 0;
  if (l.total + store + sort > e->plv_budget)
    return fail("split index: " + std::to_string(T) + " trees of " + std::to_string(n) + " taxa need " +
                std::to_string(l.total + store + sort) + " bytes of workspace (" + std::to_string(l.O) +
                " occurrences), over the budget of " + std::to_string(e->plv_budget) +
                " bytes (MI_PHYLO_PLV_BYTES); the call is not chunked: index the batch in parts");
  if (e->split_ws.ensure(l.total)) return 1;
  if (store && e->split_store.ensure(store)) return 1;
  if (sort && e->split_sort.ensure(sort)) return 1;
  return e->status.ensure(sizeof(int32_t) * kStatusWords);
}

int check_rf_shape(const mi_engine* e, int T, int n) {
  if (!e) return fail("null engine");
  if (T < 1) return fail("tree_count must be positive");
  if (n < 3) return fail("split tables need at least 3 taxa");
  if (n > kRfMaxTaxa)
    return fail("RF distances: at most " + std::to_string(kRfMaxTaxa) + " taxa (a tree's sorted index list is kept in LDS)");
  if ((size_t)T * T >= ((size_t)1 << 31)) return fail("RF distances: tree_count^2 must stay below 2^31");
  return 0;
}

}  // namespace

int run_split_index_device(mi_engine* e, hipStream_t s, const SplitIndexCall& c) {
  if (check_split_shape(e, c.T, c.n)) return 1;
  HIP_TRY(hipSetDevice(e->spec.device));
  if (!c.parent_ids) return fail("null tree arrays");
  if (c.capacity < 0) return fail("split_capacity must not be negative");
  if (!c.out_index || !c.out_count) return fail("null output pointer");
  if (c.capacity > 0 && (!c.out_bits || !c.out_first || !c.out_trees)) return fail("null output pointer");
  if (reserve_split_index(e, c.T, c.n, c.out_stats != nullptr)) return 1;
  const SplitLayout l = split_layout(c.T, c.n);
  char* ws = e->split_ws.as<char>();
  SplitArgs a{};
  a.n = c.n;
  a.T = c.T;
  a.W = split_words(c.n);
  a.capacity = c.capacity;
  a.hash_bits = e->sw.split_hash_bits;
  a.slots = (uint32_t)l.slots;
  a.parent_ids = c.parent_ids;
  a.bl = c.bl;
  a.weights = c.weights;
  a.status = e->status.as<int32_t>();
  a.store = e->split_store.as<uint32_t>();
  a.occ_bits = reinterpret_cast<uint32_t*>(ws + l.occ_bits);
  a.occ_hash = reinterpret_cast<uint64_t*>(ws + l.occ_hash);
  a.occ_slot = reinterpret_cast<int32_t*>(ws + l.occ_slot);
  a.slot_owner = reinterpret_cast<int32_t*>(ws + l.slot_owner);
  a.slot_first = reinterpret_cast<int32_t*>(ws + l.slot_first);
  a.slot_trees = reinterpret_cast<int32_t*>(ws + l.slot_trees);
  a.scan_tmp = ws + l.scan_tmp;
  a.scan_tmp_bytes = l.scan_bytes;
  if (c.out_stats) {
    char* sort = e->split_sort.as<char>();
    const size_t col = round256(l.O * 4);
    a.keys = reinterpret_cast<uint32_t*>(sort);
    a.vals = reinterpret_cast<uint32_t*>(sort + col);
    a.keys2 = reinterpret_cast<uint32_t*>(sort + 2 * col);
    a.vals2 = reinterpret_cast<uint32_t*>(sort + 3 * col);
    a.sort_tmp = sort + 4 * col;
    a.sort_tmp_bytes = split_sort_tmp_bytes(l.O);
  }
  a.out_index = c.out_index;
  a.out_count = c.out_count;
  a.out_bits = c.out_bits;
  a.out_first = c.out_first;
  a.out_trees = c.out_trees;
  a.out_stats = c.out_stats;
  if (launch_split_index(a, s)) return fail("split index: the scan or the sort could not be enqueued");
  HIP_TRY(hipGetLastError());
  e->dominant = "tree_splits_kernel";
  e->last_walk_launches = 1;
  e->last_evals = c.T;
  e->last_grad_evals = 0;
  e->last_path = "splits n=" + std::to_string(c.n) + " W=" + std::to_string(a.W) +
                 (c.n <= kSplitLdsTaxa ? " store=lds" : " store=global");
  return 0;
}

int run_rf_device(mi_engine* e, hipStream_t s, int T, int n, const int32_t* split_index, const double* bl,
                  int32_t* out_rf, double* out_bs) {
  if (check_rf_shape(e, T, n)) return 1;
  HIP_TRY(hipSetDevice(e->spec.device));
  if (!split_index) return fail("null split index");
  if (!out_rf) return fail("null output pointer");
  if (out_bs && !bl) return fail("RF distances: the branch score needs branch lengths");
  if (e->rf_ws.ensure(rf_ws_bytes(T, n))) return 1;
  const size_t TE = (size_t)T * (2 * (size_t)n - 3);
  char* ws = e->rf_ws.as<char>();
  RfArgs a{};
  a.n = n;
  a.T = T;
  a.split_index = split_index;
  a.bl = bl;
  a.sorted_length = reinterpret_cast<double*>(ws);
  a.sorted_index = reinterpret_cast<int32_t*>(ws + round256(TE * 8));
  a.sorted_count = reinterpret_cast<int32_t*>(ws + round256(TE * 8) + round256(TE * 4));
  a.out_rf = out_rf;
  a.out_bs = out_bs;
  launch_rf(a, s);
  HIP_TRY(hipGetLastError());
  e->dominant = "rf_pairs_kernel";
  e->last_walk_launches = 1;
  e->last_evals = T;
  e->last_grad_evals = 0;
  e->last_path = "rf n=" + std::to_string(n) + " T=" + std::to_string(T);
  return 0;
}

extern "C" {

int32_t mi_engine_split_index_device(mi_engine* e, void* stream, int32_t T, int32_t n, const int32_t* parent_ids,
                                     const double* bl, const double* tree_weights, int32_t capacity,
                                     int32_t* out_index, int32_t* out_count, uint32_t* out_bits, int32_t* out_first,
                                     int32_t* out_trees, double* out_stats) {
  if (!e) return fail("null engine");
  if (!e->shards.empty()) return fail(kShardedDeviceCall);
  SplitIndexCall c;
  c.T = T;
  c.n = n;
  c.capacity = capacity;
  c.parent_ids = parent_ids;
  c.bl = bl;
  c.weights = tree_weights;
  c.out_index = out_index;
  c.out_count = out_count;
  c.out_bits = out_bits;
  c.out_first = out_first;
  c.out_trees = out_trees;
  c.out_stats = out_stats;
  return run_split_index_device(e, pick_stream(e, stream), c);
}

// The host form: arrays of fixed counts, no retry.  The table rows come down whole into arrays of
// the call's own and the first S of them are handed on: the caller's rows at and above S stay.
int32_t mi_engine_split_index(mi_engine* e, int32_t T, int32_t n, const int32_t* parent_ids, const double* bl,
                              const double* tree_weights, int32_t capacity, int32_t* out_index, int32_t* out_count,
                              uint32_t* out_bits, int32_t* out_first, int32_t* out_trees, double* out_stats) {
  if (check_split_shape(e, T, n)) return 1;
  e = first_engine(e);
  if (!parent_ids) return fail("null tree arrays");
  if (capacity < 0) return fail("split_capacity must not be negative");
  if (!out_index || !out_count) return fail("null output pointer");
  if (capacity > 0 && (!out_bits || !out_first || !out_trees)) return fail("null output pointer");
  const size_t E = 2 * (size_t)n - 3, W = split_words(n), cap = capacity;
  std::vector<uint32_t> bits(cap * W);
  std::vector<int32_t> first(cap), trees(cap);
  std::vector<double> stats(out_stats ? cap * 3 : 0);
  int32_t S = 0;
  HostCall c;
  c.in = {fixed(parent_ids, (size_t)T * E), fixed(bl, (size_t)T * (E + 1)), fixed(tree_weights, T)};
  c.out = {fixed(out_index, (size_t)T * (E + 2)), fixed(&S, 1), fixed(cap ? bits.data() : nullptr, cap * W),
           fixed(cap ? first.data() : nullptr, cap), fixed(cap ? trees.data() : nullptr, cap),
           fixed(out_stats && cap ? stats.data() : nullptr, cap * 3)};
  c.enqueue = [=](mi_engine* e, int, const HostArray* in, const HostArray* out) {
    SplitIndexCall d;
    d.T = T;
    d.n = n;
    d.capacity = capacity;
    d.parent_ids = in[0].at<const int32_t>();
    d.bl = in[1].at<const double>();
    d.weights = in[2].at<const double>();
    d.out_index = out[0].at<int32_t>();
    d.out_count = out[1].at<int32_t>();
    d.out_bits = out[2].at<uint32_t>();
    d.out_first = out[3].at<int32_t>();
    d.out_trees = out[4].at<int32_t>();
    d.out_stats = out[5].at<double>();
    return run_split_index_device(e, e->stream, d);
  };
  if (run_on_engine(e, c)) return 1;
  *out_count = S;
  const size_t rows = std::min<size_t>(S, cap);
  if (rows) {
    memcpy(out_bits, bits.data(), rows * W * 4);
    memcpy(out_first, first.data(), rows * 4);
    memcpy(out_trees, trees.data(), rows * 4);
    if (out_stats) memcpy(out_stats, stats.data(), rows * 3 * 8);
  }
  return 0;
}

int32_t mi_engine_rf_distances_device(mi_engine* e, void* stream, int32_t T, int32_t n, const int32_t* split_index,
                                      const double* bl, int32_t* out_rf, double* out_bs) {
  if (!e) return fail("null engine");
  if (!e->shards.empty()) return fail(kShardedDeviceCall);
  return run_rf_device(e, pick_stream(e, stream), T, n, split_index, bl, out_rf, out_bs);
}

int32_t mi_engine_rf_distances(mi_engine* e, int32_t T, int32_t n, const int32_t* split_index, const double* bl,
                               int32_t* out_rf, double* out_bs) {
  if (check_rf_shape(e, T, n)) return 1;
  if (!split_index) return fail("null split index");
  if (!out_rf) return fail("null output pointer");
  if (out_bs && !bl) return fail("RF distances: the branch score needs branch lengths");
  const size_t E = 2 * (size_t)n - 3;
  HostCall c;
  c.in = {fixed(split_index, (size_t)T * (E + 2)), fixed(bl, (size_t)T * (E + 1))};
  c.out = {fixed(out_rf, (size_t)T * T), fixed(out_bs, (size_t)T * T)};
  c.enqueue = [=](mi_engine* e, int, const HostArray* in, const HostArray* out) {
    return run_rf_device(e, e->stream, T, n, in[0].at<const int32_t>(), in[1].at<const double>(),
                         out[0].at<int32_t>(), out[1].at<double>());
  };
  return run_on_engine(first_engine(e), c);
}

int32_t mi_engine_reserve_splits(mi_engine* e, int32_t T, int32_t n) {
  if (check_split_shape(e, T, n)) return 1;
  e = first_engine(e);
  HIP_TRY(hipSetDevice(e->spec.device));
  if (reserve_split_index(e, T, n, true)) return 1;
  if (n <= kRfMaxTaxa && (size_t)T * T < ((size_t)1 << 31) && e->rf_ws.ensure(rf_ws_bytes(T, n))) return 1;
  return 0;
}

// The majority-rule consensus of a split table.  Sets that never hold taxon 0 are pairwise
// compatible exactly when they are nested or disjoint, so the kept sets form a forest under
// inclusion; leaf 0, the maximal sets and the leaves none of them covers hang under the root.
int32_t mi_consensus_tree(int32_t n, int32_t S, const uint32_t* split_bits, const double* weight,
                          double total_weight, double threshold, int32_t* out_node_count, int32_t* out_parent_ids,
                          int32_t* out_node_split) {
  if (n < 3 || S < 0 || (S > 0 && (!split_bits || !weight)) || !out_node_count || !out_parent_ids || !out_node_split)
    return fail("mi_consensus_tree: bad arguments");
  if (!(threshold >= 0.5 && threshold < 1.0))
    return fail("mi_consensus_tree: threshold must be in [0.5, 1): only a strict majority makes the kept splits "
                "pairwise compatible");
  const int W = split_words(n);
  auto row = [&](int i) { return split_bits + (size_t)i * W; };
  auto size_of = [&](int i) {
    int c = 0;
    for (int k = 0; k < W; k++) c += __builtin_popcount(row(i)[k]);
    return c;
  };
  auto has = [&](int i, int leaf) { return (row(i)[leaf >> 5] >> (leaf & 31)) & 1u; };
  std::vector<int32_t> leaf_split(n, -1), kept, kept_size;
  for (int i = 0; i < S; i++) {
    const int c = size_of(i);
    if (has(i, 0) || c < 1 || c > n - 1 || (n & 31 && (row(i)[W - 1] >> (n & 31)) != 0))
      return fail("mi_consensus_tree: split " + std::to_string(i) + " is not a minorised split of " +
                  std::to_string(n) + " taxa");
    if (c == n - 1) leaf_split[0] = i;
    else if (c == 1) {
      for (int v = 1; v < n; v++)
        if (has(i, v)) leaf_split[v] = i;
    } else if (weight[i] > threshold * total_weight) {
      kept.push_back(i);
      kept_size.push_back(c);
    }
  }
  // ascending size (the table's order among equals): a set's parent is the first later superset
  std::vector<int> order(kept.size());
  for (size_t k = 0; k < order.size(); k++) order[k] = (int)k;
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return kept_size[x] < kept_size[y]; });
  const int K = (int)kept.size(), root = n + K;  // working ids: leaves, kept sets in `order`, the root
  for (int x = 0; x < K; x++)
    for (int y = x + 1; y < K; y++) {
      bool meet = false, x_in_y = true;
      for (int k = 0; k < W; k++) {
        const uint32_t bx = row(kept[order[x]])[k], by = row(kept[order[y]])[k];
        meet = meet || (bx & by);
        x_in_y = x_in_y && !(bx & ~by);
      }
      if (meet && (!x_in_y || kept_size[order[x]] == kept_size[order[y]]))
        return fail("mi_consensus_tree: splits " + std::to_string(kept[order[x]]) + " and " +
                    std::to_string(kept[order[y]]) + " are equal or incompatible");
    }
  std::vector<int32_t> par(root + 1, root), maxleaf(root + 1, -1);
  std::vector<std::vector<int32_t>> kids(root + 1);
  for (int v = 1; v < n; v++)
    for (int x = 0; x < K; x++)
      if (has(kept[order[x]], v)) {
        par[v] = n + x;
        break;
      }
  for (int x = 0; x < K; x++)
    for (int y = x + 1; y < K; y++) {
      bool inside = true;
      for (int k = 0; k < W && inside; k++) inside = !(row(kept[order[x]])[k] & ~row(kept[order[y]])[k]);
      if (inside) {
        par[n + x] = n + y;
        break;
      }
    }
  // (a working id is above its children's: one upward pass gives the largest leaf ids)
  for (int v = 0; v < root; v++) {
    if (v < n) maxleaf[v] = v;
    kids[par[v]].push_back(v);
    maxleaf[par[v]] = std::max(maxleaf[par[v]], maxleaf[v]);
  }
  for (int v = n; v <= root; v++)
    std::sort(kids[v].begin(), kids[v].end(), [&](int32_t x, int32_t y) { return maxleaf[x] < maxleaf[y]; });
  // leaves keep their ids, internal nodes in post-order with the children by largest leaf id
  std::vector<int32_t> new_id(root + 1, -1);
  int32_t next = n;
  std::vector<std::pair<int32_t, size_t>> walk{{root, 0}};
  while (!walk.empty()) {
    const int32_t v = walk.back().first;
    const size_t done = walk.back().second;
    if (v < n) {
      new_id[v] = v;
      walk.pop_back();
    } else if (done < kids[v].size()) {
      walk.back().second++;
      walk.push_back({kids[v][done], 0});
    } else {
      new_id[v] = next++;
      walk.pop_back();
    }
  }
  *out_node_count = root + 1;
  for (int v = 0; v < root; v++) out_parent_ids[new_id[v]] = new_id[par[v]];
  for (int v = 0; v < n; v++) out_node_split[v] = leaf_split[v];
  for (int x = 0; x < K; x++) out_node_split[new_id[n + x]] = kept[order[x]];
  out_node_split[root] = -1;
  return 0;
}

}  // extern "C"
