// Subsplit Bayesian networks: the support of a tree batch with every tree's slots
// (mi_engine_sbn_index*), the probabilities of all rootings with the expected usages
// (mi_engine_sbn_log_prob*), the segmented log-normalisation (mi_engine_sbn_normalize*),
// simple-average and EM training (mi_engine_sbn_train*), the descent table, the sampler and the
// topology gradient (mi_engine_sbn_{descent,sample,topology_gradient}*) and their
// reservation.  The device forms
// of the first three only enqueue; training reads one double per iteration and synchronises.  Any
// engine serves: the taxon count is an argument and the alignment plays no part; a sharded handle
// lets its first shard do the work.
#include <cmath>

#include "mi_phylo_engine.h"

namespace {

size_t round256(size_t x) { return (x + 255) & ~(size_t)255; }

struct Taker {
  size_t at = 0;
  size_t operator()(size_t bytes) {
    const size_t here = at;
    at += round256(bytes);
    return here;
  }
};

// the index call's block (mi_engine::sbn_index_ws): the batch's split table, then the PCSP occurrences
struct IndexLayout {
  size_t O1, O, slots, sort_bytes, scan_bytes;
  size_t split_index, split_count, split_bits, split_first, split_trees;
  size_t counts, occ_key, occ_slot, occ_pslot, slot_owner, slot_first, pslot_owner, pslot_first;
  size_t keys, keys2, vals, vals2, heads, head_scan, rank_of, sort_tmp, scan_tmp, total;
};
IndexLayout index_layout(int T, int n) {
  IndexLayout l{};
  const size_t E = 2 * (size_t)n - 3;
  l.O1 = (size_t)T * E;
  l.O = l.O1 * 6;
  l.slots = split_table_slots(l.O);
  l.sort_bytes = sbn_index_sort_tmp_bytes(l.O);
  l.scan_bytes = sbn_index_scan_tmp_bytes(l.O);
  Taker take;
  l.split_index = take((size_t)T * (E + 2) * 4);
  l.split_count = take(4);
  l.split_bits = take(l.O1 * split_words(n) * 4);
  l.split_first = take(l.O1 * 4);
  l.split_trees = take(l.O1 * 4);
  l.counts = take(16);
  l.occ_key = take(l.O * 12);
  l.occ_slot = take(l.O * 4);
  l.occ_pslot = take(l.O * 4);
  l.slot_owner = take(l.slots * 4);
  l.slot_first = take(l.slots * 4);
  l.pslot_owner = take(l.slots * 4);
  l.pslot_first = take(l.slots * 4);
  l.keys = take(l.O * 8);
  l.keys2 = take(l.O * 8);
  l.vals = take(l.O * 4);
  l.vals2 = take(l.O * 4);
  l.heads = take(l.O * 4);
  l.head_scan = take(l.O * 4);
  l.rank_of = take(l.O * 4);
  l.sort_tmp = take(l.sort_bytes);
  l.scan_tmp = take(l.scan_bytes);
  l.total = take.at;
  return l;
}

// the block of log_prob, normalize and train (mi_engine::sbn_prob_ws)
struct ProbLayout {
  size_t Q, sort_bytes;
  size_t theta, usage, keys, keys2, vals, vals2, sort_tmp;
  size_t log_m_tilde, log_m_bar, log_q, rooting, total;  // (training)
};
ProbLayout prob_layout(int T, int n, size_t P) {
  ProbLayout l{};
  const size_t E = 2 * (size_t)n - 3;
  l.Q = (size_t)T * E * 7;
  l.sort_bytes = sbn_prob_sort_tmp_bytes(l.Q, 0x7ffffffe);  // (room for keys of any width)
  Taker take;
  l.theta = take(P * 8);
  l.usage = take(l.Q * 8);
  l.keys = take(l.Q * 4);
  l.keys2 = take(l.Q * 4);
  l.vals = take(l.Q * 4);
  l.vals2 = take(l.Q * 4);
  l.sort_tmp = take(l.sort_bytes);
  l.log_m_tilde = take(P * 8);
  l.log_m_bar = take(P * 8);
  l.log_q = take((size_t)T * 8);
  l.rooting = take((size_t)T * E * 8);
  l.total = take.at;
  return l;
}

int sbn_tpw(const mi_engine* e) { return e->sw.sbn_trees_per_wave; }
size_t sbn_store_bytes(const mi_engine* e, int T, int n) {
  const int tpw = sbn_tpw(e);
  return n <= sbn_lds_taxa(tpw) ? 0 : sbn_wave_count(T, tpw) * sbn_store_bytes_per_wave(n, tpw);
}

int check_sbn_shape(const mi_engine* e, int T, int n) {
  if (!e) return fail("null engine");
  if (T < 1) return fail("tree_count must be positive");
  if (n < 3) return fail("subsplit Bayesian networks need at least 3 taxa");
  // (occurrence and entry numbers are 32-bit)
  if ((size_t)T * (2 * (size_t)n - 3) * 7 >= ((size_t)1 << 30))
    return fail("SBN: 7 tree_count (2 taxon_count - 3) must stay below 2^30");
  return 0;
}

std::string sizes(int T, int n, size_t bytes, const mi_engine* e) {
  return std::to_string(T) + " trees of " + std::to_string(n) + " taxa need " + std::to_string(bytes) +
         " bytes of workspace, over the budget of " + std::to_string(e->plv_budget) +
         " bytes (MI_PHYLO_PLV_BYTES); the call is not chunked: pass the batch in parts";
}

int reserve_sbn_index(mi_engine* e, int T, int n) {
  const IndexLayout l = index_layout(T, n);
  const size_t store = sbn_store_bytes(e, T, n);
  if (l.total + store > e->plv_budget) return fail("SBN index: " + sizes(T, n, l.total + store, e));
  if (e->sbn_index_ws.ensure(l.total)) return 1;
  if (store && e->sbn_store.ensure(store)) return 1;
  return e->status.ensure(sizeof(int32_t) * kStatusWords);
}

// the parameter count a reservation without a support allows for: every entry of every tree its own
size_t reserved_params(int T, int n) { return (size_t)T * (2 * (size_t)n - 3) * 7; }
// The block is laid out for the larger of the call's parameter count and the reservation's, so a
// reserved call finds its block in place.
ProbLayout call_layout(int T, int n, int P) {
  return prob_layout(T, n, std::max<size_t>((size_t)P, reserved_params(T, n)));
}

int reserve_sbn_prob(mi_engine* e, int T, int n, int P) {
  const ProbLayout l = call_layout(T, n, P);
  const size_t store = sbn_store_bytes(e, T, n);
  if (l.total + store > e->plv_budget) return fail("SBN: " + sizes(T, n, l.total + store, e));
  if (e->sbn_prob_ws.ensure(l.total)) return 1;
  if (store && e->sbn_store.ensure(store)) return 1;
  return e->status.ensure(sizeof(int32_t) * kStatusWords);
}
void note_call(mi_engine* e, const char* kernel, int T, int n) {
  e->dominant = kernel;
  e->last_walk_launches = 1;
  e->last_evals = T;
  e->last_grad_evals = 0;
  e->last_path = "sbn n=" + std::to_string(n) + (n <= sbn_lds_taxa(sbn_tpw(e)) ? " store=lds" : " store=global");
}

struct SbnIndexCall {
  int T = 0, n = 0, T0 = 0, root_capacity = 0, pcsp_capacity = 0;
  const int32_t* parent_ids = nullptr;
  int32_t *out_root_index = nullptr, *out_slot_index = nullptr, *out_counts = nullptr;
  uint32_t* out_split_bits = nullptr;
  int32_t *out_pcsp_clades = nullptr, *out_parent_range = nullptr, *out_pcsp_parent = nullptr;
};

int check_index_call(const mi_engine* e, const SbnIndexCall& c) {
  if (check_sbn_shape(e, c.T, c.n)) return 1;
  if (c.T0 < 1 || c.T0 > c.T) return fail("SBN index: support_tree_count must be in [1, tree_count]");
  if (c.root_capacity < 0 || c.pcsp_capacity < 0) return fail("SBN index: a capacity must not be negative");
  if (!c.parent_ids) return fail("null tree arrays");
  if (!c.out_root_index || !c.out_slot_index || !c.out_counts) return fail("null output pointer");
  if (c.root_capacity > 0 && !c.out_split_bits) return fail("null output pointer");
  if (c.pcsp_capacity > 0 && (!c.out_pcsp_clades || !c.out_parent_range || !c.out_pcsp_parent))
    return fail("null output pointer");
  return 0;
}

int run_sbn_index_device(mi_engine* e, hipStream_t s, const SbnIndexCall& c) {
  if (check_index_call(e, c)) return 1;
  HIP_TRY(hipSetDevice(e->spec.device));
  if (reserve_sbn_index(e, c.T, c.n)) return 1;
  const IndexLayout l = index_layout(c.T, c.n);
  char* ws = e->sbn_index_ws.as<char>();
  // the split table of the whole batch: every clade gets its name 2 split + side
  SplitIndexCall sc;
  sc.T = c.T;
  sc.n = c.n;
  sc.capacity = (int)l.O1;
  sc.parent_ids = c.parent_ids;
  sc.out_index = reinterpret_cast<int32_t*>(ws + l.split_index);
  sc.out_count = reinterpret_cast<int32_t*>(ws + l.split_count);
  sc.out_bits = reinterpret_cast<uint32_t*>(ws + l.split_bits);
  sc.out_first = reinterpret_cast<int32_t*>(ws + l.split_first);
  sc.out_trees = reinterpret_cast<int32_t*>(ws + l.split_trees);
  if (run_split_index_device(e, s, sc)) return 1;
  SbnIndexArgs a{};
  a.n = c.n;
  a.T = c.T;
  a.T0 = c.T0;
  a.W = split_words(c.n);
  a.tpw = sbn_tpw(e);
  a.root_capacity = c.root_capacity;
  a.pcsp_capacity = c.pcsp_capacity;
  a.hash_bits = e->sw.split_hash_bits;
  a.slots = (uint32_t)l.slots;
  a.parent_ids = c.parent_ids;
  a.status = e->status.as<int32_t>();
  a.store = e->sbn_store.as<char>();
  a.split_index = sc.out_index;
  a.split_first = sc.out_first;
  a.split_count = sc.out_count;
  a.split_bits = sc.out_bits;
  a.counts = reinterpret_cast<int32_t*>(ws + l.counts);
  a.occ_key = reinterpret_cast<int32_t*>(ws + l.occ_key);
  a.occ_slot = reinterpret_cast<int32_t*>(ws + l.occ_slot);
  a.occ_pslot = reinterpret_cast<int32_t*>(ws + l.occ_pslot);
  a.slot_owner = reinterpret_cast<int32_t*>(ws + l.slot_owner);
  a.slot_first = reinterpret_cast<int32_t*>(ws + l.slot_first);
  a.pslot_owner = reinterpret_cast<int32_t*>(ws + l.pslot_owner);
  a.pslot_first = reinterpret_cast<int32_t*>(ws + l.pslot_first);
  a.keys = reinterpret_cast<uint64_t*>(ws + l.keys);
  a.keys2 = reinterpret_cast<uint64_t*>(ws + l.keys2);
  a.vals = reinterpret_cast<uint32_t*>(ws + l.vals);
  a.vals2 = reinterpret_cast<uint32_t*>(ws + l.vals2);
  a.heads = reinterpret_cast<uint32_t*>(ws + l.heads);
  a.head_scan = reinterpret_cast<uint32_t*>(ws + l.head_scan);
  a.rank_of = reinterpret_cast<int32_t*>(ws + l.rank_of);
  a.sort_tmp = ws + l.sort_tmp;
  a.scan_tmp = ws + l.scan_tmp;
  a.sort_tmp_bytes = l.sort_bytes;
  a.scan_tmp_bytes = l.scan_bytes;
  a.out_root_index = c.out_root_index;
  a.out_slot_index = c.out_slot_index;
  a.out_counts = c.out_counts;
  a.out_split_bits = c.out_split_bits;
  a.out_pcsp_clades = c.out_pcsp_clades;
  a.out_parent_range = c.out_parent_range;
  a.out_pcsp_parent = c.out_pcsp_parent;
  if (launch_sbn_index(a, s)) return fail("SBN index: the sort or the scan could not be enqueued");
  HIP_TRY(hipGetLastError());
  note_call(e, "sbn_keys_kernel", c.T, c.n);
  return 0;
}

struct SbnProbCall {
  int T = 0, n = 0, S = 0, C = 0, parents = 0;
  bool normalized = false;
  const int32_t *parent_ids = nullptr, *root_index = nullptr, *slot_index = nullptr, *parent_range = nullptr;
  const double *log_params = nullptr, *weights = nullptr;
  double *out_rooting = nullptr, *out_log_q = nullptr, *out_counts = nullptr;
};

int check_support(int S, int C, int parents, const void* parent_range) {
  if (S < 1 || C < 0 || parents < 0 || parents > C) return fail("SBN: bad rootsplit, PCSP or parent count");
  if (parents > 0 && !parent_range) return fail("SBN: null parent_range");
  return 0;
}

int check_prob_call(const mi_engine* e, const SbnProbCall& c) {
  if (check_sbn_shape(e, c.T, c.n)) return 1;
  if (check_support(c.S, c.C, c.parents, c.parent_range)) return 1;
  if (!c.parent_ids || !c.root_index || !c.slot_index) return fail("null tree arrays");
  if (!c.log_params) return fail("null parameter vector");
  if (!c.out_rooting || !c.out_log_q) return fail("null output pointer");
  return 0;
}

SbnProbArgs prob_args(mi_engine* e, const SbnProbCall& c, const ProbLayout& l) {
  char* ws = e->sbn_prob_ws.as<char>();
  SbnProbArgs a{};
  a.n = c.n;
  a.T = c.T;
  a.tpw = sbn_tpw(e);
  a.P = c.S + c.C;
  a.parent_ids = c.parent_ids;
  a.root_index = c.root_index;
  a.slot_index = c.slot_index;
  a.weights = c.weights;
  a.status = e->status.as<int32_t>();
  a.store = e->sbn_store.as<char>();
  a.usage = reinterpret_cast<double*>(ws + l.usage);
  a.keys = reinterpret_cast<uint32_t*>(ws + l.keys);
  a.keys2 = reinterpret_cast<uint32_t*>(ws + l.keys2);
  a.vals = reinterpret_cast<uint32_t*>(ws + l.vals);
  a.vals2 = reinterpret_cast<uint32_t*>(ws + l.vals2);
  a.sort_tmp = ws + l.sort_tmp;
  a.sort_tmp_bytes = l.sort_bytes;
  return a;
}

int run_sbn_log_prob_device(mi_engine* e, hipStream_t s, const SbnProbCall& c) {
  if (check_prob_call(e, c)) return 1;
  HIP_TRY(hipSetDevice(e->spec.device));
  const int P = c.S + c.C;
  const ProbLayout l = call_layout(c.T, c.n, P);
  if (reserve_sbn_prob(e, c.T, c.n, P)) return 1;
  SbnProbArgs a = prob_args(e, c, l);
  launch_sbn_check_params(P, c.log_params, a.status, s);
  double* theta = reinterpret_cast<double*>(e->sbn_prob_ws.as<char>() + l.theta);
  if (!c.normalized) launch_sbn_normalize(c.S, c.parents, c.parent_range, c.log_params, theta, s);
  a.theta = c.normalized ? c.log_params : theta;
  a.out_rooting = c.out_rooting;
  a.out_log_q = c.out_log_q;
  a.out_counts = c.out_counts;
  if (!c.out_counts) a.usage = nullptr;
  if (launch_sbn_log_prob(a, s)) return fail("SBN log_prob: the sort could not be enqueued");
  HIP_TRY(hipGetLastError());
  note_call(e, "sbn_walk_kernel", c.T, c.n);
  return 0;
}

int run_sbn_normalize_device(mi_engine* e, hipStream_t s, int S, int C, int parents, const int32_t* parent_range,
                             const double* in, double* out) {
  if (!e) return fail("null engine");
  if (check_support(S, C, parents, parent_range)) return 1;
  if (!in || !out) return fail("null parameter vector");
  HIP_TRY(hipSetDevice(e->spec.device));
  if (e->status.ensure(sizeof(int32_t) * kStatusWords)) return 1;
  launch_sbn_check_params(S + C, in, e->status.as<int32_t>(), s);
  launch_sbn_normalize(S, parents, parent_range, in, out, s);
  HIP_TRY(hipGetLastError());
  e->dominant = "sbn_normalize_kernel";
  e->last_walk_launches = 1;
  e->last_evals = e->last_grad_evals = 0;
  e->last_path = "sbn normalize blocks=" + std::to_string(parents + 1);
  return 0;
}

struct SbnTrainCall {
  SbnProbCall p;  // (log_params, normalized and the outputs unused)
  int method = 0, max_iter = 0;
  double alpha = 0.0, score_epsilon = 0.0;
  double *out_log_params = nullptr, *out_history = nullptr;
  int32_t* out_iterations = nullptr;
};

int check_train_call(const mi_engine* e, const SbnTrainCall& c) {
  if (check_sbn_shape(e, c.p.T, c.p.n)) return 1;
  if (check_support(c.p.S, c.p.C, c.p.parents, c.p.parent_range)) return 1;
  if (!c.p.parent_ids || !c.p.root_index || !c.p.slot_index) return fail("null tree arrays");
  if (c.method != MI_SBN_SA && c.method != MI_SBN_EM) return fail("SBN training: method must be MI_SBN_SA or MI_SBN_EM");
  if (!(c.alpha >= 0.0) || std::isinf(c.alpha)) return fail("SBN training: alpha must be finite and not negative");
  if (c.max_iter < 0) return fail("SBN training: max_iter must not be negative");
  if (!(c.score_epsilon >= 0.0)) return fail("SBN training: score_epsilon must not be negative");
  if (!c.out_log_params || !c.out_iterations) return fail("null output pointer");
  if (c.method == MI_SBN_EM && c.max_iter > 0 && !c.out_history) return fail("null output pointer");
  return 0;
}

// Simple average: the log counts of the rho = 1 usage, normalised.  EM as the reference's
// ExpectationMaximization (src/sbn_probability.cpp:214-329), one double read per iteration.
int run_sbn_train_device(mi_engine* e, hipStream_t s, const SbnTrainCall& c) {
  if (check_train_call(e, c)) return 1;
  HIP_TRY(hipSetDevice(e->spec.device));
  const int T = c.p.T, n = c.p.n, P = c.p.S + c.p.C, E = 2 * n - 3;
  const ProbLayout l = call_layout(T, n, P);
  if (reserve_sbn_prob(e, T, n, P)) return 1;
  char* ws = e->sbn_prob_ws.as<char>();
  double* log_m_tilde = reinterpret_cast<double*>(ws + l.log_m_tilde);
  double* log_m_bar = reinterpret_cast<double*>(ws + l.log_m_bar);
  double* log_q = reinterpret_cast<double*>(ws + l.log_q);
  double* rooting = reinterpret_cast<double*>(ws + l.rooting);
  double* theta = c.out_log_params;
  SbnProbArgs a = prob_args(e, c.p, l);
  a.out_rooting = rooting;
  a.out_log_q = log_q;
  // the counts: every rooting with weight 1; a tree outside the support is an error
  a.uniform = 1;
  a.require_support = 1;
  a.theta = nullptr;
  a.out_counts = log_m_tilde;
  if (launch_sbn_log_prob(a, s)) return fail("SBN training: the sort could not be enqueued");
  int32_t iterations = 0;
  if (c.method == MI_SBN_EM && c.max_iter > 0) HIP_TRY(hipMemsetAsync(c.out_history, 0, sizeof(double) * c.max_iter, s));
  if (c.method == MI_SBN_SA) {
    launch_sbn_normalize(c.p.S, c.p.parents, c.p.parent_range, log_m_tilde, theta, s);
  } else {
    // m~ = counts / E, normalised: the starting point; with alpha > 0, log(alpha m~) from here on
    launch_sbn_combine(P, log_m_tilde, nullptr, -std::log((double)E), log_m_tilde, s);
    launch_sbn_normalize(c.p.S, c.p.parents, c.p.parent_range, log_m_tilde, theta, s);
    if (c.alpha > 0.0) launch_sbn_combine(P, log_m_tilde, nullptr, std::log(c.alpha), log_m_tilde, s);
    if (check_status(e, s)) return 1;
    a.uniform = 0;
    a.require_support = 0;
    a.theta = theta;
    a.out_counts = log_m_bar;
    double previous = 0.0;
    for (int it = 0; it < c.max_iter; it++) {
      if (launch_sbn_log_prob(a, s)) return fail("SBN training: the sort could not be enqueued");
      if (c.alpha > 0.0) launch_sbn_combine(P, log_m_bar, log_m_tilde, 0.0, log_m_bar, s);
      launch_sbn_normalize(c.p.S, c.p.parents, c.p.parent_range, log_m_bar, theta, s);
      launch_sbn_score(T, c.p.weights, log_q, P, c.alpha > 0.0 ? log_m_tilde : nullptr, theta, c.out_history + it, s);
      double score = 0.0;
      HIP_TRY(hipMemcpyAsync(&score, c.out_history + it, sizeof(double), hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      iterations = it + 1;
      if (it > 0) {
        const double gain = (score - previous) / std::fabs(previous);
        // (the reference's ERR_TOLERANCE, src/sbn_probability.cpp:315)
        if (!(gain > -1e-10))
          return fail("SBN training: the score decreased from " + std::to_string(previous) + " to " +
                      std::to_string(score) + " in iteration " + std::to_string(it));
        if (std::fabs(gain) < c.score_epsilon) break;
      }
      previous = score;
    }
  }
  HIP_TRY(hipMemcpyAsync(c.out_iterations, &iterations, sizeof(int32_t), hipMemcpyHostToDevice, s));
  HIP_TRY(hipGetLastError());
  if (check_status(e, s)) return 1;
  note_call(e, "sbn_walk_kernel", T, n);
  return 0;
}

// ---- the descent table, the sampler and the topology gradient ----
struct SbnDescentCall {
  int T0 = 0, n = 0, S = 0, C = 0;
  const int32_t *parent_ids = nullptr, *root_index = nullptr, *slot_index = nullptr, *pcsp_parent = nullptr;
  int32_t* out_descent = nullptr;
};

int check_descent_call(const mi_engine* e, const SbnDescentCall& c) {
  if (check_sbn_shape(e, c.T0, c.n)) return 1;
  if (c.S < 1 || c.C < 0) return fail("SBN: bad rootsplit or PCSP count");
  if (!c.parent_ids || !c.root_index || !c.slot_index) return fail("null tree arrays");
  if (c.C > 0 && !c.pcsp_parent) return fail("SBN descent: null pcsp_parent");
  if (!c.out_descent) return fail("null output pointer");
  return 0;
}

int run_sbn_descent_device(mi_engine* e, hipStream_t s, const SbnDescentCall& c) {
  if (check_descent_call(e, c)) return 1;
  HIP_TRY(hipSetDevice(e->spec.device));
  const size_t store = sbn_store_bytes(e, c.T0, c.n);
  if (store > e->plv_budget) return fail("SBN descent: " + sizes(c.T0, c.n, store, e));
  if (store && e->sbn_store.ensure(store)) return 1;
  if (e->status.ensure(sizeof(int32_t) * kStatusWords)) return 1;
  SbnDescentArgs a{};
  a.n = c.n;
  a.T0 = c.T0;
  a.tpw = sbn_tpw(e);
  a.S = c.S;
  a.C = c.C;
  a.parent_ids = c.parent_ids;
  a.root_index = c.root_index;
  a.slot_index = c.slot_index;
  a.pcsp_parent = c.pcsp_parent;
  a.status = e->status.as<int32_t>();
  a.store = e->sbn_store.as<char>();
  a.out_descent = c.out_descent;
  launch_sbn_descent(a, s);
  HIP_TRY(hipGetLastError());
  note_call(e, "sbn_descent_kernel", c.T0, c.n);
  return 0;
}

struct SbnSampleCall {
  int K = 0, n = 0, S = 0, C = 0, parents = 0;
  const int32_t *parent_range = nullptr, *descent = nullptr;
  const double* log_params = nullptr;
  uint64_t seed = 0;
  int64_t first_sample = 0;
  int32_t *out_parent_ids = nullptr, *out_root_edge = nullptr, *out_params = nullptr;
  double *out_log_prob = nullptr, *out_cdf = nullptr;
};

int check_sample_call(const mi_engine* e, const SbnSampleCall& c) {
  if (check_sbn_shape(e, c.K, c.n)) return 1;
  if (check_support(c.S, c.C, c.parents, c.parent_range)) return 1;
  if (!c.descent) return fail("SBN sample: null descent table");
  if (!c.log_params) return fail("null parameter vector");
  if (!c.out_parent_ids || !c.out_root_edge || !c.out_params || !c.out_log_prob) return fail("null output pointer");
  return 0;
}

int run_sbn_sample_device(mi_engine* e, hipStream_t s, const SbnSampleCall& c) {
  if (check_sample_call(e, c)) return 1;
  HIP_TRY(hipSetDevice(e->spec.device));
  const int P = c.S + c.C;
  const ProbLayout l = call_layout(c.K, c.n, P);
  if (reserve_sbn_prob(e, c.K, c.n, P)) return 1;
  char* ws = e->sbn_prob_ws.as<char>();
  SbnSampleArgs a{};
  a.n = c.n;
  a.K = c.K;
  a.tpw = sbn_tpw(e);
  a.S = c.S;
  a.C = c.C;
  a.parents = c.parents;
  a.parent_range = c.parent_range;
  a.descent = c.descent;
  a.phi = c.log_params;
  a.seed = c.seed;
  a.first_sample = c.first_sample;
  a.vi = e->vi_state;
  a.status = e->status.as<int32_t>();
  a.store = e->sbn_store.as<char>();
  a.cdf = c.out_cdf ? c.out_cdf : reinterpret_cast<double*>(ws + l.log_m_tilde);
  a.block_max = reinterpret_cast<double*>(ws + l.log_m_bar);  // (parents + 1 <= P)
  a.out_parent_ids = c.out_parent_ids;
  a.out_root_edge = c.out_root_edge;
  a.out_params = c.out_params;
  a.out_log_prob = c.out_log_prob;
  launch_sbn_check_params(P, c.log_params, a.status, s);
  launch_sbn_sample(a, s);
  HIP_TRY(hipGetLastError());
  note_call(e, "sbn_sample_kernel", c.K, c.n);
  return 0;
}

struct SbnGradientCall {
  SbnProbCall p;  // (weights and the rooting output unused; out_counts null)
  const double* log_f = nullptr;
  int estimator = 0;
  double *out_gradient = nullptr, *out_factors = nullptr;
};

int check_gradient_call(const mi_engine* e, const SbnGradientCall& c) {
  if (check_sbn_shape(e, c.p.T, c.p.n)) return 1;
  if (check_support(c.p.S, c.p.C, c.p.parents, c.p.parent_range)) return 1;
  if (!c.p.parent_ids || !c.p.root_index || !c.p.slot_index) return fail("null tree arrays");
  if (!c.p.log_params) return fail("null parameter vector");
  if (c.estimator != MI_SBN_FACTORS_PLAIN && c.estimator != MI_SBN_FACTORS_VIMCO && c.estimator != MI_SBN_FACTORS_GIVEN)
    return fail("SBN topology gradient: estimator must be MI_SBN_FACTORS_PLAIN, _VIMCO or _GIVEN");
  if (c.estimator == MI_SBN_FACTORS_VIMCO && c.p.T < 2)
    return fail("SBN topology gradient: the VIMCO factors need at least 2 trees");
  if (!c.log_f) return fail("SBN topology gradient: null log_f");
  if (!c.out_gradient || !c.out_factors || !c.p.out_log_q) return fail("null output pointer");
  return 0;
}

int run_sbn_gradient_device(mi_engine* e, hipStream_t s, const SbnGradientCall& c) {
  if (check_gradient_call(e, c)) return 1;
  HIP_TRY(hipSetDevice(e->spec.device));
  const int T = c.p.T, n = c.p.n, P = c.p.S + c.p.C;
  const ProbLayout l = call_layout(T, n, P);
  if (reserve_sbn_prob(e, T, n, P)) return 1;
  char* ws = e->sbn_prob_ws.as<char>();
  // the walk of log_prob: log q and the log usage of every entry, every tree with weight 1
  SbnProbArgs a = prob_args(e, c.p, l);
  launch_sbn_check_params(P, c.p.log_params, a.status, s);
  double* theta = reinterpret_cast<double*>(ws + l.theta);
  if (!c.p.normalized) launch_sbn_normalize(c.p.S, c.p.parents, c.p.parent_range, c.p.log_params, theta, s);
  a.theta = c.p.normalized ? c.p.log_params : theta;
  a.weights = nullptr;
  a.out_rooting = reinterpret_cast<double*>(ws + l.rooting);
  a.out_log_q = c.p.out_log_q;
  a.out_counts = nullptr;
  if (launch_sbn_log_prob(a, s)) return fail("SBN topology gradient: the walk could not be enqueued");
  SbnGradientArgs g{};
  g.n = n;
  g.T = T;
  g.P = P;
  g.S = c.p.S;
  g.parents = c.p.parents;
  g.estimator = c.estimator;
  g.root_index = c.p.root_index;
  g.slot_index = c.p.slot_index;
  g.parent_range = c.p.parent_range;
  g.theta = a.theta;
  g.log_f = c.log_f;
  g.usage = a.usage;
  g.keys = a.keys;
  g.keys2 = a.keys2;
  g.vals = a.vals;
  g.vals2 = a.vals2;
  g.sort_tmp = a.sort_tmp;
  g.sort_tmp_bytes = a.sort_tmp_bytes;
  g.G = reinterpret_cast<double*>(ws + l.log_m_bar);
  g.sums = reinterpret_cast<double*>(ws + l.log_q);  // (the gradient's log q is the caller's array)
  g.out_factors = c.out_factors;
  g.out_gradient = c.out_gradient;
  if (launch_sbn_gradient(g, s)) return fail("SBN topology gradient: the sort could not be enqueued");
  HIP_TRY(hipGetLastError());
  note_call(e, "sbn_walk_kernel", T, n);
  return 0;
}

}  // namespace

extern "C" {

int32_t mi_engine_sbn_index_device(mi_engine* e, void* stream, int32_t T, int32_t n, const int32_t* parent_ids,
                                   int32_t support_tree_count, int32_t rootsplit_capacity, int32_t pcsp_capacity,
                                   int32_t* out_root_index, int32_t* out_slot_index, int32_t* out_counts,
                                   uint32_t* out_split_bits, int32_t* out_pcsp_clades, int32_t* out_parent_range,
                                   int32_t* out_pcsp_parent) {
  if (!e) return fail("null engine");
  if (!e->shards.empty()) return fail(kShardedDeviceCall);
  SbnIndexCall c;
  c.T = T;
  c.n = n;
  c.T0 = support_tree_count;
  c.root_capacity = rootsplit_capacity;
  c.pcsp_capacity = pcsp_capacity;
  c.parent_ids = parent_ids;
  c.out_root_index = out_root_index;
  c.out_slot_index = out_slot_index;
  c.out_counts = out_counts;
  c.out_split_bits = out_split_bits;
  c.out_pcsp_clades = out_pcsp_clades;
  c.out_parent_range = out_parent_range;
  c.out_pcsp_parent = out_pcsp_parent;
  return run_sbn_index_device(e, pick_stream(e, stream), c);
}

// The host form: arrays of fixed counts.  The table rows come down whole into arrays of the call's
// own and the first S, C and `parents` of them are handed on: the caller's other rows stay.
int32_t mi_engine_sbn_index(mi_engine* e, int32_t T, int32_t n, const int32_t* parent_ids, int32_t support_tree_count,
                            int32_t rootsplit_capacity, int32_t pcsp_capacity, int32_t* out_root_index,
                            int32_t* out_slot_index, int32_t* out_counts, uint32_t* out_split_bits,
                            int32_t* out_pcsp_clades, int32_t* out_parent_range, int32_t* out_pcsp_parent) {
  SbnIndexCall c;
  c.T = T;
  c.n = n;
  c.T0 = support_tree_count;
  c.root_capacity = rootsplit_capacity;
  c.pcsp_capacity = pcsp_capacity;
  c.parent_ids = parent_ids;
  c.out_root_index = out_root_index;
  c.out_slot_index = out_slot_index;
  c.out_counts = out_counts;
  c.out_split_bits = out_split_bits;
  c.out_pcsp_clades = out_pcsp_clades;
  c.out_parent_range = out_parent_range;
  c.out_pcsp_parent = out_pcsp_parent;
  if (check_index_call(e, c)) return 1;
  e = first_engine(e);
  const size_t E = 2 * (size_t)n - 3, W = split_words(n), rcap = rootsplit_capacity, pcap = pcsp_capacity;
  std::vector<uint32_t> bits(rcap * W);
  std::vector<int32_t> clades(pcap * 3), range(pcap * 2), parent(pcap);
  int32_t counts[3] = {0, 0, 0};
  HostCall h;
  h.in = {fixed(parent_ids, (size_t)T * E)};
  h.out = {fixed(out_root_index, (size_t)T * E), fixed(out_slot_index, (size_t)T * E * 6), fixed(counts, 3),
           fixed(rcap ? bits.data() : nullptr, rcap * W), fixed(pcap ? clades.data() : nullptr, pcap * 3),
           fixed(pcap ? range.data() : nullptr, pcap * 2), fixed(pcap ? parent.data() : nullptr, pcap)};
  h.enqueue = [=](mi_engine* e, int, const HostArray* in, const HostArray* out) {
    SbnIndexCall d = c;
    d.parent_ids = in[0].at<const int32_t>();
    d.out_root_index = out[0].at<int32_t>();
    d.out_slot_index = out[1].at<int32_t>();
    d.out_counts = out[2].at<int32_t>();
    d.out_split_bits = out[3].at<uint32_t>();
    d.out_pcsp_clades = out[4].at<int32_t>();
    d.out_parent_range = out[5].at<int32_t>();
    d.out_pcsp_parent = out[6].at<int32_t>();
    return run_sbn_index_device(e, e->stream, d);
  };
  if (run_on_engine(e, h)) return 1;
  memcpy(out_counts, counts, sizeof counts);
  const size_t S = std::min<size_t>(counts[0], rcap), C = std::min<size_t>(counts[1], pcap);
  const size_t parents = std::min<size_t>(counts[2], pcap);
  if (S) memcpy(out_split_bits, bits.data(), S * W * 4);
  if (C) {
    memcpy(out_pcsp_clades, clades.data(), C * 12);
    memcpy(out_pcsp_parent, parent.data(), C * 4);
    memcpy(out_parent_range, range.data(), parents * 8);
  }
  return 0;
}

int32_t mi_engine_sbn_log_prob_device(mi_engine* e, void* stream, int32_t T, int32_t n, const int32_t* parent_ids,
                                      const int32_t* root_index, const int32_t* slot_index, int32_t S, int32_t C,
                                      int32_t parents, const int32_t* parent_range, const double* log_params,
                                      int32_t normalized, const double* tree_weights, double* out_rooting_log_prob,
                                      double* out_log_q, double* out_log_expected_counts) {
  if (!e) return fail("null engine");
  if (!e->shards.empty()) return fail(kShardedDeviceCall);
  SbnProbCall c;
  c.T = T;
  c.n = n;
  c.S = S;
  c.C = C;
  c.parents = parents;
  c.normalized = normalized != 0;
  c.parent_ids = parent_ids;
  c.root_index = root_index;
  c.slot_index = slot_index;
  c.parent_range = parent_range;
  c.log_params = log_params;
  c.weights = tree_weights;
  c.out_rooting = out_rooting_log_prob;
  c.out_log_q = out_log_q;
  c.out_counts = out_log_expected_counts;
  return run_sbn_log_prob_device(e, pick_stream(e, stream), c);
}

int32_t mi_engine_sbn_log_prob(mi_engine* e, int32_t T, int32_t n, const int32_t* parent_ids, const int32_t* root_index,
                               const int32_t* slot_index, int32_t S, int32_t C, int32_t parents,
                               const int32_t* parent_range, const double* log_params, int32_t normalized,
                               const double* tree_weights, double* out_rooting_log_prob, double* out_log_q,
                               double* out_log_expected_counts) {
  SbnProbCall c;
  c.T = T;
  c.n = n;
  c.S = S;
  c.C = C;
  c.parents = parents;
  c.normalized = normalized != 0;
  c.parent_ids = parent_ids;
  c.root_index = root_index;
  c.slot_index = slot_index;
  c.parent_range = parent_range;
  c.log_params = log_params;
  c.weights = tree_weights;
  c.out_rooting = out_rooting_log_prob;
  c.out_log_q = out_log_q;
  c.out_counts = out_log_expected_counts;
  if (check_prob_call(e, c)) return 1;
  const size_t E = 2 * (size_t)n - 3, P = (size_t)S + C;
  HostCall h;
  h.in = {fixed(parent_ids, (size_t)T * E), fixed(root_index, (size_t)T * E), fixed(slot_index, (size_t)T * E * 6),
          fixed(parent_range, (size_t)parents * 2), fixed(log_params, P), fixed(tree_weights, T)};
  h.out = {fixed(out_rooting_log_prob, (size_t)T * E), fixed(out_log_q, T), fixed(out_log_expected_counts, P)};
  h.enqueue = [=](mi_engine* e, int, const HostArray* in, const HostArray* out) {
    SbnProbCall d = c;
    d.parent_ids = in[0].at<const int32_t>();
    d.root_index = in[1].at<const int32_t>();
    d.slot_index = in[2].at<const int32_t>();
    d.parent_range = in[3].at<const int32_t>();
    d.log_params = in[4].at<const double>();
    d.weights = in[5].at<const double>();
    d.out_rooting = out[0].at<double>();
    d.out_log_q = out[1].at<double>();
    d.out_counts = out[2].at<double>();
    return run_sbn_log_prob_device(e, e->stream, d);
  };
  return run_on_engine(first_engine(e), h);
}

int32_t mi_engine_sbn_normalize_device(mi_engine* e, void* stream, int32_t S, int32_t C, int32_t parents,
                                       const int32_t* parent_range, const double* log_params, double* out_log_params) {
  if (!e) return fail("null engine");
  if (!e->shards.empty()) return fail(kShardedDeviceCall);
  return run_sbn_normalize_device(e, pick_stream(e, stream), S, C, parents, parent_range, log_params, out_log_params);
}

int32_t mi_engine_sbn_normalize(mi_engine* e, int32_t S, int32_t C, int32_t parents, const int32_t* parent_range,
                                const double* log_params, double* out_log_params) {
  if (!e) return fail("null engine");
  if (check_support(S, C, parents, parent_range)) return 1;
  if (!log_params || !out_log_params) return fail("null parameter vector");
  const size_t P = (size_t)S + C;
  HostCall h;
  h.in = {fixed(parent_range, (size_t)parents * 2), fixed(log_params, P)};
  h.out = {fixed(out_log_params, P)};
  h.enqueue = [=](mi_engine* e, int, const HostArray* in, const HostArray* out) {
    return run_sbn_normalize_device(e, e->stream, S, C, parents, in[0].at<const int32_t>(), in[1].at<const double>(),
                                    out[0].at<double>());
  };
  return run_on_engine(first_engine(e), h);
}

int32_t mi_engine_sbn_train_device(mi_engine* e, void* stream, int32_t T, int32_t n, const int32_t* parent_ids,
                                   const int32_t* root_index, const int32_t* slot_index, int32_t S, int32_t C,
                                   int32_t parents, const int32_t* parent_range, const double* tree_weights,
                                   int32_t method, double alpha, int32_t max_iter, double score_epsilon,
                                   double* out_log_params, double* out_score_history, int32_t* out_iterations) {
  if (!e) return fail("null engine");
  if (!e->shards.empty()) return fail(kShardedDeviceCall);
  SbnTrainCall c;
  c.p.T = T;
  c.p.n = n;
  c.p.S = S;
  c.p.C = C;
  c.p.parents = parents;
  c.p.parent_ids = parent_ids;
  c.p.root_index = root_index;
  c.p.slot_index = slot_index;
  c.p.parent_range = parent_range;
  c.p.weights = tree_weights;
  c.method = method;
  c.alpha = alpha;
  c.max_iter = max_iter;
  c.score_epsilon = score_epsilon;
  c.out_log_params = out_log_params;
  c.out_history = out_score_history;
  c.out_iterations = out_iterations;
  return run_sbn_train_device(e, pick_stream(e, stream), c);
}

int32_t mi_engine_sbn_train(mi_engine* e, int32_t T, int32_t n, const int32_t* parent_ids, const int32_t* root_index,
                            const int32_t* slot_index, int32_t S, int32_t C, int32_t parents,
                            const int32_t* parent_range, const double* tree_weights, int32_t method, double alpha,
                            int32_t max_iter, double score_epsilon, double* out_log_params, double* out_score_history,
                            int32_t* out_iterations) {
  SbnTrainCall c;
  c.p.T = T;
  c.p.n = n;
  c.p.S = S;
  c.p.C = C;
  c.p.parents = parents;
  c.p.parent_ids = parent_ids;
  c.p.root_index = root_index;
  c.p.slot_index = slot_index;
  c.p.parent_range = parent_range;
  c.p.weights = tree_weights;
  c.method = method;
  c.alpha = alpha;
  c.max_iter = max_iter;
  c.score_epsilon = score_epsilon;
  c.out_log_params = out_log_params;
  c.out_history = out_score_history;
  c.out_iterations = out_iterations;
  if (check_train_call(e, c)) return 1;
  const size_t E = 2 * (size_t)n - 3, P = (size_t)S + C;
  HostCall h;
  h.in = {fixed(parent_ids, (size_t)T * E), fixed(root_index, (size_t)T * E), fixed(slot_index, (size_t)T * E * 6),
          fixed(parent_range, (size_t)parents * 2), fixed(tree_weights, T)};
  h.out = {fixed(out_log_params, P), fixed(max_iter > 0 ? out_score_history : nullptr, max_iter), fixed(out_iterations, 1)};
  h.enqueue = [=](mi_engine* e, int, const HostArray* in, const HostArray* out) {
    SbnTrainCall d = c;
    d.p.parent_ids = in[0].at<const int32_t>();
    d.p.root_index = in[1].at<const int32_t>();
    d.p.slot_index = in[2].at<const int32_t>();
    d.p.parent_range = in[3].at<const int32_t>();
    d.p.weights = in[4].at<const double>();
    d.out_log_params = out[0].at<double>();
    d.out_history = out[1].at<double>();
    d.out_iterations = out[2].at<int32_t>();
    return run_sbn_train_device(e, e->stream, d);
  };
  return run_on_engine(first_engine(e), h);
}

int32_t mi_engine_sbn_descent_device(mi_engine* e, void* stream, int32_t T0, int32_t n, const int32_t* parent_ids,
                                     const int32_t* root_index, const int32_t* slot_index, int32_t S, int32_t C,
                                     const int32_t* pcsp_parent, int32_t* out_descent) {
  if (!e) return fail("null engine");
  if (!e->shards.empty()) return fail(kShardedDeviceCall);
  SbnDescentCall c;
  c.T0 = T0;
  c.n = n;
  c.S = S;
  c.C = C;
  c.parent_ids = parent_ids;
  c.root_index = root_index;
  c.slot_index = slot_index;
  c.pcsp_parent = pcsp_parent;
  c.out_descent = out_descent;
  return run_sbn_descent_device(e, pick_stream(e, stream), c);
}

int32_t mi_engine_sbn_descent(mi_engine* e, int32_t T0, int32_t n, const int32_t* parent_ids, const int32_t* root_index,
                              const int32_t* slot_index, int32_t S, int32_t C, const int32_t* pcsp_parent,
                              int32_t* out_descent) {
  SbnDescentCall c;
  c.T0 = T0;
  c.n = n;
  c.S = S;
  c.C = C;
  c.parent_ids = parent_ids;
  c.root_index = root_index;
  c.slot_index = slot_index;
  c.pcsp_parent = pcsp_parent;
  c.out_descent = out_descent;
  if (check_descent_call(e, c)) return 1;
  const size_t E = 2 * (size_t)n - 3, P = (size_t)S + C;
  HostCall h;
  h.in = {fixed(parent_ids, (size_t)T0 * E), fixed(root_index, (size_t)T0 * E), fixed(slot_index, (size_t)T0 * E * 6),
          fixed(pcsp_parent, (size_t)C)};
  h.out = {fixed(out_descent, P * 2)};
  h.enqueue = [=](mi_engine* e, int, const HostArray* in, const HostArray* out) {
    SbnDescentCall d = c;
    d.parent_ids = in[0].at<const int32_t>();
    d.root_index = in[1].at<const int32_t>();
    d.slot_index = in[2].at<const int32_t>();
    d.pcsp_parent = in[3].at<const int32_t>();
    d.out_descent = out[0].at<int32_t>();
    return run_sbn_descent_device(e, e->stream, d);
  };
  return run_on_engine(first_engine(e), h);
}

int32_t mi_engine_sbn_sample_device(mi_engine* e, void* stream, int32_t K, int32_t n, int32_t S, int32_t C,
                                    int32_t parents, const int32_t* parent_range, const int32_t* descent,
                                    const double* log_params, uint64_t seed, int64_t first_sample,
                                    int32_t* out_parent_ids, int32_t* out_root_edge, int32_t* out_sampled_params,
                                    double* out_log_prob, double* out_cdf) {
  if (!e) return fail("null engine");
  if (!e->shards.empty()) return fail(kShardedDeviceCall);
  SbnSampleCall c;
  c.K = K;
  c.n = n;
  c.S = S;
  c.C = C;
  c.parents = parents;
  c.parent_range = parent_range;
  c.descent = descent;
  c.log_params = log_params;
  c.seed = seed;
  c.first_sample = first_sample;
  c.out_parent_ids = out_parent_ids;
  c.out_root_edge = out_root_edge;
  c.out_params = out_sampled_params;
  c.out_log_prob = out_log_prob;
  c.out_cdf = out_cdf;
  return run_sbn_sample_device(e, pick_stream(e, stream), c);
}

int32_t mi_engine_sbn_sample(mi_engine* e, int32_t K, int32_t n, int32_t S, int32_t C, int32_t parents,
                             const int32_t* parent_range, const int32_t* descent, const double* log_params,
                             uint64_t seed, int64_t first_sample, int32_t* out_parent_ids, int32_t* out_root_edge,
                             int32_t* out_sampled_params, double* out_log_prob, double* out_cdf) {
  SbnSampleCall c;
  c.K = K;
  c.n = n;
  c.S = S;
  c.C = C;
  c.parents = parents;
  c.parent_range = parent_range;
  c.descent = descent;
  c.log_params = log_params;
  c.seed = seed;
  c.first_sample = first_sample;
  c.out_parent_ids = out_parent_ids;
  c.out_root_edge = out_root_edge;
  c.out_params = out_sampled_params;
  c.out_log_prob = out_log_prob;
  c.out_cdf = out_cdf;
  if (check_sample_call(e, c)) return 1;
  const size_t E = 2 * (size_t)n - 3, P = (size_t)S + C;
  HostCall h;
  h.in = {fixed(parent_range, (size_t)parents * 2), fixed(descent, P * 2), fixed(log_params, P)};
  h.out = {fixed(out_parent_ids, (size_t)K * E), fixed(out_root_edge, (size_t)K),
           fixed(out_sampled_params, (size_t)K * (n - 1)), fixed(out_log_prob, (size_t)K), fixed(out_cdf, P)};
  h.enqueue = [=](mi_engine* e, int, const HostArray* in, const HostArray* out) {
    SbnSampleCall d = c;
    d.parent_range = in[0].at<const int32_t>();
    d.descent = in[1].at<const int32_t>();
    d.log_params = in[2].at<const double>();
    d.out_parent_ids = out[0].at<int32_t>();
    d.out_root_edge = out[1].at<int32_t>();
    d.out_params = out[2].at<int32_t>();
    d.out_log_prob = out[3].at<double>();
    d.out_cdf = out[4].at<double>();
    return run_sbn_sample_device(e, e->stream, d);
  };
  return run_on_engine(first_engine(e), h);
}

int32_t mi_engine_sbn_topology_gradient_device(mi_engine* e, void* stream, int32_t T, int32_t n,
                                               const int32_t* parent_ids, const int32_t* root_index,
                                               const int32_t* slot_index, int32_t S, int32_t C, int32_t parents,
                                               const int32_t* parent_range, const double* log_params,
                                               int32_t normalized, const double* log_f, int32_t estimator,
                                               double* out_gradient, double* out_factors, double* out_log_q) {
  if (!e) return fail("null engine");
  if (!e->shards.empty()) return fail(kShardedDeviceCall);
  SbnGradientCall c;
  c.p.T = T;
  c.p.n = n;
  c.p.S = S;
  c.p.C = C;
  c.p.parents = parents;
  c.p.normalized = normalized != 0;
  c.p.parent_ids = parent_ids;
  c.p.root_index = root_index;
  c.p.slot_index = slot_index;
  c.p.parent_range = parent_range;
  c.p.log_params = log_params;
  c.p.out_log_q = out_log_q;
  c.log_f = log_f;
  c.estimator = estimator;
  c.out_gradient = out_gradient;
  c.out_factors = out_factors;
  return run_sbn_gradient_device(e, pick_stream(e, stream), c);
}

int32_t mi_engine_sbn_topology_gradient(mi_engine* e, int32_t T, int32_t n, const int32_t* parent_ids,
                                        const int32_t* root_index, const int32_t* slot_index, int32_t S, int32_t C,
                                        int32_t parents, const int32_t* parent_range, const double* log_params,
                                        int32_t normalized, const double* log_f, int32_t estimator,
                                        double* out_gradient, double* out_factors, double* out_log_q) {
  SbnGradientCall c;
  c.p.T = T;
  c.p.n = n;
  c.p.S = S;
  c.p.C = C;
  c.p.parents = parents;
  c.p.normalized = normalized != 0;
  c.p.parent_ids = parent_ids;
  c.p.root_index = root_index;
  c.p.slot_index = slot_index;
  c.p.parent_range = parent_range;
  c.p.log_params = log_params;
  c.p.out_log_q = out_log_q;
  c.log_f = log_f;
  c.estimator = estimator;
  c.out_gradient = out_gradient;
  c.out_factors = out_factors;
  if (check_gradient_call(e, c)) return 1;
  const size_t E = 2 * (size_t)n - 3, P = (size_t)S + C;
  HostCall h;
  h.in = {fixed(parent_ids, (size_t)T * E), fixed(root_index, (size_t)T * E), fixed(slot_index, (size_t)T * E * 6),
          fixed(parent_range, (size_t)parents * 2), fixed(log_params, P), fixed(log_f, (size_t)T)};
  h.out = {fixed(out_gradient, P), fixed(out_factors, (size_t)T), fixed(out_log_q, (size_t)T)};
  h.enqueue = [=](mi_engine* e, int, const HostArray* in, const HostArray* out) {
    SbnGradientCall d = c;
    d.p.parent_ids = in[0].at<const int32_t>();
    d.p.root_index = in[1].at<const int32_t>();
    d.p.slot_index = in[2].at<const int32_t>();
    d.p.parent_range = in[3].at<const int32_t>();
    d.p.log_params = in[4].at<const double>();
    d.log_f = in[5].at<const double>();
    d.out_gradient = out[0].at<double>();
    d.out_factors = out[1].at<double>();
    d.p.out_log_q = out[2].at<double>();
    return run_sbn_gradient_device(e, e->stream, d);
  };
  return run_on_engine(first_engine(e), h);
}

int32_t mi_engine_reserve_sbn(mi_engine* e, int32_t T, int32_t n) {
  if (check_sbn_shape(e, T, n)) return 1;
  e = first_engine(e);
  HIP_TRY(hipSetDevice(e->spec.device));
  if (mi_engine_reserve_splits(e, T, n)) return 1;
  if (reserve_sbn_index(e, T, n)) return 1;
  if (reserve_sbn_prob(e, T, n, 0)) return 1;
  sbn_prepare(n, sbn_tpw(e));
  sbn_vi_prepare(n, sbn_tpw(e));
  return 0;
}

}  // extern "C"
