// Bootstrap weights drawn on the device and the KH, SH and AU tests (mi_engine_bootstrap_weights*,
// mi_engine_topology_tests*, mi_engine_topology_tests_unrooted).  The sampler and the
// statistics are kernels_boot.hip's; the products and their row and column passes are launch_rell
// (kernels_rell.hip) as mi_engine_rell runs them.  The matrix calls need no alignment.
#include <cmath>

#include "mi_phylo_engine.h"

namespace {

const char kTopoSharded[] =
    "mi_engine_topology_tests_unrooted needs a single-device engine: the products need every tree's row on one "
    "device (mi_engine_pattern_log_likelihoods_unrooted + mi_engine_topology_tests serve a tree-sharded handle)";
const char kTopoPatternShards[] =
    "pattern-sharded engines do not run the topology tests (each shard holds a block of columns): use "
    "MI_SHARD_TREES or a single engine";
constexpr int64_t kBootMaxSites = (int64_t)1 << 33;

template <typename T>
T* take(char* base, size_t& off, size_t count) {
  char* p = base + off;
  off += align256(sizeof(T) * count);
  return reinterpret_cast<T*>(p);
}

// the pieces of e->boot_ws, 256-byte aligned: prefix sum | N | the global form's histogram rows
struct BootWorkspace {
  uint32_t *cum, *total;
  int32_t* hist;
  size_t bytes;
  BootWorkspace(int B, int P, bool forced_global, char* base) {
    size_t off = 0;
    cum = take<uint32_t>(base, off, (size_t)P + 1);
    total = take<uint32_t>(base, off, 1);
    const size_t rows = boot_hist_rows(B, P, forced_global);
    hist = rows ? take<int32_t>(base, off, rows * P) : nullptr;
    bytes = off;
  }
};

// the pieces of e->topo_ws: a block's weights and product, the row statistics, and the per-tree rows
struct TopoWorkspace {
  double *w, *c, *row_max, *row_inv, *zmax;
  double *L, *bp_scratch, *bp0, *elw0, *mean;
  int32_t *cnt_scratch, *sh, *kh, *sel;
  size_t bytes;
  TopoWorkspace(int T, int P, int maxB, char* base) {
    size_t off = 0;
    w = take<double>(base, off, (size_t)maxB * P);
    c = take<double>(base, off, (size_t)maxB * T);
    row_max = take<double>(base, off, maxB);
    row_inv = take<double>(base, off, maxB);
    zmax = take<double>(base, off, maxB);
    L = take<double>(base, off, T);
    bp_scratch = take<double>(base, off, T);
    bp0 = take<double>(base, off, T);
    elw0 = take<double>(base, off, T);
    mean = take<double>(base, off, T);
    cnt_scratch = take<int32_t>(base, off, 3 * (size_t)T);  // (the three count rows are zeroed by one launch)
    sh = cnt_scratch + T;
    kh = sh + T;
    sel = take<int32_t>(base, off, 2);
    bytes = off;
  }
};

int check_sites(int64_t sites) {
  if (sites < 1 || sites > kBootMaxSites) return fail("bootstrap weights: sites must be in [1, 2^33]");
  return 0;
}

// what the host forms refuse before any device work (the device forms: the status word)
int check_host_weights(int P, const double* w, int64_t* total) {
  double sum = 0.0;
  for (int p = 0; p < P; p++) {
    if (!(w[p] >= 0.0 && w[p] <= 1.79769313486231570e308 && w[p] == std::floor(w[p])))
      return fail(std::string(status_message(kBootBadWeight)) + " (pattern " + std::to_string(p) + ")");
    sum += std::fmin(w[p], 2147483648.0);  // (integers of at most 2^31, fewer than 2^31 of them: exact)
  }
  if (!(sum >= 1.0 && sum < 2147483648.0)) return fail(status_message(kBootBadTotal));
  *total = (int64_t)sum;
  return 0;
}

int reserve_boot(mi_engine* e, int B, int P) {
  return e->boot_ws.ensure(BootWorkspace(B, P, e->sw.boot_hist_global, nullptr).bytes);
}

BootArgs boot_args(mi_engine* e, int B, int P, const double* weights, int64_t expect_total) {
  const BootWorkspace ws(B, P, e->sw.boot_hist_global, e->boot_ws.as<char>());
  BootArgs a{};
  a.P = P;
  a.global_hist = boot_hist_global(P, e->sw.boot_hist_global) ? 1 : 0;
  a.expect_total = expect_total;
  a.weights = weights;
  a.cum = ws.cum;
  a.total = ws.total;
  a.hist = ws.hist;
  a.status = e->status.as<int32_t>();
  return a;
}

int run_boot_device(mi_engine* e, hipStream_t s, int P, const double* weights, int B, int64_t sites, uint64_t seed,
                    int64_t first_replicate, double* out) {
  HIP_TRY(hipSetDevice(e->spec.device));
  if (P <= 0 || B <= 0) return fail("pattern_count and replicate_count must be positive");
  if (!weights || !out) return fail("null pattern weights / replicate weight output");
  if (check_sites(sites)) return 1;
  if (reserve_boot(e, B, P)) return 1;
  BootArgs a = boot_args(e, B, P, weights, -1);
  a.B = B;
  a.sites = (uint64_t)sites;
  a.seed = seed;
  a.first_replicate = (uint64_t)first_replicate;
  a.out = out;
  launch_boot_prefix(a, s);
  launch_boot_sample(a, s);
  HIP_TRY(hipGetLastError());
  return 0;
}

// One call of the tests with every array pointer a device pointer (the blocks' sizes are the host's).
struct TopoCall {
  int T = 0, P = 0, K = 0;
  const double* s = nullptr;  // [T][P]
  const double* w = nullptr;  // [P]
  const int64_t* sites = nullptr;
  const int32_t* replicates = nullptr;
  uint64_t seed = 0;
  int64_t first_replicate = 0;
  double* out_table = nullptr;   // [T][kTopoColumns]
  int32_t* out_counts = nullptr;  // [K][T]
  double* out_mean = nullptr;    // [T] or nullptr
  double* out_c = nullptr;       // [B_0][T] or nullptr
  int32_t* out_best = nullptr;   // [B_0] or nullptr
};

int check_topo_shape(int T, int P, int K, const int64_t* sites, const int32_t* replicates, int* maxB) {
  if (T <= 0 || P <= 0) return fail("tree_count and pattern_count must be positive");
  if (K < 1 || K > kTopoMaxScales)
    return fail("topology tests: block_count must be in [1, " + std::to_string(kTopoMaxScales) + "]");
  if (!sites || !replicates) return fail("null sites / replicates array");
  *maxB = 0;
  for (int k = 0; k < K; k++) {
    if (check_sites(sites[k])) return 1;
    if (replicates[k] < 1) return fail("topology tests: every block needs at least one replicate");
    for (int j = 0; j < k; j++)
      if (sites[j] == sites[k]) return fail("topology tests: the blocks' sites must be pairwise distinct");
    *maxB = std::max(*maxB, (int)replicates[k]);
  }
  return 0;
}

int reserve_topo(mi_engine* e, int T, int P, int maxB) {
  return reserve_boot(e, maxB, P) || e->topo_ws.ensure(TopoWorkspace(T, P, maxB, nullptr).bytes);
}

int run_topo_device(mi_engine* e, hipStream_t st, const TopoCall& c) {
  HIP_TRY(hipSetDevice(e->spec.device));
  int maxB = 0;
  if (check_topo_shape(c.T, c.P, c.K, c.sites, c.replicates, &maxB)) return 1;
  if (!c.s || !c.w) return fail("null pattern log-likelihood matrix / pattern weights");
  if (!c.out_table || !c.out_counts) return fail("null table / count output");
  if (reserve_topo(e, c.T, c.P, maxB)) return 1;
  const int T = c.T, P = c.P;
  const TopoWorkspace ws(T, P, maxB, e->topo_ws.as<char>());
  // sites[0] must be N: the prefix sum's kernel compares them (status word)
  BootArgs boot = boot_args(e, maxB, P, c.w, c.sites[0]);
  boot.seed = c.seed;
  boot.out = ws.w;
  launch_boot_prefix(boot, st);
  launch_boot_zero(c.out_counts, (size_t)c.K * T, st);
  launch_boot_zero(ws.cnt_scratch, 3 * (size_t)T, st);
  // the observed log-likelihoods: the product with the one row w
  RellArgs r{};
  r.T = T;
  r.P = P;
  r.pattern_ll = c.s;
  r.row_max = ws.row_max;
  r.row_inv = ws.row_inv;
  r.B = 1;
  r.weights = c.w;
  r.c = ws.L;
  r.counts = ws.cnt_scratch;
  r.bp = ws.bp_scratch;
  launch_rell(r, st);
  TopoArgs ta{};
  ta.T = T;
  ta.K = c.K;
  ta.L = ws.L;
  ta.counts = c.out_counts;
  ta.bp = ws.bp0;
  ta.elw = ws.elw0;
  ta.total = boot.total;
  ta.mean = c.out_mean ? c.out_mean : ws.mean;
  ta.zmax = ws.zmax;
  ta.sel = ws.sel;
  ta.sh = ws.sh;
  ta.kh = ws.kh;
  ta.table = c.out_table;
  uint64_t first = (uint64_t)c.first_replicate;
  for (int k = 0; k < c.K; k++) {
    const int B = c.replicates[k];
    ta.sites[k] = c.sites[k];
    ta.replicates[k] = B;
    boot.B = B;
    boot.sites = (uint64_t)c.sites[k];
    boot.first_replicate = first;
    first += (uint64_t)B;
    launch_boot_sample(boot, st);
    r.B = B;
    r.weights = ws.w;
    r.c = k == 0 && c.out_c ? c.out_c : ws.c;
    r.counts = c.out_counts + (size_t)k * T;
    r.best = k == 0 ? c.out_best : nullptr;
    r.bp = k == 0 ? ws.bp0 : ws.bp_scratch;
    r.elw = k == 0 ? ws.elw0 : nullptr;
    launch_rell(r, st);
    if (k == 0) {
      ta.B = B;
      ta.c = r.c;
      launch_topo_block0(ta, st);
    }
  }
  launch_topo_table(ta, st);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" {

int32_t mi_engine_bootstrap_weights(mi_engine* e, int32_t P, const double* weights, int32_t B, int64_t sites,
                                    uint64_t seed, int64_t first_replicate, double* out_weights) {
  if (!e) return fail("null engine");
  if (P <= 0 || B <= 0) return fail("pattern_count and replicate_count must be positive");
  if (!weights || !out_weights) return fail("null pattern weights / replicate weight output");
  int64_t total = 0;
  if (check_host_weights(P, weights, &total) || check_sites(sites)) return 1;
  HostCall c;
  c.in = {fixed(weights, (size_t)P)};
  c.out = {fixed(out_weights, (size_t)B * P)};
  c.enqueue = [=](mi_engine* e, int, const HostArray* in, const HostArray* out) {
    return run_boot_device(e, e->stream, P, in[0].at<const double>(), B, sites, seed, first_replicate,
                           out[0].at<double>());
  };
  return run_on_engine(first_engine(e), c);
}

int32_t mi_engine_bootstrap_weights_device(mi_engine* e, void* stream, int32_t P, const double* weights, int32_t B,
                                           int64_t sites, uint64_t seed, int64_t first_replicate,
                                           double* out_weights) {
  if (!e) return fail("null engine");
  if (!e->shards.empty()) return fail(kShardedDeviceCall);
  return run_boot_device(e, pick_stream(e, stream), P, weights, B, sites, seed, first_replicate, out_weights);
}

int32_t mi_engine_reserve_bootstrap_weights(mi_engine* e, int32_t B, int32_t P) {
  if (!e) return fail("null engine");
  if (B <= 0 || P <= 0) return fail("replicate_count and pattern_count must be positive");
  mi_engine* one = first_engine(e);
  HIP_TRY(hipSetDevice(one->spec.device));
  return reserve_boot(one, B, P);
}

int32_t mi_engine_topology_tests(mi_engine* e, int32_t T, int32_t P, const double* pattern_ll, const double* weights,
                                 int32_t K, const int64_t* sites, const int32_t* replicates, uint64_t seed,
                                 int64_t first_replicate, double* out_table, int32_t* out_counts, double* out_mean,
                                 double* out_c, int32_t* out_best) {
  if (!e) return fail("null engine");
  int maxB = 0;
  if (check_topo_shape(T, P, K, sites, replicates, &maxB)) return 1;
  if (!pattern_ll || !weights) return fail("null pattern log-likelihood matrix / pattern weights");
  if (!out_table || !out_counts) return fail("null table / count output");
  int64_t total = 0;
  if (check_host_weights(P, weights, &total)) return 1;
  if (sites[0] != total) return fail(status_message(kBootSitesNotTotal));
  const std::vector<int64_t> sites_v(sites, sites + K);
  const std::vector<int32_t> reps_v(replicates, replicates + K);
  const size_t B0 = (size_t)replicates[0];
  HostCall c;
  c.in = {fixed(pattern_ll, (size_t)T * P), fixed(weights, (size_t)P)};
  c.out = {fixed(out_table, (size_t)T * kTopoColumns), fixed(out_counts, (size_t)K * T), fixed(out_mean, (size_t)T),
           fixed(out_c, B0 * T), fixed(out_best, B0)};
  c.enqueue = [=](mi_engine* e, int, const HostArray* in, const HostArray* out) {
    TopoCall d;
    d.T = T;
    d.P = P;
    d.K = K;
    d.s = in[0].at<const double>();
    d.w = in[1].at<const double>();
    d.sites = sites_v.data();
    d.replicates = reps_v.data();
    d.seed = seed;
    d.first_replicate = first_replicate;
    d.out_table = out[0].at<double>();
    d.out_counts = out[1].at<int32_t>();
    d.out_mean = out[2].at<double>();
    d.out_c = out[3].at<double>();
    d.out_best = out[4].at<int32_t>();
    return run_topo_device(e, e->stream, d);
  };
  return run_on_engine(first_engine(e), c);
}

int32_t mi_engine_topology_tests_device(mi_engine* e, void* stream, int32_t T, int32_t P, const double* pattern_ll,
                                        const double* weights, int32_t K, const int64_t* sites,
                                        const int32_t* replicates, uint64_t seed, int64_t first_replicate,
                                        double* out_table, int32_t* out_counts, double* out_mean, double* out_c,
                                        int32_t* out_best) {
  if (!e) return fail("null engine");
  if (!e->shards.empty()) return fail(kShardedDeviceCall);
  TopoCall d;
  d.T = T;
  d.P = P;
  d.K = K;
  d.s = pattern_ll;
  d.w = weights;
  d.sites = sites;
  d.replicates = replicates;
  d.seed = seed;
  d.first_replicate = first_replicate;
  d.out_table = out_table;
  d.out_counts = out_counts;
  d.out_mean = out_mean;
  d.out_c = out_c;
  d.out_best = out_best;
  return run_topo_device(e, pick_stream(e, stream), d);
}

int32_t mi_engine_reserve_topology_tests(mi_engine* e, int32_t T, int32_t P, int32_t max_replicates) {
  if (!e) return fail("null engine");
  if (T <= 0 || P <= 0 || max_replicates <= 0)
    return fail("tree_count, pattern_count and the largest replicate_count must be positive");
  mi_engine* one = first_engine(e);
  HIP_TRY(hipSetDevice(one->spec.device));
  return reserve_topo(one, T, P, max_replicates);
}

int32_t mi_engine_topology_tests_unrooted(mi_engine* e, int32_t T, const int32_t* parent_ids, const double* bl,
                                          const double* params, int32_t rescaling, int32_t K, const int64_t* sites,
                                          const int32_t* replicates, uint64_t seed, int64_t first_replicate,
                                          double* out_ll, double* out_pattern_ll, double* out_table,
                                          int32_t* out_counts, double* out_mean, double* out_c, int32_t* out_best) {
  if (!e) return fail("null engine");
  if (!e->shards.empty() && e->shard_mode != MI_SHARD_TREES) return fail(kTopoPatternShards);
  // (a handle of ONE shard has every tree's row on one device: that shard takes the call)
  if (e->shards.size() > 1) return fail(kTopoSharded);
  e = first_engine(e);
  if (e->s == kAa) return fail(kPatternLl4State);
  if (!parent_ids || !bl) return fail("null tree arrays");
  if (e->param_count > 0 && !params) return fail("null parameter matrix");
  int maxB = 0;
  if (check_topo_shape(T, e->P, K, sites, replicates, &maxB)) return 1;
  if (!out_ll || !out_table || !out_counts) return fail("null output pointer");
  enum { kLl, kS, kTable, kCounts, kMean, kC, kBest };
  const size_t P = e->P, B0 = (size_t)replicates[0];
  const std::vector<int64_t> sites_v(sites, sites + K);
  const std::vector<int32_t> reps_v(replicates, replicates + K);
  HostCall c;
  c.T = T;
  c.in = tree_inputs(e, parent_ids, bl, params);
  c.out = {per_tree(out_ll, 1),          per_tree(out_pattern_ll, P), per_tree(out_table, kTopoColumns),
           fixed(out_counts, (size_t)K * T), per_tree(out_mean, 1),  fixed(out_c, B0 * T),
           fixed(out_best, B0)};
  c.enqueue = [=](mi_engine* e, int T, const HostArray* in, const HostArray* out) {
    // (a matrix nobody downloads stays in the engine's workspace)
    if (!out[kS].dev && e->rell_s.ensure(sizeof(double) * (size_t)T * P)) return 1;
    double* d_s = out[kS].dev ? out[kS].at<double>() : e->rell_s.as<double>();
    if (mi_engine_pattern_log_likelihoods_unrooted_device(e, e->stream, T, in[kInParent].at<const int32_t>(),
                                                          in[kInBl].at<const double>(), params_on_device(e, in),
                                                          rescaling, out[kLl].at<double>(), d_s))
      return 1;
    // (the engine's own pattern weights: what is no integer site count goes to the status word)
    TopoCall d;
    d.T = T;
    d.P = (int)P;
    d.K = K;
    d.s = d_s;
    d.w = e->weights.as<const double>();
    d.sites = sites_v.data();
    d.replicates = reps_v.data();
    d.seed = seed;
    d.first_replicate = first_replicate;
    d.out_table = out[kTable].at<double>();
    d.out_counts = out[kCounts].at<int32_t>();
    d.out_mean = out[kMean].at<double>();
    d.out_c = out[kC].at<double>();
    d.out_best = out[kBest].at<int32_t>();
    return run_topo_device(e, e->stream, d);
  };
  return run_on_engine(e, c);
}

}  // extern "C"
