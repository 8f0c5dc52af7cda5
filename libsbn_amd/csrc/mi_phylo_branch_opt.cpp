// Maximum-likelihood branch lengths (mi_engine_optimize_branch_lengths_unrooted*).
// A host-driven loop of Hessian passes (run_hessian_device on the packed trial points) and
// step kernels.  Every check_interval passes the host reads one word: the trees still active.
// It stops at 0, and packs the active trees to the front when fewer than half of the packed
// set are left.  Nothing else is synchronised, downloaded or allocated inside the loop.
#include <cmath>

#include "mi_phylo_engine.h"

namespace {

constexpr int kBranchOptMaxIterations = 1000;

// the pieces of e->opt_ws for a batch of T trees, 256-byte aligned
struct BranchOptWorkspace {
  double *trial, *trial_full, *tr_ll, *tr_g, *tr_h, *tr_s, *g, *h, *s, *alpha, *pk_params;
  int32_t *map[2], *pk_parent, *evals, *active;
  size_t bytes;
  BranchOptWorkspace(const mi_engine* e, int T, char* base) {
    const size_t N = e->N, t = (size_t)T;
    size_t off = 0;
    auto take = [&](size_t b) {
      char* p = base + off;
      off += (b + 255) & ~(size_t)255;
      return p;
    };
    auto f64 = [&](size_t count) { return reinterpret_cast<double*>(take(sizeof(double) * count)); };
    auto i32 = [&](size_t count) { return reinterpret_cast<int32_t*>(take(sizeof(int32_t) * count)); };
    trial = f64(t * (N - 1));
    trial_full = f64(t * (N - 1));
    tr_ll = f64(t);
    tr_g = f64(t * N);
    tr_h = f64(t * N);
    tr_s = f64(t * N);
    g = f64(t * N);
    h = f64(t * N);
    s = f64(t * N);
    alpha = f64(t);
    pk_params = f64(t * std::max(e->param_count, 1));
    map[0] = i32(t);
    map[1] = i32(t);
    pk_parent = i32(t * (N - 2));
    evals = i32(t);
    active = i32(kBranchOptMaxIterations);
    bytes = off;
  }
};

}  // namespace

const mi_branch_opt_options kBranchOptDefaults = {100, 4, 1, 1e-6, 1e-8, 10.0, {0, 0, 0, 0}};

int reserve_branch_opt(mi_engine* e, int T) {
  if (reserve_hessian_calls(e, T)) return 1;
  if (e->opt_ws.ensure(BranchOptWorkspace(e, T, nullptr).bytes)) return 1;
  if (!e->opt_word) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&e->opt_word.h), 256, hipHostMallocDefault));
  return 0;
}

int check_branch_opt_options(const mi_branch_opt_options& o) {
  if (o.max_iterations < 1 || o.max_iterations > kBranchOptMaxIterations)
    return fail("branch-length optimisation: max_iterations must be in 1.." +
                std::to_string(kBranchOptMaxIterations));
  if (o.check_interval < 1) return fail("branch-length optimisation: check_interval must be positive");
  if (!(o.tolerance >= 0.0)) return fail("branch-length optimisation: tolerance must be >= 0");
  if (!(o.min_length >= 0.0) || !(o.max_length >= o.min_length) || !(o.max_length < INFINITY))
    return fail("branch-length optimisation: need 0 <= min_length <= max_length < inf");
  return 0;
}

int run_branch_opt_device(mi_engine* e, hipStream_t s, const BranchOptCall& c) {
  HIP_TRY(hipSetDevice(e->spec.device));
  if (e->s == kAa) return fail(kHessian4State);
  if (c.T <= 0) return fail("tree_count must be positive");
  if (!c.parent_ids || !c.start) return fail("null tree arrays");
  if (!c.out_bl || !c.out_ll || !c.out_status) return fail("null output pointer");
  if (e->param_count > 0 && !c.params) return fail("null parameter matrix");
  const mi_branch_opt_options o = c.options ? *c.options : kBranchOptDefaults;
  if (check_branch_opt_options(o)) return 1;
  const int T = c.T, N = e->N;
  if (reserve_branch_opt(e, T)) return 1;
  const BranchOptWorkspace w(e, T, e->opt_ws.as<char>());
  const bool pack = o.pack_active != 0;
  HIP_TRY(hipMemsetAsync(w.active, 0, sizeof(int32_t) * o.max_iterations, s));
  // (the maps are written before they are read; zeroed so that no index is ever out of range)
  if (pack) {
    HIP_TRY(hipMemsetAsync(w.map[0], 0, sizeof(int32_t) * (size_t)T, s));
    HIP_TRY(hipMemsetAsync(w.map[1], 0, sizeof(int32_t) * (size_t)T, s));
  }
  BranchOptArgs st{};
  st.N = N;
  st.T = T;
  st.count = T;
  st.evals_max = o.max_iterations;
  st.tol = o.tolerance;
  st.tmin = o.min_length;
  st.tmax = o.max_length;
  st.map = nullptr;
  st.tr_ll = w.tr_ll;
  st.tr_g = w.tr_g;
  st.tr_h = w.tr_h;
  st.tr_s = w.tr_s;
  st.trial = w.trial;
  st.trial_full = pack ? w.trial_full : nullptr;
  st.bl = c.out_bl;
  st.ll = c.out_ll;
  st.g = c.out_g ? c.out_g : w.g;
  st.h = c.out_h ? c.out_h : w.h;
  st.s = w.s;
  st.alpha = w.alpha;
  st.evals = c.out_iters ? c.out_iters : w.evals;
  st.status = c.out_status;
  st.active = w.active;
  launch_branch_opt_init(st, c.start, s);
  DeviceCall d;
  d.T = T;
  d.route_T = c.route_T ? c.route_T : T;
  d.rescaling = c.rescaling;
  d.parent_ids = c.parent_ids;
  d.bl = w.trial;
  d.params = c.params;
  d.out_ll = w.tr_ll;
  d.out_branch = w.tr_g;
  d.out_hess = w.tr_h;
  d.out_gsq = w.tr_s;
  int64_t evals = 0;
  int passes = 0, launches = 0, which = 0;
  std::string batches;  // "<trees>x<passes>,..."
  int run_trees = 0, run_len = 0;
  auto note = [&](int trees) {
    if (trees == run_trees) {
      run_len++;
      return;
    }
    if (run_len) batches += (batches.empty() ? "" : ",") + std::to_string(run_trees) + "x" + std::to_string(run_len);
    run_trees = trees;
    run_len = trees ? 1 : 0;
  };
  for (int it = 0; it < o.max_iterations; it++) {
    if (run_hessian_device(e, s, d)) return 1;
    launches += e->last_walk_launches;
    st.pass = it;
    launch_branch_opt_step(st, s);
    passes++;
    evals += d.T;
    note(d.T);
    if (it + 1 == o.max_iterations) break;  // (every tree has stopped by now)
    if ((it + 1) % o.check_interval) continue;
    HIP_TRY(hipMemcpyAsync(e->opt_word, w.active + it, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const int active = *e->opt_word;
    if (active <= 0) break;
    if (pack && 2 * active < d.T) {
      BranchOptPackArgs pa{};
      pa.N = N;
      pa.count = active;
      pa.param_count = e->param_count;
      pa.map = w.map[which];
      pa.parent_ids = c.parent_ids;
      pa.params = c.params;
      pa.trial_full = w.trial_full;
      pa.pk_parent = w.pk_parent;
      pa.pk_trial = w.trial;
      pa.pk_params = w.pk_params;
      launch_branch_opt_pack(pa, d.T, st.map, c.out_status, s);
      st.map = pa.map;
      st.count = active;
      which ^= 1;
      d.T = active;
      d.parent_ids = w.pk_parent;
      if (e->param_count > 0) d.params = w.pk_params;
    }
  }
  note(0);
  e->last_path += " opt iters=" + std::to_string(passes) + " evals=" + std::to_string(evals) +
                  " batches=" + batches + (pack ? "" : " pack=off");
  e->last_evals = evals;
  e->last_grad_evals = evals;
  e->last_walk_launches = launches;
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" {

// The host-pointer form: inputs up in one copy, the loop (which synchronises at its check
// points), outputs back in one copy and the call's one error check.  Each tree shard of a handle
// optimises its block of trees independently, one shard after the other.
int32_t mi_engine_optimize_branch_lengths_unrooted(
    mi_engine* e, int32_t T, const int32_t* parent_ids, const double* start, const double* params,
    int32_t rescaling, const mi_branch_opt_options* options, double* out_bl, double* out_ll,
    double* out_g, double* out_h, int32_t* out_iters, int32_t* out_status) {
  if (!e) return fail("null engine");
  if (e->s == kAa) return fail(kHessian4State);
  if (T <= 0) return fail("tree_count must be positive");
  if (check_branch_opt_options(options ? *options : kBranchOptDefaults)) return 1;
  if (!e->shards.empty()) {
    if (e->shard_mode != MI_SHARD_TREES)
      return fail("pattern-sharded engines do not optimise branch lengths (every iteration would "
                  "need a sum across the shards): use MI_SHARD_TREES or a single engine");
    if (!parent_ids || !start || !out_bl || !out_ll || !out_status) return fail("null tree / output pointer");
  }
  if (!parent_ids || !start) return fail("null tree arrays");
  if (!out_bl || !out_ll || !out_status) return fail("null output pointer");
  if (e->param_count > 0 && !params) return fail("null parameter matrix");
  enum { kBl, kLl, kG, kH, kIters, kStatus };
  HostCall c;
  c.T = T;
  c.one_by_one = true;
  c.in = tree_inputs(e, parent_ids, start, params);
  c.out = {per_tree(out_bl, e->N - 1), per_tree(out_ll, 1), per_tree(out_g, e->N),
           per_tree(out_h, e->N),      per_tree(out_iters, 1), per_tree(out_status, 1)};
  c.enqueue = [=](mi_engine* e, int T, const HostArray* in, const HostArray* out) {
    BranchOptCall d;
    d.T = T;
    d.rescaling = rescaling != 0;
    d.parent_ids = in[kInParent].at<const int32_t>();
    d.start = in[kInBl].at<const double>();
    d.params = params_on_device(e, in);
    d.options = options;
    d.out_bl = out[kBl].at<double>();
    d.out_ll = out[kLl].at<double>();
    d.out_g = out[kG].at<double>();
    d.out_h = out[kH].at<double>();
    d.out_iters = out[kIters].at<int32_t>();
    d.out_status = out[kStatus].at<int32_t>();
    return run_branch_opt_device(e, e->stream, d);
  };
  return run_host_call(e, c);
}

int32_t mi_engine_optimize_branch_lengths_unrooted_device(
    mi_engine* e, void* stream, int32_t T, const int32_t* parent_ids, const double* start,
    const double* params, int32_t rescaling, const mi_branch_opt_options* options, double* out_bl,
    double* out_ll, double* out_g, double* out_h, int32_t* out_iters, int32_t* out_status) {
  if (!e) return fail("null engine");
  if (e->s == kAa) return fail(kHessian4State);
  if (!e->shards.empty()) return fail(kShardedDeviceCall);
  BranchOptCall c;
  c.T = T;
  c.rescaling = rescaling != 0;
  c.parent_ids = parent_ids;
  c.start = start;
  c.params = params;
  c.options = options;
  c.out_bl = out_bl;
  c.out_ll = out_ll;
  c.out_g = out_g;
  c.out_h = out_h;
  c.out_iters = out_iters;
  c.out_status = out_status;
  return run_branch_opt_device(e, pick_stream(e, stream), c);
}

int32_t mi_engine_reserve_branch_opt(mi_engine* e, int32_t tree_count) {
  if (!e) return fail("null engine");
  if (tree_count <= 0) return fail("tree_count must be positive");
  if (e->s == kAa) return fail(kHessian4State);
  if (!e->shards.empty()) {
    if (e->shard_mode != MI_SHARD_TREES) return fail("pattern-sharded engines do not optimise branch lengths");
    return for_each_shard(e, tree_count, mi_engine_reserve_branch_opt);
  }
  HIP_TRY(hipSetDevice(e->spec.device));
  return reserve_branch_opt(e, tree_count);
}

}  // extern "C"
