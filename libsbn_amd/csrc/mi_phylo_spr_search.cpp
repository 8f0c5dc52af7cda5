// SPR moves on the device and the SPR hill-climbing search (mi_engine_spr_apply_unrooted*,
// mi_engine_spr_search_unrooted*).  The search follows the NNI search
// (mi_phylo_nni_search.cpp) step for step: a host-driven loop of rounds -- the branch-length
// optimisation (run_branch_opt_device) and the SPR scan (run_spr_device) on the packed set of
// trees that are still searching, then one step kernel that moves or stops every tree.  Once per
// round the host reads one word: the trees that moved.  It stops at 0, and packs the searching
// trees to the front when fewer than half of the packed set are left.  Nothing else is
// downloaded, uploaded or allocated inside the loop.
#include <cmath>

#include "mi_phylo_engine.h"

namespace {

constexpr int kSprSearchMaxMoves = 10000;
const char kSearch4State[] = "the SPR search is 4-state only";
const char kSearchPatternShards[] =
    "pattern-sharded engines do not run the SPR search (every optimiser iteration would need a sum "
    "across the shards): use MI_SHARD_TREES or a single engine";

// ---- taking moves ----

int reserve_spr_apply(mi_engine* e, int T) {
  if (e->spr_apply_ws.ensure(std::max<size_t>(sizeof(int32_t) * (size_t)T * spr_apply_ws_words(e->n), 256))) return 1;
  return e->status.ensure(sizeof(int32_t) * kStatusWords);
}

int run_spr_apply_device(mi_engine* e, hipStream_t s, int T, const int32_t* parent_ids, const double* bl,
                         const int32_t* moves, int32_t* out_parent_ids, double* out_bl) {
  HIP_TRY(hipSetDevice(e->spec.device));
  if (T <= 0) return fail("tree_count must be positive");
  if (!parent_ids || !bl || !moves) return fail("null tree / move arrays");
  if (!out_parent_ids || !out_bl) return fail("null output pointer");
  if (reserve_spr_apply(e, T)) return 1;
  SprApplyArgs a{};
  a.n = e->n;
  a.T = T;
  a.parent_ids = parent_ids;
  a.bl = bl;
  a.moves = moves;
  a.ws = e->spr_apply_ws.as<int32_t>();
  a.status = e->status.as<int32_t>();
  a.out_parent_ids = out_parent_ids;
  a.out_bl = out_bl;
  launch_spr_apply(a, s);
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- the search ----

struct SprSearchCall {
  int T = 0;
  bool rescaling = false;
  const int32_t* parent_ids = nullptr;
  const double* start = nullptr;
  const double* params = nullptr;
  const mi_spr_search_options* options = nullptr;
  int32_t* out_pid = nullptr;
  double* out_bl = nullptr;
  double* out_ll = nullptr;
  double* out_best_delta = nullptr;  // may be null
  int32_t* out_move_count = nullptr;
  int32_t* out_move_log = nullptr;  // may be null
  double* out_move_gain = nullptr;  // may be null
  int32_t* out_status = nullptr;
  int32_t* out_opt_status = nullptr;  // may be null
};

mi_spr_search_options search_defaults() {
  mi_spr_search_options o{};
  o.max_moves = 100;
  o.pack_active = 1;
  o.min_gain = 1e-3;
  o.radius = 0;
  o.branch_opt = kBranchOptDefaults;
  return o;
}

bool all_zero(const mi_branch_opt_options& b) {
  return b.max_iterations == 0 && b.check_interval == 0 && b.pack_active == 0 && b.tolerance == 0.0 &&
         b.min_length == 0.0 && b.max_length == 0.0;
}

// the options a call runs with (branch_opt of zeros: the optimiser's defaults), checked
int search_options(const mi_engine* e, const mi_spr_search_options* given, mi_spr_search_options* out) {
  mi_spr_search_options o = given ? *given : search_defaults();
  if (all_zero(o.branch_opt)) o.branch_opt = kBranchOptDefaults;
  if (o.max_moves < 0 || o.max_moves > kSprSearchMaxMoves)
    return fail("SPR search: max_moves must be in 0.." + std::to_string(kSprSearchMaxMoves));
  if (!(o.min_gain >= 0.0)) return fail("SPR search: min_gain must be >= 0");
  if (o.radius < 0)
    return fail("SPR search: radius must be 0 (every move) or positive, not " + std::to_string(o.radius));
  if (check_branch_opt_options(o.branch_opt)) return 1;
  // (a sharded handle owns no scan: its shards check the shape)
  if (e->shards.empty() && check_spr_shape(e, o.radius)) return 1;
  *out = o;
  return 0;
}

// the pieces of e->spr_search_ws for a batch of T trees, 256-byte aligned
struct SprSearchWorkspace {
  int32_t *pid[2], *pk_pid, *opt_status, *best, *target, *map[2], *active, *apply_ws;
  double *bl[2], *pk_bl, *pk_params, *opt_bl, *opt_ll, *delta;
  size_t bytes;
  SprSearchWorkspace(const mi_engine* e, int T, char* base) {
    const size_t N = e->N, t = (size_t)T;
    size_t off = 0;
    auto take = [&](size_t b) {
      char* p = base + off;
      off += (b + 255) & ~(size_t)255;
      return p;
    };
    auto f64 = [&](size_t count) { return reinterpret_cast<double*>(take(sizeof(double) * count)); };
    auto i32 = [&](size_t count) { return reinterpret_cast<int32_t*>(take(sizeof(int32_t) * count)); };
    for (int h = 0; h < 2; h++) {
      pid[h] = i32(t * (N - 2));
      bl[h] = f64(t * (N - 1));
    }
    pk_pid = i32(t * (N - 2));
    pk_bl = f64(t * (N - 1));
    pk_params = f64(t * std::max(e->param_count, 1));
    opt_bl = f64(t * (N - 1));
    opt_ll = f64(t);
    opt_status = i32(t);
    delta = f64(t * (N - 2) * 2);   // the scan's best_delta
    target = i32(t * (N - 2) * 2);  // ... and best_target, which the scan always writes
    best = i32(t * 3);
    map[0] = i32(t);
    map[1] = i32(t);
    active = i32(kSprSearchMaxMoves + 1);
    apply_ws = i32(std::max<size_t>(t * spr_apply_ws_words(e->n), 1));
    bytes = off;
  }
};

int reserve_spr_search(mi_engine* e, int T) {
  if (reserve_branch_opt(e, T)) return 1;
  if (reserve_spr_calls(e, T)) return 1;
  return e->spr_search_ws.ensure(SprSearchWorkspace(e, T, nullptr).bytes);
}

int run_spr_search_device(mi_engine* e, hipStream_t s, const SprSearchCall& c) {
  HIP_TRY(hipSetDevice(e->spec.device));
  if (e->s == kAa) return fail(kSearch4State);
  if (c.T <= 0) return fail("tree_count must be positive");
  if (!c.parent_ids || !c.start) return fail("null tree arrays");
  if (!c.out_pid || !c.out_bl || !c.out_ll || !c.out_move_count || !c.out_status) return fail("null output pointer");
  if (e->param_count > 0 && !c.params) return fail("null parameter matrix");
  mi_spr_search_options o;
  if (search_options(e, c.options, &o)) return 1;
  const int T = c.T, n = e->n, N = e->N;
  if (reserve_spr_search(e, T)) return 1;
  const SprSearchWorkspace w(e, T, e->spr_search_ws.as<char>());
  const bool pack = o.pack_active != 0;
  const size_t np = (size_t)N - 2, nl = (size_t)N - 1;
  HIP_TRY(hipMemcpyAsync(w.pid[0], c.parent_ids, sizeof(int32_t) * T * np, hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemcpyAsync(w.bl[0], c.start, sizeof(double) * T * nl, hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemsetAsync(w.active, 0, sizeof(int32_t) * ((size_t)o.max_moves + 1), s));
  // (the maps are written before they are read; zeroed so that no index is ever out of range)
  HIP_TRY(hipMemsetAsync(w.map[0], 0, sizeof(int32_t) * (size_t)T, s));
  HIP_TRY(hipMemsetAsync(w.map[1], 0, sizeof(int32_t) * (size_t)T, s));
  // (three taxa: no scan runs, the step kernel reads "no move")
  HIP_TRY(hipMemsetAsync(w.best, 0xff, sizeof(int32_t) * (size_t)T * 3, s));
  HIP_TRY(hipMemsetAsync(c.out_status, 0xff, sizeof(int32_t) * (size_t)T, s));  // kSprSearchActive
  HIP_TRY(hipMemsetAsync(c.out_move_count, 0, sizeof(int32_t) * (size_t)T, s));
  if (c.out_move_log && o.max_moves)
    HIP_TRY(hipMemsetAsync(c.out_move_log, 0xff, sizeof(int32_t) * (size_t)T * o.max_moves * 3, s));
  if (c.out_move_gain && o.max_moves) HIP_TRY(hipMemsetAsync(c.out_move_gain, 0, sizeof(double) * (size_t)T * o.max_moves, s));

  SprSearchStepArgs st{};
  st.n = n;
  st.max_moves = o.max_moves;
  st.min_gain = o.min_gain;
  st.map = nullptr;
  st.opt_bl = w.opt_bl;
  st.opt_ll = w.opt_ll;
  st.opt_status = w.opt_status;
  st.delta = w.delta;
  st.best = w.best;
  st.pk_pid = w.pk_pid;
  st.pk_bl = w.pk_bl;
  st.ws = w.apply_ws;
  st.engine_status = e->status.as<int32_t>();
  st.out_pid = c.out_pid;
  st.out_bl = c.out_bl;
  st.out_ll = c.out_ll;
  st.out_best_delta = c.out_best_delta;
  st.move_count = c.out_move_count;
  st.move_log = c.out_move_log;
  st.move_gain = c.out_move_gain;
  st.status = c.out_status;
  st.out_opt_status = c.out_opt_status;

  int count = T, half = 0, which = 0, rounds = 0;
  int64_t evals = 0, moves = 0;
  int launches = 0;
  std::string hess_path, batches;  // "<trees>x<rounds>,..."
  const char* hess_kernel = "";
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
  for (int r = 0; r <= o.max_moves; r++) {  // (a searching tree has moved once per round)
    const bool packed = st.map != nullptr;
    const int32_t* pid_in = packed ? w.pk_pid : w.pid[half];
    const double* params_in = packed && e->param_count > 0 ? w.pk_params : c.params;
    BranchOptCall b;
    b.T = count;
    b.route_T = T;
    b.rescaling = c.rescaling;
    b.parent_ids = pid_in;
    b.start = packed ? w.pk_bl : w.bl[half];
    b.params = params_in;
    b.options = &o.branch_opt;
    b.out_bl = w.opt_bl;
    b.out_ll = w.opt_ll;
    b.out_status = w.opt_status;
    if (run_branch_opt_device(e, s, b)) return 1;
    evals += e->last_evals;
    launches += e->last_walk_launches;
    hess_path = e->last_path.substr(0, e->last_path.find(" opt iters="));
    hess_kernel = e->dominant;
    if (n > 3) {
      DeviceCall d;
      d.T = count;
      d.route_T = T;
      d.rescaling = c.rescaling;
      d.parent_ids = pid_in;
      d.bl = w.opt_bl;
      d.params = params_in;
      d.spr_radius = o.radius;
      d.out_spr_target = w.target;
      d.out_spr_delta = w.delta;
      d.out_spr_move = w.best;
      if (run_spr_device(e, s, d)) return 1;
      evals += count;
      launches += e->last_walk_launches;
    }
    st.count = count;
    st.round = r;
    st.cur_pid = w.pid[half];
    st.cur_bl = w.bl[half];
    st.next_pid = w.pid[half ^ 1];
    st.next_bl = w.bl[half ^ 1];
    st.active = w.active + r;
    launch_spr_search_step(st, s);
    rounds++;
    note(count);
    HIP_TRY(hipMemcpyAsync(e->opt_word, w.active + r, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const int active = *e->opt_word;
    if (active <= 0) break;
    moves += active;
    if (pack && 2 * active < count) {
      BranchOptPackArgs pa{};
      pa.N = N;
      pa.count = active;
      pa.param_count = e->param_count;
      pa.map = w.map[which];
      pa.parent_ids = w.pid[half ^ 1];
      pa.params = c.params;
      pa.trial_full = w.bl[half ^ 1];
      pa.pk_parent = w.pk_pid;
      pa.pk_trial = w.pk_bl;
      pa.pk_params = w.pk_params;
      launch_branch_opt_pack(pa, count, st.map, c.out_status, s);
      st.map = pa.map;
      which ^= 1;
      count = active;
    }
    half ^= 1;
  }
  note(0);
  e->dominant = hess_kernel;
  e->last_path = hess_path + " spr-search radius=" + std::to_string(o.radius) + " rounds=" + std::to_string(rounds) +
                 " moves=" + std::to_string(moves) + " batches=" + batches + (pack ? "" : " pack=off");
  e->last_evals = evals;
  e->last_grad_evals = evals;
  e->last_walk_launches = launches;
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" {

int32_t mi_engine_spr_apply_unrooted(mi_engine* e, int32_t T, const int32_t* parent_ids, const double* bl,
                                     const int32_t* moves, int32_t* out_parent_ids, double* out_bl) {
  if (!e) return fail("null engine");
  if (T <= 0) return fail("tree_count must be positive");
  if (!parent_ids || !bl || !moves) return fail("null tree / move arrays");
  if (!out_parent_ids || !out_bl) return fail("null output pointer");
  const size_t np = 2 * e->n - 3;
  HostCall c;
  c.T = T;
  c.in = {per_tree(parent_ids, np), per_tree(bl, np + 1), per_tree(moves, 3)};
  c.out = {per_tree(out_parent_ids, np), per_tree(out_bl, np + 1)};
  c.enqueue = [](mi_engine* e, int T, const HostArray* in, const HostArray* out) {
    return run_spr_apply_device(e, e->stream, T, in[0].at<const int32_t>(), in[1].at<const double>(),
                                in[2].at<const int32_t>(), out[0].at<int32_t>(), out[1].at<double>());
  };
  // (a move needs no alignment: a sharded handle of either kind lets its first shard take them all)
  return run_on_engine(first_engine(e), c);
}

int32_t mi_engine_spr_apply_unrooted_device(mi_engine* e, void* stream, int32_t T, const int32_t* parent_ids,
                                            const double* bl, const int32_t* moves, int32_t* out_parent_ids,
                                            double* out_bl) {
  if (!e) return fail("null engine");
  if (!e->shards.empty()) return fail(kShardedDeviceCall);
  return run_spr_apply_device(e, pick_stream(e, stream), T, parent_ids, bl, moves, out_parent_ids, out_bl);
}

// The host-pointer form of the search: inputs up in one copy, the rounds, outputs back in one copy
// and the call's one error check.  Each tree shard of a handle searches from its block of trees,
// one shard after the other (the loop synchronises its device every round).
int32_t mi_engine_spr_search_unrooted(mi_engine* e, int32_t T, const int32_t* parent_ids, const double* start,
                                      const double* params, int32_t rescaling,
                                      const mi_spr_search_options* options, int32_t* out_parent_ids,
                                      double* out_bl, double* out_ll, double* out_best_delta,
                                      int32_t* out_move_count, int32_t* out_move_log, double* out_move_gain,
                                      int32_t* out_status, int32_t* out_opt_status) {
  if (!e) return fail("null engine");
  if (e->s == kAa) return fail(kSearch4State);
  if (T <= 0) return fail("tree_count must be positive");
  mi_spr_search_options o;
  if (search_options(e, options, &o)) return 1;
  if (!e->shards.empty() && e->shard_mode != MI_SHARD_TREES) return fail(kSearchPatternShards);
  if (!parent_ids || !start) return fail("null tree arrays");
  if (!out_parent_ids || !out_bl || !out_ll || !out_move_count || !out_status) return fail("null output pointer");
  if (e->param_count > 0 && !params) return fail("null parameter matrix");
  enum { kPid, kBl, kLl, kDelta, kCount, kLog, kGain, kStatus, kOpt };
  const size_t np = 2 * e->n - 3;
  HostCall c;
  c.T = T;
  c.one_by_one = true;
  c.in = tree_inputs(e, parent_ids, start, params);
  c.out = {per_tree(out_parent_ids, np),          per_tree(out_bl, np + 1),
           per_tree(out_ll, 1),                   per_tree(out_best_delta, 1),
           per_tree(out_move_count, 1),           per_tree(out_move_log, (size_t)o.max_moves * 3),
           per_tree(out_move_gain, o.max_moves),  per_tree(out_status, 1),
           per_tree(out_opt_status, 1)};
  c.enqueue = [=](mi_engine* e, int T, const HostArray* in, const HostArray* out) {
    SprSearchCall d;
    d.T = T;
    d.rescaling = rescaling != 0;
    d.parent_ids = in[kInParent].at<const int32_t>();
    d.start = in[kInBl].at<const double>();
    d.params = params_on_device(e, in);
    d.options = options;
    d.out_pid = out[kPid].at<int32_t>();
    d.out_bl = out[kBl].at<double>();
    d.out_ll = out[kLl].at<double>();
    d.out_best_delta = out[kDelta].at<double>();
    d.out_move_count = out[kCount].at<int32_t>();
    d.out_move_log = out[kLog].at<int32_t>();
    d.out_move_gain = out[kGain].at<double>();
    d.out_status = out[kStatus].at<int32_t>();
    d.out_opt_status = out[kOpt].at<int32_t>();
    return run_spr_search_device(e, e->stream, d);
  };
  return run_host_call(e, c);
}

int32_t mi_engine_spr_search_unrooted_device(mi_engine* e, void* stream, int32_t T, const int32_t* parent_ids,
                                             const double* start, const double* params, int32_t rescaling,
                                             const mi_spr_search_options* options, int32_t* out_parent_ids,
                                             double* out_bl, double* out_ll, double* out_best_delta,
                                             int32_t* out_move_count, int32_t* out_move_log,
                                             double* out_move_gain, int32_t* out_status,
                                             int32_t* out_opt_status) {
  if (!e) return fail("null engine");
  if (e->s == kAa) return fail(kSearch4State);
  if (!e->shards.empty()) return fail(kShardedDeviceCall);
  SprSearchCall c;
  c.T = T;
  c.rescaling = rescaling != 0;
  c.parent_ids = parent_ids;
  c.start = start;
  c.params = params;
  c.options = options;
  c.out_pid = out_parent_ids;
  c.out_bl = out_bl;
  c.out_ll = out_ll;
  c.out_best_delta = out_best_delta;
  c.out_move_count = out_move_count;
  c.out_move_log = out_move_log;
  c.out_move_gain = out_move_gain;
  c.out_status = out_status;
  c.out_opt_status = out_opt_status;
  return run_spr_search_device(e, pick_stream(e, stream), c);
}

int32_t mi_engine_reserve_spr_search(mi_engine* e, int32_t tree_count) {
  if (!e) return fail("null engine");
  if (tree_count <= 0) return fail("tree_count must be positive");
  if (e->s == kAa) return fail(kSearch4State);
  if (!e->shards.empty()) {
    if (e->shard_mode != MI_SHARD_TREES) return fail(kSearchPatternShards);
    return for_each_shard(e, tree_count, mi_engine_reserve_spr_search);
  }
  if (check_spr_shape(e, 0)) return 1;
  HIP_TRY(hipSetDevice(e->spec.device));
  if (reserve_spr_apply(e, tree_count)) return 1;
  return reserve_spr_search(e, tree_count);
}

}  // extern "C"
