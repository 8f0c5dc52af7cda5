// Moves on the device and the hill-climbing searches, NNI and SPR (mi_engine_{nni,spr}_apply_unrooted*,
// mi_engine_{nni,spr}_search_unrooted*).  One driver serves both kinds of
// move; a MoveKind says what differs.  The search is a host-driven loop of rounds: the
// branch-length optimisation (run_branch_opt_device) and the neighbourhood scan (run_nni_device /
// run_spr_device) on the packed set of trees that are still searching, then one step kernel
// that moves or stops every tree.  Once per round the host reads one word: the trees that
// moved.  It stops at 0, and packs the searching trees to the front when fewer than half of the
// packed set are left.  Nothing else is downloaded, uploaded or allocated inside the loop.
#include <cmath>

#include "mi_phylo_engine.h"

namespace {

constexpr int kSearchMaxMoves = 10000;

struct SearchWorkspace;
// What differs between the two kinds of move.  The buffers stay apart: an apply call may sit in a
// captured graph, and growing a buffer shared with the other kind would free what that graph reads.
struct MoveKind {
  const char *name, *tag;  // in messages; in the path string
  // the SPR scan's: a radius and a shape to check, best targets beside the deltas, and no scan
  // of three taxa (the NNI scan runs there and reports -1 itself)
  bool spr;
  int width;  // words of a move: the code 2 v + i, or the triple (s, dir, f)
  size_t (*apply_ws_words)(int n);
  Buffer mi_engine::*apply_ws, mi_engine::*search_ws;
  int (*reserve_scan)(mi_engine* e, int T);
  // a round's scan: d has the trees, the lengths and the route
  int (*scan)(mi_engine* e, hipStream_t s, DeviceCall& d, const SearchWorkspace& w, int radius);
  void (*launch_apply)(const MoveApplyArgs& a, hipStream_t s);
  void (*launch_step)(const SearchStepArgs& a, hipStream_t s);
};

std::string four_state_only(const MoveKind& k) { return std::string("the ") + k.name + " search is 4-state only"; }
std::string no_pattern_shards(const MoveKind& k) {
  return std::string("pattern-sharded engines do not run the ") + k.name +
         " search (every optimiser iteration would need a sum across the shards): use MI_SHARD_TREES or a single engine";
}

// ---- taking moves ----

int reserve_apply(const MoveKind& k, mi_engine* e, int T) {
  if ((e->*k.apply_ws).ensure(std::max<size_t>(sizeof(int32_t) * (size_t)T * k.apply_ws_words(e->n), 256))) return 1;
  return e->status.ensure(sizeof(int32_t) * kStatusWords);
}

int run_apply_device(const MoveKind& k, mi_engine* e, hipStream_t s, int T, const int32_t* parent_ids,
                     const double* bl, const int32_t* moves, int32_t* out_parent_ids, double* out_bl) {
  HIP_TRY(hipSetDevice(e->spec.device));
  if (T <= 0) return fail("tree_count must be positive");
  if (!parent_ids || !bl || !moves) return fail("null tree / move arrays");
  if (!out_parent_ids || !out_bl) return fail("null output pointer");
  if (reserve_apply(k, e, T)) return 1;
  MoveApplyArgs a{};
  a.n = e->n;
  a.T = T;
  a.parent_ids = parent_ids;
  a.bl = bl;
  a.moves = moves;
  a.ws = (e->*k.apply_ws).as<int32_t>();
  a.status = e->status.as<int32_t>();
  a.out_parent_ids = out_parent_ids;
  a.out_bl = out_bl;
  k.launch_apply(a, s);
  HIP_TRY(hipGetLastError());
  return 0;
}

int apply_host(const MoveKind& k, mi_engine* e, int32_t T, const int32_t* parent_ids, const double* bl,
               const int32_t* moves, int32_t* out_parent_ids, double* out_bl) {
  if (!e) return fail("null engine");
  if (T <= 0) return fail("tree_count must be positive");
  if (!parent_ids || !bl || !moves) return fail("null tree / move arrays");
  if (!out_parent_ids || !out_bl) return fail("null output pointer");
  const size_t np = 2 * e->n - 3;
  HostCall c;
  c.T = T;
  c.in = {per_tree(parent_ids, np), per_tree(bl, np + 1), per_tree(moves, k.width)};
  c.out = {per_tree(out_parent_ids, np), per_tree(out_bl, np + 1)};
  c.enqueue = [&k](mi_engine* e, int T, const HostArray* in, const HostArray* out) {
    return run_apply_device(k, e, e->stream, T, in[0].at<const int32_t>(), in[1].at<const double>(),
                            in[2].at<const int32_t>(), out[0].at<int32_t>(), out[1].at<double>());
  };
  // (a move needs no alignment: a sharded handle of either kind lets its first shard take them all)
  return run_on_engine(first_engine(e), c);
}

int apply_device(const MoveKind& k, mi_engine* e, void* stream, int32_t T, const int32_t* parent_ids,
                 const double* bl, const int32_t* moves, int32_t* out_parent_ids, double* out_bl) {
  if (!e) return fail("null engine");
  if (!e->shards.empty()) return fail(kShardedDeviceCall);
  return run_apply_device(k, e, pick_stream(e, stream), T, parent_ids, bl, moves, out_parent_ids, out_bl);
}

// ---- the search ----

// the options of either public struct (NULL: the defaults)
struct SearchOptions {
  int max_moves = 100, pack_active = 1;
  double min_gain = 1e-3;
  int radius = 0;
  mi_branch_opt_options branch_opt = kBranchOptDefaults;
};
SearchOptions options_of(const mi_nni_search_options* g) {
  return g ? SearchOptions{g->max_moves, g->pack_active, g->min_gain, 0, g->branch_opt} : SearchOptions();
}
SearchOptions options_of(const mi_spr_search_options* g) {
  return g ? SearchOptions{g->max_moves, g->pack_active, g->min_gain, g->radius, g->branch_opt} : SearchOptions();
}

// one search call: every pointer a host pointer, or every pointer a device pointer
struct SearchCall {
  int T = 0;
  bool rescaling = false;
  const int32_t* parent_ids = nullptr;
  const double* start = nullptr;
  const double* params = nullptr;
  SearchOptions options;
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

bool all_zero(const mi_branch_opt_options& b) {
  return b.max_iterations == 0 && b.check_interval == 0 && b.pack_active == 0 && b.tolerance == 0.0 &&
         b.min_length == 0.0 && b.max_length == 0.0;
}

// the options a call runs with (branch_opt of zeros: the optimiser's defaults), checked
int check_options(const MoveKind& k, const mi_engine* e, SearchOptions* o) {
  const std::string name = std::string(k.name) + " search: ";
  if (all_zero(o->branch_opt)) o->branch_opt = kBranchOptDefaults;
  if (o->max_moves < 0 || o->max_moves > kSearchMaxMoves)
    return fail(name + "max_moves must be in 0.." + std::to_string(kSearchMaxMoves));
  if (!(o->min_gain >= 0.0)) return fail(name + "min_gain must be >= 0");
  if (o->radius < 0) return fail(name + "radius must be 0 (every move) or positive, not " + std::to_string(o->radius));
  if (check_branch_opt_options(o->branch_opt)) return 1;
  // (a sharded handle owns no scan: its shards check the shape)
  if (k.spr && e->shards.empty() && check_spr_shape(e, o->radius)) return 1;
  return 0;
}

int check_pointers(const mi_engine* e, const SearchCall& c) {
  if (!c.parent_ids || !c.start) return fail("null tree arrays");
  if (!c.out_pid || !c.out_bl || !c.out_ll || !c.out_move_count || !c.out_status) return fail("null output pointer");
  if (e->param_count > 0 && !c.params) return fail("null parameter matrix");
  return 0;
}

// the pieces of the kind's search_ws for a batch of T trees, 256-byte aligned
struct SearchWorkspace {
  int32_t *pid[2], *pk_pid, *opt_status, *best, *target, *map[2], *active, *apply_ws;
  double *bl[2], *pk_bl, *pk_params, *opt_bl, *opt_ll, *delta;
  size_t bytes;
  SearchWorkspace(const MoveKind& k, const mi_engine* e, int T, char* base) {
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
    // the scan's outputs: NNI delta [N][2]; SPR best_delta [N-2][2] and best_target, which the scan always writes
    delta = f64(t * (k.spr ? N - 2 : N) * 2);
    target = k.spr ? i32(t * (N - 2) * 2) : nullptr;
    best = i32(t * k.width);
    map[0] = i32(t);
    map[1] = i32(t);
    active = i32(kSearchMaxMoves + 1);
    apply_ws = i32(std::max<size_t>(t * k.apply_ws_words(e->n), 1));
    bytes = off;
  }
};

int reserve_search(const MoveKind& k, mi_engine* e, int T) {
  if (reserve_branch_opt(e, T)) return 1;
  if (k.reserve_scan(e, T)) return 1;
  return (e->*k.search_ws).ensure(SearchWorkspace(k, e, T, nullptr).bytes);
}

int run_search_device(const MoveKind& k, mi_engine* e, hipStream_t s, const SearchCall& c) {
  HIP_TRY(hipSetDevice(e->spec.device));
  if (e->s == kAa) return fail(four_state_only(k));
  if (c.T <= 0) return fail("tree_count must be positive");
  if (check_pointers(e, c)) return 1;
  SearchOptions o = c.options;
  if (check_options(k, e, &o)) return 1;
  const int T = c.T, n = e->n, N = e->N;
  if (reserve_search(k, e, T)) return 1;
  const SearchWorkspace w(k, e, T, (e->*k.search_ws).as<char>());
  const bool pack = o.pack_active != 0, scans = !(k.spr && n <= 3);
  const size_t np = (size_t)N - 2, nl = (size_t)N - 1;
  HIP_TRY(hipMemcpyAsync(w.pid[0], c.parent_ids, sizeof(int32_t) * T * np, hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemcpyAsync(w.bl[0], c.start, sizeof(double) * T * nl, hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemsetAsync(w.active, 0, sizeof(int32_t) * ((size_t)o.max_moves + 1), s));
  // (the maps are written before they are read; zeroed so that no index is ever out of range)
  HIP_TRY(hipMemsetAsync(w.map[0], 0, sizeof(int32_t) * (size_t)T, s));
  HIP_TRY(hipMemsetAsync(w.map[1], 0, sizeof(int32_t) * (size_t)T, s));
  // (SPR, also where no scan runs: the step kernel reads "no move")
  if (k.spr) HIP_TRY(hipMemsetAsync(w.best, 0xff, sizeof(int32_t) * (size_t)T * k.width, s));
  HIP_TRY(hipMemsetAsync(c.out_status, 0xff, sizeof(int32_t) * (size_t)T, s));  // kSearchActive
  HIP_TRY(hipMemsetAsync(c.out_move_count, 0, sizeof(int32_t) * (size_t)T, s));
  if (c.out_move_log && o.max_moves)
    HIP_TRY(hipMemsetAsync(c.out_move_log, 0xff, sizeof(int32_t) * (size_t)T * o.max_moves * k.width, s));
  if (c.out_move_gain && o.max_moves) HIP_TRY(hipMemsetAsync(c.out_move_gain, 0, sizeof(double) * (size_t)T * o.max_moves, s));

  SearchStepArgs st{};
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
    if (scans) {
      DeviceCall d;
      d.T = count;
      d.route_T = T;
      d.rescaling = c.rescaling;
      d.parent_ids = pid_in;
      d.bl = w.opt_bl;
      d.params = params_in;
      if (k.scan(e, s, d, w, o.radius)) return 1;
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
    k.launch_step(st, s);
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
  e->last_path = hess_path + k.tag + (k.spr ? " radius=" + std::to_string(o.radius) : "") +
                 " rounds=" + std::to_string(rounds) + " moves=" + std::to_string(moves) + " batches=" + batches +
                 (pack ? "" : " pack=off");
  e->last_evals = evals;
  e->last_grad_evals = evals;
  e->last_walk_launches = launches;
  HIP_TRY(hipGetLastError());
  return 0;
}

// The host-pointer form of the search: inputs up in one copy, the rounds, outputs back in one copy
// and the call's one error check.  Each tree shard of a handle searches from its block of trees,
// one shard after the other (the loop synchronises its device every round).
int search_host(const MoveKind& k, mi_engine* e, SearchCall c) {
  if (!e) return fail("null engine");
  if (e->s == kAa) return fail(four_state_only(k));
  if (c.T <= 0) return fail("tree_count must be positive");
  if (check_options(k, e, &c.options)) return 1;
  if (!e->shards.empty() && e->shard_mode != MI_SHARD_TREES) return fail(no_pattern_shards(k));
  if (check_pointers(e, c)) return 1;
  enum { kPid, kBl, kLl, kDelta, kCount, kLog, kGain, kStatus, kOpt };
  const size_t np = 2 * e->n - 3, M = c.options.max_moves;
  HostCall h;
  h.T = c.T;
  h.one_by_one = true;
  h.in = tree_inputs(e, c.parent_ids, c.start, c.params);
  h.out = {per_tree(c.out_pid, np),         per_tree(c.out_bl, np + 1),
           per_tree(c.out_ll, 1),           per_tree(c.out_best_delta, 1),
           per_tree(c.out_move_count, 1),   per_tree(c.out_move_log, M * k.width),
           per_tree(c.out_move_gain, M),    per_tree(c.out_status, 1),
           per_tree(c.out_opt_status, 1)};
  h.enqueue = [&k, c](mi_engine* e, int T, const HostArray* in, const HostArray* out) {
    SearchCall d = c;
    d.T = T;
    d.parent_ids = in[kInParent].at<const int32_t>();
    d.start = in[kInBl].at<const double>();
    d.params = params_on_device(e, in);
    d.out_pid = out[kPid].at<int32_t>();
    d.out_bl = out[kBl].at<double>();
    d.out_ll = out[kLl].at<double>();
    d.out_best_delta = out[kDelta].at<double>();
    d.out_move_count = out[kCount].at<int32_t>();
    d.out_move_log = out[kLog].at<int32_t>();
    d.out_move_gain = out[kGain].at<double>();
    d.out_status = out[kStatus].at<int32_t>();
    d.out_opt_status = out[kOpt].at<int32_t>();
    return run_search_device(k, e, e->stream, d);
  };
  return run_host_call(e, h);
}

int search_device(const MoveKind& k, mi_engine* e, void* stream, const SearchCall& c) {
  if (!e) return fail("null engine");
  if (e->s == kAa) return fail(four_state_only(k));
  if (!e->shards.empty()) return fail(kShardedDeviceCall);
  return run_search_device(k, e, pick_stream(e, stream), c);
}

int reserve_search_entry(const MoveKind& k, mi_engine* e, int32_t tree_count) {
  if (!e) return fail("null engine");
  if (tree_count <= 0) return fail("tree_count must be positive");
  if (e->s == kAa) return fail(four_state_only(k));
  if (!e->shards.empty()) {
    if (e->shard_mode != MI_SHARD_TREES) return fail(no_pattern_shards(k));
    return for_each_shard(e, tree_count, [&k](mi_engine* shard, int32_t T) { return reserve_search_entry(k, shard, T); });
  }
  if (k.spr && check_spr_shape(e, 0)) return 1;
  HIP_TRY(hipSetDevice(e->spec.device));
  if (reserve_apply(k, e, tree_count)) return 1;
  return reserve_search(k, e, tree_count);
}

const MoveKind kNniMove = {
    "NNI", " nni-search", false, 1, nni_apply_ws_words, &mi_engine::nni_apply_ws, &mi_engine::nni_search_ws, reserve_nni_calls,
    [](mi_engine* e, hipStream_t s, DeviceCall& d, const SearchWorkspace& w, int) {
      d.out_nni = w.delta;
      d.out_best = w.best;
      return run_nni_device(e, s, d);
    },
    launch_nni_apply, launch_nni_search_step};
const MoveKind kSprMove = {
    "SPR", " spr-search", true, 3, spr_apply_ws_words, &mi_engine::spr_apply_ws, &mi_engine::spr_search_ws, reserve_spr_calls,
    [](mi_engine* e, hipStream_t s, DeviceCall& d, const SearchWorkspace& w, int radius) {
      d.spr_radius = radius;
      d.out_spr_target = w.target;
      d.out_spr_delta = w.delta;
      d.out_spr_move = w.best;
      return run_spr_device(e, s, d);
    },
    launch_spr_apply, launch_spr_search_step};

}  // namespace

extern "C" {

int32_t mi_engine_nni_apply_unrooted(mi_engine* e, int32_t T, const int32_t* parent_ids, const double* bl,
                                     const int32_t* moves, int32_t* out_parent_ids, double* out_bl) {
  return apply_host(kNniMove, e, T, parent_ids, bl, moves, out_parent_ids, out_bl);
}
int32_t mi_engine_spr_apply_unrooted(mi_engine* e, int32_t T, const int32_t* parent_ids, const double* bl,
                                     const int32_t* moves, int32_t* out_parent_ids, double* out_bl) {
  return apply_host(kSprMove, e, T, parent_ids, bl, moves, out_parent_ids, out_bl);
}

int32_t mi_engine_nni_apply_unrooted_device(mi_engine* e, void* stream, int32_t T, const int32_t* parent_ids,
                                            const double* bl, const int32_t* moves, int32_t* out_parent_ids,
                                            double* out_bl) {
  return apply_device(kNniMove, e, stream, T, parent_ids, bl, moves, out_parent_ids, out_bl);
}
int32_t mi_engine_spr_apply_unrooted_device(mi_engine* e, void* stream, int32_t T, const int32_t* parent_ids,
                                            const double* bl, const int32_t* moves, int32_t* out_parent_ids,
                                            double* out_bl) {
  return apply_device(kSprMove, e, stream, T, parent_ids, bl, moves, out_parent_ids, out_bl);
}

int32_t mi_engine_nni_search_unrooted(mi_engine* e, int32_t T, const int32_t* parent_ids, const double* start,
                                      const double* params, int32_t rescaling,
                                      const mi_nni_search_options* options, int32_t* out_parent_ids,
                                      double* out_bl, double* out_ll, double* out_best_delta,
                                      int32_t* out_move_count, int32_t* out_move_log, double* out_move_gain,
                                      int32_t* out_status, int32_t* out_opt_status) {
  return search_host(kNniMove, e,
                     {T, rescaling != 0, parent_ids, start, params, options_of(options), out_parent_ids, out_bl, out_ll,
                      out_best_delta, out_move_count, out_move_log, out_move_gain, out_status, out_opt_status});
}
int32_t mi_engine_spr_search_unrooted(mi_engine* e, int32_t T, const int32_t* parent_ids, const double* start,
                                      const double* params, int32_t rescaling,
                                      const mi_spr_search_options* options, int32_t* out_parent_ids,
                                      double* out_bl, double* out_ll, double* out_best_delta,
                                      int32_t* out_move_count, int32_t* out_move_log, double* out_move_gain,
                                      int32_t* out_status, int32_t* out_opt_status) {
  return search_host(kSprMove, e,
                     {T, rescaling != 0, parent_ids, start, params, options_of(options), out_parent_ids, out_bl, out_ll,
                      out_best_delta, out_move_count, out_move_log, out_move_gain, out_status, out_opt_status});
}

int32_t mi_engine_nni_search_unrooted_device(mi_engine* e, void* stream, int32_t T, const int32_t* parent_ids,
                                             const double* start, const double* params, int32_t rescaling,
                                             const mi_nni_search_options* options, int32_t* out_parent_ids,
                                             double* out_bl, double* out_ll, double* out_best_delta,
                                             int32_t* out_move_count, int32_t* out_move_log,
                                             double* out_move_gain, int32_t* out_status,
                                             int32_t* out_opt_status) {
  return search_device(kNniMove, e, stream,
                       {T, rescaling != 0, parent_ids, start, params, options_of(options), out_parent_ids, out_bl, out_ll,
                        out_best_delta, out_move_count, out_move_log, out_move_gain, out_status, out_opt_status});
}
int32_t mi_engine_spr_search_unrooted_device(mi_engine* e, void* stream, int32_t T, const int32_t* parent_ids,
                                             const double* start, const double* params, int32_t rescaling,
                                             const mi_spr_search_options* options, int32_t* out_parent_ids,
                                             double* out_bl, double* out_ll, double* out_best_delta,
                                             int32_t* out_move_count, int32_t* out_move_log,
                                             double* out_move_gain, int32_t* out_status,
                                             int32_t* out_opt_status) {
  return search_device(kSprMove, e, stream,
                       {T, rescaling != 0, parent_ids, start, params, options_of(options), out_parent_ids, out_bl, out_ll,
                        out_best_delta, out_move_count, out_move_log, out_move_gain, out_status, out_opt_status});
}

int32_t mi_engine_reserve_nni_search(mi_engine* e, int32_t tree_count) { return reserve_search_entry(kNniMove, e, tree_count); }
int32_t mi_engine_reserve_spr_search(mi_engine* e, int32_t tree_count) { return reserve_search_entry(kSprMove, e, tree_count); }

}  // extern "C"
