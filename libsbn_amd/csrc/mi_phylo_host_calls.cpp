// What runs a host-pointer call of the C ABI, and the plain entry points.  A call
// is its two lists of arrays and a function that enqueues its device work (HostCall,
// mi_phylo_engine.h).  From those, here and only here: staging through pinned memory with one DMA
// each way, the one synchronisation with its status check, the retry after a one-launch time-out,
// and the shards of a handle (several devices / logical shards behind one engine handle) -- trees
// dealt in contiguous blocks, or sums over site patterns added in shard order.  The offsets of it
// all are mi_phylo_host_arrays.h's.  The entry points of the optimiser, the NNI search and RELL
// describe their calls in their own files.
#include "mi_phylo_engine.h"

namespace {

// One DMA each way per host-pointer call (round 5; until then one per array: a memset, three to
// eight uploads and three to five downloads, each its own submission and its own turn on the
// stream -- 60 to 80 of the 930 microseconds of a 1000-tree DS1 call).  Inputs are packed into
// one pinned block and copied to one device block; the outputs live in one device block and
// come back as one copy, the pieces handed to the caller's arrays after the call's one
// synchronisation.  Pieces are 256-byte aligned (pack_offsets).
int upload_pack(mi_engine* e, std::vector<HostArray>& arrays, int T) {
  std::vector<size_t> off;
  const size_t total = pack_offsets(arrays, T, off);
  if (e->in_pack.ensure(std::max<size_t>(total, 256))) return 1;
  char* pin = total ? static_cast<char*>(e->pinned.alloc(total, e->stream)) : nullptr;
  if (total && !pin) return fail("pinned staging allocation failed");
  for (size_t i = 0; i < arrays.size(); i++) {
    HostArray& a = arrays[i];
    a.dev = a.host ? e->in_pack.as<char>() + off[i] : nullptr;
    if (a.host) memcpy(pin + off[i], a.host, a.bytes(T));
  }
  if (total) HIP_TRY(hipMemcpyAsync(e->in_pack.ptr, pin, total, hipMemcpyHostToDevice, e->stream));
  return 0;
}
// device addresses of the wanted outputs (before the kernels are enqueued) ...
int place_out_pack(mi_engine* e, std::vector<HostArray>& arrays, int T) {
  std::vector<size_t> off;
  const size_t total = pack_offsets(arrays, T, off);
  if (e->out_pack.ensure(std::max<size_t>(total, 256))) return 1;
  for (size_t i = 0; i < arrays.size(); i++)
    arrays[i].dev = arrays[i].host ? e->out_pack.as<char>() + off[i] : nullptr;
  return 0;
}
// ... and their one copy back (after them): the pieces are delivered by finish_host
int download_pack(mi_engine* e, const std::vector<HostArray>& arrays, int T) {
  std::vector<size_t> off;
  const size_t total = pack_offsets(arrays, T, off);
  if (!total) return 0;
  char* pin = static_cast<char*>(e->pinned.alloc(total, e->stream));
  if (!pin) return fail("pinned staging allocation failed");
  HIP_TRY(hipMemcpyAsync(pin, e->out_pack.ptr, total, hipMemcpyDeviceToHost, e->stream));
  for (size_t i = 0; i < arrays.size(); i++)
    if (arrays[i].host && arrays[i].bytes(T))
      e->pinned.pending.push_back({arrays[i].host, pin + off[i], arrays[i].bytes(T)});
  return 0;
}

// Start of a host-pointer call on one engine: inputs staged and copied up, the device work and
// the copy back enqueued on the engine's stream.
int begin_host(mi_engine* e, HostCall& c) {
  HIP_TRY(hipSetDevice(e->spec.device));
  e->fused_timed_out = false;  // (what an earlier device-pointer call left unread is not this call's)
  e->pinned.reset();  // nothing of an earlier (possibly failed) call is delivered late
  // The status word is sticky (the *_device calls never clear it).  A host-pointer call
  // reports ITS OWN errors only: whatever an earlier device-pointer call left unread on this
  // engine's stream is dropped here, not blamed on this batch.
  if (e->status.ensure(sizeof(int32_t) * kStatusWords)) return 1;
  HIP_TRY(hipMemsetAsync(e->status.ptr, 0, sizeof(int32_t) * kStatusWords, e->stream));
  if (upload_pack(e, c.in, c.T) || place_out_pack(e, c.out, c.T)) return 1;
  // (outputs nobody wants have no device address: a null pointer skips their work)
  if (c.enqueue(e, c.T, c.in.data(), c.out.data())) return 1;
  return download_pack(e, c.out, c.T);
}

// End of a host-pointer call: one synchronisation (inside check_status), then the staged
// outputs are copied to the caller's buffers.  A time-out of the one-launch call (see
// check_status) does not reach the caller of a call that retries: the call is run again, now
// through the four-launch sequence -- fresh launches in the same process, nothing else is
// restarted -- and ITS results and errors are what the caller gets (the reference never fails
// spuriously: src/engine.cpp:54-92).
int finish_host(mi_engine* e, HostCall& c) {
  int rc = check_status(e, e->stream);
  if (e->fused_timed_out && c.retry) {
    e->fused_fallbacks++;
    rc = begin_host(e, c);
    if (rc == 0) rc = check_status(e, e->stream);
  }
  e->fused_timed_out = false;
  // (deliver_on_error: the call marks what it refused inside its outputs, and the caller gets them with the
  // error.  The stream idle again says that the error is check_status's, read after its synchronisation: the
  // staged bytes are the call's.  After a HIP error they are not, and nothing is delivered.)
  if (rc == 0 || (c.deliver_on_error && hipStreamQuery(e->stream) == hipSuccess)) e->pinned.flush();
  e->pinned.reset();
  return rc;
}

// A sharded handle: trees dealt to the shards in contiguous blocks (what
// FatBeagleParallelize's work queue does with thread_count FatBeagles,
// fat_beagle.hpp:119-149), or -- few trees, very long alignments -- every shard evaluates
// all trees on its own block of site patterns.  What is a sum (over the call, or over the
// patterns) every shard leaves in scratch of its own, added in shard order afterwards:
// deterministic.  The call is begun on every shard before it is finished on any, so the devices
// work side by side -- unless its work synchronises its device itself.
int run_shards(mi_engine* e, HostCall& c) {
  const int D = (int)e->shards.size();
  const bool patterns = e->shard_mode != MI_SHARD_TREES;
  for (const HostArray& a : c.out)
    if (patterns && a.host && a.combine == kPerTree)
      return fail("internal error: a pattern-sharded handle was handed an output that is no sum over site patterns");
  const size_t per = shard_scratch_count(c.out, c.T, patterns);
  e->shard_sums.assign((size_t)D * per, 0.0);
  std::vector<HostCall> calls;
  std::vector<mi_engine*> begun;
  calls.reserve(D);
  int rc = 0;
  for (int i = 0; i < D && !rc; i++) {
    int32_t first = 0, count = c.T;
    if (!patterns) mi_shard_range(c.T, D, i, &first, &count);
    if (count == 0) continue;
    calls.push_back(c);
    HostCall& s = calls.back();
    s.T = count;
    slice_trees(s.in, first);
    slice_trees(s.out, first);
    point_at_scratch(s.out, c.T, patterns, e->shard_sums.data() + begun.size() * per);
    begun.push_back(e->shards[i]);
    e->shards[i]->status_tree_offset = first;
    rc = c.one_by_one ? run_on_engine(e->shards[i], s) : begin_host(e->shards[i], s);
  }
  if (!c.one_by_one)
    for (size_t k = 0; k < begun.size(); k++) rc |= finish_host(begun[k], calls[k]);
  if (rc) return 1;
  add_shards(c.out, c.T, patterns, e->shard_sums.data(), per, (int)begun.size());
  return 0;
}

const char kRootedPatternShards[] =
    "pattern-sharded engines evaluate unrooted calls only (the log-det-Jacobian "
    "and the rooted chain rule are not sums over site patterns)";

// The argument checks every plain call begins with, in the order callers know them.  `refusal`:
// what a pattern-sharded handle answers a call that is no plain sum over site patterns.
int check_tree_call(const mi_engine* e, int T, const void* parent_ids, const void* bl, const void* params,
                    const char* refusal = nullptr) {
  if (!e) return fail("null engine");
  if (T <= 0) return fail("tree_count must be positive");
  if (refusal && !e->shards.empty() && e->shard_mode != MI_SHARD_TREES) return fail(refusal);
  if (!parent_ids || !bl) return fail("null tree arrays");
  if (e->param_count > 0 && !params) return fail("null parameter matrix");
  return 0;
}

// a plain call: one device call, run again after a one-launch time-out
int run_plain(mi_engine* e, HostCall& c) {
  c.retry = true;
  return run_host_call(e, c);
}

}  // namespace

int run_on_engine(mi_engine* e, HostCall& c) {
  if (begin_host(e, c)) {
    e->pinned.reset();
    return 1;
  }
  return finish_host(e, c);
}

int run_host_call(mi_engine* e, HostCall& c) { return e->shards.empty() ? run_on_engine(e, c) : run_shards(e, c); }

extern "C" {

int32_t mi_shard_range(int32_t total, int32_t shard_count, int32_t shard, int32_t* begin,
                       int32_t* count) {
  if (total < 0 || shard_count <= 0 || shard < 0 || shard >= shard_count)
    return fail("mi_shard_range: bad arguments");
  // sizes differ by at most one, the larger blocks first (libsbn_amd/sharding.py: tree_shard)
  const int32_t base = total / shard_count, extra = total % shard_count;
  if (begin) *begin = shard * base + (shard < extra ? shard : extra);
  if (count) *count = base + (shard < extra ? 1 : 0);
  return 0;
}

int32_t mi_engine_log_likelihoods_unrooted(mi_engine* e, int32_t T, const int32_t* parent_ids,
                                           const double* bl, const double* params,
                                           int32_t rescaling, double* out_ll) {
  if (!out_ll) return fail("null output");
  if (check_tree_call(e, T, parent_ids, bl, params)) return 1;
  HostCall c;
  c.T = T;
  c.in = tree_inputs(e, parent_ids, bl, params);
  c.out = {per_tree(out_ll, 1, kPerTreeSum)};
  c.enqueue = [=](mi_engine* e, int T, const HostArray* in, const HostArray* out) {
    return mi_engine_log_likelihoods_unrooted_device(e, e->stream, T, in[kInParent].at<const int32_t>(),
                                                     in[kInBl].at<const double>(), params_on_device(e, in),
                                                     rescaling, out[0].at<double>());
  };
  return run_plain(e, c);
}

int32_t mi_engine_gradients_unrooted(mi_engine* e, int32_t T, const int32_t* parent_ids,
                                     const double* bl, const double* params, int32_t rescaling,
                                     double* out_ll, double* out_branch, double* out_site,
                                     double* out_subst) {
  if (!out_ll || !out_branch) return fail("null output");
  if (check_tree_call(e, T, parent_ids, bl, params)) return 1;
  HostCall c;
  c.T = T;
  c.in = tree_inputs(e, parent_ids, bl, params);
  // (a block the model does not have is not wanted either)
  c.out = {per_tree(out_ll, 1, kPerTreeSum), per_tree(out_branch, e->N, kPerTreeSum),
           per_tree(e->K > 1 ? out_site : nullptr, 1, kPerTreeSum),
           per_tree(e->spec.subst_model == MI_SUBST_GTR ? out_subst : nullptr, 8, kPerTreeSum)};
  c.enqueue = [=](mi_engine* e, int T, const HostArray* in, const HostArray* out) {
    return mi_engine_gradients_unrooted_device(e, e->stream, T, in[kInParent].at<const int32_t>(),
                                               in[kInBl].at<const double>(), params_on_device(e, in), rescaling,
                                               out[0].at<double>(), out[1].at<double>(), out[2].at<double>(),
                                               out[3].at<double>());
  };
  return run_plain(e, c);
}

int32_t mi_engine_branch_hessian_unrooted(mi_engine* e, int32_t T, const int32_t* parent_ids,
                                          const double* bl, const double* params, int32_t rescaling,
                                          double* out_ll, double* out_branch, double* out_hess,
                                          double* out_gsq) {
  if (!out_hess) return fail("null branch-Hessian output");
  if (e && e->s == kAa) return fail(kHessian4State);
  if (check_tree_call(e, T, parent_ids, bl, params)) return 1;
  HostCall c;
  c.T = T;
  c.in = tree_inputs(e, parent_ids, bl, params);
  // (H = D2 term - S adds up pattern shard by pattern shard like the rest)
  c.out = {per_tree(out_ll, 1, kPerTreeSum), per_tree(out_branch, e->N, kPerTreeSum),
           per_tree(out_hess, e->N, kPerTreeSum), per_tree(out_gsq, e->N, kPerTreeSum)};
  c.enqueue = [=](mi_engine* e, int T, const HostArray* in, const HostArray* out) {
    return mi_engine_branch_hessian_unrooted_device(e, e->stream, T, in[kInParent].at<const int32_t>(),
                                                    in[kInBl].at<const double>(), params_on_device(e, in),
                                                    rescaling, out[0].at<double>(), out[1].at<double>(),
                                                    out[2].at<double>(), out[3].at<double>());
  };
  return run_plain(e, c);
}

int32_t mi_engine_nni_scan_unrooted(mi_engine* e, int32_t T, const int32_t* parent_ids, const double* bl,
                                    const double* params, int32_t rescaling, double* out_ll,
                                    double* out_delta, int32_t* out_best) {
  if (!out_delta) return fail("null NNI delta output");
  if (e && e->s == kAa) return fail(kNni4State);
  if (check_tree_call(e, T, parent_ids, bl, params)) return 1;
  // (pattern shards: the deltas add up; the best move is no sum and is taken from theirs below)
  const bool patterns = !e->shards.empty() && e->shard_mode != MI_SHARD_TREES;
  HostCall c;
  c.T = T;
  c.in = tree_inputs(e, parent_ids, bl, params);
  c.out = {per_tree(out_ll, 1, kPerTreeSum), per_tree(out_delta, (size_t)e->N * 2, kPerTreeSum),
           per_tree(patterns ? nullptr : out_best, 1)};
  c.enqueue = [=](mi_engine* e, int T, const HostArray* in, const HostArray* out) {
    return mi_engine_nni_scan_unrooted_device(e, e->stream, T, in[kInParent].at<const int32_t>(),
                                              in[kInBl].at<const double>(), params_on_device(e, in), rescaling,
                                              out[0].at<double>(), out[1].at<double>(), out[2].at<int32_t>());
  };
  if (run_plain(e, c)) return 1;
  if (patterns && out_best)
    for (int t = 0; t < T; t++) out_best[t] = nni_best_move(e->n, out_delta + (size_t)t * e->N * 2);
  return 0;
}

int32_t mi_engine_pattern_log_likelihoods_unrooted(mi_engine* e, int32_t T, const int32_t* parent_ids,
                                                   const double* bl, const double* params, int32_t rescaling,
                                                   double* out_ll, double* out_pattern_ll) {
  if (!out_pattern_ll) return fail("null per-pattern log-likelihood output");
  if (e && e->s == kAa) return fail(kPatternLl4State);
  if (check_tree_call(e, T, parent_ids, bl, params,
                      "pattern-sharded engines do not hand out per-pattern log-likelihoods (each shard holds a "
                      "block of columns): use MI_SHARD_TREES or a single engine"))
    return 1;
  HostCall c;
  c.T = T;
  c.in = tree_inputs(e, parent_ids, bl, params);
  c.out = {per_tree(out_ll, 1, kPerTreeSum), per_tree(out_pattern_ll, e->P)};
  c.enqueue = [=](mi_engine* e, int T, const HostArray* in, const HostArray* out) {
    return mi_engine_pattern_log_likelihoods_unrooted_device(
        e, e->stream, T, in[kInParent].at<const int32_t>(), in[kInBl].at<const double>(), params_on_device(e, in),
        rescaling, out[0].at<double>(), out[1].at<double>());
  };
  return run_plain(e, c);
}

int32_t mi_engine_ancestral_states_unrooted(mi_engine* e, int32_t T, const int32_t* parent_ids, const double* bl,
                                            const double* params, int32_t rescaling, double* out_ll,
                                            double* out_state, int8_t* out_map, double* out_cat, double* out_rate,
                                            double* out_tip) {
  if (!out_state) return fail("null state-posterior output");
  if (e && e->s == kAa) return fail(kAncestral4State);
  if (check_tree_call(e, T, parent_ids, bl, params,
                      "pattern-sharded engines do not hand out per-pattern posteriors (each shard holds a block of "
                      "columns): use MI_SHARD_TREES or a single engine"))
    return 1;
  const size_t n = e->n, P = e->P;
  HostCall c;
  c.T = T;
  c.in = tree_inputs(e, parent_ids, bl, params);
  c.out = {per_tree(out_ll, 1, kPerTreeSum), per_tree(out_state, (n - 2) * P * 4), per_tree(out_map, (n - 2) * P),
           per_tree(out_cat, P * e->K),       per_tree(out_rate, P),                per_tree(out_tip, n * P * 4)};
  c.enqueue = [=](mi_engine* e, int T, const HostArray* in, const HostArray* out) {
    return mi_engine_ancestral_states_unrooted_device(
        e, e->stream, T, in[kInParent].at<const int32_t>(), in[kInBl].at<const double>(), params_on_device(e, in),
        rescaling, out[0].at<double>(), out[1].at<double>(), out[2].at<int8_t>(), out[3].at<double>(),
        out[4].at<double>(), out[5].at<double>());
  };
  return run_plain(e, c);
}

int32_t mi_engine_placement_unrooted(mi_engine* e, int32_t T, const int32_t* parent_ids, const double* bl,
                                     const double* params, int32_t rescaling, int32_t Q, int32_t C,
                                     const int8_t* query_states, const int32_t* column_pattern,
                                     const double* column_weights, int32_t G, const double* pendant_lengths,
                                     double* out_ll, double* out_edge_ll, int8_t* out_pendant_index,
                                     int32_t* out_best_edge, double* out_lwr, double* out_edge_tables) {
  if (!out_edge_ll) return fail("null edge log-likelihood output");
  if (e && e->s == kAa) return fail(kPlacement4State);
  if (check_tree_call(e, T, parent_ids, bl, params,
                      "pattern-sharded engines do not place queries (each shard holds a block of columns): use "
                      "MI_SHARD_TREES or a single engine"))
    return 1;
  if (check_placement_shape(e, Q, C, G)) return 1;
  if (!query_states || !column_pattern || !pendant_lengths) return fail("null query / column / pendant array");
  for (int g = 0; g < G; g++)
    if (!(pendant_lengths[g] >= 0.0 && pendant_lengths[g] <= 1.79769313486231570e308))
      return fail(std::string(status_message(kBadPendantLength)) + " (pendant " + std::to_string(g) + ")");
  for (int c = 0; c < C; c++)
    if (column_pattern[c] < 0 || column_pattern[c] >= e->P)
      return fail(std::string(status_message(kBadColumnPattern)) + " (column " + std::to_string(c) + ")");
  enum { kInQuery = kTreeInputs, kInColumn, kInWeights, kInPendant };
  const size_t E = 2 * (size_t)e->n - 3, QE = (size_t)Q * E;
  HostCall c;
  c.T = T;
  c.in = tree_inputs(e, parent_ids, bl, params);
  c.in.push_back(fixed(query_states, (size_t)Q * C));
  c.in.push_back(fixed(column_pattern, C));
  c.in.push_back(fixed(column_weights, C));
  c.in.push_back(fixed(pendant_lengths, G));
  c.out = {per_tree(out_ll, 1),           per_tree(out_edge_ll, QE), per_tree(out_pendant_index, QE),
           per_tree(out_best_edge, Q),    per_tree(out_lwr, QE),     per_tree(out_edge_tables, E * G * 5 * e->P)};
  c.enqueue = [=](mi_engine* e, int T, const HostArray* in, const HostArray* out) {
    return mi_engine_placement_unrooted_device(
        e, e->stream, T, in[kInParent].at<const int32_t>(), in[kInBl].at<const double>(), params_on_device(e, in),
        rescaling, Q, C, in[kInQuery].at<const int8_t>(), in[kInColumn].at<const int32_t>(),
        in[kInWeights].at<const double>(), G, in[kInPendant].at<const double>(), out[0].at<double>(),
        out[1].at<double>(), out[2].at<int8_t>(), out[3].at<int32_t>(), out[4].at<double>(), out[5].at<double>());
  };
  return run_plain(e, c);
}

int32_t mi_engine_spr_scan_unrooted(mi_engine* e, int32_t T, const int32_t* parent_ids, const double* bl,
                                    const double* params, int32_t rescaling, int32_t radius, double* out_ll,
                                    int32_t* out_best_target, double* out_best_delta, int32_t* out_best_move,
                                    double* out_delta) {
  if (!out_best_target || !out_best_delta) return fail("null best-target / best-delta output");
  if (e && e->s == kAa) return fail(kSpr4State);
  if (check_tree_call(e, T, parent_ids, bl, params,
                      "pattern-sharded engines do not scan SPR neighbourhoods (the best target of a prune is no sum "
                      "over site patterns): use MI_SHARD_TREES or a single engine"))
    return 1;
  if (check_spr_shape(e, radius)) return 1;
  const size_t E = 2 * (size_t)e->n - 3;
  HostCall c;
  c.T = T;
  c.in = tree_inputs(e, parent_ids, bl, params);
  c.out = {per_tree(out_ll, 1), per_tree(out_best_target, 2 * E), per_tree(out_best_delta, 2 * E),
           per_tree(out_best_move, 3), per_tree(out_delta, 2 * E * E)};
  c.enqueue = [=](mi_engine* e, int T, const HostArray* in, const HostArray* out) {
    return mi_engine_spr_scan_unrooted_device(e, e->stream, T, in[kInParent].at<const int32_t>(),
                                              in[kInBl].at<const double>(), params_on_device(e, in), rescaling, radius,
                                              out[0].at<double>(), out[1].at<int32_t>(), out[2].at<double>(),
                                              out[3].at<int32_t>(), out[4].at<double>());
  };
  return run_plain(e, c);
}

// Starting trees: arrays of fixed counts, no per-tree ones -- a tree-sharded
// handle lets its first shard do the work (every shard holds the whole alignment); neighbour
// joining needs no alignment and goes to the first shard of any handle.  No retry.
int32_t mi_engine_pairwise_distances(mi_engine* e, int32_t B, const double* weights, const double* params,
                                     const mi_distance_options* options, double* out_dist, double* out_counts,
                                     int8_t* out_status) {
  if (check_distance_call(e, B)) return 1;
  e = first_engine(e);
  if (!weights && B != 1) return fail("pairwise distances: without replicate weights replicate_count is 1");
  if (e->param_count > 0 && !params) return fail("null parameter row");
  if (!out_dist) return fail("null distance output");
  mi_distance_options o;
  if (distance_options(options, &o)) return 1;
  const size_t n = e->n, pairs = n * (n - 1) / 2;
  HostCall c;
  c.in = {fixed(weights, (size_t)B * e->P), fixed(e->param_count > 0 ? params : nullptr, e->param_count)};
  c.out = {fixed(out_dist, (size_t)B * n * n), fixed(out_counts, (size_t)B * pairs * 16),
           fixed(out_status, (size_t)B * pairs)};
  c.enqueue = [=](mi_engine* e, int, const HostArray* in, const HostArray* out) {
    PairDistanceCall d;
    d.B = B;
    d.weights = in[0].at<const double>();
    d.params = in[1].dev ? in[1].at<const double>() : e->in_pack.as<const double>();
    d.options = &o;
    d.out_dist = out[0].at<double>();
    d.out_counts = out[1].at<double>();
    d.out_status = out[2].at<int8_t>();
    return run_pair_distances_device(e, e->stream, d);
  };
  return run_on_engine(e, c);
}

int32_t mi_engine_neighbour_joining(mi_engine* e, int32_t B, int32_t n, const double* dist, double min_length,
                                    double max_length, int32_t* out_parent_ids, double* out_bl) {
  if (!e) return fail("null engine");
  if (B < 1) return fail("replicate_count must be positive");
  if (n < 3) return fail("neighbour joining needs at least 3 taxa");
  if (!dist) return fail("null distance matrices");
  if (!out_parent_ids || !out_bl) return fail("null output pointer");
  if (!(min_length < max_length)) return fail("neighbour joining: need min_length < max_length");
  const size_t np = 2 * (size_t)n - 3;
  HostCall c;
  c.in = {fixed(dist, (size_t)B * n * n)};
  c.out = {fixed(out_parent_ids, (size_t)B * np), fixed(out_bl, (size_t)B * (np + 1))};
  c.enqueue = [=](mi_engine* e, int, const HostArray* in, const HostArray* out) {
    return run_nj_device(e, e->stream, B, n, in[0].at<const double>(), min_length, max_length,
                         out[0].at<int32_t>(), out[1].at<double>());
  };
  return run_on_engine(first_engine(e), c);
}

int32_t mi_engine_starting_trees_unrooted(mi_engine* e, int32_t B, const double* weights, const double* params,
                                          const mi_distance_options* options, int32_t* out_parent_ids,
                                          double* out_bl, double* out_dist) {
  if (check_distance_call(e, B)) return 1;
  e = first_engine(e);
  if (!weights && B != 1) return fail("pairwise distances: without replicate weights replicate_count is 1");
  if (e->param_count > 0 && !params) return fail("null parameter row");
  if (!out_parent_ids || !out_bl) return fail("null output pointer");
  mi_distance_options o;
  if (distance_options(options, &o)) return 1;
  const size_t n = e->n, np = 2 * n - 3;
  HostCall c;
  c.in = {fixed(weights, (size_t)B * e->P), fixed(e->param_count > 0 ? params : nullptr, e->param_count)};
  c.out = {fixed(out_parent_ids, (size_t)B * np), fixed(out_bl, (size_t)B * (np + 1)),
           fixed(out_dist, (size_t)B * n * n)};
  c.enqueue = [=](mi_engine* e, int, const HostArray* in, const HostArray* out) {
    PairDistanceCall d;
    d.B = B;
    d.weights = in[0].at<const double>();
    d.params = in[1].dev ? in[1].at<const double>() : e->in_pack.as<const double>();
    d.options = &o;
    d.out_dist = out[2].at<double>();
    return run_start_trees_device(e, e->stream, d, out[0].at<int32_t>(), out[1].at<double>());
  };
  return run_on_engine(e, c);
}

int32_t mi_engine_gradients_unrooted_reduced(mi_engine* e, int32_t T, const int32_t* parent_ids,
                                             const double* bl, const double* params,
                                             int32_t rescaling, const int32_t* branch_index,
                                             const double* tree_weights, int32_t index_count,
                                             double* out_sums, double* out_index_gradient,
                                             double* out_ll) {
  if (!out_sums || !branch_index || index_count < 0 || (index_count > 0 && !out_index_gradient))
    return fail("null output / index");
  if (check_tree_call(e, T, parent_ids, bl, params)) return 1;
  enum { kInIndex = kTreeInputs, kInWeights };
  HostCall c;
  c.T = T;
  c.in = tree_inputs(e, parent_ids, bl, params);
  c.in.push_back(per_tree(branch_index, e->N));
  c.in.push_back(per_tree(tree_weights, 1));
  // fused reductions of a variational-inference step: sum w logL and sum w site gradient [2], [index_count]
  c.out = {per_tree(out_ll, 1, kPerTreeSum), fixed(out_sums, 2, kCallSum),
           fixed(out_index_gradient, index_count, kCallSum)};
  c.enqueue = [=](mi_engine* e, int T, const HostArray* in, const HostArray* out) {
    return mi_engine_gradients_unrooted_reduced_device(
        e, e->stream, T, in[kInParent].at<const int32_t>(), in[kInBl].at<const double>(), params_on_device(e, in),
        rescaling, in[kInIndex].at<const int32_t>(), in[kInWeights].at<const double>(), index_count,
        out[1].at<double>(), out[2].at<double>(), out[0].at<double>());
  };
  return run_plain(e, c);
}

int32_t mi_engine_log_likelihoods_rooted(mi_engine* e, int32_t T, const int32_t* parent_ids,
                                         const double* bl, const double* params,
                                         const double* rates, const double* heights,
                                         const double* bounds, int32_t with_jacobian,
                                         int32_t rescaling, double* out_ll) {
  if (!out_ll) return fail("null output");
  if (check_tree_call(e, T, parent_ids, bl, params, kRootedPatternShards)) return 1;
  enum { kInRates = kTreeInputs, kInHeights, kInBounds };
  // (the time tree travels whole or not at all)
  const bool tt = rates && heights && bounds;
  HostCall c;
  c.T = T;
  c.in = tree_inputs(e, parent_ids, bl, params, true);
  c.in.push_back(per_tree(tt ? rates : nullptr, e->N - 1));
  c.in.push_back(per_tree(tt ? heights : nullptr, e->N));
  c.in.push_back(per_tree(tt ? bounds : nullptr, e->N));
  c.out = {per_tree(out_ll, 1)};
  c.enqueue = [=](mi_engine* e, int T, const HostArray* in, const HostArray* out) {
    return mi_engine_log_likelihoods_rooted_device(
        e, e->stream, T, in[kInParent].at<const int32_t>(), in[kInBl].at<const double>(), params_on_device(e, in),
        in[kInRates].at<const double>(), in[kInHeights].at<const double>(), in[kInBounds].at<const double>(),
        with_jacobian, rescaling, out[0].at<double>());
  };
  return run_plain(e, c);
}

int32_t mi_engine_gradients_rooted(mi_engine* e, int32_t T, const int32_t* parent_ids,
                                   const double* bl, const double* params, const double* rates,
                                   const int32_t* rate_counts, const double* heights,
                                   const double* bounds, const double* ratios,
                                   int32_t rescaling, double* out_ll, double* out_ratios,
                                   double* out_clock, double* out_site, double* out_subst) {
  if (!out_ll || !out_ratios || !out_clock) return fail("null output");
  if (!rates || !rate_counts || !heights || !bounds || !ratios)
    return fail("Attempted access of a time tree member that requires the time tree to be "
                "initialized. Have you set dates for your time trees, and initialized the "
                "time trees?");
  if (check_tree_call(e, T, parent_ids, bl, params, kRootedPatternShards)) return 1;
  for (int t = 0; t < T; t++)
    if (rate_counts[t] != 1 && rate_counts[t] != e->N - 1) return fail(status_message(kBadRateCount));
  enum { kInRates = kTreeInputs, kInHeights, kInBounds, kInCounts, kInRatios };
  HostCall c;
  c.T = T;
  c.in = tree_inputs(e, parent_ids, bl, params, true);
  c.in.push_back(per_tree(rates, e->N - 1));
  c.in.push_back(per_tree(heights, e->N));
  c.in.push_back(per_tree(bounds, e->N));
  c.in.push_back(per_tree(rate_counts, 1));
  c.in.push_back(per_tree(ratios, e->n - 1));
  c.out = {per_tree(out_ll, 1), per_tree(out_ratios, e->n - 1), per_tree(out_clock, e->N - 1),
           per_tree(e->K > 1 ? out_site : nullptr, 1),
           per_tree(e->spec.subst_model == MI_SUBST_GTR ? out_subst : nullptr, 8)};
  c.enqueue = [=](mi_engine* e, int T, const HostArray* in, const HostArray* out) {
    return mi_engine_gradients_rooted_device(
        e, e->stream, T, in[kInParent].at<const int32_t>(), in[kInBl].at<const double>(), params_on_device(e, in),
        in[kInRates].at<const double>(), in[kInCounts].at<const int32_t>(), in[kInHeights].at<const double>(),
        in[kInBounds].at<const double>(), in[kInRatios].at<const double>(), rescaling, out[0].at<double>(),
        out[1].at<double>(), out[2].at<double>(), out[3].at<double>(), out[4].at<double>());
  };
  return run_plain(e, c);
}

}  // extern "C"
