// Starting trees: pairwise maximum-likelihood distances from the engine's
// alignment, neighbour joining of a batch of distance matrices, and the two in one call
// (mi_engine_pairwise_distances_device, mi_engine_neighbour_joining_device,
// mi_engine_starting_trees_unrooted_device, mi_engine_reserve_start_trees).  The device forms
// only enqueue; their host-pointer forms are described in mi_phylo_host_calls.cpp.
#include <cmath>

#include "mi_phylo_engine.h"

const mi_distance_options kDistanceDefaults = {50, 0, 1e-10, 1e-8, 10.0, {0, 0, 0, 0}};
const char kDistance4State[] = "pairwise distances and starting trees are 4-state only";
const char kDistancePatternShards[] =
    "pattern-sharded engines do not compute pairwise distances (each shard holds a block of columns): use "
    "MI_SHARD_TREES or a single engine";

namespace {

constexpr int kDistanceMaxIterations = 1000;

size_t pair_count(int n) { return (size_t)n * (n - 1) / 2; }
size_t counts_bytes_per_replicate(int n) { return pair_count(n) * 16 * sizeof(double); }
// replicates whose counts the workspace holds at once: what the arena budget allows, one at
// least (and no more than the second grid dimension of the distance kernel can count)
int chunk_replicates(const mi_engine* e, int B) {
  const size_t per = counts_bytes_per_replicate(e->n);
  const size_t fit = std::min<size_t>(std::max<size_t>(e->plv_budget / per, 1), 65535);
  return (int)std::min<size_t>(fit, (size_t)B);
}

// what does not depend on the replicate count: the tip codes (made once), the model instance
int reserve_distance_engine(mi_engine* e, hipStream_t s) {
  if (e->status.ensure(sizeof(int32_t) * kStatusWords)) return 1;
  if (e->dist_model.ensure(sizeof(DevModel))) return 1;
  if (!e->dist_codes.ptr) {
    const size_t bytes = (size_t)distance_code_rows(e->n) * distance_code_stride(e->P);
    if (e->dist_codes.ensure(bytes)) return 1;
    // (an engine made from tip partials classifies those; else the compact states)
    const bool partials = !e->spec.use_tip_states && e->tip_partials.ptr;
    launch_distance_codes(e->tip_states.as<int8_t>(), partials ? e->tip_partials.as<double>() : nullptr, e->n, e->P,
                          e->dist_codes.as<uint8_t>(), s);
    HIP_TRY(hipGetLastError());
    // (the codes are the engine's from now on, whatever stream a later call runs on)
    HIP_TRY(hipStreamSynchronize(s));
  }
  return 0;
}

int reserve_nj(mi_engine* e, int B, int n) {
  nj_prepare(n);
  if (n > kNjLdsTaxa && e->nj_ws.ensure(nj_ws_bytes(n) * (size_t)B)) return 1;
  return e->status.ensure(sizeof(int32_t) * kStatusWords);
}

}  // namespace

int distance_options(const mi_distance_options* in, mi_distance_options* out) {
  mi_distance_options o = in ? *in : kDistanceDefaults;
  if (o.max_iterations == 0) o.max_iterations = kDistanceDefaults.max_iterations;
  if (o.tolerance == 0.0) o.tolerance = kDistanceDefaults.tolerance;
  if (o.min_length == 0.0) o.min_length = kDistanceDefaults.min_length;
  if (o.max_length == 0.0) o.max_length = kDistanceDefaults.max_length;
  if (o.max_iterations < 1 || o.max_iterations > kDistanceMaxIterations)
    return fail("pairwise distances: max_iterations must be in 1.." + std::to_string(kDistanceMaxIterations));
  if (!(o.tolerance > 0.0)) return fail("pairwise distances: tolerance must be positive");
  if (!(o.min_length > 0.0) || !(o.min_length < o.max_length) || !(o.max_length < INFINITY))
    return fail("pairwise distances: need 0 < min_length < max_length < inf");
  *out = o;
  return 0;
}

int check_distance_call(const mi_engine* e, int B) {
  if (!e) return fail("null engine");
  if (e->s == kAa) return fail(kDistance4State);
  if (!e->shards.empty() && e->shard_mode != MI_SHARD_TREES) return fail(kDistancePatternShards);
  if (B < 1) return fail("replicate_count must be positive");
  return 0;
}

int run_pair_distances_device(mi_engine* e, hipStream_t s, const PairDistanceCall& c) {
  HIP_TRY(hipSetDevice(e->spec.device));
  if (check_distance_call(e, c.B)) return 1;
  if (!c.weights && c.B != 1) return fail("pairwise distances: without replicate weights replicate_count is 1");
  if (e->param_count > 0 && !c.params) return fail("null parameter row");
  if (!c.out_dist) return fail("null distance output");
  mi_distance_options o;
  if (distance_options(c.options, &o)) return 1;
  const int n = e->n, B = c.B;
  if (reserve_distance_engine(e, s)) return 1;
  const int chunk = chunk_replicates(e, B);
  if (e->dist_counts.ensure(counts_bytes_per_replicate(n) * (size_t)chunk)) return 1;

  // the call's one model instance, by the set-up every other call uses (no trees in this launch)
  DeviceCall d;
  d.T = 1;
  d.params = c.params;
  CallPlan p{};
  p.models_per_tree = 1;
  ModelSetupArgs ms = model_setup_args(e, d, p);
  ms.models = e->dist_model.as<DevModel>();
  TreeSetupArgs none{};
  none.n = e->n;
  none.status = e->status.as<int32_t>();
  launch_setup(none, ms, e->sw, s);

  DistanceArgs a{};
  a.n = n;
  a.n4 = distance_code_rows(n);
  a.P = e->P;
  a.Pp = distance_code_stride(e->P);
  a.K = e->K;
  a.codes = e->dist_codes.as<uint8_t>();
  a.counts = e->dist_counts.as<double>();
  a.model = e->dist_model.as<DevModel>();
  a.tmin = o.min_length;
  a.tmax = o.max_length;
  a.tol = o.tolerance;
  a.max_iter = o.max_iterations;
  const size_t pairs = pair_count(n);
  int chunks = 0;
  for (int first = 0; first < B; first += chunk, chunks++) {
    a.B = std::min(chunk, B - first);
    a.weights = c.weights ? c.weights + (size_t)first * e->P : e->weights.as<double>();
    a.out_dist = c.out_dist + (size_t)first * n * n;
    a.out_counts = c.out_counts ? c.out_counts + (size_t)first * pairs * 16 : nullptr;
    a.out_status = c.out_status ? c.out_status + (size_t)first * pairs : nullptr;
    launch_pair_distances(a, s);
  }
  HIP_TRY(hipGetLastError());
  e->dominant = pair_counts_kernel_name();
  e->last_walk_launches = chunks;
  e->last_evals = B;
  e->last_grad_evals = 0;
  e->last_path = "pair_counts B=" + std::to_string(B) + " chunks=" + std::to_string(chunks);
  return 0;
}

int run_nj_device(mi_engine* e, hipStream_t s, int B, int n, const double* dist, double tmin, double tmax,
                  int32_t* out_parent_ids, double* out_bl) {
  HIP_TRY(hipSetDevice(e->spec.device));
  if (B < 1) return fail("replicate_count must be positive");
  if (n < 3) return fail("neighbour joining needs at least 3 taxa");
  if (!dist) return fail("null distance matrices");
  if (!out_parent_ids || !out_bl) return fail("null output pointer");
  if (!(tmin < tmax)) return fail("neighbour joining: need min_length < max_length");
  if (reserve_nj(e, B, n)) return 1;
  NjArgs a{};
  a.n = n;
  a.B = B;
  a.tmin = tmin;
  a.tmax = tmax;
  a.dist = dist;
  a.ws = e->nj_ws.as<char>();
  a.status = e->status.as<int32_t>();
  a.out_parent_ids = out_parent_ids;
  a.out_bl = out_bl;
  launch_nj(a, s);
  HIP_TRY(hipGetLastError());
  e->dominant = "nj_kernel";
  e->last_walk_launches = 1;
  e->last_evals = B;
  e->last_grad_evals = 0;
  e->last_path = "nj n=" + std::to_string(n) + (n <= kNjLdsTaxa ? " store=lds" : " store=global");
  return 0;
}

int run_start_trees_device(mi_engine* e, hipStream_t s, const PairDistanceCall& c, int32_t* out_parent_ids,
                           double* out_bl) {
  HIP_TRY(hipSetDevice(e->spec.device));
  if (check_distance_call(e, c.B)) return 1;
  if (!out_parent_ids || !out_bl) return fail("null output pointer");
  mi_distance_options o;
  if (distance_options(c.options, &o)) return 1;
  PairDistanceCall pd = c;
  if (!pd.out_dist) {
    if (e->dist_matrix.ensure(sizeof(double) * (size_t)c.B * e->n * e->n)) return 1;
    pd.out_dist = e->dist_matrix.as<double>();
  }
  if (run_pair_distances_device(e, s, pd)) return 1;
  const std::string counts_path = e->last_path;
  const int chunks = e->last_walk_launches;
  if (run_nj_device(e, s, c.B, e->n, pd.out_dist, o.min_length, o.max_length, out_parent_ids, out_bl)) return 1;
  e->dominant = pair_counts_kernel_name();
  e->last_walk_launches = chunks;  // (the call's chunks are the distance half's)
  e->last_path = counts_path + " | " + e->last_path;
  return 0;
}

extern "C" {

int32_t mi_engine_pairwise_distances_device(mi_engine* e, void* stream, int32_t B, const double* weights,
                                            const double* params, const mi_distance_options* options,
                                            double* out_dist, double* out_counts, int8_t* out_status) {
  if (!e) return fail("null engine");
  if (!e->shards.empty()) return fail(kShardedDeviceCall);
  PairDistanceCall c;
  c.B = B;
  c.weights = weights;
  c.params = params;
  c.options = options;
  c.out_dist = out_dist;
  c.out_counts = out_counts;
  c.out_status = out_status;
  return run_pair_distances_device(e, pick_stream(e, stream), c);
}

int32_t mi_engine_neighbour_joining_device(mi_engine* e, void* stream, int32_t B, int32_t n, const double* dist,
                                           double min_length, double max_length, int32_t* out_parent_ids,
                                           double* out_bl) {
  if (!e) return fail("null engine");
  if (!e->shards.empty()) return fail(kShardedDeviceCall);
  return run_nj_device(e, pick_stream(e, stream), B, n, dist, min_length, max_length, out_parent_ids, out_bl);
}

int32_t mi_engine_starting_trees_unrooted_device(mi_engine* e, void* stream, int32_t B, const double* weights,
                                                 const double* params, const mi_distance_options* options,
                                                 int32_t* out_parent_ids, double* out_bl, double* out_dist) {
  if (!e) return fail("null engine");
  if (!e->shards.empty()) return fail(kShardedDeviceCall);
  PairDistanceCall c;
  c.B = B;
  c.weights = weights;
  c.params = params;
  c.options = options;
  c.out_dist = out_dist;
  return run_start_trees_device(e, pick_stream(e, stream), c, out_parent_ids, out_bl);
}

int32_t mi_engine_reserve_start_trees(mi_engine* e, int32_t B) {
  if (check_distance_call(e, B)) return 1;
  e = first_engine(e);
  HIP_TRY(hipSetDevice(e->spec.device));
  if (reserve_distance_engine(e, e->stream)) return 1;
  if (e->dist_counts.ensure(counts_bytes_per_replicate(e->n) * (size_t)chunk_replicates(e, B))) return 1;
  if (e->dist_matrix.ensure(sizeof(double) * (size_t)B * e->n * e->n)) return 1;
  return reserve_nj(e, B, e->n);
}

}  // extern "C"
