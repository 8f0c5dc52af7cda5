// Per-pattern log-likelihoods (device form), the RELL re-summation with its reductions, the
// fused bootstrap call and the tree-mixture marginal (mi_engine_pattern_log_likelihoods_unrooted_device,
// mi_engine_rell*, mi_engine_rell_bootstrap_unrooted, mi_engine_pattern_mixture*).
// The per-pattern values come out of the log-likelihood call itself (run_device with
// DeviceCall::out_pattern_ll: the PATTERN_LL variant of its kernel); everything after that works
// on matrices and needs no alignment.
#include "mi_phylo_engine.h"

namespace {

const char kRellSharded[] =
    "mi_engine_rell_bootstrap_unrooted needs a single-device engine: the product needs every "
    "tree's row on one device (mi_engine_pattern_log_likelihoods_unrooted + mi_engine_rell "
    "serve a tree-sharded handle)";

// the pieces of e->rell_ws, 256-byte aligned: [B][T] product | row maxima | 1 / denominators | counts
struct RellWorkspace {
  double *c, *row_max, *row_inv;
  int32_t* counts;
  size_t bytes;
  RellWorkspace(int B, int T, char* base) {
    size_t off = 0;
    auto take = [&](size_t b) {
      char* p = base + off;
      off += align256(b);
      return p;
    };
    c = reinterpret_cast<double*>(take(sizeof(double) * (size_t)B * T));
    row_max = reinterpret_cast<double*>(take(sizeof(double) * (size_t)B));
    row_inv = reinterpret_cast<double*>(take(sizeof(double) * (size_t)B));
    counts = reinterpret_cast<int32_t*>(take(sizeof(int32_t) * (size_t)T));
    bytes = off;
  }
};

int check_rell(int B, int T, int P, const void* s, const void* w, const void* bp) {
  if (B <= 0 || T <= 0 || P <= 0) return fail("replicate_count, tree_count and pattern_count must be positive");
  if (!s || !w) return fail("null pattern log-likelihood / replicate weight matrix");
  if (!bp) return fail("null bootstrap-proportion output");
  return 0;
}

int run_mixture_device(mi_engine* e, hipStream_t st, int T, int P, const double* s, const double* lw,
                       const double* pw, double* out_pattern, double* out_total) {
  HIP_TRY(hipSetDevice(e->spec.device));
  if (T <= 0 || P <= 0) return fail("tree_count and pattern_count must be positive");
  if (!s || !pw) return fail("null pattern log-likelihood matrix / pattern weights");
  if (!out_pattern || !out_total) return fail("null output pointer");
  MixtureArgs a{};
  a.T = T;
  a.P = P;
  a.pattern_ll = s;
  a.log_weights = lw;
  a.pattern_weights = pw;
  a.out_pattern = out_pattern;
  a.out_total = out_total;
  launch_pattern_mixture(a, st);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace

int reserve_rell(mi_engine* e, int B, int T) {
  return e->rell_ws.ensure(RellWorkspace(B, T, nullptr).bytes);
}

int run_rell_device(mi_engine* e, hipStream_t s, int B, int T, int P, const double* pattern_ll, const double* weights,
                    double* out_c, int32_t* out_best, double* out_bp, double* out_elw) {
  HIP_TRY(hipSetDevice(e->spec.device));
  if (check_rell(B, T, P, pattern_ll, weights, out_bp)) return 1;
  if (reserve_rell(e, B, T)) return 1;
  const RellWorkspace w(B, T, e->rell_ws.as<char>());
  HIP_TRY(hipMemsetAsync(w.counts, 0, sizeof(int32_t) * (size_t)T, s));
  RellArgs a{};
  a.B = B;
  a.T = T;
  a.P = P;
  a.pattern_ll = pattern_ll;
  a.weights = weights;
  a.c = out_c ? out_c : w.c;
  a.row_max = w.row_max;
  a.row_inv = w.row_inv;
  a.counts = w.counts;
  a.best = out_best;
  a.bp = out_bp;
  a.elw = out_elw;
  launch_rell(a, s);
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" {

int32_t mi_engine_pattern_log_likelihoods_unrooted_device(mi_engine* e, void* stream, int32_t T,
                                                          const int32_t* parent_ids, const double* bl,
                                                          const double* params, int32_t rescaling, double* out_ll,
                                                          double* out_pattern_ll) {
  if (!e) return fail("null engine");
  if (e->s == kAa) return fail(kPatternLl4State);
  if (!e->shards.empty()) return fail(kShardedDeviceCall);
  if (!out_pattern_ll) return fail("null per-pattern log-likelihood output");
  DeviceCall d;
  d.T = T;
  d.rescaling = rescaling != 0;
  d.parent_ids = parent_ids;
  d.bl = bl;
  d.params = params;
  d.out_ll = out_ll;
  d.out_pattern_ll = out_pattern_ll;
  return run_device(e, pick_stream(e, stream), d);
}

// The host-pointer forms: inputs up in one copy, the work, outputs back in one copy and the call's
// one error check.
int32_t mi_engine_rell(mi_engine* e, int32_t B, int32_t T, int32_t P, const double* pattern_ll, const double* weights,
                       double* out_c, int32_t* out_best, double* out_bp, double* out_elw) {
  if (!e) return fail("null engine");
  if (check_rell(B, T, P, pattern_ll, weights, out_bp)) return 1;
  HostCall c;
  c.in = {fixed(pattern_ll, (size_t)T * P), fixed(weights, (size_t)B * P)};
  c.out = {fixed(out_c, (size_t)B * T), fixed(out_best, B), fixed(out_bp, T), fixed(out_elw, T)};
  c.enqueue = [=](mi_engine* e, int, const HostArray* in, const HostArray* out) {
    return run_rell_device(e, e->stream, B, T, P, in[0].at<const double>(), in[1].at<const double>(),
                           out[0].at<double>(), out[1].at<int32_t>(), out[2].at<double>(), out[3].at<double>());
  };
  // (the product needs no alignment: a sharded handle of either kind lets its first shard do it)
  return run_on_engine(first_engine(e), c);
}

int32_t mi_engine_rell_device(mi_engine* e, void* stream, int32_t B, int32_t T, int32_t P, const double* pattern_ll,
                              const double* weights, double* out_c, int32_t* out_best, double* out_bp,
                              double* out_elw) {
  if (!e) return fail("null engine");
  if (!e->shards.empty()) return fail(kShardedDeviceCall);
  return run_rell_device(e, pick_stream(e, stream), B, T, P, pattern_ll, weights, out_c, out_best, out_bp, out_elw);
}

int32_t mi_engine_reserve_rell(mi_engine* e, int32_t B, int32_t T, int32_t P) {
  if (!e) return fail("null engine");
  if (B <= 0 || T <= 0 || P <= 0) return fail("replicate_count, tree_count and pattern_count must be positive");
  mi_engine* one = e->shards.empty() ? e : e->shards[0];
  HIP_TRY(hipSetDevice(one->spec.device));
  return reserve_rell(one, B, T);
}

int32_t mi_engine_rell_bootstrap_unrooted(mi_engine* e, int32_t T, const int32_t* parent_ids, const double* bl,
                                          const double* params, int32_t rescaling, int32_t B, const double* weights,
                                          double* out_ll, double* out_pattern_ll, double* out_c, int32_t* out_best,
                                          double* out_bp, double* out_elw) {
  if (!e) return fail("null engine");
  // (a handle of ONE shard has every tree's row on one device: that shard takes the call)
  if (e->shards.size() > 1) return fail(kRellSharded);
  e = first_engine(e);
  if (e->s == kAa) return fail(kPatternLl4State);
  if (T <= 0 || B <= 0) return fail("tree_count and replicate_count must be positive");
  if (!parent_ids || !bl) return fail("null tree arrays");
  if (e->param_count > 0 && !params) return fail("null parameter matrix");
  if (!weights) return fail("null replicate weight matrix");
  if (!out_ll || !out_bp) return fail("null output pointer");
  enum { kInWeights = kTreeInputs };
  enum { kLl, kS, kC, kBest, kBp, kElw };
  const size_t P = e->P;
  HostCall c;
  c.T = T;
  c.in = tree_inputs(e, parent_ids, bl, params);
  c.in.push_back(fixed(weights, (size_t)B * P));
  c.out = {per_tree(out_ll, 1),  per_tree(out_pattern_ll, P), fixed(out_c, (size_t)B * T),
           fixed(out_best, B),   per_tree(out_bp, 1),         per_tree(out_elw, 1)};
  c.enqueue = [=](mi_engine* e, int T, const HostArray* in, const HostArray* out) {
    // (a matrix nobody downloads stays in the engine's workspace)
    if (!out[kS].dev && e->rell_s.ensure(sizeof(double) * (size_t)T * P)) return 1;
    double* d_s = out[kS].dev ? out[kS].at<double>() : e->rell_s.as<double>();
    if (mi_engine_pattern_log_likelihoods_unrooted_device(e, e->stream, T, in[kInParent].at<const int32_t>(),
                                                          in[kInBl].at<const double>(), params_on_device(e, in),
                                                          rescaling, out[kLl].at<double>(), d_s))
      return 1;
    return run_rell_device(e, e->stream, B, T, (int)P, d_s, in[kInWeights].at<const double>(), out[kC].at<double>(),
                           out[kBest].at<int32_t>(), out[kBp].at<double>(), out[kElw].at<double>());
  };
  return run_on_engine(e, c);
}

int32_t mi_engine_pattern_mixture(mi_engine* e, int32_t T, int32_t P, const double* pattern_ll,
                                  const double* tree_log_weights, const double* pattern_weights,
                                  double* out_pattern, double* out_total) {
  if (!e) return fail("null engine");
  if (T <= 0 || P <= 0) return fail("tree_count and pattern_count must be positive");
  if (!pattern_ll || !pattern_weights) return fail("null pattern log-likelihood matrix / pattern weights");
  if (!out_pattern || !out_total) return fail("null output pointer");
  HostCall c;
  c.in = {fixed(pattern_ll, (size_t)T * P), fixed(tree_log_weights, T), fixed(pattern_weights, P)};
  c.out = {fixed(out_pattern, P), fixed(out_total, 1)};
  c.enqueue = [=](mi_engine* e, int, const HostArray* in, const HostArray* out) {
    return run_mixture_device(e, e->stream, T, P, in[0].at<const double>(), in[1].at<const double>(),
                              in[2].at<const double>(), out[0].at<double>(), out[1].at<double>());
  };
  return run_on_engine(first_engine(e), c);
}

int32_t mi_engine_pattern_mixture_device(mi_engine* e, void* stream, int32_t T, int32_t P, const double* pattern_ll,
                                         const double* tree_log_weights, const double* pattern_weights,
                                         double* out_pattern, double* out_total) {
  if (!e) return fail("null engine");
  if (!e->shards.empty()) return fail(kShardedDeviceCall);
  return run_mixture_device(e, pick_stream(e, stream), T, P, pattern_ll, tree_log_weights, pattern_weights,
                            out_pattern, out_total);
}

}  // extern "C"
