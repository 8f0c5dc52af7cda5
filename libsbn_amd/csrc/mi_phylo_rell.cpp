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

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

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

// The host-pointer forms on one engine (as mi_phylo_nni_search.cpp's): inputs up in one copy,
// the work, outputs back in one copy and the call's one error check.
int begin_host(mi_engine* e) {
  HIP_TRY(hipSetDevice(e->spec.device));
  e->fused_timed_out = false;
  e->pinned.reset();
  if (e->status.ensure(sizeof(int32_t) * kStatusWords)) return 1;
  HIP_TRY(hipMemsetAsync(e->status.ptr, 0, sizeof(int32_t) * kStatusWords, e->stream));
  return 0;
}
int finish_host(mi_engine* e) {
  int rc = check_status(e, e->stream);
  e->fused_timed_out = false;
  if (rc == 0) e->pinned.flush();
  e->pinned.reset();
  return rc;
}

int run_rell_host(mi_engine* e, int B, int T, int P, const double* s, const double* w, double* out_c,
                  int32_t* out_best, double* out_bp, double* out_elw) {
  if (check_rell(B, T, P, s, w, out_bp)) return 1;
  if (begin_host(e)) return 1;
  const void *d_s, *d_w;
  if (upload_pack(e, {{s, sizeof(double) * (size_t)T * P, &d_s}, {w, sizeof(double) * (size_t)B * P, &d_w}})) return 1;
  double *o_c, *o_best, *o_bp, *o_elw;  // (o_best: int32)
  const std::initializer_list<OutPiece> outs = {{out_c, out_c ? (size_t)B * T : 0, &o_c},
                                                {out_best, out_best ? (size_t)B : 0, &o_best, sizeof(int32_t)},
                                                {out_bp, (size_t)T, &o_bp},
                                                {out_elw, out_elw ? (size_t)T : 0, &o_elw}};
  if (place_out_pack(e, outs)) return 1;
  if (run_rell_device(e, e->stream, B, T, P, static_cast<const double*>(d_s), static_cast<const double*>(d_w),
                      out_c ? o_c : nullptr, out_best ? reinterpret_cast<int32_t*>(o_best) : nullptr, o_bp,
                      out_elw ? o_elw : nullptr))
    return 1;
  if (download_pack(e, outs)) return 1;
  return finish_host(e);
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

int run_mixture_host(mi_engine* e, int T, int P, const double* s, const double* lw, const double* pw,
                     double* out_pattern, double* out_total) {
  if (T <= 0 || P <= 0) return fail("tree_count and pattern_count must be positive");
  if (!s || !pw) return fail("null pattern log-likelihood matrix / pattern weights");
  if (!out_pattern || !out_total) return fail("null output pointer");
  if (begin_host(e)) return 1;
  const void *d_s, *d_lw, *d_pw;
  if (upload_pack(e, {{s, sizeof(double) * (size_t)T * P, &d_s},
                      {lw, sizeof(double) * (size_t)T, &d_lw},
                      {pw, sizeof(double) * (size_t)P, &d_pw}}))
    return 1;
  double *o_p, *o_t;
  const std::initializer_list<OutPiece> outs = {{out_pattern, (size_t)P, &o_p}, {out_total, 1, &o_t}};
  if (place_out_pack(e, outs)) return 1;
  if (run_mixture_device(e, e->stream, T, P, static_cast<const double*>(d_s), static_cast<const double*>(d_lw),
                         static_cast<const double*>(d_pw), o_p, o_t))
    return 1;
  if (download_pack(e, outs)) return 1;
  return finish_host(e);
}

struct BootstrapCall {
  int T = 0, B = 0, rescaling = 0;
  const int32_t* parent_ids = nullptr;
  const double* bl = nullptr;
  const double* params = nullptr;
  const double* weights = nullptr;
  double* out_ll = nullptr;
  double* out_s = nullptr;  // may be null
  double* out_c = nullptr;  // may be null
  int32_t* out_best = nullptr;  // may be null
  double* out_bp = nullptr;
  double* out_elw = nullptr;  // may be null
};

int run_bootstrap_host(mi_engine* e, const BootstrapCall& h) {
  const int T = h.T, B = h.B, n = e->n, P = e->P;
  if (e->s == kAa) return fail(kPatternLl4State);
  if (T <= 0 || B <= 0) return fail("tree_count and replicate_count must be positive");
  if (!h.parent_ids || !h.bl) return fail("null tree arrays");
  if (e->param_count > 0 && !h.params) return fail("null parameter matrix");
  if (!h.weights) return fail("null replicate weight matrix");
  if (!h.out_ll || !h.out_bp) return fail("null output pointer");
  if (begin_host(e)) return 1;
  const void *d_parent, *d_bl, *d_params, *d_w;
  if (upload_pack(e, {{h.parent_ids, sizeof(int32_t) * (size_t)T * (2 * n - 3), &d_parent},
                      {h.bl, sizeof(double) * (size_t)T * (2 * n - 2), &d_bl},
                      {e->param_count > 0 ? h.params : nullptr, sizeof(double) * (size_t)T * e->param_count, &d_params},
                      {h.weights, sizeof(double) * (size_t)B * P, &d_w}}))
    return 1;
  if (!d_params) d_params = e->in_pack.ptr;
  // (matrices nobody downloads stay in the engine's workspace)
  if (!h.out_s && e->rell_s.ensure(sizeof(double) * (size_t)T * P)) return 1;
  double *o_ll, *o_s, *o_c, *o_best, *o_bp, *o_elw;  // (o_best: int32)
  const std::initializer_list<OutPiece> outs = {{h.out_ll, (size_t)T, &o_ll},
                                                {h.out_s, h.out_s ? (size_t)T * P : 0, &o_s},
                                                {h.out_c, h.out_c ? (size_t)B * T : 0, &o_c},
                                                {h.out_best, h.out_best ? (size_t)B : 0, &o_best, sizeof(int32_t)},
                                                {h.out_bp, (size_t)T, &o_bp},
                                                {h.out_elw, h.out_elw ? (size_t)T : 0, &o_elw}};
  if (place_out_pack(e, outs)) return 1;
  double* d_s = h.out_s ? o_s : e->rell_s.as<double>();
  if (mi_engine_pattern_log_likelihoods_unrooted_device(e, e->stream, T, static_cast<const int32_t*>(d_parent),
                                                        static_cast<const double*>(d_bl),
                                                        static_cast<const double*>(d_params), h.rescaling, o_ll, d_s))
    return 1;
  if (run_rell_device(e, e->stream, B, T, P, d_s, static_cast<const double*>(d_w), h.out_c ? o_c : nullptr,
                      h.out_best ? reinterpret_cast<int32_t*>(o_best) : nullptr, o_bp, h.out_elw ? o_elw : nullptr))
    return 1;
  if (download_pack(e, outs)) return 1;
  return finish_host(e);
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

int32_t mi_engine_rell(mi_engine* e, int32_t B, int32_t T, int32_t P, const double* pattern_ll, const double* weights,
                       double* out_c, int32_t* out_best, double* out_bp, double* out_elw) {
  if (!e) return fail("null engine");
  // (the product needs no alignment: a sharded handle of either kind lets its first shard do it)
  mi_engine* one = e->shards.empty() ? e : e->shards[0];
  one->status_tree_offset = 0;
  if (run_rell_host(one, B, T, P, pattern_ll, weights, out_c, out_best, out_bp, out_elw)) {
    one->pinned.reset();
    return 1;
  }
  return 0;
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
  if (e->shards.size() == 1) e = e->shards[0];
  BootstrapCall h;
  h.T = T;
  h.B = B;
  h.rescaling = rescaling;
  h.parent_ids = parent_ids;
  h.bl = bl;
  h.params = params;
  h.weights = weights;
  h.out_ll = out_ll;
  h.out_s = out_pattern_ll;
  h.out_c = out_c;
  h.out_best = out_best;
  h.out_bp = out_bp;
  h.out_elw = out_elw;
  e->status_tree_offset = 0;
  if (run_bootstrap_host(e, h)) {
    e->pinned.reset();
    return 1;
  }
  return 0;
}

int32_t mi_engine_pattern_mixture(mi_engine* e, int32_t T, int32_t P, const double* pattern_ll,
                                  const double* tree_log_weights, const double* pattern_weights,
                                  double* out_pattern, double* out_total) {
  if (!e) return fail("null engine");
  mi_engine* one = e->shards.empty() ? e : e->shards[0];
  one->status_tree_offset = 0;
  if (run_mixture_host(one, T, P, pattern_ll, tree_log_weights, pattern_weights, out_pattern, out_total)) {
    one->pinned.reset();
    return 1;
  }
  return 0;
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
