// Host-pointer entry points of the C ABI: staging through pinned memory, one DMA each way per
// call, and the sharded handles (several devices / logical shards behind one engine handle).
#include "mi_phylo_engine.h"

namespace {

// One host-pointer call; `begin` stages the inputs, enqueues the device call and the
// downloads on the engine's stream, `finish_host_call` synchronises once and hands the
// staged outputs over.  A sharded handle begins the call on every shard before it finishes
// any, so the devices work side by side.
struct HostCall {
  bool gradient = false, rooted = false;
  int T = 0, rescaling = 0, with_jacobian = 0;
  const int32_t* parent_ids = nullptr;
  const double* bl = nullptr;
  const double* params = nullptr;
  const double* rates = nullptr;
  const int32_t* rate_counts = nullptr;
  const double* heights = nullptr;
  const double* bounds = nullptr;
  const double* ratios = nullptr;
  double* out_ll = nullptr;
  double* out_a = nullptr;  // branch gradient [T][N] (unrooted) / ratios [T][n-1] (rooted)
  double* out_b = nullptr;  // clock gradient [T][N-1] (rooted)
  double* out_site = nullptr;
  double* out_subst = nullptr;
  // branch-length Hessian call (mi_engine_branch_hessian_unrooted): out_ll and out_a
  // (gradient) may be null there
  bool hessian = false;
  double* out_h = nullptr;  // [T][N]
  double* out_s = nullptr;  // [T][N] or null
  // NNI neighbourhood scan (mi_engine_nni_scan_unrooted): out_ll and out_best may be null there
  bool nni = false;
  double* out_nni = nullptr;    // [T][N][2]
  int32_t* out_best = nullptr;  // [T] or null
  // per-pattern log-likelihoods (mi_engine_pattern_log_likelihoods_unrooted): out_ll may be null there
  bool pattern = false;
  double* out_pattern = nullptr;  // [T][P]
  // ancestral states (mi_engine_ancestral_states_unrooted): out_ll and all but out_anc_state may be null there
  bool ancestral = false;
  double* out_anc_state = nullptr;  // [T][n-2][P][4]
  int8_t* out_anc_map = nullptr;    // [T][n-2][P]
  double* out_anc_cat = nullptr;    // [T][P][K]
  double* out_anc_rate = nullptr;   // [T][P]
  double* out_anc_tip = nullptr;    // [T][n][P][4]
  // fused reductions of a variational-inference step (mi_engine_gradients_unrooted_reduced)
  bool reduced = false;
  const int32_t* branch_index = nullptr;  // [T][N]
  const double* tree_weights = nullptr;   // [T] or null
  int index_count = 0;
  double* out_sum = nullptr;         // [2]: sum w logL, sum w site gradient
  double* out_index_grad = nullptr;  // [index_count]
};

// One DMA each way per host-pointer call (round 5; until then one per array: a memset, three to
// eight uploads and three to five downloads, each its own submission and its own turn on the
// stream -- 60 to 80 of the 930 microseconds of a 1000-tree DS1 call).  Inputs are packed into
// one pinned block and copied to one device block; the outputs live in one device block and
// come back as one copy, the pieces handed to the caller's arrays after the call's one
// synchronisation.  Pieces are 256-byte aligned.
// (InPiece, OutPiece: mi_phylo_engine.h)
size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
size_t padded_bytes(const OutPiece& p) { return align256(p.elem * p.count); }

}  // namespace

int upload_pack(mi_engine* e, std::initializer_list<InPiece> pieces) {
  size_t total = 0;
  for (const InPiece& p : pieces) total += p.host ? align256(p.bytes) : 0;
  if (e->in_pack.ensure(std::max<size_t>(total, 256))) return 1;
  char* pin = total ? static_cast<char*>(e->pinned.alloc(total, e->stream)) : nullptr;
  if (total && !pin) return fail("pinned staging allocation failed");
  size_t off = 0;
  for (const InPiece& p : pieces) {
    if (!p.host) {
      *p.dev = nullptr;
      continue;
    }
    memcpy(pin + off, p.host, p.bytes);
    *p.dev = static_cast<char*>(e->in_pack.ptr) + off;
    off += align256(p.bytes);
  }
  if (total) HIP_TRY(hipMemcpyAsync(e->in_pack.ptr, pin, total, hipMemcpyHostToDevice, e->stream));
  return 0;
}
// device addresses of the outputs (before the kernels are enqueued) ...
int place_out_pack(mi_engine* e, std::initializer_list<OutPiece> pieces) {
  size_t total = 0;
  for (const OutPiece& p : pieces) total += padded_bytes(p);
  if (e->out_pack.ensure(std::max<size_t>(total, 256))) return 1;
  size_t off = 0;
  for (const OutPiece& p : pieces) {
    *p.dev = reinterpret_cast<double*>(static_cast<char*>(e->out_pack.ptr) + off);
    off += padded_bytes(p);
  }
  return 0;
}
// ... and their one copy back (after them): the wanted pieces are delivered by finish_host_call
int download_pack(mi_engine* e, std::initializer_list<OutPiece> pieces) {
  size_t total = 0;
  for (const OutPiece& p : pieces) total += padded_bytes(p);
  if (!total) return 0;
  char* pin = static_cast<char*>(e->pinned.alloc(total, e->stream));
  if (!pin) return fail("pinned staging allocation failed");
  HIP_TRY(hipMemcpyAsync(pin, e->out_pack.ptr, total, hipMemcpyDeviceToHost, e->stream));
  size_t off = 0;
  for (const OutPiece& p : pieces) {
    if (p.host && p.count) e->pinned.pending.push_back({p.host, pin + off, p.elem * p.count});
    off += padded_bytes(p);
  }
  return 0;
}

namespace {

int begin_host_call(mi_engine* e, const HostCall& h) {
  const int T = h.T, n = e->n, N = e->N;
  if (T <= 0) return fail("tree_count must be positive");
  if (!h.parent_ids || !h.bl) return fail("null tree arrays");
  if (e->param_count > 0 && !h.params) return fail("null parameter matrix");
  HIP_TRY(hipSetDevice(e->spec.device));
  e->fused_timed_out = false;  // (what an earlier device-pointer call left unread is not this call's)
  e->pinned.reset();  // nothing of an earlier (possibly failed) call is delivered late
  // The status word is sticky (the *_device calls never clear it).  A host-pointer call
  // reports ITS OWN errors only: whatever an earlier device-pointer call left unread on this
  // engine's stream is dropped here, not blamed on this batch.
  HIP_TRY(hipMemsetAsync(e->status.ptr, 0, sizeof(int32_t) * kStatusWords, e->stream));
  const size_t np = h.rooted ? 2 * n - 2 : 2 * n - 3, nb = np + 1;
  const bool tt = h.rooted && h.rates && h.heights && h.bounds;
  const bool gtr = e->spec.subst_model == MI_SUBST_GTR;
  if (h.rooted && h.gradient) {
    if (!tt || !h.rate_counts || !h.ratios) return fail("null time-tree arrays");
    for (int t = 0; t < T; t++)
      if (h.rate_counts[t] != 1 && h.rate_counts[t] != N - 1)
        return fail(status_message(kBadRateCount));
  }
  const void *d_parent, *d_bl, *d_params, *d_rates, *d_heights, *d_bounds, *d_counts, *d_ratios,
      *d_index, *d_weights;
  if (upload_pack(e, {{h.parent_ids, sizeof(int32_t) * (size_t)T * np, &d_parent},
                      {h.bl, sizeof(double) * (size_t)T * nb, &d_bl},
                      {e->param_count > 0 ? h.params : nullptr, sizeof(double) * (size_t)T * e->param_count, &d_params},
                      {tt ? h.rates : nullptr, sizeof(double) * (size_t)T * (N - 1), &d_rates},
                      {tt ? h.heights : nullptr, sizeof(double) * (size_t)T * N, &d_heights},
                      {tt ? h.bounds : nullptr, sizeof(double) * (size_t)T * N, &d_bounds},
                      {h.rooted && h.gradient ? h.rate_counts : nullptr, sizeof(int32_t) * (size_t)T, &d_counts},
                      {h.rooted && h.gradient ? h.ratios : nullptr, sizeof(double) * (size_t)T * (n - 1), &d_ratios},
                      {h.reduced ? h.branch_index : nullptr, sizeof(int32_t) * (size_t)T * N, &d_index},
                      {h.reduced ? h.tree_weights : nullptr, sizeof(double) * (size_t)T, &d_weights}}))
    return 1;
  // (an engine without parameters still hands the kernels a valid pointer)
  if (!d_params) d_params = e->in_pack.ptr;
  auto P32 = [](const void* p) { return static_cast<const int32_t*>(p); };
  auto F64 = [](const void* p) { return static_cast<const double*>(p); };
  double *o_ll, *o_a, *o_b, *o_site, *o_subst, *o_sum, *o_index;
  if (h.hessian) {
    double *o_h, *o_s;
    const std::initializer_list<OutPiece> outs = {{h.out_ll, h.out_ll ? (size_t)T : 0, &o_ll},
                                                  {h.out_a, h.out_a ? (size_t)T * N : 0, &o_a},
                                                  {h.out_h, (size_t)T * N, &o_h},
                                                  {h.out_s, h.out_s ? (size_t)T * N : 0, &o_s}};
    if (place_out_pack(e, outs)) return 1;
    if (mi_engine_branch_hessian_unrooted_device(e, e->stream, T, P32(d_parent), F64(d_bl), F64(d_params),
                                                 h.rescaling, h.out_ll ? o_ll : nullptr,
                                                 h.out_a ? o_a : nullptr, o_h, h.out_s ? o_s : nullptr))
      return 1;
    return download_pack(e, outs);
  }
  if (h.nni) {
    double *o_d, *o_best;
    const std::initializer_list<OutPiece> outs = {{h.out_ll, h.out_ll ? (size_t)T : 0, &o_ll},
                                                  {h.out_nni, (size_t)T * N * 2, &o_d},
                                                  {h.out_best, h.out_best ? (size_t)T : 0, &o_best, sizeof(int32_t)}};
    if (place_out_pack(e, outs)) return 1;
    if (mi_engine_nni_scan_unrooted_device(e, e->stream, T, P32(d_parent), F64(d_bl), F64(d_params), h.rescaling,
                                           h.out_ll ? o_ll : nullptr, o_d,
                                           h.out_best ? reinterpret_cast<int32_t*>(o_best) : nullptr))
      return 1;
    return download_pack(e, outs);
  }
  if (h.pattern) {
    double* o_p;
    const std::initializer_list<OutPiece> outs = {{h.out_ll, h.out_ll ? (size_t)T : 0, &o_ll},
                                                  {h.out_pattern, (size_t)T * e->P, &o_p}};
    if (place_out_pack(e, outs)) return 1;
    if (mi_engine_pattern_log_likelihoods_unrooted_device(e, e->stream, T, P32(d_parent), F64(d_bl), F64(d_params),
                                                          h.rescaling, h.out_ll ? o_ll : nullptr, o_p))
      return 1;
    return download_pack(e, outs);
  }
  if (h.ancestral) {
    // (what nobody asked for is neither computed nor placed nor copied)
    double *o_state, *o_map, *o_cat, *o_rate, *o_tip;
    const size_t P = e->P, rows = (size_t)T * (n - 2) * P;
    const std::initializer_list<OutPiece> outs = {{h.out_ll, h.out_ll ? (size_t)T : 0, &o_ll},
                                                  {h.out_anc_state, rows * 4, &o_state},
                                                  {h.out_anc_map, h.out_anc_map ? rows : 0, &o_map, sizeof(int8_t)},
                                                  {h.out_anc_cat, h.out_anc_cat ? (size_t)T * P * e->K : 0, &o_cat},
                                                  {h.out_anc_rate, h.out_anc_rate ? (size_t)T * P : 0, &o_rate},
                                                  {h.out_anc_tip, h.out_anc_tip ? (size_t)T * n * P * 4 : 0, &o_tip}};
    if (place_out_pack(e, outs)) return 1;
    if (mi_engine_ancestral_states_unrooted_device(e, e->stream, T, P32(d_parent), F64(d_bl), F64(d_params), h.rescaling,
                                                   h.out_ll ? o_ll : nullptr, o_state,
                                                   h.out_anc_map ? reinterpret_cast<int8_t*>(o_map) : nullptr,
                                                   h.out_anc_cat ? o_cat : nullptr, h.out_anc_rate ? o_rate : nullptr,
                                                   h.out_anc_tip ? o_tip : nullptr))
      return 1;
    return download_pack(e, outs);
  }
  if (!h.gradient) {
    const std::initializer_list<OutPiece> outs = {{h.out_ll, (size_t)T, &o_ll}};
    if (place_out_pack(e, outs)) return 1;
    int rc;
    if (!h.rooted)
      rc = mi_engine_log_likelihoods_unrooted_device(e, e->stream, T, P32(d_parent), F64(d_bl),
                                                     F64(d_params), h.rescaling, o_ll);
    else
      rc = mi_engine_log_likelihoods_rooted_device(e, e->stream, T, P32(d_parent), F64(d_bl),
                                                   F64(d_params), F64(d_rates), F64(d_heights),
                                                   F64(d_bounds), h.with_jacobian, h.rescaling, o_ll);
    if (rc) return 1;
    return download_pack(e, outs);
  }
  const bool site = e->K > 1, want_site = site && h.out_site, want_subst = gtr && h.out_subst;
  if (!h.rooted && h.reduced) {
    const std::initializer_list<OutPiece> outs = {{h.out_ll, (size_t)T, &o_ll},
                                                  {h.out_sum, 2, &o_sum},
                                                  {h.out_index_grad, (size_t)h.index_count, &o_index}};
    if (place_out_pack(e, outs)) return 1;
    if (mi_engine_gradients_unrooted_reduced_device(e, e->stream, T, P32(d_parent), F64(d_bl), F64(d_params),
                                                    h.rescaling, P32(d_index), F64(d_weights),
                                                    h.index_count, o_sum, o_index, o_ll))
      return 1;
    return download_pack(e, outs);
  }
  // (outputs nobody wants are neither computed -- NULL skips their work -- nor copied)
  const size_t a_count = h.rooted ? (size_t)T * (n - 1) : (size_t)T * N;
  const std::initializer_list<OutPiece> outs = {{h.out_ll, (size_t)T, &o_ll},
                                                {h.out_a, a_count, &o_a},
                                                {h.out_b, h.rooted ? (size_t)T * (N - 1) : 0, &o_b},
                                                {h.out_site, want_site ? (size_t)T : 0, &o_site},
                                                {h.out_subst, want_subst ? (size_t)T * 8 : 0, &o_subst}};
  if (place_out_pack(e, outs)) return 1;
  int rc;
  if (!h.rooted)
    rc = mi_engine_gradients_unrooted_device(e, e->stream, T, P32(d_parent), F64(d_bl), F64(d_params),
                                             h.rescaling, o_ll, o_a, want_site ? o_site : nullptr,
                                             want_subst ? o_subst : nullptr);
  else
    rc = mi_engine_gradients_rooted_device(e, e->stream, T, P32(d_parent), F64(d_bl), F64(d_params),
                                           F64(d_rates), P32(d_counts), F64(d_heights), F64(d_bounds),
                                           F64(d_ratios), h.rescaling, o_ll, o_a, o_b,
                                           want_site ? o_site : nullptr, want_subst ? o_subst : nullptr);
  if (rc) return 1;
  return download_pack(e, outs);
}

// End of a host-pointer call: one synchronisation (inside check_status), then the staged
// outputs are copied to the caller's buffers.  A time-out of the one-launch call (see
// check_status) does not reach the caller: the call is run again, now through the four-launch
// sequence -- fresh launches in the same process, nothing else is restarted -- and ITS results
// and errors are what the caller gets (the reference never fails spuriously:
// src/engine.cpp:54-92).
int finish_host_call(mi_engine* e, const HostCall& h) {
  int rc = check_status(e, e->stream);
  if (e->fused_timed_out) {
    e->fused_timed_out = false;
    e->fused_fallbacks++;
    e->pinned.reset();
    rc = begin_host_call(e, h);
    if (rc == 0) rc = check_status(e, e->stream);
    e->fused_timed_out = false;
  }
  if (rc == 0) e->pinned.flush();
  e->pinned.reset();
  return rc;
}

// A sharded handle: trees dealt to the shards in contiguous blocks (what
// FatBeagleParallelize's work queue does with thread_count FatBeagles,
// fat_beagle.hpp:119-149), or -- few trees, very long alignments -- every shard evaluates
// all trees on its own block of site patterns and the per-tree results, sums over
// patterns every one of them, are added in shard order.
int run_sharded(mi_engine* e, const HostCall& h) {
  const int D = (int)e->shards.size(), T = h.T;
  const int n = e->n, N = e->N;
  if (T <= 0) return fail("tree_count must be positive");
  if (e->shard_mode == MI_SHARD_TREES) {
    std::vector<int> started;
    std::vector<HostCall> calls(D);
    int rc = 0;
    for (int i = 0; i < D && !rc; i++) {
      int32_t b = 0, c = 0;
      mi_shard_range(T, D, i, &b, &c);
      if (c == 0) continue;
      HostCall s = h;
      s.T = c;
      const size_t np = h.rooted ? 2 * n - 2 : 2 * n - 3, nb = np + 1;
      s.parent_ids = h.parent_ids + (size_t)b * np;
      s.bl = h.bl + (size_t)b * nb;
      if (h.params) s.params = h.params + (size_t)b * e->param_count;
      if (h.rates) s.rates = h.rates + (size_t)b * (N - 1);
      if (h.rate_counts) s.rate_counts = h.rate_counts + b;
      if (h.heights) s.heights = h.heights + (size_t)b * N;
      if (h.bounds) s.bounds = h.bounds + (size_t)b * N;
      if (h.ratios) s.ratios = h.ratios + (size_t)b * (n - 1);
      if (h.out_ll) s.out_ll = h.out_ll + b;
      if (h.out_a) s.out_a = h.out_a + (size_t)b * (h.rooted ? n - 1 : N);
      if (h.out_b) s.out_b = h.out_b + (size_t)b * (N - 1);
      if (h.out_site) s.out_site = h.out_site + b;
      if (h.out_subst) s.out_subst = h.out_subst + (size_t)b * 8;
      if (h.out_h) s.out_h = h.out_h + (size_t)b * N;
      if (h.out_s) s.out_s = h.out_s + (size_t)b * N;
      if (h.out_nni) s.out_nni = h.out_nni + (size_t)b * N * 2;
      if (h.out_best) s.out_best = h.out_best + b;
      if (h.out_pattern) s.out_pattern = h.out_pattern + (size_t)b * e->P;
      if (h.out_anc_state) s.out_anc_state = h.out_anc_state + (size_t)b * (n - 2) * e->P * 4;
      if (h.out_anc_map) s.out_anc_map = h.out_anc_map + (size_t)b * (n - 2) * e->P;
      if (h.out_anc_cat) s.out_anc_cat = h.out_anc_cat + (size_t)b * e->P * e->K;
      if (h.out_anc_rate) s.out_anc_rate = h.out_anc_rate + (size_t)b * e->P;
      if (h.out_anc_tip) s.out_anc_tip = h.out_anc_tip + (size_t)b * n * e->P * 4;
      if (h.reduced) {
        s.branch_index = h.branch_index + (size_t)b * N;
        if (h.tree_weights) s.tree_weights = h.tree_weights + b;
        e->shard_sums.resize((size_t)D * (2 + h.index_count));
        s.out_sum = e->shard_sums.data() + (size_t)i * (2 + h.index_count);
        s.out_index_grad = s.out_sum + 2;
      }
      e->shards[i]->status_tree_offset = b;
      calls[i] = s;
      rc = begin_host_call(e->shards[i], s);
      started.push_back(i);
    }
    for (int i : started) rc |= finish_host_call(e->shards[i], calls[i]);
    if (rc) return 1;
    if (h.reduced) {  // partial sums added in shard order: deterministic
      h.out_sum[0] = h.out_sum[1] = 0;
      for (int k = 0; k < h.index_count; k++) h.out_index_grad[k] = 0;
      for (int i : started) {
        const double* s = e->shard_sums.data() + (size_t)i * (2 + h.index_count);
        h.out_sum[0] += s[0];
        h.out_sum[1] += s[1];
        for (int k = 0; k < h.index_count; k++) h.out_index_grad[k] += s[2 + k];
      }
    }
    return 0;
  }
  // pattern shards: only what is a plain sum over site patterns
  if (h.pattern)
    return fail("pattern-sharded engines do not hand out per-pattern log-likelihoods (each shard holds a "
                "block of columns): use MI_SHARD_TREES or a single engine");
  if (h.ancestral)
    return fail("pattern-sharded engines do not hand out per-pattern posteriors (each shard holds a block of "
                "columns): use MI_SHARD_TREES or a single engine");
  if (h.rooted)
    return fail("pattern-sharded engines evaluate unrooted calls only (the log-det-Jacobian "
                "and the rooted chain rule are not sums over site patterns)");
  // (a Hessian call: per shard logL, gradient, H and S, [T] + 3 [T][N]; H = D2 term - S adds
  // up shard by shard like the rest)
  // (an NNI scan: per shard logL and delta, [T] + [T][N][2]; the best move is taken from the sums)
  const size_t per = (size_t)T * (1 + (h.gradient ? N + 1 + 8 : 0) + (h.hessian ? 3 * N : 0) + (h.nni ? 2 * N : 0)) + 2 + h.index_count;
  e->shard_sums.assign((size_t)D * per, 0.0);
  int rc = 0, started = 0;
  std::vector<HostCall> calls(D);
  for (int i = 0; i < D && !rc; i++, started++) {
    double* base = e->shard_sums.data() + (size_t)i * per;
    HostCall s = h;
    s.out_ll = base;
    if (h.hessian) {
      s.out_a = h.out_a ? base + T : nullptr;
      s.out_h = base + (size_t)T * (1 + N);
      s.out_s = h.out_s ? base + (size_t)T * (1 + 2 * N) : nullptr;
    }
    if (h.nni) {
      s.out_nni = base + T;
      s.out_best = nullptr;
    }
    if (h.gradient) {
      s.out_a = base + T;
      s.out_site = h.out_site ? base + (size_t)T * (1 + N) : nullptr;
      s.out_subst = h.out_subst ? base + (size_t)T * (2 + N) : nullptr;
    }
    if (h.reduced) {
      s.out_sum = base + (size_t)T * (1 + (h.gradient ? N + 1 + 8 : 0));
      s.out_index_grad = s.out_sum + 2;
    }
    calls[i] = s;
    rc = begin_host_call(e->shards[i], s);
  }
  for (int i = 0; i < started; i++) rc |= finish_host_call(e->shards[i], calls[i]);
  if (rc) return 1;
  auto add = [&](double* out, size_t off, size_t count) {
    if (!out) return;
    for (size_t k = 0; k < count; k++) {
      double sum = 0;
      for (int i = 0; i < D; i++) sum += e->shard_sums[(size_t)i * per + off + k];
      out[k] = sum;
    }
  };
  add(h.out_ll, 0, T);
  if (h.hessian) {
    add(h.out_a, T, (size_t)T * N);
    add(h.out_h, (size_t)T * (1 + N), (size_t)T * N);
    add(h.out_s, (size_t)T * (1 + 2 * N), (size_t)T * N);
  }
  if (h.nni) {
    add(h.out_nni, T, (size_t)T * N * 2);
    if (h.out_best)
      for (int t = 0; t < T; t++) h.out_best[t] = nni_best_move(n, h.out_nni + (size_t)t * N * 2);
  }
  if (h.gradient) {
    add(h.out_a, T, (size_t)T * N);
    if (e->K > 1) add(h.out_site, (size_t)T * (1 + N), T);
    if (e->spec.subst_model == MI_SUBST_GTR) add(h.out_subst, (size_t)T * (2 + N), (size_t)T * 8);
  }
  if (h.reduced) {
    const size_t off = (size_t)T * (1 + (h.gradient ? N + 1 + 8 : 0));
    add(h.out_sum, off, 2);
    add(h.out_index_grad, off + 2, h.index_count);
  }
  return 0;
}

int run_host(mi_engine* e, const HostCall& h) {
  if (!e) return fail("null engine");
  if (!e->shards.empty()) return run_sharded(e, h);
  if (begin_host_call(e, h)) {
    e->pinned.reset();
    return 1;
  }
  return finish_host_call(e, h);
}

}  // namespace

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
  HostCall h;
  h.T = T;
  h.rescaling = rescaling;
  h.parent_ids = parent_ids;
  h.bl = bl;
  h.params = params;
  h.out_ll = out_ll;
  return run_host(e, h);
}

int32_t mi_engine_gradients_unrooted(mi_engine* e, int32_t T, const int32_t* parent_ids,
                                     const double* bl, const double* params, int32_t rescaling,
                                     double* out_ll, double* out_branch, double* out_site,
                                     double* out_subst) {
  if (!out_ll || !out_branch) return fail("null output");
  HostCall h;
  h.gradient = true;
  h.T = T;
  h.rescaling = rescaling;
  h.parent_ids = parent_ids;
  h.bl = bl;
  h.params = params;
  h.out_ll = out_ll;
  h.out_a = out_branch;
  h.out_site = out_site;
  h.out_subst = out_subst;
  return run_host(e, h);
}

int32_t mi_engine_branch_hessian_unrooted(mi_engine* e, int32_t T, const int32_t* parent_ids,
                                          const double* bl, const double* params, int32_t rescaling,
                                          double* out_ll, double* out_branch, double* out_hess,
                                          double* out_gsq) {
  if (!out_hess) return fail("null branch-Hessian output");
  if (e && e->s == kAa) return fail(kHessian4State);
  HostCall h;
  h.hessian = true;
  h.T = T;
  h.rescaling = rescaling;
  h.parent_ids = parent_ids;
  h.bl = bl;
  h.params = params;
  h.out_ll = out_ll;
  h.out_a = out_branch;
  h.out_h = out_hess;
  h.out_s = out_gsq;
  return run_host(e, h);
}

int32_t mi_engine_nni_scan_unrooted(mi_engine* e, int32_t T, const int32_t* parent_ids, const double* bl,
                                    const double* params, int32_t rescaling, double* out_ll,
                                    double* out_delta, int32_t* out_best) {
  if (!out_delta) return fail("null NNI delta output");
  if (e && e->s == kAa) return fail(kNni4State);
  HostCall h;
  h.nni = true;
  h.T = T;
  h.rescaling = rescaling;
  h.parent_ids = parent_ids;
  h.bl = bl;
  h.params = params;
  h.out_ll = out_ll;
  h.out_nni = out_delta;
  h.out_best = out_best;
  return run_host(e, h);
}

int32_t mi_engine_pattern_log_likelihoods_unrooted(mi_engine* e, int32_t T, const int32_t* parent_ids,
                                                   const double* bl, const double* params, int32_t rescaling,
                                                   double* out_ll, double* out_pattern_ll) {
  if (!out_pattern_ll) return fail("null per-pattern log-likelihood output");
  if (e && e->s == kAa) return fail(kPatternLl4State);
  HostCall h;
  h.pattern = true;
  h.T = T;
  h.rescaling = rescaling;
  h.parent_ids = parent_ids;
  h.bl = bl;
  h.params = params;
  h.out_ll = out_ll;
  h.out_pattern = out_pattern_ll;
  return run_host(e, h);
}

int32_t mi_engine_ancestral_states_unrooted(mi_engine* e, int32_t T, const int32_t* parent_ids, const double* bl,
                                            const double* params, int32_t rescaling, double* out_ll,
                                            double* out_state, int8_t* out_map, double* out_cat, double* out_rate,
                                            double* out_tip) {
  if (!out_state) return fail("null state-posterior output");
  if (e && e->s == kAa) return fail(kAncestral4State);
  HostCall h;
  h.ancestral = true;
  h.T = T;
  h.rescaling = rescaling;
  h.parent_ids = parent_ids;
  h.bl = bl;
  h.params = params;
  h.out_ll = out_ll;
  h.out_anc_state = out_state;
  h.out_anc_map = out_map;
  h.out_anc_cat = out_cat;
  h.out_anc_rate = out_rate;
  h.out_anc_tip = out_tip;
  return run_host(e, h);
}

int32_t mi_engine_gradients_unrooted_reduced(mi_engine* e, int32_t T, const int32_t* parent_ids,
                                             const double* bl, const double* params,
                                             int32_t rescaling, const int32_t* branch_index,
                                             const double* tree_weights, int32_t index_count,
                                             double* out_sums, double* out_index_gradient,
                                             double* out_ll) {
  if (!out_sums || !branch_index || index_count < 0 || (index_count > 0 && !out_index_gradient))
    return fail("null output / index");
  HostCall h;
  h.gradient = true;
  h.reduced = true;
  h.T = T;
  h.rescaling = rescaling;
  h.parent_ids = parent_ids;
  h.bl = bl;
  h.params = params;
  h.branch_index = branch_index;
  h.tree_weights = tree_weights;
  h.index_count = index_count;
  h.out_sum = out_sums;
  h.out_index_grad = out_index_gradient;
  h.out_ll = out_ll;
  return run_host(e, h);
}

int32_t mi_engine_log_likelihoods_rooted(mi_engine* e, int32_t T, const int32_t* parent_ids,
                                         const double* bl, const double* params,
                                         const double* rates, const double* heights,
                                         const double* bounds, int32_t with_jacobian,
                                         int32_t rescaling, double* out_ll) {
  if (!out_ll) return fail("null output");
  HostCall h;
  h.rooted = true;
  h.T = T;
  h.rescaling = rescaling;
  h.with_jacobian = with_jacobian;
  h.parent_ids = parent_ids;
  h.bl = bl;
  h.params = params;
  h.rates = rates;
  h.heights = heights;
  h.bounds = bounds;
  h.out_ll = out_ll;
  return run_host(e, h);
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
  HostCall h;
  h.gradient = true;
  h.rooted = true;
  h.T = T;
  h.rescaling = rescaling;
  h.parent_ids = parent_ids;
  h.bl = bl;
  h.params = params;
  h.rates = rates;
  h.rate_counts = rate_counts;
  h.heights = heights;
  h.bounds = bounds;
  h.ratios = ratios;
  h.out_ll = out_ll;
  h.out_a = out_ratios;
  h.out_b = out_clock;
  h.out_site = out_site;
  h.out_subst = out_subst;
  return run_host(e, h);
}

}  // extern "C"
