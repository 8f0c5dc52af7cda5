// The variational fit over the rooted trees of the subsplit DAG: the pieces of a
// step as calls of their own (mi_gp_reserve_vi, mi_gp_log_normalize, mi_gp_branch_sample,
// mi_gp_branch_gradient, mi_gp_topology_gradient), the fit object (mi_gp_vi_create), its step as one
// chain of launches and its rooted particles (mi_gp_vi_particles).  The kernels are kernels_gp_vi.hip's,
// the tree-building and de-rooting kernels kernels_gp_trees.hip's, the factors kernels_sbn_vi.hip's,
// the optimiser kernels_vi_fit.hip's.  A *_device form enqueues on the caller's stream and allocates and
// synchronises nothing; a host form reserves on first use and is one HostCall on the object's engine
// (DESIGN.md 4.14).  Every mi_vi_* call serves the fit made here (mi_phylo_vi.cpp).
#include <cmath>
#include <vector>

#include "mi_phylo_engine.h"
#include "mi_phylo_gp_host.h"
#include "mi_phylo_gp_vi.h"
#include "mi_phylo_vi_host.h"

namespace {

int check_rate(double rate) {
  if (!(rate > 0.0) || std::isinf(rate)) return fail("generalized pruning: prior_rate must be finite and positive");
  return 0;
}
int check_estimator(int estimator, int T) {
  if (estimator != MI_SBN_FACTORS_PLAIN && estimator != MI_SBN_FACTORS_VIMCO && estimator != MI_SBN_FACTORS_GIVEN)
    return fail("generalized pruning: estimator must be MI_SBN_FACTORS_PLAIN, MI_SBN_FACTORS_VIMCO or MI_SBN_FACTORS_GIVEN");
  if (estimator == MI_SBN_FACTORS_VIMCO && T < 2) return fail("generalized pruning: the VIMCO estimator needs at least 2 trees");
  return 0;
}

// ---- the launches, from device pointers ----
void enqueue_normalize(const mi_gp* g, hipStream_t s, const double* log_params, double* out_log_q, double* out_q) {
  GpViNormArgs a{};
  a.n = g->d.n;
  a.nodes = g->d.nodes;
  a.R = g->d.R;
  a.G = g->d.G;
  a.block_range = g->d_block;
  a.log_params = log_params;
  a.status = g->e->status.as<int32_t>();
  a.out_log_q = out_log_q;
  a.out_q = out_q;
  launch_gp_vi_normalize(a, s);
}

void enqueue_factors(hipStream_t s, int T, int estimator, const double* log_f, double* sums, double* out_factors) {
  SbnGradientArgs a{};
  a.T = T;
  a.estimator = estimator;
  a.log_f = log_f;
  a.sums = sums;
  a.out_factors = out_factors;
  launch_sbn_factors(a, s);
}

// the sort's arrays of a reservation or of a fit
struct SortWork {
  uint32_t *keys, *keys2, *vals, *vals2;
  void* tmp;
  size_t tmp_bytes;
};
int enqueue_sums(const mi_gp* g, hipStream_t s, int T, const int32_t* entries, const double* terms, const double* factors,
                 const double* q, const SortWork& w, double* usage, double* out_q_gradient, double* out_gradient) {
  GpViSumsArgs a{};
  a.n = g->d.n;
  a.T = T;
  a.G = g->d.G;
  a.nodes = g->d.nodes;
  a.R = g->d.R;
  a.entries = entries;
  a.block_range = g->d_block;
  a.terms = terms;
  a.factors = factors;
  a.q = q;
  a.keys = w.keys;
  a.keys2 = w.keys2;
  a.vals = w.vals;
  a.vals2 = w.vals2;
  a.sort_tmp = w.tmp;
  a.sort_tmp_bytes = w.tmp_bytes;
  a.usage = usage;
  a.out_q_gradient = out_q_gradient;
  a.out_gradient = out_gradient;
  if (launch_gp_vi_sums(a, s)) return fail("generalized pruning: the radix sort of the particles' entries failed");
  return 0;
}

// ---- the by-value calls' reservation ----
size_t lay_vi(const mi_gp* g, int cap, char* base, mi_gp::ViWork& w) {
  const size_t G = g->d.G, N = 2 * (size_t)g->d.n - 1, T = (size_t)cap;
  Cutter c{base};
  c.take(w.log_q, G);
  c.take(w.qn, G);
  c.take(w.usage, G);
  c.take(w.sums, 2);
  c.take(w.factors, T);
  c.take(w.terms, T * (N - 1) * 2);
  return c.at;
}

int reserve_vi(mi_gp* g, int cap) {
  if (cap < 1) return fail("generalized pruning: tree_capacity must be positive");
  if ((size_t)cap * (2 * (size_t)g->d.n - 1) >= ((size_t)1 << 32))
    return fail("generalized pruning: " + std::to_string(cap) + " trees of " + std::to_string(g->d.n) +
                " taxa have 2^32 (tree, node) positions or more; take fewer trees per call");
  if (mi_gp_reserve_trees(g, cap)) return 1;
  if (cap <= g->vi_capacity) return 0;
  mi_engine* e = g->e;
  mi_gp::ViWork w{};
  const size_t bytes = lay_vi(g, cap, nullptr, w);
  if (bytes > e->plv_budget)
    return fail("generalized pruning: the variational workspace of " + std::to_string(cap) + " trees of " + std::to_string(g->d.n) +
                " taxa takes " + std::to_string(bytes) + " bytes, over the budget of " + std::to_string(e->plv_budget) +
                " bytes (MI_PHYLO_PLV_BYTES); take fewer trees per call");
  HIP_TRY(hipSetDevice(e->spec.device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  g->vi_capacity = 0;
  if (g->vi_ws.ensure(bytes)) return 1;
  HIP_TRY(hipMemset(g->vi_ws.ptr, 0, bytes));
  lay_vi(g, cap, g->vi_ws.as<char>(), g->vw);
  g->vi_capacity = cap;
  return 0;
}

int check_vi_reserved(const mi_gp* g, int T, const char* call) {
  if (T < 1) return fail("tree_count must be positive");
  if (T > g->vi_capacity)
    return fail(std::string("generalized pruning: ") + call + " of " + std::to_string(T) + " trees, mi_gp_reserve_vi reserved " +
                std::to_string(g->vi_capacity) + " (the device form allocates nothing)");
  return 0;
}

SortWork sort_of(const mi_gp* g) {
  const GpTrainArgs& t = g->train;
  return SortWork{t.keys, t.keys2, t.vals, t.vals2, t.sort_tmp, t.sort_tmp_bytes};
}

void note(mi_gp* g, const char* kernel, const char* what, int T) {
  mi_engine* e = g->e;
  e->dominant = kernel;
  e->last_path = std::string(what) + " n=" + std::to_string(g->d.n) + " T=" + std::to_string(T) + " G=" + std::to_string(g->d.G);
}

// ---- the fit ----
size_t cut_fit(mi_vi* v, char* base) {
  const size_t K = v->K, N = 2 * (size_t)v->n - 1, G = v->P;
  Cutter c{base};
  c.take(v->state, 1);
  c.take(v->phi, G);
  c.take(v->q, 2 * G);
  c.take(v->m_sbn, G);
  c.take(v->v_sbn, G);
  c.take(v->m_q, 2 * G);
  c.take(v->v_q, 2 * G);
  c.take(v->params, K * (size_t)v->pc);
  c.take(v->log_q, G);
  c.take(v->qn, G);
  c.take(v->r_parents, K * (N - 1));
  c.take(v->r_entries, K * N);
  c.take(v->r_lengths, K * N);
  c.take(v->eps, K * (N - 1));
  c.take(v->lqt, K);
  c.take(v->lqb, K);
  c.take(v->lprior, K);
  c.take(v->all_pid, K * (N - 2));
  c.take(v->bl, K * (N - 1));
  c.take(v->edge, K);
  c.take(v->new_id, K * N);
  c.take(v->ll, K);
  c.take(v->g, K * N);
  c.take(v->terms, K * (N - 1) * 2);
  c.take(v->f, K);
  c.take(v->sums, 2);
  c.take(v->factors, K);
  c.take(v->keys, K * N);
  c.take(v->keys2, K * N);
  c.take(v->vals, K * N);
  c.take(v->vals2, K * N);
  v->sort_bytes = gp_train_sort_tmp_bytes(K * N);
  c.take(v->sort_tmp, v->sort_bytes);
  c.take(v->usage, G);
  c.take(v->qgrad, 2 * G);
  c.take(v->grad, G);
  c.take(v->block_flags, (size_t)v->blocks);
  c.take(v->trace, 6 * (size_t)v->o.max_steps);
  return c.at;
}

}  // namespace

std::string gp_vi_path(const mi_vi* v, int steps) {
  return "gp_vi_fit n=" + std::to_string(v->n) + " K=" + std::to_string(v->K) + " G=" + std::to_string(v->P) +
         " steps=" + std::to_string(steps) + " | " + v->grad_path;
}

// normalise | CDF, build | branch draw | de-root | likelihood gradient | terms | factors | ordered sums | update
int gp_vi_enqueue_step(mi_vi* v, hipStream_t s) {
  mi_gp* g = v->gp;
  mi_engine* e = v->e;
  const int K = v->K, n = v->n;
  if (K > g->tree_capacity) return fail("variational fit: the object's tree reservation is gone");
  enqueue_normalize(g, s, v->phi, v->log_q, v->qn);
  GpTreesArgs t = g->t;  // (the object's tables, CDF workspace and per-tree store; the fit's table)
  t.q = v->qn;
  t.b = nullptr;
  launch_gp_tree_cdf(t, nullptr, s);
  launch_gp_tree_build(t, K, 1, v->o.seed, 0, v->state, v->r_parents, v->r_entries, v->lqt, nullptr, s);
  GpViSampleArgs b{};
  b.n = n;
  b.T = K;
  b.G = v->P;
  b.entries = v->r_entries;
  b.q_params = v->q;
  b.seed = v->o.seed;
  b.vi = v->state;
  b.prior_rate = v->o.prior_rate;
  b.status = e->status.as<int32_t>();
  b.out_lengths = v->r_lengths;
  b.out_epsilon = v->eps;
  b.out_log_q = v->lqb;
  b.out_log_prior = v->lprior;
  launch_gp_vi_branch_sample(b, s);
  HIP_TRY(hipGetLastError());
  if (mi_engine_deroot_trees_mapped_device(e, s, K, n, v->r_parents, v->r_lengths, v->all_pid, v->bl, v->edge, v->new_id)) return 1;
  if (mi_engine_gradients_unrooted_device(e, s, K, v->all_pid, v->bl, v->params, 0, v->ll, v->g, nullptr, nullptr)) return 1;
  v->grad_path = e->last_path;
  GpViTermsArgs c{};
  c.n = n;
  c.T = K;
  c.G = v->P;
  c.entries = v->r_entries;
  c.q_params = v->q;
  c.lengths = v->r_lengths;
  c.epsilon = v->eps;
  c.new_id = v->new_id;
  c.branch_gradient = v->g;
  c.log_likelihoods = v->ll;
  c.log_prior = v->lprior;
  c.log_q_branch = v->lqb;
  c.log_q_topology = v->lqt;
  c.beta = 1.0;
  c.prior_rate = v->o.prior_rate;
  c.vi = v->state;
  c.status = e->status.as<int32_t>();
  c.terms = v->terms;
  c.out_log_f = v->f;
  launch_gp_vi_terms(c, s);
  enqueue_factors(s, K, v->o.estimator, v->f, v->sums, v->factors);
  const SortWork w{v->keys, v->keys2, v->vals, v->vals2, v->sort_tmp, v->sort_bytes};
  if (enqueue_sums(g, s, K, v->r_entries, v->terms, v->factors, v->qn, w, v->usage, v->qgrad, v->grad)) return 1;
  HIP_TRY(hipGetLastError());
  return vi_enqueue_update(v, s, v->grad, v->qgrad, v->ll, v->lprior, v->lqt, v->lqb, nullptr);
}

extern "C" {

int32_t mi_gp_reserve_vi(mi_gp* g, int32_t tree_capacity) {
  if (!g) return fail("null object");
  return reserve_vi(g, tree_capacity);
}

int32_t mi_gp_log_normalize_device(mi_gp* g, void* stream, const double* log_params, double* out_log_q, double* out_q) {
  if (!g) return fail("null object");
  if (!log_params || !out_q) return fail("null input or output pointer");
  if (g->vi_capacity < 1) return fail("generalized pruning: mi_gp_log_normalize_device before mi_gp_reserve_vi");
  HIP_TRY(hipSetDevice(g->e->spec.device));
  enqueue_normalize(g, pick_stream(g->e, stream), log_params, out_log_q, out_q);
  HIP_TRY(hipGetLastError());
  note(g, "gp_vi_normalize_kernel", "gp_vi_normalize", 0);
  return 0;
}
int32_t mi_gp_log_normalize(mi_gp* g, const double* log_params, double* out_log_q, double* out_q) {
  if (!g) return fail("null object");
  if (!log_params) return fail("null input pointer");
  if (g->vi_capacity < 1 && reserve_vi(g, 1)) return 1;
  const size_t G = g->d.G;
  Unwanted spare;
  HostCall c;
  c.in = {fixed(log_params, G)};
  c.out = {fixed(out_log_q, G), fixed(spare(out_q, G), G)};
  c.enqueue = [=](mi_engine* e, int, const HostArray* in, const HostArray* out) {
    return mi_gp_log_normalize_device(g, e->stream, in[0].at<const double>(), out[0].at<double>(), out[1].at<double>());
  };
  return run_on_engine(g->e, c);
}

int32_t mi_gp_branch_sample_device(mi_gp* g, void* stream, int32_t T, const int32_t* entries, const double* q_params, uint64_t seed,
                                   int64_t first_sample, double prior_rate, const double* epsilon_in, double* out_lengths,
                                   double* out_epsilon, double* out_log_q, double* out_log_prior) {
  if (!g) return fail("null object");
  if (!entries || !q_params || !out_lengths || !out_epsilon || !out_log_q || !out_log_prior)
    return fail("null input or output pointer");
  if (check_vi_reserved(g, T, "mi_gp_branch_sample_device")) return 1;
  if (first_sample < 0) return fail("generalized pruning: first_sample must not be negative");
  if (check_rate(prior_rate)) return 1;
  HIP_TRY(hipSetDevice(g->e->spec.device));
  GpViSampleArgs a{};
  a.n = g->d.n;
  a.T = T;
  a.G = g->d.G;
  a.entries = entries;
  a.q_params = q_params;
  a.seed = seed;
  a.first_sample = first_sample;
  a.prior_rate = prior_rate;
  a.epsilon_in = epsilon_in;
  a.status = g->e->status.as<int32_t>();
  a.out_lengths = out_lengths;
  a.out_epsilon = out_epsilon;
  a.out_log_q = out_log_q;
  a.out_log_prior = out_log_prior;
  launch_gp_vi_branch_sample(a, pick_stream(g->e, stream));
  HIP_TRY(hipGetLastError());
  note(g, "gp_vi_branch_sample_kernel", "gp_vi_branch_sample", T);
  return 0;
}
int32_t mi_gp_branch_sample(mi_gp* g, int32_t T, const int32_t* entries, const double* q_params, uint64_t seed, int64_t first_sample,
                            double prior_rate, const double* epsilon_in, double* out_lengths, double* out_epsilon,
                            double* out_log_q, double* out_log_prior) {
  if (!g) return fail("null object");
  if (!entries || !q_params) return fail("null input pointer");
  if (T < 1) return fail("tree_count must be positive");
  if (reserve_vi(g, T)) return 1;
  const size_t N = 2 * (size_t)g->d.n - 1, G = g->d.G, K = (size_t)T;
  Unwanted spare;
  HostCall c;
  c.in = {fixed(entries, K * N), fixed(q_params, 2 * G), fixed(epsilon_in, K * (N - 1))};
  c.out = {fixed(spare(out_lengths, K * N), K * N), fixed(spare(out_epsilon, K * (N - 1)), K * (N - 1)),
           fixed(spare(out_log_q, K), K), fixed(spare(out_log_prior, K), K)};
  c.enqueue = [=](mi_engine* e, int, const HostArray* in, const HostArray* out) {
    return mi_gp_branch_sample_device(g, e->stream, T, in[0].at<const int32_t>(), in[1].at<const double>(), seed, first_sample,
                                      prior_rate, in[2].at<const double>(), out[0].at<double>(), out[1].at<double>(),
                                      out[2].at<double>(), out[3].at<double>());
  };
  return run_on_engine(g->e, c);
}

int32_t mi_gp_branch_gradient_device(mi_gp* g, void* stream, int32_t T, const int32_t* entries, const double* q_params,
                                     const double* lengths, const double* epsilon, const double* log_q_branch,
                                     const double* log_prior, const int32_t* new_id, const double* branch_gradient,
                                     const double* log_likelihoods, const double* log_q_topology, const double* tree_weights,
                                     double beta, double prior_rate, double* out_gradient, double* out_log_f) {
  if (!g) return fail("null object");
  if (!entries || !q_params || !lengths || !epsilon || !log_q_branch || !log_prior || !new_id || !branch_gradient ||
      !log_likelihoods || !out_gradient || !out_log_f)
    return fail("null input or output pointer");
  if (check_vi_reserved(g, T, "mi_gp_branch_gradient_device")) return 1;
  if (check_rate(prior_rate)) return 1;
  mi_engine* e = g->e;
  HIP_TRY(hipSetDevice(e->spec.device));
  hipStream_t s = pick_stream(e, stream);
  GpViTermsArgs a{};
  a.n = g->d.n;
  a.T = T;
  a.G = g->d.G;
  a.entries = entries;
  a.q_params = q_params;
  a.lengths = lengths;
  a.epsilon = epsilon;
  a.new_id = new_id;
  a.branch_gradient = branch_gradient;
  a.log_likelihoods = log_likelihoods;
  a.log_prior = log_prior;
  a.log_q_branch = log_q_branch;
  a.log_q_topology = log_q_topology;
  a.weights = tree_weights;
  a.beta = beta;
  a.prior_rate = prior_rate;
  a.status = e->status.as<int32_t>();
  a.terms = g->vw.terms;
  a.out_log_f = out_log_f;
  launch_gp_vi_terms(a, s);
  if (enqueue_sums(g, s, T, entries, g->vw.terms, nullptr, nullptr, sort_of(g), nullptr, out_gradient, nullptr)) return 1;
  HIP_TRY(hipGetLastError());
  note(g, "gp_vi_runs_kernel", "gp_vi_branch_gradient", T);
  return 0;
}
int32_t mi_gp_branch_gradient(mi_gp* g, int32_t T, const int32_t* entries, const double* q_params, const double* lengths,
                              const double* epsilon, const double* log_q_branch, const double* log_prior, const int32_t* new_id,
                              const double* branch_gradient, const double* log_likelihoods, const double* log_q_topology,
                              const double* tree_weights, double beta, double prior_rate, double* out_gradient,
                              double* out_log_f) {
  if (!g) return fail("null object");
  if (!entries || !q_params || !lengths || !epsilon || !log_q_branch || !log_prior || !new_id || !branch_gradient ||
      !log_likelihoods)
    return fail("null input pointer");
  if (T < 1) return fail("tree_count must be positive");
  if (reserve_vi(g, T)) return 1;
  const size_t N = 2 * (size_t)g->d.n - 1, G = g->d.G, K = (size_t)T;
  Unwanted spare;
  HostCall c;
  c.in = {fixed(entries, K * N),         fixed(q_params, 2 * G),  fixed(lengths, K * N),   fixed(epsilon, K * (N - 1)),
          fixed(log_q_branch, K),        fixed(log_prior, K),     fixed(new_id, K * N),    fixed(branch_gradient, K * N),
          fixed(log_likelihoods, K),     fixed(log_q_topology, K), fixed(tree_weights, K)};
  c.out = {fixed(spare(out_gradient, 2 * G), 2 * G), fixed(spare(out_log_f, K), K)};
  c.enqueue = [=](mi_engine* e, int, const HostArray* in, const HostArray* out) {
    return mi_gp_branch_gradient_device(g, e->stream, T, in[0].at<const int32_t>(), in[1].at<const double>(),
                                        in[2].at<const double>(), in[3].at<const double>(), in[4].at<const double>(),
                                        in[5].at<const double>(), in[6].at<const int32_t>(), in[7].at<const double>(),
                                        in[8].at<const double>(), in[9].at<const double>(), in[10].at<const double>(), beta,
                                        prior_rate, out[0].at<double>(), out[1].at<double>());
  };
  return run_on_engine(g->e, c);
}

int32_t mi_gp_topology_gradient_device(mi_gp* g, void* stream, int32_t T, const int32_t* entries, const double* log_params,
                                       const double* log_f, int32_t estimator, double* out_gradient, double* out_factors) {
  if (!g) return fail("null object");
  if (!entries || !log_params || !log_f || !out_gradient) return fail("null input or output pointer");
  if (check_vi_reserved(g, T, "mi_gp_topology_gradient_device")) return 1;
  if (check_estimator(estimator, T)) return 1;
  mi_engine* e = g->e;
  HIP_TRY(hipSetDevice(e->spec.device));
  hipStream_t s = pick_stream(e, stream);
  const mi_gp::ViWork& w = g->vw;
  double* factors = out_factors ? out_factors : w.factors;
  enqueue_normalize(g, s, log_params, nullptr, w.qn);
  enqueue_factors(s, T, estimator, log_f, w.sums, factors);
  if (enqueue_sums(g, s, T, entries, nullptr, factors, w.qn, sort_of(g), w.usage, nullptr, out_gradient)) return 1;
  HIP_TRY(hipGetLastError());
  note(g, "gp_vi_runs_kernel", "gp_vi_topology_gradient", T);
  return 0;
}
int32_t mi_gp_topology_gradient(mi_gp* g, int32_t T, const int32_t* entries, const double* log_params, const double* log_f,
                                int32_t estimator, double* out_gradient, double* out_factors) {
  if (!g) return fail("null object");
  if (!entries || !log_params || !log_f) return fail("null input pointer");
  if (T < 1) return fail("tree_count must be positive");
  if (check_estimator(estimator, T)) return 1;
  if (reserve_vi(g, T)) return 1;
  const size_t N = 2 * (size_t)g->d.n - 1, G = g->d.G, K = (size_t)T;
  Unwanted spare;
  HostCall c;
  c.in = {fixed(entries, K * N), fixed(log_params, G), fixed(log_f, K)};
  c.out = {fixed(spare(out_gradient, G), G), fixed(out_factors, K)};
  c.enqueue = [=](mi_engine* e, int, const HostArray* in, const HostArray* out) {
    return mi_gp_topology_gradient_device(g, e->stream, T, in[0].at<const int32_t>(), in[1].at<const double>(),
                                          in[2].at<const double>(), estimator, out[0].at<double>(), out[1].at<double>());
  };
  return run_on_engine(g->e, c);
}

int32_t mi_gp_vi_create(mi_gp* g, const double* model_params, int32_t P, const double* log_params, int32_t V,
                        const double* q_params, const mi_vi_options* options, mi_vi** out) {
  if (!g) return fail("null object");
  if (!out) return fail("null output pointer");
  *out = nullptr;
  if (g->several_shards) return fail(kShardedDeviceCall);
  if (!options) return fail("variational fit: null options");
  if (options->rows != 1) return fail("variational fit: a fit over a subsplit DAG has one variable per entry; rows must be 1");
  if (vi_check_options(*options)) return 1;
  mi_engine* e = g->e;
  const int n = g->d.n, G = g->d.G, K = options->particle_count;
  if (P != G || V != G)
    return fail("variational fit: the DAG has " + std::to_string(G) + " entries, the tables given " + std::to_string(P) +
                " log parameters and " + std::to_string(V) + " branch-length variables");
  if (!log_params || !q_params) return fail("variational fit: null initial tables");
  for (int j = 0; j < G; j++)
    if (std::isnan(log_params[j]) || log_params[j] == INFINITY)
      return fail("variational fit: log_params must be finite or -inf (entry " + std::to_string(j) + ")");
  if (e->param_count > 0 && !model_params) return fail("variational fit: this engine's model takes parameters");
  if ((size_t)K * (2 * (size_t)n - 1) >= ((size_t)1 << 32)) return fail("variational fit: too many particles for this taxon count");
  if (mi_gp_reserve_trees(g, K) || mi_engine_reserve(e, K, 1) || mi_engine_reserve_deroot(e, K, n)) return 1;
  HIP_TRY(hipSetDevice(e->spec.device));
  if (e->status.ensure(sizeof(int32_t) * kStatusWords)) return 1;
  mi_vi* v = new mi_vi;
  v->e = e;
  v->gp = g;
  v->o = *options;
  v->n = n;
  v->E = 2 * n - 3;
  v->K = K;
  v->R = 1;
  v->S = g->d.R;
  v->P = G;
  v->V = G;
  v->pc = e->param_count;
  v->blocks = vi_update_blocks(G, G);
  const size_t bytes = cut_fit(v, nullptr);
  ViState st{};
  st.first_sample = options->first_sample;
  st.K = K;
  st.anneal_steps = options->anneal_steps;
  st.b0 = st.b1 = 1.0;
  st.step[0] = options->step_size[0];
  st.step[1] = options->step_size[1];
  st.sbn_step = options->sbn_step_size;
  std::vector<double> rows((size_t)K * v->pc);
  for (int k = 0; k < K && model_params; k++)
    for (int j = 0; j < v->pc; j++) rows[(size_t)k * v->pc + j] = model_params[j];
  auto fill = [&]() -> int {
    if (v->pool.ensure(bytes)) return 1;
    HIP_TRY(hipMemset(v->pool.ptr, 0, bytes));  // (the moments start from zero)
    cut_fit(v, v->pool.as<char>());
    if (upload(v->state, &st, sizeof st) || upload(v->phi, log_params, sizeof(double) * G) ||
        upload(v->q, q_params, sizeof(double) * 2 * G) || upload(v->params, rows.data(), sizeof(double) * rows.size()))
      return 1;
    HIP_TRY(hipDeviceSynchronize());  // (the block is whole before a step on any stream reads it)
    return 0;
  };
  if (fill()) {
    delete v;
    return 1;
  }
  *out = v;
  return 0;
}

int32_t mi_gp_vi_particles(mi_vi* v, int32_t* parent_ids, int32_t* entries, double* lengths, double* ll, double* lqt, double* lqb,
                           double* lprior) {
  if (!v) return fail("null fit");
  if (!v->gp) return fail("variational fit: not a fit over a subsplit DAG; mi_vi_particles gives its particles");
  if (!parent_ids) return fail("null output pointer");
  HIP_TRY(hipSetDevice(v->e->spec.device));
  HIP_TRY(hipStreamSynchronize(v->e->stream));
  const size_t K = v->K, N = 2 * (size_t)v->n - 1, d = sizeof(double);
  return download(parent_ids, v->r_parents, sizeof(int32_t) * K * (N - 1)) ||
         download(entries, v->r_entries, sizeof(int32_t) * K * N) || download(lengths, v->r_lengths, d * K * N) ||
         download(ll, v->ll, d * K) || download(lqt, v->lqt, d * K) || download(lqb, v->lqb, d * K) ||
         download(lprior, v->lprior, d * K);
}

}  // extern "C"
