// PSP indexing and the log-normal branch-length models of a variational step:
// the PSP numbering of a support (mi_engine_psp_table*), every tree's index rows
// (mi_engine_psp_index*), the draw with log q and the prior (mi_engine_branch_model_sample*), the
// gradient with respect to the (mu, sigma) tables and log_f (mi_engine_branch_model_gradient*) and
// their reservation.  The device forms only enqueue and report through the status word.  Any engine
// serves: the taxon count is an argument and the alignment plays no part; a sharded handle lets its
// first shard do the work.
#include <cmath>

#include "mi_phylo_engine.h"

namespace {

size_t round256(size_t x) { return (x + 255) & ~(size_t)255; }

// the gradient call's block (mi_engine::branch_ws)
struct GradientLayout {
  size_t Q, sort_bytes;
  size_t terms, keys, keys2, vals, vals2, sort_tmp, total;
};
GradientLayout gradient_layout(int T, int n, int R) {
  GradientLayout l{};
  const size_t E = 2 * (size_t)n - 3;
  l.Q = (size_t)T * R * E;
  l.sort_bytes = branch_model_sort_tmp_bytes(l.Q);
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t here = at;
    at += round256(bytes);
    return here;
  };
  l.terms = take((size_t)T * E * 16);
  l.keys = take(l.Q * 4);
  l.keys2 = take(l.Q * 4);
  l.vals = take(l.Q * 4);
  l.vals2 = take(l.Q * 4);
  l.sort_tmp = take(l.sort_bytes);
  l.total = at;
  return l;
}

int check_shape(const mi_engine* e, int T, int n, int R) {
  if (!e) return fail("null engine");
  if (T < 1) return fail("tree_count must be positive");
  if (n < 3) return fail("the branch-length models need at least 3 taxa");
  if (R != 1 && R != 3) return fail("branch model: rows must be 1 (splits) or 3 (rootsplit, down PSP, up PSP)");
  // (entry numbers are 32-bit)
  if ((size_t)T * (2 * (size_t)n - 3) * 3 >= ((size_t)1 << 30))
    return fail("branch model: 3 tree_count (2 taxon_count - 3) must stay below 2^30");
  return 0;
}

int reserve_gradient(mi_engine* e, int T, int n, int R) {
  const GradientLayout l = gradient_layout(T, n, R);
  if (l.total > e->plv_budget)
    return fail("branch model: " + std::to_string(T) + " trees of " + std::to_string(n) + " taxa need " +
                std::to_string(l.total) + " bytes of workspace, over the budget of " + std::to_string(e->plv_budget) +
                " bytes (MI_PHYLO_PLV_BYTES); the call is not chunked: pass the batch in parts");
  if (e->branch_ws.ensure(l.total)) return 1;
  return e->status.ensure(sizeof(int32_t) * kStatusWords);
}

void note_call(mi_engine* e, const char* kernel, int T, int n, int R) {
  e->dominant = kernel;
  e->last_walk_launches = 1;
  e->last_evals = T;
  e->last_grad_evals = 0;
  e->last_path = "branch_model n=" + std::to_string(n) + " rows=" + std::to_string(R);
}

struct PspTableCall {
  int S = 0, C = 0;
  const int32_t* pcsp_clades = nullptr;
  int32_t *out_psp_of_pcsp = nullptr, *out_counts = nullptr;
};

int check_table_call(const mi_engine* e, const PspTableCall& c) {
  if (!e) return fail("null engine");
  if (c.S < 1 || c.C < 0) return fail("PSP table: bad rootsplit or PCSP count");
  if (c.C > 0 && (!c.pcsp_clades || !c.out_psp_of_pcsp)) return fail("PSP table: null pcsp_clades or output pointer");
  if (!c.out_counts) return fail("null output pointer");
  return 0;
}

int run_psp_table_device(mi_engine* e, hipStream_t s, const PspTableCall& c) {
  if (check_table_call(e, c)) return 1;
  HIP_TRY(hipSetDevice(e->spec.device));
  PspTableArgs a{};
  a.S = c.S;
  a.C = c.C;
  a.pcsp_clades = c.pcsp_clades;
  a.out_psp_of_pcsp = c.out_psp_of_pcsp;
  a.out_counts = c.out_counts;
  launch_psp_table(a, s);
  HIP_TRY(hipGetLastError());
  e->dominant = "psp_table_kernel";
  e->last_walk_launches = 1;
  e->last_evals = e->last_grad_evals = 0;
  e->last_path = "psp_table pcsps=" + std::to_string(c.C);
  return 0;
}

struct PspIndexCall {
  int T = 0, n = 0, S = 0, C = 0, V = 0, R = 0;
  const int32_t *root_index = nullptr, *slot_index = nullptr, *psp_of_pcsp = nullptr;
  int32_t* out_index = nullptr;
};

int check_index_call(const mi_engine* e, const PspIndexCall& c) {
  if (check_shape(e, c.T, c.n, c.R)) return 1;
  if (c.S < 1 || c.C < 0 || c.V < c.S || c.V > c.S + c.C) return fail("PSP index: bad rootsplit, PCSP or variable count");
  if (!c.root_index || (c.R == 3 && !c.slot_index)) return fail("null tree arrays");
  if (c.R == 3 && c.C > 0 && !c.psp_of_pcsp) return fail("PSP index: null psp_of_pcsp");
  if (!c.out_index) return fail("null output pointer");
  return 0;
}

int run_psp_index_device(mi_engine* e, hipStream_t s, const PspIndexCall& c) {
  if (check_index_call(e, c)) return 1;
  HIP_TRY(hipSetDevice(e->spec.device));
  PspIndexArgs a{};
  a.n = c.n;
  a.T = c.T;
  a.S = c.S;
  a.C = c.C;
  a.V = c.V;
  a.R = c.R;
  a.root_index = c.root_index;
  a.slot_index = c.slot_index;
  a.psp_of_pcsp = c.psp_of_pcsp;
  a.out_index = c.out_index;
  launch_psp_index(a, s);
  HIP_TRY(hipGetLastError());
  note_call(e, "psp_index_kernel", c.T, c.n, c.R);
  return 0;
}

struct BranchSampleCall {
  int T = 0, n = 0, R = 0, V = 0;
  const int32_t* index = nullptr;
  const double *q_params = nullptr, *epsilon_in = nullptr;
  uint64_t seed = 0;
  int64_t first_sample = 0;
  double prior_rate = 0.0;
  double *out_bl = nullptr, *out_epsilon = nullptr, *out_log_q = nullptr, *out_log_prior = nullptr;
};

int check_rate(double rate) {
  if (!(rate > 0.0) || std::isinf(rate)) return fail("branch model: prior_rate must be finite and positive");
  return 0;
}

int check_sample_call(const mi_engine* e, const BranchSampleCall& c) {
  if (check_shape(e, c.T, c.n, c.R)) return 1;
  if (c.V < 1) return fail("branch model: variable_count must be positive");
  if (check_rate(c.prior_rate)) return 1;
  if (!c.index || !c.q_params) return fail("branch model: null index or q_params");
  if (!c.out_bl || !c.out_epsilon || !c.out_log_q || !c.out_log_prior) return fail("null output pointer");
  return 0;
}

int run_branch_sample_device(mi_engine* e, hipStream_t s, const BranchSampleCall& c) {
  if (check_sample_call(e, c)) return 1;
  HIP_TRY(hipSetDevice(e->spec.device));
  if (e->status.ensure(sizeof(int32_t) * kStatusWords)) return 1;
  BranchSampleArgs a{};
  a.n = c.n;
  a.T = c.T;
  a.R = c.R;
  a.V = c.V;
  a.index = c.index;
  a.q_params = c.q_params;
  a.seed = c.seed;
  a.first_sample = c.first_sample;
  a.vi = e->vi_state;
  a.prior_rate = c.prior_rate;
  a.epsilon_in = c.epsilon_in;
  a.status = e->status.as<int32_t>();
  a.out_bl = c.out_bl;
  a.out_epsilon = c.out_epsilon;
  a.out_log_q = c.out_log_q;
  a.out_log_prior = c.out_log_prior;
  launch_branch_sample(a, s);
  HIP_TRY(hipGetLastError());
  note_call(e, "branch_sample_kernel", c.T, c.n, c.R);
  return 0;
}

struct BranchGradientCall {
  int T = 0, n = 0, R = 0, V = 0;
  const int32_t* index = nullptr;
  const double *q_params = nullptr, *bl = nullptr, *epsilon = nullptr, *log_q_branch = nullptr, *log_prior = nullptr;
  const double *branch_gradient = nullptr, *log_likelihoods = nullptr, *log_q_topology = nullptr, *weights = nullptr;
  double beta = 1.0, prior_rate = 0.0;
  double *out_gradient = nullptr, *out_log_f = nullptr;
};

int check_gradient_call(const mi_engine* e, const BranchGradientCall& c) {
  if (check_shape(e, c.T, c.n, c.R)) return 1;
  if (c.V < 1) return fail("branch model: variable_count must be positive");
  if (check_rate(c.prior_rate)) return 1;
  if (!std::isfinite(c.beta)) return fail("branch model: beta must be finite");
  if (!c.index || !c.q_params) return fail("branch model: null index or q_params");
  if (!c.bl || !c.epsilon || !c.log_q_branch || !c.log_prior) return fail("branch model: null sample arrays");
  if (!c.branch_gradient || !c.log_likelihoods) return fail("branch model: null branch_gradient or log_likelihoods");
  if (!c.out_gradient || !c.out_log_f) return fail("null output pointer");
  return 0;
}

int run_branch_gradient_device(mi_engine* e, hipStream_t s, const BranchGradientCall& c) {
  if (check_gradient_call(e, c)) return 1;
  HIP_TRY(hipSetDevice(e->spec.device));
  if (reserve_gradient(e, c.T, c.n, c.R)) return 1;
  const GradientLayout l = gradient_layout(c.T, c.n, c.R);
  char* ws = e->branch_ws.as<char>();
  BranchGradientArgs a{};
  a.n = c.n;
  a.T = c.T;
  a.R = c.R;
  a.V = c.V;
  a.index = c.index;
  a.q_params = c.q_params;
  a.bl = c.bl;
  a.epsilon = c.epsilon;
  a.log_q_branch = c.log_q_branch;
  a.log_prior = c.log_prior;
  a.branch_gradient = c.branch_gradient;
  a.log_likelihoods = c.log_likelihoods;
  a.log_q_topology = c.log_q_topology;
  a.weights = c.weights;
  a.beta = c.beta;
  a.prior_rate = c.prior_rate;
  a.vi = e->vi_state;
  a.status = e->status.as<int32_t>();
  a.terms = reinterpret_cast<double*>(ws + l.terms);
  a.keys = reinterpret_cast<uint32_t*>(ws + l.keys);
  a.keys2 = reinterpret_cast<uint32_t*>(ws + l.keys2);
  a.vals = reinterpret_cast<uint32_t*>(ws + l.vals);
  a.vals2 = reinterpret_cast<uint32_t*>(ws + l.vals2);
  a.sort_tmp = ws + l.sort_tmp;
  a.sort_tmp_bytes = l.sort_bytes;
  a.out_gradient = c.out_gradient;
  a.out_log_f = c.out_log_f;
  if (launch_branch_gradient(a, s)) return fail("branch model gradient: the sort could not be enqueued");
  HIP_TRY(hipGetLastError());
  note_call(e, "branch_runs_kernel", c.T, c.n, c.R);
  return 0;
}

}  // namespace

extern "C" {

int32_t mi_engine_psp_table_device(mi_engine* e, void* stream, int32_t S, int32_t C, const int32_t* pcsp_clades,
                                   int32_t* out_psp_of_pcsp, int32_t* out_counts) {
  if (!e) return fail("null engine");
  if (!e->shards.empty()) return fail(kShardedDeviceCall);
  PspTableCall c;
  c.S = S;
  c.C = C;
  c.pcsp_clades = pcsp_clades;
  c.out_psp_of_pcsp = out_psp_of_pcsp;
  c.out_counts = out_counts;
  return run_psp_table_device(e, pick_stream(e, stream), c);
}

int32_t mi_engine_psp_table(mi_engine* e, int32_t S, int32_t C, const int32_t* pcsp_clades, int32_t* out_psp_of_pcsp,
                            int32_t* out_counts) {
  PspTableCall c;
  c.S = S;
  c.C = C;
  c.pcsp_clades = pcsp_clades;
  c.out_psp_of_pcsp = out_psp_of_pcsp;
  c.out_counts = out_counts;
  if (check_table_call(e, c)) return 1;
  HostCall h;
  h.in = {fixed(pcsp_clades, (size_t)C * 3)};
  h.out = {fixed(out_psp_of_pcsp, (size_t)C), fixed(out_counts, 2)};
  h.enqueue = [=](mi_engine* e, int, const HostArray* in, const HostArray* out) {
    PspTableCall d = c;
    d.pcsp_clades = in[0].at<const int32_t>();
    d.out_psp_of_pcsp = out[0].at<int32_t>();
    d.out_counts = out[1].at<int32_t>();
    return run_psp_table_device(e, e->stream, d);
  };
  return run_on_engine(first_engine(e), h);
}

int32_t mi_engine_psp_index_device(mi_engine* e, void* stream, int32_t T, int32_t n, const int32_t* root_index,
                                   const int32_t* slot_index, int32_t S, int32_t C, const int32_t* psp_of_pcsp,
                                   int32_t V, int32_t rows, int32_t* out_index) {
  if (!e) return fail("null engine");
  if (!e->shards.empty()) return fail(kShardedDeviceCall);
  PspIndexCall c;
  c.T = T;
  c.n = n;
  c.S = S;
  c.C = C;
  c.V = V;
  c.R = rows;
  c.root_index = root_index;
  c.slot_index = slot_index;
  c.psp_of_pcsp = psp_of_pcsp;
  c.out_index = out_index;
  return run_psp_index_device(e, pick_stream(e, stream), c);
}

int32_t mi_engine_psp_index(mi_engine* e, int32_t T, int32_t n, const int32_t* root_index, const int32_t* slot_index,
                            int32_t S, int32_t C, const int32_t* psp_of_pcsp, int32_t V, int32_t rows,
                            int32_t* out_index) {
  PspIndexCall c;
  c.T = T;
  c.n = n;
  c.S = S;
  c.C = C;
  c.V = V;
  c.R = rows;
  c.root_index = root_index;
  c.slot_index = slot_index;
  c.psp_of_pcsp = psp_of_pcsp;
  c.out_index = out_index;
  if (check_index_call(e, c)) return 1;
  const size_t E = 2 * (size_t)n - 3;
  HostCall h;
  h.in = {fixed(root_index, (size_t)T * E), fixed(slot_index, (size_t)T * E * 6), fixed(psp_of_pcsp, (size_t)C)};
  h.out = {fixed(out_index, (size_t)T * rows * E)};
  h.enqueue = [=](mi_engine* e, int, const HostArray* in, const HostArray* out) {
    PspIndexCall d = c;
    d.root_index = in[0].at<const int32_t>();
    d.slot_index = in[1].at<const int32_t>();
    d.psp_of_pcsp = in[2].at<const int32_t>();
    d.out_index = out[0].at<int32_t>();
    return run_psp_index_device(e, e->stream, d);
  };
  return run_on_engine(first_engine(e), h);
}

int32_t mi_engine_branch_model_sample_device(mi_engine* e, void* stream, int32_t T, int32_t n, int32_t rows,
                                             const int32_t* index, int32_t V, const double* q_params, uint64_t seed,
                                             int64_t first_sample, double prior_rate, const double* epsilon_in,
                                             double* out_branch_lengths, double* out_epsilon, double* out_log_q,
                                             double* out_log_prior) {
  if (!e) return fail("null engine");
  if (!e->shards.empty()) return fail(kShardedDeviceCall);
  BranchSampleCall c;
  c.T = T;
  c.n = n;
  c.R = rows;
  c.V = V;
  c.index = index;
  c.q_params = q_params;
  c.seed = seed;
  c.first_sample = first_sample;
  c.prior_rate = prior_rate;
  c.epsilon_in = epsilon_in;
  c.out_bl = out_branch_lengths;
  c.out_epsilon = out_epsilon;
  c.out_log_q = out_log_q;
  c.out_log_prior = out_log_prior;
  return run_branch_sample_device(e, pick_stream(e, stream), c);
}

int32_t mi_engine_branch_model_sample(mi_engine* e, int32_t T, int32_t n, int32_t rows, const int32_t* index, int32_t V,
                                      const double* q_params, uint64_t seed, int64_t first_sample, double prior_rate,
                                      const double* epsilon_in, double* out_branch_lengths, double* out_epsilon,
                                      double* out_log_q, double* out_log_prior) {
  BranchSampleCall c;
  c.T = T;
  c.n = n;
  c.R = rows;
  c.V = V;
  c.index = index;
  c.q_params = q_params;
  c.seed = seed;
  c.first_sample = first_sample;
  c.prior_rate = prior_rate;
  c.epsilon_in = epsilon_in;
  c.out_bl = out_branch_lengths;
  c.out_epsilon = out_epsilon;
  c.out_log_q = out_log_q;
  c.out_log_prior = out_log_prior;
  if (check_sample_call(e, c)) return 1;
  const size_t E = 2 * (size_t)n - 3;
  HostCall h;
  h.in = {fixed(index, (size_t)T * rows * E), fixed(q_params, (size_t)V * 2), fixed(epsilon_in, (size_t)T * E)};
  h.out = {fixed(out_branch_lengths, (size_t)T * (E + 1)), fixed(out_epsilon, (size_t)T * E), fixed(out_log_q, (size_t)T),
           fixed(out_log_prior, (size_t)T)};
  h.enqueue = [=](mi_engine* e, int, const HostArray* in, const HostArray* out) {
    BranchSampleCall d = c;
    d.index = in[0].at<const int32_t>();
    d.q_params = in[1].at<const double>();
    d.epsilon_in = in[2].at<const double>();
    d.out_bl = out[0].at<double>();
    d.out_epsilon = out[1].at<double>();
    d.out_log_q = out[2].at<double>();
    d.out_log_prior = out[3].at<double>();
    return run_branch_sample_device(e, e->stream, d);
  };
  return run_on_engine(first_engine(e), h);
}

int32_t mi_engine_branch_model_gradient_device(mi_engine* e, void* stream, int32_t T, int32_t n, int32_t rows,
                                               const int32_t* index, int32_t V, const double* q_params,
                                               const double* branch_lengths, const double* epsilon,
                                               const double* log_q_branch, const double* log_prior,
                                               const double* branch_gradient, const double* log_likelihoods,
                                               const double* log_q_topology, const double* tree_weights, double beta,
                                               double prior_rate, double* out_gradient, double* out_log_f) {
  if (!e) return fail("null engine");
  if (!e->shards.empty()) return fail(kShardedDeviceCall);
  BranchGradientCall c;
  c.T = T;
  c.n = n;
  c.R = rows;
  c.V = V;
  c.index = index;
  c.q_params = q_params;
  c.bl = branch_lengths;
  c.epsilon = epsilon;
  c.log_q_branch = log_q_branch;
  c.log_prior = log_prior;
  c.branch_gradient = branch_gradient;
  c.log_likelihoods = log_likelihoods;
  c.log_q_topology = log_q_topology;
  c.weights = tree_weights;
  c.beta = beta;
  c.prior_rate = prior_rate;
  c.out_gradient = out_gradient;
  c.out_log_f = out_log_f;
  return run_branch_gradient_device(e, pick_stream(e, stream), c);
}

int32_t mi_engine_branch_model_gradient(mi_engine* e, int32_t T, int32_t n, int32_t rows, const int32_t* index,
                                        int32_t V, const double* q_params, const double* branch_lengths,
                                        const double* epsilon, const double* log_q_branch, const double* log_prior,
                                        const double* branch_gradient, const double* log_likelihoods,
                                        const double* log_q_topology, const double* tree_weights, double beta,
                                        double prior_rate, double* out_gradient, double* out_log_f) {
  BranchGradientCall c;
  c.T = T;
  c.n = n;
  c.R = rows;
  c.V = V;
  c.index = index;
  c.q_params = q_params;
  c.bl = branch_lengths;
  c.epsilon = epsilon;
  c.log_q_branch = log_q_branch;
  c.log_prior = log_prior;
  c.branch_gradient = branch_gradient;
  c.log_likelihoods = log_likelihoods;
  c.log_q_topology = log_q_topology;
  c.weights = tree_weights;
  c.beta = beta;
  c.prior_rate = prior_rate;
  c.out_gradient = out_gradient;
  c.out_log_f = out_log_f;
  if (check_gradient_call(e, c)) return 1;
  const size_t E = 2 * (size_t)n - 3, t = (size_t)T;
  HostCall h;
  h.in = {fixed(index, t * rows * E),   fixed(q_params, (size_t)V * 2), fixed(branch_lengths, t * (E + 1)),
          fixed(epsilon, t * E),        fixed(log_q_branch, t),         fixed(log_prior, t),
          fixed(branch_gradient, t * (E + 2)), fixed(log_likelihoods, t), fixed(log_q_topology, t),
          fixed(tree_weights, t)};
  h.out = {fixed(out_gradient, (size_t)V * 2), fixed(out_log_f, t)};
  h.enqueue = [=](mi_engine* e, int, const HostArray* in, const HostArray* out) {
    BranchGradientCall d = c;
    d.index = in[0].at<const int32_t>();
    d.q_params = in[1].at<const double>();
    d.bl = in[2].at<const double>();
    d.epsilon = in[3].at<const double>();
    d.log_q_branch = in[4].at<const double>();
    d.log_prior = in[5].at<const double>();
    d.branch_gradient = in[6].at<const double>();
    d.log_likelihoods = in[7].at<const double>();
    d.log_q_topology = in[8].at<const double>();
    d.weights = in[9].at<const double>();
    d.out_gradient = out[0].at<double>();
    d.out_log_f = out[1].at<double>();
    return run_branch_gradient_device(e, e->stream, d);
  };
  return run_on_engine(first_engine(e), h);
}

int32_t mi_engine_reserve_branch_model(mi_engine* e, int32_t T, int32_t n, int32_t rows) {
  if (check_shape(e, T, n, rows)) return 1;
  e = first_engine(e);
  HIP_TRY(hipSetDevice(e->spec.device));
  return reserve_gradient(e, T, n, rows);
}

}  // extern "C"
