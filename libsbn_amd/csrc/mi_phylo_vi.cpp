// A device-resident variational fit: the fit object and its device state
// (mi_engine_vi_create, mi_vi_destroy, mi_vi_get_state, mi_vi_set_state), one step as one chain of
// launches (mi_vi_step_device), the fit (mi_vi_fit), the optimiser as a call of its own
// (mi_vi_update*) and the last step's particles (mi_vi_particles).  A step is made of the existing
// device forms; the sampler, the branch-length draw and its gradient read first_sample and beta
// from the fit's state (mi_engine::vi_state) instead of their by-value arguments.
#include <cmath>
#include <vector>

#include "mi_phylo_engine.h"
#include "mi_phylo_vi_host.h"

int vi_check_options(const mi_vi_options& o) {
  if (o.particle_count < 1) return fail("variational fit: particle_count must be positive");
  if (o.rows != 1 && o.rows != 3) return fail("variational fit: rows must be 1 (splits) or 3 (rootsplit, down PSP, up PSP)");
  if (o.estimator != MI_SBN_FACTORS_PLAIN && o.estimator != MI_SBN_FACTORS_VIMCO)
    return fail("variational fit: estimator must be MI_SBN_FACTORS_PLAIN or MI_SBN_FACTORS_VIMCO");
  if (o.estimator == MI_SBN_FACTORS_VIMCO && o.particle_count < 2)
    return fail("variational fit: the VIMCO estimator needs at least 2 particles");
  if (o.anneal_steps < 0) return fail("variational fit: anneal_steps must not be negative");
  if (o.max_steps < 1) return fail("variational fit: max_steps must be positive");
  if (!(o.prior_rate > 0.0) || std::isinf(o.prior_rate)) return fail("variational fit: prior_rate must be finite and positive");
  for (double s : o.step_size)
    if (!(s > 0.0) || std::isinf(s)) return fail("variational fit: step_size must be finite and positive");
  if (!(o.sbn_step_size >= 0.0) || std::isinf(o.sbn_step_size))
    return fail("variational fit: sbn_step_size must be finite and not negative");
  if (!(o.step_decay > 0.0 && o.step_decay <= 1.0)) return fail("variational fit: step_decay must be in (0, 1]");
  if (!(o.adam_beta0 >= 0.0 && o.adam_beta0 < 1.0) || !(o.adam_beta1 >= 0.0 && o.adam_beta1 < 1.0))
    return fail("variational fit: adam_beta0 and adam_beta1 must be in [0, 1)");
  if (!(o.adam_epsilon >= 0.0) || std::isinf(o.adam_epsilon))
    return fail("variational fit: adam_epsilon must be finite and not negative");
  return 0;
}

namespace {


size_t cut(mi_vi* v, char* base) {
  const size_t K = v->K, E = v->E, T = (size_t)v->T0 + K, P = v->P, V = v->V, W = ((size_t)v->n + 31) / 32;
  Cutter c{base};
  c.take(v->state, 1);
  c.take(v->phi, P);
  c.take(v->q, 2 * V);
  c.take(v->m_sbn, P);
  c.take(v->v_sbn, P);
  c.take(v->m_q, 2 * V);
  c.take(v->v_q, 2 * V);
  c.take(v->d_range, 2 * (size_t)v->parents);
  c.take(v->d_desc, 2 * P);
  c.take(v->d_psp, (size_t)v->C);
  c.take(v->params, K * (size_t)v->pc);
  c.take(v->all_pid, T * E);
  c.take(v->root, T * E);
  c.take(v->slot, T * 2 * E * 3);
  c.take(v->counts, 3);
  c.take(v->bits, (size_t)v->S * W);
  c.take(v->clades, 3 * (size_t)v->C);
  c.take(v->prange, 2 * (size_t)v->C);
  c.take(v->pparent, (size_t)v->C);
  c.take(v->edge, K);
  c.take(v->sparams, K * ((size_t)v->n - 1));
  c.take(v->index, K * (size_t)v->R * E);
  c.take(v->lp, K);
  c.take(v->bl, K * (E + 1));
  c.take(v->eps, K * E);
  c.take(v->lqb, K);
  c.take(v->lprior, K);
  c.take(v->ll, K);
  c.take(v->g, K * (E + 2));
  c.take(v->rooting, K * E);
  c.take(v->lqt, K);
  c.take(v->qgrad, 2 * V);
  c.take(v->f, K);
  c.take(v->grad, P);
  c.take(v->factors, K);
  c.take(v->glq, K);
  c.take(v->block_flags, (size_t)v->blocks);
  c.take(v->trace, 6 * (size_t)v->o.max_steps);
  return c.at;
}

// the support of a fit, once, through the host forms: index, descent table, PSP table
struct SupportTables {
  int S = 0, C = 0, parents = 0, V = 0;
  std::vector<int32_t> prange, descent, psp;
};
int support_tables(mi_engine* e, int T0, const int32_t* parent_ids, SupportTables& t) {
  const int n = e->n;
  const size_t rcap = (size_t)T0 * (2 * (size_t)n - 3), pcap = rcap * 6, W = ((size_t)n + 31) / 32;
  std::vector<int32_t> root(rcap), slot(rcap * 6), clades(pcap * 3), pparent(pcap);
  std::vector<uint32_t> bits(rcap * W);
  t.prange.resize(pcap * 2);
  int32_t counts[3] = {}, table_counts[2] = {};
  if (mi_engine_sbn_index(e, T0, n, parent_ids, T0, (int32_t)rcap, (int32_t)pcap, root.data(), slot.data(), counts,
                          bits.data(), clades.data(), t.prange.data(), pparent.data()))
    return 1;
  t.S = counts[0], t.C = counts[1], t.parents = counts[2];
  t.descent.resize(2 * ((size_t)t.S + t.C));
  t.psp.resize((size_t)t.C);
  if (mi_engine_sbn_descent(e, T0, n, parent_ids, root.data(), slot.data(), t.S, t.C, pparent.data(), t.descent.data()))
    return 1;
  if (mi_engine_psp_table(e, t.S, t.C, clades.data(), t.psp.data(), table_counts)) return 1;
  t.V = table_counts[1];
  return 0;
}

std::string fit_path(const mi_vi* v, int steps) {
  if (v->gp) return gp_vi_path(v, steps);
  return "vi_fit n=" + std::to_string(v->n) + " K=" + std::to_string(v->K) + " rows=" + std::to_string(v->R) +
         " steps=" + std::to_string(steps) + " | " + v->grad_path;
}

}  // namespace

int vi_enqueue_update(mi_vi* v, hipStream_t s, const double* g_sbn, const double* g_q, const double* ll, const double* lprior,
                      const double* lqt, const double* lqb, double* out_row) {
  if (!g_sbn || !g_q || !ll || !lprior || !lqt || !lqb) return fail("variational fit: null gradient or term array");
  ViUpdateArgs a{};
  a.P = v->P;
  a.V = v->V;
  a.K = v->K;
  a.S = v->T0 > 0 ? v->S : v->V;  // (a fit of the tables alone: every variable)
  a.beta0 = v->o.adam_beta0;
  a.beta1 = v->o.adam_beta1;
  a.epsilon = v->o.adam_epsilon;
  a.decay = v->o.step_decay;
  a.state = v->state;
  a.g_sbn = g_sbn;
  a.g_q = g_q;
  a.log_lik = ll;
  a.log_prior = lprior;
  a.log_q_top = lqt;
  a.log_q_branch = lqb;
  a.phi = v->phi;
  a.q_params = v->q;
  a.m_sbn = v->m_sbn;
  a.v_sbn = v->v_sbn;
  a.m_q = v->m_q;
  a.v_q = v->v_q;
  a.block_flags = v->block_flags;
  a.trace = v->trace;
  a.max_steps = v->o.max_steps;
  a.out_row = out_row;
  launch_vi_update(a, s);
  HIP_TRY(hipGetLastError());
  return 0;
}

namespace {

int enqueue_step(mi_vi* v, hipStream_t s) {
  mi_engine* e = v->e;
  const int n = v->n, K = v->K, T0 = v->T0, S = v->S, C = v->C, E = v->E;
  int32_t* samples = v->all_pid + (size_t)T0 * E;
  const int32_t* s_root = v->root + (size_t)T0 * E;
  const int32_t* s_slot = v->slot + (size_t)T0 * 2 * E * 3;
  // (the two arguments the state replaces are passed as 0 and 1; the kernels do not read them)
  if (mi_engine_sbn_sample_device(e, s, K, n, S, C, v->parents, v->d_range, v->d_desc, v->phi, v->o.seed, 0, samples,
                                  v->edge, v->sparams, v->lp, nullptr))
    return 1;
  if (mi_engine_sbn_index_device(e, s, T0 + K, n, v->all_pid, T0, S, C, v->root, v->slot, v->counts, v->bits, v->clades,
                                 v->prange, v->pparent))
    return 1;
  if (mi_engine_psp_index_device(e, s, K, n, s_root, s_slot, S, C, v->d_psp, v->V, v->R, v->index)) return 1;
  if (mi_engine_branch_model_sample_device(e, s, K, n, v->R, v->index, v->V, v->q, v->o.seed, 0, v->o.prior_rate,
                                           nullptr, v->bl, v->eps, v->lqb, v->lprior))
    return 1;
  if (mi_engine_gradients_unrooted_device(e, s, K, samples, v->bl, v->params, 0, v->ll, v->g, nullptr, nullptr)) return 1;
  v->grad_path = e->last_path;
  if (mi_engine_sbn_log_prob_device(e, s, K, n, samples, s_root, s_slot, S, C, v->parents, v->d_range, v->phi, 0, nullptr,
                                    v->rooting, v->lqt, nullptr))
    return 1;
  if (mi_engine_branch_model_gradient_device(e, s, K, n, v->R, v->index, v->V, v->q, v->bl, v->eps, v->lqb, v->lprior,
                                             v->g, v->ll, v->lqt, nullptr, 1.0, v->o.prior_rate, v->qgrad, v->f))
    return 1;
  if (mi_engine_sbn_topology_gradient_device(e, s, K, n, samples, s_root, s_slot, S, C, v->parents, v->d_range, v->phi, 0,
                                             v->f, v->o.estimator, v->grad, v->factors, v->glq))
    return 1;
  return vi_enqueue_update(v, s, v->grad, v->qgrad, v->ll, v->lprior, v->lqt, v->lqb, nullptr);
}

int step(mi_vi* v, hipStream_t s) {
  mi_engine* e = v->e;
  if (v->T0 < 1 && !v->gp)
    return fail("variational fit: a fit without a support holds the tables only; it takes updates, no steps");
  HIP_TRY(hipSetDevice(e->spec.device));
  e->vi_state = v->state;
  const int rc = v->gp ? gp_vi_enqueue_step(v, s) : enqueue_step(v, s);
  e->vi_state = nullptr;
  if (rc) return 1;
  e->dominant = "vi_finish_kernel";
  e->last_path = fit_path(v, 1);
  return 0;
}

int read_state(mi_vi* v, ViState& st) {
  HIP_TRY(hipSetDevice(v->e->spec.device));
  HIP_TRY(hipStreamSynchronize(v->e->stream));
  return download(&st, v->state, sizeof st);
}

}  // namespace

extern "C" {

int32_t mi_vi_default_options(mi_vi_options* o) {
  if (!o) return fail("null output pointer");
  *o = mi_vi_options{};
  o->particle_count = 10;
  o->rows = 3;
  o->estimator = MI_SBN_FACTORS_VIMCO;
  o->max_steps = 1000;
  o->prior_rate = 10.0;
  o->step_size[0] = o->step_size[1] = 0.001;
  o->sbn_step_size = 0.001;
  o->step_decay = 0.99;
  o->adam_beta0 = 0.9;
  o->adam_beta1 = 0.999;
  o->adam_epsilon = 1e-8;
  return 0;
}

int32_t mi_engine_vi_create(mi_engine* e, int32_t T0, const int32_t* parent_ids, const double* model_params, int32_t P,
                            const double* log_params, int32_t V, const double* q_params, const mi_vi_options* options,
                            mi_vi** out) {
  if (!e) return fail("null engine");
  if (!out) return fail("null output pointer");
  *out = nullptr;
  if (e->shards.size() == 1) e = e->shards[0];  // (a handle of one shard is its one engine)
  if (!e->shards.empty()) return fail(kShardedDeviceCall);
  if (!options) return fail("variational fit: null options");
  if (vi_check_options(*options)) return 1;
  if (T0 < 0) return fail("variational fit: support_tree_count must not be negative");
  if (P < 0 || V < 0 || (size_t)P + 2 * (size_t)V < 1 || (size_t)P + 2 * (size_t)V >= ((size_t)1 << 31))
    return fail("variational fit: bad parameter or variable count");
  if ((P > 0 && !log_params) || (V > 0 && !q_params)) return fail("variational fit: null initial tables");
  if (T0 > 0 && !parent_ids) return fail("variational fit: null support trees");
  if (T0 > 0 && e->param_count > 0 && !model_params) return fail("variational fit: this engine's model takes parameters");
  const int n = e->n, E = 2 * n - 3, K = options->particle_count, R = options->rows;
  SupportTables t;
  if (T0 > 0) {
    if (support_tables(e, T0, parent_ids, t)) return 1;
    const int want_V = R == 1 ? t.S : t.V;
    if (P != t.S + t.C || V != want_V)
      return fail("variational fit: the support has " + std::to_string(t.S + t.C) + " SBN parameters and " +
                  std::to_string(want_V) + " branch-length variables, the tables given " + std::to_string(P) + " and " +
                  std::to_string(V));
    if (mi_engine_reserve_sbn(e, T0 + K, n) || mi_engine_reserve(e, K, 1) || mi_engine_reserve_branch_model(e, K, n, R))
      return 1;
  }
  const int S = t.S, C = t.C, parents = t.parents;
  const std::vector<int32_t>&prange = t.prange, &descent = t.descent, &psp = t.psp;
  HIP_TRY(hipSetDevice(e->spec.device));
  if (e->status.ensure(sizeof(int32_t) * kStatusWords)) return 1;
  mi_vi* v = new mi_vi;
  v->e = e;
  v->o = *options;
  v->n = n;
  v->E = E;
  v->T0 = T0;
  v->K = K;
  v->R = R;
  v->S = S;
  v->C = C;
  v->parents = parents;
  v->P = P;
  v->V = V;
  v->pc = e->param_count;
  v->blocks = vi_update_blocks(P, V);
  const size_t bytes = cut(v, nullptr);
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
    cut(v, v->pool.as<char>());
    if (upload(v->state, &st, sizeof st) || upload(v->phi, log_params, sizeof(double) * P) ||
        upload(v->q, q_params, sizeof(double) * 2 * V) || upload(v->d_range, prange.data(), sizeof(int32_t) * 2 * parents) ||
        upload(v->d_desc, descent.data(), sizeof(int32_t) * descent.size()) || upload(v->d_psp, psp.data(), sizeof(int32_t) * C) ||
        upload(v->params, rows.data(), sizeof(double) * rows.size()) ||
        upload(v->all_pid, parent_ids, sizeof(int32_t) * (size_t)T0 * E))
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

void mi_vi_destroy(mi_vi* v) {
  if (!v) return;
  (void)hipSetDevice(v->e->spec.device);
  (void)hipStreamSynchronize(v->e->stream);
  delete v;
}

int32_t mi_vi_sizes(const mi_vi* v, int32_t* out) {
  if (!v || !out) return fail("null fit or output pointer");
  const int32_t sizes[9] = {v->n, v->K, v->R, v->S, v->C, v->parents, v->V, v->o.max_steps, v->P};
  std::copy(sizes, sizes + 9, out);
  return 0;
}

int32_t mi_vi_step_device(mi_vi* v, void* stream) {
  if (!v) return fail("null fit");
  return step(v, pick_stream(v->e, stream));
}

int32_t mi_vi_fit(mi_vi* v, int32_t steps, int32_t check_interval, double* out_trace) {
  if (!v) return fail("null fit");
  if (steps < 1) return fail("variational fit: steps must be positive");
  if (!out_trace) return fail("null output pointer");
  mi_engine* e = v->e;
  ViState st;
  if (read_state(v, st)) return 1;
  if (st.t < 0 || st.t + steps > v->o.max_steps)
    return fail("variational fit: " + std::to_string(steps) + " steps after " + std::to_string(st.t) +
                " are beyond the trace capacity of " + std::to_string(v->o.max_steps) + " (max_steps)");
  for (int i = 0; i < steps; i++) {
    if (step(v, e->stream)) return 1;
    if (check_interval > 0 && (i + 1) % check_interval == 0 && i + 1 < steps && mi_engine_check_status(e, nullptr)) return 1;
  }
  if (mi_engine_check_status(e, nullptr)) return 1;
  e->last_path = fit_path(v, steps);
  return download(out_trace, v->trace + 6 * (size_t)st.t, sizeof(double) * 6 * (size_t)steps);
}

int32_t mi_vi_trace(mi_vi* v, int32_t first, int32_t count, double* out_trace) {
  if (!v) return fail("null fit");
  if (!out_trace) return fail("null output pointer");
  ViState st;
  if (read_state(v, st)) return 1;
  if (first < 0 || count < 0 || (int64_t)first + count > std::min<int64_t>(st.t, v->o.max_steps))
    return fail("variational fit: trace rows [" + std::to_string(first) + ", " + std::to_string((int64_t)first + count) +
                ") are not all written: " + std::to_string(st.t) + " steps so far, capacity " +
                std::to_string(v->o.max_steps));
  return download(out_trace, v->trace + 6 * (size_t)first, sizeof(double) * 6 * (size_t)count);
}

int32_t mi_vi_update_device(mi_vi* v, void* stream, const double* g_sbn, const double* g_q, const double* ll,
                            const double* lprior, const double* lqt, const double* lqb, double* out_row) {
  if (!v) return fail("null fit");
  HIP_TRY(hipSetDevice(v->e->spec.device));
  return vi_enqueue_update(v, pick_stream(v->e, stream), g_sbn, g_q, ll, lprior, lqt, lqb, out_row);
}

int32_t mi_vi_update(mi_vi* v, const double* g_sbn, const double* g_q, const double* ll, const double* lprior,
                     const double* lqt, const double* lqb, double* out_row) {
  if (!v) return fail("null fit");
  if (!g_sbn || !g_q || !ll || !lprior || !lqt || !lqb) return fail("variational fit: null gradient or term array");
  const size_t K = v->K;
  HostCall c;
  c.in = {fixed(g_sbn, (size_t)v->P), fixed(g_q, 2 * (size_t)v->V), fixed(ll, K), fixed(lprior, K), fixed(lqt, K), fixed(lqb, K)};
  c.out = {fixed(out_row, 6)};
  c.enqueue = [=](mi_engine* e, int, const HostArray* in, const HostArray* out) {
    return vi_enqueue_update(v, e->stream, in[0].at<const double>(), in[1].at<const double>(), in[2].at<const double>(),
                             in[3].at<const double>(), in[4].at<const double>(), in[5].at<const double>(), out[0].at<double>());
  };
  return run_on_engine(v->e, c);
}

int32_t mi_vi_get_state(mi_vi* v, double* phi, double* q, double* sbn_moments, double* q_moments, double* scalars,
                        int64_t* counters) {
  if (!v) return fail("null fit");
  ViState st;
  if (read_state(v, st)) return 1;
  const size_t P = v->P, Q = 2 * (size_t)v->V, d = sizeof(double);
  if (download(phi, v->phi, d * P) || download(q, v->q, d * Q) || download(sbn_moments, v->m_sbn, d * P) ||
      download(sbn_moments ? sbn_moments + P : nullptr, v->v_sbn, d * P) || download(q_moments, v->m_q, d * Q) ||
      download(q_moments ? q_moments + Q : nullptr, v->v_q, d * Q))
    return 1;
  if (scalars) {
    const double s[5] = {st.b0, st.b1, st.step[0], st.step[1], st.sbn_step};
    std::copy(s, s + 5, scalars);
  }
  if (counters) {
    counters[0] = st.t;
    counters[1] = st.a;
    counters[2] = st.first_sample;
  }
  return 0;
}

int32_t mi_vi_set_state(mi_vi* v, const double* phi, const double* q, const double* sbn_moments, const double* q_moments,
                        const double* scalars, const int64_t* counters) {
  if (!v) return fail("null fit");
  if (!phi || !q || !sbn_moments || !q_moments || !scalars || !counters) return fail("variational fit: null state array");
  if (counters[0] < 0 || counters[1] < 0 || counters[1] > counters[0])
    return fail("variational fit: the state's counters must satisfy 0 <= a <= t");
  ViState st;
  if (read_state(v, st)) return 1;
  st.t = counters[0];
  st.a = counters[1];
  st.first_sample = counters[2];
  st.b0 = scalars[0];
  st.b1 = scalars[1];
  st.step[0] = scalars[2];
  st.step[1] = scalars[3];
  st.sbn_step = scalars[4];
  const size_t P = v->P, Q = 2 * (size_t)v->V, d = sizeof(double);
  if (upload(v->state, &st, sizeof st) || upload(v->phi, phi, d * P) || upload(v->q, q, d * Q) ||
      upload(v->m_sbn, sbn_moments, d * P) || upload(v->v_sbn, sbn_moments + P, d * P) ||
      upload(v->m_q, q_moments, d * Q) || upload(v->v_q, q_moments + Q, d * Q))
    return 1;
  return 0;
}

int32_t mi_vi_particles(mi_vi* v, int32_t* pid, double* bl, double* ll, double* lqt, double* lqb, double* lprior) {
  if (!v) return fail("null fit");
  if (v->gp)
    return fail("variational fit: a fit over a subsplit DAG has rooted particles; mi_gp_vi_particles gives them");
  if (!pid) return fail("null output pointer");
  HIP_TRY(hipSetDevice(v->e->spec.device));
  HIP_TRY(hipStreamSynchronize(v->e->stream));
  const size_t K = v->K, E = v->E, d = sizeof(double);
  if (download(pid, v->all_pid + (size_t)v->T0 * E, sizeof(int32_t) * K * E) || download(bl, v->bl, d * K * (E + 1)) ||
      download(ll, v->ll, d * K) || download(lqt, v->lqt, d * K) || download(lqb, v->lqb, d * K) ||
      download(lprior, v->lprior, d * K))
    return 1;
  return 0;
}

}  // extern "C"
