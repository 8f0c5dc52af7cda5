// A variational fit over the rooted trees of a subsplit DAG through the C++ Engine adapter
// (libsbn_amd/csrc/host/engine.hpp): the reference's five_taxon example, its rooted trees the DAG, the
// object's own q and made-up log-normal tables as the start, five annealed steps of eight particles
// through GeneralizedPruning::ViCreate and Engine::ViFit, then the last step's rooted particles.
// Prints the inputs and results (doubles as hexadecimal floats) for the test that makes the same
// calls from Python.  Exit code 0 = all checks passed.
#include <cmath>
#include <cstdio>
#include <string>

#include "../../libsbn_amd/csrc/host/engine.hpp"

using namespace mihost;

static int failures = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::printf("CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      failures++;                                                        \
    }                                                                    \
  } while (0)

template <typename V>
static void print(const char* name, const V& values, const char* format) {
  std::printf("%s", name);
  for (const auto x : values) std::printf(format, x);
  std::printf("\n");
}

int main(int argc, char** argv) {
  const std::string data = argc > 1 ? argv[1] : "tests/golden/data";
  const PhyloModelSpecification simple{"JC69", "constant", "strict"};
  auto five = TreeCollection::ParseNewickFile(data + "/five_taxon_rooted.nwk");
  SitePattern pattern(Alignment::ReadFasta(data + "/five_taxon.fasta"), five.taxon_names_);
  Engine engine(EngineSpecification{1, {}, true}, simple, pattern);

  std::vector<int32_t> parents;
  for (const auto& tree : five.trees_) parents.insert(parents.end(), tree.parent_ids.begin(), tree.parent_ids.end());
  const std::vector<double> model_row((size_t)engine.ParameterCount(), 1.0);
  const GeneralizedPruning gp = engine.GpCreate(five.TreeCount(), parents, {}, model_row);
  const auto gp_sizes = gp.Sizes();
  const size_t n = 5, K = 8, steps = 5, R = (size_t)gp_sizes[2], G = (size_t)gp_sizes[3];

  std::vector<double> log_params = gp.SbnParameters(), q(2 * G);
  for (double& x : log_params) x = std::log(x);
  for (size_t j = 0; j < G; j++) {
    q[2 * j] = j < R ? 0.0 : -2.0 - 0.05 * (double)(j % 9);
    q[2 * j + 1] = j < R ? 1.0 : 0.3;
  }
  mi_vi_options options = Engine::ViDefaultOptions();
  options.particle_count = (int32_t)K;
  options.rows = 1;
  options.anneal_steps = 4;
  options.max_steps = 8;
  options.step_size[0] = 0.01;
  options.step_size[1] = 0.005;
  options.seed = 20261021;
  const VariationalFit fit = gp.ViCreate(log_params, q, options, model_row);
  const auto sizes = fit.Sizes();
  CHECK(sizes[0] == (int32_t)n && sizes[1] == (int32_t)K && sizes[2] == 1 && sizes[3] == (int32_t)R);
  CHECK(sizes[6] == (int32_t)G && sizes[8] == (int32_t)G);

  const std::vector<double> trace = engine.ViFit(fit, steps, 2);
  CHECK(trace.size() == 6 * steps);
  for (size_t t = 0; t < steps; t++) {
    CHECK(trace[6 * t] == (t < 4 ? (double)(t + 1) / 4.0 : 1.0));  // beta
    CHECK(std::isfinite(trace[6 * t + 1]) && trace[6 * t + 1] <= trace[6 * t + 2]);
    CHECK(trace[6 * t + 5] == 1.0);
  }
  const ViStateResult state = engine.ViState(fit);
  CHECK(state.counters_[0] == (int64_t)steps && state.counters_[1] == (int64_t)steps);
  CHECK(state.log_params_ != log_params && state.q_params_ != q);
  for (size_t j = 0; j < 2 * R; j++) CHECK(state.q_params_[j] == q[j]);  // (rootsplit rows are carried)
  const GpViParticles particles = gp.ViParticles(fit);
  CHECK(gp.TreeIndex(K, particles.parent_ids_).entries_ == particles.entries_);
  for (size_t k = 0; k < K; k++) CHECK(particles.branch_lengths_[k * (2 * n - 1) + 2 * n - 2] == 0.0);

  mi_vi_options bad = options;
  bad.rows = 3;
  bool refused = false;
  try {
    gp.ViCreate(log_params, q, bad, model_row);
  } catch (const std::runtime_error&) {
    refused = true;
  }
  CHECK(refused);

  print("log_params", log_params, " %a");
  print("q_params", q, " %a");
  print("trace", trace, " %a");
  print("fitted_log_params", state.log_params_, " %a");
  print("fitted_q_params", state.q_params_, " %a");
  print("particle_parent_ids", particles.parent_ids_, " %d");
  print("particle_lengths", particles.branch_lengths_, " %a");
  print("particle_log_likelihoods", particles.log_likelihoods_, " %a");
  std::printf(failures ? "FAILED (%d)\n" : "status all checks passed\n", failures);
  return failures ? 1 : 0;
}
