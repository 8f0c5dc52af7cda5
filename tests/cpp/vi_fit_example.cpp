// A device-resident variational fit through the C++ Engine adapter
// (libsbn_amd/csrc/host/engine.hpp): the reference's five_taxon example, its trees the support, the
// simple-average SBN and made-up log-normal tables as the start, five annealed steps of eight
// particles through Engine::ViCreate and ViFit, then one update from made-up gradients through
// ViUpdate.  Prints the inputs and results (doubles as hexadecimal floats) for the test that makes
// the same calls from Python.  Exit code 0 = all checks passed.
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
  auto five = TreeCollection::ParseNewickFile(data + "/five_taxon_unrooted.nwk");
  SitePattern pattern(Alignment::ReadFasta(data + "/five_taxon.fasta"), five.taxon_names_);
  Engine engine(EngineSpecification{1, {}, true}, simple, pattern);

  const size_t T = five.TreeCount(), n = 5, K = 8, steps = 5;
  std::vector<int32_t> parents;
  for (const auto& tree : five.trees_) parents.insert(parents.end(), tree.parent_ids.begin(), tree.parent_ids.end());
  const SbnSupport support = engine.SbnIndex(T, n, parents);
  const SbnTraining sa = engine.SbnTrain(support, MI_SBN_SA);
  const PspNumbering table = engine.PspTable(support);
  const size_t S = table.rootsplit_count_, V = table.variable_count_, P = support.ParameterCount();
  std::vector<double> q(2 * V);
  for (size_t j = 0; j < V; j++) {
    q[2 * j] = j < S ? -2.0 - 0.05 * (double)j : 0.01 * (double)(j % 7);
    q[2 * j + 1] = j < S ? 0.5 : 0.02;
  }

  mi_vi_options options = Engine::ViDefaultOptions();
  options.particle_count = (int32_t)K;
  options.anneal_steps = 4;
  options.max_steps = 8;
  options.step_size[0] = 0.01;
  options.step_size[1] = 0.005;
  options.seed = 20261021;
  const std::vector<double> model_row((size_t)engine.ParameterCount(), 1.0);
  const VariationalFit fit = engine.ViCreate(T, parents, sa.log_params_, q, options, model_row);
  const auto sizes = fit.Sizes();
  CHECK(sizes[0] == (int32_t)n && sizes[1] == (int32_t)K && sizes[2] == 3 && sizes[6] == (int32_t)V && sizes[8] == (int32_t)P);

  const std::vector<double> trace = engine.ViFit(fit, steps, 2);
  CHECK(trace.size() == 6 * steps);
  for (size_t t = 0; t < steps; t++) {
    CHECK(trace[6 * t] == (t < 4 ? (double)(t + 1) / 4.0 : 1.0));           // beta
    CHECK(std::isfinite(trace[6 * t + 1]) && std::isfinite(trace[6 * t + 2]));
    CHECK(trace[6 * t + 1] <= trace[6 * t + 2]);                            // the mean is below the logsumexp bound
    CHECK(trace[6 * t + 5] == 1.0);
  }
  const ViStateResult state = engine.ViState(fit);
  CHECK(state.counters_[0] == (int64_t)steps && state.counters_[1] == (int64_t)steps && state.counters_[2] == 0);
  CHECK(state.scalars_[2] == trace[6 * (steps - 1) + 3] && state.scalars_[3] == trace[6 * (steps - 1) + 4]);
  CHECK(state.log_params_ != sa.log_params_ && state.q_params_ != q);
  bool refused = false;
  try {
    engine.ViFit(fit, 4);  // (five of eight rows are written)
  } catch (const std::runtime_error&) {
    refused = true;
  }
  CHECK(refused);

  std::vector<double> ll(K), lprior(K), lqt(K), lqb(K);
  for (size_t k = 0; k < K; k++) {
    ll[k] = -1.0 * (double)k;
    lprior[k] = 0.5 * (double)k;
    lqt[k] = 0.25 * (double)k;
    lqb[k] = 0.125 * (double)k;
  }
  const auto row = engine.ViUpdate(fit, std::vector<double>(P, 1.0), std::vector<double>(2 * V, 1.0), ll, lprior, lqt, lqb);
  CHECK(row[0] == 1.0 && row[5] == 1.0 && engine.ViState(fit).counters_[0] == (int64_t)steps + 1);

  print("support", parents, " %d");
  print("log_params", sa.log_params_, " %a");
  print("q_params", q, " %a");
  print("trace", trace, " %a");
  print("fitted_log_params", state.log_params_, " %a");
  print("fitted_q_params", state.q_params_, " %a");
  print("update_row", row, " %a");
  std::printf(failures ? "FAILED (%d)\n" : "status all checks passed\n", failures);
  return failures ? 1 : 0;
}
