// Sampling from a subsplit Bayesian network and the topology gradient through the C++ Engine
// adapter (libsbn_amd/csrc/host/engine.hpp): the support of the reference's five_taxon example,
// simple-average parameters, 64 trees drawn, indexed behind the support trees, and the VIMCO
// gradient for made-up log_f.  Prints the inputs and results (doubles as hexadecimal floats) for
// the test that makes the same calls from Python.  Exit code 0 = all checks passed.
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
  auto hello = TreeCollection::ParseNewickFile(data + "/hello.nwk");
  SitePattern pattern(Alignment::ReadFasta(data + "/hello.fasta"), hello.taxon_names_);
  Engine engine(EngineSpecification{1, {}, true}, simple, pattern);

  auto five = TreeCollection::ParseNewickFile(data + "/five_taxon_unrooted.nwk");
  const size_t T = five.TreeCount(), n = 5, E = 2 * n - 3, K = 64;
  std::vector<int32_t> parents;
  for (const auto& tree : five.trees_) parents.insert(parents.end(), tree.parent_ids.begin(), tree.parent_ids.end());
  const SbnSupport support = engine.SbnIndex(T, n, parents);
  const size_t P = support.ParameterCount();
  const std::vector<int32_t> descent = engine.SbnDescent(support);
  CHECK(descent.size() == 2 * P);
  for (const int32_t e : descent) CHECK(e >= -(int32_t)n && e < (int32_t)support.parent_count_);

  const SbnTraining sa = engine.SbnTrain(support, MI_SBN_SA);
  const SbnSamples drawn = engine.SbnSample(support, descent, sa.log_params_, K, 20261020);
  for (size_t k = 0; k < K; k++) {
    CHECK(drawn.root_edge_[k] >= 0 && drawn.root_edge_[k] < (int32_t)E);
    CHECK(std::isfinite(drawn.log_prob_[k]) && drawn.log_prob_[k] <= 0.0);
    for (size_t v = 0; v < E; v++) CHECK(drawn.parent_ids_[k * E + v] > (int32_t)v && drawn.parent_ids_[k * E + v] <= (int32_t)E);
  }
  // a sample depends on (seed, first_sample + k) alone
  const SbnSamples tail = engine.SbnSample(support, descent, sa.log_params_, 4, 20261020, 60);
  for (size_t i = 0; i < 4 * E; i++) CHECK(tail.parent_ids_[i] == drawn.parent_ids_[60 * E + i]);

  // the samples behind the support trees: every one lies inside the support
  std::vector<int32_t> all = parents;
  all.insert(all.end(), drawn.parent_ids_.begin(), drawn.parent_ids_.end());
  const SbnSupport both = engine.SbnIndex(T + K, n, all, T);
  CHECK(both.ParameterCount() == P);
  for (size_t i = T * E; i < (T + K) * E; i++) CHECK(both.root_index_[i] < (int32_t)support.rootsplit_count_);
  std::vector<double> log_f(K);
  for (size_t k = 0; k < K; k++) log_f[k] = -70.0 - 0.25 * (double)k;
  const SbnGradient g = engine.SbnTopologyGradient(both, sa.log_params_, log_f, MI_SBN_FACTORS_VIMCO, T);
  // the gradient with respect to unnormalised parameters adds up to zero within every block
  double block = 0.0;
  for (size_t j = 0; j < support.rootsplit_count_; j++) block += g.gradient_[j];
  CHECK(std::fabs(block) < 1e-9);
  for (size_t k = 0; k < K; k++) CHECK(std::isfinite(g.log_q_[k]) && g.log_q_[k] >= drawn.log_prob_[k] - 1e-12);

  print("support", parents, " %d");
  print("log_params", sa.log_params_, " %a");
  print("first_tree", std::vector<int32_t>(drawn.parent_ids_.begin(), drawn.parent_ids_.begin() + E), " %d");
  print("root_edges", drawn.root_edge_, " %d");
  print("log_prob", drawn.log_prob_, " %a");
  print("gradient", g.gradient_, " %a");
  std::printf(failures ? "FAILED (%d)\n" : "status all checks passed\n", failures);
  return failures ? 1 : 0;
}
