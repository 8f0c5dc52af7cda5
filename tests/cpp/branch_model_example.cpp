// PSP indexing and the log-normal branch-length models through the C++ Engine adapter
// (libsbn_amd/csrc/host/engine.hpp): the support of the reference's five_taxon example, 64 trees
// drawn from its simple-average SBN and indexed behind the support trees, their PSP rows, one draw
// of branch lengths, and the gradient with log_f for made-up branch gradients and log-likelihoods.
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
  auto hello = TreeCollection::ParseNewickFile(data + "/hello.nwk");
  SitePattern pattern(Alignment::ReadFasta(data + "/hello.fasta"), hello.taxon_names_);
  Engine engine(EngineSpecification{1, {}, true}, simple, pattern);

  auto five = TreeCollection::ParseNewickFile(data + "/five_taxon_unrooted.nwk");
  const size_t T = five.TreeCount(), n = 5, E = 2 * n - 3, K = 64;
  std::vector<int32_t> parents;
  for (const auto& tree : five.trees_) parents.insert(parents.end(), tree.parent_ids.begin(), tree.parent_ids.end());
  const SbnSupport support = engine.SbnIndex(T, n, parents);
  const SbnTraining sa = engine.SbnTrain(support, MI_SBN_SA);
  const SbnSamples drawn = engine.SbnSample(support, engine.SbnDescent(support), sa.log_params_, K, 20261021);
  std::vector<int32_t> all = parents;
  all.insert(all.end(), drawn.parent_ids_.begin(), drawn.parent_ids_.end());
  const SbnSupport both = engine.SbnIndex(T + K, n, all, T);

  const PspNumbering table = engine.PspTable(both);
  const size_t S = table.rootsplit_count_, V = table.variable_count_;
  CHECK(S == support.rootsplit_count_ && V > S && V <= support.ParameterCount());
  const std::vector<int32_t> index = engine.PspIndex(both, table, 3, T);
  CHECK(index.size() == K * 3 * E);
  for (size_t k = 0; k < K; k++)
    for (size_t v = 0; v < E; v++) {
      const int32_t split = index[(k * 3 + 0) * E + v], down = index[(k * 3 + 1) * E + v], up = index[(k * 3 + 2) * E + v];
      CHECK(split >= 0 && split < (int32_t)S);                          // every sample lies inside the support
      CHECK(v < n ? down == (int32_t)V : (down >= (int32_t)S && down < (int32_t)V));  // no PSP below a pendant edge
      CHECK(up >= (int32_t)S && up < (int32_t)V);
    }
  const std::vector<int32_t> splits = engine.PspIndex(both, table, 1, T);
  for (size_t k = 0; k < K; k++)
    for (size_t v = 0; v < E; v++) CHECK(splits[k * E + v] == index[k * 3 * E + v]);

  // the split rows carry the log-normal parameters, the PSP rows small corrections
  std::vector<double> q(2 * V);
  for (size_t j = 0; j < V; j++) {
    q[2 * j] = j < S ? -2.0 - 0.05 * (double)j : 0.01 * (double)(j % 7);
    q[2 * j + 1] = j < S ? 0.5 : 0.02;
  }
  const BranchModelDraw draw = engine.BranchModelSample(K, n, 3, index, q, 20261021, 5);
  for (size_t k = 0; k < K; k++) {
    CHECK(draw.branch_lengths_[k * (E + 1) + E] == 0.0 && std::isfinite(draw.log_q_[k]) && std::isfinite(draw.log_prior_[k]));
    for (size_t v = 0; v < E; v++) CHECK(draw.branch_lengths_[k * (E + 1) + v] > 0.0);
  }
  // a particle depends on (seed, first_sample + t) alone; the same epsilon handed back gives the same bits
  const BranchModelDraw tail = engine.BranchModelSample(
      4, n, 3, std::vector<int32_t>(index.begin() + 60 * 3 * E, index.end()), q, 20261021, 65);
  for (size_t i = 0; i < 4 * E; i++) CHECK(tail.epsilon_[i] == draw.epsilon_[60 * E + i]);
  const BranchModelDraw again = engine.BranchModelSample(K, n, 3, index, q, 0, 0, 10.0, draw.epsilon_);
  CHECK(again.branch_lengths_ == draw.branch_lengths_ && again.log_q_ == draw.log_q_);

  std::vector<double> g(K * (E + 2), 0.0), ll(K);
  for (size_t k = 0; k < K; k++) {
    ll[k] = -70.0 - 0.25 * (double)k;
    for (size_t v = 0; v < E; v++) g[k * (E + 2) + v] = 3.0 - 0.5 * (double)v + 0.01 * (double)k;
  }
  const BranchModelGradientResult grad = engine.BranchModelGradient(K, n, 3, index, q, draw, g, ll, drawn.log_prob_, {}, 0.5);
  CHECK(grad.gradient_.size() == 2 * V && grad.log_f_.size() == K);
  for (size_t k = 0; k < K; k++)
    CHECK(grad.log_f_[k] == ((0.5 * ll[k] + draw.log_prior_[k]) - drawn.log_prob_[k]) - draw.log_q_[k]);
  for (const double x : grad.gradient_) CHECK(std::isfinite(x));

  print("support", parents, " %d");
  print("log_params", sa.log_params_, " %a");
  print("first_index", std::vector<int32_t>(index.begin(), index.begin() + 3 * E), " %d");
  print("log_q", draw.log_q_, " %a");
  print("first_lengths", std::vector<double>(draw.branch_lengths_.begin(), draw.branch_lengths_.begin() + E + 1), " %a");
  print("gradient", grad.gradient_, " %a");
  print("log_f", grad.log_f_, " %a");
  std::printf(failures ? "FAILED (%d)\n" : "status all checks passed\n", failures);
  return failures ? 1 : 0;
}
