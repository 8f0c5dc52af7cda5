// Subsplit Bayesian networks through the C++ Engine adapter (libsbn_amd/csrc/host/engine.hpp): the
// support of the reference's five_taxon example (twelve rootsplits, the PCSP block of parent
// 00001|11110: src/unrooted_sbn_instance.hpp:104-118), simple-average and EM training on it and
// the probabilities of its trees.  Exit code 0 = all checks passed.
#include <cmath>
#include <cstdio>
#include <set>
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

int main(int argc, char** argv) {
  const std::string data = argc > 1 ? argv[1] : "tests/golden/data";
  const PhyloModelSpecification simple{"JC69", "constant", "strict"};
  auto hello = TreeCollection::ParseNewickFile(data + "/hello.nwk");
  SitePattern pattern(Alignment::ReadFasta(data + "/hello.fasta"), hello.taxon_names_);
  Engine engine(EngineSpecification{1, {}, true}, simple, pattern);

  auto five = TreeCollection::ParseNewickFile(data + "/five_taxon_unrooted.nwk");
  const size_t T = five.TreeCount(), n = 5, E = 2 * n - 3;
  CHECK(T == 4);
  std::vector<int32_t> parents;
  for (const auto& tree : five.trees_) parents.insert(parents.end(), tree.parent_ids.begin(), tree.parent_ids.end());
  const SbnSupport support = engine.SbnIndex(T, n, parents);
  CHECK(support.rootsplit_count_ == 12);
  const size_t S = support.rootsplit_count_, P = support.ParameterCount();

  // a clade 2 split + side as the reference prints it
  auto clade = [&](int32_t c) {
    std::string s;
    for (size_t i = 0; i < n; i++) s += (((support.bits_[c >> 1] >> i) & 1u) != (uint32_t)(c & 1)) ? '1' : '0';
    return s;
  };
  std::set<std::string> block;
  int32_t block_parent = -1;
  for (size_t i = 0; i < support.pcsp_count_; i++) {
    const int32_t* k = &support.pcsp_clades_[3 * i];
    if (clade(k[0]) == "00001" && clade(k[1]) == "11110") {
      block.insert(clade(k[2]));
      CHECK(block_parent < 0 || block_parent == support.pcsp_parent_[i]);
      block_parent = support.pcsp_parent_[i];
    }
  }
  CHECK((block == std::set<std::string>{"01110", "00010", "01000", "00100"}));
  CHECK(block_parent >= 0 && support.parent_range_[2 * block_parent + 1] - support.parent_range_[2 * block_parent] == 4);
  for (size_t i = 0; i < support.slot_index_.size(); i++)
    CHECK(support.slot_index_[i] >= -1 && support.slot_index_[i] < (int32_t)P);

  // simple average: normalised blocks, every tree's probability positive, at most 1 in all
  const SbnTraining sa = engine.SbnTrain(support, MI_SBN_SA);
  CHECK(sa.score_history_.empty());
  double z = 0.0;
  for (size_t j = 0; j < S; j++) z += std::exp(sa.log_params_[j]);
  CHECK(std::fabs(z - 1.0) < 1e-12);
  const SbnProbabilities p = engine.SbnLogProb(support, sa.log_params_, true, true);
  double total = 0.0;
  for (size_t t = 0; t < T; t++) {
    CHECK(std::isfinite(p.log_q_[t]) && p.log_q_[t] < 0.0);
    total += std::exp(p.log_q_[t]);
    double m = -INFINITY;
    for (size_t v = 0; v < E; v++) m = std::fmax(m, p.rooting_log_prob_[t * E + v]);
    CHECK(m <= p.log_q_[t]);
  }
  CHECK(total <= 1.0 + 1e-12);
  // the expected rootsplit usages of the four trees add up to four
  double used = 0.0;
  for (size_t j = 0; j < S; j++) used += std::exp(p.log_expected_counts_[j]);
  CHECK(std::fabs(used - 4.0) < 1e-10);

  // EM never lowers the score; unnormalised parameters are normalised by the call
  const SbnTraining em = engine.SbnTrain(support, MI_SBN_EM, {}, 0.0, 5);
  CHECK(em.score_history_.size() == 5);
  for (size_t i = 1; i < em.score_history_.size(); i++)
    CHECK(em.score_history_[i] >= em.score_history_[i - 1] - 1e-10 * std::fabs(em.score_history_[i - 1]));
  std::vector<double> shifted = sa.log_params_;
  for (double& x : shifted) x += 3.0;
  const SbnProbabilities q = engine.SbnLogProb(support, shifted);
  for (size_t t = 0; t < T; t++) CHECK(std::fabs(q.log_q_[t] - p.log_q_[t]) < 1e-12);

  std::printf(failures ? "FAILED (%d)\n" : "sbn_example: all checks passed\n", failures);
  return failures ? 1 : 0;
}
