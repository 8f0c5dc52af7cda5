// Split tables through the C++ Engine adapter (libsbn_amd/csrc/host/engine.hpp): the twelve
// rootsplits of the reference's five_taxon example (src/unrooted_sbn_instance.hpp:104-106), RF
// distances between its trees and the consensus of one tree's copies.  Exit code 0 = all checks
// passed.
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
  const size_t T = five.TreeCount(), n = 5;
  CHECK(T == 4);
  std::vector<int32_t> parents;
  std::vector<double> lengths;
  for (const auto& tree : five.trees_) {
    parents.insert(parents.end(), tree.parent_ids.begin(), tree.parent_ids.end());
    lengths.insert(lengths.end(), tree.branch_lengths.begin(), tree.branch_lengths.end());
  }
  CHECK(parents.size() == T * (2 * n - 3));
  CHECK(lengths.size() == T * (2 * n - 2));
  const SplitTable table = engine.SplitIndex(T, n, parents, lengths);
  const std::set<std::string> want{"01110", "01010", "00101", "00111", "00001", "00011",
                                   "00010", "00100", "00110", "01000", "01111", "01001"};
  std::set<std::string> got;
  for (size_t k = 0; k < table.split_count_; k++) {
    std::string s;
    for (size_t i = 0; i < n; i++) s += (table.bits_[k] >> i) & 1u ? '1' : '0';
    got.insert(s);
  }
  CHECK(table.split_count_ == 12);
  CHECK(got == want);
  for (size_t v = 0; v < 2 * n - 3; v++) CHECK(table.split_index_[v] == (int32_t)v);
  CHECK(table.split_index_[2 * n - 3] == -1 && table.split_index_[2 * n - 2] == -1);
  for (size_t v = 0; v < n; v++) CHECK(table.trees_[v] == 4 && table.stats_[3 * v] == 4.0);

  const TreeDistances d = engine.RfDistances(T, n, table.split_index_, lengths);
  for (size_t a = 0; a < T; a++) {
    CHECK(d.rf_[a * T + a] == 0 && d.branch_score_[a * T + a] == 0.0);
    for (size_t b = 0; b < T; b++) {
      CHECK(d.rf_[a * T + b] == d.rf_[b * T + a] && d.rf_[a * T + b] % 2 == 0 && d.rf_[a * T + b] <= 4);
      CHECK(d.branch_score_[a * T + b] == d.branch_score_[b * T + a]);
    }
  }

  // three copies of tree 1: its consensus is the tree itself
  std::vector<int32_t> copies;
  for (int c = 0; c < 3; c++) copies.insert(copies.end(), parents.begin() + 7, parents.begin() + 14);
  const SplitTable own = engine.SplitIndex(3, n, copies);
  CHECK(own.split_count_ == 7);
  std::vector<double> weight(own.trees_.begin(), own.trees_.end());
  const ConsensusTreeResult tree = ConsensusTree(n, own.bits_, weight, 3.0);
  CHECK(tree.node_split_.size() == 2 * n - 2);
  CHECK(tree.parent_ids_ == std::vector<int32_t>(copies.begin(), copies.begin() + 7));
  bool refused = false;
  try {
    ConsensusTree(n, own.bits_, weight, 3.0, 0.49);
  } catch (const std::runtime_error&) {
    refused = true;
  }
  CHECK(refused);

  std::printf(failures ? "FAILED (%d)\n" : "splits_example: all checks passed\n", failures);
  return failures ? 1 : 0;
}
