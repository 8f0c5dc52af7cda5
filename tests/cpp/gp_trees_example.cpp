// Trees of the subsplit DAG through the C++ Engine adapter (libsbn_amd/csrc/host/engine.hpp): the
// reference's five_taxon_rooted example through Engine::GpCreateDag -- the index of the loaded trees,
// the rooted TrainSimpleAverage, sampled and enumerated trees, and de-rooting.  Prints the results
// (doubles as hexadecimal floats) for the test that makes the same calls from Python.
// Exit code 0 = all checks passed.
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

static void print(const char* name, const std::vector<double>& values) {
  std::printf("%s", name);
  for (const double x : values) std::printf(" %a", x);
  std::printf("\n");
}
static void print(const char* name, const std::vector<int32_t>& values) {
  std::printf("%s", name);
  for (const int32_t x : values) std::printf(" %d", x);
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
  const GeneralizedPruning gp = engine.GpCreateDag(five.TreeCount(), parents);
  const auto sizes = gp.Sizes();
  CHECK(sizes[0] == 5 && sizes[2] == 3 && sizes[3] == 34);
  const int32_t G = sizes[3];
  CHECK(gp.TopologyCount() == 4);

  const GpTreeIndexResult index = gp.TreeIndex(five.TreeCount(), parents);
  for (const int32_t e : index.entries_) CHECK(e >= 0 && e < G);
  const std::vector<double> q = gp.TrainSimpleAverage(index.entries_);
  CHECK(q == gp.SbnParameters());
  CHECK(std::fabs(q[0] + q[1] + q[2] - 1.0) < 1e-12);

  const GpTreesResult sampled = gp.SampleTrees(8, 42, 3);
  CHECK(gp.TreeIndex(8, sampled.parent_ids_).entries_ == sampled.entries_);
  CHECK(gp.TreeLogProb(sampled.entries_) == sampled.log_q_);
  CHECK(gp.TreeBranchLengths(sampled.entries_) == sampled.branch_lengths_);
  const GpTreesResult all = gp.EnumerateTrees(0, 4);
  double total = 0.0;
  for (const double x : all.log_q_) total += std::exp(x);
  CHECK(std::fabs(total - 1.0) < 1e-12);
  const DerootedTrees unrooted = engine.DerootTrees(4, 5, all.parent_ids_, all.branch_lengths_);
  for (const int32_t p : unrooted.parent_ids_) CHECK(p >= 5 && p <= 7);

  bool refused = false;
  try {
    gp.Populate();
  } catch (const std::runtime_error&) {
    refused = true;
  }
  CHECK(refused);
  refused = false;
  try {
    gp.EnumerateTrees(3, 2);
  } catch (const std::runtime_error&) {
    refused = true;
  }
  CHECK(refused);

  print("entries", index.entries_);
  print("trained_q", q);
  print("sampled_parent_ids", sampled.parent_ids_);
  print("sampled_log_q", sampled.log_q_);
  print("enumerated_parent_ids", all.parent_ids_);
  print("enumerated_log_q", all.log_q_);
  print("derooted_parent_ids", unrooted.parent_ids_);
  print("derooted_lengths", unrooted.branch_lengths_);
  print("root_edge", unrooted.root_edge_);
  return failures ? 1 : 0;
}
