// Quartet hybrid marginals through the C++ Engine adapter (libsbn_amd/csrc/host/engine.hpp): the
// reference's second-simplest hybrid DAG through Engine::GpCreate -- the request tables, the hybrid
// marginals with their summands and the SBN estimate that prefers them.  Prints the results
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

int main(int argc, char** argv) {
  const std::string data = argc > 1 ? argv[1] : "tests/golden/data";
  const PhyloModelSpecification simple{"JC69", "constant", "strict"};
  auto trees = TreeCollection::ParseNewickFile(data + "/second-simplest-hybrid-marginal.nwk");
  SitePattern pattern(Alignment::ReadFasta(data + "/7-taxon-slice-of-ds1.fasta"), trees.taxon_names_);
  Engine engine(EngineSpecification{1, {}, true}, simple, pattern);

  std::vector<int32_t> parents;
  for (const auto& tree : trees.trees_) parents.insert(parents.end(), tree.parent_ids.begin(), tree.parent_ids.end());
  const std::vector<double> model_row((size_t)engine.ParameterCount(), 1.0);
  const GeneralizedPruning gp = engine.GpCreate(trees.TreeCount(), parents, {}, model_row);
  const size_t G = gp.EntryCount();

  const GpHybridRequests req = gp.HybridRequests();
  CHECK(req.requests_.size() == 3 * G && req.SummandCount() > 0);
  size_t formed = 0, counted = 0;
  for (size_t e = 0; e < G; e++) {
    if (!req.requests_[3 * e]) continue;
    CHECK((size_t)req.requests_[3 * e + 1] == counted);
    counted += (size_t)req.requests_[3 * e + 2];
    formed++;
  }
  CHECK(formed > 0 && counted == req.SummandCount());

  const GpHybridResult hyb = gp.HybridMarginals();
  CHECK(hyb.hybrid_.size() == G && hyb.summands_.size() == req.SummandCount());
  for (size_t e = 0; e < G; e++) CHECK(req.requests_[3 * e] ? std::isfinite(hyb.hybrid_[e]) : hyb.hybrid_[e] == -INFINITY);
  const std::vector<double> q = gp.EstimateSbnParameters(true);
  CHECK(q == gp.SbnParameters());

  print("hybrid", hyb.hybrid_);
  print("summands", hyb.summands_);
  std::printf("summand_entries");
  for (const int32_t x : req.summands_) std::printf(" %d", x);
  std::printf("\n");
  print("estimated_q", q);
  return failures ? 1 : 0;
}
