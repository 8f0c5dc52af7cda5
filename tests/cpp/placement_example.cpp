// Engine::Placement of the C++ adapter (libsbn_amd/csrc/host/engine.hpp) on the hello alignment:
// five queries over the identity column map with the pattern weights, two pendant lengths, every
// optional output asked for.  Prints every value as a hexadecimal float (indices as integers), one
// "name index value" per line, for tests/test_placement_gpu.py to compare with the Python call bit
// for bit.  Query q shows state (q + c) mod 5 in column c (4: a gap).
#include <cstdio>
#include <string>

#include "../../libsbn_amd/csrc/host/engine.hpp"

using namespace mihost;

int main(int argc, char** argv) {
  const std::string data = argc > 1 ? argv[1] : "tests/golden/data";
  const PhyloModelSpecification model{"JC69", "weibull+4", "strict"};
  auto trees = TreeCollection::ParseNewickFile(data + "/hello.nwk");
  SitePattern pattern(Alignment::ReadFasta(data + "/hello.fasta"), trees.taxon_names_);
  Engine engine(EngineSpecification{1, {}, true}, model, pattern);
  ParamMatrix params(trees.TreeCount(), engine.ParameterCount());
  params.SetBlock(engine.GetPhyloModelBlockSpecification().at("Weibull shape").first, 1, {0.8});
  const size_t P = pattern.PatternCount(), Q = 5;
  std::vector<int8_t> queries(Q * P);
  std::vector<int32_t> column(P);
  for (size_t c = 0; c < P; c++) column[c] = static_cast<int32_t>(c);
  for (size_t q = 0; q < Q; q++)
    for (size_t c = 0; c < P; c++) queries[q * P + c] = static_cast<int8_t>((q + c) % 5);
  const std::vector<double> weights(pattern.GetWeights().begin(), pattern.GetWeights().end());
  const auto r = engine.Placement(trees.trees_, params, false, queries, column, weights, {0.05, 0.4}, true, true, true);
  std::printf("shape %zu %zu %zu\n", trees.TreeCount(), pattern.SequenceCount(), P);
  auto dump = [](const char* name, size_t t, const std::vector<double>& v) {
    for (size_t i = 0; i < v.size(); i++) std::printf("%s %zu %a\n", name, t * v.size() + i, v[i]);
  };
  for (size_t t = 0; t < r.size(); t++) {
    std::printf("ll %zu %a\n", t, r[t].log_likelihood_);
    dump("edge", t, r[t].edge_log_likelihoods_);
    for (size_t i = 0; i < r[t].best_edge_.size(); i++)
      std::printf("best %zu %d\n", t * r[t].best_edge_.size() + i, static_cast<int>(r[t].best_edge_[i]));
    for (size_t i = 0; i < r[t].pendant_index_.size(); i++)
      std::printf("pend %zu %d\n", t * r[t].pendant_index_.size() + i, static_cast<int>(r[t].pendant_index_[i]));
    dump("lwr", t, r[t].lwr_);
    dump("table", t, r[t].tables_);
  }
  return 0;
}
