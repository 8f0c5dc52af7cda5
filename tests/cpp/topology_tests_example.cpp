// Engine::BootstrapWeights and Engine::TopologyTests of the C++ adapter
// (libsbn_amd/csrc/host/engine.hpp) on the hello alignment.  Prints every value as a hexadecimal
// float, one "name index value" per line, for tests/test_topology_tests_gpu.py to compare with the
// Python call bit for bit.  Three scales (1, 0.5, 1.5), 64 replicates each, seed 5, first replicate 3.
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
  const size_t T = trees.TreeCount(), P = pattern.PatternCount(), B = 64;
  const auto w = engine.BootstrapWeights(4, 0, 5, 3);
  const auto r = engine.TopologyTests(trees.trees_, params, false, {1.0, 0.5, 1.5}, B, 5, 3);
  std::printf("shape %zu %zu %zu\n", T, P, B);
  auto dump = [](const char* name, const std::vector<double>& v) {
    for (size_t i = 0; i < v.size(); i++) std::printf("%s %zu %a\n", name, i, v[i]);
  };
  dump("boot.w", w);
  dump("topo.ll", r.log_likelihoods_);
  dump("topo.s", r.pattern_log_likelihoods_);
  dump("topo.table", r.table_);
  dump("topo.mean", r.column_mean_);
  for (size_t i = 0; i < r.counts_.size(); i++) std::printf("topo.counts %zu %d\n", i, r.counts_[i]);
  for (size_t i = 0; i < r.sites_.size(); i++) std::printf("topo.sites %zu %lld\n", i, static_cast<long long>(r.sites_[i]));
  return 0;
}
