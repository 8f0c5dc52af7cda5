// Engine::AncestralStates of the C++ adapter (libsbn_amd/csrc/host/engine.hpp) on the hello
// alignment, every optional output asked for.  Prints every value as a hexadecimal float (map
// states as integers), one "name index value" per line, for tests/test_ancestral_gpu.py to
// compare with the Python call bit for bit.
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
  const auto r = engine.AncestralStates(trees.trees_, params, false, true, true, true);
  std::printf("shape %zu %zu %zu\n", trees.TreeCount(), pattern.SequenceCount(), pattern.PatternCount());
  auto dump = [](const char* name, size_t t, const std::vector<double>& v) {
    for (size_t i = 0; i < v.size(); i++) std::printf("%s %zu %a\n", name, t * v.size() + i, v[i]);
  };
  for (size_t t = 0; t < r.size(); t++) {
    std::printf("ll %zu %a\n", t, r[t].log_likelihood_);
    dump("state", t, r[t].state_posteriors_);
    for (size_t i = 0; i < r[t].map_states_.size(); i++)
      std::printf("map %zu %d\n", t * r[t].map_states_.size() + i, static_cast<int>(r[t].map_states_[i]));
    dump("cat", t, r[t].category_posteriors_);
    dump("rate", t, r[t].pattern_rates_);
    dump("tip", t, r[t].tip_posteriors_);
  }
  return 0;
}
