// Engine::SprSearch and Engine::SprApply of the C++ adapter (libsbn_amd/csrc/host/engine.hpp)
// on DS1's ten sampled trees: prints, per tree, what tests/test_spr_search_gpu.py compares
// with the Python result -- status, moves, log-likelihood (hexadecimal, exact), parent ids.
#include <cstdio>
#include <string>

#include "../../libsbn_amd/csrc/host/engine.hpp"

using namespace mihost;

int main(int argc, char** argv) {
  const std::string data = argc > 1 ? argv[1] : "tests/golden/data";
  const PhyloModelSpecification simple{"JC69", "constant", "strict"};
  auto trees = TreeCollection::ParseNexusFile(data + "/DS1.subsampled_10.t");
  SitePattern pattern(Alignment::ReadFasta(data + "/DS1.fasta"), trees.taxon_names_);
  Engine engine(EngineSpecification{1, {}, true}, simple, pattern);
  ParamMatrix params(trees.TreeCount(), engine.ParameterCount());
  mi_spr_search_options options{};
  options.max_moves = 2;
  options.pack_active = 1;
  options.min_gain = 1e-3;
  options.radius = 3;
  const auto ends = engine.SprSearch(trees.trees_, params, false, &options);
  std::vector<int32_t> first;
  for (size_t t = 0; t < ends.size(); t++) {
    const auto& e = ends[t];
    std::printf("tree %zu status %d opt %d ll %a delta %a moves", t, e.status_, e.branch_opt_status_,
                e.log_likelihood_, e.best_delta_);
    for (int32_t m : e.moves_) std::printf(" %d", m);
    std::printf(" parents");
    for (int32_t p : e.parent_ids_) std::printf(" %d", p);
    std::printf("\n");
    for (int i = 0; i < 3; i++) first.push_back(e.moves_.empty() ? -1 : e.moves_[i]);
  }
  // the first move of every tree taken on its own: the tree the search went to
  const auto moved = engine.SprApply(trees.trees_, first);
  for (size_t t = 0; t < moved.size(); t++) {
    std::printf("applied %zu move %d %d %d parents", t, first[3 * t], first[3 * t + 1], first[3 * t + 2]);
    for (int32_t p : moved[t].first) std::printf(" %d", p);
    std::printf("\n");
  }
  std::printf("done\n");
  return 0;
}
