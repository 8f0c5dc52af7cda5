// The offset arithmetic of the host-pointer calls (libsbn_amd/csrc/mi_phylo_host_arrays.h), checked
// without a device: for array lists shaped like every call kind's, tree counts 1, 2, 5, 11 and
// 1 to 4 shards, that the tree slices cover every byte of every wanted per-tree array exactly
// once and stay inside it, that the packed block's pieces are 256-byte aligned and disjoint, and
// that the scratch of the shards is laid out without overlap and added up in full.  Every array
// is a heap block of exactly its size, so built with -fsanitize=address,undefined a slice that
// reaches outside its array stops the program.
//   g++ -std=c++17 -g -fsanitize=address,undefined tests/cpp/host_arrays_check.cpp -o check && ./check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../libsbn_amd/csrc/mi_phylo_host_arrays.h"

namespace {

int failures = 0;
#define CHECK(cond, ...)                       \
  do {                                         \
    if (!(cond)) {                             \
      failures++;                              \
      std::printf("FAILED %s: ", #cond);       \
      std::printf(__VA_ARGS__);                \
      std::printf("\n");                       \
    }                                          \
  } while (0)

// 8 taxa, 40 patterns, 4 categories, a GTR model's 12 parameters
constexpr size_t n = 8, N = 2 * n - 1, P = 40, K = 4, kParams = 12, kIndexCount = 9, kMaxMoves = 3;
double* const F64 = reinterpret_cast<double*>(1);  // "wanted": replaced by a real block in walk()
int32_t* const I32 = reinterpret_cast<int32_t*>(1);
int8_t* const I8 = reinterpret_cast<int8_t*>(1);
double* const NO_F64 = nullptr;
int8_t* const NO_I8 = nullptr;

struct Kind {
  std::string name;
  std::vector<HostArray> in, out;
};

std::vector<HostArray> tree_inputs(bool rooted = false) {
  const size_t np = rooted ? 2 * n - 2 : 2 * n - 3;
  return {per_tree(I32, np), per_tree(F64, np + 1), per_tree(F64, kParams)};
}
std::vector<HostArray> plus(std::vector<HostArray> a, const std::vector<HostArray>& b) {
  a.insert(a.end(), b.begin(), b.end());
  return a;
}

// the lists of the entry points (include/mi_phylo.h gives the shapes), optional outputs on and off
std::vector<Kind> kinds() {
  const Combine S = kPerTreeSum;
  return {
      {"log_likelihoods", tree_inputs(), {per_tree(F64, 1, S)}},
      {"gradients", tree_inputs(), {per_tree(F64, 1, S), per_tree(F64, N, S), per_tree(F64, 1, S), per_tree(F64, 8, S)}},
      {"gradients, branch block only", tree_inputs(), {per_tree(F64, 1, S), per_tree(F64, N, S), per_tree(NO_F64, 1, S), per_tree(NO_F64, 8, S)}},
      {"gradients_reduced", plus(tree_inputs(), {per_tree(I32, N), per_tree(F64, 1)}),
       {per_tree(F64, 1, S), fixed(F64, 2, kCallSum), fixed(F64, kIndexCount, kCallSum)}},
      {"gradients_reduced, no weights, no logL", plus(tree_inputs(), {per_tree(I32, N), per_tree(NO_F64, 1)}),
       {per_tree(NO_F64, 1, S), fixed(F64, 2, kCallSum), fixed(F64, kIndexCount, kCallSum)}},
      {"branch_hessian", tree_inputs(), {per_tree(F64, 1, S), per_tree(F64, N, S), per_tree(F64, N, S), per_tree(F64, N, S)}},
      {"branch_hessian, H only", tree_inputs(), {per_tree(NO_F64, 1, S), per_tree(NO_F64, N, S), per_tree(F64, N, S), per_tree(NO_F64, N, S)}},
      {"nni_scan", tree_inputs(), {per_tree(F64, 1, S), per_tree(F64, N * 2, S), per_tree(I32, 1)}},
      {"pattern_log_likelihoods", tree_inputs(), {per_tree(F64, 1, S), per_tree(F64, P)}},
      {"ancestral_states", tree_inputs(),
       {per_tree(F64, 1, S), per_tree(F64, (n - 2) * P * 4), per_tree(I8, (n - 2) * P), per_tree(F64, P * K), per_tree(F64, P), per_tree(F64, n * P * 4)}},
      {"ancestral_states, states only", tree_inputs(),
       {per_tree(NO_F64, 1, S), per_tree(F64, (n - 2) * P * 4), per_tree(NO_I8, (n - 2) * P), per_tree(NO_F64, P * K), per_tree(NO_F64, P), per_tree(NO_F64, n * P * 4)}},
      {"rooted_log_likelihoods", plus(tree_inputs(true), {per_tree(F64, N - 1), per_tree(F64, N), per_tree(F64, N)}), {per_tree(F64, 1)}},
      {"rooted_gradients",
       plus(tree_inputs(true), {per_tree(F64, N - 1), per_tree(F64, N), per_tree(F64, N), per_tree(I32, 1), per_tree(F64, n - 1)}),
       {per_tree(F64, 1), per_tree(F64, n - 1), per_tree(F64, N - 1), per_tree(F64, 1), per_tree(F64, 8)}},
      {"optimize_branch_lengths", tree_inputs(),
       {per_tree(F64, N - 1), per_tree(F64, 1), per_tree(F64, N), per_tree(NO_F64, N), per_tree(I32, 1), per_tree(I32, 1)}},
      {"nni_apply", {per_tree(I32, 2 * n - 3), per_tree(F64, 2 * n - 2), per_tree(I32, 1)}, {per_tree(I32, 2 * n - 3), per_tree(F64, 2 * n - 2)}},
      {"nni_search", tree_inputs(),
       {per_tree(I32, 2 * n - 3), per_tree(F64, 2 * n - 2), per_tree(F64, 1), per_tree(F64, 1), per_tree(I32, 1), per_tree(I32, kMaxMoves),
        per_tree(F64, kMaxMoves), per_tree(I32, 1), per_tree(I32, 1)}},
      {"spr_apply", {per_tree(I32, 2 * n - 3), per_tree(F64, 2 * n - 2), per_tree(I32, 3)}, {per_tree(I32, 2 * n - 3), per_tree(F64, 2 * n - 2)}},
      {"spr_search", tree_inputs(),
       {per_tree(I32, 2 * n - 3), per_tree(F64, 2 * n - 2), per_tree(F64, 1), per_tree(F64, 1), per_tree(I32, 1), per_tree(I32, 3 * kMaxMoves),
        per_tree(F64, kMaxMoves), per_tree(I32, 1), per_tree(I32, 1)}},
  };
}
// (not per tree throughout: these go to one engine whole, so only their packing is checked)
std::vector<Kind> unsharded_kinds(size_t T) {
  const size_t B = 7, G = 23, V = 5;  // replicates; DAG entries; a fit's branch-length variables
  int32_t* const NO_I32 = nullptr;
  return {
      // the trees of the subsplit DAG, de-rooting, the pieces of a rooted variational step, the optimiser call
      {"gp_tree_index", {fixed(I32, T * (N - 1))}, {fixed(I32, T * N), fixed(I32, T * N)}},
      {"gp_tree_index, no nodes", {fixed(I32, T * (N - 1))}, {fixed(I32, T * N), fixed(NO_I32, T * N)}},
      {"gp_tree_log_prob", {fixed(I32, T * N)}, {fixed(F64, T)}},
      {"gp_tree_branch_lengths", {fixed(I32, T * N)}, {fixed(F64, T * N)}},
      {"gp_train_simple_average", {fixed(I32, T * N), fixed(F64, T)}, {fixed(F64, G)}},
      {"gp_train_simple_average, no weights, no q", {fixed(I32, T * N), fixed(NO_F64, T)}, {fixed(NO_F64, G)}},
      {"gp_sample_trees", {}, {fixed(I32, T * (N - 1)), fixed(I32, T * N), fixed(F64, T), fixed(F64, T * N), fixed(F64, G)}},
      {"gp_enumerate_trees, no lengths", {}, {fixed(I32, T * (N - 1)), fixed(I32, T * N), fixed(F64, T), fixed(NO_F64, T * N), fixed(NO_F64, G)}},
      {"deroot_trees_mapped", {fixed(I32, T * (N - 1)), fixed(F64, T * N)},
       {fixed(I32, T * (N - 2)), fixed(F64, T * (N - 1)), fixed(I32, T), fixed(I32, T * N)}},
      {"deroot_trees, no lengths", {fixed(I32, T * (N - 1)), fixed(NO_F64, T * N)},
       {fixed(I32, T * (N - 2)), fixed(NO_F64, T * (N - 1)), fixed(I32, T), fixed(NO_I32, T * N)}},
      {"gp_log_normalize", {fixed(F64, G)}, {fixed(F64, G), fixed(F64, G)}},
      {"gp_log_normalize, no log q", {fixed(F64, G)}, {fixed(NO_F64, G), fixed(F64, G)}},
      {"gp_branch_sample", {fixed(I32, T * N), fixed(F64, 2 * G), fixed(F64, T * (N - 1))},
       {fixed(F64, T * N), fixed(F64, T * (N - 1)), fixed(F64, T), fixed(F64, T)}},
      {"gp_branch_sample, no epsilon given", {fixed(I32, T * N), fixed(F64, 2 * G), fixed(NO_F64, T * (N - 1))},
       {fixed(F64, T * N), fixed(F64, T * (N - 1)), fixed(F64, T), fixed(F64, T)}},
      {"gp_branch_gradient",
       {fixed(I32, T * N), fixed(F64, 2 * G), fixed(F64, T * N), fixed(F64, T * (N - 1)), fixed(F64, T), fixed(F64, T), fixed(I32, T * N),
        fixed(F64, T * N), fixed(F64, T), fixed(F64, T), fixed(F64, T)},
       {fixed(F64, 2 * G), fixed(F64, T)}},
      {"gp_branch_gradient, no log q of the topology, no weights",
       {fixed(I32, T * N), fixed(F64, 2 * G), fixed(F64, T * N), fixed(F64, T * (N - 1)), fixed(F64, T), fixed(F64, T), fixed(I32, T * N),
        fixed(F64, T * N), fixed(F64, T), fixed(NO_F64, T), fixed(NO_F64, T)},
       {fixed(F64, 2 * G), fixed(F64, T)}},
      {"gp_topology_gradient", {fixed(I32, T * N), fixed(F64, G), fixed(F64, T)}, {fixed(F64, G), fixed(F64, T)}},
      {"gp_topology_gradient, no factors", {fixed(I32, T * N), fixed(F64, G), fixed(F64, T)}, {fixed(F64, G), fixed(NO_F64, T)}},
      {"vi_update", {fixed(F64, G), fixed(F64, 2 * V), fixed(F64, T), fixed(F64, T), fixed(F64, T), fixed(F64, T)}, {fixed(F64, 6)}},
      {"vi_update, the tables' one element, no row", {fixed(F64, 1), fixed(F64, 0), fixed(F64, T), fixed(F64, T), fixed(F64, T), fixed(F64, T)},
       {fixed(NO_F64, 6)}},
      {"rell", {fixed(F64, T * P), fixed(F64, B * P)}, {fixed(F64, B * T), fixed(I32, B), fixed(F64, T), fixed(NO_F64, T)}},
      {"rell_bootstrap", plus(tree_inputs(), {fixed(F64, B * P)}),
       {per_tree(F64, 1), per_tree(NO_F64, P), fixed(F64, B * T), fixed(I32, B), per_tree(F64, 1), per_tree(F64, 1)}},
      {"pattern_mixture", {fixed(F64, T * P), fixed(NO_F64, T), fixed(F64, P)}, {fixed(F64, P), fixed(F64, 1)}},
  };
}

// every wanted array becomes a zeroed heap block of exactly its size
void allocate(std::vector<HostArray>& arrays, int T) {
  for (HostArray& a : arrays)
    if (a.host) a.host = std::calloc(a.bytes(T) ? a.bytes(T) : 1, 1);
}
void release(std::vector<HostArray>& arrays) {
  for (HostArray& a : arrays) std::free(a.host);
}

void shard_range(int total, int shards, int shard, int* begin, int* count) {  // (mi_shard_range)
  const int base = total / shards, extra = total % shards;
  *begin = shard * base + (shard < extra ? shard : extra);
  *count = base + (shard < extra ? 1 : 0);
}

void check_pack(const Kind& k, const std::vector<HostArray>& arrays, int T) {
  std::vector<size_t> off;
  const size_t total = pack_offsets(arrays, T, off);
  CHECK(off.size() == arrays.size(), "%s", k.name.c_str());
  CHECK(total % 256 == 0, "%s: block of %zu bytes", k.name.c_str(), total);
  size_t end = 0;  // of the pieces so far: list order is block order, so disjoint means off >= end
  for (size_t i = 0; i < arrays.size(); i++) {
    if (!arrays[i].host) continue;
    CHECK(off[i] % 256 == 0, "%s: piece %zu at %zu", k.name.c_str(), i, off[i]);
    CHECK(off[i] >= end, "%s: piece %zu at %zu overlaps the one before (ends at %zu)", k.name.c_str(), i, off[i], end);
    end = off[i] + arrays[i].bytes(T);
    CHECK(end <= total, "%s: piece %zu ends at %zu of %zu", k.name.c_str(), i, end, total);
  }
}

// tree shards: the slices of one list written shard by shard
void check_slices(const Kind& k, const std::vector<HostArray>& arrays, int T, int D) {
  for (int i = 0; i < D; i++) {
    int first, count;
    shard_range(T, D, i, &first, &count);
    if (!count) continue;
    std::vector<HostArray> s = arrays;
    slice_trees(s, first);
    for (size_t j = 0; j < s.size(); j++) {
      if (!s[j].host || !s[j].per_tree || added_across_shards(s[j], false)) continue;
      const char* base = static_cast<const char*>(arrays[j].host);
      char* p = static_cast<char*>(s[j].host);
      const size_t bytes = s[j].bytes(count);
      CHECK(p >= base && p + bytes <= base + arrays[j].bytes(T), "%s: array %zu, shard %d of %d, T=%d leaves its array",
            k.name.c_str(), j, i, D, T);
      for (size_t b = 0; b < bytes; b++)
        CHECK(p[b] == 0, "%s: array %zu byte %zu covered twice (shard %d of %d, T=%d)", k.name.c_str(), j, b, i, D, T);
      std::memset(p, 1 + i, bytes);
    }
  }
  for (size_t j = 0; j < arrays.size(); j++) {
    if (!arrays[j].host || !arrays[j].per_tree || added_across_shards(arrays[j], false)) continue;
    const char* base = static_cast<const char*>(arrays[j].host);
    for (size_t b = 0; b < arrays[j].bytes(T); b++)
      CHECK(base[b] != 0, "%s: array %zu byte %zu not covered (%d shards, T=%d)", k.name.c_str(), j, b, D, T);
  }
}

// what is added across shards: every shard's outputs land in its own scratch, disjoint, and the sum is whole
void check_sums(const Kind& k, std::vector<HostArray>& outs, int T, int D, bool patterns) {
  const size_t per = shard_scratch_count(outs, T, patterns);
  double* scratch = static_cast<double*>(std::calloc(per ? D * per : 1, sizeof(double)));  // exactly D blocks
  for (int i = 0; i < D; i++) {
    std::vector<HostArray> s = outs;
    point_at_scratch(s, T, patterns, scratch + (size_t)i * per);
    for (size_t j = 0; j < s.size(); j++) {
      if (!added_across_shards(outs[j], patterns)) {
        CHECK(s[j].host == outs[j].host, "%s: output %zu moved", k.name.c_str(), j);
        continue;
      }
      CHECK(outs[j].elem == sizeof(double), "%s: output %zu is summed but no double", k.name.c_str(), j);
      double* p = static_cast<double*>(s[j].host);
      CHECK(p >= scratch + (size_t)i * per && p + s[j].count(T) <= scratch + (size_t)(i + 1) * per,
            "%s: output %zu of shard %d outside its scratch", k.name.c_str(), j, i);
      for (size_t x = 0; x < s[j].count(T); x++) {
        CHECK(p[x] == 0, "%s: scratch of output %zu element %zu used twice", k.name.c_str(), j, x);
        p[x] = (double)((i + 1) * (j + 1));
      }
    }
  }
  add_shards(outs, T, patterns, scratch, per, D);
  for (size_t j = 0; j < outs.size(); j++) {
    if (!added_across_shards(outs[j], patterns)) continue;
    const double* out = static_cast<const double*>(outs[j].host);
    for (size_t x = 0; x < outs[j].count(T); x++)
      CHECK(out[x] == (double)((j + 1) * D * (D + 1) / 2), "%s: output %zu element %zu = %g (%d shards, T=%d)",
            k.name.c_str(), j, x, out[x], D, T);
  }
  std::free(scratch);
}

}  // namespace

int main() {
  int walked = 0;
  for (int T : {1, 2, 5, 11}) {
    for (Kind& k : unsharded_kinds(T)) {
      check_pack(k, k.in, T);
      check_pack(k, k.out, T);
    }
    for (int D = 1; D <= 4; D++)
      for (Kind& k : kinds()) {
        check_pack(k, k.in, T);
        check_pack(k, k.out, T);
        for (bool patterns : {false, true}) {
          bool served = true;  // (pattern shards refuse what is per tree only)
          for (const HostArray& a : k.out) served = served && !(patterns && a.host && a.combine == kPerTree);
          if (!served) continue;
          allocate(k.in, T);
          allocate(k.out, T);
          if (!patterns) {
            check_slices(k, k.in, T, D);
            check_slices(k, k.out, T, D);
          }
          check_sums(k, k.out, T, D, patterns);
          release(k.in);
          release(k.out);
          for (HostArray& a : k.in) a.host = a.host ? F64 : nullptr;
          for (HostArray& a : k.out) a.host = a.host ? F64 : nullptr;
          walked++;
        }
      }
  }
  std::printf("%d lists walked, %d failures\n", walked, failures);
  return failures ? 1 : 0;
}
