// The arrays of a host-pointer call and the arithmetic on them: where each lies in the one packed
// block that travels each way, which part of it a tree shard gets, and where the shards of a
// handle leave what is added up afterwards.  Plain C++ -- no HIP, no engine -- so that
// tests/cpp/host_arrays_check.cpp can compile and check it without a device; the copies
// themselves are mi_phylo_host_calls.cpp's.
#pragma once
#include <cstddef>
#include <vector>

// How an output combines across the shards of a handle.
enum Combine {
  kPerTree,     // tree shards slice it; pattern shards cannot serve it
  kPerTreeSum,  // per tree, and a sum over site patterns: tree shards slice it, pattern shards add it
  kCallSum      // a sum over the whole call (not per tree): either kind of shard adds it
};

struct HostArray {
  void* host = nullptr;  // the caller's array (an input is only read); null: absent / not wanted
  size_t elem = 0;       // bytes per element
  size_t per_tree = 0;   // elements per tree, or ...
  size_t fixed = 0;      // ... of an array that is not per tree, elements in all
  Combine combine = kPerTree;  // (outputs)
  void* dev = nullptr;   // its device address during the call; null when absent
  size_t count(int T) const { return per_tree ? per_tree * (size_t)T : fixed; }
  size_t bytes(int T) const { return elem * count(T); }
  template <typename U>
  U* at() const { return static_cast<U*>(dev); }
};
template <typename U>
HostArray per_tree(const U* host, size_t elements_per_tree, Combine combine = kPerTree) {
  return {const_cast<U*>(host), sizeof(U), elements_per_tree, 0, combine, nullptr};
}
template <typename U>
HostArray fixed(const U* host, size_t elements, Combine combine = kPerTree) {
  return {const_cast<U*>(host), sizeof(U), 0, elements, combine, nullptr};
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// One block for the present arrays of a list, each piece 256-byte aligned, in list order:
// their offsets (an absent array has none to speak of) and the block's size.
inline size_t pack_offsets(const std::vector<HostArray>& arrays, int T, std::vector<size_t>& offsets) {
  size_t total = 0;
  offsets.clear();
  for (const HostArray& a : arrays) {
    offsets.push_back(total);
    if (a.host) total += align256(a.bytes(T));
  }
  return total;
}

// A tree shard's view of a list: every per-tree array from tree `first` on.
inline void slice_trees(std::vector<HostArray>& arrays, int first) {
  for (HostArray& a : arrays)
    if (a.host && a.per_tree) a.host = static_cast<char*>(a.host) + a.elem * a.per_tree * (size_t)first;
}

// Outputs that every shard writes to scratch of its own, to be added in shard order: the sums
// over the call, and under pattern shards what is a sum over site patterns.  (All are doubles.)
inline bool added_across_shards(const HostArray& a, bool pattern_shards) {
  return a.host && (a.combine == kCallSum || (pattern_shards && a.combine == kPerTreeSum));
}
inline size_t shard_scratch_count(const std::vector<HostArray>& outs, int T, bool pattern_shards) {
  size_t count = 0;
  for (const HostArray& a : outs)
    if (added_across_shards(a, pattern_shards)) count += a.count(T);
  return count;
}
// (T: the caller's tree count, as in shard_scratch_count and add_shards -- the layout is one)
inline void point_at_scratch(std::vector<HostArray>& outs, int T, bool pattern_shards, double* scratch) {
  for (HostArray& a : outs)
    if (added_across_shards(a, pattern_shards)) {
      a.host = scratch;
      scratch += a.count(T);
    }
}
// the caller's arrays = the scratch blocks (`stride` doubles apart) added from zero in shard order
inline void add_shards(const std::vector<HostArray>& outs, int T, bool pattern_shards, const double* scratch,
                       size_t stride, int shards) {
  size_t off = 0;
  for (const HostArray& a : outs) {
    if (!added_across_shards(a, pattern_shards)) continue;
    double* out = static_cast<double*>(a.host);
    for (size_t k = 0; k < a.count(T); k++) {
      double sum = 0;
      for (int i = 0; i < shards; i++) sum += scratch[(size_t)i * stride + off + k];
      out[k] = sum;
    }
    off += a.count(T);
  }
}
