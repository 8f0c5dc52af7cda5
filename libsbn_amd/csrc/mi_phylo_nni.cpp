// Host side of the NNI neighbourhood scan: the neighbour trees themselves
// (mi_nni_neighbour: what a caller needs to TAKE the move the scan recommends) and the best
// move of a tree from its delta.  Plain host arithmetic: no device is touched.
#include <cmath>

#include "mi_phylo_engine.h"

// The largest delta of a tree's [N][2], the lowest code 2 v + i among equals, NaN entries
// passed over; -1 for a tree without inner edges.  (nni_finalize_kernel, kernels_nni.hip, takes
// the same decision on the device.)
int32_t nni_best_move(int n, const double* delta) {
  if (n <= 3) return -1;
  double best = -HUGE_VAL;
  int32_t code = 2 * n;
  for (int c = 2 * n; c < 2 * (2 * n - 3); c++)
    if (delta[c] > best) {
      best = delta[c];
      code = c;
    }
  return code;
}

extern "C" {

int32_t mi_nni_neighbour(int32_t n, const int32_t* parent_ids, const double* bl, int32_t node, int32_t which,
                         int32_t* out_parent_ids, double* out_bl) {
  if (n < 3 || !parent_ids || !bl || !out_parent_ids || !out_bl) return fail("mi_nni_neighbour: bad arguments");
  const int root = 2 * n - 3;
  if (node < n || node >= root)
    return fail("mi_nni_neighbour: node " + std::to_string(node) + " is not the lower end of an inner edge");
  if (which != 0 && which != 1) return fail("mi_nni_neighbour: which must be 0 or 1");
  // children in child order (ascending largest leaf id); ids are a post-order, so one upward
  // pass gives the largest leaf ids
  std::vector<int32_t> par(parent_ids, parent_ids + root), maxleaf(root + 1, -1);
  std::vector<std::vector<int32_t>> kids(root + 1);
  for (int v = 0; v < root; v++) {
    if (par[v] <= v || par[v] > root || par[v] < n) return fail(status_message(kBadParentIds));
    kids[par[v]].push_back(v);
  }
  for (int v = 0; v <= root; v++) {
    if (v < n) maxleaf[v] = v;
    else if (kids[v].size() != (v == root ? 3u : 2u))
      return fail(status_message(v == root ? kNotTrifurcatingRoot : kNotBifurcating));
    if (v < root) maxleaf[par[v]] = std::max(maxleaf[par[v]], maxleaf[v]);
  }
  auto by_maxleaf = [&](int32_t x, int32_t y) { return maxleaf[x] < maxleaf[y]; };
  for (int v = n; v <= root; v++) std::sort(kids[v].begin(), kids[v].end(), by_maxleaf);
  // the exchange: `moved` (b for neighbour 0, a for neighbour 1) and c swap parents
  const int u = par[node];
  const int32_t moved = kids[node][which == 0 ? 1 : 0];
  const int32_t c = kids[u][0] != node ? kids[u][0] : kids[u][1];
  std::replace(kids[node].begin(), kids[node].end(), moved, c);
  std::replace(kids[u].begin(), kids[u].end(), c, moved);
  // renumber: leaves keep their ids, internal nodes in post-order with the children ordered
  // by largest leaf id (node.cpp:32-59); largest leaf ids change on the path from u to the root
  std::fill(maxleaf.begin() + n, maxleaf.end(), -1);
  std::vector<int32_t> stack{root}, order;  // pre-order, parents first
  while (!stack.empty()) {
    const int32_t v = stack.back();
    stack.pop_back();
    order.push_back(v);
    for (int32_t k : kids[v]) stack.push_back(k);
  }
  for (size_t i = order.size(); i-- > 0;)
    for (int32_t k : kids[order[i]]) maxleaf[order[i]] = std::max(maxleaf[order[i]], maxleaf[k]);
  for (int v = n; v <= root; v++) std::sort(kids[v].begin(), kids[v].end(), by_maxleaf);
  std::vector<int32_t> new_id(root + 1, -1);
  int32_t next = n;
  // (node << 2 | children already pushed)
  std::vector<int64_t> walk{(int64_t)root << 2};
  while (!walk.empty()) {
    const int64_t item = walk.back();
    const int32_t v = (int32_t)(item >> 2);
    const size_t done = (size_t)(item & 3);
    if (v < n) {
      new_id[v] = v;
      walk.pop_back();
    } else if (done < kids[v].size()) {
      walk.back() = item + 1;
      walk.push_back((int64_t)kids[v][done] << 2);
    } else {
      new_id[v] = next++;
      walk.pop_back();
    }
  }
  out_bl[root] = bl[root];
  for (int v = n; v <= root; v++)
    for (int32_t k : kids[v]) {
      out_parent_ids[new_id[k]] = new_id[v];
      out_bl[new_id[k]] = bl[k];
    }
  return 0;
}

}  // extern "C"
