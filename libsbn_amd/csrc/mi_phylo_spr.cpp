// Host side of the SPR neighbourhood scan: the neighbour trees themselves
// (mi_spr_neighbour: what a caller needs to TAKE the move the scan recommends).  Plain host
// arithmetic: no device is touched.
#include <algorithm>

#include "mi_phylo_engine.h"

extern "C" {

int32_t mi_spr_neighbour(int32_t n, const int32_t* parent_ids, const double* bl, int32_t s, int32_t dir, int32_t f,
                         int32_t* out_parent_ids, double* out_bl) {
  if (n < 3 || !parent_ids || !bl || !out_parent_ids || !out_bl) return fail("mi_spr_neighbour: bad arguments");
  const int root = 2 * n - 3;
  std::vector<int32_t> par(parent_ids, parent_ids + root);
  std::vector<std::vector<int32_t>> kids(root + 1);
  for (int v = 0; v < root; v++) {
    if (par[v] <= v || par[v] > root || par[v] < n) return fail(status_message(kBadParentIds));
    kids[par[v]].push_back(v);
  }
  for (int v = n; v <= root; v++)
    if (kids[v].size() != (v == root ? 3u : 2u))
      return fail(status_message(v == root ? kNotTrifurcatingRoot : kNotBifurcating));
  if (s < 0 || s >= root) return fail("mi_spr_neighbour: pruned edge " + std::to_string(s) + " is no edge of the tree");
  if (f < 0 || f >= root) return fail("mi_spr_neighbour: target edge " + std::to_string(f) + " is no edge of the tree");
  if (dir != 0 && dir != 1) return fail("mi_spr_neighbour: dir must be 0 or 1");
  if (dir == 1 && s < n) return fail("mi_spr_neighbour: a leaf edge has no dir = 1 moves");
  // the node that goes (hub), what hangs from the new node, the two neighbours the merged edge joins
  const int hub = dir == 0 ? par[s] : s;
  const int moving = dir == 0 ? s : par[s];
  std::vector<int32_t> joined;
  for (int32_t k : kids[hub])
    if (k != moving) joined.push_back(k);
  if (hub != root && moving != par[hub]) joined.push_back(par[hub]);
  // f inside clade s?
  bool inside = false;
  for (int v = f; v < root; v = par[v])
    if (v == s) {
      inside = true;
      break;
    }
  // (the merged edge goes by the names of the edges it is made of: both carry the hub at one end)
  const bool merged = f == hub || par[f] == hub;
  if (merged || (dir == 0 ? inside : !inside))
    return fail("mi_spr_neighbour: (" + std::to_string(s) + ", " + std::to_string(dir) + ", " + std::to_string(f) +
                ") is no move: the target is " + (merged ? "the merged edge" : "in the moving part"));

  // the neighbour as an undirected graph; node root + 1 is the new attachment node
  const int attach = root + 1;
  struct Link {
    int32_t to;
    double length;
  };
  std::vector<std::vector<Link>> adj(root + 2);
  auto link = [&](int a, int b, double t) {
    adj[a].push_back({b, t});
    adj[b].push_back({a, t});
  };
  for (int v = 0; v < root; v++) {
    if (v == hub || par[v] == hub || v == f) continue;
    link(v, par[v], bl[v]);
  }
  // hub's other two edges become one: below-and-above (t_y + t_u) or two children (t_y1 + t_y2, t_a + t_b)
  auto edge_length = [&](int x) { return hub != root && x == par[hub] ? bl[hub] : bl[x]; };
  link(joined[0], joined[1], edge_length(joined[0]) + edge_length(joined[1]));
  link(f, attach, 0.5 * bl[f]);
  link(attach, par[f], 0.5 * bl[f]);
  link(attach, moving, bl[s]);

  // root it (the caller's root if it survives), children by largest leaf id, internal nodes in post-order
  const int top = hub == root ? attach : root;
  std::vector<int32_t> up(root + 2, -1), order, maxleaf(root + 2, -1);
  std::vector<double> up_length(root + 2, 0.0);
  std::vector<int32_t> stack{top};
  up[top] = top;
  while (!stack.empty()) {
    const int32_t v = stack.back();
    stack.pop_back();
    order.push_back(v);
    for (const Link& l : adj[v])
      if (l.to != up[v]) {
        up[l.to] = v;
        up_length[l.to] = l.length;
        stack.push_back(l.to);
      }
  }
  std::vector<std::vector<int32_t>> sons(root + 2);
  for (size_t i = order.size(); i-- > 0;) {
    const int32_t v = order[i];
    if (v < n) maxleaf[v] = v;
    if (v != top) {
      sons[up[v]].push_back(v);
      maxleaf[up[v]] = std::max(maxleaf[up[v]], maxleaf[v]);
    }
  }
  for (auto& k : sons) std::sort(k.begin(), k.end(), [&](int32_t x, int32_t y) { return maxleaf[x] < maxleaf[y]; });
  std::vector<int32_t> new_id(root + 2, -1);
  int32_t next = n;
  // (node << 2 | children already pushed)
  std::vector<int64_t> walk{(int64_t)top << 2};
  while (!walk.empty()) {
    const int64_t item = walk.back();
    const int32_t v = (int32_t)(item >> 2);
    const size_t done = (size_t)(item & 3);
    if (v < n) {
      new_id[v] = v;
      walk.pop_back();
    } else if (done < sons[v].size()) {
      walk.back() = item + 1;
      walk.push_back((int64_t)sons[v][done] << 2);
    } else {
      new_id[v] = next++;
      walk.pop_back();
    }
  }
  out_bl[root] = bl[root];
  for (int32_t v : order)
    if (v != top) {
      out_parent_ids[new_id[v]] = new_id[up[v]];
      out_bl[new_id[v]] = up_length[v];
    }
  return 0;
}

}  // extern "C"
