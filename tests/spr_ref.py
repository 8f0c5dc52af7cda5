"""Reference for the SPR neighbourhood scan, straight from the public definition
(include/mi_phylo.h) and independent of the library: which (s, dir, f) are moves and at what
distance, the neighbour trees rebuilt as nested subtrees and renumbered the way the reference
numbers trees (tree_utils._polish's rule: leaves keep their ids, internal nodes in post-order,
children ordered by largest leaf id), every branch length carried along with its edge; split sets
with their lengths for comparing trees; a plain pruning log-likelihood for tip vectors the oracle
does not take; and the rescaling exponents a post-order pass stores, for showing that a case
exercises them."""
import functools
import sys

import numpy as np

from dense_ref import LD, expm

sys.setrecursionlimit(max(sys.getrecursionlimit(), 5000))

REL = 1e-10  # the project's standing tolerance
# the oracle's float64 build against its longdouble build on the GPU tests' inputs must stay below
# this, relative to |logL| (tests/test_spr_ref.py measures it)
FLOAT64_CAP = 1e-12


class _Sub:
    """A subtree with the branch above it."""
    __slots__ = ("leaf", "kids", "length", "maxleaf")

    def __init__(self, leaf, kids, length):
        self.leaf, self.kids, self.length = leaf, kids, length
        self.maxleaf = leaf if kids is None else max(k.maxleaf for k in kids)


def tree(n, pid):
    """(parent [2n-3] as ints, children of every internal node, the leaf set below every node)."""
    return _tree(n, tuple(int(p) for p in pid))


@functools.lru_cache(maxsize=64)
def _tree(n, pid):
    root = 2 * n - 3
    par = list(pid)
    assert len(par) == root and all(max(v, n - 1) < par[v] <= root for v in range(root))
    kids = {v: [] for v in range(n, root + 1)}
    below = [frozenset([v]) if v < n else frozenset() for v in range(root + 1)]
    for v in range(root):  # ids are a post-order
        kids[par[v]].append(v)
        below[par[v]] = below[par[v]] | below[v]
    assert all(len(kids[v]) == (3 if v == root else 2) for v in kids)
    return par + [-1], kids, below  # (the root's parent: none)


def _prune(n, pid, s, d):
    """The pruned tree of (s, d) as an undirected graph on the caller's node ids, None if (s, d)
    prunes nothing: (adjacency {node: set of nodes}, the two ends of the merged edge, the node
    that went, the neighbour of it that the moving part hangs from)."""
    root = 2 * n - 3
    par, kids, _ = tree(n, pid)
    if d == 1 and s < n:
        return None
    hub = par[s] if d == 0 else s
    moving = s if d == 0 else par[s]
    adj = {v: set() for v in range(root + 1)}
    for v in range(root):
        adj[v].add(par[v])
        adj[par[v]].add(v)
    ends = sorted(adj[hub] - {moving})
    assert len(ends) == 2
    # what moves leaves the graph with the node that went
    gone, stack = {hub}, [moving]
    while stack:
        v = stack.pop()
        gone.add(v)
        stack.extend(x for x in adj[v] if x not in gone)
    rest = {v: {x for x in adj[v] if x not in gone} for v in adj if v not in gone}
    rest[ends[0]].add(ends[1])
    rest[ends[1]].add(ends[0])
    return rest, ends, hub, moving


def targets(n, pid, s, d):
    """{f: distance} of the valid targets of (s, d), by the definition's two rules: which edges
    (sets of edge names) and how far (nodes on the path from the merged edge)."""
    root = 2 * n - 3
    par, kids, below = tree(n, pid)
    if d == 1 and s < n:
        return {}
    inside = {v for v in range(root) if below[v] <= below[s]}  # s and the edges of clade s
    if d == 0:
        u = par[s]
        merged = {x for x in kids[u] if x != s} | ({u} if u != root else set())
        valid = set(range(root)) - inside - merged
    else:
        valid = inside - {s} - set(kids[s])
    rest, ends, _, _ = _prune(n, pid, s, d)
    dist, seen, frontier = {}, set(ends), [(ends[0], 1), (ends[1], 1)]
    while frontier:
        x, k = frontier.pop()
        for y in rest[x]:
            if y in seen:
                continue
            seen.add(y)
            dist[y if par[y] == x else x] = k  # the edge's name: its lower end
            frontier.append((y, k + 1))
    assert set(dist) == valid, (s, d, sorted(dist), sorted(valid))
    return dist


def moves(n, pid, radius=0):
    """Every move (s, d, f, distance) within the radius (0: all), in code order (2 s + d) E + f."""
    out = []
    for s in range(2 * n - 3):
        for d in (0, 1):
            reach = targets(n, pid, s, d)
            out += [(s, d, f, reach[f]) for f in sorted(reach) if radius == 0 or reach[f] <= radius]
    return out


def neighbour(n, pid, bl, s, d, f, known_move=False):
    """(parent ids [2n-3], branch lengths [2n-2]) of the tree the move (s, d, f) leads to.
    known_move: (s, d, f) came out of moves() or targets(); it is not looked up again."""
    root = 2 * n - 3
    bl = np.asarray(bl, dtype=np.float64)
    par, kids, _ = tree(n, pid)
    assert known_move or f in targets(n, pid, s, d), (s, d, f)
    rest, ends, hub, moving = _prune(n, pid, s, d)

    def length(x, y):  # of the edge between neighbours x and y of the caller's tree
        return bl[x] if par[x] == y else bl[y]

    new = root + 1  # the attachment node
    links = {}  # {node: {neighbour: length}}

    def link(x, y, t):
        links.setdefault(x, {})[y] = t
        links.setdefault(y, {})[x] = t

    for x in rest:
        for y in rest[x]:
            if x < y and {x, y} != set(ends) and {x, y} != {f, par[f]}:
                link(x, y, length(x, y))
    link(ends[0], ends[1], length(ends[0], hub) + length(ends[1], hub))
    link(f, new, 0.5 * bl[f])
    link(new, par[f], 0.5 * bl[f])
    # the moving part, untouched, on the branch of the cut edge
    adj = {v: set() for v in range(root + 1)}
    for v in range(root):
        adj[v].add(par[v])
        adj[par[v]].add(v)
    seen, stack = {hub, moving}, [moving]
    while stack:
        x = stack.pop()
        for y in adj[x]:
            if y not in seen:
                seen.add(y)
                link(x, y, length(x, y))
                stack.append(y)
    link(new, moving, bl[s])

    def build(x, above, t):
        if x < n:
            return _Sub(x, None, t)
        return _Sub(None, [build(y, x, links[x][y]) for y in links[x] if y != above], t)

    top = root if hub != root else new
    nested = build(top, None, bl[root])
    out_pid = np.full(root, -1, np.int32)
    out_bl = np.zeros(root + 1)
    next_id = [n]

    def visit(t):
        if t.kids is None:
            me = t.leaf
        else:
            ids = [visit(k) for k in sorted(t.kids, key=lambda k: k.maxleaf)]
            me = next_id[0]
            next_id[0] += 1
            for k in ids:
                out_pid[k] = me
        out_bl[me] = t.length
        return me

    assert visit(nested) == root
    return out_pid, out_bl


def splits(n, pid, bl):
    """{split: length} over all 2n-3 edges, a split as the frozenset of the side without leaf 0."""
    _, _, below = tree(n, pid)
    everything = frozenset(range(n))
    out = {}
    for v in range(2 * n - 3):
        side = below[v] if 0 not in below[v] else everything - below[v]
        assert side not in out
        out[side] = float(bl[v])
    return out


# ---- likelihoods by plain pruning (tip vectors of any kind) ----

def pattern_lik(pid, bl, Q, pi, cat_rates, cat_weights, tips, dtype=LD, memo=None):
    """[P] pattern likelihoods of an unrooted tree: tips [n][P][4]; memo: matrices by length."""
    pid = np.asarray(pid, int)
    root = len(pid)
    n = (root + 3) // 2
    Q, pi = np.asarray(Q, dtype), np.asarray(pi, dtype)
    r, c = np.asarray(cat_rates, dtype), np.asarray(cat_weights, dtype)
    t = np.asarray(bl, dtype)
    memo = {} if memo is None else memo
    vec = [np.broadcast_to(np.asarray(tips[v], dtype), (len(r),) + np.shape(tips[v])) for v in range(n)]
    vec += [None] * (root + 1 - n)
    for v in range(root):
        key = float(t[v])
        if key not in memo:
            memo[key] = np.stack([expm(Q * (rk * t[v])) for rk in r])
        m = np.matmul(memo[key][:, None], vec[v][..., None])[..., 0]  # [K][P][4]
        vec[pid[v]] = m if vec[pid[v]] is None else vec[pid[v]] * m
    return np.einsum("k,kpi,i->p", c, vec[root], pi)


def log_likelihood(pid, bl, Q, pi, cat_rates, cat_weights, tips, weights, dtype=LD, memo=None):
    w = np.asarray(weights, dtype)
    keep = w != 0
    lik = pattern_lik(pid, bl, Q, pi, cat_rates, cat_weights, tips, dtype, memo)
    return np.sum(w[keep] * np.log(lik[keep]))


# ---- the exponents a rescaling post-order pass stores ----

def down_exponents(pid, bl, Q, cat_rates, tips):
    """[2n-2][P] int: the cumulative power of two a post-order pass with rescaling has taken out
    of the vector of every node but the root (0 at the leaves): each internal node's vectors are
    divided by 2^ilogb(largest entry over the categories) and the exponents add up the tree."""
    pid = np.asarray(pid, int)
    root = len(pid)
    n = (root + 3) // 2
    r = np.asarray(cat_rates, np.float64)
    Q = np.asarray(Q, np.float64)
    P = np.shape(tips)[1]
    vec = [np.broadcast_to(np.asarray(tips[v], np.float64), (len(r), P, 4)) for v in range(n)] + [None] * (root - n)
    cum = np.zeros((root, P), int)
    kids = [[] for _ in range(root + 1)]
    for v in range(root):
        kids[pid[v]].append(v)
    for v in range(n, root):
        prod = 1.0
        for k in kids[v]:
            Pm = np.stack([expm(Q * (rk * float(bl[k]))) for rk in r])
            prod = prod * np.matmul(Pm[:, None], vec[k][..., None])[..., 0]
            cum[v] += cum[k]
        ex = np.frexp(np.max(prod, axis=(0, 2)))[1] - 1  # ilogb
        vec[v] = np.ldexp(prod, -ex[None, :, None])
        cum[v] += ex
    return cum


# ---- decisions ----

def table(n, E_moves, values):
    """[E][2][E] with -inf where there is no move: values[i] belongs to E_moves[i] = (s, d, f, ...)."""
    E = 2 * n - 3
    out = np.full((E, 2, E), -np.inf)
    for m, x in zip(E_moves, values):
        out[m[0], m[1], m[2]] = x
    return out


def decisions(tab):
    """From a table [E][2][E]: best target [E][2] (-1: none), best delta [E][2], the margin to the
    second-best target [E][2] (inf where there are fewer than two), best move (s, d, f) or
    (-1, -1, -1), its margin to the second-best entry of the whole table."""
    E = tab.shape[0]
    target = np.full((E, 2), -1, np.int32)
    best = np.full((E, 2), -np.inf)
    margin = np.full((E, 2), np.inf)
    for s in range(E):
        for d in (0, 1):
            row = tab[s, d]
            if np.all(np.isneginf(row)):
                continue
            target[s, d] = int(np.argmax(row))
            best[s, d] = row[target[s, d]]
            rest = np.delete(row, target[s, d])
            if np.any(~np.isneginf(rest)):
                margin[s, d] = best[s, d] - np.max(rest)
    flat = tab.reshape(-1)
    if np.all(np.isneginf(flat)):
        return target, best, margin, (-1, -1, -1), np.inf
    code = int(np.argmax(flat))
    rest = np.delete(flat, code)
    move_margin = flat[code] - np.max(rest) if np.any(~np.isneginf(rest)) else np.inf
    return target, best, margin, (code // (2 * E), (code // E) % 2, code % E), move_margin
