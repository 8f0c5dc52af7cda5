"""Trees of the subsplit DAG, restated in numpy on top of gp_ref.py independently of the library
(DESIGN.md 4.27): the index of a rooted tree by frozensets, log q by math.fsum, the rooted
TrainSimpleAverage by dicts, the sampler with the Philox of sbn_vi_ref.py, unranking in the order
of gp_ref.enumerate_trees, the numbering rule of built trees, and de-rooting.
"""
import bisect
import math
import sys

import numpy as np

import gp_ref as GR
import sbn_vi_ref as V

sys.setrecursionlimit(max(sys.getrecursionlimit(), 10000))


# ---------------------------------------------------------------- the index
def tree_index(d, pid):
    """(entries [2n-1], nodes [2n-1]) of one rooted tree: per tree node the DAG node (-1: not in
    the DAG) and the entry into it (the root: its rootsplit entry); the sentinel is d.G."""
    n, kids, taxa = GR._tree_nodes(pid)
    N = 2 * n - 1
    node_of = {key: i for i, key in enumerate(d.clades) if i >= d.n}
    roots = {int(d.entries[i][2]): i for i in range(d.R)}
    nodes, clade_of = np.full(N, -1, np.int32), {}
    nodes[:n] = np.arange(n)
    for v in range(n, N):
        a, b = kids[v]
        if min(taxa[b]) < min(taxa[a]):
            a, b = b, a
        nodes[v] = node_of.get((taxa[a], taxa[b]), -1)
        clade_of[a], clade_of[b] = 0, 1
    entries = np.full(N, d.G, np.int32)
    for v in range(N - 1):
        p = int(pid[v])
        if nodes[p] >= 0 and nodes[v] >= 0:
            entries[v] = d.index.get((int(nodes[p]), clade_of[v], int(nodes[v])), d.G)
    if nodes[N - 1] >= 0:
        entries[N - 1] = roots.get(int(nodes[N - 1]), d.G)
    return entries, nodes


def index_batch(d, pids):
    out = [tree_index(d, pid) for pid in np.atleast_2d(pids)]
    return np.stack([e for e, _ in out]), np.stack([v for _, v in out])


def log_q(d, q, entries):
    """sum of log q over the entries; -inf at a sentinel or a zero parameter"""
    terms = []
    for e in entries:
        if e < 0 or e >= d.G or q[e] == 0.0:
            return -math.inf
        terms.append(math.log(q[e]))
    return math.fsum(terms)


def branch_lengths(d, b, entries, missing):
    out = [b[e] if 0 <= e < d.G else missing for e in entries]
    out[-1] = 0.0
    return np.array(out)


def blocks(d):
    """(begin, end) of the rootsplits and of every (node, clade), in the order of the entries"""
    out = [(0, d.R)]
    for v in range(d.n, d.node_count):
        for c in range(2):
            out.append(tuple(int(x) for x in d.block_range[v, c]))
    return out


def simple_average(d, entries, weights=None):
    """the rooted TrainSimpleAverage: {entry: sum of the weights of the trees that use it},
    normalised over the rootsplits and per block; a block whose total is 0 gets zeros"""
    entries = np.atleast_2d(entries)
    weights = np.ones(len(entries)) if weights is None else np.asarray(weights, float)
    count = {}
    for t, row in enumerate(entries):
        for e in row:
            if not 0 <= e < d.G:
                raise ValueError(f"tree {t} is not in the DAG")
            count[int(e)] = count.get(int(e), 0.0) + weights[t]
    q = np.zeros(d.G)
    for lo, hi in blocks(d):
        total = math.fsum(count.get(i, 0.0) for i in range(lo, hi))
        for i in range(lo, hi):
            q[i] = count.get(i, 0.0) / total if total else 0.0
    return q


# ---------------------------------------------------------------- building trees
def number_tree(n, root_entry, tree):
    """The numbering rule of built trees.  tree: a taxon, or ((entry, subtree), (entry, subtree)).
    Leaves by taxon, internal nodes in post-order, children ordered by largest leaf id, root 2n-2:
    (parent_ids [2n-2], entries [2n-1])."""
    pid, ent, counter = np.full(2 * n - 2, -1, np.int32), np.full(2 * n - 1, -1, np.int32), [n]

    def largest(t):
        return t if isinstance(t, int) else max(largest(t[0][1]), largest(t[1][1]))

    def visit(t):
        if isinstance(t, int):
            return t
        kids = sorted(t, key=lambda k: largest(k[1]))
        ids = [visit(k[1]) for k in kids]
        me = counter[0]
        counter[0] += 1
        for (e, _), i in zip(kids, ids):
            pid[i], ent[i] = me, e
        return me

    root = visit(tree)
    assert root == 2 * n - 2
    ent[root] = root_entry
    return pid, ent


def cdf(d, q):
    """per block and over the rootsplits: cdf[j] = sum_{i <= j} q_i, ascending, one accumulator"""
    out = np.zeros(d.G)
    for lo, hi in blocks(d):
        total = 0.0
        for i in range(lo, hi):
            total = total + float(q[i])
            out[i] = total
    return out


def _draw(cdf_values, b, e, u):
    total = cdf_values[e - 1]
    if not total > 0.0:
        raise ValueError(f"empty block [{b}, {e})")
    j = bisect.bisect_right(cdf_values, u * total, b, e)
    return j if j < e else bisect.bisect_left(cdf_values, total, b, e)


def sample_tree(d, cdf_values, seed, t):
    """sample t: (parent_ids, entries) by the numbering rule.  Draw 0 picks the rootsplit; at a node
    clade 0's block is drawn, its child's subtree descended, then clade 1's block."""
    cdf_values = [float(x) for x in cdf_values]
    draws = [0]

    def pick(lo, hi):
        j = _draw(cdf_values, lo, hi, V.uniform(seed, t, draws[0]))
        draws[0] += 1
        return j

    def below(v):
        if v < d.n:
            return v
        sides = []
        for c in range(2):
            e = pick(*(int(x) for x in d.block_range[v, c]))
            sides.append((e, below(int(d.entries[e][2]))))
        return tuple(sides)

    r = pick(0, d.R)
    return number_tree(d.n, r, below(int(d.entries[r][2])))


def unrank(d, r):
    """tree number r of the DAG in the order of gp_ref.enumerate_trees, as a tuple of entries
    (its rootsplit entry first), by integer counts: clade 0 the slow digit, clade 1 the fast one"""
    count = {v: 1 for v in range(d.n)}
    for v in sorted(range(d.n, d.node_count), key=lambda v: (d.levels[v], v)):
        count[v] = 1
        for c in range(2):
            count[v] *= sum(count[int(d.entries[i][2])] for i in range(*d.block_range[v, c]))

    def in_block(lo, hi, r):
        for i in range(lo, hi):
            c = count[int(d.entries[i][2])]
            if r < c:
                return i, r
            r -= c
        raise IndexError("rank beyond the topology count")

    def below(v, r):
        if v < d.n:
            return v
        base = sum(count[int(d.entries[i][2])] for i in range(*d.block_range[v, 1]))
        sides = []
        for c, rc in ((0, r // base), (1, r % base)):
            e, rest = in_block(int(d.block_range[v, c][0]), int(d.block_range[v, c][1]), rc)
            sides.append((e, below(int(d.entries[e][2]), rest)))
        return tuple(sides)

    e, rest = in_block(0, d.R, r)
    return e, below(int(d.entries[e][2]), rest)


def flatten(root_entry, tree):
    """the entries of a built tree in the order of gp_ref.enumerate_trees"""
    if isinstance(tree, int):
        return (root_entry,)
    (e0, t0), (e1, t1) = tree
    return (root_entry,) + flatten(e0, t0) + flatten(e1, t1)


def enumerate_numbered(d, first=0, count=None):
    """(parent_ids [count][2n-2], entries [count][2n-1]) of trees first .. first + count - 1"""
    total = int(round(d.topology_count))
    count = total - first if count is None else count
    out = [number_tree(d.n, *unrank(d, r)) for r in range(first, first + count)]
    return np.stack([p for p, _ in out]), np.stack([e for _, e in out])


# ---------------------------------------------------------------- de-rooting
def deroot(pid, bl=None):
    """Node::Deroot of one rooted tree (parent ids [2n-2], root 2n-2): (parent ids [2n-3],
    lengths [2n-2] or None, root edge), renumbered in the unrooted convention."""
    n, kids, taxa = GR._tree_nodes(pid)
    root = 2 * n - 2
    a, b = kids[root]
    x, y = (a, b) if n - 1 in taxa[a] else (b, a)
    if x < n:
        x, y = y, x
    out, lengths, counter = np.full(2 * n - 3, -1, np.int32), np.zeros(2 * n - 2), [n]

    def visit(v):
        if v < n:
            return v
        below = list(kids[v]) + ([y] if v == x else [])
        below.sort(key=lambda k: max(taxa[k]))
        ids = [visit(k) for k in below]
        me = counter[0]
        counter[0] += 1
        for k, i in zip(below, ids):
            out[i] = me
            if bl is not None:
                lengths[i] = bl[k] + (bl[x] if k == y else 0.0)
        if v == x:
            visit.edge = ids[below.index(y)]
        return me

    assert visit(x) == 2 * n - 3
    return out, (lengths if bl is not None else None), visit.edge


def nni_neighbours(pid):
    """the rooted NNI neighbours of one rooted tree (parent-id form, children before parents): for
    every internal non-root node v, either child of v swapped with v's sibling"""
    pid = np.asarray(pid)
    n = len(pid) // 2 + 1
    out = []
    for v in range(n, 2 * n - 2):
        p = int(pid[v])
        sib = next(u for u in range(2 * n - 2) if pid[u] == p and u != v)
        for c in [u for u in range(2 * n - 2) if pid[u] == v]:
            kids = {}
            for u, w in enumerate(pid):
                kids.setdefault(int(w), []).append(u)
            kids[v][kids[v].index(c)] = sib
            kids[p][kids[p].index(sib)] = c
            new, res, counter = {}, np.zeros(2 * n - 2, np.int32), [n]

            def walk(u):
                if u < n:
                    return u
                ids = [walk(k) for k in kids[u]]
                me = counter[0]
                counter[0] += 1
                for i in ids:
                    res[i] = me
                return me

            walk(2 * n - 2)
            out.append(res)
    return np.stack(out)
