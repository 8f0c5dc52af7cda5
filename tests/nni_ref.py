"""Reference for the NNI neighbourhood scan, straight from the public definition
(include/mi_phylo.h) and independent of the library: the neighbour trees rebuilt as nested
subtrees and renumbered the way the reference numbers trees (tree_utils._polish's rule: leaves
keep their ids, internal nodes in post-order, children ordered by largest leaf id), every
branch length carried along with its subtree; split sets for comparing topologies."""
import sys

import numpy as np

sys.setrecursionlimit(max(sys.getrecursionlimit(), 5000))


class _Sub:
    """A subtree with the branch above it."""
    __slots__ = ("leaf", "kids", "length", "maxleaf")

    def __init__(self, leaf, kids, length):
        self.leaf, self.kids, self.length = leaf, kids, length
        self.maxleaf = leaf if kids is None else max(k.maxleaf for k in kids)


def children(n, pid):
    """Children of every node of the caller's tree in child order (ascending largest leaf id)."""
    root = 2 * n - 3
    kids = {v: [] for v in range(n, root + 1)}
    for v in range(root):
        kids[int(pid[v])].append(v)
    maxleaf = list(range(n)) + [0] * (root + 1 - n)
    for v in range(n, root + 1):  # ids are a post-order
        maxleaf[v] = max(maxleaf[c] for c in kids[v])
        kids[v].sort(key=lambda c: maxleaf[c])
    return kids


def inner_edges(n):
    """Lower ends of the inner edges: every internal node but the root."""
    return range(n, 2 * n - 3)


def neighbour(n, pid, bl, v, which):
    """(parent ids [2n-3], branch lengths [2n-2]) of neighbour `which` of inner edge v."""
    root = 2 * n - 3
    pid = np.asarray(pid)
    bl = np.asarray(bl, dtype=np.float64)
    assert n <= v < root and which in (0, 1)
    kids = children(n, pid)
    a, b = kids[v]
    u = int(pid[v])
    c = [x for x in kids[u] if x != v][0]
    keep, moved = (a, b) if which == 0 else (b, a)

    def build(x):
        if x < n:
            return _Sub(x, None, bl[x])
        if x == v:  # v keeps one child and takes c
            return _Sub(None, [build(keep), build(c)], bl[v])
        if x == u:  # the other child takes c's place
            return _Sub(None, [build(moved if k == c else k) for k in kids[u]], bl[u])
        return _Sub(None, [build(k) for k in kids[x]], bl[x])

    tree = build(root)
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

    assert visit(tree) == root
    return out_pid, out_bl


def all_neighbours(n, pid, bl):
    """Every (v, i) in code order 2 v + i with its rebuilt tree: [(v, i, pid', bl')]."""
    return [(v, i) + neighbour(n, pid, bl, v, i) for v in inner_edges(n) for i in (0, 1)]


def splits(n, pid):
    """The non-trivial splits of an unrooted tree, each as the frozenset of the side without leaf 0."""
    root = 2 * n - 3
    below = [frozenset([v]) if v < n else frozenset() for v in range(root + 1)]
    for v in range(root):
        below[int(pid[v])] = below[int(pid[v])] | below[v]
    everything = frozenset(range(n))
    out = set()
    for v in range(n, root):
        side = below[v] if 0 not in below[v] else everything - below[v]
        out.add(side)
    return out


def best_move(n, delta):
    """2 v + i of the largest delta over the inner edges, the lowest code among equals (-1: none)."""
    if n <= 3:
        return -1
    codes = np.arange(2 * n, 2 * (2 * n - 3))
    flat = np.asarray(delta).reshape(-1)[codes]
    return int(codes[int(np.argmax(flat))])
