"""Split tables of tree batches in plain Python: a split is an int whose bit i is
taxon i, minorised as the reference does (Bitset::Minorize, src/bitset.cpp:147-152: a set that
holds taxon 0 is replaced by its complement); the distinct splits of a batch are numbered by first
occurrence in (tree, edge) order.  Everything the engine's split calls compute, restated with
ints, dicts and math.fsum: the table, its statistics, Robinson-Foulds distances, the squared
branch score and the majority-rule consensus tree."""
import math
from fractions import Fraction

import numpy as np


def taxon_count(pid):
    return (len(pid) + 3) // 2


def edge_splits(pid):
    """[2n-3] minorised split of every edge, as ints."""
    n = taxon_count(pid)
    below = [1 << v if v < n else 0 for v in range(2 * n - 2)]
    for v in range(2 * n - 3):  # a parent's id is above its children's
        below[int(pid[v])] |= below[v]
    everyone = (1 << n) - 1
    return [everyone ^ below[v] if below[v] & 1 else below[v] for v in range(2 * n - 3)]


def split_set(pid):
    """The tree as the set of its splits, each a frozenset of leaves (never leaf 0)."""
    n = taxon_count(pid)
    return {frozenset(i for i in range(n) if s >> i & 1) for s in edge_splits(pid)}


def table(pids):
    """(index [T][2n-1] int32, splits [S] ints, first [S], trees [S]) of parent ids [T][2n-3]."""
    pids = np.asarray(pids)
    T, E = pids.shape
    number, splits, first, trees = {}, [], [], []
    index = np.full((T, E + 2), -1, np.int32)
    for t in range(T):
        for v, s in enumerate(edge_splits(pids[t])):
            if s not in number:
                number[s] = len(splits)
                splits.append(s)
                first.append(t * (E + 2) + v)
                trees.append(0)
            index[t, v] = number[s]
            trees[number[s]] += 1
    return index, splits, np.array(first, np.int32), np.array(trees, np.int32)


def words(splits, n):
    """[S][W] uint32 stored form of int splits."""
    W = (n + 31) // 32
    return np.array([[(s >> (32 * k)) & 0xFFFFFFFF for k in range(W)] for s in splits], np.uint32).reshape(len(splits), W)


def strings(splits, n):
    return ["".join("1" if s >> i & 1 else "0" for i in range(n)) for s in splits]


def stats(index, S, bls=None, weights=None, ordered=False):
    """[S][3] sum w, sum w l, sum w l^2 over the trees that hold a split: math.fsum of the rounded
    products, or (ordered) one accumulator in ascending tree order."""
    T, N = index.shape
    cols = [[[] for _ in range(3)] for _ in range(S)]
    for t in range(T):
        w = 1.0 if weights is None else float(weights[t])
        for v in range(N - 2):
            l = 0.0 if bls is None else float(bls[t][v])
            c = cols[index[t, v]]
            c[0].append(w)
            c[1].append(w * l if bls is not None else 0.0)
            c[2].append(w * (l * l) if bls is not None else 0.0)
    out = np.zeros((S, 3))
    for k in range(S):
        for j in range(3):
            if ordered:
                acc = 0.0
                for x in cols[k][j]:
                    acc += x
                out[k, j] = acc
            else:
                out[k, j] = math.fsum(cols[k][j])
    return out


def rf(index, n):
    """[T][T] Robinson-Foulds distances over the nontrivial splits (index >= n)."""
    sets = [{int(k) for k in row[:-2] if k >= n} for row in index]
    return np.array([[len(a ^ b) for b in sets] for a in sets], np.int32)


def branch_score(index, bls, ordered=False):
    """[T][T] squared Kuhner-Felsenstein branch scores: exactly rounded (integer arithmetic on the
    lengths scaled by their common power-of-two denominator), or (ordered) one accumulator over
    the ascending split indices of either tree."""
    T = index.shape[0]
    maps = [{int(k): float(bls[t][v]) for v, k in enumerate(index[t][:-2]) if k >= 0} for t in range(T)]
    den = max([Fraction(l).denominator for m in maps for l in m.values()] + [1])
    scaled = [{k: int(Fraction(l) * den) for k, l in m.items()} for m in maps]
    out = np.zeros((T, T))
    for a in range(T):
        for b in range(a, T):
            keys = sorted(set(maps[a]) | set(maps[b]))
            if ordered:
                acc = 0.0
                for k in keys:
                    d = maps[a].get(k, 0.0) - maps[b].get(k, 0.0)
                    acc += d * d
                out[a, b] = out[b, a] = acc
            else:
                total = sum((scaled[a].get(k, 0) - scaled[b].get(k, 0)) ** 2 for k in keys)
                out[a, b] = out[b, a] = float(Fraction(total, den * den))
    return out


def popcount(s):
    return bin(s).count("1")


def consensus(n, splits, weight, total, threshold):
    """(parent ids [m-1], node split [m]) of the majority-rule consensus: the nontrivial splits
    with weight > threshold * total, as a tree in the reference's convention."""
    assert 0.5 <= threshold < 1
    leaf_split = [-1] * n
    kept = []
    for i, s in enumerate(splits):
        c = popcount(s)
        if c == n - 1:
            leaf_split[0] = i
        elif c == 1:
            leaf_split[s.bit_length() - 1] = i
        elif weight[i] > threshold * total:
            kept.append(i)
    kept.sort(key=lambda i: popcount(splits[i]))
    parent_set = {}
    for x, i in enumerate(kept):
        parent_set[i] = next((j for j in kept[x + 1:] if splits[i] & ~splits[j] == 0), None)
    kids = {None: [0]}
    for i in kept:
        kids.setdefault(parent_set[i], []).append(("set", i))
        kids.setdefault(i, [])
    for v in range(1, n):
        kids[next((i for i in kept if splits[i] >> v & 1), None)].append(v)

    def maxleaf(c):
        return c if isinstance(c, int) else splits[c[1]].bit_length() - 1

    parent, node_split, next_id = {}, {}, [n]

    def visit(c):
        if isinstance(c, int):
            node_split[c] = leaf_split[c]
            return c
        ids = [visit(k) for k in sorted(kids[c[1]], key=maxleaf)]
        me = next_id[0]
        next_id[0] += 1
        node_split[me] = -1 if c[1] is None else c[1]
        for k in ids:
            parent[k] = me
        return me

    root = visit(("set", None))
    return (np.array([parent[v] for v in range(root)], np.int32),
            np.array([node_split[v] for v in range(root + 1)], np.int32))


def reroot(pid, bl, new_root):
    """The same unrooted tree with its trifurcation at internal node `new_root`, renumbered in
    the reference's convention: (parent ids [2n-3], branch lengths [2n-2])."""
    n = taxon_count(pid)
    root = 2 * n - 3
    adj = {v: [] for v in range(root + 1)}
    for v in range(root):
        adj[v].append((int(pid[v]), float(bl[v])))
        adj[int(pid[v])].append((v, float(bl[v])))
    assert n <= new_root <= root
    parent, length, next_id = {}, {}, [n]

    def build(v, up):
        kids = [(build(k, v), l) for k, l in adj[v] if k != up]
        if not kids:
            return (v, v, None)  # (largest leaf id, node, children)
        kids.sort(key=lambda c: c[0][0])
        return (max(c[0][0] for c in kids), v, kids)

    def number(t):
        if t[2] is None:
            return t[1]
        ids = [(number(c), l) for c, l in t[2]]
        me = next_id[0]
        next_id[0] += 1
        for k, l in ids:
            parent[k], length[k] = me, l
        return me

    top = number(build(new_root, None))
    assert top == root
    return (np.array([parent[v] for v in range(root)], np.int32),
            np.array([length[v] for v in range(root)] + [0.0]))


def random_batch(n, T, rng, dyadic=False):
    """T trees of n taxa in which splits are shared: random trees, a duplicate, and the same
    topology under another rooting.  Lengths are multiples of 2^-10 when dyadic."""
    import tree_utils as TU
    pids, bls = TU.random_trees(n, T, rng)
    if dyadic:
        bls = np.round(bls * 1024 + 1) / 1024
        bls[:, -1] = 0.0
    if T >= 3:
        pids[T - 1] = pids[0]
    if T >= 2 and n >= 4:
        pids[1], bls[1] = reroot(pids[0], bls[0], int(rng.integers(n, 2 * n - 3)))
    return pids, bls
