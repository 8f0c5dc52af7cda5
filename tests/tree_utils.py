"""Synthetic inputs for parity tests: random topologies numbered exactly as the
reference numbers them (leaves keep ids, internal nodes in post-order with
children ordered by max leaf id -- node.cpp:32-59,341-357)."""
import numpy as np


def _polish(tree, n):
    """tree: nested tuples / ints. Returns parent-id vector (root excluded)."""
    parent = {}
    next_id = [n]

    def maxleaf(t):
        return t if isinstance(t, int) else max(maxleaf(c) for c in t)

    def visit(t):
        if isinstance(t, int):
            return t
        kids = sorted(t, key=maxleaf)
        ids = [visit(c) for c in kids]
        me = next_id[0]
        next_id[0] += 1
        for c in ids:
            parent[c] = me
        return me

    root = visit(tree)
    return np.array([parent[v] for v in range(root)], dtype=np.int32)


def random_topology(n, rng, rooted=False):
    """Uniform random-join topology on n leaves; unrooted = trifurcation at the root."""
    parts = list(range(n))
    target = 1 if rooted else 3
    while len(parts) > target:
        i, j = sorted(rng.choice(len(parts), size=2, replace=False))
        b = parts.pop(j)
        a = parts.pop(i)
        parts.append((a, b))
    tree = tuple(parts) if not rooted else parts[0]
    return _polish(tree, n)


def ladder_topology(n, rooted=False):
    t = 0
    if rooted:
        # (n-1, (n-2, ... (1, 0))) as _polish numbers it, written out: the nesting is too deep
        # for its recursion from about 330 taxa on.  Leaves 0 and 1 hang under node n, leaf
        # i >= 2 and internal node n + i - 2 under node n + i - 1.
        pid = np.empty(2 * n - 2, dtype=np.int32)
        pid[:2] = n
        pid[2:n] = n + np.arange(1, n - 1)
        pid[n:] = n + np.arange(1, n - 1)
        return pid
    for i in range(1, n - 2):
        t = (i, t)
    return _polish((t, n - 2, n - 1), n)


def balanced_topology(n, rooted=False):
    """Most balanced tree on n leaves (pairs joined level by level): the worst case for
    the number of simultaneously live partial-likelihood vectors of a post-order walk."""
    parts = list(range(n))
    target = 1 if rooted else 3
    while len(parts) > target:
        nxt = [(parts[i], parts[i + 1]) for i in range(0, len(parts) - 1, 2)]
        if len(parts) % 2:
            nxt.append(parts[-1])
        if len(nxt) < target:  # unrooted: stop at the trifurcation
            nxt = [parts[0], parts[1]] + ([tuple(parts[2:])] if len(parts) > 3 else parts[2:])
        parts = nxt
    tree = tuple(parts) if not rooted else parts[0]
    return _polish(tree, n)


def random_trees(n, T, rng, rooted=False, mean_bl=0.1):
    nodes = 2 * n - 1 if rooted else 2 * n - 2
    pids = np.stack([random_topology(n, rng, rooted) for _ in range(T)])
    bls = rng.exponential(mean_bl, size=(T, nodes))
    bls[:, -1] = 0.0
    return pids, bls


def random_alignment(n, P, rng, gap_fraction=0.05):
    """Random tip states 0..3 with some gaps (code 4); integer-valued weights."""
    tips = rng.integers(0, 4, size=(n, P)).astype(np.int32)
    tips[rng.random((n, P)) < gap_fraction] = 4
    weights = rng.integers(1, 6, size=P).astype(np.float64)
    return tips, weights


def random_gtr_params(T, rng):
    rates = rng.dirichlet(10 * np.ones(6), size=T)
    freqs = rng.dirichlet(10 * np.ones(4), size=T)
    return rates, freqs


def clocklike_rooted_tree(n, rng, topology=None, isochronous=False):
    """Rooted topology + tip dates + branch lengths consistent with node heights.
    topology: a rooted parent-id vector (ladder_topology(n, rooted=True), ...) instead of a
    random one.  isochronous: every tip date 0 -- all bounds are then equal and every epoch
    term of the ratio transform takes its bound[v] == bound[c] branch.  With both left out the
    draws from rng are what they have always been (the seeded inputs of other tests, and the
    input hashes of golden/call_paths.json, rest on that)."""
    pid = random_topology(n, rng, rooted=True) if topology is None else \
        np.asarray(topology, dtype=np.int32)
    N = 2 * n - 1
    assert pid.shape == (N - 1,)
    if isochronous:
        dates = np.zeros(n)
    else:
        dates = np.round(rng.uniform(0, 3, size=n), 3)
        dates[rng.integers(n)] = 0.0
    h = np.zeros(N)
    h[:n] = dates
    kids = {}
    for v, p in enumerate(pid):
        kids.setdefault(int(p), []).append(v)
    for v in range(n, N):
        h[v] = max(h[c] for c in kids[v]) + rng.uniform(0.05, 1.0)
    bl = np.zeros(N)
    for v, p in enumerate(pid):
        bl[v] = h[p] - h[v]
    return pid, bl, dates


def heights_from_ratios(n, parent_ids, bounds, ratios):
    """Node heights of a time tree from its height ratios (ratios[n-2] is the root height),
    top-down: a parent has a larger id than its children, so descending ids do it."""
    N = 2 * n - 1
    h = np.zeros(N)
    h[:n] = bounds[:n]
    h[N - 1] = ratios[n - 2]
    for v in range(N - 2, n - 1, -1):
        h[v] = bounds[v] + ratios[v - n] * (h[parent_ids[v]] - bounds[v])
    return h


def branch_lengths_from_heights(parent_ids, h):
    """bl[v] = h[parent[v]] - h[v]; the root's entry is 0."""
    bl = np.zeros(len(h))
    bl[:-1] = h[np.asarray(parent_ids)] - h[:-1]
    return bl


def rooted_batch(n, T, rng, topologies=None, isochronous=None):
    """T clock-like rooted trees as the rooted calls take them: the stacked
    parent ids, branch lengths, node heights, node bounds, height ratios.
    topologies / isochronous: one entry per tree (None: random topology / random dates)."""
    import oracle_lib as O
    cols = [[] for _ in range(5)]
    for t in range(T):
        pid, bl, dates = clocklike_rooted_tree(
            n, rng, None if topologies is None else topologies[t],
            bool(isochronous is not None and isochronous[t]))
        for col, x in zip(cols, (pid, bl) + tuple(O.time_tree_init(n, pid, bl, dates))):
            col.append(x)
    return tuple(np.stack(c) for c in cols)
