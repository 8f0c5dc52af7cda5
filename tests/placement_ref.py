"""A plain reference for the placement call (TEST INFRASTRUCTURE ONLY; numpy only): DESIGN.md 4.17
for one unrooted 4-state tree, in np.longdouble.

Deliberately not the kernels' algorithm.  `insertion_tables` and `explicit_ll` have no pre-order
pass and no table of the kernels' kind: per (edge, pendant length) the tree on n+1 taxa is built
explicitly -- a new node halves the edge, the query hangs from it -- and pruned from its root.
`explicit_ll` does so for one query row, column by column; `insertion_tables` prunes that same
tree once for each of the five things a query column can show (A, C, G, T, gap), which is what
explicit_ll computes for a column of that pattern and state, so that summing its entries over a
query's columns (`score`) is explicit insertion for every query at once.  `formula_tables` is the
table form of the definitions (post-order and pre-order vectors, M, Z, S); the CPU tests hold it
to explicit insertion, the GPU tests use it where a tree is too large to insert into edge by
edge.  Transition matrices are dense_ref.expm's (Taylor series, no eigensystem)."""
from types import SimpleNamespace

import numpy as np

from dense_ref import LD, expm, gtr_q, tip_vectors  # noqa: F401  (gtr_q, tip_vectors: for the callers)

REL = 1e-10  # the project's standing tolerance
# the float64-against-longdouble disagreement of this reference on the GPU tests' inputs must stay
# below this (tests/test_placement_ref.py measures it)
FLOAT64_CAP = 1e-12
EXCLUDED = 0.01  # at most this share of a case's best_edge / pendant_index entries may be left out

QUERY_VECTORS = np.concatenate([np.eye(4), np.ones((1, 4))])  # what a query column shows: A C G T gap


def _tree(parent_ids):
    pid = np.asarray(parent_ids, int)
    root = len(pid)
    n = (root + 3) // 2
    assert np.all(pid > np.arange(root)) and np.all(pid <= root)
    kids = [[] for _ in range(root + 1)]
    for v, p in enumerate(pid):
        kids[p].append(v)
    assert all(len(kids[v]) == (3 if v == root else 2) for v in range(n, root + 1))
    return pid, root, n, kids


def _mats(Q, r, t, memo=None):
    """[K][4][4] transition matrices of one length; memo: those already formed, by length."""
    if memo is None:
        return np.stack([expm(Q * (rk * t)) for rk in r])
    if t not in memo:
        memo[t] = _mats(Q, r, t)
    return memo[t]


def _apply(Pm, L):
    """P L per category: Pm [K][4][4], L [..., K or 1, P, 4] -> [..., K, P, 4]."""
    return np.matmul(Pm[:, None], L[..., None])[..., 0]


def _prune(kids, root, length, tipvec, Q, pi, r, c, memo=None):
    """Pattern likelihoods of a tree given as child lists: length[v] of the edge above v, tipvec[v]
    [..., 1, P, 4] of a leaf (leading axes broadcast).  Returns [..., P]."""
    def vector(v):
        if not kids[v]:
            return tipvec[v]
        out = None
        for u in kids[v]:
            m = _apply(_mats(Q, r, length[u], memo), vector(u))
            out = m if out is None else out * m
        return out
    return np.einsum("k,...kpi,i->...p", c, vector(root), pi)


def _inserted(kids, root, t, e, pendant):
    """Child lists and lengths of the tree with the query (node root + 1) on the midpoint of edge
    e (the new internal node: root + 2)."""
    q, m = root + 1, root + 2
    k2 = [list(x) for x in kids] + [[], [e, q]]
    for x in k2[:root + 1]:
        if e in x:
            x[x.index(e)] = m
    length = dict(enumerate(t[:root]))
    length[e] = t[e] / 2
    length[m] = t[e] / 2
    length[q] = pendant
    return k2, length


def _setup(parent_ids, lengths, Q, pi, cat_rates, cat_weights, tips, dtype):
    pid, root, n, kids = _tree(parent_ids)
    t = np.asarray(lengths, dtype)
    tips = np.asarray(tips, dtype)
    assert tips.shape[0] == n and tips.shape[2] == 4
    return SimpleNamespace(pid=pid, root=root, n=n, kids=kids, t=t, Q=np.asarray(Q, dtype), pi=np.asarray(pi, dtype),
                           r=np.asarray(cat_rates, dtype), c=np.asarray(cat_weights, dtype), tips=tips,
                           P=tips.shape[1], dtype=dtype)


def pattern_lik(parent_ids, lengths, Q, pi, cat_rates, cat_weights, tips, dtype=LD):
    """[P] pattern likelihoods of the tree itself."""
    x = _setup(parent_ids, lengths, Q, pi, cat_rates, cat_weights, tips, dtype)
    tipvec = {v: x.tips[v][None] for v in range(x.n)}
    return _prune(x.kids, x.root, dict(enumerate(x.t[:x.root])), tipvec, x.Q, x.pi, x.r, x.c)


def insertion_tables(parent_ids, lengths, Q, pi, cat_rates, cat_weights, tips, pendants, dtype=LD):
    """[E][G][5][P]: the log pattern likelihood of the (n+1)-taxon tree with the query on edge e
    by pendant length g showing code a at (a column of) pattern p.  Also returns [E][G][5][P] raw
    likelihoods (for sum_a Z = L_p)."""
    x = _setup(parent_ids, lengths, Q, pi, cat_rates, cat_weights, tips, dtype)
    tipvec = {v: x.tips[v][None, None] for v in range(x.n)}  # [1][1][P][4]
    tipvec[x.root + 1] = np.broadcast_to(QUERY_VECTORS.astype(dtype)[:, None, None, :], (5, 1, x.P, 4))
    E, G = x.root, len(pendants)
    lik = np.empty((E, G, 5, x.P), dtype)
    memo = {}
    for e in range(E):
        for g, l in enumerate(pendants):
            kids, length = _inserted(x.kids, x.root, x.t, e, dtype(l))
            lik[e, g] = _prune(kids, x.root, length, tipvec, x.Q, x.pi, x.r, x.c, memo)
    with np.errstate(divide="ignore"):
        return np.log(lik), lik


def explicit_ll(parent_ids, lengths, Q, pi, cat_rates, cat_weights, tips, query, column_pattern, column_weights,
                edge, pendant, dtype=LD):
    """One (query, edge, pendant length): the weighted log-likelihood of the (n+1)-taxon alignment
    over the query's columns -- column c carries the tips of pattern column_pattern[c] and the
    query's state -- on the explicitly built tree.  Columns of weight 0 are left out."""
    x = _setup(parent_ids, lengths, Q, pi, cat_rates, cat_weights, tips, dtype)
    col = np.asarray(column_pattern, int)
    w = np.asarray(column_weights, dtype)
    tipvec = {v: x.tips[v][col][None] for v in range(x.n)}
    tipvec[x.root + 1] = QUERY_VECTORS.astype(dtype)[np.minimum(np.asarray(query, int) & 0xFF, 4)][None]
    kids, length = _inserted(x.kids, x.root, x.t, edge, dtype(pendant))
    lik = _prune(kids, x.root, length, tipvec, x.Q, x.pi, x.r, x.c)
    keep = w != 0
    with np.errstate(divide="ignore"):
        return np.sum(w[keep] * np.log(lik[keep]))


def formula_tables(parent_ids, lengths, Q, pi, cat_rates, cat_weights, tips, pendants, dtype=LD):
    """The table form of the definitions: S [E][G][5][P], Z [E][G][4][P], s [P]."""
    x = _setup(parent_ids, lengths, Q, pi, cat_rates, cat_weights, tips, dtype)
    root, n, K = x.root, x.n, len(x.r)
    Pm = [_mats(x.Q, x.r, x.t[v]) for v in range(root)]
    L, msg = [None] * (root + 1), [None] * root
    for v in range(root + 1):  # post-order: L [K][P][4]
        L[v] = np.broadcast_to(x.tips[v], (K,) + x.tips[v].shape) if v < n else \
            np.prod([msg[u] for u in x.kids[v]], axis=0)
        if v < root:
            msg[v] = _apply(Pm[v], L[v])
    lik = np.einsum("k,kpi,i->p", x.c, L[root], x.pi)
    s = np.log(lik)
    top = [None] * root  # pre-order: the vector at the top of the edge above v (it carries pi)
    for v in range(root - 1, -1, -1):
        a = x.pid[v]
        others = np.prod([msg[u] for u in x.kids[a] if u != v], axis=0)
        above = x.pi[None, None, :] if a == root else _apply(np.swapaxes(Pm[a], 1, 2), top[a])
        top[v] = above * others
    E, G = root, len(pendants)
    Z = np.empty((E, G, 4, x.P), dtype)
    for e in range(E):
        H = _mats(x.Q, x.r, x.t[e] / 2)
        M = _apply(np.swapaxes(H, 1, 2), top[e]) * _apply(H, L[e])  # [K][P][4]
        for g, l in enumerate(pendants):
            R = _mats(x.Q, x.r, dtype(l))
            Z[e, g] = np.einsum("k,kpj,kja->ap", x.c, M, R)
    S = np.empty((E, G, 5, x.P), dtype)
    with np.errstate(divide="ignore"):
        S[:, :, :4] = s + np.log(Z / np.sum(Z, axis=2, keepdims=True))
    S[:, :, 4] = s
    return S, Z, s


def score(S, queries, column_pattern, column_weights):
    """ll [Q][E][G] = sum_c w_c S[e][g][x[q][c]][pattern(c)], columns of weight 0 skipped."""
    x = np.asarray(queries).astype(int)
    code = np.where((x >= 0) & (x <= 3), x, 4)
    col = np.asarray(column_pattern, int)
    w = np.asarray(column_weights, S.dtype)
    keep = np.nonzero(w != 0)[0]
    out = np.empty((len(code),) + S.shape[:2], S.dtype)
    for q in range(len(code)):
        out[q] = np.sum(w[keep] * S[:, :, code[q, keep], col[keep]], axis=-1)
    return out


def summarise(ll):
    """From ll [Q][E][G]: edge_ll, pendant_index, the gap between the two best pendant lengths
    (inf for G = 1), best_edge, the gap between the two best edges, lwr."""
    edge_ll = np.max(ll, axis=2)
    pend = np.argmax(ll, axis=2).astype(np.int8)
    if ll.shape[2] > 1:
        top = np.sort(ll, axis=2)
        pend_gap = top[..., -1] - top[..., -2]
    else:
        pend_gap = np.full(edge_ll.shape, np.inf)
    best = np.argmax(edge_ll, axis=1).astype(np.int32)
    top = np.sort(edge_ll, axis=1)
    edge_gap = top[:, -1] - top[:, -2]
    z = np.exp(edge_ll - np.max(edge_ll, axis=1, keepdims=True))
    return SimpleNamespace(edge_ll=edge_ll, pendant_index=pend, pendant_gap=pend_gap, best_edge=best,
                           edge_gap=edge_gap, lwr=z / np.sum(z, axis=1, keepdims=True))


def star3_closed_form(t, pendant, tip_states, code):
    """JC69, one category, the 3-taxon star, one pattern: S for a query on edge 0 showing `code`,
    by hand.  With p(x) = 1/4 + 3/4 e^(-4x/3), q(x) = 1/4 - 1/4 e^(-4x/3): the centre is summed
    out of the three tips and the midpoint of edge 0, the midpoint out of tip 0, the centre and the
    query.  Returns (S, s)."""
    t = np.asarray(t, LD)

    def pr(x, same):
        e = np.exp(-LD(4) * x / 3)
        return LD(1) / 4 + LD(3) / 4 * e if same else LD(1) / 4 - LD(1) / 4 * e

    a0, a1, a2 = tip_states
    lik = sum(LD(1) / 4 * pr(t[0], u == a0) * pr(t[1], u == a1) * pr(t[2], u == a2) for u in range(4))
    s = np.log(lik)
    if code > 3:
        return s, s
    Z = np.zeros(4, LD)
    for a in range(4):
        for m in range(4):  # midpoint state
            below = pr(t[0] / 2, m == a0) * pr(LD(pendant), m == a)
            Z[a] += sum(LD(1) / 4 * pr(t[0] / 2, u == m) * pr(t[1], u == a1) * pr(t[2], u == a2)
                        for u in range(4)) * below
    return s + np.log(Z[code] / Z.sum()), s
