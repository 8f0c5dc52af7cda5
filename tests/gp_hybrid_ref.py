"""Quartet hybrid marginals of generalized pruning, restated by TREE ENUMERATION.

No DAG vector is walked here.  For a central entry e = (t,c) -> s and one summand (g, sigma, rho, o)
of its request (rootward, sister, rotated, sorted), per pattern

    l_p = sum_{trees T of the DAG that contain g, sigma, e, rho and o}
              [ q(T) / (q_g q_sigma q_e q_rho q_o) ] L_p(T)

with q(T) the product over all entries of T, its rootsplit included, and L_p(T) plain single-tree
pruning (gp_ref.tree_likelihood).  Then

    summand   = log(inv[g] q_sigma q_rho q_o) + sum_p w_p (log l_p - log Pr(u))
    hybrid[e] = logsumexp of e's summands, g outermost, then sigma, rho, o innermost

with Pr = gp_ref.node_probabilities, inv = gp_ref.inverted_probabilities and u the parent node of g.
An entry whose request is not fully formed has -inf.
"""
import numpy as np

import gp_ref as R

# the project's own designed batch of 11 taxa: one entry has all four lists longer than one
ELEVEN = ["(((((0,(1,2)),(3,(4,5))),(6,(7,8))),9),10);",
          "(((((1,(0,2)),(4,(3,5))),(7,(6,8))),10),9);",
          "(((((2,(0,1)),(5,(3,4))),(8,(6,7))),9),10);"]
ELEVEN_WIDE_ENTRY = "00000011100|11111100000|00011100000"   # lists 2 / 3 / 3 / 3


def parent_ids_of_newick(text):
    """a rooted bifurcating Newick string over integer taxon names 0..n-1, no branch lengths: the
    parent-id form (children before parents, root last)"""
    pos, leaves = [0], []

    def parse():
        if text[pos[0]] == "(":
            pos[0] += 1
            kids = [parse()]
            while text[pos[0]] == ",":
                pos[0] += 1
                kids.append(parse())
            assert text[pos[0]] == ")" and len(kids) == 2
            pos[0] += 1
            return kids
        start = pos[0]
        while text[pos[0]].isdigit():
            pos[0] += 1
        leaves.append(int(text[start:pos[0]]))
        return leaves[-1]

    tree = parse()
    n = len(leaves)
    assert sorted(leaves) == list(range(n))
    pid, counter = {}, [n]

    def number(node):
        if not isinstance(node, list):
            return node
        kids = [number(k) for k in node]
        me = counter[0]
        counter[0] += 1
        for k in kids:
            pid[k] = me
        return me

    number(tree)
    return np.array([pid[v] for v in range(2 * n - 2)], np.int32)


def eleven_batch():
    return np.stack([parent_ids_of_newick(t) for t in ELEVEN])


class ExactModel(R.Model):
    """P(0) is the identity exactly (as the library's I + V diag(expm1(lambda b)) V^-1 is), so that
    a likelihood that is zero is zero here too"""

    def transition(self, b, order=0, dtype=np.float64):
        if order == 0 and b == 0:
            return np.eye(4, dtype=dtype)
        return super().transition(b, order, dtype)


class Requests:
    """per entry: lists [G] of (rootward, sister, rotated, sorted) entry lists, formed [G],
    first_summand [G], summand_count [G]; summands [S][4] in summand order"""


def requests(d):
    out = Requests()
    into = {}
    for i in range(d.R, d.G):
        into.setdefault(int(d.entries[i][2]), []).append(i)   # (ascending; rootsplit entries left out)
    out.lists, out.formed = [], np.zeros(d.G, bool)
    out.first_summand, out.summand_count = np.zeros(d.G, np.int32), np.zeros(d.G, np.int32)
    summands = []
    for e in range(d.G):
        if e < d.R:
            out.lists.append(([], [], [], []))
            continue
        t, c, s = (int(x) for x in d.entries[e])
        block = lambda v, k: list(range(*d.block_range[v, k])) if v >= d.n else []  # noqa: E731
        four = (into.get(t, []), block(t, 1 - c), block(s, 1), block(s, 0))
        out.lists.append(four)
        if all(four):
            out.formed[e] = True
            out.first_summand[e] = len(summands)
            summands += [(g, a, r, o) for g in four[0] for a in four[1] for r in four[2] for o in four[3]]
            out.summand_count[e] = len(summands) - out.first_summand[e]
    out.summands = np.array(summands, np.int32).reshape(-1, 4)
    return out


def logsumexp_in_order(x):
    x = np.asarray(x, float)
    top = np.max(x)
    if top == -np.inf:
        return -np.inf
    total = 0.0
    for v in x:
        total += np.exp(v - top)
    return float(top + np.log(total))


class Hybrid:
    """hybrid [G], summands [S], trees_per_summand [S], requests"""


def hybrid(d, q, b, tips, weights, model, log_domain=False):
    """the restatement; log_domain: every tree scored in the log domain (deep trees)"""
    q, b, w = np.asarray(q, float), np.asarray(b, float), np.asarray(weights, float)
    req = requests(d)
    trees = R.enumerate_trees(d)
    tipv = R.tip_vectors(tips)
    with np.errstate(divide="ignore"):
        logL = np.stack([R.tree_likelihood(d, t, b, tipv, model, log_domain=True) if log_domain
                         else np.log(R.tree_likelihood(d, t, b, tipv, model)) for t in trees])   # [T][P]
    member = np.zeros((d.G, len(trees)), bool)
    for k, t in enumerate(trees):
        member[list(t), k] = True
    logq = np.log(q)
    log_q_tree = np.array([np.sum(logq[list(t)]) for t in trees])
    node, inv = R.node_probabilities(d, q), R.inverted_probabilities(d, q)
    out = Hybrid()
    out.requests = req
    out.summands = np.full(len(req.summands), -np.inf)
    out.trees_per_summand = np.zeros(len(req.summands), int)
    out.hybrid = np.full(d.G, -np.inf)
    on = w > 0
    for e in np.flatnonzero(req.formed):
        first, count = req.first_summand[e], req.summand_count[e]
        for k in range(first, first + count):
            g, a, r, o = req.summands[k]
            five = [g, a, e, r, o]
            through = np.flatnonzero(np.all(member[five], axis=0))
            out.trees_per_summand[k] = len(through)
            terms = (log_q_tree[through] - np.sum(logq[five]))[:, None] + logL[through]   # [trees][P]
            top = np.max(terms, axis=0)
            with np.errstate(divide="ignore", invalid="ignore"):
                log_l = np.where(top == -np.inf, -np.inf,
                                 top + np.log(np.sum(np.exp(terms - np.where(top == -np.inf, 0.0, top)), axis=0)))
                u = int(d.entries[g][0])
                per_pattern = np.where(on, w * (log_l - np.log(node[u])), 0.0)
                out.summands[k] = np.log(inv[g] * q[a] * q[r] * q[o]) + np.sum(per_pattern)
        out.hybrid[e] = logsumexp_in_order(out.summands[first:first + count])
    return out


def sbn_estimate_rule(d, q, per_gpcsp, hybrid_values):
    """the reference's UpdateSBNProbabilities with hybrid marginals: per block softmax(hybrid + log q)
    if every entry of the block has a finite hybrid marginal, else softmax(per-entry + log q); the
    rootsplits always the second form; a block of one entry gets 1.  Also returns the blocks that
    took the hybrid values, as (begin, end)."""
    q, new, took = np.asarray(q, float), np.array(q, float), []

    def block(lo, hi, may):
        if hi - lo == 1:
            new[lo] = 1.0
            return
        use = may and bool(np.all(np.isfinite(hybrid_values[lo:hi])))
        x = (hybrid_values if use else per_gpcsp)[lo:hi] + np.log(q[lo:hi])
        new[lo:hi] = np.exp(x - logsumexp_in_order(x))
        if use:
            took.append((int(lo), int(hi)))

    block(0, d.R, False)
    for v in range(d.n, d.node_count):
        for c in range(2):
            block(*d.block_range[v, c], True)
    return new, took
