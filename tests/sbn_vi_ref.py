"""Sampling from a subsplit Bayesian network and the gradient of the variational objective in
plain Python, on top of tests/sbn_ref.py: Philox4x32-10, the descent table from
the clade sets (not from slots), the sampler over a GIVEN CDF with the de-rooting rule and
tree_utils._polish's numbering, the gradient of log q by enumerating rootings with math.fsum (the
reference's GradientOfLogQ, src/unrooted_sbn_instance.cpp:128-174) and the plain and VIMCO factors
(src/generic_sbn_instance.hpp:398-431)."""
import bisect
import math
import sys

import sbn_ref as R

NEG_INF = float("-inf")
M32 = 0xFFFFFFFF
sys.setrecursionlimit(max(sys.getrecursionlimit(), 10000))  # (the sampler recurses once per level of a tree)


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al. 2011): counter [4], key [2] of 32-bit words -> [4] words."""
    c0, c1, c2, c3 = (int(x) & M32 for x in counter)
    k0, k1 = (int(x) & M32 for x in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return [c0, c1, c2, c3]


def uniform(seed, t, i):
    """u in [0, 1) of draw i of sample t: key (seed lo, seed hi), counter (i, 0, t lo, t hi)."""
    seed, t = int(seed) & (2 ** 64 - 1), int(t) & (2 ** 64 - 1)
    w = philox4x32_10([i, 0, t & M32, t >> 32], [seed & M32, seed >> 32])
    return float(((w[0] << 32) | w[1]) >> 11) * 2.0 ** -53


def descent_table(support):
    """[P][2] of a sbn_ref.Support, from the clade sets: >= 0 a block (index into parent_range),
    < 0 the leaf ~value.  Raises KeyError if a subsplit a parameter leads to is not a parent of
    the support (the support is closed: it never is)."""
    n, S = support.n, support.S
    everything = frozenset(range(n))
    block_of = {}
    for f, b in zip(support.pcsps, support.pcsp_parent):
        block_of[f[:2]] = b

    def entry(sister, focal):
        if len(focal) == 1:
            return ~min(focal)
        return block_of[(sister, focal)]

    out = []
    for s in support.rootsplits:
        out.append([entry(everything - s, s), entry(s, everything - s)])
    for sister, focal, child in support.pcsps:
        other = focal - child
        out.append([entry(other, child), entry(child, other)])
    return out


def cdf(phi, blocks):
    """cdf[j] = sum_{i <= j in block} exp(phi_i - m), m the block's maximum; fsum per entry."""
    out = [0.0] * len(phi)
    for b, e in blocks:
        m = max(phi[b:e])
        terms = [0.0 if m == NEG_INF or x == NEG_INF else math.exp(x - m) for x in phi[b:e]]
        for j in range(b, e):
            out[j] = math.fsum(terms[:j - b + 1])
    return out


def _draw(cdf_values, b, e, u):
    """The smallest j of [b, e) with cdf[j] > u cdf[e-1]; if x rounded up to the total, the
    smallest j that reaches the total.  (Bisection: the CDF is non-decreasing within a block.)"""
    total = cdf_values[e - 1]
    if not total > 0.0:
        raise ValueError("empty block")
    j = bisect.bisect_right(cdf_values, u * total, b, e)
    return j if j < e else bisect.bisect_left(cdf_values, total, b, e)


def polish(tree, n):
    """tree_utils._polish with the ids of the top-level children: (parent ids, [their ids]).
    (The largest leaf of every subtree is found once, not once per ancestor.)"""
    parent, next_id, largest = {}, [n], {}

    def maxleaf(t):
        if isinstance(t, int):
            return t
        if id(t) not in largest:
            largest[id(t)] = max(maxleaf(c) for c in t)
        return largest[id(t)]

    def visit(t):
        if isinstance(t, int):
            return t, []
        kids = sorted(t, key=maxleaf)
        ids = [visit(c)[0] for c in kids]
        me = next_id[0]
        next_id[0] += 1
        for c in ids:
            parent[c] = me
        return me, list(zip(kids, ids))

    root, top = visit(tree)
    return [parent[v] for v in range(root)], top


def sample(n, S, parent_range, descent, cdf_values, seed, t):
    """Sample t: (parent ids [2n-3], root edge, sampled parameters [n-1]).  Draw 0 is the
    rootsplit; entry 0's subtree before entry 1's; every block visit takes one draw."""
    chosen = []

    def visit(b, e):
        j = _draw(cdf_values, b, e, uniform(seed, t, len(chosen)))
        chosen.append(j)
        kids = []
        for entry in descent[j]:
            kids.append(~entry if entry < 0 else visit(*parent_range[entry]))
        return tuple(kids)

    a, b = visit(0, S)

    def largest(tree):
        return tree if isinstance(tree, int) else max(largest(c) for c in tree)

    x, y = (a, b) if largest(a) == n - 1 else (b, a)
    if isinstance(x, int):
        x, y = y, x
    pid, top = polish((x[0], x[1], y), n)
    edge = [i for kid, i in top if (kid == y if isinstance(y, int) else kid is y)]
    return pid, edge[0], chosen


def log_prob_of_sample(phi, blocks, chosen):
    """sum over the sampled parameters of log softmax within their block (fsum)."""
    block_of = {}
    for b, e in blocks:
        for j in range(b, e):
            block_of[j] = (b, e)
    return math.fsum(phi[j] - R.logsumexp(phi[slice(*block_of[j])]) for j in chosen)


def grad_log_q(rep, theta, blocks):
    """d log q / d phi [P] of one tree (rep: its [2n-3] index lists) under normalised theta, by
    enumerating the rootings as GradientOfLogQ does: every rooting in the support adds
    rho ([i in rooting] - exp(theta_i)) to every i of the blocks its parameters lie in.  A tree
    with log q = -inf gives zeros."""
    P = len(theta)
    block_of = {}
    for b, e in blocks:
        for j in range(b, e):
            block_of[j] = (b, e)
    lp = R.rooting_log_probs(rep, theta)
    lq = R.logsumexp(lp)
    terms = [[] for _ in range(P)]
    if lq == NEG_INF:
        return [0.0] * P, lq
    for r, x in zip(rep, lp):
        if x == NEG_INF:
            continue
        rho = math.exp(x - lq)
        inside = set(r)
        for j in r:
            for i in range(*block_of[j]):
                terms[i].append(rho * ((1.0 if i in inside else 0.0) - math.exp(theta[i])))
    return [math.fsum(x) for x in terms], lq


def plain_factors(log_f):
    K = len(log_f)
    log_F = R.logsumexp(log_f)
    return [(log_F - math.log(K)) - math.exp(f - log_F) for f in log_f]


def vimco_factors(log_f):
    K = len(log_f)
    total = math.fsum(log_f)
    out = plain_factors(log_f)
    for t in range(K):
        perturbed = list(log_f)
        perturbed[t] = (total - log_f[t]) / (K - 1)
        out[t] -= R.logsumexp(perturbed) - math.log(K)
    return out


def topology_gradient(reps, theta, blocks, factors):
    """sum_t a_t grad log q_t [P] (fsum over the trees), and log q [T]."""
    grads, lqs = zip(*(grad_log_q(rep, theta, blocks) for rep in reps))
    P = len(theta)
    return [math.fsum(a * g[j] for a, g in zip(factors, grads)) for j in range(P)], list(lqs)
