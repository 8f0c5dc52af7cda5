"""A plain reference for the ancestral-state call (TEST INFRASTRUCTURE ONLY; numpy only): the
joints, posteriors and map states of DESIGN.md 4.13 for one unrooted 4-state tree, in
np.longdouble.

Deliberately not the kernel's algorithm: there is no pre-order pass.  J[v][p][s], the joint of
"node v is in state s" and the data of pattern p, is the pattern likelihood with L_v replaced by
L_v o e_s, pruned again from v up to the root (the `replaced` of dense_ref.branch_derivatives);
the category terms come from the root vector per category.  Transition matrices are
dense_ref.expm's (Taylor series, no eigensystem)."""
from types import SimpleNamespace

import numpy as np

from dense_ref import LD, expm, gtr_q, tip_vectors  # noqa: F401  (gtr_q, tip_vectors: for the callers)

# How a GPU result is held against this reference: entries of at least SMALL to
# REL relative, the project's standing figure; entries below it to ABS_FLOOR absolute, 16 times
# the largest disagreement on such entries between this file evaluated in float64 and in
# longdouble over the GPU tests' inputs (tests/test_ancestral_ref.py measures it again and holds
# the constant to it: 6.65e-21 measured); rows sum to 1 within ROW_SUM; map states are compared
# where the reference's two largest posteriors are more than MAP_MARGIN apart, and at most
# MAP_EXCLUDED of a case's (node, pattern) entries may be left out that way.
REL = 1e-10
SMALL = 1e-6
ABS_FLOOR = 1.1e-19
ABS_FLOOR_CAP = 1e-12
ROW_SUM = 8 * 2.0 ** -53
MAP_MARGIN = 1e-9
MAP_EXCLUDED = 0.01


def cat_row_sum(K):
    """Bound on |sum_k cat_post - 1|: K correctly rounded quotients of one sum of K terms."""
    return max(8, 2 * K) * 2.0 ** -53


def ancestral(parent_ids, lengths, Q, pi, cat_rates, cat_weights, tips, dtype=LD, with_tips=True):
    """One unrooted tree: parent ids [2n-3] (root = node 2n-3, a parent's id above its
    children's), lengths [2n-2] (the root's entry is not read), Q [4][4], pi [4], category rates
    and weights [K], tip vectors [n][P][4] (gaps, 0/1 masks or real values).

    Returns, everything in `dtype` and unweighted: joint [n-2][P][4] = J of the internal nodes
    n .. 2n-3 (row v - n), state_post (its rows normalised), map_state [n-2][P] (argmax, lowest
    among equals), margin [n-2][P] (largest minus second-largest posterior), lik [P] the pattern
    likelihood, cat_joint / cat_post [P][K], pattern_rate [P] and, with_tips, tip_joint /
    tip_post [n][P][4] = the same joint at the leaves."""
    pid = np.asarray(parent_ids, int)
    root = len(pid)
    n = (root + 3) // 2
    t = np.asarray(lengths, dtype)
    Q, pi = np.asarray(Q, dtype), np.asarray(pi, dtype)
    r, c = np.asarray(cat_rates, dtype), np.asarray(cat_weights, dtype)
    tips = np.asarray(tips, dtype)
    assert tips.shape[0] == n and tips.shape[2] == 4
    assert np.all(pid > np.arange(root)) and np.all(pid <= root)
    K, P = len(r), tips.shape[1]
    kids = [[] for _ in range(root + 1)]
    for v, p in enumerate(pid):
        kids[p].append(v)
    assert all(len(kids[v]) == (3 if v == root else 2) for v in range(n, root + 1))
    Pm = np.stack([np.stack([expm(Q * (r[k] * t[v])) for k in range(K)]) for v in range(root)])

    # post-order: L[v][k][p][i] and the message of v to its parent, P_v L_v
    L = [None] * (root + 1)
    msg = [None] * root
    for v in range(root + 1):
        if v < n:
            L[v] = np.broadcast_to(tips[v], (K,) + tips[v].shape)
        else:
            L[v] = np.prod([msg[u] for u in kids[v]], axis=0)
        if v < root:
            msg[v] = np.einsum("kij,kpj->kpi", Pm[v], L[v])
    eye = np.eye(4, dtype=dtype)

    def joint(v):
        """[P][4]: per state s, the pattern likelihood with L_v replaced by L_v o e_s."""
        x = L[v][None] * eye[:, None, None, :]  # [s][k][p][i]
        while v != root:
            m = np.einsum("kij,skpj->skpi", Pm[v], x)
            a = pid[v]
            x = m * np.prod([msg[u] for u in kids[a] if u != v], axis=0)[None]
            v = a
        return np.einsum("k,skpi,i->ps", c, x, pi)

    def normalise(j):
        with np.errstate(invalid="ignore", divide="ignore"):
            return j / np.sum(j, axis=-1, keepdims=True)

    out = SimpleNamespace()
    out.joint = np.stack([joint(v) for v in range(n, root + 1)])
    out.state_post = normalise(out.joint)
    out.map_state = np.argmax(np.nan_to_num(out.state_post, nan=0.0), axis=-1).astype(np.int8)
    top = np.sort(out.state_post, axis=-1)
    out.margin = top[..., 3] - top[..., 2]
    out.cat_joint = c[None, :] * np.einsum("kpi,i->pk", L[root], pi)
    out.lik = np.sum(out.cat_joint, axis=1)
    out.cat_post = normalise(out.cat_joint)
    out.pattern_rate = out.cat_post @ r
    if with_tips:
        out.tip_joint = np.stack([joint(v) for v in range(n)])
        out.tip_post = normalise(out.tip_joint)
    return out


def brute_force(parent_ids, lengths, Q, pi, cat_rates, cat_weights, tips, dtype=LD):
    """joint [n-2][P][4] and cat_joint [P][K] of a SMALL tree by enumerating every assignment of
    states to the internal nodes (4^(n-2) of them): no pruning at all."""
    import itertools
    pid = np.asarray(parent_ids, int)
    root = len(pid)
    n = (root + 3) // 2
    t = np.asarray(lengths, dtype)
    Q, pi = np.asarray(Q, dtype), np.asarray(pi, dtype)
    r, c = np.asarray(cat_rates, dtype), np.asarray(cat_weights, dtype)
    tips = np.asarray(tips, dtype)
    K, P = len(r), tips.shape[1]
    joint = np.zeros((n - 2, P, 4), dtype)
    cat_joint = np.zeros((P, K), dtype)
    for k in range(K):
        Pm = [expm(Q * (r[k] * t[v])) for v in range(root)]
        for states in itertools.product(range(4), repeat=n - 2):
            x = dict(zip(range(n, root + 1), states))
            val = np.full(P, pi[x[root]], dtype)
            for v in range(root):
                row = Pm[v][x[pid[v]]]
                val = val * (tips[v] @ row if v < n else row[x[v]])
            cat_joint[:, k] += c[k] * val
            for v in range(n, root + 1):
                joint[v - n, :, x[v]] += c[k] * val
    return joint, cat_joint


def errors(got, want):
    """(largest relative error on the entries of `want` of at least SMALL, largest absolute error
    on the others) of a float64 array against a reference array; a NaN in either gives NaN."""
    got, want = np.asarray(got, LD), np.asarray(want, LD)
    assert got.shape == want.shape, (got.shape, want.shape)
    big = want >= SMALL
    diff = np.abs(got - want)
    rel = np.max(diff[big] / want[big]) if np.any(big) else LD(0)
    low = np.max(diff[~big]) if np.any(~big) else LD(0)
    return float(rel), float(low)


def check(got, want, label=""):
    """Holds a float64 result to the reference: REL on the large entries, ABS_FLOOR on the small."""
    rel, low = errors(got, want)
    assert rel <= REL and low <= ABS_FLOOR, (label, rel, low)
    return rel, low


def check_rows(post, bound, label=""):
    """Rows of posteriors sum to 1 within `bound` (summed in longdouble)."""
    worst = float(np.max(np.abs(np.sum(np.asarray(post, LD), axis=-1) - 1)))
    assert worst <= bound, (label, worst)
    return worst


def check_map(got, ref, label=""):
    """Map states against the reference's where its two largest posteriors are MAP_MARGIN apart;
    returns the share of entries left out (at most MAP_EXCLUDED)."""
    clear = ref.margin > MAP_MARGIN
    excluded = 1.0 - float(np.mean(clear))
    assert excluded <= MAP_EXCLUDED, (label, excluded)
    assert np.array_equal(np.asarray(got)[clear], ref.map_state[clear]), label
    return excluded
