"""References for the per-pattern log-likelihoods, the RELL re-summation and the tree-mixture
marginal (TEST INFRASTRUCTURE ONLY; never imports the library).

s[t][p] = log L_p(tree t) comes from the CPU oracle evaluated on ONE-PATTERN alignments of weight
1: a Spec with pattern_count = 1 per column (the way oracle_lib.unrooted_by_pattern_blocks cuts
its blocks).  Every s is below -1 for the alignments the tests draw (a column with a resolved
state costs at least log 4), so the terms are like-signed, nothing cancels and a relative
tolerance is meaningful.  The RELL, ELW and mixture references
are numpy in long double."""
import numpy as np

import oracle_lib as O
import tree_utils as TU

LD = np.longdouble


def site(K):
    return "constant" if K == 1 else f"weibull+{K}"


def params(spec, T, **blocks):
    """[T][param_count] parameter matrix from named blocks (clock rate 1)."""
    pc, lay = O.param_count(spec), O.param_layout(spec)
    pr = np.zeros((T, pc))
    for key, val in blocks.items():
        val = np.asarray(val, float)
        pr[:, lay[key]:lay[key] + val.shape[-1]] = val
    if lay["clock rate"] >= 0:
        pr[:, lay["clock rate"]] = 1.0
    return pr


def model_params(spec, subst, K, T, rng):
    """Per-tree model rows: random GTR rates / frequencies, random Weibull shapes."""
    blocks = {}
    if subst == "GTR":
        gr, gf = TU.random_gtr_params(T, rng)
        blocks.update({"GTR rates": gr, "frequencies": gf})
    if K > 1:
        blocks["Weibull shape"] = rng.uniform(0.4, 1.6, size=(T, 1))
    return params(spec, T, **blocks)


def pattern_log_likelihoods(spec, tips, parent_ids, bl, pr, rescaling=False):
    """s [T][P] from the oracle: column p alone, weight 1."""
    tips = np.asarray(tips, np.int32)
    T, P = len(parent_ids), tips.shape[1]
    sub = O.Spec(spec.taxon_count, 1, spec.state_count, spec.category_count, spec.subst_model,
                 spec.site_model, spec.clock_model, spec.use_tip_states)
    one = np.ones(1)
    s = np.empty((T, P))
    for p in range(P):
        s[:, p] = O.unrooted_log_likelihoods(sub, np.ascontiguousarray(tips[:, p:p + 1]), one,
                                             parent_ids, bl, pr, rescaling, 1)
    return s


def rell(s, w):
    """(C [B][T] long double, best [B], bp [T], elw [T] long double) of s [T][P], W [B][P]."""
    s, w = np.asarray(s, LD), np.asarray(w, LD)
    c = w @ s.T
    return (c,) + reductions(c)


def reductions(c):
    """(best, bp, elw) of a given C [B][T]: first index among equals; elw in long double."""
    c = np.asarray(c)
    B, T = c.shape
    best = np.argmax(c, axis=1)
    bp = np.bincount(best, minlength=T) / B
    cl = c.astype(LD)
    e = np.exp(cl - cl.max(axis=1, keepdims=True))
    elw = (e / e.sum(axis=1, keepdims=True)).sum(axis=0) / B
    return best, bp, elw


def top_two_gap(c):
    """Per replicate, (largest - second largest) / |largest| of C (inf for one tree)."""
    c = np.asarray(c, LD)
    if c.shape[1] < 2:
        return np.full(c.shape[0], np.inf)
    top = np.sort(c, axis=1)[:, -2:]
    return np.asarray((top[:, 1] - top[:, 0]) / np.abs(top[:, 1]), float)


def mixture(s, pattern_weights, tree_log_weights=None):
    """(logsumexp_t(s[t][p] + lw_t) [P], its weighted sum) in long double."""
    s = np.asarray(s, LD)
    T = s.shape[0]
    lw = np.full(T, -np.log(LD(T))) if tree_log_weights is None else np.asarray(tree_log_weights, LD)
    x = s + lw[:, None]
    m = x.max(axis=0)
    per = m + np.log(np.exp(x - m).sum(axis=0))
    return per, (np.asarray(pattern_weights, LD) * per).sum()


def shape(name, rng):
    """The topologies of tests/test_nni_scan_gpu.py's smallest shapes, T = 3 trees each."""
    if name == "n4":
        return 4, np.stack([TU.random_topology(4, rng) for _ in range(3)])
    if name == "n5":
        return 5, np.stack([TU.random_topology(5, rng) for _ in range(3)])
    if name == "balanced8":
        return 8, np.stack([TU.balanced_topology(8)] * 3)
    if name == "ladder9":
        return 9, np.stack([TU.ladder_topology(9)] * 3)
    return 12, np.stack([TU.random_topology(12, rng) for _ in range(3)])


SHAPES = ("n4", "n5", "balanced8", "ladder9", "random12")


def case(name, P, subst, K, seed):
    """(tips, weights, parent ids, branch lengths, spec, parameter rows) of one shape."""
    rng = np.random.default_rng(seed)
    n, pids = shape(name, rng)
    T = len(pids)
    tips, w = TU.random_alignment(n, P, rng)
    bls = rng.uniform(0.01, 0.5, size=(T, 2 * n - 2))
    bls[:, -1] = 0.0
    spec = O.make_spec(n, P, subst, site(K))
    return tips, w, pids, bls, spec, model_params(spec, subst, K, T, rng)


def bootstrap_case(n, P, K, B, seed):
    """A random tree and all its NNI neighbours at branch length 0.1, with replicate weights:
    (tips, weights, parent ids [T][2n-3], branch lengths, replicate weights [B][P], spec, params)."""
    import nni_ref as R
    rng = np.random.default_rng(seed)
    tips, w = TU.random_alignment(n, P, rng)
    pid = TU.random_topology(n, rng)
    W = rng.multinomial(int(w.sum()), w / w.sum(), B).astype(np.float64)
    bl = np.full(2 * n - 2, 0.1)
    bl[-1] = 0.0
    trees = [(pid, bl)] + [(x[2], x[3]) for x in R.all_neighbours(n, pid, bl)]
    pids = np.stack([t[0] for t in trees]).astype(np.int32)
    bls = np.stack([t[1] for t in trees])
    spec = O.make_spec(n, P, "JC69", site(K))
    pr = params(spec, len(pids), **({"Weibull shape": np.full((len(pids), 1), 0.7)} if K > 1 else {}))
    return tips, w, pids, bls, W, spec, pr
