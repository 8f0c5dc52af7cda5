"""Committed inputs of the starting-tree tests (TEST INFRASTRUCTURE ONLY): small alignments evolved
along random trees, the model rows they are measured under, and distance matrices for neighbour
joining.  tests/test_start_trees_ref.py checks on the CPU what the GPU tests rely on (the margins
of the cases whose topology is compared across implementations)."""
import numpy as np

import start_trees_ref as R
import tree_utils as TU

# seeds of the alignments whose neighbour-joining topology the GPU test compares with the
# reference's (smallest relative Q margin of any round >= 1e-9: test_start_trees_ref.py)
MEASURED_SEEDS = (11, 12, 13)
MEASURED_N, MEASURED_SITES = 8, 400


def evolved_alignment(n, sites, seed, gap_fraction=0.02, mean_bl=0.05):
    """Tip states [n][sites] evolved under JC69 along a random tree (so that the distances carry
    a tree), a few gaps, integer pattern weights 1..3."""
    rng = np.random.default_rng(seed)
    pid, bl = TU.random_trees(n, 1, rng, mean_bl=mean_bl)
    pid, bl = pid[0], bl[0] + 0.02
    root = 2 * n - 3
    state = np.zeros((root + 1, sites), np.int64)
    state[root] = rng.integers(0, 4, sites)
    for v in range(root - 1, -1, -1):  # a parent's id is above its children's
        stay = rng.random(sites) < np.exp(-4.0 * bl[v] / 3.0)  # (else a uniform draw: JC69)
        state[v] = np.where(stay, state[pid[v]], rng.integers(0, 4, sites))
    tips = state[:n].astype(np.int32)
    tips[rng.random((n, sites)) < gap_fraction] = 4
    weights = rng.integers(1, 4, size=sites).astype(np.float64)
    return tips, weights


def gtr_weibull_row(seed):
    """One parameter row of a GTR + Weibull(4) engine without a clock: rates [6], frequencies [4],
    shape -- and the same as (rates, freqs, category rates, category weights)."""
    rng = np.random.default_rng(1000 + seed)
    rates, freqs = TU.random_gtr_params(1, rng)
    shape = float(rng.uniform(1.0, 2.0))
    row = np.concatenate([rates[0], freqs[0], [shape]])
    cr, cw = R.weibull_categories(4, shape)
    return row, rates[0], freqs[0], cr, cw


def measured_case(seed):
    tips, weights = evolved_alignment(MEASURED_N, MEASURED_SITES, seed)
    return (tips, weights) + gtr_weibull_row(seed)


def reference_distances(tips, weights, lik, tmin=1e-8, tmax=10.0):
    """[n][n] long-double maximisers of the pair likelihoods (as float64)."""
    n = tips.shape[0]
    counts = R.pair_counts(tips, weights[None])[0]
    d = np.zeros((n, n))
    for q, (i, j) in enumerate(R.pair_index(n)):
        d[i, j] = d[j, i] = float(lik.maximiser(counts[q], tmin, tmax))
    return d


def dyadic_tree_matrix(n, seed, kind="random"):
    """(parent ids, branch lengths, path-length matrix) of a tree whose lengths are multiples of
    2^-10: every sum in neighbour joining's rule is exact."""
    rng = np.random.default_rng(seed)
    if kind == "random":
        pid = TU.random_topology(n, rng)
    elif kind == "ladder":
        pid = TU.ladder_topology(n)
    else:
        pid = TU.balanced_topology(n)
    bl = rng.integers(1, 512, size=2 * n - 2) / 1024.0
    bl[-1] = 0.0
    return pid, bl, R.path_lengths(pid, bl)


def noisy_matrix(n, seed):
    """An additive matrix of a random tree with generic (not dyadic) lengths plus 1 % noise: no
    ties, raw neighbour-joining lengths of either sign."""
    rng = np.random.default_rng(seed)
    pid, bl = TU.random_trees(n, 1, rng)
    d = R.path_lengths(pid[0], bl[0])
    d = d * rng.uniform(0.99, 1.01, size=d.shape)
    d = np.triu(d, 1)
    return d + d.T


# Seven taxa, generic distances: with seven clusters (r - 2 = 5, the product inexact) the rule's
# Q -- the product, then two subtractions, each rounded -- is smallest at slots (4, 6), while a
# fused (r-2) d - R_i, rounded once, makes (1, 5) the smallest (test_start_trees_ref.py checks
# both): an implementation that contracts the product into the subtraction joins another pair.
_CONTRACTION_SENSITIVE = (
    '0x1.7b9f2c08948bap+0', '0x1.a14c0288781c4p-1', '0x1.a1a589f792919p+0', '0x1.b7e8747d7f07cp-1',
    '0x1.9c6bbbd71823ep+0', '0x1.1420ae8ef9ef1p+0', '0x1.3e80537b138d4p+0', '0x1.4204e6e41f56cp+0',
    '0x1.e611bdbb0263ap-1', '0x1.38a653ff82962p-1', '0x1.32835079b2bbfp+0', '0x1.a77bf31c9d224p-1',
    '0x1.6afda2ea42f8fp+0', '0x1.24ad6e18ea40ap-1', '0x1.b17b1f8023de6p-1', '0x1.9e0e0410a3b72p+0',
    '0x1.b03789138c6e4p+0', '0x1.502a62c6104f8p+0', '0x1.1315b663318bdp+0', '0x1.7a84d29431802p-2',
    '0x1.9be3dab863c06p+0')


def contraction_sensitive_matrix():
    n = 7
    d = np.zeros((n, n))
    d[np.triu_indices(n, 1)] = [float.fromhex(x) for x in _CONTRACTION_SENSITIVE]
    return d + d.T
