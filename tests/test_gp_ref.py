"""tests/gp_ref.py (the numpy restatement the GPU tests of generalized pruning compare against)
checked on the CPU against the reference's known answers (src/gp_doctest.cpp) and against itself."""
import numpy as np
import pytest

import gp_ref as R

HELLO_LENGTHS = {"jupiter": 0.113, "mars": 0.15, "saturn": 0.1}   # the inner branch: 0.22, the root: 0


def _hello(fasta):
    pids, _, tips, w, names = R.load_case("hello_rooted.nwk", fasta)
    d = R.build_dag(pids)
    b = np.zeros(d.G)
    for i in range(d.R, d.G):
        s = d.entries[i][2]
        b[i] = HELLO_LENGTHS[names[s]] if s < d.n else 0.22
    return d, b, tips, w, names


def test_hello_classical_likelihood():
    d, b, tips, w, _ = _hello("hello.fasta")
    assert (d.R, d.G, d.topology_count) == (1, 5, 1.0)
    v = R.values(d, np.ones(d.G), b, tips, w, R.Model())
    assert np.all(np.abs(v["full"] - -84.77961943) < 1e-6)
    assert abs(v["log_marginal"] - -84.77961943) < 1e-6


def test_hello_single_nucleotide_derivative_of_root_to_jupiter():
    d, b, tips, w, names = _hello("hello_single_nucleotide.fasta")
    root = d.entries[0][2]
    e = next(i for i in range(d.R, d.G) if d.entries[i][0] == root and d.entries[i][2] == names.index("jupiter"))
    v = R.values(d, np.ones(d.G), b, tips, w, R.Model())
    assert abs(v["full"][e] - -4.806671945) < 1e-6
    assert abs(v["derivative"][e] - -0.6109379521) < 1e-6


def test_four_taxon_priors():
    pids = R.load_case("four-taxon-two-tree-rootsplit-uncertainty.nwk", "four-numbered-taxa.fasta")[0]
    d = R.build_dag(pids)
    q = dict(zip(R.strings(d), R.uniform_prior(d)))
    # the reference's names 0001|1110 and 0011|1100 in the representation PrettyIndexer gives rootsplits
    assert abs(q["0001"] - 2 / 3) < 1e-10 and abs(q["0011"] - 1 / 3) < 1e-10
    assert abs(q["0001|1110|0110"] - 1 / 2) < 1e-10 and abs(q["0001|1110|0010"] - 1 / 2) < 1e-10


def test_node_and_inverted_probabilities_of_five_taxon_rooted_more_2():
    """compared as sorted vectors: the reference's numbering is not reproducible"""
    pids = R.load_case("five_taxon_rooted_more_2.nwk", "five_taxon.fasta")[0]
    d = R.build_dag(pids)
    q = R.uniform_prior(d)
    node = [1, 1, 1, 1, 1, 0.5, 0.25, 0.75, 0.25, 0.5, 0.25, 0.25, 0.5, 0.5, 0.25]
    inverted = [1, 1, 1, 1 / 3, 0.5, 1, 0.5, 1, 1, 1, 0.5, 2 / 3, 0.5, 0.5, 0.5, 0.5, 0.5, 0.25, 0.5, 0.25, 0.25,
                0.75, 0.75, 0.25]
    assert (d.node_count, d.G) == (15, 24)
    assert np.allclose(np.sort(R.node_probabilities(d, q)), np.sort(node), rtol=0, atol=1e-12)
    assert np.allclose(np.sort(R.inverted_probabilities(d, q)), np.sort(inverted), rtol=0, atol=1e-12)


def test_five_taxon_rooted_spans_four_topologies():
    pids = R.load_case("five_taxon_rooted.nwk", "five_taxon.fasta")[0]
    d = R.build_dag(pids)
    assert d.topology_count == 4.0 and len(set(R.enumerate_trees(d))) == 4 and d.R == 3


def test_numbering_rule():
    pids = R.load_case("ds1-reduced-5.nwk", "ds1-reduced-5.fasta")[0]
    d = R.build_dag(pids)
    e = d.entries
    assert np.all(e[:d.R, 0] == -1) and len(set(e[:d.R, 2])) == d.R
    keys = [tuple(x) for x in e[d.R:]]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)          # blocks by node, clade, child
    first_seen = [int(e[i][2]) for i in range(d.R)]
    assert first_seen[0] == d.per_tree[0][0][2 * d.n - 2]                   # rootsplits by first occurrence
    for v in range(d.n, d.node_count):                                       # clade 0 holds the lowest taxon
        assert min(d.clades[v][0]) < min(d.clades[v][1])
        for c in range(2):
            lo, hi = d.block_range[v, c]
            assert hi > lo and all(d.clades[int(e[i][2])][0] | d.clades[int(e[i][2])][1] == d.clades[v][c]
                                   for i in range(lo, hi))
    seen = []                                                                # subsplits by first occurrence
    for node, _ in d.per_tree:
        seen += [node[v] for v in range(d.n, 2 * d.n - 1) if node[v] not in seen]
    assert seen == list(range(d.n, d.node_count))
    assert len(R.enumerate_trees(d)) == d.topology_count


def test_random_batches_span_few_trees_and_cover_the_shapes():
    sizes, through0, through1 = set(), 0, 0
    for i in range(len(R.RANDOM_CASES)):
        pids = R.random_case(i)[0]
        n = pids.shape[1] // 2 + 1
        assert 6 <= n <= 8 and np.all(pids > np.arange(2 * n - 2))
        d = R.build_dag(pids)
        assert d.topology_count <= 2000 and len(R.enumerate_trees(d)) == d.topology_count
        s, a, b = R.shape_summary(d)
        sizes, through0, through1 = sizes | s, max(through0, a), max(through1, b)
    assert {1, 2} <= sizes and max(sizes) >= 3 and through0 >= 2 and through1 >= 2


def test_every_tree_enters_each_leaf_once_and_priors_sum_to_one():
    pids, tips, w = R.random_case(2)
    d = R.build_dag(pids)
    q = R.random_q(d, np.random.default_rng(1))
    trees = R.enumerate_trees(d)
    assert abs(sum(np.prod(q[list(t)]) for t in trees) - 1) < 1e-12
    b = np.random.default_rng(2).uniform(0.02, 0.4, d.G)
    br = R.brute_force(d, q, b, tips, R.Model([0.1, 0.3, 0.1, 0.1, 0.3, 0.1], [0.3, 0.2, 0.2, 0.3]))
    for x in range(d.n):
        into = [i for i in range(d.R, d.G) if d.entries[i][2] == x]
        assert np.allclose(br.through[into].sum(0), br.M, rtol=1e-12, atol=0)
    assert np.allclose((q[:d.R, None] * br.through[:d.R]).sum(0), br.M, rtol=1e-12, atol=0)


@pytest.mark.parametrize("gtr", [False, True])
def test_analytic_derivatives_match_long_double_differences(gtr):
    pids, tips, w = R.random_case(0)
    d = R.build_dag(pids)
    model = R.Model([0.1, 0.3, 0.1, 0.1, 0.3, 0.1], [0.3, 0.2, 0.2, 0.3]) if gtr else R.Model()
    q = R.random_q(d, np.random.default_rng(3))
    b = np.random.default_rng(4).uniform(0.02, 0.4, d.G)
    b[:d.R] = 0.0
    v = R.values(d, q, b, tips, w, model)
    h = np.longdouble(1e-5)
    for e in range(d.R, d.G, 5):
        hi, lo, mid = (b.astype(np.longdouble) for _ in range(3))
        hi[e] += h
        lo[e] -= h
        f = [R.log_marginal(d, q, x, tips, w, model, np.longdouble) for x in (lo, mid, hi)]
        assert abs(float((f[2] - f[0]) / (2 * h)) - v["g"][e]) <= 1e-6 * max(abs(v["g"][e]), 1.0)
        assert abs(float((f[2] - 2 * f[1] + f[0]) / (h * h)) - v["H"][e]) <= 1e-4 * max(abs(v["H"][e]), v["S"][e])
    assert abs(float(f[1]) - v["log_marginal"]) <= 1e-12 * abs(v["log_marginal"])


def test_log_domain_pruning_agrees_with_plain_pruning():
    pids, tips, w = R.random_case(1)
    d = R.build_dag(pids)
    q, b = R.uniform_prior(d), np.full(d.G, 0.3)
    plain = R.log_marginal(d, q, b, tips, w, R.Model())
    assert abs(R.log_marginal_deep(d, q, b, tips, w, R.Model()) - plain) <= 1e-12 * abs(plain)


def test_restated_rule_converges_and_never_accepts_a_fall():
    pids, bl, tips, w, _ = R.load_case("hello_rooted_two_trees.nwk", "hello.fasta")
    d = R.build_dag(pids)
    q, model = R.uniform_prior(d), R.Model()
    assert np.allclose(R.hot_start(d, bl)[d.R:] > 0, True)

    def evaluate(x):
        v = R.values(d, q, x, tips, w, model)
        return v["log_marginal"], v["g"], v["H"], v["S"]
    b0 = np.full(d.G, 0.1)
    b0[:d.R] = 0.0
    x, trace, evaluations, status = R.optimize(evaluate, b0, d.R, tolerance=1e-4)
    assert status == 0 and evaluations == len(trace) and np.all(x[:d.R] == 0.0)
    assert np.all(np.diff(trace) >= -2.0 ** -48 * np.abs(trace[:-1])) and trace[-1] > trace[0]
    g = R.values(d, q, x, tips, w, model)["g"]
    assert R.criterion(x, g, d.R, np.exp(-13.9), np.exp(1.1)) <= 1e-4


def test_rooting_above_leaf_zero_keeps_the_splits():
    import tree_utils as TU
    rng = np.random.default_rng(5)
    pid = TU.random_topology(9, rng)
    rooted = R.root_above_leaf0(pid)
    n = 9
    assert np.all(rooted > np.arange(2 * n - 2)) and rooted[0] == 2 * n - 2
    def splits(p, nodes):
        taxa = {v: frozenset([v]) for v in range(n)}
        for v, parent in enumerate(p):
            taxa[int(parent)] = taxa.get(int(parent), frozenset()) | taxa[v]
        full = frozenset(range(n))
        return {min(s, full - s, key=sorted) for s in taxa.values() if 1 < len(s) < n - 1}
    assert splits(pid, 2 * n - 2) == splits(rooted, 2 * n - 1)
