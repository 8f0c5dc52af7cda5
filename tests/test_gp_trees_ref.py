"""The restatement of the tree side of generalized pruning (tests/gp_trees_ref.py) against the
reference's known answers (rooted_sbn_instance.hpp, gp_doctest.cpp) and against itself.  CPU only.
Entries are matched by their strings() name; leaf entries (child part all zeros) have no
counterpart in the reference's rooted SBN and are left out."""
import csv
import math
import os

import numpy as np
import pytest

import gp_ref as GR
import gp_trees_ref as TR


def load_trees(nwk):
    from libsbn_amd import _hostapi
    tc = _hostapi.TreeCollection.of_newick_file(os.path.join(GR.GOLDEN, nwk))
    return np.stack(tc.parent_ids).astype(np.int32), np.stack(tc.branch_lengths), list(tc.taxon_names)


def named(d, values):
    """{name: value} of the entries whose child is no leaf"""
    return {s: float(values[i]) for i, s in enumerate(GR.strings(d)) if i < d.R or set(s.split("|")[2]) != {"0"}}


def trained(nwk):
    pids, _, _ = load_trees(nwk)
    d = GR.build_dag(pids)
    entries, nodes = TR.index_batch(d, pids)
    assert (entries < d.G).all() and (nodes >= 0).all()
    return d, TR.simple_average(d, entries)


FIVE_TAXON_SA = {"00111": 0.25, "01111": 0.5, "00010": 0.25, "00100|01010|00010": 1, "00111|11000|01000": 1,
                 "00100|00011|00001": 1, "11000|00111|00011": 1, "00100|11001|01001": 1, "10000|01001|00001": 1,
                 "01000|00111|00010": 1, "10000|01111|00001": 0.5, "10000|01111|00111": 0.5, "00010|00101|00001": 1,
                 "00001|01110|00100": 1, "00010|11101|00100": 1}


def test_simple_average_on_five_taxon_rooted():
    d, q = trained("five_taxon_rooted.nwk")
    got = named(d, q)
    assert set(got) == set(FIVE_TAXON_SA)
    for name, value in FIVE_TAXON_SA.items():
        assert got[name] == pytest.approx(value, abs=1e-12), name


def test_rooted_indexer_representation():
    pids, _, _ = load_trees("five_taxon_rooted.nwk")
    d = GR.build_dag(pids)
    entries, _ = TR.tree_index(d, np.array([5, 5, 7, 6, 6, 8, 7, 8], np.int32))   # ((0,1),(2,(3,4)))
    names = GR.strings(d)
    got = {names[e] for e in entries if set(names[e].split("|")[-1]) != {"0"} or e < d.R}
    assert got == {"00111", "11000|00111|00011", "00100|00011|00001", "00111|11000|01000"}


def test_simple_average_on_twenty_taxa():
    d, q = trained("rooted_simple_average.nwk")
    with open(os.path.join(GR.GOLDEN, "rooted_simple_average_results.csv")) as f:
        correct = {row[0].replace("|", ""): float(row[1]) for row in csv.reader(f) if row}   # (compared with the pipes stripped)
    got = named(d, q)
    assert {name.replace("|", "") for name in got} == set(correct)
    for name, value in got.items():
        assert abs(value - correct[name.replace("|", "")]) < 1e-6, name


SUBSPLIT_PROBABILITIES = {"0011111000": 0.5, "0111110000": 0.3, "0001011101": 0.2, "1100100100": 0.2, "0100000111": 0.1,
                          "0111000001": 0.2, "0101000100": 0.2, "1000001001": 0.2, "0010000011": 0.4, "0011000001": 0.2,
                          "1000001000": 0.5, "0100000010": 0.2, "0100000001": 0.2, "0010000010": 0.2, "0001000001": 0.4}


def test_unconditional_subsplit_probabilities():
    d, q = trained("five_taxon_rooted_more.nwk")
    prob = GR.node_probabilities(d, q)

    def bits(s):
        return "".join("1" if x in s else "0" for x in range(d.n))

    seen = set()
    assert d.node_count - d.n == len(SUBSPLIT_PROBABILITIES)
    for v in range(d.n, d.node_count):
        a, b = bits(d.clades[v][0]), bits(d.clades[v][1])
        name = a + b if a + b in SUBSPLIT_PROBABILITIES else b + a   # (the reference's chunk order is its bitset order)
        assert name in SUBSPLIT_PROBABILITIES and name not in seen
        seen.add(name)
        assert abs(prob[v] - SUBSPLIT_PROBABILITIES[name]) < 1e-8, name


def test_five_taxon_dag_has_four_distinct_trees():
    pids, _, _ = load_trees("five_taxon_rooted.nwk")
    d = GR.build_dag(pids)
    assert d.topology_count == 4
    built, entries = TR.enumerate_numbered(d)
    assert len({tuple(p) for p in built}) == 4
    for p, e in zip(built, entries):   # a built tree indexes to its own entries, and its nodes are the DAG's
        again, nodes = TR.tree_index(d, p)
        assert (again == e).all() and (nodes >= 0).all()


def _clades(pid):
    n, kids, taxa = GR._tree_nodes(pid)
    return {taxa[v] for v in range(n, 2 * n - 1)}


def test_complete_rooted_tree_collection():
    """GPInstance: GenerateCompleteRootedTreeCollection -- the two topologies of
    ((0,1),(2,(3,4))) and (1,(0,(2,(3,4)))), every edge carrying the length of the entry it is named by"""
    pids, _, names = load_trees("5-taxon-only-rootward-uncertainty.nwk")
    assert names == ["0", "1", "2", "3", "4"]
    d = GR.build_dag(pids)
    assert d.G == 14 and d.topology_count == 2
    b = np.arange(d.G, dtype=float)
    built, entries = TR.enumerate_numbered(d)
    f = frozenset
    expected = [{f([0, 1]), f([3, 4]), f([2, 3, 4]), f(range(5))}, {f([3, 4]), f([2, 3, 4]), f([0, 2, 3, 4]), f(range(5))}]
    assert [_clades(p) for p in built] == expected
    strings = GR.strings(d)

    def bits(s):
        return "".join("1" if x in s else "0" for x in range(d.n))

    for p, e in zip(built, entries):
        n, kids, taxa = GR._tree_nodes(p)
        lengths = TR.branch_lengths(d, b, e, -1.0)
        for v in range(2 * n - 2):
            sister = taxa[int(p[v])] - taxa[v]
            if v < n:
                child = frozenset()
            else:
                x, y = (taxa[k] for k in kids[v])
                child = y if min(x) < min(y) else x
            assert strings[e[v]] == bits(sister) + "|" + bits(taxa[v]) + "|" + bits(child)
            assert lengths[v] == e[v]
        assert lengths[-1] == 0.0 and e[-1] < d.R


@pytest.mark.parametrize("case", range(len(GR.RANDOM_CASES)))
def test_unranking_follows_enumerate_trees(case):
    pids, _, _ = GR.random_case(case)
    d = GR.build_dag(pids)
    trees = GR.enumerate_trees(d)
    assert len(trees) == int(d.topology_count)
    q = GR.random_q(d, np.random.default_rng(5))
    total = 0.0
    for r, tree in enumerate(trees):
        root_entry, built = TR.unrank(d, r)
        assert TR.flatten(root_entry, built) == tuple(tree)
        pid, entries = TR.number_tree(d.n, root_entry, built)
        again, _ = TR.tree_index(d, pid)
        assert (again == entries).all() and sorted(entries) == sorted(tree)
        total += math.exp(TR.log_q(d, q, entries))
    assert abs(total - 1.0) < 1e-12


# K = 4096 at a fixed seed: every tree's count lies within 5 sqrt(K q (1 - q)) of K q (the seed was
# kept after the check held here; the bound is 5 standard deviations of a binomial count)
SAMPLER_SEED, SAMPLER_K = 20260417, 4096


def test_sampler_frequencies():
    d, q = trained("five_taxon_rooted.nwk")
    values = TR.cdf(d, q)
    built, entries = TR.enumerate_numbered(d)
    prob = {tuple(p): math.exp(TR.log_q(d, q, e)) for p, e in zip(built, entries)}
    assert abs(sum(prob.values()) - 1.0) < 1e-12
    counts = dict.fromkeys(prob, 0)
    for t in range(SAMPLER_K):
        pid, e = TR.sample_tree(d, values, SAMPLER_SEED, t)
        counts[tuple(pid)] += 1   # (KeyError: a sampled tree outside the DAG)
    for tree, p in prob.items():
        assert abs(counts[tree] - SAMPLER_K * p) <= 5 * math.sqrt(SAMPLER_K * p * (1 - p)), (tree, counts[tree], p)


def test_deroot():
    rng = np.random.default_rng(3)
    for n in (3, 4, 5, 9):
        for pid in GR.nni_batch(n, 6, 2, rng):
            bl = rng.uniform(0.1, 1.0, 2 * n - 1)
            bl[-1] = 0.0
            out, lengths, edge = TR.deroot(pid, bl)
            # ids: children before parents, root 2n-3 with three children, every other internal node two
            assert all(out[v] > v and out[v] >= n for v in range(2 * n - 3))
            arity = np.bincount(out, minlength=2 * n - 2)[n:]
            assert arity[-1] == 3 and (arity[:-1] == 2).all()
            # the same splits: every rooted clade below the root's children is a clade or a complement
            below = {v: frozenset([v]) for v in range(n)}
            for v in range(2 * n - 3):
                below[int(out[v])] = below.get(int(out[v]), frozenset()) | below[v]
            everything = frozenset(range(n))
            rooted = {min(c, everything - c, key=sorted) for c in _clades(pid) if 1 < len(c) < n - 1}
            unrooted = {min(below[v], everything - below[v], key=sorted) for v in range(n, 2 * n - 3) if 1 < len(below[v]) < n - 1}
            assert rooted == unrooted
            assert lengths.sum() == pytest.approx(bl.sum()) and lengths[-1] == 0.0
            # the root edge carries both root edges' lengths
            n_, kids, taxa = GR._tree_nodes(pid)
            a, b = kids[2 * n - 2]
            assert lengths[edge] == pytest.approx(bl[a] + bl[b])
            # the trifurcation holds taxon n-1 below one of its two own children unless that root child was a leaf
            x = a if n - 1 in taxa[a] else b
            if x >= n:
                assert n - 1 not in below[edge]
