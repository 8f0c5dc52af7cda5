"""The plain-Python restatement of split tables (tests/splits_ref.py) pinned to the reference,
and mi_consensus_tree (host arithmetic: no device) against it."""
import json
import os

import numpy as np
import pytest

import nni_ref
import oracle_lib as O
import splits_ref as R
import start_trees_ref
import tree_utils as TU

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_five_taxon_rootsplits_are_the_references():
    with open(os.path.join(GOLDEN, "split_kats.json")) as fh:
        want = json.load(fh)["five_taxon_rootsplits"]["strings"]
    assert len(want) == len(set(want)) == 12
    st = O.load_struct("five_taxon")
    assert st["taxon_names"] == [f"x{i}" for i in range(5)]
    _, _, pids, _ = O.struct_arrays(st)
    index, splits, first, trees = R.table(pids)
    assert set(R.strings(splits, 5)) == set(want)
    import libsbn_amd as L
    assert L.split_strings(R.words(splits, 5), 5) == R.strings(splits, 5)
    # numbering by first occurrence: tree 0's edge v has index v, its leaves come first
    assert list(index[0]) == [0, 1, 2, 3, 4, 5, 6, -1, -1]
    assert list(first[:7]) == list(range(7)) and np.all(trees[:5] == 4)
    assert all("1" not in s[0] for s in R.strings(splits, 5))


def test_ds1_split_sets_are_those_of_the_private_helpers():
    _, _, pids, bls = O.struct_arrays(O.load_struct("ds1_top100"))
    assert len(pids) == 100
    index, splits, first, trees = R.table(pids)
    n = 27
    for t in range(100):
        mine = R.split_set(pids[t])
        assert mine == set(start_trees_ref.splits(pids[t], bls[t]).keys())
        assert {s for s in mine if len(s) > 1 and len(s) < n - 1} == nni_ref.splits(n, pids[t])
        assert len(set(index[t][:-2])) == 2 * n - 3  # each split at most once per tree
    assert trees.sum() == 100 * (2 * n - 3) and np.all(np.diff(first) > 0)
    # appending trees changes nothing earlier
    head = R.table(pids[:40])
    assert np.array_equal(head[0], index[:40]) and head[1] == splits[:len(head[1])]


def _consensus(n, splits, weight, total, threshold):
    import libsbn_amd as L
    return L.consensus_tree(n, R.words(splits, n), weight, total, threshold)


@pytest.mark.parametrize("n,seed", [(4, 0), (5, 1), (12, 2), (33, 3), (65, 4)])
def test_consensus_of_rootings_of_one_tree_is_that_tree(n, seed):
    import libsbn_amd as L
    rng = np.random.default_rng(seed)
    pid, bl = TU.random_trees(n, 1, rng)
    trees = [pid[0]] + [R.reroot(pid[0], bl[0], v)[0] for v in range(n, 2 * n - 3)]
    index, splits, first, counts = R.table(np.stack(trees))
    assert len(splits) == 2 * n - 3 and np.all(counts == len(trees))
    got_pid, got_split = _consensus(n, splits, counts.astype(float), float(len(trees)), 0.5)
    assert len(got_pid) == 2 * n - 3 and len(got_split) == 2 * n - 2
    assert R.split_set(got_pid) == R.split_set(pid[0])
    want_pid, want_split = R.consensus(n, splits, counts, len(trees), 0.5)
    assert np.array_equal(got_pid, want_pid) and np.array_equal(got_split, want_split)
    # each node's entry is the table index of its edge
    assert [splits[k] for k in got_split[:-1]] == R.edge_splits(got_pid) and got_split[-1] == -1
    # a valid tree of every unrooted call (mi_nni_neighbour checks the form); n = 4 has one inner edge
    L.nni_neighbour(n, got_pid, np.ones(2 * n - 2), n, 0)


@pytest.mark.parametrize("n", [3, 4, 9, 40])
def test_consensus_is_a_star_when_no_split_reaches_the_threshold(n):
    rng = np.random.default_rng(n)
    pids, _ = TU.random_trees(n, 6, rng)
    index, splits, first, counts = R.table(pids)
    pid, node_split = _consensus(n, splits, counts.astype(float), 6.0, 0.999)
    keep = [i for i, s in enumerate(splits) if 1 < R.popcount(s) < n - 1 and counts[i] == 6]
    if not keep:
        assert len(pid) == n and np.all(pid == n) and list(node_split) == list(range(n)) + [-1]
    # weights of 0: nothing is kept, whatever the trees
    pid, node_split = _consensus(n, splits, np.zeros(len(splits)), 6.0, 0.5)
    assert len(pid) == n and np.all(pid == n) and list(node_split) == list(range(n)) + [-1]


@pytest.mark.parametrize("n,T,threshold,seed", [(6, 5, 0.5, 0), (12, 9, 0.5, 1), (12, 9, 0.75, 2), (40, 7, 0.5, 3)])
def test_partly_resolved_consensus_follows_the_convention(n, T, threshold, seed):
    """Trees a few NNI moves apart share most splits: the consensus is partly resolved, numbered
    with the children by largest leaf id, in post-order."""
    import libsbn_amd as L
    rng = np.random.default_rng(seed)
    pid, bl = TU.random_trees(n, 1, rng)
    trees = [pid[0]]
    for _ in range(T - 1):
        p, b = trees[int(rng.integers(len(trees)))], np.ones(2 * n - 2)
        for _ in range(2):
            p, b = L.nni_neighbour(n, p, b, int(rng.integers(n, 2 * n - 3)), int(rng.integers(2)))
        trees.append(p)
    index, splits, first, counts = R.table(np.stack(trees))
    w = rng.integers(1, 4, size=T).astype(float)
    weight = R.stats(index, len(splits), None, w)[:, 0]
    got_pid, got_split = _consensus(n, splits, weight, w.sum(), threshold)
    want_pid, want_split = R.consensus(n, splits, weight, w.sum(), threshold)
    assert np.array_equal(got_pid, want_pid) and np.array_equal(got_split, want_split)
    m = len(got_split)
    assert n + 1 <= m <= 2 * n - 2
    kept = {splits[k] for k in got_split[n:-1]}
    assert kept == {s for i, s in enumerate(splits) if 1 < R.popcount(s) < n - 1 and weight[i] > threshold * w.sum()}
    # post-order ids, children by largest leaf id: a parent is above its children, and the
    # internal nodes are numbered in the order their subtrees close
    assert np.all(got_pid > np.arange(m - 1)) and np.sum(got_pid == m - 1) >= 3


def test_consensus_refuses_a_threshold_below_one_half():
    _, splits, _, counts = R.table(TU.random_trees(6, 3, np.random.default_rng(0))[0])
    for bad in (0.49, 1.0, float("nan")):
        with pytest.raises(RuntimeError, match=r"threshold must be in \[0.5, 1\)"):
            _consensus(6, splits, counts.astype(float), 3.0, bad)
    # splits that cannot sit in one tree are refused, not built
    with pytest.raises(RuntimeError, match="incompatible"):
        _consensus(5, [0b00110, 0b01100], np.ones(2), 1.0, 0.5)
