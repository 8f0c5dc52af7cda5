"""mi_nni_neighbour (libsbn_amd.nni_neighbour): the trees the NNI neighbourhood scan scores.
Pure host arithmetic, no GPU: checked against tests/nni_ref.py, which rebuilds each neighbour
from the public definition as nested subtrees and renumbers it with tree_utils._polish's
rule."""
import numpy as np
import pytest

import nni_ref as R
import tree_utils as TU


def _trees(n):
    rng = np.random.default_rng(100 + n)
    out = [("ladder", TU.ladder_topology(n)), ("balanced", TU.balanced_topology(n))]
    out += [(f"random{i}", TU.random_topology(n, rng)) for i in range(3)]
    return [(name, pid, np.round(rng.uniform(0.01, 0.9, size=2 * n - 2), 6)) for name, pid in out]


def _neighbour(n, pid, bl, v, i):
    from libsbn_amd import nni_neighbour
    return nni_neighbour(n, pid, bl, v, i)


@pytest.mark.parametrize("n", [4, 5, 8, 27])
def test_matches_the_definition(n):
    for name, pid, bl in _trees(n):
        for v, i, want_pid, want_bl in R.all_neighbours(n, pid, bl):
            got_pid, got_bl = _neighbour(n, pid, bl, v, i)
            assert np.array_equal(got_pid, want_pid), (name, v, i, got_pid, want_pid)
            assert np.array_equal(got_bl, want_bl), (name, v, i)


@pytest.mark.parametrize("n", [4, 5, 8, 27])
def test_neighbours_are_distinct_topologies(n):
    for name, pid, bl in _trees(n):
        own = R.splits(n, pid)
        seen = [frozenset(R.splits(n, _neighbour(n, pid, bl, v, i)[0]))
                for v in R.inner_edges(n) for i in (0, 1)]
        assert len(seen) == 2 * (n - 3)
        assert len(set(seen)) == len(seen), name
        assert frozenset(own) not in seen, name
        # one split exchanged for another
        assert all(len(s) == n - 3 and len(s & own) == n - 4 for s in seen), name


@pytest.mark.parametrize("n", [4, 5, 8, 27])
def test_a_move_can_be_undone(n):
    """In the neighbour, the edge whose split is new has two neighbours of its own: exactly one
    of them is the tree the move started from."""
    for name, pid, bl in _trees(n):
        own = R.splits(n, pid)
        for v in R.inner_edges(n):
            for i in (0, 1):
                npid, nbl = _neighbour(n, pid, bl, v, i)
                below = [frozenset([x]) if x < n else frozenset() for x in range(2 * n - 2)]
                for x in range(2 * n - 3):
                    below[npid[x]] = below[npid[x]] | below[x]
                new = [x for x in R.inner_edges(n)
                       if (below[x] if 0 not in below[x] else frozenset(range(n)) - below[x]) not in own]
                assert len(new) == 1, (name, v, i)
                back = [R.splits(n, _neighbour(n, npid, nbl, new[0], j)[0]) == own for j in (0, 1)]
                assert sum(back) == 1, (name, v, i, back)


def test_branch_lengths_travel_with_their_subtrees():
    """Leaves keep their ids and lengths; the multiset of lengths is unchanged."""
    n = 8
    for name, pid, bl in _trees(n):
        for v, i, _, _ in R.all_neighbours(n, pid, bl):
            _, got = _neighbour(n, pid, bl, v, i)
            assert np.array_equal(got[:n], bl[:n])
            assert np.array_equal(np.sort(got), np.sort(bl))


def test_refusals():
    from libsbn_amd import nni_neighbour
    n = 6
    _, pid, bl = _trees(n)[2]
    for node in list(range(n)) + [2 * n - 3, 2 * n - 2, -1]:
        with pytest.raises(RuntimeError, match="inner edge"):
            nni_neighbour(n, pid, bl, node, 0)
    for which in (2, -1):
        with pytest.raises(RuntimeError, match="which"):
            nni_neighbour(n, pid, bl, n, which)
    bad = pid.copy()
    bad[0] = 0
    with pytest.raises(RuntimeError):
        nni_neighbour(n, bad, bl, n, 0)
    # three taxa: no inner edge at all
    with pytest.raises(RuntimeError, match="inner edge"):
        nni_neighbour(3, np.array([3, 3, 3], np.int32), np.zeros(4), 3, 0)
