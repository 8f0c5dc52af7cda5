"""tests/start_trees_ref.py checked by routes that do not share its code, and the properties of
the committed cases that tests/test_start_trees_gpu.py relies on (no GPU needed)."""
import numpy as np
import pytest

import start_trees_cases as Cs
import start_trees_ref as R
import tree_utils as TU

LD = np.longdouble


def test_counts_against_a_plain_loop():
    rng = np.random.default_rng(3)
    tips, w = TU.random_alignment(5, 23, rng, gap_fraction=0.2)
    W = np.stack([w, rng.integers(0, 4, 23).astype(float)])
    got = R.pair_counts(tips, W)
    for q, (i, j) in enumerate(R.pair_index(5)):
        for r in range(2):
            want = np.zeros((4, 4), np.int64)
            for p in range(23):
                if tips[i, p] < 4 and tips[j, p] < 4:
                    want[tips[i, p], tips[j, p]] += int(W[r, p])
            assert np.array_equal(got[r, q], want)


def test_codes_from_partials():
    v = np.array([[[1, 0, 0, 0], [0, 0, 1, 0], [1, 1, 1, 1], [1, 1, 0, 0], [0.5, 0, 0, 0], [0, 0, 0, 0],
                   [1, 0, 0.25, 0]]], float)
    assert R.codes_from_partials(v).tolist() == [[0, 2, 4, 4, 4, 4, 4]]


def test_jc69_maximiser_meets_the_closed_form():
    lik = R.PairLikelihood(np.ones(6), np.full(4, 0.25), [1.0], [1.0])
    rng = np.random.default_rng(5)
    for _ in range(6):
        N = rng.integers(0, 40, size=(4, 4)) + 60 * np.eye(4, dtype=np.int64)
        share = 1 - np.trace(N) / N.sum()
        want = R.jc69_distance(share)
        got = lik.maximiser(N)
        assert abs(got - want) <= 1e-15 * want, (got, want)
        _, g, h = lik.derivatives(N, want)
        assert abs(g / h) <= 1e-15 * want


def test_derivatives_against_differences():
    row, rates, freqs, cr, cw = Cs.gtr_weibull_row(2)
    lik = R.PairLikelihood(rates, freqs, cr, cw)
    N = np.arange(16).reshape(4, 4) + 30 * np.eye(4)
    t, h = LD(0.3), LD(1e-5)
    l0, g0, h0 = lik.derivatives(N, t)
    lp, gp, _ = lik.derivatives(N, t + h)
    lm, gm, _ = lik.derivatives(N, t - h)
    assert abs((lp - lm) / (2 * h) - g0) <= 1e-8 * abs(g0)
    assert abs((gp - gm) / (2 * h) - h0) <= 1e-8 * abs(h0)


@pytest.mark.parametrize("kind", ["random", "ladder", "balanced"])
@pytest.mark.parametrize("n", [3, 4, 5, 12, 33])
def test_neighbour_joining_recovers_additive_dyadic_trees(kind, n):
    """Path-length distances of a tree with lengths in multiples of 2^-10: every sum of the rule
    is exact, so NJ returns exactly that topology (as splits: where the trifurcation sits is
    the rule's, not the tree's) and its lengths."""
    pid, bl, d = Cs.dyadic_tree_matrix(n, 40 + n, kind)
    got_pid, got_bl = R.neighbour_joining(d)
    want, got = R.splits(pid, bl), R.splits(got_pid, got_bl)
    assert want.keys() == got.keys()
    assert max(abs(want[k] - got[k]) for k in want) <= 1e-12
    assert got_bl[-1] == 0.0
    # the result is in the reference's numbering: leaves keep their ids, parents above children
    assert np.all(got_pid > np.arange(2 * n - 3)) and np.all(got_pid >= n)


def test_lowest_pair_wins_among_equal_q():
    """All distances equal: every Q of every round is equal, so the joins are (0, 1), then (0, 2)
    ... -- a ladder on the slots."""
    n = 6
    d = np.ones((n, n)) - np.eye(n)
    pid, bl = R.neighbour_joining(d)
    want = TU._polish(((((0, 1), 2), 3), 4, 5), n)
    assert np.array_equal(pid, want)


def test_negative_raw_lengths_are_clamped():
    d = np.array([[0, 1.0, 1.0, 5.0], [0, 0, 0.1, 1.0], [0, 0, 0, 1.0], [0, 0, 0, 0]])
    pid, bl = R.neighbour_joining(d, 1e-8, 10.0)
    assert bl[:-1].min() == 1e-8 and bl[-1] == 0.0


def test_the_contraction_sensitive_matrix_is_sensitive():
    """On this matrix the rule (every operation rounded once) and a fused (r-2) d - R_i join
    different pairs in the first round: the GPU test on it tells the two apart."""
    d = Cs.contraction_sensitive_matrix()
    assert R.first_join(d) == (4, 6) and R.first_join(d, fused=True) == (1, 5)
    pid, bl = R.neighbour_joining(d)
    fused_pid, fused_bl = R.neighbour_joining(d, fused=True)
    assert pid[4] == pid[6] and fused_pid[1] == fused_pid[5]
    assert not np.array_equal(pid, fused_pid) and not np.array_equal(bl, fused_bl)


@pytest.mark.parametrize("seed", Cs.MEASURED_SEEDS)
def test_margins_of_the_measured_cases(seed):
    """The cases whose topology the GPU test compares with the reference's: the smallest relative
    margin between the best and the second-best Q of any round must be >= 1e-9 (measured
    distances carry about 1e-10 of solver tolerance).  The two cherries of the last four clusters
    always tie -- Q(a, b) = Q(c, d) identically -- and give the same unrooted tree with the
    trifurcation in another place: across implementations the trees are compared as splits."""
    tips, weights, row, rates, freqs, cr, cw = Cs.measured_case(seed)
    d = Cs.reference_distances(tips, weights, R.PairLikelihood(rates, freqs, cr, cw))
    assert np.all(d[np.triu_indices(len(d), 1)] > 1e-8) and d.max() < 10.0
    margins = []
    R.neighbour_joining(d, margins=margins)
    print(f"seed {seed}: smallest relative Q margin {min(margins):.3e}")
    assert min(margins) >= 1e-9
