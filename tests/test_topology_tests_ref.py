"""The plain restatement of the bootstrap sampler and the KH / SH / AU tests
(tests/topology_tests_ref.py) checked on its own: row properties and the multinomial law of the
sampler, the double-precision AU fit against 50-digit mpmath, and known answers."""
import math

import numpy as np
import pytest

import sbn_vi_ref as V
import topology_tests_ref as R

W8 = [3, 0, 1, 12, 40, 7, 0, 1]


def test_vectorised_philox_is_the_scalar_one():
    rng = np.random.default_rng(0)
    cs = rng.integers(0, 2 ** 32, size=(50, 4), dtype=np.uint64)
    key = (0x9E3779B9, 0x12345678)
    got = R.philox_many(cs[:, 0], cs[:, 1], cs[:, 2], cs[:, 3], key)
    for i in range(50):
        assert [int(g[i]) for g in got] == V.philox4x32_10([int(x) for x in cs[i]], key)
    for n in (1, 2, 7):
        assert R.draws(5, 2 ** 32 + 9, n) == R.draws_scalar(5, 2 ** 32 + 9, n)


def test_rows_sum_to_n_skip_empty_patterns_and_depend_on_the_replicate_number_only():
    for n in (1, 2, 63, 64, 90):
        W = R.bootstrap_weights(W8, 9, n, seed=11, first_replicate=2 ** 32 + 5)
        assert W.shape == (9, 8) and np.all(W.sum(axis=1) == n)
        assert np.all(W[:, 1] == 0) and np.all(W[:, 6] == 0)
        assert np.all(W == np.floor(W)) and np.all(W >= 0)
        later = R.bootstrap_weights(W8, 2, n, seed=11, first_replicate=2 ** 32 + 12)
        assert np.array_equal(later, W[7:])
        assert not np.array_equal(R.bootstrap_weights(W8, 9, n, seed=12, first_replicate=2 ** 32 + 5), W) or n == 1
    # an odd n is the even one without its last draw
    cum, _ = R.prefix_sum(W8)
    x = R.draws(3, 4, 8)
    assert R.draws(3, 4, 7) == x[:7]
    with pytest.raises(ValueError):
        R.prefix_sum([1.5, 2])
    with pytest.raises(ValueError):
        R.prefix_sum([0, 0])
    with pytest.raises(ValueError):
        R.prefix_sum([2.0 ** 30, 2.0 ** 30])


@pytest.mark.parametrize("n", [32, 64, 90])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_column_means_follow_the_multinomial_law(n, seed):
    """Column means of B = 4000 rows within 6 standard errors sqrt(n q (1 - q) / B) of n q.  (Nine
    cases x six live patterns: a 6 sigma cap fails a correct sampler about once in 1e7 runs, and
    the draws are fixed by the seed.)"""
    B = 4000
    q = np.array(W8, float) / sum(W8)
    W = R.bootstrap_weights(W8, B, n, seed)
    se = np.sqrt(n * q * (1 - q) / B)
    dev = np.abs(W.mean(axis=0) - n * q)
    live = q > 0
    print(f"n={n} seed={seed}: largest deviation {float((dev[live] / se[live]).max()):.2f} standard errors")
    assert np.all(dev[live] <= 6 * se[live]) and np.all(dev[~live] == 0)


def test_au_fit_in_double_agrees_with_mpmath():
    """300 random ten-scale count tables, B_k = 1000: |double - mpmath| <= 1e-10 in d, c and p."""
    rng = np.random.default_rng(7)
    scales = np.array([1.0, 0.5, 0.6, 0.7, 0.8, 0.9, 1.1, 1.2, 1.3, 1.4])
    from scipy.special import ndtr
    N, worst, fitted = 1949, 0.0, 0
    sites = np.floor(scales * N + 0.5).astype(np.int64)
    reps = np.full(10, 1000)
    for _ in range(300):
        d, c = rng.uniform(-2.5, 2.5), rng.uniform(-0.5, 1.5)
        r = sites / N
        cnt = rng.binomial(1000, ndtr(-(d * np.sqrt(r) + c / np.sqrt(r))))
        p, dd, cc, rss, usable = R.au_fit(cnt, sites, reps, N)
        mp_p, mp_d, mp_c, mp_rss, mp_usable = R.au_fit_mp(cnt, sites, reps, N)
        assert usable == mp_usable == int(np.sum((cnt > 0) & (cnt < 1000)))
        if usable < 2:
            assert p is None and math.isnan(dd) and math.isnan(cc) and math.isnan(rss)
            continue
        fitted += 1
        worst = max(worst, abs(float(mp_p - p)), abs(float(mp_d - dd)), abs(float(mp_c - cc)))
        assert abs(float(mp_rss - rss)) <= 1e-10 * max(1.0, float(mp_rss))
    print(f"AU fit, double against 50 digits: largest difference {worst:.2e} over {fitted} fitted tables")
    assert fitted >= 200 and worst <= 1e-10


def _case(T, P, seed):
    rng = np.random.default_rng(seed)
    s = rng.uniform(-9.0, -2.0, size=(T, P))
    w = rng.integers(0, 5, size=P).astype(np.float64)
    w[0] = 3.0
    return s, w


def test_two_equal_rows_follow_the_tie_rules():
    s, w = _case(2, 13, 1)
    s[1] = s[0]
    N = int(w.sum())
    table, counts, mean, c0, best0 = R.topology_tests(s, w, [N, N // 2, 2 * N], [40, 30, 30], seed=3)
    col = dict(zip(R.COLUMNS, table.T))
    assert np.array_equal(col["bp"], [1.0, 0.0]) and np.array_equal(counts, [[40, 0], [30, 0], [30, 0]])
    assert np.array_equal(col["p_kh"], [1.0, 1.0]) and np.array_equal(col["p_sh"], [1.0, 1.0])
    assert np.array_equal(col["delta"], [0.0, 0.0]) and np.array_equal(col["usable"], [0.0, 0.0])
    assert np.array_equal(col["p_au"], col["bp"]) and np.all(np.isnan(col["d"]))


def test_one_tree():
    s, w = _case(1, 7, 2)
    N = int(w.sum())
    table, counts, mean, c0, best0 = R.topology_tests(s, w, [N, N + 3], [16, 16], seed=1)
    col = dict(zip(R.COLUMNS, table.T))
    assert col["p_kh"][0] == 1.0 and col["p_sh"][0] == 1.0 and col["bp"][0] == 1.0 and col["elw"][0] == 1.0
    assert col["usable"][0] == 0 and col["p_au"][0] == 1.0 and col["delta"][0] == 0.0
    assert col["L"][0] == float(np.dot(w, s[0]))


def test_a_tree_worse_on_every_pattern_by_a_constant_never_wins():
    s, w = _case(3, 21, 4)
    s[1], s[2] = s[0] - 0.5, s[0] - 0.25  # (every centred row is then zero up to rounding: only the gaps in L decide)
    N = int(w.sum())
    table, counts, mean, c0, best0 = R.topology_tests(s, w, [N, N // 2, N + N // 2], [50, 50, 50], seed=9)
    col = dict(zip(R.COLUMNS, table.T))
    assert np.all(counts[:, 1:] == 0) and np.all(col["usable"] == 0) and np.array_equal(col["bp"], [1.0, 0.0, 0.0])
    assert np.array_equal(col["p_sh"], [1.0, 0.0, 0.0]) and np.array_equal(col["p_kh"], [1.0, 0.0, 0.0])
    assert math.isnan(col["d"][2]) and col["p_au"][2] == 0.0
    assert np.array_equal(mean, R.column_means(c0))
    with pytest.raises(ValueError):
        R.topology_tests(s, w, [N + 1, N], [4, 4])
    with pytest.raises(ValueError):
        R.topology_tests(s, w, [N, N], [4, 4])
