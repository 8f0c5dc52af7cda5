"""The references of the per-pattern / RELL tests (tests/rell_ref.py) and the host helper
rell_weights, on the CPU."""
import numpy as np
import pytest

import oracle_lib as O
import rell_ref as RR


@pytest.mark.parametrize("name,P,subst,K", [("n4", 13, "JC69", 1), ("balanced8", 17, "GTR", 4),
                                            ("ladder9", 65, "JC69", 6), ("random12", 131, "GTR", 2)])
def test_per_pattern_values_sum_to_the_oracle_total(name, P, subst, K):
    tips, w, pids, bls, spec, pr = RR.case(name, P, subst, K, 77)
    s = RR.pattern_log_likelihoods(spec, tips, pids, bls, pr)
    total = O.unrooted_log_likelihoods(spec, tips, w, pids, bls, pr, False, 1)
    assert s.shape == (len(pids), P) and np.all(s < -1)  # like-signed terms: no cancellation
    err = np.abs(s @ w - total)
    print(name, (err / np.abs(total)).max())
    assert np.all(err <= P * 2.0 ** -52 * np.abs(total))
    # rescaling changes nothing beyond rounding
    sr = RR.pattern_log_likelihoods(spec, tips, pids, bls, pr, rescaling=True)
    assert np.all(np.abs(sr - s) <= 4 * 2.0 ** -52 * np.abs(s))


def test_rell_weights():
    import libsbn_amd as L
    w = np.array([3.0, 1.0, 0.0, 5.0, 2.0])
    a = L.rell_weights(w, 7, 11)
    assert a.shape == (7, 5) and a.dtype == np.float64
    assert np.all(a.sum(axis=1) == w.sum()) and np.all(a[:, 2] == 0) and np.all(a == np.rint(a))
    assert np.array_equal(a, L.rell_weights(w, 7, 11))
    assert not np.array_equal(a, L.rell_weights(w, 7, 12))
    assert np.array_equal(a, np.random.default_rng(11).multinomial(11, w / 11, 7))
    with pytest.raises(RuntimeError):
        L.rell_weights([1.5, 2.0], 3, 0)


def test_numpy_references_on_a_hand_made_case():
    # two trees, three patterns; replicate 0 favours tree 0, replicate 1 ties, replicate 2 favours tree 1
    s = np.array([[-1.0, -2.0, -4.0], [-2.0, -2.0, -3.0]])
    w = np.array([[2.0, 0.0, 0.0], [1.0, 5.0, 1.0], [0.0, 1.0, 2.0]])
    c, best, bp, elw = RR.rell(s, w)
    assert np.array_equal(np.asarray(c, float), [[-2.0, -4.0], [-15.0, -15.0], [-10.0, -8.0]])
    assert np.array_equal(best, [0, 0, 1])  # the tie goes to the lower index
    assert np.array_equal(bp, [2 / 3, 1 / 3])
    e2 = np.exp(-2.0)
    want = np.array([1 / (1 + e2) + 0.5 + e2 / (1 + e2), e2 / (1 + e2) + 0.5 + 1 / (1 + e2)]) / 3
    assert np.allclose(np.asarray(elw, float), want, rtol=0, atol=1e-15) and abs(float(elw.sum()) - 1) < 1e-15
    assert np.array_equal(RR.top_two_gap(c), [1.0, 0.0, 0.25])
    per, total = RR.mixture(s, [1.0, 2.0, 1.0])
    want = np.log(0.5 * (np.exp(s[0]) + np.exp(s[1])))
    assert np.allclose(np.asarray(per, float), want, rtol=0, atol=1e-15)
    assert abs(float(total) - (want[0] + 2 * want[1] + want[2])) < 1e-14
    # equal trees: the mixture of copies is the tree itself
    per, _ = RR.mixture(np.stack([s[0]] * 4), [1.0, 1.0, 1.0])
    assert np.allclose(np.asarray(per, float), s[0], rtol=0, atol=1e-15)
