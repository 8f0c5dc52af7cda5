"""tests/dense_ref.py checked by routes that do not share its code: the 80-bit oracle's
log-likelihood and gradient, the closed form of a three-taxon star tree, finite differences of the
oracle's gradient -- and, for the inputs of every case of tests/test_branch_hessian_edges_gpu.py,
that FP64 evaluators sit a factor of 100 inside the tolerances the GPU test uses.  Below the
line: the same for the 20-state form of the reference and tests/test_aa_edges_gpu.py."""
from types import SimpleNamespace

import numpy as np
import pytest

import aa_edge_cases as E2
import aa_utils as A
import dense_ref as D
import hessian_edge_cases as E
import hessian_fd as H
import oracle_lib as O
import tree_utils as TU


@pytest.fixture
def ld_oracle():
    """The oracle in long double with the expm1 form of the transition matrices."""
    O.select("ld")
    O.set_transition_mode(1)
    yield
    O.set_transition_mode(0)
    O.select("f64")


class SimpleCase:
    def __init__(self, tips, w, pids, bls, spec, pr, rates, freqs):
        self.tips, self.w, self.pids, self.bls, self.spec, self.pr = tips, w, pids, bls, spec, pr
        self.rates, self.freqs = rates, freqs

    def reference(self, t):
        Q, pi = D.gtr_q(self.rates[t], self.freqs[t])
        m = O.model_set(self.spec, self.pr[t])
        K = self.spec.category_count
        return D.branch_derivatives(self.pids[t], self.bls[t], Q, pi, m.cat_rates[:K], m.cat_weights[:K],
                                    D.tip_vectors(self.tips), self.w)


def _gtr_gamma4(n, P, T, seed, special):
    """Random GTR + Gamma4 trees; `special` lengths go to the first internal branch, then to
    random other branches."""
    rng = np.random.default_rng(seed)
    tips, w = TU.random_alignment(n, P, rng)
    pids, bls = TU.random_trees(n, T, rng)
    for t in range(T):
        where = [n] + list(rng.choice([j for j in range(2 * n - 3) if j != n], len(special) - 1, replace=False))
        bls[t, where] = special
    spec = O.make_spec(n, P, "GTR", "weibull+4")
    rates, freqs = TU.random_gtr_params(T, rng)
    lay = O.param_layout(spec)
    pr = np.zeros((T, O.param_count(spec)))
    pr[:, lay["GTR rates"]:lay["GTR rates"] + 6] = rates
    pr[:, lay["frequencies"]:lay["frequencies"] + 4] = freqs
    pr[:, lay["Weibull shape"]] = rng.uniform(0.4, 1.6, size=T)
    pr[:, lay["clock rate"]] = 1.0
    return SimpleCase(tips, w, pids, bls, spec, pr, rates, freqs)


def test_q_is_the_oracles():
    c = _gtr_gamma4(5, 3, 4, 1, (0.1,))
    for t in range(4):
        Q, pi = D.gtr_q(c.rates[t], c.freqs[t], np.float64)
        m = O.model_set(c.spec, c.pr[t])
        assert np.array_equal(Q.reshape(-1), np.array(m.Q[:16]))
        assert np.array_equal(pi, np.array(m.pi[:4]))
        assert abs(-np.sum(pi * np.diag(Q)) - 1.0) <= 4e-16


def test_tip_vectors():
    v = D.tip_vectors(np.array([[0, 3], [4, 9]]))
    assert v.dtype == np.longdouble
    assert np.array_equal(v, [[[1, 0, 0, 0], [0, 0, 0, 1]], [[1, 1, 1, 1], [1, 1, 1, 1]]])


def test_expm_against_the_jc69_closed_form():
    Q, _ = D.gtr_q(np.ones(6), np.full(4, 0.25))
    for t in (0.0, 1e-8, 1e-4, 0.3, 10.0, 90.0):
        e1 = np.expm1(-D.LD(4) * D.LD(t) / 3)  # P = I + expm1(-4t/3) (I - 1/4)
        want = np.eye(4, dtype=D.LD) + e1 * (np.eye(4, dtype=D.LD) - 0.25)
        got = D.expm(Q * D.LD(t))
        assert np.max(np.abs(got - want)) <= 1e-17, t
        off = ~np.eye(4, dtype=bool)
        assert np.all(np.abs(got[off] - want[off]) <= 1e-16 * want[off]), t  # relative, off-diagonal


def test_log_likelihood_and_gradient_match_the_80_bit_oracle(ld_oracle):
    """One branch each of length 0, 1e-8 and 7.  Measured: 6e-18 and 6e-14."""
    c = _gtr_gamma4(9, 13, 3, 2, (0.0, 1e-8, 7.0))
    out = O.unrooted_gradients(c.spec, c.tips, c.w, c.pids, c.bls, c.pr)
    for t in range(3):
        ref = c.reference(t)
        ll = abs(out["log_likelihood"][t] - ref.log_likelihood) / abs(ref.log_likelihood)
        g = np.max(np.abs(out["branch_lengths"][t, :-2] - ref.g[:-2]) / ref.A1[:-2])
        print(f"tree {t}: logL {float(ll):.1e} relative, g {float(g):.1e} of A1")
        assert ll <= 1e-15
        assert g <= 1e-12
        assert np.all(ref.g[-2:] == 0)


def test_star_tree_closed_form():
    rng = np.random.default_rng(3)
    P = 50
    tips = rng.integers(0, 5, size=(3, P)).astype(np.int32)
    w = rng.integers(1, 4, size=P).astype(float)
    lengths = np.array([0.05, 0.17, 0.42, 0.0])
    ll0, g0, h0, s0 = H.jc69_star_tree(tips, w, lengths[:3])
    Q, pi = D.gtr_q(np.ones(6), np.full(4, 0.25))
    ref = D.branch_derivatives([3, 3, 3], lengths, Q, pi, [1.0], [1.0], D.tip_vectors(tips), w)
    assert abs(ref.log_likelihood - ll0) <= 1e-13 * abs(ll0)
    for got, want in ((ref.g, g0), (ref.H, h0), (ref.S, s0)):
        assert np.max(np.abs(got[:3] - want)) <= 1e-13 * np.max(np.abs(want))
        assert np.all(got[3:] == 0)


def test_hessian_matches_finite_differences_of_the_80_bit_oracle(ld_oracle):
    """Branches of at least 1e-3 (the differences' step is 1e-4 t_j).  Measured: 2e-12."""
    c = _gtr_gamma4(9, 13, 2, 4, (7.0, 1e-8))
    c.bls[:, :-1] = np.where(c.bls[:, :-1] == 1e-8, 1e-8, np.maximum(c.bls[:, :-1], 2e-3))
    fd = H.fd_hessian_diagonal(c.spec, c.tips, c.w, c.pids, c.bls, c.pr)
    for t in range(2):
        ref = c.reference(t)
        keep = c.bls[t, :-1] >= 1e-3
        assert keep.sum() == len(keep) - 1 and np.any(c.bls[t, :-1] == 7.0)
        err = np.abs(fd[t, :-2] - ref.H[:-2]) / (ref.A2[:-2] + ref.S[:-2])
        print(f"tree {t}: H - FD {float(np.max(err[keep])):.1e} of A2 + S")
        assert np.max(err[keep]) <= 1e-9


@pytest.mark.parametrize("K", [1, 4])
def test_zero_weight_cases_are_their_twins_with_two_weights_zeroed(K):
    """hessian_edge_cases.references leaves patterns of weight 0 out: the reference of a "-zeros"
    case is the full-weight case's on the other 23 patterns."""
    full, zeros = E.inputs(f"weights-K{K}"), E.inputs(f"weights-K{K}-zeros")
    keep = np.ones(full.case.P, bool)
    keep[list(E.ZEROED)] = False
    assert np.all(full.w > 0) and np.array_equal(zeros.w, np.where(keep, full.w, 0.0))
    for name in ("states", "pids", "bls", "pr"):
        assert np.array_equal(getattr(full, name), getattr(zeros, name)), name
    for a, b in zip(E.references(f"weights-K{K}"), E.references(f"weights-K{K}-zeros")):
        assert abs(a.W - b.W - np.sum(full.w[~keep])) <= 1e-18 * a.W and np.all(a.S[:-2] > b.S[:-2])


def _worst(got, want, tol):
    got = np.asarray(got)
    assert np.all(np.isfinite(got)), got
    return float(np.max(np.abs(got[:-2] - want[:-2]) / tol[:-2]))


def _larger(a, b):
    """max that hands a NaN on (Python's max(x, nan) is x)."""
    return float(np.maximum(a, b))


@pytest.mark.parametrize("name", [c.name for c in E.CASES])
def test_fp64_evaluators_sit_inside_the_gpu_tolerances(name):
    """The tolerance form of the GPU test with 1e-12 in place of 1e-10, on the GPU test's own
    inputs: the f64 oracle's gradient in both transition modes (tip states; it takes no tip
    vectors), and g, S, H of dense_ref itself evaluated in float64 (every case).  Measured: see
    the print."""
    x = E.inputs(name)
    refs = E.references(name)
    worst = dict(oracle_g=0.0, g=0.0, S=0.0, H=0.0)
    f64 = E.references(name, np.float64)
    for t, (ref, low) in enumerate(zip(refs, f64)):
        tol = D.tolerances(ref, 1e-12)
        for key in ("g", "S", "H"):
            worst[key] = _larger(worst[key], _worst(getattr(low, key), getattr(ref, key), getattr(tol, key)))
    if x.states is not None:
        for mode in (0, 1):
            O.set_transition_mode(mode)
            try:
                out = O.unrooted_gradients(x.spec, x.states, x.w, x.pids, x.bls, x.pr)
            finally:
                O.set_transition_mode(0)
            for t, ref in enumerate(refs):
                worst["oracle_g"] = _larger(worst["oracle_g"], _worst(out["branch_lengths"][t], ref.g,
                                                                      D.tolerances(ref, 1e-12).g))
                assert np.isfinite(out["log_likelihood"][t])
                assert abs(out["log_likelihood"][t] - ref.log_likelihood) <= 1e-12 * abs(ref.log_likelihood)
    print(name, " ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert np.all(np.array(list(worst.values())) <= 1.0), worst


# ---------------------------------------------------------------------------------------------
# Any state count, and the derivative by the Weibull shape: the reference of
# tests/test_aa_edges_gpu.py (inputs: tests/aa_edge_cases.py)

def test_reversible_q_at_four_states_is_gtr_q_and_at_twenty_the_oracles():
    rng = np.random.default_rng(11)
    rates, freqs = TU.random_gtr_params(1, rng)
    for dtype in (np.float64, D.LD):
        assert np.array_equal(D.reversible_q(rates[0], freqs[0], dtype)[0],
                              D.gtr_q(rates[0], freqs[0], dtype)[0])
    ex, fr = A.random_reversible_model(rng)
    O.set_reversible_model(ex, fr)
    m = O.model_set(A.oracle_spec(4, 1, "constant"), np.ones(1))
    Q, pi = D.reversible_q(ex, fr, np.float64)
    assert np.array_equal(pi, np.array(m.pi[:20]))
    assert np.max(np.abs(Q.reshape(-1) - np.array(m.Q[:400]))) <= 4e-16 * np.max(np.abs(Q))
    assert abs(-np.sum(pi * np.diag(Q)) - 1.0) <= 4e-16


def test_tip_vectors_of_twenty_states():
    v = D.tip_vectors(np.array([[0, 19], [20, 25]]), s=20)
    assert v.dtype == np.longdouble and v.shape == (2, 2, 20)
    assert np.array_equal(v[0], np.eye(20)[[0, 19]]) and np.all(v[1] == 1)


@pytest.mark.parametrize("K", [1, 2, 4, 8])
def test_weibull_is_the_80_bit_oracles(K, ld_oracle):
    for shape in (0.3, 0.77, 1.0, 2.0):
        r, c, dr = D.weibull(K, shape)
        assert r.dtype == np.longdouble and abs(np.sum(r * c) - 1) <= 1e-18
        for got, want in zip((r, c, dr), O.weibull_rates(K, shape)):
            assert np.all(np.abs(got - want) <= 1e-15 * np.abs(want)), (K, shape, got, want)
    assert D.weibull(1, 0.5)[0][0] == 1 and D.weibull(1, 0.5)[2][0] == 0


def _aa_trees(K, model, seed):
    """Three 6-taxon 20-state trees with a branch each of 0, 1e-8 and 7."""
    rng = np.random.default_rng(seed)
    n, P, T = 6, 10, 3
    tips, w = A.random_aa_alignment(n, P, rng)
    pids, bls = TU.random_trees(n, T, rng)
    for t in range(T):
        where = [n] + list(rng.choice([j for j in range(2 * n - 3) if j != n], 2, replace=False))
        bls[t, where] = (0.0, 1e-8, 7.0)
    site = "constant" if K == 1 else f"weibull+{K}"
    pr = A.params_for(site, T, rng)
    ex, fr = E2.wag() if model == "WAG" else A.random_reversible_model(rng)
    return SimpleNamespace(n=n, P=P, K=K, tips=tips, w=w, pids=pids, bls=bls, pr=pr, ex=ex, fr=fr,
                           spec=A.oracle_spec(n, P, site))


def _aa_reference(c, t, lengths=None, shape=None):
    Q, pi = D.reversible_q(c.ex, c.fr)
    r, cw, dr = D.weibull(c.K, c.pr[t, 0] if shape is None else shape)
    return D.branch_derivatives(c.pids[t], c.bls[t] if lengths is None else lengths, Q, pi, r, cw,
                                D.tip_vectors(c.tips, s=20), c.w, cat_rate_derivs=dr if c.K > 1 else None,
                                hessian=False)


@pytest.mark.parametrize("K,model", [(1, "WAG"), (4, "WAG"), (1, "random"), (4, "random")])
def test_twenty_state_reference_matches_the_80_bit_oracle(K, model, ld_oracle):
    """log L, every branch and the shape derivative in the tolerance form with eps = 1e-15."""
    c = _aa_trees(K, model, 40 + K)
    O.set_reversible_model(c.ex, c.fr)
    out = O.unrooted_gradients(c.spec, c.tips, c.w, c.pids, c.bls, c.pr, True)
    for t in range(3):
        ref = _aa_reference(c, t)
        assert not hasattr(ref, "H")
        assert abs(out["log_likelihood"][t] - ref.log_likelihood) <= 1e-15 * abs(ref.log_likelihood)
        tol = D.tolerances(ref, 1e-15)
        worst = np.max(np.abs(out["branch_lengths"][t, :-2] - ref.g[:-2]) / tol.g[:-2])
        print(f"K={K} {model} tree {t}: g {float(worst):.2e} of the bound")
        assert worst <= 1.0 and np.all(ref.g[-2:] == 0)
        if K > 1:
            bound = D.LD(1e-15) * (ref.A_site + ref.W * ref.rho_site * np.sum(c.bls[t]))
            assert abs(out["site_model"][t] - ref.g_site) <= bound


def test_twenty_state_gradients_are_central_differences_of_the_references_own_log_likelihood():
    """g_j and g_site against (log L(+h) - log L(-h)) / 2h of the same reference, long double,
    h = 1e-6: ties g_site to something that is not its own formula."""
    c = _aa_trees(4, "random", 50)
    h = D.LD(1e-6)
    for t in range(2):
        ref = _aa_reference(c, t)
        j = int(np.argmax((c.bls[t] > 0.01) & (c.bls[t] < 1.0)))  # a branch of ordinary length
        assert 0.01 < c.bls[t, j] < 1.0
        lp, lm = c.bls[t].astype(D.LD), c.bls[t].astype(D.LD)
        lp[j] += h
        lm[j] -= h
        fd = (_aa_reference(c, t, lengths=lp).log_likelihood -
              _aa_reference(c, t, lengths=lm).log_likelihood) / (2 * h)
        assert abs(fd - ref.g[j]) <= 1e-9 * abs(ref.g[j]), (float(fd), float(ref.g[j]))
        a = D.LD(c.pr[t, 0])
        fd = (_aa_reference(c, t, shape=a + h).log_likelihood -
              _aa_reference(c, t, shape=a - h).log_likelihood) / (2 * h)
        assert abs(fd - ref.g_site) <= 1e-9 * abs(ref.g_site), (float(fd), float(ref.g_site))


@pytest.mark.parametrize("K", [1, 4])
def test_aa_zero_weight_cases_are_their_twins_with_two_weights_zeroed(K):
    full, zeros = E2.inputs(f"weights-K{K}"), E2.inputs(f"weights-K{K}-zeros")
    keep = np.ones(full.case.P, bool)
    keep[list(E2.ZEROED)] = False
    assert set(full.w) == set(E2.WEIGHTS) and np.array_equal(zeros.w, np.where(keep, full.w, 0.0))
    for name in ("states", "pids", "bls", "pr"):
        assert np.array_equal(getattr(full, name), getattr(zeros, name)), name
    for a, b in zip(E2.references(f"weights-K{K}"), E2.references(f"weights-K{K}-zeros")):
        assert abs(a.W - b.W - np.sum(full.w[~keep])) <= 1e-18 * a.W
        # (two non-negative terms fewer per branch; on a saturated branch they are below the sum's rounding)
        assert np.all(a.A1 >= b.A1 * (1 - D.LD(1e-17))) and np.sum(a.A1) > np.sum(b.A1)
        assert a.log_likelihood < b.log_likelihood


def test_aa_edge_inputs_are_what_their_names_say():
    for c in E2.CASES:
        x = E2.inputs(c.name)
        if not c.rooted:
            assert all(np.any(x.bls[:, :-1] == v) for v in (0.0, 1e-8, 10.0)), c.name
            assert np.all(np.sum(x.bls[:, :-1] == 0.0, axis=1) == 1), c.name
        assert x.states.shape == (c.n, c.P) and x.pr.shape == (len(x.pids), 1 + (c.K > 1))
    x = E2.inputs("tips-columns")
    assert np.all(x.states[:, 5] == 20) and np.all(x.states[:, 11] == 7)
    a, b = E2.inputs("tips-gaps20"), E2.inputs("tips-gaps20-onehot")
    assert np.array_equal(a.states, b.states) and a.partials is None and b.partials.shape == (8, 25, 20)
    assert 0.1 < np.mean(a.states == 20) < 0.3
    assert len(E2.inputs("launches-n9-K4-P65").pids) == 5
    assert abs(sum(c.model == "WAG" for c in E2.CASES) - len(E2.CASES) / 2) <= 3  # (twins share a model)
    assert [E2.aa_tiles(P) for P in (1, 64, 65, 129, 257)] == [4, 4, 8, 12, 20]


@pytest.mark.parametrize("name", [c.name for c in E2.CASES])
def test_fp64_oracle_sits_a_factor_of_ten_inside_the_aa_bounds(name):
    """The bounds of tests/test_aa_edges_gpu.py on its own inputs: the f64 oracle in its expm1 form
    (the engine's form) has every ratio at most 0.1.  Measured: see the print."""
    x = E2.inputs(name)
    refs = E2.references(name)
    O.set_reversible_model(*x.model)
    O.set_transition_mode(1)
    try:
        if x.case.rooted:
            ll = O.rooted_log_likelihoods(x.spec, x.states, x.w, x.pids, x.bls, x.pr, x.rates, x.heights,
                                          x.bounds, True, True)
            out = O.rooted_gradients(x.spec, x.states, x.w, x.pids, x.bls, x.pr, x.rates, x.rate_counts,
                                     x.heights, x.bounds, x.ratios, True)
            r = E2.ratios(refs, x, ll, site=out["site_model"], clock=out["clock_model"][:, 0])
            r["logL-of-gradients"] = E2.ratios(refs, x, out["log_likelihood"], jacobian=False)["logL"]
        else:
            ll = O.unrooted_log_likelihoods(x.spec, x.states, x.w, x.pids, x.bls, x.pr, True)
            out = O.unrooted_gradients(x.spec, x.states, x.w, x.pids, x.bls, x.pr, True)
            r = E2.ratios(refs, x, ll, out["branch_lengths"], out.get("site_model"))
            r["logL-of-gradients"] = E2.ratios(refs, x, out["log_likelihood"])["logL"]
    finally:
        O.set_transition_mode(0)
    print(name, " ".join(f"{k} {v:.1e}" for k, v in r.items()))
    assert E2.within(r, 0.1), r
