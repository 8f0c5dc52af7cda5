"""tests/ancestral_ref.py checked by routes that do not share its code (brute-force enumeration
of every internal-state assignment, dense_ref's log-likelihood), the absolute floor it sets for
small entries measured on the GPU tests' inputs, the map-state exclusions of those inputs held to
their cap -- and the two CPU checks of the call's Python surface.  No GPU is needed."""
import numpy as np
import pytest

import ancestral_cases as AC
import ancestral_ref as A
import dense_ref as D
import oracle_lib as O
import tree_utils as TU

LD = A.LD
EPS = float(np.finfo(LD).eps)


def _small(n, subst, K, seed, P=11):
    rng = np.random.default_rng(seed)
    pid = TU.random_topology(n, rng)
    states, w = TU.random_alignment(n, P, rng, gap_fraction=0.15)
    states[:, 3] = 4  # an all-gap column
    assert np.any(states[:, :3] > 3) or np.any(states[:, 4:] > 3)
    bl = rng.uniform(0.01, 0.8, size=2 * n - 2)
    bl[-1] = 0.0
    spec = O.make_spec(n, P, subst, AC.site(K))
    pr, rates, freqs = AC.params(spec, subst, K, 1, rng)
    Q, pi = A.gtr_q(rates[0], freqs[0])
    m = O.model_set(spec, pr[0])
    return pid, bl, Q, pi, np.array(m.cat_rates[:K]), np.array(m.cat_weights[:K]), A.tip_vectors(states), w


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("subst", ["JC69", "GTR"])
@pytest.mark.parametrize("n", [4, 5])
def test_reference_against_brute_force(n, subst, K):
    pid, bl, Q, pi, r, c, tips, w = _small(n, subst, K, 100 * n + 10 * K + (subst == "GTR"))
    ref = A.ancestral(pid, bl, Q, pi, r, c, tips)
    joint, cat_joint = A.brute_force(pid, bl, Q, pi, r, c, tips)
    # sums of at most 4^(n-2) K non-negative products of at most 2n factors each
    tol = 4 ** (n - 2) * K * 4 * n * EPS
    assert np.all(np.abs(ref.joint - joint) <= tol * joint)
    assert np.all(np.abs(ref.cat_joint - cat_joint) <= tol * cat_joint)
    # sum_s J[v][p][s] is the pattern likelihood at every node, the leaves included
    assert np.all(np.abs(ref.joint.sum(axis=-1) - ref.lik) <= tol * ref.lik)
    assert np.all(np.abs(ref.tip_joint.sum(axis=-1) - ref.lik) <= tol * ref.lik)
    assert np.all(np.abs(ref.cat_joint.sum(axis=-1) - ref.lik) <= tol * ref.lik)
    # rows sum to 1
    for post in (ref.state_post, ref.cat_post, ref.tip_post):
        assert np.all(np.abs(post.sum(axis=-1) - 1) <= 8 * EPS)
    assert np.all(np.abs(ref.pattern_rate - ref.cat_post @ np.asarray(r, LD)) <= 8 * EPS)
    if K == 1:
        assert np.all(ref.cat_post == 1) and np.all(ref.pattern_rate == LD(r[0]))
    # the all-gap column: the posterior is pi at every node, cat_post = c (float64 inputs sum to 1
    # to float64 rounding only: normalised here as the posteriors are)
    pin, cn = np.asarray(pi, LD) / np.sum(np.asarray(pi, LD)), np.asarray(c, LD) / np.sum(np.asarray(c, LD))
    assert np.all(np.abs(ref.state_post[:, 3] - pin) <= 64 * EPS)
    assert np.all(np.abs(ref.cat_post[3] - cn) <= 64 * EPS)
    # sum_p w_p log sum_s J equals dense_ref's log-likelihood
    dense = D.branch_derivatives(pid, bl, Q, pi, r, c, tips, w)
    ll = np.sum(np.asarray(w, LD) * np.log(ref.joint[-1].sum(axis=-1)))
    assert abs(ll - dense.log_likelihood) <= 64 * EPS * abs(dense.log_likelihood)


def test_unambiguous_tips_get_their_own_vector():
    pid, bl, Q, pi, r, c, tips, w = _small(5, "GTR", 4, 77)
    ref = A.ancestral(pid, bl, Q, pi, r, c, tips)
    known = tips.sum(axis=-1) == 1
    assert np.any(known) and np.any(~known)
    assert np.all(ref.tip_post[known] == tips[known])


def _gpu_inputs():
    for name in AC.SHAPES:
        for subst in AC.SUBSTS:
            for K in AC.KS:
                for P in AC.PS:
                    yield f"{name} {subst} K={K} P={P}", AC.parity(name, subst, K, P), True
    for name in ("balanced8", "random12"):
        for subst in AC.SUBSTS:
            for K in (1, 4):
                for form in ("masks", "real"):
                    yield f"{name} {subst} K={K} {form}", AC.partials(name, subst, K, form), True


def test_floor_and_map_exclusions_on_the_gpu_tests_inputs():
    """The absolute floor for entries below SMALL: 16 times the largest disagreement on them
    between the reference in float64 and in longdouble, over every input of the GPU tests; the
    constant in ancestral_ref.py covers it, is not more than twice it, and stays below the cap.
    The same loop holds the map-state exclusions of every case to their cap."""
    worst, worst_at, most_excluded = 0.0, "", 0.0
    for label, x, tips in _gpu_inputs():
        lo = AC.reference(x, np.float64, with_tips=tips)
        hi = AC.parity_reference(x.name, x.subst, x.K, x.P) if x.states is not None else AC.reference(x)
        excluded = 0.0
        for a, b in zip(lo, hi):
            pairs = [(a.state_post, b.state_post), (a.cat_post, b.cat_post), (a.pattern_rate, b.pattern_rate)]
            if tips:
                pairs.append((a.tip_post, b.tip_post))
            for got, want in pairs:
                rel, low = A.errors(got, want)
                assert rel <= 1e-12, (label, rel)  # (the reference itself is nowhere near REL)
                if low > worst:
                    worst, worst_at = low, label
            excluded += float(np.mean(b.margin <= A.MAP_MARGIN)) / len(hi)
        assert excluded <= A.MAP_EXCLUDED, (label, excluded)
        most_excluded = max(most_excluded, excluded)
    print(f"float64 against longdouble on entries below {A.SMALL}: {worst:.3e} ({worst_at}); "
          f"floor 16 x = {16 * worst:.3e}; constant {A.ABS_FLOOR:.3e}; map states left out: at most "
          f"{100 * most_excluded:.3f} % of a case")
    assert 16 * worst <= A.ABS_FLOOR <= 32 * worst, (worst, A.ABS_FLOOR)
    assert A.ABS_FLOOR <= A.ABS_FLOOR_CAP


def test_ladder200_map_exclusions():
    x = AC.ladder200()
    ref = AC.reference(x, with_tips=False)[0]
    assert float(np.mean(ref.margin <= A.MAP_MARGIN)) <= A.MAP_EXCLUDED
    assert np.min(ref.lik) > 0


# ---- the call's Python surface: these two fail without the feature ----

def test_symbols_are_bound():
    from libsbn_amd import _capi
    for name in ("mi_engine_ancestral_states_unrooted", "mi_engine_ancestral_states_unrooted_device",
                 "mi_engine_reserve_ancestral"):
        assert name in _capi.SYMBOLS, name


def test_without_a_device_the_call_raises_instead_of_falling_back():
    import libsbn_amd as L
    assert hasattr(L.Engine, "ancestral_states") and hasattr(L.Engine, "ancestral_states_device")
    x = AC.parity("n4", "JC69", 1, 13)
    if L._capi.load().mi_device_count() == 0:
        with pytest.raises(RuntimeError, match="no HIP device"):
            AC.engine(x).ancestral_states(x.pids, x.bls, x.pr)
    else:  # (a machine with a device gets the result: tests/test_ancestral_gpu.py checks it)
        assert AC.engine(x).ancestral_states(x.pids, x.bls, x.pr).state_posteriors.shape == (AC.T, 2, 13, 4)
