"""The four calls of the HBM-streamed kernel family on the same inputs: the
gradient call on the HBM path, the branch-length Hessian call, the NNI scan and the
ancestral-state call share the lane context, the post-order pass and the tile sums, so their
log-likelihoods are one number, bit for bit, and the Hessian call's branch gradient is the
gradient call's.  The corners the pairwise tests leave out: three taxa (no inner edge) and a
random 12-taxon tree, a second tile with one live lane (P = 65), one and four categories,
rescaling off and on, compact states and real-valued tip partials -- every instantiation of
every member's (rescaling, tip partials) ladder."""
import numpy as np
import pytest

import ancestral_cases as AC
import ancestral_ref as A
import oracle_lib as O
import tree_utils as TU

pytestmark = pytest.mark.gpu

P, T = 65, 3


def _case(n, K, form):
    rng = np.random.default_rng(4100 + 100 * n + 10 * K + (form == "real"))
    pids = np.stack([TU.random_topology(n, rng) for _ in range(T)])
    states, w = TU.random_alignment(n, P, rng)
    vectors = None
    if form == "real":
        vectors = A.tip_vectors(states, np.float64)
        vectors[:3] = 1.0 - rng.uniform(0.0, 0.95, size=vectors[:3].shape)
        states = None
    bls = rng.uniform(0.01, 0.5, size=(T, 2 * n - 2))
    bls[:, -1] = 0.0
    spec = O.make_spec(n, P, "GTR", AC.site(K))
    pr = AC.params(spec, "GTR", K, T, rng)[0]
    return states, vectors, w, pids, bls, pr


@pytest.mark.parametrize("form", ["states", "real"])
@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("n", [3, 12])
def test_four_calls_one_log_likelihood(monkeypatch, n, K, form):
    import libsbn_amd as L
    states, vectors, w, pids, bls, pr = _case(n, K, form)
    spec = L.PhyloModelSpecification("GTR", AC.site(K), "strict")
    if form == "states":
        # (real-valued partials take the HBM kernels anyway)
        monkeypatch.setenv("MI_PHYLO_GRADIENT_PATH", "hbm")
        eng = L.Engine(spec, states, w, device=0)
    else:
        eng = L.Engine(spec, None, w, device=0, use_tip_states=False, tip_partials=vectors)
    for rescaling in (False, True):
        grad = eng.gradients(pids, bls, pr, rescaling=rescaling, gradient_blocks=())
        assert eng.last_call_info()[0] == "gradient_hbm_kernel"
        ll = np.array([x.log_likelihood for x in grad])
        g = np.stack([x.gradient["branch_lengths"] for x in grad])
        assert np.all(np.isfinite(ll)) and np.all(np.isfinite(g))
        hll, hg, _ = eng.branch_hessian(pids, bls, pr, rescaling=rescaling)
        assert eng.last_call_info()[0] == "gradient_hbm_hess_kernel"
        sll = eng.nni_scan(pids, bls, pr, rescaling=rescaling)[0]
        assert eng.last_call_info()[0] == "nni_scan_hbm_kernel"
        all_ = eng.ancestral_states(pids, bls, pr, rescaling=rescaling).log_likelihoods
        assert eng.last_call_info()[0] == "ancestral_hbm_kernel"
        tag = f"n={n} K={K} {form} rescaling={rescaling}"
        assert np.array_equal(hll, ll), tag
        assert np.array_equal(sll, ll), tag
        assert np.array_equal(all_, ll), tag
        assert np.array_equal(hg, g), tag
