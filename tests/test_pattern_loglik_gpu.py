"""Per-pattern log-likelihoods (mi_engine_pattern_log_likelihoods_unrooted, Engine.pattern_log_likelihoods):
s[t][p] = log L_p(tree t), unweighted, out of the log-likelihood call's own kernels.  The
reference is the CPU oracle on one-pattern alignments of weight 1 (tests/rell_ref.py):
|got - oracle| <= 1e-10 |oracle| per entry, the project's standing tolerance.

Pattern counts 13, 16, 17, 65, 131: the matrix-core kernel takes 64, 32 or 16 patterns per wave
for K = 1, 2, >= 4 and the VALU kernel 64 -- a partial tile, an exact tile and a tile plus one
in each."""
import numpy as np
import pytest

import oracle_lib as O
import rell_ref as RR
import tree_utils as TU

pytestmark = pytest.mark.gpu

TOL = 1e-10
KERNELS = {"mfma": "loglik_mfma_kernel", "valu": "loglik_onchip_kernel"}
PATTERNS = (13, 16, 17, 65, 131)


def _engine(subst, K, tips, w, **kw):
    import libsbn_amd as L
    return L.Engine(L.PhyloModelSpecification(subst, RR.site(K), "strict"), tips, w, device=0, **kw)


def _one_hot(tips):
    parts = np.zeros(tips.shape + (4,))
    for s in range(4):
        parts[..., s] = (tips == s) | (tips > 3)
    return parts


def _check(eng, kernel, spec, tips, w, pids, bls, pr, label):
    """Both rescaling settings: against the oracle, the call's line, logL bit for bit, the sum."""
    T, P = len(pids), tips.shape[1]
    for rescaling in (False, True):
        want = RR.pattern_log_likelihoods(spec, tips, pids, bls, pr, rescaling)
        ll, s = eng.pattern_log_likelihoods(pids, bls, pr, rescaling=rescaling)
        path = eng.last_call_path()
        assert eng.last_call_info()[:2] == (kernel, T), (label, eng.last_call_info())
        assert path.startswith(kernel + " ") and " pattern_ll" in path and ("rescaled" in path) == rescaling, path
        assert s.shape == (T, P)
        worst = np.max(np.abs(s - want) / np.abs(want))
        print(f"{label} rescaling={int(rescaling)}: worst {worst:.2e}")
        assert np.all(np.abs(s - want) <= TOL * np.abs(want)), (label, rescaling, worst)
        # the sums are the log-likelihood call's, bit for bit, and the rows add up to them
        plain = eng.log_likelihoods(pids, bls, pr, rescaling=rescaling)
        assert " pattern_ll" not in eng.last_call_path()
        assert np.array_equal(ll, plain), (label, rescaling)
        assert np.all(np.abs(s @ w - ll) <= P * 2.0 ** -52 * np.abs(ll)), (label, rescaling)


@pytest.mark.parametrize("path", ["mfma", "valu"])
@pytest.mark.parametrize("K", [1, 2, 4, 6])
@pytest.mark.parametrize("subst", ["JC69", "GTR"])
def test_matches_oracle(monkeypatch, subst, K, path):
    monkeypatch.setenv("MI_PHYLO_LOGLIK_PATH", path)  # (read when the engine is created)
    for k, name in enumerate(RR.SHAPES):
        for P in PATTERNS:
            tips, w, pids, bls, spec, pr = RR.case(name, P, subst, K, 5000 + 100 * K + 10 * k + P)
            eng = _engine(subst, K, tips, w)
            _check(eng, KERNELS[path], spec, tips, w, pids, bls, pr, f"{path} {name} {subst} K={K} P={P}")
            eng.close()


@pytest.mark.parametrize("subst,K", [("JC69", 4), ("GTR", 1), ("GTR", 6)])
def test_one_hot_tip_partials(monkeypatch, subst, K):
    """use_tip_states=False: the VALU kernel's other instantiation (tip partials)."""
    monkeypatch.setenv("MI_PHYLO_LOGLIK_PATH", "valu")
    for k, name in enumerate(("n5", "random12")):
        for P in (17, 65):
            tips, w, pids, bls, spec, pr = RR.case(name, P, subst, K, 6000 + 10 * K + k + P)
            eng = _engine(subst, K, None, w, use_tip_states=False, tip_partials=_one_hot(tips))
            _check(eng, KERNELS["valu"], spec, tips, w, pids, bls, pr, f"partials {name} {subst} K={K} P={P}")
            eng.close()


EDGE = [("JC69", 1), ("GTR", 4), ("JC69", 6)]
GAP_COLUMNS = (5, 24)


def _edge_case(subst, K):
    """balanced8 x 25 patterns with two all-gap columns and three patterns of weight 0."""
    tips, w, pids, bls, spec, pr = RR.case("balanced8", 25, subst, K, 7000 + K)
    tips[:, GAP_COLUMNS] = 4
    w[[3, 5, 17]] = 0.0
    return tips, w, pids, bls, spec, pr


@pytest.mark.parametrize("path", ["mfma", "valu"])
@pytest.mark.parametrize("subst,K", EDGE)
def test_weight_zero_patterns_and_all_gap_columns_are_finite(monkeypatch, subst, K, path):
    """Patterns of weight 0 are reported like the others; every value is finite."""
    monkeypatch.setenv("MI_PHYLO_LOGLIK_PATH", path)
    tips, w, pids, bls, spec, pr = _edge_case(subst, K)
    eng = _engine(subst, K, tips, w)
    for rescaling in (False, True):
        ll, s = eng.pattern_log_likelihoods(pids, bls, pr, rescaling=rescaling)
        assert eng.last_call_info()[0] == KERNELS[path]
        assert np.all(np.isfinite(s)) and np.all(np.isfinite(ll))
        keep = [p for p in range(25) if p not in GAP_COLUMNS]
        want = RR.pattern_log_likelihoods(spec, tips[:, keep], pids, bls, pr, rescaling)
        assert np.all(np.abs(s[:, keep] - want) <= TOL * np.abs(want))
        assert np.array_equal(ll, eng.log_likelihoods(pids, bls, pr, rescaling=rescaling))


@pytest.mark.parametrize("path", ["mfma", "valu"])
@pytest.mark.parametrize("subst,K", EDGE)
def test_all_gap_column_gives_exactly_zero(monkeypatch, subst, K, path):
    """An all-gap column has likelihood 1 whatever the tree: log L_p == 0.0 exactly.  (The
    log-likelihood call's arithmetic gives such a column a few units of 2^-53 either side of 0 --
    the rows of V exp(L t) V^-1 sum to 1 only to rounding --; the per-pattern output reports the
    exact value, the sums keep the log-likelihood call's bits.)"""
    monkeypatch.setenv("MI_PHYLO_LOGLIK_PATH", path)
    tips, w, pids, bls, spec, pr = _edge_case(subst, K)
    eng = _engine(subst, K, tips, w)
    for rescaling in (False, True):
        ll, s = eng.pattern_log_likelihoods(pids, bls, pr, rescaling=rescaling)
        gaps = s[:, GAP_COLUMNS]
        print(f"all-gap {path} {subst} K={K} rescaling={int(rescaling)}: {gaps.ravel().tolist()}")
        assert np.all(gaps == 0.0), gaps
        assert not np.any(np.signbit(gaps))
        assert np.array_equal(ll, eng.log_likelihoods(pids, bls, pr, rescaling=rescaling))


@pytest.mark.parametrize("K,rescaling", [(1, False), (4, True), (6, False)])
def test_device_entry_equals_host_call(K, rescaling):
    import torch
    tips, w, pids, bls, spec, pr = RR.case("random12", 131, "GTR", K, 8000 + K)
    T, P = len(pids), 131
    eng = _engine("GTR", K, tips, w)
    ll, s = eng.pattern_log_likelihoods(pids, bls, pr, rescaling=rescaling)
    dev = torch.device("cuda", 0)
    d_pid = torch.from_numpy(pids).to(dev)
    d_bl, d_pr = torch.from_numpy(bls).to(dev), torch.from_numpy(pr).to(dev)
    d_ll = torch.empty(T, dtype=torch.float64, device=dev)
    d_s = torch.empty((T, P), dtype=torch.float64, device=dev)
    eng.reserve(T, False)
    stream = torch.cuda.current_stream().cuda_stream
    for out_ll in (d_ll.data_ptr(), d_ll.data_ptr(), None):  # the second call: the same bits again
        d_s.fill_(float("nan"))
        eng.pattern_log_likelihoods_device(stream, T, d_pid.data_ptr(), d_bl.data_ptr(), d_pr.data_ptr(),
                                           d_s.data_ptr(), out_ll=out_ll, rescaling=rescaling)
        eng.check_status(stream)
        assert np.array_equal(d_s.cpu().numpy(), s)
        assert np.array_equal(d_ll.cpu().numpy(), ll)
    assert " pattern_ll" in eng.last_call_path()


def test_tree_sharded_handle_equals_single_engine():
    rng = np.random.default_rng(9)
    n, P, T = 9, 65, 7
    tips, w = TU.random_alignment(n, P, rng)
    pids, bls = TU.random_trees(n, T, rng)
    spec = O.make_spec(n, P, "GTR", "weibull+4")
    pr = RR.model_params(spec, "GTR", 4, T, rng)
    ll, s = _engine("GTR", 4, tips, w).pattern_log_likelihoods(pids, bls, pr)
    sharded = _engine("GTR", 4, tips, w, shard_devices=[0, 0, 0], shard_mode="trees")
    sll, ss = sharded.pattern_log_likelihoods(pids, bls, pr)
    assert np.array_equal(sll, ll) and np.array_equal(ss, s)
    by_patterns = _engine("GTR", 4, tips, w, shard_devices=[0, 0, 0], shard_mode="patterns")
    with pytest.raises(RuntimeError, match="pattern-sharded"):
        by_patterns.pattern_log_likelihoods(pids, bls, pr)


def test_twenty_state_engine_is_refused():
    import libsbn_amd as L
    rng = np.random.default_rng(10)
    n, P = 5, 13
    tips = rng.integers(0, 20, size=(n, P)).astype(np.int32)
    eng = L.Engine(L.PhyloModelSpecification("WAG", "constant", "strict"), tips, np.ones(P), device=0)
    pids, bls = TU.random_trees(n, 2, rng)
    with pytest.raises(RuntimeError, match="4-state"):
        eng.pattern_log_likelihoods(pids, bls)


def test_no_trees_gives_empty_arrays():
    tips, w, pids, bls, spec, pr = RR.case("n5", 13, "JC69", 1, 1)
    ll, s = _engine("JC69", 1, tips, w).pattern_log_likelihoods(pids[:0], bls[:0])
    assert ll.shape == (0,) and s.shape == (0, 13)
