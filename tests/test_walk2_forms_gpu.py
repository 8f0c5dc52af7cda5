"""The second-generation walk has one body (gradient_walk_body) and two instantiation ladders:
gradient_walk_kernel (the gradient call under MI_PHYLO_GRADIENT_WALK=v2) and
gradient_walk_hess_kernel (the branch-length Hessian call).  Here the two are held to each
other on every form of the body: compact tip words with 16 and 8 columns and full words
(K = 1, 2, 4), rescaling off and on, stored vectors in LDS and in the arena, and -- three
12-taxon trees: a ladder, a balanced and a random one -- every configuration of a macro's child
(tip, stored, unstored over two stored / tip + stored / stored + tip / two tips).  49 patterns:
the last tile has one live column at every K (48 + 1, 24 + 24 + 1, 4 x 12 + 1).  A 3-taxon tree
(one macro, no inner edge) with the LDS store, and the analytic GTR gradient, which only the
gradient ladder has, against the oracle."""
import functools

import numpy as np
import pytest

import oracle_lib as O
import tree_utils as TU

pytestmark = pytest.mark.gpu

GRAD = "gradient_walk_kernel"
HESS = "gradient_walk_hess_kernel"
HBM = "gradient_hbm_hess_kernel"
SITE = {1: "constant", 2: "weibull+2", 4: "weibull+4"}
N_TAXA, P = 12, 49


def _engine(subst, site, tips, w):
    import libsbn_amd as L
    return L.Engine(L.PhyloModelSpecification(subst, site, "strict"), tips, w, device=0)


def _readonly(*arrays):
    for x in arrays:
        x.setflags(write=False)
    return arrays


def child_configurations(pids, n):
    """The configurations of the children of a tree's macros, as the set-up classes them: an
    internal node whose children are all tips or stored nodes is not stored (its vector is
    recomputed where it is needed); every other internal node, and the root, is a macro."""
    r = len(pids)  # the trifurcation (k0, k1, k2) is walked as r = (k1, k2), r + 1 = (k0, r)
    N = r + 2
    kids = {v: [c for c in range(r) if pids[c] == v] for v in range(n, r + 1)}

    def max_leaf(v):
        return v if v < n else max(max_leaf(c) for c in kids[v])

    for v in kids:  # (a node's children: by the largest leaf id below them)
        kids[v].sort(key=max_leaf)
    kids[r + 1] = [kids[r].pop(0), r]
    stored = {}
    for v in sorted(kids, key=lambda v: _height(v, kids)):
        stored[v] = v == N - 1 or not all(c < n or stored[c] for c in kids[v])
    found = set()
    for v in kids:
        if not stored[v]:
            continue
        for c in kids[v]:
            if c < n:
                found.add("tip")
            elif stored[c]:
                found.add("stored")
            else:
                found.add("unstored:" + "".join("t" if g < n else "s" for g in kids[c]))
    return found


def _height(v, kids):
    return 0 if v not in kids else 1 + max(_height(c, kids) for c in kids[v])


@functools.lru_cache(maxsize=None)
def _case(n):
    """Alignment and trees, shared and read-only: the three 12-taxon topologies, or one 3-taxon tree."""
    rng = np.random.default_rng(2025 + n)
    tips, w = TU.random_alignment(n, P, rng)
    if n == 3:
        pids = np.array([[3, 3, 3]], np.int32)
    else:
        # (a random topology that has an unstored child over tip + stored: the ladder has stored + tip)
        pids = np.stack([TU.ladder_topology(n), TU.balanced_topology(n),
                         TU.random_topology(n, np.random.default_rng(1))]).astype(np.int32)
    bls = rng.uniform(0.01, 0.5, size=(len(pids), 2 * n - 2))
    bls[:, -1] = 0.0
    return _readonly(tips, w, pids, bls)


@functools.lru_cache(maxsize=None)
def _params(n, subst, K):
    import test_gpu_parity as TG
    T = len(_case(n)[2])
    rng = np.random.default_rng(31 * K + n)
    spec = O.make_spec(n, P, subst, SITE[K])
    blocks = {}
    if subst == "GTR":
        blocks["GTR rates"], blocks["frequencies"] = TU.random_gtr_params(T, rng)
    if K > 1:
        blocks["Weibull shape"] = rng.uniform(0.4, 1.6, size=(T, 1))
    return spec, _readonly(TG._params(spec, T, **blocks))[0]


@functools.lru_cache(maxsize=None)
def _oracle(n, subst, K, rescaling):
    tips, w, pids, bls = _case(n)
    spec, pr = _params(n, subst, K)
    og = O.unrooted_gradients(spec, tips, w, pids, bls, pr, rescaling, 4)
    return {k: _readonly(np.asarray(v))[0] for k, v in og.items()}


@functools.lru_cache(maxsize=None)
def _hbm_hessian(n, K, rescaling):
    """(log L, g, H, S) of the HBM-streamed Hessian kernel: the store setting does not reach it."""
    tips, w, pids, bls = _case(n)
    _, pr = _params(n, "JC69", K)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("MI_PHYLO_GRADIENT_PATH", "hbm")
        mp.delenv("MI_PHYLO_GRADIENT_STORE", raising=False)
        eng = _engine("JC69", SITE[K], tips, w)
    out = eng.branch_hessian(pids, bls, pr, rescaling=rescaling, squared_gradient=True)
    assert eng.last_call_path().startswith(HBM + " store=hbm "), eng.last_call_path()
    return _readonly(*out)


def _gradient(eng, n, subst, K, rescaling, blocks=()):
    tips, w, pids, bls = _case(n)
    res = eng.gradients(pids, bls, _params(n, subst, K)[1], rescaling, gradient_blocks=blocks)
    return np.array([x.log_likelihood for x in res]), res


def _check_path(eng, kernel, store, rescaling, K, word=None):
    p = eng.last_call_path()
    assert p.startswith(f"{kernel} store={store} "), p
    assert ("rescaled" in p) == rescaling and p.endswith(f" K={K}"), p
    assert word is None or f" {word} " in p, p
    assert eng.last_call_info()[0] == kernel


def _hold_the_forms_to_each_other(monkeypatch, n, K, rescaling, store):
    tips, w, pids, bls = _case(n)
    _, pr = _params(n, "JC69", K)
    monkeypatch.setenv("MI_PHYLO_GRADIENT_STORE", store)
    hess = _engine("JC69", SITE[K], tips, w)
    monkeypatch.setenv("MI_PHYLO_GRADIENT_WALK", "v2")
    grad = _engine("JC69", SITE[K], tips, w)

    ll, g, h, s = hess.branch_hessian(pids, bls, pr, rescaling=rescaling, squared_gradient=True)
    _check_path(hess, HESS, store, rescaling, K, "hess")
    vll, res = _gradient(grad, n, "JC69", K, rescaling)
    _check_path(grad, GRAD, store, rescaling, K)
    vg = np.stack([x.gradient["branch_lengths"] for x in res])

    # the two ladders of the one body: the same bits
    assert np.array_equal(ll, vll), np.max(np.abs(ll - vll))
    assert np.array_equal(g, vg), np.max(np.abs(g - vg))
    # the gradient call against the oracle
    og = _oracle(n, "JC69", K, rescaling)
    assert np.all(np.abs(vll - og["log_likelihood"]) <= 1e-10 * np.abs(og["log_likelihood"]))
    for t in range(len(pids)):
        assert np.max(np.abs(vg[t] - og["branch_lengths"][t])) <= 1e-10 * np.max(np.abs(og["branch_lengths"][t])), t
    # the second-order outputs against the other implementation
    for x, y in zip((ll, g, h, s), _hbm_hessian(n, K, rescaling)):
        assert np.max(np.abs(x - y)) <= 1e-12 * np.max(np.abs(y))


def test_the_three_trees_give_every_child_configuration():
    """(no GPU work: what the parametrised test below relies on)"""
    pids = _case(N_TAXA)[2]
    found = set().union(*(child_configurations(p, N_TAXA) for p in pids))
    assert found == {"tip", "stored", "unstored:ss", "unstored:ts", "unstored:st", "unstored:tt"}, found
    assert child_configurations(_case(3)[2][0], 3) <= {"tip", "unstored:tt"}


@pytest.mark.parametrize("store", ["lds", "arena"])
@pytest.mark.parametrize("rescaling", [False, True], ids=["plain", "rescaled"])
@pytest.mark.parametrize("K", [1, 2, 4])
def test_hessian_and_gradient_forms_agree(monkeypatch, K, rescaling, store):
    _hold_the_forms_to_each_other(monkeypatch, N_TAXA, K, rescaling, store)


@pytest.mark.parametrize("rescaling", [False, True], ids=["plain", "rescaled"])
@pytest.mark.parametrize("K", [1, 2, 4])
def test_three_taxa_have_no_inner_edge(monkeypatch, K, rescaling):
    _hold_the_forms_to_each_other(monkeypatch, 3, K, rescaling, "lds")


@pytest.mark.parametrize("store", ["lds", "arena"])
@pytest.mark.parametrize("rescaling", [False, True], ids=["plain", "rescaled"])
def test_analytic_gtr_gradient_matches_oracle(monkeypatch, rescaling, store):
    """The SUBST form (the gradient ladder only), at the bar of test_both_gradient_stores_match_oracle."""
    import test_gpu_parity as TG
    tips, w, pids, _ = _case(N_TAXA)
    monkeypatch.setenv("MI_PHYLO_GRADIENT_STORE", store)
    monkeypatch.setenv("MI_PHYLO_GRADIENT_WALK", "v2")
    monkeypatch.setenv("MI_PHYLO_SUBST_GRADIENT", "analytic")
    eng = _engine("GTR", SITE[4], tips, w)
    ll, res = _gradient(eng, N_TAXA, "GTR", 4, rescaling, blocks=None)
    _check_path(eng, GRAD, store, rescaling, 4, "analytic")
    og = _oracle(N_TAXA, "GTR", 4, rescaling)
    for t in range(len(pids)):
        assert abs(ll[t] - og["log_likelihood"][t]) <= 1e-10 * abs(og["log_likelihood"][t])
        assert TG._close(res[t].gradient["branch_lengths"], og["branch_lengths"][t]), t
